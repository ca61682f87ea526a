"""Host side of training from whole scenes (scenes.py, csrc/scene.hip's argument checks, the CLI's scene listing): the window table
against an independent enumeration, the eight codes against their index formulas, rua_scene_windows' refusals (no launch: safe
without a GPU), the converter from the reference's inputs, and the patch list / split / shard bookkeeping against the file path."""
import ctypes
import os
import sys

import numpy as np
import pytest
from numpy.lib.stride_tricks import sliding_window_view

from resunet_a_mltsk_keras_amd import _lib as L
from resunet_a_mltsk_keras_amd import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def scene(rng, H, W, C=3, classes=5):
    return rng.integers(0, 256, (H, W, C)).astype(np.uint8), rng.integers(0, classes, (H, W)).astype(np.uint8)


def reference_copies(w):
    """The reference's five copies of a window, in its order (as is, rot90 once, rot90 twice, flip axis 0, flip axis 1)."""
    return [w, np.rot90(w, 1), np.rot90(w, 2), np.flip(w, 0), np.flip(w, 1)]


# ---- 1. window_table ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shapes,P,stride", [([(70, 90)], 32, 16), ([(75, 101)], 32, 16), ([(70, 90), (64, 40)], 32, 8)])
def test_window_table_against_sliding_window_view(shapes, P, stride):
    rng = np.random.default_rng(len(shapes) * 100 + shapes[0][1])
    sc = [scene(rng, H, W) for H, W in shapes]
    images, maps = [s[0] for s in sc], [s[1] for s in sc]
    wins_img, wins_cls, count = [], [], 0
    for im, cm in zip(images, maps):
        vi = sliding_window_view(im, (P, P, im.shape[2]))[::stride, ::stride, 0]           # [nrow][ncol][P][P][C]
        vc = sliding_window_view(cm, (P, P))[::stride, ::stride]
        nrow, ncol = vi.shape[:2]
        assert nrow == (im.shape[0] - P) // stride + 1 and ncol == (im.shape[1] - P) // stride + 1
        count += nrow * ncol
        wins_img += list(vi.reshape(nrow * ncol, P, P, im.shape[2]))
        wins_cls += list(vc.reshape(nrow * ncol, P, P))
    aug = scenes.window_table([im.shape for im in images], P, stride, True)
    plain = scenes.window_table([im.shape for im in images], P, stride, False)
    assert aug.dtype == np.int32 and aug.shape == (count * 5, 4) and plain.shape == (count, 4)
    assert (plain[:, 3] == 0).all() and np.array_equal(aug[::5, :3], plain[:, :3])
    gi, gc = scenes.host_windows(images, maps, aug, P)
    pi, pc = scenes.host_windows(images, maps, plain, P)
    for i in range(count):
        assert np.array_equal(pi[i], wins_img[i]) and np.array_equal(pc[i], wins_cls[i]), i
        for j, (ci, cc) in enumerate(zip(reference_copies(wins_img[i]), reference_copies(wins_cls[i]))):
            assert np.array_equal(gi[5 * i + j], ci) and np.array_equal(gc[5 * i + j], cc), (i, j)
    with pytest.raises(ValueError, match="smaller than"):
        scenes.window_table([(31, 90)], 32, 16, True)


# ---- 2. the eight codes -------------------------------------------------------------------------------------------------------
def test_codes_are_the_eight_symmetries():
    rng = np.random.default_rng(2)
    P = 6
    img, cls = scene(rng, P, P, 3, 200)
    table = np.array([[0, 0, 0, c] for c in range(8)], np.int32)
    gi, gc = scenes.host_windows([img], [cls], table, P)
    assert len({gi[c].tobytes() for c in range(8)}) == 8
    assert np.array_equal(gi[5], np.rot90(np.rot90(np.rot90(img))))
    i, j = np.meshgrid(np.arange(P), np.arange(P), indexing="ij")
    formulas = {0: (i, j), 1: (j, P - 1 - i), 2: (P - 1 - i, P - 1 - j), 3: (P - 1 - i, j), 4: (i, P - 1 - j), 5: (P - 1 - j, i),
                6: (j, i), 7: (P - 1 - j, P - 1 - i)}
    for c, (a, b) in formulas.items():
        assert np.array_equal(gi[c], img[a, b]), c
        assert np.array_equal(gc[c], cls[a, b]), c                                        # the class map gets the same transform
    # rectangular patches: the four codes that keep the shape
    img, cls = scene(rng, 4, 7, 2, 200)
    ri, rc = scenes.host_windows([img], [cls], np.array([[0, 0, 0, c] for c in (0, 2, 3, 4)], np.int32), (4, 7))
    i, j = np.meshgrid(np.arange(4), np.arange(7), indexing="ij")
    for k, (a, b) in enumerate([(i, j), (3 - i, 6 - j), (3 - i, j), (i, 6 - j)]):
        assert np.array_equal(ri[k], img[a, b]) and np.array_equal(rc[k], cls[a, b])
    for c in (1, 5, 6, 7):
        with pytest.raises(ValueError, match=f"row 0: code {c} transposes"):
            scenes.host_windows([img], [cls], np.array([[0, 0, 0, c]], np.int32), (4, 7))


# ---- 3. argument validation without a launch ----------------------------------------------------------------------------------
def test_scene_windows_argument_validation_without_launch():
    """Every case breaks exactly one precondition of a valid call, so none of them reaches a launch; ScenePool.batch refuses the
    same rows in the same words."""
    lib = L.lib()
    fn = lib.raw("rua_scene_windows")
    A = 1 << 24                                               # fake, suitably aligned addresses: never dereferenced on the host
    shapes = [(40, 50), (64, 33)]
    n = len(shapes)
    ptrs = (ctypes.c_void_p * n)(A, A)
    hs, ws = (ctypes.c_int32 * n)(*[s[0] for s in shapes]), (ctypes.c_int32 * n)(*[s[1] for s in shapes])
    good = np.array([[0, 8, 18, 0], [1, 32, 1, 7], [0, 0, 0, 4]], np.int32)

    def call(table, PH=32, PW=32, Cin=3, N=None, img_out=A, cls_out=A, scene_cls=ptrs):
        t = np.ascontiguousarray(table, dtype=np.int32)
        return fn(ptrs, scene_cls, hs, ws, n, t.ctypes.data, len(t) if N is None else N, PH, PW, Cin, img_out, cls_out, None)

    general = [(dict(img_out=None), b"required"), (dict(cls_out=None), b"together"), (dict(scene_cls=None), b"together"),
               (dict(N=0), b"N 0"), (dict(Cin=17), b"Cin 17"), (dict(Cin=0), b"Cin 0"), (dict(PH=513), b"512"), (dict(PW=0), b"512"),
               (dict(img_out=A + 2), b"4-byte")]
    for change, msg in general:
        assert call(good, **change) == -1, change
        assert msg in lib.dll.rua_last_error(), (change, lib.dll.rua_last_error())

    pool = scenes.ScenePool([np.zeros(s + (3,), np.uint8) for s in shapes], [np.zeros(s, np.uint8) for s in shapes], device="cpu")
    assert pool.batch(good, 32).shape == (3, 32, 32, 3)
    rows = [([2, 0, 0, 0], "scene 2 outside 0..1"), ([-1, 0, 0, 0], "scene -1 outside 0..1"),
            ([0, 9, 18, 0], "window (9, 18) + 32 x 32 leaves its 40 x 50 scene"),          # one pixel over the bottom border
            ([0, 8, 19, 0], "window (8, 19) + 32 x 32 leaves its 40 x 50 scene"),          # one pixel over the right border
            ([1, 33, 1, 0], "leaves its 64 x 33 scene"), ([1, 32, 2, 0], "leaves its 64 x 33 scene"),
            ([0, -1, 0, 0], "leaves its"), ([0, 0, -1, 0], "leaves its"),
            ([0, 0, 0, 8], "code 8 outside 0..7"), ([0, 0, 0, -1], "code -1 outside 0..7")]
    for at in (0, 2):                                          # the bad row first, and behind two good ones
        for row, msg in rows:
            table = np.concatenate([good[:at], np.array([row], np.int32)])
            assert call(table) == -1, row
            err = lib.dll.rua_last_error().decode()
            assert f"row {at}: " in err and msg in err, (row, err)
            with pytest.raises(ValueError) as exc:
                pool.batch(table, 32)
            assert str(exc.value) == err, (str(exc.value), err)
    for code in (1, 5, 6, 7):                                  # transposing codes on a rectangular patch
        table = np.array([[0, 0, 0, 0], [0, 0, 0, code]], np.int32)
        assert call(table, PH=16, PW=24) == -1
        err = lib.dll.rua_last_error().decode()
        assert f"row 1: code {code} transposes" in err and "16 x 24" in err, err
        with pytest.raises(ValueError) as exc:
            pool.batch(table, (16, 24))
        assert str(exc.value) == err
    with pytest.raises(ValueError, match="N 0"):
        pool.batch(np.zeros((0, 4), np.int32), 32)
    with pytest.raises(ValueError, match="smaller than"):
        scenes.ScenePool([np.zeros((40, 50, 3), np.uint8)], None, patch=64, device="cpu")
    with pytest.raises(ValueError, match="channels"):
        scenes.ScenePool([np.zeros((40, 50, 3), np.uint8), np.zeros((40, 50, 4), np.uint8)], None, device="cpu")
    with pytest.raises(ValueError, match="class map"):
        scenes.ScenePool([np.zeros((40, 50, 3), np.uint8)], [np.zeros((40, 51), np.uint8)], device="cpu")


def test_the_three_table_checkers_share_their_words():
    """One bad table per row rule: check_table, check_own and check_view_table (those of them that have the rule) refuse it with
    the same text under their own kernel's name - only an ownership row's subject differs, a "row" for rua_scene_stitch and a
    "group" for rua_scene_stitch_views.  check_own has its own rule for the code, check_table takes no ownership table."""
    shapes = [(40, 57), (32, 32)]
    good, full = [[0, 0, 0, 0], [1, 0, 0, 0]], [[0, 32, 0, 32]] * 2
    checkers = {"rua_scene_windows": lambda rows, own, patch: scenes.check_table(shapes, np.array(rows), patch),
                "rua_scene_stitch": lambda rows, own, patch: scenes.check_own(shapes, np.array(rows), np.array(own), patch, 5),
                "rua_scene_stitch_views": lambda rows, own, patch: scenes.check_view_table(shapes, np.array(rows), np.array(own), 1, patch, 5)}
    for name, check in checkers.items():                       # the good table passes all three
        check(good, full, 32)
    rules = [((32, 32), [[0, 0, 0, 0], [2, 0, 0, 0]], full, "row 1: scene 2 outside 0..1", tuple(checkers)),
             ((32, 32), [[0, 0, 0, 0], [0, 0, 26, 0]], full, "row 1: window (0, 26) + 32 x 32 leaves its 40 x 57 scene", tuple(checkers)),
             ((32, 32), [[0, 0, 0, 0], [1, 0, 0, 9]], full, "row 1: code 9 outside 0..7", ("rua_scene_windows", "rua_scene_stitch_views")),
             ((16, 48), [[0, 0, 0, 0], [0, 3, 5, 6]], [[0, 16, 0, 48]] * 2, "row 1: code 6 transposes and needs a square patch (got 16 x 48)",
              ("rua_scene_windows", "rua_scene_stitch_views")),
             ((32, 32), good, [[0, 32, 0, 32], [0, 33, 0, 32]], "{what} 1: owned rows 0..33, columns 0..32 outside the 32 x 32 window",
              ("rua_scene_stitch", "rua_scene_stitch_views"))]
    for patch, rows, own, text, who in rules:
        for name in who:
            with pytest.raises(ValueError) as exc:
                checkers[name](rows, own, patch)
            assert str(exc.value) == name + ": " + text.format(what="row" if name == "rua_scene_stitch" else "group"), (name, text)


# ---- 4. converter, scene directories, materialize -----------------------------------------------------------------------------
def test_converter_round_trip_and_scene_directories(tmp_path):
    rng = np.random.default_rng(4)
    H, W = 40, 52
    cls = rng.integers(0, 5, (H, W)).astype(np.uint8)
    colour_of = {v: k for k, v in scenes.ISPRS_COLOURS.items()}
    assert sorted(colour_of) == [0, 1, 2, 3, 4]
    ref_chw = np.stack([np.vectorize(lambda v, ch=ch: colour_of[v][ch])(cls) for ch in range(3)]).astype(np.uint8)
    img_chw = rng.integers(0, 256, (3, H, W)).astype(np.uint8)
    img, back = scenes.convert_reference_inputs(img_chw, ref_chw)
    assert back.dtype == np.uint8 and np.array_equal(back, cls)
    assert img.shape == (H, W, 3) and np.array_equal(img, img_chw.transpose(1, 2, 0))
    bad = ref_chw.copy()
    bad[:, 7, 9] = (1, 2, 3)
    bad[:, 30, 2] = (9, 9, 9)
    with pytest.raises(ValueError, match=r"unknown colour \(1, 2, 3\) at row 7, column 9"):
        scenes.convert_reference_inputs(img_chw, bad)

    # the command line: scene directory + materialised compact layout
    np.save(tmp_path / "Image_Train.npy", img_chw)
    np.save(tmp_path / "Reference_Train.npy", ref_chw)
    root, dst = str(tmp_path / "scene_dir"), str(tmp_path / "patches")
    assert scenes.main(["--image", str(tmp_path / "Image_Train.npy"), "--reference", str(tmp_path / "Reference_Train.npy"), "--dst", root,
                        "--materialize", dst, "-ps", "16", "--stride", "12", "--data_aug", "yes"]) == 0
    names, images, maps = scenes.load_scene_dir(root)
    assert names == ["scene"] and np.array_equal(images[0], img) and np.array_equal(maps[0], cls)
    table = scenes.window_table([img.shape], 16, 12, True)
    assert len(table) == 3 * 4 * 5
    wi, wc = scenes.host_windows([img], [cls], table, 16)
    assert sorted(os.listdir(os.path.join(dst, "images"))) == sorted(scenes.patch_name(k) for k in range(len(table)))
    for k in range(len(table)):
        assert np.array_equal(np.load(os.path.join(dst, "images", f"patch_{k}.npy")), wi[k]), k
        assert np.array_equal(np.load(os.path.join(dst, "labels", "classes", f"patch_{k}.npy")), wc[k]), k
        assert scenes.patch_index(os.path.join(dst, "images", scenes.patch_name(k))) == k

    # several scenes, paired by name; a missing label is reported by name
    two = str(tmp_path / "two")
    a, b = scene(rng, 20, 24), scene(rng, 33, 17)
    scenes.save_scene_dir(two, ["b_scene", "a_scene"], [b[0], a[0]], [b[1], a[1]])
    names, images, maps = scenes.load_scene_dir(two)
    assert names == ["a_scene", "b_scene"]
    assert np.array_equal(images[0], a[0]) and np.array_equal(maps[1], b[1])
    assert scenes.materialize(two, str(tmp_path / "two_patches"), 16, 8, False) == 1 * 2 + 3 * 1   # (20 - 16) // 8 + 1 = 1 row x 2 columns, 3 rows x 1 column
    os.remove(os.path.join(two, "labels", "scenes", "b_scene.npy"))
    with pytest.raises(FileNotFoundError, match="b_scene.npy"):
        scenes.load_scene_dir(two)


# ---- 5. the CLI's listing, split and shards -----------------------------------------------------------------------------------
def test_cli_scene_listing_matches_the_materialised_dataset(tmp_path):
    sys.path.insert(0, ROOT)
    import train_ISPRS as cli
    a = cli.build_parser().parse_args([])
    assert a.scene_dataset is False and a.stride == 32 and a.data_aug is True
    b = cli.build_parser().parse_args("--scene_dataset yes --stride 16 --data_aug no -ps 64 --norm_type 2".split())
    assert b.scene_dataset is True and b.stride == 16 and b.data_aug is False and b.patch_size == 64 and b.norm_type == 2

    rng = np.random.default_rng(5)
    sc = [scene(rng, 40, 44), scene(rng, 24, 30)]
    root, dst = str(tmp_path / "scenes"), str(tmp_path / "patches")
    scenes.save_scene_dir(root, ["s0", "s1"], [s[0] for s in sc], [s[1] for s in sc])
    n = scenes.materialize(root, dst, 16, 8, True)
    assert n == (4 * 4 + 2 * 2) * 5                            # 100 patches: patch_10 sorts before patch_2
    _, images, maps = scenes.load_scene_dir(root)
    table = scenes.window_table([im.shape for im in images], 16, 8, True)
    xs_f, ys_f = cli.list_compact_dataset(dst)
    xs_s, ys_s = cli.list_scene_dataset(len(table))
    assert [os.path.basename(p) for p in xs_f] == xs_s and [os.path.basename(p) for p in ys_f["classes"]] == ys_s["classes"]
    f_tr, fy_tr, f_va, fy_va = cli.split_dataset(xs_f, ys_f)
    s_tr, sy_tr, s_va, sy_va = cli.split_dataset(xs_s, ys_s)
    assert [os.path.basename(p) for p in f_tr] == s_tr and [os.path.basename(p) for p in f_va] == s_va
    assert sy_tr["classes"] == s_tr and sy_va["classes"] == s_va and len(s_tr) + len(s_va) == n
    for path in f_tr + f_va:                                   # every name maps back to the right table row
        k = scenes.patch_index(path)
        wi, wc = scenes.host_windows(images, maps, table[k:k + 1], 16)
        assert np.array_equal(np.load(path), wi[0]), path
        assert np.array_equal(np.load(path.replace(os.path.join("images", ""), os.path.join("labels", "classes", ""))), wc[0]), path

    # a pass of the loader: the file loader's batches, byte for byte, for every rank
    from resunet_a_mltsk_keras_amd.loader import PrefetchLoader
    pool = scenes.ScenePool(images, maps, patch=16, device="cpu")
    order = np.random.default_rng(0).permutation(len(s_tr))
    rows_tr = table[[scenes.patch_index(p) for p in s_tr]]
    for world in (1, 2, 4):
        for rank in range(world):
            files = PrefetchLoader(f_tr, fy_tr, 8, order=order, pin=False, rank=rank, world=world, keep_dtype=True)
            sl = scenes.SceneLoader(pool, rows_tr, 8, order=order, rank=rank, world=world)
            assert len(files) == len(sl) == len(s_tr) // 8
            for (xf, yf), (sb, none) in zip(files, sl):
                assert none is None and sb.shape == tuple(xf.shape)
                wi, wc = sb.host()
                assert np.array_equal(xf.numpy(), wi) and np.array_equal(yf["classes"].numpy(), wc)


def test_scene_batch_shard_is_the_models_local_batch():
    """SceneBatch.shard(rank, world) against the slices Model._local_batch takes of an array batch."""
    from resunet_a_mltsk_keras_amd.keras_api import Model
    rng = np.random.default_rng(6)
    img, cls = scene(rng, 30, 30)
    pool = scenes.ScenePool([img], [cls], patch=8, device="cpu")
    table = scenes.window_table([img.shape], 8, 2, True)[:8]
    batch = pool.batch(table)
    gi, gc = batch.host()

    class Eng:
        world = 1

    class Stub:
        engine = Eng()

    import torch.distributed as dist
    real = dist.get_rank
    try:
        for world in (1, 2, 4):
            Eng.world = world
            for rank in range(world):
                dist.get_rank = lambda group=None, r=rank: r
                xi, yi = Model._local_batch(Stub(), gi, gc)
                sh = batch.shard(rank, world)
                assert len(sh) == 8 // world
                si, sc_ = sh.host()
                assert np.array_equal(si, xi) and np.array_equal(sc_, yi), (world, rank)
    finally:
        dist.get_rank = real
    with pytest.raises(ValueError, match="not divisible"):
        batch.shard(0, 3)
    with pytest.raises(ValueError, match="not divisible"):
        scenes.SceneLoader(pool, table, 8, world=3)
