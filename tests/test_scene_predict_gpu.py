"""GPU tests of whole-scene evaluation: rua_scene_stitch (csrc/scene.hip) byte for byte against scenes.host_stitch through the C ABI,
its argument checks, Engine.predict_scene against host_stitch of the probabilities it stitched, against the existing predict() route,
and eval_scenes_ISPRS.py (the scene-directory counterpart of test_ISPRS.py) against Model.evaluate_scenes."""
import ctypes
import os

import numpy as np
import pytest
import torch

from resunet_a_mltsk_keras_amd import _lib as L
from resunet_a_mltsk_keras_amd import scenes

from _scene_util import FILL, NCLS, blob_pool, blob_scene, conf_pattern, guarded_maps, new_engine, new_model, read_guarded, table_of

pytestmark = pytest.mark.gpu


def make_inputs(seed, shapes, N, PH, PW, C):
    """p: random fp32 with about 5 % of the pixels holding an exact tie at the maximum; class maps uniform in 0..C-1 with some 255s."""
    rng = np.random.default_rng(seed)
    p = rng.random((N, PH, PW, C), dtype=np.float32)
    tie = np.argwhere(rng.random((N, PH, PW)) < 0.05)
    a = rng.integers(0, C, len(tie))
    b = (a + rng.integers(1, C, len(tie))) % C               # another class
    p[tie[:, 0], tie[:, 1], tie[:, 2], a] = 2.0
    p[tie[:, 0], tie[:, 1], tie[:, 2], b] = 2.0
    maps = []
    for H, W in shapes:
        m = rng.integers(0, C, (H, W)).astype(np.uint8)
        m[rng.random((H, W)) < 0.02] = 255
        maps.append(m)
    return p, maps


def run_stitch(p, rows, own, shapes, class_maps, C=None, expect_error=None):
    """rua_scene_stitch into 0xEE-filled maps with a guard region behind each and a pre-filled confusion matrix; returns
    (maps, confusion - its initial pattern or None) and checks the guards.  expect_error: the call must fail with this text and
    leave every output as it was."""
    dev = torch.device("cuda")
    N, PH, PW, Cp = p.shape
    C = Cp if C is None else C
    n = len(shapes)
    pd = torch.from_numpy(np.ascontiguousarray(p)).to(dev)
    pred = guarded_maps(shapes)
    cls = None if class_maps is None else [torch.from_numpy(m).to(dev) for m in class_maps]
    conf0 = conf_pattern(C)
    conf = None if class_maps is None else torch.from_numpy(conf0).to(dev)
    pred_ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in pred])
    cls_ptrs = None if cls is None else (ctypes.c_void_p * n)(*[t.data_ptr() for t in cls])
    hs, ws = (ctypes.c_int32 * n)(*[h for h, _ in shapes]), (ctypes.c_int32 * n)(*[w for _, w in shapes])
    r, o = np.ascontiguousarray(rows, dtype=np.int32), np.ascontiguousarray(own, dtype=np.int32)
    args = (pd.data_ptr(), N, PH, PW, C, r.ctypes.data, o.ctypes.data, pred_ptrs, cls_ptrs, hs, ws, n,
            None if conf is None else conf.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    if expect_error is not None:
        with pytest.raises(L.RuaError, match=expect_error):
            L.lib().call("rua_scene_stitch", *args)
    else:
        L.lib().call("rua_scene_stitch", *args)
    torch.cuda.synchronize()
    maps = read_guarded(pred, shapes)
    cm = None if conf is None else conf.cpu().numpy() - conf0
    if expect_error is not None:
        assert all((m == FILL).all() for m in maps) and (cm is None or (cm == 0).all()), "a refused call wrote something"
    return maps, cm


def assert_stitch(p, rows, own, shapes, class_maps):
    got_maps, got_cm = run_stitch(p, rows, own, shapes, class_maps)
    want_maps, want_cm = scenes.host_stitch(p, rows, own, shapes, class_maps, fill=FILL)
    for s, (g, w) in enumerate(zip(got_maps, want_maps)):
        bad = np.argwhere(g != w)
        assert bad.size == 0, (f"scene {s}", len(bad), "first at", tuple(bad[0]), int(g[tuple(bad[0])]), int(w[tuple(bad[0])]))
    if class_maps is None:
        assert got_cm is None and want_cm is None
    else:
        assert np.array_equal(got_cm, want_cm), (got_cm - want_cm)
    return want_maps


# (40, 57): an odd width, so scene rows start at every byte phase; 57 - 32 = 25 and 40 - 32 = 8 are no multiples of the stride: the
# last windows are flush with the border.  C = 5: a pixel is 20 bytes, owned runs start at every dword phase of a 16-byte piece.
# C = 64: the widest pixel and the largest histogram (test_stitch_wide_windows: several blocks across one window row).
@pytest.mark.parametrize("C", [3, 5, 6, 64])
# The 16 x 48 patch: stride 24 along its 48 columns; along its 16 rows a stride of 24 would exceed the patch (predict_table refuses
# that: the windows would leave gaps), so 12 there.
@pytest.mark.parametrize("shapes,patch,stride", [([(40, 57), (32, 32)], (32, 32), 24), ([(40, 57)], (16, 48), (12, 24))])
def test_stitch_bitwise(shapes, patch, stride, C):
    rows, own = table_of(shapes, patch, stride)
    p, maps = make_inputs(C * 100 + patch[0], shapes, len(rows), patch[0], patch[1], C)
    want = assert_stitch(p, rows, own, shapes, maps)
    assert all((m != FILL).all() for m in want)                # the table covers every pixel
    assert_stitch(p, rows, own, shapes, None)                  # maps only: both pointers null
    half = assert_stitch(p[::2], rows[::2], own[::2], shapes, maps)
    assert any((m == FILL).any() for m in half)                # pixels nobody owns keep their bytes


def test_stitch_one_window():
    """N = 1, and a p of 31 * 33 * 5 floats - no whole number of 16-byte pieces - owned up to its last pixel."""
    p, maps = make_inputs(1, [(33, 47)], 1, 31, 33, 5)
    assert_stitch(p, np.array([[0, 1, 14, 0]], np.int32), np.array([[3, 31, 1, 33]], np.int32), [(33, 47)], maps)


def test_stitch_more_windows_than_one_launch():
    """300 windows (a launch carries 120): stride 1 on three small scenes, the first 300 rows of 361."""
    shapes = [(40, 57), (32, 32), (45, 40)]
    rows, own = table_of(shapes, 32, 1)
    assert len(rows) > 300
    rows, own = rows[:300], own[:300]
    p, maps = make_inputs(2, shapes, 300, 32, 32, 5)
    assert_stitch(p, rows, own, shapes, maps)


@pytest.mark.parametrize("C", [6, 64])
def test_stitch_wide_windows(C):
    """A 40 x 300 window is wider than what one block takes (256 columns; 64 at C = 64): several blocks share a window row."""
    shapes = [(45, 333)]
    p, maps = make_inputs(3, shapes, 2, 40, 300, C)
    rows = np.array([[0, 5, 33, 0], [0, 0, 0, 0]], np.int32)
    own = np.array([[0, 40, 0, 300], [0, 5, 1, 290]], np.int32)
    assert_stitch(p, rows, own, shapes, maps)


def test_stitch_empty_rectangles():
    shapes = [(40, 57), (32, 32)]
    rows, own = table_of(shapes, 32, 24)
    own = own.copy()
    own[3, 1] = own[3, 0]                                      # no rows
    own[5, 3] = own[5, 2]                                      # no columns
    own[len(own) - 1] = 0                                      # the padding row of a last batch
    p, maps = make_inputs(4, shapes, len(rows), 32, 32, 5)
    want = assert_stitch(p, rows, own, shapes, maps)
    assert (want[0] == FILL).any() and (want[1] == FILL).all()


def test_stitch_refuses_bad_arguments():
    shapes = [(40, 57), (32, 32)]
    rows, own = table_of(shapes, 32, 24)
    p, maps = make_inputs(5, shapes, len(rows), 32, 32, 5)

    def with_row(table, k, col, v):
        t = table.copy()
        t[k, col] = v
        return t
    run_stitch(p, with_row(rows, 2, 2, 26), own, shapes, maps, expect_error=r"row 2: window \(0, 26\) \+ 32 x 32 leaves its 40 x 57 scene")
    run_stitch(p, with_row(rows, 4, 1, -1), own, shapes, maps, expect_error="row 4: window")
    run_stitch(p, with_row(rows, 1, 0, 2), own, shapes, maps, expect_error="row 1: scene 2 outside 0..1")
    run_stitch(p, rows, with_row(own, 3, 1, 33), shapes, maps, expect_error=r"row 3: owned rows \d+\.\.33, columns")
    run_stitch(p, rows, with_row(own, 0, 2, 40), shapes, maps, expect_error="row 0: owned rows")
    run_stitch(p, with_row(rows, 5, 3, 1), own, shapes, maps, expect_error="row 5: code 1")
    run_stitch(p, rows, own, shapes, maps, C=65, expect_error="C 65 outside 1..64")
    # the host definition refuses the same rows in the same words
    with pytest.raises(ValueError, match=r"row 2: window \(0, 26\) \+ 32 x 32 leaves its 40 x 57 scene"):
        scenes.host_stitch(p, with_row(rows, 2, 2, 26), own, shapes, maps)
    with pytest.raises(ValueError, match=r"row 3: owned rows \d+\.\.33, columns"):
        scenes.host_stitch(p, rows, with_row(own, 3, 1, 33), shapes, maps)


def test_every_table_entry_point_refuses_the_same_rows_in_the_same_words():
    """The five table rules (scene out of range, window leaving its scene, code 9, a transposing code on a 16 x 48 patch, an owned
    rectangle outside the window) through every entry point that takes a window table: the message is the shared text under the
    entry point's own name, and nothing is written.  A rule an entry point does not have is skipped for it: rua_scene_stitch has
    its own rule for the code, rua_scene_windows and rua_scene_class_counts take no ownership table."""
    shapes, C, N = [(40, 57), (32, 32)], 5, 2
    good, full = np.array([[0, 0, 0, 0], [1, 0, 0, 0]], np.int32), np.array([[0, 32, 0, 32]] * 2, np.int32)
    # rule -> (PH, PW), rows, own, the text behind "NAME: " with the subject of an ownership row left open
    rules = {
        "scene": ((32, 32), [[0, 0, 0, 0], [2, 0, 0, 0]], full, "row 1: scene 2 outside 0..1"),
        "leaves": ((32, 32), [[0, 0, 0, 0], [0, 0, 26, 0]], full, "row 1: window (0, 26) + 32 x 32 leaves its 40 x 57 scene"),
        "code 9": ((32, 32), [[0, 0, 0, 0], [1, 0, 0, 9]], full, "row 1: code 9 outside 0..7"),
        "transposing": ((16, 48), [[0, 0, 0, 0], [0, 3, 5, 6]], [[0, 16, 0, 48]] * 2, "row 1: code 6 transposes and needs a square patch (got 16 x 48)"),
        "owned": ((32, 32), good, [[0, 32, 0, 32], [0, 33, 0, 32]], "{what} 1: owned rows 0..33, columns 0..32 outside the 32 x 32 window"),
    }
    has = {"rua_scene_windows": ("scene", "leaves", "code 9", "transposing"), "rua_scene_class_counts": ("scene", "leaves", "code 9", "transposing"),
           "rua_scene_stitch": ("scene", "leaves", "owned"), "rua_scene_stitch_views": tuple(rules), "rua_scene_stitch_maps": tuple(rules)}
    dev = torch.device("cuda")
    n = len(shapes)
    img = [torch.zeros((H, W, 3), dtype=torch.uint8, device=dev) for H, W in shapes]
    cls = [torch.zeros((H, W), dtype=torch.uint8, device=dev) for H, W in shapes]
    p = torch.zeros((N, 32, 32, C), dtype=torch.float32, device=dev)
    outs = {k: torch.full((size,), FILL, dtype=torch.uint8, device=dev) for k, size in
            (("img", N * 32 * 32 * 3), ("cls", N * 32 * 32), ("conf", C * C * 8), ("counts", N * (C + 1) * 4))}
    maps = guarded_maps(shapes, C)                             # the widest scene map any of the five writes
    ptrs = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])
    hs, ws = (ctypes.c_int32 * n)(*[h for h, _ in shapes]), (ctypes.c_int32 * n)(*[w for _, w in shapes])
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    calls = 0
    for name, mine in has.items():
        for rule in mine:
            (PH, PW), rows, own, text = rules[rule]
            r, o = np.ascontiguousarray(rows, dtype=np.int32), np.ascontiguousarray(own, dtype=np.int32)
            args = {
                "rua_scene_windows": (ptrs(img), ptrs(cls), hs, ws, n, r.ctypes.data, N, PH, PW, 3, outs["img"].data_ptr(), outs["cls"].data_ptr(), stream),
                "rua_scene_class_counts": (ptrs(cls), hs, ws, n, r.ctypes.data, N, PH, PW, C, outs["counts"].data_ptr(), stream),
                "rua_scene_stitch": (p.data_ptr(), N, PH, PW, C, r.ctypes.data, o.ctypes.data, ptrs(maps), ptrs(cls), hs, ws, n, outs["conf"].data_ptr(), stream),
                "rua_scene_stitch_views": (p.data_ptr(), N, 1, PH, PW, C, r.ctypes.data, o.ctypes.data, ptrs(maps), ptrs(cls), hs, ws, n,
                                           outs["conf"].data_ptr(), stream),
                "rua_scene_stitch_maps": (p.data_ptr(), N, 1, PH, PW, C, r.ctypes.data, o.ctypes.data, ptrs(maps), hs, ws, n, 0, stream),
            }[name]
            assert L.lib().raw(name)(*args) == -1, (name, rule)
            want = name + ": " + text.format(what="row" if name == "rua_scene_stitch" else "group")
            assert L.lib().dll.rua_last_error().decode() == want, (name, rule)
            calls += 1
    assert calls == 4 + 4 + 3 + 5 + 5
    torch.cuda.synchronize()
    assert all((t.cpu().numpy() == FILL).all() for t in list(outs.values()) + maps), "a refused call wrote something"


# ---- engine / model level -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pool():
    return blob_pool((128, 128))


@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("multitask", [True, False])
def test_predict_scene_is_host_stitch_of_its_probabilities(pool, multitask, use_graph):
    eng = new_engine(multitask, use_graph)
    ragged = 0
    for scene in (0, 1):
        for stride in (64, 24):
            for batch in (2, 5):
                seen = []
                pred, cm = eng.predict_scene(pool, scene, stride=stride, batch=batch, norm_type=1,
                                             on_batch=lambda r, o, p: seen.append((r.copy(), o.copy(), p.clone())))
                torch.cuda.synchronize()
                table = pool.predict_table(scene, stride)
                ragged += len(table[0]) % batch != 0
                assert len(seen) == -(-len(table[0]) // batch) and all(r.shape == (batch, 4) and tuple(p.shape) == (batch, 64, 64, NCLS) for r, _, p in seen)
                rows, own = np.concatenate([s[0] for s in seen]), np.concatenate([s[1] for s in seen])
                assert np.array_equal(rows[:len(table[0])], table[0]) and np.array_equal(own[:len(table[0])], table[1])
                assert (own[len(table[0]):] == 0).all()        # the padding owns nothing
                probs = np.concatenate([s[2].cpu().numpy() for s in seen])
                assert np.isfinite(probs).all()
                want_maps, want_cm = scenes.host_stitch(probs, rows, own, pool.shapes, pool.class_maps, NCLS)
                what = (scene, stride, batch)
                assert pred.dtype == np.uint8 and pred.shape == pool.shapes[scene] and np.array_equal(pred, want_maps[scene]), what
                assert cm.dtype == np.int64 and np.array_equal(cm, want_cm), what
                again = np.bincount(pool.class_maps[scene].astype(np.int64).ravel() * NCLS + pred.ravel(), minlength=NCLS * NCLS).reshape(NCLS, NCLS)
                assert np.array_equal(cm, again), what
    assert ragged >= 1                                         # a last batch that had to be padded


def test_predict_scene_without_class_maps_and_refusals(pool):
    eng = new_engine(False, True)
    bare = scenes.ScenePool(pool.images, None, patch=64)
    pred, cm = eng.predict_scene(bare, 1, stride=64, batch=2)
    assert cm is None and np.array_equal(pred, eng.predict_scene(pool, 1, stride=64, batch=2)[0])
    with pytest.raises(ValueError, match="norm_type"):
        eng.predict_scene(pool, 0, norm_type=3)
    with pytest.raises(ValueError, match="stride"):
        eng.predict_scene(pool, 0, stride=65)
    with pytest.raises(ValueError, match="scene 2"):
        eng.predict_scene(pool, 2)
    with pytest.raises(ValueError, match="batch"):
        eng.predict_scene(pool, 0, batch=0)
    with pytest.raises(ValueError, match="patch"):
        eng.predict_scene(scenes.ScenePool(pool.images, None, patch=32), 0)


def test_predict_scene_against_the_predict_route(pool):
    """The 128 x 128 scene at stride 64 (four tiles, owned in full): the map against the mosaic of np.argmax(Model.predict(...)["seg"]).
    Two predict calls that agree bitwise demand exact equality; otherwise agreement wherever the first call's top-two margin exceeds
    ten times the largest difference between the calls (the twins rule), and that must exclude less than 1 % of the pixels."""
    m = new_model()
    rows, own = pool.predict_table(1, 64)
    a = m.predict(pool.batch(rows), batch_size=2, norm_type=1)["seg"]
    b = m.predict(pool.batch(rows), batch_size=2, norm_type=1)["seg"]
    pred, cm = m.predict_scene(pool, 1, stride=64, batch=2, norm_type=1)
    assert (own == [0, 64, 0, 64]).all() and cm.sum() == 128 * 128

    def mosaic(tiles):
        out = np.zeros((128, 128), tiles.dtype)
        for t, (_, r, c, _) in zip(tiles, rows.tolist()):
            out[r:r + 64, c:c + 64] = t
        return out
    want = mosaic(np.argmax(a, -1))
    if np.array_equal(a, b):
        print("predict is deterministic: exact comparison")
        assert np.array_equal(pred, want)
    else:
        spread = float(np.abs(a - b).max())
        top = np.sort(a, axis=-1)
        sure = mosaic(top[..., -1] - top[..., -2] > 10 * spread)
        print(f"predict differs between calls by up to {spread:.3g}: {100 * (1 - sure.mean()):.3f} % of the pixels excluded")
        assert 1 - sure.mean() < 0.01
        assert np.array_equal(pred[sure], want[sure])


def test_cli_scores_a_scene_directory(tmp_path):
    """eval_scenes_ISPRS.py --scene_dataset yes --stride 32 on a tiny scene directory: its maps, matrix and metrics against evaluate_scenes."""
    import eval_scenes_ISPRS
    from resunet_a_mltsk_keras_amd.keras_api import load_model
    sc = [blob_scene(300, 90, 70), blob_scene(301, 64, 100)]
    root, path, out = str(tmp_path / "scenes"), str(tmp_path / "m.h5"), str(tmp_path / "preds")
    scenes.save_scene_dir(root, ["a_tile", "b_tile"], [s[0] for s in sc], [s[1] for s in sc])
    new_model(seed=11, depth=4, split_k=True).save(path)         # four levels: a small file; split_k as load_model leaves it
    res = eval_scenes_ISPRS.main(["--use_multitasking", "--model_path", path, "--dataset_path", root, "-ps", "64", "--num_classes", str(NCLS),
                           "--output_path", out, "--scene_dataset", "yes", "--stride", "32", "--batch_size", "4"])
    names, images, class_maps = scenes.load_scene_dir(root)
    maps, cm = load_model(path, compile=False).evaluate_scenes(scenes.ScenePool(images, class_maps, patch=64), stride=32, batch_size=4, norm_type=1)
    assert cm.sum() == 90 * 70 + 64 * 100 and np.array_equal(res["confusion_matrix"], cm)
    per_scene = 0
    for name, want, (img, _) in zip(names, maps, sc):
        got = np.load(os.path.join(out, f"pred_seg_reconstructed_{name}.npy"))
        assert got.dtype == np.uint8 and np.array_equal(got, want)
        per_scene = per_scene + np.load(os.path.join(out, f"confusion_matrix_{name}.npy"))
        assert os.path.getsize(os.path.join(out, f"pred_seg_reconstructed_{name}.ppm")) > 3 * want.size
    assert np.array_equal(per_scene, cm)
    acc, f1, rec, prec = eval_scenes_ISPRS.metrics_from_confusion(cm)
    assert res["accuracy"] == acc and np.array_equal(res["f1"], f1) and np.array_equal(res["recall"], rec) and np.array_equal(res["precision"], prec)
    assert acc == pytest.approx(100.0 * np.concatenate([(m == c).ravel() for m, c in zip(maps, class_maps)]).mean())
