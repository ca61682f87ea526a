"""GPU tests of the eroded ground truth: rua_scene_erode (csrc/scene.hip) through the C ABI, byte for byte against scenes.host_erode
and count for count against scenes.host_erode_confusion - several scenes of odd widths in one call, scenes smaller than the radius,
class edges on the kernel's tile borders, accumulation, a cell of 2^20 counts and the refusals - then ScenePool.eroded_maps,
Model.predict_scene(erode=) and eval_scenes_ISPRS.py --erode_boundary.  Bytes and integers only: every comparison is exact."""
import ctypes
import os

import numpy as np
import pytest
import torch

from resunet_a_mltsk_keras_amd import _lib as L
from resunet_a_mltsk_keras_amd import scenes

from _scene_util import FILL, NCLS, blob_scene, conf_pattern, guarded_maps, new_model

pytestmark = pytest.mark.gpu

TILE_H, TILE_W = 32, 256                                     # csrc/scene.hip: SE_TH, SE_TW
CONF_GUARD = 64                                              # int64 cells behind the matrix
RADII = [0, 1, 2, 3, 7, 16]
# one call: a single pixel, a flat and a tall sliver, a scene smaller than every radius from 3 on in both directions, and one that
# spans three tiles down and across; odd widths, so every row starts at another byte phase
SHAPES = [(1, 1), (5, 300), (300, 1), (2, 3), (2 * TILE_H + 11, 2 * TILE_W + 19)]


def blocky(seed, H, W, C=5, region=16):
    """Uniform region x region blocks of classes 0..C-1 with a sprinkle of 255 and of the value C (both "no class")."""
    rng = np.random.default_rng(seed)
    f = rng.integers(0, C, (H // region + 1, W // region + 1)).astype(np.uint8)
    m = np.ascontiguousarray(np.kron(f, np.ones((region, region), np.uint8))[:H, :W])
    m[rng.random(m.shape) < 0.003] = 255
    m[rng.random(m.shape) < 0.003] = C
    return m


def run_erode(maps, r, preds=None, C=0, out=True, expect_error=None, nscenes=None, tweak=None):
    """rua_scene_erode on these class maps: the eroded maps into FILL-ed buffers with a guard region behind each (out=False: no
    scene_out), the matrix (with preds) into a pre-filled one with guard cells behind it.  Calls twice: the maps must be identical
    both times and the second call must add to the matrix what the first added.  Returns (maps or None, int64 [C][C] or None).
    tweak(a) may change the argument dict before the call; expect_error: the call must fail with RUA_ERR_ARG and this text and
    leave every buffer as it was."""
    dev = torch.device("cuda")
    n = len(maps)
    shapes = [m.shape for m in maps]
    cls = [torch.from_numpy(np.ascontiguousarray(m)).to(dev) for m in maps]
    outs = guarded_maps(shapes)
    prd = None if preds is None else [torch.from_numpy(np.ascontiguousarray(p)).to(dev) for p in preds]
    cells = max(C, 1) ** 2
    conf0 = np.concatenate([conf_pattern(max(C, 1)).ravel(), np.full(CONF_GUARD, -7, np.int64)])
    conf = torch.from_numpy(conf0).to(dev)
    arr = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])
    a = dict(cls=arr(cls), h=(ctypes.c_int32 * n)(*[s[0] for s in shapes]), w=(ctypes.c_int32 * n)(*[s[1] for s in shapes]),
             n=n if nscenes is None else nscenes, r=r, out=arr(outs) if out else None, pred=None if prd is None else arr(prd), C=C,
             conf=None if prd is None else conf.data_ptr())
    if tweak is not None:
        tweak(a)
    args = (a["cls"], a["h"], a["w"], a["n"], a["r"], a["out"], a["pred"], a["C"], a["conf"], ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    def fetch():
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in outs], conf.cpu().numpy(), [t.cpu().numpy() for t in cls]
    if expect_error is not None:
        assert L.lib().raw("rua_scene_erode")(*args) == -1
        err = L.lib().dll.rua_last_error().decode()
        assert err.startswith("rua_scene_erode: ") and expect_error in err, err
        o, c, k = fetch()
        assert all((x == FILL).all() for x in o) and np.array_equal(c, conf0), "a refused call wrote something"
        assert all(np.array_equal(x, m) for x, m in zip(k, maps))
        return None
    L.lib().call("rua_scene_erode", *args)
    o1, c1, _ = fetch()
    L.lib().call("rua_scene_erode", *args)
    o2, c2, k = fetch()
    assert all(np.array_equal(x, m) for x, m in zip(k, maps)), "the class maps were written"
    for x, y, (H, W) in zip(o1, o2, shapes):
        assert (x[H * W:] == FILL).all(), "bytes behind an eroded map were written"
        assert np.array_equal(x, y), "a second call gave another map"
        if not out:
            assert (x == FILL).all()
    assert (c1[cells:] == -7).all() and (c2[cells:] == -7).all(), "cells behind the matrix were written"
    got_maps = [x[:H * W].reshape(H, W) for x, (H, W) in zip(o1, shapes)] if out else None
    if prd is None:
        assert np.array_equal(c1, conf0) and np.array_equal(c2, conf0)
        return got_maps, None
    cm = (c1 - conf0)[:cells].reshape(C, C)
    assert np.array_equal((c2 - c1)[:cells].reshape(C, C), cm), "the second call did not add what the first added"
    return got_maps, cm


def assert_maps(got, maps, r):
    for s, (g, m) in enumerate(zip(got, maps)):
        want = scenes.host_erode(m, r)
        bad = np.argwhere(g != want)
        assert bad.size == 0, (f"scene {s} {m.shape} radius {r}", len(bad), "first at", tuple(bad[0]), int(g[tuple(bad[0])]), int(want[tuple(bad[0])]))


@pytest.fixture(scope="module")
def five_maps():
    maps = [blocky(10 + s, H, W) for s, (H, W) in enumerate(SHAPES)]
    for m in maps:
        if m.size >= 256:                                       # "everything eroded" must not hide a wrong interior
            kept = float((scenes.host_erode(m, 3) != 255).mean())
            assert 0.2 <= kept <= 0.9, (m.shape, kept)
    return maps


# ---- 1. bytes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", RADII)
def test_erode_bytes_of_five_scenes_in_one_call(five_maps, r):
    assert any(H > 2 * TILE_H and W > 2 * TILE_W and W % 2 for H, W in SHAPES) and any(max(s) < 3 for s in SHAPES)
    got, cm = run_erode(five_maps, r)
    assert cm is None
    assert_maps(got, five_maps, r)


def test_one_pixel_erodes_the_lattice_disc_and_a_uniform_map_nothing():
    one = np.full((41, 41), 2, np.uint8)
    one[20, 20] = 4
    flat = np.full((TILE_H + 9, TILE_W + 45), 3, np.uint8)
    for r in RADII:
        (g1, g2), _ = run_erode([one, flat], r)
        assert np.array_equal(g2, flat)
        assert np.array_equal(g1, scenes.host_erode(one, r))
        if r == 3:
            assert int((g1 == 255).sum()) == 29
            assert g1[23, 20] == 255 and g1[22, 22] == 255 and g1[23, 21] == 2 and g1[21, 23] == 2


@pytest.mark.parametrize("r", [1, 3, 16])
def test_class_edges_on_tile_borders(r):
    """A horizontal edge between rows TILE_H - 1 and TILE_H, a vertical one between columns TILE_W - 1 and TILE_W, and both one
    pixel further, where the tile's halo has to bring the other class in."""
    H, W = 2 * TILE_H + 5, 2 * TILE_W + 7
    maps = []
    for row, col in [(TILE_H, W), (H, TILE_W), (TILE_H, TILE_W), (TILE_H + 1, TILE_W - 1), (2 * TILE_H, 2 * TILE_W)]:
        m = np.zeros((H, W), np.uint8)
        m[row:, :] = 1
        m[:, col:] += 2
        maps.append(m)
    got, _ = run_erode(maps, r)
    assert_maps(got, maps, r)
    assert (got[2][TILE_H - r:TILE_H + r, :] == 255).all() and (got[2][:, TILE_W - r:TILE_W + r] == 255).all()
    assert got[2][TILE_H - r - 1, 0] == 0 and got[2][0, TILE_W + r] == 2


# ---- 2. the matrix ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 5, 6, 64])
def test_confusion_against_the_host(C):
    rng = np.random.default_rng(C)
    shapes = [(TILE_H + 13, TILE_W + 31), (5, 300), (1, 1)]
    maps = [blocky(C * 10 + s, H, W, C=C) for s, (H, W) in enumerate(shapes)]
    preds = [rng.integers(0, C + 1, s).astype(np.uint8) for s in shapes]          # the value C: a prediction that is skipped
    for p in preds:
        p[rng.random(p.shape) < 0.01] = 255
    for r in (0, 3, 7):
        want = sum(scenes.host_erode_confusion(m, p, r, C) for m, p in zip(maps, preds))
        both_maps, both = run_erode(maps, r, preds, C)
        assert np.array_equal(both, want), (r, both - want)
        assert_maps(both_maps, maps, r)
        none, alone = run_erode(maps, r, preds, C, out=False)                       # the matrix alone: no scene_out
        assert none is None and np.array_equal(alone, want)
        assert want.sum() <= sum(int(((m < C) & (p < C)).sum()) for m, p in zip(maps, preds))
    assert any((p >= C).any() for p in preds) and any((m >= C).any() for m in maps)


def test_uniform_map_puts_2_to_20_counts_into_one_cell():
    m, p = np.full((1024, 1024), 2, np.uint8), np.full((1024, 1024), 4, np.uint8)
    _, cm = run_erode([m], 3, [p], 6)
    want = np.zeros((6, 6), np.int64)
    want[2, 4] = 1 << 20
    assert np.array_equal(cm, want)
    p[:, ::2] = 6                                               # every other prediction is no class: skipped
    _, cm = run_erode([m], 3, [p], 6, out=False)
    want[2, 4] = 1 << 19
    assert np.array_equal(cm, want)


# ---- 3. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_leave_every_buffer_alone():
    rng = np.random.default_rng(7)
    maps = [blocky(70, 40, 57), blocky(71, 33, 20)]
    preds = [rng.integers(0, 5, m.shape).astype(np.uint8) for m in maps]
    run_erode(maps, -1, preds, 5, expect_error="radius -1 outside 0..16")
    run_erode(maps, 17, preds, 5, expect_error="radius 17 outside 0..16")
    run_erode(maps, 3, None, 0, out=False, expect_error="nothing to do")
    run_erode(maps, 3, preds, 5, tweak=lambda a: a.update(conf=None), expect_error="scene_pred and confusion go together")
    run_erode(maps, 3, preds, 5, tweak=lambda a: a.update(pred=None), expect_error="scene_pred and confusion go together")
    run_erode(maps, 3, preds, 0, expect_error="C 0 outside 1..64")
    run_erode(maps, 3, preds, 65, expect_error="C 65 outside 1..64")
    run_erode(maps, 3, preds, 5, tweak=lambda a: a["out"].__setitem__(1, a["cls"][1]), expect_error="scene 1: scene_out is scene_cls")
    run_erode(maps, 3, preds, 5, tweak=lambda a: a["pred"].__setitem__(0, None), expect_error="scene 0: null pointer")
    run_erode(maps, 3, preds, 5, tweak=lambda a: a["cls"].__setitem__(1, None), expect_error="scene 1: null pointer")
    run_erode(maps, 3, preds, 5, nscenes=0, expect_error="nscenes 0")
    run_erode(maps, 3, preds, 5, tweak=lambda a: a["h"].__setitem__(1, 0), expect_error="scene 1: size 0 x 20")
    run_erode(maps, 3, preds, 5, tweak=lambda a: a.update(conf=a["conf"] + 4), expect_error="8-byte aligned")
    got, cm = run_erode(maps, 3, preds, 5)                      # and the same arguments, unbroken, go through
    assert_maps(got, maps, 3)
    assert np.array_equal(cm, sum(scenes.host_erode_confusion(m, p, 3, 5) for m, p in zip(maps, preds)))


# ---- 4. ScenePool.eroded_maps -------------------------------------------------------------------------------------------------
def test_pool_eroded_maps_equal_the_cpu_pools(five_maps):
    images = [np.zeros(m.shape + (1,), np.uint8) for m in five_maps]
    gpu, cpu = scenes.ScenePool(images, five_maps), scenes.ScenePool(images, five_maps, device="cpu")
    got, want = gpu.eroded_maps(3), cpu.eroded_maps(3)
    assert len(got) == len(want) and all(g.dtype == np.uint8 and np.array_equal(g, w) for g, w in zip(got, want))
    with pytest.raises(ValueError, match="radius 17 outside 0..16"):
        gpu.eroded_maps(17)
    with pytest.raises(ValueError, match="class maps"):
        scenes.ScenePool(images, None).eroded_maps(3)


# ---- 5. predict_scene(erode=), as tests/test_scene_predict_gpu.py builds its model and scenes ----------------------------------
def test_predict_scene_scores_on_the_eroded_ground_truth():
    sc = [blob_scene(200, 97, 113), blob_scene(201, 64, 80)]
    pool = scenes.ScenePool([s[0] for s in sc], [s[1] for s in sc], patch=64)
    m = new_model()
    for s, views in [(0, (0,)), (1, (0,)), (0, "flips")]:
        res = m.predict_scene(pool, s, stride=32, batch=4, erode=3, views=views)
        assert len(res) == 3
        pred, cm, cm_e = res
        cls = pool.class_maps[s]
        assert cm_e.dtype == np.int64 and np.array_equal(cm_e, scenes.host_erode_confusion(cls, pred, 3, NCLS)), (s, views)
        assert (cm_e <= cm).all() and 0 < cm_e.sum() < cm.sum() == cls.size
        plain = m.predict_scene(pool, s, stride=32, batch=4, erode=0, views=views)
        assert len(plain) == 2 and np.array_equal(plain[0], pred) and np.array_equal(plain[1], cm)
        if views == (0,):
            # radius 0 in matrix mode on this prediction is the matrix rua_scene_stitch counted
            _, cm0 = run_erode([cls], 0, [pred], NCLS, out=False)
            assert np.array_equal(cm0, cm)
    maps, total, total_e = m.evaluate_scenes(pool, stride=32, batch_size=4, erode=3)
    assert np.array_equal(total_e, sum(scenes.host_erode_confusion(c, p, 3, NCLS) for c, p in zip(pool.class_maps, maps)))
    assert len(m.evaluate_scenes(pool, stride=32, batch_size=4)) == 2
    bare = scenes.ScenePool(pool.images, None, patch=64)
    with pytest.raises(ValueError, match="class maps"):
        m.predict_scene(bare, 0, stride=32, batch=4, erode=3)
    with pytest.raises(ValueError, match="radius 17 outside 0..16"):
        m.predict_scene(pool, 0, stride=32, batch=4, erode=17)


def test_cli_erode_boundary(tmp_path, capsys):
    import eval_scenes_ISPRS
    from resunet_a_mltsk_keras_amd.keras_api import load_model
    sc = [blob_scene(300, 90, 70), blob_scene(301, 64, 100)]
    root, path = str(tmp_path / "scenes"), str(tmp_path / "m.h5")
    scenes.save_scene_dir(root, ["a_tile", "b_tile"], [s[0] for s in sc], [s[1] for s in sc])
    new_model(seed=11, depth=4, split_k=True).save(path)
    base = ["--use_multitasking", "--model_path", path, "--dataset_path", root, "-ps", "64", "--num_classes", str(NCLS),
            "--scene_dataset", "yes", "--stride", "32", "--batch_size", "4"]
    plain = eval_scenes_ISPRS.main(base + ["--output_path", str(tmp_path / "plain")])
    assert "Eroded ground truth" not in capsys.readouterr().out and not any(k.endswith("_eroded") for k in plain)
    res = eval_scenes_ISPRS.main(base + ["--output_path", str(tmp_path / "eroded"), "--erode_boundary", "3"])
    assert "Eroded ground truth (radius 3)" in capsys.readouterr().out.splitlines()
    names, images, class_maps = scenes.load_scene_dir(root)
    _, cm, cm_e = load_model(path, compile=False).evaluate_scenes(scenes.ScenePool(images, class_maps, patch=64), stride=32, batch_size=4,
                                                                  norm_type=1, erode=3)
    per_scene = sum(np.load(tmp_path / "eroded" / f"confusion_matrix_eroded_{n}.npy") for n in names)
    assert np.array_equal(res["confusion_matrix_eroded"], per_scene) and np.array_equal(per_scene, cm_e)
    acc, f1, rec, prec = eval_scenes_ISPRS.metrics_from_confusion(cm_e)
    assert res["accuracy_eroded"] == acc and np.array_equal(res["f1_eroded"], f1)
    assert np.array_equal(res["recall_eroded"], rec) and np.array_equal(res["precision_eroded"], prec)
    for k in ("accuracy", "f1", "recall", "precision", "confusion_matrix"):          # the unsuffixed keys and files: as without the flag
        assert np.array_equal(res[k], plain[k]), k
    assert np.array_equal(res["confusion_matrix"], cm)
    for n in names:
        for f in (f"pred_seg_reconstructed_{n}.npy", f"confusion_matrix_{n}.npy"):
            assert np.array_equal(np.load(tmp_path / "plain" / f), np.load(tmp_path / "eroded" / f)), f
        assert not os.path.exists(tmp_path / "plain" / f"confusion_matrix_eroded_{n}.npy")
