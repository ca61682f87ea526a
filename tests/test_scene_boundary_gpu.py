"""GPU tests of the boundary F1: rua_scene_boundary (csrc/scene.hip) through the C ABI, byte for byte against scenes.host_boundaries
and count for count against scenes.host_boundary_counts - several scenes of odd widths in one call, scenes smaller than the
radius, class edges on the kernel's tile borders, matches that lie in the neighbouring tile's halo, the edge of the disc,
accumulation, a cell of 2^19 counts, more scenes than one launch carries and the refusals - then ScenePool.boundary_counts /
boundary_maps, Model.predict_scene(boundary=), evaluate_scenes and eval_scenes_ISPRS.py --boundary_f1.  Bytes and integers only:
every comparison is exact."""
import ctypes
import os

import numpy as np
import pytest
import torch

from resunet_a_mltsk_keras_amd import _lib as L
from resunet_a_mltsk_keras_amd import scenes

from _scene_util import FILL, NCLS, blob_scene, guarded_maps, new_model

pytestmark = pytest.mark.gpu

TILE_H, TILE_W = 32, 128                                     # csrc/scene.hip: SB_TH, SB_TW
CHUNK = 96                                                   # csrc/scene.hip: SB_CHUNK, scenes per launch
CNT_GUARD = 64                                               # int64 cells behind the counts
RADII = [0, 1, 2, 3, 7, 16]
# one call: a single pixel, a flat and a tall sliver, a scene smaller than every radius from 3 on in both directions, and one that
# spans three tiles down and across; odd widths, so every row starts at another byte phase
SHAPES = [(1, 1), (5, 300), (300, 1), (2, 3), (2 * TILE_H + 11, 2 * TILE_W + 19)]
ALL = ("cls", "pred", "counts")


def blocky(seed, H, W, C=6, region=16):
    """Uniform region x region blocks of classes 0..C-1 with a sprinkle of 255 and of the value C (both "no class")."""
    rng = np.random.default_rng(seed)
    f = rng.integers(0, C, (H // region + 1, W // region + 1)).astype(np.uint8)
    m = np.ascontiguousarray(np.kron(f, np.ones((region, region), np.uint8))[:H, :W])
    m[rng.random(m.shape) < 0.003] = 255
    m[rng.random(m.shape) < 0.003] = C
    return m


def rolled(m, seed, C=6, noise=0.01):
    """A prediction: the map rolled by (2, 1) with `noise` of its pixels redrawn (the sprinkled no-class bytes travel along)."""
    rng = np.random.default_rng(seed)
    p = np.roll(m, (2, 1), (0, 1)).copy()
    k = rng.random(p.shape) < noise
    p[k] = rng.integers(0, C, int(k.sum())).astype(np.uint8)
    return p


def cnt_pattern(C):
    return (np.arange(4 * C, dtype=np.int64) * 7 + 3) * (1 << 33) + 5                     # non-zero in both halves of every cell


def run_boundary(maps, preds, r, C, want=ALL, expect_error=None, nscenes=None, tweak=None, same=False):
    """rua_scene_boundary on these class and prediction maps (same=True: scene_pred is scene_cls, the very pointers): the boundary
    maps into FILL-ed buffers with a guard region behind each, the counts into a pre-filled buffer with guard cells behind it;
    `want` names the outputs that are given.  Calls twice: the maps must be identical both times and the second call must add to
    the counts what the first added.  Returns (boundary maps of the class maps or None, of the predictions or None, int64 [C][4]
    or None).  tweak(a) may change the argument dict before the call; expect_error: the call must fail with RUA_ERR_ARG and this
    text and leave every buffer as it was."""
    dev = torch.device("cuda")
    n = len(maps)
    shapes = [m.shape for m in maps]
    cls = [torch.from_numpy(np.ascontiguousarray(m)).to(dev) for m in maps]
    prd = cls if same else [torch.from_numpy(np.ascontiguousarray(p)).to(dev) for p in preds]
    outs = {k: guarded_maps(shapes) for k in ("cls", "pred")}
    cells = 4 * min(max(C, 1), 64)
    cnt0 = np.concatenate([cnt_pattern(cells // 4), np.full(CNT_GUARD, -7, np.int64)])
    cnt = torch.from_numpy(cnt0).to(dev)
    arr = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])
    a = dict(cls=arr(cls), pred=arr(prd), h=(ctypes.c_int32 * n)(*[s[0] for s in shapes]), w=(ctypes.c_int32 * n)(*[s[1] for s in shapes]),
             n=n if nscenes is None else nscenes, r=r, C=C, bc=arr(outs["cls"]) if "cls" in want else None,
             bp=arr(outs["pred"]) if "pred" in want else None, cnt=cnt.data_ptr() if "counts" in want else None)
    if tweak is not None:
        tweak(a)
    args = (a["cls"], a["pred"], a["h"], a["w"], a["n"], a["r"], a["C"], a["bc"], a["bp"], a["cnt"], ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    def fetch():
        torch.cuda.synchronize()
        return {k: [t.cpu().numpy() for t in v] for k, v in outs.items()}, cnt.cpu().numpy(), [t.cpu().numpy() for t in cls], [t.cpu().numpy() for t in prd]
    if expect_error is not None:
        assert L.lib().raw("rua_scene_boundary")(*args) == -1
        err = L.lib().dll.rua_last_error().decode()
        assert err.startswith("rua_scene_boundary: ") and expect_error in err, err
        o, c, k, q = fetch()
        assert all((x == FILL).all() for v in o.values() for x in v) and np.array_equal(c, cnt0), "a refused call wrote something"
        assert all(np.array_equal(x, m) for x, m in zip(k, maps)) and all(np.array_equal(x, p) for x, p in zip(q, maps if same else preds))
        return None
    L.lib().call("rua_scene_boundary", *args)
    o1, c1, _, _ = fetch()
    L.lib().call("rua_scene_boundary", *args)
    o2, c2, k, q = fetch()
    assert all(np.array_equal(x, m) for x, m in zip(k, maps)), "the class maps were written"
    assert all(np.array_equal(x, p) for x, p in zip(q, maps if same else preds)), "the prediction maps were written"
    got = {}
    for key in ("cls", "pred"):
        for x, y, (H, W) in zip(o1[key], o2[key], shapes):
            assert (x[H * W:] == FILL).all(), "bytes behind a boundary map were written"
            assert np.array_equal(x, y), "a second call gave another map"
            if key not in want:
                assert (x == FILL).all()
        got[key] = [x[:H * W].reshape(H, W) for x, (H, W) in zip(o1[key], shapes)] if key in want else None
    assert (c1[cells:] == -7).all() and (c2[cells:] == -7).all(), "cells behind the counts were written"
    if "counts" not in want:
        assert np.array_equal(c1, cnt0) and np.array_equal(c2, cnt0)
        return got["cls"], got["pred"], None
    counts = (c1 - cnt0)[:cells].reshape(C, 4)
    assert np.array_equal((c2 - c1)[:cells].reshape(C, 4), counts), "the second call did not add what the first added"
    return got["cls"], got["pred"], counts


def assert_maps(got, maps, C, what=""):
    for s, (g, m) in enumerate(zip(got, maps)):
        want = scenes.host_boundaries(m, C)
        bad = np.argwhere(g != want)
        assert bad.size == 0, (f"{what} scene {s} {m.shape} C {C}", len(bad), "first at", tuple(bad[0]), int(g[tuple(bad[0])]), int(want[tuple(bad[0])]))


def host_counts(maps, preds, r, C):
    return sum(scenes.host_boundary_counts(m, p, r, C) for m, p in zip(maps, preds))


def assert_all(maps, preds, r, C, **kw):
    bc, bp, counts = run_boundary(maps, preds, r, C, **kw)
    assert_maps(bc, maps, C, "class map")
    assert_maps(bp, maps if kw.get("same") else preds, C, "prediction")
    want = host_counts(maps, maps if kw.get("same") else preds, r, C)
    assert np.array_equal(counts, want), (r, C, (counts - want).tolist())
    return counts


@pytest.fixture(scope="module")
def five():
    maps = [blocky(10 + s, H, W) for s, (H, W) in enumerate(SHAPES)]
    preds = [rolled(m, 40 + s) for s, m in enumerate(maps)]
    b = scenes.host_boundaries(maps[-1], 6)
    assert 0.05 <= float((b != 255).mean()) <= 0.6               # "everything is boundary" must not hide a wrong interior
    return maps, preds


# ---- 1. through the C ABI: maps and counts ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", RADII)
def test_five_scenes_in_one_call(five, r):
    assert any(H > 2 * TILE_H and W > 2 * TILE_W and W % 2 for H, W in SHAPES) and any(max(s) < 3 for s in SHAPES)
    maps, preds = five
    assert any((m >= 6).any() for m in maps) and any((p >= 6).any() for p in preds)
    counts = assert_all(maps, preds, r, 6)
    assert (counts[:, 0] > 0).all() and (counts[:, 2] > 0).all()
    if r == 0:
        assert (counts[:, 1] < counts[:, 0]).all()
    if r == 16:
        assert (counts[:, 3] > 0.9 * counts[:, 2]).all()


@pytest.mark.parametrize("C", [1, 5, 6, 64])
def test_class_counts_and_each_output_alone(C):
    shapes = [(TILE_H + 13, TILE_W + 31), (5, 300), (1, 1)]
    maps = [blocky(C * 10 + s, H, W, C=C) for s, (H, W) in enumerate(shapes)]
    preds = [rolled(m, C * 10 + 5 + s, C=C) for s, m in enumerate(maps)]
    assert any((p >= C).any() for p in preds) and any((m >= C).any() for m in maps)
    for r in (0, 3, 7):
        want = assert_all(maps, preds, r, C)
        bc, bp, counts = run_boundary(maps, preds, r, C, want=("counts",))
        assert bc is None and bp is None and np.array_equal(counts, want)
    bc, bp, counts = run_boundary(maps, preds, 3, C, want=("cls",))
    assert bp is None and counts is None
    assert_maps(bc, maps, C)
    bc, bp, counts = run_boundary(maps, preds, 3, C, want=("pred",))
    assert bc is None and counts is None
    assert_maps(bp, preds, C)


@pytest.mark.parametrize("r", [1, 3, 16])
def test_class_edges_on_and_beside_tile_borders(r):
    """A horizontal edge between rows TILE_H - 1 and TILE_H, a vertical one between columns TILE_W - 1 and TILE_W, and both one
    pixel further, where the tile's halo has to bring the other class in; the prediction has its edges one pixel off."""
    H, W = 2 * TILE_H + 5, 2 * TILE_W + 7
    maps, preds = [], []
    for row, col in [(TILE_H, W), (H, TILE_W), (TILE_H, TILE_W), (TILE_H + 1, TILE_W - 1), (2 * TILE_H, 2 * TILE_W)]:
        for m, d in ((np.zeros((H, W), np.uint8), 0), (np.zeros((H, W), np.uint8), 1)):
            m[row - d:, :] = 1
            m[:, col + d:] += 2
            (preds if d else maps).append(m)
    assert_all(maps, preds, r, 4)
    bc, _, _ = run_boundary(maps[2:3], preds[2:3], r, 4)
    b = bc[0]
    assert (b[TILE_H - 1, :TILE_W] == 0).all() and (b[TILE_H, :TILE_W] == 1).all() and (b[TILE_H - 2, :TILE_W - 1] == 255).all()
    assert (b[:TILE_H, TILE_W - 1] == 0).all() and (b[:TILE_H, TILE_W] == 2).all() and b[0, 0] == 255 and b[H - 1, W - 1] == 255


@pytest.mark.parametrize("r", [1, 2, 3, 7, 16])
def test_a_match_that_lies_radius_inside_the_neighbouring_tile(r):
    """Single pixels of class 1 on class 0: the prediction's on the last row (column) of a tile, the class map's `r` rows (columns)
    further, inside the next tile - and the other way round.  A halo one short loses the match."""
    H, W = 2 * TILE_H + 3, 2 * TILE_W + 5
    cases = [((TILE_H - 1, 40), (TILE_H - 1 + r, 40)), ((TILE_H, 41), (TILE_H - r, 41)),
             ((9, TILE_W - 1), (9, TILE_W - 1 + r)), ((10, TILE_W), (10, TILE_W - r)), ((TILE_H - 1, TILE_W - 1), (TILE_H - 1 + r, TILE_W - 1))]
    maps, preds = [], []
    for own, other in cases:
        t, p = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
        p[own], t[other] = 1, 1
        maps.append(t)
        preds.append(p)
    for t, p in zip(maps, preds):                                # scene by scene, so that a lost match cannot hide in a sum
        counts = assert_all([t], [p], r, 2)
        assert counts[1].tolist() == [1, 1, 1, 1], (r, counts.tolist())
        if r >= 2:
            short = assert_all([t], [p], r - 1, 2)
            assert short[1].tolist() == [1, 0, 1, 0]
    assert_all(maps, preds, r, 2)


@pytest.mark.parametrize("r", [1, 3, 7, 16])
def test_the_edge_of_the_disc(r):
    """A pair exactly r apart along an axis matches, a pair at (r, 1) does not; inside a tile and across tile borders."""
    H, W = TILE_H + 2 * r + 5, TILE_W + 2 * r + 8
    for y, x in [(20, 20), (TILE_H - 2, TILE_W - 2), (TILE_H + r, TILE_W + r)]:
        for dy, dx, hit in [(r, 0, 1), (-r, 0, 1), (0, r, 1), (0, -r, 1), (r, 1, 0), (-r, -1, 0), (1, r, 0), (-1, -r, 0)]:
            t, p = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
            p[y, x], t[y + dy, x + dx] = 1, 1
            counts = assert_all([t], [p], r, 2)
            assert counts[1].tolist() == [1, hit, 1, hit], (r, (y, x), (dy, dx), counts.tolist())


def test_pred_is_cls_a_uniform_map_and_no_class_bytes(five):
    maps, _ = five
    for r in (0, 3):
        counts = assert_all(maps, None, r, 6, same=True)         # the very pointers: both are only read
        assert np.array_equal(counts[:, 0], counts[:, 1]) and np.array_equal(counts[:, 2], counts[:, 3]) and np.array_equal(counts[:, 0], counts[:, 2])
    flat = np.full((TILE_H + 9, TILE_W + 45), 3, np.uint8)
    bc, bp, counts = run_boundary([flat], [flat.copy()], 16, 6)
    assert (bc[0] == 255).all() and (bp[0] == 255).all() and not counts.any()
    none = np.full((40, 50), 200, np.uint8)                      # no class anywhere: no boundary, whatever differs
    none[::3, ::5] = 7
    bc, bp, counts = run_boundary([none], [none.T.copy().reshape(40, 50)], 3, 6)
    assert (bc[0] == 255).all() and (bp[0] == 255).all() and not counts.any()


def test_checkerboard_puts_2_to_19_counts_into_a_cell():
    i, j = np.mgrid[0:1024, 0:1024]
    board = ((i + j) & 1).astype(np.uint8)
    _, _, counts = run_boundary([board], None, 0, 2, want=("counts",), same=True)           # every pixel is a boundary pixel of its class
    assert np.array_equal(counts, np.full((2, 4), 1 << 19, np.int64))
    other = (1 - board).astype(np.uint8)
    _, _, counts = run_boundary([board], [other], 0, 2, want=("counts",))                   # the classes exchanged: nothing coincides
    assert np.array_equal(counts, np.array([[1 << 19, 0, 1 << 19, 0]] * 2, np.int64))
    _, _, counts = run_boundary([board], [other], 1, 2, want=("counts",))                   # ... and everything has a partner one pixel away
    assert np.array_equal(counts, np.full((2, 4), 1 << 19, np.int64))


def test_more_scenes_than_one_launch_carries():
    rng = np.random.default_rng(5)
    n = CHUNK + 9
    shapes = [(int(rng.integers(1, 40)), int(rng.integers(1, 150))) for _ in range(n)]
    shapes[CHUNK - 1], shapes[CHUNK] = (TILE_H + 3, TILE_W + 2), (3, 2 * TILE_W + 1)          # the largest grids on either side of the cut
    maps = [blocky(500 + s, H, W, region=5) for s, (H, W) in enumerate(shapes)]
    preds = [rolled(m, 700 + s) for s, m in enumerate(maps)]
    assert_all(maps, preds, 2, 6)


# ---- 2. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_leave_every_buffer_alone():
    maps = [blocky(70, 40, 57), blocky(71, 33, 20)]
    preds = [rolled(m, 72 + s) for s, m in enumerate(maps)]
    run = lambda **kw: run_boundary(maps, preds, kw.pop("r", 3), kw.pop("C", 6), **kw)
    run(r=-1, expect_error="radius -1 outside 0..16")
    run(r=17, expect_error="radius 17 outside 0..16")
    run(C=0, expect_error="C 0 outside 1..64")
    run(C=65, expect_error="C 65 outside 1..64")
    run(nscenes=0, expect_error="nscenes 0")
    run(want=(), expect_error="nothing to do")
    run(tweak=lambda a: a.update(cls=None), expect_error="are required")
    run(tweak=lambda a: a.update(pred=None), expect_error="are required")
    run(tweak=lambda a: a.update(w=None), expect_error="are required")
    run(tweak=lambda a: a["cls"].__setitem__(1, None), expect_error="scene 1: null pointer")
    run(tweak=lambda a: a["pred"].__setitem__(0, None), expect_error="scene 0: null pointer")
    run(tweak=lambda a: a["bc"].__setitem__(1, None), expect_error="scene 1: null pointer")
    run(tweak=lambda a: a["bp"].__setitem__(0, None), expect_error="scene 0: null pointer")
    run(tweak=lambda a: a["h"].__setitem__(1, 0), expect_error="scene 1: size 0 x 20")
    run(tweak=lambda a: a["w"].__setitem__(0, -3), expect_error="scene 0: size 40 x -3")
    def oversized(a):                                            # 2^40 pixels: one too many; refused before anything is launched
        a["h"][1] = a["w"][1] = 1 << 20
    run(tweak=oversized, expect_error="scene 1: size 1048576 x 1048576")
    run(tweak=lambda a: a.update(cnt=a["cnt"] + 4), expect_error="8-byte aligned")
    run(tweak=lambda a: a["bc"].__setitem__(1, a["cls"][1]), expect_error="scene 1: bound_cls overlaps an input map")
    run(tweak=lambda a: a["bc"].__setitem__(0, a["pred"][0]), expect_error="scene 0: bound_cls overlaps an input map")
    run(tweak=lambda a: a["bp"].__setitem__(1, a["pred"][1]), expect_error="scene 1: bound_pred overlaps an input map")
    run(tweak=lambda a: a["bp"].__setitem__(0, a["cls"][0] + 57), expect_error="scene 0: bound_pred overlaps an input map")
    run(tweak=lambda a: a["bp"].__setitem__(1, a["bc"][1]), expect_error="scene 1: bound_cls overlaps bound_pred")
    # an output may share no byte with an input or an output of ANOTHER scene of the call either, nor may the counts with a map
    run(tweak=lambda a: a["bc"].__setitem__(1, a["cls"][0] + 100), expect_error="scene 1: bound_cls overlaps scene 0: scene_cls")
    run(tweak=lambda a: a["bp"].__setitem__(1, a["pred"][0] + 5), expect_error="scene 1: bound_pred overlaps scene 0: scene_pred")
    run(tweak=lambda a: a["bc"].__setitem__(1, a["bp"][0] + 8), expect_error="scene 1: bound_cls overlaps scene 0: bound_pred")
    run(tweak=lambda a: a.update(cnt=a["cls"][0] + 16), expect_error="counts overlaps scene 0: scene_cls")
    run(tweak=lambda a: a.update(cnt=a["bp"][1] - 8), expect_error="scene 1: bound_pred overlaps counts")
    _, _, counts = run(tweak=lambda a: a["pred"].__setitem__(1, a["cls"][1]))               # inputs may share a map
    assert np.array_equal(counts, host_counts(maps, [preds[0], maps[1]], 3, 6))
    assert_all(maps, preds, 3, 6)                                # and the same arguments, unbroken, go through


# ---- 3. ScenePool.boundary_counts / boundary_maps -----------------------------------------------------------------------------
def test_pool_counts_and_maps_equal_the_cpu_pools(five):
    maps, preds = five
    images = [np.zeros(m.shape + (1,), np.uint8) for m in maps]
    gpu, cpu = scenes.ScenePool(images, maps), scenes.ScenePool(images, maps, device="cpu")
    for r in (0, 3):
        got, want = gpu.boundary_counts(preds, r, 6), cpu.boundary_counts(preds, r, 6)
        assert got.dtype == np.int64 and got.shape == (5, 6, 4) and np.array_equal(got, want)
    some = [preds[0], None, preds[2], None, preds[4]]
    assert np.array_equal(gpu.boundary_counts(some, 3, 6), cpu.boundary_counts(some, 3, 6))
    got, want = gpu.boundary_maps(6), cpu.boundary_maps(6)
    assert len(got) == len(want) and all(g.dtype == np.uint8 and np.array_equal(g, w) for g, w in zip(got, want))
    with pytest.raises(ValueError, match="radius 17 outside 0..16"):
        gpu.boundary_counts(preds, 17, 6)
    with pytest.raises(ValueError, match="class maps"):
        scenes.ScenePool(images, None).boundary_counts(preds, 3, 6)
    with pytest.raises(ValueError, match="class maps"):
        scenes.ScenePool(images, None).boundary_maps(6)


# ---- 4. predict_scene(boundary=), as tests/test_scene_predict_gpu.py builds its model and scenes ---------------------------------
@pytest.fixture(scope="module")
def model_and_pool():
    sc = [blob_scene(200, 97, 113), blob_scene(201, 64, 80)]
    return new_model(), scenes.ScenePool([s[0] for s in sc], [s[1] for s in sc], patch=64)


def test_predict_scene_counts_the_boundaries_of_the_map_it_returns(model_and_pool):
    m, pool = model_and_pool
    for s, views in [(0, (0,)), (1, (0,)), (0, "flips")]:
        plain = m.predict_scene(pool, s, stride=32, batch=4, views=views)
        for r in (3, 0):
            res = m.predict_scene(pool, s, stride=32, batch=4, views=views, boundary=r)
            assert len(res) == 3
            pred, cm, counts = res
            assert counts.dtype == np.int64 and counts.shape == (NCLS, 4)
            assert np.array_equal(counts, scenes.host_boundary_counts(pool.class_maps[s], pred, r, NCLS)), (s, views, r)
            assert len(plain) == 2 and np.array_equal(plain[0], pred) and np.array_equal(plain[1], cm)
            assert counts[:, 2].sum() > 0
    bare = scenes.ScenePool(pool.images, None, patch=64)
    with pytest.raises(ValueError, match="class maps"):
        m.predict_scene(bare, 0, stride=32, batch=4, boundary=3)
    with pytest.raises(ValueError, match="radius 17 outside 0..16"):
        m.predict_scene(pool, 0, stride=32, batch=4, boundary=17)
    assert len(m.predict_scene(bare, 0, stride=32, batch=4)) == 2


def test_predict_scene_boundary_together_with_erode_and_heads(model_and_pool):
    m, pool = model_and_pool
    base = m.predict_scene(pool, 0, stride=32, batch=4, erode=3, heads=("bound",))
    res = m.predict_scene(pool, 0, stride=32, batch=4, erode=3, heads=("bound",), boundary=3)
    assert len(base) == 4 and len(res) == 5
    pred, cm, cm_e, counts, head_maps = res
    assert np.array_equal(pred, base[0]) and np.array_equal(cm, base[1]) and np.array_equal(cm_e, base[2])
    assert list(head_maps) == ["bound"] and np.array_equal(head_maps["bound"], base[3]["bound"])
    want = scenes.host_boundary_counts(pool.class_maps[0], pred, 3, NCLS)
    assert np.array_equal(counts, want)
    pred, cm, cm_e, counts = m.predict_scene(pool, 0, stride=32, batch=4, erode=3, boundary=3)
    assert np.array_equal(cm_e, base[2]) and np.array_equal(counts, want)
    pred, cm, counts, head_maps = m.predict_scene(pool, 0, stride=32, batch=4, heads=("bound",), boundary=3)
    assert np.array_equal(counts, want) and np.array_equal(head_maps["bound"], base[3]["bound"])


def test_evaluate_scenes_sums_the_counts(model_and_pool):
    m, pool = model_and_pool
    per = [m.predict_scene(pool, s, stride=32, batch=4, boundary=3)[2] for s in range(len(pool))]
    maps, total, counts = m.evaluate_scenes(pool, stride=32, batch_size=4, boundary=3)
    assert np.array_equal(counts, sum(per))
    assert np.array_equal(counts, sum(scenes.host_boundary_counts(c, p, 3, NCLS) for c, p in zip(pool.class_maps, maps)))
    assert np.array_equal(pool.boundary_counts(maps, 3, NCLS), np.stack(per))
    maps2, total2, total_e, counts2, heads = m.evaluate_scenes(pool, stride=32, batch_size=4, erode=3, heads="bound", boundary=3)
    assert np.array_equal(counts2, counts) and np.array_equal(total2, total) and len(heads) == len(pool) and total_e.shape == total.shape
    assert np.array_equal(total_e, m.evaluate_scenes(pool, stride=32, batch_size=4, erode=3)[2])
    assert len(m.evaluate_scenes(pool, stride=32, batch_size=4)) == 2
    assert np.array_equal(m.evaluate_scenes(pool, stride=32, batch_size=4, boundary=0)[2],
                          sum(scenes.host_boundary_counts(c, p, 0, NCLS) for c, p in zip(pool.class_maps, maps)))


def test_cli_boundary_f1(tmp_path, capsys):
    import eval_scenes_ISPRS
    from resunet_a_mltsk_keras_amd.keras_api import load_model
    sc = [blob_scene(300, 90, 70), blob_scene(301, 64, 100)]
    root, path = str(tmp_path / "scenes"), str(tmp_path / "m.h5")
    scenes.save_scene_dir(root, ["a_tile", "b_tile"], [s[0] for s in sc], [s[1] for s in sc])
    new_model(seed=11, depth=4, split_k=True).save(path)
    base = ["--use_multitasking", "--model_path", path, "--dataset_path", root, "-ps", "64", "--num_classes", str(NCLS),
            "--scene_dataset", "yes", "--stride", "32", "--batch_size", "4"]
    plain = eval_scenes_ISPRS.main(base + ["--output_path", str(tmp_path / "plain")])
    out_plain = capsys.readouterr().out.splitlines()
    assert not any("Boundary" in line for line in out_plain) and not any(k.startswith("boundary") for k in plain)
    res = eval_scenes_ISPRS.main(base + ["--output_path", str(tmp_path / "bf"), "--boundary_f1", "3"])
    out = capsys.readouterr().out.splitlines()
    at = out.index("Boundary F1 (tolerance 3 px)")
    assert out[at - 1] == "" and out[:at - 1] == out_plain, "the blocks before the new one changed"
    assert set(res) - set(plain) == {"boundary_counts", "boundary_precision", "boundary_recall", "boundary_f1", "boundary_f1_mean"}
    for k in plain:
        assert np.array_equal(res[k], plain[k]), k
    names, images, class_maps = scenes.load_scene_dir(root)
    _, cm, counts = load_model(path, compile=False).evaluate_scenes(scenes.ScenePool(images, class_maps, patch=64), stride=32, batch_size=4,
                                                                    norm_type=1, boundary=3)
    per_scene = [np.load(tmp_path / "bf" / f"boundary_counts_{n}.npy") for n in names]
    assert all(p.dtype == np.int64 and p.shape == (NCLS, 4) for p in per_scene)
    assert np.array_equal(res["boundary_counts"], sum(per_scene)) and np.array_equal(sum(per_scene), counts)
    for n, p, c in zip(names, per_scene, class_maps):
        pred = np.load(tmp_path / "bf" / f"pred_seg_reconstructed_{n}.npy")
        assert np.array_equal(p, scenes.host_boundary_counts(c, pred, 3, NCLS))
    want = scenes.boundary_scores(counts)
    assert np.array_equal(res["boundary_precision"], want["precision"], equal_nan=True) and np.array_equal(res["boundary_recall"], want["recall"], equal_nan=True)
    assert np.array_equal(res["boundary_f1"], want["f1"], equal_nan=True) and res["boundary_f1_mean"] == want["f1_mean"]
    assert np.array_equal(res["confusion_matrix"], cm)
    for n in names:
        for f in (f"pred_seg_reconstructed_{n}.npy", f"confusion_matrix_{n}.npy"):
            assert np.array_equal(np.load(tmp_path / "plain" / f), np.load(tmp_path / "bf" / f)), f
        assert not os.path.exists(tmp_path / "plain" / f"boundary_counts_{n}.npy")
