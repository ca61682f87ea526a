"""GPU tests of the connected regions and the sieve: rua_scene_regions and rua_scene_sieve (csrc/regions.hip) through the C ABI, bit
for bit against scenes.host_regions / host_region_counts / host_sieve, on the smallest maps at which a tiled union-find can go wrong;
the refusals; ScenePool.region_counts / sieved_maps; Engine.predict_scene(sieve=), Model.evaluate_scenes and the command line on the
64 x 64 model and the blob scenes of tests/_scene_util.py.  Bytes and integers only: every comparison is exact."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from resunet_a_mltsk_keras_amd import _lib as L
from resunet_a_mltsk_keras_amd import scenes
from _scene_util import FILL, GUARD, NCLS, blob_scene, new_model
from test_scene_regions_host import serpentine

pytestmark = pytest.mark.gpu

TILE = 32                                      # RG_T of csrc/regions.hip: a block labels a TILE x TILE tile, seams lie between tiles
CHUNK = 120                                    # RG_CHUNK: scenes per launch of rua_scene_regions (rua_scene_sieve: 80)
C6 = 6
BIG = 1 << 20                                  # a min_area above every region of these maps


def _maps():
    rng = np.random.default_rng(17)
    out = [np.full((1, 1), 2, np.uint8), rng.integers(0, 2, (1, 300)).astype(np.uint8), rng.integers(0, 2, (300, 1)).astype(np.uint8),
           np.array([[1, 0], [0, 1]], np.uint8)]
    for k, H in enumerate((TILE - 1, TILE, TILE + 1, 2 * TILE + 1)):          # blocks of 5 x 5 pixels with speckle: regions cross every seam
        for W in (TILE - 1, TILE, TILE + 1, 2 * TILE + 1):
            f = rng.integers(0, 3, (H // 5 + 1, W // 5 + 1)).astype(np.uint8)
            m = np.ascontiguousarray(np.kron(f, np.ones((5, 5), np.uint8))[:H, :W])
            m[rng.random(m.shape) < 0.03] = 3
            out.append(m)
    out += [blob_scene(100)[1], blob_scene(101, 97, 260)[1], np.full((130, 257), 1, np.uint8), serpentine(200, 203)]
    comb = np.zeros((70, 131), np.uint8)                                      # a spine along the bottom, teeth one pixel wide: joined last
    comb[:, ::2] = 1
    comb[-1] = 1
    rings = np.maximum(np.abs(np.arange(99) - 49)[:, None], np.abs(np.arange(99) - 49)[None, :])
    rings = ((rings // 2) % 3).astype(np.uint8)                               # square rings two pixels wide: every region encloses the next
    board = (np.add.outer(np.arange(70), np.arange(90)) % 2).astype(np.uint8)
    out += [comb, rings, board, rng.integers(0, 4, (75, 83)).astype(np.uint8), rng.integers(0, 256, (66, 70)).astype(np.uint8)]
    return out


MAPS = _maps()


@functools.lru_cache(maxsize=None)
def host_regions(connectivity):
    return [scenes.host_regions(m, connectivity) for m in MAPS]


def guarded(shapes, unit):
    return [torch.full((H * W * unit + GUARD,), FILL, dtype=torch.uint8, device="cuda") for H, W in shapes]


def read32(bufs, shapes):
    out = []
    for t, (H, W) in zip(bufs, shapes):
        g = t.cpu().numpy()
        assert (g[4 * H * W:] == FILL).all(), "bytes behind an int32 map were written"
        out.append(g[:4 * H * W].view(np.int32).reshape(H, W))
    return out


def read8(bufs, shapes):
    out = []
    for t, (H, W) in zip(bufs, shapes):
        g = t.cpu().numpy()
        assert (g[H * W:] == FILL).all(), "bytes behind a map were written"
        out.append(g[:H * W].reshape(H, W))
    return out


def pattern(n):
    return (np.arange(n, dtype=np.int64) * 7 + 3) * (1 << 33) + 5             # non-zero in both halves of every cell


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def arr(ts):
    return (ctypes.c_void_p * len(ts))(*[t if t is None or isinstance(t, int) else t.data_ptr() for t in ts])


def run_regions(maps, connectivity, min_area=1, C=C6, counts=True, areas=True, expect_error=None, tweak=None):
    """rua_scene_regions on these maps in ONE call: labels and areas into FILL-ed buffers with a guard region behind each, the
    counts onto a non-zero pattern with guard cells behind it.  Returns (labels, areas or None, what was added to the counts or
    None).  tweak(a) may change the argument dict; expect_error: the call must fail with RUA_ERR_ARG and this text and leave every
    buffer as it was."""
    n, shapes = len(maps), [m.shape for m in maps]
    dev = [torch.from_numpy(np.ascontiguousarray(m)).cuda() for m in maps]
    lab, are = guarded(shapes, 4), guarded(shapes, 4)
    cnt0 = np.concatenate([pattern(3 * min(max(C, 1), 64)), np.full(16, -7, np.int64)])
    cnt = torch.from_numpy(cnt0).cuda()
    a = dict(map=arr(dev), h=(ctypes.c_int32 * n)(*[s[0] for s in shapes]), w=(ctypes.c_int32 * n)(*[s[1] for s in shapes]), n=n, conn=connectivity,
             lab=arr(lab), are=arr(are) if areas else None, mn=min_area, C=C, cnt=cnt.data_ptr() if counts else None)
    if tweak is not None:
        tweak(a)
    args = (a["map"], a["h"], a["w"], a["n"], a["conn"], a["lab"], a["are"], a["mn"], a["C"], a["cnt"], stream())
    if expect_error is not None:
        assert L.lib().raw("rua_scene_regions")(*args) == -1
        err = L.lib().dll.rua_last_error().decode()
        assert err.startswith("rua_scene_regions: ") and expect_error in err, err
        torch.cuda.synchronize()
        assert all((t.cpu().numpy() == FILL).all() for t in lab + are) and np.array_equal(cnt.cpu().numpy(), cnt0), "a refused call wrote something"
        return None
    L.lib().call("rua_scene_regions", *args)
    torch.cuda.synchronize()
    assert all(np.array_equal(t.cpu().numpy(), m) for t, m in zip(dev, maps)), "the maps were written"
    c = cnt.cpu().numpy()
    assert (c[-16:] == -7).all(), "cells behind the counts were written"
    added = (c[:-16] - cnt0[:-16]).reshape(-1, 3) if counts else None
    if not counts:
        assert np.array_equal(c, cnt0)
    if areas:
        got_areas = read32(are, shapes)
    else:
        assert all((t.cpu().numpy() == FILL).all() for t in are)
        got_areas = None
    return read32(lab, shapes), got_areas, added


def run_sieve(maps, connectivity, min_area, C, mode, classes=None, expect_error=None, tweak=None):
    """rua_scene_regions, then rua_scene_sieve on its labels and areas, all maps in one call each: the sieved maps into FILL-ed
    guarded buffers, `changed` onto a non-zero pattern.  Returns (maps, what was added to changed)."""
    n, shapes = len(maps), [m.shape for m in maps]
    mn, C_, md, conn, mask, _ = scenes.check_sieve(min_area, C, mode, connectivity, classes)
    dev = [torch.from_numpy(np.ascontiguousarray(m)).cuda() for m in maps]
    lab = [torch.empty((H * W,), dtype=torch.int32, device="cuda") for H, W in shapes]
    are = [torch.empty((H * W,), dtype=torch.int32, device="cuda") for H, W in shapes]
    hs, ws = (ctypes.c_int32 * n)(*[s[0] for s in shapes]), (ctypes.c_int32 * n)(*[s[1] for s in shapes])
    L.lib().call("rua_scene_regions", arr(dev), hs, ws, n, conn, arr(lab), arr(are), 1, 1, None, stream())
    out = guarded(shapes, 1)
    nwork = sum(int(L.lib().raw("rua_scene_sieve_work_bytes")(H, W, C_)) for H, W in shapes)
    assert nwork == 12 * sum(H * W for H, W in shapes)
    work = torch.full((nwork + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    ch0 = np.concatenate([pattern(1), np.full(4, -7, np.int64)])
    ch = torch.from_numpy(ch0).cuda()
    a = dict(map=arr(dev), h=hs, w=ws, n=n, conn=conn, mn=mn, C=C_, mask=mask, mode=md, lab=arr(lab), are=arr(are), out=arr(out),
             work=work.data_ptr(), nwork=nwork, ch=ch.data_ptr())
    if tweak is not None:
        tweak(a)
    args = (a["map"], a["h"], a["w"], a["n"], a["conn"], a["mn"], a["C"], a["mask"], a["mode"], a["lab"], a["are"], a["out"], a["work"], a["nwork"],
            a["ch"], stream())
    if expect_error is not None:
        assert L.lib().raw("rua_scene_sieve")(*args) == -1
        err = L.lib().dll.rua_last_error().decode()
        assert err.startswith("rua_scene_sieve: ") and expect_error in err, err
        torch.cuda.synchronize()
        assert all((t.cpu().numpy() == FILL).all() for t in out + [work]) and np.array_equal(ch.cpu().numpy(), ch0), "a refused call wrote something"
        return None
    L.lib().call("rua_scene_sieve", *args)
    torch.cuda.synchronize()
    assert all(np.array_equal(t.cpu().numpy(), m) for t, m in zip(dev, maps)), "the maps were written"
    assert (work.cpu().numpy()[nwork:] == FILL).all(), "bytes behind the work buffer were written"
    if md == 0:
        assert (work.cpu().numpy() == FILL).all(), "mode void wrote the work buffer"
    c = ch.cpu().numpy()
    assert (c[1:] == -7).all(), "cells behind changed were written"
    return read8(out, shapes), int(c[0] - ch0[0])


# ---- 1. regions ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [4, 8])
def test_regions_equal_the_host_definition(connectivity):
    want = host_regions(connectivity)
    labels, areas, added = run_regions(MAPS, connectivity, min_area=8, C=C6)
    for k, m in enumerate(MAPS):
        assert np.array_equal(labels[k], want[k][0]), (k, m.shape, "labels")
        assert np.array_equal(areas[k], want[k][1]), (k, m.shape, "areas")
    assert np.array_equal(added, sum(scenes.host_region_counts(m, 8, C6, connectivity) for m in MAPS))
    assert int((want[-3][1] > 0).sum()) == (6300 if connectivity == 4 else 2)            # the checkerboard


def test_regions_without_areas_or_counts_and_other_thresholds():
    want = host_regions(4)
    labels, areas, added = run_regions(MAPS, 4, counts=False, areas=False)
    assert areas is None and added is None and all(np.array_equal(g, w[0]) for g, w in zip(labels, want))
    for mn, C in ((1, 4), (70, 64), (BIG, 1), ((1 << 31) - 1, 3)):
        _, _, added = run_regions(MAPS[-6:], 8, min_area=mn, C=C)
        assert np.array_equal(added, sum(scenes.host_region_counts(m, mn, C, 8) for m in MAPS[-6:])), (mn, C)


def test_more_scenes_than_one_launch_holds():
    rng = np.random.default_rng(23)
    maps = [rng.integers(0, 3, (int(rng.integers(1, 40)), int(rng.integers(1, 40)))).astype(np.uint8) for _ in range(CHUNK + 7)]
    maps[3], maps[CHUNK + 2] = MAPS[20], MAPS[21]                                        # larger scenes among small ones: blocks without a tile
    labels, areas, added = run_regions(maps, 4, min_area=3, C=3)
    for k, m in enumerate(maps):
        l, a = scenes.host_regions(m, 4)
        assert np.array_equal(labels[k], l) and np.array_equal(areas[k], a), k
    assert np.array_equal(added, sum(scenes.host_region_counts(m, 3, 3, 4) for m in maps))
    got, changed = run_sieve(maps, 4, 3, 3, "fill")
    want = [scenes.host_sieve(m, 3, 3, "fill") for m in maps]
    assert all(np.array_equal(g, w) for g, w in zip(got, want)) and changed == sum(int((w != m).sum()) for w, m in zip(want, maps))


# ---- 2. the sieve ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_area", [1, 2, 8, 70, BIG])
@pytest.mark.parametrize("mode", ["void", "fill"])
@pytest.mark.parametrize("connectivity", [4, 8])
def test_sieve_equals_the_host_definition(connectivity, mode, min_area):
    got, changed = run_sieve(MAPS, connectivity, min_area, 4, mode)
    total = 0
    for k, m in enumerate(MAPS):
        want = scenes.host_sieve(m, min_area, 4, mode, connectivity)
        assert np.array_equal(got[k], want), (k, m.shape)
        total += int((want != m).sum())
    assert changed == total
    if min_area == 1:
        assert changed == 0


@pytest.mark.parametrize("mode", ["void", "fill"])
def test_sieve_of_a_class_subset_and_many_classes(mode):
    some = MAPS[20:]
    for C, classes, conn in ((4, (1, 3), 4), (4, (), 8), (64, (0, 2, 63), 8), (1, None, 4), (2, (1,), 4)):
        got, changed = run_sieve(some, conn, 8, C, mode, classes)
        want = [scenes.host_sieve(m, 8, C, mode, conn, classes) for m in some]
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), (C, classes)
        assert changed == sum(int((w != m).sum()) for w, m in zip(want, some))


# ---- 3. refusals: RUA_ERR_ARG, the offender named, nothing written -----------------------------------------------------------------
def test_regions_refusals():
    maps = [MAPS[8], MAPS[5]]
    run = lambda **kw: run_regions(maps, kw.pop("connectivity", 4), **kw)
    run(connectivity=6, expect_error="connectivity 6 is neither 4 nor 8")
    run(min_area=0, expect_error="min_area 0 outside 1..2147483647")
    run(min_area=1 << 31, expect_error="min_area 2147483648 outside")
    run(C=0, expect_error="C 0 outside 1..64")
    run(C=65, expect_error="C 65 outside 1..64")
    run(areas=False, expect_error="counts needs areas")
    run(tweak=lambda a: a.update(n=0), expect_error="nscenes 0")
    run(tweak=lambda a: a.update(map=None), expect_error="are required")
    run(tweak=lambda a: a.update(lab=None), expect_error="are required")
    run(tweak=lambda a: a["map"].__setitem__(1, None), expect_error="scene 1: null pointer")
    run(tweak=lambda a: a["lab"].__setitem__(0, None), expect_error="scene 0: null pointer")
    run(tweak=lambda a: a["are"].__setitem__(1, None), expect_error="scene 1: null pointer")
    run(tweak=lambda a: a["h"].__setitem__(1, 0), expect_error="scene 1: size 0 x")
    run(tweak=lambda a: a["w"].__setitem__(0, -3), expect_error="x -3")

    def oversized(a):                                            # 2^31 pixels: one too many for an int32 label
        a["h"][1], a["w"][1] = 1 << 16, 1 << 15
    run(tweak=oversized, expect_error="scene 1: size 65536 x 32768")
    run(tweak=lambda a: a.update(cnt=a["cnt"] + 4), expect_error="8-byte aligned")
    run(tweak=lambda a: a["lab"].__setitem__(1, a["lab"][1] + 2), expect_error="scene 1: labels and areas must be 4-byte aligned")
    run(tweak=lambda a: a["are"].__setitem__(0, a["lab"][0] + 8), expect_error="scene 0: areas overlaps scene 0: labels")
    run(tweak=lambda a: a["lab"].__setitem__(1, a["map"][0] & ~3), expect_error="overlaps")
    run(tweak=lambda a: a.update(cnt=a["lab"][1] + 8), expect_error="overlaps")
    run(counts=False, min_area=0, C=0)                           # min_area and C are read only with counts


def test_sieve_refusals():
    maps = [MAPS[8], MAPS[5]]
    run = lambda **kw: run_sieve(maps, 4, 8, 4, kw.pop("mode", "fill"), **kw)
    run(tweak=lambda a: a.update(conn=5), expect_error="connectivity 5 is neither 4 nor 8")
    run(tweak=lambda a: a.update(mn=0), expect_error="min_area 0 outside")
    run(tweak=lambda a: a.update(mn=1 << 31), expect_error="min_area 2147483648 outside")
    run(tweak=lambda a: a.update(C=65), expect_error="C 65 outside 1..64")
    run(tweak=lambda a: a.update(mode=2), expect_error="mode 2 is neither void (0) nor fill (1)")
    run(tweak=lambda a: a.update(mask=1 << 4), expect_error="class_mask 0x10 names a class outside 0..3")
    run(tweak=lambda a: a.update(n=0), expect_error="nscenes 0")
    for key in ("map", "lab", "are", "out"):
        run(tweak=lambda a, key=key: a.update({key: None}), expect_error="are required")
        run(tweak=lambda a, key=key: a[key].__setitem__(1, None), expect_error="scene 1: null pointer")
    run(tweak=lambda a: a["h"].__setitem__(0, 0), expect_error="scene 0: size 0 x")
    run(tweak=lambda a: a.update(work=None), expect_error="mode fill needs a 4-byte aligned work buffer")
    run(tweak=lambda a: a.update(nwork=a["nwork"] - 1), expect_error="work_bytes")
    run(tweak=lambda a: a.update(ch=a["ch"] + 4), expect_error="8-byte aligned")
    run(tweak=lambda a: a["out"].__setitem__(1, a["map"][1]), expect_error="scene 1: scene_out overlaps scene 1: scene_map")
    run(tweak=lambda a: a["out"].__setitem__(0, a["map"][1] + 5), expect_error="overlaps")
    run(tweak=lambda a: a["out"].__setitem__(0, a["lab"][0] + 64), expect_error="overlaps")
    run(tweak=lambda a: a["out"].__setitem__(1, a["are"][0] + 64), expect_error="overlaps")
    run(tweak=lambda a: a["out"].__setitem__(1, a["out"][0] + 3), expect_error="overlaps")
    run(tweak=lambda a: a.update(work=a["out"][0] & ~3), expect_error="overlaps")
    run(tweak=lambda a: a.update(ch=a["out"][1] + 8), expect_error="overlaps")
    got, _ = run(mode="void", tweak=lambda a: a.update(work=None, nwork=0, ch=None))     # void needs no work buffer; changed is optional
    assert all(np.array_equal(g, scenes.host_sieve(m, 8, 4, "void")) for g, m in zip(got, maps))
    assert L.lib().raw("rua_scene_sieve_work_bytes")(0, 5, 4) == -1 and L.lib().raw("rua_scene_sieve_work_bytes")(1 << 16, 1 << 15, 4) == -1
    assert L.lib().raw("rua_scene_sieve_work_bytes")(5, 5, 65) == -1 and L.lib().raw("rua_scene_sieve_work_bytes")(6000, 6000, 6) == 12 * 36000000


# ---- 4. ScenePool ----------------------------------------------------------------------------------------------------------------
def test_pool_region_counts_and_sieved_maps_equal_the_cpu_pools():
    maps = [blob_scene(100)[1], blob_scene(101, 97, 260)[1], MAPS[-2][:64, :70].copy()]
    images = [np.zeros(m.shape + (1,), np.uint8) for m in maps]
    gpu, cpu = scenes.ScenePool(images, maps), scenes.ScenePool(images, maps, device="cpu")
    for conn in (4, 8):
        got = gpu.region_counts(min_area=8, num_classes=NCLS, connectivity=conn)
        assert got.dtype == np.int64 and got.shape == (3, NCLS, 3) and np.array_equal(got, cpu.region_counts(min_area=8, num_classes=NCLS, connectivity=conn))
    other = [maps[0][::-1].copy(), None, maps[2][::-1].copy()]
    bare = scenes.ScenePool(images, None)
    assert np.array_equal(bare.region_counts(other, min_area=3, num_classes=NCLS), cpu.region_counts(other, min_area=3, num_classes=NCLS))
    assert not bare.region_counts([None] * 3, min_area=3, num_classes=NCLS).any()
    for mode, classes, rounds, conn in (("fill", None, 1, 4), ("void", (1,), 1, 8), ("fill", (0, 2), 3, 8)):
        got, want = bare.sieved_maps(other, 8, NCLS, mode, conn, classes, rounds), cpu.sieved_maps(other, 8, NCLS, mode, conn, classes, rounds)
        assert got[1] is None and want[1] is None
        assert all(g.dtype == np.uint8 and np.array_equal(g, w) for g, w in zip(got[::2], want[::2])), (mode, classes, rounds)
    with pytest.raises(ValueError, match="rua_scene_sieve: min_area 0"):
        gpu.sieved_maps(maps, 0, NCLS, "fill")
    with pytest.raises(ValueError, match="needs maps, or the pool's class maps"):
        bare.region_counts(min_area=8, num_classes=NCLS)


# ---- 5. predict_scene(sieve=), as tests/test_scene_boundary_gpu.py builds its model and scenes -------------------------------------
@pytest.fixture(scope="module")
def model_and_pool():
    sc = [blob_scene(200, 97, 113), blob_scene(201, 64, 80)]
    return new_model(), scenes.ScenePool([s[0] for s in sc], [s[1] for s in sc], patch=64)


def check_report(pool, s, raw, res, sieve, erode=0, boundary=None):
    """res = predict_scene(sieve=) against raw = the same call without: the map is host_sieve of the raw map and every score is the
    host definition on the sieved map."""
    mn, C_, md, conn, mask, rounds = scenes.sieve_params(sieve, NCLS)
    classes = [c for c in range(C_) if (mask >> c) & 1]
    pred, cm, *more = res
    want = scenes.host_sieve(raw[0], mn, C_, scenes.SIEVE_MODES[md], conn, classes, rounds)
    assert pred.dtype == np.uint8 and np.array_equal(pred, want)
    cls = pool.class_maps[s]
    assert np.array_equal(cm, scenes.host_erode_confusion(cls, pred, 0, NCLS))
    if erode:
        assert np.array_equal(more.pop(0), scenes.host_erode_confusion(cls, pred, erode, NCLS))
    if boundary is not None:
        assert np.array_equal(more.pop(0), scenes.host_boundary_counts(cls, pred, boundary, NCLS))
    report = more.pop(0)
    assert sorted(report) == ["changed", "confusion_raw", "counts"]
    assert np.array_equal(report["confusion_raw"], raw[1])
    assert report["counts"].dtype == np.int64 and np.array_equal(report["counts"], scenes.host_region_counts(raw[0], mn, NCLS, conn))
    if rounds == 1:
        assert report["changed"] == int((pred != raw[0]).sum())
    return more


def test_predict_scene_sieve_none_is_the_call_without_it(model_and_pool):
    m, pool = model_and_pool
    for kw in (dict(), dict(erode=3, boundary=2, heads=("bound",)), dict(views="flips")):
        a, b = m.predict_scene(pool, 0, stride=32, batch=4, **kw), m.predict_scene(pool, 0, stride=32, batch=4, sieve=None, **kw)
        assert len(a) == len(b)
        for x, y in zip(a, b):
            if isinstance(x, dict):
                assert list(x) == list(y) and all(np.array_equal(x[k], y[k]) for k in x)
            else:
                assert np.array_equal(x, y)


@pytest.mark.parametrize("sieve", [8, {"min_area": 8, "mode": "void", "classes": (1, 2)}, {"min_area": 20, "connectivity": 8, "rounds": 2}])
def test_predict_scene_scores_the_sieved_map(model_and_pool, sieve):
    m, pool = model_and_pool
    for s in (0, 1):
        raw = m.predict_scene(pool, s, stride=32, batch=4)
        res = m.predict_scene(pool, s, stride=32, batch=4, sieve=sieve)
        assert len(res) == 3 and check_report(pool, s, raw, res, sieve) == []
    raw = m.predict_scene(pool, 0, stride=32, batch=4, erode=3, boundary=2)
    res = m.predict_scene(pool, 0, stride=32, batch=4, erode=3, boundary=2, sieve=sieve)
    assert len(res) == 5 and check_report(pool, 0, raw, res, sieve, erode=3, boundary=2) == []


def test_predict_scene_sieve_under_views_blend_and_heads(model_and_pool):
    m, pool = model_and_pool
    for kw in (dict(views="flips"), dict(blend="linear"), dict(scales=(1.0, 1.5))):
        raw = m.predict_scene(pool, 0, stride=32, batch=4, **kw)
        res = m.predict_scene(pool, 0, stride=32, batch=4, sieve=8, **kw)
        assert len(res) == 3 and check_report(pool, 0, raw, res, 8) == [], kw
    raw = m.predict_scene(pool, 0, stride=32, batch=4, heads=("bound",))
    res = m.predict_scene(pool, 0, stride=32, batch=4, heads=("bound",), sieve=8)
    rest = check_report(pool, 0, raw, res, 8)
    assert len(res) == 4 and len(rest) == 1 and list(rest[0]) == ["bound"] and np.array_equal(rest[0]["bound"], raw[2]["bound"])


def test_predict_scene_sieve_without_class_maps_and_refusals(model_and_pool):
    m, pool = model_and_pool
    bare = scenes.ScenePool(pool.images, None, patch=64)
    raw = m.predict_scene(bare, 0, stride=32, batch=4)
    for mode in ("void", "fill"):
        pred, cm, report = m.predict_scene(bare, 0, stride=32, batch=4, sieve={"min_area": 8, "mode": mode})
        assert cm is None and report["confusion_raw"] is None
        assert np.array_equal(pred, scenes.host_sieve(raw[0], 8, NCLS, mode))
        assert np.array_equal(report["counts"], scenes.host_region_counts(raw[0], 8, NCLS)) and report["changed"] == int((pred != raw[0]).sum())
    for wrong, text in ((0, "min_area 0"), ({"min_area": 3, "mode": "open"}, "mode 'open'"), ({"min_area": 3, "classes": (NCLS,)}, f"class {NCLS}, outside"), ("8", "sieve '8'")):
        with pytest.raises(ValueError, match=text):
            m.predict_scene(pool, 0, stride=32, batch=4, sieve=wrong)


def test_evaluate_scenes_sums_the_reports(model_and_pool):
    m, pool = model_and_pool
    sieve = {"min_area": 8, "mode": "void"}
    per = [m.predict_scene(pool, s, stride=32, batch=4, sieve=sieve) for s in range(len(pool))]
    maps, total, report = m.evaluate_scenes(pool, stride=32, batch_size=4, sieve=sieve)
    assert all(np.array_equal(a, p[0]) for a, p in zip(maps, per)) and np.array_equal(total, sum(p[1] for p in per))
    assert np.array_equal(report["counts"], sum(p[2]["counts"] for p in per)) and report["changed"] == sum(p[2]["changed"] for p in per)
    assert np.array_equal(report["confusion_raw"], m.evaluate_scenes(pool, stride=32, batch_size=4)[1])
    maps2, total2, total_e, counts, report2, heads = m.evaluate_scenes(pool, stride=32, batch_size=4, erode=3, boundary=3, heads="bound", sieve=sieve)
    assert np.array_equal(total2, total) and np.array_equal(report2["counts"], report["counts"]) and len(heads) == len(pool)
    assert np.array_equal(counts, sum(scenes.host_boundary_counts(c, p, 3, NCLS) for c, p in zip(pool.class_maps, maps)))
    assert np.array_equal(total_e, sum(scenes.host_erode_confusion(c, p, 3, NCLS) for c, p in zip(pool.class_maps, maps)))
    assert len(m.evaluate_scenes(pool, stride=32, batch_size=4)) == 2


def test_cli_sieve(tmp_path, capsys):
    import eval_scenes_ISPRS
    from resunet_a_mltsk_keras_amd.keras_api import load_model
    sc = [blob_scene(300, 90, 70), blob_scene(301, 64, 100)]
    root, path = str(tmp_path / "scenes"), str(tmp_path / "m.h5")
    scenes.save_scene_dir(root, ["a_tile", "b_tile"], [s[0] for s in sc], [s[1] for s in sc])
    new_model(seed=11, depth=4, split_k=True).save(path)
    base = ["--use_multitasking", "--model_path", path, "--dataset_path", root, "-ps", "64", "--num_classes", str(NCLS),
            "--scene_dataset", "yes", "--stride", "32", "--batch_size", "4"]
    plain = eval_scenes_ISPRS.main(base + ["--output_path", str(tmp_path / "plain")])
    capsys.readouterr()
    res = eval_scenes_ISPRS.main(base + ["--output_path", str(tmp_path / "sv"), "--sieve", "8", "--sieve_mode", "void", "--sieve_classes", "1", "2"])
    out = capsys.readouterr().out.splitlines()
    assert any(line.startswith("Before the sieve (--sieve 8, void") for line in out) and sum("pixels changed" in line for line in out) == 3
    assert set(res) - set(plain) == {"confusion_matrix_raw", "region_counts", "sieve_changed"}
    assert np.array_equal(res["confusion_matrix_raw"], plain["confusion_matrix"])
    names, images, class_maps = scenes.load_scene_dir(root)
    sieve = {"min_area": 8, "mode": "void", "classes": [1, 2]}
    maps, cm, report = load_model(path, compile=False).evaluate_scenes(scenes.ScenePool(images, class_maps, patch=64), stride=32, batch_size=4, norm_type=1, sieve=sieve)
    assert np.array_equal(res["confusion_matrix"], cm) and np.array_equal(res["region_counts"], report["counts"]) and res["sieve_changed"] == report["changed"]
    for n, c, want in zip(names, class_maps, maps):
        raw = np.load(tmp_path / "plain" / f"pred_seg_reconstructed_{n}.npy")
        pred = np.load(tmp_path / "sv" / f"pred_seg_reconstructed_{n}.npy")
        assert np.array_equal(pred, want) and np.array_equal(pred, scenes.host_sieve(raw, 8, NCLS, "void", classes=(1, 2)))
        counts = np.load(tmp_path / "sv" / f"region_counts_{n}.npy")
        assert counts.dtype == np.int64 and np.array_equal(counts, scenes.host_region_counts(raw, 8, NCLS))
        assert np.array_equal(np.load(tmp_path / "sv" / f"confusion_matrix_{n}.npy"), scenes.host_erode_confusion(c, pred, 0, NCLS))
        assert not os.path.exists(tmp_path / "plain" / f"region_counts_{n}.npy")
