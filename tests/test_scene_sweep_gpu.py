"""GPU tests of the precision-recall sweep: rua_scene_area_open and rua_scene_sweep_hist (csrc/sweep.hip) through the C ABI, bit for
bit against scenes.host_area_open / host_sweep_hist on the maps of test_scene_sweep_host.sweep_cases() - the smallest at which a
tiled, level-by-level union-find can go wrong; the refusals; ScenePool.opened_maps / sweep_hist; Engine.predict_scene(sweep=),
Model.evaluate_scenes and the command line on the 64 x 64 model and the blob scenes of tests/_scene_util.py.  Bytes and integers
only: every comparison is exact."""
import ctypes

import numpy as np
import pytest
import torch

from resunet_a_mltsk_keras_amd import _lib as L
from resunet_a_mltsk_keras_amd import scenes
from _scene_util import FILL, GUARD, NCLS, blob_scene, new_model
from test_scene_sweep_host import ALL, CASES, FIFTH, HAND, MIN_AREA, hand_made, host_open, smooth

pytestmark = pytest.mark.gpu

CHUNK = 96                                     # SW_CHUNK of csrc/sweep.hip: scenes per launch of the labelling kernels (table, histogram: 120)
NAMES = {c[0]: k for k, c in enumerate(CASES)}


def guarded(shapes, unit):
    return [torch.full((H * W * unit + GUARD,), FILL, dtype=torch.uint8, device="cuda") for H, W in shapes]


def read(bufs, shapes, unit=1):
    out = []
    for t, (H, W) in zip(bufs, shapes):
        g = t.cpu().numpy()
        assert (g[unit * H * W:] == FILL).all(), "bytes behind a map were written"
        out.append(g[:H * W].reshape(H, W) if unit == 1 else None)
    return out


def pattern(n):
    return (np.arange(n, dtype=np.int64) * 7 + 3) * (1 << 33) + 5             # non-zero in both halves of every cell


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def arr(ts):
    return (ctypes.c_void_p * len(ts))(*[t if t is None or isinstance(t, int) else t.data_ptr() for t in ts])


def interleave(m, stride, channel):
    """m as channel `channel` of an [H][W][stride] map whose other channels hold a pattern that must not influence anything."""
    full = ((np.arange(m.size * stride, dtype=np.int64) * 37 + 11) % 256).astype(np.uint8).reshape(m.shape + (stride,))
    full[..., channel] = m
    return full


def run_open(maps, levels, min_area, connectivity, stride=1, channel=0, expect_error=None, tweak=None, work=True):
    """rua_scene_area_open on these maps in ONE call: the opened maps and the two work arrays into FILL-ed buffers with a guard
    region behind each.  Returns the opened maps.  tweak(a) may change the argument dict; expect_error: the call must fail with
    RUA_ERR_ARG and this text and leave every buffer as it was."""
    n, shapes = len(maps), [m.shape for m in maps]
    host = [np.ascontiguousarray(interleave(m, stride, channel)) for m in maps]
    dev = [torch.from_numpy(h).cuda() for h in host]
    out, lab, are = guarded(shapes, 1), guarded(shapes, 4), guarded(shapes, 4)
    lv = np.array(levels, np.uint8)
    a = dict(prob=arr([t.data_ptr() + channel for t in dev]), h=(ctypes.c_int32 * n)(*[s[0] for s in shapes]), w=(ctypes.c_int32 * n)(*[s[1] for s in shapes]),
             n=n, stride=stride, lv=lv.ctypes.data, T=len(lv), mn=min_area, conn=connectivity, out=arr(out), lab=arr(lab) if work else None,
             are=arr(are) if work else None)
    if tweak is not None:
        tweak(a)
    args = (a["prob"], a["h"], a["w"], a["n"], a["stride"], a["lv"], a["T"], a["mn"], a["conn"], a["out"], a["lab"], a["are"], stream())
    if expect_error is not None:
        assert L.lib().raw("rua_scene_area_open")(*args) == -1
        err = L.lib().dll.rua_last_error().decode()
        assert err.startswith("rua_scene_area_open: ") and expect_error in err, err
        torch.cuda.synchronize()
        assert all((t.cpu().numpy() == FILL).all() for t in out + lab + are), "a refused call wrote something"
        return None
    L.lib().call("rua_scene_area_open", *args)
    torch.cuda.synchronize()
    assert all(np.array_equal(t.cpu().numpy(), h) for t, h in zip(dev, host)), "the maps were written"
    read(lab, shapes, 4), read(are, shapes, 4)
    if min_area == 1 or not work:
        assert all((t.cpu().numpy() == FILL).all() for t in lab + are), "min_area 1 touched the work arrays"
    return read(out, shapes)


def run_hist(probs, opened, cls, positive, C, stride=1, channel=0, expect_error=None, tweak=None):
    """rua_scene_sweep_hist on these scenes in ONE call, onto a non-zero pattern with guard cells behind it: what was added."""
    n, shapes = len(probs), [m.shape for m in probs]
    dev = [torch.from_numpy(np.ascontiguousarray(interleave(m, stride, channel))).cuda() for m in probs]
    od = None if opened is None else [torch.from_numpy(np.array(o)).cuda() for o in opened]         # a copy: the shared host maps are read-only
    cd = [torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in cls]
    h0 = np.concatenate([pattern(1024), np.full(16, -7, np.int64)])
    hist = torch.from_numpy(h0).cuda()
    a = dict(prob=arr([t.data_ptr() + channel for t in dev]), open=None if od is None else arr(od), cls=arr(cd),
             h=(ctypes.c_int32 * n)(*[s[0] for s in shapes]), w=(ctypes.c_int32 * n)(*[s[1] for s in shapes]), n=n, stride=stride, pos=positive, C=C,
             hist=hist.data_ptr())
    if tweak is not None:
        tweak(a)
    args = (a["prob"], a["open"], a["cls"], a["h"], a["w"], a["n"], a["stride"], a["pos"], a["C"], a["hist"], stream())
    if expect_error is not None:
        assert L.lib().raw("rua_scene_sweep_hist")(*args) == -1
        err = L.lib().dll.rua_last_error().decode()
        assert err.startswith("rua_scene_sweep_hist: ") and expect_error in err, err
        torch.cuda.synchronize()
        assert np.array_equal(hist.cpu().numpy(), h0), "a refused call wrote something"
        return None
    L.lib().call("rua_scene_sweep_hist", *args)
    torch.cuda.synchronize()
    got = hist.cpu().numpy()
    assert (got[-16:] == -7).all(), "cells behind the histogram were written"
    return (got[:-16] - h0[:-16]).reshape(2, 2, 256)


def class_map(rng, shape, C):
    """classes 0..C-1 in blocks, with speckle of "no class" bytes C, 200 and 255"""
    H, W = shape
    f = rng.integers(0, C, (H // 7 + 1, W // 7 + 1)).astype(np.uint8)
    c = np.ascontiguousarray(np.kron(f, np.ones((7, 7), np.uint8))[:H, :W])
    void = rng.random(shape) < 0.1
    c[void] = rng.choice(np.array([C, 200, 255], np.uint8), int(void.sum()))
    return c


# ---- 1. the opened map -------------------------------------------------------------------------------------------------------------
def groups():
    """the cases grouped by what one call can share: (levels, min_area) -> case indices"""
    out = {}
    for k, (_, _, levels, min_areas) in enumerate(CASES):
        for mn in min_areas:
            out.setdefault((levels, mn), []).append(k)
    return out


@pytest.mark.parametrize("connectivity", [4, 8])
def test_area_open_equals_the_host_definition(connectivity):
    """Every case at each of its min_area values; the cases that share levels and min_area go through ONE call: scenes of different
    sizes side by side."""
    calls = 0
    for (levels, mn), ks in groups().items():
        got = run_open([CASES[k][1] for k in ks], levels, mn, connectivity)
        calls += 1
        for g, k in zip(got, ks):
            assert np.array_equal(g, host_open(k, mn, connectivity)), (CASES[k][0], mn)
    assert calls < len(CASES) and any(len(ks) > 4 for ks in groups().values())


def test_hand_made_cases_settle_as_their_comments_say():
    made = hand_made()
    names = sorted(made)
    for conn in (4, 8):
        got = run_open([made[n][0] for n in names], HAND, MIN_AREA, conn)
        for g, n in zip(got, names):
            (i, j), byte = made[n][1][conn]
            assert g[i, j] == byte, (n, conn)


@pytest.mark.parametrize("stride,channel", [(6, 0), (6, 5), (64, 17)])
def test_area_open_reads_one_channel_of_an_interleaved_map(stride, channel):
    ks = [NAMES[n] for n in ("smooth", "noise", "cone_33x65", "column", "row")]                 # cases whose levels are FIFTH
    for mn in (1, 5):
        got = run_open([CASES[k][1] for k in ks], FIFTH, mn, 4, stride=stride, channel=channel)
        assert all(np.array_equal(g, host_open(k, mn, 4)) for g, k in zip(got, ks)), mn


def test_min_area_one_needs_no_work_arrays_and_is_the_table():
    ks = [NAMES[n] for n in ("noise", "sevens", "full", "zeros")]
    for levels in (ALL, (128,), (200, 10, 5)):
        got = run_open([CASES[k][1] for k in ks], levels, 1, 8, work=False)
        table = np.zeros(256, np.uint8)
        for t in sorted(levels):
            table[t:] = t
        assert all(np.array_equal(g, table[CASES[k][1]]) for g, k in zip(got, ks))


def test_more_scenes_than_one_launch_holds():
    rng = np.random.default_rng(29)
    maps = [smooth(rng, int(rng.integers(1, 40)), int(rng.integers(1, 40)), 1) for _ in range(CHUNK + 30)]
    maps[3], maps[CHUNK + 2] = CASES[NAMES["smooth"]][1], CASES[NAMES["cone_65x33"]][1]     # larger scenes among small ones: blocks without a tile
    levels = tuple(range(250, 0, -25))
    for mn in (1, 3):
        got = run_open(maps, levels, mn, 4)
        assert all(np.array_equal(g, scenes.host_area_open(m, levels, mn, 4)) for g, m in zip(got, maps)), mn
    cls = [class_map(rng, m.shape, 2) for m in maps]
    added = run_hist(maps, got, cls, 1, 2)
    assert np.array_equal(added, sum(scenes.host_sweep_hist(m, g, c, 1, 2) for m, g, c in zip(maps, got, cls)))


# ---- 2. the histogram --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride,channel", [(1, 0), (6, 0), (6, 5)])
def test_sweep_hist_equals_the_host_definition(stride, channel):
    rng = np.random.default_rng(31)
    ks = [NAMES[n] for n in ("smooth", "noise", "full", "zeros", "one", "row", "column", "cone_31x31", "cone_65x65")]
    probs = [CASES[k][1] for k in ks]
    opened = [host_open(k, CASES[k][3][-1], 4) for k in ks]
    for C, positive in ((2, 1), (6, 0), (64, 63), (1, 0)):
        cls = [class_map(rng, p.shape, C) for p in probs]
        assert any((c >= C).any() for c in cls)
        added = run_hist(probs, opened, cls, positive, C, stride, channel)
        want = sum(scenes.host_sweep_hist(p, o, c, positive, C) for p, o, c in zip(probs, opened, cls))
        assert np.array_equal(added, want), (C, positive)
        assert added[0].sum() == added[1].sum() == sum(int((c < C).sum()) for c in cls)
        added = run_hist(probs, None, cls, positive, C, stride, channel)                 # scene_open null: the probabilities themselves
        assert np.array_equal(added[0], want[0]) and np.array_equal(added[1], want[0])


# ---- 3. refusals: RUA_ERR_ARG, the offender named, nothing written -----------------------------------------------------------------
def test_area_open_refusals():
    maps = [CASES[NAMES["cone_33x33"]][1], CASES[NAMES["noise"]][1]]
    run = lambda **kw: run_open(maps, kw.pop("levels", (200, 100, 50)), kw.pop("min_area", 5), kw.pop("connectivity", 4), **kw)
    run(tweak=lambda a: a.update(T=0), expect_error="T 0 outside 1..255")
    run(tweak=lambda a: a.update(T=256), expect_error="T 256 outside 1..255")
    run(levels=(200, 0), expect_error="levels[1] = 0 outside 1..255")
    run(levels=(100, 100), expect_error="levels[1] = 100 is not below levels[0] = 100")
    run(levels=(50, 100), expect_error="strictly descending")
    run(min_area=0, expect_error="min_area 0 outside 1..2147483647")
    run(min_area=1 << 31, expect_error="min_area 2147483648 outside")
    run(connectivity=6, expect_error="connectivity 6 is neither 4 nor 8")
    run(stride=1, tweak=lambda a: a.update(stride=0), expect_error="pix_stride 0 outside 1..64")
    run(stride=1, tweak=lambda a: a.update(stride=65), expect_error="pix_stride 65 outside 1..64")
    run(tweak=lambda a: a.update(n=0), expect_error="nscenes 0")
    for key in ("prob", "lv", "out"):
        run(tweak=lambda a, key=key: a.update({key: None}), expect_error="are required")
    run(work=False, expect_error="min_area 5 needs the labels and areas work arrays")
    run(tweak=lambda a: a.update(are=None), expect_error="needs the labels and areas work arrays")
    for key in ("prob", "out", "lab", "are"):
        run(tweak=lambda a, key=key: a[key].__setitem__(1, None), expect_error="scene 1: null pointer")
    run(tweak=lambda a: a["h"].__setitem__(1, 0), expect_error="scene 1: size 0 x")
    run(tweak=lambda a: a["w"].__setitem__(0, -3), expect_error="x -3")

    def oversized(a):                                            # 2^31 pixels: one too many for an int32 label
        a["h"][1], a["w"][1] = 1 << 16, 1 << 15
    run(tweak=oversized, expect_error="scene 1: size 65536 x 32768")
    run(tweak=lambda a: a["lab"].__setitem__(1, a["lab"][1] + 2), expect_error="scene 1: labels and areas must be 4-byte aligned")
    run(tweak=lambda a: a["out"].__setitem__(1, a["prob"][1]), expect_error="scene 1: scene_open overlaps scene 1: scene_prob")
    run(tweak=lambda a: a["out"].__setitem__(0, a["prob"][1] + 5), expect_error="overlaps")
    run(tweak=lambda a: a["out"].__setitem__(1, a["out"][0] + 3), expect_error="overlaps")
    run(tweak=lambda a: a["are"].__setitem__(0, a["lab"][0] + 8), expect_error="scene 0: areas overlaps scene 0: labels")
    run(tweak=lambda a: a["lab"].__setitem__(1, a["prob"][0] & ~3), expect_error="overlaps")
    run(tweak=lambda a: a["are"].__setitem__(1, a["out"][0] & ~3), expect_error="overlaps")
    # the footprint of a channel reaches over the whole interleaved map: an output inside another channel's bytes is refused
    run(stride=6, channel=5, tweak=lambda a: a["out"].__setitem__(0, a["prob"][1] + 1), expect_error="overlaps")
    got = run_open(maps, (200, 100, 50), 1, 4, tweak=lambda a: a.update(lab=None, are=None))      # min_area 1 reads neither
    assert all(np.array_equal(g, scenes.host_area_open(m, (200, 100, 50), 1)) for g, m in zip(got, maps))


def test_sweep_hist_refusals():
    rng = np.random.default_rng(37)
    probs = [CASES[NAMES["cone_33x33"]][1], CASES[NAMES["noise"]][1]]
    cls = [class_map(rng, p.shape, 3) for p in probs]
    run = lambda **kw: run_hist(probs, kw.pop("opened", [p.copy() for p in probs]), cls, kw.pop("positive", 1), kw.pop("C", 3), **kw)
    run(C=0, expect_error="C 0 outside 1..64")
    run(C=65, expect_error="C 65 outside 1..64")
    run(positive=3, expect_error="positive 3 outside 0..2")
    run(positive=-1, expect_error="positive -1 outside 0..2")
    run(tweak=lambda a: a.update(stride=0), expect_error="pix_stride 0 outside 1..64")
    run(tweak=lambda a: a.update(stride=65), expect_error="pix_stride 65 outside 1..64")
    run(tweak=lambda a: a.update(n=0), expect_error="nscenes 0")
    for key in ("prob", "cls", "hist"):
        run(tweak=lambda a, key=key: a.update({key: None}), expect_error="are required")
    for key in ("prob", "open", "cls"):
        run(tweak=lambda a, key=key: a[key].__setitem__(1, None), expect_error="scene 1: null pointer")
    run(tweak=lambda a: a["h"].__setitem__(0, 0), expect_error="scene 0: size 0 x")

    def oversized(a):
        a["h"][1], a["w"][1] = 1 << 16, 1 << 15
    run(tweak=oversized, expect_error="scene 1: size 65536 x 32768")
    run(tweak=lambda a: a.update(hist=a["hist"] + 4), expect_error="hist must be 8-byte aligned")
    run(tweak=lambda a: a.update(hist=a["prob"][1] & ~7), expect_error="hist overlaps scene 1: scene_prob")
    run(tweak=lambda a: a.update(hist=(a["open"][0] + 8) & ~7), expect_error="overlaps")
    run(tweak=lambda a: a.update(hist=(a["cls"][1] + 8) & ~7), expect_error="overlaps")
    added = run(tweak=lambda a: a.update(cls=a["prob"]))                                  # inputs may share: a map scored against itself
    assert added[0].sum() == sum(int((p < 3).sum()) for p in probs)


# ---- 4. ScenePool ----------------------------------------------------------------------------------------------------------------
def test_pool_opened_maps_and_sweep_hist_equal_the_cpu_pools():
    rng = np.random.default_rng(41)
    shapes = [(70, 90), (33, 65), (64, 64)]
    images = [np.zeros(s + (1,), np.uint8) for s in shapes]
    cls = [class_map(rng, s, NCLS) for s in shapes]
    probs = [smooth(rng, *shapes[0]), None, rng.integers(0, 256, shapes[2]).astype(np.uint8)]
    gpu, cpu = scenes.ScenePool(images, cls), scenes.ScenePool(images, cls, device="cpu")
    for thresholds, mn, conn in ((None, 1, 4), (FIFTH, 5, 4), ([0.9, 0.5, 0.1], 69, 8)):
        got, want = gpu.opened_maps(probs, thresholds, mn, conn), cpu.opened_maps(probs, thresholds, mn, conn)
        assert got[1] is None and want[1] is None
        assert all(g.dtype == np.uint8 and np.array_equal(g, w) for g, w in zip(got[::2], want[::2])), (mn, conn)
        h = gpu.sweep_hist(probs, 1, NCLS, thresholds, mn, conn)
        assert h.dtype == np.int64 and h.shape == (3, 2, 2, 256) and np.array_equal(h, cpu.sweep_hist(probs, 1, NCLS, thresholds, mn, conn))
        assert not h[1].any() and h[0, 0].sum() == int((cls[0] < NCLS).sum())
    assert gpu.opened_maps([None] * 3) == [None] * 3 and not gpu.sweep_hist([None] * 3, 0, NCLS).any()
    with pytest.raises(ValueError, match="needs the pool's class maps"):
        scenes.ScenePool(images).sweep_hist(probs, 1, NCLS)
    with pytest.raises(ValueError, match="rua_scene_area_open: min_area 0"):
        gpu.opened_maps(probs, None, 0)
    with pytest.raises(ValueError, match=r"rua_scene_area_open: levels\[0\] = 0 outside 1..255"):
        gpu.sweep_hist(probs, 1, NCLS, [0])


# ---- 5. predict_scene(sweep=), as tests/test_scene_regions_gpu.py builds its model and scenes --------------------------------------
@pytest.fixture(scope="module")
def model_and_pool():
    sc = [blob_scene(200, 97, 113), blob_scene(201, 64, 80)]
    cls = [s[1].copy() for s in sc]
    cls[0][::9, ::7] = 255                                                               # "no class" pixels: counted nowhere
    return new_model(), scenes.ScenePool([s[0] for s in sc], cls, patch=64)


@pytest.fixture(scope="module")
def seg_maps(model_and_pool):
    """The stitched seg maps of both scenes, fetched once: what the sweep reads."""
    m, pool = model_and_pool
    return [m.predict_scene(pool, s, stride=32, batch=4, heads=("seg",)) for s in range(len(pool))]


def check_sweep(pool, s, seg, report, sweep):
    """report against the host definitions on channel `positive` of the stitched seg map"""
    positive, levels, mn, conn, want = scenes.sweep_params(sweep, NCLS)
    prob = np.ascontiguousarray(seg[..., positive])
    opened = scenes.host_area_open(prob, levels, mn, conn)
    assert sorted(report) == ["hist", "levels", "opened"]
    assert report["levels"].dtype == np.uint8 and np.array_equal(report["levels"], levels)
    assert report["hist"].dtype == np.int64 and report["hist"].shape == (2, 2, 256)
    assert np.array_equal(report["hist"], scenes.host_sweep_hist(prob, opened if mn > 1 else None, pool.class_maps[s], positive, NCLS))
    if want:
        assert report["opened"].dtype == np.uint8 and np.array_equal(report["opened"], opened)
    else:
        assert report["opened"] is None


def same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if isinstance(x, dict):
            assert list(x) == list(y) and all(np.array_equal(x[k], y[k]) for k in x)
        else:
            assert np.array_equal(x, y)


def test_predict_scene_sweep_none_is_the_call_without_it(model_and_pool):
    m, pool = model_and_pool
    for kw in (dict(), dict(erode=3, boundary=2, heads=("bound",), sieve=8), dict(views="flips")):
        same(m.predict_scene(pool, 0, stride=32, batch=4, **kw), m.predict_scene(pool, 0, stride=32, batch=4, sweep=None, **kw))


@pytest.mark.parametrize("sweep", [1, {"positive": 2, "min_area": 5, "opened": True},
                                   {"positive": 0, "thresholds": [0.9, 0.75, 0.5, 0.25, 0.1], "min_area": 69, "connectivity": 8},
                                   {"positive": 3, "thresholds": [200, 100], "opened": True}])
def test_predict_scene_sweep_equals_the_host_definitions(model_and_pool, seg_maps, sweep):
    m, pool = model_and_pool
    for s in (0, 1):
        res = m.predict_scene(pool, s, stride=32, batch=4, sweep=sweep)
        assert len(res) == 3
        same(res[:2], seg_maps[s][:2])                                                   # the seg map is stitched inside and not returned
        check_sweep(pool, s, seg_maps[s][2]["seg"], res[2], sweep)


def test_predict_scene_sweep_composes_with_the_other_scores(model_and_pool, seg_maps):
    m, pool = model_and_pool
    sweep = {"positive": 1, "min_area": 5, "thresholds": list(range(255, 0, -5))}
    kw = dict(erode=3, boundary=2, sieve={"min_area": 8, "mode": "void"})
    plain = m.predict_scene(pool, 0, stride=32, batch=4, heads=("bound", "seg"), **kw)
    res = m.predict_scene(pool, 0, stride=32, batch=4, heads=("bound", "seg"), sweep=sweep, **kw)
    assert len(res) == len(plain) + 1 == 7
    same(res[:5] + res[6:], plain)                                                       # after the sieve report, in front of the head maps
    check_sweep(pool, 0, res[6]["seg"], res[5], sweep)                                   # the probabilities, not the sieved class map
    assert np.array_equal(res[6]["seg"], seg_maps[0][2]["seg"])
    only_bound = m.predict_scene(pool, 0, stride=32, batch=4, heads=("bound",), sweep=sweep)
    assert list(only_bound[3]) == ["bound"] and np.array_equal(only_bound[2]["hist"], res[5]["hist"])
    seen = []
    m.predict_scene(pool, 1, stride=32, batch=4, heads=("bound",), sweep=1, on_heads=lambda r, o, t: seen.append(sorted(t)))
    assert seen and all(k == ["bound"] for k in seen)                                    # on_heads sees what was asked for
    flips = m.predict_scene(pool, 0, stride=32, batch=4, views="flips", heads=("seg",))
    res = m.predict_scene(pool, 0, stride=32, batch=4, views="flips", sweep=sweep)
    same(res[:2], flips[:2])
    check_sweep(pool, 0, flips[2]["seg"], res[2], sweep)


def test_predict_scene_sweep_refusals(model_and_pool):
    m, pool = model_and_pool
    bare = scenes.ScenePool(pool.images, None, patch=64)
    with pytest.raises(ValueError, match="needs the pool's class maps"):
        m.predict_scene(bare, 0, stride=32, batch=4, sweep=1)
    with pytest.raises(ValueError, match=r"predict_scene\(scales=, sweep=\): multi-scale maps of the heads are not built; give one of the two"):
        m.predict_scene(pool, 0, stride=32, batch=4, sweep=1, scales=(1.0, 1.5))
    with pytest.raises(ValueError, match=r"predict_scene\(blend=, sweep=\): blended maps of the heads are not built; give one of the two"):
        m.predict_scene(pool, 0, stride=32, batch=4, sweep=1, blend="linear")
    for wrong, text in ((NCLS, f"positive {NCLS} outside"), ({"min_area": 3}, "needs positive"), ({"positive": 1, "min_area": 0}, "min_area 0"),
                        ({"positive": 1, "thresholds": []}, "T 0 outside"), ({"positive": 1, "connectivity": 5}, "connectivity 5"), ("1", "sweep '1'")):
        with pytest.raises(ValueError, match=text):
            m.predict_scene(pool, 0, stride=32, batch=4, sweep=wrong)
    same(m.predict_scene(pool, 0, stride=32, batch=4, sweep=1, scales=(1.0,))[:2], m.predict_scene(pool, 0, stride=32, batch=4))


def test_evaluate_scenes_sums_the_histograms(model_and_pool):
    m, pool = model_and_pool
    sweep = {"positive": 1, "min_area": 5, "opened": True}
    per = [m.predict_scene(pool, s, stride=32, batch=4, sweep=sweep) for s in range(len(pool))]
    maps, total, report = m.evaluate_scenes(pool, stride=32, batch_size=4, sweep=sweep)
    assert all(np.array_equal(a, p[0]) for a, p in zip(maps, per)) and np.array_equal(total, sum(p[1] for p in per))
    assert np.array_equal(report["hist"], sum(p[2]["hist"] for p in per)) and np.array_equal(report["levels"], per[0][2]["levels"])
    assert len(report["opened"]) == len(pool) and all(np.array_equal(a, p[2]["opened"]) for a, p in zip(report["opened"], per))
    res = m.evaluate_scenes(pool, stride=32, batch_size=4, erode=3, boundary=3, heads="bound", sieve={"min_area": 8, "mode": "void"}, sweep=1)
    assert len(res) == 7 and sorted(res[4]) == ["changed", "confusion_raw", "counts"] and res[5]["opened"] is None and len(res[6]) == len(pool)
    assert np.array_equal(res[5]["hist"], m.evaluate_scenes(pool, stride=32, batch_size=4, sweep=1)[2]["hist"])
    assert len(m.evaluate_scenes(pool, stride=32, batch_size=4)) == 2


def test_cli_pr_curve(tmp_path, capsys):
    import eval_scenes_ISPRS
    from resunet_a_mltsk_keras_amd.keras_api import load_model
    sc = [blob_scene(300, 90, 70), blob_scene(301, 64, 100)]
    root, path = str(tmp_path / "scenes"), str(tmp_path / "m.h5")
    scenes.save_scene_dir(root, ["a_tile", "b_tile"], [s[0] for s in sc], [s[1] for s in sc])
    new_model(seed=11, depth=4, split_k=True).save(path)
    base = ["--use_multitasking", "--model_path", path, "--dataset_path", root, "-ps", "64", "--num_classes", str(NCLS),
            "--scene_dataset", "yes", "--stride", "32", "--batch_size", "4"]
    plain = eval_scenes_ISPRS.main(base + ["--output_path", str(tmp_path / "plain"), "--head_maps", "seg"])
    capsys.readouterr()
    res = eval_scenes_ISPRS.main(base + ["--output_path", str(tmp_path / "pr"), "--pr_curve", "1", "--pr_min_area", "5", "--pr_connectivity", "8",
                                         "--pr_thresholds"] + [str(t) for t in range(250, 0, -10)] + ["--pr_opened", "yes"])
    out = capsys.readouterr().out.splitlines()
    assert sum("average precision" in line for line in out) == 3 and sum(line.startswith("  threshold") for line in out) == 3
    assert any(line.startswith("Precision-recall sweep of class 1 (min_area 5, connectivity 8, 25 levels)") for line in out)
    assert set(res) - set(plain) == {"pr_hist", "pr_levels", "pr_scores", "average_precision"}
    assert np.array_equal(res["confusion_matrix"], plain["confusion_matrix"])
    levels = scenes.sweep_levels(list(range(250, 0, -10)))
    names, images, class_maps = scenes.load_scene_dir(root)
    total = np.zeros((2, 2, 256), np.int64)
    for k, (n, c) in enumerate(zip(names, class_maps)):
        prob = np.ascontiguousarray(plain["head_maps"][k]["seg"][..., 1])
        opened = np.load(tmp_path / "pr" / f"pr_opened_{n}.npy")
        assert opened.dtype == np.uint8 and np.array_equal(opened, scenes.host_area_open(prob, levels, 5, 8))
        hist = np.load(tmp_path / "pr" / f"pr_hist_{n}.npy")
        assert hist.dtype == np.int64 and np.array_equal(hist, scenes.host_sweep_hist(prob, opened, c, 1, NCLS))
        total += hist
    want = scenes.sweep_scores(total, levels)
    assert np.array_equal(res["pr_hist"], total) and np.array_equal(res["pr_levels"], levels) and res["average_precision"] == want["average_precision"]
    curve = np.load(tmp_path / "pr" / "pr_curve.npy")
    assert curve.shape == (9, 25) and np.array_equal(curve[0], levels) and np.array_equal(curve[1], want["tp"]) and np.array_equal(curve[5], want["recall"])
    with pytest.raises(SystemExit, match="--pr_curve excludes --scales and --blend"):
        eval_scenes_ISPRS.main(base + ["--output_path", str(tmp_path / "no"), "--pr_curve", "1", "--blend", "linear"])
    with pytest.raises(SystemExit, match="--pr_curve: rua_scene_sweep_hist: positive 4 outside 0..3"):
        eval_scenes_ISPRS.main(base + ["--output_path", str(tmp_path / "no"), "--pr_curve", "4"])
    maps, cm, report = load_model(path, compile=False).evaluate_scenes(scenes.ScenePool(images, class_maps, patch=64), stride=32, batch_size=4, norm_type=1,
                                                                       sweep={"positive": 1, "min_area": 5, "connectivity": 8, "thresholds": levels.tolist()})
    assert np.array_equal(report["hist"], total) and np.array_equal(cm, res["confusion_matrix"])
