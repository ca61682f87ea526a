"""GPU tests of multi-scale test-time augmentation for whole-scene evaluation: rua_scene_accumulate and rua_scene_argmax (csrc/scene.hip)
through the C ABI, every int32 sum, byte and count against scenes.host_accumulate / host_argmax, and their argument checks;
Engine.predict_scene(scales=) against the host definitions of the probabilities it accumulated, with erode and boundary, through
Model.evaluate_scenes and through eval_scenes_ISPRS.py --scales."""
import ctypes
import os

import numpy as np
import pytest
import torch

from resunet_a_mltsk_keras_amd import _lib as L
from resunet_a_mltsk_keras_amd import scenes

from _scene_util import FILL, GUARD, NCLS, blob_pool, blob_scene, conf_pattern, guarded_maps, new_engine, new_model, read_guarded

pytestmark = pytest.mark.gpu

f32 = np.float32
FLAT = (0, 2, 3, 4)
GUARD_WORDS, GUARD_VALUE = GUARD // 4, -0x11111112


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptrs(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def sizes(shapes):
    return (ctypes.c_int32 * len(shapes))(*[h for h, _ in shapes]), (ctypes.c_int32 * len(shapes))(*[w for _, w in shapes])


def pass_tables(shapes, patch, footprint, stride, views):
    """scale_table of every scene the footprint fits, concatenated, with the scene index in column 0: one call's groups."""
    parts = []
    for s, shp in enumerate(shapes):
        if footprint[0] <= shp[0] and footprint[1] <= shp[1]:
            rows7, own = scenes.scale_table(shp, patch, footprint, stride, views)
            rows7[:, 0] = s
            parts.append((rows7, own))
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def random_p(rng, n, patch, C):
    """float32 [n][PH][PW][C]: mostly rng.random, 3 % of the values outside 0..1, exact 0 and 1 and ties at the rounding point."""
    p = rng.random((n,) + tuple(patch) + (C,), dtype=f32)
    odd = rng.random(p.shape) < 0.03
    p[odd] = rng.choice(np.array([-0.25, 1.5, 0.0, 1.0, 2.0 ** -17, 3 * 2.0 ** -17, 0.5], f32), int(odd.sum()))
    return p


class Accumulators:
    """One pre-filled int32 [H][W][C] device accumulator per scene with a guard region behind it, and its host twin."""

    def __init__(self, rng, shapes, C):
        self.shapes, self.C = shapes, C
        self.host = [rng.integers(-50000, 50000, (H, W, C)).astype(np.int32) for H, W in shapes]
        self.dev = []
        for a in self.host:
            t = torch.full((a.size + GUARD_WORDS,), GUARD_VALUE, dtype=torch.int32, device="cuda")
            t[:a.size] = torch.from_numpy(a.ravel()).cuda()
            self.dev.append(t)

    def read(self):
        out = []
        for t, (H, W) in zip(self.dev, self.shapes):
            g = t.cpu().numpy()
            assert (g[H * W * self.C:] == GUARD_VALUE).all(), "words behind an accumulator were written"
            out.append(g[:H * W * self.C].reshape(H, W, self.C))
        return out

    def call(self, p, rows7, own, K, C=None, expect_error=None):
        pd = torch.from_numpy(np.ascontiguousarray(p)).cuda()
        r, o = np.ascontiguousarray(rows7, dtype=np.int32), np.ascontiguousarray(own, dtype=np.int32)
        hs, ws = sizes(self.shapes)
        args = (pd.data_ptr(), len(o), K, p.shape[1], p.shape[2], p.shape[3] if C is None else C, r.ctypes.data, o.ctypes.data, ptrs(self.dev),
                hs, ws, len(self.shapes), stream())
        if expect_error is None:
            L.lib().call("rua_scene_accumulate", *args)
        else:
            with pytest.raises(L.RuaError, match=expect_error):
                L.lib().call("rua_scene_accumulate", *args)
        torch.cuda.synchronize()

    def assert_equal_host(self, what):
        for s, (g, w) in enumerate(zip(self.read(), self.host)):
            bad = np.argwhere(g != w)
            assert bad.size == 0, (what, f"scene {s}", len(bad), "first at", tuple(bad[0]), int(g[tuple(bad[0])]), int(w[tuple(bad[0])]))


def accumulate_case(seed, shapes, patch, footprints, stride, views, C):
    """Every footprint one call (one pass: its groups own disjoint pixels) over all the scenes it fits, into the same pre-filled
    accumulators; the host definition adds the same passes; all sums equal at the end."""
    rng = np.random.default_rng(seed)
    codes = scenes.check_views(views, patch)
    K = len(codes)
    acc = Accumulators(rng, shapes, C)
    before = [a.copy() for a in acc.host]
    for F in footprints:
        rows7, own = pass_tables(shapes, patch, F, stride, codes)
        p = random_p(rng, len(rows7), patch, C)
        acc.call(p, rows7, own, K)
        scenes.host_accumulate(p, rows7, own, shapes, K, acc=acc.host)
    assert all((a != b).any() for a, b in zip(acc.host, before))
    acc.assert_equal_host((patch, views, C))


SHAPES = [(33, 40), (19, 23)]


# P = (8, 8) at stride 6; footprints 5 (zoomed in), 8 (the patch: pure placement), 13 and 32 (zoomed out; 32 fits the first scene only).
# C = 5: an accumulator row starts at any dword; C = 64: one tile row is 4096 elements.  Rectangles wider than a 64-column tile do
# not occur at these sizes; the (7, 9) and (2, 2) cases below and the end-to-end tests cover more than one tile per rectangle.
@pytest.mark.parametrize("C", [1, 3, 5, 64])
@pytest.mark.parametrize("views", [(0,), "aug5", "all", (5, 7)])
def test_accumulate_bitwise(views, C):
    accumulate_case(C * 10 + len(scenes.check_views(views)), SHAPES, (8, 8), [(5, 5), (8, 8), (13, 13), (32, 32)], 6, views, C)


@pytest.mark.parametrize("patch,footprints,stride", [((7, 9), [(5, 6), (7, 9), (11, 14), (25, 33)], (5, 7)),
                                                     ((4, 12), [(3, 9), (4, 12), (7, 20), (16, 40)], (3, 8))])
def test_accumulate_bitwise_odd_and_flat_patch(patch, footprints, stride):
    """Patches that are not square take the codes that do not transpose; (25, 33) and (16, 40) fit the first scene only, and a
    footprint of 25 rows at a row stride of 18 owns rectangles of more than 16 rows: two tiles."""
    accumulate_case(patch[0], SHAPES, patch, footprints, stride, FLAT, 5)


def test_accumulate_one_wide_rectangle():
    """One footprint of 100 x 150 scene pixels for a 32 x 48 window, owned in full: 7 x 3 tiles, ragged at both ends."""
    accumulate_case(3, [(100, 150)], (32, 48), [(100, 150)], (32, 48), (0, 2), 5)


def test_accumulate_more_groups_than_one_launch():
    """P = (2, 2) at stride 1 on the 19 x 23 scene: 396 groups of K = 2, a launch carries 24."""
    rows7, own = scenes.scale_table((19, 23), (2, 2), (2, 2), 1, (0, 2))
    assert len(own) == 18 * 22
    accumulate_case(4, [(19, 23)], (2, 2), [(2, 2), (3, 3)], 1, (0, 2), 3)


def test_accumulate_empty_rectangles_write_nothing():
    rng = np.random.default_rng(5)
    rows7, own = pass_tables(SHAPES, (8, 8), (13, 13), 6, (0, 3))
    p = random_p(rng, len(rows7), (8, 8), 5)
    acc = Accumulators(rng, SHAPES, 5)
    nothing = own.copy()
    nothing[::3] = 0                                           # the padding groups of a last batch
    nothing[1::3, 1] = nothing[1::3, 0]                        # no rows
    nothing[2::3, 3] = nothing[2::3, 2]                        # no columns
    acc.call(p, rows7, nothing, 2)
    acc.assert_equal_host("all empty")
    some = own.copy()
    some[::2] = nothing[::2]
    acc.call(p, rows7, some, 2)
    scenes.host_accumulate(p, rows7, some, SHAPES, 2, acc=acc.host)
    acc.assert_equal_host("half empty")


def test_accumulate_special_floats():
    rng = np.random.default_rng(6)
    rows7, own = pass_tables(SHAPES, (8, 8), (13, 13), 6, (0, 6))
    p = rng.random((len(rows7), 8, 8, 3), dtype=f32)
    odd = rng.random(p.shape) < 0.3
    p[odd] = rng.choice(np.array([np.nan, np.inf, -np.inf, -1.0, 7.0, -0.0, 1e-30, 1 - 2.0 ** -24, 2.0 ** -17], f32), int(odd.sum()))
    acc = Accumulators(rng, SHAPES, 3)
    acc.call(p, rows7, own, 2)
    scenes.host_accumulate(p, rows7, own, SHAPES, 2, acc=acc.host)
    acc.assert_equal_host("special floats")


def test_accumulate_refuses_bad_arguments():
    rng = np.random.default_rng(7)
    rows7, own = pass_tables(SHAPES, (8, 8), (13, 13), 6, (0, 6))
    p = random_p(rng, len(rows7), (8, 8), 3)
    acc = Accumulators(rng, SHAPES, 3)

    def with_cell(t, k, col, v):
        t = t.copy()
        t[k, col] = v
        return t
    refused = [
        (with_cell(rows7, 3, 0, 2), own, "rua_scene_accumulate: row 3: scene 2 outside 0..1"),
        (with_cell(rows7, 3, 0, -1), own, "rua_scene_accumulate: row 3: scene -1 outside 0..1"),
        (with_cell(rows7, 5, 0, 1), own, "rua_scene_accumulate: row 5: scene 1, but its group 2 is scene 0"),
        (with_cell(rows7, 2, 4, 7), own, r"row 2: matrix \(\d+, 7, 0, \d+\) is not axis-aligned"),
        (with_cell(rows7, 2, 3, 0), own, r"row 2: matrix \(0, 0, 0, \d+\) is not axis-aligned"),
        (with_cell(rows7, 1, 3, 9), own, r"row 1: matrix \(9, \d+, \d+, 0\) is not axis-aligned"),
        (rows7, with_cell(own, 4, 1, 34), r"group 4: rectangle rows \d+\.\.34, columns \d+\.\.\d+ outside its 33 x 40 scene"),
        (rows7, with_cell(own, 0, 2, -1), r"group 0: rectangle rows 0\.\.\d+, columns -1\.\.\d+ outside its 33 x 40 scene"),
        (rows7, with_cell(own, 0, 0, 12), "group 0: rectangle rows 12.."),
        (rows7, with_cell(own, 0, 1, 30), r"row 0: rectangle rows 0\.\.30, columns \d+\.\.\d+ of group 0 leaves the window's footprint"),
        (rows7, with_cell(own, 1, 2, 0), r"row 2: rectangle rows \d+\.\.\d+, columns 0\.\.\d+ of group 1 leaves the window's footprint"),
        (with_cell(rows7, 7, 1, int(rows7[7, 1]) + 40 * 65536), own, "row 7: rectangle .* of group 3 leaves the window's footprint"),
    ]
    assert own[0, 1] < 12 and own[1, 2] > 0
    for r, o, msg in refused:
        acc.call(p, r, o, 2, expect_error=msg)
        with pytest.raises(ValueError, match=msg):                # the host definition refuses the same tables in the same words
            scenes.host_accumulate(p, r, o, SHAPES, 2)
    acc.call(p, rows7, own, 0, expect_error="K 0 outside 1..8")
    acc.call(p, rows7, own, 9, expect_error="K 9 outside 1..8")
    acc.call(p, rows7, own, 2, C=65, expect_error="C 65 outside 1..64")
    acc.call(p, rows7, own, 2, C=0, expect_error="C 0 outside 1..64")
    frows, fown = pass_tables(SHAPES, (4, 12), (4, 12), 4, (0, 3))
    frows[3, 3:] = [0, 65536, 65536, 0]
    msg = r"row 3: matrix \(0, 65536, 65536, 0\) transposes and needs a square patch \(got 4 x 12\)"
    acc.call(np.zeros((len(frows), 4, 12, 3), f32), frows, fown, 2, expect_error=msg)
    with pytest.raises(ValueError, match=msg):
        scenes.host_accumulate(np.zeros((len(frows), 4, 12, 3), f32), frows, fown, SHAPES, 2)
    hs, ws = sizes(SHAPES)
    pd = torch.from_numpy(p).cuda()
    big = (ctypes.c_int32 * 2)(16385, 19)
    for args, msg in (((pd.data_ptr() + 4, len(own), 2, 8, 8, 3, rows7.ctypes.data, own.ctypes.data, ptrs(acc.dev), hs, ws, 2), "p must be 16-byte aligned"),
                      ((pd.data_ptr(), len(own), 2, 8, 513, 3, rows7.ctypes.data, own.ctypes.data, ptrs(acc.dev), hs, ws, 2), r"PH 8, PW 513 \(1 <= PH, PW <= 512\)"),
                      ((pd.data_ptr(), len(own), 2, 8, 8, 3, rows7.ctypes.data, own.ctypes.data, ptrs(acc.dev), big, ws, 2), r"scene 0: size 16385 x 40 \(1 <= H, W <= 16384\)"),
                      ((pd.data_ptr(), 0, 2, 8, 8, 3, rows7.ctypes.data, own.ctypes.data, ptrs(acc.dev), hs, ws, 2), r"nscenes 2, G 0 \(both >= 1\)"),
                      ((None, len(own), 2, 8, 8, 3, rows7.ctypes.data, own.ctypes.data, ptrs(acc.dev), hs, ws, 2), "are required")):
        with pytest.raises(L.RuaError, match=msg):
            L.lib().call("rua_scene_accumulate", *args, stream())
    torch.cuda.synchronize()
    acc.assert_equal_host("a refused call wrote something")


# ---- rua_scene_argmax -------------------------------------------------------------------------------------------------------------
def argmax_inputs(seed, shapes, C):
    """int32 accumulators with about 10 % planted ties (two or three classes at the maximum) and some all-equal pixels; class maps in
    0..C-1 with 3 % of 255s and, for C < 200, some labels equal to C."""
    rng = np.random.default_rng(seed)
    accs, maps = [], []
    for H, W in shapes:
        a = rng.integers(-1000, 500000, (H, W, C)).astype(np.int32)
        if C > 1:
            tie = np.argwhere(rng.random((H, W)) < 0.1)
            top = a[tie[:, 0], tie[:, 1]].max(-1) + 1
            for _ in range(3):
                a[tie[:, 0], tie[:, 1], rng.integers(0, C, len(tie))] = top
        a[rng.random((H, W)) < 0.02] = -7
        m = rng.integers(0, C, (H, W)).astype(np.uint8)
        m[rng.random((H, W)) < 0.03] = 255
        m[rng.random((H, W)) < 0.03] = C
        accs.append(a)
        maps.append(m)
    return accs, maps


def run_argmax(accs, class_maps, C=None, expect_error=None):
    shapes = [a.shape[:2] for a in accs]
    C = accs[0].shape[2] if C is None else C
    dev = [torch.from_numpy(a).cuda() for a in accs]
    pred = guarded_maps(shapes)
    cls = None if class_maps is None else [torch.from_numpy(m).cuda() for m in class_maps]
    conf0 = conf_pattern(C if 1 <= C <= 64 else 1)
    conf = None if class_maps is None else torch.from_numpy(conf0).cuda()
    hs, ws = sizes(shapes)
    args = (ptrs(dev), ptrs(pred), None if cls is None else ptrs(cls), hs, ws, len(shapes), C, None if conf is None else conf.data_ptr(), stream())
    if expect_error is None:
        L.lib().call("rua_scene_argmax", *args)
    else:
        with pytest.raises(L.RuaError, match=expect_error):
            L.lib().call("rua_scene_argmax", *args)
    torch.cuda.synchronize()
    maps = read_guarded(pred, shapes)
    cm = None if conf is None else conf.cpu().numpy() - conf0
    if expect_error is not None:
        assert all((m == FILL).all() for m in maps) and (cm is None or (cm == 0).all()), "a refused call wrote something"
    assert all(np.array_equal(d.cpu().numpy(), a) for d, a in zip(dev, accs)), "the accumulators are read only"
    return maps, cm


@pytest.mark.parametrize("C", [1, 3, 5, 64])
def test_argmax_bitwise(C):
    accs, cls = argmax_inputs(C, [(2, 2), (19, 23), (33, 40)], C)
    for class_maps in (cls, None):
        got_maps, got_cm = run_argmax(accs, class_maps)
        want_maps, want_cm = scenes.host_argmax(accs, class_maps, C)
        for s, (g, w) in enumerate(zip(got_maps, want_maps)):
            assert np.array_equal(g, w), (f"scene {s}", np.argwhere(g != w)[:3])
        assert (got_cm is None and want_cm is None) if class_maps is None else np.array_equal(got_cm, want_cm)
    if C > 1:                                                    # the inputs hold what they are meant to: uncounted labels and ties
        assert scenes.host_argmax(accs, cls, C)[1].sum() < sum(m.size for m in cls) and any((np.sort(a, -1)[..., -1] == np.sort(a, -1)[..., -2]).any() for a in accs)


@pytest.mark.parametrize("shape,C", [((520, 515), 3), ((300, 250), 64)])
def test_argmax_more_pixels_than_one_sweep(shape, C):
    """A launch has at most 1024 blocks per scene, of 256 pixels (64 at C = 64): these scenes hold a little more, so some blocks
    sweep twice and some once; the second scene of the call ends inside the first sweep."""
    assert shape[0] * shape[1] > 1024 * min(256, 4096 // C) and shape[0] * shape[1] < 2 * 1024 * min(256, 4096 // C)
    accs, cls = argmax_inputs(C + 1, [shape, (33, 40)], C)
    got_maps, got_cm = run_argmax(accs, cls)
    want_maps, want_cm = scenes.host_argmax(accs, cls, C)
    assert all(np.array_equal(g, w) for g, w in zip(got_maps, want_maps)) and np.array_equal(got_cm, want_cm)


def test_argmax_more_scenes_than_one_launch_and_refusals():
    accs, cls = argmax_inputs(9, [(3, 5)] * 101 + [(7, 2)], 3)    # a launch carries 100 scenes
    got_maps, got_cm = run_argmax(accs, cls)
    want_maps, want_cm = scenes.host_argmax(accs, cls, 3)
    assert all(np.array_equal(g, w) for g, w in zip(got_maps, want_maps)) and np.array_equal(got_cm, want_cm)
    run_argmax(accs[:2], cls[:2], C=65, expect_error="rua_scene_argmax: C 65 outside 1..64")
    run_argmax(accs[:2], cls[:2], C=0, expect_error="rua_scene_argmax: C 0 outside 1..64")
    dev, pred = [torch.from_numpy(accs[0]).cuda()], guarded_maps([(3, 5)])
    hs, ws = sizes([(3, 5)])
    conf = torch.zeros((3, 3), dtype=torch.int64, device="cuda")
    for args, msg in (((ptrs(dev), ptrs(pred), ptrs(pred), hs, ws, 1, 3, None), "scene_cls and confusion go together"),
                      ((ptrs(dev), ptrs(pred), None, hs, ws, 1, 3, conf.data_ptr()), "scene_cls and confusion go together"),
                      ((ptrs(dev), ptrs(pred), None, hs, ws, 0, 3, None), r"nscenes 0 \(>= 1\)"),
                      ((ptrs(dev), (ctypes.c_void_p * 1)(None), None, hs, ws, 1, 3, None), "scene 0: null pointer"),
                      ((ptrs(dev), ptrs(pred), None, (ctypes.c_int32 * 1)(0), ws, 1, 3, None), "scene 0: size 0 x 5 x 12"),
                      ((None, ptrs(pred), None, hs, ws, 1, 3, None), "are required")):
        with pytest.raises(L.RuaError, match=msg):
            L.lib().call("rua_scene_argmax", *args, stream())
    torch.cuda.synchronize()
    assert (read_guarded(pred, [(3, 5)])[0] == FILL).all() and (conf.cpu().numpy() == 0).all()


# ---- engine / model level -------------------------------------------------------------------------------------------------------
SCALES = (0.75, 1.0, 1.5)                                     # footprints 85, 64 and 43 of the 64 x 64 patch


@pytest.fixture(scope="module")
def pool():
    return blob_pool((128, 128))


def host_of(seen, pool, scene, K):
    """host_argmax(host_accumulate(...)) of the batches on_batch saw, in their order: (map, confusion matrix) of `scene`."""
    acc = None
    for r, o, p in seen:
        acc = scenes.host_accumulate(p, r, o, pool.shapes, K, acc=acc)
    maps, cm = scenes.host_argmax([acc[scene]], [pool.class_maps[scene]], NCLS)
    return maps[0], cm


@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("multitask", [True, False])
def test_predict_scene_scales_is_the_host_definition_of_its_probabilities(pool, multitask, use_graph):
    """The 128 x 128 scene at stride 64: covers of 4, 4 and 9 footprints.  views (0,) at batch 8 pads every pass' only or last batch,
    flips at batch 8 (G = 2) pads the pass of 9; erode and boundary score the finished map."""
    eng = new_engine(multitask, use_graph)
    scene = 1
    for views in ((0,), "flips"):
        codes = scenes.check_views(views)
        K = len(codes)
        G = max(1, 8 // K)
        seen = []
        pred, cm, cm_e, bc = eng.predict_scene(pool, scene, stride=64, batch=8, norm_type=1, views=views, scales=SCALES, erode=3, boundary=3,
                                               on_batch=lambda r, o, p: seen.append((r.copy(), o.copy(), p.cpu().numpy())))
        tables = [scenes.scale_table(pool.shapes[scene], 64, scenes.scale_footprint(64, z), 64, codes) for z in SCALES]
        assert [len(t[1]) for t in tables] == [4, 4, 9]
        assert len(seen) == sum(-(-len(t[1]) // G) for t in tables)
        assert all(r.shape == (G * K, 7) and o.shape == (G, 4) and p.shape == (G * K, 64, 64, NCLS) and (r[:, 0] == scene).all() for r, o, p in seen)
        k = 0
        for rows7, own in tables:                                 # each pass in order, its last batch padded with empty rectangles
            nb = -(-len(own) // G)
            r, o = np.concatenate([s[0] for s in seen[k:k + nb]]), np.concatenate([s[1] for s in seen[k:k + nb]])
            assert np.array_equal(r[:len(rows7), 1:], rows7[:, 1:]) and np.array_equal(o[:len(own)], own) and (o[len(own):] == 0).all()
            assert np.array_equal(r[len(rows7):], np.tile(r[len(rows7) - K:len(rows7)], (len(o) - len(own), 1)))
            k += nb
        assert all(np.isfinite(s[2]).all() for s in seen)
        want, want_cm = host_of(seen, pool, scene, K)
        what = (multitask, use_graph, views)
        assert pred.dtype == np.uint8 and pred.shape == pool.shapes[scene] and np.array_equal(pred, want), what
        assert cm.dtype == np.int64 and np.array_equal(cm, want_cm) and cm.sum() == pred.size, what
        assert np.array_equal(cm_e, scenes.host_erode_confusion(pool.class_maps[scene], pred, 3, NCLS)), what
        assert np.array_equal(bc, scenes.host_boundary_counts(pool.class_maps[scene], pred, 3, NCLS)), what
        assert len(np.unique(pred)) > 1
        plain = eng.predict_scene(pool, scene, stride=64, batch=8, norm_type=1, views=views, scales=SCALES)
        assert len(plain) == 2 and np.array_equal(plain[0], pred) and np.array_equal(plain[1], cm)


def test_scales_none_is_the_call_without_scales_and_refusals(pool, monkeypatch):
    eng = new_engine(False, True)
    lib = L.lib()
    log = []
    real = lib.call
    # the log keeps the scene entry points: what the forward between them launches depends on whether its graph is captured yet
    every = []

    def logged(name, *args):
        every.append(name)
        if name.startswith("rua_scene_"):
            log.append(name)
        return real(name, *args)
    monkeypatch.setattr(lib, "call", logged)
    results = []
    for kw in ({}, {"scales": None}, {"scales": (1.0,)}, {"scales": [1]}):
        for views in ((0,), "flips"):
            del log[:]
            results.append((eng.predict_scene(pool, 0, stride=48, batch=5, views=views, erode=2, heads=("seg",), **kw), list(log)))
    for (got, calls), (want, want_calls) in zip(results[2:], results[:2] * 3):
        assert len(got) == len(want) == 4 and all(np.array_equal(g, w) for g, w in zip(got[:3], want[:3])) and np.array_equal(got[3]["seg"], want[3]["seg"])
        assert calls == want_calls and "rua_scene_accumulate" not in calls and "rua_scene_argmax" not in calls
    assert "rua_scene_stitch" in results[0][1] and "rua_scene_stitch_views" in results[1][1]
    del log[:]
    eng.predict_scene(pool, 1, stride=64, batch=8, scales=(1.0, 2.0))
    assert log.count("rua_scene_accumulate") == 1 + 2 and log.count("rua_scene_argmax") == 1 and log.count("rua_scene_windows_affine") == 3
    assert not any(n in log for n in ("rua_scene_stitch", "rua_scene_stitch_views", "rua_scene_stitch_maps", "rua_scene_windows"))
    # refusals come before any launch
    flat = new_engine(False, False, shape=(32, 64, 3), depth=4)
    fpool = scenes.ScenePool(pool.images, pool.class_maps, patch=(32, 64))
    del every[:]
    with pytest.raises(ValueError, match="multi-scale maps of the heads are not built"):
        eng.predict_scene(pool, 1, scales=SCALES, heads=("seg",))
    with pytest.raises(ValueError, match="zoom 0.45 gives a footprint of 142 x 142, larger than the 128 x 128 scene"):
        eng.predict_scene(pool, 1, scales=(1.0, 0.45))
    for bad, msg in (((1.0, 1.0), "occurs twice"), ((), "1 to 8 distinct"), (2.0, "1 to 8 distinct"), ((0.1,), "F <= 4 P"), ((1.0, -1.0), "positive")):
        with pytest.raises(ValueError, match=msg):
            eng.predict_scene(pool, 1, scales=bad)
    with pytest.raises(ValueError, match=r"code 1 transposes and needs a square patch \(got 32 x 64\)"):
        flat.predict_scene(fpool, 1, views="aug5", scales=SCALES)
    assert every == []
    bare = scenes.ScenePool(pool.images, None, patch=64)       # no class maps: the map alone
    pred, cm = eng.predict_scene(bare, 1, stride=64, batch=8, scales=(1.0, 2.0))
    assert cm is None and np.array_equal(pred, eng.predict_scene(pool, 1, stride=64, batch=8, scales=(1.0, 2.0))[0])
    fpred, fcm = flat.predict_scene(fpool, 1, views=(0, 3), scales=(1.0, 1.6), batch=4)      # a flat patch: footprints 32 x 64 and 20 x 40
    assert fpred.shape == (128, 128) and fcm.sum() == 128 * 128


def test_evaluate_scenes_sums_the_scenes(pool):
    m = new_model()
    maps, cm, cm_e = m.evaluate_scenes(pool, stride=64, batch_size=8, norm_type=1, views="flips", erode=3, scales=SCALES)
    total, total_e = 0, 0
    for s in range(len(pool)):
        pred, c, ce = m.predict_scene(pool, s, stride=64, batch=8, norm_type=1, views="flips", erode=3, scales=SCALES)
        assert np.array_equal(maps[s], pred)
        total, total_e = total + c, total_e + ce
    assert np.array_equal(cm, total) and np.array_equal(cm_e, total_e) and cm.sum() == sum(h * w for h, w in pool.shapes)


def test_cli_scores_a_scene_directory_with_scales(tmp_path, capsys):
    """eval_scenes_ISPRS.py --scales 0.75 1 1.5 --views flips on a tiny scene directory: its maps and matrix against evaluate_scenes."""
    import eval_scenes_ISPRS
    from resunet_a_mltsk_keras_amd.keras_api import load_model
    sc = [blob_scene(300, 90, 100), blob_scene(301, 86, 120)]
    root, path, out = str(tmp_path / "scenes"), str(tmp_path / "m.h5"), str(tmp_path / "preds")
    scenes.save_scene_dir(root, ["a_tile", "b_tile"], [s[0] for s in sc], [s[1] for s in sc])
    new_model(seed=11, depth=4, split_k=True).save(path)         # four levels: a small file; split_k as load_model leaves it
    argv = ["--use_multitasking", "--model_path", path, "--dataset_path", root, "-ps", "64", "--num_classes", str(NCLS), "--output_path", out,
            "--views", "flips", "--stride", "48", "--batch_size", "8"]
    res = eval_scenes_ISPRS.main(argv + ["--scales", "0.75", "1", "1.5"])
    printed = capsys.readouterr().out
    assert "views: 0 3 4 (3 per window)" in printed and "scales: 0.75 1 1.5 (3 passes per view)" in printed
    names, images, class_maps = scenes.load_scene_dir(root)
    model = load_model(path, compile=False)
    maps, cm = model.evaluate_scenes(scenes.ScenePool(images, class_maps, patch=64), stride=48, batch_size=8, norm_type=1, views="flips", scales=SCALES)
    assert cm.sum() == 90 * 100 + 86 * 120 and np.array_equal(res["confusion_matrix"], cm)
    per_scene = 0
    for name, want in zip(names, maps):
        got = np.load(os.path.join(out, f"pred_seg_reconstructed_{name}.npy"))
        assert got.dtype == np.uint8 and np.array_equal(got, want)
        per_scene = per_scene + np.load(os.path.join(out, f"confusion_matrix_{name}.npy"))
    assert np.array_equal(per_scene, cm)
    assert res["accuracy"] == eval_scenes_ISPRS.metrics_from_confusion(cm)[0]
    with pytest.raises(SystemExit, match="--scales: scene a_tile: .* larger than the 90 x 100 scene"):
        eval_scenes_ISPRS.main(argv + ["--scales", "1", "0.6"])
