"""GPU tests of blended whole-scene prediction: rua_scene_accumulate_blend (csrc/scene.hip) through the C ABI, every int32 sum against
scenes.host_accumulate_blend - overlapping groups in one launch and across launches, any order, split calls - and its argument checks;
Engine.predict_scene(blend="linear") against the host definitions of the probabilities it accumulated, with scales, erode and
boundary, through Model.evaluate_scenes and through eval_scenes_ISPRS.py --blend."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from resunet_a_mltsk_keras_amd import _lib as L
from resunet_a_mltsk_keras_amd import scenes

from _scene_util import GUARD, NCLS, blob_pool, blob_scene, new_engine, new_model
from test_scene_blend_host import SHAPES as REFUSAL_SHAPES, blend_refusals, two_scene_tables

pytestmark = pytest.mark.gpu

f32 = np.float32
FLAT = (0, 2, 3, 4)
GUARD_WORDS, GUARD_VALUE = GUARD // 4, -0x11111112
ENTRY = "rua_scene_accumulate_blend"


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def sizes(shapes):
    return (ctypes.c_int32 * len(shapes))(*[h for h, _ in shapes]), (ctypes.c_int32 * len(shapes))(*[w for _, w in shapes])


def pass_tables(shapes, patch, footprint, stride, views):
    """blend_table of every scene the footprint fits, concatenated, with the scene index in column 0: one call's groups."""
    parts = []
    for s, shp in enumerate(shapes):
        if footprint[0] <= shp[0] and footprint[1] <= shp[1]:
            rows7, foot = scenes.blend_table(shp, patch, footprint, stride, views)
            rows7[:, 0] = s
            parts.append((rows7, foot))
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def random_p(rng, n, patch, C):
    """float32 [n][PH][PW][C]: mostly rng.random, 3 % of the values outside 0..1, exact 0 and 1 and ties at the rounding point."""
    p = rng.random((n,) + tuple(patch) + (C,), dtype=f32)
    odd = rng.random(p.shape) < 0.03
    p[odd] = rng.choice(np.array([-0.25, 1.5, 0.0, 1.0, 2.0 ** -17, 3 * 2.0 ** -17, 0.5], f32), int(odd.sum()))
    return p


class Accumulators:
    """One pre-filled int32 [H][W][C] device accumulator per scene with guard words before and behind it, and its host twin."""

    def __init__(self, rng, shapes, C, host=None):
        self.shapes, self.C = shapes, C
        self.host = [rng.integers(-50000, 50000, (H, W, C)).astype(np.int32) for H, W in shapes] if host is None else [a.copy() for a in host]
        self.dev = []
        for a in self.host:
            t = torch.full((a.size + 2 * GUARD_WORDS,), GUARD_VALUE, dtype=torch.int32, device="cuda")
            t[GUARD_WORDS:GUARD_WORDS + a.size] = torch.from_numpy(a.ravel()).cuda()
            self.dev.append(t)

    def ptrs(self):
        return (ctypes.c_void_p * len(self.dev))(*[t.data_ptr() + 4 * GUARD_WORDS for t in self.dev])

    def read(self):
        out = []
        for t, (H, W) in zip(self.dev, self.shapes):
            g, n = t.cpu().numpy(), H * W * self.C
            assert (g[:GUARD_WORDS] == GUARD_VALUE).all() and (g[GUARD_WORDS + n:] == GUARD_VALUE).all(), "words around an accumulator were written"
            out.append(g[GUARD_WORDS:GUARD_WORDS + n].reshape(H, W, self.C))
        return out

    def call(self, p, rows7, foot, K, C=None, expect_error=None):
        pd = torch.from_numpy(np.ascontiguousarray(p)).cuda()
        r, o = np.ascontiguousarray(rows7, dtype=np.int32), np.ascontiguousarray(foot, dtype=np.int32)
        hs, ws = sizes(self.shapes)
        args = (pd.data_ptr(), len(o), K, p.shape[1], p.shape[2], p.shape[3] if C is None else C, r.ctypes.data, o.ctypes.data, self.ptrs(),
                hs, ws, len(self.shapes), stream())
        if expect_error is None:
            L.lib().call(ENTRY, *args)
        else:
            with pytest.raises(L.RuaError, match=expect_error):
                L.lib().call(ENTRY, *args)
        torch.cuda.synchronize()

    def assert_equal_host(self, what):
        for s, (g, w) in enumerate(zip(self.read(), self.host)):
            bad = np.argwhere(g != w)
            assert bad.size == 0, (what, f"scene {s}", len(bad), "first at", tuple(bad[0]), int(g[tuple(bad[0])]), int(w[tuple(bad[0])]))


def blend_case(seed, shapes, patch, footprints, strides, views, C):
    """Every (footprint, stride) one call - one pass, its groups overlap - over all the scenes the footprint fits, into the same
    pre-filled accumulators; the host definition adds the same passes; all sums equal at the end."""
    rng = np.random.default_rng(seed)
    codes = scenes.check_views(views, patch)
    K = len(codes)
    acc = Accumulators(rng, shapes, C)
    before = [a.copy() for a in acc.host]
    overlap = False
    for F in footprints:
        for stride in strides:
            rows7, foot = pass_tables(shapes, patch, F, stride, codes)
            p = random_p(rng, len(rows7), patch, C)
            acc.call(p, rows7, foot, K)
            scenes.host_accumulate_blend(p, rows7, foot, shapes, K, acc=acc.host)
            overlap |= len(foot) > sum(1 for shp in shapes if F[0] <= shp[0] and F[1] <= shp[1])
    assert overlap and all((a != b).any() for a, b in zip(acc.host, before))
    acc.assert_equal_host((patch, views, C))


SHAPES = [(19, 23), (8, 8)]


# P = (8, 8); footprints 5 (zoomed in), 8 (the patch; the whole 8 x 8 scene: every weight 256) and 13 (zoomed out; the first scene only)
# at strides 3, 4 and 8 (at 8 the footprints of the 19 x 23 scene still overlap where the last one is flush with the border).
# C = 5: an accumulator row starts at any dword; C = 64: one tile row is 4096 elements.
@pytest.mark.parametrize("C", [1, 3, 5, 64])
@pytest.mark.parametrize("views", [(0,), "aug5", "all", (5, 7)])
def test_blend_bitwise(views, C):
    blend_case(C * 10 + len(scenes.check_views(views)), SHAPES, (8, 8), [(5, 5), (8, 8), (13, 13)], (3, 4, 8), views, C)


def test_blend_bitwise_odd_patch():
    """A (7, 9) patch takes the codes that do not transpose; footprints smaller, equal and larger, a stride pair."""
    blend_case(7, SHAPES[:1], (7, 9), [(5, 6), (7, 9), (11, 14)], ((3, 4), (7, 9)), FLAT, 5)


def test_blend_wide_footprints_cross_the_weight_tables_ends():
    """Footprints of 100 x 150 scene pixels for a 32 x 48 window on a 130 x 200 scene: four of them (origins 0 and 30, 0 and 50), each
    7 x 3 tiles of 16 x 64, ragged at both ends; one flat side per axis, the taper and its floor on the other."""
    rows7, foot = scenes.blend_table((130, 200), (32, 48), (100, 150), (32, 48), (0, 2))
    assert foot.tolist() == [[0, 100, 0, 150], [0, 100, 50, 200], [30, 130, 0, 150], [30, 130, 50, 200]]
    blend_case(3, [(130, 200)], (32, 48), [(100, 150)], ((32, 48),), (0, 2), 5)


def sixty_groups(rng, C=3):
    """P = F = (2, 2) at stride 1 on a 7 x 11 scene: 60 groups of K = 2, a launch carries 24, and neighbours in different launches overlap."""
    shape = (7, 11)
    rows7, foot = scenes.blend_table(shape, (2, 2), (2, 2), 1, (0, 2))
    assert len(foot) == 60 and foot[23].tolist() == [2, 4, 3, 5] and foot[33].tolist() == [3, 5, 3, 5]      # the last group of the first launch and one of the second
    return shape, rows7, foot, random_p(rng, len(rows7), (2, 2), C)


def test_blend_more_groups_than_one_launch_in_any_order_and_split():
    rng = np.random.default_rng(4)
    K = 2
    shape, rows7, foot, p = sixty_groups(rng)
    G = len(foot)
    acc = Accumulators(rng, [shape], 3)
    start = [a.copy() for a in acc.host]
    acc.call(p, rows7, foot, K)
    scenes.host_accumulate_blend(p, rows7, foot, [shape], K, acc=acc.host)
    acc.assert_equal_host("60 groups")
    want = acc.read()[0]
    # the groups in reverse order: bit for bit the same
    order = np.arange(G)[::-1]
    rev = Accumulators(rng, [shape], 3, host=start)
    rev.call(p.reshape((G, K) + p.shape[1:])[order].reshape(p.shape), rows7.reshape(G, K, 7)[order].reshape(-1, 7), foot[order], K)
    assert np.array_equal(rev.read()[0], want)
    # split over two calls into the carried accumulator, the cut inside a launch's chunk
    two = Accumulators(rng, [shape], 3, host=start)
    h = 31
    two.call(p[:h * K], rows7[:h * K], foot[:h], K)
    two.call(p[h * K:], rows7[h * K:], foot[h:], K)
    assert np.array_equal(two.read()[0], want)


def test_blend_order_and_split_on_tapered_footprints():
    """The same on footprints with real tapers: 13 x 13 at stride 6 on the 19 x 23 scene, K = 3, C = 5."""
    rng = np.random.default_rng(8)
    K = 3
    rows7, foot = scenes.blend_table(SHAPES[0], (8, 8), (13, 13), 6, (0, 3, 6))
    G = len(foot)
    p = random_p(rng, G * K, (8, 8), 5)
    acc = Accumulators(rng, SHAPES[:1], 5)
    start = [a.copy() for a in acc.host]
    acc.call(p, rows7, foot, K)
    scenes.host_accumulate_blend(p, rows7, foot, SHAPES[:1], K, acc=acc.host)
    acc.assert_equal_host("in order")
    want = acc.read()[0]
    order = np.arange(G)[::-1]
    rev = Accumulators(rng, SHAPES[:1], 5, host=start)
    rev.call(p.reshape((G, K) + p.shape[1:])[order].reshape(p.shape), rows7.reshape(G, K, 7)[order].reshape(-1, 7), foot[order], K)
    assert np.array_equal(rev.read()[0], want)
    two = Accumulators(rng, SHAPES[:1], 5, host=start)
    two.call(p[:K], rows7[:K], foot[:1], K)
    two.call(p[K:], rows7[K:], foot[1:], K)
    assert np.array_equal(two.read()[0], want)


def test_blend_empty_rectangles_among_full_ones():
    rng = np.random.default_rng(5)
    rows7, foot = pass_tables([(33, 40), (19, 23)], (8, 8), (13, 13), 6, (0, 3))
    p = random_p(rng, len(rows7), (8, 8), 5)
    acc = Accumulators(rng, [(33, 40), (19, 23)], 5)
    nothing = foot.copy()
    nothing[::3] = 0                                           # the padding groups of a last batch
    nothing[1::3, 1] = nothing[1::3, 0]                        # no rows
    nothing[2::3, 3] = nothing[2::3, 2]                        # no columns
    acc.call(p, rows7, nothing, 2)
    acc.assert_equal_host("all empty")
    some = foot.copy()
    some[::2] = nothing[::2]
    acc.call(p, rows7, some, 2)
    scenes.host_accumulate_blend(p, rows7, some, acc.shapes, 2, acc=acc.host)
    acc.assert_equal_host("half empty")


def test_blend_special_floats():
    rng = np.random.default_rng(6)
    rows7, foot = pass_tables([(33, 40), (19, 23)], (8, 8), (13, 13), 6, (0, 6))
    p = rng.random((len(rows7), 8, 8, 3), dtype=f32)
    odd = rng.random(p.shape) < 0.3
    p[odd] = rng.choice(np.array([np.nan, np.inf, -np.inf, -1.0, 7.0, -0.0, 1e-30, 1 - 2.0 ** -24, 2.0 ** -17], f32), int(odd.sum()))
    acc = Accumulators(rng, [(33, 40), (19, 23)], 3)
    acc.call(p, rows7, foot, 2)
    scenes.host_accumulate_blend(p, rows7, foot, acc.shapes, 2, acc=acc.host)
    acc.assert_equal_host("special floats")


def test_blend_refuses_bad_arguments_in_the_host_checkers_words():
    rng = np.random.default_rng(7)
    shapes = REFUSAL_SHAPES
    rows7, foot = two_scene_tables((0, 6))
    p = random_p(rng, len(rows7), (8, 8), 3)
    acc = Accumulators(rng, shapes, 3)
    for r, o, msg in blend_refusals(rows7, foot):
        acc.call(p, r, o, 2, expect_error=msg)
        with pytest.raises(ValueError, match=msg):                # the host definition refuses the same tables in the same words
            scenes.host_accumulate_blend(p, r, o, shapes, 2)
    acc.call(p, rows7, foot, 0, expect_error="rua_scene_accumulate_blend: K 0 outside 1..8")
    acc.call(p, rows7, foot, 9, expect_error="rua_scene_accumulate_blend: K 9 outside 1..8")
    acc.call(p, rows7, foot, 2, C=65, expect_error="rua_scene_accumulate_blend: C 65 outside 1..64")
    acc.call(p, rows7, foot, 2, C=0, expect_error="C 0 outside 1..64")
    frows, ffoot = scenes.blend_table(shapes[0], (4, 12), (4, 12), 4, (0, 3))
    frows[3, 3:] = [0, 65536, 65536, 0]
    msg = r"rua_scene_accumulate_blend: row 3: matrix \(0, 65536, 65536, 0\) transposes and needs a square patch \(got 4 x 12\)"
    acc.call(np.zeros((len(frows), 4, 12, 3), f32), frows, ffoot, 2, expect_error=msg)
    with pytest.raises(ValueError, match=msg):
        scenes.host_accumulate_blend(np.zeros((len(frows), 4, 12, 3), f32), frows, ffoot, shapes, 2)
    hs, ws = sizes(shapes)
    pd = torch.from_numpy(p).cuda()
    big = (ctypes.c_int32 * 2)(16385, 19)
    null = (ctypes.c_void_p * 2)(acc.ptrs()[0], None)
    G = len(foot)
    for args, msg in (((pd.data_ptr() + 4, G, 2, 8, 8, 3, rows7.ctypes.data, foot.ctypes.data, acc.ptrs(), hs, ws, 2), "rua_scene_accumulate_blend: p must be 16-byte aligned"),
                      ((pd.data_ptr(), G, 2, 8, 513, 3, rows7.ctypes.data, foot.ctypes.data, acc.ptrs(), hs, ws, 2), r"PH 8, PW 513 \(1 <= PH, PW <= 512\)"),
                      ((pd.data_ptr(), G, 2, 8, 8, 3, rows7.ctypes.data, foot.ctypes.data, acc.ptrs(), big, ws, 2), r"scene 0: size 16385 x 40 \(1 <= H, W <= 16384\)"),
                      ((pd.data_ptr(), G, 2, 8, 8, 3, rows7.ctypes.data, foot.ctypes.data, null, hs, ws, 2), "scene 1: null or misaligned accumulator"),
                      ((pd.data_ptr(), 0, 2, 8, 8, 3, rows7.ctypes.data, foot.ctypes.data, acc.ptrs(), hs, ws, 2), r"nscenes 2, G 0 \(both >= 1\)"),
                      ((None, G, 2, 8, 8, 3, rows7.ctypes.data, foot.ctypes.data, acc.ptrs(), hs, ws, 2), "rua_scene_accumulate_blend: p, windows7, own, scene_acc, scene_h and scene_w are required")):
        with pytest.raises(L.RuaError, match=msg):
            L.lib().call(ENTRY, *args, stream())
    torch.cuda.synchronize()
    acc.assert_equal_host("a refused call wrote something")
    acc.call(p, rows7, foot, 2)                                # and the tables themselves are fine
    scenes.host_accumulate_blend(p, rows7, foot, shapes, 2, acc=acc.host)
    acc.assert_equal_host("the unspoilt tables")


# ---- engine / model level -------------------------------------------------------------------------------------------------------
SCALES = (0.75, 1.0, 1.5)                                     # footprints 85, 64 and 43 of the 64 x 64 patch


@pytest.fixture(scope="module")
def pool():
    return blob_pool((128, 128))


def host_of(seen, pool, scene, K):
    """host_argmax(host_accumulate_blend(...)) of the batches on_batch saw, in their order: (map, confusion matrix) of `scene`."""
    acc = None
    for r, o, p in seen:
        acc = scenes.host_accumulate_blend(p, r, o, pool.shapes, K, acc=acc)
    maps, cm = scenes.host_argmax([acc[scene]], [pool.class_maps[scene]], NCLS)
    return maps[0], cm


@pytest.mark.parametrize("use_graph", [True, False])
def test_predict_scene_blend_is_the_host_definition_of_its_probabilities(pool, use_graph):
    """The 128 x 128 scene; stride None is half the patch: 9 footprints single-scale, 4 + 9 + 25 under the three scales.  views (0,) at
    batch 8 and flips at batch 8 (G = 2) pad the last batch of a pass; erode and boundary score the finished map."""
    eng = new_engine(True, use_graph)
    scene = 1
    for scales in (None, SCALES):
        for views in ((0,), "flips"):
            codes = scenes.check_views(views)
            K = len(codes)
            G = max(1, 8 // K)
            seen = []
            pred, cm, cm_e, bc = eng.predict_scene(pool, scene, batch=8, norm_type=1, views=views, scales=scales, blend="linear", erode=3, boundary=3,
                                                   on_batch=lambda r, o, p: seen.append((r.copy(), o.copy(), p.cpu().numpy())))
            fps = [(64, 64)] if scales is None else [scenes.scale_footprint(64, z) for z in scales]
            tables = [scenes.blend_table(pool.shapes[scene], 64, fp, (32, 32), codes) for fp in fps]
            assert [len(t[1]) for t in tables] == ([9] if scales is None else [4, 9, 25])
            assert len(seen) == sum(-(-len(t[1]) // G) for t in tables)
            assert all(r.shape == (G * K, 7) and o.shape == (G, 4) and p.shape == (G * K, 64, 64, NCLS) and (r[:, 0] == scene).all() for r, o, p in seen)
            k = 0
            for rows7, foot in tables:                                # each pass in order, its last batch padded with empty rectangles
                nb = -(-len(foot) // G)
                r, o = np.concatenate([s[0] for s in seen[k:k + nb]]), np.concatenate([s[1] for s in seen[k:k + nb]])
                assert np.array_equal(r[:len(rows7), 1:], rows7[:, 1:]) and np.array_equal(o[:len(foot)], foot) and (o[len(foot):] == 0).all()
                k += nb
            assert all(np.isfinite(s[2]).all() for s in seen)
            want, want_cm = host_of(seen, pool, scene, K)
            what = (use_graph, scales, views)
            assert pred.dtype == np.uint8 and pred.shape == pool.shapes[scene] and np.array_equal(pred, want), what
            assert cm.dtype == np.int64 and np.array_equal(cm, want_cm) and cm.sum() == pred.size, what
            assert np.array_equal(cm_e, scenes.host_erode_confusion(pool.class_maps[scene], pred, 3, NCLS)), what
            assert np.array_equal(bc, scenes.host_boundary_counts(pool.class_maps[scene], pred, 3, NCLS)), what
            assert len(np.unique(pred)) > 1
            plain = eng.predict_scene(pool, scene, batch=8, norm_type=1, views=views, scales=scales, blend="linear")
            assert len(plain) == 2 and np.array_equal(plain[0], pred) and np.array_equal(plain[1], cm)
    # (1.0,) is the single-scale blend, and an explicit stride is taken
    a = eng.predict_scene(pool, scene, batch=8, scales=(1.0,), blend="linear")
    b = eng.predict_scene(pool, scene, batch=8, stride=32, blend="linear")
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_blend_none_is_the_call_without_blend_and_refusals(pool, monkeypatch):
    eng = new_engine(False, True)
    lib = L.lib()
    log, every = [], []
    real = lib.call

    def logged(name, *args):
        every.append(name)
        if name.startswith("rua_scene_"):                       # what the forward between them launches depends on whether its graph is captured yet
            log.append(name)
        return real(name, *args)
    monkeypatch.setattr(lib, "call", logged)
    for kw in ({}, {"views": "flips"}, {"scales": (1.0, 2.0)}, {"views": "flips", "erode": 2, "heads": ("seg",)}):
        results = []
        for blend in ({}, {"blend": None}):
            del log[:]
            results.append((eng.predict_scene(pool, 0, stride=48, batch=5, **kw, **blend), list(log)))
        (want, want_calls), (got, calls) = results
        assert calls == want_calls and ENTRY not in calls and len(calls) > 1
        assert len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got[:2], want[:2]))
    del log[:]
    eng.predict_scene(pool, 1, batch=8, blend="linear")                                         # 9 footprints: two batches
    assert log.count(ENTRY) == 2 and log.count("rua_scene_argmax") == 1 and log.count("rua_scene_windows_affine") == 2
    assert not any(n in log for n in ("rua_scene_accumulate", "rua_scene_stitch", "rua_scene_stitch_views", "rua_scene_stitch_maps", "rua_scene_windows"))
    # refusals come before any launch
    del every[:]
    with pytest.raises(ValueError, match="blended maps of the heads are not built"):
        eng.predict_scene(pool, 1, blend="linear", heads=("seg",))
    for bad in ("cosine", "", 1, True, ("linear",)):
        with pytest.raises(ValueError, match="blend .*: None or one of"):
            eng.predict_scene(pool, 1, blend=bad)
    with pytest.raises(ValueError, match="check_blend_budget: K 8 views times 4096 footprints over one pixel"):
        eng.predict_scene(pool, 1, stride=1, views="all", blend="linear")
    with pytest.raises(ValueError, match="larger than the 128 x 128 scene"):
        eng.predict_scene(pool, 1, scales=(1.0, 0.45), blend="linear")
    assert every == []
    bare = scenes.ScenePool(pool.images, None, patch=64)       # no class maps: the map alone
    pred, cm = eng.predict_scene(bare, 1, batch=8, blend="linear")
    assert cm is None and np.array_equal(pred, eng.predict_scene(pool, 1, batch=8, blend="linear")[0])


def test_evaluate_scenes_and_the_cli_blend(tmp_path, capsys):
    """evaluate_scenes(blend=) sums predict_scene(blend=) over the scenes; eval_scenes_ISPRS.py --blend linear writes its maps and matrix
    and names the choice in the report, the returned dict and eval_settings.json."""
    import eval_scenes_ISPRS
    from resunet_a_mltsk_keras_amd.keras_api import load_model
    sc = [blob_scene(300, 90, 100), blob_scene(301, 86, 120)]
    root, path, out = str(tmp_path / "scenes"), str(tmp_path / "m.h5"), str(tmp_path / "preds")
    scenes.save_scene_dir(root, ["a_tile", "b_tile"], [s[0] for s in sc], [s[1] for s in sc])
    new_model(seed=11, depth=4, split_k=True).save(path)         # four levels: a small file; split_k as load_model leaves it
    argv = ["--use_multitasking", "--model_path", path, "--dataset_path", root, "-ps", "64", "--num_classes", str(NCLS), "--output_path", out,
            "--views", "flips", "--batch_size", "8", "--erode_boundary", "3"]
    res = eval_scenes_ISPRS.main(argv + ["--blend", "linear"])
    printed = capsys.readouterr().out
    assert "views: 0 3 4 (3 per window)" in printed and "blend: linear" in printed and res["blend"] == "linear"
    with open(os.path.join(out, "eval_settings.json")) as f:
        assert json.load(f) == {"views": [0, 3, 4], "scales": None, "stride": None, "blend": "linear"}
    names, images, class_maps = scenes.load_scene_dir(root)
    model = load_model(path, compile=False)
    pool = scenes.ScenePool(images, class_maps, patch=64)
    maps, cm, cm_e = model.evaluate_scenes(pool, batch_size=8, norm_type=1, views="flips", erode=3, blend="linear")
    total, total_e = 0, 0
    for s in range(len(pool)):
        pred, c, ce = model.predict_scene(pool, s, batch=8, norm_type=1, views="flips", erode=3, blend="linear")
        assert np.array_equal(maps[s], pred)
        total, total_e = total + c, total_e + ce
    assert np.array_equal(cm, total) and np.array_equal(cm_e, total_e) and cm.sum() == 90 * 100 + 86 * 120
    assert np.array_equal(res["confusion_matrix"], cm) and np.array_equal(res["confusion_matrix_eroded"], cm_e)
    for name, want in zip(names, maps):
        got = np.load(os.path.join(out, f"pred_seg_reconstructed_{name}.npy"))
        assert got.dtype == np.uint8 and np.array_equal(got, want)
    unblended = model.evaluate_scenes(pool, stride=32, batch_size=8, norm_type=1, views="flips")
    assert any((a != b).any() for a, b in zip(maps, unblended[0]))     # the blend is not the cut
    with pytest.raises(SystemExit, match="--blend and --head_maps exclude each other"):
        eval_scenes_ISPRS.main(argv + ["--blend", "linear", "--head_maps", "seg"])
