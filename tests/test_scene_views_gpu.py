"""GPU tests of test-time augmentation for whole-scene evaluation: rua_scene_stitch_views (csrc/scene.hip) byte for byte against
scenes.host_stitch_views through the C ABI - the K views of a window turned back and summed in float32 in view order -, its argument
checks, Engine.predict_scene(views=) against host_stitch_views of the probabilities it stitched and against the predict() route, and
eval_scenes_ISPRS.py --views against Model.evaluate_scenes(views=)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from resunet_a_mltsk_keras_amd import _lib as L
from resunet_a_mltsk_keras_amd import scenes

from _scene_util import FILL, NCLS, blob_pool, blob_scene, conf_pattern, guarded_maps, new_engine, new_model, read_guarded, table_of

pytestmark = pytest.mark.gpu

E = np.float32(2.0 ** -24)


def make_inputs(seed, shapes, G, codes, PH, PW, C):
    """(p [G*K][PH][PW][C], class maps).  The un-transformed stack q [G][K][PH][PW][C] comes first, p[g*K + k] = transform(q[g, k],
    code_k).  q: rng.random float32 (no subnormals); about 5 % of the pixels hold an exact tie (two classes at 2.0 in every view);
    for K >= 3 about 5 % hold the order pattern: class a (1, e, e, 0, ...) over the views, class b (e, e, 1, 0, ...), e = 2^-24, every
    other class 0.25 / K - summed in float32 in view order a is 1 and b 1 + 2^-23 (b wins), in any wider precision they tie (the
    lower index wins), in reverse order a wins.  Class maps: uniform in 0..C-1 with 2 % of 255s."""
    rng = np.random.default_rng(seed)
    K = len(codes)
    q = rng.random((G, K, PH, PW, C), dtype=np.float32)
    tie = np.argwhere(rng.random((G, PH, PW)) < 0.05)
    a = rng.integers(0, C, len(tie))
    b = (a + rng.integers(1, C, len(tie))) % C               # another class
    q[tie[:, 0], :, tie[:, 1], tie[:, 2], a] = 2.0
    q[tie[:, 0], :, tie[:, 1], tie[:, 2], b] = 2.0
    if K >= 3:
        pat = np.argwhere(rng.random((G, PH, PW)) < 0.05)
        a = rng.integers(0, C, len(pat))
        b = (a + rng.integers(1, C, len(pat))) % C
        va, vb = np.zeros(K, np.float32), np.zeros(K, np.float32)
        va[:3], vb[:3] = [1, E, E], [E, E, 1]
        q[pat[:, 0], :, pat[:, 1], pat[:, 2], :] = np.float32(0.25 / K)
        q[pat[:, 0], :, pat[:, 1], pat[:, 2], a] = va[None, :]
        q[pat[:, 0], :, pat[:, 1], pat[:, 2], b] = vb[None, :]
    p = np.stack([scenes.transform(q[g, k], c) for g in range(G) for k, c in enumerate(codes)])
    maps = []
    for H, W in shapes:
        m = rng.integers(0, C, (H, W)).astype(np.uint8)
        m[rng.random((H, W)) < 0.02] = 255
        maps.append(m)
    return np.ascontiguousarray(p), maps


def test_the_order_pattern_tells_orders_and_precisions_apart():
    """The generator's planted pixels on the host: in-order float32 gives b, float64 the tie's lower index, the reverse order a."""
    codes = scenes.VIEW_SETS["aug5"]
    rows, own = np.array([[0, 0, 0, 0]], np.int32), np.array([[0, 16, 0, 16]], np.int32)
    p, _ = make_inputs(9, [(16, 16)], 1, codes, 16, 16, 5)
    q = np.stack([scenes.transform(p[k], scenes.INVERSE[c]) for k, c in enumerate(codes)])
    planted = (q[0] == 1).sum(-1) == 1                       # class a holds 1 in view 0
    assert 3 < planted.sum() < 40
    got = scenes.host_stitch_views(p, scenes.view_rows(rows, codes), own, [(16, 16)])[0][0]
    a, b = np.argmax(q[0] == 1, -1), np.argmax(q[2] == 1, -1)
    assert (got[planted] == b[planted]).all() and (a != b)[planted].all()
    wide = np.argmax(q.astype(np.float64).sum(0), -1)
    assert (wide[planted] == np.minimum(a, b)[planted]).all()
    back = scenes.host_stitch_views(p[::-1], scenes.view_rows(rows, codes[::-1]), own, [(16, 16)])[0][0]
    assert (back[planted] == a[planted]).all()


def run_stitch(p, rows, own, shapes, class_maps, K=None, C=None, expect_error=None, name="rua_scene_stitch_views"):
    """rua_scene_stitch_views (or, with name, rua_scene_stitch) into 0xEE-filled maps with a guard region behind each and a
    pre-filled confusion matrix; returns (maps, confusion - its initial pattern or None) and checks the guards.  expect_error: the
    call must fail with this text and leave every output as it was."""
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
    tail = (PH, PW, C, r.ctypes.data, o.ctypes.data, pred_ptrs, cls_ptrs, hs, ws, n,
            None if conf is None else conf.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    if name == "rua_scene_stitch":
        args = (pd.data_ptr(), N) + tail
    else:
        K = len(r) // len(o) if K is None else K
        args = (pd.data_ptr(), len(o), K) + tail
    if expect_error is not None:
        with pytest.raises(L.RuaError, match=expect_error):
            L.lib().call(name, *args)
    else:
        L.lib().call(name, *args)
    torch.cuda.synchronize()
    maps = read_guarded(pred, shapes)
    cm = None if conf is None else conf.cpu().numpy() - conf0
    if expect_error is not None:
        assert all((m == FILL).all() for m in maps) and (cm is None or (cm == 0).all()), "a refused call wrote something"
    return maps, cm


def assert_stitch(p, rows, own, shapes, class_maps):
    got_maps, got_cm = run_stitch(p, rows, own, shapes, class_maps)
    want_maps, want_cm = scenes.host_stitch_views(p, rows, own, shapes, class_maps, fill=FILL)
    for s, (g, w) in enumerate(zip(got_maps, want_maps)):
        bad = np.argwhere(g != w)
        assert bad.size == 0, (f"scene {s}", len(bad), "first at", tuple(bad[0]), int(g[tuple(bad[0])]), int(w[tuple(bad[0])]))
    if class_maps is None:
        assert got_cm is None and want_cm is None
    else:
        assert np.array_equal(got_cm, want_cm), (got_cm - want_cm)
    return want_maps


def bitwise_case(seed, shapes, patch, stride, views, C):
    """With and without class maps, and again with every other group dropped (unowned pixels keep their bytes)."""
    codes = scenes.check_views(views, patch)
    K = len(codes)
    rows, own = table_of(shapes, patch, stride)
    G = len(rows)
    p, maps = make_inputs(seed, shapes, G, codes, patch[0], patch[1], C)
    vr = scenes.view_rows(rows, codes)
    want = assert_stitch(p, vr, own, shapes, maps)
    assert all((m != FILL).all() for m in want)                # the table covers every pixel
    assert_stitch(p, vr, own, shapes, None)                    # maps only: both pointers null
    keep = np.arange(0, G, 2)
    pk = p.reshape(G, K, *p.shape[1:])[keep].reshape(-1, *p.shape[1:])
    half = assert_stitch(pk, scenes.view_rows(rows[keep], codes), own[keep], shapes, maps)
    assert any((m == FILL).any() for m in half)


# (40, 57): an odd width, so scene rows start at every byte phase; the last windows are flush with the border.  C = 5: a pixel is 20
# bytes, view rows start at every dword phase of a 16-byte piece.  C = 3, 5, 6, 64 give tiles of 32, 28, 24 and 8 pixels: one tile
# per 32 x 32 window, ragged tiles, and 16 tiles a window.
@pytest.mark.parametrize("C", [3, 5, 6, 64])
@pytest.mark.parametrize("views", ["flips", "aug5", "all", (5, 7)])
def test_stitch_views_bitwise(views, C):
    bitwise_case(C * 100 + len(scenes.check_views(views)), [(40, 57), (32, 32)], (32, 32), 24, views, C)


@pytest.mark.parametrize("C", [3, 5, 6, 64])
def test_stitch_views_bitwise_flat_patch(C):
    """A 16 x 48 patch takes the codes that do not transpose.  Stride 24 along its 48 columns, 12 along its 16 rows (a stride may not
    exceed the patch: the windows would leave gaps)."""
    bitwise_case(C * 100 + 16, [(40, 57)], (16, 48), (12, 24), (0, 2, 3, 4), C)


def test_stitch_views_bitwise_odd_patch():
    """Patch 37, C = 5 (tiles of 28): the odd edge crosses tile borders under every symmetry."""
    bitwise_case(37, [(45, 61)], (37, 37), 20, "all", 5)


def test_one_view_of_code_0_is_scene_stitch():
    shapes = [(40, 57), (32, 32)]
    rows, own = table_of(shapes, (32, 32), 24)
    p, maps = make_inputs(11, shapes, len(rows), (0,), 32, 32, 5)
    for cm_in in (maps, None):
        got = run_stitch(p, rows, own, shapes, cm_in)
        want = run_stitch(p, rows, own, shapes, cm_in, name="rua_scene_stitch")
        assert all(np.array_equal(g, w) for g, w in zip(got[0], want[0])) and not any((m == FILL).any() for m in got[0])
        assert (got[1] is None and want[1] is None) if cm_in is None else np.array_equal(got[1], want[1])


def test_stitch_views_more_groups_than_one_launch():
    """150 groups of K = 2 (a launch carries 120): stride 1 on three small scenes, the first 150 rows of 361."""
    shapes = [(40, 57), (32, 32), (45, 40)]
    rows, own = table_of(shapes, (32, 32), 1)
    assert len(rows) > 150
    rows, own = rows[:150], own[:150]
    p, maps = make_inputs(2, shapes, 150, (6, 2), 32, 32, 5)
    assert_stitch(p, scenes.view_rows(rows, (6, 2)), own, shapes, maps)


@pytest.mark.parametrize("views", [(3, 6, 0), (0, 3, 6), (7,)])
def test_stitch_views_one_group(views):
    """G = 1, and a p of K * 31 * 31 * 5 floats - no whole number of 16-byte pieces - owned up to the window's last pixel."""
    p, maps = make_inputs(1, [(33, 47)], 1, views, 31, 31, 5)
    assert p.size % 4
    rows = scenes.view_rows(np.array([[0, 1, 14, 0]], np.int32), views)
    assert_stitch(p, rows, np.array([[3, 31, 1, 31]], np.int32), [(33, 47)], maps)
    assert_stitch(p, rows, np.array([[0, 31, 0, 31]], np.int32), [(33, 47)], maps)


def test_stitch_views_empty_rectangles():
    shapes = [(40, 57), (32, 32)]
    rows, own = table_of(shapes, (32, 32), 24)
    own = own.copy()
    own[3, 1] = own[3, 0]                                      # no rows
    own[5, 3] = own[5, 2]                                      # no columns
    own[len(own) - 1] = 0                                      # the padding group of a last batch
    p, maps = make_inputs(4, shapes, len(rows), (0, 3, 4), 32, 32, 5)
    want = assert_stitch(p, scenes.view_rows(rows, "flips"), own, shapes, maps)
    assert (want[0] == FILL).any() and (want[1] == FILL).all()


def test_stitch_views_refuses_bad_arguments():
    shapes = [(40, 57), (32, 32)]
    rows, own = table_of(shapes, (32, 32), 24)
    codes = (0, 1, 4)
    p, maps = make_inputs(5, shapes, len(rows), codes, 32, 32, 5)
    vr = scenes.view_rows(rows, codes)

    def with_row(table, k, col, v):
        t = table.copy()
        t[k, col] = v
        return t
    refused = [
        (with_row(vr, 4, 2, 23), own, r"row 4: scene 0, window \(0, 23\), but its group 1 is scene 0, window \(0, 24\)"),
        (with_row(vr, 1, 0, 1), own, r"row 1: scene 1, window \(0, 0\), but its group 0 is scene 0, window \(0, 0\)"),
        (with_row(vr, 7, 1, 8), own, r"row 7: scene 0, window \(8, 25\), but its group 2 is scene 0, window \(0, 25\)"),
        (with_row(vr, 2, 2, 26), own, r"row 2: window \(0, 26\) \+ 32 x 32 leaves its 40 x 57 scene"),
        (with_row(vr, 4, 1, -1), own, "row 4: window"),
        (with_row(vr, 3, 0, 2), own, "row 3: scene 2 outside 0..1"),
        (with_row(vr, 5, 3, 8), own, "row 5: code 8 outside 0..7"),
        (with_row(vr, 5, 3, -1), own, "row 5: code -1 outside 0..7"),
        (vr, with_row(own, 3, 1, 33), r"group 3: owned rows \d+\.\.33, columns"),
        (vr, with_row(own, 0, 2, 40), "group 0: owned rows"),
    ]
    for r, o, msg in refused:
        run_stitch(p, r, o, shapes, maps, expect_error=msg)
        with pytest.raises(ValueError, match=msg):                # the host definition refuses the same rows in the same words
            scenes.host_stitch_views(p, r, o, shapes, maps)
    run_stitch(p, vr, own, shapes, maps, C=65, expect_error="C 65 outside 1..64")
    run_stitch(p, vr, own, shapes, maps, K=0, expect_error="K 0 outside 1..8")
    run_stitch(p, vr, own, shapes, maps, K=9, expect_error="K 9 outside 1..8")
    # a transposing code on a 16 x 48 patch
    frows, fown = table_of([(40, 57)], (16, 48), (12, 24))
    fp, fmaps = make_inputs(6, [(40, 57)], len(frows), (0, 3), 16, 48, 5)
    fvr = with_row(scenes.view_rows(frows, (0, 3)), 3, 3, 6)
    msg = r"row 3: code 6 transposes and needs a square patch \(got 16 x 48\)"
    run_stitch(fp, fvr, fown, [(40, 57)], fmaps, expect_error=msg)
    with pytest.raises(ValueError, match=msg):
        scenes.host_stitch_views(fp, fvr, fown, [(40, 57)], fmaps)
    # scene_cls and confusion go together
    dev = torch.device("cuda")
    pd, out = torch.from_numpy(p).to(dev), torch.full((40 * 57,), FILL, dtype=torch.uint8, device=dev)
    one = (ctypes.c_void_p * 1)(out.data_ptr())
    with pytest.raises(L.RuaError, match="scene_cls and confusion go together"):
        L.lib().call("rua_scene_stitch_views", pd.data_ptr(), 6, 3, 32, 32, 5, vr.ctypes.data, own.ctypes.data, one, one,
                     (ctypes.c_int32 * 1)(40), (ctypes.c_int32 * 1)(57), 1, None, None)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == FILL).all()


# ---- engine / model level -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pool():
    return blob_pool((128, 128))


@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("multitask", [True, False])
def test_predict_scene_is_host_stitch_views_of_its_probabilities(pool, multitask, use_graph):
    """The 150 x 171 scene at stride 64 (9 windows) and the 128 x 128 one at stride 24 (16), views flips and all, batch 8 and 5:
    batch 5 with flips gives G = 1 (forwards of 3), with all a forward of 8; 9 windows in groups of 2 leave a padded last batch."""
    eng = new_engine(multitask, use_graph)
    ragged = 0
    for scene, stride in ((0, 64), (1, 24)):
        table = pool.predict_table(scene, stride)
        n = len(table[0])
        for views in ("flips", "all"):
            codes = scenes.VIEW_SETS[views]
            K = len(codes)
            for batch in (8, 5):
                G = max(1, batch // K)
                seen = []
                pred, cm = eng.predict_scene(pool, scene, stride=stride, batch=batch, norm_type=1, views=views,
                                             on_batch=lambda r, o, p: seen.append((r.copy(), o.copy(), p.clone())))
                torch.cuda.synchronize()
                ragged += n % G != 0
                assert len(seen) == -(-n // G)
                assert all(r.shape == (G * K, 4) and o.shape == (G, 4) and tuple(p.shape) == (G * K, 64, 64, NCLS) for r, o, p in seen)
                rows, own = np.concatenate([s[0] for s in seen]), np.concatenate([s[1] for s in seen])
                assert np.array_equal(rows[:n * K], scenes.view_rows(table[0], codes)) and np.array_equal(own[:n], table[1])
                assert (own[n:] == 0).all()                    # the padding owns nothing
                assert np.array_equal(rows[n * K:], np.tile(scenes.view_rows(table[0][-1:], codes), (len(own) - n, 1)))
                probs = np.concatenate([s[2].cpu().numpy() for s in seen])
                assert np.isfinite(probs).all()
                want_maps, want_cm = scenes.host_stitch_views(probs, rows, own, pool.shapes, pool.class_maps, NCLS)
                what = (scene, stride, views, batch)
                assert pred.dtype == np.uint8 and pred.shape == pool.shapes[scene] and np.array_equal(pred, want_maps[scene]), what
                assert cm.dtype == np.int64 and np.array_equal(cm, want_cm), what
                again = np.bincount(pool.class_maps[scene].astype(np.int64).ravel() * NCLS + pred.ravel(), minlength=NCLS * NCLS).reshape(NCLS, NCLS)
                assert np.array_equal(cm, again), what
    assert ragged >= 1                                         # a last batch that had to be padded


def test_views_none_is_the_call_without_views_and_refusals(pool):
    eng = new_engine(False, True)
    calls = []
    plain = eng.predict_scene(pool, 0, stride=24, batch=5, on_batch=lambda r, o, p: calls.append(r.shape))
    for views in ((0,), "none", [0]):
        seen = []
        got = eng.predict_scene(pool, 0, stride=24, batch=5, views=views, on_batch=lambda r, o, p: seen.append(r.shape))
        assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1]) and seen == calls and calls[0] == (5, 4)
    bare = scenes.ScenePool(pool.images, None, patch=64)
    pred, cm = eng.predict_scene(bare, 1, stride=64, batch=8, views="aug5")
    assert cm is None and np.array_equal(pred, eng.predict_scene(pool, 1, stride=64, batch=8, views="aug5")[0])
    with pytest.raises(ValueError, match="code 3 occurs twice"):
        eng.predict_scene(pool, 0, views=(0, 3, 3))
    with pytest.raises(ValueError, match="code 8 outside 0..7"):
        eng.predict_scene(pool, 0, views=(8,))
    with pytest.raises(ValueError, match="not one of"):
        eng.predict_scene(pool, 0, views="every")
    with pytest.raises(ValueError, match="K 0 outside 1..8"):
        eng.predict_scene(pool, 0, views=())
    flat = new_engine(False, False, shape=(32, 64, 3), depth=4)    # a non-square input (four levels: 4 x 8 at the bottom)
    fpool = scenes.ScenePool(pool.images, pool.class_maps, patch=(32, 64))
    with pytest.raises(ValueError, match=r"code 1 transposes and needs a square patch \(got 32 x 64\)"):
        flat.predict_scene(fpool, 1, views="aug5")


@pytest.mark.parametrize("views", ["flips", "all"])
def test_predict_scene_views_against_the_predict_route(pool, views):
    """The 128 x 128 scene at stride 64 (four tiles, owned in full): Model.predict on the view rows, every view turned back with
    INVERSE and summed in view order on the host, its arg-max mosaic against the map.  Two predict calls that agree bitwise demand
    exact equality; otherwise agreement wherever the top-two margin of the summed probabilities exceeds 10 x K x the largest
    difference between the calls (K terms, each off by at most that difference; the single-view test's factor of ten), and that
    must exclude less than 1 % of the pixels."""
    m = new_model()
    codes = scenes.VIEW_SETS[views]
    K = len(codes)
    rows, own = pool.predict_table(1, 64)
    vr = scenes.view_rows(rows, codes)
    a = m.predict(pool.batch(vr), batch_size=8, norm_type=1)["seg"]
    b = m.predict(pool.batch(vr), batch_size=8, norm_type=1)["seg"]
    pred, cm = m.predict_scene(pool, 1, stride=64, batch=8, norm_type=1, views=views)
    assert (own == [0, 64, 0, 64]).all() and cm.sum() == 128 * 128

    def summed(x):
        out = []
        for g in range(len(rows)):
            s = scenes.transform(x[g * K], scenes.INVERSE[codes[0]]).copy()
            for k in range(1, K):
                s = s + scenes.transform(x[g * K + k], scenes.INVERSE[codes[k]])
            out.append(s)
        return np.stack(out)

    def mosaic(tiles):
        out = np.zeros((128, 128), tiles.dtype)
        for t, (_, r, c, _) in zip(tiles, rows.tolist()):
            out[r:r + 64, c:c + 64] = t
        return out
    s = summed(a)
    assert s.dtype == np.float32
    want = mosaic(np.argmax(s, -1))
    if np.array_equal(a, b):
        print("predict is deterministic: exact comparison")
        assert np.array_equal(pred, want)
    else:
        spread = float(np.abs(a - b).max())
        top = np.sort(s, axis=-1)
        sure = mosaic(top[..., -1] - top[..., -2] > 10 * K * spread)
        print(f"predict differs between calls by up to {spread:.3g}: {100 * (1 - sure.mean()):.3f} % of the pixels excluded")
        assert 1 - sure.mean() < 0.01
        assert np.array_equal(pred[sure], want[sure])


def test_cli_scores_a_scene_directory_with_views(tmp_path, capsys):
    """eval_scenes_ISPRS.py --views aug5 --stride 32 on a tiny scene directory: its maps, matrix and metrics against evaluate_scenes."""
    import eval_scenes_ISPRS
    from resunet_a_mltsk_keras_amd.keras_api import load_model
    sc = [blob_scene(300, 90, 70), blob_scene(301, 64, 100)]
    root, path, out = str(tmp_path / "scenes"), str(tmp_path / "m.h5"), str(tmp_path / "preds")
    scenes.save_scene_dir(root, ["a_tile", "b_tile"], [s[0] for s in sc], [s[1] for s in sc])
    new_model(seed=11, depth=4, split_k=True).save(path)         # four levels: a small file; split_k as load_model leaves it
    res = eval_scenes_ISPRS.main(["--use_multitasking", "--model_path", path, "--dataset_path", root, "-ps", "64", "--num_classes", str(NCLS),
                                  "--output_path", out, "--views", "aug5", "--stride", "32", "--batch_size", "8"])
    assert "views: 0 1 2 3 4 (5 per window)" in capsys.readouterr().out
    names, images, class_maps = scenes.load_scene_dir(root)
    model = load_model(path, compile=False)
    maps, cm = model.evaluate_scenes(scenes.ScenePool(images, class_maps, patch=64), stride=32, batch_size=8, norm_type=1, views="aug5")
    assert cm.sum() == 90 * 70 + 64 * 100 and np.array_equal(res["confusion_matrix"], cm)
    per_scene = 0
    for name, want in zip(names, maps):
        got = np.load(os.path.join(out, f"pred_seg_reconstructed_{name}.npy"))
        assert got.dtype == np.uint8 and np.array_equal(got, want)
        per_scene = per_scene + np.load(os.path.join(out, f"confusion_matrix_{name}.npy"))
        assert os.path.getsize(os.path.join(out, f"pred_seg_reconstructed_{name}.ppm")) > 3 * want.size
    assert np.array_equal(per_scene, cm)
    acc, f1, rec, prec = eval_scenes_ISPRS.metrics_from_confusion(cm)
    assert res["accuracy"] == acc and np.array_equal(res["f1"], f1) and np.array_equal(res["recall"], rec) and np.array_equal(res["precision"], prec)
    assert eval_scenes_ISPRS.parse_views(["0", "3", "4"]) == (0, 3, 4) and eval_scenes_ISPRS.parse_views(["0,3,4"]) == (0, 3, 4)
    assert eval_scenes_ISPRS.parse_views(["all"]) == scenes.VIEW_SETS["all"]
    with pytest.raises(SystemExit):
        eval_scenes_ISPRS.parse_views(["0", "0"])
    with pytest.raises(SystemExit):
        eval_scenes_ISPRS.parse_views(["most"])
