"""GPU tests of the whole-scene head maps: rua_scene_stitch_maps (csrc/scene.hip) byte for byte against scenes.host_stitch_maps through
the C ABI - any head's window outputs under K views turned back, quantised to Q16, averaged in integers and written as uint8 maps of
Ch interleaved channels, plain and as the colour head's RGB picture -, its argument checks, Engine.predict_scene(heads=) against
host_stitch_maps of the tensors it stitched, and eval_scenes_ISPRS.py --head_maps against Model.evaluate_scenes(heads=)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from resunet_a_mltsk_keras_amd import _lib as L
from resunet_a_mltsk_keras_amd import scenes

from _scene_util import FILL, NCLS, blob_pool, blob_scene, guarded_maps, new_engine, new_model, read_guarded, table_of

pytestmark = pytest.mark.gpu

ALL_MAPS = ("seg", "bound", "dist", "color", "color_rgb")
f32 = np.float32
# quantise_q16's hard values: the clamps, NaN and the infinities, a subnormal, and exact halves (n + 0.5) / 65536 for even and odd n
SPECIAL = np.array([0.0, 1.0, 1.5, -0.25, np.nan, np.inf, -np.inf, 2.0 ** -140]
                   + [(n + 0.5) / 65536 for n in (0, 1, 2, 3, 128, 129, 32767, 32768, 65534, 65535)], f32)


def make_inputs(seed, G, codes, PH, PW, Ch, mode="plain"):
    """p [G*K][PH][PW][Ch].  The un-transformed stack q [G][K][PH][PW][Ch] comes first, p[g*K + k] = transform(q[g, k], code_k).
    q: uniform in [-0.1, 1.1).  About 5 % of the pixels hold values of SPECIAL, drawn per element.  About 5 % hold 0.5 in every
    view and channel: A = K * 32768, so 255 A + K 32768 = 128 * K * 65536 exactly, the tie of the final rounding.  For odd K > 1
    about 5 % hold 0.5 in view 0 and 0 elsewhere: 255 * 32768 + K * 32768 = (255 + K) / (2 K) * K * 65536, a whole multiple for
    K = 3 and 5.  Mode hsv_rgb: about 5 % hold the hue wrap, H alternating 0.005 / 0.995 over the views at S = V = 1, and about
    5 % have S or V exactly 0."""
    rng = np.random.default_rng(seed)
    K = len(codes)
    q = rng.random((G, K, PH, PW, Ch), dtype=f32) * f32(1.2) - f32(0.1)

    def some():
        at = np.argwhere(rng.random((G, PH, PW)) < 0.05)
        return at[:, 0], at[:, 1], at[:, 2]
    g, i, j = some()
    q[g, :, i, j, :] = SPECIAL[rng.integers(0, len(SPECIAL), (len(g), K, Ch))]
    g, i, j = some()
    q[g, :, i, j, :] = 0.5
    if K > 1 and K % 2:
        g, i, j = some()
        q[g, :, i, j, :] = 0.0
        q[g, 0, i, j, :] = 0.5
    if mode == "hsv_rgb":
        g, i, j = some()
        q[g, :, i, j, :] = 1.0
        q[g, :, i, j, 0] = np.where(np.arange(K) % 2 == 0, f32(0.005), f32(0.995))[None, :]
        g, i, j = some()
        ch = 1 + rng.integers(0, 2, len(g))
        for k in range(K):
            q[g, k, i, j, ch] = 0.0
    p = np.stack([scenes.transform(q[g, k], c) for g in range(G) for k, c in enumerate(codes)])
    return np.ascontiguousarray(p)


def test_the_planted_ties_are_exact_multiples():
    """The generator's planted pixels on the host: the numerator of the final division is a whole multiple of its denominator."""
    for K in (1, 3, 5, 8):
        a = scenes.quantise_q16(np.full(K, 0.5, f32)).sum()
        assert (255 * a + K * 32768) % (K * 65536) == 0
    for K in (3, 5):
        assert (255 * 32768 + K * 32768) % (K * 65536) == 0
    with np.errstate(invalid="ignore"):
        assert scenes.quantise_q16(SPECIAL).tolist() == [0, 65536, 65536, 0, 0, 65536, 0, 0, 0, 2, 2, 4, 128, 130, 32768, 32768, 65534, 65536]


def run_maps(p, rows, own, shapes, K=None, Ch=None, mode=0, expect_error=None, p_offset=0, null_scene=None, sizes=None, patch=None):
    """rua_scene_stitch_maps into 0xEE-filled maps with a guard region behind each; returns the maps [H][W][Ch] and checks the guards.
    expect_error: the call must fail with this text and leave every byte as it was.  The other keywords bend one argument each."""
    dev = torch.device("cuda")
    N, PH, PW, Cp = p.shape
    Ch = Cp if Ch is None else Ch
    PH, PW = (PH, PW) if patch is None else patch
    n = len(shapes)
    pd = torch.from_numpy(np.ascontiguousarray(p)).to(dev)
    out = guarded_maps(shapes, Cp)
    ptrs = (ctypes.c_void_p * n)(*[None if s == null_scene else t.data_ptr() for s, t in enumerate(out)])
    hw = shapes if sizes is None else sizes
    hs, ws = (ctypes.c_int32 * n)(*[h for h, _ in hw]), (ctypes.c_int32 * n)(*[w for _, w in hw])
    r, o = np.ascontiguousarray(rows, dtype=np.int32), np.ascontiguousarray(own, dtype=np.int32)
    K = len(r) // len(o) if K is None else K
    args = (pd.data_ptr() + p_offset, len(o), K, PH, PW, Ch, r.ctypes.data, o.ctypes.data, ptrs, hs, ws, n, mode,
            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    if expect_error is not None:
        with pytest.raises(L.RuaError, match=expect_error):
            L.lib().call("rua_scene_stitch_maps", *args)
    else:
        L.lib().call("rua_scene_stitch_maps", *args)
    torch.cuda.synchronize()
    maps = read_guarded(out, shapes, Cp)
    if expect_error is not None:
        assert all((m == FILL).all() for m in maps), "a refused call wrote something"
    return maps


def assert_maps(p, rows, own, shapes, mode="plain"):
    K = len(rows) // len(own)
    got = run_maps(p, rows, own, shapes, mode=scenes.MAP_MODES[mode])
    with np.errstate(invalid="ignore"):
        want = scenes.host_stitch_maps(p, rows, own, shapes, K, mode=mode, maps=[np.full((H, W, p.shape[3]), FILL, np.uint8) for H, W in shapes])
    for s, (g, w) in enumerate(zip(got, want)):
        bad = np.argwhere(g != w)
        assert bad.size == 0, (f"scene {s}", len(bad), "first at", tuple(bad[0]), int(g[tuple(bad[0])]), int(w[tuple(bad[0])]))
    return want


def owned_mask(rows, own, shapes, K):
    masks = [np.zeros(s, bool) for s in shapes]
    for (s, r, c, _), (r0, r1, c0, c1) in zip(rows[::K].tolist(), own.tolist()):
        masks[s][r + r0:r + r1, c + c0:c + c1] = True
    return masks


def bitwise_case(seed, shapes, patch, stride, views, Ch, mode="plain"):
    """The whole table (every pixel written), then every other group dropped (the bytes between the rectangles stay 0xEE)."""
    codes = scenes.check_views(views, patch)
    K = len(codes)
    rows, own = table_of(shapes, patch, stride)
    G = len(rows)
    p = make_inputs(seed, G, codes, patch[0], patch[1], Ch, mode)
    vr = scenes.view_rows(rows, codes)
    want = assert_maps(p, vr, own, shapes, mode)
    assert all(len(np.unique(m)) > 100 for m in want)          # not a constant picture
    keep = np.arange(0, G, 2)
    pk = p.reshape(G, K, *p.shape[1:])[keep].reshape(-1, *p.shape[1:])
    rk = scenes.view_rows(rows[keep], codes)
    half = assert_maps(pk, rk, own[keep], shapes, mode)
    for m, inside in zip(half, owned_mask(rk, own[keep], shapes, K)):
        assert (m[~inside] == FILL).all()
    assert any((~inside).any() for inside in owned_mask(rk, own[keep], shapes, K))


# (45, 61): odd sizes, the last windows flush with the border.  Ch = 5: a scene row is 305 bytes, so tile rows start at every byte
# phase and view rows at every dword phase of a 16-byte piece.  Ch = 3, 5, 6, 64 give tiles of 32, 28, 24 and 8 pixels: one tile per
# 32 x 32 window, ragged tiles, and 16 tiles a window.
@pytest.mark.parametrize("Ch", [3, 5, 6, 64])
@pytest.mark.parametrize("views", ["none", "flips", "aug5", "all", (5, 7)])
def test_stitch_maps_bitwise(views, Ch):
    bitwise_case(Ch * 100 + len(scenes.check_views(views)), [(45, 61), (32, 32)], (32, 32), 24, views, Ch)


@pytest.mark.parametrize("Ch", [3, 5, 6, 64])
def test_stitch_maps_bitwise_flat_patch(Ch):
    """A 16 x 48 patch takes the four codes that do not transpose."""
    bitwise_case(Ch * 100 + 16, [(45, 61)], (16, 48), (12, 24), (0, 2, 3, 4), Ch)


@pytest.mark.parametrize("Ch,mode", [(5, "plain"), (6, "plain"), (3, "hsv_rgb")])
def test_stitch_maps_bitwise_odd_patch(Ch, mode):
    """Patch 37 (tiles of 28, 24 and 32): the odd edge crosses tile borders under all eight symmetries."""
    bitwise_case(37 + Ch, [(45, 61)], (37, 37), 20, "all", Ch, mode)


@pytest.mark.parametrize("K", [1, 3, 8])
def test_stitch_maps_hsv_rgb(K):
    """Mode 1 against the host: the hue wrap and S or V of exactly 0 among the planted pixels."""
    views = {1: "none", 3: "flips", 8: "all"}[K]
    shapes = [(45, 61), (32, 32)]
    bitwise_case(K, shapes, (32, 32), 24, views, 3, "hsv_rgb")
    # a window of nothing but the wrap: red, not cyan
    rows = scenes.view_rows(np.array([[0, 3, 5, 0]], np.int32), views)
    p = np.ones((K, 32, 32, 3), f32)
    p[:, :, :, 0] = np.where(np.arange(K) % 2 == 0, f32(0.005), f32(0.995))[:, None, None]
    got = run_maps(p, rows, np.array([[0, 32, 0, 32]], np.int32), [(45, 61)], mode=1)[0][3:35, 5:37]
    assert (got[..., 0] >= 250).all() and (got[..., 1:] <= 16).all()


def test_stitch_maps_more_groups_than_one_launch():
    """150 groups of K = 2 (a launch carries 120): stride 1 on three small scenes, the first 150 rows of 361."""
    shapes = [(40, 57), (32, 32), (45, 40)]
    rows, own = table_of(shapes, (32, 32), 1)
    assert len(rows) > 150
    rows, own = rows[:150], own[:150]
    p = make_inputs(2, 150, (6, 2), 32, 32, 5)
    assert_maps(p, scenes.view_rows(rows, (6, 2)), own, shapes)


@pytest.mark.parametrize("views", [(3, 6, 0), (0,), (7,)])
def test_stitch_maps_one_group(views):
    """G = 1, and a p of K * 31 * 31 * 5 floats - no whole number of 16-byte pieces - owned up to the window's last pixel."""
    p = make_inputs(1, 1, views, 31, 31, 5)
    assert p.size % 4
    rows = scenes.view_rows(np.array([[0, 1, 14, 0]], np.int32), views)
    assert_maps(p, rows, np.array([[3, 31, 1, 31]], np.int32), [(33, 47)])
    assert_maps(p, rows, np.array([[0, 31, 0, 31]], np.int32), [(33, 47)])


def test_stitch_maps_empty_rectangles():
    shapes = [(45, 61), (32, 32)]
    rows, own = table_of(shapes, (32, 32), 24)
    own = own.copy()
    own[3, 1] = own[3, 0]                                      # no rows
    own[5, 3] = own[5, 2]                                      # no columns
    own[len(own) - 1] = 0                                      # the padding group of a last batch
    p = make_inputs(4, len(rows), (0, 3, 4), 32, 32, 5)
    want = assert_maps(p, scenes.view_rows(rows, "flips"), own, shapes)
    assert (want[0] == FILL).any() and (want[1] == FILL).all()


@pytest.mark.parametrize("Ch", [1, 3, 5, 6])
def test_stitch_maps_narrow_rectangles(Ch):
    """Rectangles 1 and 2 pixels wide at odd columns (and one a single pixel): Ch to 2 Ch bytes of a row whose neighbours in the same
    dword are not ours.  A dword store that spills shows in the 0xEE bytes around them."""
    shapes = [(45, 61)]
    rows = np.array([[0, 0, 0, 0], [0, 13, 29, 0], [0, 2, 7, 0], [0, 5, 11, 0]], np.int32)
    own = np.array([[1, 30, 7, 8], [0, 32, 13, 15], [31, 32, 31, 32], [3, 4, 1, 3]], np.int32)
    for views in ((0,), (4, 6, 1)):
        p = make_inputs(Ch, len(rows), views, 32, 32, Ch)
        want = assert_maps(p, scenes.view_rows(rows, views), own, shapes)
        assert (want[0] != FILL).any(2).sum() <= 29 + 64 + 1 + 2


def test_stitch_maps_refuses_bad_arguments():
    shapes = [(40, 57), (32, 32)]
    rows, own = table_of(shapes, (32, 32), 24)
    codes = (0, 1, 4)
    p = make_inputs(5, len(rows), codes, 32, 32, 3)
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
        run_maps(p, r, o, shapes, expect_error="rua_scene_stitch_maps: " + msg)
        with pytest.raises(ValueError, match=msg):                # the host definition refuses the same rows in the same words
            scenes.host_stitch_maps(p, r, o, shapes, 3)
    run_maps(p, vr, own, shapes, K=0, expect_error="K 0 outside 1..8")
    run_maps(p, vr, own, shapes, K=9, expect_error="K 9 outside 1..8")
    run_maps(p, vr, own, shapes, Ch=0, expect_error="Ch 0 outside 1..64")
    run_maps(p, vr, own, shapes, Ch=65, expect_error="Ch 65 outside 1..64")
    run_maps(p, vr, own, shapes, mode=2, expect_error=r"mode 2 \(0 plain, 1 hsv_rgb\)")
    run_maps(p, vr, own, shapes, mode=-1, expect_error="mode -1")
    run_maps(p, vr, own, shapes, Ch=5, mode=1, expect_error="mode 1 .hsv_rgb. reads H, S, V: Ch 3, got 5")
    run_maps(p, vr, own, shapes, patch=(513, 32), expect_error=r"PH 513, PW 32 \(1 <= PH, PW <= 512\)")
    run_maps(p, vr, own, shapes, patch=(32, 0), expect_error="PH 32, PW 0")
    run_maps(p, vr, own, shapes, p_offset=4, expect_error="p must be 16-byte aligned")
    run_maps(p, vr, own, shapes, null_scene=1, expect_error="scene 1: null pointer")
    run_maps(p, vr, own, shapes, sizes=[(40, 57), (1 << 20, 1 << 19)], expect_error="scene 1: size 1048576 x 524288 x 3")   # 2^39 * 3 bytes
    run_maps(p, vr, own, shapes, sizes=[(0, 57), (32, 32)], expect_error="scene 0: size 0 x 57")
    # a transposing code on a 16 x 48 patch
    frows, fown = table_of([(40, 57)], (16, 48), (12, 24))
    fp = make_inputs(6, len(frows), (0, 3), 16, 48, 5)
    fvr = with_row(scenes.view_rows(frows, (0, 3)), 3, 3, 6)
    run_maps(fp, fvr, fown, [(40, 57)], expect_error=r"row 3: code 6 transposes and needs a square patch \(got 16 x 48\)")
    # required pointers
    with pytest.raises(L.RuaError, match="scene_out, scene_h and scene_w are required"):
        L.lib().call("rua_scene_stitch_maps", None, 1, 1, 32, 32, 3, vr.ctypes.data, own.ctypes.data, None, None, None, 1, 0, None)


# ---- engine / model level -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pool():
    return blob_pool((128, 128))


@pytest.mark.parametrize("use_graph", [True, False])
def test_predict_scene_heads_are_host_stitch_maps_of_their_tensors(pool, use_graph):
    """The 150 x 171 scene at stride 64 (9 windows), views none and aug5, batch 8 and 5 (none: a padded last batch; aug5: forwards of
    one group of 5): every head's map against host_stitch_maps of the very tensors on_heads saw, and the class map and confusion
    matrix of the same call against those of heads=()."""
    eng = new_engine(True, use_graph)
    table = pool.predict_table(0, 64)
    n = len(table[0])
    padded = 0
    for views in ("none", "aug5"):
        codes = scenes.VIEW_SETS[views]
        K = len(codes)
        for batch in (8, 5):
            G = max(1, batch // K) if K > 1 else batch
            seen, plain = [], []
            pred, cm, maps = eng.predict_scene(pool, 0, stride=64, batch=batch, norm_type=1, views=views, heads=ALL_MAPS,
                                               on_batch=lambda r, o, p: plain.append(tuple(p.shape)),
                                               on_heads=lambda r, o, t: seen.append((r.copy(), o.copy(), {h: v.clone() for h, v in t.items()})))
            torch.cuda.synchronize()
            what = (views, batch)
            assert len(seen) == -(-n // G) == len(plain), what
            padded += n % G != 0
            assert tuple(maps) == ALL_MAPS
            rows, own = np.concatenate([s[0] for s in seen]), np.concatenate([s[1] for s in seen])
            assert np.array_equal(rows[:n * K], scenes.view_rows(table[0], codes)) and np.array_equal(own[:n], table[1]) and (own[n:] == 0).all()
            for h in ALL_MAPS:
                ch = 3 if h.startswith("color") else NCLS
                assert all(tuple(s[2][h].shape) == (G * K, 64, 64, ch) for s in seen), (what, h)
                t = np.concatenate([s[2][h].cpu().numpy() for s in seen])
                assert t.dtype == np.float32 and np.isfinite(t).all()
                want = scenes.host_stitch_maps(t, rows, own, pool.shapes, K, mode="hsv_rgb" if h == "color_rgb" else "plain")[0]
                got = maps[h]
                assert got.dtype == np.uint8 and got.shape == (150, 171, ch), (what, h)
                assert np.array_equal(got, want), (what, h, int((got != want).sum()))
                assert len(np.unique(got)) > 1, (what, h)         # a picture, not a constant
            assert all(np.array_equal(s[2]["color"].cpu().numpy(), s[2]["color_rgb"].cpu().numpy()) for s in seen)
            # the seg map's arg-max is the class map wherever the quantised maximum is unique (one view: the same probabilities)
            if K == 1:
                top = np.sort(maps["seg"].astype(int), -1)
                sure = top[..., -1] - top[..., -2] >= 2
                print(f"{100 * sure.mean():.1f} % of the pixels have a unique quantised maximum")
                assert np.array_equal(np.argmax(maps["seg"], -1)[sure], pred[sure])
            bare = eng.predict_scene(pool, 0, stride=64, batch=batch, norm_type=1, views=views)
            assert len(bare) == 2 and np.array_equal(bare[0], pred) and np.array_equal(bare[1], cm), what
    assert padded >= 1
    # erode keeps its place, the maps come last; a subset in the caller's order
    pred, cm, cm_e, maps = eng.predict_scene(pool, 1, stride=64, batch=4, erode=2, heads=("dist", "seg"))
    assert tuple(maps) == ("dist", "seg") and cm_e.shape == (NCLS, NCLS) and maps["dist"].shape == (128, 128, NCLS)
    assert np.array_equal(maps["seg"], eng.predict_scene(pool, 1, stride=64, batch=4, heads="seg")[2]["seg"])


def test_predict_scene_heads_refusals(pool):
    single = new_engine(False, False)
    with pytest.raises(ValueError, match="this model has no 'bound' head"):
        single.predict_scene(pool, 1, heads=("bound",))
    with pytest.raises(ValueError, match="this model has no 'color_rgb' head"):
        single.predict_scene(pool, 1, heads=("seg", "color_rgb"))
    pred, cm, maps = single.predict_scene(pool, 1, stride=64, heads=("seg",))
    assert tuple(maps) == ("seg",) and maps["seg"].shape == (128, 128, NCLS)
    multi = new_engine(True, False)
    with pytest.raises(ValueError, match="'color_rgb' needs norm_type 1"):
        multi.predict_scene(pool, 1, norm_type=2, heads=("color_rgb",))
    with pytest.raises(ValueError, match="'depth' is not one of"):
        multi.predict_scene(pool, 1, heads=("seg", "depth"))
    with pytest.raises(ValueError, match="'seg' occurs twice"):
        multi.predict_scene(pool, 1, heads=("seg", "seg"))
    assert set(multi.predict_scene(pool, 1, stride=64, norm_type=2, heads=("color",))[2]) == {"color"}


def test_cli_writes_head_maps(tmp_path, capsys):
    """eval_scenes_ISPRS.py --head_maps seg color_rgb --views flips on a tiny scene directory against Model.evaluate_scenes(heads=)."""
    import eval_scenes_ISPRS
    from resunet_a_mltsk_keras_amd.keras_api import load_model
    sc = [blob_scene(300, 90, 70), blob_scene(301, 64, 100)]
    root, path, out = str(tmp_path / "scenes"), str(tmp_path / "m.h5"), str(tmp_path / "preds")
    scenes.save_scene_dir(root, ["a_tile", "b_tile"], [s[0] for s in sc], [s[1] for s in sc])
    new_model(seed=11, depth=4, split_k=True).save(path)         # four levels: a small file; split_k as load_model leaves it
    common = ["--use_multitasking", "--model_path", path, "--dataset_path", root, "-ps", "64", "--num_classes", str(NCLS),
              "--output_path", out, "--views", "flips", "--stride", "32", "--batch_size", "8"]
    res = eval_scenes_ISPRS.main(common + ["--head_maps", "seg", "color_rgb"])
    printed = capsys.readouterr().out
    names, images, class_maps = scenes.load_scene_dir(root)
    model = load_model(path, compile=False)
    maps, cm, head_maps = model.evaluate_scenes(scenes.ScenePool(images, class_maps, patch=64), stride=32, batch_size=8, norm_type=1,
                                                views="flips", heads=("seg", "color_rgb"))
    assert np.array_equal(res["confusion_matrix"], cm) and len(head_maps) == 2 == len(res["head_maps"])
    diff_sum, diff_n = 0, 0
    for name, img, want_map, want in zip(names, images, maps, head_maps):
        assert np.array_equal(np.load(os.path.join(out, f"pred_seg_reconstructed_{name}.npy")), want_map)
        for h, ch in (("seg", NCLS), ("color_rgb", 3)):
            got = np.load(os.path.join(out, f"pred_{h}_{name}.npy"))
            assert got.dtype == np.uint8 and got.shape == img.shape[:2] + (ch,) and np.array_equal(got, want[h])
        with open(os.path.join(out, f"pred_color_rgb_{name}.ppm"), "rb") as f:
            raw = f.read()
        assert raw.startswith(f"P6\n{img.shape[1]} {img.shape[0]}\n255\n".encode()) and raw.endswith(want["color_rgb"].tobytes())
        d = np.abs(want["color_rgb"].astype(np.int64) - img.astype(np.int64))
        diff_sum, diff_n = diff_sum + int(d.sum()), diff_n + d.size
        assert f"scene {name}: colour reconstruction, mean absolute difference from the image {d.mean():.4f}" in printed
    assert res["color_mae"] == pytest.approx(diff_sum / diff_n, rel=1e-12)
    assert all(np.array_equal(a[h], b[h]) for a, b in zip(res["head_maps"], head_maps) for h in ("seg", "color_rgb"))
    # without the flag: today's keys and files
    out2 = str(tmp_path / "preds2")
    assert common[10] == out
    res2 = eval_scenes_ISPRS.main(common[:10] + [out2] + common[11:])
    assert "head_maps" not in res2 and "color_mae" not in res2 and np.array_equal(res2["confusion_matrix"], cm)
    extra = {f"pred_{h}_{name}.{ext}" for h, ext in (("seg", "npy"), ("color_rgb", "npy"), ("color_rgb", "ppm")) for name in names}
    assert set(os.listdir(out)) - set(os.listdir(out2)) == extra and set(os.listdir(out2)) <= set(os.listdir(out))
    with pytest.raises(SystemExit, match="distinct names out of"):
        eval_scenes_ISPRS.main(common + ["--head_maps", "seg", "hue"])
    with pytest.raises(SystemExit, match="needs --norm_type 1"):
        eval_scenes_ISPRS.main(common + ["--head_maps", "color_rgb", "--norm_type", "2"])
