"""Host definitions of multi-scale test-time augmentation (scenes.py): scale_footprint, scale_table - one pass' affine rows and owned
rectangles -, host_accumulate - the numpy definition of rua_scene_accumulate, windows resampled back onto the scene grid and summed
in integers - and host_argmax, rua_scene_argmax's; check_scales and the --scales flag of eval_scenes_ISPRS.py.  No GPU."""
import numpy as np
import pytest

from resunet_a_mltsk_keras_amd import scenes

SCENE, P, STRIDE = (53, 61), (8, 8), 6
FOOTPRINTS = [(5, 5), (8, 8), (13, 13), (32, 32)]
ALL = scenes.VIEW_SETS["all"]
FLAT = (0, 2, 3, 4)                                            # the codes that do not transpose
f32 = np.float32


def test_scale_footprint():
    assert scenes.scale_footprint(8, 1.0) == (8, 8) and scenes.scale_footprint((8, 8), 1) == (8, 8)
    assert scenes.scale_footprint(256, 0.75) == (341, 341) and scenes.scale_footprint(256, 1.5) == (171, 171)
    assert scenes.scale_footprint((4, 12), 2.0) == (2, 6) and scenes.scale_footprint(8, 0.25) == (32, 32) and scenes.scale_footprint(8, 4) == (2, 2)
    assert scenes.scale_footprint(3, 2.0) == (2, 2)              # floor(1.5 + 0.5)
    for zoom, msg in ((0.2, "F <= 4 P"), (6.0, "P <= 4 F"), (0, "positive"), (-1.0, "positive"), (float("nan"), "positive"),
                      (float("inf"), "positive"), ("2", "positive"), (True, "positive")):
        with pytest.raises(ValueError, match=msg):
            scenes.scale_footprint(8, zoom)
    with pytest.raises(ValueError, match="columns: zoom 4.5 gives a footprint of 1 for a patch of 6"):
        scenes.scale_footprint((4, 6), 4.5)


@pytest.mark.parametrize("F", FOOTPRINTS)
@pytest.mark.parametrize("views", [(0,), ALL])
def test_scale_table_owns_every_pixel_once_inside_the_footprints(F, views):
    rows7, own = scenes.scale_table(SCENE, P, F, STRIDE, views)
    K = len(views)
    assert rows7.dtype == np.int32 and own.dtype == np.int32 and rows7.shape == (len(own) * K, 7) and own.shape[1] == 4
    SF = min(max((2 * STRIDE * F[0] + 8) // 16, 1), F[0])
    cover, cown = scenes.predict_table(SCENE, F, SF)
    assert len(cover) == len(own)
    assert np.array_equal(own, cown + cover[:, [1, 1, 2, 2]])     # absolute scene coordinates
    owned = np.zeros(SCENE, np.int64)
    for r0, r1, c0, c1 in own.tolist():
        owned[r0:r1, c0:c1] += 1
    assert (owned == 1).all()
    assert np.array_equal(scenes.check_affine_table([SCENE], rows7, P, 3), rows7)
    t, o = scenes.check_accumulate([SCENE], rows7, own, K, P, 3)   # every rectangle inside every view's footprint
    assert np.array_equal(t, rows7) and np.array_equal(o, own)
    a = (2 * 65536 * F[0] + 8) // 16
    for g in range(len(own)):
        for k, c in enumerate(views):
            row = rows7[g * K + k]
            assert np.array_equal(row[3:].reshape(2, 2), a * scenes.SYMMETRY[c])
            A = row[3:].reshape(2, 2).astype(np.int64)
            assert row[1] == (2 * cover[g, 1] + F[0] - 1) * 32768 - ((A[0, 0] * 7 + A[0, 1] * 7) >> 1)
            assert row[2] == (2 * cover[g, 2] + F[1] - 1) * 32768 - ((A[1, 0] * 7 + A[1, 1] * 7) >> 1)


def test_scale_table_at_the_patch_cuts_the_cover():
    """F == P, code 0: host_windows_affine of the rows is host_windows of predict_table's cover, and the rows are affine_rows'."""
    rng = np.random.default_rng(0)
    img, cls = rng.integers(0, 256, SCENE + (3,)).astype(np.uint8), rng.integers(0, 5, SCENE).astype(np.uint8)
    rows7, own = scenes.scale_table(SCENE, P, P, STRIDE)
    cover, _ = scenes.predict_table(SCENE, P, STRIDE)
    assert np.array_equal(rows7, scenes.affine_rows(cover, P))
    got, want = scenes.host_windows_affine([img], [cls], rows7, P), scenes.host_windows([img], [cls], cover, P)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    allrows, _ = scenes.scale_table(SCENE, P, P, STRIDE, ALL)
    assert np.array_equal(allrows, scenes.affine_rows(scenes.view_rows(cover, ALL), P))


def test_scale_table_refusals():
    with pytest.raises(ValueError, match="predict_table: rows: stride 45, patch 60, scene 53"):
        scenes.scale_table(SCENE, (16, 16), (60, 60), 12)
    with pytest.raises(ValueError, match="scale_table: columns: footprint 1, patch 8"):
        scenes.scale_table(SCENE, P, (8, 1), 6)
    with pytest.raises(ValueError, match="scale_table: rows: stride 9, patch 8"):
        scenes.scale_table(SCENE, P, P, 9)
    with pytest.raises(ValueError, match="stride 2.0 must be an integer"):
        scenes.scale_table(SCENE, P, P, 2.0)
    with pytest.raises(ValueError, match=r"code 1 transposes and needs a square patch \(got 4 x 12\)"):
        scenes.scale_table(SCENE, (4, 12), (4, 12), 4, (0, 1))
    rows7, own = scenes.scale_table(SCENE, (4, 12), (3, 9), (2, 7), FLAT)       # a stride pair
    assert len(rows7) == 4 * len(own)


@pytest.mark.parametrize("patch,views", [(P, (0,)), (P, ALL), ((4, 12), (0,)), ((4, 12), FLAT)])
def test_a_constant_comes_back_exactly(patch, views):
    """A constant probability accumulates to exactly K * quantise_q16(c) everywhere: the bilinear weights sum to 65536."""
    K = len(views)
    for F in FOOTPRINTS if patch == P else [(3, 9), (4, 12), (7, 20), (16, 48)]:
        rows7, own = scenes.scale_table(SCENE, patch, F, (3, 6) if patch != P else STRIDE, views)
        for c in (f32(0.3), f32(1.0), f32(2.0 ** -17), f32(0.99999)):
            p = np.full((len(rows7),) + patch + (2,), c, f32)
            acc = scenes.host_accumulate(p, rows7, own, [SCENE], K)[0]
            assert acc.dtype == np.int32 and acc.shape == SCENE + (2,)
            assert (acc == K * int(scenes.quantise_q16(c))).all(), (F, float(c))


def test_at_the_patch_the_way_back_is_placement():
    """F == P: code 0 gives quantise_q16(p) placed by ownership; K views give the integer sum of the turned-back quantised views -
    host_stitch_views' geometry (transform, INVERSE), written out here without the new code."""
    rng = np.random.default_rng(1)
    cover, cown = scenes.predict_table(SCENE, P, STRIDE)
    for views in ((0,), ALL, (5, 3)):
        K = len(views)
        rows7, own = scenes.scale_table(SCENE, P, P, STRIDE, views)
        p = rng.random((len(rows7), 8, 8, 3), dtype=f32)
        want = np.zeros(SCENE + (3,), np.int64)
        for g, ((_, r, c, _), (r0, r1, c0, c1)) in enumerate(zip(cover.tolist(), cown.tolist())):
            for k, code in enumerate(views):
                want[r + r0:r + r1, c + c0:c + c1] += scenes.quantise_q16(scenes.transform(p[g * K + k], scenes.INVERSE[code]))[r0:r1, c0:c1]
        got = scenes.host_accumulate(p, rows7, own, [SCENE], K)[0]
        assert np.array_equal(got, want), views


def test_accumulate_adds_in_place_and_skips_empty_rectangles():
    rng = np.random.default_rng(2)
    shapes = [SCENE, (19, 23)]
    r0_, o0_ = scenes.scale_table(shapes[0], P, (13, 13), STRIDE, (0, 3))
    r1_, o1_ = scenes.scale_table(shapes[1], P, (5, 5), STRIDE, (0, 3))
    r1_[:, 0] = 1
    rows7, own = np.concatenate([r0_, r1_]), np.concatenate([o0_, o1_])
    p = rng.random((len(rows7), 8, 8, 3), dtype=f32)
    fresh = scenes.host_accumulate(p, rows7, own, shapes, 2)
    given = [rng.integers(-1000, 1000, s + (3,)).astype(np.int32) for s in shapes]
    before = [g.copy() for g in given]
    out = scenes.host_accumulate(p, rows7, own, shapes, 2, acc=given)
    assert all(o is g for o, g in zip(out, given))
    assert all(np.array_equal(g, b + f) for g, b, f in zip(given, before, fresh))
    own2 = own.copy()
    own2[1, 1] = own2[1, 0]
    own2[2, 3] = own2[2, 2]
    own2[len(o0_):] = 0
    part = scenes.host_accumulate(p, rows7, own2, shapes, 2)
    assert (part[1] == 0).all()
    for g in (1, 2):
        a, b, c, d = own[g]
        assert (part[0][a:b, c:d] == 0).all() and (fresh[0][a:b, c:d] > 0).any()
    a, b, c, d = own[0]
    assert np.array_equal(part[0][a:b, c:d], fresh[0][a:b, c:d])
    # views and groups in another order: the same sums
    perm = np.arange(len(own))[::-1]
    pr = rows7.reshape(len(own), 2, 7)[perm][:, ::-1].reshape(-1, 7)
    pp = p.reshape(len(own), 2, 8, 8, 3)[perm][:, ::-1].reshape(-1, 8, 8, 3)
    again = scenes.host_accumulate(pp, pr, own[perm], shapes, 2)
    assert all(np.array_equal(a_, f) for a_, f in zip(again, fresh))


def blocky(seed=5):
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 4, (SCENE[0] // 9 + 1, SCENE[1] // 9 + 1))
    return np.kron(f, np.ones((9, 9), np.int64))[:SCENE[0], :SCENE[1]].astype(np.uint8)


def test_geometry_through_the_cutting_kernel_definition():
    """Independent of the resampling code: p is the one-hot of the class window host_windows_affine cuts for each row (the nearest
    pixel), 36 passes - four footprints, each under every single code and under all eight at once - are accumulated, and host_argmax
    gives the class map back wherever no other class lies within a Chebyshev distance of 1.  A mirrored or shifted inverse fails."""
    cls = blocky()
    img = np.zeros(SCENE + (1,), np.uint8)
    acc, passes = None, 0
    for F in FOOTPRINTS:
        for views in [(c,) for c in ALL] + [ALL]:
            rows7, own = scenes.scale_table(SCENE, P, F, STRIDE, views)
            win = scenes.host_windows_affine([img], [cls], rows7, P)[1]
            p = (win[..., None] == np.arange(4)).astype(f32)
            acc = scenes.host_accumulate(p, rows7, own, [SCENE], len(views), acc=acc)
            passes += 1
    assert passes == 36
    pred, cm = scenes.host_argmax(acc, [cls], 4)
    pad = np.pad(cls, 1, mode="edge")
    inner = np.ones(SCENE, bool)
    for dy in range(3):
        for dx in range(3):
            inner &= pad[dy:dy + SCENE[0], dx:dx + SCENE[1]] == cls
    assert 1000 < inner.sum() < cls.size
    assert np.array_equal(pred[0][inner], cls[inner])
    print("disagreements outside the condition:", int((pred[0] != cls).sum()), "of", cls.size)
    assert cm.sum() == cls.size and np.trace(cm) == (pred[0] == cls).sum()
    # the control: a mirrored way back does not pass
    rows7, own = scenes.scale_table(SCENE, P, (13, 13), STRIDE, (0,))
    win = scenes.host_windows_affine([img], [cls], rows7, P)[1]
    p = (win[:, :, ::-1, None] == np.arange(4)).astype(f32)
    wrong = scenes.host_argmax(scenes.host_accumulate(np.ascontiguousarray(p), rows7, own, [SCENE], 1))[0][0]
    assert (wrong[inner] != cls[inner]).any()


def test_special_floats_follow_quantise_q16():
    rows7, own = scenes.scale_table((8, 8), P, P, 8)
    p = np.zeros((1, 8, 8, 1), f32)
    vals = [np.nan, np.inf, -np.inf, -0.5, 1.5, 0.5, 2.0 ** -17, 3 * 2.0 ** -17, -0.0, 1.0]
    p[0, :2, :5, 0] = np.array(vals, f32).reshape(2, 5)
    acc = scenes.host_accumulate(p, rows7, own, [(8, 8)], 1)[0]
    assert acc[:2, :5, 0].ravel().tolist() == [0, 65536, 0, 0, 65536, 32768, 0, 2, 0, 65536]
    assert np.array_equal(acc[..., 0], scenes.quantise_q16(p[0, ..., 0]))
    with pytest.raises(ValueError, match="p is float32"):
        scenes.host_accumulate(p.astype(np.float64), rows7, own, [(8, 8)], 1)


def test_accumulate_refusals():
    shapes = [SCENE, (19, 23)]
    rows7, own = scenes.scale_table(SCENE, P, (13, 13), STRIDE, (0, 6))
    p = np.zeros((len(rows7), 8, 8, 3), f32)

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
        (rows7, with_cell(own, 4, 1, 54), r"group 4: rectangle rows \d+\.\.54, columns \d+\.\.\d+ outside its 53 x 61 scene"),
        (rows7, with_cell(own, 0, 2, -1), r"group 0: rectangle rows 0\.\.\d+, columns -1\.\.\d+ outside its 53 x 61 scene"),
        (rows7, with_cell(own, 0, 0, 12), r"group 0: rectangle rows 12\.\.11"),
        (rows7, with_cell(own, 0, 1, 30), r"row 0: rectangle rows 0\.\.30, columns \d+\.\.\d+ of group 0 leaves the window's footprint"),
        (rows7, with_cell(own, 1, 2, 0), r"row 2: rectangle rows \d+\.\.\d+, columns 0\.\.\d+ of group 1 leaves the window's footprint"),
        (with_cell(rows7, 7, 1, int(rows7[7, 1]) + 40 * 65536), own, "row 7: rectangle .* of group 3 leaves the window's footprint"),
    ]
    for r, o, msg in refused:
        with pytest.raises(ValueError, match=msg):
            scenes.host_accumulate(p, r, o, shapes, 2)
    for K, msg in ((0, "K 0 outside 1..8"), (9, "K 9 outside 1..8"), (4, r"window rows for \d+ groups of K 4 views"), (2.0, "must be an integer")):
        with pytest.raises(ValueError, match=msg):
            scenes.host_accumulate(p, rows7, own, shapes, K)
    with pytest.raises(ValueError, match="C 65 outside 1..64"):
        scenes.host_accumulate(np.zeros((len(rows7), 8, 8, 65), f32), rows7, own, shapes, 2)
    with pytest.raises(ValueError, match=r"PH 513, PW 8 \(1 <= PH, PW <= 512\)"):
        scenes.host_accumulate(np.zeros((len(rows7), 513, 8, 1), f32), rows7, own, shapes, 2)
    with pytest.raises(ValueError, match=r"scene 1: size 16385 x 23 \(1 <= H, W <= 16384\)"):
        scenes.check_accumulate([SCENE, (16385, 23)], rows7, own, 2, P, 3)
    with pytest.raises(ValueError, match=r"nscenes 0, G \d+ \(both >= 1\)"):
        scenes.check_accumulate([], rows7, own, 2, P, 3)
    for r, o in ((rows7[:, :6], own), (rows7, own[:, :3]), (rows7.astype(np.float32), own)):
        with pytest.raises(ValueError, match=r"takes integer \[G\*K\]\[7\] rows"):
            scenes.host_accumulate(p, r, o, shapes, 2)
    with pytest.raises(ValueError, match="one view per table row"):
        scenes.host_accumulate(p[:-2], rows7, own, shapes, 2)
    with pytest.raises(ValueError, match="an accumulator is an int32 array"):
        scenes.host_accumulate(p, rows7, own, shapes, 2, acc=[np.zeros(SCENE + (3,), np.int64), np.zeros((19, 23, 3), np.int32)])
    with pytest.raises(ValueError, match="1 accumulators for 2 scenes"):
        scenes.host_accumulate(p, rows7, own, shapes, 2, acc=[np.zeros(SCENE + (3,), np.int32)])
    # a transposing matrix on a flat patch
    frows, fown = scenes.scale_table(SCENE, (4, 12), (4, 12), 4, (0, 3))
    frows = frows.copy()
    frows[3, 3:] = [0, 65536, 65536, 0]
    with pytest.raises(ValueError, match=r"row 3: matrix \(0, 65536, 65536, 0\) transposes and needs a square patch \(got 4 x 12\)"):
        scenes.host_accumulate(np.zeros((len(frows), 4, 12, 1), f32), frows, fown, [SCENE], 2)


def test_host_argmax():
    acc = np.zeros((2, 3, 3), np.int32)
    acc[0, 0] = [5, 5, 1]                                      # a tie: the first index
    acc[0, 1] = [1, 7, 7]
    acc[0, 2] = [-3, -2, -1]
    acc[1, 0] = [0, 0, 0]
    acc[1, 1] = [2, 1, 2]
    acc[1, 2] = [-1, -1, -5]
    cls = np.array([[0, 1, 3], [255, 2, 0]], np.uint8)         # 3 and 255 are >= C: not counted
    maps, cm = scenes.host_argmax([acc], [cls])
    assert maps[0].dtype == np.uint8 and maps[0].tolist() == [[0, 1, 2], [0, 0, 0]]
    want = np.zeros((3, 3), np.int64)
    want[0, 0] += 2
    want[1, 1] += 1
    want[2, 0] += 1
    assert cm.dtype == np.int64 and np.array_equal(cm, want)
    assert scenes.host_argmax([acc])[1] is None and scenes.host_argmax([acc], None, 3)[0][0].tolist() == maps[0].tolist()
    one = scenes.host_argmax([np.full((4, 5, 1), -7, np.int32)], [np.array([[0] * 5, [1] * 5, [0] * 5, [9] * 5], np.uint8)])
    assert (one[0][0] == 0).all() and one[1].tolist() == [[10]]
    for bad, msg in (([acc.astype(np.int64)], "int32 array"), ([acc, np.zeros((2, 2, 4), np.int32)], "one C for all"), ([], "nscenes 0")):
        with pytest.raises(ValueError, match=msg):
            scenes.host_argmax(bad)
    with pytest.raises(ValueError, match="num_classes is 4"):
        scenes.host_argmax([acc], None, 4)
    with pytest.raises(ValueError, match="C 65 outside 1..64"):
        scenes.host_argmax([np.zeros((2, 2, 65), np.int32)])
    with pytest.raises(ValueError, match="its class map is 2 x 3"):
        scenes.host_argmax([acc], [cls.T])


def test_check_scales():
    assert scenes.check_scales(None, 64) is None and scenes.check_scales((1.0,), 64) is None and scenes.check_scales([1], 64) is None
    assert scenes.check_scales((0.75, 1.0, 1.5), 64) == ((85, 85), (64, 64), (43, 43))
    assert scenes.check_scales((2,), (32, 64), (40, 40)) == ((16, 32),)
    for bad, msg in (((), "1 to 8 distinct"), (tuple(1 + k / 10 for k in range(9)), "1 to 8 distinct"), (1.5, "1 to 8 distinct"), ("1.5", "1 to 8 distinct"),
                     ((1.0, 1), "zoom 1 occurs twice"), ((1.0, 1.001), "give the same footprint 64 x 64"), ((0.2,), "F <= 4 P"),
                     ((1.0, -2.0), "positive"), ((1.0, "x"), "positive")):
        with pytest.raises(ValueError, match=msg):
            scenes.check_scales(bad, 64)
    with pytest.raises(ValueError, match="zoom 0.5 gives a footprint of 128 x 128, larger than the 100 x 171 scene"):
        scenes.check_scales((1.0, 0.5), 64, (100, 171))
    with pytest.raises(ValueError, match="larger than the 64 x 64 scene"):
        scenes.check_scales((0.9,), 64, (64, 64))              # refused even where it is the only scale


def test_cli_takes_scales():
    import eval_scenes_ISPRS as cli
    need = ["--model_path", "m.h5", "--dataset_path", "d"]
    assert cli.build_parser().parse_args(need).scales is None
    args = cli.build_parser().parse_args(need + ["--scales", "0.75", "1", "1.5", "--views", "flips"])
    assert args.scales == [0.75, 1.0, 1.5]
    assert cli.parse_scales(None, 64) is None and cli.parse_scales(None, 64, ("seg",)) is None
    assert cli.parse_scales(args.scales, 64) == (0.75, 1.0, 1.5) and cli.parse_scales([1.0], 256) == (1.0,)
    with pytest.raises(SystemExit, match="--scales and --head_maps exclude each other"):
        cli.parse_scales([0.75, 1.0], 64, ("seg",))
    for zooms, msg in (([0.2], "F <= 4 P"), ([8.0], "P <= 4 F"), ([1.0, 1.0], "occurs twice"), ([-1.0], "positive")):
        with pytest.raises(SystemExit, match=msg):
            cli.parse_scales(zooms, 64)
    with pytest.raises(SystemExit, match="exclude each other"):   # refused before anything is read: the paths do not exist
        cli.main(need + ["--scales", "0.75", "1", "--head_maps", "seg"])
    with pytest.raises(SystemExit, match="--scales: .*P <= 4 F"):
        cli.main(need + ["--scales", "9"])
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(need + ["--scales", "big"])
