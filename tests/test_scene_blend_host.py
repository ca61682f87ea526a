"""Host definitions of blended whole-scene prediction (scenes.py): blend_weight - the linear taper in 1/256 -, blend_table - one pass'
affine rows and full footprints -, host_accumulate_blend - the numpy definition of rua_scene_accumulate_blend, overlapping footprints
added under their weights in integers -, check_accumulate_blend and check_blend_budget.  No GPU."""
import numpy as np
import pytest

from resunet_a_mltsk_keras_amd import scenes

SCENE, P = (19, 23), (8, 8)
ALL = scenes.VIEW_SETS["all"]
f32 = np.float32


def weights(F, flat_lo=False, flat_hi=False):
    return [scenes.blend_weight(t, F, flat_lo, flat_hi) for t in range(F)]


def test_blend_weight_by_hand():
    assert weights(8) == [32, 96, 160, 224, 224, 160, 96, 32]
    assert scenes.blend_weight(0, 256, False, False) == 16          # 256 // 256 = 1: the floor
    assert weights(8, flat_lo=True) == [256, 256, 256, 256, 224, 160, 96, 32]
    assert weights(8, flat_hi=True) == [32, 96, 160, 224, 256, 256, 256, 256]
    assert weights(8, True, True) == [256] * 8
    assert weights(7) == [36, 109, 182, 256, 182, 109, 36]         # odd: the centre pixel is whole
    assert weights(7, flat_lo=True) == [256, 256, 256, 256, 182, 109, 36] and weights(7, flat_hi=True) == [36, 109, 182, 256, 256, 256, 256]
    assert weights(1) == [256] and weights(2) == [128, 128]
    for t in (-1, 8):
        with pytest.raises(ValueError, match=f"blend_weight: position {t} outside 0..7"):
            scenes.blend_weight(t, 8, False, False)


@pytest.mark.parametrize("F", [1, 2, 5, 8, 13, 64, 100, 255, 256, 341, 2048])
def test_blend_weight_is_symmetric_bounded_and_its_vector_form(F):
    for flags in ((False, False), (True, True)):
        w = weights(F, *flags)
        assert w == w[::-1] and all(16 <= v <= 256 for v in w)
    for lo in (False, True):
        for hi in (False, True):
            assert scenes._blend_axis(0, F, F, lo, hi).tolist() == weights(F, lo, hi)
            assert weights(F, lo, hi) == weights(F, hi, lo)[::-1]
    assert scenes._blend_axis(F // 3, F, F, False, True).tolist() == weights(F, False, True)[F // 3:]


@pytest.mark.parametrize("F", [2, 8, 14, 64, 256, 342])
def test_neighbouring_tapers_sum_to_one(F):
    """Even F at a stride of F / 2: position t of one footprint is position t + F / 2 of its neighbour."""
    w = weights(F)
    sums = [w[t] + w[t + F // 2] for t in range(F // 2) if w[t] > 16 and w[t + F // 2] > 16]
    assert len(sums) >= F // 2 - F // 8 and all(255 <= s <= 256 for s in sums)


def random_p(rng, n, patch, C):
    return rng.random((n,) + tuple(patch) + (C,), dtype=f32)


def test_one_footprint_that_is_the_scene_is_host_accumulate():
    rng = np.random.default_rng(0)
    rows7, foot = scenes.blend_table((8, 8), 8, 8, 8, ALL)
    assert foot.tolist() == [[0, 8, 0, 8]] and len(rows7) == 8
    assert scenes._blend_axis(0, 8, 8, True, True).tolist() == [256] * 8
    p = random_p(rng, 8, P, 5)
    got = scenes.host_accumulate_blend(p, rows7, foot, [(8, 8)], 8)
    want = scenes.host_accumulate(p, rows7, np.array([[0, 8, 0, 8]], np.int32), [(8, 8)], 8)
    assert got[0].dtype == np.int32 and np.array_equal(got[0], want[0]) and want[0].any()


@pytest.mark.parametrize("F,stride", [((8, 8), 4), ((5, 5), 3), ((13, 13), 8)])
def test_blend_table_rows_are_scale_tables_and_footprints_cover_the_scene(F, stride):
    for views in ((0,), ALL):
        rows7, foot = scenes.blend_table(SCENE, P, F, stride, views)
        srows, own = scenes.scale_table(SCENE, P, F, stride, views)
        assert rows7.dtype == np.int32 and foot.dtype == np.int32 and np.array_equal(rows7, srows) and foot.shape == own.shape
        assert ((foot[:, 1] - foot[:, 0] == F[0]) & (foot[:, 3] - foot[:, 2] == F[1])).all()
        assert (foot[:, 0] >= 0).all() and (foot[:, 1] <= SCENE[0]).all() and (foot[:, 2] >= 0).all() and (foot[:, 3] <= SCENE[1]).all()
        assert ((foot[:, 0] <= own[:, 0]) & (own[:, 1] <= foot[:, 1]) & (foot[:, 2] <= own[:, 2]) & (own[:, 3] <= foot[:, 3])).all()
        cover = np.zeros(SCENE, np.int64)
        for r0, r1, c0, c1 in foot.tolist():
            cover[r0:r1, c0:c1] += 1
        assert (cover >= 1).all() and cover.max() > 1
        t, o = scenes.check_accumulate_blend([SCENE], rows7, foot, len(views), P, 3)     # every full footprint passes the kernel's checks
        assert np.array_equal(t, rows7) and np.array_equal(o, foot)


def direct(p, rows7, foot, shape, K):
    """host_accumulate_blend spelt out pixel by pixel with blend_weight and host_accumulate on one-pixel rectangles."""
    H, W = shape
    acc = np.zeros((H, W, p.shape[-1]), np.int64)
    for g, (r0, r1, c0, c1) in enumerate(foot.tolist()):
        for y in range(r0, r1):
            wy = scenes.blend_weight(y - r0, r1 - r0, r0 == 0, r1 == H)
            for x in range(c0, c1):
                wx = scenes.blend_weight(x - c0, c1 - c0, c0 == 0, c1 == W)
                v = scenes.host_accumulate(p[g * K:(g + 1) * K], rows7[g * K:(g + 1) * K], np.array([[y, y + 1, x, x + 1]]), [shape], K)[0][y, x]
                acc[y, x] += (wy * wx * v.astype(np.int64) + 32768) >> 16
    return acc


def test_host_accumulate_blend_pixel_by_pixel():
    rng = np.random.default_rng(1)
    shape, views = (11, 13), (0, 5)
    rows7, foot = scenes.blend_table(shape, P, (5, 5), 4, views)
    p = random_p(rng, len(rows7), P, 3)
    got = scenes.host_accumulate_blend(p, rows7, foot, [shape], 2)[0]
    assert np.array_equal(got, direct(p, rows7, foot, shape, 2))


def test_a_constant_field_keeps_its_argmax_and_equal_classes_stay_equal():
    rows7, foot = scenes.blend_table(SCENE, P, (8, 8), 4, ALL)
    p = np.empty((len(rows7), 8, 8, 4), f32)
    p[:] = np.array([0.2, 0.45, 0.1, 0.25], f32)
    acc = scenes.host_accumulate_blend(p, rows7, foot, [SCENE], 8)[0]
    assert (acc.argmax(-1) == 1).all() and (acc.argmin(-1) == 2).all() and (acc > 0).all()
    p[:] = f32(0.37)
    acc = scenes.host_accumulate_blend(p, rows7, foot, [SCENE], 8)[0]
    assert (acc == acc[:, :, :1]).all() and (acc > 0).all()
    maps, _ = scenes.host_argmax([acc])
    assert (maps[0] == 0).all()


def test_order_of_groups_and_split_calls_do_not_matter():
    rng = np.random.default_rng(2)
    K = 3
    rows7, foot = scenes.blend_table(SCENE, P, (13, 13), 6, (0, 3, 6))
    G = len(foot)
    p = random_p(rng, G * K, P, 5)
    base = [rng.integers(-50000, 50000, SCENE + (5,)).astype(np.int32)]
    want = scenes.host_accumulate_blend(p, rows7, foot, [SCENE], K, acc=[base[0].copy()])[0]
    assert (want != base[0]).all()
    order = np.arange(G)[::-1]
    rrows, rp = rows7.reshape(G, K, 7)[order].reshape(-1, 7), p.reshape((G, K) + p.shape[1:])[order].reshape(p.shape)
    assert np.array_equal(scenes.host_accumulate_blend(rp, rrows, foot[order], [SCENE], K, acc=[base[0].copy()])[0], want)
    h = G // 2
    acc = scenes.host_accumulate_blend(p[:h * K], rows7[:h * K], foot[:h], [SCENE], K, acc=[base[0].copy()])
    acc = scenes.host_accumulate_blend(p[h * K:], rows7[h * K:], foot[h:], [SCENE], K, acc=acc)
    assert np.array_equal(acc[0], want)
    some = foot.copy()
    some[::2, 1] = some[::2, 0]                                  # empty rectangles add nothing
    keep = np.arange(G)[1::2]
    kr, kp = rows7.reshape(G, K, 7)[keep].reshape(-1, 7), p.reshape((G, K) + p.shape[1:])[keep].reshape((-1,) + p.shape[1:])
    assert np.array_equal(scenes.host_accumulate_blend(p, rows7, some, [SCENE], K)[0], scenes.host_accumulate_blend(kp, kr, foot[keep], [SCENE], K)[0])


def test_check_blend_budget():
    # patch 64 at stride 16, zooms whose footprints 128, 64, 32 are four scaled strides: four footprints over a pixel per axis at every
    # scale; three scales, K = 8: 8 * 48
    fps = [scenes.scale_footprint(64, z) for z in (0.5, 1.0, 2.0)]
    assert [scenes._axis_depth(256, f[0], (2 * 16 * f[0] + 64) // 128) for f in fps] == [4, 4, 4]
    # 19 pixels, footprint 8, stride 4: origins 0, 4, 8 and the flush 11 - pixel 11 lies in three
    assert scenes._axis_depth(256, 85, 21) == 5 and scenes._axis_depth(19, 8, 4) == 3 and scenes._axis_depth(8, 8, 8) == 1
    assert scenes.check_blend_budget((256, 256), 64, fps, 16, 8) == 8 * 48
    for shape, F, stride in (((19, 23), (8, 8), 4), ((33, 40), (13, 13), 6), ((19, 23), (5, 5), 3)):      # against a count of blend_table's footprints
        cover = np.zeros(shape, np.int64)
        for r0, r1, c0, c1 in scenes.blend_table(shape, 8, F, stride)[1].tolist():
            cover[r0:r1, c0:c1] += 1
        assert scenes.check_blend_budget(shape, 8, [F], stride, 1) == cover.max() > 1
    assert scenes.check_blend_budget((8, 8), 8, [(8, 8)], 4, 8) == 8
    # stride 1: 64 x 64 footprints over the middle pixels, K = 8: exactly 32768, one too many
    assert scenes._axis_depth(128, 64, 1) == 64
    with pytest.raises(ValueError, match=r"check_blend_budget: K 8 views times 4096 footprints over one pixel .* is 32768: the int32 accumulator takes fewer than 32768"):
        scenes.check_blend_budget((128, 128), 64, [(64, 64)], 1, 8)
    assert scenes.check_blend_budget((128, 128), 64, [(64, 64)], 1, 7) == 7 * 4096
    with pytest.raises(ValueError, match="fewer than 32768"):
        scenes.check_blend_budget((128, 128), 64, [(64, 64), (32, 32)], 1, 7)       # the passes add up: 7 * (4096 + 1024)
    with pytest.raises(ValueError, match="check_blend_budget: footprint 64 x 64 is larger than the 63 x 128 scene"):
        scenes.check_blend_budget((63, 128), 64, [(64, 64)], 32, 1)


SHAPES = [(33, 40), (19, 23)]


def two_scene_tables(views):
    parts = []
    for s, shp in enumerate(SHAPES):
        rows7, foot = scenes.blend_table(shp, P, (13, 13), 6, views)
        rows7[:, 0] = s
        parts.append((rows7, foot))
    return np.concatenate([a for a, _ in parts]), np.concatenate([b for _, b in parts])


def with_cell(t, k, col, v):
    t = t.copy()
    t[k, col] = v
    return t


def blend_refusals(rows7, foot):
    """(rows7, foot, message) for every refusal of a table that check_accumulate_blend and the entry point share; K = 2, C = 3."""
    return [
        (with_cell(rows7, 3, 0, 2), foot, "rua_scene_accumulate_blend: row 3: scene 2 outside 0..1"),
        (with_cell(rows7, 3, 0, -1), foot, "rua_scene_accumulate_blend: row 3: scene -1 outside 0..1"),
        (with_cell(rows7, 5, 0, 1), foot, "rua_scene_accumulate_blend: row 5: scene 1, but its group 2 is scene 0"),
        (with_cell(rows7, 2, 4, 7), foot, r"rua_scene_accumulate_blend: row 2: matrix \(\d+, 7, 0, \d+\) is not axis-aligned"),
        (with_cell(rows7, 2, 3, 0), foot, r"row 2: matrix \(0, 0, 0, \d+\) is not axis-aligned"),
        (with_cell(rows7, 1, 3, 9), foot, r"row 1: matrix \(9, \d+, \d+, 0\) is not axis-aligned"),
        (rows7, with_cell(foot, 4, 1, 34), r"rua_scene_accumulate_blend: group 4: rectangle rows \d+\.\.34, columns \d+\.\.\d+ outside its 33 x 40 scene"),
        (rows7, with_cell(foot, 0, 2, -1), r"group 0: rectangle rows 0\.\.13, columns -1\.\.13 outside its 33 x 40 scene"),
        (rows7, with_cell(foot, 0, 0, 14), "group 0: rectangle rows 14..13"),
        (rows7, with_cell(foot, 3, 1, int(foot[3, 1]) - 1), r"rua_scene_accumulate_blend: group 3: rectangle of 12 x 13, but group 0 has 13 x 13 \(the footprints of one call have one size\)"),
        (rows7, with_cell(foot, 1, 3, int(foot[1, 3]) + 1), r"group 1: rectangle of 13 x 14, but group 0 has 13 x 13"),
        # group 0 empty: the first non-empty rectangle sets the size
        (rows7, with_cell(with_cell(foot, 0, 1, 0), 1, 3, int(foot[1, 3]) + 1), r"group 2: rectangle of 13 x 13, but group 1 has 13 x 14"),
        (rows7, with_cell(foot, 0, 1, 16), r"rua_scene_accumulate_blend: row 0: rectangle rows 0\.\.16, columns 0\.\.13 of group 0 leaves the window's footprint"),
        (with_cell(rows7, 7, 1, int(rows7[7, 1]) + 40 * 65536), foot, "row 7: rectangle .* of group 3 leaves the window's footprint"),
    ]


def test_check_accumulate_blend_refuses_what_the_entry_point_refuses():
    rows7, foot = two_scene_tables((0, 6))
    assert foot[0].tolist() == [0, 13, 0, 13] and foot[1, 2] > 0
    p = np.zeros((len(rows7), 8, 8, 3), f32)
    t, o = scenes.check_accumulate_blend(SHAPES, rows7, foot, 2, P, 3)
    assert t.flags.c_contiguous and o.flags.c_contiguous and np.array_equal(t, rows7) and np.array_equal(o, foot)
    for r, o, msg in blend_refusals(rows7, foot):
        with pytest.raises(ValueError, match=msg):
            scenes.check_accumulate_blend(SHAPES, r, o, 2, P, 3)
        with pytest.raises(ValueError, match=msg):
            scenes.host_accumulate_blend(p, r, o, SHAPES, 2)
    for kw, msg in ((dict(K=0), "rua_scene_accumulate_blend: K 0 outside 1..8"), (dict(K=9), "K 9 outside 1..8"), (dict(K=True), "K True must be an integer"),
                    (dict(K=3), "rua_scene_accumulate_blend: .* window rows for .* groups of K 3 views"),
                    (dict(num_classes=65), "rua_scene_accumulate_blend: C 65 outside 1..64"), (dict(num_classes=0), "C 0 outside 1..64"),
                    (dict(patch=(8, 513)), r"rua_scene_accumulate_blend: PH 8, PW 513 \(1 <= PH, PW <= 512\)"),
                    (dict(shapes=[(16385, 40), (19, 23)]), r"rua_scene_accumulate_blend: scene 0: size 16385 x 40 \(1 <= H, W <= 16384\)"),
                    (dict(shapes=[]), r"rua_scene_accumulate_blend: nscenes 0, G \d+ \(both >= 1\)"),
                    (dict(rows7=rows7[:, :6]), "rua_scene_accumulate_blend takes integer"), (dict(foot=foot.astype(f32)), "rua_scene_accumulate_blend takes integer"),
                    (dict(rows7=rows7[:0], foot=foot[:0]), r"nscenes 2, G 0 \(both >= 1\)")):
        args = dict(shapes=SHAPES, rows7=rows7, foot=foot, K=2, patch=P, num_classes=3)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            scenes.check_accumulate_blend(args["shapes"], args["rows7"], args["foot"], args["K"], args["patch"], args["num_classes"])
    frows, ffoot = scenes.blend_table(SHAPES[0], (4, 12), (4, 12), 4, (0, 3))
    frows[3, 3:] = [0, 65536, 65536, 0]
    with pytest.raises(ValueError, match=r"rua_scene_accumulate_blend: row 3: matrix \(0, 65536, 65536, 0\) transposes and needs a square patch \(got 4 x 12\)"):
        scenes.check_accumulate_blend(SHAPES, frows, ffoot, 2, (4, 12), 3)
    # empty rectangles have no size: padding groups pass, whatever their numbers
    pad = with_cell(with_cell(foot, 2, 1, int(foot[2, 0])), 5, 3, int(foot[5, 2]))
    pad[7] = 0
    scenes.check_accumulate_blend(SHAPES, rows7, pad, 2, P, 3)
    # the existing entry point's checker takes rectangles of any sizes and keeps its own name
    scenes.check_accumulate(SHAPES, rows7, with_cell(foot, 3, 1, int(foot[3, 1]) - 1), 2, P, 3)
    with pytest.raises(ValueError, match="rua_scene_accumulate: K 9 outside 1..8"):
        scenes.check_accumulate(SHAPES, rows7, foot, 9, P, 3)
