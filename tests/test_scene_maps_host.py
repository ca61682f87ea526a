"""Host tests of the whole-scene head maps (scenes.py): quantise_q16 on the values where a float pipeline would differ, hsv_to_rgb_u8
against hand values and through the round trip with labels.rgb_to_hsv_u8, and host_stitch_maps - the numpy definition of
rua_scene_stitch_maps - against a direct loop, under permuted views, on the hue wrap, on given maps and on every refusal."""
import numpy as np
import pytest

from resunet_a_mltsk_keras_amd import labels, scenes

f32 = np.float32


def test_quantise_q16_special_values():
    x = np.array([0.0, 1.0, 1.5, -0.25, np.nan, np.inf, -np.inf, 2.0 ** -140, -0.0, 0.5, 2.0 ** -17, 1 - 2.0 ** -24], f32)
    with np.errstate(invalid="ignore"):
        got = scenes.quantise_q16(x)
    assert got.dtype == np.int64
    assert got.tolist() == [0, 65536, 65536, 0, 0, 65536, 0, 0, 0, 32768, 0, 65536]      # 2^-17 * 65536 = 0.5: the tie goes to 0
    assert scenes.quantise_q16(np.zeros((2, 3, 4), f32)).shape == (2, 3, 4)
    with pytest.raises(ValueError, match="float32"):
        scenes.quantise_q16(np.zeros(3, np.float64))


def test_quantise_q16_ties_go_to_even():
    """(n + 0.5) / 65536 is exact in float32 for n < 2^16 (17 significant bits): rint sees an exact half and must round to the even."""
    n = np.array([0, 1, 2, 3, 254, 255, 32767, 32768, 65534, 65535], np.int64)
    x = ((n.astype(np.float64) + 0.5) / 65536).astype(f32)
    assert np.array_equal(x.astype(np.float64) * 65536, n + 0.5)         # nothing was rounded on the way in
    assert np.array_equal(scenes.quantise_q16(x), n + (n & 1))
    # every n: even n stays, odd n goes up
    n = np.arange(65536, dtype=np.int64)
    assert np.array_equal(scenes.quantise_q16(((n + 0.5) / 65536).astype(f32)), n + (n & 1))


def test_hsv_to_rgb_hand_values():
    cases = [((0, 255, 255), (255, 0, 0)), ((30, 255, 255), (255, 255, 0)), ((60, 255, 255), (0, 255, 0)), ((90, 255, 255), (0, 255, 255)),
             ((120, 255, 255), (0, 0, 255)), ((150, 255, 255), (255, 0, 255)),
             ((0, 0, 0), (0, 0, 0)), ((77, 200, 0), (0, 0, 0)), ((0, 0, 255), (255, 255, 255)), ((133, 0, 255), (255, 255, 255)),
             ((179, 255, 255), (255, 0, 9)),                      # f = 29: q = (255 * 255 + 3825) // 7650 = 9 (exactly 8.5 + 0.5)
             ((15, 128, 200), (200, 150, 100))]                   # p = 99.6 -> 100, t = (200 * 5730 + 3825) // 7650 = 150
    hsv = np.array([c[0] for c in cases], np.uint8)
    assert scenes.hsv_to_rgb_u8(hsv).tolist() == [list(c[1]) for c in cases]
    assert scenes.hsv_to_rgb_u8(hsv.reshape(3, 4, 3)).shape == (3, 4, 3) and scenes.hsv_to_rgb_u8(hsv).dtype == np.uint8


def test_hsv_to_rgb_refuses_h_above_179():
    with pytest.raises(ValueError, match="H 180 above 179"):
        scenes.hsv_to_rgb_u8(np.array([[10, 1, 1], [180, 5, 5]], np.uint8))
    with pytest.raises(ValueError, match="uint8"):
        scenes.hsv_to_rgb_u8(np.zeros((4, 3), np.int32))
    with pytest.raises(ValueError, match="uint8"):
        scenes.hsv_to_rgb_u8(np.zeros((4, 4), np.uint8))


def test_hsv_round_trip_with_rgb_to_hsv_u8():
    """hsv_to_rgb_u8(rgb_to_hsv_u8(rgb)) over the whole colour cube: maximum channel error 5, mean 0.3488 (H has 180 steps for 360
    degrees, so a channel between the extremes moves by up to 255 / 60 and a rounding); greys come back exactly (S = 0)."""
    g, b = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    worst, total = 0, 0
    for r in range(256):
        rgb = np.stack([np.full_like(g, r), g, b], -1)
        back = scenes.hsv_to_rgb_u8(labels.rgb_to_hsv_u8(rgb))
        d = np.abs(back.astype(np.int16) - rgb.astype(np.int16))
        worst, total = max(worst, int(d.max())), total + int(d.sum())
        assert back[r, r].tolist() == [r, r, r]
    mean = total / (3 * 2 ** 24)
    print(f"round trip over the colour cube: maximum {worst}, mean {mean:.4f}")
    assert worst == 5, worst
    assert round(mean, 4) == 0.3488, mean


# ---- host_stitch_maps -----------------------------------------------------------------------------------------------------------
def two_window_scene(Ch, seed=0, K=1, codes=(0,), shape=(12, 20), patch=(12, 12)):
    rng = np.random.default_rng(seed)
    rows, own = scenes.predict_table(shape, patch, 8)
    assert len(rows) == 2
    q = rng.random((len(rows), K, patch[0], patch[1], Ch), dtype=f32) * f32(1.2) - f32(0.1)     # some below 0, some above 1
    p = np.stack([scenes.transform(q[g, k], c) for g in range(len(rows)) for k, c in enumerate(codes)])
    return np.ascontiguousarray(p), q, scenes.view_rows(rows, codes), own


def test_one_view_against_a_direct_loop():
    p, q, rows, own = two_window_scene(5)
    got = scenes.host_stitch_maps(p, rows, own, [(12, 20)], 1)
    assert len(got) == 1 and got[0].dtype == np.uint8 and got[0].shape == (12, 20, 5)
    want = np.zeros((12, 20, 5), np.uint8)
    seen = np.zeros((12, 20), int)
    for n, ((_, r, c, _), (r0, r1, c0, c1)) in enumerate(zip(rows.tolist(), own.tolist())):
        for i in range(r0, r1):
            for j in range(c0, c1):
                seen[r + i, c + j] += 1
                for ch in range(5):
                    x = float(p[n, i, j, ch])
                    a = int(np.rint(f32(min(max(x, 0.0), 1.0)) * f32(65536)))
                    want[r + i, c + j, ch] = (255 * a + 32768) // 65536
    assert (seen == 1).all()
    assert np.array_equal(got[0], want)
    assert np.array_equal(got[0], scenes.host_stitch_maps(p, rows, own, [(12, 20)], 1, patch=12)[0])
    # the rounded mean is within half a step of 255 * clip(x)
    mosaic = np.zeros((12, 20, 5))
    for n, ((_, r, c, _), (r0, r1, c0, c1)) in enumerate(zip(rows.tolist(), own.tolist())):
        mosaic[r + r0:r + r1, c + c0:c + c1] = np.clip(p[n, r0:r1, c0:c1].astype(np.float64), 0, 1)
    assert np.abs(got[0] - 255 * mosaic).max() <= 0.5 + 255 / 131072 + 1e-9


@pytest.mark.parametrize("codes", [(0, 3, 4), (0, 1, 2, 3, 4, 5, 6, 7), (5, 7)])
def test_plain_mode_does_not_depend_on_the_order_of_the_views(codes):
    K = len(codes)
    p, q, rows, own = two_window_scene(6, seed=K, K=K, codes=codes)
    base = scenes.host_stitch_maps(p, rows, own, [(12, 20)], K)[0]
    # the definition from the un-transformed stack
    A = scenes.quantise_q16(q).sum(1)
    for g, ((_, r, c, _), (r0, r1, c0, c1)) in enumerate(zip(rows[::K].tolist(), own.tolist())):
        want = (255 * A[g, r0:r1, c0:c1] + K * 32768) // (K * 65536)
        assert np.array_equal(base[r + r0:r + r1, c + c0:c + c1], want)
    rng = np.random.default_rng(1)
    for _ in range(4):
        perm = rng.permutation(K)
        pp = p.reshape(2, K, *p.shape[1:])[:, perm].reshape(p.shape)
        pr = rows.reshape(2, K, 4)[:, perm].reshape(-1, 4)
        assert np.array_equal(scenes.host_stitch_maps(pp, pr, own, [(12, 20)], K)[0], base)


def test_hue_wrap_is_red_not_cyan():
    """Views at hue 0.005 and 0.995, full S and V: both are red; a mean of hues would be 0.5, cyan."""
    rows = scenes.view_rows(np.array([[0, 0, 0, 0]], np.int32), (0, 3))
    own = np.array([[0, 4, 0, 4]], np.int32)
    p = np.empty((2, 4, 4, 3), f32)
    p[0], p[1] = [0.005, 1, 1], [0.995, 1, 1]
    got = scenes.host_stitch_maps(p, rows, own, [(4, 4)], 2, mode="hsv_rgb")[0]
    assert got.shape == (4, 4, 3)
    assert (got[..., 0] >= 250).all() and (got[..., 1:] <= 16).all(), got[0, 0]
    # the single views: h = 0 -> (255, 0, 0); h = 178 -> (255, 0, 17)
    one = scenes.host_stitch_maps(p[1:], rows[:1], own, [(4, 4)], 1, mode="hsv_rgb")[0]
    assert one[0, 0].tolist() == [255, 0, 17] and got[0, 0].tolist() == [255, 0, 9]      # (2 * 17 + 2) // 4 = 9
    # S = 0 is grey at V, V = 0 black, whatever the hue
    p[0], p[1] = [0.7, 0, 0.5], [0.3, 1, 0]
    got = scenes.host_stitch_maps(p, rows, own, [(4, 4)], 2, mode="hsv_rgb")[0]
    assert got[0, 0].tolist() == [(2 * 127 + 2) // 4] * 3                                  # (127, 127, 127) and (0, 0, 0)


def test_given_maps_keep_their_bytes_outside_the_rectangles():
    p, q, rows, own = two_window_scene(3)
    own = own.copy()
    own[1] = [2, 5, 3, 4]                                      # window 1 (at column 8) owns 3 x 1 pixels
    own[0] = [0, 0, 0, 12]                                     # window 0 owns nothing
    given = [np.full((12, 20, 3), 0xEE, np.uint8)]
    out = scenes.host_stitch_maps(p, rows, own, [(12, 20)], 1, maps=given)
    assert out[0] is given[0]
    inside = np.zeros((12, 20), bool)
    inside[2:5, 11:12] = True
    assert (given[0][~inside] == 0xEE).all()
    fresh = scenes.host_stitch_maps(p, rows, own, [(12, 20)], 1)[0]
    assert (fresh[~inside] == 0).all() and np.array_equal(fresh[inside], given[0][inside])
    with pytest.raises(ValueError, match="a given map is a uint8 array"):
        scenes.host_stitch_maps(p, rows, own, [(12, 20)], 1, maps=[np.zeros((12, 20), np.uint8)])


def test_255_exactly_when_every_view_is_at_least_one():
    """Every view >= 1 (1, 1.5, +inf, in any mix) gives exactly 255: the clamp keeps A at K * 65536, nothing wraps.  Below that the
    formula decides, and the test pins its threshold: out = 255 needs 255 A + K 32768 >= 255 K 65536, i.e. a total shortfall
    K * 65536 - A of at most K * 32768 // 255 (385 for K = 3) - the half step every rounded value has."""
    K = 3
    rows = scenes.view_rows(np.array([[0, 0, 0, 0]], np.int32), (0, 4, 3))
    own = np.array([[0, 2, 0, 8]], np.int32)
    p = np.ones((K, 2, 8, 1), f32)
    p[0, 0, :, 0] = [1, 1.5, np.inf, 1, 2, 1e30, 1, 1]          # view 0 is code 0: these are window pixels (0, j)
    p[1, 1, :, 0] = [3, 1, 1, np.inf, 1, 1, 1.25, 1]
    got = scenes.host_stitch_maps(p, rows, own, [(2, 8)], K)[0][..., 0]
    assert (got == 255).all()
    short = np.array([0, 1, 384, 385, 386, 771, 20000, 65536], np.int64)      # of view 0 alone; (n + 0) / 65536 is exact
    p = np.ones((K, 2, 8, 1), f32)
    p[0, 0, :, 0] = ((65536 - short) / 65536).astype(f32)
    assert np.array_equal(scenes.quantise_q16(p[0, 0, :, 0]), 65536 - short)
    got = scenes.host_stitch_maps(p, rows, own, [(2, 8)], K)[0][..., 0]
    assert (got[1] == 255).all()
    assert got[0].tolist() == [255, 255, 255, 255, 254, 254, 229, 170]
    assert np.array_equal(got[0] == 255, short <= K * 32768 // 255)


def test_refusals_are_check_view_tables():
    shapes = [(40, 57), (32, 32)]
    parts = []
    for s, shp in enumerate(shapes):
        r, o = scenes.predict_table(shp, (32, 32), 24)
        r[:, 0] = s
        parts.append((r, o))
    rows, own = np.concatenate([x[0] for x in parts]), np.concatenate([x[1] for x in parts])
    codes = (0, 1, 4)
    vr = scenes.view_rows(rows, codes)
    p = np.zeros((len(vr), 32, 32, 3), f32)

    def with_row(table, k, col, v):
        t = table.copy()
        t[k, col] = v
        return t
    refused = [
        (with_row(vr, 4, 2, 23), own, r"row 4: scene 0, window \(0, 23\), but its group 1 is scene 0, window \(0, 24\)"),
        (with_row(vr, 1, 0, 1), own, r"row 1: scene 1, window \(0, 0\), but its group 0 is scene 0, window \(0, 0\)"),
        (with_row(vr, 2, 2, 26), own, r"row 2: window \(0, 26\) \+ 32 x 32 leaves its 40 x 57 scene"),
        (with_row(vr, 4, 1, -1), own, "row 4: window"),
        (with_row(vr, 3, 0, 2), own, "row 3: scene 2 outside 0..1"),
        (with_row(vr, 5, 3, 8), own, "row 5: code 8 outside 0..7"),
        (with_row(vr, 5, 3, -1), own, "row 5: code -1 outside 0..7"),
        (vr, with_row(own, 3, 1, 33), r"group 3: owned rows \d+\.\.33, columns"),
        (vr, with_row(own, 0, 2, 40), "group 0: owned rows"),
        (vr, own[:-1], "window rows for"),
        (vr.astype(np.float32), own, "integer"),
    ]
    for r, o, msg in refused:
        with pytest.raises(ValueError, match=msg):
            scenes.host_stitch_maps(p, r, o, shapes, 3)
    for K, msg in ((0, "K 0 outside 1..8"), (9, "K 9 outside 1..8"), (2, "window rows for"), (True, "integer")):
        with pytest.raises(ValueError, match=msg):
            scenes.host_stitch_maps(p, vr, own, shapes, K)
    with pytest.raises(ValueError, match="C 65 outside 1..64"):
        scenes.host_stitch_maps(np.zeros((len(vr), 32, 32, 65), f32), vr, own, shapes, 3)
    with pytest.raises(ValueError, match="float32"):
        scenes.host_stitch_maps(p.astype(np.float64), vr, own, shapes, 3)
    with pytest.raises(ValueError, match="one view per table row"):
        scenes.host_stitch_maps(p[:-1], vr, own, shapes, 3)
    with pytest.raises(ValueError, match="mode 'rgb'"):
        scenes.host_stitch_maps(p, vr, own, shapes, 3, mode="rgb")
    with pytest.raises(ValueError, match="hsv_rgb.*Ch 3, got 5"):
        scenes.host_stitch_maps(np.zeros((len(vr), 32, 32, 5), f32), vr, own, shapes, 3, mode="hsv_rgb")
    with pytest.raises(ValueError, match="the patch is 16 x 48"):
        scenes.host_stitch_maps(p, vr, own, shapes, 3, patch=(16, 48))
    # a transposing code on a flat patch
    frows, fown = scenes.predict_table((40, 57), (16, 48), (12, 24))
    fvr = with_row(scenes.view_rows(frows, (0, 3)), 3, 3, 6)
    with pytest.raises(ValueError, match=r"row 3: code 6 transposes and needs a square patch \(got 16 x 48\)"):
        scenes.host_stitch_maps(np.zeros((len(fvr), 16, 48, 3), f32), fvr, fown, [(40, 57)], 2)
