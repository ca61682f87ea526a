"""Host side of test-time augmentation for whole-scene evaluation: scenes.INVERSE, VIEW_SETS, check_views, view_rows,
check_view_table and scenes.host_stitch_views, the numpy definition of rua_scene_stitch_views (K views of a window turned back and
summed in float32 in view order, then host_stitch's arg-max, map and confusion matrix)."""
import numpy as np
import pytest

from resunet_a_mltsk_keras_amd import scenes

E = np.float32(2.0 ** -24)


def test_inverse_undoes_every_code():
    w = np.arange(5 * 5 * 2).reshape(5, 5, 2)
    assert scenes.INVERSE == (0, 5, 2, 3, 4, 1, 6, 7)
    for c in range(8):
        assert np.array_equal(scenes.transform(scenes.transform(w, c), scenes.INVERSE[c]), w), c
        assert scenes.INVERSE[scenes.INVERSE[c]] == c
    flat = np.arange(3 * 7).reshape(3, 7)
    for c in (0, 2, 3, 4):                                       # the codes a non-square patch may have
        t = scenes.transform(flat, c)
        assert t.shape == (3, 7) and np.array_equal(scenes.transform(t, scenes.INVERSE[c]), flat), c


def test_view_sets_and_view_rows():
    assert scenes.VIEW_SETS == {"none": (0,), "flips": (0, 3, 4), "aug5": (0, 1, 2, 3, 4), "all": (0, 1, 2, 3, 4, 5, 6, 7)}
    for name, codes in scenes.VIEW_SETS.items():
        assert scenes.check_views(name, 32) == codes and scenes.check_views(list(codes), (32, 32)) == codes
    rows = np.array([[0, 1, 2, 0], [1, 8, 24, 0], [0, 5, 5, 0]], np.int32)
    out = scenes.view_rows(rows, (5, 0, 7))
    assert out.dtype == np.int32 and out.shape == (9, 4)
    assert np.array_equal(out[:, :3], np.repeat(rows[:, :3], 3, axis=0))       # rows g*K .. g*K+K-1 are window g
    assert out[:, 3].tolist() == [5, 0, 7] * 3                                 # under the codes of views, in that order
    assert np.array_equal(scenes.view_rows(rows, "none"), rows)
    assert np.array_equal(scenes.view_rows(rows, "flips")[3:6], [[1, 8, 24, 0], [1, 8, 24, 3], [1, 8, 24, 4]])


def test_check_views_refusals():
    with pytest.raises(ValueError, match="code 3 occurs twice"):
        scenes.check_views((0, 3, 3))
    with pytest.raises(ValueError, match="code 8 outside 0..7"):
        scenes.check_views((0, 8))
    with pytest.raises(ValueError, match="K 9 outside 1..8"):
        scenes.check_views((0, 1, 2, 3, 4, 5, 6, 7, 0))
    with pytest.raises(ValueError, match="K 0 outside 1..8"):
        scenes.check_views(())
    with pytest.raises(ValueError, match=r"code 6 transposes and needs a square patch \(got 16 x 48\)"):
        scenes.check_views((0, 6), (16, 48))
    with pytest.raises(ValueError, match="not one of"):
        scenes.check_views("rotations")
    with pytest.raises(ValueError, match="integers"):
        scenes.check_views((0, 1.5))
    assert scenes.check_views((0, 2, 3, 4), (16, 48)) == (0, 2, 3, 4)          # no transposing code: any patch


def small_table():
    shapes = [(40, 57), (32, 32)]
    parts = []
    for s, shp in enumerate(shapes):
        rows, own = scenes.predict_table(shp, 32, 24)
        rows[:, 0] = s
        parts.append((rows, own))
    return shapes, np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def test_check_view_table_refusals():
    shapes, rows, own = small_table()
    vr = scenes.view_rows(rows, "flips")
    t, o, K = scenes.check_view_table(shapes, vr, own, "flips", 32, 5)
    assert K == 3 and t.dtype == np.int32 and np.array_equal(t, vr) and np.array_equal(o, own)
    assert scenes.check_view_table(shapes, vr, own, 3, 32, 5)[2] == 3

    def with_row(table, k, col, v):
        t = table.copy()
        t[k, col] = v
        return t
    with pytest.raises(ValueError, match=r"row 4: scene 0, window \(0, 23\), but its group 1 is scene 0, window \(0, 24\)"):
        scenes.check_view_table(shapes, with_row(vr, 4, 2, 23), own, 3, 32, 5)       # a group whose rows differ in origin
    with pytest.raises(ValueError, match=r"row 1: scene 1, window \(0, 0\), but its group 0 is scene 0"):
        scenes.check_view_table(shapes, with_row(vr, 1, 0, 1), own, 3, 32, 5)
    with pytest.raises(ValueError, match=f"{len(vr) - 1} window rows for {len(own)} groups of K 3"):
        scenes.check_view_table(shapes, vr[:-1], own, 3, 32, 5)                       # len(rows) no multiple of len(own)
    with pytest.raises(ValueError, match="no multiple"):
        scenes.host_stitch_views(np.zeros((len(vr) - 1, 32, 32, 5), np.float32), vr[:-1], own, shapes)
    with pytest.raises(ValueError, match="row 5: code 8 outside 0..7"):
        scenes.check_view_table(shapes, with_row(vr, 5, 3, 8), own, 3, 32, 5)
    with pytest.raises(ValueError, match="row 5: code 2, but view 2 of"):
        scenes.check_view_table(shapes, with_row(vr, 5, 3, 2), own, "flips", 32, 5)
    with pytest.raises(ValueError, match="K 9 outside 1..8"):
        scenes.check_view_table(shapes, np.repeat(rows, 9, 0), own, 9, 32, 5)
    with pytest.raises(ValueError, match=r"row 2: window \(0, 26\) \+ 32 x 32 leaves its 40 x 57 scene"):
        scenes.check_view_table(shapes, with_row(vr, 2, 2, 26), own, 3, 32, 5)
    with pytest.raises(ValueError, match=r"group 3: owned rows \d+\.\.33, columns"):
        scenes.check_view_table(shapes, vr, with_row(own, 3, 1, 33), 3, 32, 5)
    with pytest.raises(ValueError, match="C 65 outside 1..64"):
        scenes.check_view_table(shapes, vr, own, 3, 32, 65)
    flat_rows, flat_own = scenes.predict_table((40, 57), (16, 48), (12, 24))
    with pytest.raises(ValueError, match=r"row 1: code 1 transposes and needs a square patch \(got 16 x 48\)"):
        scenes.check_view_table([(40, 57)], scenes.view_rows(flat_rows, (0, 1)), flat_own, 2, (16, 48), 5)
    with pytest.raises(ValueError, match=r"code 1 transposes and needs a square patch \(got 16 x 48\)"):
        scenes.check_view_table([(40, 57)], scenes.view_rows(flat_rows, (0, 1)), flat_own, (0, 1), (16, 48), 5)


def class_maps_of(rng, shapes, C):
    maps = []
    for H, W in shapes:
        m = rng.integers(0, C, (H, W)).astype(np.uint8)
        m[rng.random((H, W)) < 0.02] = 255
        maps.append(m)
    return maps


def test_one_view_of_code_0_is_host_stitch():
    shapes, rows, own = small_table()
    rng = np.random.default_rng(0)
    p = rng.random((len(rows), 32, 32, 5), dtype=np.float32)
    maps = class_maps_of(rng, shapes, 5)
    for cm_in in (maps, None):
        got = scenes.host_stitch_views(p, rows, own, shapes, cm_in, fill=0xEE)
        want = scenes.host_stitch(p, rows, own, shapes, cm_in, fill=0xEE)
        assert all(np.array_equal(g, w) for g, w in zip(got[0], want[0]))
        assert (got[1] is None and want[1] is None) if cm_in is None else np.array_equal(got[1], want[1])
    with pytest.raises(ValueError, match="float32"):
        scenes.host_stitch_views(p.astype(np.float64), rows, own, shapes)


@pytest.mark.parametrize("views", ["flips", "aug5", "all", (5, 7)])
def test_views_of_one_common_window_give_its_map(views):
    """p[g*K + k] = transform(q[g], code_k): every view turned back is q, K * q is exact for q in k / 64, so the map is q's."""
    shapes, rows, own = small_table()
    codes = scenes.check_views(views)
    K = len(codes)
    rng = np.random.default_rng(1)
    q = (rng.integers(0, 65, (len(rows), 32, 32, 5)) / 64).astype(np.float32)
    p = np.stack([scenes.transform(q[g], c) for g in range(len(rows)) for c in codes])
    maps = class_maps_of(rng, shapes, 5)
    got = scenes.host_stitch_views(p, scenes.view_rows(rows, codes), own, shapes, maps, fill=0xEE)
    want = scenes.host_stitch(q, rows, own, shapes, maps, fill=0xEE)
    assert all(np.array_equal(g, w) for g, w in zip(got[0], want[0])) and np.array_equal(got[1], want[1])
    assert not any((m == 0xEE).any() for m in got[0])


def test_the_sum_runs_in_view_order_in_float32():
    """Class a holds (1, e, e) over three views, class b (e, e, 1), e = 2^-24, everything else 0.25 / K: in order and in float32
    a sums to 1 (1 + e rounds to 1, twice) and b to 1 + 2^-23 (e + e = 2^-23 is kept by 1 + .): b wins.  The views in reverse
    order exchange the two.  An exact sum is a tie: the lower index."""
    assert np.float32(1) + E == np.float32(1) and (E + E) + np.float32(1) == np.float32(1 + 2.0 ** -23)
    shapes, rows, own = [(8, 8)], np.array([[0, 0, 0, 0]], np.int32), np.array([[0, 8, 0, 8]], np.int32)
    codes = (0, 3, 4)
    for a, b in ((1, 3), (3, 1)):
        q = np.full((3, 8, 8, 5), 0.25 / 3, np.float32)
        q[:, :, :, a] = np.array([1, E, E], np.float32)[:, None, None]
        q[:, :, :, b] = np.array([E, E, 1], np.float32)[:, None, None]
        p = np.stack([scenes.transform(q[k], c) for k, c in enumerate(codes)])
        got = scenes.host_stitch_views(p, scenes.view_rows(rows, codes), own, shapes)[0][0]
        assert (got == b).all()
        back = scenes.host_stitch_views(p[::-1], scenes.view_rows(rows, codes[::-1]), own, shapes)[0][0]
        assert (back == a).all()
        assert (np.argmax(q.astype(np.float64).sum(0), -1) == min(a, b)).all()
