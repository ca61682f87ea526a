"""Host tests of the precision-recall sweep: scenes.host_area_open against a restatement with scipy.ndimage.label per level and against
the shrinking-set construction the kernel uses (only the unsettled pixels are labelled, a component settles by its size or by touching
a settled pixel), nestedness and monotone recall, the level table of min_area 1, scenes.sweep_scores by hand and against
sklearn's average_precision_score, scenes.sweep_levels and its refusals, and the cpu pool.  Bytes and integers only: every comparison
of maps and counts is exact.  The reference's own function, skimage.morphology.area_opening, is not installed where these tests were
written, so it is restated here through component sizes and no fixture made from it is committed.
sweep_cases() are the maps the GPU tests (test_scene_sweep_gpu.py) share."""
import functools

import numpy as np
import pytest

from resunet_a_mltsk_keras_amd import scenes
from test_scene_regions_host import serpentine

TILE = 32                                      # SW_T of csrc/sweep.hip: the hand-made cases are placed by it
ALL = tuple(range(255, 0, -1))
FIFTH = tuple(range(255, 0, -5))
MIN_AREA = 5                                   # of the hand-made cases
HAND = (250, 220, 200, 199, 198, 180, 170, 150, 100, 60)                          # ... and their levels: every byte they hold, and two between


def cone(H, W):
    """A cone around (TILE - 2, TILE - 2), or the last pixel of a smaller map: its level sets are diamonds that grow across both
    seams of the first tile level by level."""
    ci, cj = min(H - 1, TILE - 2), min(W - 1, TILE - 2)
    d = np.abs(np.arange(H) - ci)[:, None] + np.abs(np.arange(W) - cj)[None, :]
    return np.clip(255 - 4 * d, 0, 255).astype(np.uint8)


def smooth(rng, H, W, r=3):
    a = rng.random((H + 2 * r, W + 2 * r))
    s = sum(a[i:i + H, j:j + W] for i in range(2 * r + 1) for j in range(2 * r + 1))
    s = (s - s.min()) / (s.max() - s.min())
    return np.rint(255 * s).astype(np.uint8)


def blank():
    return np.zeros((2 * TILE + 1, 2 * TILE + 1), np.uint8)


def hand_made():
    """name -> (map, {connectivity: (pixel, expected opened byte)}) at MIN_AREA and the levels HAND: one rule of the construction each."""
    T = TILE
    out = {}
    m = blank()                                # a speck of one pixel at 200 that has 3 pixels at 199 and 5 at 198: settled two levels later
    m[10, 10], m[10, 9], m[10, 11], m[9, 10], m[11, 10] = 200, 199, 199, 198, 198
    out["speck_grows"] = (m, {4: ((10, 10), 198), 8: ((10, 10), 198)})
    m = blank()                                # two pixels at 150, never 5: settled at 100 through a pixel that touches a settled block by an edge
    m[5:15, 5:15] = 220
    m[10, 15], m[10, 16], m[10, 17] = 100, 150, 150
    out["touch_edge"] = (m, {4: ((10, 17), 100), 8: ((10, 17), 100)})
    m = blank()                                # ... by a diagonal only: connectivity 4 never settles it
    m[5:15, 5:15] = 220
    m[15, 15], m[15, 16], m[15, 17] = 100, 150, 150
    out["touch_diagonal"] = (m, {4: ((15, 17), 0), 8: ((15, 17), 100)})
    m = blank()                                # the settled neighbour lies across a tile seam: only the halo shows it
    m[5:15, T - 10:T] = 220
    m[10, T], m[10, T + 1] = 100, 150
    out["halo_seam"] = (m, {4: ((10, T + 1), 100), 8: ((10, T + 1), 100)})
    m = blank()                                # ... across a tile corner: the halo's corner, connectivity 8 only
    m[T - 10:T, T - 10:T] = 220
    m[T, T], m[T, T + 1] = 100, 150
    out["halo_corner"] = (m, {4: ((T, T + 1), 0), 8: ((T, T + 1), 100)})
    m = blank()                                # 3 + 3 pixels over a seam make 6 >= 5; 2 + 2 stay out; the same over a horizontal seam
    m[40, T - 3:T + 3] = 180
    m[44, T - 2:T + 2] = 180
    m[T - 3:T + 3, 50] = 170
    out["split_sum"] = (m, {4: ((40, T + 2), 180), 8: ((44, T), 0)})
    m = blank()                                # 2 + 2 pixels over a seam, the settled block touches the part that does not hold the root
    m[50:60, T + 2:T + 12] = 220
    m[55, T - 2:T + 2] = 100
    out["split_touch"] = (m, {4: ((55, T - 2), 100), 8: ((55, T - 2), 100)})
    return out


def sweep_cases():
    """(name, uint8 map, levels, min_areas): the maps of the GPU tests, the smallest at which each step of the kernels can go wrong."""
    rng = np.random.default_rng(23)
    T = TILE
    out = [(name, m, HAND, (MIN_AREA,)) for name, (m, _) in sorted(hand_made().items())]
    for H in (T - 1, T, T + 1, 2 * T + 1):
        for W in (T - 1, T, T + 1, 2 * T + 1):
            out.append((f"cone_{H}x{W}", cone(H, W), FIFTH, (1, 69) if H == W else (5,)))
    out += [("one", np.full((1, 1), 9, np.uint8), ALL, (1, 2)), ("row", smooth(rng, 1, 300, 2), FIFTH, (1, 2, 5, 300, 301)),
            ("column", smooth(rng, 300, 1, 2), FIFTH, (2, 69))]
    comb = np.zeros((36, 67), np.uint8)        # teeth one pixel wide that fade towards the spine along the bottom: joined at the last level
    comb[:, ::2] = 1
    comb[-1] = 1
    comb *= (255 - 7 * np.arange(36)).astype(np.uint8)[:, None]
    serp = serpentine(34, 35) * (255 - 7 * np.arange(34)).astype(np.uint8)[:, None]
    out += [("comb", comb, ALL, (2, 69)), ("serpentine", serp, ALL, (5, 69))]
    n = (2 * T + 1) ** 2
    out += [("zeros", blank(), FIFTH, (1, 5)), ("full", np.full((2 * T + 1, 2 * T + 1), 255, np.uint8), FIFTH, (1, 5, n, n + 1)),
            ("sevens", np.full((T + 1, T - 1), 7, np.uint8), (200, 10, 5), (1, 2, (T + 1) * (T - 1), (T + 1) * (T - 1) + 1))]
    noise = rng.integers(0, 256, (2 * T + 1, T + 1)).astype(np.uint8)
    out += [("noise", noise, FIFTH, (1, 2, 5, 69)), ("noise_one_level", noise, (128,), (1, 2, 5)),
            ("noise_all", rng.integers(0, 256, (T + 1, T + 1)).astype(np.uint8), ALL, (2, 5)),
            ("noise_between", (noise // 4) * 4, tuple(range(254, 0, -4)), (1, 5)),                      # no level is a byte of the map
            ("smooth", smooth(rng, 2 * T + 1, 2 * T + 1), FIFTH, (1, 2, 5, 69, n, n + 1)), ("smooth_all", smooth(rng, T + 1, 2 * T + 1), ALL, (69,))]
    return out


@functools.lru_cache(maxsize=None)
def host_open(k, min_area, connectivity):
    """host_area_open of case k, computed once and shared: read only."""
    _, m, levels, _ = sweep_cases()[k]
    out = scenes.host_area_open(m, levels, min_area, connectivity)
    out.setflags(write=False)
    return out


def scipy_open(m, levels, min_area, connectivity):
    """The reference's protocol restated: binarise at every level, keep the components of at least min_area pixels, and remember the
    highest level at which a pixel was kept."""
    from scipy import ndimage
    st = ndimage.generate_binary_structure(2, 1 if connectivity == 4 else 2)
    out = np.zeros(m.shape, np.uint8)
    for t in sorted(levels, reverse=True):
        lab, n = ndimage.label(m >= t, st)
        size = np.bincount(lab.ravel(), minlength=n + 1)
        kept = (lab > 0) & (size[lab] >= min_area)
        out[kept & (out == 0)] = t
    return out


def shrinking_open(m, levels, min_area, connectivity):
    """The construction of csrc/sweep.hip: label only U = {m >= t and G == 0}; a component of U settles if it has min_area pixels or
    one of its pixels has a neighbour with G != 0."""
    H, W = m.shape
    G = np.zeros((H, W), np.uint8)
    steps = ((-1, 0), (1, 0), (0, -1), (0, 1)) + (((-1, -1), (-1, 1), (1, -1), (1, 1)) if connectivity == 8 else ())
    for t in sorted(levels, reverse=True):
        U = (m >= t) & (G == 0)
        labels, areas = scenes.host_regions(U.astype(np.uint8), connectivity)
        pad = np.pad(G != 0, 1)
        near = np.zeros((H, W), bool)
        for dy, dx in steps:
            near |= pad[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
        touched = np.zeros(H * W, bool)
        touched[labels[U & near]] = True
        settle = U & ((areas.ravel()[labels] >= min_area) | touched[labels])
        G[settle] = t
    return G


CASES = sweep_cases()
IDS = [c[0] for c in CASES]


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("k", range(len(CASES)), ids=IDS)
def test_host_area_open_equals_scipy_per_level(k, connectivity):
    pytest.importorskip("scipy.ndimage")
    _, m, levels, min_areas = CASES[k]
    for mn in min_areas:
        got = host_open(k, mn, connectivity)
        assert got.dtype == np.uint8 and got.shape == m.shape
        assert np.array_equal(got, scipy_open(m, levels, mn, connectivity)), mn


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("k", range(len(CASES)), ids=IDS)
def test_the_definition_equals_the_shrinking_set_construction(k, connectivity):
    _, m, levels, min_areas = CASES[k]
    for mn in min_areas:
        assert np.array_equal(host_open(k, mn, connectivity), shrinking_open(m, levels, mn, connectivity)), mn


def test_hand_made_cases_settle_as_their_comments_say():
    names = {c[0]: k for k, c in enumerate(CASES)}
    for name, (m, want) in hand_made().items():
        for conn, ((i, j), byte) in want.items():
            assert host_open(names[name], MIN_AREA, conn)[i, j] == byte, (name, conn)
    a, b = (host_open(names["touch_diagonal"], MIN_AREA, c) for c in (4, 8))
    assert not np.array_equal(a, b)


@pytest.mark.parametrize("connectivity", [4, 8])
def test_kept_sets_are_nested_and_recall_is_monotone(connectivity):
    names = {c[0]: k for k, c in enumerate(CASES)}
    k = names["smooth"]
    _, m, levels, _ = CASES[k]
    rng = np.random.default_rng(3)
    cls = (smooth(rng, *m.shape) > 120).astype(np.uint8)
    cls[rng.random(m.shape) < 0.05] = 9
    for mn in (1, 5, 69):
        G = host_open(k, mn, connectivity)
        assert (G <= m).all() and np.isin(G, (0,) + levels).all()
        from_levels = [scenes.host_area_open(m, (t,), mn, connectivity) > 0 for t in levels]
        for t, one, lower in zip(levels, from_levels, from_levels[1:] + [np.ones(m.shape, bool)]):
            assert np.array_equal(G >= t, one) and (lower | ~one).all()             # {G >= t} is the opening at t, inside the next one
        s = scenes.sweep_scores(scenes.host_sweep_hist(m, None if mn == 1 else G, cls, 1, 2), levels)
        assert (np.diff(s["recall"]) >= 0).all() and (np.diff(s["tp"]) >= 0).all() and (np.diff(s["fn"]) <= 0).all()
        for i, t in enumerate(levels):                                              # the suffix sums against direct counts
            kept, pred = G >= t, m >= t
            assert s["tp"][i] == (kept & (cls == 1)).sum() and s["fp"][i] == (kept & (cls == 0)).sum()
            assert s["fn"][i] == (~pred & (cls == 1)).sum() and s["removed"][i] == (pred & ~kept & (cls < 2)).sum()


def test_min_area_one_is_the_level_table():
    rng = np.random.default_rng(4)
    m = rng.integers(0, 256, (40, 50)).astype(np.uint8)
    for levels in (ALL, FIFTH, (128,), (200, 10, 5)):
        table = np.zeros(256, np.uint8)
        for t in sorted(levels):
            table[t:] = t
        for conn in (4, 8):
            assert np.array_equal(scenes.host_area_open(m, levels, 1, conn), table[m])
    assert np.array_equal(scenes.host_area_open(m, None, 1), m)


def test_sweep_scores_by_hand():
    prob = np.array([[200, 200, 100, 0],
                     [200, 50, 100, 0],
                     [0, 0, 0, 100],
                     [200, 0, 0, 0]], np.uint8)
    cls = np.array([[1, 1, 0, 0],
                    [0, 1, 1, 0],
                    [0, 0, 9, 1],
                    [1, 0, 0, 0]], np.uint8)
    levels = (200, 100, 50)
    G = scenes.host_area_open(prob, levels, 2)
    assert G.tolist() == [[200, 200, 100, 0], [200, 50, 100, 0], [0, 0, 0, 0], [0, 0, 0, 0]]
    h = scenes.host_sweep_hist(prob, G, cls, 1, 2)
    assert h.shape == (2, 2, 256) and h.dtype == np.int64 and h[0].sum() == 15 and h[1].sum() == 15
    assert h[0, 1, 200] == 3 and h[0, 0, 200] == 1 and h[1, 1, 200] == 2 and h[1, 1, 0] == 2 and h[0, 1, 100] == 2 and h[1, 1, 100] == 1
    s = scenes.sweep_scores(h, levels)
    assert s["levels"].tolist() == [200, 100, 50] and s["valid"] == 15
    assert s["tp"].tolist() == [2, 3, 4] and s["fp"].tolist() == [1, 2, 2] and s["fn"].tolist() == [3, 1, 0] and s["removed"].tolist() == [1, 2, 2]
    assert np.array_equal(s["recall"], np.array([2 / 5, 3 / 4, 1.0])) and np.array_equal(s["precision"], np.array([2 / 3, 3 / 5, 4 / 6]))
    assert np.array_equal(s["alarm_area"], np.array([3, 5, 6]) / 15) and np.array_equal(s["f1"], np.array([4 / 8, 6 / 9, 8 / 10]))
    assert s["average_precision"] == pytest.approx(2 / 5 * 2 / 3 + (3 / 4 - 2 / 5) * 3 / 5 + (1 - 3 / 4) * 4 / 6, abs=1e-15)
    empty = scenes.sweep_scores(np.zeros((2, 2, 256), np.int64), levels)                # 0 / 0 gives 0
    assert not empty["recall"].any() and not empty["precision"].any() and not empty["alarm_area"].any() and empty["average_precision"] == 0.0
    assert np.array_equal(scenes.host_sweep_hist(prob, None, cls, 1, 2)[1], h[0])
    with pytest.raises(ValueError, match="positive 2 outside 0..1"):
        scenes.host_sweep_hist(prob, None, cls, 2, 2)
    with pytest.raises(ValueError, match=r"integer \[2\]\[2\]\[256\]"):
        scenes.sweep_scores(np.zeros((2, 256)))


def test_average_precision_equals_sklearn():
    metrics = pytest.importorskip("sklearn.metrics")
    rng = np.random.default_rng(6)
    prob = np.clip(smooth(rng, 60, 70), 1, 255).astype(np.uint8)                        # every byte in 1..255: no pixel below all levels
    cls = (prob.astype(np.int64) + rng.integers(-80, 80, prob.shape) > 128).astype(np.uint8)
    s = scenes.sweep_scores(scenes.host_sweep_hist(prob, None, cls, 1, 2))
    want = metrics.average_precision_score(cls.ravel(), prob.ravel().astype(np.float64))
    assert abs(s["average_precision"] - want) <= 4 * 255 * np.finfo(np.float64).eps       # a sum of 255 terms below 1, each rounded


def test_sweep_levels_and_refusals():
    assert scenes.sweep_levels().tolist() == list(range(255, 0, -1)) and scenes.sweep_levels().dtype == np.uint8
    assert scenes.sweep_levels([0.5, 1.0, 0.001, 0.5]).tolist() == [255, 128, 1]
    assert scenes.sweep_levels([3, 200, 3, np.uint8(7)]).tolist() == [200, 7, 3]
    assert scenes.sweep_levels(np.array([0.1, 0.9])).tolist() == [230, 26] and scenes.sweep_levels(17).tolist() == [17]
    with pytest.raises(ValueError, match=r"rua_scene_area_open: T 0 outside 1..255"):
        scenes.sweep_levels([])
    with pytest.raises(ValueError, match=r"rua_scene_area_open: levels\[1\] = 0 outside 1..255"):
        scenes.sweep_levels([5, 0])
    with pytest.raises(ValueError, match=r"rua_scene_area_open: levels\[0\] = 256 outside 1..255"):
        scenes.sweep_levels([256])
    with pytest.raises(ValueError, match=r"outside \(0, 1\]"):
        scenes.sweep_levels([1.5])
    with pytest.raises(ValueError, match="min_area 0 outside 1..2147483647"):
        scenes.host_area_open(np.zeros((2, 2), np.uint8), None, 0)
    with pytest.raises(ValueError, match="connectivity 6 is neither 4 nor 8"):
        scenes.host_area_open(np.zeros((2, 2), np.uint8), None, 1, 6)
    assert scenes.sweep_params(1, 3)[0] == 1 and scenes.sweep_params(1, 3)[1].tolist() == list(ALL) and scenes.sweep_params(1, 3)[2:] == (1, 4, False)
    assert scenes.sweep_params({"positive": 0, "thresholds": [0.5], "min_area": 69, "connectivity": 8, "opened": True}, 3)[2:] == (69, 8, True)
    with pytest.raises(ValueError, match="unknown key 'area'"):
        scenes.sweep_params({"positive": 1, "area": 3}, 3)
    with pytest.raises(ValueError, match="positive 3 outside 0..2"):
        scenes.sweep_params(3, 3)
    with pytest.raises(ValueError, match="needs positive"):
        scenes.sweep_params({}, 3)


def test_cpu_pool_opened_maps_and_sweep_hist():
    rng = np.random.default_rng(8)
    shapes = [(40, 44), (33, 65), (20, 20)]
    images = [np.zeros((H, W, 3), np.uint8) for H, W in shapes]
    cls = [rng.integers(0, 4, s).astype(np.uint8) for s in shapes]
    probs = [smooth(rng, *shapes[0]), None, rng.integers(0, 256, shapes[2]).astype(np.uint8)]
    pool = scenes.ScenePool(images, cls, device="cpu")
    got = pool.opened_maps(probs, FIFTH, 5, 8)
    assert got[1] is None and all(np.array_equal(got[s], scenes.host_area_open(probs[s], FIFTH, 5, 8)) for s in (0, 2))
    h = pool.sweep_hist(probs, 1, 3, FIFTH, 5, 8)
    assert h.shape == (3, 2, 2, 256) and h.dtype == np.int64 and not h[1].any()
    assert all(np.array_equal(h[s], scenes.host_sweep_hist(probs[s], got[s], cls[s], 1, 3)) for s in (0, 2))
    h1 = pool.sweep_hist(probs, 0, 3)
    assert np.array_equal(h1[0], scenes.host_sweep_hist(probs[0], None, cls[0], 0, 3)) and np.array_equal(h1[:, 0], h1[:, 1])
    with pytest.raises(ValueError, match="needs the pool's class maps"):
        scenes.ScenePool(images, device="cpu").sweep_hist(probs, 1, 3)
    with pytest.raises(ValueError, match="2 maps for 3 scenes"):
        pool.opened_maps(probs[:2])
