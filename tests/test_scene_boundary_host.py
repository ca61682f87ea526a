"""Host tests of the boundary F1: scenes.host_boundaries against a pixel loop and against scipy's erosion, host_boundary_counts
against scipy's dilation by a disc (B_c = (m == c) & ~binary_erosion(m == c, cross, border_value=1), matched with
binary_dilation(B_c(other), disc)), the properties the counts must have, boundary_scores on hand values, the refusals, the cpu
pool and the command line's refusals.  Bytes and integers only: every comparison is exact."""
import numpy as np
import pytest
from scipy import ndimage

from resunet_a_mltsk_keras_amd import scenes

SHAPES = [(1, 1), (5, 300), (300, 1), (2, 3), (75, 531)]
RADII = [0, 1, 2, 3, 7, 16]
CLASSES = [1, 5, 6, 64]
CROSS = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], bool)


def blocky(seed, H, W, C=6, region=16, sprinkle=True):
    """Uniform region x region blocks of classes 0..C-1, with a sprinkle of 255 and of the value C (both "no class")."""
    rng = np.random.default_rng(seed)
    f = rng.integers(0, C, (H // region + 1, W // region + 1)).astype(np.uint8)
    m = np.ascontiguousarray(np.kron(f, np.ones((region, region), np.uint8))[:H, :W])
    if sprinkle:
        m[rng.random(m.shape) < 0.003] = 255
        m[rng.random(m.shape) < 0.003] = C
    return m


def rolled(m, seed, C=6, noise=0.01):
    """A prediction of that kind: the map rolled by (2, 1) with `noise` of its pixels redrawn."""
    rng = np.random.default_rng(seed)
    p = np.roll(m, (2, 1), (0, 1)).copy()
    k = rng.random(p.shape) < noise
    p[k] = rng.integers(0, C, int(k.sum())).astype(np.uint8)
    return p


def disc(r):
    y, x = np.mgrid[-r:r + 1, -r:r + 1]
    return y * y + x * x <= r * r


def scipy_boundaries(m, C):
    out = np.full(m.shape, 255, np.uint8)
    for c in range(C):
        k = m == c
        out[k & ~ndimage.binary_erosion(k, CROSS, border_value=1)] = c
    return out


def scipy_counts(t, p, r, C):
    bt, bp = scipy_boundaries(t, C), scipy_boundaries(p, C)
    out = np.zeros((C, 4), np.int64)
    for c in range(C):
        kt, kp = bt == c, bp == c
        if kt.any() and kp.any():                               # the dilation of nothing is nothing
            out[c] = (kp.sum(), (kp & ndimage.binary_dilation(kt, disc(r))).sum(), kt.sum(), (kt & ndimage.binary_dilation(kp, disc(r))).sum())
        else:
            out[c] = (kp.sum(), 0, kt.sum(), 0)
    return out


def loop_boundaries(m, C):
    H, W = m.shape
    out = np.full((H, W), 255, np.uint8)
    for i in range(H):
        for j in range(W):
            nb = [(i - 1, j), (i + 1, j), (i, j - 1), (i, j + 1)]
            if m[i, j] < C and any(0 <= a < H and 0 <= b < W and m[a, b] != m[i, j] for a, b in nb):
                out[i, j] = m[i, j]
    return out


@pytest.fixture(scope="module")
def pairs():
    """{(shape, C): (class map, prediction)} for the five shapes and four class counts."""
    out = {}
    for k, (H, W) in enumerate(SHAPES):
        for C in CLASSES:
            m = blocky(100 * k + C, H, W, C=C)
            out[(H, W), C] = (m, rolled(m, 7 * k + C, C=C))
    return out


# ---- 1. the boundary image -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", CLASSES)
def test_boundaries_against_a_pixel_loop_and_scipy_erosion(pairs, C):
    for shape in SHAPES:
        for m in pairs[shape, C]:
            got = scenes.host_boundaries(m, C)
            assert got.dtype == np.uint8 and got.shape == m.shape
            assert np.array_equal(got, scipy_boundaries(m, C)), (shape, C)
            if m.size <= 1500:
                assert np.array_equal(got, loop_boundaries(m, C)), (shape, C)
    m = blocky(5, 40, 37, C=C)
    assert (m >= C).any() and np.array_equal(scenes.host_boundaries(m, C), loop_boundaries(m, C))


def test_a_single_odd_pixel_and_a_no_class_byte():
    m = np.full((9, 11), 2, np.uint8)
    m[4, 5] = 4
    b = scenes.host_boundaries(m, 6)
    assert int((b == 4).sum()) == 1 and int((b == 2).sum()) == 4 and int((b == 255).sum()) == m.size - 5
    assert b[4, 5] == 4 and b[3, 5] == b[5, 5] == b[4, 4] == b[4, 6] == 2 and b[3, 4] == 255
    m[4, 5] = 255                                               # no class: no boundary pixel itself, but its neighbours are
    b = scenes.host_boundaries(m, 6)
    assert b[4, 5] == 255 and int((b == 2).sum()) == 4
    m[4, 5] = 6                                                 # the value C is no class either
    assert np.array_equal(scenes.host_boundaries(m, 6), b)
    assert (scenes.host_boundaries(np.full((7, 5), 3, np.uint8), 6) == 255).all()             # the scene border is no boundary
    assert (scenes.host_boundaries(np.full((1, 1), 0, np.uint8), 1) == 255).all()


# ---- 2. the counts -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", RADII)
def test_counts_against_scipy_dilation(pairs, r):
    for (shape, C), (m, p) in pairs.items():
        got = scenes.host_boundary_counts(m, p, r, C)
        assert got.dtype == np.int64 and got.shape == (C, 4)
        assert np.array_equal(got, scipy_counts(m, p, r, C)), (shape, C, r)


def test_counts_properties():
    m = blocky(1, 75, 531, sprinkle=False)
    p = rolled(m, 2)
    by_r = [scenes.host_boundary_counts(m, p, r, 6) for r in range(0, 17)]
    for r, c in enumerate(by_r):
        same = scenes.host_boundary_counts(m, m, r, 6)          # pred is class_map: everything matches at every radius
        assert np.array_equal(same[:, 0], same[:, 1]) and np.array_equal(same[:, 2], same[:, 3]) and np.array_equal(same[:, 0], same[:, 2])
        swapped = scenes.host_boundary_counts(p, m, r, 6)       # exchanging the maps exchanges the column pairs
        assert np.array_equal(swapped[:, [2, 3, 0, 1]], c)
        assert (c[:, 1] <= c[:, 0]).all() and (c[:, 3] <= c[:, 2]).all()
        if r:                                                   # monotone in the radius; n does not depend on it
            assert (c[:, [1, 3]] >= by_r[r - 1][:, [1, 3]]).all() and np.array_equal(c[:, [0, 2]], by_r[0][:, [0, 2]])
    # the roll by (2, 1) puts every true edge sqrt(5) from its copy: out of reach at radius 1, in reach at radius 3
    assert any(by_r[1][c, 3] < by_r[1][c, 2] and by_r[3][c, 3] == by_r[3][c, 2] > 0 for c in range(6))
    assert (by_r[0][:, 1] < by_r[1][:, 1]).all() and (by_r[1][:, 1] < by_r[3][:, 1]).all() and (by_r[3][:, 1] < by_r[16][:, 1]).all()
    assert (by_r[3][:, 1] < by_r[3][:, 0]).any() and (by_r[3][:, 0] != by_r[3][:, 2]).any()      # the two directions differ


def test_the_edge_of_the_disc():
    for r in (1, 3, 7, 16):
        t, p = np.zeros((40, 40), np.uint8), np.zeros((40, 40), np.uint8)
        t[20, 3] = 1
        p[20 - r, 3] = 1                                        # exactly r apart along an axis: a match
        c = scenes.host_boundary_counts(t, p, r, 2)
        assert c[1].tolist() == [1, 1, 1, 1]
        p[:] = 0
        p[20 - r, 4] = 1                                        # (r, 1): r^2 + 1 > r^2, no match
        c = scenes.host_boundary_counts(t, p, r, 2)
        assert c[1].tolist() == [1, 0, 1, 0]
        assert scenes.host_boundary_counts(t, p, r - 1, 2)[1].tolist() == [1, 0, 1, 0]


# ---- 3. the scores -------------------------------------------------------------------------------------------------------------
def test_boundary_scores_on_hand_values():
    counts = np.array([[10, 5, 20, 20],      # P 50, R 100: F1 200 * 50 / 150
                       [0, 0, 0, 0],         # no boundary in either map: nan, nan, nan
                       [4, 0, 0, 0],         # predicted only: P 0, R nan, F1 0
                       [0, 0, 7, 0],         # true only: P nan, R 0, F1 0
                       [3, 0, 5, 0]], np.int64)     # both, nothing matched: P 0, R 0, F1 0
    s = scenes.boundary_scores(counts)
    assert s["precision"][0] == 50 and s["recall"][0] == 100 and s["f1"][0] == pytest.approx(2 * 50 * 100 / 150, rel=1e-15)
    assert np.isnan([s["precision"][1], s["recall"][1], s["f1"][1]]).all()
    assert s["precision"][2] == 0 and np.isnan(s["recall"][2]) and s["f1"][2] == 0
    assert np.isnan(s["precision"][3]) and s["recall"][3] == 0 and s["f1"][3] == 0
    assert s["precision"][4] == 0 and s["recall"][4] == 0 and s["f1"][4] == 0
    assert s["f1_mean"] == pytest.approx(2 * 50 * 100 / 150 / 4, rel=1e-15)
    none = scenes.boundary_scores(np.zeros((3, 4), np.int64))
    assert np.isnan(none["f1"]).all() and np.isnan(none["f1_mean"])
    summed = scenes.boundary_scores(np.stack([counts, counts, 2 * counts]))                  # several scenes: summed, then scored
    assert all(np.array_equal(summed[k], s[k], equal_nan=True) for k in ("precision", "recall", "f1")) and summed["f1_mean"] == s["f1_mean"]
    for bad in (np.zeros((3, 3), np.int64), np.zeros((3, 4)), np.zeros((4,), np.int64), np.array([[1, 2, 0, 0]]), np.array([[-1, 0, 0, 0]])):
        with pytest.raises(ValueError, match="boundary counts"):
            scenes.boundary_scores(bad)


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals():
    m = blocky(3, 20, 30)
    assert scenes.check_tolerance(None) is None and scenes.check_tolerance(0) == 0 and scenes.check_tolerance(np.int64(16)) == 16
    for bad, text in ((17, "radius 17 outside 0..16"), (-1, "radius -1 outside 0..16"), (True, "radius True is no integer"), (3.0, "radius 3.0 is no integer"), ("3", "radius '3' is no integer")):
        with pytest.raises(ValueError, match="rua_scene_boundary: " + text):
            scenes.check_tolerance(bad)
        with pytest.raises(ValueError, match="rua_scene_boundary: " + text):
            scenes.host_boundary_counts(m, m, bad, 6)
    with pytest.raises(ValueError, match="rua_scene_boundary: radius None"):
        scenes.host_boundary_counts(m, m, None, 6)
    for C in (0, 65, True, 6.0):
        with pytest.raises(ValueError, match="rua_scene_boundary: C .* outside 1..64"):
            scenes.host_boundaries(m, C)
        with pytest.raises(ValueError, match="rua_scene_boundary: C .* outside 1..64"):
            scenes.host_boundary_counts(m, m, 3, C)
    with pytest.raises(ValueError, match=r"rua_scene_boundary: the prediction map is \(20, 29\), the class map \(20, 30\)"):
        scenes.host_boundary_counts(m, m[:, :29], 3, 6)
    for bad in (m.astype(np.int32), m[0], np.zeros((0, 4), np.uint8)):
        with pytest.raises(ValueError, match="rua_scene_boundary: .* uint8 H x W"):
            scenes.host_boundaries(bad, 6)
        with pytest.raises(ValueError, match="rua_scene_boundary: .* uint8 H x W"):
            scenes.host_boundary_counts(m, bad, 3, 6)


# ---- 5. the cpu pool -----------------------------------------------------------------------------------------------------------
def test_cpu_pool_boundary_counts_and_maps():
    maps = [blocky(20 + s, H, W) for s, (H, W) in enumerate(SHAPES)]
    preds = [rolled(m, 30 + s) for s, m in enumerate(maps)]
    images = [np.zeros(m.shape + (1,), np.uint8) for m in maps]
    pool = scenes.ScenePool(images, maps, device="cpu")
    got = pool.boundary_counts(preds, 3, 6)
    assert got.dtype == np.int64 and got.shape == (5, 6, 4)
    assert all(np.array_equal(got[s], scenes.host_boundary_counts(maps[s], preds[s], 3, 6)) for s in range(5))
    some = pool.boundary_counts([preds[0], None, preds[2], None, preds[4]], 3, 6)           # None: skipped, its rows stay 0
    assert np.array_equal(some[[0, 2, 4]], got[[0, 2, 4]]) and not some[[1, 3]].any()
    bm = pool.boundary_maps(6)
    assert len(bm) == 5 and all(np.array_equal(b, scenes.host_boundaries(m, 6)) for b, m in zip(bm, maps))
    with pytest.raises(ValueError, match="class maps"):
        scenes.ScenePool(images, None, device="cpu").boundary_counts(preds, 3, 6)
    with pytest.raises(ValueError, match="class maps"):
        scenes.ScenePool(images, None, device="cpu").boundary_maps(6)
    with pytest.raises(ValueError, match="4 prediction maps for 5 scenes"):
        pool.boundary_counts(preds[:4], 3, 6)
    with pytest.raises(ValueError, match="scene 1: the prediction map is"):
        pool.boundary_counts([preds[0], preds[0]] + preds[2:], 3, 6)
    with pytest.raises(ValueError, match="radius 17 outside 0..16"):
        pool.boundary_counts(preds, 17, 6)
    with pytest.raises(ValueError, match="C 65 outside 1..64"):
        pool.boundary_counts(preds, 3, 65)


# ---- 6. the command line refuses a bad tolerance before it loads anything -------------------------------------------------------
@pytest.mark.parametrize("word,text", [("17", "radius 17 outside 0..16"), ("-1", "radius -1 outside 0..16")])
def test_cli_refuses_a_bad_tolerance_before_loading(tmp_path, word, text):
    import eval_scenes_ISPRS
    argv = ["--model_path", str(tmp_path / "no_model.h5"), "--dataset_path", str(tmp_path / "no_scenes"), "--output_path", str(tmp_path / "out"),
            "--boundary_f1", word]
    with pytest.raises(SystemExit) as exc:
        eval_scenes_ISPRS.main(argv)
    assert "--boundary_f1: rua_scene_boundary: " + text in str(exc.value)
    assert not (tmp_path / "out").exists()
    assert eval_scenes_ISPRS.build_parser().parse_args(argv[:-2]).boundary_f1 is None
