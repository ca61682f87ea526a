"""Host tests of the connected regions and the sieve: scenes.host_regions against scipy.ndimage.label (the smallest index of every
component through ndimage.minimum), hand-written 5 x 5 maps for every rule of scenes.host_sieve, void mode on a binary map against
scipy's component sizes, scenes.check_sieve, the argument errors of predict_scene, the cpu pool and the command line's flags.
Bytes and integers only: every comparison is exact."""
import numpy as np
import pytest

from resunet_a_mltsk_keras_amd import scenes
from _scene_util import blob_scene


def serpentine(H=200, W=203):
    """A one-pixel path of class 1 that runs along every other row and turns at alternating ends: one region, the longest chain."""
    m = np.zeros((H, W), np.uint8)
    m[::2] = 1
    for k, i in enumerate(range(1, H, 2)):
        m[i, W - 1 if k % 2 == 0 else 0] = 1
    return m


def region_maps():
    rng = np.random.default_rng(5)
    return {"blob": blob_scene(100)[1], "blob2": blob_scene(101, 97, 260)[1], "serpentine": serpentine(),
            "noise": rng.integers(0, 4, (60, 77)).astype(np.uint8), "bytes": rng.integers(0, 256, (50, 41)).astype(np.uint8),
            "one": np.full((1, 1), 3, np.uint8), "row": rng.integers(0, 2, (1, 300)).astype(np.uint8)}


def scipy_labels(m, connectivity):
    from scipy import ndimage
    st = ndimage.generate_binary_structure(2, 1 if connectivity == 4 else 2)
    idx = np.arange(m.size, dtype=np.int64).reshape(m.shape)
    out = np.zeros(m.shape, np.int64)
    for v in np.unique(m):
        lab, n = ndimage.label(m == v, st)
        first = ndimage.minimum(idx, lab, np.arange(1, n + 1)).astype(np.int64)
        out[lab > 0] = first[lab[lab > 0] - 1]
    return out


# ---- 1. regions ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", sorted(region_maps()))
def test_host_regions_equal_scipy_label(name, connectivity):
    pytest.importorskip("scipy.ndimage")
    m = region_maps()[name]
    labels, areas = scenes.host_regions(m, connectivity)
    assert labels.dtype == np.int32 and areas.dtype == np.int32 and labels.shape == areas.shape == m.shape
    want = scipy_labels(m, connectivity)
    assert np.array_equal(labels, want)
    assert np.array_equal(areas.ravel(), np.bincount(want.ravel(), minlength=m.size))          # at the roots, 0 elsewhere
    idx = np.arange(m.size).reshape(m.shape)
    assert np.array_equal(areas > 0, labels == idx) and int(areas.sum()) == m.size


def test_host_regions_by_hand_and_counts():
    m = np.array([[0, 0, 1, 9, 9],
                  [0, 1, 1, 9, 0],
                  [2, 2, 1, 0, 0],
                  [2, 0, 2, 0, 1],
                  [0, 2, 0, 1, 1]], np.uint8)
    l4, a4 = scenes.host_regions(m, 4)
    assert l4.tolist() == [[0, 0, 2, 3, 3], [0, 2, 2, 3, 9], [10, 10, 2, 9, 9], [10, 16, 17, 9, 19], [20, 21, 22, 19, 19]]
    assert a4.ravel()[[0, 2, 3, 9, 10, 16, 17, 19, 20, 21, 22]].tolist() == [3, 4, 3, 4, 3, 1, 1, 3, 1, 1, 1] and a4.sum() == 25
    l8, _ = scenes.host_regions(m, 8)
    assert l8.tolist() == [[0, 0, 2, 3, 3], [0, 2, 2, 3, 9], [10, 10, 2, 9, 9], [10, 9, 10, 9, 19], [9, 10, 9, 19, 19]]
    # per class: regions, those below 3 pixels, their pixels; byte 9 is no class for C = 3
    assert scenes.host_region_counts(m, 3, 3, 4).tolist() == [[5, 3, 3], [2, 0, 0], [3, 2, 2]]
    assert scenes.host_region_counts(m, 3, 3, 8).tolist() == [[2, 0, 0], [2, 0, 0], [1, 0, 0]]
    assert scenes.host_region_counts(m, 1, 3, 4)[:, 1:].tolist() == [[0, 0]] * 3
    assert scenes.host_region_counts(m, 5, 10, 4)[9].tolist() == [1, 1, 3]


# ---- 2. the sieve's rules, one 5 x 5 map each -------------------------------------------------------------------------------------
def test_tie_goes_to_the_lowest_class():
    m = np.array([[2, 2, 2, 2, 2],
                  [2, 2, 2, 2, 2],
                  [1, 1, 3, 2, 2],
                  [1, 1, 1, 1, 1],
                  [1, 1, 1, 1, 1]], np.uint8)          # the 3 has two neighbours of class 2 and two of class 1
    out = scenes.host_sieve(m, 2, 4, "fill")
    assert out[2, 2] == 1 and (np.delete(out.ravel(), 12) == np.delete(m.ravel(), 12)).all()
    m[3, 2] = 2                                        # three votes against one
    assert scenes.host_sieve(m, 2, 4, "fill")[2, 2] == 2


def test_a_region_without_a_kept_neighbour_stays():
    m = (np.add.outer(np.arange(5), np.arange(5)) % 2).astype(np.uint8)   # a checkerboard: every region is one pixel
    assert np.array_equal(scenes.host_sieve(m, 2, 2, "fill"), m)          # all small, nobody kept: nothing to vote with
    assert (scenes.host_sieve(m, 2, 2, "void") == 255).all()


def test_a_class_outside_classes_donates_and_is_never_sieved():
    m = np.array([[0, 0, 0, 0, 0],
                  [0, 1, 0, 2, 0],
                  [0, 0, 0, 0, 0],
                  [0, 0, 3, 1, 0],
                  [0, 0, 0, 0, 0]], np.uint8)
    out = scenes.host_sieve(m, 2, 4, "fill", classes=(1,))
    assert out[1, 1] == 0 and out[1, 3] == 2 and out[3, 2] == 3           # only class 1 is sieved
    assert out[3, 3] == 0                                                  # votes: 0 three times, and the unsieved 3 once - it is kept
    m[2, 3], m[4, 3], m[3, 4] = 3, 3, 3                                    # now the kept class 3 has all four votes
    assert scenes.host_sieve(m, 2, 4, "fill", classes=(1,))[3, 3] == 3
    assert scenes.host_sieve(m, 2, 4, "fill", classes=())[3, 3] == 1      # no class named: the identity


def test_bytes_beyond_C_are_never_changed_and_never_donate():
    m = np.array([[7, 7, 7, 7, 7],
                  [7, 7, 1, 7, 7],
                  [7, 7, 7, 7, 0],
                  [9, 7, 7, 0, 0],
                  [7, 7, 7, 0, 2]], np.uint8)
    for mode in ("fill", "void"):
        out = scenes.host_sieve(m, 4, 4, mode)
        assert np.array_equal(out[m >= 4], m[m >= 4])                      # the single 9 stays, the 7s stay
        assert out[1, 2] == (1 if mode == "fill" else 255)                 # its neighbours are no class: no vote
        assert out[4, 4] == (0 if mode == "fill" else 255)                 # the kept 0s (4 pixels) vote
        assert np.array_equal(out[m == 0], m[m == 0])


def test_votes_are_4_adjacent_under_connectivity_8():
    m = np.array([[0, 0, 0, 0, 0],
                  [0, 2, 2, 2, 0],
                  [0, 2, 1, 2, 0],
                  [0, 2, 2, 0, 0],
                  [0, 0, 0, 3, 3]], np.uint8)
    # under 8 the 3s (2 pixels) are one region; its 4-neighbours are 0 only, though a 2 touches it diagonally
    out = scenes.host_sieve(m, 3, 4, "fill", connectivity=8)
    assert out[4, 3] == 0 and out[4, 4] == 0 and out[2, 2] == 2
    # under 8 the ring of 2s (7 pixels) and the 0s are kept; the 1 sees four 2s
    m2 = np.array([[1, 0, 0, 0, 0],
                   [0, 1, 0, 0, 0],
                   [0, 0, 2, 2, 2],
                   [0, 0, 2, 2, 2],
                   [0, 0, 2, 2, 2]], np.uint8)
    assert np.array_equal(scenes.host_sieve(m2, 2, 3, "fill", connectivity=8), m2)         # the two 1s are one region of 2 pixels
    assert scenes.host_sieve(m2, 3, 3, "fill", connectivity=8)[:2, :2].tolist() == [[0, 0], [0, 0]]
    assert scenes.host_sieve(m2, 2, 3, "fill", connectivity=4)[:2, :2].tolist() == [[0, 0], [0, 0]]


def test_min_area_1_is_the_identity_and_an_area_of_min_area_stays():
    for m in region_maps().values():
        for mode in ("fill", "void"):
            for conn in (4, 8):
                assert np.array_equal(scenes.host_sieve(m, 1, 4, mode, conn), m)
    m = np.zeros((5, 5), np.uint8)
    m[1, 1:4] = 1
    assert np.array_equal(scenes.host_sieve(m, 3, 2, "void"), m) and (scenes.host_sieve(m, 4, 2, "void")[1, 1:4] == 255).all()


def test_rounds():
    m = np.array([[0, 0, 0, 0, 0],
                  [0, 1, 1, 1, 0],
                  [0, 1, 2, 1, 0],
                  [0, 1, 1, 1, 0],
                  [0, 0, 0, 0, 0]], np.uint8)          # a speckle (2) nested in a speckle (the ring of eight 1s) on a kept ground
    one = scenes.host_sieve(m, 9, 3, "fill")
    assert one[2, 2] == 2 and (np.delete(one.ravel(), 12) == 0).all()    # round 1: the 2 has no kept neighbour, the ring goes to 0
    two = scenes.host_sieve(m, 9, 3, "fill", rounds=2)
    assert (two == 0).all()                                               # round 2: the 2 now lies in a kept region
    for r in (3, 4):
        assert np.array_equal(scenes.host_sieve(m, 9, 3, "fill", rounds=r), two)             # stable: further rounds change nothing
    assert np.array_equal(scenes.host_sieve(two, 9, 3, "fill"), two)
    blob = blob_scene(100)[1]
    stable = scenes.host_sieve(blob, 8, 4, "fill", rounds=4)
    assert np.array_equal(scenes.host_sieve(stable, 8, 4, "fill"), stable)


@pytest.mark.parametrize("connectivity", [4, 8])
def test_void_on_a_binary_map_is_an_area_opening(connectivity):
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(11)
    m = (rng.random((90, 113)) < 0.45).astype(np.uint8)
    lab, n = ndimage.label(m == 1, ndimage.generate_binary_structure(2, 1 if connectivity == 4 else 2))
    size = np.bincount(lab.ravel(), minlength=n + 1)
    for area in (2, 5, 69):
        want = m.copy()
        want[(lab > 0) & (size[lab] < area)] = 255                        # area_opening keeps size >= area; the rest leaves the score
        assert np.array_equal(scenes.host_sieve(m, area, 2, "void", connectivity, classes=(1,)), want)


# ---- 3. refusals -----------------------------------------------------------------------------------------------------------------
def test_check_sieve():
    assert scenes.check_sieve(69, 6) == (69, 6, 1, 4, 63, 1)
    assert scenes.check_sieve(np.int64(1), 64, "void", 8, (0, 63), 4) == (1, 64, 0, 8, 1 | 1 << 63, 4)
    assert scenes.check_sieve(2, 3, classes=1)[4] == 2 and scenes.check_sieve(2, 3, classes=())[4] == 0
    assert scenes.sieve_params(69, 6) == (69, 6, 1, 4, 63, 1)
    assert scenes.sieve_params({"min_area": 5, "mode": "void", "classes": [1], "rounds": 2, "connectivity": 8}, 6) == (5, 6, 0, 8, 2, 2)
    bad = [(dict(min_area=0), "min_area 0 outside 1..2147483647"), (dict(min_area=1 << 31), "min_area 2147483648 outside"),
           (dict(min_area=2.0), "min_area 2.0 outside"), (dict(min_area=True), "min_area True outside"),
           (dict(num_classes=0), "C 0 outside 1..64"), (dict(num_classes=65), "C 65 outside 1..64"),
           (dict(mode="open"), r"mode 'open' is neither void \(0\) nor fill \(1\)"), (dict(mode=1), "mode 1 is neither"),
           (dict(connectivity=6), "connectivity 6 is neither 4 nor 8"), (dict(connectivity="4"), "connectivity '4' is neither 4 nor 8"),
           (dict(classes=(6,)), "class_mask names class 6, outside 0..5"), (dict(classes=(-1,)), "class_mask names class -1"),
           (dict(classes=(1.0,)), "class_mask names class 1.0"), (dict(rounds=0), "rounds 0 outside 1..4"), (dict(rounds=5), "rounds 5 outside 1..4")]
    for kw, text in bad:
        args = dict(min_area=3, num_classes=6)
        args.update(kw)
        with pytest.raises(ValueError, match="rua_scene_sieve: " + text):
            scenes.check_sieve(**args)
    m = blob_scene(100)[1]
    with pytest.raises(ValueError, match="rua_scene_sieve: mode 'open'"):
        scenes.host_sieve(m, 3, 4, "open")
    with pytest.raises(ValueError, match="rua_scene_regions: connectivity 6"):
        scenes.host_regions(m, 6)
    with pytest.raises(ValueError, match="rua_scene_regions: min_area 0"):
        scenes.host_region_counts(m, 0, 4)
    for wrong in (m.astype(np.int32), m[0], np.zeros((0, 4), np.uint8)):
        with pytest.raises(ValueError, match="rua_scene_regions: .* uint8 H x W"):
            scenes.host_regions(wrong)
        with pytest.raises(ValueError, match="rua_scene_sieve: .* uint8 H x W"):
            scenes.host_sieve(wrong, 3, 4, "fill")
    for wrong, text in ((3.5, "sieve 3.5: None, a minimum area"), ("69", "sieve '69': None, a minimum area"), ({"mode": "void"}, "the dict needs min_area"),
                        ({"min_area": 3, "area": 4}, "unknown key 'area'"), (0, "min_area 0 outside")):
        with pytest.raises(ValueError, match=text):
            scenes.sieve_params(wrong, 6)


class _Stop(Exception):
    pass


def test_predict_scene_refuses_a_bad_sieve_before_any_work():
    """Engine.predict_scene checks `sieve` first: a stand-in for the engine that has nothing but the configuration gets as far as the
    ValueError for a bad value, and for a good one as far as the next thing predict_scene touches."""
    from types import SimpleNamespace
    from resunet_a_mltsk_keras_amd.engine import Engine

    def touched(*a, **k):
        raise _Stop()
    fake = SimpleNamespace(cfg=SimpleNamespace(input_shape=(64, 64, 3), num_classes=4), _check_map_heads=touched)
    for wrong, text in ((0, "rua_scene_sieve: min_area 0"), ({"min_area": 3, "mode": "open"}, "mode 'open'"), ({"min_area": 3, "classes": (4,)}, "class 4, outside 0..3"),
                        ({"min_area": 3, "rounds": 9}, "rounds 9"), ({"min_area": 3, "connectivity": 5}, "connectivity 5"), ("fill", "sieve 'fill'")):
        with pytest.raises(ValueError, match=text):
            Engine.predict_scene(fake, None, 0, sieve=wrong)
    with pytest.raises(_Stop):
        Engine.predict_scene(fake, None, 0, sieve={"min_area": 69, "mode": "void", "classes": (1,)})


# ---- 4. the cpu pool -------------------------------------------------------------------------------------------------------------
def test_cpu_pool_region_counts_and_sieved_maps():
    maps = [blob_scene(100)[1], blob_scene(101, 97, 260)[1]]
    images = [np.zeros(m.shape + (1,), np.uint8) for m in maps]
    pool = scenes.ScenePool(images, maps, device="cpu")
    got = pool.region_counts(min_area=8, num_classes=4)
    assert got.dtype == np.int64 and got.shape == (2, 4, 3)
    assert all(np.array_equal(got[s], scenes.host_region_counts(maps[s], 8, 4)) for s in range(2))
    other = [maps[0][::-1].copy(), None]
    some = scenes.ScenePool(images, None, device="cpu").region_counts(other, min_area=8, num_classes=4, connectivity=8)
    assert np.array_equal(some[0], scenes.host_region_counts(other[0], 8, 4, 8)) and not some[1].any()
    out = pool.sieved_maps(other, 8, 4, "fill", rounds=2)
    assert out[1] is None and np.array_equal(out[0], scenes.host_sieve(other[0], 8, 4, "fill", rounds=2))
    with pytest.raises(ValueError, match="needs maps, or the pool's class maps"):
        scenes.ScenePool(images, None, device="cpu").region_counts(min_area=8, num_classes=4)
    with pytest.raises(ValueError, match="rua_scene_sieve: 1 maps for 2 scenes"):
        pool.sieved_maps(maps[:1], 8, 4, "fill")
    with pytest.raises(ValueError, match=r"rua_scene_sieve: scene 1: the map is \(150, 171\)"):
        pool.sieved_maps([maps[0], maps[0]], 8, 4, "fill")
    with pytest.raises(ValueError, match="rua_scene_regions: C 65"):
        pool.region_counts(min_area=8, num_classes=65)


# ---- 5. the command line ---------------------------------------------------------------------------------------------------------
def test_cli_flags_and_refusals(tmp_path):
    import eval_scenes_ISPRS
    base = ["--model_path", str(tmp_path / "no_model.h5"), "--dataset_path", str(tmp_path / "no_scenes"), "--output_path", str(tmp_path / "out")]
    a = eval_scenes_ISPRS.build_parser().parse_args(base)
    assert a.sieve is None and a.sieve_mode == "fill" and a.sieve_connectivity == 4 and a.sieve_classes is None and a.sieve_rounds == 1
    a = eval_scenes_ISPRS.build_parser().parse_args(base + ["--sieve", "69", "--sieve_mode", "void", "--sieve_classes", "1", "--sieve_connectivity", "8",
                                                            "--sieve_rounds", "2"])
    assert (a.sieve, a.sieve_mode, a.sieve_classes, a.sieve_connectivity, a.sieve_rounds) == (69, "void", [1], 8, 2)
    for words, text in ((["--sieve", "0"], "min_area 0 outside 1..2147483647"), (["--sieve", "5", "--sieve_connectivity", "6"], "connectivity 6 is neither 4 nor 8"),
                        (["--sieve", "5", "--sieve_classes", "1", "9"], "class_mask names class 9"), (["--sieve", "5", "--sieve_rounds", "5"], "rounds 5 outside 1..4")):
        with pytest.raises(SystemExit) as exc:
            eval_scenes_ISPRS.main(base + words)
        assert "--sieve: rua_scene_sieve: " + text in str(exc.value)
        assert not (tmp_path / "out").exists()
