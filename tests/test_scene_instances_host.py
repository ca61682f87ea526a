"""Host tests of the instances: hand-computed maps for every rule of scenes.host_seed_map and scenes.host_instances, host_instances
against a brute-force loop over pixels and seed pixels, the identity with scenes.host_regions at radius 0, scenes.host_instance_match
against pair counting in a dict, a worked example of scenes.instance_scores, scenes.instance_params, the C ABI's declarations and its
refusals through the built library without a launch, the cpu pool and the command line's flags.  Integers only: every comparison is
exact."""
import os

import numpy as np
import pytest

from resunet_a_mltsk_keras_amd import _lib as L
from resunet_a_mltsk_keras_amd import scenes
from _scene_util import blob_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rua_scene_seed_map", "rua_scene_instances", "rua_scene_instances_work_bytes", "rua_scene_instance_match",
           "rua_scene_instance_match_work_bytes")


def brute_instances(cls, marker, C, classes, min_seed, radius, connectivity):
    """host_instances' definition, pixel by pixel over every seed pixel of the map: (inst, n, ungrown)."""
    H, W = cls.shape
    labels, areas = scenes.host_regions(marker, connectivity)
    roots = [x for x in range(H * W) if areas.ravel()[x] >= max(min_seed, 1) and marker.ravel()[x] < C]
    number = {r: k for k, r in enumerate(roots)}
    seeds = [(i, j, int(marker[i, j]), number[int(labels[i, j])]) for i in range(H) for j in range(W) if int(labels[i, j]) in number]
    inst, ungrown = np.full((H, W), -1, np.int32), 0
    for i in range(H):
        for j in range(W):
            c = int(cls[i, j])
            if c >= C or c not in classes:
                continue
            best = min((((i - y) ** 2 + (j - x) ** 2, k) for y, x, m, k in seeds if m == c and (i - y) ** 2 + (j - x) ** 2 <= radius ** 2), default=None)
            if best is None:
                ungrown += 1
            else:
                inst[i, j] = best[1]
    return inst, len(roots), ungrown


def dict_match(inst_p, table_p, inst_g, n_g):
    pairs = {}
    for P, g in zip(inst_p.ravel().tolist(), inst_g.ravel().tolist()):
        if 0 <= P < len(table_p) and 0 <= g < n_g:
            pairs[(P, g)] = pairs.get((P, g), 0) + 1
    out = np.tile(np.array([-1, 0], np.int32), (len(table_p), 1))
    for (P, g), k in pairs.items():
        if 2 * k > int(table_p[P, 2]):
            assert out[P, 0] == -1
            out[P] = (g, k)
    return out


def table_of(inst, n):
    """an instance table with the columns the match and the scores read: class 1, the area"""
    t = np.zeros((n, 8), np.int32)
    t[:, 1] = 1
    t[:, 2] = np.bincount(inst[inst >= 0], minlength=n)
    return t


# the three hand cases of the match, shared with tests/test_scene_instances_gpu.py: (inst_p, table_p, inst_g, n_g, expected)
def match_cases():
    g = np.full((6, 8), -1, np.int32)
    g[:, 0:2], g[:, 2:4], g[:, 4:6] = 0, 1, 2
    half = np.full((6, 8), -1, np.int32)
    half[0:2, 0:4] = 0                                       # four pixels on object 0, four on object 1: no majority
    half[4:6, 0:3] = 1                                       # four on object 0, two on object 1
    three = np.full((6, 8), -1, np.int32)
    three[0, 0:6] = 0                                        # two pixels on each of three objects
    three[2:5, 1:4] = 1                                      # three on object 0, six on object 1
    off = np.full((6, 8), -1, np.int32)
    off[:, 6:8] = 0                                          # entirely off every object
    off[0, 0] = 1
    return [(half, table_of(half, 2), g, 3, [[-1, 0], [0, 4]]), (three, table_of(three, 2), g, 3, [[-1, 0], [1, 6]]),
            (off, table_of(off, 2), g, 3, [[-1, 0], [0, 1]])]


# ---- 1. the rules, one small map each ----------------------------------------------------------------------------------------------
def test_the_pixel_midway_between_two_seeds_goes_to_the_lower_id():
    cls = np.ones((3, 9), np.uint8)
    marker = np.full((3, 9), 255, np.uint8)
    marker[1, 2] = marker[1, 6] = 1
    inst, table, n, ungrown = scenes.host_instances(cls, marker, num_classes=2, classes=[1], radius=2)
    assert n == 2 and inst[1].tolist() == [0, 0, 0, 0, 0, 1, 1, 1, 1] and inst[0].tolist() == [-1, 0, 0, 0, -1, 1, 1, 1, -1]
    assert ungrown == 6 and int((inst == -1).sum()) == 6            # the corners and the midway column of rows 0 and 2: 5 > 4
    assert table.tolist() == [[11, 1, 11, 1, 0, 0, 2, 4], [15, 1, 10, 1, 0, 5, 2, 8]] and table.dtype == np.int32 and inst.dtype == np.int32


def test_a_pixel_takes_the_seed_of_its_own_class_not_the_nearest_seed():
    cls = np.array([[1, 1, 1, 1, 2, 2]], np.uint8)
    marker = np.array([[1, 255, 255, 255, 2, 255]], np.uint8)
    inst, table, n, ungrown = scenes.host_instances(cls, marker, num_classes=3, classes=[1, 2], radius=3)
    assert inst.tolist() == [[0, 0, 0, 0, 1, 1]] and n == 2 and ungrown == 0          # column 3: beside the class-2 seed, three from its own
    assert table[:, 1].tolist() == [1, 2] and table[:, 2].tolist() == [4, 2]
    only1 = scenes.host_instances(cls, marker, num_classes=3, classes=[1], radius=3)
    assert only1[0].tolist() == [[0, 0, 0, 0, -1, -1]] and only1[2] == 2 and only1[3] == 0 and only1[1][1].tolist() == [4, 2, 0, 1, 1, 6, -1, -1]


def test_beyond_the_radius_below_min_seed_and_bytes_beyond_C():
    cls = np.array([[1, 1, 1, 1, 1, 1, 7, 1]], np.uint8)
    marker = np.array([[1, 1, 255, 255, 255, 255, 7, 1]], np.uint8)
    inst, table, n, ungrown = scenes.host_instances(cls, marker, num_classes=2, classes=[1], radius=2)
    assert inst.tolist() == [[0, 0, 0, 0, -1, 1, -1, 1]] and n == 2 and ungrown == 1   # column 4 is 3 from seed 0 and 3 from seed 1; 7 >= C
    inst, table, n, ungrown = scenes.host_instances(cls, marker, num_classes=2, classes=[1], radius=2, min_seed=2)
    assert inst.tolist() == [[0, 0, 0, 0, -1, -1, -1, -1]] and n == 1 and ungrown == 3  # the one-pixel seed does not exist
    assert table.tolist() == [[0, 1, 4, 2, 0, 0, 0, 3]]
    inst, _, n, ungrown = scenes.host_instances(cls, marker, num_classes=8, classes=[1, 7], radius=2)
    assert inst[0, 6] == 1 and n == 3                                                   # with C = 8 the byte 7 is a class like any other
    inst, table, n, ungrown = scenes.host_instances(cls, marker, num_classes=2, classes=[1], radius=0, max_instances=1)
    assert n == 2 and len(table) == 1 and inst.tolist() == [[0, 0, -1, -1, -1, -1, -1, 1]] and ungrown == 4   # the table is capped, the ids are not


def test_seed_map_rules():
    cls = np.array([[0, 1, 1, 2, 9, 1]], np.uint8)
    bound = np.zeros((1, 6, 3), np.uint8)
    dist = np.full((1, 6, 3), 200, np.uint8)
    bound[0, 1, 1], bound[0, 2, 2], dist[0, 5, 1], dist[0, 3, 2] = 128, 255, 99, 100
    kw = dict(num_classes=3, classes=[1, 2])
    assert scenes.host_seed_map(cls, **kw).tolist() == [[255, 1, 1, 2, 255, 1]]
    assert scenes.host_seed_map(cls, bound, **kw).tolist() == [[255, 255, 1, 2, 255, 1]]         # 128 is not below 128; the other channel does not count
    assert scenes.host_seed_map(cls, bound, bound_below=129, **kw).tolist() == [[255, 1, 1, 2, 255, 1]]
    assert scenes.host_seed_map(cls, bound, dist, dist_at_least=100, **kw).tolist() == [[255, 255, 1, 2, 255, 255]]
    assert scenes.host_seed_map(cls, None, dist, dist_at_least=101, **kw).tolist() == [[255, 1, 1, 255, 255, 255]]
    full = np.full((1, 6, 3), 255, np.uint8)
    assert scenes.host_seed_map(cls, full, bound_below=256, **kw).tolist() == [[255, 1, 1, 2, 255, 1]]   # 256 switches the test off
    assert scenes.host_seed_map(cls, num_classes=3, classes=[]).tolist() == [[255] * 6]
    for kw2, text in ((dict(bound_below=0), "bound_below 0 outside 1..256"), (dict(bound_below=257), "bound_below 257"), (dict(dist_at_least=256), "dist_at_least 256 outside 0..255"),
                      (dict(classes=[3]), "class_mask names class 3, outside 0..2"), (dict(num_classes=65), "C 65 outside 1..64")):
        args = dict(num_classes=3, classes=[1])
        args.update(kw2)
        with pytest.raises(ValueError, match="rua_scene_seed_map: " + text):
            scenes.host_seed_map(cls, **args)
    with pytest.raises(ValueError, match=r"the boundary map is a uint8 \[1\]\[6\]\[3\] map"):
        scenes.host_seed_map(cls, bound[..., :2], num_classes=3, classes=[1])


# ---- 2. against the brute-force loop, and the identity with host_regions --------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("radius,min_seed", [(0, 1), (1, 1), (3, 2), (5, 1), (16, 3)])
def test_host_instances_equal_the_brute_force_loop(radius, min_seed, connectivity):
    rng = np.random.default_rng(100 * radius + connectivity)
    for H, W in ((9, 13), (20, 17), (1, 25)):
        cls = np.kron(rng.integers(0, 4, (H // 4 + 1, W // 4 + 1)), np.ones((4, 4), np.int64))[:H, :W].astype(np.uint8)
        cls[rng.random(cls.shape) < 0.05] = 200
        marker = np.where(rng.random(cls.shape) < 0.25, cls, 255).astype(np.uint8)
        marker[rng.random(cls.shape) < 0.03] = 1                          # marker bytes that differ from the class map's
        inst, table, n, ungrown = scenes.host_instances(cls, marker, num_classes=3, classes=[0, 2], min_seed=min_seed, radius=radius, connectivity=connectivity)
        want, wn, wu = brute_instances(cls, marker, 3, (0, 2), min_seed, radius, connectivity)
        assert np.array_equal(inst, want) and (n, ungrown) == (wn, wu) and len(table) == n
        for k in range(n):
            ii, jj = np.nonzero(inst == k)
            box = [int(ii.min()), int(jj.min()), int(ii.max()), int(jj.max())] if len(ii) else [H, W, -1, -1]
            assert table[k, 2] == len(ii) and table[k, 4:].tolist() == box
        labels, areas = scenes.host_regions(marker, connectivity)
        assert np.array_equal(table[:, 3], areas.ravel()[table[:, 0]]) and np.array_equal(table[:, 1], marker.ravel()[table[:, 0]])
        assert (np.diff(table[:, 0]) > 0).all()


@pytest.mark.parametrize("connectivity", [4, 8])
def test_without_head_maps_and_at_radius_0_the_instances_are_the_regions(connectivity):
    for cls in (blob_scene(100)[1], blob_scene(101, 97, 260)[1]):
        classes = [1, 3]
        marker = scenes.host_seed_map(cls, num_classes=4, classes=classes)
        inst, table, n, ungrown = scenes.host_instances(cls, marker, num_classes=4, classes=classes, radius=0, connectivity=connectivity)
        labels, areas = scenes.host_regions(cls, connectivity)
        chosen = np.isin(cls, classes)
        roots = np.flatnonzero((areas.ravel() > 0) & chosen.ravel())
        assert n == len(roots) and ungrown == 0 and np.array_equal(table[:, 0], roots)
        assert np.array_equal(table[:, 2], areas.ravel()[roots]) and np.array_equal(table[:, 3], table[:, 2])
        assert np.array_equal(inst >= 0, chosen) and np.array_equal(table[inst[chosen], 0], labels[chosen])


# ---- 3. the match and the scores ------------------------------------------------------------------------------------------------------
def test_match_by_hand():
    for inst_p, table_p, inst_g, n_g, want in match_cases():
        got = scenes.host_instance_match(inst_p, table_p, inst_g, n_g)
        assert got.dtype == np.int32 and got.tolist() == want
        assert np.array_equal(got, dict_match(inst_p, table_p, inst_g, n_g))
    inst_p, table_p, inst_g, n_g, _ = match_cases()[0]
    assert scenes.host_instance_match(inst_p, table_p, inst_g, 0).tolist() == [[-1, 0], [-1, 0]]
    assert scenes.host_instance_match(inst_p, table_p[:0], inst_g, 3).shape == (0, 2)


def test_match_equals_pair_counting():
    rng = np.random.default_rng(3)
    cls = blob_scene(100)[1]
    g, tg, ng, _ = scenes.host_instances(cls, scenes.host_seed_map(cls, num_classes=4, classes=[0, 1, 2, 3]), num_classes=4, classes=[0, 1, 2, 3], radius=0)
    other = np.roll(cls, (2, 3), (0, 1))
    marker = np.where(rng.random(cls.shape) < 0.6, other, 255).astype(np.uint8)
    p, tp, n_p, _ = scenes.host_instances(other, marker, num_classes=4, classes=[0, 1, 2], min_seed=2, radius=3)
    got = scenes.host_instance_match(p, tp, g, ng)
    assert np.array_equal(got, dict_match(p, tp, g, ng)) and (got[:, 0] >= 0).sum() > 20 and (got[:, 0] < 0).sum() > 0
    same = scenes.host_instance_match(g, tg, g, ng)
    assert np.array_equal(same[:, 0], np.arange(ng)) and np.array_equal(same[:, 1], tg[:, 2])


def test_instance_scores_worked_example():
    # class 1: three predictions against two objects; class 2: one object, never predicted
    table_p = np.zeros((3, 8), np.int32)
    table_g = np.zeros((3, 8), np.int32)
    table_p[:, 1], table_p[:, 2] = (1, 1, 1), (10, 10, 8)
    table_g[:, 1], table_g[:, 2] = (1, 1, 2), (10, 12, 5)
    match = np.array([[0, 10], [1, 8], [-1, 0]], np.int32)          # IoU 10 / 10 = 1 and 8 / (10 + 12 - 8) = 4 / 7 = 0.571...
    sc = scenes.instance_scores(table_p, table_g, match, 3)
    assert sc["iou_percent"].tolist() == list(range(50, 100, 5))
    assert sc["tp"][1].tolist() == [2, 2, 1, 1, 1, 1, 1, 1, 1, 1] and not sc["tp"][[0, 2]].any()
    assert sc["fp"][1].tolist() == [1, 1, 2, 2, 2, 2, 2, 2, 2, 2] and sc["fn"][1].tolist() == [0, 0, 1, 1, 1, 1, 1, 1, 1, 1] and sc["fn"][2].tolist() == [1] * 10
    assert sc["n_pred"].tolist() == [0, 3, 0] and sc["n_true"].tolist() == [0, 2, 1]
    assert np.isclose(sc["precision"][1, 0], 200 / 3) and sc["recall"][1, 0] == 100 and np.isclose(sc["f1_50"][1], 80) and np.isclose(sc["f1"][1, 2], 40)
    assert np.isclose(sc["f1_mean"][1], (2 * 80 + 8 * 40) / 10) and np.isnan(sc["f1_50"][0]) and sc["f1_50"][2] == 0 and np.isnan(sc["precision"][2, 0])
    # strictness: IoU exactly 1/2 is no match at 50; a class mismatch is none at all
    table_p[0, 2], table_g[0, 2], match[0] = 10, 20, (0, 10)
    assert scenes.instance_scores(table_p, table_g, match, 3, (50,))["tp"][1].tolist() == [1]
    table_g[0, 1] = 2
    assert scenes.instance_scores(table_p, table_g, match, 3, 50)["tp"].ravel().tolist() == [0, 1, 0]
    both = scenes.sum_instance_scores([sc, sc])
    assert np.array_equal(both["tp"], 2 * sc["tp"]) and np.array_equal(both["f1"][1], sc["f1"][1]) and both["n_true"].tolist() == [0, 4, 2]
    for wrong, text in (((40,), "iou_percent 40 outside 50..99"), ((), "non-empty"), ((50, 50), "distinct"), ((55.0,), "iou_percent 55.0")):
        with pytest.raises(ValueError, match=text):
            scenes.instance_scores(table_p, table_g, match, 3, wrong)
    with pytest.raises(ValueError, match=r"match is an integer \[3\]\[2\]"):
        scenes.instance_scores(table_p, table_g, match[:2], 3)


def test_instance_params():
    p = scenes.instance_params(2, 4)
    assert p == dict(classes=(2,), mask=4, bound_below=128, dist_at_least=0, min_seed=1, radius=4, connectivity=4, iou_percent=tuple(range(50, 100, 5)),
                     max_instances=1 << 20, map=False)
    assert scenes.instance_params([3, 1], 4)["classes"] == (1, 3)
    p = scenes.instance_params({"classes": [1], "bound_below": 0.5, "dist_at_least": 0.2, "min_seed": 8, "radius": 16, "connectivity": 8,
                                "iou_percent": (50, 75), "max_instances": 10, "map": True}, 6)
    assert (p["bound_below"], p["dist_at_least"], p["min_seed"], p["radius"], p["connectivity"], p["iou_percent"], p["max_instances"], p["map"]) == \
        (128, 51, 8, 16, 8, (50, 75), 10, True)
    assert scenes.instance_params({"classes": 0, "bound_below": 256, "dist_at_least": 0.0}, 1)["bound_below"] == 256
    assert scenes.instance_params({"classes": 0, "bound_below": 0.0}, 1)["bound_below"] == 1 and scenes.instance_params({"classes": 0, "bound_below": 1.0}, 1)["bound_below"] == 255
    bad = [("1", "instances '1': None, a class index"), (1.5, "instances 1.5"), ({"radius": 3}, "the dict needs classes"), ({"classes": 1, "seed": 3}, "unknown key 'seed'"),
           (4, "class_mask names class 4, outside 0..3"), ({"classes": [1], "radius": 17}, "rua_scene_instances: radius 17 outside 0..16"),
           ({"classes": [1], "min_seed": 0}, "min_seed 0 outside"), ({"classes": [1], "connectivity": 6}, "connectivity 6 is neither 4 nor 8"),
           ({"classes": [1], "bound_below": 1.5}, "bound_below 1.5 outside 0..1"), ({"classes": [1], "bound_below": 0}, "bound_below 0 outside 1..256"),
           ({"classes": [1], "dist_at_least": 256}, "dist_at_least 256 outside 0..255"), ({"classes": [1], "max_instances": 0}, "max_instances 0 outside"),
           ({"classes": [1], "iou_percent": (30,)}, "iou_percent 30 outside 50..99")]
    for wrong, text in bad:
        with pytest.raises(ValueError, match=text):
            scenes.instance_params(wrong, 4)


class _Stop(Exception):
    pass


def test_predict_scene_refuses_bad_instances_before_any_work():
    """Engine.predict_scene checks `instances` first: a stand-in for the engine that has nothing but the configuration gets as far as
    the ValueError for a bad value, and for a good one as far as the next thing predict_scene touches."""
    from types import SimpleNamespace
    from resunet_a_mltsk_keras_amd.engine import Engine

    def touched(*a, **k):
        raise _Stop()
    for multitask in (True, False):
        fake = SimpleNamespace(cfg=SimpleNamespace(input_shape=(64, 64, 3), num_classes=4, multitasking=multitask), _check_map_heads=touched)
        for wrong, text in (("cars", "instances 'cars'"), ({"classes": [4]}, "class 4, outside 0..3"), ({"classes": [1], "radius": 20}, "radius 20 outside 0..16")):
            with pytest.raises(ValueError, match=text):
                Engine.predict_scene(fake, None, 0, instances=wrong)
        for kw in (dict(scales=(1.0, 1.5)), dict(blend="linear")):
            if multitask:
                with pytest.raises(ValueError, match="head threshold and scales or blend"):
                    Engine.predict_scene(fake, None, 0, instances=1, **kw)
            with pytest.raises(_Stop):
                Engine.predict_scene(fake, None, 0, instances={"classes": [1], "bound_below": 256}, **kw)
        if multitask:
            with pytest.raises(_Stop):
                Engine.predict_scene(fake, None, 0, instances=1)
            with pytest.raises(_Stop):
                Engine.predict_scene(fake, None, 0, instances=1, scales=(1.0,))
        else:
            with pytest.raises(ValueError, match="this model has no 'bound' head"):
                Engine.predict_scene(fake, None, 0, instances=1)
            with pytest.raises(ValueError, match="this model has no 'dist' head"):
                Engine.predict_scene(fake, None, 0, instances={"classes": 1, "bound_below": 256, "dist_at_least": 3})


# ---- 4. the C ABI: declarations, and every refusal through the built library without a launch -----------------------------------------
def test_abi_is_declared_exported_and_built():
    hdr = open(os.path.join(ROOT, "include", "rua_hip.h")).read()
    for sym in SYMBOLS:
        assert sym in L.EXPORTED_SYMBOLS and sym + "(" in hdr, sym
    from resunet_a_mltsk_keras_amd import build as B
    assert "instances.hip" in B.SOURCES
    src = open(os.path.join(ROOT, "resunet_a_mltsk_keras_amd", "csrc", "instances.hip")).read()
    assert "asm" not in src and "getenv" not in src


def _last():
    return L.lib().dll.rua_last_error().decode()


A = 1 << 24                                                    # fake, suitably aligned addresses, 16 MiB apart: never dereferenced
CLS, BND, DST, MRK, LAB, ARE, WRK, INS, TAB, NN, INS_G, MAT = (A * k for k in range(1, 13))


def test_seed_map_refusals_without_a_launch():
    fn = L.lib().raw("rua_scene_seed_map")

    def call(cls=CLS, bound=BND, dist=DST, H=30, W=40, C=4, mask=6, bb=128, da=0, marker=MRK):
        return fn(cls, bound, dist, H, W, C, mask, bb, da, marker, None)
    cases = [(dict(cls=None), "cls and marker are required"), (dict(marker=None), "cls and marker are required"), (dict(H=0), "size 0 x 40"), (dict(W=-1), "size 30 x -1"),
             (dict(H=1 << 16, W=1 << 15), "size 65536 x 32768 (H * W < 2^31"), (dict(C=0), "C 0 outside 1..64"), (dict(C=65), "C 65 outside 1..64"),
             (dict(mask=1 << 4), "class_mask 0x10 names a class outside 0..3"), (dict(bb=0), "bound_below 0 outside 1..256"), (dict(bb=257), "bound_below 257"),
             (dict(da=-1), "dist_at_least -1 outside 0..255"), (dict(da=256), "dist_at_least 256"), (dict(marker=CLS), "marker overlaps cls"),
             (dict(marker=CLS + 1199), "marker overlaps cls"), (dict(marker=BND + 4 * 1200 - 1), "marker overlaps bound"), (dict(marker=DST - 1), "marker"),
             (dict(marker=DST + 100), "overlaps")]
    for change, text in cases:
        assert call(**change) == -1, change
        assert _last().startswith("rua_scene_seed_map: ") and text in _last(), (change, _last())


def test_instances_refusals_without_a_launch():
    lib = L.lib()
    fn, need = lib.raw("rua_scene_instances"), lib.raw("rua_scene_instances_work_bytes")
    assert need(30, 40) == 4 * (1200 + 2) and need(32, 32) == 4 * 1025 and need(6000, 6000) == 4 * (36000000 + 35157)
    assert need(0, 4) == -1 and need(4, -1) == -1 and need(1 << 16, 1 << 15) == -1

    def call(cls=CLS, marker=MRK, lab=LAB, are=ARE, H=30, W=40, C=4, mask=6, ms=1, r=4, work=WRK, nwork=4 * 1202, inst=INS, table=TAB, cap=100, n=NN):
        return fn(cls, marker, lab, are, H, W, C, mask, ms, r, work, nwork, inst, table, cap, n, None)
    cases = [(dict(H=0), "size 0 x 40"), (dict(H=1 << 16, W=1 << 15), "size 65536 x 32768"), (dict(C=65), "C 65 outside 1..64"), (dict(mask=16), "class_mask 0x10"),
             (dict(ms=0), "min_seed 0 outside 1..2147483647"), (dict(ms=1 << 31), "min_seed 2147483648"), (dict(r=-1), "radius -1 outside 0..16"),
             (dict(r=17), "radius 17 outside 0..16"), (dict(cap=0), "max_instances 0 outside 1..2147483647"), (dict(cap=1 << 31), "max_instances 2147483648"),
             (dict(lab=LAB + 2), "4-byte aligned"), (dict(inst=INS + 1), "4-byte aligned"), (dict(table=TAB + 2), "4-byte aligned"), (dict(n=NN + 3), "4-byte aligned"),
             (dict(work=None), "work buffer is required"), (dict(work=WRK + 2), "work buffer is required"), (dict(nwork=4 * 1202 - 1), "work_bytes 4807, the scene needs 4808"),
             (dict(inst=LAB), "inst overlaps labels"), (dict(inst=ARE + 4796), "inst overlaps areas"), (dict(table=INS + 4796), "overlaps"),
             (dict(n=TAB + 3196), "n overlaps table"), (dict(n=TAB + 3200), None), (dict(work=MRK - 4804), "marker overlaps work"), (dict(inst=CLS - 4796), "cls overlaps inst"),
             (dict(table=WRK + 4804), "table overlaps work"), (dict(table=NN - 3196), "overlaps")]
    for key in ("cls", "marker", "lab", "are", "inst", "table", "n"):
        cases.append(({key: None}, "are required"))
    for change, text in cases:
        if text is None:
            continue                                         # a valid call: it would launch
        assert call(**change) == -1, change
        assert _last().startswith("rua_scene_instances: ") and text in _last(), (change, _last())


def test_match_refusals_without_a_launch():
    lib = L.lib()
    fn, need = lib.raw("rua_scene_instance_match"), lib.raw("rua_scene_instance_match_work_bytes")
    assert [need(10, g) for g in (0, 1, 2, 3, 1024, 1025, 1 << 17)] == [80, 80, 120, 160, 480, 520, 760] and need(0, 5) == 0
    assert need(-1, 5) == -1 and need(5, 1 << 31) == -1

    def call(inst_p=INS, area=TAB + 8, Np=10, inst_g=INS_G, Ng=7, H=30, W=40, work=WRK, nwork=200, match=MAT):
        return fn(inst_p, area, Np, inst_g, Ng, H, W, work, nwork, match, None)
    cases = [(dict(inst_p=None), "inst_p and inst_g are required"), (dict(inst_g=None), "inst_p and inst_g are required"), (dict(W=0), "size 30 x 0"),
             (dict(H=1 << 16, W=1 << 15), "size 65536 x 32768"), (dict(Np=-1), "Np -1 outside"), (dict(Ng=1 << 31), "Ng 2147483648 outside"),
             (dict(area=TAB + 9), "4-byte aligned"), (dict(match=MAT + 2), "4-byte aligned"), (dict(area=None), "are required with Np > 0"),
             (dict(match=None), "are required with Np > 0"), (dict(work=None), "are required with Np > 0"), (dict(nwork=199), "work_bytes 199, the tables need 200"),
             (dict(match=INS + 4796), "match overlaps inst_p"), (dict(match=INS_G), "match overlaps inst_g"), (dict(match=TAB + 8 + 9 * 32), "match overlaps area_p"),
             (dict(work=MAT + 76), "overlaps"), (dict(work=INS_G - 196), "inst_g overlaps work")]
    for change, text in cases:
        assert call(**change) == -1, change
        assert _last().startswith("rua_scene_instance_match: ") and text in _last(), (change, _last())
    assert call(Np=0, area=None, match=None, work=None, nwork=0) == 0          # no row to write: nothing is launched


# ---- 5. the cpu pool and the command line --------------------------------------------------------------------------------------------
def test_cpu_pool_instances_and_match():
    maps = [blob_scene(100)[1], blob_scene(101, 97, 260)[1]]
    images = [np.zeros(m.shape + (1,), np.uint8) for m in maps]
    pool = scenes.ScenePool(images, maps, device="cpu")
    rng = np.random.default_rng(9)
    bound = [rng.integers(0, 256, m.shape + (4,)).astype(np.uint8) for m in maps]
    kw = dict(num_classes=4, classes=[1, 2], min_seed=2, radius=3)
    got = pool.instances(maps, bound, **kw)
    for s, m in enumerate(maps):
        want = scenes.host_instances(m, scenes.host_seed_map(m, bound[s], num_classes=4, classes=[1, 2]), **kw)
        assert all(np.array_equal(a, b) for a, b in zip(got[s], want))
    some = pool.instances([maps[0], None], num_classes=4, classes=[1], radius=0, want_map=False)
    assert some[1] is None and some[0][0] is None and some[0][2] == len(some[0][1])
    gt = pool.instances(maps, num_classes=4, classes=[1, 2], radius=0)
    match = pool.instance_match(got[0][0], got[0][1], gt[0][0], gt[0][1])
    assert np.array_equal(match, scenes.host_instance_match(got[0][0], got[0][1], gt[0][0], gt[0][2]))
    with pytest.raises(ValueError, match=f"scene 0 holds {got[0][2]} seeds, max_instances is 3"):
        pool.instances(maps, bound, max_instances=3, **kw)
    with pytest.raises(ValueError, match="rua_scene_instances: 1 maps for 2 scenes"):
        pool.instances(maps[:1], num_classes=4, classes=[1])
    with pytest.raises(ValueError, match="rua_scene_seed_map: 1 boundary maps for 2 scenes"):
        pool.instances(maps, bound[:1], num_classes=4, classes=[1])
    with pytest.raises(ValueError, match="scene 1: the distance map is a uint8"):
        pool.instances(maps, None, [None, bound[0]], num_classes=4, classes=[1])


def test_cli_flags_and_refusals(tmp_path):
    import eval_scenes_ISPRS
    base = ["--model_path", str(tmp_path / "no_model.h5"), "--dataset_path", str(tmp_path / "no_scenes"), "--output_path", str(tmp_path / "out")]
    a = eval_scenes_ISPRS.build_parser().parse_args(base)
    assert a.instances is None and (a.inst_bound, a.inst_dist, a.inst_min_seed, a.inst_radius, a.inst_connectivity, a.inst_map) == (0.5, 0.0, 8, 4, 4, False)
    assert eval_scenes_ISPRS.parse_instances(a) is None
    a = eval_scenes_ISPRS.build_parser().parse_args(base + ["--instances", "1", "4", "--inst_bound", "1", "--inst_dist", "0.2", "--inst_min_seed", "3", "--inst_radius", "6",
                                                            "--inst_connectivity", "8", "--inst_map", "yes"])
    assert eval_scenes_ISPRS.parse_instances(a) == dict(classes=[1, 4], bound_below=256, dist_at_least=0.2, min_seed=3, radius=6, connectivity=8, map=True)
    for words, text in ((["--instances", "9"], "class_mask names class 9"), (["--instances", "1", "--inst_radius", "17"], "radius 17 outside 0..16"),
                        (["--instances", "1", "--inst_bound", "1.5"], "bound_below 1.5 outside 0..1"), (["--instances", "1", "--inst_min_seed", "0"], "min_seed 0 outside"),
                        (["--instances", "1", "--blend", "linear"], "excludes --scales and --blend"), (["--instances", "1", "--scales", "1", "1.5"], "excludes --scales and --blend")):
        with pytest.raises(SystemExit) as exc:
            eval_scenes_ISPRS.main(base + words)
        assert "--instances" in str(exc.value) and text in str(exc.value)
        assert not (tmp_path / "out").exists()
