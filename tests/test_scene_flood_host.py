"""Host tests of the flood: hand-worked maps for every rule of scenes.host_flood, host_flood against a loop over pixels and rounds
written here, the two touching discs that the bounded grow cannot separate and the flood can, scenes.flood_params and
scenes.instance_params, the C ABI's declarations and its refusals through the built library without a launch, the cpu pool and the
command line's flags.  Integers only: every comparison is exact."""
import os

import numpy as np
import pytest

from resunet_a_mltsk_keras_amd import _lib as L
from resunet_a_mltsk_keras_amd import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def flood(cls, height, inst, C=2, classes=(1,), **kw):
    cls, inst = np.asarray(cls, np.uint8), np.asarray(inst, np.int32)
    height = None if height is None else np.asarray(height, np.uint8)
    return scenes.host_flood(cls, height, inst, num_classes=C, classes=list(classes), **kw)


def loop_flood(cls, height, inst, C, classes, connectivity, J, floor, drain):
    """host_flood's definition, round by round and pixel by pixel, the whole schedule: (inst, settled, last_round)."""
    H, W = cls.shape
    cur = inst.copy()
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if connectivity == 8 else [])
    schedule = [t for t in range(255, floor - 1, -1) for _ in range(J)] + [floor] * drain

    def h(i, j):
        return 255 if height is None else int(height[i, j]) if height.ndim == 2 else int(height[i, j, cls[i, j]])
    open_ = [(i, j) for i in range(H) for j in range(W) if cls[i, j] < C and int(cls[i, j]) in classes and cur[i, j] < 0]
    settled = last = 0
    for r, t in enumerate(schedule):
        new = {}
        for i, j in open_:
            if h(i, j) < t:
                continue
            ids = [int(cur[i + dy, j + dx]) for dy, dx in steps
                   if 0 <= i + dy < H and 0 <= j + dx < W and cur[i + dy, j + dx] >= 0 and cls[i + dy, j + dx] == cls[i, j]]
            if ids:
                new[(i, j)] = min(ids)
        for (i, j), k in new.items():
            cur[i, j] = k
        if new:
            settled, last = settled + len(new), r + 1
            open_ = [p for p in open_ if p not in new]
    return cur, settled, last


# ---- 1. hand-worked cases -------------------------------------------------------------------------------------------------------------
def test_strip_with_descending_heights():
    cls = [[1] * 9]
    inst = [[7] + [-1] * 8]
    height = [[255, 254, 253, 252, 251, 250, 249, 248, 247]]
    got, settled, last = flood(cls, height, inst)
    assert got.tolist() == [[7] * 9] and (settled, last) == (8, 9)         # pixel k joins in round k (level 255 - k, index k): last_round = 9
    # heights that fall two levels per pixel: pixel k waits for level 255 - 2 k, round index 2 k
    got, settled, last = flood(cls, [[255 - 2 * k for k in range(9)]], inst)
    assert got.tolist() == [[7] * 9] and (settled, last) == (8, 17)
    # a rising height is no obstacle once the level is below the lowest pixel on the way
    got, settled, last = flood(cls, [[255, 100, 200, 200, 200, 200, 200, 200, 200]], inst)
    assert got.tolist() == [[7] * 9] and (settled, last) == (8, 156 + 7)    # pixel 1 at level 100 (round index 155), then one per round


def test_plateau_wider_than_rounds_per_level_finishes_at_later_levels():
    cls, inst, height = [[1] * 7], [[0] + [-1] * 6], [[200] * 7]
    got, settled, last = flood(cls, height, inst)                            # J = 1: one pixel per level from level 200 on
    assert got.tolist() == [[0] * 7] and (settled, last) == (6, 55 + 6)
    got, settled, last = flood(cls, height, inst, rounds_per_level=3)       # J = 3: three at level 200 (rounds 165..167), three at 199
    assert got.tolist() == [[0] * 7] and (settled, last) == (6, 165 + 6)
    got, settled, last = flood(cls, height, inst, floor=200)                # the schedule ends at level 200: one pixel only
    assert got.tolist() == [[0, 0, -1, -1, -1, -1, -1]] and (settled, last) == (1, 56)


def test_two_ids_meet_and_the_smaller_wins():
    cls = [[1] * 7]
    got, settled, last = flood(cls, None, [[5, -1, -1, -1, -1, -1, 2]])
    assert got.tolist() == [[5, 5, 5, 2, 2, 2, 2]] and (settled, last) == (5, 3)      # the middle pixel has both beside it in round 3
    got, _, _ = flood([[1, 1, 1], [1, 1, 1], [1, 1, 1]], None, [[9, -1, 4], [-1, -1, -1], [3, -1, 8]])
    # round 1: (0,1) <- min(9, 4) = 4, (1,0) <- min(9, 3) = 3, (1,2) <- min(4, 8) = 4, (2,1) <- min(3, 8) = 3; round 2: centre <- min(4, 3, 4, 3) = 3
    assert got.tolist() == [[9, 4, 4], [3, 3, 4], [3, 3, 8]]


def test_class_border_unchosen_class_and_bytes_beyond_c():
    cls = [[1, 1, 2, 2, 0, 0, 7, 1]]
    inst = [[0, -1, -1, -1, -1, 3, -1, -1]]
    got, settled, last = flood(cls, None, inst, C=3, classes=(1, 2))
    assert got.tolist() == [[0, 0, -1, -1, -1, 3, -1, -1]] and (settled, last) == (1, 1)   # class 2 has no seed, 0 is not chosen, 7 >= C
    # a settled pixel of another class is no neighbour, and what lies on unchosen pixels stays as it is
    got, _, _ = flood([[1, 2, 2]], None, [[4, -1, -1]], C=3, classes=(1, 2))
    assert got.tolist() == [[4, -1, -1]]
    got, _, _ = flood([[0, 0, 1, 1]], None, [[6, -5, 2, -7]], C=2, classes=(1,))
    assert got.tolist() == [[6, -5, 2, 2]]


def test_floor_stops_and_drain_extends():
    cls, inst = [[1] * 6], [[0] + [-1] * 5]
    height = [[255, 250, 120, 120, 99, 255]]
    got, settled, last = flood(cls, height, inst, floor=120)                # 136 rounds: pixel 1 at level 250, pixel 2 at level 120, the last round
    assert got.tolist() == [[0, 0, 0, -1, -1, -1]] and (settled, last) == (2, 136) and scenes.flood_rounds(1, 120, 0) == 136
    got, settled, last = flood(cls, height, inst, floor=121)
    assert got.tolist() == [[0, 0, -1, -1, -1, -1]] and (settled, last) == (1, 6)
    got, settled, last = flood(cls, height, inst, floor=120, drain=5)       # the drain gives pixel 3 its round; height 99 stays below the floor
    assert got.tolist() == [[0, 0, 0, 0, -1, -1]] and (settled, last) == (3, 137)
    got, settled, last = flood(cls, height, inst, floor=100)                # a lower floor does what the drain did
    assert got.tolist() == [[0, 0, 0, 0, -1, -1]] and (settled, last) == (3, 137)
    got, settled, last = flood(cls, [[255, 100, 100, 100, 100, 100]], inst, floor=100, drain=3)
    assert got.tolist() == [[0, 0, 0, 0, 0, -1]] and (settled, last) == (4, 159) and scenes.flood_rounds(1, 100, 3) == 159


def test_no_height_is_a_bfs_of_reach_r():
    cls = np.ones((1, 40), np.uint8)
    inst = np.full((1, 40), -1, np.int32)
    inst[0, 0] = 0
    for floor, drain, J in ((255, 0, 1), (250, 0, 1), (250, 7, 1), (253, 2, 3)):
        R = scenes.flood_rounds(J, floor, drain)
        got, settled, last = flood(cls, None, inst, floor=floor, drain=drain, rounds_per_level=J)
        assert got[0].tolist() == [0] * (R + 1) + [-1] * (39 - R) and (settled, last) == (R, R)
    # geodesic: round the corner of a wall of another class, not through it
    cls = np.ones((5, 5), np.uint8)
    cls[0:4, 2] = 0
    inst = np.full((5, 5), -1, np.int32)
    inst[0, 0] = 0
    got, settled, last = flood(cls, None, inst, floor=248)                  # 8 rounds: down 4, right 3 and up 1 to (3, 3) are 8 steps, (2, 3) is 9 away
    assert got[2, 3] == -1 and got[1, 3] == -1 and got[3, 3] == 0 and got[4, 4] == 0 and (got[:, 2] == -1).sum() == 4


def test_eight_and_four_connectivity_through_a_diagonal_gap():
    cls = [[1, 0], [0, 1]]
    inst = [[3, -1], [-1, -1]]
    assert flood(cls, None, inst)[0].tolist() == [[3, -1], [-1, -1]]
    assert flood(cls, None, inst, connectivity=8)[0].tolist() == [[3, -1], [-1, 3]]


# ---- 2. against the loop ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_host_flood_is_the_loop(seed):
    rng = np.random.default_rng(seed)
    H, W = int(rng.integers(1, 14)), int(rng.integers(1, 14))
    base = rng.integers(0, 3, (H // 3 + 1, W // 3 + 1))
    cls = np.kron(base, np.ones((3, 3), int))[:H, :W].astype(np.uint8)
    cls[rng.random((H, W)) < 0.1] = rng.integers(0, 5)                      # some noise, bytes beyond C among it
    inst = np.where(rng.random((H, W)) < 0.08, rng.integers(0, 6, (H, W)), -1).astype(np.int32)
    inst[cls >= 3] = -1
    kind = seed % 3
    height = None if kind == 0 else rng.integers(200, 256, (H, W) if kind == 1 else (H, W, 3)).astype(np.uint8)
    conn, J, floor, drain = (4, 8)[seed % 2], 1 + seed % 3, (200, 230, 255)[seed % 3], (0, 3, 9)[(seed // 2) % 3]
    classes = [0, 2] if seed % 2 else [0, 1, 2]
    want = loop_flood(cls, height, inst, 3, classes, conn, J, floor, drain)
    got = scenes.host_flood(cls, height, inst, num_classes=3, classes=classes, connectivity=conn, rounds_per_level=J, floor=floor, drain=drain)
    assert np.array_equal(got[0], want[0]) and got[1:] == want[1:]
    assert got[1] == int(((got[0] >= 0) & (inst < 0)).sum())


# ---- 3. two touching discs ----------------------------------------------------------------------------------------------------------------
def two_discs():
    """(cls, height [H][W], truth ids): two discs of radius 34, centres 58 apart, one class; the exact distance to the other class
    scaled to bytes; the two halves on either side of the bisector."""
    H, W = 96, 160
    yy, xx = np.mgrid[:H, :W]
    inside = ((yy - 48) ** 2 + (xx - 51) ** 2 <= 34 * 34) | ((yy - 48) ** 2 + (xx - 109) ** 2 <= 34 * 34)
    oy, ox = np.nonzero(~inside)
    d2 = np.full((H, W), 1 << 30, np.int64)
    for k0 in range(0, len(oy), 512):                                                   # exact: the minimum over every pixel outside
        d2 = np.minimum(d2, ((yy[..., None] - oy[k0:k0 + 512]) ** 2 + (xx[..., None] - ox[k0:k0 + 512]) ** 2).min(-1))
    d = np.sqrt(d2.astype(np.float64))
    height = np.rint(255.0 * d / d.max()).astype(np.uint8)
    truth = np.where(inside, (xx >= 80).astype(np.int32), -1).astype(np.int32)
    return inside.astype(np.uint8), height, truth


def test_two_discs_radius_falls_short_and_the_flood_does_not():
    cls, height, truth = two_discs()
    assert int(cls.sum()) == 7013
    marker = scenes.host_seed_map(cls, None, np.stack([height, height], -1), num_classes=2, classes=[1], dist_at_least=160)
    table_g = np.zeros((2, 8), np.int32)
    table_g[:, 1] = 1
    table_g[:, 2] = np.bincount(truth[truth >= 0], minlength=2)

    def scored(inst, table):
        match = scenes.host_instance_match(inst, table, truth, 2)
        return scenes.instance_scores(table, table_g, match, 2, 50)

    inst4, table4, n, ungrown4 = scenes.host_instances(cls, marker, num_classes=2, classes=[1], radius=4)
    assert n == 2 and ungrown4 > 3500
    sc = scored(inst4, table4)
    assert sc["tp"][1, 0] == 0 and sc["fp"][1, 0] == 2                      # neither instance reaches IoU 0.5 with its half
    inst0, table0, n, _ = scenes.host_instances(cls, marker, num_classes=2, classes=[1], radius=0)
    got, settled, last = scenes.host_flood(cls, height, inst0, num_classes=2, classes=[1])
    table, ungrown = scenes.flood_table(got, table0, cls, num_classes=2, classes=[1])
    assert ungrown == 0 and settled == 7013 - int((inst0 >= 0).sum()) and 0 < last < 256
    assert table[:, 2].sum() == 7013 and np.array_equal(table[:, [0, 1, 3]], table0[:, [0, 1, 3]])
    sc = scored(got, table)
    assert sc["tp"][1, 0] == 2 and sc["fp"][1, 0] == 0 and sc["fn"][1, 0] == 0
    differ = int((got != truth).sum())
    print("pixels off the bisector split:", differ, "of 7013; last round", last)
    assert differ <= 70                                                     # at most 1 % of the class pixels


# ---- 4. parameters ------------------------------------------------------------------------------------------------------------------------
def test_flood_params_and_instance_params():
    assert scenes.flood_params(None) is None and scenes.flood_params(False) is None
    assert scenes.flood_params(True) == dict(rounds_per_level=1, floor=0, drain=0, rounds=256) == scenes.flood_params({})
    assert scenes.flood_params({"rounds_per_level": 3, "floor": 100, "drain": 7}) == dict(rounds_per_level=3, floor=100, drain=7, rounds=475)
    assert scenes.flood_params({"floor": 0.5})["floor"] == 128 and scenes.flood_params({"floor": 1.0})["floor"] == 255
    assert scenes.flood_params({"floor": 0.0})["floor"] == 0 and scenes.flood_params({"floor": 0.2})["floor"] == 51
    bad = [(1, "flood 1: None, True or a dict of rounds_per_level, floor, drain"), ("yes", "flood 'yes'"), ({"level": 3}, "flood: unknown key 'level'"),
           ({"rounds_per_level": 0}, "rua_scene_flood: rounds_per_level 0 outside 1..16"), ({"rounds_per_level": 17}, "rounds_per_level 17 outside 1..16"),
           ({"rounds_per_level": 1.0}, "rounds_per_level 1.0 outside"), ({"floor": 256}, "rua_scene_flood: floor 256 outside 0..255"),
           ({"floor": -1}, "floor -1 outside 0..255"), ({"floor": 1.5}, "floor 1.5 outside 0..1"), ({"drain": -1}, "rua_scene_flood: drain -1 outside 0..4096"),
           ({"drain": 4097}, "drain 4097 outside 0..4096")]
    for wrong, text in bad:
        with pytest.raises(ValueError, match=text):
            scenes.flood_params(wrong)
    for wrong, text in (((65, 0), "rua_scene_flood: C 65 outside 1..64"), ((4, [4]), "rua_scene_flood: class_mask names class 4, outside 0..3"),
                        ((4, [1], 6), "rua_scene_flood: connectivity 6 is neither 4 nor 8")):
        with pytest.raises(ValueError, match=text):
            scenes.check_flood(*wrong)
    assert scenes.check_flood(4, [1, 2], 8, 2, 3, 4) == (4, 6, 8, 2, 3, 4)
    # instance_params: the key is in the result only if it was given
    assert "flood" not in scenes.instance_params(2, 4) and "flood" not in scenes.instance_params({"classes": 2, "outlines": True}, 4)
    assert scenes.instance_params({"classes": 2, "flood": True}, 4)["flood"] == dict(rounds_per_level=1, floor=0, drain=0, rounds=256)
    assert scenes.instance_params({"classes": 2, "flood": {"drain": 9}}, 4)["flood"]["rounds"] == 265
    assert scenes.instance_params({"classes": 2, "flood": None}, 4)["flood"] is None
    with pytest.raises(ValueError, match="drain 5000 outside 0..4096"):
        scenes.instance_params({"classes": 2, "flood": {"drain": 5000}}, 4)
    # host_flood's own refusals
    cls, inst = np.ones((3, 4), np.uint8), np.full((3, 4), -1, np.int32)
    for kw, text in ((dict(cls=cls.astype(np.int32)), "the class map is a non-empty uint8"), (dict(inst=inst.astype(np.int64)), "inst is a non-empty int32"),
                     (dict(inst=inst[:2]), r"inst is \(2, 4\), the class map \(3, 4\)"), (dict(height=np.zeros((3, 4, 3), np.uint8)), r"the height is None or a uint8 \[3\]\[4\]"),
                     (dict(height=np.zeros((3, 4), np.int32)), "the height is None or a uint8"), (dict(rounds_per_level=0), "rounds_per_level 0 outside 1..16")):
        args = dict(cls=cls, height=None, inst=inst)
        extra = {k: v for k, v in kw.items() if k not in args}
        args.update({k: v for k, v in kw.items() if k in args})
        with pytest.raises(ValueError, match=text):
            scenes.host_flood(args["cls"], args["height"], args["inst"], num_classes=2, classes=[1], **extra)


# ---- 5. the C ABI: declarations, and every refusal through the built library without a launch ---------------------------------------------
def test_abi_is_declared_exported_and_built():
    hdr = open(os.path.join(ROOT, "include", "rua_hip.h")).read()
    for sym in ("rua_scene_flood", "rua_scene_flood_work_bytes"):
        assert sym in L.EXPORTED_SYMBOLS and sym + "(" in hdr, sym
    from resunet_a_mltsk_keras_amd import build as B
    assert "flood.hip" in B.SOURCES
    src = open(os.path.join(ROOT, "resunet_a_mltsk_keras_amd", "csrc", "flood.hip")).read()
    assert "asm" not in src and "getenv" not in src


A = 1 << 24                                                    # fake, suitably aligned addresses, 16 MiB apart: never dereferenced
CLS, HGT, WRK, INS, TAB, NN, STA = (A * k for k in range(1, 8))


def test_flood_refusals_without_a_launch():
    lib = L.lib()
    fn, need = lib.raw("rua_scene_flood"), lib.raw("rua_scene_flood_work_bytes")
    assert need(30, 40) == 4 * (1200 + 2) and need(32, 32) == 4 * 1025 and need(33, 65) == 4 * (33 * 65 + 6) and need(6000, 6000) == 4 * (36000000 + 188 * 188)
    assert need(0, 4) == -1 and need(4, -1) == -1 and need(1 << 16, 1 << 15) == -1

    def call(cls=CLS, height=HGT, stride=4, per_class=1, H=30, W=40, C=4, mask=6, conn=4, J=1, floor=0, drain=0, work=WRK, nwork=4 * 1202, inst=INS, table=TAB,
             cap=100, n=NN, stats=STA):
        return fn(cls, height, stride, per_class, H, W, C, mask, conn, J, floor, drain, work, nwork, inst, table, cap, n, stats, None)
    cases = [(dict(cls=None), "cls, inst and stats are required"), (dict(inst=None), "cls, inst and stats are required"), (dict(stats=None), "cls, inst and stats are required"),
             (dict(H=0), "size 0 x 40"), (dict(W=-1), "size 30 x -1"), (dict(H=1 << 16, W=1 << 15), "size 65536 x 32768 (H * W < 2^31"),
             (dict(C=0), "C 0 outside 1..64"), (dict(C=65), "C 65 outside 1..64"), (dict(mask=16), "class_mask 0x10 names a class outside 0..3"),
             (dict(conn=6), "connectivity 6 is neither 4 nor 8"), (dict(J=0), "rounds_per_level 0 outside 1..16"), (dict(J=17), "rounds_per_level 17 outside 1..16"),
             (dict(floor=-1), "floor -1 outside 0..255"), (dict(floor=256), "floor 256 outside 0..255"), (dict(drain=-1), "drain -1 outside 0..4096"),
             (dict(drain=4097), "drain 4097 outside 0..4096"), (dict(per_class=2), "per_class 2 (0 or 1)"), (dict(stride=0), "pix_stride 0 outside 1..256"),
             (dict(stride=257), "pix_stride 257 outside 1..256"), (dict(stride=3), "pix_stride 3 below C 4 with per_class"), (dict(n=None), "n is required with a table"),
             (dict(cap=0), "max_instances 0 outside 1..2147483647"), (dict(cap=1 << 31), "max_instances 2147483648"), (dict(inst=INS + 2), "4-byte aligned"),
             (dict(table=TAB + 1), "4-byte aligned"), (dict(n=NN + 2), "4-byte aligned"), (dict(stats=STA + 3), "4-byte aligned"),
             (dict(work=None), "work buffer is required"), (dict(work=WRK + 2), "work buffer is required"), (dict(nwork=4807), "work_bytes 4807, the scene needs 4808"),
             (dict(inst=CLS - 4796), "cls overlaps inst"), (dict(inst=HGT + 4796), "inst overlaps height"), (dict(work=INS - 4804), "inst overlaps work"),
             (dict(table=INS + 4796), "table overlaps inst"), (dict(n=TAB + 3196), "n overlaps table"), (dict(stats=NN + 4), "stats overlaps n"),
             (dict(stats=WRK + 4804), "stats overlaps work"), (dict(stats=INS), "overlaps")]
    for change, text in cases:
        assert call(**change) == -1, change
        last = lib.dll.rua_last_error().decode()
        assert last.startswith("rua_scene_flood: ") and text in last, (change, last)


# ---- 6. the cpu pool and the command line ----------------------------------------------------------------------------------------------
def test_cpu_pool_instances_with_flood():
    from _scene_util import blob_scene
    maps = [blob_scene(100)[1], blob_scene(101, 97, 260)[1]]
    images = [np.zeros(m.shape + (1,), np.uint8) for m in maps]
    pool = scenes.ScenePool(images, maps, device="cpu")
    rng = np.random.default_rng(9)
    dist = [rng.integers(0, 256, m.shape + (4,)).astype(np.uint8) for m in maps]
    kw = dict(num_classes=4, classes=[1, 2], min_seed=2, radius=1, dist_at_least=128)
    plain = pool.instances(maps, None, dist, **kw)
    assert all(len(t) == 4 for t in plain)
    for fl, height in ((True, dist), ({"floor": 0.5, "drain": 3, "rounds_per_level": 2}, dist), (True, None)):
        fp = scenes.flood_params(fl)
        got = pool.instances(maps, None, dist, flood=fl, **kw) if height is not None else \
            pool.instances(maps, flood=fl, num_classes=4, classes=[1, 2], min_seed=2, radius=1)
        for s, m in enumerate(maps):
            base = plain[s] if height is not None else scenes.host_instances(m, scenes.host_seed_map(m, num_classes=4, classes=[1, 2]), num_classes=4,
                                                                              classes=[1, 2], min_seed=2, radius=1)
            inst, settled, last = scenes.host_flood(m, None if height is None else height[s], base[0], num_classes=4, classes=[1, 2],
                                                    rounds_per_level=fp["rounds_per_level"], floor=fp["floor"], drain=fp["drain"])
            table, ungrown = scenes.flood_table(inst, base[1], m, num_classes=4, classes=[1, 2])
            assert len(got[s]) == 5 and np.array_equal(got[s][0], inst) and np.array_equal(got[s][1], table) and got[s][2:4] == (base[2], ungrown)
            assert got[s][4] == {"settled": settled, "last_round": last, "rounds": fp["rounds"]}
            assert ungrown == base[3] - settled
    some = pool.instances([maps[0], None], flood=True, num_classes=4, classes=[1], radius=0, want_map=False)
    assert some[1] is None and some[0][0] is None and len(some[0]) == 5
    with pytest.raises(ValueError, match="drain 9999 outside 0..4096"):
        pool.instances(maps, flood={"drain": 9999}, num_classes=4, classes=[1])


def test_cli_flags_and_refusals(tmp_path):
    import eval_scenes_ISPRS
    base = ["--model_path", str(tmp_path / "no_model.h5"), "--dataset_path", str(tmp_path / "no_scenes"), "--output_path", str(tmp_path / "out")]
    a = eval_scenes_ISPRS.build_parser().parse_args(base)
    assert (a.inst_flood, a.inst_flood_rounds, a.inst_flood_floor, a.inst_flood_drain) == (False, 1, 0.0, 0)
    a = eval_scenes_ISPRS.build_parser().parse_args(base + ["--instances", "1"])
    assert "flood" not in eval_scenes_ISPRS.parse_instances(a)
    a = eval_scenes_ISPRS.build_parser().parse_args(base + ["--instances", "1", "--inst_flood", "yes"])
    assert eval_scenes_ISPRS.parse_instances(a)["flood"] == dict(rounds_per_level=1, floor=0.0, drain=0)
    a = eval_scenes_ISPRS.build_parser().parse_args(base + ["--instances", "1", "--inst_flood", "yes", "--inst_flood_rounds", "2", "--inst_flood_floor", "0.25",
                                                            "--inst_flood_drain", "40"])
    inst = eval_scenes_ISPRS.parse_instances(a)
    assert inst["flood"] == dict(rounds_per_level=2, floor=0.25, drain=40)
    from resunet_a_mltsk_keras_amd.scenes import instance_params
    assert instance_params(inst, 6)["flood"] == dict(rounds_per_level=2, floor=64, drain=40, rounds=2 * 192 + 40)
    for words, text in ((["--inst_flood", "yes"], "--inst_flood needs --instances"),
                        (["--instances", "1", "--inst_flood", "yes", "--inst_flood_rounds", "17"], "rounds_per_level 17 outside 1..16"),
                        (["--instances", "1", "--inst_flood", "yes", "--inst_flood_floor", "1.5"], "floor 1.5 outside 0..1"),
                        (["--instances", "1", "--inst_flood", "yes", "--inst_flood_drain", "-1"], "drain -1 outside 0..4096")):
        with pytest.raises(SystemExit) as exc:
            eval_scenes_ISPRS.main(base + words)
        assert text in str(exc.value)
        assert not (tmp_path / "out").exists()
