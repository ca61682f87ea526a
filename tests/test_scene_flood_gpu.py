"""rua_scene_flood on the GPU against scenes.host_flood and scenes.flood_table, bit for bit: inst, table, n and stats, on the smallest
maps at which the kernel can go wrong - one pixel, strips, sizes round a tile, several tiles -, both connectivities, level changes,
the start of the drain and the end of the schedule inside a launch, every form of the height, seeds in tile corners and on the
border, two classes, plateaus with competing ids, a corridor through every tile seam, idle maps, a capped table and none at all;
guard regions behind every output, refusals that write nothing, two runs with the same bytes; then ScenePool.instances(flood=),
predict_scene(instances={..., "flood": ...}) and the command line."""
import ctypes

import numpy as np
import pytest
import torch

from resunet_a_mltsk_keras_amd import _lib as L
from resunet_a_mltsk_keras_amd import scenes
from _scene_util import FILL, GUARD, NCLS, blob_pool, blob_scene, new_model

pytestmark = pytest.mark.gpu

S = 8                                          # FL_S of csrc/flood.hip: rounds per launch


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def guarded(a):
    """a device buffer that holds the bytes of `a` and GUARD bytes of FILL behind them"""
    raw = np.concatenate([np.ascontiguousarray(a).view(np.uint8).ravel(), np.full(GUARD, FILL, np.uint8)])
    return torch.from_numpy(raw).cuda()


def read(buf, like):
    g = buf.cpu().numpy()
    assert (g[like.nbytes:] == FILL).all(), "bytes behind a buffer were written"
    return g[:like.nbytes].view(like.dtype).reshape(like.shape).copy()


def fake_table(rng, N, cap):
    """rows with fixed columns to keep and area / box columns to overwrite"""
    t = rng.integers(-5, 1000, (min(N, cap), 8)).astype(np.int32)
    return t


def run_flood(cls, height, inst, *, C, classes, conn=4, J=1, floor=0, drain=0, table=None, N=0, cap=None, raw=False):
    """One call.  Returns (inst, table or None, n or None, stats) as the device left them; inputs and guards are checked."""
    H, W = cls.shape
    mask = sum(1 << c for c in classes)
    nwork = int(L.lib().raw("rua_scene_flood_work_bytes")(H, W))
    assert nwork == 4 * (H * W + ((H + 31) // 32) * ((W + 31) // 32))
    d_cls, d_inst = guarded(cls), guarded(inst)
    d_h = None if height is None else guarded(height)
    work = torch.full((nwork + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    stats0 = np.array([-7, -7], np.int32)
    d_stats = guarded(stats0)
    d_table = d_n = None
    if table is not None:
        cap = len(table) if cap is None else cap
        full = np.full((cap, 8), -99, np.int32)
        full[:len(table)] = table
        n0 = np.array([N, 12345], np.int32)
        d_table, d_n = guarded(full), guarded(n0)
    stride, per_class = (1, 0) if height is None or height.ndim == 2 else (height.shape[2], 1)
    L.lib().call("rua_scene_flood", d_cls.data_ptr(), None if d_h is None else d_h.data_ptr(), stride, per_class, H, W, C, mask, conn, J, floor, drain,
                 work.data_ptr(), nwork, d_inst.data_ptr(), None if d_table is None else d_table.data_ptr(), cap if table is not None else 0,
                 None if d_n is None else d_n.data_ptr(), d_stats.data_ptr(), stream())
    torch.cuda.synchronize()
    assert np.array_equal(read(d_cls, cls), cls), "the class map was written"
    if height is not None:
        assert np.array_equal(read(d_h, height), height), "the height was written"
    assert (work.cpu().numpy()[nwork:] == FILL).all(), "bytes behind the work buffer were written"
    out = (read(d_inst, inst), None if table is None else read(d_table, full), None if table is None else read(d_n, n0), read(d_stats, stats0))
    return tuple(None if a is None else a.tobytes() for a in out) if raw else out


def check(cls, height, inst, *, C, classes, conn=4, J=1, floor=0, drain=0, N=None, cap=None, seed=0, with_table=True):
    """the device against the host; returns the host's (inst, settled, last_round)"""
    want, settled, last = scenes.host_flood(cls, height, inst, num_classes=C, classes=classes, connectivity=conn, rounds_per_level=J, floor=floor, drain=drain)
    N = int(inst.max()) + 1 if N is None else N
    table = None
    if with_table:
        cap = max(N, 1) if cap is None else cap
        table = fake_table(np.random.default_rng(seed), N, cap)
    got, gtable, gn, gstats = run_flood(cls, height, inst, C=C, classes=classes, conn=conn, J=J, floor=floor, drain=drain, table=table, N=N, cap=cap)
    what = (cls.shape, conn, J, floor, drain, None if height is None else height.shape)
    assert np.array_equal(got, want), what
    assert gstats.tolist() == [settled, last], (what, gstats, settled, last)
    if with_table:
        wtable, ungrown = scenes.flood_table(want, table, cls, num_classes=C, classes=classes)
        assert np.array_equal(gtable[:len(table)], wtable), what
        assert (gtable[len(table):] == -99).all(), "table rows from min(N, max_instances) on were written"
        assert gn.tolist() == [N, ungrown], what
    return want, settled, last


def random_case(rng, H, W, kind, lo=150):
    """a blocky map of the classes 0..2 with some other bytes, sparse ids 0..5, and a height: kind 0 none, 1 [H][W], 2 [H][W][3]"""
    cls = np.kron(rng.integers(0, 3, (H // 9 + 1, W // 9 + 1)), np.ones((9, 9), np.int64))[:H, :W].astype(np.uint8)
    other = rng.random((H, W)) < 0.03
    cls[other] = rng.integers(0, 6, int(other.sum()))
    inst = np.where(rng.random((H, W)) < 0.02, rng.integers(0, 6, (H, W)), -1).astype(np.int32)
    # plateaus of equal height, the top one at 255: a schedule that ends at level 255 still has pixels to settle
    height = None if kind == 0 else np.minimum(rng.integers(lo, 264, (H, W) if kind == 1 else (H, W, 3)) // 8 * 8, 255).astype(np.uint8)
    return cls, height, inst


SHAPES = [(1, 1), (1, 70), (70, 1), (31, 33), (64, 64), (75, 70), (97, 130)]
# (connectivity, J, floor, drain): level changes fall inside a launch with J = 1, 2, 3; R = 256, 317, 468, 1, 6, 775: only the first is a multiple of S
SCHEDULES = [(4, 1, 0, 0), (8, 2, 100, 5), (4, 3, 100, 0), (8, 1, 255, 0), (4, 1, 255, 5), (8, 3, 0, 7)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_shapes_schedules_and_heights(shape):
    rng = np.random.default_rng(shape[0] * 131 + shape[1])
    for k, (conn, J, floor, drain) in enumerate(SCHEDULES):
        assert (scenes.flood_rounds(J, floor, drain) % S == 0) == (k == 0)
        cls, height, inst = random_case(rng, *shape, kind=k % 3, lo=60 if floor == 100 else 150)
        classes = [0, 1, 2] if k % 2 else [1, 2]
        _, settled, _ = check(cls, height, inst, C=3, classes=classes, conn=conn, J=J, floor=floor, drain=drain, N=6, seed=k)
        if shape == (97, 130):
            assert settled > 0, (k, "the schedule settled nothing: the case checks the idle path only")
    if shape == (1, 1):
        one = np.array([[1]], np.uint8)
        assert check(one, None, np.array([[-1]], np.int32), C=2, classes=[1], N=0)[1:] == (0, 0)
        assert check(one, None, np.array([[4]], np.int32), C=2, classes=[1], N=5)[1:] == (0, 0)


def test_seeds_in_tile_corners_and_on_the_border():
    H, W = 97, 130
    cls = np.ones((H, W), np.uint8)
    inst = np.full((H, W), -1, np.int32)
    for k, p in enumerate([(0, 0), (31, 31), (32, 32), (31, 32), (96, 129), (63, 64), (0, 129), (96, 0), (64, 127), (95, 96)]):
        inst[p] = 9 - k
    for conn in (4, 8):
        _, settled, last = check(cls, None, inst, C=2, classes=[1], conn=conn, floor=230, drain=3)            # 29 rounds: a partial fill over the seams
        assert last == 29 and 0 < settled < H * W - 10
        _, settled, last = check(cls, None, inst, C=2, classes=[1], conn=conn)                                 # and the whole map
        assert settled == H * W - 10 and last < 256


def test_two_classes_side_by_side_and_plateaus_with_competing_ids():
    H, W = 40, 75
    cls = np.ones((H, W), np.uint8)
    cls[:, 37:] = 2
    cls[20:, :] = 3 - cls[20:, :]
    inst = np.full((H, W), -1, np.int32)
    inst[5, 5], inst[5, 70], inst[35, 36], inst[35, 38], inst[19, 30] = 3, 0, 2, 1, 4
    height = np.full((H, W), 200, np.uint8)                                 # one plateau: the ids advance one pixel per round and meet
    for conn in (4, 8):
        want, settled, _ = check(cls, height, inst, C=3, classes=[1, 2], conn=conn, J=2, floor=150)
        assert settled == H * W - 5 and len(np.unique(want)) == 5
        for k, p in enumerate([(5, 5), (5, 70), (35, 36), (35, 38)]):
            assert (cls[want == want[p]] == cls[p]).all()                   # no id crossed a class border
    steps = np.full((H, W, 3), 255, np.uint8)
    steps[..., 1] = 255 - 4 * (np.arange(W)[None, :] // 6)                  # terraces six pixels wide for class 1, J = 1: each finishes at later levels
    steps[..., 2] = 255 - (np.arange(H)[:, None] // 3)
    check(cls, steps, inst, C=3, classes=[1, 2], conn=4)
    check(cls, steps, inst, C=3, classes=[2], conn=8, J=3, floor=250, drain=11)


def serpentine(n=66):
    """a corridor one pixel wide through an n x n map: every other row, joined at alternating ends"""
    cls = np.zeros((n, n), np.uint8)
    cls[::2] = 1
    for k, i in enumerate(range(1, n - 1, 2)):
        cls[i, n - 1 if k % 2 == 0 else 0] = 1
    return cls


def test_a_corridor_through_every_tile_seam():
    cls = serpentine()
    length = int(cls.sum())
    assert length == 33 * 66 + 32
    inst = np.full(cls.shape, -1, np.int32)
    inst[0, 0] = 0
    want, settled, last = check(cls, None, inst, C=2, classes=[1], floor=255, drain=2300)                      # 2301 rounds, 288 launches
    assert settled == last == length - 1 and (want[cls == 1] == 0).all()
    _, settled, last = check(cls, None, inst, C=2, classes=[1], floor=255, drain=1000)                         # cut short: last_round == R
    assert settled == last == 1001


def test_idle_maps_leave_zero_stats():
    rng = np.random.default_rng(5)
    cls, height, inst = random_case(rng, 75, 70, 1)
    none = np.full_like(inst, -1)
    assert check(cls, height, none, C=3, classes=[0, 1, 2], N=0)[1:] == (0, 0)                                 # no seed
    full = np.where(cls < 3, 2, -1).astype(np.int32)
    want, settled, last = check(cls, height, full, C=3, classes=[0, 1, 2], N=3)                                # nothing left to settle
    assert (settled, last) == (0, 0) and np.array_equal(want, full)
    assert check(cls, height, inst, C=3, classes=[], N=6)[1:] == (0, 0)                                        # no class chosen


def test_capped_table_and_no_table():
    rng = np.random.default_rng(6)
    cls, height, inst = random_case(rng, 75, 70, 2)
    check(cls, height, inst, C=3, classes=[0, 1, 2], N=6, cap=4, floor=100)                                    # ids 4 and 5 have no row
    check(cls, height, inst, C=3, classes=[0, 1, 2], N=9, cap=20, floor=100)                                   # rows without a pixel: area 0, box H, W, -1, -1
    check(cls, height, inst, C=3, classes=[0, 1, 2], floor=100, with_table=False)
    # one large instance over many tiles: the tile's dominant id is gathered in LDS
    cls = np.ones((97, 130), np.uint8)
    inst = np.full((97, 130), -1, np.int32)
    inst[50, 60], inst[0, 0] = 1, 0
    check(cls, None, inst, C=2, classes=[1], conn=8, N=2)


def test_two_runs_give_the_same_bytes():
    rng = np.random.default_rng(7)
    cls, height, inst = random_case(rng, 97, 130, 2)
    table = fake_table(rng, 6, 6)
    kw = dict(C=3, classes=[0, 1, 2], conn=8, J=2, floor=90, drain=3, table=table, N=6, raw=True)
    assert run_flood(cls, height, inst, **kw) == run_flood(cls, height, inst, **kw)


def test_refusals_write_nothing():
    H, W, C = 30, 40, 4
    nw = int(L.lib().raw("rua_scene_flood_work_bytes")(H, W))
    cls = torch.ones((H, W), dtype=torch.uint8, device="cuda")
    height = torch.zeros((H, W, C), dtype=torch.uint8, device="cuda")
    bufs = {k: torch.full((n + GUARD,), FILL, dtype=torch.uint8, device="cuda") for k, n in (("work", nw), ("inst", 4 * H * W), ("table", 320), ("n", 8), ("stats", 8))}
    p = {k: t.data_ptr() for k, t in bufs.items()}
    names = ("cls", "height", "stride", "per_class", "H", "W", "C", "mask", "conn", "J", "floor", "drain", "work", "nwork", "inst", "table", "cap", "n", "stats")
    base = dict(cls=cls.data_ptr(), height=height.data_ptr(), stride=C, per_class=1, H=H, W=W, C=C, mask=6, conn=4, J=1, floor=0, drain=0, work=p["work"], nwork=nw,
                inst=p["inst"], table=p["table"], cap=10, n=p["n"], stats=p["stats"])
    call = lambda **kw: L.lib().call("rua_scene_flood", *[{**base, **kw}[k] for k in names], stream())
    for kw, text in ((dict(cls=None), "cls, inst and stats are required"), (dict(inst=None), "cls, inst and stats are required"), (dict(stats=None), "are required"),
                     (dict(H=0), "size 0 x 40"), (dict(H=1 << 16, W=1 << 15), "size 65536 x 32768"), (dict(C=65), "C 65 outside 1..64"),
                     (dict(mask=16), "class_mask 0x10 names a class outside 0..3"), (dict(conn=5), "connectivity 5 is neither 4 nor 8"),
                     (dict(J=0), "rounds_per_level 0 outside 1..16"), (dict(J=17), "rounds_per_level 17 outside 1..16"), (dict(floor=-1), "floor -1 outside 0..255"),
                     (dict(floor=256), "floor 256 outside 0..255"), (dict(drain=-1), "drain -1 outside 0..4096"), (dict(drain=4097), "drain 4097 outside 0..4096"),
                     (dict(per_class=2), "per_class 2"), (dict(stride=0), "pix_stride 0 outside 1..256"), (dict(stride=3), "pix_stride 3 below C 4 with per_class"),
                     (dict(n=None), "n is required with a table"), (dict(cap=0), "max_instances 0 outside"), (dict(inst=p["inst"] + 2), "4-byte aligned"),
                     (dict(table=p["table"] + 1), "4-byte aligned"), (dict(stats=p["stats"] + 2), "4-byte aligned"), (dict(work=None), "work buffer is required"),
                     (dict(work=p["work"] + 1), "work buffer is required"), (dict(nwork=nw - 1), f"work_bytes {nw - 1}, the scene needs {nw}"),
                     (dict(inst=cls.data_ptr()), "inst overlaps cls|cls overlaps inst"), (dict(inst=height.data_ptr() + 8), "inst overlaps height"),
                     (dict(stats=p["inst"] + 16), "stats overlaps inst"), (dict(n=p["table"] + 316), "n overlaps table"), (dict(table=p["work"] + 64), "table overlaps work"),
                     (dict(stats=p["n"] + 4), "stats overlaps n")):
        with pytest.raises(L.RuaError, match=text):
            call(**kw)
    torch.cuda.synchronize()
    assert all((t.cpu().numpy() == FILL).all() for t in bufs.values())
    assert (cls.cpu().numpy() == 1).all() and (height.cpu().numpy() == 0).all()


# ---- ScenePool, predict_scene and the command line -------------------------------------------------------------------------------------
def test_pool_instances_with_flood_equal_the_cpu_pool():
    pool = blob_pool()
    cpu = scenes.ScenePool(pool.images, pool.class_maps, patch=64, device="cpu")
    rng = np.random.default_rng(11)
    maps = list(pool.class_maps)
    dist = [(rng.integers(0, 256, m.shape + (NCLS,)) // 16 * 16).astype(np.uint8) for m in maps]
    kw = dict(num_classes=NCLS, classes=[1, 2, 3], min_seed=2, radius=1, dist_at_least=160)
    for fl, d, conn in ((True, dist, 4), ({"rounds_per_level": 2, "floor": 0.4, "drain": 6}, dist, 8), (True, [dist[0], None], 4)):
        got = pool.instances(maps, None, d, flood=fl, connectivity=conn, **kw)
        want = cpu.instances(maps, None, d, flood=fl, connectivity=conn, **kw)
        for g, w in zip(got, want):
            assert len(g) == 5 and all(np.array_equal(a, b) for a, b in zip(g[:4], w[:4])) and g[4] == w[4]
    plain = pool.instances(maps, None, dist, **kw)
    assert all(len(t) == 4 for t in plain)
    flooded = pool.instances(maps, None, dist, flood=True, **kw)
    assert all(f[4]["settled"] == p[3] - f[3] > 0 for f, p in zip(flooded, plain))


@pytest.fixture(scope="module")
def model_and_pool():
    return new_model(), blob_pool()


PARENT_KEYS = ["gt_n", "gt_table", "inst", "match", "n", "scores", "table", "ungrown"]


def test_predict_scene_floods_before_match_and_outlines(model_and_pool):
    m, pool = model_and_pool
    base = {"classes": [1, 2, 3], "min_seed": 2, "radius": 1, "map": True}
    for extra, fl in ((dict(), True), (dict(connectivity=8), {"rounds_per_level": 2, "floor": 0.3, "drain": 4})):
        plain = m.predict_scene(pool, 0, stride=32, batch=4, heads=("dist",), instances={**base, **extra})
        res = m.predict_scene(pool, 0, stride=32, batch=4, instances={**base, **extra, "flood": fl, "outlines": True})
        before, dist, report = plain[-2], plain[-1]["dist"], res[-1]
        assert sorted(before) == PARENT_KEYS and sorted(set(report) - set(before)) == ["flood", "outlines", "outlines_true"]
        assert np.array_equal(res[0], plain[0]) and np.array_equal(res[1], plain[1])
        fp, conn = scenes.flood_params(fl), extra.get("connectivity", 4)
        inst, settled, last = scenes.host_flood(plain[0], dist, before["inst"], num_classes=NCLS, classes=[1, 2, 3], connectivity=conn,
                                                rounds_per_level=fp["rounds_per_level"], floor=fp["floor"], drain=fp["drain"])
        table, ungrown = scenes.flood_table(inst, before["table"], plain[0], num_classes=NCLS, classes=[1, 2, 3])
        print("predict_scene flood:", report["flood"], "ungrown", before["ungrown"], "->", report["ungrown"])
        assert report["flood"] == {"height": "dist", "rounds": fp["rounds"], "settled": settled, "last_round": last} and settled > 0
        assert np.array_equal(report["inst"], inst) and np.array_equal(report["table"], table) and report["ungrown"] == ungrown == before["ungrown"] - settled
        assert report["n"] == before["n"] and np.array_equal(report["gt_table"], before["gt_table"])
        # the match and the outlines read the flooded map
        gt = scenes.host_object_bank([pool.class_maps[0]], NCLS, [1, 2, 3], connectivity=conn)[0][0]
        assert np.array_equal(report["match"], scenes.host_instance_match(inst, table, gt, report["gt_n"]))
        want = scenes.host_outlines(inst, conn)
        assert np.array_equal(report["outlines"][0], want[0]) and np.array_equal(report["outlines"][1], want[1])
        off = m.predict_scene(pool, 0, stride=32, batch=4, instances={**base, **extra, "flood": None})[-1]
        assert sorted(off) == PARENT_KEYS and np.array_equal(off["inst"], before["inst"])
    # without a height: with blend= no maps of the heads are built
    kw = dict(stride=32, batch=4, blend="linear")
    plain = m.predict_scene(pool, 0, instances={**base, "bound_below": 256, "radius": 0}, **kw)
    res = m.predict_scene(pool, 0, instances={**base, "bound_below": 256, "radius": 0, "flood": True}, **kw)
    assert res[-1]["flood"]["height"] is None and res[-1]["flood"]["settled"] == 0 and np.array_equal(res[-1]["inst"], plain[-1]["inst"])


def test_cli_inst_flood(tmp_path, capsys):
    import eval_scenes_ISPRS
    sc = [blob_scene(300, 90, 70), blob_scene(301, 64, 100)]
    root, path = str(tmp_path / "scenes"), str(tmp_path / "m.h5")
    scenes.save_scene_dir(root, ["a_tile", "b_tile"], [s[0] for s in sc], [s[1] for s in sc])
    new_model(seed=11, depth=4, split_k=True).save(path)
    base = ["--use_multitasking", "--model_path", path, "--dataset_path", root, "-ps", "64", "--num_classes", str(NCLS),
            "--scene_dataset", "yes", "--stride", "32", "--batch_size", "4"]
    inst = ["--instances", "0", "1", "2", "3", "--inst_min_seed", "2", "--inst_radius", "1", "--inst_map", "yes"]
    eval_scenes_ISPRS.main(base + ["--output_path", str(tmp_path / "plain")] + inst)
    assert "the flood settled" not in capsys.readouterr().out
    res = eval_scenes_ISPRS.main(base + ["--output_path", str(tmp_path / "flood"), "--inst_flood", "yes", "--inst_flood_drain", "4"] + inst)
    out = capsys.readouterr().out.splitlines()
    lines = [line for line in out if "the flood settled" in line]
    assert len(lines) == 2 and all("down the distance map" in line and "of 260)" in line for line in lines)
    total = 0
    for n in ("a_tile", "b_tile"):
        a, b = np.load(tmp_path / "plain" / f"inst_map_{n}.npy"), np.load(tmp_path / "flood" / f"inst_map_{n}.npy")
        assert ((a == b) | (a < 0)).all()                                   # a settled pixel never changes
        total += int(((a < 0) & (b >= 0)).sum())
        area = np.load(tmp_path / "flood" / f"instances_{n}.npy")[:, 2]
        assert np.array_equal(area, np.bincount(b[b >= 0], minlength=len(area)))
    assert res["flood_settled"] == total > 0
