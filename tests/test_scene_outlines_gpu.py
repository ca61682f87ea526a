"""GPU tests of the outlines: rua_scene_outline_count and rua_scene_outline_rings (csrc/outlines.hip) through the C ABI into FILL-ed
buffers with a guard region behind every output and behind the used part of the work buffer, bit for bit against
scenes.host_outlines, on the smallest maps at which a chunked numbering, strips with a halo, pointer jumping and a segmented sum
can go wrong; ScenePool.outlines; Engine.predict_scene(instances={..., "outlines": True}) and the command line on the 64 x 64 model
and the blob scenes of tests/_scene_util.py.  Integers only: every comparison is exact."""
import ctypes
import json

import numpy as np
import pytest
import torch

from resunet_a_mltsk_keras_amd import _lib as L
from resunet_a_mltsk_keras_amd import scenes
from _scene_util import FILL, GUARD, NCLS, blob_pool, blob_scene, new_model
from test_scene_outlines_host import diagonal, nested, serpentine

pytestmark = pytest.mark.gpu

CHUNK = 1024                                   # OL_CHUNK of csrc/outlines.hip: pixels, edges or rings per block of a scan


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def guarded(nbytes):
    return torch.full((nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")


def read(buf, nbytes, dtype, shape):
    g = buf.cpu().numpy()
    assert (g[nbytes:] == FILL).all(), "bytes behind an output were written"
    return g[:nbytes].view(dtype).reshape(shape).copy()


def work_bytes(H, W, E):
    return int(L.lib().raw("rua_scene_outline_work_bytes")(H, W, E))


def run_count(inst, conn):
    """rua_scene_outline_count: (the device map, the device buffer of base, base, E, V)"""
    H, W = inst.shape
    d = torch.from_numpy(np.ascontiguousarray(inst)).cuda()
    nwork = work_bytes(H, W, 0)
    assert nwork == 8 * ((H * W + CHUNK - 1) // CHUNK)
    base, n, work = guarded(4 * H * W), guarded(16), guarded(nwork)
    L.lib().call("rua_scene_outline_count", d.data_ptr(), H, W, conn, base.data_ptr(), work.data_ptr(), nwork, n.data_ptr(), stream())
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), inst), "the map was written"
    assert (work.cpu().numpy()[nwork:] == FILL).all(), "bytes behind the work buffer were written"
    E, V = read(n, 16, np.int64, (2,)).tolist()
    return d, base, read(base, 4 * H * W, np.int32, (H, W)), E, V


def run_outlines(inst, conn=4, raw=False):
    """Both calls.  Returns (rings rows 0..R-1, verts); the ring rows from R on must hold FILL.  raw: the bytes of base, rings, verts."""
    H, W = inst.shape
    d, base_buf, base, E, V = run_count(inst, conn)
    nwork = work_bytes(H, W, E)
    assert nwork >= 24 * E and 0 <= V <= E <= 4 * H * W and V % 2 == 0
    work, rings, verts, nr = guarded(nwork), guarded(24 * (V // 4)), guarded(8 * V), guarded(8)
    null = E == 0
    L.lib().call("rua_scene_outline_rings", d.data_ptr(), base_buf.data_ptr(), H, W, conn, E, V, None if null else work.data_ptr(), nwork,
                 None if null else rings.data_ptr(), None if null else verts.data_ptr(), nr.data_ptr(), stream())
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), inst), "the map was written"
    assert np.array_equal(read(base_buf, 4 * H * W, np.int32, (H, W)), base), "base was written"
    if null:
        assert (work.cpu().numpy() == FILL).all()
    assert (work.cpu().numpy()[nwork:] == FILL).all(), "bytes behind the work buffer were written"
    R = int(read(nr, 8, np.int64, (1,))[0])
    rows = read(rings, 24 * (V // 4), np.int32, (V // 4, 6))
    assert 0 <= R <= V // 4 and (rows[R:].view(np.uint8) == FILL).all(), "ring rows from R on were written"
    vs = read(verts, 8 * V, np.int32, (V, 2))
    if raw:
        return base.tobytes(), rows.tobytes(), vs.tobytes()
    return rows[:R], vs, base, E


def host_base(inst, conn):
    exists, _ = scenes._outline_edges(inst, conn)
    per = exists.reshape(-1, 4).sum(1)
    return (np.cumsum(per) - per).reshape(inst.shape).astype(np.int32), int(per.sum())


def check(inst, conns=(4, 8)):
    out = None
    for conn in conns:
        rings, verts, base, E = run_outlines(inst, conn)
        want = scenes.host_outlines(inst, conn)
        wbase, wE = host_base(inst, conn)
        assert E == wE and np.array_equal(base, wbase), (inst.shape, conn, "base")
        assert np.array_equal(rings, want[0]), (inst.shape, conn, "rings", rings[:4].tolist(), want[0][:4].tolist())
        assert np.array_equal(verts, want[1]), (inst.shape, conn, "verts", int((verts != want[1]).any(1).sum()))
        out = out or (rings, verts)
    return out


def noise(rng, H, W, lo=-1, hi=6):
    return rng.integers(lo, hi, (H, W)).astype(np.int32)


# ---- 1. the two calls against the host definition ----------------------------------------------------------------------------------
def test_one_pixel_no_object_and_one_object():
    rings, verts = check(np.zeros((1, 1), np.int32))
    assert rings.tolist() == [[0, 0, 0, 4, 1, 4]] and verts.tolist() == [[0, 1], [1, 1], [1, 0], [0, 0]]
    for empty in (np.full((1, 1), -1, np.int32), np.full((37, 53), -1, np.int32), np.full((3, 5), -(2**31), np.int32)):
        rings, verts = check(empty)
        assert rings.shape == (0, 6) and verts.shape == (0, 2)
    rings, verts = check(np.full((64, 64), 7, np.int32))
    assert rings.tolist() == [[7, 0, 0, 4, 4096, 256]]


def test_strips_round_a_power_of_two():
    for W, length in ((31, 64), (32, 66), (33, 68)):
        for m in (np.zeros((1, W), np.int32), np.zeros((W, 1), np.int32)):
            rings, verts = check(m)
            assert rings[0, 3:].tolist() == [4, W, length] and len(rings) == 1


def test_diagonal_checkerboard_and_the_nested_square():
    assert len(check(diagonal(), (4,))[0]) == 2 and check(diagonal(), (8,))[0].tolist() == [[0, 0, 0, 8, 2, 8]]
    board = np.where(np.add.outer(np.arange(6), np.arange(6)) % 2 == 0, 0, -1).astype(np.int32)
    assert len(check(board, (4,))[0]) == 18 and len(check(board, (8,))[0]) == 1 + 8          # 8: one outer ring and the eight enclosed pixels
    two = np.where(np.add.outer(np.arange(6), np.arange(6)) % 2 == 0, 3, 4).astype(np.int32)   # both colours are objects
    check(two)
    rings, verts = check(nested())
    assert rings.tolist() == [[0, 0, 0, 4, 25, 20], [0, 6, 4, 4, -9, 12], [0, 48, 8, 4, 1, 4]]


def test_a_serpentine_longer_than_a_chunk():
    m = serpentine(40, 70)
    rings, verts = check(m)
    assert len(rings) == 1 and rings[0, 5] > CHUNK and rings[0, 5] == 2 * (m >= 0).sum() + 2 and rings[0, 4] == (m >= 0).sum()
    check(serpentine(40, 70).T.copy())
    filled = np.where(m >= 0, 0, 1).astype(np.int32)                                        # the gaps are an object too: two long rings side by side
    check(filled)


def test_noise_with_many_small_rings_and_ids_in_several_pieces():
    rng = np.random.default_rng(17)
    rings, verts = check(noise(rng, 37, 53))
    assert (rings[:, 5] == 4).sum() > 100 and len(rings) > 4 * 7
    check(noise(rng, 53, 37, -2, 2))
    check(noise(rng, 8, 300, 0, 2))                                                          # no pixel without an object


def test_objects_on_chunk_seams():
    H, W = 33, 1025
    rng = np.random.default_rng(23)
    m = np.full((H, W), -1, np.int32)
    for x in range(CHUNK - 2, H * W - 2, CHUNK):                                            # a few pixels either side of every chunk seam
        m.ravel()[x:x + 4] = x // CHUNK % 3
    m[:, 1022:1025] = np.where(rng.random((H, 3)) < 0.6, 4, m[:, 1022:1025])                # and down the last columns: row ends inside chunks
    m[1:, 0] = np.where(rng.random(H - 1) < 0.6, 4, m[1:, 0])
    m[10:14, 500:520] = 5
    check(m)
    check(np.kron(rng.integers(-1, 3, (5, 129)), np.ones((7, 8), np.int64)).astype(np.int32)[:H, :W])


def test_more_chunks_than_one_pass_of_the_scan_and_ids_near_the_top():
    H, W = 520, 530                                                                          # 270 chunks of pixels, more of edges: two passes of 256
    rng = np.random.default_rng(29)
    big = 2**31 - 1
    m = np.where(rng.random((H, W)) < 0.5, big, big - 1).astype(np.int32)
    m[100:140] = np.where(rng.random((40, W)) < 0.5, -1, big - 2)
    m[200:330, 20:500] = big - 3                                                             # about 60 chunks of pixels without an edge
    rings, verts, base, E = run_outlines(m, 4)
    want = scenes.host_outlines(m, 4)
    assert np.array_equal(rings, want[0]) and np.array_equal(verts, want[1]) and np.array_equal(base, host_base(m, 4)[0])
    assert E > 256 * CHUNK and len(rings) > 8 * CHUNK and rings[:, 0].min() == big - 3 and rings[:, 0].max() == big
    check(m[:70, :90], (8,))


def test_two_runs_give_the_same_bytes():
    rng = np.random.default_rng(31)
    m = np.kron(rng.integers(-1, 4, (12, 15)), np.ones((5, 6), np.int64)).astype(np.int32)
    m[rng.random(m.shape) < 0.05] = 9
    for conn in (4, 8):
        assert run_outlines(m, conn, raw=True) == run_outlines(m, conn, raw=True)


# ---- 2. the argument checks fire before anything is written --------------------------------------------------------------------------
def test_refusals_write_nothing():
    H, W = 6, 9
    inst = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    nw0, E, V = work_bytes(H, W, 0), 2 * (H + W), 4
    nw = work_bytes(H, W, E)
    bufs = {k: guarded(n) for k, n in (("base", 4 * H * W + 8), ("work", nw), ("n", 16), ("rings", 24), ("verts", 8 * V), ("nr", 8))}
    p = {k: t.data_ptr() for k, t in bufs.items()}
    count = lambda **kw: L.lib().call("rua_scene_outline_count", *[{**dict(inst=inst.data_ptr(), H=H, W=W, conn=4, base=p["base"], work=p["work"], nwork=nw0, n=p["n"]), **kw}[k]
                                                                   for k in ("inst", "H", "W", "conn", "base", "work", "nwork", "n")], stream())
    ring = lambda **kw: L.lib().call("rua_scene_outline_rings", *[{**dict(inst=inst.data_ptr(), base=p["base"], H=H, W=W, conn=4, E=E, V=V, work=p["work"], nwork=nw,
                                                                          rings=p["rings"], verts=p["verts"], nr=p["nr"]), **kw}[k]
                                                                  for k in ("inst", "base", "H", "W", "conn", "E", "V", "work", "nwork", "rings", "verts", "nr")], stream())
    for call, kw, text in ((count, dict(H=1 << 15, W=(1 << 14) + 1), r"size 32768 x 16385 \(1 <= H, W and H \* W <= 2\^29"),
                           (count, dict(H=0), "size 0 x 9"),
                           (count, dict(conn=5), "connectivity 5 is neither 4 nor 8"),
                           (count, dict(base=p["base"] + 2), "inst and base must be 4-byte aligned"),
                           (count, dict(nwork=nw0 - 1), f"work_bytes {nw0 - 1}, the map needs {nw0}"),
                           (count, dict(base=inst.data_ptr()), "base overlaps inst"),
                           (count, dict(n=p["base"] + 8), "n overlaps base|base overlaps n"),
                           (count, dict(n=None), "inst, base and n are required"),
                           (ring, dict(H=1 << 15, W=(1 << 14) + 1), "size 32768 x 16385"),
                           (ring, dict(conn=5), "connectivity 5 is neither 4 nor 8"),
                           (ring, dict(base=p["base"] + 2), "inst, base and rings must be 4-byte aligned"),
                           (ring, dict(verts=inst.data_ptr()), "verts overlaps inst"),
                           (ring, dict(rings=p["base"] + 4), "rings overlaps base|base overlaps rings"),
                           (ring, dict(nwork=nw - 1), f"work_bytes {nw - 1}, {E} edges need {nw}"),
                           (ring, dict(work=p["work"] + 8), "16-byte aligned work buffer"),
                           (ring, dict(E=4 * H * W + 1), f"E {4 * H * W + 1} outside 0..4 H W = {4 * H * W}"),
                           (ring, dict(V=E + 2), f"V {E + 2} with E {E}"),
                           (ring, dict(V=5, verts=guarded(64).data_ptr()), f"V 5 with E {E}"),
                           (ring, dict(E=0, V=4), "V 4 with E 0"),
                           (ring, dict(rings=None), "rings and verts are required with E > 0")):
        with pytest.raises(L.RuaError, match=text):
            call(**kw)
    torch.cuda.synchronize()
    assert all((t.cpu().numpy() == FILL).all() for t in bufs.values()) and (inst.cpu().numpy() == 0).all()
    assert work_bytes(1 << 15, (1 << 14) + 1, 0) == -1 and work_bytes(0, 4, 0) == -1 and work_bytes(2, 2, 17) == -1 and work_bytes(2, 2, -1) == -1
    assert work_bytes(1 << 15, 1 << 14, 0) == 8 << 19
    count()                                                                                # and the same arguments, unchanged, pass
    ring()
    torch.cuda.synchronize()
    assert read(bufs["n"], 16, np.int64, (2,)).tolist() == [E, V] and read(bufs["rings"], 24, np.int32, (6,)).tolist() == [0, 0, 0, 4, H * W, E]


# ---- 3. ScenePool --------------------------------------------------------------------------------------------------------------------
def same_outlines(got, want):
    return got[0].dtype == np.int32 and got[1].dtype == np.int32 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_pool_outlines_equal_the_host_on_the_pools_own_maps():
    pool = blob_pool()
    with pytest.raises(ValueError, match="no object bank yet"):
        pool.outlines()
    pool.object_bank(NCLS, [1, 2, 3])
    for conn in (4, 8):
        got = pool.outlines(connectivity=conn)
        assert len(got) == 2 and all(same_outlines(g, scenes.host_outlines(m, conn)) for g, m in zip(got, pool.inst_maps)) and len(got[0][0]) > 20
    rng = np.random.default_rng(37)
    given = [noise(rng, *pool.shapes[0]), None]
    got = pool.outlines(given, 8)
    assert got[1] is None and same_outlines(got[0], scenes.host_outlines(given[0], 8))
    cpu = scenes.ScenePool(pool.images, pool.class_maps, patch=64, device="cpu")
    assert same_outlines(cpu.outlines(given)[0], pool.outlines(given)[0])
    empty = pool.outlines([np.full(pool.shapes[0], -1, np.int32), None])[0]
    assert empty[0].shape == (0, 6) and empty[1].shape == (0, 2)
    for wrong, text in (([given[0]], "1 maps for 2 scenes"), ([given[0][:5], None], "scene 0: the map is"), ([given[0].astype(np.int64), None], "int32 H x W")):
        with pytest.raises(ValueError, match=text):
            pool.outlines(wrong)
    with pytest.raises(ValueError, match="connectivity 6"):
        pool.outlines(given, 6)


# ---- 4. predict_scene(instances={..., "outlines": True}) and the command line ------------------------------------------------------
@pytest.fixture(scope="module")
def model_and_pool():
    return new_model(), blob_pool()


def test_predict_scene_outlines_equal_the_host_on_the_returned_map(model_and_pool):
    m, pool = model_and_pool
    base = {"classes": [1, 2, 3], "bound_below": 256, "min_seed": 2, "map": True}
    for extra, kw in ((dict(), dict()), (dict(connectivity=8, radius=2), dict(sieve=8))):
        plain = m.predict_scene(pool, 0, stride=32, batch=4, instances={**base, **extra}, **kw)
        res = m.predict_scene(pool, 0, stride=32, batch=4, instances={**base, **extra, "outlines": True}, **kw)
        report, before = res[-1], plain[-1]
        assert sorted(set(report) - set(before)) == ["outlines", "outlines_true"]
        conn = extra.get("connectivity", 4)
        assert same_outlines(report["outlines"], scenes.host_outlines(report["inst"], conn)) and len(report["outlines"][0]) >= report["n"] > 0
        gt = scenes.host_object_bank([pool.class_maps[0]], NCLS, [1, 2, 3], connectivity=conn)[0][0]
        assert same_outlines(report["outlines_true"], scenes.host_outlines(gt, conn))
        # without the key: what it returned before, and the other entries are the same with it
        assert np.array_equal(res[0], plain[0]) and np.array_equal(res[1], plain[1])
        assert all(np.array_equal(report[k], before[k]) for k in ("table", "gt_table", "match", "inst")) and report["n"] == before["n"]
        off = m.predict_scene(pool, 0, stride=32, batch=4, instances={**base, **extra, "outlines": False}, **kw)[-1]
        assert sorted(off) == sorted(before)
    bare = scenes.ScenePool(pool.images, None, patch=64)
    report = m.predict_scene(bare, 1, stride=32, batch=4, instances={**base, "map": False, "outlines": True})[-1]
    assert report["outlines_true"] is None and "inst" not in report and len(report["outlines"][0]) >= report["n"]
    polys = scenes.outline_polygons(*report["outlines"], table=report["table"])
    assert sum(p["area"] for p in polys) == report["table"][:, 2].sum() and {p["class"] for p in polys} <= {1, 2, 3}


def test_cli_polygons(tmp_path, capsys):
    import eval_scenes_ISPRS
    sc = [blob_scene(300, 90, 70), blob_scene(301, 64, 100)]
    root, path = str(tmp_path / "scenes"), str(tmp_path / "m.h5")
    scenes.save_scene_dir(root, ["a_tile", "b_tile"], [s[0] for s in sc], [s[1] for s in sc])
    new_model(seed=11, depth=4, split_k=True).save(path)
    base = ["--use_multitasking", "--model_path", path, "--dataset_path", root, "-ps", "64", "--num_classes", str(NCLS),
            "--scene_dataset", "yes", "--stride", "32", "--batch_size", "4"]
    with pytest.raises(SystemExit, match="--polygons needs --instances"):
        eval_scenes_ISPRS.main(base + ["--output_path", str(tmp_path / "no"), "--polygons", "yes"])
    inst = ["--instances", "0", "1", "2", "3", "--inst_bound", "1", "--inst_min_seed", "2", "--inst_radius", "3", "--inst_map", "yes"]   # no head test: objects whatever the model
    eval_scenes_ISPRS.main(base + ["--output_path", str(tmp_path / "obj")] + inst)
    capsys.readouterr()
    res = eval_scenes_ISPRS.main(base + ["--output_path", str(tmp_path / "poly"), "--polygons", "yes", "--poly_truth", "yes"] + inst)
    out = capsys.readouterr().out.splitlines()
    assert any(line.startswith("Polygons") for line in out) and "polygon_counts" in res
    total = 0
    for n in ("a_tile", "b_tile"):
        assert not (tmp_path / "obj" / f"polygons_{n}.geojson").exists()
        inst_map = np.load(tmp_path / "poly" / f"inst_map_{n}.npy")
        assert np.array_equal(inst_map, np.load(tmp_path / "obj" / f"inst_map_{n}.npy"))
        rings, verts = scenes.host_outlines(inst_map)
        with open(tmp_path / "poly" / f"polygons_{n}.geojson") as f:
            doc = json.load(f)
        assert doc["type"] == "FeatureCollection" and len(doc["features"]) == int((rings[:, 4] > 0).sum()) > 0
        assert sum(len(f["geometry"]["coordinates"]) - 1 for f in doc["features"]) == int((rings[:, 4] < 0).sum())
        assert {f["properties"]["class"] for f in doc["features"]} <= {0, 1, 2, 3}
        with open(tmp_path / "poly" / f"polygons_true_{n}.geojson") as f:
            assert len(json.load(f)["features"]) > 0
        total += len(doc["features"])
    assert int(res["polygon_counts"][:, 0].sum()) == total
    # simplified and filtered: never more features, and every ring still closed with at least four corners
    eval_scenes_ISPRS.main(base + ["--output_path", str(tmp_path / "simple"), "--polygons", "yes", "--poly_simplify", "1.5", "--poly_min_area", "6"] + inst)
    with open(tmp_path / "simple" / "polygons_a_tile.geojson") as f:
        doc = json.load(f)
    assert 0 < len(doc["features"]) and all(f["properties"]["area"] >= 6 and all(len(r) >= 5 and r[0] == r[-1] for r in f["geometry"]["coordinates"]) for f in doc["features"])
    assert not (tmp_path / "simple" / "polygons_true_a_tile.geojson").exists()
