"""GPU tests of the instances: rua_scene_seed_map, rua_scene_instances (after rua_scene_regions) and rua_scene_instance_match
(csrc/instances.hip) through the C ABI into FILL-ed buffers with a guard region behind every output, bit for bit against
scenes.host_seed_map / host_instances / host_instance_match, on the smallest maps at which a chunked numbering, a tiled search with a
halo and a bitwise majority can go wrong; ScenePool.instances / instance_match; Engine.predict_scene(instances=),
Model.evaluate_scenes and the command line on the 64 x 64 model and the blob scenes of tests/_scene_util.py.  Integers only: every
comparison is exact."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from resunet_a_mltsk_keras_amd import _lib as L
from resunet_a_mltsk_keras_amd import scenes
from _scene_util import FILL, GUARD, NCLS, blob_pool, blob_scene, new_engine, new_model
from test_scene_instances_host import match_cases

pytestmark = pytest.mark.gpu

TILE = 32                                      # IN_T of csrc/instances.hip: a block grows a TILE x TILE tile
CHUNK = 1024                                   # IN_CHUNK: pixels per block of the seed numbering; the scan takes 256 chunks per pass
C4 = 4


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def guarded(nbytes):
    return torch.full((nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")


def read(buf, nbytes, dtype, shape):
    g = buf.cpu().numpy()
    assert (g[nbytes:] == FILL).all(), "bytes behind an output were written"
    return g[:nbytes].view(dtype).reshape(shape).copy()


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ptr(t):
    return None if t is None else t.data_ptr()


def run_seed_map(cls, bound, dist, C, classes, bound_below=128, dist_at_least=0):
    H, W = cls.shape
    mask = sum(1 << c for c in classes)
    d = [dev(cls), dev(bound), dev(dist)]
    out = guarded(H * W)
    L.lib().call("rua_scene_seed_map", ptr(d[0]), ptr(d[1]), ptr(d[2]), H, W, C, mask, bound_below, dist_at_least, out.data_ptr(), stream())
    torch.cuda.synchronize()
    assert np.array_equal(d[0].cpu().numpy(), cls), "the class map was written"
    return read(out, H * W, np.uint8, (H, W))


def run_instances(cls, marker, C, classes, min_seed=1, radius=4, connectivity=4, cap=None, raw=False):
    """rua_scene_regions of the marker, then rua_scene_instances: inst, the table, n and the work buffer lie in FILL-ed buffers with a
    guard region behind each.  Returns (inst, table rows 0..min(N, cap)-1, N, ungrown); the table rows from N on must hold FILL.
    raw: the four output buffers' bytes instead (determinism)."""
    H, W = cls.shape
    cap = H * W if cap is None else cap
    mask = sum(1 << c for c in classes)
    dc, dm = dev(cls), dev(marker)
    lab, are = (torch.empty((H * W,), dtype=torch.int32, device="cuda") for _ in range(2))
    one = lambda v, t=ctypes.c_void_p: (t * 1)(v)
    L.lib().call("rua_scene_regions", one(dm.data_ptr()), one(H, ctypes.c_int32), one(W, ctypes.c_int32), 1, connectivity, one(lab.data_ptr()),
                 one(are.data_ptr()), 1, 1, None, stream())
    nwork = int(L.lib().raw("rua_scene_instances_work_bytes")(H, W))
    assert nwork == 4 * (H * W + (H * W + CHUNK - 1) // CHUNK)
    work, inst, table, n = guarded(nwork), guarded(4 * H * W), guarded(32 * cap), guarded(8)
    L.lib().call("rua_scene_instances", dc.data_ptr(), dm.data_ptr(), lab.data_ptr(), are.data_ptr(), H, W, C, mask, min_seed, radius, work.data_ptr(), nwork,
                 inst.data_ptr(), table.data_ptr(), cap, n.data_ptr(), stream())
    torch.cuda.synchronize()
    assert np.array_equal(dc.cpu().numpy(), cls) and np.array_equal(dm.cpu().numpy(), marker), "an input was written"
    assert (work.cpu().numpy()[nwork:] == FILL).all(), "bytes behind the work buffer were written"
    N, ungrown = read(n, 8, np.int32, (2,)).tolist()
    rows = read(table, 32 * cap, np.int32, (cap, 8))
    assert (rows[min(N, cap):].view(np.uint8) == FILL).all(), "table rows from N on were written"
    got = read(inst, 4 * H * W, np.int32, (H, W))
    if raw:
        return got.tobytes(), rows.tobytes(), (N, ungrown)
    return got, rows[:min(N, cap)], N, ungrown


def check_instances(cls, marker, C, classes, **kw):
    got = run_instances(cls, marker, C, classes, **kw)
    hk = dict(kw)
    if "cap" in hk:
        hk["max_instances"] = hk.pop("cap")
    want = scenes.host_instances(cls, marker, num_classes=C, classes=list(classes), **hk)
    assert np.array_equal(got[0], want[0]), (cls.shape, kw, "inst", int((got[0] != want[0]).sum()))
    assert np.array_equal(got[1], want[1]), (cls.shape, kw, "table")
    assert got[2:] == want[2:], (cls.shape, kw, got[2:], want[2:])
    return want


def run_match(inst_p, table_p, inst_g, Ng, raw=False):
    H, W = inst_p.shape
    Np = len(table_p)
    dp, dg, dt = dev(inst_p), dev(inst_g), dev(table_p) if Np else None
    nwork = int(L.lib().raw("rua_scene_instance_match_work_bytes")(Np, Ng))
    assert nwork == 4 * Np * (max(Ng - 1, 0).bit_length() + 2)
    work, match = guarded(nwork), guarded(8 * Np)
    L.lib().call("rua_scene_instance_match", dp.data_ptr(), dt.data_ptr() + 8 if Np else None, Np, dg.data_ptr(), Ng, H, W, work.data_ptr(), nwork,
                 match.data_ptr(), stream())
    torch.cuda.synchronize()
    assert np.array_equal(dp.cpu().numpy(), inst_p) and np.array_equal(dg.cpu().numpy(), inst_g) and (not Np or np.array_equal(dt.cpu().numpy(), table_p))
    assert (work.cpu().numpy()[nwork:] == FILL).all(), "bytes behind the work buffer were written"
    got = read(match, 8 * Np, np.int32, (Np, 2))
    return got.tobytes() if raw else got


def seeded(cls, rng, share, C=C4):
    """a marker: the class map's byte on a random share of 3 x 3 blocks, 255 elsewhere - seeds of a few pixels with gaps between them"""
    H, W = cls.shape
    keep = np.kron(rng.random((H // 3 + 1, W // 3 + 1)) < share, np.ones((3, 3), bool))[:H, :W]
    return np.where(keep & (cls < C), cls, 255).astype(np.uint8)


def blocky(rng, H, W, k=5, classes=3):
    m = np.kron(rng.integers(0, classes, (H // k + 1, W // k + 1)), np.ones((k, k), np.int64))[:H, :W].astype(np.uint8)
    m[rng.random(m.shape) < 0.02] = 200
    return m


def _maps():
    rng = np.random.default_rng(29)
    shapes = [(1, 1), (1, 300), (300, 1)] + [(H, W) for H in (31, 32, 33, 65) for W in (31, 32, 33, 65)] + [(70, 131)]
    out = []
    for H, W in shapes:
        cls = blocky(rng, H, W)
        out.append((cls, seeded(cls, rng, 0.3)))
    return out


MAPS = _maps()


@functools.lru_cache(maxsize=None)
def blob_with_boundary():
    """blob_scene(100)'s class map with a synthetic boundary map: 255 on the class boundaries (scenes.host_boundaries), dilated by one
    pixel, 40 elsewhere, in every channel but a random one per pixel; and a distance map that rises with the distance from the band."""
    cls = blob_scene(100)[1]
    H, W = cls.shape
    band = scenes.host_boundaries(cls, NCLS) != 255
    wide = band.copy()
    wide[1:] |= band[:-1]; wide[:-1] |= band[1:]; wide[:, 1:] |= band[:, :-1]; wide[:, :-1] |= band[:, 1:]
    rng = np.random.default_rng(41)
    bound = np.where(wide, 255, 40).astype(np.uint8)[..., None].repeat(NCLS, 2)
    bound[np.arange(H)[:, None], np.arange(W)[None, :], rng.integers(0, NCLS, (H, W))] = 127
    dist = np.where(wide, 20, 180).astype(np.uint8)[..., None].repeat(NCLS, 2)
    dist[band] = 0
    return cls, np.ascontiguousarray(bound), np.ascontiguousarray(dist)


# ---- 1. the seed map --------------------------------------------------------------------------------------------------------------
def test_seed_map_equals_the_host_definition():
    rng = np.random.default_rng(5)
    for H, W in ((1, 1), (1, 300), (33, 65), (70, 131)):
        cls = rng.integers(0, 6, (H, W)).astype(np.uint8)
        cls[rng.random((H, W)) < 0.1] = 255
        bound, dist = (rng.integers(0, 256, (H, W, 5)).astype(np.uint8) for _ in range(2))
        for b, d, bb, da, classes in ((None, None, 128, 0, (0, 1, 2, 3, 4)), (bound, None, 128, 0, (1, 3)), (None, dist, 128, 77, (0, 4)), (bound, dist, 1, 255, (2,)),
                                      (bound, dist, 256, 0, (0, 2)), (bound, dist, 200, 30, ())):
            want = scenes.host_seed_map(cls, b, d, num_classes=5, classes=list(classes), bound_below=bb, dist_at_least=da)
            assert np.array_equal(run_seed_map(cls, b, d, 5, classes, bb, da), want), (H, W, bb, da, classes)
    cls, bound, dist = blob_with_boundary()
    want = scenes.host_seed_map(cls, bound, dist, num_classes=NCLS, classes=[1, 2, 3], dist_at_least=100)
    assert np.array_equal(run_seed_map(cls, bound, dist, NCLS, (1, 2, 3), 128, 100), want) and 0 < (want != 255).sum() < (cls != 0).sum()
    cls64 = rng.integers(0, 64, (40, 50)).astype(np.uint8)
    b64 = rng.integers(0, 256, (40, 50, 64)).astype(np.uint8)
    assert np.array_equal(run_seed_map(cls64, b64, None, 64, (0, 63, 31)), scenes.host_seed_map(cls64, b64, num_classes=64, classes=[0, 63, 31]))


# ---- 2. instances -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [0, 1, 4, 16])
@pytest.mark.parametrize("connectivity,min_seed", [(4, 1), (8, 5)])
def test_instances_equal_the_host_definition(radius, connectivity, min_seed):
    for cls, marker in MAPS:
        check_instances(cls, marker, C4, (0, 2), min_seed=min_seed, radius=radius, connectivity=connectivity)


@pytest.mark.parametrize("connectivity,min_seed", [(8, 1), (4, 5)])
def test_instances_other_pairs_and_every_class(connectivity, min_seed):
    for cls, marker in MAPS[3::3]:
        for radius in (1, 16):
            check_instances(cls, marker, C4, (0, 1, 2, 3), min_seed=min_seed, radius=radius, connectivity=connectivity)


def test_blob_scene_with_a_boundary_map():
    cls, bound, dist = blob_with_boundary()
    marker = run_seed_map(cls, bound, dist, NCLS, (1, 2, 3), 128, 100)
    for radius, min_seed in ((0, 1), (2, 4), (4, 1), (16, 8)):
        inst, table, n, ungrown = check_instances(cls, marker, NCLS, (1, 2, 3), min_seed=min_seed, radius=radius)
        assert n > 20
    # without head maps and at radius 0: the connected regions of the chosen classes
    plain = run_seed_map(cls, None, None, NCLS, (1, 3))
    inst, table, n, ungrown = run_instances(cls, plain, NCLS, (1, 3), radius=0, connectivity=8)
    labels, areas = scenes.host_regions(cls, 8)
    chosen = np.isin(cls, (1, 3))
    assert ungrown == 0 and np.array_equal(table[:, 0], np.flatnonzero((areas.ravel() > 0) & chosen.ravel())) and np.array_equal(table[inst[chosen], 0], labels[chosen])


def test_seeds_on_both_sides_of_a_tile_seam_and_of_a_tile_corner():
    cls = np.ones((2 * TILE + 6, 2 * TILE + 6), np.uint8)
    for places in ([(10, TILE - 2), (10, TILE + 2)],                                              # the tie pixel (10, TILE) goes to the lower id
                   [(TILE - 2, 5), (TILE + 2, 5)], [(TILE - 2, TILE - 2), (TILE + 1, TILE + 1)], [(TILE + 1, TILE - 2), (TILE - 2, TILE + 1)],
                   [(TILE - 1, TILE - 1), (TILE - 1, TILE), (TILE, TILE - 1), (TILE, TILE)], [(0, 0), (2 * TILE + 5, 2 * TILE + 5), (TILE - 16, TILE), (TILE + 16, TILE - 1)]):
        marker = np.full(cls.shape, 255, np.uint8)
        for i, j in places:
            marker[i, j] = 1
        for radius in (1, 2, 4, 16):
            inst, table, n, ungrown = check_instances(cls, marker, 2, (1,), radius=radius)
            assert n == (1 if places[0] == (TILE - 1, TILE - 1) else len(places))              # the four pixels round the corner are one seed
    marker = np.full(cls.shape, 255, np.uint8)
    marker[10, TILE - 2] = marker[10, TILE + 2] = 1
    assert run_instances(cls, marker, 2, (1,), radius=2)[0][10, TILE - 2:TILE + 3].tolist() == [0, 0, 0, 1, 1]
    two = cls.copy()
    two[:, TILE:] = 2                                                                          # a class edge on the seam: nothing grows across it
    marker[10, TILE + 2] = 2
    inst = check_instances(two, marker, 3, (1, 2), radius=4)[0]
    assert inst[10, TILE - 1] == 0 and inst[10, TILE] == 1


def test_more_chunks_than_one_pass_of_the_scan():
    H, W = 520, 530                                                                            # 270 chunks of 1024 pixels: two passes of 256
    rng = np.random.default_rng(31)
    cls = blocky(rng, H, W, 7)
    marker = seeded(cls, rng, 0.2)
    marker[40:230] = 255                                                                       # about 98 chunks without a seed, then seeds again
    marker[300:310] = 255
    marker[H - 2:, W - 8:] = 255
    marker[H - 1, W - 6:] = cls[H - 1, W - 6:] = 3                                             # a seed of six pixels in the last, partial chunk
    for radius, conn, min_seed in ((0, 4, 1), (4, 8, 5)):
        inst, table, n, ungrown = check_instances(cls, marker, C4, (0, 1, 2), min_seed=min_seed, radius=radius, connectivity=conn)
        chunk_of = table[:, 0] // CHUNK
        assert n > 2000 and chunk_of.max() == 269 and len(np.unique(chunk_of)) < 180 and (chunk_of > 256).any()


def test_no_seed_and_more_seeds_than_the_table_holds():
    cls, marker = MAPS[-1]
    nothing = np.full(cls.shape, 255, np.uint8)
    inst, table, n, ungrown = check_instances(cls, nothing, C4, (0, 2), radius=4)
    assert n == 0 and len(table) == 0 and (inst == -1).all() and ungrown == int(np.isin(cls, (0, 2)).sum())
    full = check_instances(cls, marker, C4, (0, 2), radius=4)
    for cap in (1, 7, full[2] - 1, full[2], full[2] + 1):
        inst, table, n, ungrown = check_instances(cls, marker, C4, (0, 2), radius=4, cap=cap)
        assert n == full[2] and len(table) == min(cap, n) and np.array_equal(inst, full[0]) and np.array_equal(table, full[1][:cap])


# ---- 3. the match -----------------------------------------------------------------------------------------------------------------
def objects_of(cls, C, classes, connectivity=4):
    marker = scenes.host_seed_map(cls, num_classes=C, classes=list(classes))
    return scenes.host_instances(cls, marker, num_classes=C, classes=list(classes), radius=0, connectivity=connectivity)


def test_match_hand_cases_and_empty_tables():
    for inst_p, table_p, inst_g, n_g, want in match_cases():
        assert run_match(inst_p, table_p, inst_g, n_g).tolist() == want
        assert run_match(inst_p, table_p, inst_g, 0).tolist() == [[-1, 0]] * len(table_p)                      # Ng = 0
        assert run_match(inst_p, table_p, inst_g, 1).tolist() == scenes.host_instance_match(inst_p, table_p, inst_g, 1).tolist()
        assert run_match(inst_p, table_p[:0], inst_g, n_g).shape == (0, 2)                                    # Np = 0
        assert run_match(inst_p, table_p, inst_g, 64).tolist() == want                                         # an upper bound of Ng
    inst_p, table_p, inst_g, n_g, want = match_cases()[0]
    more = np.concatenate([table_p, np.zeros((5, 8), np.int32)])                                               # an upper bound of Np: rows of area 0
    assert run_match(inst_p, more, inst_g, n_g).tolist() == want + [[-1, 0]] * 5


def test_match_of_one_pixel_objects_with_10_bit_ids():
    board = (np.add.outer(np.arange(40), np.arange(40)) % 2).astype(np.uint8)
    inst_g, table_g, ng, _ = objects_of(board, 2, (1,))
    assert ng == 800 and (ng - 1).bit_length() == 10
    rng = np.random.default_rng(7)
    cls = np.kron(rng.integers(0, 2, (10, 10)), np.ones((4, 4), np.int64)).astype(np.uint8)                    # 4 x 4 blocks: eight objects each, no majority
    cls[rng.random(cls.shape) < 0.1] ^= 1
    inst_p, table_p, n_p, _ = objects_of(cls, 2, (1,))
    got = run_match(inst_p, table_p, inst_g, ng)
    assert np.array_equal(got, scenes.host_instance_match(inst_p, table_p, inst_g, ng))
    assert (got[:, 0] >= 0).sum() >= 3 and (got[:, 0] < 0).sum() >= 3
    same = run_match(inst_g, table_g, inst_g, ng)
    assert np.array_equal(same[:, 0], np.arange(ng)) and (same[:, 1] == 1).all()


def test_match_reaches_the_high_bits():
    H, W = 520, 530
    board = (np.add.outer(np.arange(H), np.arange(W)) % 2).astype(np.uint8)
    inst_g, table_g, ng, _ = objects_of(board, 2, (0, 1))
    assert ng == H * W > 1 << 17 and np.array_equal(inst_g.ravel(), np.arange(H * W))
    got = run_instances(board, board, 2, (0, 1), radius=0)                                                    # the kernels number them the same
    assert got[2] == ng and np.array_equal(got[0], inst_g) and np.array_equal(got[1], table_g)
    rng = np.random.default_rng(13)
    marker = np.where(rng.random((H, W)) < 0.3, board, 255).astype(np.uint8)
    inst_p, table_p, n_p, _ = scenes.host_instances(board, marker, num_classes=2, classes=[0, 1], radius=0)
    match = run_match(inst_p, table_p, inst_g, ng)
    assert np.array_equal(match[:, 0], table_p[:, 0]) and (match[:, 1] == 1).all() and match[:, 0].max() > 1 << 18
    rows = blocky(rng, H, W, 9, 2)                                                                             # large predictions: no object holds half of one
    inst_p, table_p, n_p, _ = objects_of(rows, 2, (0, 1))
    match = run_match(inst_p, table_p, inst_g, ng)
    assert np.array_equal(match, scenes.host_instance_match(inst_p, table_p, inst_g, ng)) and (match[table_p[:, 2] > 1, 0] == -1).all()


def test_two_runs_give_the_same_bytes():
    cls, bound, dist = blob_with_boundary()
    marker = run_seed_map(cls, bound, dist, NCLS, (1, 2, 3), 128, 100)
    assert np.array_equal(marker, run_seed_map(cls, bound, dist, NCLS, (1, 2, 3), 128, 100))
    assert run_instances(cls, marker, NCLS, (1, 2, 3), radius=4, raw=True) == run_instances(cls, marker, NCLS, (1, 2, 3), radius=4, raw=True)
    inst_p, table_p, n_p, _ = scenes.host_instances(cls, marker, num_classes=NCLS, classes=[1, 2, 3], radius=4)
    inst_g, table_g, ng, _ = objects_of(cls, NCLS, (1, 2, 3))
    assert run_match(inst_p, table_p, inst_g, ng, raw=True) == run_match(inst_p, table_p, inst_g, ng, raw=True)


# ---- 4. ScenePool -----------------------------------------------------------------------------------------------------------------
def test_pool_instances_and_match_equal_the_cpu_pool():
    cls, bound, dist = blob_with_boundary()
    maps = [cls, blob_scene(101, 97, 260)[1]]
    images = [np.zeros(m.shape + (1,), np.uint8) for m in maps]
    gpu, cpu = scenes.ScenePool(images, None), scenes.ScenePool(images, None, device="cpu")
    kw = dict(num_classes=NCLS, classes=[1, 2, 3], dist_at_least=100, min_seed=2, radius=3)
    got, want = gpu.instances([cls, None], [bound, None], [dist, None], **kw), cpu.instances([cls, None], [bound, None], [dist, None], **kw)
    assert got[1] is None and want[1] is None and all(np.array_equal(a, b) for a, b in zip(got[0], want[0])) and got[0][2] > 20
    gt, gt_want = gpu.instances(maps, num_classes=NCLS, classes=[1, 2, 3], radius=0, connectivity=8, want_map=True), cpu.instances(maps, num_classes=NCLS, classes=[1, 2, 3], radius=0, connectivity=8)
    assert all(np.array_equal(a, b) for s in range(2) for a, b in zip(gt[s], gt_want[s]))
    match = gpu.instance_match(got[0][0], got[0][1], gt[0][0], gt[0][1])
    assert match.dtype == np.int32 and np.array_equal(match, cpu.instance_match(got[0][0], got[0][1], gt[0][0], gt[0][1])) and (match[:, 0] >= 0).any()
    assert gpu.instances(maps, num_classes=NCLS, classes=[1], want_map=False)[0][0] is None
    with pytest.raises(ValueError, match=f"scene 0 holds {got[0][2]} seeds, max_instances is 5"):
        gpu.instances([cls, None], [bound, None], [dist, None], max_instances=5, **kw)


# ---- 5. predict_scene(instances=) -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model_and_pool():
    return new_model(), blob_pool()


def same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is b
    return np.array_equal(a, b, equal_nan=True) if isinstance(a, np.ndarray) and a.dtype.kind == "f" else np.array_equal(a, b)


def check_report(pool, s, pred, heads, report, inst):
    p = scenes.instance_params(inst, NCLS)
    kw = dict(num_classes=NCLS, classes=list(p["classes"]))
    marker = scenes.host_seed_map(pred, heads.get("bound") if p["bound_below"] < 256 else None, heads.get("dist") if p["dist_at_least"] > 0 else None,
                                  bound_below=p["bound_below"], dist_at_least=p["dist_at_least"], **kw)
    inst_p, table_p, n, ungrown = scenes.host_instances(pred, marker, min_seed=p["min_seed"], radius=p["radius"], connectivity=p["connectivity"], **kw)
    assert sorted(report) == sorted(["n", "ungrown", "table", "gt_n", "gt_table", "match", "scores"] + (["inst"] if p["map"] else []))
    assert report["n"] == n and report["ungrown"] == ungrown and report["table"].dtype == np.int32 and np.array_equal(report["table"], table_p)
    if p["map"]:
        assert report["inst"].dtype == np.int32 and np.array_equal(report["inst"], inst_p)
    if pool.class_maps is None:
        assert report["gt_n"] is None and report["gt_table"] is None and report["match"] is None and report["scores"] is None
        return n
    cls = pool.class_maps[s]
    inst_g, table_g, ng, _ = scenes.host_instances(cls, scenes.host_seed_map(cls, **kw), radius=0, connectivity=p["connectivity"], **kw)
    match = scenes.host_instance_match(inst_p, table_p, inst_g, ng)
    assert report["gt_n"] == ng and np.array_equal(report["gt_table"], table_g) and np.array_equal(report["match"], match)
    assert same(report["scores"], scenes.instance_scores(table_p, table_g, match, NCLS, p["iou_percent"]))
    return n


INSTANCES = [{"classes": [1, 2], "bound_below": 256, "map": True}, {"classes": [0, 1, 2, 3], "bound_below": 0.5, "dist_at_least": 0.45, "radius": 6, "map": True},
             {"classes": [3], "bound_below": 140, "min_seed": 3, "radius": 16, "connectivity": 8, "iou_percent": (50, 75)}, 2]


@pytest.mark.parametrize("k", range(len(INSTANCES)))
def test_predict_scene_instances_equal_the_host_pipeline(model_and_pool, k):
    m, pool = model_and_pool
    inst = INSTANCES[k]
    for s, kw in ((0, dict()), (1, dict()), (0, dict(sieve=8)), (0, dict(views="flips"))):
        pred, cm, *rest = m.predict_scene(pool, s, stride=32, batch=4, heads=("bound", "dist"), **kw)
        res = m.predict_scene(pool, s, stride=32, batch=4, instances=inst, **kw)
        assert len(res) == len(rest) + 2 and np.array_equal(res[0], pred) and np.array_equal(res[1], cm)
        check_report(pool, s, pred, rest[-1], res[-1], inst)
    # with the head maps asked for, and with every other report: the instances come after the sweep report and before the head maps
    pred, cm, *rest = m.predict_scene(pool, 0, stride=32, batch=4, heads=("dist", "bound"), erode=3, boundary=2, sieve=8, sweep=1)
    res = m.predict_scene(pool, 0, stride=32, batch=4, heads=("dist", "bound"), erode=3, boundary=2, sieve=8, sweep=1, instances=inst)
    assert len(res) == len(rest) + 3 and all(same(a, b) for a, b in zip(res[:6] + res[7:], (pred, cm) + tuple(rest)))
    check_report(pool, 0, pred, rest[-1], res[6], inst)


def test_predict_scene_instances_none_is_the_call_without_it(model_and_pool):
    m, pool = model_and_pool
    for kw in (dict(), dict(erode=3, boundary=2, heads=("bound",), sieve=8), dict(views="flips", sweep=1)):
        a, b = m.predict_scene(pool, 0, stride=32, batch=4, **kw), m.predict_scene(pool, 0, stride=32, batch=4, instances=None, **kw)
        assert len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))


def test_predict_scene_instances_without_class_maps_under_blend_and_refusals(model_and_pool):
    m, pool = model_and_pool
    bare = scenes.ScenePool(pool.images, None, patch=64)
    inst = {"classes": [1, 2], "bound_below": 256, "min_seed": 4}
    pred, cm, report = m.predict_scene(bare, 0, stride=32, batch=4, instances=inst)
    assert cm is None and check_report(bare, 0, pred, {}, report, inst) > 0
    for kw in (dict(blend="linear"), dict(scales=(1.0, 1.5))):                                 # with both head tests off it works everywhere
        pred, cm, report = m.predict_scene(pool, 0, stride=32, batch=4, instances=inst, **kw)
        assert np.array_equal(pred, m.predict_scene(pool, 0, stride=32, batch=4, **kw)[0])
        check_report(pool, 0, pred, {}, report, inst)
        with pytest.raises(ValueError, match="head threshold and scales or blend"):
            m.predict_scene(pool, 0, stride=32, batch=4, instances=[1, 2], **kw)
    for wrong, text in (("1", "instances '1'"), ({"classes": [NCLS]}, f"class {NCLS}, outside"), ({"classes": 1, "radius": 17}, "radius 17 outside 0..16"),
                        ({"classes": 1, "grow": 2}, "unknown key 'grow'")):
        with pytest.raises(ValueError, match=text):
            m.predict_scene(pool, 0, stride=32, batch=4, instances=wrong)
    with pytest.raises(ValueError, match="the scene holds [0-9]+ seeds, max_instances is 2"):
        m.predict_scene(pool, 0, stride=32, batch=4, instances={"classes": [0, 1, 2, 3], "bound_below": 256, "max_instances": 2})


def test_single_task_model_needs_the_head_tests_off():
    m = new_engine(False, False)
    pool = blob_pool((64, 80))
    with pytest.raises(ValueError, match="this model has no 'bound' head"):
        m.predict_scene(pool, 1, batch=2, instances=1)
    inst = {"classes": [0, 1, 2, 3], "bound_below": 256}
    pred, cm, report = m.predict_scene(pool, 1, batch=2, instances=inst)
    check_report(pool, 1, pred, {}, report, inst)


def test_evaluate_scenes_lists_the_reports_and_sums_the_scores(model_and_pool):
    m, pool = model_and_pool
    inst = {"classes": [1, 2], "bound_below": 0.5, "min_seed": 2}
    per = [m.predict_scene(pool, s, stride=32, batch=4, instances=inst) for s in range(len(pool))]
    maps, total, objects = m.evaluate_scenes(pool, stride=32, batch_size=4, instances=inst)
    assert all(np.array_equal(a, p[0]) for a, p in zip(maps, per)) and np.array_equal(total, sum(p[1] for p in per))
    assert len(objects["scenes"]) == len(pool) and all(same(a, p[2]) for a, p in zip(objects["scenes"], per))
    assert same(objects["scores"], scenes.sum_instance_scores([p[2]["scores"] for p in per]))
    maps2, total2, swept, objects2, heads = m.evaluate_scenes(pool, stride=32, batch_size=4, instances=inst, sweep=1, heads="bound")
    assert same(objects2, objects) and len(heads) == len(pool) and "hist" in swept
    assert len(m.evaluate_scenes(pool, stride=32, batch_size=4)) == 2


def test_cli_instances(tmp_path, capsys):
    import eval_scenes_ISPRS
    from resunet_a_mltsk_keras_amd.keras_api import load_model
    sc = [blob_scene(300, 90, 70), blob_scene(301, 64, 100)]
    root, path = str(tmp_path / "scenes"), str(tmp_path / "m.h5")
    scenes.save_scene_dir(root, ["a_tile", "b_tile"], [s[0] for s in sc], [s[1] for s in sc])
    new_model(seed=11, depth=4, split_k=True).save(path)
    base = ["--use_multitasking", "--model_path", path, "--dataset_path", root, "-ps", "64", "--num_classes", str(NCLS),
            "--scene_dataset", "yes", "--stride", "32", "--batch_size", "4"]
    plain = eval_scenes_ISPRS.main(base + ["--output_path", str(tmp_path / "plain")])
    capsys.readouterr()
    res = eval_scenes_ISPRS.main(base + ["--output_path", str(tmp_path / "obj"), "--instances", "1", "2", "--inst_min_seed", "2", "--inst_radius", "3", "--inst_map", "yes"])
    out = capsys.readouterr().out.splitlines()
    assert any(line.startswith("Objects of the classes 1 2") for line in out) and sum("predicted objects" in line for line in out) == 2
    assert set(res) - set(plain) == {"instance_scores", "instance_counts"} and np.array_equal(res["confusion_matrix"], plain["confusion_matrix"])
    names, images, class_maps = scenes.load_scene_dir(root)
    inst = {"classes": [1, 2], "bound_below": 0.5, "dist_at_least": 0.0, "min_seed": 2, "radius": 3, "map": True}
    _, _, objects = load_model(path, compile=False).evaluate_scenes(scenes.ScenePool(images, class_maps, patch=64), stride=32, batch_size=4, norm_type=1, instances=inst)
    assert same(res["instance_scores"], objects["scores"])
    for n, report in zip(names, objects["scenes"]):
        table = np.load(tmp_path / "obj" / f"instances_{n}.npy")
        assert table.dtype == np.int32 and np.array_equal(table, report["table"])
        assert np.array_equal(np.load(tmp_path / "obj" / f"inst_map_{n}.npy"), report["inst"])
        assert not (tmp_path / "plain" / f"instances_{n}.npy").exists()
    sc6 = np.load(tmp_path / "obj" / "instance_scores.npy")
    assert sc6.shape == (NCLS, 6) and np.array_equal(sc6[:, 0], objects["scores"]["n_pred"]) and np.array_equal(sc6[:, 4], objects["scores"]["f1_50"], equal_nan=True)
