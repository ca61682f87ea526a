"""The channel-sliced form of the fused BatchNorm launches (rua_bn_fwd, rua_bn_fwd_group, rua_bn_bwd, rua_bn_bwd_group on small maps; csrc/elementwise.hip,
bn_fwd_sliced_body / bn_bwd_sliced_body) through the C ABI, at the smallest shapes where it can go wrong: fewer pixels than a wave, than a block step (256 / S
pixels), a ragged last step, uneven parts, one and three slices of S = 4 and S = 8 pieces, C = 1024, one to four branches, 1 / 3 / 8 / 32 input replicas and
1 / 4 / 32 replicas of the statistics outputs with values already in them.  Every case asserts that the route query reports the sliced form.

Against the float64 references of tests/_bn_pool_ref.py, with the checkers and the bounds tests/test_bn_gpu.py derives for the pixel-major form (the two forms share
their formulas and their per-piece expression): published coefficients to one float32 ulp, the forward sweep to one ulp of the storage type, dx to the counted
bound n U32 T + one storage ulp, dgamma / dbeta to two ulp.  skip_stats / dx_stats are exact on integer data, on top of what the buffers held.  With the tuning key
bn_sliced at 0 and at 1 on the same inputs every output is bit-identical (the produced sums on integer data, where no summation order rounds); where the route keeps
P at or below the replicas of the outputs, two launches on random data produce the same bits in the sums.  Every written buffer sits between guard regions."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _bn_pool_ref as R  # noqa: E402
import test_bn_gpu as B  # noqa: E402  (descriptor builders, input makers and checkers of the pixel-major tests)
from _kernel_util import Guarded, stream  # noqa: E402
from resunet_a_mltsk_keras_amd import _lib as L  # noqa: E402

f32, f64 = np.float32, np.float64
F32, BF16 = L.RUA_F32, L.RUA_BF16
DTYPES, DT_IDS = [F32, BF16], {F32: "f32", BF16: "bf16"}
PIXELS = [1, 7, 8, 9, 31, 32, 33, 257]
IN_R = [1, 3, 8, 32]


def chan(dt, S, slices):
    return S * B.vec(dt) * slices


def bits(buf):
    a = buf.get()                                            # (asserts the guard regions)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)


def route_of(name, d):
    r = L.lib().raw(name)(C.byref(d))
    return r & 255, r >> 8


# ---- forward -----------------------------------------------------------------------------------------------------------------------------
# (dt, C, M, nb, relu, training, input replicas, branch 1 with statistics of its own, out_stats, forced parts or 0, S the route has to report)
def fwd_cases():
    out = []
    for dt in DTYPES:
        for i, M in enumerate(PIXELS):                                                          # one slice of whole lines
            out.append((dt, chan(dt, 8, 1), M, 1 + i % 4, i % 2, 1, IN_R[i % 4], 0, 0, 0, 8))
        for M in (33, 257):                                                                     # half-line slices, one and three
            out += [(dt, chan(dt, 4, 1), M, 2, 1, 1, 3, 0, 0, 0, 4), (dt, chan(dt, 4, 3), M, 3, 0, 1, 8, 1, 0, 0, 4)]
        out.append((dt, chan(dt, 8, 3), 257, 4, 1, 1, 32, 1, 0, 0, 8))                          # three slices
        out.append((dt, 1024, 70, 2, 1, 1, 8, 0, 0, 0, 8))
        out.append((dt, chan(dt, 8, 1), 33, 2, 1, 0, 1, 0, 0, 0, 8))                            # inference
        out.append((dt, chan(dt, 8, 3), 70, 3, 0, 1, 3, 1, 1, 0, 8))                            # out_stats (no ReLU), branch 1 on statistics of its own
        out.append((dt, chan(dt, 8, 1), 1000, 1, 1, 1, 1, 0, 0, 7, 8))                          # 7 parts of 142 / 143 pixels
    return out


def fwd_id(c):
    dt, Cc, M, nb, relu, tr, rin, own, ost, forced, S = c
    return f"{DT_IDS[dt]}-C{Cc}-M{M}-nb{nb}-relu{relu}-train{tr}-Rin{rin}-own{own}-ostats{ost}-P{forced}-S{S}"


def run_fwd(case, sliced):
    dt, Cc, M, nb, relu, training, rin, own, ostats, forced, S = case
    rng = np.random.default_rng(1000 * Cc + M + 10 * nb + relu)
    x = B.sweep_input(rng, M, Cc, dt)
    x64 = x.astype(f64)
    tot, count = np.stack([x64.sum(0), (x64 * x64).sum(0)]), float(M)
    xd, shd = B.tbuf(x, dt), Guarded(B.split(tot, rin, rng))
    hs = []
    for b in range(nb):
        if own and b == 1:
            o = B.made_stats(rng, Cc, count, 3)
            h, s = B.fwd_branch(rng, Cc, o[0], out_stats=bool(ostats))
            s["stats"] = (Guarded(o[1]), 3)
        else:
            h, s = B.fwd_branch(rng, Cc, tot, out_stats=bool(ostats))
        s["out"] = Guarded(R.storage_bits(np.full((M, Cc), np.nan, f32), B.bf(dt)))
        hs.append((h, s))
    d = B.fwd_desc(dt, M, Cc, nb, relu, training, count, count, xd, (shd, rin), [s for _, s in hs])
    with B.tuning(bn_sliced=sliced, bn_sliced_parts=forced):
        route = route_of("rua_bn_fwd_route", d)
        L.lib().call("rua_bn_fwd", C.byref(d), stream())
        torch.cuda.synchronize()
    snap = {f"{k}{b}": bits(s[k]) for b, (_, s) in enumerate(hs) for k in ("scale", "shift", "mean", "rstd", "mm", "mv", "out", "out_stats") if k in s}
    assert np.array_equal(xd.get(), R.storage_bits(x, B.bf(dt)))
    return route, hs, x, snap, count


@pytest.mark.parametrize("case", fwd_cases(), ids=[fwd_id(c) for c in fwd_cases()])
def test_bn_fwd_sliced(case):
    dt, Cc, M, nb, relu, training, rin, own, ostats, forced, S = case
    route, hs, x, snap, count = run_fwd(case, 1)
    assert route[0] == S and route[1] >= 1, "not the sliced form"
    assert route[1] == forced or not forced
    for h, s in hs:
        scale, shift = B.check_fwd_coefficients(h, s, count, count, training)
        B.check_sweep(x, scale, shift, relu, s["out"], dt)
    r0, _, _, snap0, _ = run_fwd(case, 0)
    assert r0 == (0, 0)
    assert same(snap, snap0), [k for k in snap if not np.array_equal(snap[k], snap0[k])]


# ---- backward ----------------------------------------------------------------------------------------------------------------------------
# (dt, C, M, nb, masked, dskip, accumulate, dx_stats replicas or 0, skip_stats replicas or 0, branch with stats2_out or None, input replicas per branch, forced parts, S)
def bwd_cases():
    flags = [(1, 0, 1, 0, 0, 32), (2, 1, 1, 1, 4, 0), (3, 0, 0, 0, 32, 0), (4, 1, 1, 0, 4, 32), (1, 1, 0, 1, 0, 0), (2, 0, 1, 1, 32, 4), (3, 1, 1, 1, 0, 4), (4, 0, 1, 0, 32, 32)]
    out = []
    for dt in DTYPES:
        for i, M in enumerate(PIXELS):                                                          # one slice of whole lines; replicas of 1 only where eight steps reach
            nb, mk, sk, acc, dxs, sks = flags[i]
            if M <= 256 and i % 3 == 0:
                dxs, sks = min(dxs, 1), min(sks, 1)
            out.append((dt, chan(dt, 8, 1), M, nb, mk, sk, acc, dxs, sks, None, (IN_R[i % 4:] + IN_R[:i % 4])[:nb], 0, 8))
        for M in (33, 257):                                                                     # half-line slices: one, two and three
            out += [(dt, chan(dt, 4, 1), M, 2, 1, 1, 0, 1, 4, None, [3, 32], 0, 4), (dt, chan(dt, 4, 2), M, 3, 1, 1, 1, 4, 4, None, [1, 8, 3], 0, 4),
                    (dt, chan(dt, 4, 3), M, 4, 0, 1, 1, 0, 0, None, [8, 1, 32, 3], 0, 4)]
        # three slices (no statistics outputs: rua_bn_bwd takes them only where the pieces of a row divide 256, in either form) and four
        out.append((dt, chan(dt, 8, 3), 257, 4, 1, 1, 1, 0, 0, None, [32, 8, 3, 1], 0, 8))
        out.append((dt, chan(dt, 8, 4), 257, 4, 1, 1, 1, 32, 4, None, [32, 8, 3, 1], 0, 8))
        out.append((dt, 1024, 70, 2, 1, 1, 0, 4, 32, None, [8, 3], 0, 8))
        out.append((dt, chan(dt, 8, 1), 33, 2, 1, 1, 0, 0, 0, 1, [1, 3], 0, 8))                 # stats2_out on branch 1
        out.append((dt, chan(dt, 8, 1), 1000, 3, 1, 1, 1, 4, 4, None, [3, 8, 1], 7, 8))         # 7 parts of 142 / 143 pixels onto 4 replicas
    return out


def bwd_id(c):
    dt, Cc, M, nb, mk, sk, acc, dxs, sks, s2o, rin, forced, S = c
    return f"{DT_IDS[dt]}-C{Cc}-M{M}-nb{nb}-mask{mk}-skip{sk}-acc{acc}-dxs{dxs}-sks{sks}-s2o{s2o}-Rin{'.'.join(map(str, rin))}-P{forced}-S{S}"


def bwd_problem(case, integer):
    """Inputs and the float64 reference.  integer: x, g, dskip and the old dx are integers in [-8, 8], stats2 is zero and gamma rstd is +-1 or +-2, so B = C = 0, A is
    +-1 / +-2 and dx = [old] + [dskip] + sum_b A_b g_b m_b is an integer of at most 80: dx, its sums and the sums of dx x are exact in either storage type."""
    dt, Cc, M, nb, masked, use_skip, acc, dxs, sks, s2o, rin, forced, S = case
    rng = np.random.default_rng(Cc * 7 + M + 100 * nb + 10 * masked + 3 * use_skip + acc + 5 * dxs + sks + integer)
    x, ms, mt, g, masks, dskip, old = B.bwd_inputs(rng, dt, Cc, M, nb, masked)
    if integer:
        x = rng.integers(-8, 9, (M, Cc)).astype(f32)
        g = [rng.integers(-8, 9, (M, Cc)).astype(f32) for _ in range(nb)]
        masks = [R.relu_mask(x, ms[b], mt[b]) if masked else None for b in range(nb)]
        gamma = [rng.choice([-1.0, 1.0], Cc).astype(f32) for _ in range(nb)]
        rstd = [rng.choice([1.0, 2.0], Cc).astype(f32) for _ in range(nb)]
    else:
        gamma = [B.signed(rng, 0.5, 1.5, Cc) for _ in range(nb)]
        rstd = [rng.uniform(0.5, 2.0, Cc).astype(f32) for _ in range(nb)]
    mean = [rng.standard_normal(Cc).astype(f32) for _ in range(nb)]
    count, x64 = float(M), x.astype(f64)
    As, Bs, Cs, parts, grads, starts = [], [], [], [], [], []
    for b in range(nb):
        gm = np.where(masks[b], g[b].astype(f64), 0.0) if masked else g[b].astype(f64)
        sg, sgx = gm.sum(0), (gm * x64).sum(0)
        if integer:
            pb = np.zeros((rin[b], 2, Cc))
            tot = pb.sum(0)
        else:
            slot1 = (gm * (ms[b].astype(f64) * x64 + mt[b])).sum(0) if s2o == b else sgx
            pb = B.split(np.stack([sg, slot1]), rin[b], rng)
            tot = pb.sum(0) if s2o != b else np.stack([sg, sgx])
        A, Bq, Cq, dga, dbe = R.bn_bwd_coeffs(tot[0], tot[1], count, gamma[b], mean[b], rstd[b])
        As.append(A); Bs.append(Bq); Cs.append(Cq); parts.append(pb); grads.append((dga, dbe))
        starts.append((B.grad_start(rng, dga), B.grad_start(rng, dbe)))
    ref, T = R.bn_bwd_apply(x64, g, As, masks, sum(Bs), sum(Cs), dskip if use_skip else None, old if acc else None)
    spre = rng.integers(1, 6, (max(sks, 1), 2, Cc)).astype(f64)
    dpre = rng.integers(1, 6, (max(dxs, 1), 2, Cc)).astype(f64)
    return dict(x=x, ms=ms, mt=mt, g=g, dskip=dskip, old=old, gamma=gamma, mean=mean, rstd=rstd, parts=parts, grads=grads, starts=starts, ref=ref, T=T,
                spre=spre, dpre=dpre, count=count)


def bwd_launch(case, q, sliced, group=None):
    """One rua_bn_bwd launch on fresh device buffers; returns (route, buffers).  group: a list the descriptor is appended to instead (rua_bn_bwd_group)."""
    dt, Cc, M, nb, masked, use_skip, acc, dxs, sks, s2o, rin, forced, S = case
    xd, gd, skd, dxd = B.tbuf(q["x"], dt), [B.tbuf(a, dt) for a in q["g"]], B.tbuf(q["dskip"], dt), B.tbuf(q["old"], dt)
    keep = [[B.fbuf(q[k][b]) for k in ("gamma", "mean", "rstd", "ms", "mt")] + [B.fbuf(q["starts"][b][0]), B.fbuf(q["starts"][b][1])] for b in range(nb)]
    st2 = [Guarded(p) for p in q["parts"]]
    skst, dxst = Guarded(q["spre"], guard=max(256, q["spre"][0].nbytes)), Guarded(q["dpre"], guard=max(256, q["dpre"][0].nbytes))
    e = L.BnBwdDesc()
    e.x, e.dskip, e.dx, e.M, e.C, e.dtype, e.nb, e.masked, e.accumulate, e.count = xd.ptr, skd.ptr if use_skip else None, dxd.ptr, M, Cc, dt, nb, masked, acc, q["count"]
    for b in range(nb):
        br, k = e.br[b], keep[b]
        br.g, br.stats2, br.replicas, br.stats2_out = gd[b].ptr, st2[b].ptr, rin[b], int(s2o == b)
        br.gamma, br.mean, br.rstd, br.scale, br.shift, br.dgamma, br.dbeta = (p.ptr for p in k)
    if sks:
        e.skip_stats, e.skip_replicas = skst.ptr, sks
    if dxs:
        e.dx_stats, e.dx_replicas = dxst.ptr, dxs
    bufs = dict(x=xd, dx=dxd, skst=skst, dxst=dxst, keep=keep, st2=st2, gd=gd, skd=skd)
    if group is not None:
        group.append(e)
        return None, bufs
    with B.tuning(bn_sliced=sliced, bn_sliced_parts=forced, bn_sliced_s=4 if S == 4 else 0):     # (the key matters where whole lines would fit too: two half-line slices)
        route = route_of("rua_bn_bwd_route", e)
        L.lib().call("rua_bn_bwd", C.byref(e), stream())
        torch.cuda.synchronize()
    return route, bufs


def bwd_snap(bufs, nb):
    s = {"dx": bits(bufs["dx"]), "skip_stats": bits(bufs["skst"]), "dx_stats": bits(bufs["dxst"])}       # the replicas as they lie (the forms spread them differently)
    s["skip_sum"], s["dx_sum"] = bufs["skst"].get().sum(0).view(np.uint64), bufs["dxst"].get().sum(0).view(np.uint64)
    for b in range(nb):
        s[f"dgamma{b}"], s[f"dbeta{b}"] = bits(bufs["keep"][b][5]), bits(bufs["keep"][b][6])
    return s


def check_bwd_bounds(case, q, bufs):
    dt, Cc, M, nb, masked, use_skip, acc = case[:7]
    B.check_dx(bufs["dx"], dt, q["ref"], q["T"], 6 * nb - 1 + use_skip + acc)
    for b in range(nb):
        assert B.within_ulps(bufs["keep"][b][5].get(), q["starts"][b][0].astype(f64) + q["grads"][b][0], 2), ("dgamma", b)
        assert B.within_ulps(bufs["keep"][b][6].get(), q["starts"][b][1].astype(f64) + q["grads"][b][1], 2), ("dbeta", b)
    assert np.array_equal(bufs["x"].get(), R.storage_bits(q["x"], B.bf(dt)))


def check_exact_sums(case, q, bufs):
    """Integer data: dx is the reference, bit for bit, and the replica-summed statistics outputs are what they held plus the integer sums."""
    dt, Cc, M, nb, masked, use_skip, acc, dxs, sks = case[:9]
    assert np.array_equal(B.tval(bufs["dx"], dt), q["ref"])
    got, pre = bufs["skst"].get().sum(0), q["spre"].sum(0)
    assert np.array_equal(got[0], pre[0] + (q["dskip"].astype(f64).sum(0) if sks else 0.0)) and np.array_equal(got[1], pre[1])
    got, pre = bufs["dxst"].get().sum(0), q["dpre"].sum(0)
    x64 = q["x"].astype(f64)
    assert np.array_equal(got[0], pre[0] + (q["ref"].sum(0) if dxs else 0.0)) and np.array_equal(got[1], pre[1] + ((q["ref"] * x64).sum(0) if dxs else 0.0))


@pytest.mark.parametrize("case", bwd_cases(), ids=[bwd_id(c) for c in bwd_cases()])
def test_bn_bwd_sliced(case):
    dt, Cc, M, nb, masked, use_skip, acc, dxs, sks, s2o, rin, forced, S = case
    outs = [r for r in (dxs, sks) if r]
    for integer in (1, 0):
        q = bwd_problem(case, integer)
        route, bufs = bwd_launch(case, q, 1)
        assert route[0] == S and route[1] >= 1, "not the sliced form"
        assert route[1] == forced if forced else all(route[1] <= r for r in outs)
        check_bwd_bounds(case, q, bufs)
        snap = bwd_snap(bufs, nb)
        r0, bufs0 = bwd_launch(case, q, 0)
        assert r0 == (0, 0)
        snap0 = bwd_snap(bufs0, nb)
        if integer:
            check_exact_sums(case, q, bufs)
            check_exact_sums(case, q, bufs0)
            differ = [k for k in snap if k not in ("skip_stats", "dx_stats") and not np.array_equal(snap[k], snap0[k])]
            assert not differ, differ
        else:
            differ = [k for k in snap if k not in ("skip_stats", "dx_stats", "skip_sum", "dx_sum") and not np.array_equal(snap[k], snap0[k])]
            assert not differ, differ
            if all(route[1] <= r for r in outs):             # one add per address: the same bits from launch to launch
                again = bwd_snap(bwd_launch(case, q, 1)[1], nb)
                assert same(snap, again), [k for k in snap if not np.array_equal(snap[k], again[k])]


# ---- groups: members of 1 / 5 / 33 / 70 pixels side by side --------------------------------------------------------------------------------
GROUP_M = [1, 5, 33, 70]


@pytest.mark.parametrize("S", [8, 4])
@pytest.mark.parametrize("dt", DTYPES, ids=[DT_IDS[d] for d in DTYPES])
def test_bn_fwd_group_sliced(dt, S):
    Cc = chan(dt, S, 3)
    lib = L.lib()
    snaps = {}
    for sliced in (1, 0):
        runs, arr = [], (L.BnFwdDesc * len(GROUP_M))()
        for i, M in enumerate(GROUP_M):
            rng = np.random.default_rng(17 * Cc + M)
            x = B.sweep_input(rng, M, Cc, dt)
            x64 = x.astype(f64)
            tot = np.stack([x64.sum(0), (x64 * x64).sum(0)])
            xd, shd = B.tbuf(x, dt), Guarded(B.split(tot, IN_R[i], rng))
            h, s = B.fwd_branch(rng, Cc, tot, out_stats=True)
            s["out"] = Guarded(R.storage_bits(np.full((M, Cc), np.nan, f32), B.bf(dt)))
            arr[i] = B.fwd_desc(dt, M, Cc, 1, 0, 1, float(M), float(M), xd, (shd, IN_R[i]), [s])
            runs.append((h, s, x, xd, shd, M))
        with B.tuning(bn_sliced=sliced):
            routes = [route_of("rua_bn_fwd_route", arr[i]) for i in range(len(GROUP_M))]
            lib.call("rua_bn_fwd_group", arr, len(GROUP_M), stream())
            torch.cuda.synchronize()
            assert lib.raw("rua_bn_fwd_group_last_grids")() == (1 if sliced else len(GROUP_M))      # (12 / 24 pieces per row: pixel-major goes member by member)
        assert all(r[0] == (S if sliced else 0) for r in routes), routes
        for h, s, x, xd, shd, M in runs:
            if sliced:
                scale, shift = B.check_fwd_coefficients(h, s, float(M), float(M), 1)
                B.check_sweep(x, scale, shift, 0, s["out"], dt)
        snaps[sliced] = {f"{k}{i}": bits(s[k]) for i, (h, s, *_) in enumerate(runs) for k in ("scale", "shift", "mean", "rstd", "mm", "mv", "out", "out_stats")}
    assert same(snaps[1], snaps[0]), [k for k in snaps[1] if not np.array_equal(snaps[1][k], snaps[0][k])]


@pytest.mark.parametrize("S,masked", [(8, 1), (4, 0)])
@pytest.mark.parametrize("dt", DTYPES, ids=[DT_IDS[d] for d in DTYPES])
def test_bn_bwd_group_sliced(dt, S, masked):
    Cc = chan(dt, S, 3)
    lib = L.lib()
    cases = [(dt, Cc, M, 1, masked, i % 2, (i + 1) % 2, 0, 0, None, [IN_R[i]], 0, S) for i, M in enumerate(GROUP_M)]
    qs = [bwd_problem(c, 0) for c in cases]
    snaps = {}
    for sliced in (1, 0):
        ds, bufs = [], []
        for c, q in zip(cases, qs):
            bufs.append(bwd_launch(c, q, sliced, group=ds)[1])
        arr = (L.BnBwdDesc * len(ds))(*ds)
        with B.tuning(bn_sliced=sliced):
            routes = [route_of("rua_bn_bwd_route", arr[i]) for i in range(len(ds))]
            lib.call("rua_bn_bwd_group", arr, len(ds), stream())
            torch.cuda.synchronize()
            assert lib.raw("rua_bn_bwd_group_last_grids")() == (1 if sliced else len(ds))           # (12 / 24 pieces per row: pixel-major goes member by member)
        assert all(r[0] == (S if sliced else 0) for r in routes), routes
        for c, q, b in zip(cases, qs, bufs):
            check_bwd_bounds(c, q, b)
        snaps[sliced] = {f"{k}{i}": v for i, b in enumerate(bufs) for k, v in bwd_snap(b, 1).items()}
    assert same(snaps[1], snaps[0]), [k for k in snaps[1] if not np.array_equal(snaps[1][k], snaps[0][k])]
