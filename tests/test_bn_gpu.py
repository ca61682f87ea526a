"""The BatchNorm family of librua_hip.so through the C ABI, every kernel alone against the float64 references of tests/_bn_pool_ref.py (checked against
torch autograd in tests/test_bn_pool_ref_host.py): rua_col_stats / rua_col_stats2 exactly on integer data, rua_bn_finalize / rua_bn_bwd_finalize and the
prologue of rua_bn_fwd to one float32 ulp from host-made statistics, the sweeps of rua_bn_apply / rua_bn_fwd to one ulp of the storage type, and
rua_bn_bwd_apply / rua_bn_bwd to a bound counted from the float32 roundings on the kernel's path.  No kernel's output is compared with another kernel's.
A "piece" is the 16-byte vector a thread moves (8 bf16 / 4 fp32 channels), CG = C / 8 or C / 4 the pieces of a row: the fused forms keep their
coefficients in registers where CG divides 256 (and the tuning key bn_regs is on) and read them from an LDS table elsewhere.  Every buffer a kernel
writes sits between guard regions (tests/_kernel_util.py: Guarded)."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _bn_pool_ref as R  # noqa: E402
from _kernel_util import U32, Guarded, stream, ulp_of, worst_ratio  # noqa: E402
from resunet_a_mltsk_keras_amd import _lib as L  # noqa: E402

f32, f64 = np.float32, np.float64
F32, BF16 = L.RUA_F32, L.RUA_BF16
DTYPES = [F32, BF16]
DT_IDS = ["f32", "bf16"]
EPS, MOM = float(f32(1e-3)), float(f32(0.99))     # float32 values, as the C ABI takes them
G20 = 2.0 ** -20                                             # grid of the host-made statistics: sums of such parts are exact in float64 in any order
NANF = np.uint32(0x7FC00000)
PAST_CAP = 2048 * 256 + 257                                  # pieces: one wrap of the 2048-block grid and a ragged rest


def bf(dt):
    return dt == BF16


def vec(dt):
    return 8 if bf(dt) else 4


def fbuf(a):
    return Guarded(np.ascontiguousarray(a, f32))


def fnan(n):
    """float32 output buffer filled with NaN: what a kernel leaves out shows."""
    return Guarded(np.full(n, NANF, np.uint32).view(f32))


def tbuf(a, dt):
    return Guarded(R.storage_bits(np.asarray(a, f32), bf(dt)))


def tval(buf, dt):
    b = buf.get()
    return (R.bf16_value(b) if bf(dt) else b.view(f32)).astype(f64)


def ptr(buf):
    return buf.ptr if buf is not None else None


def split(total, Rn, rng, grid=None):
    """[Rn] + total.shape: uneven parts whose sum is total (exactly, in any order, where total lies on `grid`); with Rn > 2 replica 1 holds zeros."""
    total = np.asarray(total, f64)
    fr = rng.uniform(0.0, 1.0, (Rn,) + total.shape) ** 3
    if Rn > 2:
        fr[1] = 0.0
    parts = total * (fr / fr.sum(0))
    if grid:
        parts = np.round(parts / grid) * grid
    parts[-1] = total - parts[:-1].sum(0)
    return parts


@contextlib.contextmanager
def tuning(**kv):
    lib = L.lib()
    before = {k: lib.get_tuning(k) for k in kv}
    try:
        lib.set_tuning(**kv)
        yield
    finally:
        lib.set_tuning(**before)


def within_ulps(got, ref, n=1, dt=F32):
    return worst_ratio(np.abs(np.asarray(got, f64) - ref), n * ulp_of(ref, dt)) <= 1.0


def signed(rng, lo, hi, n):
    return (rng.uniform(lo, hi, n) * rng.choice([-1.0, 1.0], n)).astype(f32)


# ---- rua_col_stats / rua_col_stats2: exact -----------------------------------------------------------------------------------------------
STATS = ([(BF16, 8, M, 1) for M in (1, 255, 256, 257, 5000)] + [(F32, 4, M, 2) for M in (257, 5000)]            # one piece per row: 256 rows per block and step
         + [(dt, 32, M, Rn) for dt in DTYPES for M in (640, 20000) for Rn in (1, 4, 32)]           # 20000: the unrolled sweep (8 / 4 deep) and its tail
         + [(BF16, 2048, 70, 2), (F32, 2048, 70, 2)])                                              # 256 groups: one row per step; 512 groups: gridDim.y = 2


def stats_variants():
    return [("x", None, None, 0), ("g", None, None, 0), ("g x>0", None, None, 1), ("g -x+0.5>0", -1.0, 0.5, 1), ("g x-2>0", 1.0, -2.0, 1)]


def check_stats(dt, Cc, M, Rn, seed):
    """Integers in [-8, 8] and M * 64 < 2^24: every float32 partial sum and every float64 add is exact, so the replica-summed buffer is the sum, bit for bit,
    on top of the integers the buffer held."""
    assert M * 64 < 2 ** 24
    rng = np.random.default_rng(seed)
    lib = L.lib()
    x = rng.integers(-8, 9, (M, Cc)).astype(f32)
    g = rng.integers(-8, 9, (M, Cc)).astype(f32)
    if M >= 255:
        assert (x == 2).any() and (x == 0).any()
    xd, gd = tbuf(x, dt), tbuf(g, dt)
    x64, g64 = x.astype(f64), g.astype(f64)
    for name, ms, mt, masked in stats_variants():
        pre = rng.integers(-5, 6, (Rn, 2, Cc)).astype(f64)
        st = Guarded(pre, guard=max(256, pre[0].nbytes))                                    # a guard the size of a replica: a replica index one too far lands in it
        if name == "x":
            lib.call("rua_col_stats", xd.ptr, M, Cc, st.ptr, Rn, dt, stream())
            want = np.stack([x64.sum(0), (x64 * x64).sum(0)])
        else:
            msd = fbuf(np.full(Cc, ms)) if ms is not None else None
            mtd = fbuf(np.full(Cc, mt)) if mt is not None else None
            lib.call("rua_col_stats2", gd.ptr, xd.ptr, ptr(msd), ptr(mtd), masked, M, Cc, st.ptr, Rn, dt, stream())
            m = ((1.0 if ms is None else ms) * x64 + (0.0 if mt is None else mt)) > 0 if masked else np.ones_like(x64, bool)
            gm = np.where(m, g64, 0.0)
            want = np.stack([gm.sum(0), (gm * x64).sum(0)])
        torch.cuda.synchronize()
        got = st.get().sum(0)
        assert np.array_equal(got, pre.sum(0) + want), (name, float(np.abs(got - pre.sum(0) - want).max()))


@pytest.mark.parametrize("dt,Cc,M,Rn", STATS, ids=[f"{DT_IDS[dt == BF16]}-C{c}-M{m}-R{r}" for dt, c, m, r in STATS])
def test_col_stats_exact(dt, Cc, M, Rn):
    check_stats(dt, Cc, M, Rn, seed=Cc + M + Rn)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_col_stats_exact_with_two_blocks(dt):
    """stats_blocks = 2: each thread sweeps ~150 rows - many rounds of the unrolled loop, and both replicas of R = 2 take one block's sums."""
    with tuning(stats_blocks=2):
        check_stats(dt, 32, 20000, 2, seed=77)


def test_col_stats_refusals_leave_the_buffer_alone():
    lib, s = L.lib(), stream()
    rng = np.random.default_rng(3)
    x = tbuf(rng.integers(-8, 9, (64, 64)).astype(f32), BF16)
    pre = rng.integers(-5, 6, (4, 2, 64)).astype(f64)
    st = Guarded(pre)
    one, two = lib.raw("rua_col_stats"), lib.raw("rua_col_stats2")
    bad = [("R = 3", one(x.ptr, 64, 32, st.ptr, 3, BF16, s)), ("C = 40", one(x.ptr, 64, 40, st.ptr, 4, BF16, s)), ("C = 12", one(x.ptr, 64, 12, st.ptr, 4, BF16, s)),
           ("dtype", one(x.ptr, 64, 32, st.ptr, 4, 7, s)), ("M = 0", one(x.ptr, 0, 32, st.ptr, 4, BF16, s)), ("null x", one(None, 64, 32, st.ptr, 4, BF16, s)),
           ("null g", two(None, x.ptr, None, None, 0, 64, 32, st.ptr, 4, BF16, s)), ("2: R = 3", two(x.ptr, x.ptr, None, None, 0, 64, 32, st.ptr, 3, BF16, s)),
           ("2: C = 40", two(x.ptr, x.ptr, None, None, 1, 64, 40, st.ptr, 4, BF16, s)), ("2: dtype", two(x.ptr, x.ptr, None, None, 1, 64, 32, st.ptr, 4, -1, s)),
           ("2: M = 0", two(x.ptr, x.ptr, None, None, 1, 0, 32, st.ptr, 4, BF16, s)), ("f32 C = 6", one(x.ptr, 64, 6, st.ptr, 4, F32, s))]
    torch.cuda.synchronize()
    assert all(rc != 0 for _, rc in bad), [n for n, rc in bad if rc == 0]
    assert np.array_equal(st.get().view(np.uint64), pre.view(np.uint64))


# ---- rua_bn_finalize / rua_bn_bwd_finalize / the prologue of rua_bn_fwd: one float32 ulp -----------------------------------------------------
def made_stats(rng, Cc, count, Rn):
    """([2][C] totals, [Rn][2][C] parts) of sum x, sum x^2 on the 2^-20 grid; channel 0 is a constant 1000.0: s2 / count - mean^2 cancels to 0."""
    mean, var = rng.standard_normal(Cc) * 2.0, rng.uniform(0.1, 3.0, Cc)
    tot = np.round(np.stack([mean * count, (var + mean * mean) * count]) / G20) * G20
    tot[:, 0] = 1000.0 * count, 1.0e6 * count
    return tot, split(tot, Rn, rng, G20)


def fwd_reference(tot, count, bessel_n, gamma, beta, mm, mv, training):
    """float64 (scale, shift, mean, rstd, new moving mean, new moving variance) of one branch."""
    if training:
        mean, var = R.bn_moments(tot[0], tot[1], count)
        nmm, nmv = R.bn_moving(mm, mv, mean, var, MOM, bessel_n) if mm is not None else (None, None)
    else:
        mean, var, nmm, nmv = mm.astype(f64), mv.astype(f64), mm.astype(f64), mv.astype(f64)
    scale, shift, rstd = R.bn_coeffs(mean, var, gamma, beta, EPS)
    return scale, shift, mean, rstd, nmm, nmv, var


@pytest.mark.parametrize("training", [1, 0])
@pytest.mark.parametrize("Rn", [1, 3, 8])
@pytest.mark.parametrize("Cc", [1, 63, 64, 65, 1000])
def test_bn_finalize_within_one_ulp(Cc, Rn, training):
    """The kernel computes in double and casts once, so every published float32 is within one ulp of the float64 reference: scale, shift, mean, rstd and
    the moving statistics (Bessel factor bessel_n / (bessel_n - 1); none at bessel_n = 1).  Blocks of 64 threads: C = 63, 64, 65 sit around one block.
    Also with the optional pointers null, and with count = bessel_n = 1.  In inference the moving statistics are the statistics and stay as they are."""
    lib = L.lib()
    for count, bessel_n, nulls in ((37.0, 37.0, False), (37.0, 37.0, True), (1.0, 1.0, False)):
        rng = np.random.default_rng(1000 * Cc + 10 * Rn + training)
        tot, parts = made_stats(rng, Cc, count, Rn)
        gamma, beta = signed(rng, 0.5, 1.5, Cc), rng.standard_normal(Cc).astype(f32)
        mm, mv = rng.standard_normal(Cc).astype(f32), rng.uniform(0.5, 2.0, Cc).astype(f32)
        moving = training == 0 or not nulls
        sc, sh, me, rs, nmm, nmv, var = fwd_reference(tot, count, bessel_n, gamma, beta, mm if moving else None, mv, training)
        if training:
            assert var[0] == 0.0 and rs[0] == 1.0 / np.sqrt(f64(EPS))
        st, gd, bd = Guarded(parts), fbuf(gamma), fbuf(beta)
        mmd, mvd = (fbuf(mm), fbuf(mv)) if moving else (None, None)
        out = [fnan(Cc) for _ in range(4)]
        o = out if not nulls else out[:2] + [None, None]
        lib.call("rua_bn_finalize", st.ptr, Rn, count, bessel_n, gd.ptr, bd.ptr, ptr(mmd), ptr(mvd), MOM, EPS, training,
                 o[0].ptr, o[1].ptr, ptr(o[2]), ptr(o[3]), Cc, stream())
        torch.cuda.synchronize()
        for name, buf, ref in (("scale", o[0], sc), ("shift", o[1], sh), ("mean", o[2], me), ("rstd", o[3], rs), ("moving mean", mmd, nmm), ("moving var", mvd, nmv)):
            if buf is not None:
                assert within_ulps(buf.get(), ref), (name, count, nulls)
        if not training:
            assert np.array_equal(mmd.get().view(np.uint32), mm.view(np.uint32)) and np.array_equal(mvd.get().view(np.uint32), mv.view(np.uint32))
        assert np.array_equal(st.get(), parts)


def made_stats2(rng, Cc, Rn):
    tot = np.round(np.stack([rng.standard_normal(Cc) * 5.0, rng.standard_normal(Cc) * 10.0]) / G20) * G20
    return tot, split(tot, Rn, rng, G20)


def grad_start(rng, d):
    """A non-zero start of a parameter gradient with the sign of what is added: the float32 sum then has two roundings (the cast of the addend, the add),
    each at most half an ulp of the result."""
    return np.copysign(rng.uniform(0.25, 1.0, d.shape), d).astype(f32)


@pytest.mark.parametrize("Rn", [1, 3, 8])
@pytest.mark.parametrize("Cc", [1, 63, 64, 65, 1000])
def test_bn_bwd_finalize_within_one_ulp(Cc, Rn):
    """A, B, C within one float32 ulp of the float64 reference; dgamma / dbeta add onto a non-zero start (and may be null)."""
    lib = L.lib()
    for nulls in (False, True):
        rng = np.random.default_rng(2000 * Cc + Rn)
        tot, parts = made_stats2(rng, Cc, Rn)
        gamma, mean, rstd = signed(rng, 0.5, 1.5, Cc), rng.standard_normal(Cc).astype(f32), rng.uniform(0.5, 2.0, Cc).astype(f32)
        A, B, Cq, dga, dbe = R.bn_bwd_coeffs(tot[0], tot[1], 37.0, gamma, mean, rstd)
        g0, b0 = grad_start(rng, dga), grad_start(rng, dbe)
        st, gd, md, rd = Guarded(parts), fbuf(gamma), fbuf(mean), fbuf(rstd)
        dgd, dbd = (None, None) if nulls else (fbuf(g0), fbuf(b0))
        co = [fnan(Cc) for _ in range(3)]
        lib.call("rua_bn_bwd_finalize", st.ptr, Rn, 37.0, gd.ptr, md.ptr, rd.ptr, ptr(dgd), ptr(dbd), co[0].ptr, co[1].ptr, co[2].ptr, Cc, stream())
        torch.cuda.synchronize()
        for name, buf, ref in (("A", co[0], A), ("B", co[1], B), ("C", co[2], Cq)):
            assert within_ulps(buf.get(), ref), (name, nulls)
        if not nulls:
            assert within_ulps(dgd.get(), g0.astype(f64) + dga), "dgamma"
            assert within_ulps(dbd.get(), b0.astype(f64) + dbe), "dbeta"


def fwd_desc(dt, M, Cc, nb, relu, training, count, bessel_n, x, shared, branches):
    """rua_bn_fwd_desc from Guarded buffers; branches: dicts of gamma, beta, mm, mv, scale, shift, mean, rstd, out, stats (buffer, replicas), out_stats."""
    d = L.BnFwdDesc()
    d.x, d.M, d.C, d.dtype, d.nb, d.relu, d.training = ptr(x), M, Cc, dt, nb, relu, training
    d.stats, d.replicas = (shared[0].ptr, shared[1]) if shared else (None, 0)
    d.count, d.bessel_n, d.momentum, d.eps = count, bessel_n, MOM, EPS
    for b, s in enumerate(branches):
        br = d.br[b]
        br.gamma, br.beta, br.moving_mean, br.moving_var = s["gamma"].ptr, s["beta"].ptr, ptr(s.get("mm")), ptr(s.get("mv"))
        br.scale, br.shift, br.mean, br.rstd, br.out = s["scale"].ptr, s["shift"].ptr, ptr(s.get("mean")), ptr(s.get("rstd")), ptr(s.get("out"))
        if s.get("stats"):
            br.stats, br.replicas = s["stats"][0].ptr, s["stats"][1]
        br.out_stats = ptr(s.get("out_stats"))
    return d


def fwd_branch(rng, Cc, tot, moving=True, mean_rstd=True, out_stats=False):
    """One branch's host values (h) and device buffers (s); tot: the statistics this branch normalises with."""
    h = {"gamma": signed(rng, 0.5, 1.5, Cc), "beta": rng.standard_normal(Cc).astype(f32), "tot": tot,
         "mm": rng.standard_normal(Cc).astype(f32) if moving else None, "mv": rng.uniform(0.5, 2.0, Cc).astype(f32)}
    s = {"gamma": fbuf(h["gamma"]), "beta": fbuf(h["beta"]), "scale": fnan(Cc), "shift": fnan(Cc)}
    if moving:
        s["mm"], s["mv"] = fbuf(h["mm"]), fbuf(h["mv"])
    if mean_rstd:
        s["mean"], s["rstd"] = fnan(Cc), fnan(Cc)
    if out_stats:
        s["out_stats"] = Guarded(np.full(2 * Cc, np.nan))
    return h, s


def check_fwd_coefficients(h, s, count, bessel_n, training):
    """What a rua_bn_fwd launch published for one branch against the float64 reference, one float32 ulp; returns the published (scale, shift)."""
    sc, sh, me, rs, nmm, nmv, var = fwd_reference(h["tot"], count, bessel_n, h["gamma"], h["beta"], h["mm"], h["mv"], training)
    for name, key, ref in (("scale", "scale", sc), ("shift", "shift", sh), ("mean", "mean", me), ("rstd", "rstd", rs), ("moving mean", "mm", nmm), ("moving var", "mv", nmv)):
        if key in s:
            assert within_ulps(s[key].get(), ref), name
    if not training:
        assert np.array_equal(s["mm"].get().view(np.uint32), h["mm"].view(np.uint32)) and np.array_equal(s["mv"].get().view(np.uint32), h["mv"].view(np.uint32))
    if "out_stats" in s:
        o1, o2 = R.bn_out_stats(count, h["beta"], sc, var)
        got = s["out_stats"].get()
        assert (np.abs(got - np.concatenate([o1, o2])) <= 1e-12 * np.abs(np.concatenate([o1, o2]))).all(), "out_stats"
    return s["scale"].get(), s["shift"].get()


@pytest.mark.parametrize("dt,Cc,R0,Rs", [(BF16, 64, 1, 3), (BF16, 1000, 3, 8), (F32, 1000, 8, 1), (F32, 4, 3, 3)])
def test_bn_fwd_coefficients_only_with_own_and_shared_statistics(dt, Cc, R0, Rs):
    """out == NULL, nb = 3: branch 0 normalises with statistics of its own, branches 1 and 2 with the shared ones; out_stats (float64, 1e-12) on branches 0 and
    2, moving statistics on 0 and 1, mean / rstd on 0 and 2.  One block, whatever M says."""
    rng = np.random.default_rng(Cc + R0)
    count = 37.0
    own, own_parts = made_stats(rng, Cc, count, R0)
    sh_tot, sh_parts = made_stats(rng, Cc, count, Rs)
    ownd, shd = Guarded(own_parts), Guarded(sh_parts)
    hs = [fwd_branch(rng, Cc, own, True, True, True), fwd_branch(rng, Cc, sh_tot, True, False, False), fwd_branch(rng, Cc, sh_tot, False, True, True)]
    hs[0][1]["stats"] = (ownd, R0)
    d = fwd_desc(dt, 5, Cc, 3, 0, 1, count, count, None, (shd, Rs), [s for _, s in hs])
    L.lib().call("rua_bn_fwd", C.byref(d), stream())
    torch.cuda.synchronize()
    for h, s in hs:
        check_fwd_coefficients(h, s, count, count, 1)


# ---- the sweeps of rua_bn_fwd / rua_bn_apply: one ulp of the storage type ------------------------------------------------------------------
def sweep_input(rng, M, Cc, dt):
    x = R.round_storage(rng.standard_normal((M, Cc)) * 1.5 + 0.3, bf(dt))
    x[rng.random(x.shape) < 0.02] = 0.0
    return x


def check_sweep(x, scale, shift, relu, out, dt):
    """out against [relu](scale x + shift) in float64 from the float32 coefficients: the kernel's one fma is correctly rounded, the storage rounding is the
    second half ulp; under ReLU a reference <= 0 has to come out as +0, bit for bit."""
    ref = R.bn_apply(x, scale.astype(f64), shift.astype(f64), relu)
    got = tval(out, dt)
    assert worst_ratio(np.abs(got - ref), ulp_of(ref, dt)) <= 1.0
    if relu:
        off = R.bn_apply(x, scale.astype(f64), shift.astype(f64), False) <= 0
        assert off.any() and (out.get()[off] == 0).all()


FWD_SWEEPS = ([(dt, 32, 77, nb, relu, 1, {}) for dt in DTYPES for nb in (1, 2, 3, 4) for relu in (0, 1)]        # registers; 77 rows: ragged against 256 threads
              + [(dt, 32, 77, nb, relu, 1, {"bn_regs": 0}) for dt in DTYPES for nb, relu in ((2, 1), (4, 0))]          # the table by key
              + [(dt, 40 if dt == BF16 else 24, 77, nb, 1, 1, {}) for dt in DTYPES for nb in (1, 3)]                   # the table by shape: 5 / 6 groups
              + [(dt, 512, 300, 2, 1, 1, {"bn_grid": 3}) for dt in DTYPES]                                            # replicas C >= 512: three blocks wrap, ragged tail
              + [(BF16, 8, PAST_CAP, 1, 1, 1, {})]                                                                     # past the 2048 blocks of grid_for
              + [(dt, 32, 77, 2, 1, 0, {}) for dt in DTYPES])                                                          # inference, outside a group


def sweep_id(c):
    return f"{DT_IDS[c[0] == BF16]}-C{c[1]}-M{c[2]}-nb{c[3]}-relu{c[4]}-train{c[5]}" + "".join(f"-{k}{v}" for k, v in c[6].items())


@pytest.mark.parametrize("case", FWD_SWEEPS, ids=[sweep_id(c) for c in FWD_SWEEPS])
def test_bn_fwd_sweep(case):
    """The launch's coefficients as in the prologue tests (statistics host-made from the float64 sums of x; with nb >= 3 branch 1 brings statistics of its
    own), then every output element against the float32 coefficients the launch published."""
    dt, Cc, M, nb, relu, training, tune = case
    rng = np.random.default_rng(Cc * 1000 + M % 1000 + 10 * nb + relu + 2 * training + len(tune))
    x = sweep_input(rng, M, Cc, dt)
    x64 = x.astype(f64)
    tot = np.stack([x64.sum(0), (x64 * x64).sum(0)])
    count = float(M)
    xd, shd = tbuf(x, dt), Guarded(split(tot, 2, rng))
    hs, own = [], None
    for b in range(nb):
        if nb >= 3 and b == 1:
            own = made_stats(rng, Cc, count, 3)
            h, s = fwd_branch(rng, Cc, own[0])
            s["stats"] = (Guarded(own[1]), 3)
        else:
            h, s = fwd_branch(rng, Cc, tot)
        s["out"] = Guarded(R.storage_bits(np.full((M, Cc), np.nan, f32), bf(dt)))
        hs.append((h, s))
    d = fwd_desc(dt, M, Cc, nb, relu, training, count, count, xd, (shd, 2), [s for _, s in hs])
    with tuning(**tune):
        L.lib().call("rua_bn_fwd", C.byref(d), stream())
        torch.cuda.synchronize()
    for h, s in hs:
        scale, shift = check_fwd_coefficients(h, s, count, count, training)
        check_sweep(x, scale, shift, relu, s["out"], dt)
    assert np.array_equal(xd.get(), R.storage_bits(x, bf(dt)))


APPLY_SWEEPS = ([(dt, 32, 77, nb, relu) for dt in DTYPES for nb in (1, 4) for relu in (0, 1)] + [(BF16, 40, 77, 3, 1), (F32, 24, 77, 2, 0), (BF16, 8, PAST_CAP, 1, 1)])


@pytest.mark.parametrize("dt,Cc,M,nb,relu", APPLY_SWEEPS, ids=[f"{DT_IDS[c[0] == BF16]}-C{c[1]}-M{c[2]}-nb{c[3]}-relu{c[4]}" for c in APPLY_SWEEPS])
def test_bn_apply_sweep(dt, Cc, M, nb, relu):
    rng = np.random.default_rng(Cc + M % 1000 + 10 * nb + relu)
    x = sweep_input(rng, M, Cc, dt)
    xd = tbuf(x, dt)
    sc, sh = [signed(rng, 0.5, 2.0, Cc) for _ in range(nb)], [rng.standard_normal(Cc).astype(f32) for _ in range(nb)]
    scd, shd = [fbuf(a) for a in sc], [fbuf(a) for a in sh]
    outs = [Guarded(R.storage_bits(np.full((M, Cc), np.nan, f32), bf(dt))) for _ in range(nb)]
    L.lib().call("rua_bn_apply", xd.ptr, nb, L.ptr_array([b.ptr for b in scd]), L.ptr_array([b.ptr for b in shd]), relu,
                 L.ptr_array([o.ptr for o in outs]), M, Cc, dt, stream())
    torch.cuda.synchronize()
    for b in range(nb):
        check_sweep(x, sc[b], sh[b], relu, outs[b], dt)


# ---- rua_bn_bwd / rua_bn_bwd_apply ---------------------------------------------------------------------------------------------------------
def bwd_grid(pieces, rmax, Cc, nb):
    """Blocks of a rua_bn_bwd launch (the launcher's rule): 256 pieces per block, at most 2048, and at most 2 (4 from 2^20 pieces) per compute unit
    where the prologue is long (rmax * C * nb >= 512)."""
    g = max(1, min(2048, (pieces + 255) // 256))
    cap = L.lib().get_tuning("bn_grid") or (4 if pieces >= 1 << 20 else 2) * torch.cuda.get_device_properties(0).multi_processor_count
    return min(g, cap) if rmax * Cc * nb >= 512 else g


def bwd_inputs(rng, dt, Cc, M, nb, masked):
    """x in multiples of 1/8 within [-4, 4], mask scale in {+-0.5, +-1, +-2}, mask shift in multiples of 1/16: the float32 fma of the mask is exact and some
    elements land on exactly zero (off, by the strict >).  g is Gaussian in the storage type, dskip and the old dx are integers in [-8, 8]."""
    x = (rng.integers(-32, 33, (M, Cc)) / 8.0).astype(f32)
    ms = [(rng.choice([0.5, 1.0, 2.0], Cc) * rng.choice([-1.0, 1.0], Cc)).astype(f32) for _ in range(nb)]
    mt = [(rng.integers(-32, 33, Cc) / 16.0).astype(f32) for _ in range(nb)]
    g = [R.round_storage(rng.standard_normal((M, Cc)), bf(dt)) for _ in range(nb)]
    masks = [R.relu_mask(x, ms[b], mt[b]) if masked else None for b in range(nb)]
    if masked and M * Cc >= 5000:
        assert all((ms[b].astype(f64) * x + mt[b] == 0).any() for b in range(nb))
    dskip, old = rng.integers(-8, 9, (M, Cc)).astype(f32), rng.integers(-8, 9, (M, Cc)).astype(f32)
    return x, ms, mt, g, masks, dskip, old


def check_dx(dxd, dt, ref, T, n):
    err = np.abs(tval(dxd, dt) - ref)
    r = worst_ratio(err, n * U32 * T + ulp_of(ref, dt))
    assert r <= 1.0, (r, n)


# (dt, C, M, nb, masked, dskip, accumulate, dx_stats replicas or 0, skip_stats, branch with stats2_out or None, tuning)
def bwd_cases():
    flags = [(1, 0, 1, 0, 0, 1), (1, 1, 0, 1, 1, 0), (2, 0, 0, 0, 1, 0), (2, 1, 1, 1, 0, 0), (3, 0, 1, 1, 1, 1), (3, 1, 0, 0, 0, 0), (4, 0, 0, 1, 0, 0), (4, 1, 1, 0, 1, 1),
             (1, 0, 0, 1, 0, 0), (1, 1, 1, 0, 0, 1), (4, 1, 0, 1, 0, 0), (4, 0, 1, 1, 2, 0)]
    out = [(dt, 32, 333, *f, None, {}) for dt in DTYPES for f in flags]                                   # registers, CG = 4 / 8: the shuffle fold
    for dt, Cc in ((BF16, 512), (F32, 1024)):                                                            # 64 / 256 groups: the fold through LDS alone
        out += [(dt, Cc, 40, 2, 1, 1, 0, 2, 1, None, {}), (dt, Cc, 40, 1, 0, 1, 1, 1, 1, None, {})]
    out += [(dt, 32, 333, *f, None, {"bn_regs": 0}) for dt in DTYPES for f in ((2, 1, 1, 1, 2, 1), (4, 0, 1, 0, 0, 0))]        # the table by key
    out += [(dt, 40 if dt == BF16 else 24, 333, *f, None, {}) for dt in DTYPES for f in ((2, 1, 1, 1, 0, 0), (3, 0, 1, 0, 0, 0))]   # the table by shape
    out += [(dt, 32, 333, 2, 1, 1, 0, 0, 0, 1, {}) for dt in DTYPES]                                     # stats2_out on branch 1
    out += [(dt, 32, 300, 1, 1, 0, 0, 8, 0, None, {}) for dt in DTYPES]                                  # 5 / 10 blocks onto 8 replicas: some receive nothing
    return out


BWD = bwd_cases()


def bwd_id(c):
    dt, Cc, M, nb, mk, sk, acc, dxs, sks, s2o, tune = c
    return (f"{DT_IDS[dt == BF16]}-C{Cc}-M{M}-nb{nb}-mask{mk}-skip{sk}-acc{acc}-dxs{dxs}-sks{sks}" + (f"-s2o{s2o}" if s2o is not None else "")
            + "".join(f"-{k}{v}" for k, v in tune.items()))


@pytest.mark.parametrize("case", BWD, ids=[bwd_id(c) for c in BWD])
def test_bn_bwd(case):
    """dx = [old] + [dskip] + B x + C + sum_b A_b g_b m_b against float64, with A_b, B_b, C_b from host-made stats2 (float64 sums of the reference, split
    unevenly over the replicas) and caller-made gamma, mean, rstd, scale, shift.
    Bound per element: n U32 T + one ulp of the storage type, T the sum of the terms' absolute values and n the float32 roundings of bn_bwd_body:
    the casts of A_b, B_b, C_b to float (3 nb), the branch sums of B and C (the first add onto 0.f is exact: 2 (nb - 1)), acc = fma(B, x, C) (1),
    acc += dskip (1 if given), acc += old (1 if accumulate), acc = fma(A_b, g_b m_b, acc) (nb): n = 6 nb - 1 + [dskip] + [accumulate].  The register
    form and the table form round at the same places.
    dgamma / dbeta: two float32 ulp on a non-zero start.  skip_stats slot 0: exact (integers).  dx_stats slots 0 / 1 against the float64 sums of the
    reference dx and dx x: (p + 8) U32 sum |summand| per channel, p the pieces a thread sweeps under the launcher's grid."""
    dt, Cc, M, nb, masked, use_skip, acc, dxs, sks, s2o, tune = case
    rng = np.random.default_rng(Cc * 7 + M + 100 * nb + 10 * masked + 3 * use_skip + acc + 5 * dxs + sks + len(tune))
    x, ms, mt, g, masks, dskip, old = bwd_inputs(rng, dt, Cc, M, nb, masked)
    count, x64 = float(M), x.astype(f64)
    reps = [2, 1, 3, 8][:nb]
    gamma = [signed(rng, 0.5, 1.5, Cc) for _ in range(nb)]
    mean, rstd = [rng.standard_normal(Cc).astype(f32) for _ in range(nb)], [rng.uniform(0.5, 2.0, Cc).astype(f32) for _ in range(nb)]
    As, Bs, Cs, st2, starts, grads = [], [], [], [], [], []
    for b in range(nb):
        gm = np.where(masks[b], g[b].astype(f64), 0.0) if masked else g[b].astype(f64)
        sg, sgx = gm.sum(0), (gm * x64).sum(0)
        slot1 = (gm * (ms[b].astype(f64) * x64 + mt[b])).sum(0) if s2o == b else sgx          # stats2_out: sum g m OUT, out = scale x + shift
        parts = split(np.stack([sg, slot1]), reps[b], rng)
        tot = parts.sum(0) if s2o != b else np.stack([sg, sgx])
        A, B, Cq, dga, dbe = R.bn_bwd_coeffs(tot[0], tot[1], count, gamma[b], mean[b], rstd[b])
        As.append(A); Bs.append(B); Cs.append(Cq); st2.append(Guarded(parts)); grads.append((dga, dbe))
        starts.append((grad_start(rng, dga), grad_start(rng, dbe)))
    ref, T = R.bn_bwd_apply(x64, g, As, masks, sum(Bs), sum(Cs), dskip if use_skip else None, old if acc else None)
    xd, gd, skd, dxd = tbuf(x, dt), [tbuf(a, dt) for a in g], tbuf(dskip, dt), tbuf(old, dt)
    keep = [[fbuf(a[b]) for a in (gamma, mean, rstd, ms, mt)] + [fbuf(starts[b][0]), fbuf(starts[b][1])] for b in range(nb)]
    e = L.BnBwdDesc()
    e.x, e.dskip, e.dx, e.M, e.C, e.dtype, e.nb, e.masked, e.accumulate, e.count = xd.ptr, skd.ptr if use_skip else None, dxd.ptr, M, Cc, dt, nb, masked, acc, count
    for b in range(nb):
        br, k = e.br[b], keep[b]
        br.g, br.stats2, br.replicas, br.stats2_out = gd[b].ptr, st2[b].ptr, reps[b], int(s2o == b)
        br.gamma, br.mean, br.rstd, br.scale, br.shift, br.dgamma, br.dbeta = (q.ptr for q in k)
    spre = rng.integers(1, 6, (2, 2, Cc)).astype(f64)
    dpre = rng.integers(1, 6, (max(dxs, 1), 2, Cc)).astype(f64)
    skst, dxst = Guarded(spre), Guarded(dpre)
    if sks:
        e.skip_stats, e.skip_replicas = skst.ptr, 2
    if dxs:
        e.dx_stats, e.dx_replicas = dxst.ptr, dxs
    with tuning(**tune):
        L.lib().call("rua_bn_bwd", C.byref(e), stream())
        torch.cuda.synchronize()
        p = -(-(M * Cc // vec(dt)) // (256 * bwd_grid(M * Cc // vec(dt), max(reps), Cc, nb)))
    check_dx(dxd, dt, ref, T, 6 * nb - 1 + use_skip + acc)
    for b in range(nb):
        assert within_ulps(keep[b][5].get(), starts[b][0].astype(f64) + grads[b][0], 2), ("dgamma", b)
        assert within_ulps(keep[b][6].get(), starts[b][1].astype(f64) + grads[b][1], 2), ("dbeta", b)
    got = skst.get().sum(0)
    assert np.array_equal(got[0], spre.sum(0)[0] + (dskip.astype(f64).sum(0) if sks else 0.0)) and np.array_equal(got[1], spre.sum(0)[1])
    got = dxst.get().sum(0) - dpre.sum(0)
    if dxs:
        for slot, summand in ((0, ref), (1, ref * x64)):
            r = worst_ratio(np.abs(got[slot] - summand.sum(0)), (p + 8) * U32 * np.abs(summand).sum(0))
            assert r <= 1.0, ("dx_stats", slot, r, p)
    else:
        assert (got == 0).all()
    assert np.array_equal(xd.get(), R.storage_bits(x, bf(dt)))


APPLY_BWD = [(BF16 if (nb + mk + sk + acc) % 2 else F32, nb, mk, sk, acc) for nb in (1, 4) for mk in (0, 1) for sk in (0, 1) for acc in (0, 1)]


@pytest.mark.parametrize("dt,nb,masked,use_skip,acc", APPLY_BWD, ids=[f"{DT_IDS[c[0] == BF16]}-nb{c[1]}-mask{c[2]}-skip{c[3]}-acc{c[4]}" for c in APPLY_BWD])
def test_bn_bwd_apply(dt, nb, masked, use_skip, acc):
    """The same expression with caller-made float32 A, B, C.  Roundings of bn_bwd_apply_kernel: the branch sums of B and C (2 (nb - 1)), acc = fma(B, x, C) (1),
    the adds of dskip and of the old dx (1 each), one fma per branch (nb): n = 3 nb - 1 + [dskip] + [accumulate].  C = 40 bf16 / 24 fp32: pieces of a row
    that do not divide the 256 threads (the kernel reads its coefficients from the LDS table at any shape)."""
    Cc, M = (40 if dt == BF16 else 24), 333
    rng = np.random.default_rng(50 + 8 * nb + 4 * masked + 2 * use_skip + acc)
    x, ms, mt, g, masks, dskip, old = bwd_inputs(rng, dt, Cc, M, nb, masked)
    A = [signed(rng, 0.5, 2.0, Cc) for _ in range(nb)]
    B, Cq = [(rng.standard_normal(Cc) * 0.1).astype(f32) for _ in range(nb)], [(rng.standard_normal(Cc) * 0.5).astype(f32) for _ in range(nb)]
    ref, T = R.bn_bwd_apply(x.astype(f64), g, A, masks, sum(b.astype(f64) for b in B), sum(c.astype(f64) for c in Cq), dskip if use_skip else None, old if acc else None)
    xd, gd, skd, dxd = tbuf(x, dt), [tbuf(a, dt) for a in g], tbuf(dskip, dt), tbuf(old, dt)
    bufs = [[fbuf(a[b]) for b in range(nb)] for a in (A, B, Cq, ms, mt)]
    arr = [L.ptr_array([q.ptr for q in col]) for col in bufs]
    L.lib().call("rua_bn_bwd_apply", nb, L.ptr_array([q.ptr for q in gd]), arr[0], arr[1], arr[2], arr[3], arr[4], masked, xd.ptr,
                 skd.ptr if use_skip else None, dxd.ptr, acc, M, Cc, dt, stream())
    torch.cuda.synchronize()
    check_dx(dxd, dt, ref, T, 3 * nb - 1 + use_skip + acc)


def test_bn_refusals_leave_the_outputs_alone():
    """An unknown dtype in rua_bn_apply / rua_bn_bwd_apply / rua_bn_fwd / rua_bn_bwd, and skip_stats / dx_stats at C = 40 bf16 (five channel groups: a thread does
    not stay on one group): non-zero, nothing written."""
    lib, s = L.lib(), stream()
    rng = np.random.default_rng(8)
    M, Cc = 64, 40
    x = (rng.integers(-32, 33, (M, Cc)) / 8.0).astype(f32)
    xd, gd = tbuf(x, BF16), tbuf(x, BF16)
    coef = fbuf(np.ones(Cc))
    pat = np.full((M, Cc), 0x7FC0, np.uint16)
    out = Guarded(pat)
    one = L.ptr_array([coef.ptr])
    bad = [("apply dtype", lib.raw("rua_bn_apply")(xd.ptr, 1, one, one, 1, L.ptr_array([out.ptr]), M, Cc, 7, s)),
           ("apply C = 12", lib.raw("rua_bn_apply")(xd.ptr, 1, one, one, 1, L.ptr_array([out.ptr]), M, 12, BF16, s)),
           ("bwd_apply dtype", lib.raw("rua_bn_bwd_apply")(1, L.ptr_array([gd.ptr]), one, one, one, one, one, 1, xd.ptr, None, out.ptr, 0, M, Cc, 7, s)),
           ("bwd_apply dtype -1", lib.raw("rua_bn_bwd_apply")(1, L.ptr_array([gd.ptr]), one, one, one, one, one, 1, xd.ptr, None, out.ptr, 0, M, Cc, -1, s))]
    st = Guarded(np.ones((2, 2, Cc)))
    side = Guarded(np.ones((2, 2, Cc)))
    for name, dtype, sks, dxs in (("bwd skip_stats at C = 40", BF16, 1, 0), ("bwd dx_stats at C = 40", BF16, 0, 1), ("bwd dtype", 7, 0, 0)):
        e = L.BnBwdDesc()
        e.x, e.dskip, e.dx, e.M, e.C, e.dtype, e.nb, e.masked, e.accumulate, e.count = xd.ptr, gd.ptr, out.ptr, M, Cc, dtype, 1, 0, 0, float(M)
        br = e.br[0]
        br.g, br.stats2, br.replicas, br.gamma, br.mean, br.rstd = gd.ptr, st.ptr, 2, coef.ptr, coef.ptr, coef.ptr
        if sks:
            e.skip_stats, e.skip_replicas = side.ptr, 2
        if dxs:
            e.dx_stats, e.dx_replicas = side.ptr, 2
        bad.append((name, lib.raw("rua_bn_bwd")(C.byref(e), s)))
    h, sb = fwd_branch(rng, Cc, None)
    sb["out"] = out
    d = fwd_desc(7, M, Cc, 1, 1, 1, float(M), float(M), xd, (st, 2), [sb])
    bad.append(("fwd dtype", lib.raw("rua_bn_fwd")(C.byref(d), s)))
    torch.cuda.synchronize()
    assert all(rc != 0 for _, rc in bad), [n for n, rc in bad if rc == 0]
    assert np.array_equal(out.get(), pat) and (side.get() == 1).all() and np.isnan(sb["scale"].get()).all()
