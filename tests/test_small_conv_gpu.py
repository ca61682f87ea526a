"""The stem and head kernels of csrc/small_conv.hip through the C ABI, on every path their launchers choose between.

1. Exact-integer cases.  Inputs are small integers (head weights: multiples of 1/64, or of 1/4 in the backward), so every product and every partial sum
   is a multiple of one grid step and stays below 2^24 steps: whatever the order of fmas, shuffles, LDS folds, float atomics and fp64 atomics, the
   fp32 result is the exact value, and the reference is float64 numpy (RNE to bf16 where the output is stored as bf16).  Each test checks the 2^24
   condition on the host with the SUMS OF ABSOLUTE VALUES of its own data (they bound every partial sum in every order) before it compares bits.
2. Real-valued cases against a float64 reference of the stored inputs, with per-element bounds k * u * S (u = 2^-24, S = |b| + sum |x_i w_i|), k the
   number of fp32 roundings on the longest path of the kernel form, written next to each use.
3. The fused head + loss entry points on the generic kernel and the CO = 8 forms.
4. Refusals.

Every output buffer has one guard row behind its last; the tuning keys a test sets are restored in a `finally` (tuning()).

Worst observed error / bound of the real-valued groups (MI355X, 256 CUs; pytest -s prints them):

  group                                              worst ratio
  stem forward y, fp32 (register and LDS forms)           0.690
  stem forward y, bf16 (the storage rounding dominates)   0.995
  head forward z, vector forms (head_fwd2, generic)       0.284
  head forward z, head_fwd3 (hi + lo)                     0.141
  head forward p vs float64 of the device's z             0.069
  saturating logits, p                                    0.001
  head backward dx, fp32                                  0.950
  head backward dx, bf16 (the storage rounding dominates) 0.996
  head backward dW / db / dxsum                           0.007
  stem backward dW / db                                   0.005

The ratios near 1 are bounds that are attained, not luck: a bf16 store errs by up to 2^-8 of a value just above a power of two, and a chain of two fmas
whose first product dominates errs by nearly 2 u S.  The summation bounds count the worst case of every add and are far from attained.
"""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from _kernel_util import bits_of, dev, stream, tdt, up, vec, worst_ratio  # noqa: E402
from resunet_a_mltsk_keras_amd import _lib as L  # noqa: E402

f32, f64 = np.float32, np.float64
F32, BF16 = L.RUA_F32, L.RUA_BF16
U = 2.0 ** -24                                                # unit roundoff of float32
GUARD = -77.0                                                 # exact in bf16; no result of an exact case reaches a whole row of it
ACTS = (L.ACT_NONE, L.ACT_SOFTMAX, L.ACT_SIGMOID)
DTN = {F32: "f32", BF16: "bf16"}


@functools.lru_cache(maxsize=None)
def cus():
    n = C.c_int32(0)
    assert L.lib().raw("rua_device_info")(C.byref(n), None, None, 0) == 0 and n.value > 0
    return n.value


@contextlib.contextmanager
def tuning(**kv):
    lib = L.lib()
    old = {k: lib.get_tuning(k) for k in kv}
    try:
        lib.set_tuning(**kv)
        yield
    finally:
        lib.set_tuning(**old)


def ptr(t):
    return None if t is None else t.data_ptr()


def ints(rng, lo, hi, shape):
    return rng.integers(lo, hi + 1, shape).astype(f64)


def fdev(a):
    return up(np.asarray(a, f32))


def sdev(a, dt):
    """Device copy in the storage type (RNE from float32, rounded on the host)."""
    return torch.from_numpy(np.ascontiguousarray(a, f32)).to(tdt(dt)).to(dev())


def stored(a, dt):
    """float64 of what sdev(a, dt) holds."""
    return torch.from_numpy(np.asarray(a, f32)).to(tdt(dt)).double().numpy()


def guarded(M, Cc, dtype):
    return torch.full((M + 1, Cc), GUARD, dtype=dtype, device=dev())


def guard_ok(t):
    return bool((t[-1] == GUARD).all())


def want_bits(v, dt):
    """Bits of the exact values v in the storage type: v must be float32-exact (checked), then RNE to bf16."""
    a = np.asarray(v, f64).astype(f32)
    assert np.array_equal(a.astype(f64), v)
    return bits_of(torch.from_numpy(a).to(tdt(dt)))


def exact_ok(abs_sums, lsb):
    """The condition of the method: sum |terms| of every output, in units of the grid step, is below 2^24 - so is every partial sum in any order."""
    assert float(np.max(abs_sums)) / lsb < 2.0 ** 24, float(np.max(abs_sums)) / lsb


def gamma(k):
    """k roundings: k u to first order (the second-order term, k u / 2 of it, is below 1e-5 of the bound for every k here)."""
    return k * U


def within(name, got, ref, bound):
    r = worst_ratio(np.abs(np.asarray(got, f64) - ref), bound)
    print(f"{name}: worst error / bound {r:.3f}")
    assert r <= 1.0, (name, r)
    return r


# ================================================================ stem forward ============================================================
def stem_call(x, w, b, M, Cin, Cout, dt, R=0, pack=False):
    """rua_stem_fwd (R = 0), rua_stem_fwd_stats (R replicas) or rua_stem_fwd_pack: (rc, y with guard row, stats [2 Cout] folded over replicas, xpack)."""
    lib = L.lib()
    y = guarded(M, Cout, tdt(dt))
    st = torch.zeros(max(R, 1) * 2 * Cout, dtype=torch.float64, device=dev())
    xp = guarded(M, 16, torch.bfloat16) if pack else None
    if pack:
        rc = lib.raw("rua_stem_fwd_pack")(ptr(x), ptr(w), ptr(b), ptr(y), M, Cin, Cout, dt, ptr(st) if R else None, max(R, 1), ptr(xp), stream())
    elif R:
        rc = lib.raw("rua_stem_fwd_stats")(ptr(x), ptr(w), ptr(b), ptr(y), M, Cin, Cout, dt, ptr(st), R, stream())
    else:
        rc = lib.raw("rua_stem_fwd")(ptr(x), ptr(w), ptr(b), ptr(y), M, Cin, Cout, dt, stream())
    torch.cuda.synchronize()
    return rc, y, st.view(max(R, 1), 2 * Cout).sum(0).cpu().numpy(), xp


def xpack_bits(x, M, Cin):
    xp = np.zeros((M, 16))
    xp[:, :Cin] = x                                            # hi = x, lo = 0 (x is bf16-exact), the column of ones
    xp[:, 15] = 1
    return want_bits(xp, BF16)


def stem_check(x, w, b, xd, wd, bd, M, Cin, Cout, dt, R, pack, what):
    yr = x @ w.T + b
    exact_ok(np.abs(x) @ np.abs(w).T + np.abs(b), 1.0)
    rc, y, st, xp = stem_call(xd, wd, bd, M, Cin, Cout, dt, R, pack)
    assert rc == 0, what
    assert np.array_equal(bits_of(y[:M]), want_bits(yr, dt)) and guard_ok(y), what
    if R:
        assert np.array_equal(st, np.concatenate([yr.sum(0), (yr * yr).sum(0)])), what
    if pack:
        assert np.array_equal(bits_of(xp[:M]), xpack_bits(x, M, Cin)) and guard_ok(xp), what
    return bits_of(y[:M]), st


STEM_CIN = [1, 3, 4, 6, 7, 8, 9, 16]
STEM_COUT = [8, 16, 24, 32, 128, 256]
STEM_M = [1, 63, 255, 256, 257]


@pytest.mark.parametrize("Cin", STEM_CIN)
@pytest.mark.parametrize("dt", [F32, BF16])
def test_stem_fwd_exact(dt, Cin):
    """y bit for bit, the statistics as exact integer sums over R replicas, xpack, and stem_reg = 0 (the LDS form) against 1 (the register form: runtime
    Cin for 1, 4, 8 - stem_fwd_reg_kernel<T, ST, 0> -, the 3 / 6 / 7 forms otherwise; Cin 9, 16 and Cout 24 take the LDS form whatever the key)."""
    rng = np.random.default_rng([Cin, dt, 1])
    for Cout in STEM_COUT:
        w, b = ints(rng, -1, 1, (Cout, Cin)), ints(rng, -1, 1, Cout)
        wd, bd = fdev(w), fdev(b)
        reg_ok = Cin <= 8 and 256 % (Cout // 8) == 0
        for M in STEM_M:
            x = ints(rng, -2, 2, (M, Cin))
            xd = fdev(x)
            exact_ok(M * 33.0 ** 2, 1.0)                       # the statistics: fp32 partial sums inside a block (fp64 from there) are part of the whole sum of y^2
            seen = []
            for reg in ((1, 0) if reg_ok else (1,)):
                with tuning(stem_reg=reg):
                    what = (DTN[dt], Cin, Cout, M, reg)
                    seen.append([stem_check(x, w, b, xd, wd, bd, M, Cin, Cout, dt, 0, False, what)[0]])
                    if Cout == 24:                               # three channel groups do not divide the block: no statistics
                        assert stem_call(xd, wd, bd, M, Cin, Cout, dt, 4)[0] != 0
                        continue
                    for R in (1, 4, 8):
                        seen[-1].append(stem_check(x, w, b, xd, wd, bd, M, Cin, Cout, dt, R, False, what + (R,))[1])
                    if reg_ok and Cin <= 7 and Cout >= 16 and reg == 1:
                        stem_check(x, w, b, xd, wd, bd, M, Cin, Cout, dt, 8, True, what + ("pack",))
                        stem_check(x, w, b, xd, wd, bd, M, Cin, Cout, dt, 0, True, what + ("pack, no stats",))
            if len(seen) == 2:                                   # the register form is bit-identical to the LDS form
                assert all(np.array_equal(a, c) for a, c in zip(seen[0], seen[1])), (DTN[dt], Cin, Cout, M)


@pytest.mark.parametrize("form,dt,Cin,Cout,R,pack", [
    ("reg", F32, 4, 8, 0, 0), ("reg", BF16, 6, 8, 0, 0), ("reg", F32, 7, 8, 8, 0), ("reg", BF16, 3, 8, 4, 0), ("reg", BF16, 8, 8, 1, 0),
    ("reg", BF16, 6, 16, 8, 1), ("reg", F32, 5, 16, 0, 1),
    ("lds", F32, 3, 8, 0, 0), ("lds", BF16, 9, 8, 0, 0), ("lds", F32, 6, 8, 8, 0), ("lds", BF16, 16, 16, 4, 0)])
def test_stem_fwd_past_the_grid_cap(form, dt, Cin, Cout, R, pack):
    """One size just past each form's grid cap, ragged: (stats ? 4 : 8) * CUs blocks of the register form, 4096 (2 * CUs with statistics) of the LDS form.
    Some threads make one sweep more than the others, and the register form's prefetch runs with a successor and without one."""
    rng = np.random.default_rng([Cin, Cout, dt, R, 2])
    CG8 = Cout // 8
    blocks = ((4 if R else 8) * cus()) if form == "reg" else (2 * cus() if R else 4096)
    sweeps = 2 if R else 1
    M = blocks * 256 * sweeps // CG8 + 77
    assert (M * CG8 + 255) // 256 > blocks                      # the cap binds
    x, w, b = ints(rng, -2, 2, (M, Cin)), ints(rng, -1, 1, (Cout, Cin)), ints(rng, -1, 1, Cout)
    exact_ok((sweeps + 1) * 256 * 33.0 ** 2, 1.0)              # statistics: what ONE block sums in fp32
    with tuning(stem_reg=1 if form == "reg" else 0):
        stem_check(x, w, b, fdev(x), fdev(w), fdev(b), M, Cin, Cout, dt, R, bool(pack), (form, DTN[dt], Cin, Cout, M))


# ================================================================ stem backward ===========================================================
def stem_bwd_pl(Cin, Cout):
    """Rows a block of stem_bwd_kernel takes per step, as rua_stem_bwd picks the instantiation: <T, 8, 1024>, <T, 8, 256> (Cout 128, 256), <T, 16, 256>."""
    nt = 1024 if (Cin <= 8 and 16 * Cout * 9 * 4 <= 64 * 1024 and 1024 % (Cout // 8) == 0) else 256
    return nt // (Cout // 8)


@pytest.mark.parametrize("dt,Cin,Cout", [(F32, 6, 32), (BF16, 3, 32), (BF16, 8, 8), (F32, 4, 8), (BF16, 5, 256), (F32, 7, 128), (BF16, 12, 32),
                                         (F32, 16, 16), (BF16, 9, 256)])
def test_stem_bwd_exact(dt, Cin, Cout):
    """dW and db as exact integer sums; a second call without db accumulates into dW and leaves db alone.  The last size gives every block more than
    2 * PL rows: the two-row loop runs, then the tail."""
    rng = np.random.default_rng([Cin, Cout, dt, 3])
    lib = L.lib()
    PL = stem_bwd_pl(Cin, Cout)
    for M in [1, 63, 64, 65, 129, 70001, cus() * (2 * PL + 1) + 5]:
        x, dy = ints(rng, -2, 2, (M, Cin)), ints(rng, -4, 4, (M, Cout))
        exact_ok(2 * np.abs(dy).T @ np.abs(x), 1.0)
        exact_ok(np.abs(dy).sum(0), 1.0)
        xd, dyd = fdev(x), sdev(dy, dt)
        dw, db = torch.zeros((Cout, Cin), device=dev()), torch.zeros(Cout, device=dev())
        lib.call("rua_stem_bwd", ptr(xd), ptr(dyd), ptr(dw), ptr(db), M, Cin, Cout, dt, stream())
        torch.cuda.synchronize()
        assert np.array_equal(dw.cpu().numpy(), dy.T @ x) and np.array_equal(db.cpu().numpy(), dy.sum(0)), (M,)
        lib.call("rua_stem_bwd", ptr(xd), ptr(dyd), ptr(dw), None, M, Cin, Cout, dt, stream())
        torch.cuda.synchronize()
        assert np.array_equal(dw.cpu().numpy(), 2 * (dy.T @ x)) and np.array_equal(db.cpu().numpy(), dy.sum(0)), (M, "second call")


@pytest.mark.parametrize("Cin,Cout", [(3, 32), (6, 32), (7, 16), (4, 16), (1, 32)])
def test_stem_bwd_packed_route_exact(Cin, Cout):
    """rua_stem_fwd_pack -> rua_conv_wgrad on the packed input (kind 3, asserted) -> rua_stem_bwd_fold, twice: exact sums, tmp left zero."""
    rng = np.random.default_rng([Cin, Cout, 4])
    lib = L.lib()
    dt = BF16
    for M in (2048, 4099, 70001):
        x, w, b, dy = ints(rng, -2, 2, (M, Cin)), ints(rng, -1, 1, (Cout, Cin)), ints(rng, -1, 1, Cout), ints(rng, -4, 4, (M, Cout))
        exact_ok(2 * np.abs(dy).T @ np.abs(x), 1.0)
        exact_ok(2 * np.abs(dy).sum(0), 1.0)
        rc, _, _, xp = stem_call(fdev(x), fdev(w), fdev(b), M, Cin, Cout, dt, 0, True)
        assert rc == 0 and np.array_equal(bits_of(xp[:M]), xpack_bits(x, M, Cin))
        dyd = sdev(dy, dt)
        tmp, ws = torch.zeros((Cout, 16), device=dev()), torch.zeros(8 << 20, device=dev())
        d = L.WgradDesc()
        d.a, d.C, d.Hs, d.Ws = xp.data_ptr(), 16, 1, M
        d.dy, d.Cout, d.H, d.W = dyd.data_ptr(), Cout, 1, M
        d.N, d.stride, d.dil, d.taps, d.dtype = 1, 1, 1, 1, dt
        d.dw, d.workspace, d.workspace_bytes = tmp.data_ptr(), ws.data_ptr(), ws.numel() * 4
        assert lib.raw("rua_wgrad_kind")(C.byref(d)) == 3
        dw, db = torch.zeros((Cout, Cin), device=dev()), torch.zeros(Cout, device=dev())
        for _ in range(2):
            lib.call("rua_conv_wgrad", C.byref(d), stream())
            lib.call("rua_stem_bwd_fold", ptr(tmp), ptr(dw), ptr(db), Cin, Cout, stream())
        torch.cuda.synchronize()
        assert np.array_equal(dw.cpu().numpy(), 2 * (dy.T @ x)) and np.array_equal(db.cpu().numpy(), 2 * dy.sum(0)), (M,)
        assert not tmp.any()


# ================================================================ head forward ============================================================
# (id, storage type, Cin, tuning keys): which kernel rua_head_fwd launches follows from its conditions - head_fwd3 for bf16 Cin = 32, head_fwd2 for
# Cin = 32 otherwise or with head_fwd3 = 0, the generic head_fwd_kernel for every other Cin or with both keys 0
HEAD_FORMS = [("fwd3", BF16, 32, {}), ("fwd2", F32, 32, {}), ("fwd2", BF16, 32, {"head_fwd3": 0}),
              ("generic", BF16, 8, {}), ("generic", BF16, 16, {}), ("generic", BF16, 64, {}), ("generic", BF16, 256, {}),
              ("generic", F32, 4, {}), ("generic", F32, 64, {}), ("generic", F32, 256, {}),
              ("generic", BF16, 32, {"head_fwd3": 0, "head_fwd2": 0}), ("generic", F32, 32, {"head_fwd2": 0})]
FORM_IDS = [f"{n}-{DTN[d]}-{c}" for n, d, c, _ in HEAD_FORMS]


def head_call(xd, wd, bd, M, Cin, Cout, act, dt, want_z=True):
    z, p = (guarded(M, Cout, torch.float32) if want_z else None), guarded(M, Cout, torch.float32)
    L.lib().call("rua_head_fwd", ptr(xd), ptr(wd), ptr(bd), ptr(z), ptr(p), M, Cin, Cout, act, dt, stream())
    torch.cuda.synchronize()
    return z, p


def head_exact_check(rng, M, Cin, Cout, dt, acts, what):
    x, w, b = ints(rng, -8, 8, (M, Cin)), ints(rng, -64, 64, (Cout, Cin)) / 64, ints(rng, -64, 64, Cout) / 64
    exact_ok(np.abs(x) @ np.abs(w).T + np.abs(b), 1 / 64)
    zb = want_bits(x @ w.T + b, F32)
    xd, wd, bd = sdev(x, dt), fdev(w), fdev(b)
    for act in acts:
        z, p = head_call(xd, wd, bd, M, Cin, Cout, act, dt)
        assert np.array_equal(bits_of(z[:M]), zb), what + (act,)
        assert guard_ok(z) and guard_ok(p) and not torch.isnan(p).any(), what + (act,)
        if act == L.ACT_NONE:
            assert np.array_equal(bits_of(p[:M]), zb), what


@pytest.mark.parametrize("form,dt,Cin,keys", HEAD_FORMS, ids=FORM_IDS)
def test_head_fwd_exact(form, dt, Cin, keys):
    rng = np.random.default_rng([Cin, dt, len(keys), 5])
    with tuning(**keys):
        for Cout in range(1, 9):
            for M in (1, 31, 63, 64, 65, 255, 257, 700):
                head_exact_check(rng, M, Cin, Cout, dt, ACTS, (form, DTN[dt], Cin, Cout, M))


@pytest.mark.parametrize("form,dt,Cin,Cout,keys", [("fwd3", BF16, 32, 8, {}), ("fwd3", BF16, 32, 6, {}), ("fwd2", F32, 32, 5, {}), ("fwd2", F32, 32, 3, {}),
                                                   ("fwd2", BF16, 32, 7, {"head_fwd3": 0}), ("generic", BF16, 8, 1, {})])
def test_head_fwd_second_pass(form, dt, Cin, Cout, keys):
    """Sizes at which a block of head_fwd3 / head_fwd2 makes a second pass that ends ragged (from the launchers' blocks per CU and smallest block), and
    one past the 4096-block cap of the generic kernel."""
    rng = np.random.default_rng([Cin, Cout, dt, 6])
    with tuning(**keys):
        if form == "fwd3":
            bpc = L.lib().get_tuning("head_fwd3_bpc") or 4
            M = 256 * bpc * cus() + 256 + 33                    # 257 pixels per block and up: 512; the last block holds 256 + 33
        elif form == "fwd2":
            PL = 256 // (32 // vec(dt))
            M = PL * 4 * cus() + PL + 33
        else:
            M = 4096 * 256 + 33
        head_exact_check(rng, M, Cin, Cout, dt, (L.ACT_NONE, L.ACT_SOFTMAX), (form, DTN[dt], Cin, Cout, M))


# ================================================================ head backward ===========================================================
def head_bwd_grid(M, Cin, Cout, sums):
    blocks = L.lib().get_tuning("head_blocks") or 2 * cus()
    rpb = max(64, (M + blocks - 1) // blocks)
    return (M + rpb - 1) // rpb, rpb, Cout * Cin + Cout + (Cin if sums else 0)


def head_bwd_call(xd, dzd, wd, M, Cin, Cout, dt, acc=0, mask=0, dx0=None, want_dx=True, want_db=True, sums=False, scratch="none", fetch_dx=True):
    """rua_head_bwd / rua_head_bwd_sums into dW = 1, db = 2, dxsum = 3 (they accumulate): float64 copies of dW, db, dxsum and the bits of dx."""
    lib = L.lib()
    dx = guarded(M, Cin, tdt(dt)) if want_dx else None
    if want_dx and acc:
        dx[:M] = dx0
    dw = torch.full((Cout, Cin), 1.0, device=dev())
    db = torch.full((Cout,), 2.0, device=dev()) if want_db else None
    dxs = torch.full((Cin,), 3.0, device=dev()) if sums else None
    g, _, ne = head_bwd_grid(M, Cin, Cout, sums)
    scr = torch.full((g * ne + 1,), GUARD, device=dev()) if scratch != "none" else None
    nbytes = 0 if scr is None else g * ne * 4 - (4 if scratch == "short" else 0)
    if sums:
        lib.call("rua_head_bwd_sums", ptr(xd), ptr(dzd), ptr(wd), ptr(dx), acc, ptr(dw), ptr(db), ptr(dxs), ptr(scr), nbytes, M, Cin, Cout, dt, mask, stream())
    else:
        lib.call("rua_head_bwd", ptr(xd), ptr(dzd), ptr(wd), ptr(dx), acc, ptr(dw), ptr(db), ptr(scr), nbytes, M, Cin, Cout, dt, mask, stream())
    torch.cuda.synchronize()
    if scr is not None:
        assert scr[-1] == GUARD
        if scratch == "short":                                   # four bytes short: the atomic path, the buffer stays untouched
            assert bool((scr == GUARD).all())
    if dx is not None:
        assert guard_ok(dx)
    out = [t.double().cpu().numpy() if t is not None else None for t in (dw, db, dxs)]
    return out + [bits_of(dx[:M]) if dx is not None and fetch_dx else None]


def head_bwd_ref(x, dz, w, dx0, acc, mask):
    o = dz @ w + (dx0 if acc else 0.0)
    if mask:
        o = np.where(x > 0, o, 0.0)
    return 1 + dz.T @ x, 2 + dz.sum(0), 3 + o.sum(0), o


def head_bwd_exact_case(x, dz, w, dx0, xd, dzd, wd, dx0d, M, Cin, Cout, dt, acc, mask, sums, with_dx, what):
    """The three scratch variants of one case: each exact, hence bit-identical to each other."""
    dwr, dbr, sr, o = head_bwd_ref(x, dz, w, dx0, acc, mask)
    ob = want_bits(o, dt) if with_dx else None
    for scratch in ("none", "ok", "short"):
        fetch = with_dx and (scratch == "none" or M < 4096)      # the large sizes: dx is compared once, dW / db / dxsum for all three
        dw, db, dxs, dxb = head_bwd_call(xd, dzd, wd, M, Cin, Cout, dt, acc, mask, dx0d, with_dx, True, sums and with_dx, scratch, fetch)
        assert np.array_equal(dw, dwr) and np.array_equal(db, dbr), what + (scratch,)
        if sums and with_dx:
            assert np.array_equal(dxs, sr), what + (scratch,)
        if fetch:
            assert np.array_equal(dxb, ob), what + (scratch,)


HEAD_BWD = [(BF16, 8), (BF16, 32), (BF16, 64), (BF16, 256), (F32, 4), (F32, 32), (F32, 128), (F32, 256)]


@pytest.mark.parametrize("dt,Cin", HEAD_BWD, ids=[f"{DTN[d]}-{c}" for d, c in HEAD_BWD])
def test_head_bwd_exact(dt, Cin):
    """dW, db, dxsum exact and dx bit for bit (RNE of the exact value) for Cout 1..8 (head_bwd_kernel<T, 8> and the 6 / 3 forms).  Small sizes: accumulate_dx
    x mask_dx x the three scratch variants, then dx = NULL and db = NULL.  Large sizes (the pair loop; with 2 * CUs blocks its `more` branch needs more
    than 3 * PL rows per block, which the last size gives Cin = 32 and any size gives the wide Cin): one flag pair per Cout, all four over the Couts."""
    rng = np.random.default_rng([Cin, dt, 7])
    PL = 256 // (Cin // vec(dt))
    esz = 2 if dt == BF16 else 4
    small, large = [1, 63, 64, 65, 200], [40017, 70001]
    if Cin == 32:
        large.append(2 * cus() * (3 * PL + 1) + 17)
    for M in small + large:
        x, dz8, dx0 = ints(rng, -8, 8, (M, Cin)), ints(rng, -4, 4, (M, 8)), ints(rng, -4, 4, (M, Cin))
        with_dx = 3 * M * Cin * esz <= 64 << 20                 # x, dx and its preset together within 64 MB; beyond: the dx = NULL form only
        xd, dx0d = sdev(x, dt), (sdev(dx0, dt) if with_dx else None)
        for Cout in range(1, 9):
            dz = np.ascontiguousarray(dz8[:, :Cout])
            w = ints(rng, -4, 4, (Cout, Cin)) / 4               # k / 64 with k a multiple of 16: dx and dxsum are multiples of 1 / 4
            exact_ok(np.abs(dz).T @ np.abs(x) + 1, 1.0)
            exact_ok((np.abs(dz) @ np.abs(w) + np.abs(dx0)).sum(0) + 3, 1 / 4)
            dzd, wd = fdev(dz), fdev(w)
            what = (DTN[dt], Cin, Cout, M)
            flags = [(a, m) for a in (0, 1) for m in (0, 1)] if M in small else [((Cout >> 1) & 1, Cout & 1)]
            for acc, mask in flags:
                head_bwd_exact_case(x, dz, w, dx0, xd, dzd, wd, dx0d, M, Cin, Cout, dt, acc, mask, (acc + mask + Cout) % 2 == 0 or M not in small,
                                    with_dx, what + (acc, mask))
            if M in small or not with_dx:
                dwr, dbr, _, o = head_bwd_ref(x, dz, w, dx0, 0, 1)
                dw, db, _, dxb = head_bwd_call(xd, dzd, wd, M, Cin, Cout, dt, 0, 1, None, False, True, False, "ok")        # dx = NULL
                assert np.array_equal(dw, dwr) and np.array_equal(db, dbr) and dxb is None, what + ("dx NULL",)
            if M in small:
                dw, db, dxs, dxb = head_bwd_call(xd, dzd, wd, M, Cin, Cout, dt, 0, 1, None, True, False, True, "none")      # db = NULL
                assert np.array_equal(dw, dwr) and db is None and np.array_equal(dxs, 3 + o.sum(0)) and np.array_equal(dxb, want_bits(o, dt)), what + ("db NULL",)


@pytest.mark.parametrize("dt,Cin,Cout", [(BF16, 32, 6), (BF16, 32, 8), (F32, 32, 3), (BF16, 64, 2), (F32, 4, 5)])
def test_head_bwd_one_block_equals_the_default_grid(dt, Cin, Cout):
    """head_blocks = 1: one block walks every row through the pair loop and its `more` branch; same bits as the default grid (both exact)."""
    rng = np.random.default_rng([Cin, Cout, dt, 8])
    PL = 256 // (Cin // vec(dt))
    for M in (200, 4 * PL + 3, 40017):
        x, dz, dx0, w = ints(rng, -8, 8, (M, Cin)), ints(rng, -4, 4, (M, Cout)), ints(rng, -4, 4, (M, Cin)), ints(rng, -4, 4, (Cout, Cin)) / 4
        exact_ok(np.abs(dz).T @ np.abs(x) + 1, 1.0)
        exact_ok((np.abs(dz) @ np.abs(w) + np.abs(dx0)).sum(0) + 3, 1 / 4)
        xd, dzd, wd, dx0d = sdev(x, dt), fdev(dz), fdev(w), sdev(dx0, dt)
        dwr, dbr, sr, o = head_bwd_ref(x, dz, w, dx0, 1, 1)
        outs = []
        for blocks in (0, 1):
            with tuning(head_blocks=blocks):
                for scratch in ("none", "ok"):
                    outs.append(head_bwd_call(xd, dzd, wd, M, Cin, Cout, dt, 1, 1, dx0d, True, True, True, scratch))
        for dw, db, dxs, dxb in outs:
            assert np.array_equal(dw, dwr) and np.array_equal(db, dbr) and np.array_equal(dxs, sr) and np.array_equal(dxb, want_bits(o, dt)), (M,)


# ================================================================ real-valued cases =======================================================
MR = 4099


def stored_out_bound(ref, bound, dt):
    """A bf16-stored output adds one RNE rounding of the computed value: 2^-8 (|ref| + bound) covers the half ulp of anything within the bound."""
    return bound + (2.0 ** -8 * (np.abs(ref) + bound) if dt == BF16 else 0.0)


@pytest.mark.parametrize("dt,Cin,Cout,reg", [(F32, 6, 32, 1), (BF16, 6, 32, 1), (F32, 4, 16, 1), (BF16, 7, 8, 1), (F32, 6, 32, 0), (BF16, 12, 32, 1), (F32, 6, 24, 1),
                                             (BF16, 16, 256, 1)])
def test_stem_fwd_real(dt, Cin, Cout, reg):
    """y = b + sum_c x_c w_c as a chain of Cin fmas that starts at the bias (both forms): Cin roundings."""
    rng = np.random.default_rng([Cin, Cout, dt, reg, 9])
    x, w, b = (rng.standard_normal(s).astype(f32).astype(f64) for s in ((MR, Cin), (Cout, Cin), (Cout,)))
    with tuning(stem_reg=reg):
        rc, y, _, _ = stem_call(fdev(x), fdev(w), fdev(b), MR, Cin, Cout, dt)
    assert rc == 0 and guard_ok(y)
    ref, S = x @ w.T + b, np.abs(x) @ np.abs(w).T + np.abs(b)
    within(f"stem fwd y {DTN[dt]} {Cin}->{Cout} reg={reg}", y[:MR].double().cpu().numpy(), ref, stored_out_bound(ref, gamma(Cin) * S, dt))


def head_k(form, dt, Cin):
    """fp32 roundings on the longest path to a logit.  generic: Cin fmas from the bias.  head_fwd2: VEC fmas (the first one rounds the product alone), log2(32 / VEC)
    shuffle adds, the bias add."""
    if form == "generic":
        return Cin
    return vec(dt) + (2 if dt == BF16 else 3) + 1


def act_ref(z, act):
    """float64 activation of the device's own logits and the per-element tolerance: 1e-5 relative, 2^-24 |z_c - max z| (|z_c| for the sigmoid) for the
    rounding of the exponent's argument, 2^-126 absolute."""
    z = z.astype(f64)
    if act == L.ACT_SOFTMAX:
        d = z - z.max(1, keepdims=True)
        e = np.exp(d)
        pr = e / e.sum(1, keepdims=True)
    else:
        d = z
        with np.errstate(over="ignore"):
            pr = 1.0 / (1.0 + np.exp(-z))
    return pr, pr * (1e-5 + U * np.abs(d)) + 2.0 ** -126


REAL_FORMS = [("fwd3", BF16, 32, {}), ("fwd2", F32, 32, {}), ("fwd2", BF16, 32, {"head_fwd3": 0}), ("generic", BF16, 64, {}), ("generic", F32, 16, {}),
              ("generic", BF16, 32, {"head_fwd3": 0, "head_fwd2": 0})]
REAL_IDS = [f"{n}-{DTN[d]}-{c}" for n, d, c, _ in REAL_FORMS]


@pytest.mark.parametrize("form,dt,Cin,keys", REAL_FORMS, ids=REAL_IDS)
def test_head_fwd_real(form, dt, Cin, keys):
    rng = np.random.default_rng([Cin, dt, len(keys), 10])
    x = stored(rng.standard_normal((MR, Cin)), dt)
    xd = sdev(x, dt)
    for Cout in (2, 5, 6):
        w, b = rng.standard_normal((Cout, Cin)).astype(f32).astype(f64) / 4, rng.standard_normal(Cout).astype(f32).astype(f64)
        ref, S = x @ w.T + b, np.abs(x) @ np.abs(w).T + np.abs(b)
        # head_fwd3: the weights as bf16 hi + lo (the lo part rounded to 8 bits: 2^-16 relative to each product), two chains of 32 fp32 adds on the matrix
        # pipe and the bias add
        bound = (gamma(64 + 1) + 2.0 ** -16) * S if form == "fwd3" else gamma(head_k(form, dt, Cin)) * S
        for act in (L.ACT_SOFTMAX, L.ACT_SIGMOID):
            with tuning(**keys):
                z, p = head_call(xd, fdev(w), fdev(b), MR, Cin, Cout, act, dt)
            assert guard_ok(z) and guard_ok(p)
            zg = z[:MR].cpu().numpy()
            within(f"head fwd z {form} {DTN[dt]} {Cin}->{Cout}", zg, ref, bound)
            pr, tol = act_ref(zg, act)
            within(f"head fwd p {form} {DTN[dt]} {Cin}->{Cout} act={act}", p[:MR].cpu().numpy(), pr, tol)


@pytest.mark.parametrize("form,dt,Cin,keys", REAL_FORMS, ids=REAL_IDS)
def test_head_fwd_saturating_logits(form, dt, Cin, keys):
    """Logits of exactly +T, -T and 0 (one-hot integer x, weights of +-T): T = 60 for the softmax and, beyond expf's range - what the subtraction of the
    row maximum is for -, 100; T = 100 for the sigmoid, where expf(-z) is inf."""
    M = 777
    for Cout in (2, 5, 8):
        j = np.arange(M) % Cout
        x = np.zeros((M, Cin))
        x[np.arange(M), j] = 1
        for act, T in ((L.ACT_SOFTMAX, 60.0), (L.ACT_SOFTMAX, 100.0), (L.ACT_SIGMOID, 100.0)):
            w = np.zeros((Cout, Cin))
            for c in range(Cout):
                w[(c + 1) % Cout, c] = -T                       # input c on: class c at +T, the next class at -T, the others 0
                w[c, c] = T
            with tuning(**keys):
                z, p = head_call(sdev(x, dt), fdev(w), None, M, Cin, Cout, act, dt)
            zg, pg = z[:M].cpu().numpy(), p[:M].cpu().numpy()
            assert np.array_equal(zg, x @ w.T) and guard_ok(p)
            assert not np.isnan(pg).any()
            pr, tol = act_ref(zg, act)
            within(f"saturating p {form} {DTN[dt]} Cout={Cout} act={act} T={T}", pg, pr, tol)
            if act == L.ACT_SOFTMAX:
                assert np.abs(pg.astype(f64).sum(1) - 1).max() <= 8 * U
            r32 = pr.astype(f32)
            sat = (r32 == 0) | (r32 == 1)
            assert sat.any() and np.array_equal(pg[sat], r32[sat])


@pytest.mark.parametrize("dt,Cin", [(BF16, 32), (F32, 32), (BF16, 64), (F32, 4), (BF16, 256)])
def test_head_bwd_real(dt, Cin):
    """dx: a chain of Cout fmas from 0 (or from the stored dx): Cout roundings, + the storage rounding.  dW, db, dxsum: rows per thread (sequential adds)
    + PL / 4 + 2 (the column fold of the block's tile), then blocks / 64 + 64 through the scratch buffer or one atomic per block without it."""
    rng = np.random.default_rng([Cin, dt, 11])
    M = MR
    PL = 256 // (Cin // vec(dt))
    x, dx0 = stored(rng.standard_normal((M, Cin)), dt), stored(rng.standard_normal((M, Cin)), dt)
    xd, dx0d = sdev(x, dt), sdev(dx0, dt)
    worst = [0.0, 0.0]
    for Cout in (2, 5, 6):
        dz, w = rng.standard_normal((M, Cout)).astype(f32).astype(f64), rng.standard_normal((Cout, Cin)).astype(f32).astype(f64) / 4
        g, rpb, _ = head_bwd_grid(M, Cin, Cout, True)
        for acc, mask, scratch in ((0, 0, "none"), (1, 1, "ok"), (1, 0, "short")):
            dw, db, dxs, dxb = head_bwd_call(xd, fdev(dz), fdev(w), M, Cin, Cout, dt, acc, mask, dx0d, True, True, True, scratch)
            dwr, dbr, _, o = head_bwd_ref(x, dz, w, dx0, acc, mask)
            So = np.abs(dz) @ np.abs(w) + (np.abs(dx0) if acc else 0.0)
            if mask:
                So = np.where(x > 0, So, 0.0)
            bo = stored_out_bound(o, gamma(Cout) * So, dt)
            dxg = torch.from_numpy(dxb.view(np.int16) if dt == BF16 else dxb.view(np.int32)).view(tdt(dt)).double().numpy()
            worst[0] = max(worst[0], within(f"head bwd dx {DTN[dt]} {Cin} Cout={Cout} {acc}{mask}", dxg, o, bo))
            k = -(-rpb // PL) + PL // 4 + 2 + (-(-g // 64) + 64 if scratch == "ok" else g)
            worst[1] = max(worst[1], within("head bwd dW", dw, dwr, gamma(k) * (np.abs(dz).T @ np.abs(x) + 1)))
            worst[1] = max(worst[1], within("head bwd db", db, dbr, gamma(k) * (np.abs(dz).sum(0) + 2)))
            # dxsum adds the values of dx BEFORE their storage rounding: their own error (gamma(Cout) So) rides along
            worst[1] = max(worst[1], within("head bwd dxsum", dxs, 3 + o.sum(0), gamma(k) * (So.sum(0) + 3) + gamma(Cout) * So.sum(0)))
    print(f"head bwd real {DTN[dt]} Cin={Cin}: dx {worst[0]:.3f}, sums {worst[1]:.3f}")


@pytest.mark.parametrize("dt,Cin,Cout", [(F32, 6, 32), (BF16, 7, 256), (BF16, 12, 32)])
def test_stem_bwd_real(dt, Cin, Cout):
    """dW, db: rows per thread, 6 shuffle adds at the most, one add per wave of the block, one atomic per block."""
    rng = np.random.default_rng([Cin, Cout, dt, 12])
    M = MR
    x, dy = rng.standard_normal((M, Cin)).astype(f32).astype(f64), stored(rng.standard_normal((M, Cout)), dt)
    xd, dyd = fdev(x), sdev(dy, dt)
    dw, db = torch.zeros((Cout, Cin), device=dev()), torch.zeros(Cout, device=dev())
    L.lib().call("rua_stem_bwd", ptr(xd), ptr(dyd), ptr(dw), ptr(db), M, Cin, Cout, dt, stream())
    torch.cuda.synchronize()
    PL = stem_bwd_pl(Cin, Cout)
    blocks = L.lib().get_tuning("stem_blocks") or cus()
    rpb = max(64, -(-M // blocks))
    k = -(-rpb // PL) + 6 + 16 + -(-M // rpb)
    within(f"stem bwd dW {DTN[dt]} {Cin}->{Cout}", dw.double().cpu().numpy(), dy.T @ x, gamma(k) * (np.abs(dy).T @ np.abs(x)))
    within(f"stem bwd db {DTN[dt]} {Cin}->{Cout}", db.double().cpu().numpy(), dy.sum(0), gamma(k) * np.abs(dy).sum(0))


# ================================================================ fused head + loss =======================================================
def moments(p, y, keep):
    """[B][C][6] of rua_tanimoto_sums in float64, over the pixels of `keep` [B][HW]."""
    P, Y, K = p.astype(f64), y.astype(f64), keep[:, :, None].astype(f64)
    return np.stack([(K * P).sum(1), (K * (1 - Y)).sum(1), (K * P * Y).sum(1), (K * (P * P + Y * Y)).sum(1), (K * (1 - P) * (1 - Y)).sum(1),
                     (K * ((1 - P) ** 2 + (1 - Y) ** 2)).sum(1)], axis=-1)


def metric_counts(p, y, keep):
    p, y = p[keep], y[keep]
    t, q = y > 0.5, p > 0.5
    return np.array([(p.argmax(1) == y.argmax(1)).sum(), (t & q).sum(), (~t & q).sum(), (~t & ~q).sum(), (t & ~q).sum()], f64)


def loss_call(name, xd, wd, bd, yd, B, HW, Cin, Cout, act, dt, R=1, vm=None, want_z=True, want_sums=True, want_metrics=True):
    lib = L.lib()
    M = B * HW
    z, p = (guarded(M, Cout, torch.float32) if want_z else None), guarded(M, Cout, torch.float32)
    s = torch.zeros(R * B * Cout * 6, dtype=torch.float64, device=dev()) if want_sums else None
    m = torch.zeros(5, dtype=torch.float64, device=dev()) if want_metrics else None
    if name == "rua_head_fwd_loss":
        rc = lib.raw(name)(ptr(xd), ptr(wd), ptr(bd), ptr(z), ptr(p), ptr(yd), ptr(s), ptr(m), B, HW, Cin, Cout, act, dt, stream())
    elif name == "rua_head_fwd_loss_rep":
        rc = lib.raw(name)(ptr(xd), ptr(wd), ptr(bd), ptr(z), ptr(p), ptr(yd), ptr(s), R, ptr(m), B, HW, Cin, Cout, act, dt, stream())
    else:
        rc = lib.raw(name)(ptr(xd), ptr(wd), ptr(bd), ptr(z), ptr(p), ptr(yd), ptr(s), R, ptr(m), B, HW, Cin, Cout, act, dt, ptr(vm), stream())
    torch.cuda.synchronize()
    return rc, z, p, (s.view(R, B, Cout, 6).sum(0).cpu().numpy() if want_sums else None), (m.cpu().numpy() if want_metrics else None)


def loss_case(rng, B, HW, Cin, Cout, act, dt, full):
    M = B * HW
    xd = sdev(rng.standard_normal((M, Cin)), dt)
    wd, bd = fdev(rng.standard_normal((Cout, Cin)) / 4), fdev(rng.standard_normal(Cout))
    y = np.eye(Cout, dtype=f32)[rng.integers(0, Cout, M)]
    yd = fdev(y)
    z0, p0 = head_call(xd, wd, bd, M, Cin, Cout, act, dt)
    pg = p0[:M].cpu().numpy()
    void = rng.random((B, HW)) < 0.3
    if B > 1:
        void[1] = True                                           # a whole void sample
    vm = up(np.where(void, rng.integers(1, 256, void.shape), 0).astype(np.uint8))
    everything = np.ones((B, HW), bool)
    runs = [("rua_head_fwd_loss_rep", 8, None)]
    if full:
        runs += [("rua_head_fwd_loss", 1, None), ("rua_head_fwd_loss_rep", 1, None), ("rua_head_fwd_loss_void", 1, vm)]
    runs.append(("rua_head_fwd_loss_void", 8, vm))
    for name, R, mask in runs:
        what = (name, R, B, HW, Cin, Cout, act, DTN[dt])
        rc, z, p, s, m = loss_call(name, xd, wd, bd, yd, B, HW, Cin, Cout, act, dt, R, mask)
        assert rc == 0 and torch.equal(z, z0) and torch.equal(p, p0), what            # guard rows included
        keep = ~void if mask is not None else everything
        assert np.allclose(s, moments(pg.reshape(B, HW, Cout), y.reshape(B, HW, Cout), keep), rtol=2e-5, atol=1e-3), what
        assert np.array_equal(m, metric_counts(pg, y, keep.reshape(-1))), what
        if mask is not None and B > 1:
            assert not s[1].any()
    rc, z, p, s, m = loss_call("rua_head_fwd_loss_void", xd, wd, bd, yd, B, HW, Cin, Cout, act, dt, 8, vm, want_z=False, want_metrics=False)   # z = NULL
    assert rc == 0 and torch.equal(p, p0)
    assert np.allclose(s, moments(pg.reshape(B, HW, Cout), y.reshape(B, HW, Cout), ~void), rtol=2e-5, atol=1e-3)
    for name in ("rua_head_fwd_loss", "rua_head_fwd_loss_rep", "rua_head_fwd_loss_void"):
        assert loss_call(name, xd, wd, bd, yd, B, HW, Cin, Cout, act, dt, 1, None, want_sums=False, want_metrics=False)[0] != 0      # nothing to accumulate


LOSS_FORMS = [("generic", BF16, 64, {}), ("generic", F32, 16, {}), ("fwd3", BF16, 32, {}), ("fwd2", F32, 32, {}), ("fwd2", BF16, 32, {"head_fwd3": 0})]


@pytest.mark.parametrize("form,dt,Cin,keys", LOSS_FORMS, ids=[f"{n}-{DTN[d]}-{c}" for n, d, c, _ in LOSS_FORMS])
def test_head_fwd_loss_paths(form, dt, Cin, keys):
    """head_fwd_loss_kernel (generic) and the CO = 8 forms of head_fwd2 / head_fwd3 with LOSS, with and without a void mask."""
    rng = np.random.default_rng([Cin, dt, len(keys), 13])
    with tuning(**keys):
        for Cout in (2, 5, 8):
            for HW in (1, 255, 700):
                for act in (L.ACT_SOFTMAX, L.ACT_SIGMOID):
                    loss_case(rng, 3, HW, Cin, Cout, act, dt, full=True)


def test_head_fwd3_loss_three_passes_per_block():
    """B = 1024, HW = 700: one block per sample, three passes, the last ragged."""
    loss_case(np.random.default_rng(14), 1024, 700, 32, 2, L.ACT_SOFTMAX, BF16, full=False)


# ================================================================ refusals ================================================================
def test_refusals():
    lib = L.lib()
    t = torch.zeros(1 << 16, device=dev())
    d8 = torch.zeros(1 << 16, dtype=torch.float64, device=dev())
    a, s = t.data_ptr(), stream()
    M = 64
    for Cin, Cout in ((0, 32), (17, 32), (6, 12), (6, 264)):
        assert lib.raw("rua_stem_fwd")(a, a, a, a, M, Cin, Cout, F32, s) != 0
        assert lib.raw("rua_stem_fwd_stats")(a, a, a, a, M, Cin, Cout, F32, d8.data_ptr(), 4, s) != 0
        assert lib.raw("rua_stem_bwd")(a, a, a, a, M, Cin, Cout, F32, s) != 0
    assert lib.raw("rua_stem_fwd_pack")(a, a, a, a, M, 8, 32, BF16, d8.data_ptr(), 4, a, s) != 0
    assert lib.raw("rua_stem_fwd_pack")(a, a, a, a, M, 6, 8, BF16, d8.data_ptr(), 4, a, s) != 0
    assert lib.raw("rua_stem_bwd_fold")(a, a, a, 8, 32, s) != 0
    assert lib.raw("rua_stem_bwd")(a, a, a, a, M, 6, 24, F32, s) != 0
    for dt, Cin, Cout in ((F32, 32, 0), (BF16, 32, 9), (BF16, 12, 6), (F32, 6, 6), (F32, 264, 6), (BF16, 264, 6)):
        assert lib.raw("rua_head_fwd")(a, a, a, a, a, M, Cin, Cout, L.ACT_SOFTMAX, dt, s) != 0
        assert lib.raw("rua_head_fwd_loss")(a, a, a, a, a, a, d8.data_ptr(), d8.data_ptr(), 1, M, Cin, Cout, L.ACT_SOFTMAX, dt, s) != 0
        assert lib.raw("rua_head_bwd")(a, a, a, a, 0, a, a, None, 0, M, Cin, Cout, dt, 0, s) != 0
    assert lib.raw("rua_head_bwd")(a, a, a, a, 0, a, a, None, 0, M, 24, 6, BF16, 0, s) != 0
    assert lib.raw("rua_head_bwd_sums")(a, a, a, None, 0, a, a, a, None, 0, M, 32, 6, BF16, 0, s) != 0
    for R in (0, 65):
        assert lib.raw("rua_head_fwd_loss_rep")(a, a, a, a, a, a, d8.data_ptr(), R, d8.data_ptr(), 1, M, 32, 6, L.ACT_SOFTMAX, BF16, s) != 0
        assert lib.raw("rua_head_fwd_loss_void")(a, a, a, a, a, a, d8.data_ptr(), R, d8.data_ptr(), 1, M, 32, 6, L.ACT_SOFTMAX, BF16, None, s) != 0
    torch.cuda.synchronize()
    assert not t.any() and not d8.any()                          # nothing ran
