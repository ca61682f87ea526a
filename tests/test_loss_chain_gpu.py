"""The first half of csrc/loss_optim.hip through the C ABI: the Tanimoto moments, the finalizers, the gradient with respect to the logits, the
segmentation counts, the plain per-pixel losses, and the fused producers of csrc/small_conv.hip that fill the same moments.  Every comparison is
with the float64 references of tests/_loss_ref.py (checked against the oracle in tests/test_loss_ref_host.py), never with another kernel.

1. Exact cases.  p and y are multiples of 1/8 in [0, 1], so every term of the six moments is a multiple of 1/64 no larger than 2 and any partial sum
   of n pixels is exact in fp32 while 128 n < 2^24 (asserted on the block size of each launch): the moments equal the float64 reference bit for bit
   on every route, with every mask form, whatever the order.  The counts of rua_seg_metrics are integers and exact on any data; multiples of 1/8
   make ties of the argmax and values of exactly 0.5 the rule.
2. Real-valued cases with counted bounds k * u * S, u = 2^-24: S the sum of the absolute values of the terms that form an element, k the number of
   fp32 roundings on the longest path, written next to each use.  A libm call (expf, logf, log1pf) counts as two ulps = 4 u.
3. The finalizers are driven from host-made float64 moments, so any class volume V can be planted: V = 0 (the weight is replaced by the largest
   finite one), every V = 0 (all weights 0), V = 1e-21 (infinite under the reference's float32 rule, finite in float64) and V = 2e-19 (finite).
   Loss: 64 * 2^-53 relative, a float64 evaluation of the same expressions.  coef and per_sample are stored as float32: half a float32 ulp of the
   reference plus 64 * 2^-53 of the magnitudes that form the value.
4. Refusals leave their outputs alone.

Every buffer a kernel writes sits between guard regions (Guarded); tuning keys are restored in a `finally` (tuning()).

Worst observed error / bound of the real-valued groups (MI355X, 256 CUs; pytest -s prints them):

  group                                                        worst ratio
  Tanimoto moments, vector and scalar kernels                       0.028
  finalize, _rep, _multi: loss, per_sample, coef                    1.000
  rua_tanimoto_ratio                                                0.999
  sums -> finalize -> dz against autograd: dz                       0.016
  the same chain: loss                                              0.002
  head dz, plain kinds (C = 1, 3, 5, 6, 8; p off alignment)         0.756
  head dz past the grid cap                                         0.651
  head dz multi, unequal heads                                      0.550
  pixel loss, per pixel                                             0.744
  pixel loss, total                                                 0.111
  fused head + loss moments: generic / head_fwd2 / head_fwd3        0.147 / 0.080 / 0.085

The finalizers' 1.000 is a bound that is attained, not luck: among thousands of float32 stores some value lies next to the midpoint of two floats and
errs by the half ulp the bound grants (the float64 part of the allowance is ~1e-7 of it).  The summation bounds count the worst case of every add and
are far from attained; the chain's bound multiplies the moments' count through the finalizer's quotients.

Three places where counting found more than the first model of a bound held, each written where it is used:
  - per_sample is stored as float32 like coef, so it has the half ulp of the store on top of its float64 allowance;
  - c0's allowance takes the absolute values of the products inside kap, not |kap|: kap is a difference itself (for C = 1 it cancels to ~1e-5 of its
    terms), and with |kap| the float64 reference misses an exact (200-bit) evaluation of the planted cases by up to 140 bounds;
  - the per-pixel losses add 2^-126 per operation to k u S: log1p(exp(-100)) = 3.7e-44 is a denormal float32 and has no relative accuracy.
"""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _loss_ref as R  # noqa: E402
from _kernel_util import Guarded, dev, stream, ulp_of, up, worst_ratio  # noqa: E402
from resunet_a_mltsk_keras_amd import _lib as L  # noqa: E402

f32, f64 = np.float32, np.float64
U = 2.0 ** -24                                                # unit roundoff of float32
D64 = 64 * 2.0 ** -53                                         # the float64 allowance of the finalizer tests
MAX_HEADS = 8                                                 # RUA_MAX_HEADS of include/rua_hip.h
SOFTMAX, SIGMOID, NONE = L.ACT_SOFTMAX, L.ACT_SIGMOID, L.ACT_NONE
ACTN = {SOFTMAX: "softmax", SIGMOID: "sigmoid", NONE: "none"}
KINDN = {L.LOSS_TANIMOTO: "tanimoto", L.LOSS_WCE: "wce", L.LOSS_CE_LOGITS: "ce", L.LOSS_BCE_LOGITS: "bce", L.LOSS_MSE: "mse"}
assert (R.TANIMOTO, R.WCE, R.CE_LOGITS, R.BCE_LOGITS, R.MSE) == (L.LOSS_TANIMOTO, L.LOSS_WCE, L.LOSS_CE_LOGITS, L.LOSS_BCE_LOGITS, L.LOSS_MSE)
assert (R.ACT_NONE, R.ACT_SOFTMAX, R.ACT_SIGMOID) == (NONE, SOFTMAX, SIGMOID)


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


def cdiv(a, b):
    return -(-a // b)


def within(name, got, ref, bound):
    r = worst_ratio(np.abs(np.asarray(got, f64) - ref), bound)
    print(f"{name}: worst error / bound {r:.3f}")
    assert r <= 1.0, (name, r)
    return r


def dyadic(rng, shape):
    return (rng.integers(0, 9, shape) / 8).astype(f32)


def shifted(a):
    """(tensor that owns the memory, address of a copy of `a` that starts 4 bytes into the allocation): aligned to 4 bytes and to nothing more."""
    a = np.ascontiguousarray(a, f32).reshape(-1)
    t = torch.zeros(a.size + 1, dtype=torch.float32, device=dev())
    t[1:] = torch.from_numpy(a).to(dev())
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + 4


def softmax32(z):
    e = np.exp(z - z.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(f32)


def sigmoid32(z):
    return (1.0 / (1.0 + np.exp(-z))).astype(f32)


def probabilities(rng, shape, act):
    z = rng.standard_normal(shape) * 2
    return softmax32(z) if act == SOFTMAX else sigmoid32(z)


def labels(rng, shape, act):
    """One-hot under a softmax, independent 0 / 1 channels under a sigmoid."""
    if act == SOFTMAX:
        return np.eye(shape[-1], dtype=f32)[rng.integers(0, shape[-1], shape[:-1])]
    return (rng.random(shape) > 0.6).astype(f32)


# ---- void masks -----------------------------------------------------------------------------------------------------------------
MASK_FORMS = ("none", "random", "one_per_group", "whole_groups")


def void_of(rng, form, B, HW, G):
    """[B][HW] bool, True = void, or None.  Groups are the G consecutive pixels a thread of the vector kernels takes at once."""
    if form == "none":
        return None
    void = np.zeros((B, HW), bool)
    ng = HW // G
    if form == "random":
        void = rng.random((B, HW)) < 0.3
    elif form == "one_per_group" and ng:
        idx = rng.integers(0, G, (B, ng)) + G * np.arange(ng)[None, :]
        np.put_along_axis(void, idx, True, axis=1)
    elif form == "whole_groups" and ng:
        void[:, :ng * G] = np.repeat(rng.random((B, ng)) < 0.4, G, axis=1)
    return void


def mask_bytes(rng, void):
    """Device bytes 1..255 on the void pixels, 0 elsewhere, at an odd address (the mask has no alignment)."""
    b = np.where(void, rng.integers(1, 256, void.shape), 0).astype(np.uint8).reshape(-1)
    t = torch.zeros(b.size + 1, dtype=torch.uint8, device=dev())
    t[1:] = torch.from_numpy(b).to(dev())
    return t, t.data_ptr() + 1


def with_nan(a, void):
    if void is None:
        return a
    a = a.copy()
    a[void] = np.nan
    return a


# ================================================================ rua_tanimoto_sums ======================================================
VEC_G = {6: 2, 3: 4, 2: 2}                                   # pixels per thread and iteration of tanimoto_sums_vec<C, G>


def sums_route(HW, Cc, aligned, tani_vec):
    return bool(tani_vec) and HW % 4 == 0 and aligned and Cc in VEC_G


def sums_grid(HW, Cc, vec):
    """(terms one thread adds to one of its accumulators, pixels of a block) as the launchers of rua_tanimoto_sums_void size their grids."""
    if vec:
        G = VEC_G[Cc]
        gpb = cdiv(max(cdiv(HW // G, 64), 256), 256) * 256
        return gpb // 256 * G, gpb * G
    ppb = cdiv(max(cdiv(HW, 128), 1024), 256) * 256
    return ppb // 256, ppb


def prefill(B, Cc):
    """Non-zero dyadic values: the kernels ADD into sums."""
    return ((np.arange(B * Cc * 6) % 37 + 1) / 64).reshape(B, Cc, 6).astype(f64)


def call_sums(p_ptr, y_ptr, vm_ptr, B, HW, Cc, sums_ptr):
    lib = L.lib()
    if vm_ptr is None:
        rc = lib.raw("rua_tanimoto_sums")(p_ptr, y_ptr, B, HW, Cc, sums_ptr, stream())
    else:
        rc = lib.raw("rua_tanimoto_sums_void")(p_ptr, y_ptr, vm_ptr, B, HW, Cc, sums_ptr, stream())
    torch.cuda.synchronize()
    return rc


def sums_exact(rng, B, HW, Cc, form, shift=None):
    """One exact case under the tuning in force: the moments of multiples of 1/8, bit for bit.  Returns what the kernel left in sums."""
    tani_vec = L.lib().get_tuning("tani_vec")
    vec = sums_route(HW, Cc, shift is None, tani_vec)
    void = void_of(rng, form, B, HW, VEC_G.get(Cc, 2))
    p, y = dyadic(rng, (B, HW, Cc)), dyadic(rng, (B, HW, Cc))
    keep = np.ones((B, HW), bool) if void is None else ~void
    want = prefill(B, Cc) + R.moments(p, y, keep)
    # the condition of the method, for BOTH routes' blocks (a term is at most 2 = 128 / 64)
    assert 128 * max(sums_grid(HW, Cc, True)[1] if Cc in VEC_G else 0, sums_grid(HW, Cc, False)[1]) < 2 ** 24
    pn, yn = with_nan(p, void), with_nan(y, void)
    pt, pp = shifted(pn) if shift == "p" else (up(pn), None)
    yt, yp = shifted(yn) if shift == "y" else (up(yn), None)
    vt, vp = mask_bytes(rng, void) if void is not None else (None, None)
    out = Guarded(prefill(B, Cc))
    rc = call_sums(pp or pt.data_ptr(), yp or yt.data_ptr(), vp, B, HW, Cc, out.ptr)
    got = out.get()
    what = (B, HW, Cc, form, shift, "vec" if vec else "scalar")
    assert rc == 0, what
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (what, np.abs(got - want).max())
    return got


@pytest.mark.parametrize("Cc", [6, 3, 2])
def test_sums_exact_on_the_vector_route_and_with_it_switched_off(Cc):
    """HW = 36868: 18434 groups of two (C = 6, 2) in blocks of 512 - two iterations per thread, the last block holds 2 groups; HW = 65540: 16385
    groups of four (C = 3), one group in the last block.  The same seed under tani_vec = 0 sends the same inputs through the scalar kernel: both
    equal the reference, so the routes agree bit for bit."""
    for HW in (4, 8, 1020, 1024, 36868, 65540):
        for form in MASK_FORMS:
            seed = [Cc, HW, MASK_FORMS.index(form), 21]
            with tuning(tani_vec=1):
                assert sums_route(HW, Cc, True, L.lib().get_tuning("tani_vec"))
                a = sums_exact(np.random.default_rng(seed), 3, HW, Cc, form)
            with tuning(tani_vec=0):
                b = sums_exact(np.random.default_rng(seed), 3, HW, Cc, form)
            assert np.array_equal(a, b)
    assert sums_grid(36868, 6, True) == (4, 1024) and 36868 // 2 % 512 == 2 and sums_grid(65540, 3, True) == (8, 2048) and 65540 // 4 % 512 == 1


@pytest.mark.parametrize("Cc", [6, 3, 2])
def test_sums_exact_on_the_scalar_route_of_the_vector_class_counts(Cc):
    with tuning(tani_vec=1):
        for HW in (1, 3, 4321, 65541):
            for form in MASK_FORMS:
                sums_exact(np.random.default_rng([Cc, HW, MASK_FORMS.index(form), 22]), 3, HW, Cc, form)
        for shift in ("p", "y"):
            for form in ("none", "one_per_group"):
                sums_exact(np.random.default_rng([Cc, ord(shift), 23]), 3, 1024, Cc, form, shift=shift)


@pytest.mark.parametrize("Cc", [1, 4, 5, 7, 8])
def test_sums_exact_for_the_other_class_counts(Cc):
    for HW in (1, 255, 257, 65541):
        for form in MASK_FORMS:
            sums_exact(np.random.default_rng([Cc, HW, MASK_FORMS.index(form), 24]), 3, HW, Cc, form)


def test_sums_refusals_leave_the_sums_alone():
    t = torch.zeros(64, device=dev())
    out = Guarded(prefill(1, 8))
    a = t.data_ptr()
    assert call_sums(a, a, None, 1, 4, 0, out.ptr) != 0
    assert call_sums(a, a, None, 1, 4, 9, out.ptr) != 0
    assert call_sums(a, a, None, 1, 0, 6, out.ptr) != 0
    assert call_sums(None, a, None, 1, 4, 6, out.ptr) != 0
    assert call_sums(a, None, None, 1, 4, 6, out.ptr) != 0
    assert call_sums(a, a, None, 1, 4, 6, None) != 0
    assert call_sums(a, a, a, 0, 4, 6, out.ptr) != 0
    assert np.array_equal(out.get(), prefill(1, 8))


# Roundings of one moment on its longest path: the T terms a thread adds (T - 1 adds, and the fma of columns 2 and 4 is the add), the roundings
# inside a term - at most 5, in column 5: q = 1 - p and m = 1 - l (each enters squared: 2 + 2 u of the term), q * q, m * m and their sum count
# 2 + 2 + 1 against the larger square - and 6 shuffle levels.  The waves' sums and the blocks' atomics are fp64.  Every term is >= 0, so the
# bound is relative to the moment itself.
def sums_k(T):
    return T + 5 + 6


@pytest.mark.parametrize("Cc,HW", [(6, 36868), (3, 65540), (2, 36868), (6, 4321), (1, 65541), (5, 65541), (8, 65541)])
def test_sums_real_valued(Cc, HW):
    rng = np.random.default_rng([Cc, HW, 25])
    B = 3
    worst = 0.0
    for act in (SOFTMAX, SIGMOID):
        for form in ("none", "random"):
            void = void_of(rng, form, B, HW, 2)
            p, y = probabilities(rng, (B, HW, Cc), act), labels(rng, (B, HW, Cc), act)
            keep = np.ones((B, HW), bool) if void is None else ~void
            ref = R.moments(p, y, keep)
            pt, yt = up(with_nan(p, void)), up(with_nan(y, void))
            vt, vp = mask_bytes(rng, void) if void is not None else (None, None)
            out = Guarded(np.zeros((B, Cc, 6)))
            assert call_sums(pt.data_ptr(), yt.data_ptr(), vp, B, HW, Cc, out.ptr) == 0
            T, _ = sums_grid(HW, Cc, sums_route(HW, Cc, True, L.lib().get_tuning("tani_vec")))
            worst = max(worst, within(f"sums C={Cc} HW={HW} {ACTN[act]} {form}", out.get(), ref, sums_k(T) * U * ref))
    print(f"tanimoto sums real C={Cc} HW={HW}: {worst:.3f}")


# ================================================================ the finalizers =========================================================
def host_sums(p, y, q, m):
    """Moments [B][C][6] from float64 p, y and their complements given separately (a planted complement volume of 1e-21 does not survive 1 - y)."""
    return np.stack([p.sum(1), m.sum(1), (p * y).sum(1), (p * p + y * y).sum(1), (q * m).sum(1), (q * q + m * m).sum(1)], axis=-1)


PLANTS = ("none", "one_zero", "all_zero", "1e-21", "2e-19")


def planted_sums(rng, B, Cc, plant, term):
    """Moments of random data in which class c of term 1 (the prediction volumes, column 0) or of term 2 (the complement label volumes, column 1)
    has the planted mean volume; the other columns follow from the same scaled data, so the moments stay those of an image."""
    HWs = 16
    p, y = rng.random((B, HWs, Cc)), (rng.random((B, HWs, Cc)) > 0.6).astype(f64)
    q, m = 1.0 - p, 1.0 - y
    a = p if term == 1 else m
    c = min(1, Cc - 1)
    if plant == "one_zero":
        a[:, :, c] = 0.0
    elif plant == "all_zero":
        a[:] = 0.0
    elif plant != "none":
        a[:, :, c] *= float(plant) / (a[:, :, c].sum() / B)
    if term == 1:
        q = 1.0 - p
    else:
        y = 1.0 - m
    s = host_sums(p, y, q, m)
    if plant in ("1e-21", "2e-19"):
        V = s[:, c, 0 if term == 1 else 1].sum() / B
        assert abs(V - float(plant)) < 1e-6 * float(plant) and not (5e-20 <= V <= 1.2e-19)
    return s, c


def call_finalize(sums, B, Cc, gs, want_per=True, want_coef=True):
    sd = up(np.ascontiguousarray(sums, f64))
    loss, per, coef = Guarded(np.full(1, -3.0)), Guarded(np.full(B, -3.0, f32)), Guarded(np.full((B, Cc, 3), -3.0, f32))
    rc = L.lib().raw("rua_tanimoto_finalize")(sd.data_ptr(), B, 16, Cc, gs, loss.ptr, coef.ptr if want_coef else None, per.ptr if want_per else None, stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert torch.equal(sd.cpu(), torch.from_numpy(np.ascontiguousarray(sums, f64)))                  # one replica: sums is only read
    return loss.get()[0], per.get(), coef.get()


def check_final(name, fin, loss, per, coef, per_given=True, coef_given=True):
    """Loss: D64 relative.  per_sample and coef are float32 stores of float64 values: half an ulp of the store plus D64 of the magnitudes (c1 and c2
    are sums of same-signed terms; c0 = kap + a2 (F2 - E2) is a difference, and kap is one too - sum_n Spl E1 - F1 (SS - Spl), which for C = 1
    cancels to ~1e-5 of its terms - so c0's allowance is on the absolute values of all those products, _loss_ref.finalize().coef_mag.  With |kap|
    in their place the float64 reference itself is up to 140 bounds away from an exact evaluation of the planted cases)."""
    assert abs(loss - fin.loss) <= D64 * abs(fin.loss), (name, loss, fin.loss)
    r = 0.0
    if per_given:
        r = max(r, worst_ratio(np.abs(per.astype(f64) - fin.per_sample), 0.5 * ulp_of(fin.per_sample, L.RUA_F32) + D64 * np.abs(fin.per_sample)))
    else:
        assert (per == f32(-3.0)).all()
    if coef_given and fin.coef is not None:
        assert np.isfinite(fin.coef).all() and np.abs(fin.coef).max() < 3e38, name
        r = max(r, worst_ratio(np.abs(coef.astype(f64) - fin.coef), 0.5 * ulp_of(fin.coef, L.RUA_F32) + D64 * fin.coef_mag))
    else:
        assert coef is None or (coef == f32(-3.0)).all()
    assert r <= 1.0, (name, r)
    return r


@pytest.mark.parametrize("Cc", [1, 3, 6, 8])
@pytest.mark.parametrize("B", [1, 3, 64, 65, 256])
def test_finalize(B, Cc):
    """B > 64: the one wave strides over the samples; B = 256 fills the E / F tables."""
    rng = np.random.default_rng([B, Cc, 31])
    gs = float(f32(0.7 / B))
    worst = 0.0
    for plant in PLANTS:
        for term in (1, 2):
            if plant == "none" and term == 2:
                continue
            s, c = planted_sums(rng, B, Cc, plant, term)
            fin = R.finalize(s, B, Cc, gs)
            rep = fin.replaced1 if term == 1 else fin.replaced2
            assert rep.tolist() == [(plant in ("one_zero", "1e-21") and i == c) or plant == "all_zero" for i in range(Cc)], (plant, term)
            if plant == "all_zero":
                assert not (fin.w1 if term == 1 else fin.w2).any()
            worst = max(worst, check_final((B, Cc, plant, term), fin, *call_finalize(s, B, Cc, gs)))
    s, _ = planted_sums(rng, B, Cc, "one_zero", 1)
    fin = R.finalize(s, B, Cc, gs)
    check_final((B, Cc, "no per_sample"), fin, *call_finalize(s, B, Cc, gs, want_per=False), per_given=False)
    check_final((B, Cc, "no coef"), fin, *call_finalize(s, B, Cc, gs, want_coef=False), coef_given=False)
    print(f"tanimoto finalize B={B} C={Cc}: {worst:.3f}")


def test_finalize_refusals():
    sd = up(np.ones(257 * 8 * 6))
    loss, per = Guarded(np.full(1, -3.0)), Guarded(np.full(257, -3.0, f32))
    lib = L.lib()
    for B, Cc in ((0, 6), (257, 6), (3, 0), (3, 9)):
        assert lib.raw("rua_tanimoto_finalize")(sd.data_ptr(), B, 16, Cc, 0.1, loss.ptr, None, per.ptr, stream()) != 0
        assert lib.raw("rua_tanimoto_ratio")(sd.data_ptr(), B, Cc, loss.ptr, per.ptr, stream()) != 0
    assert lib.raw("rua_tanimoto_finalize")(None, 3, 16, 6, 0.1, loss.ptr, None, per.ptr, stream()) != 0
    assert lib.raw("rua_tanimoto_finalize")(sd.data_ptr(), 3, 16, 6, 0.1, None, None, per.ptr, stream()) != 0
    assert lib.raw("rua_tanimoto_ratio")(sd.data_ptr(), 3, 6, loss.ptr, None, stream()) != 0
    for rep in (0, 65):
        assert lib.raw("rua_tanimoto_finalize_rep")(sd.data_ptr(), rep, 3, 16, 6, 0.1, loss.ptr, None, per.ptr, stream()) != 0
    torch.cuda.synchronize()
    assert loss.get()[0] == -3.0 and (per.get() == f32(-3.0)).all() and bool((sd == 1).all())


def replica_sums(rng, reps, B, Cc):
    """[reps + 1][B][C][6]: every replica holds the moments of its own random pixels; the slot behind them starts as -3."""
    buf = np.full((reps + 1, B, Cc, 6), -3.0)
    for r in range(reps):
        buf[r], _ = planted_sums(rng, B, Cc, "none", 1)
    return buf


@pytest.mark.parametrize("B", [1, 256])
@pytest.mark.parametrize("reps", [1, 2, 7, 64])
def test_finalize_rep_folds_in_replica_order(reps, B):
    rng = np.random.default_rng([reps, B, 32])
    Cc, gs = 6, float(f32(0.25))
    buf = replica_sums(rng, reps, B, Cc)
    folded = R.fold(buf[:reps], reps)
    fin = R.finalize(folded, B, Cc, gs)
    sd = Guarded(buf)
    loss, per, coef = Guarded(np.full(1, -3.0)), Guarded(np.full(B, -3.0, f32)), Guarded(np.full((B, Cc, 3), -3.0, f32))
    seen = []
    for _ in range(2):
        assert L.lib().raw("rua_tanimoto_finalize_rep")(sd.ptr, reps, B, 16, Cc, gs, loss.ptr, coef.ptr, per.ptr, stream()) == 0
        torch.cuda.synchronize()
        seen.append((sd.get(), loss.get(), per.get(), coef.get()))
    got = seen[0][0]
    assert np.array_equal(got[:reps].view(np.uint64), buf[:reps].view(np.uint64))                    # the replicas are only read
    if reps > 1:
        assert np.array_equal(got[reps].view(np.uint64), folded.view(np.uint64))
    else:
        assert (got[1] == -3.0).all()                                                                # one replica: nothing to fold, nothing stored
    for a, b in zip(seen[0], seen[1]):                                                               # a second call changes no bit anywhere
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    r = check_final((reps, B), fin, seen[0][1][0], seen[0][2], seen[0][3])
    print(f"tanimoto finalize_rep replicas={reps} B={B}: {r:.3f}")


HEAD_SETS = [(3, 6, 2, 0.25), (1, 1, 1, 0.5), (64, 3, 1, 1 / 64), (65, 8, 7, 0.1), (256, 2, 1, 0.003), (5, 4, 64, 1.5), (2, 7, 3, 0.2), (256, 8, 2, 1e-3)]


@pytest.mark.parametrize("nh", [1, 4, MAX_HEADS])
def test_finalize_multi_head_by_head(nh):
    """Heads of different B, C, replicas and grad_scale in one launch, each against the reference; some without per_sample or coef."""
    rng = np.random.default_rng([nh, 33])
    heads, keep = [], []
    for i, (B, Cc, reps, gs) in enumerate(HEAD_SETS[:nh]):
        gs = float(f32(gs))
        buf = replica_sums(rng, reps, B, Cc)
        sd = Guarded(buf)
        loss, per, coef = Guarded(np.full(1, -3.0)), Guarded(np.full(B, -3.0, f32)), Guarded(np.full((B, Cc, 3), -3.0, f32))
        t = L.TaniHead()
        t.sums, t.replicas, t.B, t.C, t.grad_scale, t.loss_out = sd.ptr, reps, B, Cc, gs, loss.ptr
        t.coef, t.per_sample = (coef.ptr if i % 3 != 1 else None), (per.ptr if i % 3 != 2 else None)
        heads.append(t)
        keep.append((B, Cc, reps, gs, buf, sd, loss, per, coef, i % 3 != 1, i % 3 != 2))
    ta = (L.TaniHead * nh)(*heads)
    assert L.lib().raw("rua_tanimoto_finalize_multi")(ta, nh, stream()) == 0
    torch.cuda.synchronize()
    worst = 0.0
    for B, Cc, reps, gs, buf, sd, loss, per, coef, has_coef, has_per in keep:
        folded = R.fold(buf[:reps], reps)
        got = sd.get()
        assert np.array_equal(got[:reps].view(np.uint64), buf[:reps].view(np.uint64))
        assert np.array_equal(got[reps].view(np.uint64), (folded if reps > 1 else buf[reps]).view(np.uint64))
        worst = max(worst, check_final((nh, B, Cc, reps), R.finalize(folded, B, Cc, gs), loss.get()[0], per.get(), coef.get(), has_per, has_coef))
    print(f"tanimoto finalize_multi {nh} heads: {worst:.3f}")


def test_finalize_multi_refusals():
    rng = np.random.default_rng(34)
    B, Cc = 3, 6
    sd, loss = Guarded(replica_sums(rng, 1, B, Cc)), Guarded(np.full(1, -3.0))

    def head(B_):
        t = L.TaniHead()
        t.sums, t.replicas, t.B, t.C, t.grad_scale, t.loss_out, t.coef, t.per_sample = sd.ptr, 1, B_, Cc, 0.1, loss.ptr, None, None
        return t
    lib = L.lib()
    nine = (L.TaniHead * 9)(*[head(B) for _ in range(9)])
    assert lib.raw("rua_tanimoto_finalize_multi")(nine, 0, stream()) != 0
    assert lib.raw("rua_tanimoto_finalize_multi")(nine, 9, stream()) != 0
    two = (L.TaniHead * 2)(head(B), head(257))
    assert lib.raw("rua_tanimoto_finalize_multi")(two, 2, stream()) != 0
    torch.cuda.synchronize()
    assert loss.get()[0] == -3.0                                                                     # nothing ran, the good first head neither


@pytest.mark.parametrize("Cc", [1, 3, 6, 8])
@pytest.mark.parametrize("B", [1, 3, 65, 256])
def test_ratio_is_the_single_form(B, Cc):
    rng = np.random.default_rng([B, Cc, 35])
    worst = 0.0
    for plant in ("none", "one_zero", "1e-21"):
        s, _ = planted_sums(rng, B, Cc, plant, 1)
        fin = R.finalize(s, B, Cc, 0.0, single=True)
        sd = up(s)
        mean, per = Guarded(np.full(1, -3.0)), Guarded(np.full(B, -3.0, f32))
        assert L.lib().raw("rua_tanimoto_ratio")(sd.data_ptr(), B, Cc, mean.ptr, per.ptr, stream()) == 0
        torch.cuda.synchronize()
        assert fin.coef is None
        worst = max(worst, check_final((B, Cc, plant), fin, mean.get()[0], per.get(), None, coef_given=False))
    print(f"tanimoto ratio B={B} C={Cc}: {worst:.3f}")


# ================================================================ rua_head_dz ============================================================
# Roundings of one element of dz on its longest path, against the scale _loss_ref.dz() returns with it (the absolute values of the terms through the
# activation's Jacobian).  The Jacobian itself: softmax p_c (g_c - sum_j g_j p_j) - C fmas for the dot product, the difference, the product = C + 2;
# sigmoid g p (1 - p) = 3; none = 0.
def jac_k(act, Cc):
    return {SOFTMAX: Cc + 2, SIGMOID: 3, NONE: 0}[act]


def dz_k(kind, act, Cc):
    if kind == L.LOSS_TANIMOTO:                               # fma(k1, p, fma(k2, y, k0)): 2, then the Jacobian
        return 2 + jac_k(act, Cc)
    if kind == L.LOSS_CE_LOGITS:                              # sum y: C - 1 adds; p * sy, - y, * gs
        return Cc - 1 + 3
    if kind == L.LOSS_BCE_LOGITS:                             # (p - y) * gs / C
        return 3
    if kind == L.LOSS_MSE:                                    # 2 (p - y) * gs / C: 3 (the doubling is exact), then the Jacobian
        return 3 + jac_k(act, Cc)
    # weighted CE: S = sum p: C - 1; u = p / S: 1 more (C); h = -y cw / u: + 2 (C + 2); hu = sum h u (every h <= 0): h's C + 2, u's C, C fmas
    # (3 C + 2); h - hu: + 1, on |h| + |hu| (3 C + 3); / S: its C - 1 and the division (4 C + 3); * gs (4 C + 4); then the Jacobian
    return 4 * Cc + 4 + jac_k(act, Cc)


def call_dz(kind, act, p_ptr, y_ptr, coef_ptr, cw_ptr, gs, B, HW, Cc):
    out = Guarded(np.full((B, HW, Cc), 7.0, f32))
    rc = L.lib().raw("rua_head_dz")(kind, act, p_ptr, y_ptr, coef_ptr, cw_ptr, gs, B, HW, Cc, out.ptr, stream())
    torch.cuda.synchronize()
    assert rc == 0
    return out.get()


def dz_inputs(rng, kind, act, B, HW, Cc):
    """(p, y, coef, cw, gs), all float32-exact.  The two logits kinds take p = softmax / sigmoid of the logits, whatever `act` says."""
    pact = SOFTMAX if kind in (L.LOSS_CE_LOGITS, L.LOSS_WCE) else SIGMOID if kind == L.LOSS_BCE_LOGITS else act if act != NONE else SIGMOID
    p = probabilities(rng, (B, HW, Cc), pact)
    y = rng.random((B, HW, Cc)).astype(f32) if kind == L.LOSS_MSE else labels(rng, (B, HW, Cc), pact)
    coef = rng.standard_normal((B, Cc, 3)).astype(f32) if kind == L.LOSS_TANIMOTO else None
    cw = (1 + 9 * rng.random(Cc)).astype(f32) if kind == L.LOSS_WCE else None
    return p, y, coef, cw, float(f32(0.7 / (B * HW)))


def check_dz(name, kind, act, got, p, y, coef, cw, gs):
    ref, scale = R.dz(kind, act, p, y, coef=coef, cw=cw, grad_scale=gs, with_scale=True)
    return within(name, got, ref, dz_k(kind, act, p.shape[-1]) * U * scale)


PLAIN = [(L.LOSS_WCE, SOFTMAX), (L.LOSS_CE_LOGITS, SOFTMAX), (L.LOSS_BCE_LOGITS, SIGMOID), (L.LOSS_MSE, SOFTMAX), (L.LOSS_MSE, SIGMOID), (L.LOSS_MSE, NONE)]


@pytest.mark.parametrize("Cc", [1, 3, 5, 6, 8])
def test_head_dz_plain_kinds(Cc):
    """C = 6 and C = 3 have kernels of their own (C = 6 reads its rows as float2); the other counts share the generic body."""
    rng = np.random.default_rng([Cc, 41])
    B, HW = 3, 257
    worst = 0.0
    for kind, act in PLAIN:
        p, y, coef, cw, gs = dz_inputs(rng, kind, act, B, HW, Cc)
        pt, yt, cwt = up(p), up(y), (up(cw) if cw is not None else None)
        got = call_dz(kind, act, pt.data_ptr(), yt.data_ptr(), None, cwt.data_ptr() if cw is not None else None, gs, B, HW, Cc)
        worst = max(worst, check_dz(f"dz {KINDN[kind]} {ACTN[act]} C={Cc}", kind, act, got, p, y, coef, cw, gs))
    if Cc == 6:                                               # p four bytes off 8-byte alignment under the float2 loads
        kind, act = L.LOSS_MSE, SOFTMAX
        p, y, coef, cw, gs = dz_inputs(rng, kind, act, B, HW, Cc)
        (pt, pp), yt = shifted(p), up(y)
        assert pp % 8 == 4
        got = call_dz(kind, act, pp, yt.data_ptr(), None, None, gs, B, HW, Cc)
        worst = max(worst, check_dz("dz mse softmax C=6, p off alignment", kind, act, got, p, y, coef, cw, gs))
    print(f"head dz plain kinds C={Cc}: {worst:.3f}")


def test_head_dz_past_the_grid_cap():
    """B = 64: at most 4096 / 64 = 64 blocks of 256 pixels per sample, HW = 16640 = 65 * 256: every thread runs its loop twice, the second time only
    in the first block."""
    rng = np.random.default_rng(42)
    B, HW, Cc, kind, act = 64, 16640, 2, L.LOSS_MSE, SIGMOID
    assert HW > 256 * (4096 // B)
    p, y, coef, cw, gs = dz_inputs(rng, kind, act, B, HW, Cc)
    pt, yt = up(p), up(y)
    got = call_dz(kind, act, pt.data_ptr(), yt.data_ptr(), None, None, gs, B, HW, Cc)
    r = check_dz("dz mse sigmoid past the cap", kind, act, got, p, y, coef, cw, gs)
    print(f"head dz past the grid cap: {r:.3f}")


def test_head_dz_multi_with_unequal_heads():
    """One launch, blockIdx.z = head: the grid is sized by the largest B and HW, so the smaller heads' surplus blocks must do nothing."""
    rng = np.random.default_rng(43)
    specs = [(L.LOSS_TANIMOTO, SOFTMAX, 3, 257, 6), (L.LOSS_WCE, SOFTMAX, 2, 300, 5), (L.LOSS_BCE_LOGITS, SIGMOID, 5, 16, 3), (L.LOSS_MSE, SIGMOID, 1, 1000, 1),
             (L.LOSS_TANIMOTO, SIGMOID, 4, 1, 8), (L.LOSS_CE_LOGITS, SOFTMAX, 1, 2000, 6)]
    heads, keep = [], []
    for kind, act, B, HW, Cc in specs:
        p, y, coef, cw, gs = dz_inputs(rng, kind, act, B, HW, Cc)
        pt, yt = up(p), up(y)
        ct, wt = (up(coef) if coef is not None else None), (up(cw) if cw is not None else None)
        out = Guarded(np.full((B, HW, Cc), 7.0, f32))
        d = L.DzHead()
        d.kind, d.act, d.p, d.y, d.grad_scale, d.B, d.HW, d.C, d.dz = kind, act, pt.data_ptr(), yt.data_ptr(), gs, B, HW, Cc, out.ptr
        d.coef, d.class_w = (ct.data_ptr() if ct is not None else None), (wt.data_ptr() if wt is not None else None)
        heads.append(d)
        keep.append((kind, act, p, y, coef, cw, gs, out, pt, yt, ct, wt))
    da = (L.DzHead * len(heads))(*heads)
    assert L.lib().raw("rua_head_dz_multi")(da, len(heads), stream()) == 0
    torch.cuda.synchronize()
    worst = 0.0
    for kind, act, p, y, coef, cw, gs, out, *_ in keep:
        worst = max(worst, check_dz(f"dz multi {KINDN[kind]} {ACTN[act]} {p.shape}", kind, act, out.get(), p, y, coef, cw, gs))
    assert L.lib().raw("rua_head_dz_multi")(da, 0, stream()) != 0 and L.lib().raw("rua_head_dz_multi")(da, 9, stream()) != 0
    print(f"head dz multi: {worst:.3f}")


# ---- sums -> finalize -> dz against float64 autograd of the oracle --------------------------------------------------------------
# The moments carry k_s = sums_k(T) roundings each, relative (they are sums of non-negative terms).  Through the finalizer (float64):
#   V -> w = 1 / V^2: 2 k_s;  N = sum w Spl: 3 k_s;  SS - Spl >= SS / 2 >= Spl, so the difference carries 3 k_s and D = sum w (SS - Spl): 5 k_s;
#   a = w / E^2: 12 k_s;  c1 = -2 (a1 F1 + a2 F2): 15 k_s;  c2 = a1 (E1 + F1) + a2 (E2 + F2): 17 k_s;
#   c0 = kap + a2 (F2 - E2): kap = -2 / (V^3 B) sum_n (Spl E1 - F1 (SS - Spl)) / E1^2 carries 3 + 16 = 19 k_s.
# Then the float32 store of the coefficient (1) and rua_head_dz (dz_k).  The loss: F / E carries 8 k_s and is at most 1.
def chain_k(T, act, Cc):
    return 19 * sums_k(T) + 1 + dz_k(L.LOSS_TANIMOTO, act, Cc)


@pytest.mark.parametrize("act", [SOFTMAX, SIGMOID], ids=["softmax", "sigmoid"])
@pytest.mark.parametrize("B,HW,Cc", [(1, 4, 6), (3, 257, 3), (65, 16, 6), (256, 8, 2), (2, 300, 5)])
def test_chain_against_autograd_of_the_oracle(B, HW, Cc, act):
    from oracle import resuneta_ref as ref
    rng = np.random.default_rng([B, HW, Cc, act, 44])
    wgt = 0.7
    gs = float(f32(wgt / B))
    p, y = probabilities(rng, (B, HW, Cc), act), labels(rng, (B, HW, Cc), act)
    pq = torch.from_numpy(p.astype(f64)).requires_grad_(True)
    nchw = lambda t: t.reshape(B, HW, 1, Cc).permute(0, 3, 1, 2)
    per_t = ref.tanimoto_dual_loss(nchw(torch.from_numpy(y.astype(f64))), nchw(pq))
    (gs * per_t.sum()).backward()
    gp = pq.grad.numpy()
    P = p.astype(f64)
    want, _ = R.jacobian(act, P, gp, np.abs(gp))
    fin = R.finalize(R.moments(p, y, np.ones((B, HW), bool)), B, Cc, gs)
    assert not fin.replaced1.any() and not fin.replaced2.any()
    _, scale = R.dz(L.LOSS_TANIMOTO, act, p, y, coef=fin.coef, with_scale=True)
    pt, yt = up(p), up(y)
    sums, loss, coef = Guarded(np.zeros((B, Cc, 6))), Guarded(np.full(1, -3.0)), Guarded(np.full((B, Cc, 3), -3.0, f32))
    lib = L.lib()
    assert call_sums(pt.data_ptr(), yt.data_ptr(), None, B, HW, Cc, sums.ptr) == 0
    assert lib.raw("rua_tanimoto_finalize")(sums.ptr, B, HW, Cc, gs, loss.ptr, coef.ptr, None, stream()) == 0
    torch.cuda.synchronize()
    got = call_dz(L.LOSS_TANIMOTO, act, pt.data_ptr(), yt.data_ptr(), coef.ptr, None, gs, B, HW, Cc)
    T, _ = sums_grid(HW, Cc, sums_route(HW, Cc, True, lib.get_tuning("tani_vec")))
    ks = sums_k(T)
    want_loss = float(per_t.detach().mean())
    assert abs(loss.get()[0] - want_loss) <= 8 * ks * U, (loss.get()[0], want_loss)
    r = within(f"chain dz B={B} HW={HW} C={Cc} {ACTN[act]}", got, want, chain_k(T, act, Cc) * U * scale)
    print(f"tanimoto chain B={B} HW={HW} C={Cc} {ACTN[act]}: dz {r:.3f}, loss {abs(loss.get()[0] - want_loss) / (8 * ks * U):.3f}")


# ================================================================ rua_seg_metrics ========================================================
def metric_data(rng, M, Cc):
    """Multiples of 1/8: ties are the rule.  The first rows hold exactly 0.5 everywhere, an all-equal row and a row whose maximum repeats."""
    p, y = dyadic(rng, (M, Cc)), dyadic(rng, (M, Cc))
    rows = [np.full(Cc, 0.5), np.full(Cc, 0.25), np.r_[0.125, np.full(Cc - 1, 0.75)] if Cc > 1 else np.array([0.75])]
    for i, r in enumerate(rows):
        if i < M:
            p[i] = r
        if M - 1 - i >= 0:
            y[M - 1 - i] = r
    return p, y


def metrics_case(rng, M, Cc, form, shift=False):
    p, y = metric_data(rng, M, Cc)
    void = void_of(rng, form, 1, M, 2)
    keep = np.ones(M, bool) if void is None else ~void[0]
    pre = np.array([3.0, 5.0, 7.0, 11.0, 13.0])
    want = pre + R.metric_counts(p, y, keep)
    pn, yn = with_nan(p, None if void is None else void[0]), with_nan(y, None if void is None else void[0])
    pt, pp = shifted(pn) if shift else (up(pn), None)
    yt = up(yn)
    vt, vp = mask_bytes(rng, void) if void is not None else (None, None)
    out = Guarded(pre)
    lib = L.lib()
    if vp is None:
        rc = lib.raw("rua_seg_metrics")(pp or pt.data_ptr(), yt.data_ptr(), M, Cc, out.ptr, stream())
    else:
        rc = lib.raw("rua_seg_metrics_void")(pp or pt.data_ptr(), yt.data_ptr(), vp, M, Cc, out.ptr, stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert np.array_equal(out.get(), want), (M, Cc, form, shift, out.get(), want)


@pytest.mark.parametrize("Cc", [1, 2, 3, 6, 7])
def test_metrics_exact(Cc):
    """C = 6 and C = 2 with an even M and aligned pointers take the vector kernel (grid capped at 256 blocks of 512 pixels = 131072: M = 131074 gives
    the first thread a second iteration); an odd M or a shifted pointer sends them to the scalar kernel, whose grid is capped at CUs / 2 blocks."""
    for M in (1, 2, 255, 131074, 131075):
        for form in MASK_FORMS:
            metrics_case(np.random.default_rng([Cc, M, MASK_FORMS.index(form), 51]), M, Cc, form)
    metrics_case(np.random.default_rng([Cc, 52]), 256, Cc, "one_per_group", shift=True)
    with tuning(metrics_blocks=2):                           # scalar kernel (odd C, or M odd): 1500 pixels over 2 blocks - three iterations, the last ragged
        for M in (1500, 1501):
            for form in ("none", "random"):
                metrics_case(np.random.default_rng([Cc, M, 53]), M, Cc, form)


def test_metrics_refusals():
    t = torch.zeros(64, device=dev())
    out = Guarded(np.arange(5.0))
    lib, a = L.lib(), t.data_ptr()
    assert lib.raw("rua_seg_metrics")(a, a, 0, 6, out.ptr, stream()) != 0
    assert lib.raw("rua_seg_metrics")(a, a, 4, 0, out.ptr, stream()) != 0
    assert lib.raw("rua_seg_metrics")(None, a, 4, 6, out.ptr, stream()) != 0
    assert lib.raw("rua_seg_metrics")(a, a, 4, 6, None, stream()) != 0
    torch.cuda.synchronize()
    assert np.array_equal(out.get(), np.arange(5.0))


# ================================================================ rua_pixel_loss =========================================================
# Per pixel, against float64 of the stored inputs, k * u * S (a libm call: 2 ulps = 4 u of its result; an input error d moves exp by d and log by
# d / x):
#   MSE   d = y - p (1, squared: 2), C fmas, / C: k = C + 3 on S = l (every term >= 0).
#   BCE   per class max(z, 0) - z y + log1p(exp(-|z|)): the product 1, the two adds 2, exp 4 -> log1p's result moves by at most 4, log1p 4: 11 on
#         |max(z, 0)| + |z y| + log1p; C adds, / C: k = C + 12 on S = mean of those.
#   CE    s = sum exp(z - mx) >= 1: the difference 1 moves exp by |z - mx| u, and x e^-x <= 1 / e: C / e + 4 + (C - 1) <= 1.4 C + 3 of s;
#         log s: that + 4 |log s|; lse = mx + log s: + 1 on |lse|; z - lse 1, * y 1, C adds on |y (z - lse)|:
#         k = 2 C + 3 (>= C + 2, 1.4 C + 3, 4) on S = sum |y| (|z - lse| + |lse| + |log s| + 1).
#   WCE   S_ = sum p: C - 1; q = p / S_: C; the clip passes a relative error through or removes it; log moves by C u, logf 4 |log u|; * y, * cw: 2;
#         C adds: k = C + 6 on S = sum |y cw| (1 + |log u|).
# k u S is a relative model; below the smallest normal float32, 2^-126, no operation has relative accuracy (gradual underflow, or a libm that flushes:
# the pixel z = -100, y = 0 of one sigmoid channel has the loss log1p(exp(-100)) = 3.7e-44, 27 denormal steps), so each of the k operations may also
# err by 2^-126: the bound is k (u S + 2^-126).
# The total: (n_thread + 16) u sum |l|, n_thread the pixels one thread adds up (6 shuffle levels, the waves' sums in fp64).
TINY = 2.0 ** -126


def pixel_ref_and_bound(kind, p, z, y, cw):
    Cc = p.shape[-1]
    ref = R.pixel_loss(kind, p, z, y, cw)
    P, Z, Y = p.astype(f64), z.astype(f64), y.astype(f64)
    if kind == L.LOSS_MSE:
        return ref, (Cc + 3) * (U * ref + TINY)
    if kind == L.LOSS_BCE_LOGITS:
        S = (np.maximum(Z, 0) + np.abs(Z * Y) + np.log1p(np.exp(-np.abs(Z)))).mean(-1)
        return ref, (Cc + 12) * (U * S + TINY)
    if kind == L.LOSS_CE_LOGITS:
        lse = R.log_sum_exp(Z)
        logs = lse - Z.max(-1, keepdims=True)
        S = (np.abs(Y) * (np.abs(Z - lse) + np.abs(lse) + np.abs(logs) + 1)).sum(-1)
        return ref, (2 * Cc + 3) * (U * S + TINY)
    u, _ = R.clipped_share(P)
    S = (np.abs(Y * cw.astype(f64)) * (1 + np.abs(np.log(u)))).sum(-1)
    return ref, (Cc + 6) * (U * S + TINY)


def pixel_inputs(rng, kind, M, Cc):
    z = (rng.standard_normal((M, Cc)) * 2).astype(f32)
    p = softmax32(z.astype(f64)) if kind != L.LOSS_BCE_LOGITS else sigmoid32(z.astype(f64))
    y = labels(rng, (M, Cc), SIGMOID if kind == L.LOSS_BCE_LOGITS else SOFTMAX) if kind != L.LOSS_MSE else rng.random((M, Cc)).astype(f32)
    cw = (1 + 9 * rng.random(Cc)).astype(f32)
    r = min(M, 4)                                             # planted extreme rows
    if kind == L.LOSS_BCE_LOGITS:
        z[:r] = np.where(np.arange(Cc)[None, :] % 2 == np.arange(r)[:, None] % 2, 100.0, -100.0)
        y[:r] = (np.arange(r)[:, None] // 2 + np.arange(Cc)[None, :]) % 2          # saturated towards the label and away from it
    elif kind == L.LOSS_CE_LOGITS:
        z[:r, 0] = 1e4
        y[:r] = np.eye(Cc, dtype=f32)[np.arange(r) % Cc]
    elif kind == L.LOSS_WCE:
        p[:r] = 1e-9                                          # shares below 1e-7, and one above 1 - 1e-7 (C > 1; C = 1: the share is 1)
        p[:r, 0] = 1.0
        y[:r] = np.eye(Cc, dtype=f32)[np.arange(r) % Cc]
        if Cc > 1:
            q = p[0].astype(f64) / p[0].astype(f64).sum()
            assert q[0] > 1 - 1e-7 and q[1] < 1e-7
    return p, z, y, cw


PIXEL_KINDS = (L.LOSS_WCE, L.LOSS_CE_LOGITS, L.LOSS_BCE_LOGITS, L.LOSS_MSE)


def pixel_case(rng, kind, M, Cc):
    p, z, y, cw = pixel_inputs(rng, kind, M, Cc)
    ref, bound = pixel_ref_and_bound(kind, p, z, y, cw)
    pt, zt, yt, ct = up(p), up(z), up(y), up(cw)
    blocks = min(1024, cdiv(M, 256))
    n_thread = cdiv(M, blocks * 256)
    # the blocks add their sums onto the 2.5 the test left in loss_out, in fp64: one rounding of the running total per block
    tot_bound = (n_thread + 16) * U * np.abs(ref).sum() + blocks * 2.0 ** -53 * (2.5 + np.abs(ref).sum())
    worst = [0.0, 0.0]
    for want_pp in (True, False):
        out, pp = Guarded(np.full(1, 2.5)), Guarded(np.full(M, -3.0, f32))
        rc = L.lib().raw("rua_pixel_loss")(kind, pt.data_ptr(), zt.data_ptr(), yt.data_ptr(), ct.data_ptr(), M, Cc, out.ptr, pp.ptr if want_pp else None, stream())
        torch.cuda.synchronize()
        assert rc == 0
        name = f"pixel loss {KINDN[kind]} M={M} C={Cc}"
        if want_pp:
            worst[0] = within(name + " per pixel", pp.get(), ref, bound)
        else:
            assert (pp.get() == f32(-3.0)).all()
        worst[1] = max(worst[1], within(name + " total", out.get()[0] - 2.5, ref.sum(), tot_bound))
    return worst


@pytest.mark.parametrize("Cc", [1, 5, 9, 64])
@pytest.mark.parametrize("M", [1, 257, 300000])
def test_pixel_loss_plain_kinds(M, Cc):
    """M = 300000 is past the cap of 1024 blocks (262144 pixels): the first threads add two pixels.  With C = 64 that size runs one kind (CE, whose
    loop over the classes is the longest): three tensors of 19 M floats each for all four would be most of the file's time."""
    kinds = PIXEL_KINDS if M * Cc < 4_000_000 else (L.LOSS_CE_LOGITS,)
    worst = [0.0, 0.0]
    for kind in kinds:
        w = pixel_case(np.random.default_rng([M, Cc, kind, 61]), kind, M, Cc)
        worst = [max(a, b) for a, b in zip(worst, w)]
    print(f"pixel loss M={M} C={Cc}: per pixel {worst[0]:.3f}, total {worst[1]:.3f}")


def test_pixel_loss_refusals():
    t = torch.ones(64 * 65, device=dev())
    out = Guarded(np.full(1, 2.5))
    lib, a = L.lib(), t.data_ptr()
    assert lib.raw("rua_pixel_loss")(L.LOSS_MSE, a, a, a, a, 4, 65, out.ptr, None, stream()) != 0
    assert lib.raw("rua_pixel_loss")(L.LOSS_MSE, a, a, a, a, 0, 5, out.ptr, None, stream()) != 0
    assert lib.raw("rua_pixel_loss")(L.LOSS_TANIMOTO, a, a, a, a, 4, 5, out.ptr, None, stream()) != 0
    assert lib.raw("rua_pixel_loss")(L.LOSS_WCE, a, a, a, None, 4, 5, out.ptr, None, stream()) != 0
    assert lib.raw("rua_pixel_loss")(L.LOSS_CE_LOGITS, a, None, a, a, 4, 5, out.ptr, None, stream()) != 0
    torch.cuda.synchronize()
    assert out.get()[0] == 2.5


# ================================================================ the fused producers ====================================================
# rua_head_fwd_loss, _rep and _void fill the same moments from the probabilities they have in registers.  Their sums are compared with moments() of
# the p THE SAME LAUNCH wrote, so the convolution and the activation do not enter.  Roundings: no kernel form gives a lane more than one pixel in 32
# of its block (the generic kernel: one in 256; head_fwd2: one in 64 or in 32; head_fwd3: one in 256), and no launcher's block is larger than the
# generic one's, so a lane adds at most ppb / 32 terms; then the 5 inside a term and at most 6 shuffle levels, as in sums_k().
def fused_k(B, HW):
    per_sample = max(1, cdiv(2 * cus(), B))
    ppb = cdiv(max(cdiv(HW, per_sample), 256), 256) * 256
    return sums_k(cdiv(ppb, 32))


FUSED_FORMS = [("generic", L.RUA_F32, 16), ("co8", L.RUA_F32, 32), ("co8", L.RUA_BF16, 32)]


@pytest.mark.parametrize("form,dt,Cin", FUSED_FORMS, ids=["generic-f32-16", "fwd2-f32-32", "fwd3-bf16-32"])
def test_fused_head_loss_moments(form, dt, Cin):
    """Cout in {2, 5, 8}: none of them has a kernel form of its own, so Cin = 32 runs the CO = 8 instantiations of head_fwd2 (fp32) and head_fwd3 (bf16)."""
    rng = np.random.default_rng([Cin, dt, 71])
    lib = L.lib()
    B = 3
    worst = 0.0
    for Cout in (2, 5, 8):
        for HW in (1, 255, 700):
            for act in (SOFTMAX, SIGMOID):
                M = B * HW
                x = rng.standard_normal((M, Cin)).astype(f32)
                xd = torch.from_numpy(x).to(torch.bfloat16 if dt == L.RUA_BF16 else torch.float32).to(dev())
                wd, bd = up((rng.standard_normal((Cout, Cin)) / 4).astype(f32)), up(rng.standard_normal(Cout).astype(f32))
                y = labels(rng, (B, HW, Cout), act)
                yd = up(y)
                void = void_of(rng, "random", B, HW, 2)
                void[1] = True                                # a whole void sample
                vt, vp = mask_bytes(rng, void)
                for name, reps, mask in (("rua_head_fwd_loss", 1, None), ("rua_head_fwd_loss_rep", 1, None), ("rua_head_fwd_loss_rep", 8, None),
                                         ("rua_head_fwd_loss_void", 1, vp), ("rua_head_fwd_loss_void", 8, vp)):
                    z, p = Guarded(np.full((M, Cout), 7.0, f32)), Guarded(np.full((M, Cout), 7.0, f32))
                    s, m = Guarded(np.zeros((reps, B, Cout, 6))), Guarded(np.zeros(5))
                    head = (xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), z.ptr, p.ptr, yd.data_ptr(), s.ptr)
                    tail = (m.ptr, B, HW, Cin, Cout, act, dt)
                    if name == "rua_head_fwd_loss":
                        rc = lib.raw(name)(*head, *tail, stream())
                    elif name == "rua_head_fwd_loss_rep":
                        rc = lib.raw(name)(*head, reps, *tail, stream())
                    else:
                        rc = lib.raw(name)(*head, reps, *tail, mask, stream())
                    torch.cuda.synchronize()
                    assert rc == 0
                    pg = p.get().reshape(B, HW, Cout)
                    assert np.isfinite(pg).all() and not (pg == 7.0).all()
                    keep = ~void if mask is not None else np.ones((B, HW), bool)
                    ref = R.moments(pg, y, keep)
                    got = R.fold(s.get(), reps)
                    what = f"{name} R={reps} {form} Cout={Cout} HW={HW} {ACTN[act]}"
                    r = worst_ratio(np.abs(got - ref), fused_k(B, HW) * U * ref)
                    assert r <= 1.0, (what, r)
                    worst = max(worst, r)
                    assert np.array_equal(m.get(), R.metric_counts(pg, y, keep)), what
                    if mask is not None:
                        assert not got[1].any()
    print(f"fused head + loss moments {form} Cin={Cin}: {worst:.3f}")
