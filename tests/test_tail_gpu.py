"""The tail of a training step through the C ABI: rua_lr_step, rua_adam_step_w / rua_sgd_step_w (and their _w-less forms) against float64 references
computed on the CPU.

The optimizer references are fed what the kernels are fed: the float32-rounded scalars beta1, beta2, eps, lr_t, grad_scale and the float32 state
(1.f - beta is exact in float32 for both betas, so the reference's 1 - beta is the kernel's).  A fresh state is uploaded before every checked step,
so the bounds are ONE-step rounding bounds, derived and not measured.  With u = 2^-23, gg = g * grad_scale, delta = lr_t * m' / (sqrt(v') + eps):

  Adam   |m' - m'_ref|   <= 4u (beta1 |m| + (1 - beta1) |gg|)                                     =: e_m    (three roundings, or two with an fma)
         |v' - v'_ref|   <= 4u v'_ref
         |th' - th'_ref| <= u |th'_ref| + 4e-6 |delta_ref| + lr_t e_m / (sqrt(v'_ref) + eps)      (about 32 ulp for the divide, the root and v')
  SGD    |vel' - vel'_ref| <= 4u (mu |vel| + |lr gg|)                                             =: e_v
         |th' - th'_ref|   <= u |th'_ref| + e_v

Every test prints the worst observed ratio to its bound (pytest -s shows them)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from _kernel_util import U32, bits_of, dev, frozen, stream, up, worst_ratio  # noqa: E402
from resunet_a_mltsk_keras_amd import _lib as L  # noqa: E402

f32, f64 = np.float32, np.float64
B1, B2, EPS = f32(0.9), f32(0.999), f32(1e-7)                 # what the engine passes (Keras' defaults), as the kernels receive them
MU = f32(0.8)
LR_ADAM, LR_SGD = f32(1.2345e-3), f32(0.1)
GUARD_BITS = 0x5A5A                                           # the two bf16 elements behind a weight copy
ADAM_N = [1, 3, 4, 7, 1023, 4096 * 1024 + 1203]               # the last: first wrap of the capped grid (4096 blocks x 256 threads x 4), ragged tail
SGD_N = [1, 3, 1023, 4096 * 256 + 777]                        # the last: first wrap of the capped grid (4096 x 256), ragged
# grad_scale, zero_grad, rate from the device, bf16 copy
VARIANTS = [(1.0, 1, True, True), (0.125, 0, False, True), (0.125, 1, True, False), (1.0, 0, False, False),
            (0.125, 1, True, True)]                           # the last: the bf16 engine's own call


SEED = 7


def normal_range(v1):
    """The reference's second moments are zero or at least 8 x the smallest normal float32: the relative bounds apply."""
    nz = v1[v1 > 0]
    assert nz.size == 0 or nz.min() >= 2.0 ** -123, float(nz.min())


def lr_ref(t, lr, b1, b2):
    return float(lr) * np.sqrt(1.0 - float(b2) ** t) / (1.0 - float(b1) ** t)


# ---- rua_lr_step ------------------------------------------------------------------------------------------------------------------------
def lr_call(state, out, adam, b1=0.9, b2=0.999):
    return L.lib().raw("rua_lr_step")(state.data_ptr() if state is not None else None, out.data_ptr() if out is not None else None,
                                      adam, b1, b2, stream())


@pytest.mark.parametrize("lr", [1e-3, 0.1])
@pytest.mark.parametrize("t", [1, 2, 3, 10, 1000, 100000])
def test_lr_step_counter_and_rate(t, lr):
    worst = 0.0
    for adam in (1, 0):
        state = up(np.array([t - 1, lr], f64))
        out = up(np.array([-1.0], f32))
        assert lr_call(state, out, adam) == 0
        torch.cuda.synchronize()
        st = state.cpu().numpy()
        assert st[0] == float(t) and bits_of(state)[1] == np.array([lr], f64).view(np.uint64)[0], (t, lr, st)
        got = out.cpu().numpy()[0]
        if adam:
            exp = f32(lr_ref(t, lr, 0.9, 0.999))
            ulps = abs(float(got) - float(exp)) / float(np.spacing(exp))
            worst = max(worst, ulps)
            assert ulps <= 1.0, (t, lr, got, exp)
        else:
            assert got == f32(lr) and np.array([got]).view(np.uint32)[0] == np.array([lr], f32).view(np.uint32)[0], (t, lr, got)
    print(f"rua_lr_step t={t} lr={lr}: {worst:.2f} ulp from float32(float64 rate)")


@pytest.mark.parametrize("adam", [1, 0])
def test_lr_step_three_calls_without_a_host_push(adam):
    """The captured-step contract: the counter lives on the device, nothing is pushed between replays."""
    t, lr = 7, 1e-3
    state, out = up(np.array([t - 1, lr], f64)), up(np.zeros(1, f32))
    got = []
    for _ in range(3):
        assert lr_call(state, out, adam) == 0
        got.append(out.cpu().numpy()[0])
    assert state.cpu().numpy()[0] == t + 2
    for k, g in enumerate(got):
        exp = f32(lr_ref(t + k, lr, 0.9, 0.999)) if adam else f32(lr)
        assert abs(float(g) - float(exp)) <= (float(np.spacing(exp)) if adam else 0.0), (k, g, exp)
    if adam:
        assert got[0] != got[1] != got[2]                     # the rate does move at t = 7, 8, 9


def test_lr_step_null_pointers():
    state, out = up(np.array([3.0, 1e-3], f64)), up(np.array([0.5], f32))
    assert lr_call(None, out, 1) != 0
    assert lr_call(state, None, 1) != 0
    torch.cuda.synchronize()
    assert state.cpu().numpy().tolist() == [3.0, 1e-3] and out.cpu().numpy()[0] == f32(0.5)


# ---- the optimizers, one step at a time -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tail_inputs(n):
    """Seeded state of n elements: gradients over fifteen decades, moments over seven, zeros every 7th (g), 5th (m, v / vel), 11th (theta) element -
    every 35th element is what the 64-byte padding of a slice holds (g = m = v = 0), roughly a tenth have eps above sqrt(v'), some have m and g cancel.
    The bounds are relative, so they hold where nothing underflows: of 4.2 M such draws a handful have (1 - beta2) gg^2 below the smallest normal
    float32 (1.2e-38), where a float32 result is only good to 2^-149.  SEED is one for which the REFERENCE's v' stays normal at every size used here
    (normal_range asserts it); the code under test had no part in choosing it."""
    rng = np.random.default_rng([n, SEED])
    g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-12, 3, n)).astype(f32)
    m = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 1, n)).astype(f32)
    v = ((rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 1, n)) ** 2).astype(f32)
    th = rng.standard_normal(n).astype(f32)
    g[::7] = 0
    m[::5] = 0
    v[::5] = 0
    th[::11] = 0
    return frozen(th, g, m, v)


@functools.lru_cache(maxsize=4)
def adam_ref(n, gs):
    """(th', m', v') in float64 and the three bounds of the module docstring."""
    th, g, m, v = (a.astype(f64) for a in tail_inputs(n))
    b1, b2, eps, lr = f64(B1), f64(B2), f64(EPS), f64(LR_ADAM)
    gg = g * f64(f32(gs))
    m1 = b1 * m + (1 - b1) * gg
    v1 = b2 * v + (1 - b2) * gg * gg
    normal_range(v1)
    den = np.sqrt(v1) + eps
    delta = lr * m1 / den
    th1 = th - delta
    e_m = 4 * U32 * (b1 * np.abs(m) + (1 - b1) * np.abs(gg))
    e_v = 4 * U32 * v1
    e_th = U32 * np.abs(th1) + 4e-6 * np.abs(delta) + lr * e_m / den
    return frozen(th1, m1, v1, e_th, e_m, e_v)


@functools.lru_cache(maxsize=4)
def sgd_ref(n, gs):
    th, g, vel, _ = (a.astype(f64) for a in tail_inputs(n))
    mu, lr = f64(MU), f64(LR_SGD)
    gg = g * f64(f32(gs))
    vel1 = mu * vel - lr * gg
    th1 = th + vel1
    e_v = 4 * U32 * (mu * np.abs(vel) + np.abs(lr * gg))
    e_th = U32 * np.abs(th1) + e_v
    return frozen(th1, vel1, e_th, e_v)


def wcopy_buffer(th):
    """bf16(theta) as the engine's forward copy holds it before a step, and two guard elements behind it."""
    w = torch.cat([torch.from_numpy(np.array(th)).to(torch.bfloat16).view(torch.int16),
                   torch.full((2,), GUARD_BITS, dtype=torch.int16)])
    return w.to(dev())


def check_wcopy(wd, thd, n):
    """Every element of the copy - the scalar tail's too - is torch-CPU's bf16 of the theta' the kernel wrote; the guards are untouched."""
    w = bits_of(wd.view(torch.bfloat16))
    exp = bits_of(thd.cpu().to(torch.bfloat16))
    bad = np.flatnonzero(w[:n] != exp)
    assert bad.size == 0, (n, len(bad), "first at", int(bad[0]), hex(int(w[bad[0]])), hex(int(exp[bad[0]])))
    assert (w[n:] == GUARD_BITS).all(), (n, w[n:])


def run_adam(n, gs, zero, dev_lr, wc, entry="rua_adam_step_w"):
    th, g, m, v = tail_inputs(n)
    thd, gd, md, vd = up(th), up(g), up(m), up(v)
    wd = wcopy_buffer(th) if wc else None
    lrd = up(np.array([LR_ADAM], f32)) if dev_lr else None
    host_lr = 0.0 if dev_lr else float(LR_ADAM)              # with a device rate the host value is wrong on purpose (the engine passes 0.0)
    args = [thd.data_ptr(), gd.data_ptr(), md.data_ptr(), vd.data_ptr(), n, host_lr, lrd.data_ptr() if dev_lr else None,
            float(B1), float(B2), float(EPS), gs, zero]
    if entry == "rua_adam_step_w":
        args.append(wd.data_ptr() if wc else None)
    L.lib().call(entry, *args, stream())
    torch.cuda.synchronize()
    return thd, gd, md, vd, wd


@pytest.mark.parametrize("gs,zero,dev_lr,wc", VARIANTS)
@pytest.mark.parametrize("n", ADAM_N)
def test_adam_one_step(n, gs, zero, dev_lr, wc):
    th, g, m, v = tail_inputs(n)
    th1, m1, v1, e_th, e_m, e_v = adam_ref(n, gs)
    thd, gd, md, vd, wd = run_adam(n, gs, zero, dev_lr, wc)
    got_th, got_m, got_v = (t.cpu().numpy() for t in (thd, md, vd))
    r_m = worst_ratio(np.abs(got_m.astype(f64) - m1), e_m)
    r_v = worst_ratio(np.abs(got_v.astype(f64) - v1), e_v)
    r_th = worst_ratio(np.abs(got_th.astype(f64) - th1), e_th)
    print(f"adam n={n} gs={gs} zero={zero} dev_lr={dev_lr} wcopy={wc}: worst ratio to the bound m {r_m:.3f} v {r_v:.3f} theta {r_th:.3f}")
    assert r_m <= 1.0 and r_v <= 1.0 and r_th <= 1.0, (n, r_m, r_v, r_th)
    # the gradient: +0 everywhere, or as it was
    assert (bits_of(gd) == (0 if zero else g.view(np.uint32))).all()
    # padding (g = m = v = 0) never drifts
    pad = np.arange(0, n, 35)
    assert (g[pad] == 0).all() and (m[pad] == 0).all() and (v[pad] == 0).all()
    assert (bits_of(thd)[pad] == th.view(np.uint32)[pad]).all()
    assert (bits_of(md)[pad] == 0).all() and (bits_of(vd)[pad] == 0).all()
    if wc:
        check_wcopy(wd, thd, n)
        before = bits_of(torch.from_numpy(th[pad]).to(torch.bfloat16))
        assert (bits_of(wd.view(torch.bfloat16))[pad] == before).all()
    else:
        # without a copy the _w entry point IS the plain one
        th2, g2, m2, v2, _ = run_adam(n, gs, zero, dev_lr, False, entry="rua_adam_step")
        for a, b in ((thd, th2), (gd, g2), (md, m2), (vd, v2)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_adam_second_moment_in_the_subnormal_range():
    """What tail_inputs leaves out: v = 0 and |g| near 1e-19, so that (1 - beta2) gg^2 is a float32 subnormal (1e-43 .. 1e-40).  The product
    ((1 - beta2) gg) gg rounds once onto the subnormal grid (spacing 2^-149), beta2 * 0 and the sum are exact: v' within 4u v'_ref + 2^-149, so a
    v' flushed to zero fails.  sqrt(v') ~ 1e-21 stays far below eps, theta' keeps its bound of the module docstring; every other theta is zero, so
    that the step itself (~1e-16) is what is compared there.  19 elements: four 16-byte groups and a scalar tail of three."""
    n = 19
    g = (10.0 ** np.linspace(-20.0, -18.5, n) * np.where(np.arange(n) % 3 == 0, -1.0, 1.0)).astype(f32)
    th = np.where(np.arange(n) % 2 == 0, 0.0, np.linspace(-1.5, 1.5, n)).astype(f32)
    m, v = np.zeros(n, f32), np.zeros(n, f32)
    b1, b2, eps, lr = f64(B1), f64(B2), f64(EPS), f64(LR_ADAM)
    gg = g.astype(f64)
    m1 = (1 - b1) * gg
    v1 = (1 - b2) * gg * gg
    assert (v1 > 2.0 ** -149).all() and (v1 < 2.0 ** -127).all()
    den = np.sqrt(v1) + eps
    delta = lr * m1 / den
    th1 = th.astype(f64) - delta
    e_m = 4 * U32 * (1 - b1) * np.abs(gg)
    e_v = 4 * U32 * v1 + 2.0 ** -149
    e_th = U32 * np.abs(th1) + 4e-6 * np.abs(delta) + lr * e_m / den
    thd, gd, md, vd, wd = up(th), up(g), up(m), up(v), wcopy_buffer(th)
    L.lib().call("rua_adam_step_w", thd.data_ptr(), gd.data_ptr(), md.data_ptr(), vd.data_ptr(), n, float(LR_ADAM), None, float(B1), float(B2),
                 float(EPS), 1.0, 0, wd.data_ptr(), stream())
    torch.cuda.synchronize()
    got_v = vd.cpu().numpy()
    r_m = worst_ratio(np.abs(md.cpu().numpy().astype(f64) - m1), e_m)
    r_v = worst_ratio(np.abs(got_v.astype(f64) - v1), e_v)
    r_th = worst_ratio(np.abs(thd.cpu().numpy().astype(f64) - th1), e_th)
    print(f"adam, subnormal v': worst ratio to the bound m {r_m:.3f} v {r_v:.3f} theta {r_th:.3f}")
    assert (got_v > 0).all(), got_v
    assert r_m <= 1.0 and r_v <= 1.0 and r_th <= 1.0, (r_m, r_v, r_th)
    check_wcopy(wd, thd, n)


def test_adam_misaligned_buffers_are_refused_untouched():
    n = 64
    th, g, m, v = tail_inputs(1023)
    raw = L.lib().raw("rua_adam_step_w")
    for which in range(5):
        bufs = [up(a[:n + 4]) for a in (th, g, m, v)]
        wd = wcopy_buffer(th[:n + 4])
        before = [bits_of(b) for b in bufs] + [bits_of(wd.view(torch.bfloat16))]
        ptrs = [b.data_ptr() for b in bufs] + [wd.data_ptr()]
        ptrs[which] += 2 if which == 4 else 4
        rc = raw(ptrs[0], ptrs[1], ptrs[2], ptrs[3], n, float(LR_ADAM), None, float(B1), float(B2), float(EPS), 1.0, 1, ptrs[4], stream())
        torch.cuda.synchronize()
        assert rc != 0, which
        after = [bits_of(b) for b in bufs] + [bits_of(wd.view(torch.bfloat16))]
        for a, b in zip(before, after):
            assert (a == b).all(), which


def run_sgd(n, gs, zero, dev_lr, wc, entry="rua_sgd_step_w"):
    th, g, vel, _ = tail_inputs(n)
    thd, gd, vd = up(th), up(g), up(vel)
    wd = wcopy_buffer(th) if wc else None
    lrd = up(np.array([LR_SGD], f32)) if dev_lr else None
    args = [thd.data_ptr(), gd.data_ptr(), vd.data_ptr(), n, 0.0 if dev_lr else float(LR_SGD), lrd.data_ptr() if dev_lr else None,
            float(MU), gs, zero]
    if entry == "rua_sgd_step_w":
        args.append(wd.data_ptr() if wc else None)
    L.lib().call(entry, *args, stream())
    torch.cuda.synchronize()
    return thd, gd, vd, wd


@pytest.mark.parametrize("gs,zero,dev_lr,wc", VARIANTS)
@pytest.mark.parametrize("n", SGD_N)
def test_sgd_one_step(n, gs, zero, dev_lr, wc):
    th, g, vel, _ = tail_inputs(n)
    th1, vel1, e_th, e_v = sgd_ref(n, gs)
    thd, gd, vd, wd = run_sgd(n, gs, zero, dev_lr, wc)
    r_v = worst_ratio(np.abs(vd.cpu().numpy().astype(f64) - vel1), e_v)
    r_th = worst_ratio(np.abs(thd.cpu().numpy().astype(f64) - th1), e_th)
    print(f"sgd n={n} gs={gs} zero={zero} dev_lr={dev_lr} wcopy={wc}: worst ratio to the bound vel {r_v:.3f} theta {r_th:.3f}")
    assert r_v <= 1.0 and r_th <= 1.0, (n, r_v, r_th)
    assert (bits_of(gd) == (0 if zero else g.view(np.uint32))).all()
    pad = np.arange(0, n, 35)
    assert (bits_of(thd)[pad] == th.view(np.uint32)[pad]).all()
    assert (bits_of(vd)[pad] == 0).all()                      # mu * (+0) - lr * (+0) * gs is +0, fused or not
    if wc:
        check_wcopy(wd, thd, n)
        assert (bits_of(wd.view(torch.bfloat16))[pad] == bits_of(torch.from_numpy(th[pad]).to(torch.bfloat16))).all()
    else:
        th2, g2, v2, _ = run_sgd(n, gs, zero, dev_lr, False, entry="rua_sgd_step")
        for a, b in ((thd, th2), (gd, g2), (vd, v2)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- five steps on device state only: the counter, the rate and the kernel that reads it --------------------------------------------------
CHAIN_N, CHAIN_STEPS, CHAIN_T0, CHAIN_GS = 4099, 5, 7, 0.125


def test_adam_five_chained_steps_on_device_state():
    """rua_lr_step -> rua_adam_step_w(lr_t_dev) five times, nothing pushed from the host, against oracle/naive_ops.adam_step in float64 (which
    derives the rate from t itself).  Bound: the one-step bounds of the five steps, summed along the reference's trajectory - every one-step
    bound allows four times the worst case of the kernel's roundings (u/2 each), which leaves room for what a step inherits through beta < 1."""
    from oracle import naive_ops as nv
    n = CHAIN_N
    th, g, m, v = tail_inputs(n)
    b1, b2, eps, lr = float(B1), float(B2), float(EPS), float(LR_ADAM)
    thd, gd, md, vd, wd = up(th), up(g), up(m), up(v), wcopy_buffer(th)
    state, lrd = up(np.array([CHAIN_T0, lr], f64)), up(np.zeros(1, f32))
    r_th, r_m, r_v = th.astype(f64), m.astype(f64), v.astype(f64)
    gg = g.astype(f64) * CHAIN_GS
    b_th, b_m, b_v = np.zeros(n), np.zeros(n), np.zeros(n)
    for k in range(CHAIN_STEPS):
        L.lib().call("rua_lr_step", state.data_ptr(), lrd.data_ptr(), 1, b1, b2, stream())
        L.lib().call("rua_adam_step_w", thd.data_ptr(), gd.data_ptr(), md.data_ptr(), vd.data_ptr(), n, 0.0, lrd.data_ptr(), b1, b2, eps,
                     CHAIN_GS, 0, wd.data_ptr(), stream())
        t = CHAIN_T0 + 1 + k
        e_m = 4 * U32 * (b1 * np.abs(r_m) + (1 - b1) * np.abs(gg))
        new_th, r_m, r_v = nv.adam_step(r_th, gg, r_m, r_v, t, lr, b1, b2, eps)
        normal_range(r_v)
        den = np.sqrt(r_v) + eps
        b_m += e_m
        b_v += 4 * U32 * r_v
        b_th += U32 * np.abs(new_th) + 4e-6 * np.abs(r_th - new_th) + lr_ref(t, lr, b1, b2) * e_m / den
        r_th = new_th
    torch.cuda.synchronize()
    assert state.cpu().numpy()[0] == CHAIN_T0 + CHAIN_STEPS
    assert abs(float(lrd.cpu().numpy()[0]) - lr_ref(CHAIN_T0 + CHAIN_STEPS, lr, b1, b2)) <= np.spacing(f32(lr_ref(CHAIN_T0 + CHAIN_STEPS, lr, b1, b2)))
    q_m = worst_ratio(np.abs(md.cpu().numpy().astype(f64) - r_m), b_m)
    q_v = worst_ratio(np.abs(vd.cpu().numpy().astype(f64) - r_v), b_v)
    q_th = worst_ratio(np.abs(thd.cpu().numpy().astype(f64) - r_th), b_th)
    print(f"adam, {CHAIN_STEPS} chained steps from t={CHAIN_T0}: worst ratio to the summed bound m {q_m:.3f} v {q_v:.3f} theta {q_th:.3f}")
    assert q_m <= 1.0 and q_v <= 1.0 and q_th <= 1.0, (q_m, q_v, q_th)
    assert (bits_of(gd) == g.view(np.uint32)).all()
    check_wcopy(wd, thd, n)


def test_sgd_five_chained_steps_on_device_state():
    """The same with momentum SGD against naive_ops.sgd_step: rua_lr_step(adam = 0) hands the base rate through."""
    from oracle import naive_ops as nv
    n = CHAIN_N
    th, g, vel, _ = tail_inputs(n)
    mu, lr = float(MU), float(LR_SGD)
    thd, gd, vd, wd = up(th), up(g), up(vel), wcopy_buffer(th)
    state, lrd = up(np.array([CHAIN_T0, lr], f64)), up(np.zeros(1, f32))
    r_th, r_v = th.astype(f64), vel.astype(f64)
    gg = g.astype(f64) * CHAIN_GS
    b_th, b_v = np.zeros(n), np.zeros(n)
    for k in range(CHAIN_STEPS):
        L.lib().call("rua_lr_step", state.data_ptr(), lrd.data_ptr(), 0, 0.9, 0.999, stream())
        L.lib().call("rua_sgd_step_w", thd.data_ptr(), gd.data_ptr(), vd.data_ptr(), n, 0.0, lrd.data_ptr(), mu, CHAIN_GS, 0, wd.data_ptr(), stream())
        e_v = 4 * U32 * (mu * np.abs(r_v) + np.abs(lr * gg))
        r_th, r_v = nv.sgd_step(r_th, gg, r_v, lr, mu)
        b_v += e_v
        b_th += U32 * np.abs(r_th) + e_v
    torch.cuda.synchronize()
    assert state.cpu().numpy()[0] == CHAIN_T0 + CHAIN_STEPS and lrd.cpu().numpy()[0] == LR_SGD
    q_v = worst_ratio(np.abs(vd.cpu().numpy().astype(f64) - r_v), b_v)
    q_th = worst_ratio(np.abs(thd.cpu().numpy().astype(f64) - r_th), b_th)
    print(f"sgd, {CHAIN_STEPS} chained steps: worst ratio to the summed bound vel {q_v:.3f} theta {q_th:.3f}")
    assert q_v <= 1.0 and q_th <= 1.0, (q_v, q_th)
    check_wcopy(wd, thd, n)


# ---- the engine's own tail ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt", ["adam", "sgd"])
def test_engine_step_leaves_the_bf16_copy_of_its_master_and_zero_padding(opt):
    """After a training step of the bf16 engine the forward-layout copy is bf16 of the fp32 master, element for element, and the padding between the
    64-byte aligned slices of the flat buffer is still zero.  (Two engine runs are not compared bit for bit: atomic-order noise makes them differ.)"""
    from resunet_a_mltsk_keras_amd.synthetic import make_batch
    from test_model_gpu import make_pair
    shape, C = (64, 64, 6), 6
    _, eng = make_pair(shape, C, True, 32, "tanimoto", opt, dtype="bf16", seed=5, split_k=False)
    x, y = make_batch(2, 64, 6, C, True, seed=40, block=16)
    P0 = eng.P.cpu().numpy().copy()
    assert np.all(np.isfinite(eng.train_step(x, y)))
    torch.cuda.synchronize()
    nw = eng.params.nw
    assert 0 < nw <= eng.params.n
    P = eng.P.cpu()
    assert np.abs(P.numpy() - P0).max() > 0                   # the step did move the weights
    assert (bits_of(eng.Wf[:nw]) == bits_of(P[:nw].to(torch.bfloat16))).all()
    pad = np.ones(eng.params.n, bool)
    for e in eng.params.entries:
        pad[e["off"]:e["off"] + e["size"]] = False
    assert pad.any()
    assert (P.numpy()[pad] == 0).all()
    assert (eng.M1.cpu().numpy()[pad] == 0).all()
