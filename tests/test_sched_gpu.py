"""rua_lr_schedule_step and rua_ema_step through the C ABI against schedules.host_lr / schedules.host_ema.

Rate kernel: every kind runs 48 launches from t = 0 with decay_steps = 20 (warm-up 5, three piecewise boundaries), as Adam and as SGD, nothing
pushed from the host in between.  state[0] advances by one per launch, state[1] holds the scheduled rate, and
    |lr_out - float32(host)| <= ulp32(host) + 2^-40 * (largest rate of the schedule)
with host = host_lr(t - 1), times Adam's bias correction in float64.  The device's fp64 pow, cos and sqrt are off by a few fp64 ulps on quantities
no larger than that rate: that can move a float32 rounding by one ulp at most, and leaves a residue of that size where a cosine or a power ends
at exactly zero.  Table look-ups, the constant kind and the clamped tails involve no such function: their rate (state[1], and lr_out without the
bias correction) is exact.  A constant schedule gives rua_lr_step's bits.

rua_ema_step: bit for bit host_ema on ema and theta for n of 1, 3, 4 (16-byte tails), 1023 (less than one block's float4s), 4101 and 24583
(several blocks, ragged); 16 guard elements behind every buffer hold a sentinel no launch may touch."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from _kernel_util import bits_of, stream, up  # noqa: E402
from resunet_a_mltsk_keras_amd import _lib as L  # noqa: E402
from resunet_a_mltsk_keras_amd import schedules as SC  # noqa: E402

f32, f64 = np.float32, np.float64
B1, B2 = 0.9, 0.999
LAUNCHES = 48
GUARD = 16
SENT = f32(7.25)
SENT_BITS = 0x5A5A

# name -> (schedule, first step from which the rate is a constant that no pow / cos residue touches, or None)
KINDS = {
    "cosine": (SC.CosineDecay(3e-3, 20, alpha=0.1), 20),
    "cosine_to_zero": (SC.CosineDecay(3e-3, 20), 20),
    "cosine_warmup": (SC.CosineDecay(1e-4, 20, alpha=0.05, warmup_target=3e-3, warmup_steps=5), 25),
    "exponential": (SC.ExponentialDecay(3e-3, 20, 0.5), None),
    "exponential_staircase": (SC.ExponentialDecay(3e-3, 20, 0.5, staircase=True), None),
    "polynomial": (SC.PolynomialDecay(3e-3, 20, end_learning_rate=1e-5, power=2.0), 20),
    "polynomial_sqrt_cycle": (SC.PolynomialDecay(3e-3, 20, end_learning_rate=0.0, power=0.5, cycle=True), None),
    "piecewise": (SC.PiecewiseConstantDecay([3, 20, 33], [1e-3, 3e-3, 7e-4, 1e-4]), 0),
    "inverse_time": (SC.InverseTimeDecay(3e-3, 20, 0.7), None),
    "inverse_time_staircase": (SC.InverseTimeDecay(3e-3, 20, 0.7, staircase=True), None),
    "constant": (SC.Constant(1.2345e-3), 0),
}


def bias(t, adam):
    return np.sqrt(f64(1.0) - f64(B2) ** t) / (f64(1.0) - f64(B1) ** t) if adam else f64(1.0)


def sched_call(state, out, sched, adam):
    return L.lib().raw("rua_lr_schedule_step")(state.data_ptr(), out.data_ptr(), SC.to_struct(sched), adam, B1, B2, stream())


@pytest.mark.parametrize("adam", [1, 0], ids=["adam", "sgd"])
@pytest.mark.parametrize("name", list(KINDS))
def test_rate_of_48_launches(name, adam):
    sched, exact_from = KINDS[name]
    state, out = up(np.array([0.0, -1.0], f64)), up(np.full(4, -1.0, f32))
    worst, top = 0.0, sched.max_rate()
    for k in range(LAUNCHES):
        assert sched_call(state, out, sched, adam) == 0
        st, got = state.cpu().numpy(), out.cpu().numpy()
        t = k + 1
        rate = SC.host_lr(sched, t - 1)
        host = f64(rate) * bias(t, adam)
        assert st[0] == t
        bound = float(np.spacing(f32(host))) + 2.0 ** -40 * top
        err = abs(float(got[0]) - float(f32(host)))
        worst = max(worst, err / bound)
        assert err <= bound, (name, t, got[0], host)
        assert abs(st[1] - rate) <= 2.0 ** -40 * top, (name, t, st[1], rate)      # the base rate the weight decay reads
        if exact_from is not None and t - 1 >= exact_from:
            assert st[1] == rate, (name, t, st[1], rate)
            if not adam:
                assert got[0] == f32(rate) and got[:1].view(np.uint32)[0] == np.array([rate], f32).view(np.uint32)[0], (name, t, got[0], rate)
        assert (got[1:] == -1.0).all()
    print(f"rua_lr_schedule_step {name} {'adam' if adam else 'sgd'}: worst ratio to the bound {worst:.3f}")


@pytest.mark.parametrize("adam", [1, 0], ids=["adam", "sgd"])
def test_constant_schedule_gives_rua_lr_step_s_bits(adam):
    lr = 1.2345e-3
    sa, oa = up(np.array([0.0, lr], f64)), up(np.zeros(1, f32))
    sb, ob = up(np.array([0.0, -1.0], f64)), up(np.zeros(1, f32))
    for k in range(LAUNCHES):
        L.lib().call("rua_lr_step", sa.data_ptr(), oa.data_ptr(), adam, B1, B2, stream())
        assert sched_call(sb, ob, SC.Constant(lr), adam) == 0
        assert (bits_of(oa) == bits_of(ob)).all(), k
        assert (bits_of(sa) == bits_of(sb)).all(), k


def test_rate_kernel_resumes_from_a_pushed_counter_and_refuses_bad_tables():
    sched = KINDS["cosine_warmup"][0]
    state, out = up(np.array([17.0, 0.0], f64)), up(np.zeros(1, f32))
    assert sched_call(state, out, sched, 0) == 0
    assert state.cpu().numpy()[0] == 18.0
    host = SC.host_lr(sched, 17)
    assert abs(float(out.cpu().numpy()[0]) - float(f32(host))) <= float(np.spacing(f32(host))) + 2.0 ** -40 * sched.max_rate()
    raw = L.lib().raw("rua_lr_schedule_step")
    st = SC.to_struct(sched)
    st.decay_steps = 0.0
    assert raw(state.data_ptr(), out.data_ptr(), st, 0, B1, B2, stream()) != 0
    st = SC.to_struct(KINDS["piecewise"][0])
    st.n_boundaries = 17
    assert raw(state.data_ptr(), out.data_ptr(), st, 0, B1, B2, stream()) != 0
    st = SC.to_struct(sched)
    st.kind = 6
    assert raw(state.data_ptr(), out.data_ptr(), st, 0, B1, B2, stream()) != 0
    assert raw(None, out.data_ptr(), SC.to_struct(sched), 0, B1, B2, stream()) != 0
    assert state.cpu().numpy()[0] == 18.0


# ---- rua_ema_step -----------------------------------------------------------------------------------------------------------------------
def ema_inputs(n):
    rng = np.random.default_rng([n, 23])
    N = n + GUARD
    e = (rng.standard_normal(N) * 10.0 ** rng.uniform(-6, 2, N)).astype(f32)
    th = (rng.standard_normal(N) * 10.0 ** rng.uniform(-6, 2, N)).astype(f32)
    e[::7] = 0
    th[::5] = 0
    e[n:] = SENT
    th[n:] = SENT
    return e, th


def bf16_bits(a):
    return bits_of(torch.from_numpy(np.ascontiguousarray(a, f32)).to(torch.bfloat16))


def ema_case(n, t, mom, every, flag, with_copy):
    """One launch on fresh buffers; returns nothing, asserts everything."""
    e, th = ema_inputs(n)
    ed, thd = up(e), up(th)
    wd = up(np.full(n + GUARD, SENT_BITS, np.uint16).view(np.int16)).view(torch.bfloat16) if with_copy else None
    state = up(np.array([float(t), 1e-3], f64))
    fl = None if flag is None else up(np.array([flag, 0, 0, 0], np.int32))
    L.lib().call("rua_ema_step", ed.data_ptr(), thd.data_ptr(), wd.data_ptr() if with_copy else None, n, float(mom), state.data_ptr(), every,
                 fl.data_ptr() if fl is not None else None, stream())
    torch.cuda.synchronize()
    skipped = bool(flag)
    e_ref, th_ref = SC.host_ema(e[:n], th[:n], mom, t, every, skipped=skipped)
    tag = (n, t, every, flag, with_copy)
    assert (bits_of(ed)[:n] == e_ref.view(np.uint32)).all(), tag
    assert (bits_of(thd)[:n] == th_ref.view(np.uint32)).all(), tag
    assert (bits_of(ed)[n:] == np.array([SENT], f32).view(np.uint32)[0]).all() and (bits_of(thd)[n:] == np.array([SENT], f32).view(np.uint32)[0]).all(), tag
    over = every > 0 and t % every == 0 and not skipped
    if not over:
        assert (bits_of(thd)[:n] == th[:n].view(np.uint32)).all(), tag             # theta untouched
    if skipped:
        assert (bits_of(ed)[:n] == e[:n].view(np.uint32)).all(), tag
    if with_copy:
        wb = bits_of(wd)
        assert (wb[n:] == SENT_BITS).all(), tag
        assert (wb[:n] == (bf16_bits(e_ref) if over else SENT_BITS)).all(), tag    # written by an overwrite only, then bf16(ema)
    assert state.cpu().numpy().tolist() == [float(t), 1e-3]


@pytest.mark.parametrize("n", [1, 3, 4, 1023, 4101, 24583])
def test_ema_step_against_the_host_definition(n):
    for t in (1, 2):
        for flag in (None, 0, 1):
            for with_copy in (False, True):
                ema_case(n, t, 0.9, 0, flag, with_copy)
    for t in (2, 3):                                                               # t = 2: theta untouched; t = 3: theta = ema, wcopy = bf16(ema)
        for flag in (None, 1):
            for with_copy in (False, True):
                ema_case(n, t, 0.9, 3, flag, with_copy)
    ema_case(n, 1, 0.99, 1, 0, True)                                               # first step and overwrite at once: everything is theta
    ema_case(n, 4, 0.999, 2, None, True)
    ema_case(n, 5, 1.0, 0, None, False)                                            # momentum 1: the average stands still
    ema_case(n, 5, 0.0, 0, None, False)                                            # momentum 0: the average is theta


def test_ema_step_refuses_bad_arguments():
    e, th = ema_inputs(64)
    ed, thd, state = up(e), up(th), up(np.array([2.0, 0.0], f64))
    raw = L.lib().raw("rua_ema_step")
    ok = lambda *a: raw(*a, stream())
    assert ok(ed.data_ptr(), thd.data_ptr(), None, 64, 1.5, state.data_ptr(), 0, None) != 0
    assert ok(ed.data_ptr(), thd.data_ptr(), None, 64, 0.9, state.data_ptr(), -1, None) != 0
    assert ok(ed.data_ptr(), thd.data_ptr(), None, 0, 0.9, state.data_ptr(), 0, None) != 0
    assert ok(ed.data_ptr(), ed.data_ptr(), None, 64, 0.9, state.data_ptr(), 0, None) != 0
    assert ok(ed.data_ptr() + 4, thd.data_ptr(), None, 32, 0.9, state.data_ptr(), 0, None) != 0
    assert ok(ed.data_ptr(), thd.data_ptr(), None, 64, 0.9, None, 0, None) != 0
    torch.cuda.synchronize()
    assert (bits_of(ed) == e.view(np.uint32)).all() and (bits_of(thd) == th.view(np.uint32)).all()
