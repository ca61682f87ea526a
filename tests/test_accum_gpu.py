"""rua_accum_gate, rua_accum_step and the gated forms of the rate kernels, the sum of squares and the finisher through the C ABI.

rua_accum_step: bit for bit accum.host_accumulate (NaN compared as NaN) on g and on the accumulator, for n = 4 (one 16-byte access), 20 (five
accesses, less than a wave), 22 (the element-by-element tail), 8192 * 3 + 4 (several blocks) and 2^22 + 12 * 4096 + 3 (the grid is capped at
4096 blocks, one pass of it covers 2^22 elements: the grid-stride loop, and a tail behind it), K = 2 and 3, hold and update, over normal
values, +-0, +-Inf and NaN, with guard elements on both sides of both buffers.
The gate: 2K + 1 launches give the hold pattern 1..1 0 1..1 0 1 and the counter 1 .. K-1 0 1 .. K-1 0 1.
The gated kernels: hold = 1 leaves every output buffer's pattern in place (the finisher writes only its two flags, 0 and 1); hold = 0 gives
the ungated entry point's bits on the same inputs (the finisher's second flag repeats the first)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from _kernel_util import bits_of, dev, stream, up  # noqa: E402
from resunet_a_mltsk_keras_amd import _lib as L  # noqa: E402
from resunet_a_mltsk_keras_amd import accum as AC  # noqa: E402
from resunet_a_mltsk_keras_amd import clip as CL  # noqa: E402
from resunet_a_mltsk_keras_amd import schedules as SC  # noqa: E402

f32, f64 = np.float32, np.float64
GUARD = 16                                                   # floats: keeps the inner buffer 16-byte aligned
SENT = f32(7.25)
GRID_PASS = 4096 * 256 * 4                                   # elements one pass of the largest grid covers
SIZES = [4, 20, 22, 8192 * 3 + 4, GRID_PASS + 12 * 4096 + 3]
B1, B2 = 0.9, 0.999


@functools.lru_cache(maxsize=None)
def values(n):
    """(g, a): seeded normal-range values with every special value against every special value in the first 49 pairs (and again at the end)."""
    rng = np.random.default_rng([n, 5])
    g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-8, 6, n)).astype(f32)
    a = (rng.standard_normal(n) * 10.0 ** rng.uniform(-8, 6, n)).astype(f32)
    sp = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.5, -3e38], f32)
    gg, aa = np.repeat(sp, 7), np.tile(sp, 7)
    m = min(n, 49)
    g[:m], a[:m] = gg[:m], aa[:m]
    g[n - m:], a[n - m:] = gg[::-1][:m], aa[::-1][:m]
    g[::13] = 0
    g.flags.writeable = a.flags.writeable = False
    return g, a


def guarded(x):
    return up(np.concatenate([np.full(GUARD, SENT, f32), x, np.full(GUARD, SENT, f32)]))


def same_bits(got, want):
    """Bit for bit, NaN compared as NaN (a NaN's payload is the adder's business)."""
    nan = np.isnan(want)
    return (np.isnan(got) == nan).all() and (got.view(np.uint32)[~nan] == want.view(np.uint32)[~nan]).all()


@pytest.mark.parametrize("hold", [1, 0], ids=["hold", "update"])
@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("n", SIZES)
def test_accum_step_is_the_host_definition(n, k, hold):
    g, a = values(n)
    gd, ad = guarded(g), guarded(a)
    flag = up(np.array([hold, 0, 0, 0], np.int32))
    L.lib().call("rua_accum_step", gd.data_ptr() + 4 * GUARD, ad.data_ptr() + 4 * GUARD, n, k, flag.data_ptr(), stream())
    a2, g_out, _ = AC.host_accumulate(a, g, 0 if hold else k - 1, k)
    got_g, got_a = gd.cpu().numpy(), ad.cpu().numpy()
    for buf in (got_g, got_a):
        assert (buf[:GUARD] == SENT).all() and (buf[GUARD + n:] == SENT).all()
    assert same_bits(got_a[GUARD:GUARD + n], a2)
    assert same_bits(got_g[GUARD:GUARD + n], g if hold else g_out)                 # a hold step leaves g to the flagged optimizer
    if not hold:
        assert not np.signbit(got_a[GUARD:GUARD + n]).any()                        # the reset is +0
    assert flag.cpu().numpy().tolist() == [hold, 0, 0, 0]


def test_accum_step_refuses_bad_arguments():
    g, a = values(20)
    gd, ad, flag = guarded(g), guarded(a), up(np.zeros(4, np.int32))
    raw = L.lib().raw("rua_accum_step")
    gp, ap = gd.data_ptr() + 4 * GUARD, ad.data_ptr() + 4 * GUARD
    for args in ((None, ap, 20, 2, flag.data_ptr()), (gp, None, 20, 2, flag.data_ptr()), (gp, ap, 0, 2, flag.data_ptr()), (gp, ap, 20, 1, flag.data_ptr()),
                 (gp, ap, 20, 2, None), (gp + 4, ap, 16, 2, flag.data_ptr()), (gp, gp, 20, 2, flag.data_ptr())):
        assert raw(*args, stream()) != 0
    assert same_bits(gd.cpu().numpy()[GUARD:GUARD + 20], g) and same_bits(ad.cpu().numpy()[GUARD:GUARD + 20], a)


@pytest.mark.parametrize("k", [2, 3, 5])
def test_gate_pattern_and_counter(k):
    st = up(np.array([0, 7, 7, 7], np.int32))
    hold = up(np.array([9, 7, 7, 7], np.int32))
    holds, counts = [], []
    for _ in range(2 * k + 1):
        L.lib().call("rua_accum_gate", st.data_ptr(), k, hold.data_ptr(), stream())
        s, h = st.cpu().numpy(), hold.cpu().numpy()
        assert (s[1:] == 7).all() and (h[1:] == 7).all()
        holds.append(int(h[0])); counts.append(int(s[0]))
    cycle_h, cycle_c = [1] * (k - 1) + [0], list(range(1, k)) + [0]
    assert holds == cycle_h * 2 + [1] and counts == cycle_c * 2 + [1]
    # a counter pushed from outside (a checkpoint in mid-cycle): the next launch closes the cycle
    st[0] = k - 1
    L.lib().call("rua_accum_gate", st.data_ptr(), k, hold.data_ptr(), stream())
    assert int(st.cpu()[0]) == 0 and int(hold.cpu()[0]) == 0
    raw = L.lib().raw("rua_accum_gate")
    assert raw(st.data_ptr(), 1, hold.data_ptr(), stream()) != 0 and raw(None, 2, hold.data_ptr(), stream()) != 0


SCHED = SC.CosineDecay(1e-4, 20, alpha=0.05, warmup_target=3e-3, warmup_steps=5)


def rate_call(gated, sched, state, out, adam, hold):
    lib = L.lib()
    tail = ((hold.data_ptr(),) if gated else ()) + (stream(),)
    if sched is None:
        lib.call("rua_lr_step" + ("_gated" if gated else ""), state.data_ptr(), out.data_ptr(), adam, B1, B2, *tail)
    else:
        lib.call("rua_lr_schedule_step" + ("_gated" if gated else ""), state.data_ptr(), out.data_ptr(), SC.to_struct(sched), adam, B1, B2, *tail)


@pytest.mark.parametrize("adam", [1, 0], ids=["adam", "sgd"])
@pytest.mark.parametrize("sched", [None, SCHED], ids=["constant", "schedule"])
def test_gated_rate_kernels(sched, adam):
    one, zero = up(np.array([1, 0, 0, 0], np.int32)), up(np.zeros(4, np.int32))
    s0, o0 = np.array([6.0, 2.5e-3], f64), np.full(4, -1.0, f32)
    state, out = up(s0), up(o0)
    rate_call(True, sched, state, out, adam, one)
    assert (bits_of(state) == s0.view(np.uint64)).all() and (bits_of(out) == o0.view(np.uint32)).all()
    ref_s, ref_o = up(s0), up(o0)
    for _ in range(3):                                                             # hold = 0: the ungated entry point, launch for launch
        rate_call(True, sched, state, out, adam, zero)
        rate_call(False, sched, ref_s, ref_o, adam, None)
        assert (bits_of(state) == bits_of(ref_s)).all() and (bits_of(out) == bits_of(ref_o)).all()
    assert state.cpu().numpy()[0] == 9.0 and (out.cpu().numpy()[1:] == -1.0).all()
    rate_call(True, sched, state, out, adam, one)                                  # ... and a hold step in between leaves the counter where it was
    assert (bits_of(state) == bits_of(ref_s)).all() and (bits_of(out) == bits_of(ref_o)).all()


def raw_table(a):
    return torch.from_numpy(np.frombuffer(a.tobytes(), dtype=np.uint8).copy()).to(dev())


@functools.lru_cache(maxsize=None)
def table():
    ch = CL.OPT_CHUNK
    entries, off = [], 0
    for name, size in (("a/kernel", 1), ("b/bias", 3), ("c/kernel", ch + 1), ("d/kernel", 2 * ch + 5), ("e/kernel", 40), ("e/kernel", ch + 7)):
        entries.append(dict(name=name, off=off, size=size))
        off += (size + 15) // 16 * 16
    chunks, vars_, names = CL.build_chunk_table(entries, ())
    rng = np.random.default_rng(3)
    g = (rng.standard_normal(off) * 10.0 ** rng.uniform(-6, 2, off)).astype(f32)
    return chunks, vars_, g


def finisher_buffers(nc, nv):
    return dict(partials=up(np.full(nc, -1.0, f64)), var_ss=up(np.full(nv, -2.0, f64)), coef=up(np.full(nv, -3.0, f32)), flag=up(np.full(4, 9, np.int32)),
                report=up(np.array([-4.0, -5.0, 2.0, 3.0], f64)))


def run_finisher(gated, gd, cd, vd, nc, nv, mode, c, skip, hold):
    b, lib = finisher_buffers(nc, nv), L.lib()
    tail = ((hold.data_ptr(),) if gated else ()) + (stream(),)
    sfx = "_gated" if gated else ""
    lib.call("rua_grad_sumsq" + sfx, gd.data_ptr(), cd.data_ptr(), nc, b["partials"].data_ptr(), *tail)
    lib.call("rua_clip_finish" + sfx, b["partials"].data_ptr(), nc, vd.data_ptr(), nv, mode, float(c), 0.5, skip, b["var_ss"].data_ptr(), b["coef"].data_ptr(),
             b["flag"].data_ptr(), b["report"].data_ptr(), *tail)
    return b


@pytest.mark.parametrize("poison", [False, True], ids=["finite", "inf"])
@pytest.mark.parametrize("mode", [CL.CLIP_NONE, CL.CLIP_GLOBAL_NORM, CL.CLIP_NORM], ids=["none", "global", "norm"])
def test_gated_sumsq_and_finisher(mode, poison):
    chunks, vars_, g = table()
    g = g.copy()
    if poison:
        big = int(np.argmax(chunks["len"]))                                          # a full chunk: the element lies inside it
        g[int(chunks["off"][big]) + 2] = np.inf
    nc, nv = len(chunks), len(vars_)
    gd, cd, vd = up(g), raw_table(chunks), raw_table(vars_)
    one, zero = up(np.array([1, 0, 0, 0], np.int32)), up(np.zeros(4, np.int32))
    fresh = finisher_buffers(nc, nv)
    held = run_finisher(True, gd, cd, vd, nc, nv, mode, 1e-3, 1, one)
    for key in ("partials", "var_ss", "coef", "report"):
        assert (bits_of(held[key]) == bits_of(fresh[key])).all(), key
    assert held["flag"].cpu().numpy().tolist() == [0, 1, 9, 9]                     # not skipped; hold or skipped
    upd = run_finisher(True, gd, cd, vd, nc, nv, mode, 1e-3, 1, zero)
    ref = run_finisher(False, gd, cd, vd, nc, nv, mode, 1e-3, 1, None)
    for key in ("partials", "var_ss", "coef", "report"):
        assert (bits_of(upd[key]) == bits_of(ref[key])).all(), key
    skip = 1 if poison else 0
    assert ref["flag"].cpu().numpy().tolist() == [skip, 9, 9, 9]
    assert upd["flag"].cpu().numpy().tolist() == [skip, skip, 9, 9]
    assert upd["report"].cpu().numpy()[2] == 2.0 + skip
    assert (bits_of(gd) == g.view(np.uint32)).all()
