"""LAMB through the C ABI: rua_lamb_moments, rua_lamb_finish and rua_lamb_apply against lamb.py's float32 definition.

The table is tests/test_clip_gpu.py's, rebuilt here: variables of 1, 3, 16, CHUNK - 1, CHUNK, CHUNK + 1 and 2 * CHUNK + 5 elements and one variable
made of two entries; gradients span fifteen decades, zeros are sprinkled into g, m, v and theta.  Padding between the slices and 16 guard elements
behind every buffer hold a sentinel that no kernel may touch.

What is compared how:
  m', v', u      bit for bit lamb.host_lamb_step's: every float32 operation of the kernel is rounded on its own and IEEE, as numpy's are
  pw, pu         sums of squares that are exact in float64 and non-negative: ANY order of L terms is within L * 2^-53 (relative) of the exact sum,
                 and so is numpy's - the test allows L * 2^-53 between the two, as test_clip_gpu.py does for rua_grad_sumsq
  ratio          the float64 sums may differ in their last bits, so the rounding to float32 can fall on either side: one float32 ulp
  theta'         bit for bit the host's GIVEN the device's ratio read back (host_lamb_step(ratio=...))"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from _kernel_util import bits_of, dev, frozen, stream, up  # noqa: E402
from resunet_a_mltsk_keras_amd import _lib as L  # noqa: E402
from resunet_a_mltsk_keras_amd import clip as CL  # noqa: E402
from resunet_a_mltsk_keras_amd import lamb as LB  # noqa: E402

f32, f64 = np.float32, np.float64
CH = CL.OPT_CHUNK
B1, B2, EPS = f32(0.9), f32(0.999), f32(1e-7)
LR, LR_BASE = f32(1.2345e-3), 1e-3
WD = 0.05
GUARD = 16
SENT = f32(7.25)                                             # padding and guards of the float buffers
SENT_BITS = 0x5A5A                                           # ... of the bf16 copy
STALE_BITS = 0x1234                                          # the bf16 copy inside the chunks before a run: whatever is there afterwards was written
SIZES = [("a/kernel", 1), ("b/bias", 3), ("c/gamma", 16), ("d/kernel", CH - 1), ("e/kernel", CH), ("f/beta", CH + 1), ("g/kernel", 2 * CH + 5),
         ("h/kernel", 40), ("h/kernel", CH + 7), ("h/bias", 5)]
EXCLUDE = ("bias", "gamma", "beta")


@functools.lru_cache(maxsize=None)
def table():
    entries, off = [], 0
    for name, size in SIZES:
        entries.append(dict(name=name, off=off, size=size))
        off += (size + 15) // 16 * 16
    chunks, vars_, names = CL.build_chunk_table(entries, EXCLUDE)
    inside = CL.covered(chunks, off) == 1
    assert inside.sum() == sum(s for _, s in SIZES) and (CL.covered(chunks, off) <= 1).all()
    return frozen(chunks, vars_, inside) + (names, off)


@functools.lru_cache(maxsize=None)
def inputs():
    chunks, vars_, inside, names, n = table()
    rng = np.random.default_rng([n, 11])
    N = n + GUARD
    g = (rng.standard_normal(N) * 10.0 ** rng.uniform(-12, 3, N)).astype(f32)
    m = (rng.standard_normal(N) * 10.0 ** rng.uniform(-6, 1, N)).astype(f32)
    v = ((rng.standard_normal(N) * 10.0 ** rng.uniform(-6, 1, N)) ** 2).astype(f32)
    th = rng.standard_normal(N).astype(f32)
    g[::7] = 0
    m[::5] = 0
    v[::5] = 0
    th[::11] = 0
    out = np.ones(N, bool)
    out[:n] = ~inside
    for a in (th, g, m, v):
        a[out] = SENT
    return frozen(th, g, m, v, out)


def var_slices(name):
    chunks, vars_, inside, names, n = table()
    k = names.index(name)
    return [slice(int(c["off"]), int(c["off"] + c["len"])) for c in chunks[vars_[k]["chunk_begin"]:vars_[k]["chunk_end"]]]


def raw_table(a):
    return torch.from_numpy(np.frombuffer(a.tobytes(), dtype=np.uint8).copy()).to(dev())


def wcopy_buffer(out):
    w = np.full(out.size, STALE_BITS, np.uint16)
    w[out] = SENT_BITS
    return torch.from_numpy(w.view(np.int16).copy()).to(dev())


def coef_vector(per_var):
    nv = len(table()[1])
    return (np.linspace(0.25, 1.0, nv) if per_var else np.ones(nv)).astype(f32)


def value_gradient(gs):
    """inputs()' gradient with elements whose g * gs is exactly +1, -1 (the clip value), one ulp inside and well outside."""
    chunks, vars_, inside, names, n = table()
    g = inputs()[1].copy()
    idx = np.flatnonzero(inside)[::97]
    vals = np.array([1.0, -1.0, np.nextafter(f32(1), f32(0)), -np.nextafter(f32(1), f32(0)), 3.5, -1e3], f32) / f32(gs)   # gs a power of two: exact
    g[idx] = np.resize(vals, idx.size)
    return g


def run_lamb(g=None, th=None, m=None, *, t=4, gs=1.0, coef=None, cv=0.0, wd=0.0, wc=True, flag=None, report=None):
    """The three launches on fresh device copies of inputs() (g, th, m replaced where given); the state after pass 1 is kept next to the end state."""
    chunks, vars_, inside, names, n = table()
    th0, g0, m0, v0, out = inputs()
    thd, gd, md, vd = up(th0 if th is None else th), up(g0 if g is None else g), up(m0 if m is None else m), up(v0)
    wd_ = wcopy_buffer(out) if wc else None
    chunks_d, vars_d = raw_table(chunks), raw_table(vars_)
    nc, nv = len(chunks), len(vars_)
    coef_d = up(coef_vector(False) if coef is None else coef)
    lrd, state = up(np.array([LR], f32)), up(np.array([float(t), LR_BASE], f64))
    pw, pu = up(np.full(nc + 2, -1.0, f64)), up(np.full(nc + 2, -1.0, f64))
    var_wu, ratio = up(np.full(2 * nv + 2, -1.0, f64)), up(np.full(nv + 2, -1.0, f32))
    report = up(np.zeros(4, f64)) if report is None else report
    fl = up(np.array([flag, 0, 0, 0], np.int32)) if flag is not None else None
    flp = fl.data_ptr() if fl is not None else None
    lib, s = L.lib(), stream()
    lib.call("rua_lamb_moments", thd.data_ptr(), gd.data_ptr(), md.data_ptr(), vd.data_ptr(), chunks_d.data_ptr(), nc, vars_d.data_ptr(), coef_d.data_ptr(), flp,
             state.data_ptr(), float(B1), float(B2), float(EPS), float(gs), float(cv), float(wd), pw.data_ptr(), pu.data_ptr(), s)
    torch.cuda.synchronize()
    after1 = dict(th=thd.clone(), u=gd.clone(), m=md.clone(), v=vd.clone())
    lib.call("rua_lamb_finish", pw.data_ptr(), pu.data_ptr(), nc, vars_d.data_ptr(), nv, flp, var_wu.data_ptr(), ratio.data_ptr(), report.data_ptr(), s)
    lib.call("rua_lamb_apply", thd.data_ptr(), gd.data_ptr(), chunks_d.data_ptr(), nc, vars_d.data_ptr(), ratio.data_ptr(), flp, lrd.data_ptr(), state.data_ptr(),
             float(wd), 1, wd_.data_ptr() if wc else None, s)
    torch.cuda.synchronize()
    return dict(th=thd, g=gd, m=md, v=vd, w=wd_, pw=pw, pu=pu, var_wu=var_wu, ratio=ratio, report=report, after1=after1)


def host(g=None, th=None, m=None, *, t=4, gs=1.0, coef=None, cv=0.0, wd=0.0, ratio=None):
    chunks, vars_, inside, names, n = table()
    th0, g0, m0, v0, out = inputs()
    return LB.host_lamb_step((th0 if th is None else th)[:n], (g0 if g is None else g)[:n], (m0 if m is None else m)[:n], v0[:n], chunks, vars_, t=t, lr=LR,
                             lr_base=LR_BASE, beta_1=B1, beta_2=B2, eps=EPS, grad_scale=gs, coef=coef, clipvalue=cv or None, weight_decay=wd, ratio=ratio)


def check_untouched(r, wc=True):
    th0, g0, m0, v0, out = inputs()
    n = table()[4]
    nc, nv = len(table()[0]), len(table()[1])
    for name, a in (("th", th0), ("g", g0), ("m", m0), ("v", v0)):
        assert (bits_of(r[name])[out] == a.view(np.uint32)[out]).all(), name
    for name, a in (("th", th0), ("u", g0), ("m", m0), ("v", v0)):
        assert (bits_of(r["after1"][name])[out] == a.view(np.uint32)[out]).all(), name
    if wc:
        assert (bits_of(r["w"].view(torch.bfloat16))[out] == SENT_BITS).all()
    assert (r["pw"].cpu().numpy()[nc:] == -1).all() and (r["pu"].cpu().numpy()[nc:] == -1).all()
    assert (r["var_wu"].cpu().numpy()[2 * nv:] == -1).all() and (r["ratio"].cpu().numpy()[nv:] == -1).all()


def ulps32(got, exp):
    exp = np.asarray(exp, f32)
    return float(np.max(np.abs(np.asarray(got, f64) - exp.astype(f64)) / np.spacing(np.abs(exp)).astype(f64)))


CASES = {"plain": dict(gs=1.0), "scaled, per-variable coefficient, decay": dict(gs=0.125, per_var=True, wd=WD),
         "scaled, clip value": dict(gs=0.125, cv=1.0), "coefficient and decay": dict(gs=1.0, per_var=True, wd=WD), "decay alone": dict(gs=1.0, wd=WD)}


def case_args(case):
    c = CASES[case]
    g = value_gradient(c["gs"]) if c.get("cv") else None
    return g, dict(gs=c["gs"], coef=coef_vector(c.get("per_var", False)), cv=c.get("cv", 0.0), wd=c.get("wd", 0.0))


# ---- the three kernels against the host definition ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [1, 2, 1000])
@pytest.mark.parametrize("case", list(CASES))
def test_the_update_against_the_host_definition(case, t):
    chunks, vars_, inside, names, n = table()
    th0, g0, m0, v0, out = inputs()
    g, kw = case_args(case)
    r = run_lamb(g, t=t, **kw)
    h = host(g, t=t, **kw)
    # pass 1: m', v', u bit for bit; theta only read
    a1 = r["after1"]
    for k, hk in (("m", "m"), ("v", "v"), ("u", "u")):
        got, want = bits_of(a1[k])[:n][inside], h[hk].view(np.uint32)[inside]
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (k, bad.size, bad[:5], got[bad[:5]], want[bad[:5]])
    assert (bits_of(a1["th"]) == th0.view(np.uint32)).all()
    assert (bits_of(r["m"]) == bits_of(a1["m"])).all() and (bits_of(r["v"]) == bits_of(a1["v"])).all()      # pass 2 leaves the moments alone
    pw, pu = r["pw"].cpu().numpy(), r["pu"].cpu().numpy()
    worst = 0.0
    for k, (off, ln, _) in enumerate(chunks.tolist()):
        for got, x in ((pw[k], h["th1"][off:off + ln].astype(f64)), (pu[k], h["u"][off:off + ln].astype(f64))):
            ref = np.dot(x, x)
            assert abs(got - ref) <= ln * 2.0 ** -53 * ref, (k, got, ref)
            worst = max(worst, abs(got - ref) / (ln * 2.0 ** -53 * ref) if ref > 0 else 0.0)
    # the finisher: one ulp of the host's ratio; the report
    ratio = r["ratio"].cpu().numpy()[:len(vars_)]
    rep, hrep = r["report"].cpu().numpy(), LB.host_ratio_report(h["W"], h["U"])
    ul = ulps32(ratio, h["ratio"])
    print(f"{case} t={t}: partials' worst ratio to L * 2^-53: {worst:.3f}; ratio {ul:.2f} ulp; ratios {ratio.min():.4g} .. {ratio.max():.4g}, forced {int(rep[2])}")
    assert ul <= 1.0
    assert rep[0] == ratio.min() and rep[1] == ratio.max() and rep[2] == hrep["forced"] and rep[3] == 1
    assert names[0] == "a/kernel" and th0[0] == 0 and ratio[0] == 1.0 and hrep["forced"] >= 1             # the one-element variable sits on a planted zero
    assert len(np.unique(ratio)) >= len(vars_) - 2                                                      # per variable: they do differ
    # pass 2: bit for bit given the device's ratio; the gradient's slot is +0, the bf16 copy is bf16(theta')
    h2 = host(g, t=t, ratio=ratio, **kw)
    got, want = bits_of(r["th"])[:n][inside], h2["theta"].view(np.uint32)[inside]
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, ("theta", bad.size, bad[:5], got[bad[:5]], want[bad[:5]])
    assert (got != th0[:n].view(np.uint32)[inside]).any()                                                # the weights did move (a small ratio leaves many
                                                                                                         # steps below half an ulp of their weight)
    assert (bits_of(r["g"])[:n][inside] == 0).all()
    w = bits_of(r["w"].view(torch.bfloat16))[:n][inside]
    assert (w == bits_of(r["th"].cpu()[:n][torch.from_numpy(inside.copy())].to(torch.bfloat16))).all()
    check_untouched(r)
    if CASES[case].get("cv"):
        assert np.abs(h["gg"]).max() == 1.0 and (np.abs(h["gg"][np.flatnonzero(inside)[::97]]) == 1.0).sum() >= 4
    if CASES[case].get("wd"):
        dec = np.zeros(n, bool)
        for off, ln, var in chunks.tolist():
            dec[off:off + ln] = bool(vars_["decay"][var])
        assert (h["th1"][dec] != th0[:n][dec]).any() and (h["th1"][inside & ~dec] == th0[:n][inside & ~dec]).all()


def test_two_runs_give_identical_bits_and_no_bf16_copy_changes_nothing_else():
    g, kw = case_args("scaled, per-variable coefficient, decay")
    a, b, c = run_lamb(g, **kw), run_lamb(g, **kw), run_lamb(g, wc=False, **kw)
    for other in (b, c):
        for k in ("th", "g", "m", "v", "pw", "pu", "var_wu", "ratio", "report"):
            assert (bits_of(a[k]) == bits_of(other[k])).all(), k
        assert (bits_of(a["after1"]["u"]) == bits_of(other["after1"]["u"])).all()
    check_untouched(c, wc=False)


def test_undecayed_variables_match_the_run_without_decay_bit_for_bit():
    chunks, vars_, inside, names, n = table()
    a, b = run_lamb(wd=WD), run_lamb(wd=0.0)
    keep, moved = np.zeros(n, bool), 0
    for off, ln, var in chunks.tolist():
        keep[off:off + ln] = not vars_["decay"][var]
    assert keep.any() and [nm for nm, v in zip(names, vars_) if not v["decay"]] == ["b/bias", "c/gamma", "f/beta", "h/bias"]
    for k in ("th", "m", "v"):
        x, y = bits_of(a[k])[:n], bits_of(b[k])[:n]
        assert (x[keep] == y[keep]).all(), k
        moved += int((x[inside & ~keep] != y[inside & ~keep]).sum())
    assert moved > 0
    assert (bits_of(a["w"].view(torch.bfloat16))[:n][keep] == bits_of(b["w"].view(torch.bfloat16))[:n][keep]).all()
    ra, rb = a["ratio"].cpu().numpy(), b["ratio"].cpu().numpy()
    und = np.array([not v["decay"] for v in vars_])
    assert (ra[:len(vars_)][und] == rb[:len(vars_)][und]).all() and (ra[:len(vars_)][~und] != rb[:len(vars_)][~und]).any()


# ---- the finisher -------------------------------------------------------------------------------------------------------------------------------
def test_zero_norms_give_ratio_one_and_are_counted():
    chunks, vars_, inside, names, n = table()
    th0, g0, m0, v0, out = inputs()
    th, g, m = th0.copy(), g0.copy(), m0.copy()
    for sl in var_slices("h/kernel"):                                                # the two-entry variable: an all-zero variable
        th[sl] = 0
    for sl in var_slices("f/beta"):                                                  # an all-zero update: g and m zero (v stays)
        g[sl] = 0
        m[sl] = 0
    base = run_lamb()
    r = run_lamb(g, th, m)
    ratio, rep = r["ratio"].cpu().numpy()[:len(vars_)], r["report"].cpu().numpy()
    wu = r["var_wu"].cpu().numpy()
    kh, kf = names.index("h/kernel"), names.index("f/beta")
    assert wu[kh] == 0 and wu[len(vars_) + kf] == 0 and wu[len(vars_) + kh] > 0 and wu[kf] > 0
    assert ratio[kh] == 1.0 and ratio[kf] == 1.0
    assert rep[2] == base["report"].cpu().numpy()[2] + 2
    h = host(g, th, m)
    assert rep[2] == LB.host_ratio_report(h["W"], h["U"])["forced"] and ulps32(ratio, h["ratio"]) <= 1.0
    # ratio 1 is a plain Adam step of the base rate there: theta' = th1 - lr * u, bit for bit
    h2 = host(g, th, m, ratio=ratio)
    assert (bits_of(r["th"])[:n][inside] == h2["theta"].view(np.uint32)[inside]).all()
    for sl in var_slices("f/beta"):
        assert (bits_of(r["th"])[sl] == th0[sl].view(np.uint32)).all()                # u = 0: the weights stay


@pytest.mark.parametrize("layout", ["a variable across the tile edge", "more variables than a tile"])
def test_finisher_adds_in_chunk_order_beyond_one_tile(layout):
    """The finisher stages the partials through LDS 4096 at a time: with more chunks in a variable than the block has threads, a variable across
    the tile edge and more variables than a tile, both sums of every variable are still the bits of a serial loop in chunk order."""
    TILE = 4096
    if layout == "a variable across the tile edge":
        ranges = [(0, 10), (10, TILE + 104), (TILE + 104, TILE + 105), (TILE + 105, 2 * TILE + 300)]
    else:
        ranges = [(k, k + 1) for k in range(TILE + 37)]
    nc, nv = ranges[-1][1], len(ranges)
    rng = np.random.default_rng(nc)
    pw = (rng.standard_normal(nc) ** 2 * 10.0 ** rng.uniform(-20, 6, nc)).astype(f64)
    pu = (rng.standard_normal(nc) ** 2 * 10.0 ** rng.uniform(-20, 6, nc)).astype(f64)
    if nv > TILE:
        pw[5] = 0.0                                                                  # forced ones on both sides of the tile edge
        pu[TILE + 20] = 0.0
    vars_ = np.array([(a, b, 1, 0) for a, b in ranges], dtype=CL.VAR_DTYPE)
    pw_d, pu_d, vars_d = up(pw), up(pu), raw_table(vars_)
    var_wu, ratio, report = up(np.full(2 * nv + 2, -1.0, f64)), up(np.full(nv + 2, -1.0, f32)), up(np.zeros(4, f64))
    L.lib().call("rua_lamb_finish", pw_d.data_ptr(), pu_d.data_ptr(), nc, vars_d.data_ptr(), nv, None, var_wu.data_ptr(), ratio.data_ptr(), report.data_ptr(), stream())
    torch.cuda.synchronize()
    exp = np.zeros(2 * nv, f64)
    for half, part in enumerate((pw, pu)):
        for v, (a, b) in enumerate(ranges):
            acc = 0.0
            for x in part[a:b].tolist():
                acc += x
            exp[half * nv + v] = acc
    got = var_wu.cpu().numpy()
    assert (got[:2 * nv].view(np.uint64) == exp.view(np.uint64)).all() and (got[2 * nv:] == -1).all()
    want = LB.host_ratio_report(exp[:nv], exp[nv:])
    rt, rep = ratio.cpu().numpy(), report.cpu().numpy()
    assert ulps32(rt[:nv], want["ratio"]) <= 1.0 and (rt[nv:] == -1).all()
    assert rep[0] == rt[:nv].min() and rep[1] == rt[:nv].max() and rep[2] == want["forced"] == (2 if nv > TILE else 0) and rep[3] == 1


def test_report_counts_updates_over_several_calls_and_not_the_flagged_ones():
    report = up(np.zeros(4, f64))
    for flag in (None, None, 1, 0, None):
        r = run_lamb(report=report, flag=flag)
    rep = report.cpu().numpy()
    assert rep[3] == 4 and rep[0] == r["ratio"].cpu().numpy()[:len(table()[1])].min()


# ---- the flag -----------------------------------------------------------------------------------------------------------------------------------
def test_flag_set_only_the_gradient_is_zeroed_and_the_bf16_copy_rewritten():
    chunks, vars_, inside, names, n = table()
    th0, g0, m0, v0, out = inputs()
    report = up(np.array([0.5, 2.0, 1.0, 7.0], f64))
    r = run_lamb(wd=WD, flag=1, report=report)
    for k, a in (("th", th0), ("m", m0), ("v", v0)):
        assert (bits_of(r[k]) == a.view(np.uint32)).all(), k
    for k in ("pw", "pu", "var_wu", "ratio"):
        assert (r[k].cpu().numpy() == -1).all(), k
    assert r["report"].cpu().numpy().tolist() == [0.5, 2.0, 1.0, 7.0]
    assert (bits_of(r["after1"]["u"])[:n][inside] == 0).all() and (bits_of(r["g"])[:n][inside] == 0).all()      # pass 1 already zeroed it
    w = bits_of(r["w"].view(torch.bfloat16))[:n][inside]
    assert (w == bits_of(torch.from_numpy(th0[:n][inside]).to(torch.bfloat16))).all() and (w != STALE_BITS).any()
    check_untouched(r)
    # an armed flag that is not set changes nothing
    a, b = run_lamb(wd=WD, flag=0), run_lamb(wd=WD)
    for k in ("th", "g", "m", "v", "pw", "pu", "ratio", "report"):
        assert (bits_of(a[k]) == bits_of(b[k])).all(), k


# ---- a NaN in one variable's gradient, no flag armed: plain arithmetic ------------------------------------------------------------------------------
def test_a_nan_gradient_stays_inside_its_variable():
    chunks, vars_, inside, names, n = table()
    g0 = inputs()[1]
    k = names.index("e/kernel")
    sl = var_slices("e/kernel")[0]
    g = g0.copy()
    g[sl.start + 77] = np.nan
    clean, r = run_lamb(), run_lamb(g)
    ratio = r["ratio"].cpu().numpy()[:len(vars_)]
    assert ratio[k] == 1.0 and np.isnan(r["var_wu"].cpu().numpy()[len(vars_) + k])
    assert r["report"].cpu().numpy()[2] == clean["report"].cpu().numpy()[2] + 1
    th = r["th"].cpu().numpy()
    assert np.isnan(th[sl.start + 77]) and np.isfinite(np.delete(th[sl], 77)).all()
    other = inside.copy()
    other[sl] = False
    for key in ("th", "m", "v"):
        assert (bits_of(r[key])[:n][other] == bits_of(clean[key])[:n][other]).all(), key
    assert (np.delete(ratio, k) == np.delete(clean["ratio"].cpu().numpy()[:len(vars_)], k)).all()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_nothing_is_written():
    chunks, vars_, inside, names, n = table()
    th0, g0, m0, v0, out = inputs()
    bufs = [up(a) for a in (th0, g0, m0, v0)]
    wd_ = wcopy_buffer(out)
    chunks_d, vars_d = raw_table(chunks), raw_table(vars_)
    nc, nv = len(chunks), len(vars_)
    pw, pu, var_wu = up(np.full(nc, -1.0, f64)), up(np.full(nc, -1.0, f64)), up(np.full(2 * nv, -1.0, f64))
    coef, ratio, report = up(np.ones(nv, f32)), up(np.full(nv, -1.0, f32)), up(np.full(4, -2.0, f64))
    lrd, state = up(np.array([LR], f32)), up(np.array([4.0, LR_BASE], f64))
    watched = bufs + [wd_.view(torch.bfloat16), pw, pu, var_wu, ratio, report]
    before = [bits_of(t) for t in watched]
    lib, s = L.lib(), stream()
    P = [t.data_ptr() for t in bufs]
    mom, fin, app = (lib.raw(k) for k in ("rua_lamb_moments", "rua_lamb_finish", "rua_lamb_apply"))
    rcs = []
    ma = [P[0], P[1], P[2], P[3], chunks_d.data_ptr(), nc, vars_d.data_ptr(), coef.data_ptr(), None, state.data_ptr(), float(B1), float(B2), float(EPS), 1.0, 0.0,
          0.0, pw.data_ptr(), pu.data_ptr(), s]
    for i, bad in ((0, None), (1, None), (2, None), (3, None), (4, None), (5, 0), (5, -1), (6, None), (7, None), (9, None), (16, None), (17, None),
                   (0, P[0] + 4), (1, P[1] + 8), (2, P[2] + 4), (3, P[3] + 12), (4, chunks_d.data_ptr() + 8), (8, coef.data_ptr() + 2),
                   (9, state.data_ptr() + 4), (16, pw.data_ptr() + 4), (17, pw.data_ptr()), (10, 1.0), (10, -0.1), (11, 1.0), (11, float("nan")),
                   (12, 0.0), (12, -1e-7), (12, float("inf")), (15, -0.5)):
        a = list(ma)
        a[i] = bad
        rcs.append(mom(*a))
    fa = [pw.data_ptr(), pu.data_ptr(), nc, vars_d.data_ptr(), nv, None, var_wu.data_ptr(), ratio.data_ptr(), report.data_ptr(), s]
    for i, bad in ((0, None), (1, None), (2, 0), (2, -2), (3, None), (4, 0), (4, -1), (6, None), (7, None), (8, None), (0, pw.data_ptr() + 4),
                   (6, var_wu.data_ptr() + 4), (7, ratio.data_ptr() + 2), (3, vars_d.data_ptr() + 8)):
        a = list(fa)
        a[i] = bad
        rcs.append(fin(*a))
    aa = [P[0], P[1], chunks_d.data_ptr(), nc, vars_d.data_ptr(), ratio.data_ptr(), None, lrd.data_ptr(), state.data_ptr(), 0.0, 1, wd_.data_ptr(), s]
    for i, bad in ((0, None), (1, None), (2, None), (3, 0), (3, -1), (4, None), (5, None), (7, None), (8, None), (0, P[0] + 4), (1, P[1] + 8),
                   (11, wd_.data_ptr() + 2), (9, -0.5), (8, state.data_ptr() + 4)):
        a = list(aa)
        a[i] = bad
        rcs.append(app(*a))
    torch.cuda.synchronize()
    assert all(rc == -1 for rc in rcs), rcs
    for t, b in zip(watched, before):
        assert (bits_of(t) == b).all()
