"""Gradient clipping, decoupled weight decay and the non-finite step skip through the C ABI: rua_grad_sumsq, rua_clip_finish, rua_adam_step_seg /
rua_sgd_step_seg and rua_state_copy against clip.py's float64 definitions.

The table has variables of 1, 3, 16, CHUNK - 1, CHUNK, CHUNK + 1 and 2 * CHUNK + 5 elements and one variable made of two entries; gradients span
fifteen decades as tests/test_tail_gpu.py's do.  Padding between the slices and 16 guard elements behind every buffer hold a sentinel that no
kernel may touch.

Sum of squares: the square of a float32 is exact in float64 and the terms are non-negative, so ANY summation order of L terms is within
L * 2^-53 (relative) of the exact sum - and so is numpy's float64 sum: the test allows L * 2^-53 between the two, the bound of ONE of them, as the
tightest statement that needs no knowledge of either order.  Two runs give identical bits.

The optimizers: test_tail_gpu.py's one-step bounds (u = 2^-23, a fresh state before every step), widened by what the new operations round:
  gradient  gg = clampv((g * gs) * coef): one more multiplication (one u), and the finisher's float32 coef may sit one ulp (one u) from the
            reference's, which is computed from numpy's sums: K = 2 more u on the gradient, so K on m', 2K on v' (gg squared), K on delta through
            sqrt(v') and through m'.  The clamp is exact.
  decay     th1 = th - th * d: two operations, one u each: E_dec = u |th d| + u |th1| (decaying variables only).
  Adam   |m' - m'_ref|   <= (4 + K) u (beta1 |m| + (1 - beta1) |gg|)                                          =: e_m
         |v' - v'_ref|   <= (4 + 2K) u v'_ref + 4 * 2^-149        (the absolute term: up to four roundings may land on the subnormal grid)
         |th' - th'_ref| <= u |th'_ref| + E_dec + (4e-6 + K u) |delta_ref| + lr_t e_m / (sqrt(v'_ref) + eps)
  SGD    |vel' - vel'_ref| <= (4 + K) u (mu |vel| + |lr gg|)                                                  =: e_v
         |th' - th'_ref|   <= u |th'_ref| + E_dec + e_v
Every test prints the worst observed ratio to its bound (pytest -s shows them)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from _kernel_util import U32, bits_of, dev, frozen, stream, up, worst_ratio  # noqa: E402
from resunet_a_mltsk_keras_amd import _lib as L  # noqa: E402
from resunet_a_mltsk_keras_amd import clip as CL  # noqa: E402

f32, f64 = np.float32, np.float64
CH = CL.OPT_CHUNK
B1, B2, EPS, MU = f32(0.9), f32(0.999), f32(1e-7), f32(0.8)
LR_ADAM, LR_SGD, LR_BASE = f32(1.2345e-3), f32(0.1), 1e-3
WD = 0.05
K = 2
GUARD = 16
SENT = f32(7.25)                                             # padding and guards of the float buffers
SENT_BITS = 0x5A5A                                           # ... of the bf16 copy
SIZES = [("a/kernel", 1), ("b/bias", 3), ("c/gamma", 16), ("d/kernel", CH - 1), ("e/kernel", CH), ("f/beta", CH + 1), ("g/kernel", 2 * CH + 5),
         ("h/kernel", 40), ("h/kernel", CH + 7), ("h/bias", 5)]
EXCLUDE = ("bias", "gamma", "beta")
MODES = ["none", "global", "norm", "value"]


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
    """Seeded state as test_tail_gpu.tail_inputs draws it, the sentinel on the padding and the guards."""
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


def raw_table(a):
    return torch.from_numpy(np.frombuffer(a.tobytes(), dtype=np.uint8).copy()).to(dev())


def wcopy_buffer(th, out):
    w = torch.from_numpy(np.array(th)).to(torch.bfloat16).view(torch.int16).clone()
    w[torch.from_numpy(out.copy())] = SENT_BITS
    return w.to(dev())


def ptr(t):
    return t.data_ptr() if t is not None else None


def run_sumsq(gd, chunks_d, vars_d, n_chunks, n_vars, mode, c, gs, skip, report=None):
    partials = up(np.full(n_chunks, -1.0, f64))
    var_ss, coef = up(np.full(n_vars, -1.0, f64)), up(np.full(n_vars, -1.0, f32))
    flag = up(np.full(4, 9, np.int32))
    report = up(np.zeros(4, f64)) if report is None else report
    L.lib().call("rua_grad_sumsq", gd.data_ptr(), chunks_d.data_ptr(), n_chunks, partials.data_ptr(), stream())
    L.lib().call("rua_clip_finish", partials.data_ptr(), n_chunks, vars_d.data_ptr(), n_vars, mode, float(c), float(gs), int(skip), var_ss.data_ptr(), coef.data_ptr(),
                 flag.data_ptr(), report.data_ptr(), stream())
    return partials, var_ss, coef, flag, report


def mode_args(mode, g, gs):
    """(C mode, c, host keyword) of a mode name; the norms come from the host's float64 sums of THIS gradient."""
    chunks, vars_, inside, names, n = table()
    per, total = CL.host_sumsq(g[:n], chunks, vars_)
    if mode == "global":
        c = 0.37 * gs * np.sqrt(total)
        return CL.CLIP_GLOBAL_NORM, c, dict(global_clipnorm=c)
    if mode == "norm":
        c = float(np.median(gs * np.sqrt(per)))              # variables on both sides of it
        return CL.CLIP_NORM, c, dict(clipnorm=c)
    if mode == "value":
        return CL.CLIP_VALUE, 1.0, dict(clipvalue=1.0)
    return CL.CLIP_NONE, 0.0, {}


def run_step(opt, g, mode, c, wd, gs, wc, skip=False, th=None):
    """sum of squares -> finisher -> segmented optimizer on fresh device copies of inputs() (g, th replaced where given)."""
    chunks, vars_, inside, names, n = table()
    th0, _, m0, v0, out = inputs()
    th0 = th0 if th is None else th
    thd, gd, md, vd = up(th0), up(g), up(m0), up(v0)
    wd_ = wcopy_buffer(th0, out) if wc else None
    chunks_d, vars_d = raw_table(chunks), raw_table(vars_)
    lrd = up(np.array([LR_ADAM if opt == "adam" else LR_SGD], f32))
    state = up(np.array([4.0, LR_BASE], f64))
    partials, var_ss, coef, flag, report = run_sumsq(gd, chunks_d, vars_d, len(chunks), len(vars_), mode, c, gs, skip)
    fl = flag.data_ptr() if skip else None
    cv = float(c) if mode == CL.CLIP_VALUE else 0.0
    if opt == "adam":
        L.lib().call("rua_adam_step_seg", thd.data_ptr(), gd.data_ptr(), md.data_ptr(), vd.data_ptr(), chunks_d.data_ptr(), len(chunks), vars_d.data_ptr(),
                     coef.data_ptr(), fl, lrd.data_ptr(), state.data_ptr(), float(B1), float(B2), float(EPS), gs, cv, float(wd), 1, ptr(wd_), stream())
    else:
        L.lib().call("rua_sgd_step_seg", thd.data_ptr(), gd.data_ptr(), md.data_ptr(), chunks_d.data_ptr(), len(chunks), vars_d.data_ptr(),
                     coef.data_ptr(), fl, lrd.data_ptr(), state.data_ptr(), float(MU), gs, cv, float(wd), 1, ptr(wd_), stream())
    torch.cuda.synchronize()
    return dict(th=thd, g=gd, m=md, v=vd, w=wd_, coef=coef, var_ss=var_ss, flag=flag, report=report, partials=partials)


def value_gradient(gs):
    """inputs()' gradient with elements whose g * gs is exactly +1, -1 (the clip value), just inside and well outside."""
    chunks, vars_, inside, names, n = table()
    g = inputs()[1].copy()
    idx = np.flatnonzero(inside)[::97]
    vals = np.array([1.0, -1.0, np.nextafter(f32(1), f32(0)), -np.nextafter(f32(1), f32(0)), 3.5, -1e3], f32) / f32(gs)   # gs a power of two: exact
    g[idx] = np.resize(vals, idx.size)
    return g


def check_untouched(r, wc):
    th0, g0, m0, v0, out = inputs()
    for name, a in (("th", th0), ("g", g0), ("m", m0), ("v", v0)):
        assert (bits_of(r[name])[out] == a.view(np.uint32)[out]).all(), name
    if wc:
        assert (bits_of(r["w"].view(torch.bfloat16))[out] == SENT_BITS).all()


# ---- sum of squares and the coefficient ---------------------------------------------------------------------------------------------------
def test_sumsq_matches_float64_and_repeats_bit_for_bit():
    chunks, vars_, inside, names, n = table()
    g = inputs()[1]
    gd, chunks_d, vars_d = up(g), raw_table(chunks), raw_table(vars_)
    a = run_sumsq(gd, chunks_d, vars_d, len(chunks), len(vars_), CL.CLIP_NONE, 0.0, 1.0, 0)
    b = run_sumsq(gd, chunks_d, vars_d, len(chunks), len(vars_), CL.CLIP_NONE, 0.0, 1.0, 0)
    torch.cuda.synchronize()
    for x, y in zip(a[:2], b[:2]):
        assert (bits_of(x) == bits_of(y)).all()
    per, total = CL.host_sumsq(g[:n], chunks, vars_)
    got = a[1].cpu().numpy()
    sizes = np.array([sum(int(c["len"]) for c in chunks[v["chunk_begin"]:v["chunk_end"]]) for v in vars_])
    assert names[7] == "h/kernel" and sizes[7] == 40 + CH + 7                     # the two-entry variable is one
    worst = worst_ratio(np.abs(got - per), sizes * 2.0 ** -53 * per)
    norm = a[4].cpu().numpy()[0]
    L_all = int(sizes.sum())
    r_tot = abs(norm ** 2 - total) / (total * (L_all + 4) * 2.0 ** -53)            # norm = sqrt(total), squared again: two more roundings each way
    print(f"sum of squares: worst per-variable ratio to L * 2^-53: {worst:.3f}; total: {r_tot:.3f}")
    assert worst <= 1.0 and r_tot <= 1.0
    pc = a[0].cpu().numpy()
    for k, (off, ln, _) in enumerate(chunks.tolist()):
        x = g[off:off + ln].astype(f64)
        assert abs(pc[k] - np.dot(x, x)) <= ln * 2.0 ** -53 * np.dot(x, x), k
    assert (bits_of(gd) == g.view(np.uint32)).all()                                # read only


def coef_ulps(got, exp):
    exp = np.asarray(exp, f32)
    return float(np.max(np.abs(got.astype(f64) - exp.astype(f64)) / np.spacing(exp).astype(f64)))


@pytest.mark.parametrize("gs", [1.0, 0.125])
def test_global_coefficient_below_at_above_and_zero(gs):
    chunks, vars_, inside, names, n = table()
    g = inputs()[1]
    gd, chunks_d, vars_d = up(g), raw_table(chunks), raw_table(vars_)
    _, total = CL.host_sumsq(g[:n], chunks, vars_)
    norm = gs * np.sqrt(total)
    for c, one in ((2.0 * norm, True), (0.5 * norm, False), (1e-3 * norm, False)):
        _, _, coef, flag, report = run_sumsq(gd, chunks_d, vars_d, len(chunks), len(vars_), CL.CLIP_GLOBAL_NORM, c, gs, 0)
        got, rep = coef.cpu().numpy(), report.cpu().numpy()
        exp = f32(c / max(norm, c))
        ulps = coef_ulps(got, np.full(len(vars_), exp))
        print(f"global coefficient gs={gs} c/norm={c / norm:g}: {ulps:.2f} ulp")
        assert ulps <= 1.0 and (got == got[0]).all()
        if one:
            assert (got == 1.0).all() and rep[1] == 1.0 and rep[3] == 0
        else:
            assert rep[1] == got[0] and rep[3] == 1
        assert abs(rep[0] - norm) <= 1e-12 * norm and flag.cpu().numpy()[0] == 0
    # norm exactly c: a gradient with one non-zero element, 3.0, so that sqrt(9) * gs is exact; and the zero gradient
    g1 = np.where(inputs()[4], SENT, f32(0)).astype(f32)
    for val in (3.0, 0.0):
        g1[int(chunks[3]["off"]) + 5] = val
        _, _, coef, _, report = run_sumsq(up(g1), chunks_d, vars_d, len(chunks), len(vars_), CL.CLIP_GLOBAL_NORM, 3.0 * gs if val else 0.7, gs, 0)
        assert (coef.cpu().numpy() == 1.0).all() and report.cpu().numpy()[0] == val * gs and report.cpu().numpy()[3] == 0


def test_per_variable_coefficient_and_the_two_entry_variable():
    chunks, vars_, inside, names, n = table()
    g = inputs()[1]
    gd, chunks_d, vars_d = up(g), raw_table(chunks), raw_table(vars_)
    per, _ = CL.host_sumsq(g[:n], chunks, vars_)
    norms = np.sqrt(per)
    c = float(np.median(norms))
    assert (norms > c).any() and (norms < c).any()
    _, _, coef, _, report = run_sumsq(gd, chunks_d, vars_d, len(chunks), len(vars_), CL.CLIP_NORM, c, 1.0, 0)
    got = coef.cpu().numpy()
    assert len(got) == len(names) == len(SIZES) - 1                               # h/kernel's two entries: one coefficient
    exp = (c / np.maximum(norms, c)).astype(f32)
    ulps = coef_ulps(got, exp)
    print(f"per-variable coefficient: {ulps:.2f} ulp")
    assert ulps <= 1.0 and (got[norms <= c] == 1.0).all() and (got[norms > c * (1 + 1e-6)] < 1.0).all()
    assert report.cpu().numpy()[1] == got.min() and report.cpu().numpy()[3] == 1


@pytest.mark.parametrize("layout", ["a variable across the tile edge", "more variables than a tile"])
def test_finisher_adds_in_chunk_order_beyond_one_tile(layout):
    """The finisher stages partials (and the variables' sums) through LDS 4096 at a time: with more of them than that, every variable's sum and
    the total are still the bits of a serial loop in chunk / variable order."""
    TILE = 4096
    if layout == "a variable across the tile edge":
        ranges = [(0, 10), (10, TILE + 104), (TILE + 104, TILE + 105), (TILE + 105, 2 * TILE + 300)]
    else:
        ranges = [(k, k + 1) for k in range(TILE + 37)]
    nc, nv = ranges[-1][1], len(ranges)
    rng = np.random.default_rng(nc)
    part = (rng.standard_normal(nc) ** 2 * 10.0 ** rng.uniform(-20, 6, nc)).astype(f64)
    vars_ = np.array([(a, b, 1, 0) for a, b in ranges], dtype=CL.VAR_DTYPE)
    partials, vars_d = up(part), raw_table(vars_)
    var_ss, coef, flag, report = up(np.full(nv, -1.0, f64)), up(np.full(nv, -1.0, f32)), up(np.full(4, 9, np.int32)), up(np.zeros(4, f64))
    c = 1e-3
    L.lib().call("rua_clip_finish", partials.data_ptr(), nc, vars_d.data_ptr(), nv, CL.CLIP_NORM, c, 1.0, 1, var_ss.data_ptr(), coef.data_ptr(), flag.data_ptr(),
                 report.data_ptr(), stream())
    torch.cuda.synchronize()
    exp, total = np.zeros(nv, f64), 0.0
    for v, (a, b) in enumerate(ranges):
        acc = 0.0
        for x in part[a:b].tolist():
            acc += x
        exp[v] = acc
        total += acc
    assert (bits_of(var_ss) == exp.view(np.uint64)).all()
    rep = report.cpu().numpy()
    assert abs(rep[0] - np.sqrt(total)) <= np.spacing(np.sqrt(total)) and flag.cpu().numpy()[0] == 0
    want = (c / np.maximum(np.sqrt(exp), c)).astype(f32)
    got = coef.cpu().numpy()
    assert coef_ulps(got, want) <= 1.0 and rep[1] == got.min() and (got < 1).any()


# ---- the segmented optimizers ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gs,wc", [(1.0, True), (0.125, False), (0.125, True), (1.0, False)])
@pytest.mark.parametrize("decay", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("opt", ["adam", "sgd"])
def test_segmented_step_against_the_host_definition(opt, mode, decay, gs, wc):
    chunks, vars_, inside, names, n = table()
    th0, g0, m0, v0, out = inputs()
    g = value_gradient(gs) if mode == "value" else g0
    cmode, c, kw = mode_args(mode, g, gs)
    wd = WD if decay else 0.0
    lr = f64(LR_ADAM if opt == "adam" else LR_SGD)
    ref = CL.host_clipped_step(th0[:n], g[:n], m0[:n], v0[:n], chunks, vars_, optimizer=opt, lr=lr, lr_base=LR_BASE, beta_1=f64(B1), beta_2=f64(B2),
                               eps=f64(EPS), momentum=f64(MU), grad_scale=f64(f32(gs)), weight_decay=wd, **kw)
    r = run_step(opt, g, cmode, c, wd, gs, wc)
    ins = np.flatnonzero(inside)
    th64, gg, th1 = th0[:n].astype(f64)[ins], ref["gg"][ins], ref["th1"][ins]
    d = f64(f32(wd * LR_BASE))
    decays = np.zeros(n, bool)
    for off, ln, var in chunks.tolist():
        decays[off:off + ln] = bool(wd) and bool(vars_["decay"][var])
    e_dec = np.where(decays[ins], U32 * np.abs(th64 * d) + U32 * np.abs(th1), 0.0)
    got_th, got_m = r["th"].cpu().numpy()[:n][ins].astype(f64), r["m"].cpu().numpy()[:n][ins].astype(f64)
    if opt == "adam":
        m1, v1 = ref["m"][ins], ref["v"][ins]
        den = np.sqrt(v1) + f64(EPS)
        delta = lr * m1 / den
        e_m = (4 + K) * U32 * (f64(B1) * np.abs(m0[:n][ins].astype(f64)) + (1 - f64(B1)) * np.abs(gg))
        e_v = (4 + 2 * K) * U32 * v1 + 4 * 2.0 ** -149
        e_th = U32 * np.abs(ref["theta"][ins]) + e_dec + (4e-6 + K * U32) * np.abs(delta) + lr * e_m / den
        got_v = r["v"].cpu().numpy()[:n][ins].astype(f64)
        ratios = dict(m=worst_ratio(np.abs(got_m - m1), e_m), v=worst_ratio(np.abs(got_v - v1), e_v),
                      theta=worst_ratio(np.abs(got_th - ref["theta"][ins]), e_th))
    else:
        vel1 = ref["m"][ins]
        e_v = (4 + K) * U32 * (f64(MU) * np.abs(m0[:n][ins].astype(f64)) + np.abs(lr * gg))
        e_th = U32 * np.abs(ref["theta"][ins]) + e_dec + e_v
        ratios = dict(vel=worst_ratio(np.abs(got_m - vel1), e_v), theta=worst_ratio(np.abs(got_th - ref["theta"][ins]), e_th))
        assert (bits_of(r["v"]) == v0.view(np.uint32)).all()                      # SGD has no second moment: never touched
    print(f"{opt} mode={mode} decay={decay} gs={gs} wcopy={wc}: worst ratio to the bound " + " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), ratios
    if decay:
        assert decays.any() and not decays[inside].all()
        assert np.abs(th1 - th64)[decays[ins]].max() > 0                          # the decay did act
    assert (bits_of(r["g"])[:n][inside] == 0).all()                              # the gradient: +0 inside every chunk
    check_untouched(r, wc)
    if wc:
        w = bits_of(r["w"].view(torch.bfloat16))[:n][inside]
        assert (w == bits_of(r["th"].cpu()[:n][torch.from_numpy(inside.copy())].to(torch.bfloat16))).all()
    if mode == "value":
        # the planted elements: g * gs exactly +-c (they pass as they are), one ulp inside, and beyond (they leave as exactly +-c) - all under the bound above
        idx = np.flatnonzero(inside)[::97]
        at = np.abs(ref["gg"][idx]) == 1.0
        assert at.sum() >= idx.size // 2 and np.abs(ref["gg"][:n]).max() == 1.0


@pytest.mark.parametrize("opt", ["adam", "sgd"])
def test_undecayed_variables_match_the_run_without_decay_bit_for_bit(opt):
    chunks, vars_, inside, names, n = table()
    g = inputs()[1]
    cmode, c, _ = mode_args("global", g, 1.0)
    a, b = run_step(opt, g, cmode, c, WD, 1.0, True), run_step(opt, g, cmode, c, 0.0, 1.0, True)
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


# ---- the skip -------------------------------------------------------------------------------------------------------------------------------
def poison_positions():
    chunks = table()[0]
    big = [k for k in range(len(chunks)) if chunks[k]["len"] == CH][0]
    ragged = [k for k in range(len(chunks)) if chunks[k]["len"] % 4 == 3 and chunks[k]["len"] > 4][0]
    return {"first of a chunk": int(chunks[big]["off"]), "last of a chunk": int(chunks[big]["off"]) + CH - 1,
            "ragged tail": int(chunks[ragged]["off"] + chunks[ragged]["len"]) - 1}


@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan])
@pytest.mark.parametrize("where", ["first of a chunk", "last of a chunk", "ragged tail"])
@pytest.mark.parametrize("opt,mode", [("adam", "global"), ("sgd", "none"), ("adam", "value")])
def test_nonfinite_gradient_skips_the_step(opt, mode, where, bad):
    chunks, vars_, inside, names, n = table()
    th0, g0, m0, v0, out = inputs()
    cmode, c, _ = mode_args(mode, g0, 1.0)
    g = g0.copy()
    g[poison_positions()[where]] = bad
    r = run_step(opt, g, cmode, c, WD, 1.0, True, skip=True)
    for k, a in (("th", th0), ("m", m0), ("v", v0)):
        assert (bits_of(r[k]) == a.view(np.uint32)).all(), k
    assert (bits_of(r["g"])[:n][inside] == 0).all()
    check_untouched(r, True)
    w = bits_of(r["w"].view(torch.bfloat16))[:n][inside]
    assert (w == bits_of(torch.from_numpy(th0[:n][inside]).to(torch.bfloat16))).all()
    rep = r["report"].cpu().numpy()
    assert r["flag"].cpu().numpy()[0] == 1 and rep[2] == 1 and rep[3] == 0
    # the BatchNorm state: the backup comes back bit for bit over a poisoned S
    rng = np.random.default_rng(3)
    s_before = rng.standard_normal(83).astype(f32)
    backup, S = up(np.zeros(83, f32)), up(s_before)
    L.lib().call("rua_state_copy", backup.data_ptr(), S.data_ptr(), 83, None, stream())
    S.fill_(float("nan"))
    L.lib().call("rua_state_copy", S.data_ptr(), backup.data_ptr(), 83, r["flag"].data_ptr(), stream())
    torch.cuda.synchronize()
    assert (bits_of(S) == s_before.view(np.uint32)).all()


def test_finite_gradient_with_the_flag_armed_steps_and_leaves_the_state_alone():
    chunks, vars_, inside, names, n = table()
    g0 = inputs()[1]
    cmode, c, _ = mode_args("global", g0, 1.0)
    a, b = run_step("adam", g0, cmode, c, WD, 1.0, True, skip=True), run_step("adam", g0, cmode, c, WD, 1.0, True, skip=False)
    for k in ("th", "m", "v", "g"):
        assert (bits_of(a[k]) == bits_of(b[k])).all(), k
    assert a["flag"].cpu().numpy()[0] == 0 and a["report"].cpu().numpy()[2] == 0
    assert (bits_of(a["th"]) != inputs()[0].view(np.uint32)).any()
    s_now = np.arange(40, dtype=f32)
    S, backup = up(s_now), up(np.full(40, -1.0, f32))
    L.lib().call("rua_state_copy", S.data_ptr(), backup.data_ptr(), 40, a["flag"].data_ptr(), stream())
    torch.cuda.synchronize()
    assert (bits_of(S) == s_now.view(np.uint32)).all()
    # without skip_nonfinite a non-finite sum raises no flag
    g = g0.copy()
    g[0] = np.inf
    r = run_sumsq(up(g), raw_table(chunks), raw_table(vars_), len(chunks), len(vars_), CL.CLIP_NONE, 0.0, 1.0, 0)
    assert r[3].cpu().numpy()[0] == 0 and r[4].cpu().numpy()[2] == 0 and np.isinf(r[4].cpu().numpy()[0])


def test_skipped_and_clipped_counts_accumulate_in_the_report():
    chunks, vars_, inside, names, n = table()
    g0 = inputs()[1]
    cmode, c, _ = mode_args("global", g0, 1.0)
    chunks_d, vars_d = raw_table(chunks), raw_table(vars_)
    bad = g0.copy()
    bad[5 * 16] = np.nan
    report = up(np.zeros(4, f64))
    for g in (g0, bad, g0, bad, bad):
        run_sumsq(up(g), chunks_d, vars_d, len(chunks), len(vars_), cmode, c, 1.0, 1, report=report)
    rep = report.cpu().numpy()
    assert rep[2] == 3 and rep[3] == 2 and np.isnan(rep[0])


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_nothing_is_written():
    chunks, vars_, inside, names, n = table()
    th0, g0, m0, v0, out = inputs()
    bufs = [up(a) for a in (th0, g0, m0, v0)]
    wd_ = wcopy_buffer(th0, out)
    chunks_d, vars_d = raw_table(chunks), raw_table(vars_)
    nc, nv = len(chunks), len(vars_)
    partials, var_ss, coef = up(np.full(nc, -1.0, f64)), up(np.full(nv, -1.0, f64)), up(np.full(nv, 1.0, f32))
    flag, report = up(np.zeros(4, np.int32)), up(np.full(4, -2.0, f64))
    lrd, state = up(np.array([LR_ADAM], f32)), up(np.array([4.0, LR_BASE], f64))
    watched = bufs + [wd_.view(torch.bfloat16), partials, var_ss, coef, report]
    before = [bits_of(t) for t in watched]
    lib, s = L.lib(), stream()
    P = [t.data_ptr() for t in bufs]
    sumsq, fin, adam, sgd, cp = (lib.raw(k) for k in ("rua_grad_sumsq", "rua_clip_finish", "rua_adam_step_seg", "rua_sgd_step_seg", "rua_state_copy"))
    rcs = [sumsq(None, chunks_d.data_ptr(), nc, partials.data_ptr(), s), sumsq(P[1], None, nc, partials.data_ptr(), s),
           sumsq(P[1], chunks_d.data_ptr(), nc, None, s), sumsq(P[1], chunks_d.data_ptr(), 0, partials.data_ptr(), s),
           sumsq(P[1], chunks_d.data_ptr(), -3, partials.data_ptr(), s), sumsq(P[1] + 4, chunks_d.data_ptr(), nc, partials.data_ptr(), s)]
    fa = [partials.data_ptr(), nc, vars_d.data_ptr(), nv, CL.CLIP_GLOBAL_NORM, 1.0, 1.0, 0, var_ss.data_ptr(), coef.data_ptr(), flag.data_ptr(), report.data_ptr(), s]
    for i, bad in ((0, None), (1, 0), (1, -2), (2, None), (3, 0), (4, 7), (5, 0.0), (5, -1.0), (8, None), (9, None), (10, None), (11, None),
                   (0, partials.data_ptr() + 4)):
        a = list(fa)
        a[i] = bad
        rcs.append(fin(*a))
    aa = [P[0], P[1], P[2], P[3], chunks_d.data_ptr(), nc, vars_d.data_ptr(), coef.data_ptr(), None, lrd.data_ptr(), state.data_ptr(), float(B1), float(B2),
          float(EPS), 1.0, 0.0, 0.0, 1, wd_.data_ptr(), s]
    for i, bad in ((0, None), (1, None), (2, None), (3, None), (4, None), (5, 0), (5, -1), (6, None), (7, None), (9, None), (10, None),
                   (0, P[0] + 4), (1, P[1] + 8), (2, P[2] + 4), (3, P[3] + 12), (18, wd_.data_ptr() + 2), (16, -0.5)):
        a = list(aa)
        a[i] = bad
        rcs.append(adam(*a))
    sa = [P[0], P[1], P[2], chunks_d.data_ptr(), nc, vars_d.data_ptr(), coef.data_ptr(), None, lrd.data_ptr(), state.data_ptr(), float(MU), 1.0, 0.0, 0.0, 1,
          wd_.data_ptr(), s]
    for i, bad in ((0, None), (1, None), (2, None), (3, None), (4, 0), (5, None), (6, None), (8, None), (9, None), (0, P[0] + 4), (15, wd_.data_ptr() + 2)):
        a = list(sa)
        a[i] = bad
        rcs.append(sgd(*a))
    rcs += [cp(None, P[1], 16, None, s), cp(P[0], None, 16, None, s), cp(P[0], P[1], 0, None, s), cp(P[0] + 4, P[1], 16, None, s)]
    torch.cuda.synchronize()
    assert all(rc != 0 for rc in rcs), rcs
    for t, b in zip(watched, before):
        assert (bits_of(t) == b).all()
