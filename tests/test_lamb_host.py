"""lamb.py's host definitions (no GPU): host_lamb_step against a float64 restatement of its formulas, host_powi, the zero-norm rule, option
validation and the header's declarations.

The bound of test_host_step_is_the_float64_formulas_within_the_rounding_of_its_operations.  e = 2^-24 is the unit roundoff of float32: every
float32 operation returns its exact result times (1 + delta), |delta| <= e (the data keep every intermediate normal - asserted -, and the
square root obeys the same model).  Both sides use the SAME float32-rounded scalars (1 - beta, c1, c2, d, eps, grad_scale, coef, the ratio), so
only the element operations differ.  Following an error E_x = |x_f32 - x_f64| through the formulas, to first order:
  th1 = th - th d                   E_th1 = e (|th d| + |th1|)                              a product and a difference
  gg  = (g gs) cf                   E_g   = 2 e |gg|                                        two products; the clamp is exact
  m'  = m + (gg - m) om1            E_m   = om1 E_g + 2 e |b| + e |m'|,  b = (gg - m) om1   difference, product, sum
  v'  = v + (gg gg - v) om2         E_q   = 2 |gg| E_g + e gg^2 = 5 e gg^2
                                    E_v   = om2 E_q + 2 e |b2| + e |v'|, b2 = (gg^2 - v) om2
  mh  = m' / c1,  vh = v' / c2      E_mh  = E_m / c1 + e |mh|,  E_vh = E_v / c2 + e |vh|
  s   = sqrt(vh)                    E_s   = E_vh / sqrt(vh) + e s      (|sqrt(x + D) - sqrt(x)| = |D| / (sqrt(x + D) + sqrt(x)) <= |D| / sqrt(x);
                                                                        vh = 0 is exact on both sides)
  den = s + eps                     E_den = E_s + e den
  u   = mh / den                    E_u   = (E_mh + |u| E_den) / (den - E_den) + e |u|
  step = ratio lr                   one product: e |step|
  th' = th1 - step u                E_th  = E_th1 + |step| E_u + 2 e |step u| + e |th'|
Every count of roundings is below 32, so the neglected higher orders are below 32 e = 2^-19 of the first: the test allows (1 + 2^-10) times it.
The ratio: W and U are sums of squares, |W_f32 - W| <= sum of (2 |th1| E_th1 + E_th1^2) =: E_W (U alike; the float64 sums themselves add L * 2^-53),
and sqrt(W / U) moves by at most half the two relative errors, plus e for the rounding to float32."""
import os
import re

import numpy as np
import pytest

from resunet_a_mltsk_keras_amd import clip as CL
from resunet_a_mltsk_keras_amd import lamb as LB
from resunet_a_mltsk_keras_amd.engine import LossSpec
from resunet_a_mltsk_keras_amd.keras_api import Lamb

from _lamb_ref import E, SLACK, float64_step, worst

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64
SIZES = [("a/kernel", 1), ("b/bias", 3), ("c/kernel", 37), ("d/kernel", 16), ("d/kernel", 21), ("e/gamma", 5)]


def small_table():
    entries, off = [], 0
    for name, size in SIZES:
        entries.append(dict(name=name, off=off, size=size))
        off += (size + 15) // 16 * 16
    chunks, vars_, names = CL.build_chunk_table(entries, ("bias", "gamma"), chunk=16)
    return chunks, vars_, names, off


def small_inputs(n):
    rng = np.random.default_rng(5)
    g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 1, n)).astype(f32)
    m = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 0, n)).astype(f32)
    v = ((rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 0, n)) ** 2).astype(f32)
    th = rng.standard_normal(n).astype(f32)
    g[::7] = 0; m[::5] = 0; v[::5] = 0; th[::11] = 0
    return th, g, m, v


@pytest.mark.parametrize("t", [1, 2, 1000])
@pytest.mark.parametrize("opts", [dict(), dict(wd=0.05), dict(cv=0.5, gs=0.125), dict(wd=0.05, coefs=True, gs=0.125)])
def test_host_step_is_the_float64_formulas_within_the_rounding_of_its_operations(t, opts):
    chunks, vars_, names, n = small_table()
    th, g, m, v = small_inputs(n)
    wd, cv, gs = opts.get("wd", 0.0), opts.get("cv"), opts.get("gs", 1.0)
    coef = (np.linspace(0.3, 1.0, len(vars_)).astype(f32) if opts.get("coefs") else np.ones(len(vars_), f32))
    kw = dict(t=t, lr=1.2345e-3, lr_base=1e-3, beta_1=0.9, beta_2=0.999, eps=1e-7, grad_scale=gs, coef=coef, clipvalue=cv, weight_decay=wd)
    r = LB.host_lamb_step(th, g, m, v, chunks, vars_, **kw)
    for k in ("theta", "m", "v", "u", "th1"):
        assert r[k].dtype == f32
        nz = np.abs(r[k][r[k] != 0])
        assert nz.min() > 2.0 ** -100                                             # the relative error model holds: nothing near the subnormals
    ref = float64_step(th, g, m, v, chunks, vars_, t=t, lr=kw["lr"], lr_base=1e-3, b1=0.9, b2=0.999, eps=1e-7, gs=gs, coef=coef, cv=cv, wd=wd,
                       ratio=r["ratio"])
    inside = CL.covered(chunks, n) == 1
    ratios = {k: worst(np.abs(r[k].astype(f64) - ref[k])[inside], SLACK * ref[e][inside])
              for k, e in (("th1", "E_th1"), ("m", "E_m"), ("v", "E_v"), ("u", "E_u"), ("theta", "E_th"))}
    ok = (ref["W"] > 0) & (ref["U"] > 0)
    assert ok.sum() >= len(vars_) - 1 and (r["ratio"][~ok] == 1.0).all()            # a one-element variable may sit on a planted zero
    W, U = ref["W"][ok], ref["U"][ok]
    e_ratio = np.sqrt(W) / np.sqrt(U) * (0.5 * (ref["EW"][ok] / W + ref["EU"][ok] / U) + E)
    ratios["ratio"] = worst(np.abs(r["ratio"][ok].astype(f64) - np.sqrt(W) / np.sqrt(U)), SLACK * e_ratio)
    print(f"t={t} {opts}: worst error / bound " + " ".join(f"{k} {x:.3f}" for k, x in ratios.items()))
    assert all(x <= 1.0 for x in ratios.values()), ratios
    assert max(ratios.values()) > 0.01                                            # the bound is of the error's order, not a blanket
    assert (r["theta"][~inside] == th[~inside]).all() and (r["g"][inside] == 0).all() and (r["g"][~inside] == g[~inside]).all()
    assert (r["W"] == [sum(r["pw"][a:b].tolist()) for a, b in zip(vars_["chunk_begin"], vars_["chunk_end"])]).all()
    if wd:
        dec = np.zeros(n, bool)
        for off, ln, var in chunks.tolist():
            dec[off:off + ln] = bool(vars_["decay"][var])
        assert (r["th1"][inside & ~dec] == th[inside & ~dec]).all() and (r["th1"][inside & dec] != th[inside & dec]).any()
    if cv:
        assert np.abs(r["gg"]).max() == f32(cv)
    # the ratio handed in is the ratio applied
    r2 = LB.host_lamb_step(th, g, m, v, chunks, vars_, ratio=np.full(len(vars_), 2.0, f32), **kw)
    assert (r2["ratio"] == 2.0).all() and (r2["u"].view(np.uint32) == r["u"].view(np.uint32)).all() and (r2["theta"] != r["theta"]).any()


@pytest.mark.parametrize("beta", [0.9, 0.999, float(f32(0.9)), float(f32(0.999)), 0.98, 0.5, 0.0])
def test_powi_is_pow_within_two_ulp(beta):
    """host_powi carries a remainder next to the value, so its value is within one ulp of beta^t; the C library's pow is within one ulp too:
    two ulp between them at the most.  (10^6: both underflow to zero, where 1 - beta^t is 1.)"""
    for t in (1, 2, 3, 1000, 10 ** 6):
        h, p = LB.host_powi(beta, t), beta ** t
        ulps = abs(h - p) / np.spacing(p) if p > 0 else abs(h - p)
        print(f"beta={beta!r} t={t}: {ulps:.1f} ulp")
        assert ulps <= 2.0, (beta, t, h, p)
    assert LB.host_powi(beta, 0) == 1.0 and LB.host_powi(beta, 1) == beta
    with pytest.raises(ValueError):
        LB.host_powi(beta, -1)


def test_bias_corrections_are_float32_of_one_minus_the_power():
    c1, c2 = LB.bias_corrections(0.9, 0.999, 1)
    assert c1.dtype == f32 and c1 == f32(1.0 - float(f32(0.9))) and c2 == f32(1.0 - float(f32(0.999)))
    c1, c2 = LB.bias_corrections(0.9, 0.999, 10 ** 6)
    assert c1 == 1.0 and c2 == 1.0


def test_zero_and_nan_norms_give_ratio_one():
    chunks, vars_, names, n = small_table()
    th, g, m, v = small_inputs(n)
    th, g, m = th.copy(), g.copy(), m.copy()
    th[0], g[0] = 0.5, 0.3                                                            # a/kernel's one element sat on the planted zeros
    rows = {names[c["var"]]: (int(c["off"]), int(c["len"])) for c in chunks[::-1]}     # a variable's first chunk
    a, la = rows["b/bias"]
    th[a:a + la] = 0                                                                  # an all-zero variable
    b, lb = rows["e/gamma"]
    g[b:b + lb] = 0; m[b:b + lb] = 0                                                  # an all-zero update
    c, _ = rows["c/kernel"]
    g[c + 2] = np.nan                                                                 # a NaN sum
    r = LB.host_lamb_step(th, g, m, v, chunks, vars_, t=3, lr=1e-3)
    iv = {nm: k for k, nm in enumerate(names)}
    assert r["W"][iv["b/bias"]] == 0 and r["U"][iv["e/gamma"]] == 0 and np.isnan(r["U"][iv["c/kernel"]])
    for nm in ("b/bias", "e/gamma", "c/kernel"):
        assert r["ratio"][iv[nm]] == 1.0, nm
    for nm in ("a/kernel", "d/kernel"):
        assert r["ratio"][iv[nm]] != 1.0 and np.isfinite(r["ratio"][iv[nm]])
    rep = LB.host_ratio_report(r["W"], r["U"], updates=4)
    assert rep["forced"] == 3 and rep["updates"] == 4 and (rep["ratio"] == r["ratio"]).all()
    assert rep["min_ratio"] == r["ratio"].min() and rep["max_ratio"] == r["ratio"].max()
    sl = slice(c, c + 16)
    assert np.isnan(r["theta"][c + 2]) and np.isfinite(np.delete(r["theta"][sl], 2)).all()      # plain arithmetic on the NaN, nowhere else
    assert (LB.host_ratio([4.0, 0.0, np.nan, 1.0, np.inf], [1.0, 1.0, 1.0, 0.0, 1.0]) == f32([2.0, 1.0, 1.0, 1.0, np.inf])).all()


def test_option_validation():
    LB.check_options(0.0, 0.0, 1e-30)
    for kw in (dict(beta_1=1.0), dict(beta_1=-0.1), dict(beta_2=1.0), dict(beta_2=float("nan")), dict(epsilon=0.0), dict(epsilon=-1e-7),
               dict(epsilon=float("inf")), dict(epsilon=1e-60), dict(beta_1=True), dict(epsilon="1e-7")):
        with pytest.raises(ValueError):
            LB.check_options(**kw)
        with pytest.raises(ValueError):
            Lamb(**kw)
    o = Lamb()
    assert (o.kind, o.lr.value, o.beta_1, o.beta_2, o.epsilon) == ("lamb", 1e-3, 0.9, 0.999, 1e-7)
    o = Lamb(learning_rate=0.02, epsilon=1e-6, global_clipnorm=1.0, weight_decay=0.01, skip_nonfinite=True, use_ema=True, gradient_accumulation_steps=4)
    o.exclude_from_weight_decay(var_names=["bias"])
    assert o.epsilon == 1e-6 and o.clip_options()["global_clipnorm"] == 1.0 and o.clip_options()["decay_exclude"] == ["bias"]
    assert o.sched_options()["use_ema"] and o.accum_options() == dict(gradient_accumulation_steps=4)
    with pytest.raises(ValueError, match="only one"):
        Lamb(clipnorm=1.0, clipvalue=1.0)
    from resunet_a_mltsk_keras_amd.engine import Engine, ModelConfig
    eng = Engine(ModelConfig(input_shape=(64, 64, 3), num_classes=4), _layout_only=True)
    for kw in (dict(epsilon=0.0), dict(beta_1=1.0), dict(beta_2=-1.0)):
        with pytest.raises(ValueError):
            eng.compile(LossSpec(optimizer="lamb", **kw))
    with pytest.raises(ValueError):
        eng.compile(LossSpec(optimizer="lars"))
    import utils
    assert utils.Lamb is Lamb


def test_header_declares_the_three_entry_points():
    hdr = open(os.path.join(ROOT, "include", "rua_hip.h")).read()
    for name, nargs in (("rua_lamb_moments", 19), ("rua_lamb_finish", 10), ("rua_lamb_apply", 13)):
        mt = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert mt, name
        assert len(mt.group(1).split(",")) == nargs, name
        from resunet_a_mltsk_keras_amd import _lib as L
        assert len(L._SIGS[name][0]) == nargs
    assert "const int32_t* flag" in re.search(r"int\s+rua_lamb_apply\s*\(([^)]*)\)", hdr).group(1)
