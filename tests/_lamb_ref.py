"""What tests/test_lamb_host.py and tests/test_lamb_engine_gpu.py share: lamb.py's formulas restated plainly in float64, with the first-order bound of
the float32 rounding errors that tests/test_lamb_host.py derives in its docstring.  A plain module (no tests, no fixtures)."""
import numpy as np

from resunet_a_mltsk_keras_amd import lamb as LB

f32, f64 = np.float32, np.float64
E = 2.0 ** -24                                               # the unit roundoff of float32
SLACK = 1.0 + 2.0 ** -10                                     # the higher orders: every count of roundings is below 32, 32 E = 2^-19


def float64_step(th, g, m, v, chunks, vars_, *, t, lr, lr_base, b1, b2, eps, gs, coef, cv, wd, ratio):
    """The module docstring's formulas, plainly, in float64, with the float32-rounded scalars host_lamb_step uses; also the error bounds."""
    th, g, m, v = (np.asarray(a, f64) for a in (th, g, m, v))
    om1, om2 = f64(f32(1.0) - f32(b1)), f64(f32(1.0) - f32(b2))
    c1, c2 = (f64(c) for c in LB.bias_corrections(b1, b2, t))
    d, e_, gs_ = f64(f32(wd * lr_base)), f64(f32(eps)), f64(f32(gs))
    out = {k: np.zeros_like(th) for k in ("th1", "m", "v", "u", "theta", "E_th1", "E_m", "E_v", "E_u", "E_th")}
    out["theta"][:] = th
    W, U, EW, EU = (np.zeros(len(vars_), f64) for _ in range(4))
    for off, ln, var in chunks.tolist():
        sl = slice(off, off + ln)
        dec = bool(wd) and bool(vars_["decay"][var])
        th1 = th[sl] - th[sl] * d if dec else th[sl]
        E_th1 = E * (np.abs(th[sl] * d) + np.abs(th1)) if dec else np.zeros(ln)
        gg = (g[sl] * gs_) * f64(coef[var])
        if cv:
            gg = np.clip(gg, -cv, cv)
        E_g = 2 * E * np.abs(gg)
        b = (gg - m[sl]) * om1
        m1 = m[sl] + b
        E_m = om1 * E_g + 2 * E * np.abs(b) + E * np.abs(m1)
        b2_ = (gg * gg - v[sl]) * om2
        v1 = v[sl] + b2_
        E_v = om2 * 5 * E * gg * gg + 2 * E * np.abs(b2_) + E * np.abs(v1)
        mh, vh = m1 / c1, v1 / c2
        E_mh, E_vh = E_m / c1 + E * np.abs(mh), E_v / c2 + E * np.abs(vh)
        s = np.sqrt(vh)
        E_s = np.where(vh > 0, E_vh / np.where(vh > 0, s, 1.0), 0.0) + E * s
        den = s + e_
        E_den = E_s + E * den
        u = mh / den
        E_u = (E_mh + np.abs(u) * E_den) / (den - E_den) + E * np.abs(u)
        step = f64(ratio[var]) * f64(f32(lr))
        th2 = th1 - step * u
        E_th = E_th1 + abs(step) * E_u + 2 * E * np.abs(step * u) + E * np.abs(th2)
        for k, x in (("th1", th1), ("m", m1), ("v", v1), ("u", u), ("theta", th2), ("E_th1", E_th1), ("E_m", E_m), ("E_v", E_v), ("E_u", E_u), ("E_th", E_th)):
            out[k][sl] = x
        W[var] += np.dot(th1, th1); U[var] += np.dot(u, u)
        EW[var] += np.sum(2 * np.abs(th1) * E_th1 + E_th1 ** 2) + ln * 2.0 ** -53 * np.dot(th1, th1)
        EU[var] += np.sum(2 * np.abs(u) * E_u + E_u ** 2) + ln * 2.0 ** -53 * np.dot(u, u)
    out.update(W=W, U=U, EW=EW, EU=EU)
    return out


def worst(err, bound):
    err, bound = np.asarray(err, f64), np.asarray(bound, f64)
    return float(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf)).max())
