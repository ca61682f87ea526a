"""Host definition of the LAMB optimizer (You et al. 2019; keras.optimizers.Lamb of Keras 3): what rua_lamb_moments, rua_lamb_finish and
rua_lamb_apply compute on the GPU (include/rua_hip.h, csrc/lamb.hip).  Pure numpy.

LAMB is Adam's direction with a per-VARIABLE step: ratio = ||w|| / ||u||, u the bias-corrected Adam direction of the variable - which is why
one rate carries across batch sizes.  A variable is one Keras name, as for clipnorm (clip.build_chunk_table).

host_lamb_step works in float32 with every operation rounded on its own, in the order the kernels use, so m', v', u and - given the same
ratio - theta' are the kernels' bits.  Per element of a chunk of variable var:
  th1 = decays(var) and wd != 0 ? th - th * d : th          d = float32(wd * lr_base)                    (as clip.host_clipped_step)
  gg  = clampv((g * grad_scale) * coef[var])                                                             (as clip.host_clipped_step)
  m'  = m + (gg - m) * (1 - beta1)                          Keras' form; (1 - beta1) is the float32 difference
  v'  = v + (gg * gg - v) * (1 - beta2)
  u   = (m' / c1) / (sqrt(v' / c2) + eps)                   c1 = float32(1 - beta1^t), c2 = float32(1 - beta2^t), beta^t = host_powi
per variable (float64; the squares of float32 values are exact there):
  W = sum of th1^2, U = sum of u^2                          one partial per chunk, the chunks of a variable added in order
  ratio = float32(sqrt(W) / sqrt(U)) if W > 0 and U > 0 else 1        a zero or NaN sum gives 1, as Keras' nested `where` does
and per element again:
  theta' = th1 - (ratio * lr) * u                           the step is ONE float32 product per variable
t is the update count after this step's increment (what the rate kernel leaves in lr_state[0]); lr the rate of this update - the base
rate, schedule applied: LAMB's bias correction sits in u, not in the rate."""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np

f32, f64 = np.float32, np.float64


def check_options(beta_1=0.9, beta_2=0.999, epsilon=1e-7) -> None:
    """0 <= beta < 1 and epsilon > 0 (finite numbers, not bools): ValueError otherwise.  Unlike Adam's, epsilon is a free kernel argument."""
    num = lambda x: not isinstance(x, bool) and isinstance(x, (int, float, np.integer, np.floating)) and np.isfinite(x)
    for k, b in (("beta_1", beta_1), ("beta_2", beta_2)):
        if not num(b) or not 0.0 <= b < 1.0:
            raise ValueError(f"{k}={b!r}: a number in [0, 1)")
    if not num(epsilon) or not epsilon > 0.0 or not f32(epsilon) > 0.0:
        raise ValueError(f"epsilon={epsilon!r}: a positive number (in float32)")


_SPLIT = 134217729.0                                         # 2^27 + 1: Veltkamp's splitter for float64


def _two_prod(a: float, b: float):
    """(p, e) with p = fl(a * b) and p + e = a * b exactly (Dekker): what fma(a, b, -p) gives the kernel."""
    p = a * b
    c = _SPLIT * a
    ah = c - (c - a)
    al = a - ah
    c = _SPLIT * b
    bh = c - (c - b)
    bl = b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _dd_mul(xh: float, xl: float, yh: float, yl: float):
    """The product of two (value, remainder) pairs, operation for operation lamb_dd_mul of csrc/lamb.hip."""
    p, e = _two_prod(xh, yh)
    e = e + (xh * yl + xl * yh)
    s = p + e
    return s, e - (s - p)


def host_powi(beta: float, t: int) -> float:
    """beta^t for an integer t >= 0 by binary exponentiation in a fixed order.  The kernel runs the same loop, so both sides hold the same
    bits and neither side's pow is involved.  Plain float64 products would lose about t / 4 ulp (a squaring doubles the error it inherits:
    37 .. 209 ulp at t = 1000), so the running power and the result are pairs of float64 (value, remainder) with exact product remainders:
    a pair is within about 2^-100 of exact per product, and the value returned is within one ulp of beta^t."""
    t = int(t)
    if t < 0:
        raise ValueError(f"t={t}: a non-negative integer")
    rh, rl, ph, pl = 1.0, 0.0, float(beta), 0.0
    while t > 0:
        if t & 1:
            rh, rl = _dd_mul(rh, rl, ph, pl)
        t >>= 1
        if t:
            ph, pl = _dd_mul(ph, pl, ph, pl)
    return rh


def bias_corrections(beta_1: float, beta_2: float, t: int):
    """(c1, c2) as float32, from the float32 betas the kernel receives."""
    return f32(1.0 - host_powi(float(f32(beta_1)), t)), f32(1.0 - host_powi(float(f32(beta_2)), t))


def host_ratio(W, U) -> np.ndarray:
    """float32 trust ratio per variable from the float64 sums; 1 where a sum is zero or NaN."""
    W, U = np.asarray(W, f64), np.asarray(U, f64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ok = (W > 0) & (U > 0)
        return np.where(ok, (np.sqrt(W) / np.sqrt(U)).astype(f32), f32(1.0)).astype(f32)


def host_ratio_report(W, U, updates: int = 1) -> Dict[str, object]:
    """What rua_lamb_finish leaves in its report after `updates` updates, the last of them with these sums: dict(min_ratio, max_ratio,
    forced - the variables whose ratio the zero / NaN rule set to 1 -, updates, ratio - the float32 array)."""
    W, U = np.asarray(W, f64), np.asarray(U, f64)
    r = host_ratio(W, U)
    with np.errstate(invalid="ignore"):
        forced = int((~((W > 0) & (U > 0))).sum())
        mn, mx = float(np.fmin.reduce(r, initial=np.inf)), float(np.fmax.reduce(r, initial=-np.inf))
    return dict(min_ratio=mn, max_ratio=mx, forced=forced, updates=int(updates), ratio=r)


def host_lamb_step(theta, g, m, v, chunks, vars_, *, t: int, lr: float, lr_base: Optional[float] = None, beta_1: float = 0.9, beta_2: float = 0.999,
                   eps: float = 1e-7, grad_scale: float = 1.0, coef: Optional[Sequence[float]] = None, clipvalue: Optional[float] = None,
                   weight_decay: float = 0.0, ratio: Optional[Sequence[float]] = None) -> Dict[str, object]:
    """One LAMB update over the chunk table in float32 (module docstring).  theta, g, m, v: flat arrays; coef: the clip finisher's float32
    coefficient per variable (None: ones); clipvalue: None or c > 0; lr_base: the rate the decay uses (default lr), a float64 as lr_state[1]
    is; ratio: None, or the per-variable ratios to apply instead of this function's own (a test hands over the device's).
    Returns dict(theta, m, v, u, th1, gg - flat float32, padding untouched -, g - zeroed inside the chunks -, pw, pu - float64 per chunk -,
    W, U - float64 per variable -, ratio - float32 per variable, the one applied -, c1, c2)."""
    th, gr, m1, v1 = (np.array(a, f32) for a in (theta, g, m, v))
    nv = len(vars_)
    cf = np.ones(nv, f32) if coef is None else np.asarray(coef, f32)
    b1, b2, e, gs = f32(beta_1), f32(beta_2), f32(eps), f32(grad_scale)
    om1, om2 = f32(1.0) - b1, f32(1.0) - b2
    c1, c2 = bias_corrections(b1, b2, t)
    wd = float(weight_decay or 0.0)
    d = f32(wd * float(lr if lr_base is None else lr_base))
    cv = f32(clipvalue) if clipvalue is not None and clipvalue > 0 else None
    th1_all, u_all, gg_all = th.copy(), np.zeros_like(th), np.zeros_like(th)
    pw, pu = np.zeros(len(chunks), f64), np.zeros(len(chunks), f64)
    W, U = np.zeros(nv, f64), np.zeros(nv, f64)
    rows = chunks.tolist()
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        for k, (off, ln, var) in enumerate(rows):
            sl = slice(off, off + ln)
            x = th[sl]
            if wd != 0.0 and vars_["decay"][var]:
                x = x - x * d
            gg = (gr[sl] * gs) * cf[var]
            if cv is not None:
                gg = np.where(gg < -cv, -cv, np.where(gg > cv, cv, gg)).astype(f32)
            mm = m1[sl] + (gg - m1[sl]) * om1
            vv = v1[sl] + (gg * gg - v1[sl]) * om2
            u = (mm / c1) / (np.sqrt(vv / c2) + e)
            assert x.dtype == gg.dtype == mm.dtype == vv.dtype == u.dtype == f32
            th1_all[sl], gg_all[sl], m1[sl], v1[sl], u_all[sl] = x, gg, mm, vv, u
            x64, u64 = x.astype(f64), u.astype(f64)
            pw[k], pu[k] = float(np.dot(x64, x64)), float(np.dot(u64, u64))
            W[var] = W[var] + pw[k]                         # chunks of a variable are adjacent and in order
            U[var] = U[var] + pu[k]
        r = host_ratio(W, U) if ratio is None else np.asarray(ratio, f32)
        lr32 = f32(lr)
        for off, ln, var in rows:
            sl = slice(off, off + ln)
            step = r[var] * lr32
            th[sl] = th1_all[sl] - step * u_all[sl]
            gr[sl] = 0.0
    return dict(theta=th, m=m1, v=v1, u=u_all, th1=th1_all, gg=gg_all, g=gr, pw=pw, pu=pu, W=W, U=U, ratio=r, c1=c1, c2=c2)
