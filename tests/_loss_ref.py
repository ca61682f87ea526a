"""Float64 numpy references of the loss chain of csrc/loss_optim.hip: the Tanimoto moments, the finalizer that turns them into the loss and the
gradient coefficients, the fold of replicated moments, the segmentation counts, the plain per-pixel losses and the gradient with respect to the
logits.  No GPU and no torch: tests/test_loss_ref_host.py checks these against the oracle, tests/test_loss_chain_gpu.py checks the kernels against
these.  A plain module (no tests, no fixtures).

Layouts are the kernels': p, y [B][HW][C] (or [M][C]), keep [B][HW] (or [M]) True where a pixel counts, sums [B][C][6], coef [B][C][3]."""
import types

import numpy as np

f32, f64 = np.float32, np.float64
TANIMOTO, WCE, CE_LOGITS, BCE_LOGITS, MSE = 0, 1, 2, 3, 4      # RUA_LOSS_* of include/rua_hip.h
ACT_NONE, ACT_SOFTMAX, ACT_SIGMOID = 0, 1, 2
SMOOTH = 1e-5
EPS32 = f32(1e-7)                                             # Keras' epsilon as the kernels hold it, and 1 - epsilon in float32
ONE_M_EPS32 = f32(1) - EPS32


def moments(p, y, keep):
    """sums[n][c] = {sum p, sum (1-l), sum p l, sum p^2 + l^2, sum (1-p)(1-l), sum (1-p)^2 + (1-l)^2} over the pixels of `keep`; what p and y hold
    elsewhere (NaN included) does not matter."""
    K = np.asarray(keep, bool)[:, :, None]
    P, Y = np.where(K, np.asarray(p, f64), 0.0), np.where(K, np.asarray(y, f64), 0.0)
    Q, M_ = np.where(K, 1.0 - P, 0.0), np.where(K, 1.0 - Y, 0.0)
    return np.stack([P.sum(1), M_.sum(1), (P * Y).sum(1), (P * P + Y * Y).sum(1), (Q * M_).sum(1), (Q * Q + M_ * M_).sum(1)], axis=-1)


def weight_is_infinite(V):
    """The reference's rule (multitasking_utils.py:46-53 runs in float32): reciprocal(V ** 2) is inf when the float32 square is too small, not only
    at V == 0."""
    v = np.asarray(V, f64).astype(f32)
    with np.errstate(divide="ignore", over="ignore", under="ignore"):
        return ~np.isfinite(f32(1) / (v * v))


def class_weights(V):
    """(w [C] float64, replaced [C] bool): 1 / V^2 in float64 where the float32 rule leaves it finite, the largest of those elsewhere (0 if none)."""
    V = np.asarray(V, f64)
    inf = weight_is_infinite(V)
    w = np.zeros_like(V)
    w[~inf] = 1.0 / (V[~inf] * V[~inf])
    w[inf] = w[~inf].max() if (~inf).any() else 0.0
    return w, inf


def finalize(sums, B, C, grad_scale, single=False):
    """Tanimoto_dual_loss (multitasking_utils.py:71-85) from the moments.  Returns a namespace:
      loss        mean over the samples of per_sample
      per_sample  [B]: 1 - (F1 / E1 + F2 / E2) / 2; single: F1 / E1, Tanimoto_loss itself with the class weights from column 0
      coef        [B][C][3] (None if single): d(grad_scale * sum_n per_sample[n]) / dp[n][i][c] = coef[n][c][0] + coef[n][c][1] p + coef[n][c][2] y
      coef_mag    the same sums with every term's absolute value (what a rounding error of the evaluation scales with)
      w1, w2, replaced1, replaced2
    The sums over the samples and over the classes run in index order, as the kernel's do, so a float64 evaluation of the same expressions agrees
    to a few ulps.  The first term's weights come from the prediction volumes and carry gradient, except for a replaced class: its weight is a
    copy of another class's, and the rule gives it none."""
    s = np.asarray(sums, f64).reshape(B, C, 6)
    V1, V2 = np.zeros(C), np.zeros(C)
    for n in range(B):
        V1 += s[n, :, 0]
        V2 += s[n, :, 1]
    V1, V2 = V1 / B, V2 / B
    w1, r1 = class_weights(V1)
    w2, r2 = class_weights(V2)
    N1, D1, N2, D2 = np.zeros(B), np.zeros(B), np.zeros(B), np.zeros(B)
    for c in range(C):
        N1 += w1[c] * s[:, c, 2]
        D1 += w1[c] * (s[:, c, 3] - s[:, c, 2])
        N2 += w2[c] * s[:, c, 4]
        D2 += w2[c] * (s[:, c, 5] - s[:, c, 4])
    E1, F1, E2, F2 = D1 + SMOOTH, N1 + SMOOTH, D2 + SMOOTH, N2 + SMOOTH
    per = F1 / E1 if single else 1.0 - 0.5 * (F1 / E1 + F2 / E2)
    out = types.SimpleNamespace(loss=float(per.sum() / B), per_sample=per, coef=None, coef_mag=None, w1=w1, w2=w2, replaced1=r1, replaced2=r2)
    if single:
        return out
    # d(F1 / E1)[n] / d w1_c = (Spl E1 - F1 (SS - Spl)) / E1^2, summed over n; d w1_c / dp = -2 / (V1_c^3 B) for every pixel of class c
    R, Rm = np.zeros(C), np.zeros(C)
    for n in range(B):
        R += (s[n, :, 2] * E1[n] - F1[n] * (s[n, :, 3] - s[n, :, 2])) / (E1[n] * E1[n])
        Rm += (np.abs(s[n, :, 2]) * E1[n] + F1[n] * np.abs(s[n, :, 3] - s[n, :, 2])) / (E1[n] * E1[n])
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        kap = np.where(r1, 0.0, -2.0 / (V1 * V1 * V1 * B) * R)
        kapm = np.where(r1, 0.0, 2.0 / (V1 * V1 * V1 * B) * Rm)
    a1, a2 = w1[None, :] / (E1 * E1)[:, None], w2[None, :] / (E2 * E2)[:, None]
    e1, g1, e2, g2 = E1[:, None], F1[:, None], E2[:, None], F2[:, None]
    sc = -0.5 * float(grad_scale)
    out.coef = sc * np.stack([kap[None, :] + a2 * (g2 - e2), -2.0 * a1 * g1 - 2.0 * a2 * g2, a1 * (e1 + g1) + a2 * (e2 + g2)], axis=-1)
    # c0 is a difference twice over: kap + a2 (F2 - E2), and kap itself sums Spl E1 - F1 (SS - Spl) over the samples (for C = 1 the weight cancels
    # out of F1 / E1 up to `smooth`, so kap is ~1e-5 of its terms).  Its magnitude takes the absolute value of every product.
    out.coef_mag = abs(sc) * np.stack([kapm[None, :] + a2 * (g2 + e2), 2.0 * a1 * g1 + 2.0 * a2 * g2, a1 * (e1 + g1) + a2 * (e2 + g2)], axis=-1)
    return out


def fold(sums, replicas):
    """The sum of `replicas` copies [replicas][...] in replica order, from 0."""
    s = np.asarray(sums, f64)
    assert s.shape[0] == replicas
    a = np.zeros(s.shape[1:])
    for r in range(replicas):
        a = a + s[r]
    return a


def metric_counts(p, y, keep):
    """{argmax p == argmax y, TP, FP, TN, FN} over the pixels of `keep`: the first maximum wins, a class is on when its value is strictly above 0.5."""
    k = np.asarray(keep, bool).reshape(-1)
    p, y = np.asarray(p).reshape(k.size, -1)[k], np.asarray(y).reshape(k.size, -1)[k]
    t, q = y > 0.5, p > 0.5
    return np.array([(p.argmax(1) == y.argmax(1)).sum(), (t & q).sum(), (~t & q).sum(), (~t & ~q).sum(), (t & ~q).sum()], f64)


def clipped_share(p):
    """u = clip(p / sum p, eps, 1 - eps) with the float32 bounds, and where u lies strictly inside."""
    p = np.asarray(p, f64)
    q = p / p.sum(-1, keepdims=True)
    return np.clip(q, f64(EPS32), f64(ONE_M_EPS32)), (q >= f64(EPS32)) & (q <= f64(ONE_M_EPS32))


def log_sum_exp(z):
    z = np.asarray(z, f64)
    mx = z.max(-1, keepdims=True)
    return mx + np.log(np.exp(z - mx).sum(-1, keepdims=True))


def pixel_loss(kind, p, z, y, cw):
    """[M] losses of the four plain kinds (utils.py:481-490; Keras' CategoricalCrossentropy / BinaryCrossentropy on logits, MeanSquaredError)."""
    y = np.asarray(y, f64)
    if kind == WCE:
        u, _ = clipped_share(p)
        return -(y * np.log(u) * np.asarray(cw, f64)).sum(-1)
    if kind == CE_LOGITS:
        z = np.asarray(z, f64)
        return -(y * (z - log_sum_exp(z))).sum(-1)
    if kind == BCE_LOGITS:
        z = np.asarray(z, f64)
        return (np.maximum(z, 0.0) - z * y + np.log1p(np.exp(-np.abs(z)))).mean(-1)
    assert kind == MSE
    return ((y - np.asarray(p, f64)) ** 2).mean(-1)


def jacobian(act, p, g, gm):
    """(dz, scale) from the gradient g with respect to the activation's output p; gm >= |g| is g's own scale."""
    if act == ACT_SOFTMAX:
        return p * (g - (g * p).sum(-1, keepdims=True)), np.abs(p) * (gm + (gm * np.abs(p)).sum(-1, keepdims=True))
    if act == ACT_SIGMOID:
        return g * p * (1.0 - p), gm * np.abs(p * (1.0 - p))
    return g, gm


def dz(kind, act, p, y, coef=None, cw=None, grad_scale=1.0, with_scale=False):
    """d(loss) / d(logits) [B][HW][C] from the stored activations p.  The two logits kinds use p = softmax(z) / sigmoid(z) directly; the others go
    through dp and the activation's Jacobian.  with_scale: also the sum of the absolute values of the terms that form each element."""
    p, y, gs = np.asarray(p, f64), np.asarray(y, f64), float(grad_scale)
    C = p.shape[-1]
    if kind == CE_LOGITS:
        sy = y.sum(-1, keepdims=True)
        out, mag = (p * sy - y) * gs, (np.abs(p * sy) + np.abs(y)) * abs(gs)
    elif kind == BCE_LOGITS:
        out, mag = (p - y) * gs / C, (np.abs(p) + np.abs(y)) * abs(gs) / C
    else:
        if kind == TANIMOTO:
            k = np.asarray(coef, f64).reshape(p.shape[0], 1, C, 3)
            g, gm = k[..., 0] + k[..., 1] * p + k[..., 2] * y, np.abs(k[..., 0]) + np.abs(k[..., 1] * p) + np.abs(k[..., 2] * y)
        elif kind == WCE:
            u, inside = clipped_share(p)
            S = p.sum(-1, keepdims=True)
            h = np.where(inside, -y * np.asarray(cw, f64) / u, 0.0)
            hu = (h * u).sum(-1, keepdims=True)
            g, gm = (h - hu) / S * gs, (np.abs(h) + np.abs(hu)) / np.abs(S) * abs(gs)
        else:
            assert kind == MSE
            g = 2.0 * (p - y) * gs / C
            gm = np.abs(g)
        out, mag = jacobian(act, p, g, gm)
    return (out, mag) if with_scale else out
