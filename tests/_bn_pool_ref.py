"""Plain float64 numpy references of the BatchNorm family and the pooling family of librua_hip.so (include/rua_hip.h), for tests/test_bn_gpu.py and
tests/test_pool_gpu.py.  No GPU, no torch: tests/test_bn_pool_ref_host.py checks every function here against torch-CPU, so the GPU tests may trust them.
Channels-last throughout: BatchNorm tensors are [M][C], pooling tensors [N][H][W][C]."""
import numpy as np

f32, f64 = np.float32, np.float64


# ---- bf16 on bit patterns ----------------------------------------------------------------------------------------------------------------
def bf16_bits(a):
    """uint16 bit patterns of float32 values rounded to bf16, round to nearest even (a NaN stays a quiet NaN of its sign)."""
    u = np.ascontiguousarray(a, f32).view(np.uint32)
    r = ((u + (np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1)))) >> np.uint32(16)).astype(np.uint16)
    nan = np.isnan(np.asarray(a, f32))
    return np.where(nan, ((u >> np.uint32(16)) | np.uint32(0x40)).astype(np.uint16), r)


def bf16_value(bits):
    """float32 values of bf16 bit patterns."""
    return (np.ascontiguousarray(bits, np.uint16).astype(np.uint32) << np.uint32(16)).view(f32)


def round_storage(a, bf16):
    """float32 array holding a rounded to the storage type (float32, or bf16 kept in float32)."""
    a = np.asarray(a, f64).astype(f32)
    return bf16_value(bf16_bits(a)) if bf16 else a


def storage_bits(a, bf16):
    """Bit patterns (uint16 / uint32) of float32 values stored in the storage type."""
    return bf16_bits(a) if bf16 else np.ascontiguousarray(a, f32).view(np.uint32).copy()


# ---- BatchNorm forward -------------------------------------------------------------------------------------------------------------------
def bn_moments(s1, s2, count):
    """mean and biased variance (clamped at 0) of a channel from sum x and sum x^2."""
    mean = np.asarray(s1, f64) / count
    var = np.maximum(np.asarray(s2, f64) / count - mean * mean, 0.0)
    return mean, var


def bn_coeffs(mean, var, gamma, beta, eps):
    """(scale, shift, rstd): out = scale * x + shift is gamma * (x - mean) * rstd + beta."""
    rstd = 1.0 / np.sqrt(np.asarray(var, f64) + f64(eps))
    scale = np.asarray(gamma, f64) * rstd
    return scale, np.asarray(beta, f64) - np.asarray(mean, f64) * scale, rstd


def bn_moving(mmean, mvar, mean, var, momentum, bessel_n):
    """Moving statistics after one training step: the variance enters unbiased (Bessel factor n / (n - 1) for n > 1)."""
    mom = f64(momentum)
    unb = var * (bessel_n / (bessel_n - 1.0)) if bessel_n > 1 else var
    return np.asarray(mmean, f64) * mom + mean * (1.0 - mom), np.asarray(mvar, f64) * mom + unb * (1.0 - mom)


def bn_out_stats(count, beta, scale, var):
    """(sum, sum of squares) of a training-mode BatchNorm's output without ReLU, from its coefficients: mean beta, variance scale^2 var."""
    beta, scale = np.asarray(beta, f64), np.asarray(scale, f64)
    return count * beta, count * (beta * beta + scale * scale * var)


def bn_apply(x, scale, shift, relu):
    y = np.asarray(scale, f64) * np.asarray(x, f64) + np.asarray(shift, f64)
    return np.maximum(y, 0.0) if relu else y


# ---- BatchNorm backward ------------------------------------------------------------------------------------------------------------------
def bn_bwd_coeffs(sg, sgx, count, gamma, mean, rstd):
    """(A, B, C, dgamma, dbeta) from sum g m and sum g m x: the input gradient of one branch is A g m + B x + C."""
    sg, sgx, gamma, mean, rstd = (np.asarray(a, f64) for a in (sg, sgx, gamma, mean, rstd))
    dbeta = sg
    dgamma = rstd * (sgx - mean * sg)
    s = gamma * rstd
    return s, -s * rstd * dgamma / count, -s * dbeta / count + s * rstd * mean * dgamma / count, dgamma, dbeta


def stats2_from_out(sg, sgo, scale, shift, mean):
    """sum g x from sum g out, out = scale x + shift (rua_bn_bwd_branch.stats2_out); a channel with scale == 0 falls back to mean * sum g."""
    sg, sgo, scale, shift = (np.asarray(a, f64) for a in (sg, sgo, scale, shift))
    ok = scale != 0
    return np.where(ok, (sgo - shift * sg) / np.where(ok, scale, 1.0), np.asarray(mean, f64) * sg)


def relu_mask(x, mscale, mshift):
    """Where the ReLU behind the BatchNorm let the gradient through: mscale x + mshift > 0, strictly."""
    return (np.asarray(mscale, f64) * np.asarray(x, f64) + np.asarray(mshift, f64)) > 0


def bn_bwd_apply(x, gs, As, masks, B, C, dskip=None, old=None):
    """(dx, T): dx = [old] + [dskip] + B x + C + sum_b A_b g_b m_b in float64 and T, the sum of the absolute values of those terms.
    B and C are the sums over the branches; masks[b] is a boolean array or None."""
    x = np.asarray(x, f64)
    t = [np.asarray(B, f64) * x, np.broadcast_to(np.asarray(C, f64), x.shape)]
    if dskip is not None:
        t.append(np.asarray(dskip, f64))
    if old is not None:
        t.append(np.asarray(old, f64))
    for g, A, m in zip(gs, As, masks):
        gm = np.asarray(g, f64) if m is None else np.where(m, np.asarray(g, f64), 0.0)
        t.append(np.asarray(A, f64) * gm)
    return sum(t), sum(np.abs(a) for a in t)


# ---- pooling -----------------------------------------------------------------------------------------------------------------------------
def windows(x, k):
    """[N][H/k][W/k][C][k*k]: the k x k windows of x, positions row-major (a * k + b)."""
    N, H, W, Cc = x.shape
    return x.reshape(N, H // k, k, W // k, k, Cc).transpose(0, 1, 3, 5, 2, 4).reshape(N, H // k, W // k, Cc, k * k)


def maxpool_scan(x, k):
    """(values, argmax bytes) of the k x k max-pool: a row-major scan with `v > best` from -inf.  The first maximum wins (-0.0 and +0.0 tie),
    NaN never wins, a window of only NaN and / or -inf gives -inf and byte 0.  Values keep the dtype (and the bits) of x."""
    w = windows(np.asarray(x), k)
    best = np.full(w.shape[:-1], -np.inf, w.dtype)
    bi = np.zeros(w.shape[:-1], np.int64)
    with np.errstate(invalid="ignore"):
        for p in range(k * k):
            v = w[..., p]
            on = v > best
            best = np.where(on, v, best)
            bi = np.where(on, p, bi)
    return best, bi.astype(np.uint8)


def maxpool_derive(y_half, idx_half, k_half):
    """The 2k max-pool from the k max-pool [N][Hh][Wh][C] and its argmax bytes: of the four k-winners of a 2k window the greater value wins,
    on equal values the smaller row-major position inside the 2k window."""
    kp, k = k_half, 2 * k_half
    N, Hp, Wp, Cc = y_half.shape
    best = np.full((N, Hp // 2, Wp // 2, Cc), -np.inf, y_half.dtype)
    bi = np.full(best.shape, k * k, np.int64)
    for u in range(4):
        v = y_half[:, (u >> 1)::2, (u & 1)::2, :]
        pp = idx_half[:, (u >> 1)::2, (u & 1)::2, :].astype(np.int64)
        pos = ((u >> 1) * kp + pp // kp) * k + (u & 1) * kp + pp % kp
        on = (v > best) | ((v == best) & (pos < bi))
        best = np.where(on, v, best)
        bi = np.where(on, pos, bi)
    return best, bi.astype(np.uint8)


def maxpool_scatter(shape, gs, idxs, ks, old=None):
    """dx [N][H][W][C] in float32: old (or 0), then + g[u] where the argmax byte of the pixel's k[u]-window names the pixel, u in order -
    float32 additions old, g[0], g[1], g[2].  The caller rounds the result once to the storage type."""
    N, H, W, Cc = shape
    o = np.zeros(shape, f32) if old is None else np.array(old, f32)
    hh, ww = np.arange(H)[:, None], np.arange(W)[None, :]
    for g, idx, k in zip(gs, idxs, ks):
        pos = ((hh % k) * k + (ww % k))[None, :, :, None]
        gi = np.repeat(np.repeat(np.asarray(g, f32), k, 1), k, 2)
        ii = np.repeat(np.repeat(np.asarray(idx).astype(np.int64), k, 1), k, 2)
        o = np.where(ii == pos, (o + gi).astype(f32), o)
    return o


def sumpool(x, k):
    """Sums over the k x k windows, float64."""
    return windows(np.asarray(x, f64), k).sum(-1)
