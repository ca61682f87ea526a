"""What tests/test_conv_exact_gpu.py and tests/test_conv_exact_host.py share: the case tables, small-integer data, float64 references and the exact comparison.
A plain module (no tests, no fixtures).

With ternary activations / weights / output gradients and small integer biases, residuals and bases, every product and every partial sum of a convolution
or a weight gradient is an integer below 2**24: exact in bf16 and fp32 alike, in any summation order (fp32 atomics, K slabs, block partials) and in the
fp64 statistics.  The bound of the comparison is therefore ZERO.  The preconditions (checked by the host test on the reference alone and again by every
GPU case before it launches): stored outputs within +-256 (every integer up to 256 is a bf16 value), accumulators below 2**24, outputs of >= 50 distinct
values, and no pixel that could drop out unseen."""
import dataclasses
import functools
import zlib
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

BF16, F32 = "bf16", "f32"
DISTINCT = 50                                                # distinct values a reference y / dW has to take
STAT_R = 2                                                   # stats_replicas of every statistics case (summed on the host)


# ---------------------------------------------------------------------------------------------------------------- data
def seed_of(name):
    return zlib.crc32(name.encode())


def ternary(rng, shape, p, scale=1, pos=0.5):
    """{-scale, 0, scale}, a share p of the entries nonzero; pos (a number, or an array that broadcasts to the shape): the share of the nonzero entries that are
    positive.  Short sums of unbiased signs take few values (K = 32: some 40): where a case says `skew`, the signs lean one way by an amount that differs from
    channel to channel, which spreads the sums over a multiple of that range - the entries stay ternary."""
    sign = np.where(rng.random(shape) < pos, scale, -scale)
    return (sign * (rng.random(shape) < p)).astype(np.float32)


def lean(rng, n, skew):
    """per-channel shares of positive signs, spread evenly over 0.5 +- 0.45 and shuffled (skew 0: 0.5 everywhere)"""
    return 0.5 + (0.45 * rng.permutation(np.linspace(-1.0, 1.0, n)) if skew else np.zeros(n))


def ints(rng, lo, hi, shape):
    return rng.integers(lo, hi + 1, size=shape).astype(np.float32)


def pick(rng, values, shape):
    return rng.choice(np.array(values, np.float32), size=shape).astype(np.float32)


def every_pixel_nonzero(rng, t, scale=1):
    """t [N][H][W][C] ternary: a pixel whose vector is all zero gets one +-scale entry (so that no pixel can drop out of a sum unseen)"""
    flat = t.reshape(-1, t.shape[-1])
    dead = np.flatnonzero(~flat.any(axis=1))
    flat[dead, rng.integers(0, t.shape[-1], size=dead.size)] = rng.choice(np.array([-scale, scale], np.float32), size=dead.size)
    return t


# ---------------------------------------------------------------------------------------------------------------- references (float64)
def conv_ref(x, w, dil, taps, stride=1, up=0):
    """x [N][Hs][Ws][C], w [taps][Cout][C] (tap = ky * 3 + kx) -> float64 [N][H][W][Cout]: zero padding dil, nearest upsampling by 2**up folded into the read"""
    xt = torch.from_numpy(np.ascontiguousarray(x)).double().permute(0, 3, 1, 2)
    if up:
        xt = xt.repeat_interleave(1 << up, 2).repeat_interleave(1 << up, 3)
    k = 3 if taps == 9 else 1
    Cout, Cin = w.shape[1], w.shape[2]
    wt = torch.from_numpy(np.ascontiguousarray(w)).double().reshape(k, k, Cout, Cin).permute(2, 3, 0, 1)
    y = F.conv2d(xt, wt, None, stride=stride, padding=dil * (k // 2), dilation=dil)
    return y.permute(0, 2, 3, 1).contiguous().numpy()


def wgrad_ref(a, dy, dil, taps, stride=1):
    """dW[t][co][c] = sum over pixels of dy[n, h, w, co] * a[n, h * stride + dy_t * dil, w * stride + dx_t * dil, c] in float64: one matrix product per tap"""
    N, Hs, Ws, Cs = a.shape
    _, H, W, Cout = dy.shape
    k = 3 if taps == 9 else 1
    p = dil * (k // 2)
    ap = np.pad(a.astype(np.float64), ((0, 0), (p, p), (p, p), (0, 0)))
    g = dy.astype(np.float64).reshape(-1, Cout)
    out = np.empty((taps, Cout, Cs), np.float64)
    for t in range(taps):
        ky, kx = divmod(t, k)
        sl = ap[:, ky * dil:ky * dil + (H - 1) * stride + 1:stride, kx * dil:kx * dil + (W - 1) * stride + 1:stride, :]
        out[t] = g.T @ sl.reshape(-1, Cs)
    return out


def frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
        elif isinstance(v, list):
            for a in v:
                if isinstance(a, np.ndarray):
                    a.flags.writeable = False
    return d


# ---------------------------------------------------------------------------------------------------------------- forward cases
# epilogues:  "res"   y = conv + bias (+ bias_more) + aux                 statistics mode 1: sum y, sum y^2
#             "mask"  y = conv * (mscale * aux + mshift > 0)              statistics mode 2: sum y, sum y * aux
#             "relu"  y = max(conv + bias, 0)                             no statistics
#             "acc"   y[:, ::2, ::2] += conv (+ bias)   (accumulate, out_stride 2) no statistics
#             "aux3"  y = conv (+ bias); aux is the second statistics operand only  statistics mode 2
#             "resp"  y = conv + bias (+ bias_more) + aux                 no statistics
#             "macc"  y = (y + conv) * (mscale * aux + mshift > 0)        statistics mode 2 (accumulate under the mask: the data-gradient form)
@dataclass(frozen=True)
class Fwd:
    name: str
    dt: str
    N: int
    H: int
    W: int
    segs: tuple                      # ((C, up_shift, dil, taps), ...)
    Cout: int
    epi: str
    kid: int                         # rua_conv_kernel_id the case must be planned on
    stride: int = 1
    px: float = 0.5                  # share of nonzero activations
    pw: float = 0.5                  # share of nonzero weights
    norm: int = 0                    # normalise on load of segment 0: 0 no, 1 scale / shift, 2 scale / shift + ReLU
    ws: bool = False                 # give a workspace (split K)
    split: bool = False              # the plan must take K slices
    tune: tuple = ()                 # ((key, value, default), ...) set around the plan and the launch
    nmore: int = 0                   # bias_more vectors
    mask_bias: bool = False          # "mask" / "macc" / "aux3" / "acc": the descriptor carries the bias vectors too (added before the mask)
    skew: float = 0.0                # short K: share of positive activations 0.5 + skew / 2, the weights' signs lean per output channel (see ternary)

    @property
    def K(self):
        return sum(c * t for c, _, _, t in self.segs)


def fwd_data(c):
    rng = np.random.default_rng(seed_of(c.name))
    d = {"x": [], "w": []}
    for i, (Cs, up, dil, taps) in enumerate(c.segs):
        Hs, Ws = (c.H * c.stride) >> up, (c.W * c.stride) >> up
        scale = 2 if (c.norm and i == 0) else 1
        d["x"].append(ternary(rng, (c.N, Hs, Ws, Cs), c.px, scale, 0.5 + c.skew / 2))
        d["w"].append(ternary(rng, (taps, c.Cout, Cs), c.pw, 1, lean(rng, c.Cout, c.skew).reshape(1, c.Cout, 1)))
    d["bias"] = ints(rng, -4, 4, c.Cout)
    d["more"] = [ints(rng, -4, 4, c.Cout) for _ in range(c.nmore)]
    shape = (c.N, c.H, c.W, c.Cout)
    if c.epi == "res":
        d["aux"] = ints(rng, -8, 8, shape)
    elif c.epi == "resp":
        d["aux"] = ints(rng, -8, 8, shape)
    elif c.epi in ("mask", "aux3", "macc"):
        d["aux"] = ints(rng, -3, 3, shape)
        d["mscale"], d["mshift"] = pick(rng, [-1, 1], c.Cout), pick(rng, [-1, 0, 1], c.Cout)
        if c.epi == "macc":
            d["y0"] = ints(rng, -8, 8, shape)
    elif c.epi == "acc":
        d["y0"] = ints(rng, -8, 8, (c.N, 2 * c.H, 2 * c.W, c.Cout))
    if c.norm:
        Cs = c.segs[0][0]
        d["in_scale"], d["in_shift"] = pick(rng, [-1, -0.5, 0.5, 1], Cs), pick(rng, [-1, 0, 1], Cs)
    return d


def normalised(x, scale, shift, relu):
    v = x.astype(np.float64) * scale + shift
    return np.maximum(v, 0.0) if relu else v


def fwd_conv(c, d):
    """sum over the segments of the convolutions alone (float64)"""
    out = 0
    for i, (Cs, up, dil, taps) in enumerate(c.segs):
        x = d["x"][i]
        if c.norm and i == 0:
            x = normalised(x, d["in_scale"], d["in_shift"], c.norm == 2)
        out = out + conv_ref(x, d["w"][i], dil, taps, c.stride, up)
    return out


def open_one_channel(c, d, conv):
    """ReLU-mask cases: at every pixel the mask is opened (argument 2 > 0) in the channel where the masked value is largest, so that every output pixel is
    nonzero in some channel however few channels there are - a pixel the statistics skipped would otherwise go unseen where it happens to be all zero"""
    v = conv + (d["bias"].astype(np.float64) if c.mask_bias else 0.0) + (d["y0"] if c.epi == "macc" else 0.0)
    flat = np.abs(v).reshape(-1, c.Cout)
    j = flat.argmax(axis=1)
    assert (flat[np.arange(len(j)), j] > 0).all(), (c.name, "a pixel whose convolution is zero in every channel")
    aux = d["aux"].reshape(-1, c.Cout)
    aux[np.arange(len(j)), j] = d["mscale"][j] * (2 - d["mshift"][j])          # mscale * aux + mshift = 2 (mscale = +-1)


def fwd_epilogue(c, d, conv):
    """-> y as stored (float64), statistics [2][Cout] or None"""
    bias = d["bias"].astype(np.float64)
    for m in d["more"]:
        bias = bias + m
    stats = None
    if c.epi == "res":
        y = conv + bias + d["aux"]
        stats = np.stack([y.sum(axis=(0, 1, 2)), (y * y).sum(axis=(0, 1, 2))])
    elif c.epi == "resp":
        y = conv + bias + d["aux"]
    elif c.epi in ("mask", "macc"):
        a = d["aux"].astype(np.float64)
        y = conv + bias if c.mask_bias else conv
        if c.epi == "macc":
            y = y + d["y0"]
        y = y * ((d["mscale"] * a + d["mshift"]) > 0)
        stats = np.stack([y.sum(axis=(0, 1, 2)), (y * a).sum(axis=(0, 1, 2))])
    elif c.epi == "aux3":
        a = d["aux"].astype(np.float64)
        y = conv + bias if c.mask_bias else conv
        stats = np.stack([y.sum(axis=(0, 1, 2)), (y * a).sum(axis=(0, 1, 2))])
    elif c.epi == "relu":
        y = np.maximum(conv + bias, 0.0)
    elif c.epi == "acc":
        y = d["y0"].astype(np.float64).copy()
        y[:, ::2, ::2, :] += conv + bias if c.mask_bias else conv
    else:
        raise ValueError(c.epi)
    return y, stats


@functools.lru_cache(maxsize=4)
def fwd_case(c):
    """data + reference of a forward case, computed once and left unchanged"""
    d = fwd_data(c)
    conv = fwd_conv(c, d)
    if c.epi in ("mask", "macc"):
        open_one_channel(c, d, conv)
    y, stats = fwd_epilogue(c, d, conv)
    d.update(conv=conv, y=y, stats=stats)
    return frozen(d)


def check_fwd_preconditions(c, d):
    """preconditions 1 - 3 of a forward case on its reference"""
    y, stats = d["y"], d["stats"]
    assert np.abs(y).max() <= 256, (c.name, "stored |y| beyond the integers bf16 holds", float(np.abs(y).max()))
    assert np.array_equal(y, np.rint(y)), (c.name, "the reference is not integral")
    xmax = max(float(np.abs(x).max()) for x in d["x"])
    if c.norm:
        xmax = max(xmax, float(np.abs(normalised(d["x"][0], d["in_scale"], d["in_shift"], c.norm == 2)).max()))
    assert c.K * xmax * 1.0 + 64 < 2 ** 24, (c.name, "fp32 accumulator")
    if c.norm:
        xin = normalised(d["x"][0], d["in_scale"], d["in_shift"], c.norm == 2)
        assert np.array_equal(xin, np.rint(xin)) and np.abs(xin).max() <= 3, (c.name, "normalised input")
    assert np.unique(y).size >= DISTINCT, (c.name, "y takes too few values", int(np.unique(y).size))
    if stats is not None:
        assert np.abs(stats).max() < 2 ** 53
        # (2 * Cout numbers: as many distinct values as 50 only where there are that many channels)
        assert np.unique(stats).size >= min(DISTINCT, c.Cout), (c.name, "statistics", int(np.unique(stats).size))
        assert np.abs(y).reshape(-1, c.Cout).max(axis=1).min() > 0, (c.name, "an output pixel is zero in every channel")
    if c.epi in ("mask", "aux3", "macc"):
        arg = d["mscale"] * d["aux"] + d["mshift"]
        assert (arg == 0).mean() > 0.05 and (arg > 0).mean() > 0.2 and (arg < 0).mean() > 0.2, (c.name, "mask argument")


# ---------------------------------------------------------------------------------------------------------------- weight-gradient cases
@dataclass(frozen=True)
class Wg:
    name: str
    dt: str
    N: int
    Hs: int
    Ws: int
    C: int
    Cout: int
    dil: int
    taps: int
    kind: int                        # rua_wgrad_kind the case must be planned on
    stride: int = 1
    img: int = 0                     # rua_wgrad_img_kind
    ws: bool = False                 # workspace of rua_wgrad_workspace_bytes
    pa: float = 0.5
    pdy: float = 0.5
    norm: int = 0
    tune: tuple = ()
    skew: float = 0.0                # few pixels: the signs of a and dy lean per channel (see ternary)

    @property
    def H(self):
        return self.Hs // self.stride

    @property
    def W(self):
        return self.Ws // self.stride


def wg_data(c):
    rng = np.random.default_rng(seed_of(c.name))
    a = every_pixel_nonzero(rng, ternary(rng, (c.N, c.Hs, c.Ws, c.C), c.pa, 2 if c.norm else 1, lean(rng, c.C, c.skew)), 2 if c.norm else 1)
    dy = every_pixel_nonzero(rng, ternary(rng, (c.N, c.H, c.W, c.Cout), c.pdy, 1, lean(rng, c.Cout, c.skew)))
    d = {"a": a, "dy": dy, "base": ints(rng, -8, 8, (c.taps, c.Cout, c.C))}
    if c.norm:
        # scale +-1 / +-0.5 on {-2, 0, 2}, shift in {-1, 0, 1}: integers in [-3, 3]; check_wg_preconditions looks at the NORMALISED pixels (a ReLU could empty one)
        d["in_scale"], d["in_shift"] = pick(rng, [-1, -0.5, 0.5, 1], c.C), pick(rng, [-1, 0, 1], c.C)
    return d


def wg_input(c, d):
    return normalised(d["a"], d["in_scale"], d["in_shift"], c.norm == 2) if c.norm else d["a"].astype(np.float64)


@functools.lru_cache(maxsize=4)
def wg_case(c):
    d = wg_data(c)
    d["grad"] = wgrad_ref(wg_input(c, d), d["dy"], c.dil, c.taps, c.stride)
    d["dw"] = d["grad"] + d["base"]
    return frozen(d)


def check_wg_preconditions(c, d):
    ain = wg_input(c, d)
    assert np.array_equal(ain, np.rint(ain)) and np.abs(ain).max() <= 3
    assert c.N * c.H * c.W * np.abs(ain).max() * np.abs(d["dy"]).max() + 8 < 2 ** 24, (c.name, "fp32 accumulator")
    assert np.array_equal(d["dw"], np.rint(d["dw"]))
    assert np.unique(d["dw"]).size >= DISTINCT, (c.name, "dW takes too few values", int(np.unique(d["dw"]).size))
    assert np.unique(d["grad"]).size >= DISTINCT, (c.name, "the gradient alone takes too few values", int(np.unique(d["grad"]).size))
    assert ain.reshape(-1, c.C).any(axis=1).all(), (c.name, "a pixel of a is zero in every channel")
    assert d["dy"].reshape(-1, c.Cout).any(axis=1).all(), (c.name, "a pixel of dy is zero in every channel")


# ---------------------------------------------------------------------------------------------------------------- comparison
def mismatch(got, exp, what, route, axes):
    """None if got == exp element for element, else the message: how many differ, the first index, got and expected there, the route"""
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    if np.array_equal(got, exp):
        return None
    bad = np.argwhere(~(got == exp))
    first = tuple(int(i) for i in bad[0])
    last = tuple(int(i) for i in bad[-1])
    return (f"{what}: {len(bad)} of {got.size} elements differ; first at {axes} = {first} (last at {last}): got {got[first]!r}, expected {exp[first]!r}; "
            f"route: {route}")


def assert_exact(got, exp, what, route, axes):
    msg = mismatch(got, exp, what, route, axes)
    assert msg is None, msg


# ---------------------------------------------------------------------------------------------------------------- the case tables
def _fwd_cases():
    out = []

    def add(name, dt, N, H, W, segs, Cout, kid, epis, **kw):
        for e in epis:
            epi, norm = (e[:-2], 2) if e.endswith("+n") else (e[:-2], 1) if e.endswith("+m") else (e, 0)      # +n: BatchNorm + ReLU on load, +m: without the ReLU
            out.append(Fwd(f"{name}-{dt}-{e}", dt, N, H, W, tuple(segs), Cout, epi, kid, norm=norm, **kw))

    BOTH = ("res", "mask")
    SK = dict(px=0.9, pw=0.9, skew=0.6)                       # K <= 144
    # conv_igemm (id 0); in bf16 the 1x1 shapes of <= 4096 pixels with 16-channel sources belong to conv_small (id 6)
    for dt in (F32, BF16):
        add("igemm-2x16x16-32-32-d1", dt, 2, 16, 16, [(32, 0, 1, 9)], 32, 0, BOTH + ("relu", "aux3"), px=2 / 3, pw=2 / 3, skew=0.6, mask_bias=True, nmore=2)
        add("igemm-2x16x16-16-32-d15", dt, 2, 16, 16, [(16, 0, 15, 9)], 32, 0, BOTH, **SK)
        add("igemm-3x8x8-40-8", dt, 3, 8, 8, [(40, 0, 1, 9)], 8, 0, BOTH + ("acc",), px=2 / 3, pw=2 / 3, skew=0.6)
        add("pw-2x16x16-32-64-s2", dt, 2, 16, 16, [(32, 0, 1, 1)], 64, 0 if dt == F32 else 6, BOTH, stride=2, **SK)
        add("seg2-2x16x16", dt, 2, 16, 16, [(16, 1, 1, 1), (32, 0, 1, 1)], 32, 0 if dt == F32 else 6, BOTH, **SK)
        add("seg5-1x16x16", dt, 1, 16, 16, [(8, 0, 1, 1), (8, 1, 1, 1), (8, 2, 1, 1), (8, 3, 1, 1), (32, 0, 1, 1)], 32, 0, BOTH, **SK)
        add("acc-2x8x8-64-32", dt, 2, 8, 8, [(64, 0, 1, 1)], 32, 0 if dt == F32 else 6, ("acc",), **SK)
    dt = BF16
    add("acc-2x8x8-32-32-d3", dt, 2, 8, 8, [(32, 0, 3, 9)], 32, 0, ("acc", "macc"), px=2 / 3, pw=2 / 3, skew=0.6)
    # conv_dma (id 1): Cout >= 128 from a source that is no multiple of 64 channels, a small map (64-channel tiles)
    add("dma-2x8x8-32-128", dt, 2, 8, 8, [(32, 0, 1, 9)], 128, 1, BOTH + ("relu", "acc", "aux3", "macc"), px=2 / 3, pw=2 / 3, skew=0.6, mask_bias=True)
    # conv_dmap (id 2): 128-row tiles, 64-row tiles, split K
    add("dmap-2x8x8-128-256", dt, 2, 8, 8, [(128, 0, 1, 9)], 256, 2, BOTH + ("relu", "acc", "aux3", "macc"), px=2 / 3, pw=0.5, mask_bias=True)
    add("dmap-8x32x32-128-256-d3", dt, 8, 32, 32, [(128, 0, 3, 9)], 256, 2, BOTH + ("relu",), px=2 / 3, pw=0.5)
    add("dmap-splitk-2x8x8-256-128", dt, 2, 8, 8, [(256, 0, 1, 9)], 128, 2, BOTH + ("relu", "acc", "aux3", "macc"), px=0.5, pw=0.5, ws=True, split=True, mask_bias=True)
    # conv_halo (id 3): the width is no multiple of 128
    for dil in (3, 31):
        add(f"halo-1x272x248-d{dil}", dt, 1, 272, 248, [(32, 0, dil, 9)], 32, 3, BOTH + (("macc", "relu") if dil == 3 else ("aux3",)), px=2 / 3, pw=2 / 3)
    # conv_pw (id 4)
    add("pw-1x256x256-seg2", dt, 1, 256, 256, [(16, 1, 1, 1), (32, 0, 1, 1)], 32, 4, BOTH + ("aux3", "macc"), **SK)
    add("pw-1x256x256-k96", dt, 1, 256, 256, [(32, 1, 1, 1), (64, 0, 1, 1)], 32, 4, ("relu",), **SK)      # (K = 96: ReLU leaves >= 50 values)
    add("pw-2x256x128-32-8", dt, 2, 256, 128, [(32, 0, 1, 1)], 8, 4, BOTH + ("macc",), **SK)
    # conv_strip (id 5): 256- and 128-pixel strips, plain and normalised on load
    for dil in (1, 31):
        add(f"strip-1x256x256-d{dil}", dt, 1, 256, 256, [(32, 0, dil, 9)], 32, 5, BOTH + ("res+n", "mask+n") + (("relu", "res+m") if dil == 1 else ()), px=2 / 3, pw=2 / 3)
    add("strip-2x256x128-d3", dt, 2, 256, 128, [(32, 0, 3, 9)], 32, 5, BOTH + ("res+n", "relu+n", "mask+n"), px=2 / 3, pw=2 / 3)
    # conv_small (id 6)
    add("small-3x5x7-48+16-40", dt, 3, 5, 7, [(48, 0, 1, 1), (16, 0, 1, 1)], 40, 6, BOTH + ("aux3", "acc", "macc"), **SK)
    add("small-8x8x8-512-1024-s2", dt, 8, 8, 8, [(512, 0, 1, 1)], 1024, 6, BOTH + ("acc", "aux3"), stride=2, px=0.5, pw=0.5)
    add("small-8x16x16-256u1+512-512", dt, 8, 16, 16, [(256, 1, 1, 1), (512, 0, 1, 1)], 512, 6, BOTH + ("relu", "macc"), px=0.5, pw=0.5)
    # conv_img (id 7, opt-in) and conv_img2 (id 8, the default): whole images resident, K slices + finisher
    for kern, kid, tune in (("img2", 8, ()), ("img", 7, (("conv_img2", 0, 1), ("conv_img", 1, 0)))):
        add(f"{kern}-8x8x8-1024-1024", dt, 8, 8, 8, [(1024, 0, 1, 9)], 1024, kid, BOTH + ("macc", "aux3"), px=0.5, pw=0.25, ws=True, tune=tune)
        add(f"{kern}-8x16x16-512-512", dt, 8, 16, 16, [(512, 0, 1, 9)], 512, kid, BOTH + ("relu", "aux3"), px=0.5, pw=0.25, ws=True, split=True, tune=tune)
    # conv_band128m as a sum over segments (id 9)
    add("band128sum-2x64x64-128-d1+15", dt, 2, 64, 64, [(128, 0, 1, 9), (128, 0, 15, 9)], 128, 9, ("resp",), px=0.5, pw=0.5, ws=True, nmore=1)
    return out


def _wg_cases():
    out = []
    for dt in (F32, BF16):
        for ws in (False, True):
            tag = f"{dt}-{'slabs' if ws else 'atomics'}"
            out += [
                Wg(f"tiles-2x16x16-32-32-d1-{tag}", dt, 2, 16, 16, 32, 32, 1, 9, 0, ws=ws),
                Wg(f"tiles-1x24x20-64-32-d3-{tag}", dt, 1, 24, 20, 64, 32, 3, 9, 0, ws=ws),
                Wg(f"tiles-2x16x16-16-48-d15-{tag}", dt, 2, 16, 16, 16, 48, 15, 9, 0, ws=ws),
                Wg(f"tiles-2x16x16-32-64-s2-{tag}", dt, 2, 16, 16, 32, 64, 1, 1, 0, stride=2, ws=ws, pa=0.9, pdy=0.9, skew=0.6),
                Wg(f"tiles-1x12x12-8-8-{tag}", dt, 1, 12, 12, 8, 8, 1, 9, 0, ws=ws, pa=0.9, pdy=0.9, skew=0.6),
            ]
    dt = BF16
    out += [
        # whole-image kernels (within kind 0)
        Wg("img-8x8x8-64-64", dt, 8, 8, 8, 64, 64, 1, 9, 0, img=1, ws=True),
        Wg("imgs-4x16x16-512-256", dt, 4, 16, 16, 512, 256, 1, 9, 0, img=2, ws=True),
        # all-taps (kind 1)
        Wg("taps-2x64x64x32-d1", dt, 2, 64, 64, 32, 32, 1, 9, 1, ws=True),
        Wg("taps-2x64x64x32-d31", dt, 2, 64, 64, 32, 32, 31, 9, 1, ws=True),
        Wg("taps-3x7x128x32-d3", dt, 3, 7, 128, 32, 32, 3, 9, 1, ws=True),
        Wg("rows32-8x16x256x32-r127", dt, 8, 16, 256, 32, 32, 1, 9, 1, ws=True, tune=(("wgrad_rows", 127, 127),)),
        Wg("rows32-8x16x256x32-r255", dt, 8, 16, 256, 32, 32, 1, 9, 1, ws=True, tune=(("wgrad_rows", 255, 127),)),
        Wg("rows64-1x128x128x64-d31", dt, 1, 128, 128, 64, 64, 31, 9, 1, ws=True),
        Wg("rowsx0-1x7x64x128-d3", dt, 1, 7, 64, 128, 128, 3, 9, 1, ws=True),
        Wg("rowsx1-2x32x32x256-d1", dt, 2, 32, 32, 256, 256, 1, 9, 1, ws=True),
        Wg("rowsx1-2x32x32x256-d16", dt, 2, 32, 32, 256, 256, 16, 9, 1, ws=True),
        Wg("taps-norm-2x64x128x32-d3", dt, 2, 64, 128, 32, 32, 3, 9, 1, ws=True, norm=2),
        Wg("taps-norm-1x128x128x64-d1", dt, 1, 128, 128, 64, 64, 1, 9, 1, ws=True, norm=1),
        # wgrad_dmap (kind 2): 36 tiles, 64 stages
        Wg("dmap-4x32x32-256-256-d3", dt, 4, 32, 32, 256, 256, 3, 9, 2),
        Wg("dmap-4x32x32-256-256-d3-slabs", dt, 4, 32, 32, 256, 256, 3, 9, 2, ws=True, tune=(("wgrad_rows", 0, 127),)),
        # wgrad_pw (kind 3): 2048 pixels
        Wg("pw-2x32x32-32-8", dt, 2, 32, 32, 32, 8, 1, 1, 3, ws=True, pa=1.0, pdy=1.0),
        Wg("pw-2x64x64-32-64-s2", dt, 2, 64, 64, 32, 64, 1, 1, 3, stride=2, ws=True, pa=2 / 3, pdy=2 / 3),
        Wg("pw-2x32x32-32-8-replicas", dt, 2, 32, 32, 32, 8, 1, 1, 3, ws=True, pa=1.0, pdy=1.0, tune=(("wgrad_pw", 1, 3),)),
    ]
    return out


FWD_CASES = _fwd_cases()
WG_CASES = _wg_cases()
# conv_dmap members that walk back to back through ONE grid (rua_conv_fwd_group with the tuning key dmap_chain): three dilation branches, each with its own epilogue
CHAIN_CASES = [dataclasses.replace(next(c for c in FWD_CASES if c.name == "dmap-8x32x32-128-256-d3-bf16-mask"), name=f"dmap-chain-m{i}-d{dil}", segs=((128, 0, dil, 9),))
               for i, dil in enumerate((1, 3, 15))]


# ---------------------------------------------------------------------------------------------------------------- band forms: several 3x3 convolutions in one launch
# form "sum":   rua_conv_fwd_sum - y = aux + sum_b (conv_b(norm_b(x_b)) + bias_b), one output (conv_band32 / conv_band64)
# form "group": rua_conv_fwd_group - independent members, each with its own epilogue (conv_band64m / conv_band128m):
#               kind "first": one shared input, normalised on load by the member's own in_scale / in_shift (+ ReLU), bias, statistics mode 1
#               kind "dgrad": own inputs, ReLU mask from the member's aux, statistics mode 2
@dataclass(frozen=True)
class Band:
    name: str
    form: str
    N: int
    H: int
    W: int
    C: int
    dils: tuple
    kind: str                        # sum: "plain" / "norm"; group: "first" / "dgrad"
    expect: int                      # sum: rua_conv_sum_kernel (1 conv_band32, 2 conv_band64); group: the band flag of the plan (1 conv_band64m, 2 conv_band128m)
    px: float = 0.5
    pw: float = 0.25


def band_data(c):
    rng = np.random.default_rng(seed_of(c.name))
    nb = len(c.dils)
    shape = (c.N, c.H, c.W, c.C)
    normed = c.kind in ("norm", "first")
    shared = c.form == "group" and c.kind == "first"
    d = {"x": [ternary(rng, shape, c.px, 2 if normed else 1) for _ in range(1 if shared else nb)],
         "w": [ternary(rng, (9, c.C, c.C), c.pw) for _ in range(nb)],
         "bias": [ints(rng, -4, 4, c.C) for _ in range(nb)]}
    if normed:
        d["in_scale"] = [pick(rng, [-1, -0.5, 0.5, 1], c.C) for _ in range(nb)]
        d["in_shift"] = [pick(rng, [-1, 0, 1], c.C) for _ in range(nb)]
    if c.form == "sum":
        d["aux"] = ints(rng, -8, 8, shape)
    elif c.kind == "dgrad":
        d["aux"] = [ints(rng, -3, 3, shape) for _ in range(nb)]
        d["mscale"] = [pick(rng, [-1, 1], c.C) for _ in range(nb)]
        d["mshift"] = [pick(rng, [-1, 0, 1], c.C) for _ in range(nb)]
    return d


@functools.lru_cache(maxsize=2)
def band_case(c):
    d = band_data(c)
    nb = len(c.dils)
    normed = c.kind in ("norm", "first")
    convs = []
    for b in range(nb):
        x = d["x"][0 if len(d["x"]) == 1 else b]
        if normed:
            x = normalised(x, d["in_scale"][b], d["in_shift"][b], True)
        convs.append(conv_ref(x, d["w"][b], c.dils[b], 9))
    if c.form == "sum":
        y = d["aux"].astype(np.float64)
        for b in range(nb):
            y = y + convs[b] + d["bias"][b]
        d["y"], d["stats"] = [y], [None]
    else:
        d["y"], d["stats"] = [], []
        for b in range(nb):
            if c.kind == "first":
                y = convs[b] + d["bias"][b]
                st = np.stack([y.sum(axis=(0, 1, 2)), (y * y).sum(axis=(0, 1, 2))])
            else:
                a = d["aux"][b].astype(np.float64)
                y = convs[b] * ((d["mscale"][b] * a + d["mshift"][b]) > 0)
                st = np.stack([y.sum(axis=(0, 1, 2)), (y * a).sum(axis=(0, 1, 2))])
            d["y"].append(y); d["stats"].append(st)
    for y in d["y"]:
        y.flags.writeable = False
    return frozen(d)


def check_band_preconditions(c, d):
    amax = 3.0 if c.kind in ("norm", "first") else 1.0
    assert 9 * c.C * len(c.dils) * amax + 64 < 2 ** 24
    for b, (y, st) in enumerate(zip(d["y"], d["stats"])):
        assert np.abs(y).max() <= 256, (c.name, b, float(np.abs(y).max()))
        assert np.array_equal(y, np.rint(y))
        assert np.unique(y).size >= DISTINCT, (c.name, b, int(np.unique(y).size))
        if st is not None:
            assert np.unique(st).size >= min(DISTINCT, c.C), (c.name, b)
            assert np.abs(y).reshape(-1, c.C).max(axis=1).min() > 0, (c.name, b, "an output pixel is zero in every channel")


SUM_CASES = [
    Band("sum-band32-1x256x256x32", "sum", 1, 256, 256, 32, (1, 3, 15, 31), "norm", 1),
    Band("sum-band32-plain-1x256x256x32", "sum", 1, 256, 256, 32, (31, 1), "plain", 1, pw=0.5),
    Band("sum-band64-1x128x128x64", "sum", 1, 128, 128, 64, (1, 3, 15, 31), "norm", 2),
]
GROUP_CASES = [
    Band("group-band64m-first-1x128x128x64", "group", 1, 128, 128, 64, (1, 3, 15, 31), "first", 1),
    Band("group-band64m-dgrad-1x128x128x64", "group", 1, 128, 128, 64, (1, 3, 15, 31), "dgrad", 1, pw=0.5),
    Band("group-band128m-first-2x64x64x128", "group", 2, 64, 64, 128, (1, 3, 15), "first", 2),
    Band("group-band128m-dgrad-2x64x64x128", "group", 2, 64, 64, 128, (1, 3, 15), "dgrad", 2, pw=0.5),
]


# ---------------------------------------------------------------------------------------------------------------- grouped, batched and deferred weight gradients
@dataclass(frozen=True)
class WgGroup:
    name: str
    form: str                        # "group": rua_conv_wgrad_group of all-taps members sharing one round of blocks; "batch": the batched form (batch = 1) of unequal
    members: tuple                   # generic members; "deferred": rua_conv_wgrad(defer = 1) per member, then ONE rua_wgrad_reduce_batch


def _wg_groups():
    g, b, q = "wgroup-alltaps4", "wgroup-batch3", "wgroup-deferred2"
    return [
        WgGroup(g, "group", tuple(Wg(f"{g}-m{i}-d{dil}", BF16, 2, 64, 64, 32, 32, dil, 9, 1, ws=True) for i, dil in enumerate((1, 3, 15, 31)))),
        WgGroup(b, "batch", (Wg(f"{b}-m0", BF16, 2, 16, 16, 32, 32, 1, 9, 0, ws=True), Wg(f"{b}-m1", BF16, 1, 24, 20, 64, 32, 3, 9, 0, ws=True),
                             Wg(f"{b}-m2", BF16, 2, 16, 16, 32, 64, 1, 1, 0, stride=2, ws=True, pa=0.9, pdy=0.9, skew=0.6))),
        WgGroup(q, "deferred", (Wg(f"{q}-m0", BF16, 2, 64, 64, 32, 32, 3, 9, 1, ws=True), Wg(f"{q}-m1", BF16, 2, 16, 16, 32, 32, 1, 9, 0, ws=True))),
    ]


WG_GROUPS = _wg_groups()
