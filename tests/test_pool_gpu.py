"""The pooling entry points of librua_hip.so through the C ABI - rua_maxpool_fwd, rua_maxpool_derive, rua_maxpool_bwd, rua_maxpool_bwd_multi,
rua_sumpool, rua_sumpool_pyramid - bit for bit against the numpy references of tests/_bn_pool_ref.py (checked against torch-CPU in
tests/test_bn_pool_ref_host.py).  The data are small integers, so ties are the rule and the first-maximum rule of include/rua_hip.h decides every
argmax byte; one tensor carries planted windows of equal values, -inf, NaN and signed zeros.  A "piece" is the 16-byte vector a thread moves
(8 bf16 / 4 fp32 channels); every output sits between guard regions (tests/_kernel_util.py: Guarded)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _bn_pool_ref as R  # noqa: E402
from _kernel_util import Guarded, bit_dtype, stream  # noqa: E402
from resunet_a_mltsk_keras_amd import _lib as L  # noqa: E402

f32, f64 = np.float32, np.float64
LAYOUTS = [(L.RUA_BF16, 8), (L.RUA_F32, 4), (L.RUA_BF16, 24)]            # one piece per pixel in both types, three pieces
LAYOUT_IDS = ["bf16-C8", "f32-C4", "bf16-C24"]
SHAPES = [(2, 48, 48), (1, 32, 16)]
QNAN = {L.RUA_F32: 0x7FC00000, L.RUA_BF16: 0x7FC0}


def bf(dt):
    return dt == L.RUA_BF16


def bits(a, dt):
    return R.storage_bits(np.asarray(a, f32), bf(dt))


def values(b, dt):
    return R.bf16_value(b) if bf(dt) else b.view(f32)


def ints(rng, shape, lo, hi):
    return rng.integers(lo, hi + 1, shape).astype(f32)


def planted(rng, Cc):
    """(1, 48, 48, C) of integers in [-3, 3] with, per channel c % 4 of the top-left 16 x 16 corner: only NaN / only -inf / NaN and -inf mixed / all equal;
    below it a 16 x 16 corner of zeros whose first column is -0.0; NaN sprinkled beside finite values everywhere else."""
    x = ints(rng, (1, 48, 48, Cc), -3, 3)
    x[rng.random(x.shape) < 0.1] = np.nan
    mix = np.where(rng.random((16, 16)) < 0.5, np.nan, -np.inf).astype(f32)
    for c in range(Cc):
        x[0, :16, :16, c] = (np.nan, -np.inf, 0, 2.0)[c % 4]
        if c % 4 == 2:
            x[0, :16, :16, c] = mix
    x[0, 16:32, :16, :] = 0.0
    x[0, 16:32, 0:16:2, :] = -0.0
    x[0, 32:48, :16, :] = 0.0
    x[0, 32:48, 1:16:2, :] = -0.0
    x[0, 47, 47, :] = 9.0                                    # the only maximum at the last position of its window: byte 255 at k = 16
    x[0, 8, 32, :] = 9.0                                     # ... and at position 128 at k = 16
    return x


def tensors(k, Cc, seed):
    """The test tensors a window k divides: the two shapes of small integers and the planted one."""
    rng = np.random.default_rng(seed)
    out = [ints(rng, (N, H, W, Cc), -3, 3) for N, H, W in SHAPES if H % k == 0 and W % k == 0]
    return out + [planted(rng, Cc)]


def fwd(x, k, dt):
    N, H, W, Cc = x.shape
    xd = Guarded(bits(x, dt))
    y = Guarded(np.full((N, H // k, W // k, Cc), QNAN[dt], bit_dtype(dt)))
    idx = Guarded(np.full((N, H // k, W // k, Cc), 0xEE, np.uint8))
    L.lib().call("rua_maxpool_fwd", xd.ptr, y.ptr, idx.ptr, N, H, W, Cc, k, dt, stream())
    torch.cuda.synchronize()
    assert np.array_equal(xd.get(), bits(x, dt))
    return y, idx


def same(got, want, what):
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    assert bad.size == 0, (what, len(bad), "first at", np.unravel_index(int(bad[0]), got.shape), int(got.reshape(-1)[bad[0]]), int(want.reshape(-1)[bad[0]]))


@pytest.mark.parametrize("k", [1, 2, 3, 4, 8, 16])
@pytest.mark.parametrize("dt,Cc", LAYOUTS, ids=LAYOUT_IDS)
def test_maxpool_fwd_values_and_argmax_bytes(dt, Cc, k):
    """k = 2, 4, 8 take the unrolled kernels, 1, 3, 16 the run-time loop; at k = 16 the positions fill the byte (255)."""
    for x in tensors(k, Cc, 100 + k):
        y, idx = fwd(x, k, dt)
        wy, wi = R.maxpool_scan(x, k)
        same(y.get(), bits(wy, dt), ("values", x.shape))
        same(idx.get(), wi, ("argmax", x.shape))
    if k == 16:
        assert wi.max() == 255 and (wi == 128).any()                             # the planted tensor comes last


@pytest.mark.parametrize("kh", [1, 2, 4, 8])
@pytest.mark.parametrize("dt,Cc", LAYOUTS, ids=LAYOUT_IDS)
def test_maxpool_derive_is_the_direct_scan_with_2k(dt, Cc, kh):
    """y_half / idx_half come from a direct launch with k_half; the derived 2k pool has to be the reference scan with 2k, values and bytes -
    also where the direct launch answered -inf / byte 0 for a window without a finite value.  k_half = 8: the search starts at 256, beyond a byte.  (The four candidates' positions differ, so `pos < bi` and `pos <= bi` in the kernel are one function; preferring
    the larger position on a tie fails every case here.)"""
    for x in tensors(2 * kh, Cc, 200 + kh):
        N, H, W, _ = x.shape
        yh, ih = fwd(x, kh, dt)
        y = Guarded(np.full((N, H // (2 * kh), W // (2 * kh), Cc), QNAN[dt], bit_dtype(dt)))
        idx = Guarded(np.full(y.shape, 0xEE, np.uint8))
        L.lib().call("rua_maxpool_derive", yh.ptr, ih.ptr, y.ptr, idx.ptr, N, H // kh, W // kh, Cc, kh, dt, stream())
        torch.cuda.synchronize()
        wy, wi = R.maxpool_scan(x, 2 * kh)
        same(y.get(), bits(wy, dt), ("values", x.shape))
        same(idx.get(), wi, ("argmax", x.shape))


def gauss(rng, shape, dt):
    return R.round_storage(rng.standard_normal(shape) * 2.0, bf(dt))


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("dt,Cc", LAYOUTS, ids=LAYOUT_IDS)
def test_maxpool_bwd_scatter(dt, Cc, acc):
    """dx = [old +] g at the position the argmax byte names, +0 (or old) elsewhere; float32 old + g rounded once.  The argmax bytes are the reference's."""
    for k in (1, 2, 3, 16):
        rng = np.random.default_rng(300 + k + acc)
        x = tensors(k, Cc, 300 + k)[0]
        N, H, W, _ = x.shape
        _, wi = R.maxpool_scan(x, k)
        g, old = gauss(rng, wi.shape, dt), gauss(rng, x.shape, dt)
        gd, idd, dx = Guarded(bits(g, dt)), Guarded(wi), Guarded(bits(old, dt))
        L.lib().call("rua_maxpool_bwd", gd.ptr, idd.ptr, dx.ptr, acc, N, H, W, Cc, k, dt, stream())
        torch.cuda.synchronize()
        want = R.maxpool_scatter(x.shape, [g], [wi], [k], old=old if acc else None)
        same(dx.get(), bits(want, dt), ("dx", k))
        assert np.array_equal(gd.get(), bits(g, dt)) and np.array_equal(idd.get(), wi)


MULTI = [((2, 32, 32), (2, 4, 8)), ((1, 16, 64), (2, 4, 8)), ((2, 24, 40), (2, 4, 8)), ((2, 24, 48), (2, 3, 8))]      # the first two: shifts and masks


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("dt,Cc", LAYOUTS, ids=LAYOUT_IDS)
def test_maxpool_bwd_multi_scatter(dt, Cc, n, acc):
    """Up to three pooled gradients through the argmax bytes of forward launches of this test, float32 additions old, g[0], g[1], g[2], rounded once.
    Power-of-two shapes, channel groups and windows take the shift-and-mask form (C = 24: three groups, the division form), (2, 24, 40) and the
    window 3 the division form."""
    for (N, H, W), ks in MULTI:
        ks = ks[:n]
        rng = np.random.default_rng(400 + 10 * n + acc + H)
        x = ints(rng, (N, H, W, Cc), -3, 3)
        idxs, gs, keep = [], [], []
        for k in ks:
            y, idx = fwd(x, k, dt)
            wi = idx.get()
            same(wi, R.maxpool_scan(x, k)[1], ("argmax", k))
            g = gauss(rng, wi.shape, dt)
            idxs.append(wi); gs.append(g); keep += [idx, Guarded(bits(g, dt))]
        old = gauss(rng, x.shape, dt)
        dx = Guarded(bits(old, dt))
        dyp = L.ptr_array([keep[2 * u + 1].ptr for u in range(n)])
        ixp = L.ptr_array([keep[2 * u].ptr for u in range(n)])
        ksa = (C.c_int32 * n)(*ks)
        L.lib().call("rua_maxpool_bwd_multi", n, dyp, ixp, ksa, dx.ptr, acc, N, H, W, Cc, dt, stream())
        torch.cuda.synchronize()
        want = R.maxpool_scatter(x.shape, gs, idxs, ks, old=old if acc else None)
        same(dx.get(), bits(want, dt), ("dx", (N, H, W), ks))


def test_maxpool_bwd_past_the_capped_grid():
    """(2, 192, 192, 64) bf16: 589824 pieces against 2048 x 256 threads - the grid wraps once, with a ragged rest."""
    dt, k, shape = L.RUA_BF16, 2, (2, 192, 192, 64)
    rng = np.random.default_rng(5)
    wi = rng.integers(0, 4, (2, 96, 96, 64)).astype(np.uint8)
    g, old = gauss(rng, wi.shape, dt), gauss(rng, shape, dt)
    assert shape[0] * shape[1] * shape[2] * (shape[3] // 8) > 2048 * 256
    gd, idd, dx = Guarded(bits(g, dt)), Guarded(wi), Guarded(bits(old, dt))
    L.lib().call("rua_maxpool_bwd", gd.ptr, idd.ptr, dx.ptr, 1, *shape, k, dt, stream())
    torch.cuda.synchronize()
    same(dx.get(), bits(R.maxpool_scatter(shape, [g], [wi], [k], old=old), dt), "dx")


@pytest.mark.parametrize("dt,Cc", LAYOUTS, ids=LAYOUT_IDS)
def test_sumpool_window_sums(dt, Cc):
    """Integers in [-2, 2]: every partial sum is exact in float32, so the result is the float64 sum rounded once to the storage type."""
    for k in (1, 2, 3, 4, 8, 16):
        for N, H, W in SHAPES:
            if H % k or W % k:
                continue
            x = ints(np.random.default_rng(500 + k), (N, H, W, Cc), -2, 2)
            xd = Guarded(bits(x, dt))
            y = Guarded(np.full((N, H // k, W // k, Cc), QNAN[dt], bit_dtype(dt)))
            L.lib().call("rua_sumpool", xd.ptr, y.ptr, N, H, W, Cc, k, dt, stream())
            torch.cuda.synchronize()
            same(y.get(), bits(R.sumpool(x, k), dt), ("sum", k, (N, H, W)))


@pytest.mark.parametrize("dt,Cc", LAYOUTS, ids=LAYOUT_IDS)
def test_sumpool_pyramid_is_three_window_sums(dt, Cc):
    for N, H, W in [(2, 48, 48), (1, 32, 16), (3, 8, 24)]:
        x = ints(np.random.default_rng(600 + H), (N, H, W, Cc), -2, 2)
        xd = Guarded(bits(x, dt))
        ys = [Guarded(np.full((N, H // k, W // k, Cc), QNAN[dt], bit_dtype(dt))) for k in (2, 4, 8)]
        L.lib().call("rua_sumpool_pyramid", xd.ptr, ys[0].ptr, ys[1].ptr, ys[2].ptr, N, H, W, Cc, dt, stream())
        torch.cuda.synchronize()
        for y, k in zip(ys, (2, 4, 8)):
            same(y.get(), bits(R.sumpool(x, k), dt), ("sum", k, (N, H, W)))


def test_pooling_refusals_leave_the_outputs_alone():
    """What the launchers' host-side checks reject returns non-zero before any launch."""
    lib, dt, Cc = L.lib(), L.RUA_BF16, 8
    rng = np.random.default_rng(9)
    N, H, W = 1, 32, 32
    x = Guarded(bits(ints(rng, (N, H, W, Cc), -3, 3), dt))
    big = np.full((N, H, W, Cc), QNAN[dt], np.uint16)
    y, y2, idx, idx2 = Guarded(big), Guarded(big), Guarded(np.full(big.shape, 0xEE, np.uint8)), Guarded(np.full(big.shape, 0xEE, np.uint8))
    s = stream()
    bad = [
        ("H % k", lib.raw("rua_maxpool_fwd")(x.ptr, y.ptr, idx.ptr, N, H, W, Cc, 3, dt, s)),
        ("k = 17", lib.raw("rua_maxpool_fwd")(x.ptr, y.ptr, idx.ptr, N, 34, 34, Cc, 17, dt, s)),
        ("idx + 4", lib.raw("rua_maxpool_fwd")(x.ptr, y.ptr, idx.ptr + 4, N, H, W, Cc, 2, dt, s)),
        ("C = 12", lib.raw("rua_maxpool_fwd")(x.ptr, y.ptr, idx.ptr, N, H, W, 12, 2, dt, s)),
        ("dtype", lib.raw("rua_maxpool_fwd")(x.ptr, y.ptr, idx.ptr, N, H, W, Cc, 2, 7, s)),
        ("bwd H % k", lib.raw("rua_maxpool_bwd")(x.ptr, idx.ptr, y.ptr, 0, N, H, W, Cc, 3, dt, s)),
        ("bwd idx + 4", lib.raw("rua_maxpool_bwd")(x.ptr, idx.ptr + 4, y.ptr, 0, N, H, W, Cc, 2, dt, s)),
        ("bwd C = 12", lib.raw("rua_maxpool_bwd")(x.ptr, idx.ptr, y.ptr, 0, N, H, W, 12, 2, dt, s)),
        ("derive k_half = 16", lib.raw("rua_maxpool_derive")(x.ptr, idx.ptr, y.ptr, idx2.ptr, N, 2, 2, Cc, 16, dt, s)),
        ("derive odd H_half", lib.raw("rua_maxpool_derive")(x.ptr, idx.ptr, y.ptr, idx2.ptr, N, 3, 4, Cc, 2, dt, s)),
        ("derive idx + 4", lib.raw("rua_maxpool_derive")(x.ptr, idx.ptr, y.ptr, idx2.ptr + 4, N, 4, 4, Cc, 2, dt, s)),
        ("derive idx_half + 4", lib.raw("rua_maxpool_derive")(x.ptr, idx.ptr + 4, y.ptr, idx2.ptr, N, 4, 4, Cc, 2, dt, s)),
        ("derive C = 12", lib.raw("rua_maxpool_derive")(x.ptr, idx.ptr, y.ptr, idx2.ptr, N, 4, 4, 12, 2, dt, s)),
        ("sumpool H % k", lib.raw("rua_sumpool")(x.ptr, y.ptr, N, H, W, Cc, 3, dt, s)),
        ("sumpool C = 12", lib.raw("rua_sumpool")(x.ptr, y.ptr, N, H, W, 12, 2, dt, s)),
        ("pyramid H % 8", lib.raw("rua_sumpool_pyramid")(x.ptr, y.ptr, y2.ptr, y2.ptr, N, 12, 16, Cc, dt, s)),
    ]
    for n, ks in ((4, (2, 2, 2, 2)), (0, ()), (2, (2, 3)), (2, (2, 64))):
        m = max(n, 1)
        dyp, ixp = L.ptr_array([x.ptr] * m), L.ptr_array([idx.ptr] * m)
        ksa = (C.c_int32 * m)(*(ks if ks else (2,)))
        bad.append((f"multi n = {n} ks = {ks}", lib.raw("rua_maxpool_bwd_multi")(n, dyp, ixp, ksa, y.ptr, 0, N, H, W, Cc, dt, s)))
    dyp, ixp, ksa = L.ptr_array([x.ptr]), L.ptr_array([idx.ptr + 4]), (C.c_int32 * 1)(2)
    bad.append(("multi idx + 4", lib.raw("rua_maxpool_bwd_multi")(1, dyp, ixp, ksa, y.ptr, 0, N, H, W, Cc, dt, s)))
    bad.append(("multi C = 12", lib.raw("rua_maxpool_bwd_multi")(1, dyp, L.ptr_array([idx.ptr]), ksa, y.ptr, 0, N, H, W, 12, dt, s)))
    torch.cuda.synchronize()
    assert all(rc != 0 for _, rc in bad), [name for name, rc in bad if rc == 0]
    assert (y.get() == QNAN[dt]).all() and (y2.get() == QNAN[dt]).all() and (idx.get() == 0xEE).all() and (idx2.get() == 0xEE).all()
