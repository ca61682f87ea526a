"""tests/_bn_pool_ref.py against torch-CPU, without a GPU: the float64 BatchNorm formulas against torch autograd through relu(gamma * xhat + beta),
the max-pool scan and its scatter against F.max_pool2d and its autograd on tie-free data, the bf16 rounding against tensor.to(torch.bfloat16).
What torch leaves open (ties, NaN, -inf, the sign of zero) is asserted here as the rule include/rua_hip.h states."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _bn_pool_ref as R

f32, f64 = np.float32, np.float64


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, f64))


def close(a, b, tol=1e-10):
    a, b = np.asarray(a, f64), np.asarray(b, f64)
    return float(np.abs(a - b).max()) <= tol * max(1.0, float(np.abs(b).max()))


def test_bn_forward_and_backward_equal_torch_autograd():
    """Two branches on one input plus a skip gradient: out_b = relu(gamma_b xhat + beta_b); dx, dgamma, dbeta, the moving statistics with the
    Bessel factor, out_stats and the stats2_out conversion."""
    rng = np.random.default_rng(1)
    M, Cc, eps, mom = 257, 24, 1e-3, 0.9
    x = rng.standard_normal((M, Cc)) * 1.5 + 0.3
    gam = [rng.uniform(0.5, 1.5, Cc) * rng.choice([-1.0, 1.0], Cc) for _ in range(2)]
    bet = [rng.standard_normal(Cc) for _ in range(2)]
    g = [rng.standard_normal((M, Cc)) for _ in range(2)]
    dskip = rng.standard_normal((M, Cc))
    mm0, mv0 = rng.standard_normal(Cc), rng.uniform(0.5, 2.0, Cc)

    xt = t64(x).requires_grad_(True)
    gt, bt = [t64(a).requires_grad_(True) for a in gam], [t64(a).requires_grad_(True) for a in bet]
    rm, rv = t64(mm0).clone(), t64(mv0).clone()
    pre = [F.batch_norm(xt, rm if b == 0 else None, rv if b == 0 else None, gt[b], bt[b], training=True, momentum=1.0 - mom, eps=eps) for b in range(2)]
    loss = sum((torch.relu(pre[b]) * t64(g[b])).sum() for b in range(2)) + (xt * t64(dskip)).sum()
    loss.backward()

    mean, var = R.bn_moments(x.sum(0), (x * x).sum(0), float(M))
    assert close(mean, x.mean(0)) and close(var, x.var(0))
    nmm, nmv = R.bn_moving(mm0, mv0, mean, var, mom, float(M))
    assert close(nmm, rm.numpy()) and close(nmv, rv.numpy())
    As, Bs, Cs, masks = [], [], [], []
    for b in range(2):
        scale, shift, rstd = R.bn_coeffs(mean, var, gam[b], bet[b], eps)
        out = R.bn_apply(x, scale, shift, relu=False)
        assert close(out, pre[b].detach().numpy())
        assert close(R.bn_apply(x, scale, shift, relu=True), torch.relu(pre[b]).detach().numpy())
        o1, o2 = R.bn_out_stats(float(M), bet[b], scale, var)
        assert close(o1, out.sum(0), 1e-9) and close(o2, (out * out).sum(0), 1e-9)
        m = R.relu_mask(x, scale, shift)
        assert (m == (pre[b].detach().numpy() > 0)).all()
        sg, sgx = (g[b] * m).sum(0), (g[b] * m * x).sum(0)
        assert close(R.stats2_from_out(sg, (g[b] * m * out).sum(0), scale, shift, mean), sgx, 1e-9)
        A, B, Cc_, dga, dbe = R.bn_bwd_coeffs(sg, sgx, float(M), gam[b], mean, rstd)
        assert close(dga, gt[b].grad.numpy(), 1e-9) and close(dbe, bt[b].grad.numpy(), 1e-9)
        As.append(A); Bs.append(B); Cs.append(Cc_); masks.append(m)
    dx, T = R.bn_bwd_apply(x, g, As, masks, sum(Bs), sum(Cs), dskip=dskip)
    assert close(dx, xt.grad.numpy(), 1e-9)
    assert (T >= np.abs(dx) * (1 - 1e-12)).all()
    old = rng.standard_normal((M, Cc))
    dx2, _ = R.bn_bwd_apply(x, g, As, masks, sum(Bs), sum(Cs), dskip=dskip, old=old)
    assert close(dx2, xt.grad.numpy() + old, 1e-9)
    dx3, _ = R.bn_bwd_apply(x, g, As, [None, None], sum(Bs), sum(Cs))
    assert close(dx3, sum(Bs) * x + sum(Cs) + As[0] * g[0] + As[1] * g[1], 1e-12)


def test_bn_edges_of_the_formulas():
    """bessel_n = 1 leaves the variance biased; a constant channel clamps at 0 and rstd = 1 / sqrt(eps); scale == 0 in the stats2_out conversion."""
    mean, var = R.bn_moments(np.array([3000.0]), np.array([3.0e6]), 3.0)
    assert mean[0] == 1000.0 and var[0] == 0.0
    _, _, rstd = R.bn_coeffs(mean, var, np.ones(1), np.zeros(1), f32(1e-3))
    assert rstd[0] == 1.0 / np.sqrt(f64(f32(1e-3)))
    assert R.bn_moments(np.array([1.0]), np.array([0.5]), 1.0)[1][0] == 0.0           # a negative difference clamps
    mm, mv = R.bn_moving(np.zeros(1), np.ones(1), np.array([2.0]), np.array([4.0]), 0.5, 1.0)
    assert mm[0] == 1.0 and mv[0] == 2.5
    mm, mv = R.bn_moving(np.zeros(1), np.ones(1), np.array([2.0]), np.array([4.0]), 0.5, 5.0)
    assert mv[0] == 0.5 + 0.5 * 5.0
    assert R.stats2_from_out(np.array([2.0]), np.array([7.0]), np.array([0.0]), np.array([1.0]), np.array([3.0]))[0] == 6.0


def tie_free(rng, shape):
    n = int(np.prod(shape))
    return (rng.permutation(n).astype(f64) - n // 2).reshape(shape) / 8.0


@pytest.mark.parametrize("k", [1, 2, 3, 4, 8, 16])
def test_maxpool_scan_and_scatter_equal_torch(k):
    rng = np.random.default_rng(k)
    N, H, W, Cc = 2, 2 * k * 2, 3 * k, 5
    x = tie_free(rng, (N, H, W, Cc))
    xt = t64(x).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    yt, it = F.max_pool2d(xt, k, return_indices=True)
    y, idx = R.maxpool_scan(x, k)
    assert np.array_equal(y, yt.detach().permute(0, 2, 3, 1).numpy())
    flat = it.permute(0, 2, 3, 1).numpy()                                       # index into the H x W plane
    pos = (flat // W % k) * k + flat % W % k
    assert np.array_equal(idx, pos.astype(np.uint8))
    g = rng.integers(-8, 9, y.shape).astype(f64)
    (yt * t64(g).permute(0, 3, 1, 2)).sum().backward()
    want = xt.grad.permute(0, 2, 3, 1).numpy()
    assert np.array_equal(R.maxpool_scatter(x.shape, [g], [idx], [k]), want.astype(f32))
    old = rng.integers(-8, 9, x.shape).astype(f32)
    assert np.array_equal(R.maxpool_scatter(x.shape, [g], [idx], [k], old=old), (want + old).astype(f32))
    assert np.array_equal(R.sumpool(x, k), F.avg_pool2d(xt.detach(), k).permute(0, 2, 3, 1).numpy() * (k * k))


def test_maxpool_scatter_of_several_windows_is_the_sum_of_the_single_ones():
    rng = np.random.default_rng(3)
    shape = (2, 24, 40, 4)
    x = tie_free(rng, shape)
    ks = (2, 4, 8)
    got = [R.maxpool_scan(x, k) for k in ks]
    gs = [rng.integers(-8, 9, y.shape).astype(f32) for y, _ in got]
    old = rng.integers(-8, 9, shape).astype(f32)
    want = old + sum(R.maxpool_scatter(shape, [g], [i], [k]) for g, (_, i), k in zip(gs, got, ks))
    assert np.array_equal(R.maxpool_scatter(shape, gs, [i for _, i in got], ks, old=old), want)


@pytest.mark.parametrize("kh", [1, 2, 4, 8])
def test_maxpool_derive_equals_the_direct_scan(kh):
    """Tie-free data and small integers (ties everywhere): the 2k pool derived from the k pool is the direct 2k scan, values and bytes."""
    rng = np.random.default_rng(10 + kh)
    shape = (2, 4 * kh, 6 * kh, 3)
    for x in (tie_free(rng, shape), rng.integers(-3, 4, shape).astype(f64)):
        yh, ih = R.maxpool_scan(x, kh)
        y, i = R.maxpool_derive(yh, ih, kh)
        yd, idd = R.maxpool_scan(x, 2 * kh)
        assert np.array_equal(y, yd) and np.array_equal(i, idd)


def test_maxpool_rule_on_special_windows():
    """All equal -> byte 0; only -inf, only NaN, NaN with -inf -> -inf and byte 0; NaN beside finite values never wins; -0.0 before +0.0 stays -0.0
    at the first position; the derived form agrees on every one of them."""
    nan, inf = np.nan, np.inf
    wins = [[5, 5, 5, 5], [-inf] * 4, [nan] * 4, [nan, -inf, nan, -inf], [nan, 1, 2, nan], [nan, nan, nan, -7], [-0.0, 0.0, 0.0, -0.0],
            [0.0, -0.0, -0.0, 0.0], [-inf, -inf, -inf, -1e30]]
    x = np.array(wins, f32).reshape(len(wins), 2, 2, 1).transpose(3, 1, 0, 2).reshape(1, 2, 2 * len(wins), 1)
    y, i = R.maxpool_scan(x, 2)
    y, i = y.reshape(-1), i.reshape(-1)
    assert list(i) == [0, 0, 0, 0, 2, 3, 0, 0, 3]
    want = np.array([5, -inf, -inf, -inf, 2, -7, -0.0, 0.0, -1e30], f32)
    assert np.array_equal(y.view(np.uint32), want.view(np.uint32))
    big = np.tile(x, (1, 2, 2, 1))                                              # 4 x 4 windows made of these 2 x 2 ones
    yh, ih = R.maxpool_scan(big, 2)
    yd, idd = R.maxpool_derive(yh, ih, 2)
    y4, i4 = R.maxpool_scan(big, 4)
    assert np.array_equal(yd.view(np.uint32), y4.view(np.uint32)) and np.array_equal(idd, i4)


def test_bf16_rounding_equals_torch():
    """Every class: random values, every tie and its neighbours around a few exponents, the carry into the exponent, overflow to Inf, subnormals."""
    rng = np.random.default_rng(7)
    hi = np.concatenate([np.arange(0x3F00, 0x4100), np.arange(0x7F00, 0x7F81), np.arange(0x0000, 0x0100), np.arange(0xBF00, 0xC000)]).astype(np.uint32) << 16
    u = np.concatenate([hi | lo for lo in (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF)] + [(rng.standard_normal(4096) * 3).astype(f32).view(np.uint32)])
    u = u[~np.isnan(u.astype(np.uint32).view(f32))]
    a = u.astype(np.uint32).view(f32)
    want = torch.from_numpy(a.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(R.bf16_bits(a), want)
    assert np.array_equal(R.bf16_value(want), torch.from_numpy(a.copy()).to(torch.bfloat16).float().numpy())
    assert np.array_equal(R.round_storage(a.astype(f64), True).view(np.uint32) >> 16, want.astype(np.uint32))
    q = R.bf16_bits(np.array([np.nan, -np.nan], f32))
    assert np.isnan(R.bf16_value(q)).all()
