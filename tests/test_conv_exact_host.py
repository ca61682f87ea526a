"""The preconditions of the exact-arithmetic convolution tests (tests/test_conv_exact_gpu.py), on the float64 references alone - no GPU, no library call.

For every case of the tables in tests/_exact_util.py: the stored outputs are integers within +-256 (bf16 holds them), the fp32 accumulators stay below 2**24,
the outputs take >= 50 distinct values, no pixel can drop out of a weight gradient or of the statistics unseen.  And the point of the exercise: mutants of the
reference that the tolerance tests of tests/test_kernels_gpu.py let through (a column left out of the statistics, a pixel left out of dW, eight channels of one
tap misread at one edge pixel) compare UNEQUAL here."""
import numpy as np
import pytest
import torch

import _exact_util as X


@pytest.mark.parametrize("c", X.FWD_CASES + X.CHAIN_CASES, ids=[c.name for c in X.FWD_CASES + X.CHAIN_CASES])
def test_forward_case_preconditions(c):
    X.check_fwd_preconditions(c, X.fwd_case(c))


WG_ALL = X.WG_CASES + [m for g in X.WG_GROUPS for m in g.members]


@pytest.mark.parametrize("c", WG_ALL, ids=[c.name for c in WG_ALL])
def test_wgrad_case_preconditions(c):
    X.check_wg_preconditions(c, X.wg_case(c))


@pytest.mark.parametrize("c", X.SUM_CASES + X.GROUP_CASES, ids=[c.name for c in X.SUM_CASES + X.GROUP_CASES])
def test_band_case_preconditions(c):
    X.check_band_preconditions(c, X.band_case(c))


def test_case_names_are_unique_and_tables_cover_every_route():
    names = [c.name for c in X.FWD_CASES + X.CHAIN_CASES + X.WG_CASES + X.SUM_CASES + X.GROUP_CASES + X.WG_GROUPS + [m for g in X.WG_GROUPS for m in g.members]]
    assert len(names) == len(set(names))
    assert {c.kid for c in X.FWD_CASES} == set(range(10))                      # conv_igemm .. conv_img2 and conv_band128m as a sum
    assert {(c.kind, c.img) for c in X.WG_CASES} == {(0, 0), (0, 1), (0, 2), (1, 0), (2, 0), (3, 0)}
    for c in X.FWD_CASES:                                                       # every route runs the residual + statistics and the ReLU-mask + statistics epilogue
        if c.epi == "res":
            assert any(o.name == c.name[:-3] + "mask" for o in X.FWD_CASES) or c.norm, c.name


def test_references_agree_with_autograd():
    """the per-tap matrix products of wgrad_ref against the gradient PyTorch derives from conv_ref's convolution; strides, dilation, both kernel sizes"""
    rng = np.random.default_rng(5)
    for (N, Hs, Ws, Cs, Cout, stride, dil, taps) in [(2, 9, 7, 8, 16, 1, 2, 9), (1, 8, 12, 16, 8, 2, 1, 1), (2, 6, 6, 8, 8, 1, 7, 9)]:
        a, dy = X.ternary(rng, (N, Hs, Ws, Cs), 0.6), X.ternary(rng, (N, Hs // stride, Ws // stride, Cout), 0.6)
        k = 3 if taps == 9 else 1
        w = torch.zeros((Cout, Cs, k, k), dtype=torch.float64, requires_grad=True)
        y = torch.nn.functional.conv2d(torch.from_numpy(a).double().permute(0, 3, 1, 2), w, None, stride=stride, padding=dil * (k // 2), dilation=dil)
        y.backward(torch.from_numpy(dy).double().permute(0, 3, 1, 2))
        exp = w.grad.permute(2, 3, 0, 1).reshape(taps, Cout, Cs).numpy()
        assert np.array_equal(X.wgrad_ref(a, dy, dil, taps, stride), exp)


# ------------------------------------------------------------------------------------------------------------ sensitivity (precondition 4)
def rel_err(got, exp):
    """the measure of tests/test_kernels_gpu.py: largest absolute error over largest absolute value"""
    got = np.asarray(got, np.float64); exp = np.asarray(exp, np.float64)
    return float(np.abs(got - exp).max() / (np.abs(exp).max() + 1e-12))


def bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).float().numpy()


def stats_without_last_column(y):
    v = y[:, :, :-1, :]
    return np.stack([v.sum(axis=(0, 1, 2)), (v * v).sum(axis=(0, 1, 2))])


def misread_tap(x, w, y, dil):
    """y with channels 0..7 of the centre-row left tap at the edge pixel (0, H/2, W-1) read from the pixel one row further down instead"""
    H, W = y.shape[1], y.shape[2]
    h, wq = H // 2, W - 1
    t, hh, ww = 3, h, wq - dil                                                 # tap (ky, kx) = (1, 0): the pixel dil to the left
    assert ww >= 0 and hh + 1 < H
    out = y.copy()
    out[0, h, wq, :] += w[t][:, :8].astype(np.float64) @ (x[0, hh + 1, ww, :8].astype(np.float64) - x[0, hh, ww, :8].astype(np.float64))
    return out


FWD_SENS = next(c for c in X.FWD_CASES if c.name == "strip-1x256x256-d1-bf16-res")        # 1 x 256 x 256, C = 32: the first row of the issue's table
WG_SENS = next(c for c in X.WG_CASES if c.name == "rows32-8x16x256x32-r127")


def test_exact_comparison_catches_what_the_tolerances_let_through():
    # --- exact data: every mutant is unequal
    c, d = FWD_SENS, X.fwd_case(FWD_SENS)
    y, st = d["y"], d["stats"]
    mut = stats_without_last_column(y)
    assert X.mismatch(mut[0], st[0], "sum v", "-", "(c,)") and X.mismatch(mut[1], st[1], "sum v^2", "-", "(c,)")
    assert (mut[0] != st[0]).sum() >= c.Cout - 2                               # not by a channel or two: nearly every channel's sum moves
    ymut = misread_tap(d["x"][0], d["w"][0], y, c.segs[0][2])
    msg = X.mismatch(ymut, y, "y", "host", "(n, h, w, c)")
    assert msg and f"(0, {c.H // 2}, {c.W - 1}," in msg and "route: host" in msg
    g, gd = WG_SENS, X.wg_case(WG_SENS)
    dy = gd["dy"].copy()
    dy[0, 0, 0, :] = 0                                                         # the corner pixel contributes nothing
    gmut = X.wgrad_ref(gd["a"], dy, g.dil, g.taps, g.stride) + gd["base"]
    assert X.mismatch(gmut, gd["dw"], "dW", "host", "(tap, co, c)")
    # a pixel counted twice
    dy[0, 0, 0, :] = 2 * gd["dy"][0, 0, 0, :]
    assert X.mismatch(X.wgrad_ref(gd["a"], dy, g.dil, g.taps, g.stride) + gd["base"], gd["dw"], "dW", "host", "(tap, co, c)")

    # --- the same mutants on the Gaussian data of tests/test_kernels_gpu.py stay under that file's bounds (tol = 2e-2 for bf16: 5 * tol + 1e-4 for the statistics,
    # 2e-2 for the weight gradients of the generic, wgrad_dmap, wgrad_pw and whole-image kernels): the gap this file closes
    rng = np.random.default_rng(1)
    N, H, W, Cs = 1, 256, 256, 32
    x = bf16(rng.standard_normal((N, H, W, Cs)))
    w = bf16(rng.standard_normal((9, Cs, Cs)) / np.sqrt(9 * Cs))
    bias = rng.standard_normal(Cs).astype(np.float32)
    res = bf16(rng.standard_normal((N, H, W, Cs)))
    yg = X.conv_ref(x, w, 1, 9) + bias.astype(np.float64) + res
    sg, sm = np.stack([yg.sum(axis=(0, 1, 2)), (yg * yg).sum(axis=(0, 1, 2))]), stats_without_last_column(yg)
    e1, e2 = rel_err(sm[0], sg[0]), rel_err(sm[1], sg[1])
    ey = rel_err(misread_tap(x, w, yg, 1), yg)
    a, dyg = bf16(rng.standard_normal((N, H, W, Cs))), bf16(rng.standard_normal((N, H, W, Cs)))
    gg = X.wgrad_ref(a, dyg, 1, 9)
    dyg[0, 0, 0, :] = 0
    eg = rel_err(X.wgrad_ref(a, dyg, 1, 9), gg)
    print(f"Gaussian 1x256x256x32: last column out of the statistics: sum v {e1:.4f}, sum v^2 {e2:.4f} (bound 0.1001 / 0.10); corner pixel out of dW {eg:.4f} "
          f"(bound 2e-2); eight channels of one tap misread at an edge pixel {ey:.4f} (bound 2e-2)")
    assert 0 < e1 < 5 * 2e-2 + 1e-4 and 0 < e2 < 5 * 2e-2
    assert 0 < eg < 2e-2
    assert ey > 0                                                              # (at the bound, above or below it by the draw: 0.02 .. 0.05 - reported, not asserted)
