"""The float64 references of tests/_loss_ref.py against the oracle, and why tests/test_loss_chain_gpu.py compares the way it does - no GPU, no library
call.

1. finalize(moments()) followed by dz() against torch float64 autograd of oracle/resuneta_ref.py::tanimoto_dual_loss, and the single form against
   oracle/naive_ops.py::tanimoto_loss.  The oracle is float64, so its weight 1 / V^2 is infinite only at V == 0; these inputs keep every V far from
   the float32 window, where the two rules agree.
2. The infinite-weight rule against the oracle evaluated in float32 at V in {0, 1e-21, 2e-19}: the first two overflow, 2e-19 does not.  Nothing is
   placed between 5e-20 and 1.2e-19, where the answer depends on whether denormals are flushed.
3. Faults that allclose(rtol=2e-5, atol=1e-3) on the moments lets through - a pixel left out, a mask byte read from the neighbour of its group -
   compare unequal on the data of the exact tests (multiples of 1/8), and an fp32 accumulation of that data in any order is the float64 sum."""
import numpy as np
import pytest
import torch

import _loss_ref as R
from oracle import naive_ops as nv
from oracle import resuneta_ref as ref

f32, f64 = np.float32, np.float64


def activations(rng, B, HW, C, act):
    z = rng.standard_normal((B, HW, C)) * 2
    zt = torch.from_numpy(z).requires_grad_(True)
    return zt, (torch.softmax(zt, -1) if act == R.ACT_SOFTMAX else torch.sigmoid(zt))


def nchw(t, H, W):
    return t.reshape(t.shape[0], H, W, t.shape[-1]).permute(0, 3, 1, 2)


@pytest.mark.parametrize("act", [R.ACT_SOFTMAX, R.ACT_SIGMOID], ids=["softmax", "sigmoid"])
@pytest.mark.parametrize("C", [1, 3, 6, 8])
@pytest.mark.parametrize("B", [1, 3, 70])
def test_finalize_and_dz_against_autograd_of_the_oracle(B, C, act):
    rng = np.random.default_rng([B, C, act, 1])
    H, W, wgt = 3, 4, 0.7
    HW = H * W
    zt, pt = activations(rng, B, HW, C, act)
    y = rng.random((B, HW, C))
    per_t = ref.tanimoto_dual_loss(nchw(torch.from_numpy(y), H, W), nchw(pt, H, W))
    (wgt * per_t.mean()).backward()
    p = pt.detach().numpy()
    fin = R.finalize(R.moments(p, y, np.ones((B, HW), bool)), B, C, wgt / B)
    assert not fin.replaced1.any() and not fin.replaced2.any()
    per = per_t.detach().numpy()
    assert np.abs(fin.per_sample - per).max() <= 1e-12 * np.abs(per).max()
    assert abs(fin.loss - per.mean()) <= 1e-12 * abs(per.mean())
    got, scale = R.dz(R.TANIMOTO, act, p, y, coef=fin.coef, with_scale=True)
    want = zt.grad.numpy()
    assert np.abs(got - want).max() <= 1e-10 * scale.max(), np.abs(got - want).max() / scale.max()
    assert (fin.coef_mag >= np.abs(fin.coef) * (1 - 1e-12)).all()


@pytest.mark.parametrize("C", [1, 3, 6, 8])
@pytest.mark.parametrize("B", [1, 3, 70])
def test_single_form_against_naive_ops(B, C):
    rng = np.random.default_rng([B, C, 2])
    H, W = 3, 4
    label, pred = rng.random((B, H, W, C)), rng.random((B, H, W, C))
    want = nv.tanimoto_loss(label, pred)
    # Tanimoto_loss(label, pred): the weights come from the volumes of its FIRST argument, so the moments are taken with p := label, y := pred
    fin = R.finalize(R.moments(label.reshape(B, H * W, C), pred.reshape(B, H * W, C), np.ones((B, H * W), bool)), B, C, 0.0, single=True)
    assert fin.coef is None
    assert np.abs(fin.per_sample - want).max() <= 1e-12 * np.abs(want).max()
    assert abs(fin.loss - want.mean()) <= 1e-12 * abs(want.mean())


@pytest.mark.parametrize("V,infinite", [(0.0, True), (1e-21, True), (2e-19, False)])
def test_infinite_weight_rule_is_the_float32_one(V, infinite):
    """Class 1 of three has the volume V; the oracle runs in float32 as the reference model does."""
    rng = np.random.default_rng(3)
    B, H, W, C = 2, 2, 2, 3
    label = (rng.integers(1, 5, (B, H * W, C)) / 8).astype(f32)
    pred = (rng.integers(1, 5, (B, H * W, C)) / 8).astype(f32)
    label[:, :, 1] = 0
    label[:, 0, 1] = f32(V)                                                    # one pixel per sample holds the whole volume: mean over the samples = V
    assert not (5e-20 <= V <= 1.2e-19)
    assert bool(R.weight_is_infinite(np.array([V]))[0]) == infinite
    lt, pt = nchw(torch.from_numpy(label), H, W), nchw(torch.from_numpy(pred), H, W)
    assert lt.dtype == torch.float32
    vli = lt.sum(dim=(2, 3)).mean(dim=0)
    assert bool(torch.isinf(1.0 / vli ** 2)[1]) == infinite                    # what tanimoto_loss does first
    want = ref.tanimoto_loss(lt, pt).numpy()
    assert np.isfinite(want).all()
    fin = R.finalize(R.moments(label, pred, np.ones((B, H * W), bool)), B, C, 0.0, single=True)
    assert bool(fin.replaced1[1]) == infinite and not fin.replaced1[[0, 2]].any()
    assert np.abs(fin.per_sample - want).max() <= 1e-5 * np.abs(want).max()
    if infinite:
        assert fin.w1[1] == max(fin.w1[0], fin.w1[2])
    if V == 1e-21:
        # the rule "infinite only at V^2 == 0" keeps 1 / V^2 = 1e42 (finite in float64): class 1 then outweighs the others by 40 orders of magnitude
        # and the value moves far outside what float32 can blur
        s = R.moments(label, pred, np.ones((B, H * W), bool))
        w = np.array([fin.w1[0], 1.0 / (float(f32(V)) ** 2), fin.w1[2]])
        wrong = ((w * s[:, :, 2]).sum(1) + 1e-5) / ((w * (s[:, :, 3] - s[:, :, 2])).sum(1) + 1e-5)
        assert np.abs(wrong - want).max() > 0.1 * np.abs(want).max()


def test_all_weights_infinite_become_zero():
    w, inf = R.class_weights(np.array([0.0, 1e-21, 0.0]))
    assert inf.all() and not w.any()


# ---- what the exact comparison sees and the old tolerance does not ---------------------------------------------------------------
def emulated_sums(p, y, keep, order=None):
    """A host model of the kernels' accumulation: every term in float32, a block's 1024 pixels (taken in `order` if given) summed in float32 one
    after the other, the blocks' sums added in float64."""
    K = keep[:, :, None]
    a, l = p.astype(f32), y.astype(f32)
    q, m = f32(1) - a, f32(1) - l
    cols = [a, m, a * l, a * a + l * l, q * m, q * q + m * m]
    out = []
    for t in cols:
        t = np.where(K, t, f32(0))
        if order is not None:
            t = t[:, order]
        B, HW, C = t.shape
        pad = -HW % 1024
        t = np.concatenate([t, np.zeros((B, pad, C), f32)], axis=1).reshape(B, -1, 1024, C)
        blocks = np.cumsum(t, axis=2, dtype=f32)[:, :, -1]
        assert blocks.dtype == f32
        out.append(blocks.astype(f64).sum(1))
    return np.stack(out, axis=-1)


def neighbour_mask(keep, G):
    """A kernel that reads the mask byte of pixel g of a group of G from pixel (g + 1) % G."""
    B, HW = keep.shape
    return np.roll(keep.reshape(B, HW // G, G), -1, axis=2).reshape(B, HW)


def dyadic(rng, shape):
    return (rng.integers(0, 9, shape) / 8).astype(f32)


def test_fp32_sums_of_eighths_are_exact_in_any_order():
    rng = np.random.default_rng(4)
    B, HW, C = 1, 70000, 3
    assert 128 * HW < 2 ** 24
    p, y = dyadic(rng, (B, HW, C)), dyadic(rng, (B, HW, C))
    keep = np.ones((B, HW), bool)
    want = R.moments(p, y, keep)
    assert np.array_equal(emulated_sums(p, y, keep), want)
    assert np.array_equal(emulated_sums(p, y, keep, rng.permutation(HW)), want)


def test_the_old_tolerance_misses_a_dropped_pixel_and_a_neighbours_mask_byte():
    rng = np.random.default_rng(5)
    old = dict(rtol=2e-5, atol=1e-3)
    B, HW, C = 1, 400000, 2
    z = rng.standard_normal((B, HW, C)) * 2
    z[0, 777] = [9.0, -9.0]
    e = np.exp(z - z.max(-1, keepdims=True))
    p = (e / e.sum(-1, keepdims=True)).astype(f32)
    y = np.eye(C, dtype=f32)[rng.integers(0, C, (B, HW))]
    assert p[0, 777, 1] < 1e-3
    keep = np.ones((B, HW), bool)
    want = R.moments(p, y, keep)
    assert np.allclose(emulated_sums(p, y, keep), want, **old)
    dropped = keep.copy()
    dropped[0, 777] = False                                                   # the fault: one pixel never reaches the sums
    assert np.allclose(emulated_sums(p, y, dropped), want, **old)             # ... and the old comparison passes
    one_void = keep.copy()
    one_void[0, 1000] = False
    want_v = R.moments(p, y, one_void)
    assert np.allclose(emulated_sums(p, y, neighbour_mask(one_void, 2)), want_v, **old)
    # the same faults on the data of the exact tests
    HWx = 36868
    assert 128 * HWx < 2 ** 24
    px, yx = dyadic(rng, (B, HWx, C)), dyadic(rng, (B, HWx, C))
    keepx = np.ones((B, HWx), bool)
    wantx = R.moments(px, yx, keepx)
    assert np.array_equal(emulated_sums(px, yx, keepx), wantx)
    for i in (0, 777, HWx - 1):
        d = keepx.copy()
        d[0, i] = False
        assert not np.array_equal(emulated_sums(px, yx, d), wantx), i
    per_group = keepx.copy()
    per_group[0, rng.integers(0, 2, HWx // 2) + 2 * np.arange(HWx // 2)] = False      # exactly one void pixel in every group of two
    wantg = R.moments(px, yx, per_group)
    assert np.array_equal(emulated_sums(px, yx, per_group), wantg)
    assert not np.array_equal(emulated_sums(px, yx, neighbour_mask(per_group, 2)), wantg)


def test_counts_take_the_first_maximum_and_a_strict_half():
    p = np.array([[0.5, 0.5, 0.25], [0.25, 0.75, 0.75], [0.125, 0.125, 0.125]], f32)
    y = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]], f32)
    # argmax p: 0, 1, 0; argmax y: 1, 2, 0 -> one hit.  p > .5: row 1 twice; y > .5: once per row
    assert R.metric_counts(p, y, np.ones(3, bool)).tolist() == [1.0, 1.0, 1.0, 5.0, 2.0]
    assert R.metric_counts(p, y, np.array([False, False, True])).tolist() == [1.0, 0.0, 0.0, 2.0, 1.0]


@pytest.mark.parametrize("kind,act", [(R.WCE, R.ACT_SOFTMAX), (R.CE_LOGITS, R.ACT_SOFTMAX), (R.BCE_LOGITS, R.ACT_SIGMOID), (R.MSE, R.ACT_SOFTMAX),
                                      (R.MSE, R.ACT_SIGMOID)])
def test_plain_losses_and_their_dz_against_autograd_of_the_oracle(kind, act):
    rng = np.random.default_rng([kind, act, 6])
    B, H, W, C, wgt = 2, 3, 4, 5, 0.7
    HW, M = H * W, B * H * W
    zt, pt = activations(rng, B, HW, C, act)
    y = rng.random((B, HW, C))
    cw = np.array([4.3, 2.9, 3.9, 5.6, 37.0])
    yt, pn, zn = nchw(torch.from_numpy(y), H, W), nchw(pt, H, W), nchw(zt, H, W)
    if kind == R.WCE:
        lt = -(yt * torch.log(torch.clamp(pn / pn.sum(1, keepdim=True), float(R.EPS32), float(R.ONE_M_EPS32))) * torch.from_numpy(cw)[None, :, None, None]).sum(1)
    elif kind == R.CE_LOGITS:
        lt = ref.categorical_ce_logits(yt, zn)
    elif kind == R.BCE_LOGITS:
        lt = ref.binary_ce_logits(yt, zn)
    else:
        lt = ref.mse(yt, pn)
    (wgt * lt.mean()).backward()
    p = pt.detach().numpy()
    got = R.pixel_loss(kind, p.reshape(M, C), zt.detach().numpy().reshape(M, C), y.reshape(M, C), cw)
    want = lt.detach().numpy().reshape(M)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    g, scale = R.dz(kind, act, p, y, cw=cw, grad_scale=wgt / M, with_scale=True)
    assert np.abs(g - zt.grad.numpy()).max() <= 1e-10 * scale.max()
