"""GPU tests of training on partly labelled patches: rua_void_mask bit for bit against labels.host_void_mask, the masked loss kernels
(fused head forward on every dispatch path, stand-alone sums / pixel losses / metrics / dz) against the unmasked kernels run on the
compacted valid pixels and against the fp64 oracle, and the engine with LossSpec.ignore_void through keras_api.Model."""
import ctypes as C

import numpy as np
import pytest
import torch

from resunet_a_mltsk_keras_amd import _lib as L
from resunet_a_mltsk_keras_amd import compact, labels, scenes

from _scene_util import GUARD, HEADS, NCLS, SHAPE, blob_pool, new_training_model, state
from test_scenes_gpu import compare_with_twins

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda", 0)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev())


def u8(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint8)).to(dev())


def rel_err(got, exp):
    got = np.asarray(got, np.float64); exp = np.asarray(exp, np.float64)
    return float(np.abs(got - exp).max() / (np.abs(exp).max() + 1e-12))


# ---- 1. rua_void_mask ------------------------------------------------------------------------------------------------------------
def void_case(H, W, seed, Cc=4):
    """Three patches: void corners, the whole last row of patch 0 void (patch 1's first rows must not see it), sparse void bytes of the
    values C, 200 and 255."""
    rng = np.random.default_rng(seed)
    cls = rng.integers(0, Cc, (3, H, W)).astype(np.uint8)
    cls[0, 0, 0], cls[0, 0, W - 1], cls[1, H - 1, 0], cls[1, H - 1, W - 1] = Cc, 200, 255, Cc
    cls[0, H - 1, :] = 255
    for v in (Cc, 200, 255):
        cls[2][rng.random((H, W)) < 0.01] = v
    return cls


def run_void_mask(cls, Cc, margin, shift=0):
    """rua_void_mask into a pattern-filled buffer `shift` bytes off its allocation, with guard bytes in front of and behind the output."""
    n = cls.size
    src = torch.full((n + 8,), 0, dtype=torch.uint8, device=dev())
    src[shift:shift + n] = u8(cls).reshape(-1)
    out = torch.full((GUARD + n + GUARD,), 0xA5, dtype=torch.uint8, device=dev())
    N, H, W = cls.shape
    L.lib().call("rua_void_mask", src.data_ptr() + shift, N, H, W, Cc, margin, out.data_ptr() + GUARD + shift, stream())
    torch.cuda.synchronize()
    g = out.cpu().numpy()
    assert (g[:GUARD + shift] == 0xA5).all() and (g[GUARD + shift + n:] == 0xA5).all(), "bytes around the mask were written"
    return g[GUARD + shift:GUARD + shift + n].reshape(cls.shape)


@pytest.mark.parametrize("H,W", [(5, 7), (33, 64), (64, 61)])
@pytest.mark.parametrize("margin", [0, 1, 2, 8])
def test_void_mask_bitwise(H, W, margin):
    cls = void_case(H, W, H * 100 + W)
    want = labels.host_void_mask(cls, 4, margin)
    for shift in (0, 1):                                       # the mask has no alignment of its own
        assert np.array_equal(run_void_mask(cls, 4, margin, shift), want), shift
    valid = np.random.default_rng(1).integers(0, 4, (3, H, W)).astype(np.uint8)
    assert not run_void_mask(valid, 4, margin).any()
    assert (run_void_mask(np.full((3, H, W), 4, np.uint8), 4, margin) == 255).all()
    assert want.any() and (margin >= 5 or not want.all())


def test_void_mask_limits():
    fn = L.lib().raw("rua_void_mask")
    a = torch.zeros(64, dtype=torch.uint8, device=dev())
    p = a.data_ptr()
    ok = (p, 1, 4, 4, 4, 2, p + 32)
    for i, bad in ((2, 0), (2, 513), (3, 0), (3, 513), (4, 0), (4, 256), (5, -1), (5, 17), (1, 0)):
        args = list(ok)
        args[i] = bad
        assert fn(*args, None) != 0, (i, bad)
    assert fn(p, 8192, 512, 512, 4, 2, p + 32, None) != 0      # N*H*W = 2^31
    assert fn(None, 1, 4, 4, 4, 2, p + 32, None) != 0 and fn(p, 1, 4, 4, 4, 2, None, None) != 0


# ---- helpers of the kernel-level tests -----------------------------------------------------------------------------------------------
def random_void(rng, B, HW, share=0.3, all_void=None):
    """[B][HW] bool, about `share` void, a different number per sample; sample `all_void` entirely void."""
    v = np.stack([rng.random(HW) < share * (0.6 + 0.4 * n) for n in range(B)])
    if all_void is not None:
        v[all_void] = True
    assert len({int(x.sum()) for x in v}) == B
    return v


def sums_of_valid(p, y, void, Cc):
    """rua_tanimoto_sums (the unmasked kernel) with B = 1 on each sample's compacted valid pixels: [B][C][6] (zeros for a sample without any)."""
    B = void.shape[0]
    out = np.zeros((B, Cc, 6))
    for n in range(B):
        keep = torch.from_numpy(~void[n]).to(dev())
        K = int(keep.sum())
        if K == 0:
            continue
        pc, yc = p[n][keep].contiguous(), y[n][keep].contiguous()
        s = torch.zeros(Cc * 6, dtype=torch.float64, device=dev())
        L.lib().call("rua_tanimoto_sums", pc.data_ptr(), yc.data_ptr(), 1, K, Cc, s.data_ptr(), stream())
        torch.cuda.synchronize()
        out[n] = s.cpu().numpy().reshape(Cc, 6)
    return out


def metrics_of_valid(p, y, void):
    p, y = p.cpu().numpy()[~void], y.cpu().numpy()[~void]
    t, q = y > 0.5, p > 0.5
    return np.array([(p.argmax(1) == y.argmax(1)).sum(), (t & q).sum(), (~t & q).sum(), (~t & ~q).sum(), (t & ~q).sum()], np.float64)


# ---- 2. the fused head forward, every dispatch path -------------------------------------------------------------------------------------
@pytest.mark.parametrize("all_void", [None, 1])
@pytest.mark.parametrize("dt,Cin,Cout,act", [(L.RUA_BF16, 32, 6, L.ACT_SOFTMAX), (L.RUA_BF16, 32, 3, L.ACT_SIGMOID), (L.RUA_F32, 32, 6, L.ACT_SOFTMAX),
                                             (L.RUA_BF16, 64, 5, L.ACT_SOFTMAX)])
def test_head_forward_with_void_mask(dt, Cin, Cout, act, all_void):
    rng = np.random.default_rng(41 + Cout + Cin)
    lib = L.lib()
    B, HW = 3, 40 * 52                                          # blocks that end inside a sample
    M = B * HW
    x = f32(rng.standard_normal((M, Cin)))
    x = x.to(torch.bfloat16 if dt == L.RUA_BF16 else torch.float32).contiguous()
    w, b = f32(rng.standard_normal((Cout, Cin)) / 4), f32(rng.standard_normal(Cout))
    lab = np.eye(Cout, dtype=np.float32)[rng.integers(0, Cout, size=M)] if act == L.ACT_SOFTMAX else (rng.random((M, Cout)) > 0.6).astype(np.float32)
    void = random_void(rng, B, HW, all_void=all_void)
    vm = u8(np.where(void, rng.integers(1, 256, void.shape), 0))              # any non-zero byte is void
    y_clean = f32(lab)
    lab_nan = lab.copy()
    lab_nan[void.reshape(-1)] = np.nan
    y = f32(lab_nan)
    z0, p0 = torch.empty((M, Cout), device=dev()), torch.empty((M, Cout), device=dev())
    lib.call("rua_head_fwd", x.data_ptr(), w.data_ptr(), b.data_ptr(), z0.data_ptr(), p0.data_ptr(), M, Cin, Cout, act, dt, stream())
    z1, p1 = torch.empty_like(z0), torch.empty_like(p0)
    s1, m1 = torch.zeros(B * Cout * 6, dtype=torch.float64, device=dev()), torch.zeros(5, dtype=torch.float64, device=dev())
    lib.call("rua_head_fwd_loss_void", x.data_ptr(), w.data_ptr(), b.data_ptr(), z1.data_ptr(), p1.data_ptr(), y.data_ptr(), s1.data_ptr(), 1, m1.data_ptr(),
             B, HW, Cin, Cout, act, dt, vm.data_ptr(), stream())
    torch.cuda.synchronize()
    assert torch.equal(z1, z0) and torch.equal(p1, p0)          # stored for every pixel, void ones included
    want = sums_of_valid(p0.view(B, HW, Cout), y_clean.view(B, HW, Cout), void, Cout)
    got = s1.cpu().numpy().reshape(B, Cout, 6)
    assert np.isfinite(got).all()
    assert np.allclose(got, want, rtol=1e-5, atol=1e-3), np.abs(got - want).max()
    if all_void is not None:
        assert not got[all_void].any()
    assert np.array_equal(m1.cpu().numpy(), metrics_of_valid(p0, y_clean, void.reshape(-1)))
    assert abs(m1[1:].sum().item() - int((~void).sum()) * Cout) < 0.5           # TP + FP + TN + FN = valid pixels x classes
    # eight replicas and the fold of rua_tanimoto_finalize_rep
    R = 8
    sr = torch.zeros((R + 1) * B * Cout * 6, dtype=torch.float64, device=dev())
    lib.call("rua_head_fwd_loss_void", x.data_ptr(), w.data_ptr(), b.data_ptr(), None, p1.data_ptr(), y.data_ptr(), sr.data_ptr(), R, None,
             B, HW, Cin, Cout, act, dt, vm.data_ptr(), stream())
    outs = []
    for sums, rep in ((torch.from_numpy(want.reshape(-1).copy()).to(dev()), 1), (sr, R)):
        lo, co = torch.zeros(1, dtype=torch.float64, device=dev()), torch.zeros(B * Cout * 3, device=dev())
        lib.call("rua_tanimoto_finalize_rep", sums.data_ptr(), rep, B, HW, Cout, 0.25, lo.data_ptr(), co.data_ptr(), None, stream())
        torch.cuda.synchronize()
        outs.append((lo.item(), co.cpu().numpy()))
    folded = sr.view(R + 1, -1)[R].cpu().numpy().reshape(B, Cout, 6)
    assert np.allclose(folded, want, rtol=1e-5, atol=1e-3)
    assert np.isfinite(outs[1][0]) and np.isfinite(outs[1][1]).all()
    assert abs(outs[1][0] - outs[0][0]) < 1e-5 * max(1.0, abs(outs[0][0]))
    # no mask: the unmasked entry point
    s2, m2, s3, m3 = torch.zeros_like(s1), torch.zeros_like(m1), torch.zeros_like(s1), torch.zeros_like(m1)
    z2, p2, z3, p3 = torch.empty_like(z0), torch.empty_like(p0), torch.empty_like(z0), torch.empty_like(p0)
    lib.call("rua_head_fwd_loss_void", x.data_ptr(), w.data_ptr(), b.data_ptr(), z2.data_ptr(), p2.data_ptr(), y_clean.data_ptr(), s2.data_ptr(), 1, m2.data_ptr(),
             B, HW, Cin, Cout, act, dt, None, stream())
    lib.call("rua_head_fwd_loss_rep", x.data_ptr(), w.data_ptr(), b.data_ptr(), z3.data_ptr(), p3.data_ptr(), y_clean.data_ptr(), s3.data_ptr(), 1, m3.data_ptr(),
             B, HW, Cin, Cout, act, dt, stream())
    torch.cuda.synchronize()
    assert torch.equal(z2, z3) and torch.equal(p2, p3) and torch.equal(m2, m3)
    assert np.allclose(s2.cpu().numpy(), s3.cpu().numpy(), rtol=1e-5, atol=1e-3)


# ---- 3. the stand-alone masked kernels, NaN everywhere a pixel is void ---------------------------------------------------------------------
KIND_ACT = [(L.LOSS_TANIMOTO, L.ACT_SOFTMAX), (L.LOSS_TANIMOTO, L.ACT_SIGMOID), (L.LOSS_WCE, L.ACT_SOFTMAX), (L.LOSS_CE_LOGITS, L.ACT_SOFTMAX),
            (L.LOSS_BCE_LOGITS, L.ACT_SIGMOID), (L.LOSS_MSE, L.ACT_SOFTMAX), (L.LOSS_MSE, L.ACT_SIGMOID)]


@pytest.mark.parametrize("B,HW,Cc", [(1, 777, 5), (3, 2080, 6), (3, 2080, 3), (3, 2080, 2)])
def test_masked_kernels_ignore_nan_at_void_pixels(B, HW, Cc):
    rng = np.random.default_rng(HW + Cc)
    lib = L.lib()
    M = B * HW
    void = random_void(rng, B, HW) if B > 1 else (rng.random((1, HW)) < 0.3)
    vflat = void.reshape(-1)
    vm = u8(np.where(void, 255, 0))
    z = (rng.standard_normal((M, Cc)) * 2).astype(np.float32)
    p = np.exp(z - z.max(1, keepdims=True)); p = (p / p.sum(1, keepdims=True)).astype(np.float32)
    y = np.eye(Cc, dtype=np.float32)[rng.integers(0, Cc, M)]
    cw = f32(rng.uniform(1, 5, Cc))
    clean = [f32(a) for a in (p, z, y)]
    nan = []
    for a in (p, z, y):
        a = a.copy(); a[vflat] = np.nan
        nan.append(f32(a))
    pn, zn, yn = nan
    pc, zc, yc = clean
    keep = torch.from_numpy(~vflat).to(dev())
    K = int(keep.sum())
    # moments
    s = torch.zeros(B * Cc * 6, dtype=torch.float64, device=dev())
    lib.call("rua_tanimoto_sums_void", pn.data_ptr(), yn.data_ptr(), vm.data_ptr(), B, HW, Cc, s.data_ptr(), stream())
    torch.cuda.synchronize()
    got = s.cpu().numpy().reshape(B, Cc, 6)
    assert np.isfinite(got).all()
    assert np.allclose(got, sums_of_valid(pc.view(B, HW, Cc), yc.view(B, HW, Cc), void, Cc), rtol=1e-5, atol=1e-3)
    # counts
    m = torch.zeros(5, dtype=torch.float64, device=dev())
    lib.call("rua_seg_metrics_void", pn.data_ptr(), yn.data_ptr(), vm.data_ptr(), M, Cc, m.data_ptr(), stream())
    torch.cuda.synchronize()
    assert np.array_equal(m.cpu().numpy(), metrics_of_valid(pc, yc, vflat))
    # pixel losses: the sum over the valid pixels = the unmasked kernel on the compacted ones
    for kind in (L.LOSS_WCE, L.LOSS_CE_LOGITS, L.LOSS_BCE_LOGITS, L.LOSS_MSE):
        lo, lo0 = torch.zeros(1, dtype=torch.float64, device=dev()), torch.zeros(1, dtype=torch.float64, device=dev())
        per = torch.full((M,), 7.0, device=dev())
        lib.call("rua_pixel_loss_void", kind, pn.data_ptr(), zn.data_ptr(), yn.data_ptr(), cw.data_ptr(), vm.data_ptr(), M, Cc, lo.data_ptr(), per.data_ptr(), stream())
        a, b_, c_ = pc[keep].contiguous(), zc[keep].contiguous(), yc[keep].contiguous()
        per0 = torch.empty((K,), device=dev())
        lib.call("rua_pixel_loss", kind, a.data_ptr(), b_.data_ptr(), c_.data_ptr(), cw.data_ptr(), K, Cc, lo0.data_ptr(), per0.data_ptr(), stream())
        torch.cuda.synchronize()
        assert np.isfinite(lo.item()) and abs(lo.item() - lo0.item()) / M < 1e-5 * max(1.0, abs(lo0.item()) / M), kind
        assert (per[~keep].view(torch.int32) == 0).all() and torch.equal(per[keep], per0), kind
    # dz: +0.0 at void, the unmasked kernel's values elsewhere
    lo, coef = torch.zeros(1, dtype=torch.float64, device=dev()), torch.zeros(B * Cc * 3, device=dev())
    lib.call("rua_tanimoto_finalize", s.data_ptr(), B, HW, Cc, 0.7 / B, lo.data_ptr(), coef.data_ptr(), None, stream())
    torch.cuda.synchronize()
    assert np.isfinite(lo.item()) and torch.isfinite(coef).all()
    for kind, act in KIND_ACT:
        gs = 0.7 / B if kind == L.LOSS_TANIMOTO else 0.7 / M
        dz, dz0 = torch.full((M, Cc), 9.0, device=dev()), torch.empty((M, Cc), device=dev())
        lib.call("rua_head_dz_void", kind, act, pn.data_ptr(), yn.data_ptr(), coef.data_ptr(), cw.data_ptr(), gs, B, HW, Cc, vm.data_ptr(), dz.data_ptr(), stream())
        lib.call("rua_head_dz", kind, act, pc.data_ptr(), yc.data_ptr(), coef.data_ptr(), cw.data_ptr(), gs, B, HW, Cc, dz0.data_ptr(), stream())
        torch.cuda.synchronize()
        assert torch.isfinite(dz).all(), (kind, act)
        assert (dz[~keep].view(torch.int32) == 0).all(), (kind, act)             # +0.0f, bit for bit
        assert torch.equal(dz[keep], dz0[keep]) and dz0[keep].abs().sum().item() > 0, (kind, act)
    # no mask: the unmasked entry points
    s0, s1 = torch.zeros_like(s), torch.zeros_like(s)
    lib.call("rua_tanimoto_sums_void", pc.data_ptr(), yc.data_ptr(), None, B, HW, Cc, s0.data_ptr(), stream())
    lib.call("rua_tanimoto_sums", pc.data_ptr(), yc.data_ptr(), B, HW, Cc, s1.data_ptr(), stream())
    m0, m1 = torch.zeros_like(m), torch.zeros_like(m)
    lib.call("rua_seg_metrics_void", pc.data_ptr(), yc.data_ptr(), None, M, Cc, m0.data_ptr(), stream())
    lib.call("rua_seg_metrics", pc.data_ptr(), yc.data_ptr(), M, Cc, m1.data_ptr(), stream())
    torch.cuda.synchronize()
    assert np.allclose(s0.cpu().numpy(), s1.cpu().numpy(), rtol=1e-5, atol=1e-3) and torch.equal(m0, m1)


# ---- 4. the losses against the oracle -----------------------------------------------------------------------------------------------------
def test_masked_losses_against_oracle():
    """Masks with the same number K of valid pixels in every sample (other pixels per sample): the valid pixels compacted to [B, C, K, 1] are an
    image the oracle takes as it is; the pixel kinds are scaled by K / (H W) for the divide-by-all-pixels rule."""
    from oracle import resuneta_ref as ref
    rng = np.random.default_rng(19)
    lib = L.lib()
    B, H, W, Cc = 2, 16, 16, 5
    HW, M, K = H * W, B * H * W, 180
    void = np.ones((B, HW), bool)
    for n in range(B):
        void[n, rng.permutation(HW)[:K]] = False
    assert not np.array_equal(void[0], void[1])
    vm = u8(np.where(void, 255, 0))
    ids = rng.integers(0, Cc - 1, size=(B, HW))                 # the last class absent everywhere: the inf-weight path
    y1h = np.eye(Cc, dtype=np.float32)[ids]
    ysoft = rng.uniform(0, 1, (B, HW, Cc)).astype(np.float32)
    cw = np.array([4.3, 2.9, 3.9, 5.6, 37.0], np.float32)
    wce = ref.weighted_cce(cw)
    keep = torch.from_numpy(~void)
    for kind, act in KIND_ACT:
        y = ysoft if (kind == L.LOSS_MSE or (kind, act) == (L.LOSS_TANIMOTO, L.ACT_SIGMOID)) else y1h
        z = (rng.standard_normal((B, HW, Cc)) * 2).astype(np.float32)
        zt = torch.from_numpy(z).double().requires_grad_(True)
        cut = lambda t: torch.stack([t[n][keep[n]] for n in range(B)]).permute(0, 2, 1).unsqueeze(-1)          # [B, C, K, 1]
        zc, yc = cut(zt), cut(torch.from_numpy(y).double())
        pcut = torch.softmax(zc, 1) if act == L.ACT_SOFTMAX else torch.sigmoid(zc)
        wgt = 0.7
        if kind == L.LOSS_TANIMOTO:
            lt = ref.tanimoto_dual_loss(yc, pcut).mean()
        elif kind == L.LOSS_WCE:
            lt = wce(yc, pcut).double().mean() * K / HW
        elif kind == L.LOSS_CE_LOGITS:
            lt = ref.categorical_ce_logits(yc, zc).mean() * K / HW
        elif kind == L.LOSS_BCE_LOGITS:
            lt = ref.binary_ce_logits(yc, zc).mean() * K / HW
        else:
            lt = ref.mse(yc, pcut).mean() * K / HW
        (wgt * lt).backward()
        gz = zt.grad.numpy()                                     # zero at the void pixels
        with torch.no_grad():
            pfull = torch.softmax(zt, 2) if act == L.ACT_SOFTMAX else torch.sigmoid(zt)
        bad = lambda a: np.where(void[..., None], np.nan, a)    # nothing at a void pixel is read
        pd, yd, zd = f32(bad(pfull.numpy())), f32(bad(y)), f32(bad(z))
        scal = torch.zeros(16, dtype=torch.float64, device=dev())
        dz = torch.empty((B, HW, Cc), device=dev())
        cwd, coef = f32(cw), torch.zeros(B * Cc * 3, device=dev())
        if kind == L.LOSS_TANIMOTO:
            sums = torch.zeros(B * Cc * 6, dtype=torch.float64, device=dev())
            lib.call("rua_tanimoto_sums_void", pd.data_ptr(), yd.data_ptr(), vm.data_ptr(), B, HW, Cc, sums.data_ptr(), stream())
            lib.call("rua_tanimoto_finalize", sums.data_ptr(), B, HW, Cc, wgt / B, scal.data_ptr(), coef.data_ptr(), None, stream())
            gs, norm = wgt / B, 1.0
        else:
            lib.call("rua_pixel_loss_void", kind, pd.data_ptr(), zd.data_ptr(), yd.data_ptr(), cwd.data_ptr(), vm.data_ptr(), M, Cc, scal.data_ptr(), None, stream())
            gs, norm = wgt / M, 1.0 / M
        lib.call("rua_head_dz_void", kind, act, pd.data_ptr(), yd.data_ptr(), coef.data_ptr(), cwd.data_ptr(), gs, B, HW, Cc, vm.data_ptr(), dz.data_ptr(), stream())
        torch.cuda.synchronize()
        print(f"kind {kind} act {act}: loss {float(scal[0]) * norm:.8f} oracle {float(lt):.8f}, dz rel err {rel_err(dz.cpu().numpy(), gz):.2e}")
        assert abs(float(scal[0]) * norm - float(lt.detach())) < 1e-5 * max(1.0, abs(float(lt))), (kind, act)
        assert rel_err(dz.cpu().numpy(), gz) < 2e-4, (kind, act)


# ---- 5. rua_head_dz_multi_void ----------------------------------------------------------------------------------------------------------
def test_multi_head_dz_void_equals_the_per_head_launches():
    rng = np.random.default_rng(78)
    lib = L.lib()
    B, HW = 3, 40 * 52
    M = B * HW
    vm = u8(np.where(random_void(rng, B, HW), 255, 0))
    heads = [(6, L.ACT_SOFTMAX, L.LOSS_TANIMOTO), (6, L.ACT_SIGMOID, L.LOSS_TANIMOTO), (6, L.ACT_SOFTMAX, L.LOSS_CE_LOGITS), (3, L.ACT_SIGMOID, L.LOSS_MSE)]
    keep, dh, pairs = [], [], []
    for Cc, act, kind in heads:
        p = f32(rng.random((M, Cc)))
        if act == L.ACT_SOFTMAX:
            p = p / p.sum(1, keepdim=True)
        y = f32(rng.random((M, Cc)) > 0.6)
        co = f32(rng.standard_normal(B * Cc * 3))
        dz0, dz1 = torch.full((M, Cc), 3.0, device=dev()), torch.full((M, Cc), 5.0, device=dev())
        lib.call("rua_head_dz_void", kind, act, p.data_ptr(), y.data_ptr(), co.data_ptr(), None, 0.5 / B, B, HW, Cc, vm.data_ptr(), dz0.data_ptr(), stream())
        d = L.DzHead(); d.kind, d.act, d.p, d.y, d.coef, d.class_w, d.grad_scale, d.B, d.HW, d.C, d.dz = kind, act, p.data_ptr(), y.data_ptr(), co.data_ptr(), None, 0.5 / B, B, HW, Cc, dz1.data_ptr()
        dh.append(d); keep += [p, y, co]; pairs.append((dz0, dz1))
    da = (L.DzHead * len(dh))(*dh)
    lib.call("rua_head_dz_multi_void", da, len(dh), vm.data_ptr(), stream())
    torch.cuda.synchronize()
    for dz0, dz1 in pairs:
        assert torch.equal(dz0.view(torch.int32), dz1.view(torch.int32)) and dz0.abs().sum().item() > 0
    # one mask for all heads: heads that disagree in B or HW are refused (without a mask they are not)
    for field, val in (("HW", HW // 2), ("B", 2)):
        old = getattr(da[3], field)
        setattr(da[3], field, val)
        assert lib.raw("rua_head_dz_multi_void")(da, len(dh), vm.data_ptr(), None) != 0, field
        setattr(da[3], field, old)
    assert lib.raw("rua_head_dz_multi_void")(da, 0, vm.data_ptr(), None) != 0


# ---- 6. the engine ------------------------------------------------------------------------------------------------------------------------
def void_model(use_graph, ignore_void, seed=3):
    """_scene_util.new_training_model with the option."""
    from multitasking_utils import Tanimoto_dual_loss
    from resunet_a_mltsk_keras_amd.engine import ModelConfig
    from resunet_a_mltsk_keras_amd.keras_api import Adam, Model
    m = Model(ModelConfig(input_shape=SHAPE, num_classes=NCLS, multitasking=True), dtype="f32", seed=seed)
    m.engine.split_k = False
    m.engine.use_graph = use_graph
    loss = Tanimoto_dual_loss()
    m.compile(optimizer=Adam(lr=1e-3, beta_1=0.9), loss={h: loss for h in HEADS}, loss_weights={h: 1.0 for h in HEADS},
              metrics={"seg": ["accuracy"]}, ignore_void=ignore_void)
    return m


def rows_of(seed, B=2):
    rng = np.random.default_rng(seed)
    return np.array([[int(rng.integers(0, 2)), int(rng.integers(0, 150 - 64 + 1)), int(rng.integers(0, 171 - 64 + 1)), int(rng.integers(0, 8))]
                     for _ in range(B)], np.int32)


@pytest.fixture(scope="module")
def clean_batches():
    """Three compact batches (uint8 image, uint8 class map) without a void byte."""
    pool = blob_pool()
    return [pool.batch(rows_of(s)).host() for s in (11, 12, 13)]


def paint(cls, seed, value=255):
    """A copy of the class maps with two void rectangles per sample, other ones for every seed."""
    rng = np.random.default_rng(seed)
    out = cls.copy()
    for n in range(out.shape[0]):
        for _ in range(2):
            i, j = int(rng.integers(0, 48)), int(rng.integers(0, 48))
            out[n, i:i + int(rng.integers(4, 16)), j:j + int(rng.integers(4, 16))] = value
    return out


@pytest.fixture(scope="module")
def void_batches(clean_batches):
    return [(img, paint(cls, 50 + k)) for k, (img, cls) in enumerate(clean_batches)]


def run_steps(m, batches, **kw):
    """Two training steps, an evaluation, the weights afterwards."""
    out = {"train metrics": [m.train_on_batch(*batches[0], norm_type=1, **kw), m.train_on_batch(*batches[1], norm_type=1, **kw)],
           "test metrics": m.test_on_batch(*batches[2], norm_type=1, **kw)}
    out["weights after two steps"] = state(m)
    return {k: np.asarray(v, np.float64) for k, v in out.items()}


@pytest.fixture(scope="module")
def eager_void_twins(void_batches):
    return [run_steps(void_model(False, True), void_batches) for _ in range(3)]


@pytest.mark.parametrize("use_graph", [True, False])
def test_engine_without_void_bytes_the_option_changes_nothing(clean_batches, use_graph):
    twins = [run_steps(new_training_model(use_graph), clean_batches) for _ in range(3)]
    compare_with_twins(twins, run_steps(void_model(use_graph, True), clean_batches), f"option on, no void byte, use_graph={use_graph}")


def test_engine_captured_step_reads_the_current_mask(void_batches, eager_void_twins):
    """The two training batches have different void rectangles: a captured step that kept the first mask would not match the eager runs."""
    assert not np.array_equal(labels.host_void_mask(void_batches[0][1], NCLS, 2), labels.host_void_mask(void_batches[1][1], NCLS, 2))
    compare_with_twins(eager_void_twins, run_steps(void_model(True, True), void_batches), "graph against eager")


@pytest.mark.parametrize("value", [4, 200])
def test_engine_any_void_byte_value_is_the_same_void(void_batches, eager_void_twins, value):
    repainted = [(img, np.where(cls == 255, value, cls).astype(np.uint8)) for img, cls in void_batches]
    assert all((c >= NCLS).any() for _, c in repainted)
    compare_with_twins(eager_void_twins, run_steps(void_model(False, True), repainted), f"void bytes {value}")


def test_engine_float_batches_with_a_void_mask_train_like_class_map_batches(void_batches, eager_void_twins):
    """The float layout with the caller's mask (labels.host_void_mask of the class maps) against the class-map batches."""
    fb = []
    for img, cls in void_batches:
        t = compact.host_targets(img, cls, NCLS, 1, True)
        fb.append((t["x"], {h: t[h] for h in HEADS}, labels.host_void_mask(cls, NCLS, 2)))
    m = void_model(False, True)
    out = {"train metrics": [m.train_on_batch(fb[0][0], fb[0][1], void_mask=fb[0][2]), m.train_on_batch(fb[1][0], fb[1][1], void_mask=fb[1][2] != 0)],
           "test metrics": m.test_on_batch(fb[2][0], fb[2][1], void_mask=torch.from_numpy(fb[2][2]))}
    out["weights after two steps"] = state(m)
    compare_with_twins(eager_void_twins, {k: np.asarray(v, np.float64) for k, v in out.items()}, "float batches + void_mask")


def bias_gradient_deviation(ignore_void, img, cls):
    """forward_backward on a fresh engine; per head max |bias gradient - sum over pixels of the fp64 dz autograd gives for the (masked) dual
    Tanimoto loss of that head's logits|, and the scale of the gradient."""
    from oracle import resuneta_ref as ref
    m = void_model(False, ignore_void)
    eng = m.engine
    g = eng.forward_backward(torch.from_numpy(img), torch.from_numpy(cls), norm_type=1)
    torch.cuda.synchronize()
    B = img.shape[0]
    void = g.void_u8.cpu().numpy().reshape(B, -1) != 0 if g.void_u8 is not None else np.zeros((B, SHAPE[0] * SHAPE[1]), bool)
    counts = {int(v.sum()) for v in void}
    assert len(counts) == 1, "the check compacts the valid pixels: every sample needs the same number of them"
    assert bool(void.any()) == (ignore_void is not None)
    keep = torch.from_numpy(~void)
    devs = {}
    for h in g.heads:
        Cc = h["C"]
        zt = h["z"].t.detach().cpu().double().reshape(B, -1, Cc).requires_grad_(True)
        yt = h["y"].t.detach().cpu().double().reshape(B, -1, Cc)
        cut = lambda t: torch.stack([t[n][keep[n]] for n in range(B)]).permute(0, 2, 1).unsqueeze(-1)
        zc = cut(zt)
        pc = torch.softmax(zc, 1) if h["act"] == L.ACT_SOFTMAX else torch.sigmoid(zc)
        ref.tanimoto_dual_loss(cut(yt), pc).mean().backward()
        want = zt.grad.sum((0, 1)).numpy()
        off = h["lay"]["bias"]
        got = eng.G[off:off + Cc].detach().cpu().numpy().astype(np.float64)
        devs[h["name"]] = (float(np.abs(got - want).max()), float(np.abs(want).max()))
    return devs


def test_engine_bias_gradients_are_the_masked_losses(clean_batches):
    img, cls = clean_batches[0]
    base = bias_gradient_deviation(None, img, cls)
    voided = cls.copy()
    voided[0, 10:22, 30:41] = 255                               # the same rectangle elsewhere in each sample, away from the border: the
    voided[1, 40:52, 8:19] = 255                                # dilated masks have the same number of pixels
    cand = bias_gradient_deviation(2, img, voided)
    for h in HEADS:
        print(f"{h}: bias gradient deviation {cand[h][0]:.3g} with voids (scale {cand[h][1]:.3g}), {base[h][0]:.3g} without (scale {base[h][1]:.3g})")
        assert cand[h][0] <= 10 * base[h][0] + 1e-6 * max(1.0, cand[h][1]), (h, cand[h], base[h])


def test_engine_metrics_count_valid_pixels_only(void_batches):
    m = void_model(True, True)
    img, cls = void_batches[2]
    m.train_on_batch(*void_batches[0], norm_type=1)
    res = m.test_on_batch(img, cls, norm_type=1, return_dict=True)
    p = m.predict(img, batch_size=img.shape[0], norm_type=1)["seg"].reshape(-1, NCLS)
    valid = labels.host_void_mask(cls, NCLS, 2).reshape(-1) == 0
    y = compact.onehot(cls, NCLS).reshape(-1, NCLS)
    assert 0 < valid.sum() < valid.size
    want = metrics_of_valid(torch.from_numpy(p), torch.from_numpy(y), ~valid)
    names = ["seg_true_positives", "seg_false_positives", "seg_true_negatives", "seg_false_negatives"]
    assert [res[k] for k in names] == [float(v) for v in want[1:]]
    assert res["seg_accuracy"] == float(want[0] / valid.sum())
    assert sum(res[k] for k in names) == valid.sum() * NCLS


def plan_names(g):
    return {k: [c[1] for c in getattr(g, k).calls] for k in ("fwd", "loss_plan", "bwd")}


@pytest.mark.parametrize("fuse", [True, False])
def test_engine_recorded_plans(fuse):
    plans = {}
    for opt in (None, 2):
        m = void_model(True, opt)
        m.engine.fuse_head_loss = fuse
        plans[opt] = {tr: plan_names(m.engine.graph(2, tr)) for tr in (True, False)}
    for tr in (True, False):
        off, on = plans[None][tr], plans[2][tr]
        assert not [n for k in off for n in off[k] if n.endswith("_void")]
        assert {k: len(v) for k, v in off.items()} == {k: len(v) for k, v in on.items()}
        swapped = {n for k in on for n in on[k] if n.endswith("_void")}
        assert swapped >= ({"rua_head_fwd_loss_void"} if fuse else {"rua_tanimoto_sums_void", "rua_seg_metrics_void"})
        assert ("rua_head_dz_multi_void" in swapped) == tr
        # every other entry is the entry it was
        for k in off:
            assert [n for n in off[k] if n + "_void" not in swapped and n != "rua_head_fwd_loss_rep"] == \
                   [n for n in on[k] if not n.endswith("_void")], k


@pytest.mark.parametrize("use_graph", [True, False])
def test_engine_all_void_samples_and_batches(clean_batches, use_graph):
    m = void_model(use_graph, True)
    img, cls = clean_batches[0]
    one = cls.copy(); one[1] = 255
    for c in (one, one, np.full_like(cls, 255), np.full_like(cls, 255)):
        res = m.train_on_batch(img, c, norm_type=1)
        assert np.isfinite(res).all(), res
    res = m.test_on_batch(img, np.full_like(cls, 255), norm_type=1, return_dict=True)
    assert np.isfinite(list(res.values())).all() and res["seg_accuracy"] == 0.0 and res["seg_true_positives"] == 0.0
    assert np.isfinite(state(m)).all()


def test_model_refusals_come_before_any_launch(clean_batches):
    img, cls = clean_batches[0]
    t = compact.host_targets(img, cls, NCLS, 1, True)
    x, y = t["x"], {h: t[h] for h in HEADS}
    mask = np.zeros(cls.shape, np.uint8)
    off = new_training_model(True)
    with pytest.raises(ValueError, match="ignore_void"):
        off.train_on_batch(x, y, void_mask=mask)
    with pytest.raises(ValueError, match="ignore_void"):
        off.test_on_batch(x, y, void_mask=mask)
    assert not off.engine.graphs
    on = void_model(True, True)
    pool = blob_pool()
    with pytest.raises(ValueError, match="derive their own mask"):
        on.train_on_batch(img, cls, norm_type=1, void_mask=mask)
    with pytest.raises(ValueError, match="derive their own mask"):
        on.train_on_batch(pool.batch(rows_of(1)), norm_type=1, void_mask=mask)
    for bad in (mask[:1], mask[:, :32], mask.reshape(2, -1)):
        with pytest.raises(ValueError, match="shape"):
            on.train_on_batch(x, y, void_mask=bad)
    for bad in (mask.astype(np.float32), mask.astype(np.int32), mask.tolist()):
        with pytest.raises(ValueError, match="uint8 or bool"):
            on.test_on_batch(x, y, void_mask=bad)
    with pytest.raises(ValueError, match="ignore_void"):
        void_model(True, 17)
    assert not on.engine.graphs                                 # nothing was built, let alone launched


Q = 1 << 16


@pytest.mark.parametrize("affine", [False, True])
def test_engine_scene_batches_with_void_train_like_compact_batches(affine):
    base = blob_pool()
    sc = (base.images, base.class_maps)
    maps = [np.array(c, copy=True) for c in sc[1]]
    for c in maps:
        c[40:110, 50:120] = 255                                 # every window of the batches below meets the rectangle or its margin
    pool = scenes.ScenePool(sc[0], maps, patch=64)

    def batch(seed):
        rows4 = rows_of(seed)
        if not affine:
            return pool.batch(rows4)
        rng = np.random.default_rng(seed)
        return pool.affine_batch(scenes.affine_rows(rows4, 64, rng.uniform(-180, 180, 2), np.exp(rng.uniform(np.log(0.5), np.log(2.0), 2)),
                                                    rng.integers(-20 * Q, 20 * Q + 1, (2, 2))))
    bs = [batch(s) for s in (21, 22, 23)]
    hosts = [b.host() for b in bs]
    assert all((c >= NCLS).any() and (c < NCLS).any() for _, c in hosts)
    twins = [run_steps(void_model(True, True), hosts) for _ in range(3)]
    m = void_model(True, True)
    out = {"train metrics": [m.train_on_batch(bs[0], norm_type=1), m.train_on_batch(bs[1], norm_type=1)], "test metrics": m.test_on_batch(bs[2], norm_type=1)}
    out["weights after two steps"] = state(m)
    compare_with_twins(twins, {k: np.asarray(v, np.float64) for k, v in out.items()}, f"scene batches, affine={affine}")
