"""The focal kinds and label smoothing through the C ABI (rua_pixel_loss_opts, rua_head_dz_opts, rua_head_dz_multi_opts) against torch fp64 autograd
of the formulas, restated here (not imported from losses.py).  Tolerances are test_losses_against_oracle's: loss 1e-5 max(1, |loss|),
rel_err(dz) < 2e-4 - fp32 evaluation of the same formulas on the main case's inputs deviates by at most 2e-7 (loss) and 5e-7 (dz) from fp64."""
import ctypes as C

import numpy as np
import pytest
import torch

from resunet_a_mltsk_keras_amd import _lib as L
from resunet_a_mltsk_keras_amd import losses as LS

pytestmark = pytest.mark.gpu

EPS = 1e-7
SOFTMAX_KINDS = (L.LOSS_WCE, L.LOSS_CE_LOGITS, L.LOSS_FOCAL_CE)
ACT_OF = {L.LOSS_WCE: L.ACT_SOFTMAX, L.LOSS_CE_LOGITS: L.ACT_SOFTMAX, L.LOSS_FOCAL_CE: L.ACT_SOFTMAX, L.LOSS_BCE_LOGITS: L.ACT_SIGMOID,
          L.LOSS_FOCAL_BCE: L.ACT_SIGMOID}
WGT = 0.7


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


def opts(gamma=0.0, e=0.0, alpha=0.0, balance=0):
    o = L.LossOpts()
    o.gamma, o.label_smoothing, o.alpha, o.class_balance = gamma, e, alpha, balance
    return o


# ---- the formulas, fp64 torch ---------------------------------------------------------------------------------------------------------
def pow_g(q, g):
    return torch.ones_like(q) if g == 0 else torch.pow(q, g)


def loss_map(kind, p, z, y, a, o):
    """The per-pixel map [...]: p, z, y fp64 [..., C]; a fp64 [C]; o a LossOpts (gamma and alpha as the float32 values the device is given, the
    smoothing as written: 0 or 0.1)."""
    Cc = y.shape[-1]
    e = round(float(o.label_smoothing), 6)
    g, al = float(o.gamma), float(o.alpha)
    t = y * (1 - e) + e / (Cc if kind in SOFTMAX_KINDS else 2)
    if kind in (L.LOSS_WCE, L.LOSS_FOCAL_CE):
        u = torch.clamp(p / p.sum(-1, keepdim=True), EPS, 1 - EPS)
        f = pow_g(1 - u, g) if kind == L.LOSS_FOCAL_CE else 1.0
        return -(a * t * f * torch.log(u)).sum(-1)
    if kind == L.LOSS_CE_LOGITS:
        return -(t * torch.log_softmax(z, -1)).sum(-1)
    if kind == L.LOSS_BCE_LOGITS:
        return (torch.clamp(z, min=0) - z * t + torch.log1p(torch.exp(-z.abs()))).mean(-1)
    assert kind == L.LOSS_FOCAL_BCE
    oc = torch.clamp(p, EPS, 1 - EPS)
    bce = -(t * torch.log(oc) + (1 - t) * torch.log(1 - oc))
    pt = t * p + (1 - t) * (1 - p)
    w = t * al + (1 - t) * (1 - al) if o.class_balance else 1.0
    return (w * pow_g(1 - pt, g) * bce).mean(-1)


def reference(kind, z, y, a, o, M_all=None):
    """(mean loss over M_all pixels, WGT * d mean / dz, p as the device gets it) from logits z [M, C] (numpy)."""
    zt = torch.from_numpy(np.asarray(z, np.float64)).requires_grad_(True)
    p = torch.softmax(zt, -1) if kind in SOFTMAX_KINDS else torch.sigmoid(zt)
    lm = loss_map(kind, p, zt, torch.from_numpy(np.asarray(y, np.float64)), torch.from_numpy(np.asarray(a, np.float64)), o)
    mean = lm.sum() / (M_all or lm.numel())
    (WGT * mean).backward()
    return float(mean.detach()), zt.grad.numpy(), p.detach().numpy().astype(np.float32), lm.detach().numpy()


def inputs(B, HW, Cc, kind, seed=9):
    """z = 2 N(0, 1), one class absent everywhere, a uniform in [0.2, 4]."""
    rng = np.random.default_rng(seed)
    M = B * HW
    z = 2 * rng.standard_normal((M, Cc))
    if kind in SOFTMAX_KINDS:
        y = np.eye(Cc)[rng.integers(0, Cc - 1, M)]              # the last class absent
    else:
        y = (rng.random((M, Cc)) < 0.3).astype(np.float64)
        if Cc > 1:
            y[:, Cc - 1] = 0                                    # the last channel has no positive
    a = rng.uniform(0.2, 4, Cc)
    return z, y, a


def run_loss(kind, p, z, y, a, o, vm=None, per=True):
    lib = L.lib()
    M, Cc = p.shape
    out = torch.zeros(1, dtype=torch.float64, device=dev())
    pp = torch.full((M,), 7.0, device=dev()) if per else None
    lib.call("rua_pixel_loss_opts", kind, p.data_ptr(), z.data_ptr(), y.data_ptr(), a.data_ptr(), vm.data_ptr() if vm is not None else None,
             C.byref(o), M, Cc, out.data_ptr(), pp.data_ptr() if per else None, stream())
    torch.cuda.synchronize()
    return float(out[0]), pp


def run_dz(kind, p, y, a, o, B, HW, vm=None, coef=None, act=None, gs=None):
    lib = L.lib()
    M, Cc = p.shape
    dz = torch.full((M, Cc), 9.0, device=dev())
    lib.call("rua_head_dz_opts", kind, ACT_OF[kind] if act is None else act, p.data_ptr(), y.data_ptr(), coef.data_ptr() if coef is not None else None,
             a.data_ptr(), WGT / M if gs is None else gs, B, HW, Cc, vm.data_ptr() if vm is not None else None, C.byref(o), dz.data_ptr(), stream())
    torch.cuda.synchronize()
    return dz


def check(kind, z, y, a, o, B, HW, what):
    want_l, want_dz, p32, want_map = reference(kind, z, y, a, o)
    pd, zd, yd, ad = f32(p32), f32(z), f32(y), f32(np.concatenate([a, np.zeros(8)]))
    M = B * HW
    got_l, per = run_loss(kind, pd, zd, yd, ad, o)
    dz = run_dz(kind, pd, yd, ad, o, B, HW).cpu().numpy()
    e_map = float(np.abs(per.cpu().numpy() - want_map).max())
    print(f"{what}: loss {got_l / M:.8f} fp64 {want_l:.8f}, map max err {e_map:.2e}, dz rel err {rel_err(dz, want_dz):.2e}")
    assert abs(got_l / M - want_l) < 1e-5 * max(1.0, abs(want_l)), what
    assert e_map < 1e-5 * max(1.0, float(np.abs(want_map).max())), what
    assert rel_err(dz, want_dz) < 2e-4, what


# ---- 1. the main case -----------------------------------------------------------------------------------------------------------------
B0, HW0 = 3, 12 * 10                                            # M = 360: the last block is partial


@pytest.mark.parametrize("Cc", [5, 6, 3])                       # runtime C and both row forms
@pytest.mark.parametrize("e", [0.0, 0.1])
def test_focal_ce_against_fp64(Cc, e):
    z, y, a = inputs(B0, HW0, Cc, L.LOSS_FOCAL_CE)
    p = np.exp(z - z.max(1, keepdims=True)); p /= p.sum(1, keepdims=True)
    assert p.min() > 4 * EPS and 1 - p.max() > 4 * EPS           # no clip decision hangs on the precision
    assert y[:, Cc - 1].sum() == 0
    for g in (0.0, 1.0, 2.0, 3.5):
        check(L.LOSS_FOCAL_CE, z, y, a, opts(g, e), B0, HW0, f"focal CE C={Cc} gamma={g} e={e}")


@pytest.mark.parametrize("Cc", [1, 3])
@pytest.mark.parametrize("e", [0.0, 0.1])
@pytest.mark.parametrize("balance", [0, 1])
def test_binary_focal_against_fp64(Cc, e, balance):
    z, y, a = inputs(B0, HW0, Cc, L.LOSS_FOCAL_BCE)
    p = 1 / (1 + np.exp(-z))
    assert p.min() > 4 * EPS and 1 - p.max() > 4 * EPS
    for g in (0.0, 1.0, 2.0, 3.5):
        check(L.LOSS_FOCAL_BCE, z, y, a, opts(g, e, 0.3, balance), B0, HW0, f"binary focal C={Cc} gamma={g} e={e} balance={balance}")


@pytest.mark.parametrize("kind,Cc", [(L.LOSS_WCE, 5), (L.LOSS_WCE, 6), (L.LOSS_CE_LOGITS, 6), (L.LOSS_CE_LOGITS, 3), (L.LOSS_BCE_LOGITS, 1),
                                     (L.LOSS_BCE_LOGITS, 3)])
def test_smoothed_cross_entropies_against_fp64(kind, Cc):
    z, y, a = inputs(B0, HW0, Cc, kind)
    check(kind, z, y, a, opts(0.0, 0.1), B0, HW0, f"kind {kind} C={Cc} e=0.1")


# ---- 2. the clip ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,Cc", [(L.LOSS_FOCAL_CE, 3), (L.LOSS_FOCAL_CE, 5), (L.LOSS_FOCAL_BCE, 1), (L.LOSS_FOCAL_BCE, 3)])
@pytest.mark.parametrize("g", [0.0, 1.0, 2.0, 3.5])
@pytest.mark.parametrize("e", [0.0, 0.1])
def test_clip_rows(kind, Cc, g, e):
    """Logits 21 apart: p is 7.6e-10 and 1.0f.  The fp64 side starts from the fp32 p the device is given (dL/dp by autograd, then the activation's
    Jacobian at that p), so both sides take the same clip decisions: no gradient through a clipped probability, and log 1e-7 in the loss."""
    rng = np.random.default_rng(21)
    rows = 12
    z = rng.standard_normal((rows, Cc)) * 0.1
    hot = rng.integers(0, Cc, rows)
    z[np.arange(rows), hot] += np.where(np.arange(rows) % 2 == 0, 21.0, -21.0)
    if kind == L.LOSS_FOCAL_CE:
        p = np.exp(z - z.max(1, keepdims=True)); p /= p.sum(1, keepdims=True)
        y = np.eye(Cc)[np.where(np.arange(rows) % 4 < 2, hot, (hot + 1) % Cc)]      # the label on the extreme class and off it
    else:
        p = 1 / (1 + np.exp(-z))
        y = np.zeros((rows, Cc)); y[np.arange(rows), hot] = np.arange(rows) % 4 < 2
    p32 = p.astype(np.float32)
    assert (p32 == 1.0).any() and (p32 < 1e-9).any()
    a = rng.uniform(0.2, 4, Cc)
    o = opts(g, e, 0.3, 1)
    pt = torch.from_numpy(p32.astype(np.float64)).requires_grad_(True)
    lm = loss_map(kind, pt, None, torch.from_numpy(y), torch.from_numpy(a), o)
    (WGT * lm.mean()).backward()
    gp, p64 = pt.grad, pt.detach()
    want_dz = (p64 * (gp - (gp * p64).sum(-1, keepdim=True)) if kind == L.LOSS_FOCAL_CE else gp * p64 * (1 - p64)).numpy()
    pd, yd, ad = f32(p32), f32(y), f32(np.concatenate([a, np.zeros(8)]))
    got_l, per = run_loss(kind, pd, pd, yd, ad, o)
    dz = run_dz(kind, pd, yd, ad, o, 1, rows).cpu().numpy()
    want_l = float(lm.mean().detach())
    print(f"clip kind {kind} C={Cc} gamma={g} e={e}: loss {got_l / rows:.8f} fp64 {want_l:.8f}, dz rel err {rel_err(dz, want_dz):.2e}")
    assert np.isfinite(dz).all() and np.isfinite(got_l)
    assert abs(got_l / rows - want_l) < 1e-5 * max(1.0, abs(want_l))
    assert rel_err(dz, want_dz) < 2e-4
    if kind == L.LOSS_FOCAL_CE and g == 0 and e == 0:
        # a label on a class of probability 7.6e-10: the loss term is -a log 1e-7 and nothing flows back through the clipped u
        k = [r for r in range(rows) if r % 2 == 1 and r % 4 < 2][0]
        assert abs(float(per[k]) - a[hot[k]] * -np.log(1e-7)) < 1e-4 * a[hot[k]] * 17
        assert np.abs(dz[k]).max() < 1e-6 * np.abs(want_dz).max() + 1e-12


# ---- 3. more pixels than one pass of the launch covers -----------------------------------------------------------------------------------
def test_grid_stride_loss():
    """rua_pixel_loss_opts launches at most 1024 blocks of 256 pixels: M = 262 144 + 300 needs the second pass."""
    M, Cc = 1024 * 256 + 300, 6
    z, y, a = inputs(1, M, Cc, L.LOSS_FOCAL_CE, seed=5)
    o = opts(2.0, 0.1)
    want_l, _, p32, want_map = reference(L.LOSS_FOCAL_CE, z, y, a, o)
    got_l, per = run_loss(L.LOSS_FOCAL_CE, f32(p32), f32(z), f32(y), f32(np.concatenate([a, np.zeros(8)])), o)
    per = per.cpu().numpy()
    print(f"grid-stride loss: {got_l / M:.8f} fp64 {want_l:.8f}, map max err {np.abs(per - want_map).max():.2e}")
    assert abs(got_l / M - want_l) < 1e-5 * max(1.0, abs(want_l))
    assert np.abs(per - want_map)[-400:].max() < 1e-5 * max(1.0, want_map.max()) and np.abs(per - want_map).max() < 1e-5 * max(1.0, want_map.max())


def test_grid_stride_dz():
    """rua_head_dz_opts covers 4096 / B blocks of 256 pixels per sample in one pass: B = 8, HW = 131 072 + 77 needs the second."""
    B, HW, Cc = 8, (4096 // 8) * 256 + 77, 3
    z, y, a = inputs(B, HW, Cc, L.LOSS_FOCAL_BCE, seed=6)
    o = opts(3.5, 0.1, 0.3, 1)
    _, want_dz, p32, _ = reference(L.LOSS_FOCAL_BCE, z, y, a, o)
    dz = run_dz(L.LOSS_FOCAL_BCE, f32(p32), f32(y), f32(np.concatenate([a, np.zeros(8)])), o, B, HW).cpu().numpy()
    print(f"grid-stride dz: rel err {rel_err(dz, want_dz):.2e}")
    assert rel_err(dz, want_dz) < 2e-4
    tail = np.arange(B)[:, None] * HW + np.arange(HW - 77, HW)[None]          # the pixels of the second pass, in every sample
    assert rel_err(dz[tail.reshape(-1)], want_dz[tail.reshape(-1)]) < 2e-4


def test_grid_stride_multi_dz():
    """rua_head_dz_multi_opts covers 4096 / (B n) blocks per sample and head: B = 8, four heads, HW = 32 768 + 77 needs the second pass."""
    lib = L.lib()
    B, HW = 8, (4096 // (8 * 4)) * 256 + 77
    M = B * HW
    specs = [(L.LOSS_FOCAL_CE, 6, opts(2.0, 0.1)), (L.LOSS_FOCAL_BCE, 6, opts(2.0, 0.0, 0.75, 1)), (L.LOSS_FOCAL_CE, 6, opts(0.0)),
             (L.LOSS_FOCAL_BCE, 6, opts(3.5, 0.1))]
    heads, keep, wants, outs = [], [], [], []
    for i, (kind, Cc, o) in enumerate(specs):
        z, y, a = inputs(B, HW, Cc, kind, seed=30 + i)
        _, want_dz, p32, _ = reference(kind, z, y, a, o)
        pd, yd, ad = f32(p32), f32(y), f32(np.concatenate([a, np.zeros(8)]))
        dz = torch.full((M, Cc), 9.0, device=dev())
        d = L.DzHead(); d.kind, d.act, d.p, d.y, d.coef, d.class_w, d.grad_scale, d.B, d.HW, d.C, d.dz = kind, ACT_OF[kind], pd.data_ptr(), yd.data_ptr(), None, ad.data_ptr(), WGT / M, B, HW, Cc, dz.data_ptr()
        heads.append(d); keep += [pd, yd, ad]; wants.append(want_dz); outs.append(dz)
    da, oa = (L.DzHead * 4)(*heads), (L.LossOpts * 4)(*[s[2] for s in specs])
    lib.call("rua_head_dz_multi_opts", da, oa, 4, None, stream())
    torch.cuda.synchronize()
    for i, (dz, want) in enumerate(zip(outs, wants)):
        print(f"grid-stride multi dz, head {i}: rel err {rel_err(dz.cpu().numpy(), want):.2e}")
        assert rel_err(dz.cpu().numpy(), want) < 2e-4, i


# ---- 4. void pixels -----------------------------------------------------------------------------------------------------------------------
def random_void(rng, B, HW, share=0.3, all_void=None):
    v = np.stack([rng.random(HW) < share * (0.6 + 0.4 * n) for n in range(B)])
    if all_void is not None:
        v[all_void] = True
    return v


@pytest.mark.parametrize("kind,Cc", [(L.LOSS_FOCAL_CE, 6), (L.LOSS_FOCAL_CE, 5), (L.LOSS_FOCAL_BCE, 3), (L.LOSS_FOCAL_BCE, 1), (L.LOSS_WCE, 6),
                                     (L.LOSS_CE_LOGITS, 3), (L.LOSS_BCE_LOGITS, 2)])
@pytest.mark.parametrize("all_void", [None, 1])
def test_void_pixels_leave_by_select(kind, Cc, all_void):
    rng = np.random.default_rng(40 + Cc)
    B, HW = 3, 2080
    M = B * HW
    void = random_void(rng, B, HW, all_void=all_void).reshape(-1)
    vm = u8(np.where(void, 255, 0))
    z, y, a = inputs(B, HW, Cc, kind, seed=41)
    o = opts(2.0 if kind in LS.FOCAL_KINDS else 0.0, 0.1, 0.3, 1)
    _, _, p32, _ = reference(kind, z, y, a, o)
    ad = f32(np.concatenate([a, np.zeros(8)]))
    junk = [np.nan, np.inf, -np.inf]
    bad = []
    for k, arr in enumerate((p32, z, y)):
        arr = np.array(arr, np.float32); arr[void] = junk[k]
        bad.append(f32(arr))
    pn, zn, yn = bad
    keep = torch.from_numpy(~void).to(dev())
    K = int(keep.sum())
    pc, zc, yc = (f32(np.asarray(arr, np.float32)[~void]) for arr in (p32, z, y))
    got_l, per = run_loss(kind, pn, zn, yn, ad, o, vm=vm)
    want_l, per0 = run_loss(kind, pc, zc, yc, ad, o)
    assert np.isfinite(got_l) and torch.isfinite(per).all()
    assert abs(got_l - want_l) / M < 1e-5 * max(1.0, abs(want_l) / M)
    assert (per[~keep].view(torch.int32) == 0).all() and torch.equal(per[keep], per0)
    dz = run_dz(kind, pn, yn, ad, o, B, HW, vm=vm)
    dz0 = run_dz(kind, pc, yc, ad, o, 1, K, gs=WGT / M)
    assert torch.isfinite(dz).all()
    assert (dz[~keep].view(torch.int32) == 0).all()                                        # +0.0f, bit for bit
    assert torch.equal(dz[keep], dz0) and dz0.abs().sum().item() > 0


# ---- 5. byte equality -----------------------------------------------------------------------------------------------------------------------
KIND_ACT = [(L.LOSS_TANIMOTO, L.ACT_SOFTMAX), (L.LOSS_TANIMOTO, L.ACT_SIGMOID), (L.LOSS_WCE, L.ACT_SOFTMAX), (L.LOSS_CE_LOGITS, L.ACT_SOFTMAX),
            (L.LOSS_BCE_LOGITS, L.ACT_SIGMOID), (L.LOSS_MSE, L.ACT_SOFTMAX), (L.LOSS_MSE, L.ACT_SIGMOID)]


@pytest.mark.parametrize("Cc", [6, 3, 5])
@pytest.mark.parametrize("masked", [False, True])
def test_zeroed_options_give_the_bytes_of_the_old_entries(Cc, masked):
    rng = np.random.default_rng(60 + Cc)
    lib = L.lib()
    B, HW = 3, 777
    M = B * HW
    z, y, a = inputs(B, HW, Cc, L.LOSS_WCE, seed=61)
    p = np.exp(z - z.max(1, keepdims=True)); p /= p.sum(1, keepdims=True)
    pd, zd, yd, ad = f32(p), f32(z), f32(y), f32(np.concatenate([a, np.zeros(8)]))
    coef = f32(rng.standard_normal(B * Cc * 3))
    vm = u8(np.where(random_void(rng, B, HW), 255, 0)) if masked else None
    vp = vm.data_ptr() if masked else None
    zero = opts()
    for kind in (L.LOSS_WCE, L.LOSS_CE_LOGITS, L.LOSS_BCE_LOGITS, L.LOSS_MSE):
        l0 = torch.zeros(1, dtype=torch.float64, device=dev())
        per0 = torch.full((M,), 3.0, device=dev())
        lib.call("rua_pixel_loss_void", kind, pd.data_ptr(), zd.data_ptr(), yd.data_ptr(), ad.data_ptr(), vp, M, Cc, l0.data_ptr(), per0.data_ptr(), stream())
        l1, per1 = run_loss(kind, pd, zd, yd, ad, zero, vm=vm)
        assert torch.equal(per0.view(torch.int32), per1.view(torch.int32)) and abs(l1 - float(l0[0])) <= 1e-12 * abs(l1), kind
    for kind, act in KIND_ACT:
        gs = WGT / B if kind == L.LOSS_TANIMOTO else WGT / M
        dz0 = torch.full((M, Cc), 3.0, device=dev())
        lib.call("rua_head_dz_void", kind, act, pd.data_ptr(), yd.data_ptr(), coef.data_ptr(), ad.data_ptr(), gs, B, HW, Cc, vp, dz0.data_ptr(), stream())
        dz1 = run_dz(kind, pd, yd, ad, zero, B, HW, vm=vm, coef=coef, act=act, gs=gs)
        assert torch.equal(dz0.view(torch.int32), dz1.view(torch.int32)) and dz0.abs().sum().item() > 0, (kind, act)


@pytest.mark.parametrize("masked", [False, True])
def test_multi_opts_equals_the_per_head_launches(masked):
    """Mixed kinds, old ones with zeroed options among them: every head's dz is what its own launch writes - the old entry's for an old kind
    without options."""
    rng = np.random.default_rng(78)
    lib = L.lib()
    B, HW = 3, 40 * 52
    M = B * HW
    vm = u8(np.where(random_void(rng, B, HW), 255, 0)) if masked else None
    vp = vm.data_ptr() if masked else None
    heads = [(6, L.ACT_SOFTMAX, L.LOSS_FOCAL_CE, opts(2.0, 0.1)), (6, L.ACT_SIGMOID, L.LOSS_FOCAL_BCE, opts(3.5, 0.0, 0.25, 1)),
             (6, L.ACT_SOFTMAX, L.LOSS_MSE, opts()), (3, L.ACT_SIGMOID, L.LOSS_MSE, opts()), (5, L.ACT_SOFTMAX, L.LOSS_WCE, opts(0.0, 0.1)),
             (6, L.ACT_SOFTMAX, L.LOSS_TANIMOTO, opts()), (3, L.ACT_SOFTMAX, L.LOSS_CE_LOGITS, opts()), (6, L.ACT_SIGMOID, L.LOSS_BCE_LOGITS, opts())]
    keep, dh, pairs = [], [], []
    for Cc, act, kind, o in heads:
        p = f32(rng.random((M, Cc)) * 0.98 + 0.01)
        if act == L.ACT_SOFTMAX:
            p = p / p.sum(1, keepdim=True)
        y = f32(rng.random((M, Cc)) > 0.6)
        co, cw = f32(rng.standard_normal(B * Cc * 3)), f32(rng.uniform(0.2, 4, 16))
        dz0, dz1 = torch.full((M, Cc), 3.0, device=dev()), torch.full((M, Cc), 5.0, device=dev())
        gs = 0.5 / B
        if kind <= L.LOSS_MSE and o.label_smoothing == 0:
            lib.call("rua_head_dz_void", kind, act, p.data_ptr(), y.data_ptr(), co.data_ptr(), cw.data_ptr(), gs, B, HW, Cc, vp, dz0.data_ptr(), stream())
        else:
            lib.call("rua_head_dz_opts", kind, act, p.data_ptr(), y.data_ptr(), co.data_ptr(), cw.data_ptr(), gs, B, HW, Cc, vp, C.byref(o), dz0.data_ptr(), stream())
        d = L.DzHead(); d.kind, d.act, d.p, d.y, d.coef, d.class_w, d.grad_scale, d.B, d.HW, d.C, d.dz = kind, act, p.data_ptr(), y.data_ptr(), co.data_ptr(), cw.data_ptr(), gs, B, HW, Cc, dz1.data_ptr()
        dh.append(d); keep += [p, y, co, cw]; pairs.append((dz0, dz1))
    da, oa = (L.DzHead * len(dh))(*dh), (L.LossOpts * len(dh))(*[h[3] for h in heads])
    lib.call("rua_head_dz_multi_opts", da, oa, len(dh), vp, stream())
    torch.cuda.synchronize()
    for (dz0, dz1), h in zip(pairs, heads):
        assert torch.equal(dz0.view(torch.int32), dz1.view(torch.int32)) and dz0.abs().sum().item() > 0, h[:3]
    # all heads old and without options: the old multi entry's bytes
    old = [i for i, h in enumerate(heads) if h[2] <= L.LOSS_MSE and h[3].label_smoothing == 0]
    da2, oa2 = (L.DzHead * len(old))(*[dh[i] for i in old]), (L.LossOpts * len(old))()
    for i in old:
        pairs[i][1].fill_(5.0)
    lib.call("rua_head_dz_multi_opts", da2, oa2, len(old), vp, stream())
    torch.cuda.synchronize()
    for i in old:
        assert torch.equal(pairs[i][0].view(torch.int32), pairs[i][1].view(torch.int32)), heads[i][:3]


# ---- 6. the Python callables and the argument checks ------------------------------------------------------------------------------------------
def test_callables_return_the_map():
    from resunet_a_mltsk_keras_amd import keras_api as ka
    B, H, W, Cc = 2, 9, 7, 5
    z, y, a = inputs(B, H * W, Cc, L.LOSS_FOCAL_CE, seed=3)
    p = np.exp(z - z.max(1, keepdims=True)); p = (p / p.sum(1, keepdims=True)).astype(np.float32)
    yt, yp = y.reshape(B, H, W, Cc).astype(np.float32), p.reshape(B, H, W, Cc)
    for alpha in (0.25, list(a)):
        got = ka.CategoricalFocalCrossentropy(alpha=alpha, gamma=2.0, label_smoothing=0.1)(yt, yp)
        want = LS.host_categorical_focal(yt, yp, alpha, 2.0, 0.1)
        assert got.shape == (B, H, W) and got.dtype == np.float32
        assert np.abs(got - want).max() < 1e-5 * max(1.0, np.abs(want).max())
    zb, yb, _ = inputs(B, H * W, 3, L.LOSS_FOCAL_BCE, seed=4)
    pb = (1 / (1 + np.exp(-zb))).astype(np.float32).reshape(B, H, W, 3)
    got = ka.BinaryFocalCrossentropy(apply_class_balancing=True, alpha=0.4, gamma=3.0)(yb.reshape(B, H, W, 3), pb)
    want = LS.host_binary_focal(yb.reshape(B, H, W, 3), pb, 3.0, 0.4, True)
    assert got.shape == (B, H, W) and np.abs(got - want).max() < 1e-5 * max(1.0, np.abs(want).max())
    got = ka.weighted_categorical_crossentropy(list(a), label_smoothing=0.1)(yt, yp)
    want = LS.host_categorical_focal(yt, yp, a, 0.0, 0.1)                                   # gamma 0: smoothed weighted CE
    assert np.abs(got - want).max() < 1e-5 * max(1.0, np.abs(want).max())
    with pytest.raises(ValueError, match="gamma"):
        ka.CategoricalFocalCrossentropy(gamma=0.5)(yt, yp)


def test_argument_errors_come_before_any_launch():
    """Every refusal returns RUA_ERR_ARG with its reason; the outputs keep their fill."""
    lib = L.lib()
    M, Cc = 64, 6
    t = f32(np.full((M, Cc), 1.0 / Cc))
    cw = f32(np.ones(16))
    out = torch.zeros(1, dtype=torch.float64, device=dev())
    dz = torch.full((M, Cc), 9.0, device=dev())
    err = lambda: lib.dll.rua_last_error().decode()

    def loss(kind, o, Cc=Cc, w=cw, z=t):
        return lib.raw("rua_pixel_loss_opts")(kind, t.data_ptr(), z.data_ptr() if z is not None else None, t.data_ptr(), w.data_ptr() if w is not None else None,
                                              None, C.byref(o), M, Cc, out.data_ptr(), None, None)

    def dzf(kind, act, o, Cc=Cc, w=cw):
        return lib.raw("rua_head_dz_opts")(kind, act, t.data_ptr(), t.data_ptr(), None, w.data_ptr() if w is not None else None, 0.1, 1, M, Cc, None, C.byref(o),
                                           dz.data_ptr(), None)
    for g in (0.5, -1.0, 8.5, float("nan")):
        assert loss(L.LOSS_FOCAL_CE, opts(g)) == -1 and "gamma" in err()
        assert dzf(L.LOSS_FOCAL_BCE, L.ACT_SIGMOID, opts(g)) == -1 and "gamma" in err()
    for e in (-0.1, 1.0, float("nan")):
        assert loss(L.LOSS_WCE, opts(0, e)) == -1 and "label_smoothing" in err()
        assert dzf(L.LOSS_FOCAL_CE, L.ACT_SOFTMAX, opts(2, e)) == -1 and "label_smoothing" in err()
    assert loss(L.LOSS_MSE, opts(0, 0.1)) == -1 and "no label smoothing" in err()
    assert dzf(L.LOSS_TANIMOTO, L.ACT_SOFTMAX, opts(0, 0.1)) == -1
    assert dzf(L.LOSS_MSE, L.ACT_SOFTMAX, opts(0, 0.1)) == -1 and "no label smoothing" in err()
    assert loss(L.LOSS_TANIMOTO, opts()) == -1 and "per-pixel" in err()
    assert loss(7, opts()) == -1 and dzf(7, L.ACT_SOFTMAX, opts()) == -1
    assert dzf(L.LOSS_FOCAL_CE, L.ACT_SIGMOID, opts(2)) == -1 and "softmax" in err()
    assert dzf(L.LOSS_FOCAL_CE, L.ACT_NONE, opts(2)) == -1 and "softmax" in err()
    assert dzf(L.LOSS_FOCAL_BCE, L.ACT_SOFTMAX, opts(2)) == -1 and "sigmoid" in err()
    assert dzf(L.LOSS_FOCAL_CE, L.ACT_SOFTMAX, opts(2), w=None) == -1 and "class_w" in err()
    assert loss(L.LOSS_FOCAL_CE, opts(2), w=None) == -1 and "per-class" in err()
    assert loss(L.LOSS_FOCAL_CE, opts(2), Cc=9) == -1 and "1..8" in err()
    assert dzf(L.LOSS_FOCAL_BCE, L.ACT_SIGMOID, opts(2), Cc=9) == -1 and "1..8" in err()
    assert loss(L.LOSS_CE_LOGITS, opts(0, 0.1), z=None) == -1 and "logits" in err()
    for al in (-0.1, 1.5):
        assert dzf(L.LOSS_FOCAL_BCE, L.ACT_SIGMOID, opts(2, 0, al, 1)) == -1 and "alpha" in err()
    assert dzf(L.LOSS_FOCAL_BCE, L.ACT_SIGMOID, opts(2, 0, 0.5, 2)) == -1 and "class_balance" in err()
    assert lib.raw("rua_pixel_loss_opts")(L.LOSS_FOCAL_CE, t.data_ptr(), None, t.data_ptr(), cw.data_ptr(), None, None, M, Cc, out.data_ptr(), None, None) == -1
    # the multi entry: a bad head anywhere refuses the whole call
    d = L.DzHead(); d.kind, d.act, d.p, d.y, d.coef, d.class_w, d.grad_scale, d.B, d.HW, d.C, d.dz = L.LOSS_FOCAL_CE, L.ACT_SOFTMAX, t.data_ptr(), t.data_ptr(), None, cw.data_ptr(), 0.1, 1, M, Cc, dz.data_ptr()
    d2 = L.DzHead(); d2.kind, d2.act, d2.p, d2.y, d2.coef, d2.class_w, d2.grad_scale, d2.B, d2.HW, d2.C, d2.dz = L.LOSS_FOCAL_BCE, L.ACT_SOFTMAX, t.data_ptr(), t.data_ptr(), None, None, 0.1, 1, M, Cc, dz.data_ptr()
    multi = lib.raw("rua_head_dz_multi_opts")
    assert multi((L.DzHead * 2)(d, d2), (L.LossOpts * 2)(opts(2), opts(2)), 2, None, None) == -1 and "head 1" in err() and "sigmoid" in err()
    assert multi((L.DzHead * 1)(d), (L.LossOpts * 1)(opts(0.5)), 1, None, None) == -1 and "gamma" in err()
    assert multi((L.DzHead * 1)(d), None, 1, None, None) == -1
    assert multi((L.DzHead * 1)(d), (L.LossOpts * 1)(opts(2)), 0, None, None) == -1
    torch.cuda.synchronize()
    assert float(out[0]) == 0.0 and (dz == 9.0).all()
