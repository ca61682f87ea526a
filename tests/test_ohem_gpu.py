"""Online hard example mining through the C ABI: rua_ohem_select against losses.host_ohem - drop mask, threshold key, counts and normaliser bit
for bit, the kept sum and the slot within the bound of an fp64 sum, two runs bit-identical -, its argument refusals, and rua_head_dz_sel /
rua_head_dz_multi_sel against rua_head_dz_opts / rua_head_dz_multi_opts byte for byte.

Shapes: M = 1, 255, 257 and 2 * 33 * 31 = 2046 (no multiple of 4 or of the 256-thread block; two blocks of the 1024-pixel grid), 5000 for the
maps that one pass of the radix select decides (more than one block flushes into each histogram)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from resunet_a_mltsk_keras_amd import _lib as L
from resunet_a_mltsk_keras_amd import losses as LS

pytestmark = pytest.mark.gpu

SOFTMAX_KINDS = (L.LOSS_WCE, L.LOSS_CE_LOGITS, L.LOSS_FOCAL_CE)
ACT_OF = {L.LOSS_WCE: L.ACT_SOFTMAX, L.LOSS_CE_LOGITS: L.ACT_SOFTMAX, L.LOSS_FOCAL_CE: L.ACT_SOFTMAX, L.LOSS_BCE_LOGITS: L.ACT_SIGMOID,
          L.LOSS_FOCAL_BCE: L.ACT_SIGMOID}
M_ODD = 2 * 33 * 31


def dev():
    return torch.device("cuda", 0)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev())


def u8(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint8)).to(dev())


def bits(x):
    return int(np.float32(x).view(np.uint32))


def select(Lm, valid=None, t=None, loss_weight=1.0, slot0=0.0, **o):
    """One rua_ohem_select on the map Lm (numpy float32 or a device tensor) with drop_mask, result and workspace pre-filled with junk."""
    lib = L.lib()
    pp = Lm if isinstance(Lm, torch.Tensor) else f32(Lm)
    M = pp.numel()
    vm = u8(1 - np.asarray(valid, np.uint8)) if valid is not None else None
    nws = int(lib.raw("rua_ohem_workspace_bytes")(M))
    ws = torch.full((nws // 8 + 1,), float("nan"), dtype=torch.float64, device=dev())
    drop = torch.full((M,), 0xAA, dtype=torch.uint8, device=dev())
    res = torch.full((C.sizeof(L.OhemResult),), 0xFF, dtype=torch.uint8, device=dev())
    slot = torch.full((1,), slot0, dtype=torch.float64, device=dev())
    st = torch.tensor([float(t), 0.0], dtype=torch.float64, device=dev()) if t is not None else None
    so = LS.to_ohem_struct(LS.ohem_options(**o))
    lib.call("rua_ohem_select", pp.data_ptr(), vm.data_ptr() if vm is not None else None, M, C.byref(so), st.data_ptr() if st is not None else None, loss_weight,
             ws.data_ptr(), nws, drop.data_ptr(), slot.data_ptr(), res.data_ptr(), stream())
    torch.cuda.synchronize()
    r = L.OhemResult.from_buffer_copy(res.cpu().numpy().tobytes())
    return dict(drop=drop.cpu().numpy(), slot=float(slot[0]), tau_key=int(r.tau_key), tau=bits(r.tau), n_valid=int(r.n_valid), n_kept=int(r.n_kept), K=int(r.K),
                kept_sum=float(r.kept_sum), scale=bits(r.scale), q16_used=int(r.q16_used))


def check(Lm, valid=None, t=None, loss_weight=1.0, what="", **o):
    """The device against host_ohem: everything integer and the float32s bit for bit, the sums within n_kept * 2^-52 of fsum, a second run identical."""
    Lh = Lm.cpu().numpy() if isinstance(Lm, torch.Tensor) else np.asarray(Lm, np.float32)
    host = LS.host_ohem(Lh, valid, t=t or 0, loss_weight=loss_weight, **o)
    a = select(Lm, valid, t, loss_weight, **o)
    b = select(Lm, valid, t, loss_weight, **o)
    assert np.array_equal(a["drop"], host["drop_mask"].reshape(-1)), (what, o)
    for k in ("tau_key", "n_valid", "n_kept", "K", "q16_used"):
        assert a[k] == host[k], (what, o, k, a[k], host[k])
    assert a["tau"] == bits(host["tau"]) and a["scale"] == bits(host["scale"]), (what, o)
    kept = [float(x) for x, d in zip(Lh.reshape(-1), a["drop"]) if d == 0]
    if kept and all(math.isfinite(x) for x in kept):
        exact = math.fsum(kept)
        bound = len(kept) * 2.0 ** -52
        print(f"{what} {o}: n_kept {len(kept)}, kept sum rel err {abs(a['kept_sum'] - exact) / max(abs(exact), 1e-300):.2e}, bound {bound:.2e}")
        assert abs(a["kept_sum"] - exact) <= bound * abs(exact), (what, o)
        assert abs(a["slot"] - exact / len(kept)) <= bound * abs(exact / len(kept)), (what, o)
    elif kept:                                           # a NaN or an infinity among the kept: the sum is what fp64 makes of it
        want = float(np.sum(np.asarray(kept, np.float64)))
        assert (math.isnan(a["kept_sum"]) and math.isnan(want)) or a["kept_sum"] == want, (what, o)
    else:
        assert a["kept_sum"] == 0.0 and a["slot"] == 0.0 and a["scale"] == 0, (what, o)
    for k in a:                                          # bit-identical between two runs
        same = np.array_equal(a[k], b[k]) if k == "drop" else (a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]))
        assert same, (what, o, k)
    return a, host


def synthetic():
    rng = np.random.default_rng(11)
    base = np.float32(1.7917595)                         # log 6
    bb = base.view(np.uint32)
    return {
        "one": (np.array([0.5], np.float32), None),
        "m255": (rng.random(255).astype(np.float32) * 3, None),
        "m257": (rng.random(257).astype(np.float32) * 3, None),
        "odd": (rng.random(M_ODD).astype(np.float32) * 3, None),
        "all_equal": (np.full(M_ODD, base, np.float32), None),
        "low_bits": ((bb + rng.integers(0, 1 << 10, 5000).astype(np.uint32)).view(np.float32), None),               # pass 3 decides
        "mid_bits": ((bb & np.uint32(0xFFE003FF) | (rng.integers(0, 1 << 11, 5000).astype(np.uint32) << np.uint32(10))).view(np.float32), None),     # pass 2
        "exponents": (np.ldexp(1.0, rng.integers(-120, 120, 5000)).astype(np.float32), None),                         # pass 1
        "specials": (np.array([0.0, -0.0, np.inf, np.nan, 1.0, -1.0, 1e-42, 2.0, 0.0, -0.0, 3.0], np.float32), None),
        "void30": (rng.random(M_ODD).astype(np.float32) * 3, rng.random(M_ODD) >= 0.3),
        "all_void": (rng.random(300).astype(np.float32), np.zeros(300, bool)),
    }


SYN = synthetic()


@pytest.mark.parametrize("name", list(SYN))
def test_select_equals_host(name):
    Lm, valid = SYN[name]
    nv = int(Lm.size if valid is None else valid.sum())
    pp = f32(Lm)
    check(pp, valid, what=name)                                          # a quarter
    check(pp, valid, what=name, keep_q16=32768)                          # the middle (all_equal: inside the tie)
    a, _ = check(pp, valid, what=name, keep_q16=1)                       # K = 1
    assert a["K"] == min(1, nv)
    a, _ = check(pp, valid, what=name, keep_q16=65536)                   # K = n_valid
    assert a["K"] == nv and a["n_kept"] == nv
    a, _ = check(pp, valid, what=name, keep_q16=1, min_kept=nv + 7)      # the floor above n_valid
    assert a["K"] == nv
    check(pp, valid, what=name, keep_q16=1, min_kept=max(nv // 3, 1), loss_weight=0.3)
    check(pp, valid, what=name, keep_q16=6554, warmup=4, t=2)            # the share under a warm-up, from the device's counter
    a, _ = check(pp, valid, what=name, keep_q16=6554, warmup=4, t=0)
    assert a["q16_used"] == 65536 and a["n_kept"] == nv
    # a loss threshold below, at and above the K-th value
    _, h = check(pp, valid, what=name, keep_q16=16384)
    tau = LS.ohem_unkey(h["tau_key"])
    if nv and np.isfinite(tau):
        for th in (np.nextafter(tau, np.float32(-np.inf)), tau, np.nextafter(tau, np.float32(np.inf))):
            a, _ = check(pp, valid, what=name + " thresh", keep_q16=16384, thresh=float(th))
            assert a["tau_key"] == min(h["tau_key"], int(LS.ohem_key(th)[0]))
    check(pp, valid, what=name, keep_q16=1, thresh=-1.0)                 # a threshold below every loss keeps every valid pixel
    if name == "all_equal":
        a = select(pp, keep_q16=32768)
        assert a["K"] == M_ODD // 2 and a["n_kept"] == M_ODD and not a["drop"].any()
    if name == "all_void":
        a = select(pp, valid, slot0=3.25, thresh=0.0)
        assert (a["n_valid"], a["n_kept"], a["K"], a["scale"], a["slot"]) == (0, 0, 0, 0, 3.25) and (a["drop"] == 1).all()      # the slot is unchanged
    if name == "specials":
        a = select(pp, keep_q16=1)
        assert a["tau_key"] == 0xFFFFFFFF and list(np.flatnonzero(a["drop"] == 0)) == [3] and math.isnan(a["kept_sum"])        # the NaN is the hardest
    if name == "odd":                                    # the mean is ADDED into the slot
        a = select(pp, slot0=2.0)
        assert a["slot"] == 2.0 + a["kept_sum"] / a["n_kept"]


def loss_inputs(kind, M, Cc, seed=9):
    """test_losses_gpu.py's kind of inputs: z = 2 N(0, 1), the last class absent, per-class weights uniform in [0.2, 4]."""
    rng = np.random.default_rng(seed)
    z = 2 * rng.standard_normal((M, Cc))
    if kind in SOFTMAX_KINDS:
        y = np.eye(Cc)[rng.integers(0, Cc - 1, M)]
        p = np.exp(z - z.max(-1, keepdims=True)); p /= p.sum(-1, keepdims=True)
    else:
        y = (rng.random((M, Cc)) < 0.3).astype(np.float64)
        y[:, Cc - 1] = 0
        p = 1 / (1 + np.exp(-z))
    return f32(p), f32(z), f32(y), f32(np.concatenate([rng.uniform(0.2, 4, Cc), np.zeros(8)]))


def loss_opts(kind):
    o = L.LossOpts()
    o.gamma, o.label_smoothing, o.alpha, o.class_balance = (2.0 if kind in LS.FOCAL_KINDS else 0.0), (0.1 if kind in (L.LOSS_FOCAL_CE, L.LOSS_BCE_LOGITS) else 0.0), 0.75, int(kind == L.LOSS_FOCAL_BCE)
    return o


@pytest.mark.parametrize("kind", [L.LOSS_WCE, L.LOSS_CE_LOGITS, L.LOSS_BCE_LOGITS, L.LOSS_FOCAL_CE, L.LOSS_FOCAL_BCE])
def test_select_on_real_loss_maps(kind):
    """The map as the loss entries write it (void pixels 0), with the step's void mask, on B = 2 samples of 33 x 31 pixels."""
    lib = L.lib()
    Cc = 6 if kind in SOFTMAX_KINDS else 3
    p, z, y, a = loss_inputs(kind, M_ODD, Cc)
    rng = np.random.default_rng(4)
    for valid in (None, rng.random(M_ODD) >= 0.3):
        vm = u8(1 - valid.astype(np.uint8)) if valid is not None else None
        out = torch.zeros(1, dtype=torch.float64, device=dev())
        pp = torch.full((M_ODD,), 7.0, device=dev())
        lib.call("rua_pixel_loss_opts", kind, p.data_ptr(), z.data_ptr(), y.data_ptr(), a.data_ptr(), vm.data_ptr() if vm is not None else None,
                 C.byref(loss_opts(kind)), M_ODD, Cc, out.data_ptr(), pp.data_ptr(), stream())
        check(pp, valid, what=f"kind {kind}", keep_q16=16384)
        check(pp, valid, what=f"kind {kind}", keep_q16=1, min_kept=500, thresh=LS.prob_to_thresh(0.7), loss_weight=0.7)


def test_argument_errors_come_before_any_launch():
    lib = L.lib()
    M = 300
    pp = f32(np.linspace(0, 1, M))
    nws = int(lib.raw("rua_ohem_workspace_bytes")(M))
    assert nws > 0 and lib.raw("rua_ohem_workspace_bytes")(0) == -1 and lib.raw("rua_ohem_workspace_bytes")(-5) == -1
    ws = torch.zeros(nws // 8 + 1, dtype=torch.float64, device=dev())
    drop = torch.full((M,), 0xAA, dtype=torch.uint8, device=dev())
    res = torch.full((C.sizeof(L.OhemResult),), 0xFF, dtype=torch.uint8, device=dev())
    slot = torch.full((1,), 1.5, dtype=torch.float64, device=dev())
    err = lambda: lib.dll.rua_last_error().decode()

    def call(M=M, nws=nws, pp=pp, drop=drop, **kw):
        o = L.OhemOpts()
        o.min_kept, o.keep_q16, o.warmup, o.thresh, o.has_thresh = 0, 16384, 0, 0.0, 0
        for k, v in kw.items():
            setattr(o, k, v)
        return lib.raw("rua_ohem_select")(pp.data_ptr() if pp is not None else None, None, M, C.byref(o), None, 1.0, ws.data_ptr(), nws,
                                          drop.data_ptr() if drop is not None else None, slot.data_ptr(), res.data_ptr(), None)
    assert call(M=0) == -1 and "M=" in err()
    assert call(M=-3) == -1
    for q in (0, -1, 65537):
        assert call(keep_q16=q) == -1 and "keep_q16" in err()
    assert call(min_kept=-1) == -1 and "min_kept" in err()
    assert call(warmup=-1) == -1 and "warmup" in err()
    assert call(thresh=float("nan"), has_thresh=1) == -1 and "NaN" in err()
    assert call(has_thresh=2) == -1
    assert call(nws=nws - 8) == -1 and "workspace" in err()
    assert call(nws=0) == -1
    assert call(pp=None) == -1 and call(drop=None) == -1
    assert lib.raw("rua_ohem_select")(pp.data_ptr(), None, M, None, None, 1.0, ws.data_ptr(), nws, drop.data_ptr(), slot.data_ptr(), res.data_ptr(), None) == -1
    torch.cuda.synchronize()
    assert (drop == 0xAA).all() and (res == 0xFF).all() and float(slot[0]) == 1.5 and float(ws.abs().sum()) == 0.0           # nothing was launched
    assert call(thresh=float("nan"), has_thresh=0) == 0                  # a thresh that is not in use is not looked at
    torch.cuda.synchronize()
    assert int((drop == 0).sum()) == 75


def dz_inputs(kind, B, HW, Cc, seed):
    p, z, y, a = loss_inputs(kind, B * HW, Cc, seed)
    rng = np.random.default_rng(seed + 1)
    drop = u8(rng.random(B * HW) < 0.6)
    scale = torch.tensor([0.7 / 1234.0], dtype=torch.float32, device=dev())
    return p, y, a, drop, scale


def dz_opts_ref(kind, p, y, a, o, B, HW, Cc, gs, vm):
    dz = torch.full((B * HW, Cc), 9.0, device=dev())
    L.lib().call("rua_head_dz_opts", kind, ACT_OF[kind], p.data_ptr(), y.data_ptr(), None, a.data_ptr(), gs, B, HW, Cc, vm.data_ptr() if vm is not None else None,
                 C.byref(o), dz.data_ptr(), stream())
    return dz


@pytest.mark.parametrize("kind,Cc", [(L.LOSS_FOCAL_CE, 6), (L.LOSS_CE_LOGITS, 6), (L.LOSS_WCE, 5), (L.LOSS_BCE_LOGITS, 6), (L.LOSS_FOCAL_BCE, 3)])
def test_dz_sel_bytes(kind, Cc):
    """rua_head_dz_sel = rua_head_dz_opts with grad_scale = scale_dev[0] and void_mask = drop_mask, byte for byte: softmax and sigmoid heads, with and
    without options, C = 6, 3 and the runtime-C form."""
    B, HW = 2, 33 * 31
    p, y, a, drop, scale = dz_inputs(kind, B, HW, Cc, 21)
    for o in (loss_opts(kind), L.LossOpts()) if kind not in LS.FOCAL_KINDS else (loss_opts(kind),):
        want = dz_opts_ref(kind, p, y, a, o, B, HW, Cc, float(scale[0]), drop)
        got = torch.full((B * HW, Cc), 5.0, device=dev())
        L.lib().call("rua_head_dz_sel", kind, ACT_OF[kind], p.data_ptr(), y.data_ptr(), None, a.data_ptr(), B, HW, Cc, C.byref(o), drop.data_ptr(), scale.data_ptr(),
                     got.data_ptr(), stream())
        torch.cuda.synchronize()
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
        assert (got[drop.bool()] == 0).all() and got[~drop.bool()].abs().sum() > 0


def head(kind, p, y, a, gs, B, HW, Cc, dz):
    d = L.DzHead()
    d.kind, d.act, d.p, d.y, d.coef, d.class_w, d.grad_scale, d.B, d.HW, d.C, d.dz = kind, ACT_OF[kind], p.data_ptr(), y.data_ptr(), None, a.data_ptr(), gs, B, HW, Cc, dz.data_ptr()
    return d


@pytest.mark.parametrize("with_opts", [True, False])
def test_dz_multi_sel_mixed_launch(with_opts):
    """One launch, three heads: two with a selection of their own, one without - that one gets the bytes of rua_head_dz_multi_opts (its host
    grad_scale, the shared void mask), the others those of rua_head_dz_opts with their scale and mask."""
    lib = L.lib()
    B, HW = 2, 33 * 31
    kinds = [(L.LOSS_FOCAL_CE if with_opts else L.LOSS_WCE, 6), (L.LOSS_BCE_LOGITS, 6), (L.LOSS_CE_LOGITS, 6)]
    data = [dz_inputs(k, B, HW, c, 30 + i) for i, (k, c) in enumerate(kinds)]
    os_ = [loss_opts(k) if with_opts else L.LossOpts() for k, _ in kinds]
    vm = u8(np.random.default_rng(2).random(B * HW) < 0.3)
    gs = 0.5 / (B * HW)
    got = [torch.full((B * HW, c), 5.0, device=dev()) for _, c in kinds]
    heads = (L.DzHead * 3)(*[head(k, d[0], d[1], d[2], gs, B, HW, c, g) for (k, c), d, g in zip(kinds, data, got)])
    sel = (L.DzSel * 3)()
    for i in (0, 1):
        sel[i].drop_mask, sel[i].scale_dev = data[i][3].data_ptr(), data[i][4].data_ptr()
    lib.call("rua_head_dz_multi_sel", heads, (L.LossOpts * 3)(*os_), sel, 3, vm.data_ptr(), stream())
    torch.cuda.synchronize()
    for i in (0, 1):
        k, c = kinds[i]
        want = dz_opts_ref(k, data[i][0], data[i][1], data[i][2], os_[i], B, HW, c, float(data[i][4][0]), data[i][3])
        torch.cuda.synchronize()
        assert torch.equal(got[i].view(torch.int32), want.view(torch.int32)), i
    ref = [torch.full((B * HW, c), 6.0, device=dev()) for _, c in kinds]
    rheads = (L.DzHead * 3)(*[head(k, d[0], d[1], d[2], gs, B, HW, c, g) for (k, c), d, g in zip(kinds, data, ref)])
    lib.call("rua_head_dz_multi_opts", rheads, (L.LossOpts * 3)(*os_), 3, vm.data_ptr(), stream())
    torch.cuda.synchronize()
    assert torch.equal(got[2].view(torch.int32), ref[2].view(torch.int32))
    assert not torch.equal(got[0], ref[0])
    # every sel zeroed: the whole launch is rua_head_dz_multi_opts'
    lib.call("rua_head_dz_multi_sel", heads, (L.LossOpts * 3)(*os_), (L.DzSel * 3)(), 3, vm.data_ptr(), stream())
    torch.cuda.synchronize()
    for i in range(3):
        assert torch.equal(got[i].view(torch.int32), ref[i].view(torch.int32)), i
    # refusals: half a selection, a null table
    bad = (L.DzSel * 3)()
    bad[0].drop_mask = data[0][3].data_ptr()
    assert lib.raw("rua_head_dz_multi_sel")(heads, (L.LossOpts * 3)(*os_), bad, 3, None, None) == -1 and "go together" in lib.dll.rua_last_error().decode()
    assert lib.raw("rua_head_dz_multi_sel")(heads, (L.LossOpts * 3)(*os_), None, 3, None, None) == -1
    assert lib.raw("rua_head_dz_sel")(kinds[2][0], L.ACT_SOFTMAX, data[2][0].data_ptr(), data[2][1].data_ptr(), None, data[2][2].data_ptr(), B, HW, 6,
                                      C.byref(os_[2]), None, None, got[2].data_ptr(), None) == -1
