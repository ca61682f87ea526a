"""The Lovasz-Softmax loss through the C ABI: rua_lovasz_grad against losses.host_lovasz - the sorted order, dp, the counts and the normaliser bit for
bit, the fp64 sums within n * 2^-52 (every term is non-negative: the bound of any summation order), two calls bit-identical, the slot
slot0 + loss_weight * loss -, rua_lovasz_dz against host_lovasz_dz's bits, and the argument refusals.

Shapes: with T = rua_lovasz_tile() M = 1, 63, 64, 65 (one wave and its neighbours), T - 1, T, T + 1 (one tile and its neighbours), 3 T + 17 (four
tiles, the last partial) at C = 6; C = 1 and C = 16 at M = T + 1.  The contents make every digit pass of the sort matter."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from resunet_a_mltsk_keras_amd import _lib as L
from resunet_a_mltsk_keras_amd import losses as LS

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda", 0)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev())


def tile():
    return int(L.lib().raw("rua_lovasz_tile")())


def grad(p, y, void=None, classes="present", loss_weight=1.0, slot0=0.0):
    """One rua_lovasz_grad with the workspace filled with NaN bytes and every output with sentinels."""
    lib = L.lib()
    M, Cc = p.shape
    pd, yd = f32(p), f32(y)
    vm = torch.from_numpy(np.ascontiguousarray(void, np.uint8)).to(dev()) if void is not None else None
    nws = int(lib.raw("rua_lovasz_workspace_bytes")(M, Cc))
    assert nws > 0
    ws = torch.full((nws // 8 + 1,), float("nan"), dtype=torch.float64, device=dev())
    dp = torch.full((M, Cc), 7.0, dtype=torch.float32, device=dev())
    order = torch.full((Cc, M), 0x7FFFFFFF, dtype=torch.int32, device=dev())
    res = torch.full((C.sizeof(L.LovaszResult),), 0xFF, dtype=torch.uint8, device=dev())
    slot = torch.full((1,), slot0, dtype=torch.float64, device=dev())
    lib.call("rua_lovasz_grad", pd.data_ptr(), yd.data_ptr(), vm.data_ptr() if vm is not None else None, M, Cc, int(classes == "all"), loss_weight,
             ws.data_ptr(), nws, slot.data_ptr(), dp.data_ptr(), order.data_ptr(), res.data_ptr(), stream())
    torch.cuda.synchronize()
    r = LS.lovasz_result(res.cpu().numpy().tobytes())
    r.update(dp=dp.cpu().numpy(), order=order.cpu().numpy().astype(np.int64), slot=float(slot[0]))
    return r


def same_f64(a, b):
    return a == b or (a != a and b != b)


def check(p, y, void=None, classes="present", loss_weight=1.0, slot0=0.0, what=""):
    p, y = np.ascontiguousarray(p, np.float32), np.ascontiguousarray(y, np.float32)
    Cc = p.shape[1]
    host = LS.host_lovasz(p, y, void, classes, loss_weight)
    a = grad(p, y, void, classes, loss_weight, slot0)
    b = grad(p, y, void, classes, loss_weight, slot0)
    n = host["n_valid"]
    tag = (what, classes, p.shape)
    assert (a["n_valid"], a["n_cls"]) == (n, host["n_cls"]), tag
    assert a["G"][:Cc] == host["G"] and a["G"][Cc:] == [0] * (16 - Cc), tag
    assert np.float32(a["scale"]).view(np.uint32) == np.float32(host["scale"]).view(np.uint32), tag
    for c in range(Cc):
        assert np.array_equal(a["order"][c, :n], host["order"][c]), tag + (c,)
    assert np.array_equal(a["dp"].view(np.uint32), host["dp"].view(np.uint32)), tag
    bound = max(n, 1) * 2.0 ** -52
    for c in range(Cc):
        h = host["loss_c"][c]
        if math.isfinite(h):
            assert abs(a["loss_c"][c] - h) <= bound * abs(h), tag + (c, a["loss_c"][c], h)
        else:
            assert math.isnan(a["loss_c"][c]) and math.isnan(h), tag + (c,)
    if math.isfinite(host["loss"]):
        assert abs(a["loss"] - host["loss"]) <= bound * abs(host["loss"]), tag
        want = slot0 + float(np.float32(loss_weight)) * a["loss"] if host["n_cls"] else slot0
        assert a["slot"] == want, tag
        assert abs(a["slot"] - (slot0 + float(np.float32(loss_weight)) * host["loss"])) <= bound * abs(host["loss"]) * abs(loss_weight) + 2.0 ** -52 * abs(slot0), tag
    else:
        assert math.isnan(a["loss"]) and math.isnan(a["slot"]), tag
    if host["n_cls"] == 0:
        assert a["loss"] == 0.0 and a["scale"] == 0 and not a["dp"].any() and a["slot"] == slot0, tag
    for k in ("n_valid", "n_cls", "G", "slot", "loss"):
        assert a[k] == b[k] or (k in ("slot", "loss") and same_f64(a[k], b[k])), tag + (k,)
    assert all(same_f64(u, v) for u, v in zip(a["loss_c"], b["loss_c"])), tag
    assert np.array_equal(a["dp"].view(np.uint32), b["dp"].view(np.uint32)) and np.array_equal(a["order"][:, :n], b["order"][:, :n]), tag
    return a, host


def softmax_rows(rng, M, Cc):
    z = 2 * rng.standard_normal((M, Cc))
    p = np.exp(z - z.max(-1, keepdims=True))
    return (p / p.sum(-1, keepdims=True)).astype(np.float32)


def onehot(rng, M, Cc, absent=None):
    cls = rng.integers(0, Cc, M)
    if absent is not None and Cc > 1:
        cls = np.where(cls == absent, (absent + 1) % Cc, cls)
    return np.eye(Cc, dtype=np.float32)[cls]


def byte_keys(rng, M, Cc, shift):
    """Errors whose keys differ in one byte only: built from bit patterns, as test_ohem_gpu.synthetic does.  y = 0 everywhere but in pixel 0 of
    every class (so that the classes are present): the error is p itself."""
    base = np.float32(0.3).view(np.uint32) & np.uint32(~(0xFF << shift) & 0xFFFFFFFF)
    if shift == 24:                                      # the highest byte of a non-negative float below 1: the exponents 0x00 .. 0x3E
        base = np.float32(0.3).view(np.uint32) & np.uint32(0x00FFFFFF)
        b = rng.integers(0, 0x3F, (M, Cc)).astype(np.uint32)
    else:
        b = rng.integers(0, 256, (M, Cc)).astype(np.uint32)
    p = (base | (b << np.uint32(shift))).astype(np.uint32).view(np.float32)
    y = np.zeros((M, Cc), np.float32)
    y[0, :] = 1
    return p, y


SHAPES = [(1, 6), (63, 6), (64, 6), (65, 6), ("T-1", 6), ("T", 6), ("T+1", 6), ("3T+17", 6), ("T+1", 1), ("T+1", 16)]


def resolve(M):
    T = tile()
    return {"T-1": T - 1, "T": T, "T+1": T + 1, "3T+17": 3 * T + 17}.get(M, M)


@pytest.mark.parametrize("M,Cc", SHAPES)
def test_grad_equals_host(M, Cc):
    M = resolve(M)
    rng = np.random.default_rng(1000 + M + Cc)
    p, y = softmax_rows(rng, M, Cc), onehot(rng, M, Cc)
    check(p, y, what="random")
    check(p, y, classes="all", loss_weight=0.3, slot0=2.5, what="random, weighted, slot")
    check(np.full((M, Cc), 1.0 / Cc, np.float32), y, what="uniform")
    for shift in (0, 24):
        pb, yb = byte_keys(rng, M, Cc, shift)
        check(pb, yb, what=f"byte {shift}")
    void = (rng.random(M) < 0.3).astype(np.uint8)
    pv = p.copy()
    pv[void != 0] = np.nan                               # a void pixel's probabilities are never looked at
    check(pv, y, void, what="void30")
    a, _ = check(p, y, np.ones(M, np.uint8), slot0=3.25, what="all void")
    assert (a["n_valid"], a["n_cls"], a["slot"]) == (0, 0, 3.25)
    ya = onehot(rng, M, Cc, absent=Cc - 1)
    a, h = check(p, ya, what="absent")
    b, _ = check(p, ya, classes="all", what="absent")
    if Cc > 1:
        assert a["G"][Cc - 1] == 0 and a["n_cls"] < Cc and b["n_cls"] == Cc and not a["dp"][:, Cc - 1].any()
        assert b["loss_c"][Cc - 1] == float(p[:, Cc - 1].max())          # G = 0: w_0 = 1, the class loss is the largest error
    pn = p.copy()
    pn[M // 2, :] = np.nan
    a, _ = check(pn, y, what="nan row")
    assert math.isnan(a["loss"]) and np.isfinite(a["dp"]).all() and all(a["order"][c, 0] == M // 2 for c in range(Cc))


@pytest.mark.parametrize("act", [L.ACT_SOFTMAX, L.ACT_SIGMOID])
def test_dz_bits(act):
    lib = L.lib()
    M, Cc = 1000, 6
    rng = np.random.default_rng(5)
    if act == L.ACT_SOFTMAX:
        p, y = softmax_rows(rng, M, Cc), onehot(rng, M, Cc)
    else:
        p = (1 / (1 + np.exp(-2 * rng.standard_normal((M, Cc))))).astype(np.float32)
        y = (rng.random((M, Cc)) < 0.3).astype(np.float32)
    void = (rng.random(M) < 0.3).astype(np.uint8)
    host = LS.host_lovasz(p, y, void, "present", 0.7)
    pj = p.copy()
    pj[void != 0] = np.nan                               # void pixels leave as +0.0f whatever p holds
    pd, gd = f32(pj), f32(host["dp"])
    sc = torch.tensor([float(host["scale"])], dtype=torch.float32, device=dev())
    dz = torch.full((M, Cc), 9.0, dtype=torch.float32, device=dev())
    lib.call("rua_lovasz_dz", act, pd.data_ptr(), gd.data_ptr(), sc.data_ptr(), M, Cc, dz.data_ptr(), stream())
    torch.cuda.synchronize()
    got = dz.cpu().numpy()
    want = LS.host_lovasz_dz(act, pj, host["dp"], host["scale"])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert not got[void != 0].view(np.uint32).any() and np.abs(got[void == 0]).sum() > 0


def test_argument_errors_come_before_any_launch():
    lib = L.lib()
    M, Cc = 300, 6
    rng = np.random.default_rng(2)
    p, y = f32(softmax_rows(rng, M, Cc)), f32(onehot(rng, M, Cc))
    wsb = lib.raw("rua_lovasz_workspace_bytes")
    nws = int(wsb(M, Cc))
    assert nws > 0 and wsb(0, 6) == -1 and wsb(M, 17) == -1 and wsb(M, 0) == -1 and wsb(1 << 31, 1) == -1 and wsb(1 << 30, 4) == -1
    ws = torch.zeros(nws // 8 + 1, dtype=torch.float64, device=dev())
    big = torch.zeros(17 * M, dtype=torch.float32, device=dev())
    dp = torch.full((M * 17,), 7.0, dtype=torch.float32, device=dev())
    order = torch.full((17 * M,), 0x7FFFFFFF, dtype=torch.int32, device=dev())
    res = torch.full((C.sizeof(L.LovaszResult),), 0xFF, dtype=torch.uint8, device=dev())
    slot = torch.full((1,), 1.5, dtype=torch.float64, device=dev())
    err = lambda: lib.dll.rua_last_error().decode()

    def call(M=M, Cc=Cc, nws=nws, p=p, y=y, ws=ws, allc=0):
        return lib.raw("rua_lovasz_grad")(p.data_ptr() if p is not None else None, y.data_ptr() if y is not None else None, None, M, Cc, allc, 1.0,
                                          ws.data_ptr() if ws is not None else None, nws, slot.data_ptr(), dp.data_ptr(), order.data_ptr(), res.data_ptr(), None)
    assert call(Cc=17, p=big, y=big, nws=1 << 40) == -1 and "C=" in err()
    assert call(Cc=0) == -1
    assert call(nws=nws - 8) == -1 and "workspace" in err()
    assert call(nws=0) == -1
    assert call(p=None) == -1 and call(y=None) == -1 and call(ws=None) == -1
    assert call(M=0) == -1 and call(M=-4) == -1 and call(M=1 << 31, Cc=1, nws=1 << 50) == -1 and "M=" in err()
    assert call(M=1 << 30, Cc=4, nws=1 << 50) == -1 and "2^32" in err()      # tiny real buffers: refused before anything touches them
    assert call(allc=2) == -1
    sc = torch.ones(1, dtype=torch.float32, device=dev())
    dzr = lib.raw("rua_lovasz_dz")
    assert dzr(L.ACT_NONE, p.data_ptr(), p.data_ptr(), sc.data_ptr(), M, Cc, dp.data_ptr(), None) == -1
    assert dzr(L.ACT_SOFTMAX, None, p.data_ptr(), sc.data_ptr(), M, Cc, dp.data_ptr(), None) == -1
    assert dzr(L.ACT_SOFTMAX, p.data_ptr(), p.data_ptr(), None, M, Cc, dp.data_ptr(), None) == -1
    assert dzr(L.ACT_SOFTMAX, p.data_ptr(), p.data_ptr(), sc.data_ptr(), M, 17, dp.data_ptr(), None) == -1
    torch.cuda.synchronize()
    assert (dp == 7.0).all() and (order == 0x7FFFFFFF).all() and (res == 0xFF).all() and float(slot[0]) == 1.5 and float(ws.abs().sum()) == 0.0
    assert call() == 0                                   # ... and the same buffers are fine
    torch.cuda.synchronize()
    assert float(slot[0]) > 1.5
