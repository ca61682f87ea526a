"""The Lovasz-Softmax definitions on the host (no GPU): losses.host_lovasz against an independent restatement of the paper's lovasz_grad, its
gradient against central differences, the tie rule, host_lovasz_dz against the fp64 chain rule, the option and head checks, the checkpoint
metadata round trip and the C ABI's declarations."""
import ctypes
import os

import numpy as np
import pytest

from resunet_a_mltsk_keras_amd import _lib as L
from resunet_a_mltsk_keras_amd import losses as LS
from resunet_a_mltsk_keras_amd.engine import LossSpec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def paper(p, y, void=None, classes="present"):
    """lovasz_softmax_flat / lovasz_grad of the paper's code, restated with np.cumsum in float64: per class errors sorted descending (stable, on
    the float32 errors themselves), jaccard = 1 - (gts - cumsum(fg)) / (gts + cumsum(1 - fg)), grad = its first difference."""
    p = np.asarray(p, np.float32)
    Cc = p.shape[-1]
    p, y = p.reshape(-1, Cc), np.asarray(y).reshape(-1, Cc)
    keep = np.flatnonzero(np.ones(len(p), bool) if void is None else np.asarray(void).reshape(-1) == 0)
    dp = np.zeros(p.shape, np.float32)
    losses, perms, grads = [], [], []
    for c in range(Cc):
        fg = (y[keep, c] > 0.5).astype(np.float64)
        err = np.abs(fg.astype(np.float32) - p[keep, c])
        perm = np.argsort(-err.astype(np.float64), kind="stable")
        fs = fg[perm]
        gts = fs.sum()
        inter = gts - np.cumsum(fs)
        union = gts + np.cumsum(1.0 - fs)
        jac = 1.0 - inter / union
        grad = jac.copy()
        grad[1:] = jac[1:] - jac[:-1]
        perms.append(keep[perm]); grads.append(grad)
        if len(keep) and (classes == "all" or gts > 0):
            losses.append(float(np.dot(err[perm].astype(np.float64), grad)))
            dp[keep[perm], c] = np.where(fs == 1, -grad, grad).astype(np.float32)
    return (sum(losses) / len(losses) if losses else 0.0), perms, grads, dp, len(losses)


def softmax_case(rng, M, Cc, absent=None):
    z = 2 * rng.standard_normal((M, Cc))
    p = np.exp(z - z.max(-1, keepdims=True))
    p = (p / p.sum(-1, keepdims=True)).astype(np.float32)
    cls = rng.integers(0, Cc, M)
    if absent is not None:
        cls = np.where(cls == absent, (absent + 1) % Cc, cls)
    return p, np.eye(Cc, dtype=np.float32)[cls]


def sigmoid_case(rng, M, Cc):
    p = (1 / (1 + np.exp(-2 * rng.standard_normal((M, Cc))))).astype(np.float32)
    return p, (rng.random((M, Cc)) < 0.3).astype(np.float32)


def agree(p, y, void=None, classes="present"):
    h = LS.host_lovasz(p, y, void, classes)
    loss, perms, grads, dp, ncls = paper(p, y, void, classes)
    Cc = p.shape[-1]
    assert h["n_cls"] == ncls and h["n_valid"] == (p.reshape(-1, Cc).shape[0] if void is None else int((np.asarray(void).reshape(-1) == 0).sum()))
    for c in range(Cc):
        assert np.array_equal(h["order"][c], perms[c]), c
        assert np.array_equal(h["w"][c].view(np.uint64), grads[c].view(np.uint64)), c      # the integers are exact: the same bits
        assert (h["w"][c] >= 0).all()
    assert np.array_equal(h["dp"].reshape(-1, Cc).view(np.uint32), dp.view(np.uint32))
    assert abs(h["loss"] - loss) <= 1e-12 * max(abs(loss), 1e-300) or h["loss"] == loss
    return h


@pytest.mark.parametrize("classes", ["present", "all"])
def test_host_lovasz_is_the_papers(classes):
    rng = np.random.default_rng(3)
    p, y = softmax_case(rng, 700, 6)
    agree(p, y, None, classes)
    agree(p.reshape(2, 10, 35, 6), y.reshape(2, 10, 35, 6), None, classes)
    void = rng.random(700) < 0.3
    agree(p, y, void, classes)
    ps, ys = sigmoid_case(rng, 500, 3)
    agree(ps, ys, None, classes)
    agree(ps, ys, rng.random(500) < 0.3, classes)
    pa, ya = softmax_case(rng, 400, 5, absent=4)
    h = agree(pa, ya, None, classes)
    assert h["G"][4] == 0 and h["n_cls"] == (4 if classes == "present" else 5)
    if classes == "all":
        assert h["loss_c"][4] == float(pa[:, 4].max()) and h["w"][4][0] == 1.0 and not h["w"][4][1:].any()
    else:
        assert h["loss_c"][4] == 0.0 and not h["dp"][:, 4].any()
    h = agree(p, y, np.ones(700, bool), classes)                      # all void
    assert (h["loss"], float(h["scale"]), h["n_valid"], h["n_cls"]) == (0.0, 0.0, 0, 0) and not h["dp"].any()
    h = agree(p[:1], y[:1], None, classes)                            # M = 1
    assert h["n_valid"] == 1
    full = LS.host_lovasz(p, y, None, classes, loss_weight=0.3)
    assert full["n_cls"] == 6 and float(full["scale"]) == float(np.float32(np.float64(np.float32(0.3)) / 6))


def test_gradient_matches_central_differences():
    """Errors pairwise distinct: the order is locally constant and the loss is linear in p there, so central differences of the fp64 loss give
    dp: the sign convention and the rank -> pixel scatter."""
    rng = np.random.default_rng(8)
    M, Cc = 40, 3
    for make in (softmax_case, sigmoid_case):
        p, y = make(rng, M, Cc)
        fg = y > 0.5
        e = np.abs(fg.astype(np.float32) - p)
        gap = min(np.diff(np.sort(e[:, c])).min() for c in range(Cc))
        assert gap > 0
        h = LS.host_lovasz(p, y)

        def f64_loss(q):
            tot, n = 0.0, 0
            for c in range(Cc):
                err = np.abs(fg[:, c].astype(np.float64) - q[:, c])
                perm = np.argsort(-err, kind="stable")
                fs = fg[perm, c].astype(np.float64)
                G = fs.sum()
                if G == 0:
                    continue
                jac = 1.0 - (G - np.cumsum(fs)) / (G + np.cumsum(1 - fs))
                tot += float(np.dot(err[perm], np.diff(np.concatenate([[0.0], jac]))))
                n += 1
            return tot / n
        d = float(gap) / 4
        num = np.zeros((M, Cc))
        q0 = p.astype(np.float64)
        for i in range(M):
            for c in range(Cc):
                qp, qm = q0.copy(), q0.copy()
                qp[i, c] += d; qm[i, c] -= d
                num[i, c] = (f64_loss(qp) - f64_loss(qm)) / (2 * d)
        ana = h["dp"].astype(np.float64) / h["n_cls"]
        assert np.abs(num - ana).max() <= 1e-6 * np.abs(ana).max()


def test_ties_go_in_ascending_pixel_index():
    rng = np.random.default_rng(4)
    M = 90
    vals = np.array([0.25, 0.5, 0.125], np.float32)
    p = vals[rng.integers(0, 3, (M, 2))]
    y = (rng.random((M, 2)) < 0.4).astype(np.float32)
    h = LS.host_lovasz(p, y, classes="all")
    for c in range(2):
        e = np.abs((y[:, c] > 0.5).astype(np.float32) - p[:, c])
        o = h["order"][c]
        assert sorted(o) == list(range(M))
        for a, b in zip(o[:-1], o[1:]):
            assert e[a] > e[b] or (e[a] == e[b] and a < b)
    agree(p, y, None, "all")


@pytest.mark.parametrize("act", [L.ACT_SOFTMAX, L.ACT_SIGMOID])
def test_host_dz_is_the_chain_rule(act):
    rng = np.random.default_rng(6)
    p, y = softmax_case(rng, 300, 6) if act == L.ACT_SOFTMAX else sigmoid_case(rng, 300, 6)
    void = rng.random(300) < 0.3
    h = LS.host_lovasz(p, y, void, loss_weight=0.7)
    pj = p.copy()
    pj[void] = np.nan
    dz = LS.host_lovasz_dz(act, pj, h["dp"], h["scale"])
    assert dz.dtype == np.float32 and not dz[void].view(np.uint32).any()
    g, q, sc = h["dp"].astype(np.float64), p.astype(np.float64), float(h["scale"])
    ref = sc * q * (g - (g * q).sum(-1, keepdims=True)) if act == L.ACT_SOFTMAX else sc * g * q * (1 - q)
    assert np.abs(dz[~void] - ref[~void]).max() <= 1e-6 * np.abs(ref[~void]).max()
    with pytest.raises(ValueError):
        LS.host_lovasz_dz(L.ACT_NONE, p, h["dp"], 1.0)


def test_option_and_head_checks():
    assert LS.lovasz_options() == dict(classes="present")
    LS.check_lovasz(LS.lovasz_options("all"), head="seg", num_classes=6)
    LS.check_lovasz({}, head="bound", num_classes=16)
    for bad in (dict(classes="some"), dict(per_image=True), "present"):
        with pytest.raises(ValueError):
            LS.check_lovasz(bad)
    for head in ("dist", "color"):
        with pytest.raises(ValueError, match="continuous"):
            LS.check_lovasz({}, head=head)
    with pytest.raises(ValueError):
        LS.check_lovasz({}, head="seg", num_classes=17)
    with pytest.raises(ValueError):
        LS.host_lovasz(np.zeros((2, 2), np.float32), np.zeros((2, 2)), classes="some")
    from resunet_a_mltsk_keras_amd import keras_api as K
    assert K.LovaszSoftmax.kind == L.LOSS_LOVASZ == 7 and K._LOSS_NAMES["lovasz"] == K._LOSS_NAMES["lovasz_softmax"] == L.LOSS_LOVASZ
    assert K._loss_kind("lovasz", "seg")[0] == L.LOSS_LOVASZ and K._loss_kind(K.LovaszSoftmax("all"), "bound")[0] == L.LOSS_LOVASZ
    for head in ("dist", "color"):
        with pytest.raises(ValueError, match="continuous"):
            K._loss_kind(K.LovaszSoftmax(), head)
    with pytest.raises(ValueError):
        K.LovaszSoftmax(classes="each")


def test_metadata_round_trip():
    heads = ("seg", "bound", "dist", "color")
    sp = LossSpec(kind=dict(seg=L.LOSS_LOVASZ, bound=L.LOSS_LOVASZ, dist=L.LOSS_MSE, color=L.LOSS_MSE), weight={h: 1.0 for h in heads},
                  lovasz=dict(seg=LS.lovasz_options("all")))
    lo = sp.loss_options()
    assert lo == dict(lovasz=dict(seg=dict(classes="all"), bound=dict(classes="present")))
    import json
    back = LS.options_from_meta(json.loads(json.dumps(lo)))
    assert back[LS.LOVASZ_KEY] == lo["lovasz"] and all(back[k] == {} for k in LS.OPTION_KEYS) and LS.OHEM_KEY not in back
    assert LossSpec(kind=sp.kind, weight=sp.weight, **back).loss_options() == lo
    plain = LossSpec(kind={h: L.LOSS_TANIMOTO for h in heads}, weight={h: 1.0 for h in heads})
    assert plain.loss_options() == {} and LS.LOVASZ_KEY not in LS.options_from_meta({}) and plain.head_lovasz("seg") is None


def test_abi_matches_the_header():
    hdr = open(os.path.join(ROOT, "include", "rua_hip.h")).read()
    assert "#define RUA_LOSS_LOVASZ 7" in hdr and "#define RUA_LOVASZ_MAX_C 16" in hdr
    assert "int64_t n_valid; int32_t n_cls; float scale; int64_t G[RUA_LOVASZ_MAX_C]; double loss_c[RUA_LOVASZ_MAX_C]; double loss;" in hdr
    R = L.LovaszResult
    assert ctypes.sizeof(R) == 16 + 128 + 128 + 8 and (R.n_cls.offset, R.scale.offset, R.G.offset, R.loss_c.offset, R.loss.offset) == (8, 12, 16, 144, 272)
    for sym in ("rua_lovasz_tile", "rua_lovasz_workspace_bytes", "rua_lovasz_grad", "rua_lovasz_dz"):
        assert sym in L.EXPORTED_SYMBOLS and sym in hdr
    from resunet_a_mltsk_keras_amd import build as B
    assert "lovasz.hip" in B.SOURCES
    src = open(os.path.join(ROOT, "resunet_a_mltsk_keras_amd", "csrc", "lovasz.hip")).read()
    assert "__dmul_rn" in src and "__fmul_rn" in src and "__fadd_rn" in src      # the slot and dz: nothing contracted
