"""Host side of the focal losses and label smoothing (no GPU): losses.host_* against a torch-fp64 restatement written here, the identities that
tie them to the cross-entropies the project already had, losses.check_options, train_ISPRS.py's flags and the checkpoint metadata.  The formulas
are this project's statement of Keras 3's (losses.py); no Keras is installed here to run against."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from resunet_a_mltsk_keras_amd import _lib as L
from resunet_a_mltsk_keras_amd import h5lite
from resunet_a_mltsk_keras_amd import keras_api as ka
from resunet_a_mltsk_keras_amd import losses as LS
from resunet_a_mltsk_keras_amd.engine import LossSpec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-7


def case(C, seed=9, M=97, sigmoid=False):
    rng = np.random.default_rng(seed)
    z = 2 * rng.standard_normal((M, C))
    if sigmoid:
        p = 1 / (1 + np.exp(-z))
        y = (rng.random((M, C)) < 0.3).astype(np.float64)
    else:
        p = np.exp(z - z.max(1, keepdims=True)); p /= p.sum(1, keepdims=True)
        y = np.eye(C)[rng.integers(0, C, M)]
    return y, p, rng.uniform(0.2, 4, C)


def t_focal_ce(y, p, a, g, e):
    y, p, a = (torch.from_numpy(np.asarray(v, np.float64)) for v in (y, p, a))
    C = y.shape[-1]
    t = y * (1 - e) + e / C
    u = torch.clamp(p / p.sum(-1, keepdim=True), EPS, 1 - EPS)
    f = torch.ones_like(u) if g == 0 else torch.pow(1 - u, g)
    return (-(a * t * f * torch.log(u)).sum(-1)).numpy()


def t_focal_bce(y, p, g, alpha, balance, e):
    y, p = (torch.from_numpy(np.asarray(v, np.float64)) for v in (y, p))
    t = y * (1 - e) + e / 2
    o = torch.clamp(p, EPS, 1 - EPS)
    bce = -(t * torch.log(o) + (1 - t) * torch.log(1 - o))
    pt = t * p + (1 - t) * (1 - p)
    f = torch.ones_like(pt) if g == 0 else torch.pow(1 - pt, g)
    w = t * alpha + (1 - t) * (1 - alpha) if balance else 1.0
    return (w * f * bce).mean(-1).numpy()


@pytest.mark.parametrize("C", [3, 5, 6])
@pytest.mark.parametrize("g", [0.0, 1.0, 2.0, 3.5])
@pytest.mark.parametrize("e", [0.0, 0.1])
def test_host_categorical_focal_is_the_formula(C, g, e):
    y, p, a = case(C)
    got = LS.host_categorical_focal(y, p, a, g, e)
    want = t_focal_ce(y, p, a, g, e)
    assert got.shape == (y.shape[0],) and got.dtype == np.float64
    assert np.abs(got - want).max() <= 1e-13 * max(1.0, np.abs(want).max())
    # Keras' scalar alpha is that scalar in every class
    assert np.array_equal(LS.host_categorical_focal(y, p, 0.25, g, e), LS.host_categorical_focal(y, p, [0.25] * C, g, e))


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("g", [0.0, 1.0, 2.0, 3.5])
@pytest.mark.parametrize("e,balance", [(0.0, False), (0.1, True), (0.0, True)])
def test_host_binary_focal_is_the_formula(C, g, e, balance):
    y, p, _ = case(C, sigmoid=True)
    got = LS.host_binary_focal(y, p, g, 0.3, balance, e)
    want = t_focal_bce(y, p, g, 0.3, balance, e)
    assert got.shape == (y.shape[0],)
    assert np.abs(got - want).max() <= 1e-13 * max(1.0, np.abs(want).max())


def test_identities():
    y, p, W = case(5)
    u = np.clip(p / p.sum(1, keepdims=True), EPS, 1 - EPS)
    cce = -(y * np.log(u)).sum(1)
    assert np.allclose(LS.host_categorical_focal(y, p, 1.0, 0.0, 0.0), cce, rtol=1e-14, atol=0)                       # gamma 0, a 1, e 0: categorical CE
    assert np.allclose(LS.host_categorical_focal(y, p, W, 0.0, 0.0), -(W * y * np.log(u)).sum(1), rtol=1e-14, atol=0)  # a = W: weighted CE
    yb, pb, _ = case(3, sigmoid=True)
    o = np.clip(pb, EPS, 1 - EPS)
    bce = -(yb * np.log(o) + (1 - yb) * np.log(1 - o)).mean(1)
    assert np.allclose(LS.host_binary_focal(yb, pb, 0.0), bce, rtol=1e-14, atol=0)                                     # binary gamma 0, no balancing: BCE
    for e in (0.0, 0.1, 0.9):
        t = LS.host_smooth(y, e)
        assert np.abs(t.sum(-1) - 1).max() < 1e-15 and t.min() >= 0
        tb = LS.host_smooth(yb, e, binary=True)
        assert np.abs(tb + LS.host_smooth(1 - yb, e, binary=True) - 1).max() < 1e-15     # the two outcomes of a channel still sum to 1
    assert np.array_equal(LS.host_smooth(y, 0.0), y)
    # gamma 0 is factor 1 exactly, also where 1 - u or 1 - p_t is 0 (no 0^0, no 0 * inf)
    edge_p = np.array([[1.0, 0.0, 0.0]]); edge_y = np.array([[1.0, 0.0, 0.0]])
    assert np.isfinite(LS.host_categorical_focal(edge_y, edge_p, 1.0, 0.0)).all() and np.isfinite(LS.host_binary_focal(edge_y, edge_p, 0.0)).all()
    assert LS.host_binary_focal(edge_y, edge_p, 2.0)[0] == 0.0


def test_check_options_range():
    ok = LS.check_options
    for g in (0, 1, 2, 3.5, 8):
        ok(L.LOSS_FOCAL_CE, 6, g, [1] * 6, False, 0.1)
        ok(L.LOSS_FOCAL_BCE, 3, g, 0.25, True, 0.0)
    for g in (0.5, 1e-3, 0.999, 8.5, -1, float("nan")):
        for kind in LS.FOCAL_KINDS:
            with pytest.raises(ValueError, match="gamma"):
                ok(kind, 3, g, [1] * 3 if kind == L.LOSS_FOCAL_CE else 0.5, True, 0.0)
    for e in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="label_smoothing"):
            ok(L.LOSS_WCE, 5, label_smoothing=e)
    for kind in (L.LOSS_TANIMOTO, L.LOSS_MSE):
        ok(kind, 5)
        with pytest.raises(ValueError, match="no label smoothing"):
            ok(kind, 5, label_smoothing=0.1)
    with pytest.raises(ValueError, match="alpha values"):
        ok(L.LOSS_FOCAL_CE, 6, 2, [1] * 5)
    with pytest.raises(ValueError, match="not negative"):
        ok(L.LOSS_FOCAL_CE, 3, 2, [1, -1, 1])
    with pytest.raises(ValueError, match="at most 8"):
        ok(L.LOSS_FOCAL_CE, 9, 2, [1] * 9)
    for a in (-0.1, 1.1):
        with pytest.raises(ValueError, match="alpha"):
            ok(L.LOSS_FOCAL_BCE, 3, 2, a, True)
    ok(L.LOSS_FOCAL_BCE, 3, 2, 7.0, False)                       # without balancing alpha is not looked at


def test_loss_objects_carry_their_options():
    f = ka.CategoricalFocalCrossentropy()
    assert (f.kind, f.alpha, f.gamma, f.label_smoothing) == (L.LOSS_FOCAL_CE, 0.25, 2.0, 0.0) and f.alpha_vector(3) == [0.25] * 3
    assert ka.CategoricalFocalCrossentropy(alpha=[1, 2, 3]).alpha_vector(3) == [1.0, 2.0, 3.0]
    b = ka.BinaryFocalCrossentropy()
    assert (b.kind, b.apply_class_balancing, b.alpha, b.gamma, b.label_smoothing) == (L.LOSS_FOCAL_BCE, False, 0.25, 2.0, 0.0)
    assert ka.CategoricalCrossentropy().label_smoothing == 0.0 and ka.BinaryCrossentropy(label_smoothing=0.2).label_smoothing == 0.2
    assert ka.weighted_categorical_crossentropy([1, 2], label_smoothing=0.1).label_smoothing == 0.1
    assert ka._LOSS_NAMES["categorical_focal_crossentropy"] == L.LOSS_FOCAL_CE and ka._LOSS_NAMES["binary_focal_crossentropy"] == L.LOSS_FOCAL_BCE
    for loss, head in ((f, "bound"), (f, "color"), ("categorical_focal_crossentropy", "bound")):
        with pytest.raises(ValueError, match="softmax head"):
            ka._loss_kind(loss, head)
    for loss, head in ((b, "seg"), (b, "dist"), ("binary_focal_crossentropy", "seg")):
        with pytest.raises(ValueError, match="sigmoid head"):
            ka._loss_kind(loss, head)
    opts = {k: {} for k in LS.OPTION_KEYS}
    ka._loss_head_options(ka.BinaryFocalCrossentropy(True, 0.4, 3.0, 0.1), "bound", opts)
    ka._loss_head_options(ka.CategoricalCrossentropy(), "seg", opts)
    assert opts == dict(focal_gamma={"bound": 3.0}, focal_alpha={"bound": 0.4}, class_balance={"bound": True}, label_smoothing={"bound": 0.1})


def cli():
    sys.path.insert(0, ROOT)
    import train_ISPRS
    return train_ISPRS


def test_check_loss_flags():
    c = cli()
    parse = lambda s: c.build_parser().parse_args(s.split())
    a = parse("")
    assert (a.focal_gamma, a.focal_alpha, a.bound_alpha, a.label_smoothing) == (2.0, None, None, 0.0)
    assert c.check_loss_flags(a) is None
    assert c.check_loss_flags(parse("--loss focal")) is None
    assert c.check_loss_flags(parse("--loss focal --focal_alpha 0.5 --num_classes 3")) == [0.5] * 3
    assert c.check_loss_flags(parse("--loss focal --focal_alpha 1 2 3 --num_classes 3 --focal_gamma 0 --label_smoothing 0.1")) == [1.0, 2.0, 3.0]
    assert c.check_loss_flags(parse("--loss focal --multitasking yes --bound_alpha 0.75")) is None
    assert c.check_loss_flags(parse("--loss cross_entropy --label_smoothing 0.1")) is None
    assert c.check_loss_flags(parse("--label_smoothing 0.1")) is None
    # --class_weights with --loss focal: the per-class alpha as given
    a = parse("--loss focal --focal_gamma 0 --class_weights 1 2 3 4 5")
    assert c.check_class_flags(a) == [1.0, 2.0, 3.0, 4.0, 5.0] and c.check_loss_flags(a) is None
    assert c.check_class_flags(parse("--loss focal --class_weights auto --scene_dataset yes")) == "auto"
    for bad, word in (("--loss tanimoto --label_smoothing 0.1", "Tanimoto"), ("--loss focal --focal_gamma 0.5", "gamma"),
                      ("--loss focal --focal_gamma 9", "gamma"), ("--focal_gamma 3", "--loss focal"), ("--focal_alpha 0.3", "--loss focal"),
                      ("--loss cross_entropy --bound_alpha 0.3", "--loss focal"), ("--loss focal --focal_alpha 1 2", "one per class"),
                      ("--loss focal --focal_alpha -1", "not negative"), ("--loss focal --bound_alpha 0.5", "--multitasking"),
                      ("--loss focal --multitasking yes --bound_alpha 1.5", "alpha"), ("--loss focal --label_smoothing 1", "label_smoothing"),
                      ("--label_smoothing -0.5", "label_smoothing"), ("--loss focal --focal_alpha 1 --class_weights 1 2 3 4 5", "one of them"),
                      ("--loss focal -cp x.h5 --focal_gamma 3", "checkpoint")):
        with pytest.raises(SystemExit) as exc:
            c.check_loss_flags(parse(bad))
        assert word in str(exc.value), (bad, exc.value)
    with pytest.raises(SystemExit):
        c.check_class_flags(parse("--loss cross_entropy --class_weights 1 2 3 4 5"))


def test_checkpoint_metadata_round_trip_and_old_files(tmp_path):
    sp = LossSpec(kind={"seg": L.LOSS_FOCAL_CE, "bound": L.LOSS_FOCAL_BCE, "dist": L.LOSS_MSE, "color": L.LOSS_MSE}, weight={h: 1.0 for h in ("seg", "bound", "dist", "color")},
                  class_weights=[0.5, 1.0, 2.0, 4.0], focal_gamma={"seg": 2.0, "bound": 3.5}, focal_alpha={"bound": 0.75}, class_balance={"bound": True},
                  label_smoothing={"seg": 0.1})
    meta = dict(loss=dict(kind=sp.kind, weight=sp.weight, class_weights=sp.class_weights, optimizer=sp.optimizer, lr=sp.lr, **sp.loss_options()))
    root = h5lite.Group()
    root.attrs["rua_checkpoint"] = json.dumps(meta).encode("utf8")
    path = str(tmp_path / "focal.h5")
    h5lite.write_h5(path, root)
    raw = h5lite.read_h5(path).attrs["rua_checkpoint"]
    lo = json.loads(raw.decode("utf8") if isinstance(raw, bytes) else raw)["loss"]
    back = LS.options_from_meta(lo)
    assert back == dict(focal_gamma=sp.focal_gamma, focal_alpha=sp.focal_alpha, class_balance=sp.class_balance, label_smoothing=sp.label_smoothing)
    sp2 = LossSpec(kind={k: int(v) for k, v in lo["kind"].items()}, weight=lo["weight"], class_weights=lo["class_weights"], **back)
    assert sp2.loss_options() == sp.loss_options() and sp2.kind == sp.kind
    o = sp2.head_opts("bound")
    assert (o.gamma, o.alpha, o.class_balance, o.label_smoothing) == (3.5, 0.75, 1, 0.0)
    o = sp2.head_opts("seg")
    assert (o.gamma, o.class_balance) == (2.0, 0) and abs(o.label_smoothing - 0.1) < 1e-8
    assert sp2.head_opts("dist") is None and sp2.head_opts("color") is None
    # a spec without the options: its metadata carries no such key, and a file written before they existed reads as no option
    plain = LossSpec(kind={"seg": L.LOSS_WCE}, weight={"seg": 1.0}, class_weights=[1.0] * 4)
    assert plain.loss_options() == {} and plain.head_opts("seg") is None
    old = dict(kind={"seg": 1}, weight={"seg": 1.0}, class_weights=[1.0] * 4, optimizer="adam", lr=1e-3, beta_1=0.9, beta_2=0.999, momentum=0.0)
    assert LS.options_from_meta(old) == LS.options_from_meta(json.loads(json.dumps(old))) == {k: {} for k in LS.OPTION_KEYS}
    assert LossSpec(kind=old["kind"], weight=old["weight"], **LS.options_from_meta(old)).loss_options() == {}


def test_ctypes_struct_matches_the_header():
    import ctypes
    assert ctypes.sizeof(L.LossOpts) == 16 and [f[0] for f in L.LossOpts._fields_] == ["gamma", "label_smoothing", "alpha", "class_balance"]
    hdr = open(os.path.join(ROOT, "include", "rua_hip.h")).read()
    assert "typedef struct rua_loss_opts { float gamma, label_smoothing, alpha; int32_t class_balance; } rua_loss_opts;" in hdr
    assert "#define RUA_LOSS_FOCAL_CE 5" in hdr and "#define RUA_LOSS_FOCAL_BCE 6" in hdr
    assert (L.LOSS_FOCAL_CE, L.LOSS_FOCAL_BCE) == (5, 6)
