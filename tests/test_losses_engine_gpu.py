"""Focal losses and label smoothing through the engine and the Keras surface, on the configuration of tests/test_accum_engine_gpu.py (64 x 64 x 3
input, 4 classes, batch 2, f32): the heads' bias gradients and the reported loss values against fp64 autograd of the formulas (restated in
tests/test_losses_gpu.py) on the engine's own logits, the gamma = 0 identity with weighted CE, the captured step against the eager pieces, the
recorded plans, void masks with gradient accumulation, the checkpoint and compile's refusals.

Where two engines are compared bit for bit rua_stem_bwd is pinned to one block, as tests/test_sched_engine_gpu.py explains."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from _kernel_util import bits_of  # noqa: E402
from _scene_util import blob_scene, read_scalars  # noqa: E402
from resunet_a_mltsk_keras_amd import _lib as L  # noqa: E402
from resunet_a_mltsk_keras_amd import h5lite  # noqa: E402
from resunet_a_mltsk_keras_amd import keras_api as ka  # noqa: E402
from resunet_a_mltsk_keras_amd import losses as LS  # noqa: E402
from resunet_a_mltsk_keras_amd import scenes  # noqa: E402
from resunet_a_mltsk_keras_amd.engine import HEADS, Engine, LossSpec, ModelConfig  # noqa: E402
from resunet_a_mltsk_keras_amd.synthetic import make_batch  # noqa: E402
from test_losses_gpu import loss_map, opts, rel_err  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE, NCLS, BATCH = (64, 64, 3), 4, 2
W = [0.6, 1.7, 2.9, 0.4]                                     # per-class alpha / class weights
WEIGHT = {"seg": 1.0, "bound": 0.7, "dist": 1.3, "color": 0.5}
FOCAL = dict(kind={"seg": L.LOSS_FOCAL_CE, "bound": L.LOSS_FOCAL_BCE, "dist": L.LOSS_MSE, "color": L.LOSS_MSE}, class_weights=W,
             focal_gamma={"seg": 2.0, "bound": 2.0}, focal_alpha={"bound": 0.75}, class_balance={"bound": True}, label_smoothing={"seg": 0.1})
PLAIN = dict(kind={"seg": L.LOSS_WCE, "bound": L.LOSS_BCE_LOGITS, "dist": L.LOSS_MSE, "color": L.LOSS_MSE}, class_weights=W)


def spec(base, **kw):
    return LossSpec(weight=dict(WEIGHT), lr=1e-3, **{**base, **kw})


def config(multitask=True):
    return ModelConfig(input_shape=SHAPE, num_classes=NCLS, multitasking=multitask, width=32)


def engine(sp, use_graph=None, seed=4):
    eng = Engine(config(), dtype="f32", seed=seed, split_k=False)
    eng.stem_mfma = False
    if use_graph is not None:
        eng.use_graph = use_graph
    eng.compile(sp)
    return eng


def batch(seed):
    return make_batch(BATCH, SHAPE[0], SHAPE[2], NCLS, True, seed=seed, block=16)


def bits(eng, names=("P", "M1", "V1", "S")):
    torch.cuda.synchronize()
    return [bits_of(getattr(eng, n)).copy() for n in names]


def same(a, b):
    return all((x == y).all() for x, y in zip(a, b))


@pytest.fixture
def one_block_stem():
    lib = L.lib()
    before = lib.get_tuning("stem_blocks")
    lib.set_tuning(stem_blocks=1)
    yield
    lib.set_tuning(stem_blocks=before)


def head_opts(sp, name):
    o = sp.head_opts(name)
    return o if o is not None else opts()


def head_loss_map(kind, p, z, y, a, o):
    if kind == L.LOSS_MSE:
        return ((y - p) ** 2).mean(-1)
    return loss_map(kind, p, z, y, a, o)


# ---- 1. bias gradients and loss values ----------------------------------------------------------------------------------------------------
def bias_gradient_deviation(sp, x, y):
    """forward_backward on a fresh engine; per head (max |bias gradient - loss weight * sum over pixels of the dz fp64 autograd gives for that
    head's loss on the engine's own logits|, the gradient's scale), and per head (the loss value the step reports, the formula on the engine's
    own probabilities)."""
    eng = engine(sp, use_graph=False)
    g = eng.forward_backward(x, y)
    torch.cuda.synchronize()
    reported = eng._results(g)[1:1 + len(HEADS)]
    a = torch.tensor(W, dtype=torch.float64)
    devs, vals = {}, {}
    for h, rep in zip(g.heads, reported):
        name, Cc, kind = h["name"], h["C"], sp.kind[h["name"]]
        zt = h["z"].t.detach().cpu().double().reshape(-1, Cc).requires_grad_(True)
        yt = h["y"].t.detach().cpu().double().reshape(-1, Cc)
        p = torch.softmax(zt, -1) if h["act"] == L.ACT_SOFTMAX else torch.sigmoid(zt)
        o = head_opts(sp, name)
        (sp.weight[name] * head_loss_map(kind, p, zt, yt, a, o).mean()).backward()
        want = zt.grad.sum(0).numpy()
        off = h["lay"]["bias"]
        got = eng.G[off:off + Cc].detach().cpu().numpy().astype(np.float64)
        devs[name] = (float(np.abs(got - want).max()), float(np.abs(want).max()))
        with torch.no_grad():
            p32 = h["p"].t.detach().cpu().double().reshape(-1, Cc)
            vals[name] = (float(rep), float(head_loss_map(kind, p32, zt.detach(), yt, a, o).mean()))
    return devs, vals


def test_bias_gradients_and_loss_values_are_the_formulas():
    x, y = batch(300)
    base, base_vals = bias_gradient_deviation(spec(PLAIN), x, y)
    cand, cand_vals = bias_gradient_deviation(spec(FOCAL), x, y)
    for h in HEADS:
        print(f"{h}: bias gradient deviation {cand[h][0]:.3g} focal (scale {cand[h][1]:.3g}), {base[h][0]:.3g} weighted CE / BCE / MSE (scale {base[h][1]:.3g}); "
              f"loss {cand_vals[h][0]:.8f} formula {cand_vals[h][1]:.8f}")
        assert cand[h][1] > 0
        assert cand[h][0] <= 10 * base[h][0] + 1e-6 * max(1.0, cand[h][1]), (h, cand[h], base[h])
        for got, want in (cand_vals[h], base_vals[h]):
            assert abs(got - want) < 1e-5 * max(1.0, abs(want)), (h, got, want)


# ---- 2. gamma = 0, alpha = W is weighted CE -------------------------------------------------------------------------------------------------
def test_gamma_zero_is_weighted_cross_entropy():
    x, y = batch(301)
    res = []
    for sp in (spec(PLAIN), spec(PLAIN, kind={**PLAIN["kind"], "seg": L.LOSS_FOCAL_CE}, focal_gamma={"seg": 0.0})):
        eng = engine(sp, use_graph=False)
        g = eng.forward_backward(x, y, _whole_step=True)
        torch.cuda.synchronize()
        res.append((eng._results(g)[:5], eng.G.detach().cpu().numpy().copy(), [c[1] for c in g.loss_plan.calls + g.bwd.calls]))
    (la, ga, na), (lb, gb, nb) = res
    assert "rua_pixel_loss_opts" in nb and "rua_head_dz_multi_opts" in nb and not [n for n in na if n.endswith("_opts")]
    print(f"losses {la} / {lb}, gradient rel err {rel_err(gb, ga):.2e}")
    for u, v in zip(la, lb):
        assert abs(u - v) <= 1e-6 * max(1.0, abs(u))
    assert np.abs(ga).max() > 0 and rel_err(gb, ga) < 2e-4


# ---- 3. the captured step and the plans -------------------------------------------------------------------------------------------------------
def test_captured_step_equals_the_eager_pieces(one_block_stem):
    a, b = engine(spec(FOCAL)), engine(spec(FOCAL))
    assert a.use_graph
    for k in range(3):
        x, y = batch(310 + k)
        ra = a.train_step(x, y)
        b.forward_backward(x, y, _whole_step=True)
        b.optimizer_step()
        assert np.isfinite(ra).all()
        assert same(bits(a), bits(b)), k


def plan_names(g):
    return {k: [c[1] for c in getattr(g, k).calls] for k in ("fwd", "loss_plan", "bwd")}


@pytest.mark.parametrize("multitask", [True, False])
@pytest.mark.parametrize("void", [None, 2])
def test_recorded_plans(multitask, void):
    heads = HEADS if multitask else ["seg"]
    only = lambda d: {k: v for k, v in d.items() if k in heads}
    def build(base):
        sp = LossSpec(weight=only(WEIGHT), lr=1e-3, ignore_void=void, class_weights=W, kind=only(base["kind"]),
                      **{k: only(base.get(k, {})) for k in LS.OPTION_KEYS})
        eng = Engine(config(multitask), dtype="f32", seed=4, split_k=False)
        eng.compile(sp)
        return {tr: plan_names(eng.graph(BATCH, tr)) for tr in (True, False)}
    off, on = build(PLAIN), build(FOCAL)
    sfx = "_void" if void is not None else ""
    for tr in (True, False):
        assert not [n for k in off[tr] for n in off[tr][k] if n.endswith("_opts")]           # no option: no plan names a new entry
        assert {k: len(v) for k, v in off[tr].items()} == {k: len(v) for k, v in on[tr].items()}
        assert off[tr]["fwd"] == on[tr]["fwd"]                                               # the head forward's fused metrics are untouched
        n_opts = 2 if multitask else 1                                                       # seg and bound take the entry with options, dist and color do not
        assert on[tr]["loss_plan"].count("rua_pixel_loss_opts") == n_opts and off[tr]["loss_plan"].count("rua_pixel_loss" + sfx) == len(heads)
        assert on[tr]["loss_plan"].count("rua_pixel_loss" + sfx) == len(heads) - n_opts
        dz_off = ("rua_head_dz_multi" if multitask else "rua_head_dz") + sfx
        dz_on = "rua_head_dz_multi_opts" if multitask else "rua_head_dz_opts"
        assert (off[tr]["bwd"].count(dz_off), on[tr]["bwd"].count(dz_on)) == ((1, 1) if tr else (0, 0))   # all heads' dz still leave in one launch
        swap = {"rua_pixel_loss" + sfx: "rua_pixel_loss_opts", dz_off: dz_on}
        for k in ("loss_plan", "bwd"):                                                       # every other entry is the entry it was, in its place
            assert all(a == b or swap.get(a) == b for a, b in zip(off[tr][k], on[tr][k])), k


# ---- 4. void masks and accumulation -------------------------------------------------------------------------------------------------------------
def test_void_masks_with_accumulation():
    eng = engine(spec(FOCAL, ignore_void=2, gradient_accumulation_steps=2))
    x, y = batch(320)
    before = bits(eng, ("P",))
    all_void = np.ones((BATCH,) + SHAPE[:2], np.uint8)
    for _ in range(2):                                           # one whole cycle of all-void batches: an update with a zero gradient on zero moments
        res = eng.train_step(x, y, void_mask=all_void)
        assert np.isfinite(res).all(), res
    assert eng.t == 1 and same(bits(eng, ("P",)), before)
    rng = np.random.default_rng(5)
    for k in range(4):
        x, y = batch(321 + k)
        vm = (rng.random((BATCH,) + SHAPE[:2]) < 0.3).astype(np.uint8)
        if k == 1:
            vm[1] = 1                                            # an all-void sample
        res = eng.train_step(x, y, void_mask=vm)
        assert np.isfinite(res).all(), (k, res)
    assert eng.t == 3 and np.isfinite(state_of(eng)).all() and not same(bits(eng, ("P",)), before)


def state_of(eng):
    return np.concatenate([eng.P.detach().cpu().numpy().ravel(), eng.S.detach().cpu().numpy().ravel()])


# ---- 5. the Keras surface: compile, save, load ------------------------------------------------------------------------------------------------------
def focal_losses():
    return {"seg": ka.CategoricalFocalCrossentropy(alpha=W, gamma=2.0, label_smoothing=0.1),
            "bound": ka.BinaryFocalCrossentropy(apply_class_balancing=True, alpha=0.75, gamma=3.0, label_smoothing=0.05),
            "dist": ka.MeanSquaredError(), "color": ka.MeanSquaredError()}


def keras_model(losses, seed=11):
    m = ka.Model(config(), dtype="f32", seed=seed)
    m.compile(optimizer=ka.Adam(lr=1e-3), loss=losses, loss_weights=WEIGHT)
    return m


def test_compile_save_and_load(tmp_path, one_block_stem):
    m, whole = keras_model(focal_losses()), keras_model(focal_losses())
    sp = m.engine.loss
    assert sp.kind == FOCAL["kind"] and sp.class_weights == W
    assert sp.loss_options() == dict(focal_gamma={"seg": 2.0, "bound": 3.0}, focal_alpha={"bound": 0.75}, class_balance={"bound": True},
                                     label_smoothing={"seg": 0.1, "bound": 0.05})
    m.train_on_batch(*batch(330))
    path = str(tmp_path / "focal.h5")
    m.save(path)
    m2 = ka.load_model(path)
    assert m2.engine.loss.loss_options() == sp.loss_options() and m2.engine.loss.kind == sp.kind and m2.engine.loss.class_weights == W
    m2.train_on_batch(*batch(331))
    for k in range(2):
        whole.train_on_batch(*batch(330 + k))
    assert same(bits(m2.engine), bits(whole.engine)) and m2.engine.t == whole.engine.t == 2
    # the loss names, with Keras' defaults
    named = keras_model({"seg": "categorical_focal_crossentropy", "bound": "binary_focal_crossentropy", "dist": "mse", "color": "mse"})
    assert named.engine.loss.kind == FOCAL["kind"] and named.engine.loss.class_weights == [0.25] * NCLS
    assert named.engine.loss.loss_options() == dict(focal_gamma={"seg": 2.0, "bound": 2.0})
    # a file saved without the options carries none, and loads and trains as before
    plain = keras_model({"seg": ka.weighted_categorical_crossentropy(W), "bound": ka.BinaryCrossentropy(), "dist": ka.MeanSquaredError(), "color": ka.MeanSquaredError()}, seed=5)
    x, y = batch(332)
    plain.train_on_batch(x, y)
    p2 = str(tmp_path / "plain.h5")
    plain.save(p2)
    raw = h5lite.read_h5(p2).attrs["rua_checkpoint"]
    lo = json.loads(raw.decode("utf8") if isinstance(raw, bytes) else raw)["loss"]
    assert not [k for k in LS.OPTION_KEYS if k in lo]
    back = ka.load_model(p2)
    assert back.engine.loss.loss_options() == {}
    plain.train_on_batch(x, y), back.train_on_batch(x, y)
    assert same(bits(plain.engine), bits(back.engine)) and back.engine.t == 2


def test_compile_refusals_come_before_any_launch():
    m = ka.Model(config(), dtype="f32", seed=3)
    mse = ka.MeanSquaredError()
    ok = focal_losses()
    def refuse(match, **over):
        with pytest.raises(ValueError, match=match):
            m.compile(optimizer=ka.Adam(lr=1e-3), loss={**ok, **over})
    refuse("softmax head", bound=ka.CategoricalFocalCrossentropy())                         # focal CE on a sigmoid head
    refuse("softmax head", color="categorical_focal_crossentropy")
    refuse("sigmoid head", seg=ka.BinaryFocalCrossentropy())                                # binary focal on a softmax head
    refuse("sigmoid head", dist="binary_focal_crossentropy")
    refuse("gamma", seg=ka.CategoricalFocalCrossentropy(alpha=W, gamma=0.5))                # a bad range
    refuse("gamma", bound=ka.BinaryFocalCrossentropy(gamma=9.0))
    refuse("label_smoothing", seg=ka.CategoricalFocalCrossentropy(alpha=W, label_smoothing=1.0))
    refuse("label_smoothing", bound=ka.BinaryCrossentropy(label_smoothing=-0.1))
    refuse("alpha", bound=ka.BinaryFocalCrossentropy(apply_class_balancing=True, alpha=1.5))
    refuse("alpha values", seg=ka.CategoricalFocalCrossentropy(alpha=[1.0, 2.0, 3.0]))      # a wrong alpha length
    refuse("not negative", seg=ka.CategoricalFocalCrossentropy(alpha=[1.0, 2.0, 3.0, -1.0]))
    assert not m.engine.graphs and not m._compiled
    # smoothing on Tanimoto or MSE: no loss object carries it there, the spec is refused all the same
    eng = m.engine
    for kind in (L.LOSS_TANIMOTO, L.LOSS_MSE):
        with pytest.raises(ValueError, match="no label smoothing"):
            eng.compile(LossSpec(kind={h: kind for h in HEADS}, weight=dict(WEIGHT), label_smoothing={"dist": 0.1}))
    with pytest.raises(ValueError, match="class_weights"):
        eng.compile(LossSpec(kind=FOCAL["kind"], weight=dict(WEIGHT), focal_gamma={"seg": 2.0}))
    with pytest.raises(ValueError, match="belong to the focal losses"):
        eng.compile(LossSpec(kind=PLAIN["kind"], weight=dict(WEIGHT), class_weights=W, focal_gamma={"seg": 2.0}))
    with pytest.raises(ValueError, match="not a head"):
        eng.compile(LossSpec(kind=PLAIN["kind"], weight=dict(WEIGHT), class_weights=W, label_smoothing={"segg": 0.1}))
    assert not eng.graphs and eng.loss is None


# ---- 6. the command line ----------------------------------------------------------------------------------------------------------------------
def test_cli_loss_focal_trains_and_stores_its_options(tmp_path):
    """One epoch of `--loss focal` on a seeded 160 x 192 scene (-ps 64, stride 32: 16 training windows, four steps), with the class weights of the
    windows as the per-class alpha, a balanced boundary head, smoothing and void pixels: it runs to the end, every scalar is finite and the
    saved model carries the options."""
    img, cls = blob_scene(200, 160, 192)
    root, results = str(tmp_path / "scenes"), str(tmp_path / "run")
    scenes.save_scene_dir(root, ["tile"], [img], [cls])
    cmd = [sys.executable, os.path.join(ROOT, "train_ISPRS.py"), "--resunet_a", "yes", "--multitasking", "yes", "--loss", "focal", "--focal_gamma", "3",
           "--class_weights", "auto", "--bound_alpha", "0.75", "--label_smoothing", "0.05", "--ignore_void", "yes", "--scene_dataset", "yes",
           "-rp", results, "-dp", root, "-bs", "4", "-ps", "64", "--num_classes", str(NCLS), "--epochs", "1", "--dtype", "f32", "--norm_type", "1",
           "--seed", "5", "--stride", "32", "--data_aug", "no"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "Using Focal loss (gamma 3" in r.stdout
    tr, va = read_scalars(os.path.join(results, "logs", "train", "scalars.jsonl")), read_scalars(os.path.join(results, "logs", "val", "scalars.jsonl"))
    assert tr and va and all(np.isfinite(v["value"]) for v in tr + va if v["tag"] != "Segmentation/MCC")
    raw = h5lite.read_h5(os.path.join(results, "best_model.h5")).attrs["rua_checkpoint"]
    lo = json.loads(raw.decode("utf8") if isinstance(raw, bytes) else raw)["loss"]
    assert {k: int(v) for k, v in lo["kind"].items()} == FOCAL["kind"]
    assert lo["focal_gamma"] == {"seg": 3.0, "bound": 3.0} and lo["focal_alpha"] == {"bound": 0.75} and lo["class_balance"] == {"bound": True}
    assert lo["label_smoothing"] == {"seg": 0.05, "bound": 0.05}
    assert len(lo["class_weights"]) == NCLS and all(w > 1 for w in lo["class_weights"])          # total / pixels of the class
