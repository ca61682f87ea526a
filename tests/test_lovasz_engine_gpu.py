"""The Lovasz-Softmax loss through the engine and the Keras surface, on the configuration of tests/test_ohem_engine_gpu.py (64 x 64 x 3 input, 4
classes, batch 2, f32): the step's loss against losses.host_lovasz on the step's own probabilities and targets (within n * 2^-52: every term
is non-negative), the heads' d(total)/d(logits) against host_lovasz_dz's bits, the captured step against the eager pieces, void pixels,
accumulation with a global clip norm, evaluation, the recorded plans, the checkpoint, compile's refusals and the command line.

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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE, NCLS, BATCH = (64, 64, 3), 4, 2
M = BATCH * SHAPE[0] * SHAPE[1]
W = [0.6, 1.7, 2.9, 0.4]
WEIGHT = {"seg": 1.0, "bound": 0.7, "dist": 1.3, "color": 0.5}
ACT = {"seg": L.ACT_SOFTMAX, "bound": L.ACT_SIGMOID}
LOVASZ = dict(kind={"seg": L.LOSS_LOVASZ, "bound": L.LOSS_LOVASZ, "dist": L.LOSS_MSE, "color": L.LOSS_MSE}, lovasz={"bound": LS.lovasz_options("all")})
PLAIN = dict(kind={"seg": L.LOSS_WCE, "bound": L.LOSS_BCE_LOGITS, "dist": L.LOSS_MSE, "color": L.LOSS_MSE}, class_weights=W)
NEW = ("rua_lovasz_grad", "rua_lovasz_dz")


def config(multitask=True):
    return ModelConfig(input_shape=SHAPE, num_classes=NCLS, multitasking=multitask, width=32)


def engine(sp, multitask=True, use_graph=None, seed=4):
    eng = Engine(config(multitask), dtype="f32", seed=seed, split_k=False)
    eng.stem_mfma = False
    if use_graph is not None:
        eng.use_graph = use_graph
    eng.compile(sp)
    return eng


def spec(base, **kw):
    return LossSpec(weight=dict(WEIGHT), lr=1e-3, **{**base, **kw})


def batch(seed, multitask=True):
    return make_batch(BATCH, SHAPE[0], SHAPE[2], NCLS, multitask, seed=seed, block=16)


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


def host_of(eng, head, training=True, void=None):
    """host_lovasz on the probabilities and targets the last step of `eng` left for `head`, with the head's options and loss weight."""
    h = eng.graphs[(BATCH, training)].outputs[head]
    torch.cuda.synchronize()
    p, y = h["p"].t.cpu().numpy().reshape(M, -1), h["y"].t.cpu().numpy().reshape(M, -1)
    return LS.host_lovasz(p, y, void, eng.loss.head_lovasz(head)["classes"], eng.loss.weight[head]), h, p


def assert_head(eng, res, head, void=None, what=""):
    """The report, the head's entry of the result list and (training) the head's dz against the host's definitions."""
    host, h, p = host_of(eng, head, True, void)
    rep = eng.lovasz_report()[head]
    Cc = p.shape[1]
    assert (rep["n_valid"], rep["n_cls"], rep["G"]) == (host["n_valid"], host["n_cls"], host["G"]), (what, head)
    assert np.float32(rep["scale"]).view(np.uint32) == np.float32(host["scale"]).view(np.uint32), (what, head)
    bound = max(host["n_valid"], 1) * 2.0 ** -52
    got = res[1 + HEADS.index(head)]
    print(f"{what} {head}: loss {got!r} / report {rep['loss']!r} / host {host['loss']!r}, bound {bound * abs(host['loss']):.2e}")
    assert abs(rep["loss"] - host["loss"]) <= bound * abs(host["loss"]), (what, head)
    assert abs(got - host["loss"]) <= bound * abs(host["loss"]), (what, head)
    for c in range(Cc):
        assert abs(rep["loss_c"][c] - host["loss_c"][c]) <= bound * abs(host["loss_c"][c]), (what, head, c)
    assert np.array_equal(h["lovasz"]["dp"].cpu().numpy().reshape(M, Cc).view(np.uint32), host["dp"].view(np.uint32)), (what, head)
    dz = h["dz"].t.cpu().numpy().reshape(M, Cc)
    want = LS.host_lovasz_dz(ACT[head], p, host["dp"], host["scale"])
    assert np.array_equal(dz.view(np.uint32), want.view(np.uint32)) and np.abs(dz).sum() > 0, (what, head)
    return host, dz


# ---- 1. loss and dz of a step ---------------------------------------------------------------------------------------------------------------------
def test_step_equals_the_host_definitions():
    eng = engine(spec(LOVASZ), use_graph=False)
    x, y = batch(500)
    g = eng.forward_backward(x, y, _whole_step=True)
    torch.cuda.synchronize()
    res = eng._results(g)
    assert np.isfinite(res).all()
    hs, _ = assert_head(eng, res, "seg")
    hb, _ = assert_head(eng, res, "bound")
    assert hs["n_valid"] == hb["n_valid"] == M and hb["n_cls"] == NCLS and 1 <= hs["n_cls"] <= NCLS
    assert g.outputs["seg"]["norm"] == 1.0 and eng.lovasz_report().keys() == {"seg", "bound"}
    total = sum(WEIGHT[h] * res[1 + HEADS.index(h)] for h in HEADS)
    assert abs(res[0] - total) <= 1e-12 * abs(total)
    assert np.abs(eng.G.detach().cpu().numpy()).max() > 0
    # single task: the seg head alone, its own dz launch and no other
    e1 = engine(LossSpec(kind={"seg": L.LOSS_LOVASZ}, weight={"seg": 0.8}, lr=1e-3), False, use_graph=False)
    x1, y1 = batch(501, False)
    g1 = e1.forward_backward(x1, y1, _whole_step=True)
    torch.cuda.synchronize()
    names = [c[1] for c in g1.loss_plan.calls + g1.bwd.calls]
    assert names.count("rua_lovasz_grad") == 1 and names.count("rua_lovasz_dz") == 1 and not [n for n in names if n.startswith("rua_head_dz")]
    host, h, p = host_of(e1, "seg")
    r1 = e1._results(g1)
    assert abs(r1[0] - 0.8 * host["loss"]) <= 1e-12 * abs(r1[0]) + M * 2.0 ** -52 * abs(r1[0])
    assert np.array_equal(h["dz"].t.cpu().numpy().reshape(M, NCLS).view(np.uint32), LS.host_lovasz_dz(L.ACT_SOFTMAX, p, host["dp"], host["scale"]).view(np.uint32))


# ---- 2. the captured step -------------------------------------------------------------------------------------------------------------------------
def test_captured_step_equals_the_eager_pieces(one_block_stem):
    sp = spec(LOVASZ)
    a, b = engine(sp), engine(sp, use_graph=False)
    assert a.use_graph
    seen = []
    for k in range(3):                                                   # the warm-up run and two replays, each on its own batch
        x, y = batch(510 + k)
        ra = a.train_step(x, y)
        b.forward_backward(x, y, _whole_step=True)
        b.optimizer_step()
        assert np.isfinite(ra).all()
        assert same(bits(a), bits(b)), k
        for head in ("seg", "bound"):                                    # no host scalar in between: the replay's own sort matches the host's
            assert_head(a, ra, head, what=f"replay {k}")
        seen.append(a.lovasz_report()["seg"]["loss"])
    assert len(a._captured) == 1 and len(set(seen)) == 3, seen


# ---- 3. void pixels -------------------------------------------------------------------------------------------------------------------------------
def test_void_pixels_take_no_part():
    eng = engine(spec(LOVASZ, ignore_void=0), use_graph=False)
    rng = np.random.default_rng(7)
    x, y = batch(520)
    for k, vm in enumerate(((rng.random((BATCH,) + SHAPE[:2]) < 0.3).astype(np.uint8), np.ones((BATCH,) + SHAPE[:2], np.uint8))):
        g = eng.forward_backward(x, y, _whole_step=True, void_mask=vm)
        torch.cuda.synchronize()
        res = eng._results(g)
        assert np.isfinite(res).all()
        flat = vm.reshape(-1)
        if k == 0:
            for head in ("seg", "bound"):
                host, dz = assert_head(eng, res, head, void=flat, what="void30")
                assert host["n_valid"] == int((flat == 0).sum()) and not dz[flat != 0].view(np.uint32).any() and np.abs(dz[flat == 0]).sum() > 0
        else:                                                            # an all-void batch: loss 0, scale 0, a zero gradient from these heads
            rep = eng.lovasz_report()
            for head in ("seg", "bound"):
                h = g.outputs[head]
                assert (rep[head]["n_valid"], rep[head]["n_cls"], rep[head]["scale"], rep[head]["loss"]) == (0, 0, 0.0, 0.0) and res[1 + HEADS.index(head)] == 0.0
                assert not h["dz"].t.cpu().numpy().view(np.uint32).any()


# ---- 4. accumulation and a global clip norm ---------------------------------------------------------------------------------------------------------
def test_accumulation_and_clipping_match_the_uncaptured_path(one_block_stem):
    sp = spec(LOVASZ, gradient_accumulation_steps=2, global_clipnorm=0.5)
    a, b = engine(sp), engine(sp, use_graph=False)
    for k in range(4):
        x, y = batch(530 + k)
        ra, rb = a.train_step(x, y), b.train_step(x, y)
        assert np.isfinite(ra).all() and np.allclose(ra, rb, rtol=1e-9, atol=0), k     # (the MSE heads' sums are fp64 atomics: the last bits may differ)
        assert same(bits(a), bits(b)), k
    assert a.t == b.t == 2 and a.clip_report()["norm"] > 0


# ---- 5. evaluation ----------------------------------------------------------------------------------------------------------------------------------
def test_evaluation_reports_the_same_loss():
    eng = engine(spec(LOVASZ), use_graph=False)
    x, y = batch(540)
    res = eng.test_step(x, y)
    names = [c[1] for c in eng.graphs[(BATCH, False)].loss_plan.calls]
    assert names.count("rua_lovasz_grad") == 2 and "rua_lovasz_dz" not in names
    for head in ("seg", "bound"):
        host, h, _ = host_of(eng, head, training=False)
        assert h["lovasz"]["dp"] is None                                 # the value only
        assert abs(res[1 + HEADS.index(head)] - host["loss"]) <= M * 2.0 ** -52 * abs(host["loss"]), head
    assert eng.lovasz_report()["seg"]["n_valid"] == M


# ---- 6. the recorded plans --------------------------------------------------------------------------------------------------------------------------
def plan_names(g):
    return {k: [c[1] for c in getattr(g, k).calls] for k in ("fwd", "loss_plan", "bwd")}


@pytest.mark.parametrize("void", [None, 2])
def test_recorded_plans(void):
    def build(base):
        eng = Engine(config(), dtype="f32", seed=4, split_k=False)
        eng.compile(spec(base, ignore_void=void))
        return {tr: plan_names(eng.graph(BATCH, tr)) for tr in (True, False)}
    off, on = build(PLAIN), build(LOVASZ)
    sfx = "_void" if void is not None else ""
    # without the loss: the calls of a model that never heard of it - the entries test_losses_engine_gpu.py::test_recorded_plans finds
    for tr in (True, False):
        assert not [n for k in off[tr] for n in off[tr][k] if n in NEW]
        assert off[tr]["loss_plan"].count("rua_pixel_loss" + sfx) == 4
        assert [n for n in off[tr]["bwd"] if n.startswith("rua_head_dz")] == (["rua_head_dz_multi" + sfx] if tr else [])
        assert not [n for n in off[tr]["loss_plan"] + off[tr]["bwd"] if n.startswith("rua_ohem") or n.endswith("_sel")]
    # with it: the two heads' loss entries are rua_lovasz_grad, each has a dz launch of its own, the other heads keep their single launch
    for tr in (True, False):
        assert on[tr]["fwd"] == off[tr]["fwd"]
        lp = on[tr]["loss_plan"]
        assert lp.count("rua_lovasz_grad") == 2 and lp.count("rua_pixel_loss" + sfx) == 2
        assert [("rua_pixel_loss" + sfx) if n == "rua_lovasz_grad" else n for n in lp] == off[tr]["loss_plan"]
    bw = on[True]["bwd"]
    assert bw.count("rua_lovasz_dz") == 2 and [n for n in bw if n.startswith("rua_head_dz")] == ["rua_head_dz_multi" + sfx]
    assert [n for n in bw if n != "rua_lovasz_dz"] == off[True]["bwd"]
    for i, n in enumerate(bw):                                           # each dz launch right in front of its head's backward
        if n == "rua_lovasz_dz":
            assert bw[i + 1] in ("rua_head_bwd_sums", "rua_head_dz_multi" + sfx)
    assert "rua_lovasz_dz" not in on[False]["bwd"]


# ---- 7. the Keras surface ---------------------------------------------------------------------------------------------------------------------------
def lovasz_losses():
    return {"seg": ka.LovaszSoftmax(), "bound": ka.LovaszSoftmax(classes="all"), "dist": ka.MeanSquaredError(), "color": ka.MeanSquaredError()}


def keras_model(losses, seed=11):
    m = ka.Model(config(), dtype="f32", seed=seed)
    m.compile(optimizer=ka.Adam(lr=1e-3), loss=losses, loss_weights=WEIGHT)
    return m


def test_compile_save_load_and_fine_tune(tmp_path, one_block_stem):
    m, whole = keras_model(lovasz_losses()), keras_model(lovasz_losses())
    sp = m.engine.loss
    want = {"seg": dict(classes="present"), "bound": dict(classes="all")}
    assert sp.lovasz == want and sp.loss_options() == dict(lovasz=want) and sp.kind["seg"] == sp.kind["bound"] == L.LOSS_LOVASZ
    assert m.lovasz_report() is None                                     # no step yet
    m.train_on_batch(*batch(550))
    assert set(m.lovasz_report()) == {"seg", "bound"}
    path = str(tmp_path / "lovasz.h5")
    m.save(path)
    raw = h5lite.read_h5(path).attrs["rua_checkpoint"]
    assert json.loads(raw.decode("utf8") if isinstance(raw, bytes) else raw)["loss"]["lovasz"] == want
    m2 = ka.load_model(path)
    assert m2.engine.loss.lovasz == want and m2.engine.loss.kind == sp.kind
    m2.train_on_batch(*batch(551))
    for k in range(2):
        whole.train_on_batch(*batch(550 + k))
    assert same(bits(m2.engine), bits(whole.engine)) and m2.engine.t == whole.engine.t == 2
    assert m2.lovasz_report() == whole.lovasz_report()
    # the name as a string, and a model trained under another loss re-compiled for the fine-tune
    ce = keras_model({"seg": ka.weighted_categorical_crossentropy(W), "bound": "binary_crossentropy", "dist": "mse", "color": "mse"})
    ce.train_on_batch(*batch(552))
    p2 = str(tmp_path / "ce.h5")
    ce.save(p2)
    ft = ka.load_model(p2)
    assert L.LOSS_LOVASZ not in ft.engine.loss.kind.values() and ft.lovasz_report() is None
    ft.compile(optimizer=ka.Adam(lr=1e-4), loss={"seg": "lovasz", "bound": "lovasz_softmax", "dist": "mse", "color": "mse"}, loss_weights=WEIGHT)
    assert ft.engine.loss.lovasz == {"seg": dict(classes="present"), "bound": dict(classes="present")}
    before = bits(ft.engine, ("P",))
    r = ft.train_on_batch(*batch(553))
    assert np.isfinite(r).all() and not same(before, bits(ft.engine, ("P",))) and ft.lovasz_report()["seg"]["n_valid"] == M


def test_the_loss_object_gives_the_scalar_from_the_gpu():
    rng = np.random.default_rng(8)
    yp = rng.random((2, 33, 31, NCLS)).astype(np.float32) + 0.05
    yp /= yp.sum(-1, keepdims=True)
    yt = np.eye(NCLS, dtype=np.float32)[rng.integers(0, NCLS, (2, 33, 31))]
    for classes in ("present", "all"):
        host = LS.host_lovasz(yp, yt, classes=classes)
        v = ka.LovaszSoftmax(classes)(yt, yp)
        assert isinstance(v, float) and abs(v - host["loss"]) <= host["n_valid"] * 2.0 ** -52 * host["loss"]


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_compile_refusals_come_before_any_launch():
    eng = Engine(config(), dtype="f32", seed=3, split_k=False)

    def refuse(match, base=LOVASZ, **kw):
        with pytest.raises(ValueError, match=match):
            eng.compile(spec(base, **kw))
    for head in ("dist", "color"):                                       # continuous targets
        refuse("continuous", base=dict(kind={**LOVASZ["kind"], head: L.LOSS_LOVASZ}))
    refuse("hard example mining", ohem={"seg": LS.ohem_options()})
    refuse("label smoothing", label_smoothing={"seg": 0.1})
    refuse("focal", focal_gamma={"bound": 2.0})
    refuse("classes", lovasz={"seg": dict(classes="some")})
    refuse("unknown", lovasz={"seg": dict(per_image=True)})
    refuse("a dict", lovasz={"seg": "all"})
    refuse("not a head", lovasz={"segg": LS.lovasz_options()})
    refuse("belong to a head on the Lovasz loss", base=PLAIN, lovasz={"seg": LS.lovasz_options()})
    assert not eng.graphs and eng.loss is None
    m = ka.Model(config(), dtype="f32", seed=3)
    with pytest.raises(ValueError, match="continuous"):
        m.compile(optimizer=ka.Adam(lr=1e-3), loss={"seg": "lovasz", "bound": "lovasz", "dist": "lovasz", "color": "mse"})
    with pytest.raises(ValueError, match="hard example mining"):
        m.compile(optimizer=ka.Adam(lr=1e-3), loss={"seg": ka.OnlineHardExampleMining(ka.LovaszSoftmax()), "bound": "lovasz", "dist": "mse", "color": "mse"})
    assert not m.engine.graphs and not m._compiled


# ---- 9. the command line ----------------------------------------------------------------------------------------------------------------------------
def test_cli_lovasz_trains_and_stores_its_options(tmp_path):
    """One epoch of `--loss lovasz --lovasz_classes all` on a seeded 160 x 192 scene (-ps 64, stride 32: 16 training windows, four steps) with void
    pixels: it runs to the end, every scalar is finite, the per-epoch line is printed and the saved model carries the options."""
    img, cls = blob_scene(200, 160, 192)
    root, results = str(tmp_path / "scenes"), str(tmp_path / "run")
    scenes.save_scene_dir(root, ["tile"], [img], [cls])
    base = [sys.executable, os.path.join(ROOT, "train_ISPRS.py"), "--resunet_a", "yes"]
    cmd = base + ["--multitasking", "yes", "--loss", "lovasz", "--lovasz_classes", "all", "--ignore_void", "yes", "--scene_dataset", "yes",
                  "-rp", results, "-dp", root, "-bs", "4", "-ps", "64", "--num_classes", str(NCLS), "--epochs", "1", "--dtype", "f32", "--norm_type", "1",
                  "--seed", "5", "--stride", "32", "--data_aug", "no"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "Using Lovasz-Softmax loss (classes all)" in r.stdout and r.stdout.count("Lovasz loss (last step): seg") == 1
    tr, va = read_scalars(os.path.join(results, "logs", "train", "scalars.jsonl")), read_scalars(os.path.join(results, "logs", "val", "scalars.jsonl"))
    assert tr and va and all(np.isfinite(v["value"]) for v in tr + va if v["tag"] != "Segmentation/MCC")
    raw = h5lite.read_h5(os.path.join(results, "best_model.h5")).attrs["rua_checkpoint"]
    lo = json.loads(raw.decode("utf8") if isinstance(raw, bytes) else raw)["loss"]
    assert lo["lovasz"] == {"seg": dict(classes="all"), "bound": dict(classes="all")} and lo["kind"]["seg"] == lo["kind"]["bound"] == L.LOSS_LOVASZ
    # -cp with --loss lovasz fine-tunes: the checkpoint's weights, the command line's loss (here the other classes option)
    results2 = str(tmp_path / "run2")
    cmd2 = base + ["--multitasking", "yes", "--loss", "lovasz", "-cp", os.path.join(results, "best_model.h5"), "--ignore_void", "yes", "--scene_dataset", "yes",
                   "-rp", results2, "-dp", root, "-bs", "4", "-ps", "64", "--num_classes", str(NCLS), "--epochs", "1", "--dtype", "f32", "--norm_type", "1",
                   "--seed", "5", "--stride", "32", "--data_aug", "no", "-lr", "1e-4"]
    r = subprocess.run(cmd2, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "to fine-tune under the Lovasz loss" in r.stdout and "Using Lovasz-Softmax loss (classes present)" in r.stdout
    raw = h5lite.read_h5(os.path.join(results2, "best_model.h5")).attrs["rua_checkpoint"]
    lo = json.loads(raw.decode("utf8") if isinstance(raw, bytes) else raw)["loss"]
    assert lo["lovasz"] == {"seg": dict(classes="present"), "bound": dict(classes="present")} and lo["lr"] == 1e-4
    # flags that contradict each other are refused before anything is loaded
    for bad, word in ((["--lovasz_classes", "all"], "--loss lovasz"), (["--loss", "lovasz", "--ohem", "yes"], "Lovasz"),
                      (["--loss", "lovasz", "--label_smoothing", "0.1"], "Lovasz"), (["--loss", "lovasz", "--focal_gamma", "3"], "--loss focal")):
        r = subprocess.run(base + ["-rp", results, "-dp", root] + bad, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and word in r.stderr, (bad, r.stderr[-500:])
