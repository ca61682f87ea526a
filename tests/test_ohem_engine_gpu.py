"""Online hard example mining through the engine and the Keras surface, on the configuration of tests/test_losses_engine_gpu.py (64 x 64 x 3 input,
4 classes, batch 2, f32): the mining step against the same model trained under the host-derived drop mask as its void mask, the report against
losses.host_ohem on the step's own per-pixel map, the captured step against the eager pieces, the warm-up under gradient accumulation, the
recorded plans, void masks and focal options together, the checkpoint, compile's refusals and the command line.

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
MINING = dict(kind={"seg": L.LOSS_WCE, "bound": L.LOSS_BCE_LOGITS, "dist": L.LOSS_TANIMOTO, "color": L.LOSS_TANIMOTO}, class_weights=W)
FOCAL = dict(kind={"seg": L.LOSS_FOCAL_CE, "bound": L.LOSS_FOCAL_BCE, "dist": L.LOSS_MSE, "color": L.LOSS_MSE}, class_weights=W,
             focal_gamma={"seg": 2.0, "bound": 2.0}, focal_alpha={"bound": 0.75}, class_balance={"bound": True}, label_smoothing={"seg": 0.1})
SEG_BOUND = {"seg": LS.ohem_options(keep_q16=16384), "bound": LS.ohem_options(keep_q16=LS.ohem_q16(0.1), min_kept=700, thresh=0.5)}


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


def rel_err(got, exp):
    got = np.asarray(got, np.float64); exp = np.asarray(exp, np.float64)
    return float(np.abs(got - exp).max() / (np.abs(exp).max() + 1e-12))


@pytest.fixture
def one_block_stem():
    lib = L.lib()
    before = lib.get_tuning("stem_blocks")
    lib.set_tuning(stem_blocks=1)
    yield
    lib.set_tuning(stem_blocks=before)


def host_of(eng, head, t=0, void=None):
    """host_ohem on the per-pixel map the last training step of `eng` left for `head`, with the head's options and loss weight."""
    g = eng.graphs[(BATCH, True)]
    h = g.outputs[head]
    torch.cuda.synchronize()
    pp = h["ohem"]["per_pixel"].cpu().numpy()
    o = eng.loss.head_ohem(head)
    valid = None if void is None else (np.asarray(void).reshape(-1) == 0)
    return LS.host_ohem(pp, valid, o["keep_q16"], o["min_kept"], o["thresh"], o["warmup"], t, eng.loss.weight[head]), h


def head_loss(res, head):
    """The head's loss value in a multitask result list: [total, seg, bound, dist, color, metrics ...]."""
    return res[1 + HEADS.index(head)]


def assert_report(rep, host, what=""):
    for k in ("tau_key", "K", "n_kept", "n_valid", "q16_used"):
        assert rep[k] == host[k], (what, k, rep[k], host[k])
    assert np.float32(rep["tau"]).view(np.uint32) == np.float32(host["tau"]).view(np.uint32) or (rep["tau"] != rep["tau"] and host["tau"] != host["tau"]), what
    assert np.float32(rep["scale"]).view(np.uint32) == np.float32(host["scale"]).view(np.uint32), what
    assert rep["kept"] == (host["n_kept"] / host["n_valid"] if host["n_valid"] else 0.0)
    assert abs(rep["kept_sum"] - host["kept_sum"]) <= max(host["n_kept"], 1) * 2.0 ** -51 * abs(host["kept_sum"]), what      # two fp64 sums in different orders


# ---- 1. the mining step is the void-mask step under the host's drop mask ------------------------------------------------------------------------
def test_mining_step_equals_void_mask_step():
    """Single task, OHEM on seg, against the same model compiled with ignore_void and fed the host-derived drop mask as void_mask=, its loss weight
    scaled by M / n_kept.  Tolerances: tests/test_losses_engine_gpu.py::test_gamma_zero_is_weighted_cross_entropy's, which compares two engines that
    compute the same mathematics through different entries - losses within 1e-6 max(1, |loss|), rel_err of the gradient buffer < 2e-4."""
    x, y = batch(400, False)
    sp = LossSpec(kind={"seg": L.LOSS_WCE}, weight={"seg": 0.8}, class_weights=W, lr=1e-3, ohem={"seg": LS.ohem_options(keep_q16=16384)})
    a = engine(sp, False, use_graph=False)
    g = a.forward_backward(x, y, _whole_step=True)
    torch.cuda.synchronize()
    ra, ga = a._results(g), a.G.detach().cpu().numpy().copy()
    names = [c[1] for c in g.loss_plan.calls + g.bwd.calls]
    assert names.count("rua_ohem_select") == 1 and names.count("rua_head_dz_sel") == 1 and "rua_head_dz" not in names and g.outputs["seg"]["norm"] == 1.0
    host, h = host_of(a, "seg")
    assert_report(a.ohem_report()["seg"], host)
    assert host["n_valid"] == M and host["K"] == M // 4 and M // 4 <= host["n_kept"] < M
    assert np.array_equal(h["ohem"]["drop_mask"].cpu().numpy(), host["drop_mask"])
    assert abs(ra[0] - 0.8 * host["loss"]) <= 1e-6 * max(1.0, abs(ra[0]))
    sb = LossSpec(kind={"seg": L.LOSS_WCE}, weight={"seg": 0.8 * M / host["n_kept"]}, class_weights=W, lr=1e-3, ignore_void=0)
    b = engine(sb, False, use_graph=False)
    gb_ = b.forward_backward(x, y, _whole_step=True, void_mask=host["drop_mask"].reshape((BATCH,) + SHAPE[:2]))
    torch.cuda.synchronize()
    rb, gb = b._results(gb_), b.G.detach().cpu().numpy().copy()
    print(f"n_kept {host['n_kept']} of {M}, tau {host['tau']:.6f}; loss {ra[0]:.8f} / {rb[0]:.8f}, gradient rel err {rel_err(ga, gb):.2e}")
    assert abs(ra[0] - rb[0]) <= 1e-6 * max(1.0, abs(rb[0]))
    assert np.abs(gb).max() > 0 and rel_err(ga, gb) < 2e-4
    # evaluation makes no selection: the plain mean, the plan of a model without the option
    fresh, plain = engine(sp, False, use_graph=False), engine(LossSpec(kind={"seg": L.LOSS_WCE}, weight={"seg": 0.8}, class_weights=W, lr=1e-3), False, use_graph=False)
    ev = [c[1] for c in fresh.graph(BATCH, False).loss_plan.calls]
    assert ev == [c[1] for c in plain.graph(BATCH, False).loss_plan.calls] and "rua_ohem_select" not in ev
    assert fresh.test_step(x, y) == plain.test_step(x, y) and fresh.ohem_report() is None


# ---- 2. the captured step -------------------------------------------------------------------------------------------------------------------------
def test_captured_step_equals_the_eager_pieces(one_block_stem):
    sp = spec(MINING, ohem=SEG_BOUND)
    a, b = engine(sp), engine(sp, use_graph=False)
    assert a.use_graph
    kept = []
    for k in range(3):                                                   # the warm-up run and two replays, each on its own batch
        x, y = batch(410 + k)
        ra = a.train_step(x, y)
        b.forward_backward(x, y, _whole_step=True)
        b.optimizer_step()
        assert np.isfinite(ra).all()
        assert same(bits(a), bits(b)), k
        rep = a.ohem_report()
        for head in ("seg", "bound"):                                    # no host scalar in between: the replay's own selection matches the host's
            host, _ = host_of(a, head)
            assert_report(rep[head], host, (k, head))
            assert abs(ra[1 + HEADS.index(head)] - host["loss"]) <= 1e-6 * max(1.0, host["loss"])
        kept.append((rep["seg"]["n_kept"], rep["bound"]["n_kept"], rep["seg"]["tau_key"]))
    assert len(a._captured) == 1 and len(set(kept)) == 3, kept


# ---- 3. the warm-up counts updates ----------------------------------------------------------------------------------------------------------------
def test_warmup_counts_updates_under_accumulation():
    q = LS.ohem_q16(0.25)
    sp = LossSpec(kind={"seg": L.LOSS_CE_LOGITS}, weight={"seg": 1.0}, lr=1e-3, gradient_accumulation_steps=2, ohem={"seg": LS.ohem_options(keep_q16=q, warmup=4)})
    eng = engine(sp, False)
    used = []
    for k in range(12):
        x, y = batch(420 + k % 3, False)
        eng.train_step(x, y)
        r = eng.ohem_report()["seg"]
        used.append(r["q16_used"])
        host, _ = host_of(eng, "seg", t=k // 2)
        assert_report(r, host, k)
    assert used == [LS.ohem_share(q, 4, k // 2) for k in range(12)] and used[0] == used[1] == 65536 and used[8:] == [q] * 4 and eng.t == 6
    # the eager pieces read the same counter (pushed in front of the loss plan)
    e2 = engine(LossSpec(kind={"seg": L.LOSS_CE_LOGITS}, weight={"seg": 1.0}, lr=1e-3, ohem={"seg": LS.ohem_options(keep_q16=q, warmup=4)}), False, use_graph=False)
    e2.t = 2
    e2.forward_backward(*batch(420, False), _whole_step=True)
    assert e2.ohem_report()["seg"]["q16_used"] == LS.ohem_share(q, 4, 2)


# ---- 4. multitask: one dz launch, the plans ---------------------------------------------------------------------------------------------------------
def plan_names(g):
    return {k: [c[1] for c in getattr(g, k).calls] for k in ("fwd", "loss_plan", "bwd")}


@pytest.mark.parametrize("void", [None, 2])
def test_recorded_plans(void):
    def build(**kw):
        eng = Engine(config(), dtype="f32", seed=4, split_k=False)
        eng.compile(spec(MINING, ignore_void=void, **kw))
        return {tr: plan_names(eng.graph(BATCH, tr)) for tr in (True, False)}
    off, on = build(), build(ohem=SEG_BOUND)
    sfx = "_void" if void is not None else ""
    new = ("rua_ohem_select", "rua_head_dz_sel", "rua_head_dz_multi_sel")
    # the option off: the calls of a model that never heard of it - no new entry, the entries test_losses_engine_gpu.py::test_recorded_plans finds
    for tr in (True, False):
        assert not [n for k in off[tr] for n in off[tr][k] if n in new]
        assert off[tr]["loss_plan"].count("rua_pixel_loss" + sfx) == 2
        assert off[tr]["bwd"].count("rua_head_dz_multi" + sfx) == (1 if tr else 0)
    assert on[False] == off[False]                                       # evaluation plans make no selection
    assert on[True]["fwd"] == off[True]["fwd"]
    lp = on[True]["loss_plan"]
    assert lp.count("rua_ohem_select") == 2 and [n for n in lp if n != "rua_ohem_select"] == off[True]["loss_plan"]
    for i, n in enumerate(lp):                                           # each selection right behind its head's loss entry
        if n == "rua_ohem_select":
            assert lp[i - 1] == "rua_pixel_loss" + sfx
    bw = on[True]["bwd"]
    assert bw.count("rua_head_dz_multi_sel") == 1 and not [n for n in bw if n.startswith("rua_head_dz") and n != "rua_head_dz_multi_sel"]      # ONE dz launch
    assert [("rua_head_dz_multi" + sfx) if n == "rua_head_dz_multi_sel" else n for n in bw] == off[True]["bwd"]


def test_multitask_mining_with_tanimoto_heads(one_block_stem):
    sp = spec(MINING, ohem=SEG_BOUND)
    eng, ref = engine(sp, use_graph=False), engine(spec(MINING), use_graph=False)
    x, y = batch(430)
    g = eng.forward_backward(x, y, _whole_step=True)
    gr = ref.forward_backward(x, y, _whole_step=True)
    torch.cuda.synchronize()
    res, rr = eng._results(g), ref._results(gr)
    rep = eng.ohem_report()
    assert set(rep) == {"seg", "bound"}
    for head in ("seg", "bound"):
        host, _ = host_of(eng, head)
        assert_report(rep[head], host, head)
        assert abs(res[1 + HEADS.index(head)] - host["loss"]) <= 1e-6 * max(1.0, host["loss"])
    assert rep["bound"]["K"] == 820 and rep["bound"]["n_kept"] >= 820        # the share: ceil(8192 * 6554 / 65536) = 820 > min_kept
    for head in ("dist", "color"):                                       # the Tanimoto heads are untouched: the same loss value, the same dz bytes
        i = 1 + HEADS.index(head)
        assert res[i] == rr[i]
    assert ref.ohem_report() is None


# ---- 5. void, focal and OHEM together ------------------------------------------------------------------------------------------------------------
def test_void_focal_and_mining_together():
    sp = spec(FOCAL, ignore_void=2, ohem=SEG_BOUND, skip_nonfinite=True)
    eng = engine(sp)
    rng = np.random.default_rng(6)
    for k in range(3):
        x, y = batch(440 + k)
        vm = (rng.random((BATCH,) + SHAPE[:2]) < 0.3).astype(np.uint8)
        if k == 2:
            vm[:] = 1                                                    # an all-void batch: nothing kept, scale 0, a zero gradient
        res = eng.train_step(x, y, void_mask=vm)
        assert np.isfinite(res).all(), (k, res)
        rep = eng.ohem_report()
        for head in ("seg", "bound"):
            host, h = host_of(eng, head, void=vm)
            assert_report(rep[head], host, (k, head))
            assert rep[head]["n_valid"] == int((vm == 0).sum())
            assert np.array_equal(h["ohem"]["drop_mask"].cpu().numpy(), host["drop_mask"])
            assert (host["drop_mask"][vm.reshape(-1) != 0] == 1).all()
        if k == 2:
            assert rep["seg"]["n_kept"] == 0 and rep["seg"]["scale"] == 0.0 and res[1] == 0.0
    names = plan_names(eng.graphs[(BATCH, True)])
    assert names["loss_plan"].count("rua_pixel_loss_opts") == 2 and names["bwd"].count("rua_head_dz_multi_sel") == 1


# ---- 6. the Keras surface: compile, save, load, the keep map --------------------------------------------------------------------------------------
def mining_losses():
    return {"seg": ka.OnlineHardExampleMining(ka.weighted_categorical_crossentropy(W), keep_ratio=0.25, min_kept=100, loss_thresh=1.25, warmup_steps=3),
            "bound": ka.OnlineHardExampleMining("binary_crossentropy", keep_ratio=0.5), "dist": ka.MeanSquaredError(), "color": ka.MeanSquaredError()}


def keras_model(losses, seed=11):
    m = ka.Model(config(), dtype="f32", seed=seed)
    m.compile(optimizer=ka.Adam(lr=1e-3), loss=losses, loss_weights=WEIGHT)
    return m


def test_compile_save_and_load(tmp_path, one_block_stem):
    m, whole = keras_model(mining_losses()), keras_model(mining_losses())
    sp = m.engine.loss
    want = {"seg": dict(keep_q16=16384, min_kept=100, thresh=1.25, prob_thresh=None, warmup=3), "bound": dict(keep_q16=32768, min_kept=0, thresh=None, prob_thresh=None, warmup=0)}
    assert sp.ohem == want and sp.loss_options() == dict(ohem=want) and sp.kind["seg"] == L.LOSS_WCE and sp.class_weights == W
    assert m.ohem_report() is None                                       # no training step yet
    m.train_on_batch(*batch(450))
    assert m.ohem_report()["seg"]["q16_used"] == 65536
    path = str(tmp_path / "ohem.h5")
    m.save(path)
    raw = h5lite.read_h5(path).attrs["rua_checkpoint"]
    assert json.loads(raw.decode("utf8") if isinstance(raw, bytes) else raw)["loss"]["ohem"] == want
    m2 = ka.load_model(path)
    assert m2.engine.loss.ohem == want and m2.engine.loss.kind == sp.kind
    m2.train_on_batch(*batch(451))
    for k in range(2):
        whole.train_on_batch(*batch(450 + k))
    assert same(bits(m2.engine), bits(whole.engine)) and m2.engine.t == whole.engine.t == 2
    assert m2.ohem_report() == whole.ohem_report() and m2.ohem_report()["seg"]["q16_used"] == LS.ohem_share(16384, 3, 1)      # the warm-up goes on from the file's counter


def test_keep_map_from_the_gpu():
    rng = np.random.default_rng(8)
    yp = rng.random((2, 33, 31, NCLS)).astype(np.float32) + 0.05
    yp /= yp.sum(-1, keepdims=True)
    yt = np.eye(NCLS, dtype=np.float32)[rng.integers(0, NCLS, (2, 33, 31))]
    inner = ka.weighted_categorical_crossentropy(W)
    m = ka.OnlineHardExampleMining(inner, keep_ratio=0.25, prob_thresh=0.2)
    keep = m(yt, yp)
    host = LS.host_ohem(inner(yt, yp), None, 16384, 0, LS.prob_to_thresh(0.2))
    assert keep.shape == (2, 33, 31) and keep.dtype == np.uint8 and np.array_equal(keep, 1 - host["drop_mask"]) and 0 < keep.sum() < keep.size


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_compile_refusals_come_before_any_launch():
    eng = Engine(config(), dtype="f32", seed=3, split_k=False)
    def refuse(match, base=MINING, **kw):
        with pytest.raises(ValueError, match=match):
            eng.compile(spec(base, **kw))
    refuse("Tanimoto", ohem={"dist": LS.ohem_options()})                 # a Tanimoto head has no per-pixel map
    refuse("not a head", ohem={"segg": LS.ohem_options()})
    refuse("keep_q16", ohem={"seg": dict(keep_q16=0)})
    refuse("keep_q16", ohem={"seg": dict(keep_q16=70000)})
    refuse("min_kept", ohem={"seg": dict(min_kept=-1)})
    refuse("warmup", ohem={"bound": dict(warmup=-2)})
    refuse("NaN", ohem={"seg": dict(thresh=float("nan"))})
    refuse("unknown", ohem={"seg": dict(keep_ratio=0.25)})
    refuse("a dict", ohem={"seg": 0.25})
    pt = LS.ohem_options(prob_thresh=0.7)
    refuse("prob_thresh", ohem={"seg": pt})                              # weighted CE with weights that are not 1
    refuse("prob_thresh", ohem={"bound": pt})                            # a sigmoid head's BCE
    refuse("prob_thresh", base=FOCAL, ohem={"seg": pt})
    refuse("prob_thresh", base=dict(MINING, kind={**MINING["kind"], "seg": L.LOSS_CE_LOGITS}), label_smoothing={"seg": 0.1}, ohem={"seg": pt})
    refuse("disagree", ohem={"seg": dict(prob_thresh=0.7, thresh=0.1)})
    assert not eng.graphs and eng.loss is None
    eng.compile(spec(dict(MINING, kind={**MINING["kind"], "seg": L.LOSS_CE_LOGITS}), ohem={"seg": pt}))          # plain CE takes it
    eng.compile(spec(dict(MINING, class_weights=[1.0] * NCLS), ohem={"seg": pt}))                                # ... and weighted CE with unit weights
    assert not eng.graphs
    m = ka.Model(config(), dtype="f32", seed=3)
    with pytest.raises(ValueError, match="Tanimoto"):
        m.compile(optimizer=ka.Adam(lr=1e-3), loss={"seg": ka.OnlineHardExampleMining("tanimoto"), "bound": "tanimoto", "dist": "tanimoto", "color": "tanimoto"})
    assert not m.engine.graphs and not m._compiled


# ---- 8. the command line ----------------------------------------------------------------------------------------------------------------------------
def test_cli_ohem_trains_and_stores_its_options(tmp_path):
    """Two epochs of `--ohem yes` on a seeded 160 x 192 scene (-ps 64, stride 32: 16 training windows, four steps per epoch) on the seg and boundary
    heads, with a warm-up and void pixels: it runs to the end, every scalar is finite, the per-epoch line is printed and the saved model carries
    the options."""
    img, cls = blob_scene(200, 160, 192)
    root, results = str(tmp_path / "scenes"), str(tmp_path / "run")
    scenes.save_scene_dir(root, ["tile"], [img], [cls])
    cmd = [sys.executable, os.path.join(ROOT, "train_ISPRS.py"), "--resunet_a", "yes", "--multitasking", "yes", "--loss", "weighted_cross_entropy",
           "--class_weights", "auto", "--ohem", "yes", "--ohem_keep", "0.3", "--ohem_min_kept", "500", "--ohem_thresh", "0.9", "--ohem_warmup", "3",
           "--ohem_heads", "seg", "bound", "--ignore_void", "yes", "--scene_dataset", "yes",
           "-rp", results, "-dp", root, "-bs", "4", "-ps", "64", "--num_classes", str(NCLS), "--epochs", "2", "--dtype", "f32", "--norm_type", "1",
           "--seed", "5", "--stride", "32", "--data_aug", "no"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "Online hard example mining on seg, bound" in r.stdout and r.stdout.count("Hard example mining (last step): seg kept") == 2
    tr, va = read_scalars(os.path.join(results, "logs", "train", "scalars.jsonl")), read_scalars(os.path.join(results, "logs", "val", "scalars.jsonl"))
    assert tr and va and all(np.isfinite(v["value"]) for v in tr + va if v["tag"] != "Segmentation/MCC")
    raw = h5lite.read_h5(os.path.join(results, "best_model.h5")).attrs["rua_checkpoint"]
    lo = json.loads(raw.decode("utf8") if isinstance(raw, bytes) else raw)["loss"]
    one = dict(keep_q16=LS.ohem_q16(0.3), min_kept=500, thresh=float(np.float32(0.9)), prob_thresh=None, warmup=3)
    assert lo["ohem"] == {"seg": one, "bound": one}
    # flags that contradict each other are refused before anything is loaded
    for bad, word in ((["--ohem_keep", "0.5"], "--ohem yes"), (["--ohem", "yes", "--loss", "tanimoto"], "Tanimoto"),
                      (["--ohem", "yes", "--ohem_prob", "0.7"], "--ohem_prob"), (["--ohem", "yes", "--ohem_keep", "0"], "keep_ratio"),
                      (["--ohem", "yes", "--ohem_heads", "bound"], "--multitasking")):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "train_ISPRS.py"), "--resunet_a", "yes", "-rp", results, "-dp", root] + bad, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and word in r.stderr, (bad, r.stderr[-500:])
