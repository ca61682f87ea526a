"""Gradient clipping, decoupled weight decay and the non-finite step skip through the engine and the Keras surface, on the smallest graph the engine
tests use (64 x 64 input, batch 2): the eager path against clip.host_clipped_step on the gradients read back, the whole-step HIP graph (warm-up,
capture, replay) through the report, the skip with a poisoned gradient, the default path's dispatch count and bits, and the checkpoint.

The weights are compared under tests/test_clip_gpu.py's one-step Adam bound with m = v = 0 (a fresh engine), u = 2^-23, K = 2:
  |th' - th'_ref| <= u |th'_ref| + E_dec + (4e-6 + K u) |delta_ref| + lr_t e_m / (sqrt(v'_ref) + eps),   e_m = (4 + K) u (1 - beta1) |gg|
The non-finite gradient of the graph path is NOT produced through a batch (a NaN input would run every kernel of the step on NaNs to no purpose):
the graph path is covered by the finite cases, the skip by the eager path and by the kernel tests."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from _kernel_util import U32, bits_of, worst_ratio  # noqa: E402
from resunet_a_mltsk_keras_amd import _lib as L  # noqa: E402
from resunet_a_mltsk_keras_amd import clip as CL  # noqa: E402
from resunet_a_mltsk_keras_amd import keras_api as ka  # noqa: E402
from resunet_a_mltsk_keras_amd.engine import HEADS, KERAS_EPS, Engine, LossSpec, ModelConfig  # noqa: E402
from resunet_a_mltsk_keras_amd.synthetic import make_batch  # noqa: E402

f32, f64 = np.float32, np.float64
SHAPE, NCLS, BATCH = (64, 64, 3), 4, 2
K = 2
# kernel nodes of the whole training step of this configuration on the commit before the feature (count_step_dispatches there, f32 and bf16)
PARENT_DISPATCHES = {"f32": 381, "bf16": 276}


def spec(**kw):
    return LossSpec(kind={h: L.LOSS_TANIMOTO for h in HEADS}, weight={"seg": 1.0, "bound": 0.7, "dist": 1.3, "color": 0.5}, lr=1e-3, **kw)


def engine(dtype, **kw):
    eng = Engine(ModelConfig(input_shape=SHAPE, num_classes=NCLS, multitasking=True, width=32), dtype=dtype, seed=4, split_k=False)
    eng.compile(spec(**kw))
    return eng


def batch(seed):
    return make_batch(BATCH, SHAPE[0], SHAPE[2], NCLS, True, seed=seed, block=16)


def lr_t(t, lr=1e-3, b1=0.9, b2=0.999):
    return f64(f32(lr * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)))


def check_first_step(eng, P0, G, kw, wd=0.0):
    """P after the engine's FIRST Adam step against the host definition on the gradients G read before it; returns the host result."""
    ps = eng.params
    chunks, vars_, names = CL.build_chunk_table(ps.entries, eng.loss.decay_exclude or ())
    n = ps.n
    z = np.zeros(n)
    ref = CL.host_clipped_step(P0[:n], G[:n], z, z, chunks, vars_, optimizer="adam", lr=lr_t(1), lr_base=1e-3, beta_1=f64(f32(0.9)), beta_2=f64(f32(0.999)),
                               eps=f64(f32(KERAS_EPS)), grad_scale=1.0, weight_decay=wd, **kw)
    ins = CL.covered(chunks, n) == 1
    gg, th1, th_ref = ref["gg"][ins], ref["th1"][ins], ref["theta"][ins]
    den = np.sqrt(ref["v"][ins]) + f64(f32(KERAS_EPS))
    delta = lr_t(1) * ref["m"][ins] / den
    e_m = (4 + K) * U32 * (1 - f64(f32(0.9))) * np.abs(gg)
    d = f64(f32(wd * 1e-3))
    decays = np.zeros(n, bool)
    for off, ln, var in chunks.tolist():
        decays[off:off + ln] = bool(wd) and bool(vars_["decay"][var])
    e_dec = np.where(decays[ins], U32 * np.abs(P0[:n][ins].astype(f64) * d) + U32 * np.abs(th1), 0.0)
    e_th = U32 * np.abs(th_ref) + e_dec + (4e-6 + K * U32) * np.abs(delta) + lr_t(1) * e_m / den
    got = eng.P.cpu().numpy()[:n]
    r = worst_ratio(np.abs(got[ins].astype(f64) - th_ref), e_th)
    assert (got[~ins] == 0).all()                                                  # padding stays zero
    if eng.opt_wcopy:
        assert (bits_of(eng.Wf[:ps.nw]) == bits_of(eng.P.cpu()[:ps.nw].to(torch.bfloat16))).all()
    return ref, r, (chunks, vars_, names)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_eager_global_clipnorm_against_the_host_definition(dtype):
    eng = engine(dtype)
    x, y = batch(40)
    eng.forward_backward(x, y)
    torch.cuda.synchronize()
    G, P0 = eng.G.cpu().numpy().copy(), eng.P.cpu().numpy().copy()
    chunks, vars_, _ = CL.build_chunk_table(eng.params.entries)
    _, total = CL.host_sumsq(G[:eng.params.n], chunks, vars_)
    norm = float(np.sqrt(total))
    assert np.isfinite(norm) and norm > 0
    eng.compile(spec(global_clipnorm=0.5 * norm, weight_decay=0.05, decay_exclude=list(CL.DEFAULT_DECAY_EXCLUDE)))   # the plan goes, G stays
    eng.optimizer_step()
    rep = eng.clip_report()
    L_all = int(chunks["len"].sum())
    r_norm = abs(rep["norm"] ** 2 - total) / (total * (L_all + 4) * 2.0 ** -53)
    ref, r_th, _ = check_first_step(eng, P0, G, dict(global_clipnorm=0.5 * norm), wd=0.05)
    print(f"{dtype} eager global_clipnorm: norm {rep['norm']:.6g}; ratio to the bound: norm^2 {r_norm:.3f} theta {r_th:.3f}")
    assert r_norm <= 1.0 and r_th <= 1.0
    assert rep["clipped"] == 1 and rep["skipped"] == 0
    assert abs(rep["min_coef"] - float(ref["coef"][0])) <= float(np.spacing(ref["coef"][0]))
    assert (eng.G.cpu().numpy()[:eng.params.n] == 0).all()


def test_clipnorm_gives_the_segments_of_one_kernel_one_coefficient():
    eng = engine("f32", clipnorm=1e-3)
    x, y = batch(41)
    eng.forward_backward(x, y)
    torch.cuda.synchronize()
    G, P0 = eng.G.cpu().numpy().copy(), eng.P.cpu().numpy().copy()
    eng.optimizer_step()
    ref, r_th, (chunks, vars_, names) = check_first_step(eng, P0, G, dict(clipnorm=1e-3))
    coef = eng.clip["coef"].cpu().numpy()[:len(names)]
    per_name = {}
    for e in eng.params.entries:
        per_name.setdefault(e["name"], []).append(e)
    shared = [nm for nm, es in per_name.items() if len(es) > 1]
    assert shared and len(names) == len(per_name) < len(eng.params.entries)
    worst = 0.0
    for nm in shared:
        v = names.index(nm)
        ss = sum(float(np.dot(G[e["off"]:e["off"] + e["size"]].astype(f64), G[e["off"]:e["off"] + e["size"]].astype(f64))) for e in per_name[nm])
        exp = f32(1e-3 / max(np.sqrt(ss), 1e-3))
        worst = max(worst, abs(float(coef[v]) - float(exp)) / float(np.spacing(exp)))
    print(f"clipnorm: {len(shared)} variables of several segments, worst coefficient {worst:.2f} ulp; theta ratio to the bound {r_th:.3f}")
    assert worst <= 1.0 and r_th <= 1.0
    assert (coef < 1).any() and eng.clip_report()["clipped"] == 1


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_graph_path_computes_the_coefficient_at_every_replay(dtype):
    c = 1e-3
    eng = engine(dtype, global_clipnorm=c)
    assert eng.use_graph and eng.dist is None
    norms = []
    for k, seed in enumerate((50, 51, 52)):                                        # warm-up + capture, replay, replay
        x, y = batch(seed)
        assert np.all(np.isfinite(eng.train_step(x, y)))
        rep = eng.clip_report()
        assert rep["norm"] > c and rep["min_coef"] == float(f32(c / max(rep["norm"], c))), rep
        assert rep["clipped"] == k + 1 and rep["skipped"] == 0
        norms.append(rep["norm"])
    assert BATCH in eng._captured
    print(f"{dtype} graph path: norms {norms}")
    assert len(set(norms)) == 3
    assert np.isfinite(eng.P.cpu().numpy()).all()


@pytest.mark.parametrize("dtype,opt", [("f32", "adam"), ("bf16", "adam"), ("bf16", "sgd")])
def test_eager_skip_keeps_weights_moments_and_state(dtype, opt):
    eng = engine(dtype, optimizer=opt, momentum=0.8, skip_nonfinite=True, global_clipnorm=1.0, weight_decay=0.01)
    n, ns = eng.params.n, eng.params.ns
    x, y = batch(60)
    before = [bits_of(t).copy() for t in (eng.P, eng.M1, eng.V1, eng.S)]
    eng.forward_backward(x, y)
    torch.cuda.synchronize()
    assert (bits_of(eng.S) != before[3]).any()                                    # the forward folded the batch into the moving statistics
    e = eng.params.entries[len(eng.params.entries) // 2]
    eng.G[e["off"] + e["size"] - 1] = float("inf")
    eng.S[3] = float("nan")
    eng.optimizer_step()
    rep = eng.clip_report()
    assert rep["skipped"] == 1 and rep["clipped"] == 0
    for t, b in zip((eng.P, eng.M1, eng.V1, eng.S), before):
        assert (bits_of(t) == b).all()
    assert (eng.G.cpu().numpy()[:n] == 0).all()
    if eng.opt_wcopy:
        assert (bits_of(eng.Wf[:eng.params.nw]) == bits_of(eng.P.cpu()[:eng.params.nw].to(torch.bfloat16))).all()
    assert eng.t == 1                                                             # a skipped step still costs one t
    # the next clean step moves the weights
    eng.forward_backward(x, y)
    eng.optimizer_step()
    rep = eng.clip_report()
    P = eng.P.cpu().numpy()
    assert rep["skipped"] == 1 and np.isfinite(P).all() and (bits_of(eng.P) != before[0]).any()
    assert np.isfinite(eng.S.cpu().numpy()).all() and (bits_of(eng.S) != before[3]).any()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_dispatch_counts(dtype):
    """Options off: the parent's count.  A clip option adds the sum of squares and the finisher (the segmented optimizer takes the flat one's place),
    skip_nonfinite the state's backup and restore."""
    x, y = batch(70)
    counts = {}
    for name, kw in (("off", {}), ("clip", dict(global_clipnorm=1.0)), ("all", dict(clipnorm=1.0, weight_decay=0.01, skip_nonfinite=True))):
        eng = engine(dtype, **kw)
        eng.train_step(x, y)
        counts[name] = eng.count_step_dispatches(BATCH)
    print(f"{dtype} dispatches per step: {counts}")
    assert counts["off"] == PARENT_DISPATCHES[dtype]
    assert counts["clip"] == counts["off"] + 2 and counts["all"] == counts["off"] + 4


@pytest.fixture
def one_block_stem():
    """Two runs of a training step give the same bits only if the step is a function of its inputs: every block of rua_stem_bwd ends in one float
    atomic per weight, in the order the hardware schedules the blocks.  With the tuning key stem_blocks = 1 that kernel is one block - on both
    sides alike (tests/test_scene_photo_gpu.py pins it the same way, for the same reason)."""
    lib = L.lib()
    before = lib.get_tuning("stem_blocks")
    lib.set_tuning(stem_blocks=1)
    yield
    lib.set_tuning(stem_blocks=before)


def test_options_off_is_the_parent_path_bit_for_bit(one_block_stem):
    """A LossSpec built without the new fields and one that names every one of them at its off value: the same calls, the same bits after two steps."""
    res = []
    for kw in ({}, dict(clipnorm=None, global_clipnorm=None, clipvalue=None, weight_decay=None, decay_exclude=None, skip_nonfinite=False)):
        eng = engine("f32", **kw)
        assert eng.clip is None and eng.clip_report() is None
        for seed in (80, 81):
            eng.train_step(*batch(seed))
        torch.cuda.synchronize()
        res.append([bits_of(t).copy() for t in (eng.P, eng.M1, eng.V1, eng.S)])
    for a, b in zip(*res):
        assert (a == b).all()


def test_checkpoint_restores_the_options_and_starts_the_counters_at_zero(tmp_path):
    m = ka.Model(ModelConfig(input_shape=SHAPE, num_classes=NCLS, multitasking=True), dtype="f32", seed=11)
    opt = ka.Adam(lr=1e-3, global_clipnorm=1e-3, weight_decay=0.02, skip_nonfinite=True)
    opt.exclude_from_weight_decay(var_names=["bias", "gamma", "beta"])
    m.compile(optimizer=opt, loss={h: ka.Tanimoto_dual_loss() for h in HEADS})
    x, y = make_batch(BATCH, 64, 3, NCLS, True, seed=2, block=16)
    m.train_on_batch(x, y)
    assert m.clip_report()["clipped"] == 1
    path = str(tmp_path / "clip.h5")
    m.save(path)
    m2 = ka.load_model(path)
    assert m2.engine.loss.clip_options() == m.engine.loss.clip_options() == dict(
        clipnorm=None, global_clipnorm=1e-3, clipvalue=None, weight_decay=0.02, decay_exclude=["bias", "gamma", "beta"], skip_nonfinite=True)
    assert m2.optimizer.global_clipnorm == 1e-3 and m2.optimizer.decay_exclude == ["bias", "gamma", "beta"]
    rep = m2.clip_report()
    assert rep["clipped"] == 0 and rep["skipped"] == 0
    m2.train_on_batch(x, y)
    assert m2.clip_report()["clipped"] == 1
