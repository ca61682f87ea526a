"""LAMB through the engine and the Keras surface, on the smallest graph the engine tests use (64 x 64 x 3 input, 4 classes, batch 2, width 32), in
f32 and bf16: the eager first step against lamb.host_lamb_step on the gradients read back, the whole-step HIP graph (warm-up, capture, replays)
against an eager twin, the composition with clipping, decay, a schedule, the moving average and accumulation, the skip, the checkpoint, the
report and the dispatch counts.

The first step's weights are compared twice: bit for bit with host_lamb_step given the device's ratios (everywhere), and with the float64
restatement under the bound tests/test_lamb_host.py derives, plus one float32 ulp of the ratio on the step, spacing(ratio) * lr * |u| (where
the gradient's square is a normal number: the bound's error model).

Where two engines are compared bit for bit the step has to be a function of its inputs: rua_stem_bwd is pinned to one block and, in bf16,
stem_mfma is off on both sides, as tests/test_accum_engine_gpu.py explains; its premise - train_step equals forward_backward(_whole_step=True) +
optimizer_step() bit for bit in that configuration - is asserted there."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from _kernel_util import bits_of  # noqa: E402
from _lamb_ref import SLACK, float64_step, worst  # noqa: E402
from resunet_a_mltsk_keras_amd import _lib as L  # noqa: E402
from resunet_a_mltsk_keras_amd import accum as AC  # noqa: E402
from resunet_a_mltsk_keras_amd import clip as CL  # noqa: E402
from resunet_a_mltsk_keras_amd import keras_api as ka  # noqa: E402
from resunet_a_mltsk_keras_amd import lamb as LB  # noqa: E402
from resunet_a_mltsk_keras_amd import schedules as SC  # noqa: E402
from resunet_a_mltsk_keras_amd.engine import HEADS, Engine, LossSpec, ModelConfig  # noqa: E402
from resunet_a_mltsk_keras_amd.synthetic import make_batch  # noqa: E402

f32, f64 = np.float32, np.float64
SHAPE, NCLS, BATCH = (64, 64, 3), 4, 2
DTYPES = ["f32", "bf16"]
# kernel nodes of the whole training step of this configuration under adam and under sgd with every optimizer option off: count_step_dispatches
# on commit d1b18b3 (focal losses and label smoothing), the parent of this feature
PARENT_DISPATCHES = {"f32": 381, "bf16": 276}


def spec(**kw):
    return LossSpec(kind={h: L.LOSS_TANIMOTO for h in HEADS}, weight={"seg": 1.0, "bound": 0.7, "dist": 1.3, "color": 0.5}, lr=1e-3, **kw)


def config():
    return ModelConfig(input_shape=SHAPE, num_classes=NCLS, multitasking=True, width=32)


def engine(dtype, pinned=False, **kw):
    eng = Engine(config(), dtype=dtype, seed=4, split_k=False)
    if pinned:
        eng.stem_mfma = False
    eng.compile(spec(**kw))
    return eng


def batch(seed):
    return make_batch(BATCH, SHAPE[0], SHAPE[2], NCLS, True, seed=seed, block=16)


def bits(eng, names=("P", "M1", "V1")):
    torch.cuda.synchronize()
    return [bits_of(getattr(eng, n)).copy() for n in names] + ([bits_of(eng.clip["ratio"]).copy()] if eng.clip and "ratio" in eng.clip else [])


def same(a, b):
    return len(a) == len(b) and all((x == y).all() for x, y in zip(a, b))


def ratios_of(eng):
    torch.cuda.synchronize()
    return eng.clip["ratio"].cpu().numpy()[:eng.clip["n_vars"]].copy()


def ulps32(got, exp):
    exp = np.asarray(exp, f32)
    return float(np.max(np.abs(np.asarray(got, f64) - exp.astype(f64)) / np.spacing(np.abs(exp)).astype(f64)))


@pytest.fixture
def one_block_stem():
    lib = L.lib()
    before = lib.get_tuning("stem_blocks")
    lib.set_tuning(stem_blocks=1)
    yield
    lib.set_tuning(stem_blocks=before)


def host_update(eng, P0, G, M, V, *, t, lr, lr_base=None, coef=None, ratio=None):
    sp, n = eng.loss, eng.params.n
    chunks, vars_, names = CL.build_chunk_table(eng.params.entries, sp.decay_exclude or ())
    h = LB.host_lamb_step(P0[:n], G[:n], M[:n], V[:n], chunks, vars_, t=t, lr=lr, lr_base=lr if lr_base is None else lr_base, beta_1=sp.beta_1,
                          beta_2=sp.beta_2, eps=sp.epsilon, grad_scale=1.0, coef=coef, clipvalue=sp.clipvalue, weight_decay=sp.weight_decay or 0.0, ratio=ratio)
    return h, (chunks, vars_, names)


def apply_ratios(h, chunks, ratio, lr):
    """host_lamb_step's last line with the device's ratios: theta' = th1 - (ratio * lr) * u in float32, one product per variable for the step
    (what host_lamb_step(ratio=...) returns as theta, without a second walk over the table)."""
    step = np.zeros(h["u"].size, f32)
    per_var = np.asarray(ratio, f32) * f32(lr)
    for off, ln, var in chunks.tolist():
        step[off:off + ln] = per_var[var]
    theta = h["th1"] - step * h["u"]
    assert theta.dtype == f32
    return theta


@pytest.mark.parametrize("dtype", DTYPES)
def test_eager_first_step_against_the_host_definition(dtype):
    eng = engine(dtype, optimizer="lamb")
    assert eng.clip is not None and eng.clip["plain"] and eng.clip_report() is None
    n = eng.params.n
    eng.forward_backward(*batch(40))
    torch.cuda.synchronize()
    G, P0 = eng.G.cpu().numpy().copy(), eng.P.cpu().numpy().copy()
    z = np.zeros(n, f32)
    eng.optimizer_step()
    ratio = ratios_of(eng)
    h, (chunks, vars_, names) = host_update(eng, P0, G, z, z, t=1, lr=1e-3)
    ins = CL.covered(chunks, n) == 1
    ul = ulps32(ratio, h["ratio"])
    rep = eng.trust_report()
    assert ul <= 1.0 and rep["updates"] == 1 and rep["forced"] == LB.host_ratio_report(h["W"], h["U"])["forced"]
    assert rep["min_ratio"] == ratio.min() and rep["max_ratio"] == ratio.max() and list(rep["ratios"]) == names
    # bit for bit given the device's ratios; the moments bit for bit
    P, M1, V1 = (t.cpu().numpy()[:n] for t in (eng.P, eng.M1, eng.V1))
    for got, want, k in ((P, apply_ratios(h, chunks, ratio, 1e-3), "theta"), (M1, h["m"], "m"), (V1, h["v"], "v")):
        assert (got.view(np.uint32)[ins] == want.view(np.uint32)[ins]).all(), k
    assert (P[~ins] == 0).all() and (eng.G.cpu().numpy()[:n] == 0).all()
    # the float64 formulas under the host test's bound, plus one ulp of the ratio on the step
    ref = float64_step(P0[:n], G[:n], z, z, chunks, vars_, t=1, lr=1e-3, lr_base=1e-3, b1=0.9, b2=0.999, eps=1e-7, gs=1.0, coef=np.ones(len(vars_), f32),
                       cv=None, wd=0.0, ratio=h["ratio"])
    per_el = np.zeros(n, f64)
    for off, ln, var in chunks.tolist():
        per_el[off:off + ln] = np.spacing(h["ratio"][var])
    bound = SLACK * (ref["E_th"] + per_el * 1e-3 * np.abs(ref["u"]))
    gsq = G[:n].astype(f64) ** 2
    normal = ins & ((gsq == 0) | (gsq >= 2.0 ** -100))
    r_th = worst(np.abs(P.astype(f64) - ref["theta"])[normal], bound[normal])
    print(f"{dtype} first LAMB step: ratio {ul:.2f} ulp, {ratio.min():.4g} .. {ratio.max():.4g}, forced {rep['forced']}; theta's worst error / bound {r_th:.3f} "
          f"over {normal.sum()} of {ins.sum()} elements")
    assert r_th <= 1.0 and normal.sum() >= 0.99 * ins.sum()
    assert (P[ins] != P0[:n][ins]).any()
    if eng.opt_wcopy:
        assert (bits_of(eng.Wf[:eng.params.nw]) == bits_of(eng.P.cpu()[:eng.params.nw].to(torch.bfloat16))).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_captured_step_equals_the_eager_twin_bit_for_bit(dtype, one_block_stem):
    """Warm-up and capture, then three replays: P, M1, V1 and the ratios of all four steps are an eager engine's, fed the same batches."""
    a, b = engine(dtype, pinned=True, optimizer="lamb"), engine(dtype, pinned=True, optimizer="lamb")
    assert a.use_graph and a.dist is None
    seen = []
    for k in range(4):
        x, y = batch(300 + k)
        assert np.all(np.isfinite(a.train_step(x, y)))
        b.forward_backward(x, y, _whole_step=True)
        b.optimizer_step()
        assert same(bits(a), bits(b)), (dtype, k)
        seen.append(ratios_of(a))
        assert a.trust_report()["updates"] == k + 1 == b.trust_report()["updates"]
    assert BATCH in a._captured and a.t == 4 == b.t
    assert all((seen[k] != seen[k + 1]).any() for k in range(3))                     # computed at every replay, not replayed
    assert np.isfinite(a.P.cpu().numpy()).all()
    if a.opt_wcopy:
        assert (bits_of(a.Wf[:a.params.nw]) == bits_of(a.P.cpu()[:a.params.nw].to(torch.bfloat16))).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_composition_with_clip_decay_schedule_average_and_accumulation(dtype, one_block_stem):
    """Lamb(global_clipnorm, weight_decay, CosineDecay with warm-up, use_ema, gradient_accumulation_steps=2) on the graph path, four micro-steps
    (hold, update, hold, update).  A hold step keeps P, M1, V1, the ratios, the report, the rate and the average; an update is the host
    definition applied to the mean gradient - a twin engine's gradients at the engine's weights, accumulated by accum.host_accumulate - with the
    coefficient and the rate the device used; t, the schedule and the average count updates."""
    c = 1e-3
    sched = SC.CosineDecay(1e-4, 6, alpha=0.1, warmup_target=2e-3, warmup_steps=2)
    eng = engine(dtype, pinned=True, optimizer="lamb", global_clipnorm=c, weight_decay=0.05, decay_exclude=list(CL.DEFAULT_DECAY_EXCLUDE), lr_schedule=sched,
                 use_ema=True, ema_momentum=0.9, gradient_accumulation_steps=2)
    twin = engine(dtype, pinned=True, optimizer="lamb")                             # only ever produces gradients: it never steps
    assert eng.use_graph and eng.dist is None and not eng.clip["plain"]
    n = eng.params.n
    chunks, vars_, names = CL.build_chunk_table(eng.params.entries, eng.loss.decay_exclude)
    ins = CL.covered(chunks, n) == 1
    acc, micro, updates = np.zeros(n, f32), 0, 0
    E = eng.E.cpu().numpy().copy()
    for step in range(1, 5):
        x, y = batch(320 + step)
        before, rep0, lr0 = bits(eng), eng.trust_report(), (eng.lr_state.cpu().numpy().copy(), bits_of(eng.lr_dev).copy())
        P0, M0, V0 = (t.cpu().numpy().copy() for t in (eng.P, eng.M1, eng.V1))
        assert eng.current_lr() == SC.host_lr(sched, updates)
        twin.P.copy_(eng.P); twin.S.copy_(eng.S)
        twin.params_changed()
        twin.forward_backward(x, y, _whole_step=True)
        torch.cuda.synchronize()
        g = twin.G[:n].cpu().numpy().copy()
        twin.G.zero_()
        acc, g_out, micro = AC.host_accumulate(acc, g, micro, 2)
        eng.train_step(x, y, fetch=False)
        torch.cuda.synchronize()
        assert (eng.G[:n] == 0).all()
        assert eng.accumulation_state() == dict(steps=2, micro=step % 2)
        if g_out is None:                                                            # a hold step
            assert same(bits(eng), before) and eng.trust_report() == rep0, (dtype, step)
            if step > 1:                                                             # (the first step's host push wrote the pair)
                assert (eng.lr_state.cpu().numpy() == lr0[0]).all() and (bits_of(eng.lr_dev) == lr0[1]).all()
            assert (bits_of(eng.E) == E.view(np.uint32)).all() and eng.t == updates
            continue
        updates += 1
        rate = SC.host_lr(sched, updates - 1)
        assert eng.t == updates and eng.lr_state.cpu().numpy().tolist() == [float(updates), rate]
        assert float(eng.lr_dev.cpu().numpy()[0]) == float(f32(rate))                # adam = 0: the rate itself, the bias correction is per element
        coef = eng.clip["coef"].cpu().numpy()[:len(vars_)].copy()
        per, total = CL.host_sumsq(g_out, chunks, vars_)
        assert ulps32(coef, CL.host_coef(per, total, CL.CLIP_GLOBAL_NORM, c, 1.0)) <= 1.0 and (coef < 1).all() and eng.clip_report()["clipped"] == updates
        ratio = ratios_of(eng)
        h, _ = host_update(eng, P0, g_out, M0, V0, t=updates, lr=rate, coef=coef)
        ul = ulps32(ratio, h["ratio"])
        print(f"{dtype} update {updates}: rate {rate:.6g}, coefficient {coef[0]:.4g}, ratio {ul:.2f} ulp, {ratio.min():.4g} .. {ratio.max():.4g}")
        assert ul <= 1.0
        for t_, want, k in ((eng.P, apply_ratios(h, chunks, ratio, rate), "theta"), (eng.M1, h["m"], "m"), (eng.V1, h["v"], "v")):
            assert (bits_of(t_)[:n][ins] == want.view(np.uint32)[ins]).all(), (dtype, step, k)
        assert (h["th1"][ins] != P0[:n][ins]).any()                                # the decay did act
        assert eng.trust_report()["updates"] == updates
        E, _ = SC.host_ema(E, eng.P.cpu().numpy(), 0.9, updates)
        assert (bits_of(eng.E) == E.view(np.uint32)).all(), (dtype, step)
        if eng.opt_wcopy:
            assert (bits_of(eng.Wf[:eng.params.nw]) == bits_of(eng.P.cpu()[:eng.params.nw].to(torch.bfloat16))).all()
    assert updates == 2 == eng.t and BATCH in eng._captured


@pytest.mark.parametrize("dtype", DTYPES)
def test_eager_skip_keeps_weights_moments_state_and_the_update_count(dtype):
    eng = engine(dtype, optimizer="lamb", skip_nonfinite=True, weight_decay=0.01)
    n = eng.params.n
    x, y = batch(60)
    eng.forward_backward(x, y)
    eng.optimizer_step()                                                             # one clean update first: moments and ratios are not zero
    torch.cuda.synchronize()
    before = [bits_of(t).copy() for t in (eng.P, eng.M1, eng.V1, eng.S)]
    r0, rep0 = bits_of(eng.clip["ratio"]).copy(), eng.trust_report()
    assert rep0["updates"] == 1
    eng.forward_backward(x, y)
    torch.cuda.synchronize()
    assert (bits_of(eng.S) != before[3]).any()                                        # the forward folded the batch into the moving statistics
    e = eng.params.entries[len(eng.params.entries) // 2]
    eng.G[e["off"] + e["size"] - 1] = float("inf")
    eng.S[3] = float("nan")
    eng.optimizer_step()
    assert eng.clip_report()["skipped"] == 1
    for t, b in zip((eng.P, eng.M1, eng.V1, eng.S), before):
        assert (bits_of(t) == b).all()
    assert (bits_of(eng.clip["ratio"]) == r0).all() and eng.trust_report() == rep0    # updates does not advance
    assert (eng.G.cpu().numpy()[:n] == 0).all()
    if eng.opt_wcopy:
        assert (bits_of(eng.Wf[:eng.params.nw]) == bits_of(eng.P.cpu()[:eng.params.nw].to(torch.bfloat16))).all()
    assert eng.t == 2                                                                 # a skipped step still costs one t
    eng.forward_backward(x, y)
    eng.optimizer_step()
    assert eng.trust_report()["updates"] == 2 and np.isfinite(eng.P.cpu().numpy()).all() and (bits_of(eng.P) != before[0]).any()


def keras_model(opt, seed=11, dtype="f32"):
    m = ka.Model(config(), dtype=dtype, seed=seed)
    m.compile(optimizer=opt, loss={h: ka.Tanimoto_dual_loss() for h in HEADS})
    return m


def test_checkpoint_continues_bit_for_bit(tmp_path, one_block_stem):
    mk = lambda: ka.Lamb(learning_rate=2e-3, beta_1=0.85, beta_2=0.99, epsilon=1e-6, weight_decay=0.02, clipnorm=0.5)
    m, whole = keras_model(mk()), keras_model(mk())
    for k in range(2):
        m.train_on_batch(*batch(360 + k))
    path = str(tmp_path / "lamb.h5")
    m.save(path)
    m2 = ka.load_model(path)
    o = m2.optimizer
    assert isinstance(o, ka.Lamb) and (o.kind, o.beta_1, o.beta_2, o.epsilon, o.weight_decay, o.clipnorm) == ("lamb", 0.85, 0.99, 1e-6, 0.02, 0.5)
    sp = m2.engine.loss
    assert (sp.optimizer, sp.lr, sp.beta_1, sp.beta_2, sp.epsilon) == ("lamb", 2e-3, 0.85, 0.99, 1e-6) and m2.engine.t == 2
    assert (bits_of(m2.engine.M1) == bits_of(m.engine.M1)).all() and (bits_of(m2.engine.V1) == bits_of(m.engine.V1)).all() and (m2.engine.V1 != 0).any()
    m2.train_on_batch(*batch(362))
    for k in range(3):
        whole.train_on_batch(*batch(360 + k))
    assert same(bits(m2.engine), bits(whole.engine)) and m2.engine.t == whole.engine.t == 3
    # an Adam file still loads as Adam
    plain = keras_model(ka.Adam(lr=1e-3), seed=5)
    plain.train_on_batch(*batch(370))
    p2 = str(tmp_path / "adam.h5")
    plain.save(p2)
    back = ka.load_model(p2)
    assert isinstance(back.optimizer, ka.Adam) and back.trust_report() is None and back.engine.loss.optimizer == "adam"


def test_trust_report_on_the_keras_surface():
    m = keras_model("lamb", dtype="bf16")
    assert isinstance(m.optimizer, ka.Lamb) and m.engine.loss.optimizer == "lamb"
    rep = m.trust_report()
    assert rep["updates"] == 0
    m.train_on_batch(*batch(380))
    rep = m.trust_report()
    assert sorted(rep) == ["forced", "max_ratio", "min_ratio", "ratios", "updates"]
    names = list(dict.fromkeys(e["name"] for e in m.engine.params.entries))
    assert list(rep["ratios"]) == names and any(nm.endswith("/kernel") for nm in names)
    vals = np.array(list(rep["ratios"].values()))
    assert rep["updates"] == 1 and rep["min_ratio"] == vals.min() and rep["max_ratio"] == vals.max() and 0 < rep["min_ratio"] < rep["max_ratio"]
    assert 0 <= rep["forced"] < len(names)
    for opt in (ka.Adam(lr=1e-3, global_clipnorm=1.0), ka.SGD(lr=1e-2, momentum=0.8)):
        other = keras_model(opt, dtype="bf16")
        other.train_on_batch(*batch(380))
        assert other.trust_report() is None


@pytest.mark.parametrize("dtype", DTYPES)
def test_dispatch_counts(dtype):
    """adam and sgd: the parent's count.  lamb: three launches where the segmented Adam is one - the chunk-table count + 2; with no clip, decay
    or skip option the sum of squares and the clip finisher are left out, which makes that the flat Adam count + 2."""
    x, y = batch(70)
    counts = {}
    for name, kw in (("adam", {}), ("sgd", dict(optimizer="sgd", momentum=0.8)), ("adam clip", dict(global_clipnorm=1.0)), ("lamb", dict(optimizer="lamb")),
                     ("lamb clip", dict(optimizer="lamb", global_clipnorm=1.0)), ("adam accum", dict(gradient_accumulation_steps=2)),
                     ("lamb accum", dict(optimizer="lamb", gradient_accumulation_steps=2))):
        eng = engine(dtype, **kw)
        eng.train_step(x, y)
        counts[name] = eng.count_step_dispatches(BATCH)
    print(f"{dtype} dispatches per step: {counts}")
    assert counts["adam"] == PARENT_DISPATCHES[dtype] == counts["sgd"]
    assert counts["adam clip"] == counts["adam"] + 2
    assert counts["lamb clip"] == counts["adam clip"] + 2 and counts["lamb"] == counts["adam"] + 2
    assert counts["lamb accum"] == counts["adam accum"] + 2
