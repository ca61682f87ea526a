"""Learning-rate schedules and the weights' moving average through the engine and the Keras surface, on the configuration of
tests/test_clip_engine_gpu.py (64 x 64 x 3 input, 4 classes, batch 2, width 32), in f32 and bf16: the whole-step HIP graph (warm-up, capture,
replays) against a twin engine whose constant rate the host sets before every step, the rate read back, weight decay under a schedule,
the average against schedules.host_ema on the weights read back, the skip, ema_weights(), the dispatch counts, the default path's bits and
the checkpoint.

Where two engines are compared bit for bit the step has to be a function of its inputs, and the stem's weight gradient is the one place
where it is not: rua_stem_bwd is pinned to one block, as tests/test_clip_engine_gpu.py and tests/test_scene_photo_gpu.py pin it (its blocks
end in float atomics), and in bf16 the engine switch stem_mfma is off on both sides, which sends the stem's weight gradient through that
kernel too (its default bf16 route ends in float atomics as well: conv2d/kernel and conv2d/bias, and nothing else, differ between two runs
of the unchanged step).  Everything behind the gradient - the rate kernel, the optimizer, the average - is what the comparison is about.

The weight-decay test uses test_clip_engine_gpu.py's first-step bound (m = v = 0, u = 2^-23, K = 2) with the scheduled rate in the place of the
base rate:  |th' - th'_ref| <= u |th'_ref| + E_dec + (4e-6 + K u) |delta_ref| + lr_t e_m / (sqrt(v'_ref) + eps),  e_m = (4 + K) u (1 - beta1) |gg|."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from _kernel_util import U32, bits_of, worst_ratio  # noqa: E402
from resunet_a_mltsk_keras_amd import _lib as L  # noqa: E402
from resunet_a_mltsk_keras_amd import clip as CL  # noqa: E402
from resunet_a_mltsk_keras_amd import keras_api as ka  # noqa: E402
from resunet_a_mltsk_keras_amd import schedules as SC  # noqa: E402
from resunet_a_mltsk_keras_amd.engine import HEADS, KERAS_EPS, Engine, LossSpec, ModelConfig  # noqa: E402
from resunet_a_mltsk_keras_amd.synthetic import make_batch  # noqa: E402

f32, f64 = np.float32, np.float64
SHAPE, NCLS, BATCH = (64, 64, 3), 4, 2
K = 2
# kernel nodes of the whole training step of this configuration before the clip options and before this feature (tests/test_clip_engine_gpu.py)
PARENT_DISPATCHES = {"f32": 381, "bf16": 276}
DTYPES = ["f32", "bf16"]
PIECEWISE = SC.PiecewiseConstantDecay([0, 2, 3], [2e-3, 5e-4, 1.5e-3, 2.5e-4])    # changes in front of steps 2, 4 and 5: warm-up, capture and replays all see one
COSINE = SC.CosineDecay(1e-4, 4, alpha=0.1, warmup_target=2e-3, warmup_steps=2)


def spec(**kw):
    return LossSpec(kind={h: L.LOSS_TANIMOTO for h in HEADS}, weight={"seg": 1.0, "bound": 0.7, "dist": 1.3, "color": 0.5}, lr=1e-3, **kw)


def config():
    return ModelConfig(input_shape=SHAPE, num_classes=NCLS, multitasking=True, width=32)


def engine(dtype, pinned=False, **kw):
    """pinned (with the one_block_stem fixture): a step that gives the same bits on every run, for the twin comparisons."""
    eng = Engine(config(), dtype=dtype, seed=4, split_k=False)
    if pinned:
        eng.stem_mfma = False
    eng.compile(spec(**kw))
    return eng


def batch(seed):
    return make_batch(BATCH, SHAPE[0], SHAPE[2], NCLS, True, seed=seed, block=16)


def state_bits(eng):
    torch.cuda.synchronize()
    return [bits_of(t).copy() for t in (eng.P, eng.M1, eng.V1, eng.S)]


def same(a, b):
    return all((x == y).all() for x, y in zip(a, b))


@pytest.fixture
def one_block_stem():
    lib = L.lib()
    before = lib.get_tuning("stem_blocks")
    lib.set_tuning(stem_blocks=1)
    yield
    lib.set_tuning(stem_blocks=before)


@pytest.mark.parametrize("dtype", DTYPES)
def test_schedule_through_the_graph_equals_a_host_set_rate(dtype, one_block_stem):
    """Six steps under a table schedule: warm-up and capture (1), replays (2 .. 6).  The twin has a constant rate which the host sets to
    host_lr(t) in front of every step (a host-to-device copy of lr_state each time): table look-ups are exact, so the bits agree."""
    a, b = engine(dtype, pinned=True, lr_schedule=PIECEWISE), engine(dtype, pinned=True)
    assert a.use_graph and a.dist is None
    rates = []
    for k in range(6):
        x, y = batch(100 + k)
        assert a.current_lr() == SC.host_lr(PIECEWISE, k)
        b.loss.lr = SC.host_lr(PIECEWISE, k)
        rates.append(b.loss.lr)
        ra, rb = a.train_step(x, y), b.train_step(x, y)
        assert np.all(np.isfinite(ra)) and list(ra) == list(rb)
        sa, sb = state_bits(a), state_bits(b)
        assert same(sa, sb), (dtype, k)
        assert (bits_of(a.lr_dev[:1]) == bits_of(b.lr_dev[:1])).all() and a.lr_state.cpu().numpy().tolist() == [k + 1.0, rates[-1]]
    assert BATCH in a._captured and a.t == 6 and len(set(rates)) == 4
    assert a._lr_base_dev is None                                                  # nothing but the counter was ever pushed


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("opt", ["adam", "sgd"])
def test_cosine_with_warm_up_read_back_after_every_step(dtype, opt):
    eng = engine(dtype, lr_schedule=COSINE, optimizer=opt)
    b1, b2 = f64(eng.loss.beta_1), f64(eng.loss.beta_2)
    x, y = batch(110)
    worst = 0.0
    for k in range(6):
        eng.train_step(x, y, fetch=False)
        torch.cuda.synchronize()
        t = k + 1
        rate = SC.host_lr(COSINE, k)
        host = rate * (np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t) if opt == "adam" else 1.0)
        got = float(eng.lr_dev.cpu().numpy()[0])
        bound = float(np.spacing(f32(host))) + 2.0 ** -40 * COSINE.max_rate()
        worst = max(worst, abs(got - float(f32(host))) / bound)
        assert abs(got - float(f32(host))) <= bound, (k, got, host)
        st = eng.lr_state.cpu().numpy()
        assert st[0] == t and abs(st[1] - rate) <= 2.0 ** -40 * COSINE.max_rate()
    print(f"{dtype} {opt} cosine with warm-up through the graph: worst ratio to the bound {worst:.3f}")
    assert eng.current_lr() == SC.host_lr(COSINE, 6) == 2e-3 * 0.1                 # the tail: alpha * warmup_target


@pytest.mark.parametrize("dtype", DTYPES)
def test_weight_decay_follows_the_schedule(dtype):
    sched = SC.ExponentialDecay(2e-3, 20, 0.5)                                     # 2e-3 in front of the first step; the spec's lr (1e-3) must not show
    wd, rate = 0.05, 2e-3
    eng = engine(dtype, lr_schedule=sched, weight_decay=wd, decay_exclude=list(CL.DEFAULT_DECAY_EXCLUDE))
    x, y = batch(40)
    eng.forward_backward(x, y)
    torch.cuda.synchronize()
    G, P0 = eng.G.cpu().numpy().copy(), eng.P.cpu().numpy().copy()
    eng.optimizer_step()
    torch.cuda.synchronize()
    ps = eng.params
    n = ps.n
    chunks, vars_, _ = CL.build_chunk_table(ps.entries, eng.loss.decay_exclude)
    b1, b2, eps = f64(f32(0.9)), f64(f32(0.999)), f64(f32(KERAS_EPS))
    lr1 = f64(f32(rate * np.sqrt(1.0 - 0.999 ** 1) / (1.0 - 0.9 ** 1)))
    assert abs(float(eng.lr_dev.cpu().numpy()[0]) - float(lr1)) <= float(np.spacing(f32(lr1)))
    z = np.zeros(n)
    ref = CL.host_clipped_step(P0[:n], G[:n], z, z, chunks, vars_, optimizer="adam", lr=lr1, lr_base=rate, beta_1=b1, beta_2=b2, eps=eps, grad_scale=1.0,
                               weight_decay=wd)
    ins = CL.covered(chunks, n) == 1
    gg, th1, th_ref = ref["gg"][ins], ref["th1"][ins], ref["theta"][ins]
    den = np.sqrt(ref["v"][ins]) + eps
    delta = lr1 * ref["m"][ins] / den
    e_m = (4 + K) * U32 * (1 - b1) * np.abs(gg)
    d = f64(f32(wd * rate))
    decays = np.zeros(n, bool)
    for off, ln, var in chunks.tolist():
        decays[off:off + ln] = bool(vars_["decay"][var])
    e_dec = np.where(decays[ins], U32 * np.abs(P0[:n][ins].astype(f64) * d) + U32 * np.abs(th1), 0.0)
    e_th = U32 * np.abs(th_ref) + e_dec + (4e-6 + K * U32) * np.abs(delta) + lr1 * e_m / den
    got = eng.P.cpu().numpy()[:n]
    r = worst_ratio(np.abs(got[ins].astype(f64) - th_ref), e_th)
    # the same step decayed with the spec's constant 1e-3 instead is far outside the bound: the test can tell the two apart
    other = CL.host_clipped_step(P0[:n], G[:n], z, z, chunks, vars_, optimizer="adam", lr=lr1, lr_base=1e-3, beta_1=b1, beta_2=b2, eps=eps, grad_scale=1.0,
                                 weight_decay=wd)["theta"][ins]
    r_other = worst_ratio(np.abs(other - th_ref), e_th)
    print(f"{dtype} weight decay under a schedule: theta ratio to the bound {r:.3f} (decayed at the spec's lr instead: {r_other:.3g})")
    assert decays.any() and r_other > 10.0
    assert r <= 1.0
    assert (got[~ins] == 0).all()
    assert eng.lr_state.cpu().numpy().tolist() == [1.0, rate]
    if eng.opt_wcopy:
        assert (bits_of(eng.Wf[:ps.nw]) == bits_of(eng.P.cpu()[:ps.nw].to(torch.bfloat16))).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_ema_through_the_graph(dtype):
    eng = engine(dtype, use_ema=True, ema_momentum=0.9)
    n = eng.params.n
    assert (bits_of(eng.E) == bits_of(eng.P)).all()                                # compile(): a copy of P
    E = eng.E.cpu().numpy().copy()
    for k in range(5):
        eng.train_step(*batch(120 + k), fetch=False)
        torch.cuda.synchronize()
        P = eng.P.cpu().numpy()
        E, _ = SC.host_ema(E, P, 0.9, k + 1)
        assert (bits_of(eng.E) == E.view(np.uint32)).all(), (dtype, k)
        if k:
            assert (E[:n] != P[:n]).any()
        assert (E[n:] == 0).all()                                                  # padding stays zero
    assert BATCH in eng._captured


@pytest.mark.parametrize("dtype", DTYPES)
def test_ema_overwrite_through_the_graph(dtype):
    eng = engine(dtype, use_ema=True, ema_momentum=0.9, ema_overwrite_frequency=2)
    ps = eng.params
    for k in range(5):
        E_prev = eng.E.cpu().numpy().copy()
        eng.train_step(*batch(130 + k), fetch=False)
        torch.cuda.synchronize()
        t = k + 1
        if t % 2 == 0:
            assert (bits_of(eng.P) == bits_of(eng.E)).all(), (dtype, t)
            assert (bits_of(eng.E) != E_prev.view(np.uint32)).any()
        else:
            E, _ = SC.host_ema(E_prev, eng.P.cpu().numpy(), 0.9, t)
            assert (bits_of(eng.E) == E.view(np.uint32)).all(), (dtype, t)
            assert t == 1 or (bits_of(eng.P) != bits_of(eng.E)).any()
        if eng.opt_wcopy:
            assert (bits_of(eng.Wf[:ps.nw]) == bits_of(eng.P.cpu()[:ps.nw].to(torch.bfloat16))).all(), (dtype, t)
    assert np.isfinite(eng.P.cpu().numpy()).all()


@pytest.mark.parametrize("dtype,opt", [("f32", "adam"), ("bf16", "adam"), ("bf16", "sgd")])
def test_eager_skip_keeps_the_average(dtype, opt):
    eng = engine(dtype, optimizer=opt, momentum=0.8, skip_nonfinite=True, use_ema=True, ema_momentum=0.9, ema_overwrite_frequency=2)
    x, y = batch(60)
    eng.forward_backward(x, y)
    eng.optimizer_step()                                                           # a clean step: t = 1, E = P
    torch.cuda.synchronize()
    assert eng.clip_report()["skipped"] == 0 and (bits_of(eng.E) == bits_of(eng.P)).all()
    before = [bits_of(t).copy() for t in (eng.P, eng.E, eng.M1)]
    eng.forward_backward(x, y)
    torch.cuda.synchronize()
    e = eng.params.entries[len(eng.params.entries) // 2]
    eng.G[e["off"] + e["size"] - 1] = float("inf")                                 # as tests/test_clip_engine_gpu.py poisons it
    eng.optimizer_step()                                                           # t = 2: an overwrite step, had it not been skipped
    assert eng.clip_report()["skipped"] == 1 and eng.t == 2
    for t, b in zip((eng.P, eng.E, eng.M1), before):
        assert (bits_of(t) == b).all()
    eng.forward_backward(x, y)
    eng.optimizer_step()                                                           # t = 3, clean: the average moves again
    torch.cuda.synchronize()
    E, _ = SC.host_ema(before[1].view(f32), eng.P.cpu().numpy(), 0.9, 3)
    assert eng.clip_report()["skipped"] == 1 and (bits_of(eng.E) == E.view(np.uint32)).all() and (bits_of(eng.E) != before[1]).any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_ema_weights_block(dtype, one_block_stem):
    def model():
        m = ka.Model(config(), dtype=dtype, seed=11)
        m.engine.stem_mfma = False                                                 # with one_block_stem: the same bits on every run
        m.compile(optimizer=ka.Adam(lr=2e-3, use_ema=True, ema_momentum=0.5), loss={h: ka.Tanimoto_dual_loss() for h in HEADS})
        return m
    m, twin = model(), model()
    batches = [batch(140 + k) for k in range(5)]
    for x, y in batches[:3]:
        m.train_on_batch(x, y); twin.train_on_batch(x, y)
    e = m.engine
    torch.cuda.synchronize()
    P_bits, E_bits = bits_of(e.P).copy(), bits_of(e.E).copy()
    assert (P_bits != E_bits).any()
    x = batches[0][0]
    plain = m.predict(x, batch_size=BATCH)
    with m.ema_weights():
        assert (bits_of(e.P) == E_bits).all() and (bits_of(e.E) == P_bits).all()
        inside = m.predict(x, batch_size=BATCH)
        with pytest.raises(RuntimeError, match="ema_weights"):
            m.train_on_batch(*batches[3])
        with pytest.raises(RuntimeError):
            m.finalize_ema()
    torch.cuda.synchronize()
    assert (bits_of(e.P) == P_bits).all() and (bits_of(e.E) == E_bits).all() and e.t == 3
    other = ka.Model(config(), dtype=dtype, seed=3)
    other.set_weights_dict(e.params.to_keras(E_bits.view(f32), e.S.cpu().numpy()))
    ref = other.predict(x, batch_size=BATCH)
    for h in HEADS:
        assert (inside[h].view(np.uint32) == ref[h].view(np.uint32)).all(), h
    assert any((inside[h] != plain[h]).any() for h in HEADS)
    again = m.predict(x, batch_size=BATCH)
    for h in HEADS:
        assert (again[h].view(np.uint32) == plain[h].view(np.uint32)).all(), h
    for x, y in batches[3:]:
        ra, rb = m.train_on_batch(x, y), twin.train_on_batch(x, y)
        assert list(ra) == list(rb)
    assert same(state_bits(e), state_bits(twin.engine)) and (bits_of(e.E) == bits_of(twin.engine.E)).all()
    m.optimizer.finalize_variable_values()
    assert (bits_of(e.P) == bits_of(e.E)).all() and (bits_of(e.P) == bits_of(twin.engine.E)).all()
    plain_model = ka.Model(config(), dtype=dtype, seed=11)
    plain_model.compile(optimizer=ka.Adam(lr=2e-3), loss={h: ka.Tanimoto_dual_loss() for h in HEADS})
    with pytest.raises(RuntimeError, match="use_ema"):
        plain_model.ema_weights().__enter__()


@pytest.mark.parametrize("dtype", DTYPES)
def test_dispatch_counts(dtype):
    """Options off: the parent's count.  The schedule's rate kernel takes the constant one's place; the average is one more kernel."""
    x, y = batch(70)
    counts = {}
    for name, kw in (("off", {}), ("schedule", dict(lr_schedule=COSINE)), ("ema", dict(use_ema=True)),
                     ("both", dict(lr_schedule=PIECEWISE, use_ema=True, ema_overwrite_frequency=3))):
        eng = engine(dtype, **kw)
        eng.train_step(x, y)
        counts[name] = eng.count_step_dispatches(BATCH)
    print(f"{dtype} dispatches per step: {counts}")
    assert counts["off"] == PARENT_DISPATCHES[dtype]
    assert counts["schedule"] == counts["off"]
    assert counts["ema"] == counts["off"] + 1 and counts["both"] == counts["off"] + 1


def test_options_off_is_the_parent_path_bit_for_bit(one_block_stem):
    res = []
    for kw in ({}, dict(lr_schedule=None, use_ema=False, ema_momentum=0.99, ema_overwrite_frequency=None)):
        eng = engine("f32", **kw)
        assert eng.E is None and eng._sched is None
        for seed in (80, 81):
            eng.train_step(*batch(seed))
        res.append(state_bits(eng))
        assert eng.lr_state.numel() == 2 and eng._lr_base_dev == 1e-3
    assert same(*res)


def test_checkpoint_restores_schedule_average_and_counter(tmp_path, one_block_stem):
    sched = SC.CosineDecay(1e-4, 6, alpha=0.1, warmup_target=2e-3, warmup_steps=2)
    m = ka.Model(config(), dtype="f32", seed=11)
    opt = ka.Adam(learning_rate=sched, use_ema=True, ema_momentum=0.75, ema_overwrite_frequency=7)
    m.compile(optimizer=opt, loss={h: ka.Tanimoto_dual_loss() for h in HEADS})
    assert ka.K.get_value(m.optimizer.lr) == 1e-4
    for k in range(3):
        m.train_on_batch(*batch(150 + k))
    assert ka.K.get_value(m.optimizer.lr) == SC.host_lr(sched, 3)
    with pytest.raises(TypeError, match="not settable"):
        ka.K.set_value(m.optimizer.lr, 1e-3)
    path = str(tmp_path / "sched.h5")
    m.save(path)
    m2 = ka.load_model(path)
    e, e2 = m.engine, m2.engine
    assert e2.t == 3 and e2.loss.sched_options() == e.loss.sched_options() == dict(
        lr_schedule=sched.get_config(), use_ema=True, ema_momentum=0.75, ema_overwrite_frequency=7)
    assert m2.optimizer.lr_schedule == sched and m2.optimizer.use_ema and m2.optimizer.ema_momentum == 0.75 and m2.optimizer.ema_overwrite_frequency == 7
    assert ka.K.get_value(m2.optimizer.lr) == SC.host_lr(sched, 3)
    assert (bits_of(e2.E) == bits_of(e.E)).all() and (bits_of(e2.P) == bits_of(e.P)).all() and (bits_of(e2.E) != bits_of(e2.P)).any()
    x, y = batch(160)
    ra, rb = m.train_on_batch(x, y), m2.train_on_batch(x, y)                       # the uninterrupted twin replays its graph, the loaded model warms up
    assert list(ra) == list(rb)
    assert same(state_bits(e), state_bits(e2)) and (bits_of(e.E) == bits_of(e2.E)).all()
    assert (bits_of(e.lr_dev[:1]) == bits_of(e2.lr_dev[:1])).all() and e2.lr_state.cpu().numpy()[0] == 4.0
    # a file without an average (saved by a model without use_ema), loaded and compiled with one: E starts as a copy of P
    plain = ka.Model(config(), dtype="f32", seed=5)
    plain.compile(optimizer=ka.Adam(lr=1e-3), loss={h: ka.Tanimoto_dual_loss() for h in HEADS})
    plain.train_on_batch(x, y)
    p2 = str(tmp_path / "plain.h5")
    plain.save(p2)
    back = ka.load_model(p2)
    assert back.engine.E is None and back.engine.loss.lr_schedule is None and back.optimizer.lr_schedule is None
    back.compile(optimizer=ka.Adam(lr=1e-3, use_ema=True), loss={h: ka.Tanimoto_dual_loss() for h in HEADS})
    assert (bits_of(back.engine.E) == bits_of(back.engine.P)).all()
