"""Gradient accumulation through the engine and the Keras surface, on the configuration of tests/test_clip_engine_gpu.py (64 x 64 x 3 input,
4 classes, batch 2, width 32), in f32 and bf16: the whole-step HIP graph (warm-up, capture, replays) against a twin engine compiled without the
option whose gradients the host accumulates with accum.host_accumulate, the schedule and the moving average counting updates, the skip, the
report, the dispatch counts, the checkpoint in mid-cycle and the Keras surface.

Where two engines are compared bit for bit the step has to be a function of its inputs: rua_stem_bwd is pinned to one block and, in bf16,
stem_mfma is off on both sides, as tests/test_sched_engine_gpu.py explains.  The twin comparison also rests on a premise that is asserted
here: with the option off, train_step and forward_backward(_whole_step=True) + optimizer_step() agree bit for bit in this pinned configuration
(test_premise_...).  The twin takes the chunk-table route as well, through skip_nonfinite=True (its gradients are finite, so it never skips):
accumulation always walks the chunk table, and the segmented Adam is not the flat Adam bit for bit once the moments are non-zero - measured
here: with the flat kernel as the twin the first update agreed in every bit and the second did not -, a property of the two optimizer kernels
from before this feature (tests/test_clip_engine_gpu.py compares them under a bound) and not of the accumulation.

The single-rank data-parallel path: tests/test_accum_dp_gpu.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from _kernel_util import bits_of  # noqa: E402
from resunet_a_mltsk_keras_amd import _lib as L  # noqa: E402
from resunet_a_mltsk_keras_amd import accum as AC  # noqa: E402
from resunet_a_mltsk_keras_amd import keras_api as ka  # noqa: E402
from resunet_a_mltsk_keras_amd import schedules as SC  # noqa: E402
from resunet_a_mltsk_keras_amd.engine import HEADS, Engine, LossSpec, ModelConfig  # noqa: E402
from resunet_a_mltsk_keras_amd.synthetic import make_batch  # noqa: E402

f32 = np.float32
SHAPE, NCLS, BATCH = (64, 64, 3), 4, 2
# kernel nodes of the whole training step of this configuration with every optimizer option off: count_step_dispatches on the commit before
# the clip options, unchanged by them and by the schedules (PARENT_DISPATCHES of tests/test_clip_engine_gpu.py and tests/test_sched_engine_gpu.py)
PARENT_DISPATCHES = {"f32": 381, "bf16": 276}
# launches the option adds to the flat optimizer tail (rate kernel + optimizer): the gate, rua_accum_step, the sum of squares and the finisher
ACCUM_LAUNCHES = 4
DTYPES = ["f32", "bf16"]


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


@pytest.mark.parametrize("dtype", DTYPES)
def test_premise_graph_step_equals_the_eager_pieces_with_the_option_off(dtype, one_block_stem):
    a, b = engine(dtype, pinned=True), engine(dtype, pinned=True)
    for k in range(3):
        x, y = batch(200 + k)
        a.train_step(x, y, fetch=False)
        b.forward_backward(x, y, _whole_step=True)
        b.optimizer_step()
        assert same(bits(a, ("P", "M1", "V1", "S")), bits(b, ("P", "M1", "V1", "S"))), (dtype, k)


@pytest.mark.parametrize("dtype", DTYPES)
def test_graph_path_against_a_twin_accumulated_on_the_host(dtype, one_block_stem):
    """K = 3, seven micro-steps: warm-up and capture (1), replays (2 .. 7) - two full cycles and one hold."""
    k = 3
    eng, twin = engine(dtype, pinned=True, gradient_accumulation_steps=k), engine(dtype, pinned=True, skip_nonfinite=True)
    assert eng.use_graph and eng.dist is None and twin.A is None and eng.accumulation_state() == dict(steps=3, micro=0)
    assert twin.loss.gradient_accumulation_steps is None
    n = eng.params.n
    acc, micro = np.zeros(n, f32), 0
    watched, nw = ("P", "M1", "V1"), eng.params.nw
    for step in range(1, 8):
        x, y = batch(210 + step)
        before = bits(eng, watched)
        ra = eng.train_step(x, y)
        twin.forward_backward(x, y, _whole_step=True)
        torch.cuda.synchronize()
        g = twin.G[:n].cpu().numpy().copy()
        twin.G.zero_()
        acc, g_out, micro = AC.host_accumulate(acc, g, micro, k)
        assert np.all(np.isfinite(ra))
        if g_out is None:
            assert same(bits(eng, watched), before), (dtype, step)                 # a hold step: weights and moments keep their bits
        else:
            twin.G[:n].copy_(torch.from_numpy(g_out))
            twin.optimizer_step()
            assert same(bits(eng), bits(twin)), (dtype, step)
            assert not same(bits(eng), before)
            assert twin.clip_report()["skipped"] == 0
        if eng.opt_wcopy:                                                          # the forward copy holds bf16(P) behind a hold step as behind an update
            assert (bits_of(eng.Wf[:nw]) == bits_of(eng.P.cpu()[:nw].to(torch.bfloat16))).all(), (dtype, step)
        assert (bits_of(eng.S) == bits_of(twin.S)).all() and (bits_of(eng.A[:n]) == acc.view(np.uint32)).all(), (dtype, step)
        assert (eng.G[:n] == 0).all()                                              # the arena is zero when the next step begins
        assert eng.t == step // k and eng.accumulation_state() == dict(steps=k, micro=step % k)
        assert eng.lr_state.cpu().numpy()[0] == step // k and eng.acc_state.cpu().numpy()[0] == step % k
    assert BATCH in eng._captured and eng.t == 2 == twin.t and eng.accumulation_state() == dict(steps=3, micro=1)
    assert eng.clip_report() is None                                               # no clip option: nothing to report


@pytest.mark.parametrize("dtype", DTYPES)
def test_schedule_and_average_count_updates(dtype):
    """A table whose rate changes at update 1, K = 2, five micro-steps (updates behind batches 1 and 3): the rate of an update is host_lr at the
    UPDATE index - counted in batches, the first update (batch index 1) would already run at the second rate.  The average moves once per update."""
    sched = SC.PiecewiseConstantDecay([0], [2e-3, 5e-4])
    eng = engine(dtype, gradient_accumulation_steps=2, lr_schedule=sched, use_ema=True, ema_momentum=0.9, optimizer="sgd", momentum=0.8)
    E = eng.E.cpu().numpy().copy()
    updates = 0
    for step in range(5):
        assert eng.current_lr() == SC.host_lr(sched, updates)                      # the base rate of the NEXT update
        st0, lr0, E0 = eng.lr_state.cpu().numpy().copy(), bits_of(eng.lr_dev).copy(), bits_of(eng.E).copy()
        eng.train_step(*batch(230 + step), fetch=False)
        torch.cuda.synchronize()
        if step % 2 == 0:
            if step == 0:
                st0 = np.array([0.0, 2e-3])                                        # the host's first push: no update taken, the table's first rate
            assert (eng.lr_state.cpu().numpy() == st0).all() and (bits_of(eng.lr_dev) == lr0).all() and (bits_of(eng.E) == E0).all()
        else:
            updates += 1
            rate = SC.host_lr(sched, updates - 1)
            assert eng.lr_state.cpu().numpy().tolist() == [float(updates), rate]
            assert float(eng.lr_dev.cpu().numpy()[0]) == float(f32(rate))          # SGD: the rate itself
            E, _ = SC.host_ema(E, eng.P.cpu().numpy(), 0.9, updates)
            assert (bits_of(eng.E) == E.view(np.uint32)).all(), (dtype, step)
    assert updates == 2 == eng.t and SC.host_lr(sched, 0) == 2e-3 and SC.host_lr(sched, 1) == 5e-4
    with pytest.raises(RuntimeError):
        with eng.ema_weights():
            eng.train_step(*batch(239), fetch=False)


@pytest.mark.parametrize("poisoned", [2, 1], ids=["second", "first"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_eager_skip_of_a_poisoned_cycle(dtype, poisoned):
    eng = engine(dtype, gradient_accumulation_steps=2, skip_nonfinite=True, global_clipnorm=1.0)
    n = eng.params.n
    x, y = batch(240)
    before = bits(eng)
    e = eng.params.entries[len(eng.params.entries) // 2]
    S_mid = None
    for micro in (1, 2):
        eng.forward_backward(x, y)
        torch.cuda.synchronize()
        if micro == poisoned:
            eng.G[e["off"] + e["size"] - 1] = float("inf")
        if micro == 2:
            assert (bits_of(eng.S) != S_mid).any()                                 # the second forward folded its batch in
        eng.optimizer_step()
        torch.cuda.synchronize()
        if micro == 1:
            S_mid = bits_of(eng.S).copy()
            rep = eng.clip_report()
            assert rep["skipped"] == 0 and eng.t == 0 and same(bits(eng), before)
            assert bool(np.isinf(eng.A.cpu().numpy()).any()) == (poisoned == 1)
    rep = eng.clip_report()
    assert rep["skipped"] == 1 and rep["clipped"] == 0 and eng.t == 1               # the skipped update costs one t
    assert same(bits(eng), before)
    assert (bits_of(eng.A) == 0).all() and (eng.G.cpu().numpy()[:n] == 0).all()
    assert (bits_of(eng.S) == S_mid).all()                                         # only the last micro-step's fold is put back
    if eng.opt_wcopy:
        assert (bits_of(eng.Wf[:eng.params.nw]) == bits_of(eng.P.cpu()[:eng.params.nw].to(torch.bfloat16))).all()
    for micro in (1, 2):                                                           # the next, clean cycle moves the weights
        eng.forward_backward(x, y)
        eng.optimizer_step()
    rep = eng.clip_report()
    assert rep["skipped"] == 1 and eng.t == 2 and not same(bits(eng), before)
    for t in (eng.P, eng.M1, eng.V1, eng.S, eng.A):
        assert np.isfinite(t.cpu().numpy()).all()


def test_report_describes_the_last_update():
    eng = engine("f32", gradient_accumulation_steps=2, global_clipnorm=1e-3)
    reps = []
    for step in range(5):
        eng.train_step(*batch(250 + step), fetch=False)
        reps.append(eng.clip_report())
    assert reps[0] == dict(norm=0.0, min_coef=0.0, skipped=0, clipped=0)           # nothing has been reported yet
    assert reps[1]["clipped"] == 1 and reps[1]["norm"] > 1e-3 and reps[1]["min_coef"] == float(f32(1e-3 / reps[1]["norm"]))
    assert reps[2] == reps[1] and reps[4] == reps[3]                               # a hold step changes none of the four
    assert reps[3]["clipped"] == 2 and reps[3]["norm"] != reps[1]["norm"]


@pytest.mark.parametrize("dtype", DTYPES)
def test_dispatch_counts(dtype):
    x, y = batch(70)
    counts = {}
    for name, kw in (("off", {}), ("accum", dict(gradient_accumulation_steps=4)), ("clip", dict(global_clipnorm=1.0)),
                     ("accum+clip", dict(gradient_accumulation_steps=4, global_clipnorm=1.0)),
                     ("accum+all", dict(gradient_accumulation_steps=2, clipnorm=1.0, weight_decay=0.01, skip_nonfinite=True, use_ema=True))):
        eng = engine(dtype, **kw)
        eng.train_step(x, y)
        counts[name] = eng.count_step_dispatches(BATCH)
    print(f"{dtype} dispatches per step: {counts}")
    assert counts["off"] == PARENT_DISPATCHES[dtype]
    assert counts["accum"] == counts["off"] + ACCUM_LAUNCHES
    assert counts["accum+clip"] == counts["clip"] + 2 == counts["off"] + ACCUM_LAUNCHES
    assert counts["accum+all"] == counts["off"] + ACCUM_LAUNCHES + 3               # the state's backup and restore, the average


def test_option_off_is_the_parent_path_bit_for_bit(one_block_stem):
    res = []
    for kw in ({}, dict(gradient_accumulation_steps=None)):
        eng = engine("f32", **kw)
        assert eng.A is None and eng.acc_state is None and eng.clip is None and eng.accumulation_state() is None
        for seed in (80, 81):
            eng.train_step(*batch(seed))
        res.append(bits(eng, ("P", "M1", "V1", "S")))
    assert same(*res)


def test_recompile_drops_accumulator_and_counter():
    eng = engine("f32", gradient_accumulation_steps=3)
    eng.train_step(*batch(90), fetch=False)
    assert eng.accumulation_state() == dict(steps=3, micro=1) and (eng.A != 0).any()
    eng.compile(spec(gradient_accumulation_steps=2))
    assert eng.accumulation_state() == dict(steps=2, micro=0) and (eng.A == 0).all()
    eng.compile(spec())
    assert eng.A is None and eng.accumulation_state() is None
    with pytest.raises(ValueError):
        eng.compile(spec(gradient_accumulation_steps=1))


def keras_model(seed=11, **opt_kw):
    m = ka.Model(config(), dtype="f32", seed=seed)
    m.compile(optimizer=ka.Adam(lr=1e-3, **opt_kw), loss={h: ka.Tanimoto_dual_loss() for h in HEADS})
    return m


def test_checkpoint_in_mid_cycle_continues_bit_for_bit(tmp_path, one_block_stem):
    m, whole = keras_model(gradient_accumulation_steps=3), keras_model(gradient_accumulation_steps=3)
    for k in range(4):
        m.train_on_batch(*batch(260 + k))
    assert m.accumulation_state() == dict(steps=3, micro=1) and m.engine.t == 1
    path = str(tmp_path / "accum.h5")
    m.save(path)
    m2 = ka.load_model(path)
    assert m2.accumulation_state() == dict(steps=3, micro=1) and m2.engine.t == 1 and m2.optimizer.gradient_accumulation_steps == 3
    assert m2.engine.loss.accum_options() == dict(gradient_accumulation_steps=3)
    assert (bits_of(m2.engine.A) == bits_of(m.engine.A)).all() and (m2.engine.A != 0).any()
    for k in range(4, 6):
        m2.train_on_batch(*batch(260 + k))
    for k in range(6):
        whole.train_on_batch(*batch(260 + k))
    assert same(bits(m2.engine), bits(whole.engine)) and m2.engine.t == whole.engine.t == 2
    assert m2.accumulation_state() == whole.accumulation_state() == dict(steps=3, micro=0)
    # a file saved without the option loads and trains as before
    plain = keras_model(seed=5)
    x, y = batch(270)
    plain.train_on_batch(x, y)
    p2 = str(tmp_path / "plain.h5")
    plain.save(p2)
    back = ka.load_model(p2)
    assert back.accumulation_state() is None and back.engine.A is None and back.optimizer.gradient_accumulation_steps is None
    ra, rb = plain.train_on_batch(x, y), back.train_on_batch(x, y)
    assert list(ra) == list(rb) and same(bits(plain.engine), bits(back.engine)) and back.engine.t == 2


def test_keras_surface():
    x, y = batch(280)
    for opt in (ka.Adam(lr=1e-3, gradient_accumulation_steps=2), ka.SGD(lr=1e-2, momentum=0.8, gradient_accumulation_steps=2)):
        m = ka.Model(config(), dtype="bf16", seed=11)
        m.compile(optimizer=opt, loss={h: ka.Tanimoto_dual_loss() for h in HEADS})
        assert m.accumulation_state() == dict(steps=2, micro=0)
        before = bits(m.engine, ("P",))
        r1 = m.train_on_batch(x, y)
        assert same(bits(m.engine, ("P",)), before) and m.accumulation_state() == dict(steps=2, micro=1)
        r2 = m.train_on_batch(x, y)
        assert not same(bits(m.engine, ("P",)), before) and m.accumulation_state() == dict(steps=2, micro=0)
        assert np.all(np.isfinite(r1)) and np.all(np.isfinite(r2))
    with pytest.raises(ValueError):
        ka.Adam(gradient_accumulation_steps=1)
    plain = ka.Model(config(), dtype="bf16", seed=11)
    plain.compile(optimizer=ka.Adam(lr=1e-3), loss={h: ka.Tanimoto_dual_loss() for h in HEADS})
    assert plain.accumulation_state() is None
