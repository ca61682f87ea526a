"""Host side of the learning-rate schedules and the weights' moving average (no GPU): schedules.host_lr at points whose value follows from
the formula by hand, the validation of the options, host_ema's first-step and overwrite rules, and the checkpoint metadata through h5lite.
The formulas are Keras' as its documentation states them; no Keras is installed here to run against."""
import json
import os

import numpy as np
import pytest

from resunet_a_mltsk_keras_amd import h5lite
from resunet_a_mltsk_keras_amd import keras_api as ka
from resunet_a_mltsk_keras_amd import schedules as SC
from resunet_a_mltsk_keras_amd.engine import LossSpec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
f32 = np.float32


def test_struct_matches_the_header():
    import ctypes as C
    import re
    hdr = open(os.path.join(ROOT, "include", "rua_hip.h")).read()
    assert int(re.search(r"#define\s+RUA_SCHED_MAX_BOUNDARIES\s+(\d+)", hdr).group(1)) == SC.MAX_BOUNDARIES == 16
    for name, k in zip(SC.KIND_NAMES, range(6)):
        assert int(re.search(rf"#define\s+RUA_SCHED_{name.upper()}\s+(\d+)", hdr).group(1)) == k
    assert C.sizeof(SC.RuaLrSchedule) == 6 * 4 + 8 * 8 + 16 * 8 + 17 * 8


def test_cosine_without_warmup():
    s = SC.CosineDecay(0.5, 20, alpha=0.25)
    assert SC.host_lr(s, 0) == 0.5                                                 # cos 0 = 1: (1 - a) + a
    assert SC.host_lr(s, 10) == pytest.approx(0.5 * (0.75 * 0.5 + 0.25), rel=1e-15)   # cos(pi / 2) = 6e-17, not 0
    assert SC.host_lr(s, 20) == 0.5 * 0.25                                         # cos pi = -1 exactly
    assert SC.host_lr(s, 21) == SC.host_lr(s, 10 ** 6) == 0.125                    # clamped
    assert SC.host_lr(SC.CosineDecay(1.0, 4), 4) == 0.0 and s(10) == SC.host_lr(s, 10)


def test_cosine_with_warmup():
    s = SC.CosineDecay(0.0, 20, alpha=0.0, warmup_target=0.5, warmup_steps=5)
    assert [SC.host_lr(s, k) for k in range(5)] == [0.0, 0.5 * (1 / 5), 0.5 * (2 / 5), 0.5 * (3 / 5), 0.5 * (4 / 5)]
    assert SC.host_lr(s, 5) == 0.5                                                 # the first step after the warm-up: the target
    assert SC.host_lr(s, 15) == pytest.approx(0.25, rel=1e-15)
    assert SC.host_lr(s, 25) == 0.0 and SC.host_lr(s, 400) == 0.0
    s = SC.CosineDecay(0.125, 8, warmup_target=0.375, warmup_steps=4)
    assert SC.host_lr(s, 2) == 0.25 and SC.host_lr(s, 4) == 0.375
    assert SC.host_lr(SC.CosineDecay(0.125, 8, warmup_target=0.375, warmup_steps=0), 0) == 0.375


def test_exponential_and_inverse_time_staircase():
    e, es = SC.ExponentialDecay(1.0, 20, 0.5), SC.ExponentialDecay(1.0, 20, 0.5, staircase=True)
    assert SC.host_lr(e, 0) == 1.0 and SC.host_lr(e, 20) == 0.5 and SC.host_lr(e, 40) == 0.25
    assert SC.host_lr(e, 10) == pytest.approx(0.5 ** 0.5, rel=1e-15)
    assert SC.host_lr(es, 19) == 1.0 and SC.host_lr(es, 20) == 0.5 and SC.host_lr(es, 39) == 0.5 and SC.host_lr(es, 40) == 0.25
    i, is_ = SC.InverseTimeDecay(1.0, 20, 3.0), SC.InverseTimeDecay(1.0, 20, 3.0, staircase=True)
    assert SC.host_lr(i, 0) == 1.0 and SC.host_lr(i, 20) == 0.25 and SC.host_lr(i, 10) == 1.0 / 2.5
    assert SC.host_lr(is_, 19) == 1.0 and SC.host_lr(is_, 20) == 0.25 and SC.host_lr(is_, 40) == 1.0 / 7.0


def test_polynomial_clamped_and_cycled():
    p = SC.PolynomialDecay(1.0, 20, end_learning_rate=0.5, power=2.0)
    assert SC.host_lr(p, 0) == 1.0 and SC.host_lr(p, 10) == 0.5 * 0.25 + 0.5 and SC.host_lr(p, 20) == 0.5 and SC.host_lr(p, 99) == 0.5
    c = SC.PolynomialDecay(1.0, 20, end_learning_rate=0.5, power=1.0, cycle=True)
    assert SC.host_lr(c, 0) == 1.0 and SC.host_lr(c, 10) == 0.75
    assert SC.host_lr(c, 20) == 0.5                                                # ceil(20 / 20) = 1: the end of the first period
    assert SC.host_lr(c, 21) == 0.5 * (1.0 - 21 / 40) + 0.5                        # ceil(21 / 20) = 2: the period is now 40 steps
    assert SC.host_lr(c, 40) == 0.5 and SC.host_lr(c, 41) == 0.5 * (1.0 - 41 / 60) + 0.5
    assert SC.PolynomialDecay(1.0, 20).end_learning_rate == 1e-4


def test_piecewise_holds_a_value_up_to_and_including_its_boundary():
    p = SC.PiecewiseConstantDecay([2, 4, 9], [0.5, 0.25, 0.125, 0.0625])
    assert [SC.host_lr(p, k) for k in (0, 2, 3, 4, 5, 9, 10, 1000)] == [0.5, 0.5, 0.25, 0.25, 0.125, 0.125, 0.0625, 0.0625]
    assert SC.host_lr(SC.Constant(0.3), 17) == 0.3


def test_struct_carries_the_constants():
    st = SC.to_struct(SC.CosineDecay(0.125, 8, alpha=0.5, warmup_target=0.375, warmup_steps=4))
    assert (st.kind, st.warmup, st.initial, st.decay_steps, st.alpha, st.warmup_target, st.warmup_steps) == (SC.KIND_COSINE, 1, 0.125, 8.0, 0.5, 0.375, 4.0)
    assert SC.to_struct(SC.CosineDecay(0.125, 8)).warmup == 0
    st = SC.to_struct(SC.PiecewiseConstantDecay([2, 4], [3.0, 2.0, 1.0]))
    assert st.kind == SC.KIND_PIECEWISE and st.n_boundaries == 2 and list(st.boundaries)[:2] == [2.0, 4.0] and list(st.values)[:3] == [3.0, 2.0, 1.0]
    st = SC.to_struct(SC.PolynomialDecay(1.0, 20, 0.5, 2.0, cycle=True))
    assert (st.kind, st.cycle, st.end, st.power) == (SC.KIND_POLYNOMIAL, 1, 0.5, 2.0)
    st = SC.to_struct(SC.ExponentialDecay(1.0, 20, 0.5, staircase=True))
    assert (st.kind, st.staircase, st.decay_rate) == (SC.KIND_EXPONENTIAL, 1, 0.5)


def test_schedule_validation():
    for bad in (lambda: SC.CosineDecay(0.1, 0), lambda: SC.CosineDecay(0.1, 2.5), lambda: SC.CosineDecay(-0.1, 5), lambda: SC.CosineDecay(0.1, 5, warmup_steps=-1),
                lambda: SC.ExponentialDecay(0.1, 5, float("nan")), lambda: SC.PolynomialDecay(0.1, 5, power=0.0),
                lambda: SC.PiecewiseConstantDecay(list(range(17)), [0.1] * 18), lambda: SC.PiecewiseConstantDecay([3, 3], [0.1, 0.2, 0.3]),
                lambda: SC.PiecewiseConstantDecay([3], [0.1]), lambda: SC.PiecewiseConstantDecay([], [0.1]), lambda: SC.InverseTimeDecay(0.1, True, 0.5),
                lambda: SC.schedule_from_config(dict(kind="restarts")), lambda: SC.host_lr(SC.Constant(0.1), -1)):
        with pytest.raises(ValueError):
            bad()
    assert len(SC.PiecewiseConstantDecay(list(range(16)), [0.1] * 17).boundaries) == 16
    with pytest.raises(TypeError):
        SC.host_lr(0.1, 0)


@pytest.mark.parametrize("cls", [ka.Adam, ka.SGD])
def test_optimizer_arguments(cls):
    o = cls()
    assert o.sched_options() == dict(lr_schedule=None, use_ema=False, ema_momentum=0.99, ema_overwrite_frequency=None)
    for kw in (dict(ema_momentum=1.5), dict(ema_momentum=-0.1), dict(ema_momentum="0.9"), dict(ema_overwrite_frequency=0), dict(ema_overwrite_frequency=2.0),
               dict(ema_overwrite_frequency=True)):
        with pytest.raises(ValueError):
            cls(use_ema=True, **kw)
    o = cls(use_ema=True, ema_momentum=1, ema_overwrite_frequency=3)
    assert o.sched_options() == dict(lr_schedule=None, use_ema=True, ema_momentum=1.0, ema_overwrite_frequency=3)
    s = SC.CosineDecay(0.5, 20, warmup_target=1.0, warmup_steps=5)
    o = cls(learning_rate=s)
    assert o.lr_schedule is s and o.learning_rate is o.lr
    assert ka.K.get_value(o.lr) == 0.5                                             # no engine yet: step 0
    with pytest.raises(TypeError, match="not settable"):
        ka.K.set_value(o.lr, 0.1)
    c = cls(learning_rate=0.25)
    ka.K.set_value(c.lr, 0.125)
    assert ka.K.get_value(c.lr) == 0.125 and c.lr_schedule is None
    with pytest.raises(RuntimeError):
        o.finalize_variable_values()


def test_engine_compile_refuses_bad_options_before_anything_else():
    from resunet_a_mltsk_keras_amd.engine import Engine, ModelConfig
    eng = Engine(ModelConfig(input_shape=(64, 64, 3), num_classes=4), _layout_only=True)
    for kw in (dict(use_ema=True, ema_momentum=2.0), dict(use_ema=True, ema_overwrite_frequency=0), dict(lr_schedule=0.1)):
        with pytest.raises(ValueError):
            eng.compile(LossSpec(kind={"seg": 0}, weight={"seg": 1.0}, **kw))
    assert eng.loss is None


def test_host_ema_rules():
    e = np.array([1.0, -2.0, 0.5, 3.0], f32)
    th = np.array([0.1, 0.2, 0.3, 0.4], f32)
    e1, th1 = SC.host_ema(e, th, 0.9, 1)
    assert (e1 == th).all() and (th1 == th).all() and e1 is not th                 # the first step copies, whatever the average held
    e2, th2 = SC.host_ema(e, th, 0.9, 2)
    m = f32(0.9)
    want = np.array([f32(f32(m * a) + f32(f32(f32(1) - m) * b)) for a, b in zip(e, th)], f32)
    assert e2.dtype == f32 and (e2 == want).all() and (th2 == th).all()
    for t, over in ((2, False), (3, True), (4, False), (6, True)):
        e3, th3 = SC.host_ema(e, th, 0.9, t, overwrite_every=3)
        assert (e3 == want).all() and (th3 == (want if over else th)).all()
    e4, th4 = SC.host_ema(e, th, 0.9, 1, overwrite_every=1)
    assert (e4 == th).all() and (th4 == th).all()
    e5, th5 = SC.host_ema(e, th, 0.9, 3, overwrite_every=3, skipped=True)
    assert (e5 == e).all() and (th5 == th).all()
    assert (SC.host_ema(e, th, 1.0, 2)[0] == e).all() and (SC.host_ema(e, th, 0.0, 2)[0] == th).all()


SCHEDULES = [SC.CosineDecay(0.5, 20, alpha=0.25, warmup_target=1.0, warmup_steps=5), SC.CosineDecay(0.5, 20), SC.ExponentialDecay(1e-3, 7, 0.96, staircase=True),
             SC.PolynomialDecay(1e-3, 9, 1e-5, 0.5, cycle=True), SC.PiecewiseConstantDecay([2, 4, 9], [0.5, 0.25, 0.125, 0.0625]),
             SC.InverseTimeDecay(1e-2, 3, 0.5), SC.Constant(0.3)]


@pytest.mark.parametrize("sched", SCHEDULES, ids=lambda s: type(s).__name__)
def test_checkpoint_metadata_round_trip_through_h5lite(sched, tmp_path):
    sp = LossSpec(kind={"seg": 0}, weight={"seg": 1.0}, lr_schedule=sched, use_ema=True, ema_momentum=0.875, ema_overwrite_frequency=5)
    meta = dict(format="rua-checkpoint-2", loss=dict(kind=sp.kind, weight=sp.weight, optimizer=sp.optimizer, lr=sp.lr, **sp.clip_options(), **sp.sched_options()))
    root = h5lite.Group()
    root.attrs["rua_checkpoint"] = json.dumps(meta).encode("utf8")
    og = root.require_group("optimizer_weights")
    ema = np.arange(24, dtype=f32) / f32(7)
    og.set("rua/ema:0", ema)
    path = str(tmp_path / "sched.h5")
    h5lite.write_h5(path, root)
    back = h5lite.read_h5(path)
    raw = back.attrs["rua_checkpoint"]
    lo = json.loads(raw.decode("utf8") if isinstance(raw, bytes) else raw)["loss"]
    so = ka.loss_sched_options(lo)
    assert so == dict(lr_schedule=sched, use_ema=True, ema_momentum=0.875, ema_overwrite_frequency=5)
    assert type(so["lr_schedule"]) is type(sched)
    assert all(SC.host_lr(so["lr_schedule"], k) == SC.host_lr(sched, k) for k in range(48))
    assert "rua/ema:0" in back["optimizer_weights"] and (np.asarray(back["optimizer_weights"]["rua/ema:0"]) == ema).all()
    assert ka.loss_clip_options(lo) == sp.clip_options()


def test_files_from_before_the_options_load_with_both_off():
    g = h5lite.read_h5(os.path.join(GOLD, "keras_tiny.h5"))
    assert "rua_checkpoint" not in g.attrs                                         # a Keras file: weights only, compiled by the caller
    off = dict(lr_schedule=None, use_ema=False, ema_momentum=0.99, ema_overwrite_frequency=None)
    # a checkpoint of this package written before the options existed: the `loss` metadata has none of the keys
    old = dict(kind={"seg": 0}, weight={"seg": 1.0}, class_weights=None, optimizer="adam", lr=1e-3, beta_1=0.9, beta_2=0.999, momentum=0.0)
    assert ka.loss_sched_options(old) == off and ka.loss_sched_options(json.loads(json.dumps(old))) == off
    sp = LossSpec(kind=old["kind"], weight=old["weight"], **ka.loss_sched_options(old))
    assert sp.lr_schedule is None and not sp.use_ema and sp.sched_options() == off
    assert "rua/ema:0" not in g["optimizer_weights"]
