"""Host side of gradient accumulation (no GPU): accum.check_steps, accum.host_accumulate against an fp32 loop written out here, the optimizer
classes' argument, train_ISPRS.py's flag and the checkpoint metadata.  The semantics are this project's definition of Keras 3's
gradient_accumulation_steps (accum.py); no Keras is installed here to run against."""
import json
import os

import numpy as np
import pytest

from resunet_a_mltsk_keras_amd import accum as AC
from resunet_a_mltsk_keras_amd import h5lite
from resunet_a_mltsk_keras_amd import keras_api as ka
from resunet_a_mltsk_keras_amd.engine import LossSpec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def test_check_steps():
    assert AC.check_steps(None) is None
    for k in (2, 3, 64, np.int64(5)):
        v = AC.check_steps(k)
        assert v == k and type(v) is int
    for bad in (True, False, 2.0, 0, 1, -1, -4, "2", (1 << 24) + 1):
        with pytest.raises(ValueError):
            AC.check_steps(bad)


def gradients(k, cycles, n=37, seed=0):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal(n) * 10.0 ** rng.integers(-6, 4, n)).astype(f32) for _ in range(k * cycles)]


@pytest.mark.parametrize("k", [2, 3, 5])
def test_host_accumulate_is_the_written_out_loop(k):
    gs = gradients(k, 3, seed=k)
    n = gs[0].size
    a, micro = np.zeros(n, f32), 0
    for c in range(3):
        for j in range(k):
            g = gs[c * k + j]
            # the loop, element by element, every operation rounded on its own in fp32
            acc = [f32(0)] * n
            for q in range(j):
                acc = [f32(acc[i] + gs[c * k + q][i]) for i in range(n)]
            assert all(a[i] == acc[i] for i in range(n)) and micro == j
            a2, out, micro2 = AC.host_accumulate(a, g, micro, k)
            assert a2.dtype == f32 and a2 is not a
            if j + 1 < k:
                assert out is None and micro2 == j + 1
                assert all(a2[i] == f32(acc[i] + g[i]) for i in range(n))
            else:
                assert micro2 == 0 and out.dtype == f32 and (a2 == 0).all() and not np.signbit(a2).any()
                assert all(out[i] == f32(f32(g[i] + acc[i]) / f32(k)) for i in range(n))
            a, micro = a2, micro2


def test_division_is_not_a_product_with_the_reciprocal():
    """K = 3: x / 3 and x * fl(1 / 3) differ in the last bit for many x; the inputs below hold such x, so a kernel that multiplied would be told apart."""
    g = np.arange(1, 65, dtype=f32)
    a = np.zeros(64, f32)
    for m in (0, 1):
        a, out, _ = AC.host_accumulate(a, np.zeros(64, f32), m, 3)
    _, out, _ = AC.host_accumulate(a, g, 2, 3)
    recip = (g * f32(f32(1) / f32(3))).astype(f32)
    assert (out == (g / f32(3))).all()
    assert (out != recip).any(), "the chosen inputs do not tell a division from a reciprocal multiply"
    assert int((out != recip).sum()) >= 8


def test_non_finite_values_propagate_and_the_update_resets():
    inf, nan = f32(np.inf), f32(np.nan)
    g1 = np.array([1.0, inf, -inf, nan, 2.0, 0.0], f32)
    g2 = np.array([1.0, 1.0, inf, 1.0, -inf, -0.0], f32)
    a, out, m = AC.host_accumulate(np.zeros(6, f32), g1, 0, 2)
    assert out is None and m == 1
    assert a[0] == 1 and a[1] == inf and a[2] == -inf and np.isnan(a[3]) and a[4] == 2
    a2, out, m = AC.host_accumulate(a, g2, 1, 2)
    assert m == 0 and (a2 == 0).all()
    assert out[0] == 1 and out[1] == inf and np.isnan(out[2]) and np.isnan(out[3]) and out[4] == -inf and out[5] == 0
    with pytest.raises(ValueError):
        AC.host_accumulate(a, g2, 2, 2)
    with pytest.raises(ValueError):
        AC.host_accumulate(a, g2[:3], 0, 2)
    with pytest.raises(ValueError):
        AC.host_accumulate(a, g2, 0, 1)


@pytest.mark.parametrize("cls", [ka.Adam, ka.SGD])
def test_optimizer_argument(cls):
    assert cls().accum_options() == dict(gradient_accumulation_steps=None)
    o = cls(gradient_accumulation_steps=4, global_clipnorm=1.0)
    assert o.gradient_accumulation_steps == 4 and o.accum_options() == dict(gradient_accumulation_steps=4)
    sp = LossSpec(kind={"seg": 0}, weight={"seg": 1.0}, **o.clip_options(), **o.sched_options(), **o.accum_options())
    assert sp.gradient_accumulation_steps == 4 and sp.global_clipnorm == 1.0 and sp.accum_options() == o.accum_options()
    assert LossSpec(kind={"seg": 0}, weight={"seg": 1.0}).gradient_accumulation_steps is None
    for bad in (1, 0, -2, 2.0, True):
        with pytest.raises(ValueError):
            cls(gradient_accumulation_steps=bad)


def test_engine_compile_refuses_a_bad_step_count():
    from resunet_a_mltsk_keras_amd.engine import Engine, ModelConfig
    eng = Engine(ModelConfig(input_shape=(64, 64, 3), num_classes=4), _layout_only=True)
    for bad in (1, 0, 2.5, True):
        with pytest.raises(ValueError):
            eng.compile(LossSpec(kind={"seg": 0}, weight={"seg": 1.0}, gradient_accumulation_steps=bad))
    assert eng.loss is None


def test_train_script_flag():
    import train_ISPRS as T
    p = T.build_parser()
    assert p.parse_args([]).grad_accum == 1 and T.accum_options(p.parse_args([])) == dict(gradient_accumulation_steps=None)
    assert T.accum_options(p.parse_args(["--grad_accum", "1"])) == dict(gradient_accumulation_steps=None)
    assert T.accum_options(p.parse_args(["--grad_accum", "4"])) == dict(gradient_accumulation_steps=4)
    with pytest.raises(SystemExit):
        T.accum_options(p.parse_args(["--grad_accum", "0"]))
    helps = {a.dest: a.help for a in p._actions}
    for dest in ("lr_decay_steps", "lr_warmup_steps", "ema_overwrite_frequency"):
        assert "updates, not batches" in helps[dest]


def test_checkpoint_metadata_round_trip_and_old_files(tmp_path):
    sp = LossSpec(kind={"seg": 0}, weight={"seg": 1.0}, gradient_accumulation_steps=3, skip_nonfinite=True)
    meta = dict(loss=dict(kind=sp.kind, weight=sp.weight, optimizer=sp.optimizer, lr=sp.lr, **sp.clip_options(), **sp.sched_options(), **sp.accum_options()))
    root = h5lite.Group()
    root.attrs["rua_checkpoint"] = json.dumps(meta).encode("utf8")
    og = root.require_group("optimizer_weights")
    acc = np.arange(24, dtype=f32) / f32(7)
    og.set("rua/accum:0", acc); og.set("rua/accum_micro:0", np.array(2, np.int64))
    path = str(tmp_path / "accum.h5")
    h5lite.write_h5(path, root)
    back = h5lite.read_h5(path)
    raw = back.attrs["rua_checkpoint"]
    lo = json.loads(raw.decode("utf8") if isinstance(raw, bytes) else raw)["loss"]
    assert ka.loss_accum_options(lo) == dict(gradient_accumulation_steps=3) == sp.accum_options()
    assert ka.loss_clip_options(lo) == sp.clip_options()
    assert (np.asarray(back["optimizer_weights"]["rua/accum:0"]) == acc).all() and int(back["optimizer_weights"]["rua/accum_micro:0"]) == 2
    # a checkpoint written before the option existed: the `loss` metadata has no such key
    old = dict(kind={"seg": 0}, weight={"seg": 1.0}, class_weights=None, optimizer="adam", lr=1e-3, beta_1=0.9, beta_2=0.999, momentum=0.0)
    assert ka.loss_accum_options(old) == ka.loss_accum_options(json.loads(json.dumps(old))) == dict(gradient_accumulation_steps=None)
    assert LossSpec(kind=old["kind"], weight=old["weight"], **ka.loss_accum_options(old)).gradient_accumulation_steps is None
