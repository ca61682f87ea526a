"""Host side of gradient clipping, decoupled weight decay and the non-finite step skip: clip.py's chunk-table builder and float64 step, the
optimizers' argument checks, and the options' way through LossSpec and the checkpoint metadata.  No GPU."""
import json
import os
import re

import numpy as np
import pytest

from resunet_a_mltsk_keras_amd import clip as CL
from resunet_a_mltsk_keras_amd.engine import LossSpec, ParamStore
from resunet_a_mltsk_keras_amd.keras_api import SGD, Adam, loss_clip_options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CH = CL.OPT_CHUNK


def store():
    """A two-segment 3x3 convolution (its first segment longer than two chunks), its bias, and a BatchNorm."""
    ps = ParamStore()
    ps.conv([200, 7], 10, 9, name="conv2d")
    ps.bn(10)
    return ps


def test_chunk_constant_is_the_header_s():
    hdr = open(os.path.join(ROOT, "include", "rua_hip.h")).read()
    assert int(re.search(r"#define\s+RUA_OPT_CHUNK\s+(\d+)", hdr).group(1)) == CH
    assert CH % 16 == 0 and CL.CHUNK_DTYPE.itemsize == 16 and CL.VAR_DTYPE.itemsize == 16
    modes = {k: int(v) for k, v in re.findall(r"#define\s+RUA_CLIP_(\w+)\s+(\d+)", hdr)}
    assert modes == dict(NONE=CL.CLIP_NONE, GLOBAL_NORM=CL.CLIP_GLOBAL_NORM, NORM=CL.CLIP_NORM, VALUE=CL.CLIP_VALUE)


def test_table_covers_every_entry_element_once_and_no_padding():
    ps = store()
    chunks, vars_, names = CL.build_chunk_table(ps.entries, ("bias", "gamma", "beta"))
    assert names == ["conv2d/kernel", "conv2d/bias", "batch_normalization/gamma", "batch_normalization/beta"]
    cov = CL.covered(chunks, ps.n)
    want = np.zeros(ps.n, np.int32)
    for e in ps.entries:
        want[e["off"]:e["off"] + e["size"]] = 1
    assert (cov == want).all() and (want == 0).any()                              # every element once, padding never
    assert chunks["len"].max() == CH and (chunks["len"] > 0).all() and (chunks["off"] % 16 == 0).all()
    assert ps.entries[0]["size"] == 9 * 10 * 200 > 2 * CH
    # no chunk spans entries
    for off, ln, _ in chunks.tolist():
        assert any(e["off"] <= off and off + ln <= e["off"] + e["size"] for e in ps.entries)
    # both kernel segments are variable 0, whose chunk range is theirs alone
    seg_chunks = [k for k, (off, ln, v) in enumerate(chunks.tolist()) if off < ps.entries[2]["off"]]
    assert set(chunks["var"][seg_chunks].tolist()) == {0}
    assert (vars_["chunk_begin"][0], vars_["chunk_end"][0]) == (0, len(seg_chunks)) and len(seg_chunks) == 3 + 1
    assert (np.diff(chunks["var"]) >= 0).all() and vars_["chunk_begin"][1:].tolist() == vars_["chunk_end"][:-1].tolist()
    assert vars_["chunk_end"][-1] == len(chunks)
    assert vars_["decay"].tolist() == [1, 0, 0, 0]
    assert CL.build_chunk_table(ps.entries)[1]["decay"].tolist() == [1, 1, 1, 1]
    assert CL.build_chunk_table(ps.entries, ["conv2d"])[1]["decay"].tolist() == [0, 0, 1, 1]
    small = CL.build_chunk_table(ps.entries, chunk=16)[0]
    assert small["len"].max() == 16 and (CL.covered(small, ps.n) == want).all()


def test_table_refuses_what_the_kernels_could_not_walk():
    with pytest.raises(ValueError):
        CL.build_chunk_table([dict(name="a", off=8, size=4)])
    with pytest.raises(ValueError):
        CL.build_chunk_table([dict(name="a", off=0, size=40), dict(name="b", off=32, size=4)])
    with pytest.raises(ValueError):
        CL.build_chunk_table([dict(name="a", off=0, size=4), dict(name="b", off=16, size=4), dict(name="a", off=32, size=4)])
    with pytest.raises(ValueError):
        CL.build_chunk_table([dict(name="a", off=0, size=4)], chunk=100)


@pytest.mark.parametrize("cls", [Adam, SGD])
def test_optimizer_arguments(cls):
    for kw in (dict(clipnorm=1.0, clipvalue=0.5), dict(clipnorm=1.0, global_clipnorm=1.0), dict(global_clipnorm=2.0, clipvalue=0.5)):
        with pytest.raises(ValueError, match="only one"):
            cls(**kw)
    for k in ("clipnorm", "global_clipnorm", "clipvalue"):
        for bad in (0, 0.0, -1.0, float("nan"), "1"):
            with pytest.raises(ValueError):
                cls(**{k: bad})
    with pytest.raises(ValueError):
        cls(weight_decay=-1e-4)
    o = cls(lr=0.01, clipnorm=2, weight_decay=1e-4, skip_nonfinite=True, use_ema=False, jit_compile=True, name="whatever")   # unknown keywords: swallowed
    assert o.lr.value == 0.01
    assert o.clip_options() == dict(clipnorm=2, global_clipnorm=None, clipvalue=None, weight_decay=1e-4, decay_exclude=None, skip_nonfinite=True)
    o.exclude_from_weight_decay(var_names=["bias", "gamma"])
    assert o.clip_options()["decay_exclude"] == ["bias", "gamma"]
    plain = cls()
    assert plain.clip_options() == dict(clipnorm=None, global_clipnorm=None, clipvalue=None, weight_decay=None, decay_exclude=None, skip_nonfinite=False)
    assert not LossSpec(**plain.clip_options()).clip_on()


def test_loss_spec_round_trip_through_the_checkpoint_metadata():
    sp = LossSpec(kind={"seg": 0}, weight={"seg": 1.0}, clipvalue=0.25, weight_decay=4e-5, decay_exclude=["bias", "beta"], skip_nonfinite=True)
    assert sp.clip_on()
    lo = json.loads(json.dumps(dict(kind=sp.kind, weight=sp.weight, optimizer=sp.optimizer, lr=sp.lr, **sp.clip_options())))
    back = LossSpec(kind=lo["kind"], weight=lo["weight"], **loss_clip_options(lo))
    assert back.clip_options() == sp.clip_options() and back == sp
    old = dict(kind={"seg": 0}, weight={"seg": 1.0}, optimizer="adam", lr=1e-3, beta_1=0.9, beta_2=0.999, momentum=0.8)      # written before the options existed
    off = LossSpec(kind=old["kind"], weight=old["weight"], **loss_clip_options(old))
    assert not off.clip_on() and off == LossSpec(kind={"seg": 0}, weight={"seg": 1.0})
    for kw in (dict(clipnorm=1.0), dict(global_clipnorm=1.0), dict(clipvalue=1.0), dict(weight_decay=1e-4), dict(skip_nonfinite=True)):
        assert LossSpec(**kw).clip_on()
    assert not LossSpec(weight_decay=0.0, decay_exclude=["bias"]).clip_on()


# ---- host_clipped_step against elements worked out by hand -------------------------------------------------------------------------------------
def hand_table():
    """Two variables of three elements each: "w" decays, "w/bias" does not."""
    return CL.build_chunk_table([dict(name="w", off=0, size=3), dict(name="w/bias", off=16, size=3)], ("bias",))


TH = np.zeros(32); TH[:3] = [1.0, -2.0, 0.5]; TH[16:19] = [4.0, 0.0, -1.0]
G = np.zeros(32); G[:3] = [3.0, 4.0, 0.0]; G[16:19] = [0.0, 0.0, 12.0]       # norms 5 and 12, global 13
PAD = np.r_[3:16, 19:32]


def test_host_step_global_clipnorm_by_hand():
    chunks, vars_, _ = hand_table()
    r = CL.host_clipped_step(TH, G, np.zeros(32), np.zeros(32), chunks, vars_, lr=0.1, beta_1=0.5, beta_2=0.75, eps=1e-30, global_clipnorm=6.5)
    assert r["norm"] == 13.0 and r["sumsq"].tolist() == [25.0, 144.0] and (r["coef"] == np.float32(0.5)).all() and not r["skipped"]
    # coef = 6.5 / 13 = 0.5: gg = 1.5, 2, 6; m = gg / 2, v = gg^2 / 4, so the step is lr * (gg / 2) / (|gg| / 2) = lr * sign(gg)
    assert r["gg"][[0, 1, 18]].tolist() == [1.5, 2.0, 6.0]
    assert np.allclose(r["theta"][[0, 1, 18]], [1.0 - 0.1, -2.0 - 0.1, -1.0 - 0.1], rtol=0, atol=1e-15)
    assert r["theta"][2] == 0.5 and (r["theta"][PAD] == 0).all() and (r["g"] == 0).all()
    # half the gradient norm under grad_scale 0.5: nothing is clipped at c = 6.5
    r = CL.host_clipped_step(TH, G, np.zeros(32), np.zeros(32), chunks, vars_, lr=0.1, beta_1=0.5, beta_2=0.75, eps=1e-30, global_clipnorm=6.5, grad_scale=0.5)
    assert r["norm"] == 6.5 and (r["coef"] == 1).all() and r["gg"][[0, 1, 18]].tolist() == [1.5, 2.0, 6.0]


def test_host_step_clipnorm_by_hand():
    chunks, vars_, _ = hand_table()
    r = CL.host_clipped_step(TH, G, np.zeros(32), np.zeros(32), chunks, vars_, optimizer="sgd", lr=0.5, momentum=0.0, clipnorm=6.0)
    assert r["coef"].tolist() == [1.0, 0.5]                                       # norms 5 (below c) and 12 (above)
    assert r["gg"][[0, 1, 18]].tolist() == [3.0, 4.0, 6.0]
    assert r["theta"][[0, 1, 18]].tolist() == [1.0 - 1.5, -2.0 - 2.0, -1.0 - 3.0] and r["m"][[0, 1, 18]].tolist() == [-1.5, -2.0, -3.0]


def test_host_step_clipvalue_by_hand():
    chunks, vars_, _ = hand_table()
    g = G.copy(); g[0] = 3.5; g[1] = -3.5; g[2] = 3.4999; g[17] = np.nan
    r = CL.host_clipped_step(TH, g, np.zeros(32), np.zeros(32), chunks, vars_, optimizer="sgd", lr=1.0, momentum=0.0, clipvalue=3.5)
    assert r["gg"][[0, 1, 2, 18]].tolist() == [3.5, -3.5, 3.4999, 3.5] and np.isnan(r["gg"][17])      # at +-c as they are; beyond: c; a NaN stays
    assert r["theta"][[0, 1, 18]].tolist() == [1.0 - 3.5, -2.0 + 3.5, -1.0 - 3.5] and np.isnan(r["theta"][17]) and (r["coef"] == 1).all()


def test_host_step_decay_and_momentum_by_hand():
    chunks, vars_, _ = hand_table()
    vel = np.zeros(32); vel[0] = 2.0; vel[16] = -1.0
    r = CL.host_clipped_step(TH, G, vel, None, chunks, vars_, optimizer="sgd", lr=0.25, lr_base=0.5, momentum=0.5, weight_decay=0.25)
    d = float(np.float32(0.125))                                                  # wd * lr_base, exact in float32
    # "w" decays: th1 = th * (1 - 1/8); vel' = 0.5 vel - 0.25 g; th' = th1 + vel'
    assert r["th1"][:3].tolist() == [0.875, -1.75, 0.4375] and d == 0.125
    assert r["m"][:3].tolist() == [1.0 - 0.75, -1.0, 0.0] and r["theta"][:3].tolist() == [0.875 + 0.25, -1.75 - 1.0, 0.4375]
    # "w/bias" does not: th1 = th
    assert r["th1"][16:19].tolist() == [4.0, 0.0, -1.0] and r["theta"][16:19].tolist() == [4.0 - 0.5, 0.0, -1.0 - 3.0]
    # Adam decays with the BASE rate, not the rate of the update
    a = CL.host_clipped_step(TH, G, np.zeros(32), np.zeros(32), chunks, vars_, lr=0.1, lr_base=0.5, beta_1=0.5, beta_2=0.75, eps=1e-30, weight_decay=0.25)
    assert a["th1"][0] == 0.875 and abs(a["theta"][0] - (0.875 - 0.1)) < 1e-15 and a["theta"][16] == 4.0


def test_host_step_skip_by_hand():
    chunks, vars_, _ = hand_table()
    g = G.copy(); g[18] = np.inf
    m, v = np.full(32, 0.25), np.full(32, 0.5)
    r = CL.host_clipped_step(TH, g, m, v, chunks, vars_, lr=0.1, global_clipnorm=1.0, weight_decay=0.5, skip_nonfinite=True)
    assert r["skipped"] and (r["theta"] == TH).all() and (r["m"] == m).all() and (r["v"] == v).all()
    assert (r["g"][[0, 1, 2, 16, 17, 18]] == 0).all()                             # the gradient is consumed all the same
    r = CL.host_clipped_step(TH, g, m, v, chunks, vars_, lr=0.1, global_clipnorm=1.0)
    assert not r["skipped"] and not np.isfinite(r["theta"][[0, 1, 18]]).all()     # without the option the bad value goes through
    r = CL.host_clipped_step(TH, G, m, v, chunks, vars_, lr=0.1, skip_nonfinite=True)
    assert not r["skipped"] and (r["theta"][[0, 1, 18]] != TH[[0, 1, 18]]).all()
    with pytest.raises(ValueError):
        CL.host_clipped_step(TH, G, m, v, chunks, vars_, lr=0.1, clipnorm=1.0, clipvalue=1.0)


def test_engine_compile_refuses_bad_options_before_anything_else():
    from resunet_a_mltsk_keras_amd.engine import Engine, ModelConfig
    eng = Engine(ModelConfig(input_shape=(64, 64, 3), num_classes=4), _layout_only=True)
    for kw in (dict(clipnorm=1.0, clipvalue=1.0), dict(global_clipnorm=0.0), dict(weight_decay=-1.0)):
        with pytest.raises(ValueError):
            eng.compile(LossSpec(**kw))
