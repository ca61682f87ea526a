"""CPU tests of online hard example mining: losses.host_ohem against a brute-force restatement that sorts the keys, the key order, the Q16 /
warm-up arithmetic, mmsegmentation's rule for plain cross-entropy, the option checks and refusals, the metadata round trip and the C ABI's
struct layouts."""
import ctypes
import json
import math
import os

import numpy as np
import pytest

from resunet_a_mltsk_keras_amd import _lib as L
from resunet_a_mltsk_keras_amd import losses as LS
from resunet_a_mltsk_keras_amd.engine import LossSpec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def key_of(v):
    """The key, restated with struct-free integer arithmetic on one value."""
    b = int(np.array([v], np.float32).view(np.uint32)[0])
    if (b & 0x7FFFFFFF) > 0x7F800000:
        return 0xFFFFFFFF
    return (~b & 0xFFFFFFFF) if b & 0x80000000 else (b | 0x80000000)


def brute(per_pixel, valid=None, keep_q16=16384, min_kept=0, thresh=None, warmup=0, t=0, loss_weight=1.0):
    """host_ohem restated: sort the valid keys and take the K-th from the top."""
    Lm = np.asarray(per_pixel, np.float32).reshape(-1)
    v = [True] * Lm.size if valid is None else [bool(x) for x in np.asarray(valid).reshape(-1)]
    keys = [key_of(x) for x in Lm]
    vk = sorted((k for k, ok in zip(keys, v) if ok), reverse=True)
    n_valid = len(vk)
    q = keep_q16 if warmup == 0 else 65536 - ((65536 - keep_q16) * min(t, warmup)) // warmup
    K = min(n_valid, max(min_kept, (n_valid * q + 65535) >> 16))
    tau = vk[K - 1] if K > 0 else 0xFFFFFFFF
    if thresh is not None:
        tau = min(tau, key_of(np.float32(thresh)))
    kept = [ok and k >= tau for k, ok in zip(keys, v)]
    n_kept = sum(kept)
    vals = [float(x) for x, kp in zip(Lm, kept) if kp]
    s = (math.fsum(vals) if all(math.isfinite(x) for x in vals) else float(np.sum(vals))) if n_kept else 0.0       # (fsum refuses inf - inf)
    return dict(drop=np.array([0 if kp else 1 for kp in kept], np.uint8), tau_key=tau, n_valid=n_valid, n_kept=n_kept, K=K, q16_used=q, kept_sum=s,
                scale=np.float32(np.float64(np.float32(loss_weight)) / n_kept) if n_kept else np.float32(0))


def edge_maps():
    rng = np.random.default_rng(5)
    base = np.float32(1.7917595)                         # log 6: the first steps of training
    bits = base.view(np.uint32)
    yield "one", np.array([0.5], np.float32), None
    yield "random", rng.random(257).astype(np.float32) * 3, None
    yield "all_equal", np.full(255, base, np.float32), None
    yield "low_bits", (bits + rng.integers(0, 1 << 10, 300).astype(np.uint32)).view(np.float32), None
    yield "mid_bits", (bits & np.uint32(0xFFE003FF) | (rng.integers(0, 1 << 11, 300).astype(np.uint32) << np.uint32(10))).view(np.float32), None
    yield "exponents", np.ldexp(1.0, rng.integers(-120, 120, 300)).astype(np.float32), None
    yield "specials", np.array([0.0, -0.0, np.inf, np.nan, 1.0, -1.0, -np.inf, 1e-42, 2.0, 0.0], np.float32), None
    yield "void30", rng.random(2046).astype(np.float32), (rng.random(2046) >= 0.3)
    yield "all_void", rng.random(64).astype(np.float32), np.zeros(64, bool)


@pytest.mark.parametrize("name,Lm,valid", list(edge_maps()), ids=[m[0] for m in edge_maps()])
def test_host_ohem_against_brute_force(name, Lm, valid):
    nv = int(Lm.size if valid is None else np.sum(valid))
    mid = float(np.sort(Lm[~np.isnan(Lm)])[Lm.size // 2]) if Lm.size > 1 else 0.5
    cases = [dict(), dict(keep_q16=65536), dict(keep_q16=1), dict(keep_q16=32768), dict(min_kept=nv + 5), dict(min_kept=max(nv // 2, 1), keep_q16=1),
             dict(thresh=mid), dict(thresh=-1.0, keep_q16=1), dict(thresh=1e30, keep_q16=40000), dict(keep_q16=6554, warmup=4, t=2, loss_weight=0.3)]
    for kw in cases:
        got, exp = LS.host_ohem(Lm, valid, **kw), brute(Lm, valid, **kw)
        assert np.array_equal(got["drop_mask"].reshape(-1), exp["drop"]), (name, kw)
        for k in ("tau_key", "n_valid", "n_kept", "K", "q16_used"):
            assert got[k] == exp[k], (name, kw, k, got[k], exp[k])
        assert got["n_kept"] >= got["K"]
        assert np.float32(got["scale"]).view(np.uint32) == np.float32(exp["scale"]).view(np.uint32)
        if not (math.isnan(exp["kept_sum"]) or math.isinf(exp["kept_sum"])):
            assert abs(got["kept_sum"] - exp["kept_sum"]) <= max(got["n_kept"], 1) * 2.0 ** -52 * abs(exp["kept_sum"]), (name, kw)      # an fp64 sum against fsum
            assert got["loss"] == (got["kept_sum"] / got["n_kept"] if got["n_kept"] else 0.0)
        assert np.float32(got["tau"]).view(np.uint32) == LS.ohem_unkey(exp["tau_key"]).view(np.uint32)
    # ties: K in the middle of a tie keeps the whole tie
    if name == "all_equal":
        r = LS.host_ohem(Lm, valid, keep_q16=32768)
        assert r["K"] == 128 and r["n_kept"] == 255 and not r["drop_mask"].any()
    if name == "all_void":
        r = LS.host_ohem(Lm, valid, thresh=0.0)
        assert (r["n_valid"], r["n_kept"], r["K"], r["loss"]) == (0, 0, 0, 0.0) and r["scale"] == 0 and r["drop_mask"].all()
    if name == "specials":
        r = LS.host_ohem(Lm, valid, keep_q16=1)          # K = 1: the NaN is the hardest pixel and the only one kept
        assert r["tau_key"] == 0xFFFFFFFF and list(np.flatnonzero(r["drop_mask"] == 0)) == [3] and math.isnan(r["loss"])


def test_key_order():
    vals = np.array([-np.inf, -1.0, -0.0, 0.0, 1e-42, 1.0, np.inf, np.nan], np.float32)          # (1e-42: a denormal)
    keys = LS.ohem_key(vals)
    assert keys.dtype == np.uint32 and all(int(a) < int(b) for a, b in zip(keys, keys[1:])), keys
    assert [int(k) for k in keys] == [key_of(v) for v in vals]
    assert int(keys[-1]) == 0xFFFFFFFF == int(LS.ohem_key(np.array([-np.nan], np.float32))[0]) == LS.NO_KEY
    for v in vals[:-1]:                                  # the key's inverse gives the bits back
        assert LS.ohem_unkey(LS.ohem_key(v)[0]).view(np.uint32) == np.float32(v).view(np.uint32)
    assert math.isnan(LS.ohem_unkey(0xFFFFFFFF))
    rng = np.random.default_rng(0)
    x = rng.standard_normal(1000).astype(np.float32)
    assert np.array_equal(np.argsort(LS.ohem_key(x), kind="stable"), np.argsort(x, kind="stable"))


def test_q16_and_warmup_arithmetic():
    assert LS.ohem_q16(0.25) == 16384 and LS.ohem_q16(1.0) == 65536 and LS.ohem_q16(1e-9) == 1 and LS.ohem_q16(0.1) == 6554
    for bad in (0.0, -0.1, 1.5):
        with pytest.raises(ValueError, match="keep_ratio"):
            LS.ohem_q16(bad)
    q, w = 16384, 10
    assert LS.ohem_share(q, 0, 7) == q                                       # no warm-up
    assert LS.ohem_share(q, w, 0) == 65536                                   # t = 0: everything
    assert LS.ohem_share(q, w, 5) == 65536 - ((65536 - q) * 5) // 10 == 40960        # t = warmup / 2
    assert LS.ohem_share(q, w, 10) == LS.ohem_share(q, w, 99) == q           # t >= warmup
    assert LS.ohem_share(6554, 3, 1) == 65536 - (58982 * 1) // 3 == 45876    # the division is an integer division
    assert LS.ohem_count(1000, 16384, 0) == 250 and LS.ohem_count(1001, 16384, 0) == 251 and LS.ohem_count(1000, 1, 0) == 1
    assert LS.ohem_count(1000, 16384, 400) == 400 and LS.ohem_count(1000, 16384, 4000) == 1000 and LS.ohem_count(0, 65536, 10) == 0
    assert LS.ohem_count(1 << 40, 65536, 0) == 1 << 40
    r = [LS.host_ohem(np.arange(100, dtype=np.float32), keep_q16=q, warmup=4, t=t) for t in (0, 2, 4, 9)]
    assert [x["q16_used"] for x in r] == [65536, 40960, 16384, 16384] and [x["K"] for x in r] == [100, 63, 25, 25]


def test_mmseg_rule_for_plain_ce():
    """mmsegmentation's OHEMPixelSampler with thresh = 0.7 and min_kept: sort the true-class probabilities ascending, threshold =
    max(prob[min_kept - 1], 0.7), keep prob < threshold.  Restated on the loss -log p: keep the min_kept hardest, and everything whose
    probability is at most 0.7."""
    rng = np.random.default_rng(3)
    C, M, min_kept = 6, 4000, 300
    z = rng.standard_normal((M, C)) * 2
    p = np.exp(z) / np.exp(z).sum(-1, keepdims=True)
    y = rng.integers(0, C, M)
    pt = p[np.arange(M), y].astype(np.float32)
    loss = (-np.log(pt.astype(np.float64))).astype(np.float32)
    o = LS.ohem_options(keep_q16=1, min_kept=min_kept, prob_thresh=0.7)
    assert o["thresh"] == float(np.float32(-math.log(0.7))) == LS.prob_to_thresh(0.7)
    r = LS.host_ohem(loss, keep_q16=o["keep_q16"], min_kept=o["min_kept"], thresh=o["thresh"])
    order = np.argsort(-loss, kind="stable")
    want = np.zeros(M, bool)
    want[order[:min_kept]] = True
    want |= loss >= np.float32(o["thresh"])
    want |= loss >= loss[order[min_kept - 1]]            # ties with the min_kept-th
    assert np.array_equal(r["drop_mask"] == 0, want) and r["n_kept"] >= min_kept
    few = LS.host_ohem(loss, keep_q16=1, min_kept=3900, thresh=o["thresh"])          # the floor above the threshold's count
    assert few["n_kept"] >= 3900 and few["K"] == 3900


def test_option_checks():
    ok = LS.ohem_options()
    assert ok == dict(keep_q16=16384, min_kept=0, thresh=None, prob_thresh=None, warmup=0)
    LS.check_ohem(ok)
    LS.check_ohem(dict(keep_q16=65536, min_kept=100000, thresh=0.35, warmup=1000))
    for bad, word in ((dict(keep_q16=0), "keep_q16"), (dict(keep_q16=65537), "keep_q16"), (dict(keep_q16=0.25), "keep_q16"), (dict(min_kept=-1), "min_kept"),
                      (dict(min_kept=1.5), "min_kept"), (dict(warmup=-1), "warmup"), (dict(warmup=True), "warmup"), (dict(thresh=float("nan")), "NaN"),
                      (dict(keep=3), "unknown"), (dict(prob_thresh=0.7), "disagree"), (dict(prob_thresh=0.7, thresh=0.1), "disagree")):
        with pytest.raises(ValueError, match=word):
            LS.check_ohem(bad)
    with pytest.raises(ValueError, match="one of them"):
        LS.ohem_options(thresh=0.2, prob_thresh=0.7)
    for bad in (0.0, 1.5, -1.0):
        with pytest.raises(ValueError, match="prob_thresh"):
            LS.ohem_options(prob_thresh=bad)
    with pytest.raises(ValueError, match="NaN"):
        LS.host_ohem(np.ones(4, np.float32), thresh=float("nan"))
    s = LS.to_ohem_struct(LS.ohem_options(keep_q16=100, min_kept=7, thresh=0.5, warmup=3))
    assert (s.min_kept, s.keep_q16, s.warmup, s.thresh, s.has_thresh) == (7, 100, 3, 0.5, 1)
    s = LS.to_ohem_struct(LS.ohem_options())
    assert (s.min_kept, s.keep_q16, s.warmup, s.has_thresh) == (0, 16384, 0, 0)


def test_keras_surface_options():
    from resunet_a_mltsk_keras_amd import keras_api as ka
    m = ka.OnlineHardExampleMining(ka.CategoricalCrossentropy(), keep_ratio=0.1, min_kept=50, prob_thresh=0.7, warmup_steps=20)
    assert m.kind == L.LOSS_CE_LOGITS and m.options == dict(keep_q16=6554, min_kept=50, thresh=LS.prob_to_thresh(0.7), prob_thresh=0.7, warmup=20)
    w = ka.OnlineHardExampleMining(ka.weighted_categorical_crossentropy([1, 2, 3], label_smoothing=0.1), loss_thresh=0.4)
    assert w.kind == L.LOSS_WCE and w.weights == [1.0, 2.0, 3.0] and w.label_smoothing == 0.1 and w.options["thresh"] == float(np.float32(0.4))
    f = ka.OnlineHardExampleMining("categorical_focal_crossentropy")
    assert f.kind == L.LOSS_FOCAL_CE and f.gamma == 2.0 and f.options["keep_q16"] == 16384
    assert ka.OnlineHardExampleMining("binary_crossentropy").kind == L.LOSS_BCE_LOGITS
    for kw, word in ((dict(keep_ratio=0.0), "keep_ratio"), (dict(min_kept=-3), "min_kept"), (dict(warmup_steps=-1), "warmup"),
                     (dict(loss_thresh=0.1, prob_thresh=0.5), "one of them"), (dict(prob_thresh=2.0), "prob_thresh"), (dict(loss_thresh=float("nan")), "NaN")):
        with pytest.raises(ValueError, match=word):
            ka.OnlineHardExampleMining(ka.CategoricalCrossentropy(), **kw)
    with pytest.raises(ValueError, match="nest"):
        ka.OnlineHardExampleMining(m)


def test_meta_round_trip():
    sp = LossSpec(kind={"seg": L.LOSS_CE_LOGITS, "bound": L.LOSS_FOCAL_BCE, "dist": L.LOSS_TANIMOTO, "color": L.LOSS_TANIMOTO},
                  weight={h: 1.0 for h in ("seg", "bound", "dist", "color")}, focal_gamma={"bound": 2.0},
                  ohem={"seg": LS.ohem_options(keep_q16=6554, min_kept=1000, prob_thresh=0.7, warmup=50), "bound": dict(keep_q16=32768)})
    lo = sp.loss_options()
    assert set(lo) == {"focal_gamma", "ohem"} and lo["ohem"]["bound"] == dict(keep_q16=32768)
    lo = json.loads(json.dumps(dict(kind=sp.kind, weight=sp.weight, **lo)))
    back = LS.options_from_meta(lo)
    assert back["ohem"]["seg"] == sp.ohem["seg"] and back["ohem"]["bound"] == LS.ohem_options(keep_q16=32768)
    assert np.float32(back["ohem"]["seg"]["thresh"]).view(np.uint32) == np.float32(-math.log(0.7)).view(np.uint32)      # the float32 survives the JSON text
    sp2 = LossSpec(kind=sp.kind, weight=sp.weight, **back)
    assert sp2.head_ohem("seg") == sp.head_ohem("seg") and sp2.head_ohem("bound") == sp.head_ohem("bound") and sp2.head_ohem("dist") is None
    assert sp.head_ohem("bound") == dict(keep_q16=32768, min_kept=0, thresh=None, prob_thresh=None, warmup=0)
    # a spec and a file without the option: nothing is carried, the keys of the focal options are what they were
    plain = LossSpec(kind={"seg": L.LOSS_WCE}, weight={"seg": 1.0})
    assert plain.loss_options() == {} and plain.head_ohem("seg") is None
    assert LS.options_from_meta(dict(kind={"seg": 1})) == {k: {} for k in LS.OPTION_KEYS} and LS.OHEM_KEY not in LS.OPTION_KEYS


def test_abi_structs_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "rua_hip.h")).read()
    assert "typedef struct rua_ohem_opts { int64_t min_kept; int32_t keep_q16, warmup; float thresh; int32_t has_thresh; } rua_ohem_opts;" in hdr
    assert ("typedef struct rua_ohem_result { uint32_t tau_key; float tau; int64_t n_valid, n_kept, K; double kept_sum; float scale; int32_t q16_used; } "
            "rua_ohem_result;") in hdr
    assert "typedef struct rua_dz_sel { const uint8_t* drop_mask; const float* scale_dev; } rua_dz_sel;" in hdr
    assert ctypes.sizeof(L.OhemOpts) == 24 and [f[0] for f in L.OhemOpts._fields_] == ["min_kept", "keep_q16", "warmup", "thresh", "has_thresh"]
    assert ctypes.sizeof(L.OhemResult) == 48 and L.OhemResult.scale.offset == 40 and L.OhemResult.kept_sum.offset == 32 and L.OhemResult.n_kept.offset == 16
    assert ctypes.sizeof(L.DzSel) == 16
    for sym in ("rua_ohem_select", "rua_ohem_workspace_bytes", "rua_head_dz_sel", "rua_head_dz_multi_sel"):
        assert sym in L.EXPORTED_SYMBOLS and sym in hdr
    src = open(os.path.join(ROOT, "resunet_a_mltsk_keras_amd", "csrc", "ohem.hip")).read()
    assert "SIX launches" in src and src.count("hipLaunchKernelGGL(") == 6          # the launch count the header comment states
    from resunet_a_mltsk_keras_amd import build as B
    assert "ohem.hip" in B.SOURCES
