"""What the LAMB optimizer costs next to Adam, on the chunk table of the real cfg3 bf16 engine (256 x 256 x 6, 6 classes, multitask, batch 8).

1. Kernels through the C ABI on the engine's own buffers: microseconds per launch (HIP events around REPS back-to-back launches) and the
   algorithmic bytes over that time, of rua_adam_step_seg (the yardstick: 16 read + 12 written + 4 of zeros + 2 of the bf16 copy = 34 bytes per
   element), rua_lamb_moments (16 + 12 = 28), rua_lamb_finish (two partials per chunk) and rua_lamb_apply (8 read + 4 + 4 of zeros + 2 = 18).
   By bytes the two passes are 46 / 34 = 1.35 Adams; `lamb_over_adam` is the measured ratio of (moments + finish + apply) to Adam.
2. The whole bf16 graph step, batch resident: adam (flat), adam over the chunk table (global_clipnorm), lamb, lamb + global_clipnorm - four
   engines in one process, alternated for ROUNDS rounds, so that drift shows as spread and not as a difference.
Nothing is asserted on time.  Prints one JSON line.  Usage: python tools/bench_lamb.py [--reps 50] [--rounds 3] [--steps 40] [--warmup 10] [--kernels-only]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from resunet_a_mltsk_keras_amd import _lib as L  # noqa: E402
from resunet_a_mltsk_keras_amd.engine import HEADS, KERAS_EPS, Engine, LossSpec, ModelConfig  # noqa: E402
from resunet_a_mltsk_keras_amd.synthetic import make_batch  # noqa: E402

PATCH, CH, NCLS, BATCH = 256, 6, 6, 8                       # bench.py's cfg3


def engine(**kw):
    eng = Engine(ModelConfig(input_shape=(PATCH, PATCH, CH), num_classes=NCLS, multitasking=True), dtype="bf16", seed=0)
    eng.compile(LossSpec(kind={h: L.LOSS_TANIMOTO for h in HEADS}, weight={h: 1.0 for h in HEADS}, lr=1e-3, **kw))
    return eng


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--kernels-only", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_lamb.py needs a GPU")
    lib = L.lib()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    x, y = make_batch(BATCH, PATCH, CH, NCLS, True, seed=1234)
    res = {}

    def events(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.reps

    # ---- 1. kernels: a real gradient in G (one backward), the engine's own table; after the first launch the gradient's slot holds zeros - the
    #         kernels' time does not depend on the values
    eng = engine(optimizer="lamb")
    eng.forward_backward(x, y)
    torch.cuda.synchronize()
    ck, ps = eng.clip, eng.params
    N = int(sum(e["size"] for e in ps.entries))
    res["table"] = dict(elements=N, flat=ps.n, chunks=ck["n_chunks"], variables=ck["n_vars"])
    p = lambda t: t.data_ptr()
    eng._set_lr()
    lib.call("rua_lr_step", p(eng.lr_state), p(eng.lr_dev), 0, 0.9, 0.999, s)
    rows = [
        ("rua_adam_step_seg", 34 * N, lambda: lib.call(
            "rua_adam_step_seg", p(eng.P), p(eng.G), p(eng.M1), p(eng.V1), p(ck["chunks"]), ck["n_chunks"], p(ck["vars"]), p(ck["coef"]), None, p(eng.lr_dev),
            p(eng.lr_state), 0.9, 0.999, KERAS_EPS, 1.0, 0.0, 0.0, 1, p(eng.Wf), s)),
        ("rua_lamb_moments", 28 * N, lambda: lib.call(
            "rua_lamb_moments", p(eng.P), p(eng.G), p(eng.M1), p(eng.V1), p(ck["chunks"]), ck["n_chunks"], p(ck["vars"]), p(ck["coef"]), None, p(eng.lr_state),
            0.9, 0.999, 1e-7, 1.0, 0.0, 0.0, p(ck["pw"]), p(ck["pu"]), s)),
        ("rua_lamb_finish", 16 * ck["n_chunks"], lambda: lib.call(
            "rua_lamb_finish", p(ck["pw"]), p(ck["pu"]), ck["n_chunks"], p(ck["vars"]), ck["n_vars"], None, p(ck["var_wu"]), p(ck["ratio"]), p(ck["trust"]), s)),
        ("rua_lamb_apply", 18 * N, lambda: lib.call(
            "rua_lamb_apply", p(eng.P), p(eng.G), p(ck["chunks"]), ck["n_chunks"], p(ck["vars"]), p(ck["ratio"]), None, p(eng.lr_dev), p(eng.lr_state), 0.0, 1,
            p(eng.Wf), s)),
    ]
    res["kernels"] = {}
    for _ in range(args.rounds):
        for name, nbytes, fn in rows:
            us = events(fn)
            r = res["kernels"].setdefault(name, dict(bytes=nbytes, us=[], TBps=[]))
            r["us"].append(round(us, 2)); r["TBps"].append(round(nbytes / us / 1e6, 3))
    k = res["kernels"]
    med = lambda v: sorted(v)[len(v) // 2]
    lamb_us = med(k["rua_lamb_moments"]["us"]) + med(k["rua_lamb_finish"]["us"]) + med(k["rua_lamb_apply"]["us"])
    res["lamb_over_adam"] = dict(by_bytes=round(46 / 34, 3), measured=round(lamb_us / med(k["rua_adam_step_seg"]["us"]), 3))
    assert torch.isfinite(eng.P).all()
    del eng
    torch.cuda.empty_cache()
    if args.kernels_only:
        print(json.dumps(res))
        return

    # ---- 2. the whole step ---------------------------------------------------------------------------------------------------------------
    engines = {"adam": engine(), "adam global_clipnorm": engine(global_clipnorm=1.0), "lamb": engine(optimizer="lamb"),
               "lamb global_clipnorm": engine(optimizer="lamb", global_clipnorm=1.0)}
    for e in engines.values():
        e.train_step(x, y, fetch=False)                     # warm-up + capture; the batch is resident from here on
        e.train_step(None, None, fetch=False)

    def timed(e):
        for _ in range(args.warmup):
            e.train_step(None, None, fetch=False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            e.train_step(None, None, fetch=False)
        torch.cuda.synchronize()
        return round((time.perf_counter() - t0) * 1e3 / args.steps, 4)
    steps = {k: [] for k in engines}
    for _ in range(args.rounds):
        for k, e in engines.items():
            steps[k].append(timed(e))
    trust = {k: e.trust_report() for k, e in engines.items()}
    res["step_ms"] = dict(shape=[BATCH, PATCH, PATCH, CH], dtype="bf16", path="graph", warmup=args.warmup, steps=args.steps, **steps,
                          dispatches_per_step={k: e.count_step_dispatches(BATCH) for k, e in engines.items()},
                          trust={k: None if t is None else {q: t[q] for q in ("min_ratio", "max_ratio", "forced", "updates")} for k, t in trust.items()})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
