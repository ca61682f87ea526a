"""What gradient accumulation costs, on the parameter buffer of the real cfg3 bf16 engine (256 x 256 x 6, 6 classes, multitask, batch 8).

1. Kernels through the C ABI on the engine's own buffers: microseconds per launch (HIP events around REPS back-to-back launches) and the
   algorithmic bytes over that time, of rua_accum_step on a hold step (reads g and a, writes a: 12 N bytes) and on an update step (reads
   both, writes both: 16 N) next to rua_adam_step_w (30 N; zero_grad off), of the segmented Adam under the combined flag (what a hold step
   runs in the optimizer's place: reads theta, writes g and the bf16 copy, 10 N), of the gated sum of squares on a hold step, and of the
   one-thread gate.
2. The whole bf16 graph step, batch resident: the option off and K = 4 - two engines in one process, alternated for ROUNDS rounds.  Every
   step sits between two HIP events on the compute stream (the queue stays full; one synchronise per round), and the K = 4 engine's steps
   are sorted into hold and update steps by the position in the cycle, so the two are timed apart although one captured graph runs both.

Measured on one MI355X (cfg3, N = 42.7 M flat elements, 5519 chunks), three rounds each:
   rua_adam_step_w 262.6 / 263.5 / 264.5 us (4.86 TB/s);  rua_accum_step hold 78.9 / 79.0 / 75.5 us (6.5 TB/s), update 120.5 / 120.4 /
   120.5 us (5.67 TB/s);  segmented Adam under the flag 83.9 / 83.6 / 83.7 us (5.1 TB/s);  the gated sum of squares 3.5 - 4.0 us on a hold
   step (launch latency) against 25.0 us on an update step;  the gate 3.4 - 3.5 us.
   Step (244 dispatches off, 248 on): off 5.971 / 5.967 / 5.975 ms;  K = 4 hold 5.914 / 5.913 / 5.910 ms;  update 6.149 / 6.141 / 6.145 ms.
   A hold step costs 0.058 ms LESS than the step without the option (the optimizer streams 10 N bytes instead of 30 N, the sum of squares
   exits; rua_accum_step gives 0.079 of it back).  An update step costs 0.174 ms more: rua_accum_step's 0.120 plus the 0.053 ms of the
   global_clipnorm tail tools/bench_clip.py reports are 0.173 - the step sits AT that sum, not below it (the spread of one row is 0.008).
Prints one JSON line.  Usage: python tools/bench_accum.py [--reps 50] [--rounds 3] [--steps 40] [--warmup 12] [--kernels-only]"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from resunet_a_mltsk_keras_amd import _lib as L  # noqa: E402
from resunet_a_mltsk_keras_amd.engine import HEADS, KERAS_EPS, Engine, LossSpec, ModelConfig  # noqa: E402
from resunet_a_mltsk_keras_amd.synthetic import make_batch  # noqa: E402

PATCH, CH, NCLS, BATCH = 256, 6, 6, 8                       # bench.py's cfg3
K = 4


def engine(**kw):
    eng = Engine(ModelConfig(input_shape=(PATCH, PATCH, CH), num_classes=NCLS, multitasking=True), dtype="bf16", seed=0)
    eng.compile(LossSpec(kind={h: L.LOSS_TANIMOTO for h in HEADS}, weight={h: 1.0 for h in HEADS}, optimizer="adam", lr=1e-3, **kw))
    return eng


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=12)
    ap.add_argument("--kernels-only", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_accum.py needs a GPU")
    if args.steps % K or args.warmup % K:
        sys.exit(f"--steps and --warmup must be multiples of K = {K}")
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

    # ---- 1. kernels: a real gradient in G (one backward), the engine's own buffers ---------------------------------------------------------
    eng = engine(gradient_accumulation_steps=K)
    eng.forward_backward(x, y)
    torch.cuda.synchronize()
    ps, ck = eng.params, eng.clip
    p = lambda t: t.data_ptr()
    res["buffer"] = dict(elements=int(sum(e["size"] for e in ps.entries)), flat=ps.n, chunks=ck["n_chunks"])
    eng.G.mul_(1e-3)                                          # the hold rows add it REPS times: keep the sums finite
    one = torch.tensor([1, 1, 0, 0], dtype=torch.int32, device=eng.dev)
    zero = torch.zeros(4, dtype=torch.int32, device=eng.dev)
    gate_st = torch.zeros(4, dtype=torch.int32, device=eng.dev)
    eng._set_lr()
    lib.call("rua_lr_step", p(eng.lr_state), p(eng.lr_dev), 1, 0.9, 0.999, s)
    ck["coef"].fill_(1.0)
    seg = lambda g: lib.call("rua_adam_step_seg", p(eng.P), p(g), p(eng.M1), p(eng.V1), p(ck["chunks"]), ck["n_chunks"], p(ck["vars"]), p(ck["coef"]), p(one),
                             p(eng.lr_dev), p(eng.lr_state), 0.9, 0.999, KERAS_EPS, 1.0, 0.0, 0.0, 1, p(eng.Wf), s)
    scratch_g = eng.G.clone()
    rows = [
        ("rua_adam_step_w", 30 * ps.n, lambda: lib.call("rua_adam_step_w", p(eng.P), p(eng.G), p(eng.M1), p(eng.V1), ps.n, 0.0, p(eng.lr_dev), 0.9, 0.999, KERAS_EPS,
                                                        1.0, 0, p(eng.Wf), s)),
        ("rua_accum_step hold", 12 * ps.n, lambda: lib.call("rua_accum_step", p(eng.G), p(eng.A), ps.n, K, p(one), s)),
        ("rua_accum_step update", 16 * ps.n, lambda: lib.call("rua_accum_step", p(eng.G), p(eng.A), ps.n, K, p(zero), s)),
        ("rua_adam_step_seg held", 10 * ps.n, lambda: seg(scratch_g)),
        ("rua_grad_sumsq_gated hold", 0, lambda: lib.call("rua_grad_sumsq_gated", p(eng.G), p(ck["chunks"]), ck["n_chunks"], p(ck["partials"]), p(one), s)),
        ("rua_grad_sumsq_gated update", 4 * ps.n, lambda: lib.call("rua_grad_sumsq_gated", p(eng.G), p(ck["chunks"]), ck["n_chunks"], p(ck["partials"]), p(zero), s)),
        ("rua_accum_gate", 0, lambda: lib.call("rua_accum_gate", p(gate_st), K, p(gate_st) + 4, s)),
    ]
    res["kernels"] = {}
    for _ in range(args.rounds):
        for name, nbytes, fn in rows:
            us = events(fn)
            r = res["kernels"].setdefault(name, dict(bytes=nbytes, us=[], TBps=[]))
            r["us"].append(round(us, 2)); r["TBps"].append(round(nbytes / us / 1e6, 3))
    assert torch.isfinite(eng.P).all() and torch.isfinite(eng.A).all()
    del eng, scratch_g
    torch.cuda.empty_cache()
    if args.kernels_only:
        print(json.dumps(res))
        return

    # ---- 2. the whole step ---------------------------------------------------------------------------------------------------------------
    engines = {"off": engine(), "accum": engine(gradient_accumulation_steps=K)}
    for e in engines.values():
        e.train_step(x, y, fetch=False)                     # warm-up + capture; the batch is resident from here on
        for _ in range(K - 1):
            e.train_step(None, None, fetch=False)           # ... and the K = 4 engine stands at the start of a cycle

    def timed(e):
        for _ in range(args.warmup):
            e.train_step(None, None, fetch=False)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
        torch.cuda.synchronize()
        ev[0].record()
        for i in range(args.steps):
            e.train_step(None, None, fetch=False)
            ev[i + 1].record()
        torch.cuda.synchronize()
        return [ev[i].elapsed_time(ev[i + 1]) for i in range(args.steps)]
    mean = lambda v: round(sum(v) / len(v), 4)
    steps = {"off": [], "hold": [], "update": []}
    for _ in range(args.rounds):
        for k, e in engines.items():
            assert k == "off" or e.accumulation_state()["micro"] == 0
            ms = timed(e)
            if k == "off":
                steps["off"].append(mean(ms))
            else:
                steps["hold"].append(mean([t for i, t in enumerate(ms) if i % K != K - 1]))
                steps["update"].append(mean([t for i, t in enumerate(ms) if i % K == K - 1]))
    res["step_ms"] = dict(shape=[BATCH, PATCH, PATCH, CH], dtype="bf16", path="graph", K=K, warmup=args.warmup, steps=args.steps, **steps,
                          dispatches_per_step={k: e.count_step_dispatches(BATCH) for k, e in engines.items()},
                          updates={k: e.t for k, e in engines.items()})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
