"""What a learning-rate schedule and the weights' moving average cost, on the parameter buffer of the real cfg3 bf16 engine
(256 x 256 x 6, 6 classes, multitask, batch 8).

1. Kernels through the C ABI on the engine's own buffers: microseconds per launch (HIP events around REPS back-to-back launches) and the
   algorithmic bytes over that time, of rua_ema_step (the update: reads ema and theta, writes ema, 12 N bytes; at an overwrite step it also
   writes theta and the bf16 copy, 18 N) next to rua_adam_step_w (reads theta, g, m, v, writes theta, m, v and the bf16 copy: 30 N;
   zero_grad off), and of the two one-thread rate kernels, rua_lr_step and rua_lr_schedule_step (cosine with warm-up).
2. The whole bf16 graph step, batch resident: options off, a schedule, schedule + EMA - three engines in one process, alternated for
   ROUNDS rounds, so that drift shows as spread and not as a difference.
Prints one JSON line.  Usage: python tools/bench_sched.py [--reps 50] [--rounds 3] [--steps 40] [--warmup 10] [--kernels-only]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from resunet_a_mltsk_keras_amd import _lib as L  # noqa: E402
from resunet_a_mltsk_keras_amd import schedules as SC  # noqa: E402
from resunet_a_mltsk_keras_amd.engine import HEADS, KERAS_EPS, Engine, LossSpec, ModelConfig  # noqa: E402
from resunet_a_mltsk_keras_amd.synthetic import make_batch  # noqa: E402

PATCH, CH, NCLS, BATCH = 256, 6, 6, 8                       # bench.py's cfg3
SCHEDULE = SC.CosineDecay(1e-4, 100000, alpha=0.01, warmup_target=1e-3, warmup_steps=500)


def engine(**kw):
    eng = Engine(ModelConfig(input_shape=(PATCH, PATCH, CH), num_classes=NCLS, multitasking=True), dtype="bf16", seed=0)
    eng.compile(LossSpec(kind={h: L.LOSS_TANIMOTO for h in HEADS}, weight={h: 1.0 for h in HEADS}, optimizer="adam", lr=1e-3, **kw))
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
        sys.exit("bench_sched.py needs a GPU")
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
    eng = engine(use_ema=True, ema_momentum=0.99)
    eng.forward_backward(x, y)
    torch.cuda.synchronize()
    ps = eng.params
    p = lambda t: t.data_ptr()
    res["buffer"] = dict(elements=int(sum(e["size"] for e in ps.entries)), flat=ps.n)
    st_update = torch.tensor([5.0, 1e-3], dtype=torch.float64, device=eng.dev)       # t = 5: an update, no overwrite with overwrite_every = 0
    st_rate = torch.tensor([5.0, 1e-3], dtype=torch.float64, device=eng.dev)
    lr_out = torch.zeros(4, dtype=torch.float32, device=eng.dev)
    sched = SC.to_struct(SCHEDULE)
    eng._set_lr()
    lib.call("rua_lr_step", p(eng.lr_state), p(eng.lr_dev), 1, 0.9, 0.999, s)
    rows = [
        ("rua_adam_step_w", 30 * ps.n, lambda: lib.call("rua_adam_step_w", p(eng.P), p(eng.G), p(eng.M1), p(eng.V1), ps.n, 0.0, p(eng.lr_dev), 0.9, 0.999, KERAS_EPS,
                                                        1.0, 0, p(eng.Wf), s)),
        ("rua_ema_step update", 12 * ps.n, lambda: lib.call("rua_ema_step", p(eng.E), p(eng.P), p(eng.Wf), ps.n, 0.99, p(st_update), 0, None, s)),
        ("rua_ema_step update + overwrite", 18 * ps.n, lambda: lib.call("rua_ema_step", p(eng.E), p(eng.P), p(eng.Wf), ps.n, 0.99, p(st_update), 5, None, s)),
        ("rua_lr_step", 0, lambda: lib.call("rua_lr_step", p(st_rate), p(lr_out), 1, 0.9, 0.999, s)),
        ("rua_lr_schedule_step", 0, lambda: lib.call("rua_lr_schedule_step", p(st_rate), p(lr_out), sched, 1, 0.9, 0.999, s)),
    ]
    res["kernels"] = {}
    for _ in range(args.rounds):
        for name, nbytes, fn in rows:
            us = events(fn)
            r = res["kernels"].setdefault(name, dict(bytes=nbytes, us=[], TBps=[]))
            r["us"].append(round(us, 2)); r["TBps"].append(round(nbytes / us / 1e6, 3))
    assert torch.isfinite(eng.P).all() and torch.isfinite(eng.E).all()
    del eng
    torch.cuda.empty_cache()
    if args.kernels_only:
        print(json.dumps(res))
        return

    # ---- 2. the whole step ---------------------------------------------------------------------------------------------------------------
    engines = {"off": engine(), "schedule": engine(lr_schedule=SCHEDULE), "schedule_ema": engine(lr_schedule=SCHEDULE, use_ema=True, ema_momentum=0.99)}
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
    res["step_ms"] = dict(shape=[BATCH, PATCH, PATCH, CH], dtype="bf16", path="graph", warmup=args.warmup, steps=args.steps, **steps,
                          dispatches_per_step={k: e.count_step_dispatches(BATCH) for k, e in engines.items()},
                          rate={k: e.current_lr() for k, e in engines.items()})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
