"""What gradient clipping, decoupled weight decay and the non-finite step skip cost, on the chunk table of the real cfg3 bf16 engine
(256 x 256 x 6, 6 classes, multitask, batch 8).

1. Kernels through the C ABI on the engine's own buffers: microseconds per launch (HIP events around REPS back-to-back launches) and the
   algorithmic bytes over that time, of rua_grad_sumsq, rua_clip_finish, rua_adam_step_w (the default path's optimizer, the yardstick),
   rua_adam_step_seg with every option neutral and with all of them on, and rua_state_copy.  Bytes: the sum of squares reads G (4 N); Adam
   reads theta, g, m, v and writes theta, m, v and the bf16 copy (30 N; zero_grad is off in these rows so that the gradient stays); the finisher reads the partials (8 per chunk).
2. The whole bf16 graph step, batch resident: options off, global_clipnorm on, everything on (clipnorm + weight decay + skip) - three engines
   in one process, alternated for ROUNDS rounds, so that drift shows as spread and not as a difference.
Prints one JSON line.  Usage: python tools/bench_clip.py [--reps 50] [--rounds 3] [--steps 40] [--warmup 10] [--kernels-only]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from resunet_a_mltsk_keras_amd import _lib as L  # noqa: E402
from resunet_a_mltsk_keras_amd import clip as CL  # noqa: E402
from resunet_a_mltsk_keras_amd.engine import HEADS, KERAS_EPS, Engine, LossSpec, ModelConfig  # noqa: E402
from resunet_a_mltsk_keras_amd.synthetic import make_batch  # noqa: E402

PATCH, CH, NCLS, BATCH = 256, 6, 6, 8                       # bench.py's cfg3


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
        sys.exit("bench_clip.py needs a GPU")
    lib = L.lib()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    x, y = make_batch(BATCH, PATCH, CH, NCLS, True, seed=1234)
    res = {}

    def events(fn, prep=None):
        if prep is not None:
            prep()
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

    # ---- 1. kernels: a real gradient in G (one backward), the engine's own table -----------------------------------------------------
    eng = engine(clipnorm=1.0, weight_decay=1e-4, decay_exclude=list(CL.DEFAULT_DECAY_EXCLUDE), skip_nonfinite=True)
    eng.forward_backward(x, y)
    torch.cuda.synchronize()
    ck, ps = eng.clip, eng.params
    N = int(sum(e["size"] for e in ps.entries))
    res["table"] = dict(elements=N, flat=ps.n, chunks=ck["n_chunks"], variables=ck["n_vars"], chunk=CL.OPT_CHUNK, state=ps.ns)
    p = lambda t: t.data_ptr()

    def seg(mode, c, wd, flag, cv=0.0):
        """(the finisher call that leaves this row's coefficients and flag, the timed launch)"""
        prep = lambda: lib.call("rua_clip_finish", p(ck["partials"]), ck["n_chunks"], p(ck["vars"]), ck["n_vars"], mode, c, 1.0, 1 if flag else 0, p(ck["var_sumsq"]),
                                p(ck["coef"]), p(ck["flag"]), p(ck["report"]), s)
        return prep, lambda: lib.call("rua_adam_step_seg", p(eng.P), p(eng.G), p(eng.M1), p(eng.V1), p(ck["chunks"]), ck["n_chunks"], p(ck["vars"]), p(ck["coef"]),
                                p(ck["flag"]) if flag else None, p(eng.lr_dev), p(eng.lr_state), 0.9, 0.999, KERAS_EPS, 1.0, cv, wd, 0, p(eng.Wf), s)
    eng._set_lr()
    lib.call("rua_lr_step", p(eng.lr_state), p(eng.lr_dev), 1, 0.9, 0.999, s)
    rows = [("rua_grad_sumsq", 4 * N, None, lambda: lib.call("rua_grad_sumsq", p(eng.G), p(ck["chunks"]), ck["n_chunks"], p(ck["partials"]), s))]
    rows.append(("rua_clip_finish", 8 * ck["n_chunks"], None, lambda: lib.call(
        "rua_clip_finish", p(ck["partials"]), ck["n_chunks"], p(ck["vars"]), ck["n_vars"], CL.CLIP_GLOBAL_NORM, 1.0, 1.0, 1, p(ck["var_sumsq"]), p(ck["coef"]), p(ck["flag"]),
        p(ck["report"]), s)))
    # zero_grad = 0 in the Adam rows: the gradient stays what the backward left (the store of the zeros is 4 of the 34 bytes per element)
    rows.append(("rua_adam_step_w", 30 * ps.n, None, lambda: lib.call("rua_adam_step_w", p(eng.P), p(eng.G), p(eng.M1), p(eng.V1), ps.n, 0.0, p(eng.lr_dev), 0.9, 0.999,
                                                                KERAS_EPS, 1.0, 0, p(eng.Wf), s)))
    rows.append(("rua_adam_step_seg neutral", 30 * N) + seg(CL.CLIP_NONE, 0.0, 0.0, False))
    rows.append(("rua_adam_step_seg clipnorm + decay + flag", 30 * N) + seg(CL.CLIP_NORM, 1.0, 1e-4, True))
    rows.append(("rua_state_copy", 8 * ps.ns, None, lambda: lib.call("rua_state_copy", p(ck["s_backup"]), p(eng.S), ps.ns, None, s)))
    res["kernels"] = {}
    for _ in range(args.rounds):
        for name, nbytes, prep, fn in rows:
            us = events(fn, prep)
            r = res["kernels"].setdefault(name, dict(bytes=nbytes, us=[], TBps=[]))
            r["us"].append(round(us, 2)); r["TBps"].append(round(nbytes / us / 1e6, 3))
    assert torch.isfinite(eng.P).all()
    del eng
    torch.cuda.empty_cache()
    if args.kernels_only:
        print(json.dumps(res))
        return

    # ---- 2. the whole step ---------------------------------------------------------------------------------------------------------------
    engines = {"off": engine(), "global_clipnorm": engine(global_clipnorm=1.0),
               "all": engine(clipnorm=1.0, weight_decay=1e-4, decay_exclude=list(CL.DEFAULT_DECAY_EXCLUDE), skip_nonfinite=True)}
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
                          report={k: e.clip_report() for k, e in engines.items()})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
