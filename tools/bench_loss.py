"""What the focal kinds and label smoothing cost, at cfg3's seg head (batch 8, 256 x 256, 6 classes) and on the whole cfg3 bf16 step.

1. Kernels through the C ABI, all on the SAME buffers (softmax probabilities, one-hot labels, a weight vector): microseconds per launch (HIP
   events around REPS back-to-back launches) and the algorithmic bytes over that time, of the loss entry (reads p and y: 48 bytes per pixel,
   plus 4 written with the per-pixel map) and of the dz entry (reads p and y, writes dz: 72 bytes per pixel) for weighted CE through the
   entries without options (the yardstick), weighted CE with label smoothing, focal CE at gamma 2 (the squared path), 3.5 (powf) and 0, and
   binary focal at gamma 2 on the same buffers read as six sigmoid channels.  The expectation from the code is only that the new kinds move
   the same bytes as weighted CE.
2. The whole bf16 graph step, batch resident, as `--loss weighted_cross_entropy` compiles it (weighted CE / BCE / MSE / MSE) against
   `--loss focal` (focal CE / binary focal / MSE / MSE): two engines in one process, alternated for ROUNDS rounds.

Prints one JSON line.  Usage: python tools/bench_loss.py [--reps 50] [--rounds 3] [--steps 40] [--warmup 10] [--kernels-only]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from resunet_a_mltsk_keras_amd import _lib as L  # noqa: E402
from resunet_a_mltsk_keras_amd import losses as LS  # noqa: E402
from resunet_a_mltsk_keras_amd.engine import Engine, LossSpec, ModelConfig  # noqa: E402
from resunet_a_mltsk_keras_amd.synthetic import make_batch  # noqa: E402

PATCH, CH, NCLS, BATCH = 256, 6, 6, 8                       # bench.py's cfg3
W = [1.0, 2.0, 0.5, 4.0, 1.5, 3.0]
WEIGHT = {"seg": 1.0, "bound": 1.0, "dist": 1.0, "color": 1.0}
SPECS = {
    "weighted_cross_entropy": dict(kind={"seg": L.LOSS_WCE, "bound": L.LOSS_BCE_LOGITS, "dist": L.LOSS_MSE, "color": L.LOSS_MSE}),
    "focal": dict(kind={"seg": L.LOSS_FOCAL_CE, "bound": L.LOSS_FOCAL_BCE, "dist": L.LOSS_MSE, "color": L.LOSS_MSE},
                  focal_gamma={"seg": 2.0, "bound": 2.0}),
}


def engine(name):
    eng = Engine(ModelConfig(input_shape=(PATCH, PATCH, CH), num_classes=NCLS, multitasking=True), dtype="bf16", seed=0)
    eng.compile(LossSpec(weight=dict(WEIGHT), class_weights=W, optimizer="adam", lr=1e-3, **SPECS[name]))
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
        sys.exit("bench_loss.py needs a GPU")
    lib = L.lib()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
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

    # ---- 1. kernels --------------------------------------------------------------------------------------------------------------------------
    HW = PATCH * PATCH
    M = BATCH * HW
    gen = torch.Generator(device="cuda").manual_seed(0)
    p = torch.softmax(2 * torch.randn((M, NCLS), device="cuda", generator=gen), 1).contiguous()
    y = torch.nn.functional.one_hot(torch.randint(0, NCLS, (M,), device="cuda", generator=gen), NCLS).float().contiguous()
    cw = torch.tensor(W + [0.0] * 8, device="cuda")
    dz = torch.empty((M, NCLS), device="cuda")
    per = torch.empty((M,), device="cuda")
    out = torch.zeros(1, dtype=torch.float64, device="cuda")
    d = lambda t: t.data_ptr()
    gs = 1.0 / M

    def loss_opts(kind, o):
        return lambda: lib.call("rua_pixel_loss_opts", kind, d(p), None, d(y), d(cw), None, C.byref(o), M, NCLS, d(out), d(per), s)

    def dz_opts(kind, act, o):
        return lambda: lib.call("rua_head_dz_opts", kind, act, d(p), d(y), None, d(cw), gs, BATCH, HW, NCLS, None, C.byref(o), d(dz), s)
    SM, SG = L.ACT_SOFTMAX, L.ACT_SIGMOID
    variants = [("weighted CE, smoothing 0.1", L.LOSS_WCE, SM, LS.to_struct(0.0, 0.1)),
                ("focal CE gamma 2", L.LOSS_FOCAL_CE, SM, LS.to_struct(2.0)),
                ("focal CE gamma 2, smoothing 0.1", L.LOSS_FOCAL_CE, SM, LS.to_struct(2.0, 0.1)),
                ("focal CE gamma 3.5", L.LOSS_FOCAL_CE, SM, LS.to_struct(3.5)),
                ("focal CE gamma 0", L.LOSS_FOCAL_CE, SM, LS.to_struct(0.0)),
                ("binary focal gamma 2, balanced", L.LOSS_FOCAL_BCE, SG, LS.to_struct(2.0, 0.0, 0.25, True)),
                ("binary focal gamma 3.5", L.LOSS_FOCAL_BCE, SG, LS.to_struct(3.5))]
    rows = [("loss: weighted CE (rua_pixel_loss)", 52 * M, lambda: lib.call("rua_pixel_loss", L.LOSS_WCE, d(p), None, d(y), d(cw), M, NCLS, d(out), d(per), s)),
            ("dz: weighted CE (rua_head_dz)", 72 * M, lambda: lib.call("rua_head_dz", L.LOSS_WCE, SM, d(p), d(y), None, d(cw), gs, BATCH, HW, NCLS, d(dz), s))]
    for name, kind, act, o in variants:
        rows.append(("loss: " + name, 52 * M, loss_opts(kind, o)))
        rows.append(("dz: " + name, 72 * M, dz_opts(kind, act, o)))
    res["kernels"] = dict(shape=[BATCH, PATCH, PATCH, NCLS], reps=args.reps)
    for _ in range(args.rounds):
        for name, nbytes, fn in rows:
            us = events(fn)
            r = res["kernels"].setdefault(name, dict(bytes=nbytes, us=[], TBps=[]))
            r["us"].append(round(us, 2)); r["TBps"].append(round(nbytes / us / 1e6, 3))
    assert torch.isfinite(dz).all() and torch.isfinite(per).all()
    del p, y, dz, per
    torch.cuda.empty_cache()
    if args.kernels_only:
        print(json.dumps(res))
        return

    # ---- 2. the whole step -----------------------------------------------------------------------------------------------------------------
    x, yb = make_batch(BATCH, PATCH, CH, NCLS, True, seed=1234)
    engines = {k: engine(k) for k in SPECS}
    for e in engines.values():
        e.train_step(x, yb, fetch=False)                    # warm-up + capture; the batch is resident from here on
        e.train_step(None, None, fetch=False)

    def timed(e):
        for _ in range(args.warmup):
            e.train_step(None, None, fetch=False)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.steps):
            e.train_step(None, None, fetch=False)
        e1.record()
        torch.cuda.synchronize()
        return round(e0.elapsed_time(e1) / args.steps, 4)
    steps = {k: [] for k in engines}
    for _ in range(args.rounds):
        for k, e in engines.items():
            steps[k].append(timed(e))
    res["step_ms"] = dict(shape=[BATCH, PATCH, PATCH, CH], dtype="bf16", path="graph", warmup=args.warmup, steps=args.steps, **steps,
                          dispatches_per_step={k: e.count_step_dispatches(BATCH) for k, e in engines.items()})
    assert all(np.isfinite(e.P.float().sum().item()) for e in engines.values())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
