"""What the Lovasz-Softmax loss costs, at cfg3's seg and boundary heads (batch 8, 256 x 256, 6 classes: 524288 pixels, 3.1 M (key, pixel) pairs)
and on the whole cfg3 bf16 step.

1. rua_lovasz_grad (18 launches: zero, keys, four digit passes of histogram / scan / scatter, the prefix count in three, the finisher) and
   rua_lovasz_dz through the C ABI: microseconds per call (HIP events around REPS back-to-back calls) for a random map, the UNIFORM map
   p = 1 / C (the first steps of training: every key of a class equal within the foreground and the background group, every lane of a wave on
   one digit) and the random map with 30 % void, on the softmax head and on the sigmoid head.  Next to them rua_pixel_loss + rua_head_dz of
   weighted CE on the same buffers.  Bytes per pair: the sort reads the pairs for the histogram, reads and writes them in the scatter, in each of
   the four passes - 96 B -, the key pass reads p and y and writes the pair (16 B), the prefix count reads the pairs twice (16 B) and dp is
   written (4 B): 132 B per pair and call, 0.42 GB.
2. The whole bf16 graph step, batch resident, under weighted CE / BCE (the option off) and under the Lovasz loss on seg and bound: two engines in
   one process, alternated for ROUNDS rounds.

Prints one JSON line.  Usage: python tools/bench_lovasz.py [--reps 20] [--rounds 3] [--steps 40] [--warmup 10] [--kernels-only]"""
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
SPECS = {"weighted_cross_entropy": dict(kind={"seg": L.LOSS_WCE, "bound": L.LOSS_BCE_LOGITS, "dist": L.LOSS_MSE, "color": L.LOSS_MSE}, class_weights=W),
         "lovasz": dict(kind={"seg": L.LOSS_LOVASZ, "bound": L.LOSS_LOVASZ, "dist": L.LOSS_MSE, "color": L.LOSS_MSE})}
SORT_BYTES, CALL_BYTES = 96, 132                            # per pair: the four digit passes; the whole rua_lovasz_grad call


def engine(name):
    eng = Engine(ModelConfig(input_shape=(PATCH, PATCH, CH), num_classes=NCLS, multitasking=True), dtype="bf16", seed=0)
    eng.compile(LossSpec(weight=dict(WEIGHT), optimizer="adam", lr=1e-3, **SPECS[name]))
    return eng


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--kernels-only", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_lovasz.py needs a GPU")
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
    d = lambda t: t.data_ptr()
    z = 2 * torch.randn((M, NCLS), device="cuda", generator=gen)
    maps = {"seg": dict(act=L.ACT_SOFTMAX, p=torch.softmax(z, 1).contiguous(),
                        y=torch.nn.functional.one_hot(torch.randint(0, NCLS, (M,), device="cuda", generator=gen), NCLS).float().contiguous(),
                        uniform=torch.full((M, NCLS), 1.0 / NCLS, device="cuda")),
            "bound": dict(act=L.ACT_SIGMOID, p=torch.sigmoid(z).contiguous(), y=(torch.rand((M, NCLS), device="cuda", generator=gen) < 0.1).float().contiguous(),
                          uniform=torch.full((M, NCLS), 0.5, device="cuda"))}
    cw = torch.tensor(W + [0.0] * 8, device="cuda")
    out = torch.zeros(1, dtype=torch.float64, device="cuda")
    void = (torch.rand((M,), device="cuda", generator=gen) < 0.3).to(torch.uint8)
    nws = int(lib.raw("rua_lovasz_workspace_bytes")(M, NCLS))
    ws = torch.empty(nws // 8 + 1, dtype=torch.float64, device="cuda")
    dp, dz, per = torch.empty((M, NCLS), device="cuda"), torch.empty((M, NCLS), device="cuda"), torch.empty((M,), device="cuda")
    result = torch.zeros(C.sizeof(L.LovaszResult) // 8, dtype=torch.float64, device="cuda")
    scale = d(result) + L.LovaszResult.scale.offset
    pairs = M * NCLS
    rows = []
    for head, m in maps.items():
        def grad(p, vm, m=m):
            return lambda: lib.call("rua_lovasz_grad", d(p), d(m["y"]), d(vm) if vm is not None else None, M, NCLS, 0, 1.0, d(ws), nws, d(out), d(dp), None, d(result), s)
        rows += [(f"{head}: rua_lovasz_grad, random map", CALL_BYTES * pairs, grad(m["p"], None)),
                 (f"{head}: rua_lovasz_grad, uniform map", CALL_BYTES * pairs, grad(m["uniform"], None)),
                 (f"{head}: rua_lovasz_grad, random map, 30 % void", CALL_BYTES * pairs + 2 * M, grad(m["p"], void)),
                 (f"{head}: rua_lovasz_dz", 12 * pairs, lambda m=m: lib.call("rua_lovasz_dz", m["act"], d(m["p"]), d(dp), scale, M, NCLS, d(dz), s))]
        kind = L.LOSS_WCE if head == "seg" else L.LOSS_BCE_LOGITS
        rows += [(f"{head}: rua_pixel_loss, {'weighted CE' if head == 'seg' else 'BCE'}", 8 * pairs + 4 * M,
                  lambda m=m, kind=kind: lib.call("rua_pixel_loss", kind, d(m["p"]), d(m["p"]), d(m["y"]), d(cw), M, NCLS, d(out), d(per), s)),
                 (f"{head}: rua_head_dz, {'weighted CE' if head == 'seg' else 'BCE'}", 12 * pairs,
                  lambda m=m, kind=kind: lib.call("rua_head_dz", kind, m["act"], d(m["p"]), d(m["y"]), None, d(cw), 1.0 / M, BATCH, HW, NCLS, d(dz), s))]
    res["kernels"] = dict(shape=[BATCH, PATCH, PATCH, NCLS], reps=args.reps, launches_per_grad=18, tile=int(lib.raw("rua_lovasz_tile")()), pairs=pairs,
                          sort_bytes=SORT_BYTES * pairs, call_bytes=CALL_BYTES * pairs, workspace_bytes=nws)
    for _ in range(args.rounds):
        for name, nbytes, fn in rows:
            us = events(fn)
            r = res["kernels"].setdefault(name, dict(bytes=nbytes, us=[], TBps=[]))
            r["us"].append(round(us, 2)); r["TBps"].append(round(nbytes / us / 1e6, 3))
    assert torch.isfinite(dz).all() and torch.isfinite(dp).all()
    res["kernels"]["last_result"] = {k: (float(v) if k == "scale" else v) for k, v in LS.lovasz_result(result.cpu().numpy().tobytes()).items() if k in ("n_valid", "n_cls", "scale", "loss")}
    del maps, dp, dz, ws, z
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
                          dispatches_per_step={k: e.count_step_dispatches(BATCH) for k, e in engines.items()}, report=engines["lovasz"].lovasz_report())
    assert all(np.isfinite(e.P.float().sum().item()) for e in engines.values())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
