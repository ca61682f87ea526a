"""What online hard example mining costs, at cfg3's seg head (batch 8, 256 x 256, 6 classes: 524288 pixels, a 2 MB loss map) and on the whole
cfg3 bf16 step.

1. rua_ohem_select through the C ABI (six launches: zero, three histogram passes, the mask pass, the finisher): microseconds per call (HIP
   events around REPS back-to-back calls) for a random map (the per-pixel map of weighted CE on random logits), an ALL-EQUAL map (every loss
   log 6 - the first steps of training, where every lane of a wave meets one histogram bin), the random map with 30 % void, at keep 0.25
   and 1.0; and rua_head_dz_multi_sel against rua_head_dz_multi_opts on the same four-head buffers.  The map is read four times and the mask
   written once: 17 bytes per pixel, 9 MB per call (21 with the void mask's byte read four times as well).
2. The whole bf16 graph step, batch resident, with the option off and on (seg and bound mining at keep 0.25): two engines in one process,
   alternated for ROUNDS rounds.

Prints one JSON line.  Usage: python tools/bench_ohem.py [--reps 50] [--rounds 3] [--steps 40] [--warmup 10] [--kernels-only]"""
import argparse
import ctypes as C
import json
import math
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
KIND = {"seg": L.LOSS_WCE, "bound": L.LOSS_BCE_LOGITS, "dist": L.LOSS_MSE, "color": L.LOSS_MSE}
SPECS = {"off": {}, "on": dict(ohem={"seg": LS.ohem_options(keep_q16=16384), "bound": LS.ohem_options(keep_q16=16384)})}


def engine(name):
    eng = Engine(ModelConfig(input_shape=(PATCH, PATCH, CH), num_classes=NCLS, multitasking=True), dtype="bf16", seed=0)
    eng.compile(LossSpec(kind=dict(KIND), weight=dict(WEIGHT), class_weights=W, optimizer="adam", lr=1e-3, **SPECS[name]))
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
        sys.exit("bench_ohem.py needs a GPU")
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
    p = torch.softmax(2 * torch.randn((M, NCLS), device="cuda", generator=gen), 1).contiguous()
    y = torch.nn.functional.one_hot(torch.randint(0, NCLS, (M,), device="cuda", generator=gen), NCLS).float().contiguous()
    cw = torch.tensor(W + [0.0] * 8, device="cuda")
    out = torch.zeros(1, dtype=torch.float64, device="cuda")
    random_map = torch.empty((M,), device="cuda")
    lib.call("rua_pixel_loss", L.LOSS_WCE, d(p), None, d(y), d(cw), M, NCLS, d(out), d(random_map), s)
    equal_map = torch.full((M,), math.log(NCLS), device="cuda")
    void = (torch.rand((M,), device="cuda", generator=gen) < 0.3).to(torch.uint8)
    nws = int(lib.raw("rua_ohem_workspace_bytes")(M))
    ws = torch.empty(nws // 8 + 1, dtype=torch.float64, device="cuda")
    drop = torch.empty((M,), dtype=torch.uint8, device="cuda")
    result = torch.zeros(C.sizeof(L.OhemResult) // 8, dtype=torch.float64, device="cuda")

    def select(lmap, vm, q16):
        o = LS.to_ohem_struct(LS.ohem_options(keep_q16=q16))
        return lambda: lib.call("rua_ohem_select", d(lmap), d(vm) if vm is not None else None, M, C.byref(o), None, 1.0, d(ws), nws, d(drop), d(out), d(result), s)
    rows = []
    for keep, q16 in (("0.25", 16384), ("1.0", 65536)):
        rows += [(f"select: random map, keep {keep}", 17 * M, select(random_map, None, q16)), (f"select: all-equal map, keep {keep}", 17 * M, select(equal_map, None, q16)),
                 (f"select: random map, 30 % void, keep {keep}", 21 * M, select(random_map, void, q16))]
    # the four heads' dz in one launch: rua_head_dz_multi_opts, and rua_head_dz_multi_sel with seg and bound taking the selection just made
    select(random_map, None, 16384)()
    dzs = [torch.empty((M, c), device="cuda") for c in (NCLS, NCLS, NCLS, 3)]
    p3, y3 = torch.rand((M, 3), device="cuda", generator=gen), torch.rand((M, 3), device="cuda", generator=gen)
    heads = (L.DzHead * 4)()
    for i, (kind, act, pp, yy) in enumerate(((L.LOSS_WCE, L.ACT_SOFTMAX, p, y), (L.LOSS_BCE_LOGITS, L.ACT_SIGMOID, p, y), (L.LOSS_MSE, L.ACT_SOFTMAX, p, y),
                                            (L.LOSS_MSE, L.ACT_SIGMOID, p3, y3))):
        h = heads[i]
        h.kind, h.act, h.p, h.y, h.coef, h.class_w, h.grad_scale, h.B, h.HW, h.C, h.dz = kind, act, d(pp), d(yy), None, d(cw), 1.0 / M, BATCH, HW, pp.shape[1], d(dzs[i])
    oarr, sel = (L.LossOpts * 4)(), (L.DzSel * 4)()
    for i in (0, 1):
        sel[i].drop_mask, sel[i].scale_dev = d(drop), d(result) + L.OhemResult.scale.offset
    nb = (72 * 3 + 36) * M
    rows += [("dz: four heads, rua_head_dz_multi_opts", nb, lambda: lib.call("rua_head_dz_multi_opts", heads, oarr, 4, None, s)),
             ("dz: four heads, rua_head_dz_multi_sel (seg, bound select)", nb, lambda: lib.call("rua_head_dz_multi_sel", heads, oarr, sel, 4, None, s))]
    res["kernels"] = dict(shape=[BATCH, PATCH, PATCH, NCLS], reps=args.reps, launches_per_select=6)
    for _ in range(args.rounds):
        for name, nbytes, fn in rows:
            us = events(fn)
            r = res["kernels"].setdefault(name, dict(bytes=nbytes, us=[], TBps=[]))
            r["us"].append(round(us, 2)); r["TBps"].append(round(nbytes / us / 1e6, 3))
    assert all(torch.isfinite(t).all() for t in dzs)
    del p, y, dzs, p3, y3
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
                          dispatches_per_step={k: e.count_step_dispatches(BATCH) for k, e in engines.items()}, report=engines["on"].ohem_report())
    assert all(np.isfinite(e.P.float().sum().item()) for e in engines.values())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
