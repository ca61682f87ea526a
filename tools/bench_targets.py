#!/usr/bin/env python
"""Compact training path: what building the targets on the GPU costs and what it saves.  Prints one JSON line.

  synthesis_us   rua_multitask_targets alone (x, seg, bound, dist, color from uint8 image + class map), device events around
                 `--reps` back-to-back calls after a warm-up, per call: cfg3 (B = 8, 256 x 256, 6 classes) and cfg4 (B = 4, 512 x 512)
  step_ms        train_on_batch on the single-GPU graph path, bf16, 256 x 256 x 3 (RGB: the colour target needs 3 bands), 6 classes,
                 multitask, B = 8, from pinned host batches (a ring of 3, as the loader hands them out), `--warmup` untimed and
                 `--steps` timed steps per variant, every step fetching its metrics like the training loop:
                   float_upload  the reference's layout: float32 x + four float32 targets (~50 MB per step) copied up
                   compact       uint8 image + uint8 class map (~2 MB) copied up, the targets built on the GPU
                   resident      no upload at all (train_step(None, None): the batch already on the device, as bench.py measures)
                 The variants alternate for `--rounds` rounds; every round's number is reported.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthesis_us(B, S, C, reps):
    import torch
    from resunet_a_mltsk_keras_amd import _lib as L
    rng = np.random.default_rng(0)
    img = torch.from_numpy(rng.integers(0, 256, (B, S, S, 3)).astype(np.uint8)).cuda()
    f = rng.integers(0, C, (B, S // 8 + 1, S // 8 + 1))
    cls = torch.from_numpy(np.kron(f, np.ones((1, 8, 8), np.int64))[:, :S, :S].astype(np.uint8)).cuda()
    out = {h: torch.empty((B, S, S, c), device="cuda") for h, c in (("x", 3), ("seg", C), ("bound", C), ("dist", C), ("color", 3))}
    nb = int(L.lib().raw("rua_targets_scratch_bytes")(B, C))
    scratch = torch.empty((nb,), dtype=torch.uint8, device="cuda")
    lib, st = L.lib(), torch.cuda.current_stream()

    def call():
        lib.call("rua_multitask_targets", img.data_ptr(), cls.data_ptr(), B, S, S, 3, C, 1, out["x"].data_ptr(), out["seg"].data_ptr(),
                 out["bound"].data_ptr(), out["dist"].data_ptr(), out["color"].data_ptr(), scratch.data_ptr(), nb, ctypes.c_void_p(st.cuda_stream))
    for _ in range(5):
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        call()
    e1.record()
    torch.cuda.synchronize()
    written = sum(t.numel() * 4 for t in out.values())
    us = e0.elapsed_time(e1) * 1e3 / reps
    return {"B": B, "size": S, "classes": C, "us_per_call": round(us, 2), "bytes_written": written,
            "write_GBps": round(written / us / 1e3, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    import torch
    from multitasking_utils import Tanimoto_dual_loss
    from resunet_a_mltsk_keras_amd import compact
    from resunet_a_mltsk_keras_amd.engine import HEADS, ModelConfig
    from resunet_a_mltsk_keras_amd.keras_api import Adam, Model
    if not torch.cuda.is_available():
        sys.exit("bench_targets.py needs a GPU")
    res = {"synthesis_us": {"cfg3": synthesis_us(8, 256, 6, args.reps), "cfg4": synthesis_us(4, 512, 6, args.reps)}}

    B, S, C = 8, 256, 6
    m = Model(ModelConfig(input_shape=(S, S, 3), num_classes=C, multitasking=True), dtype="bf16", seed=0)
    loss = Tanimoto_dual_loss()
    m.compile(optimizer=Adam(lr=1e-3, beta_1=0.9), loss={h: loss for h in HEADS}, loss_weights={h: 1.0 for h in HEADS},
              metrics={"seg": ["accuracy"]})
    rng = np.random.default_rng(1)
    ring_u8, ring_f32 = [], []
    for k in range(3):
        img = rng.integers(0, 256, (B, S, S, 3)).astype(np.uint8)
        f = rng.integers(0, C, (B, S // 16 + 1, S // 16 + 1))
        cls = np.kron(f, np.ones((1, 16, 16), np.int64))[:, :S, :S].astype(np.uint8)
        t = compact.host_targets(img, cls, C, 1)
        pin = lambda a: torch.from_numpy(a).pin_memory()
        ring_u8.append((pin(img), pin(cls)))
        ring_f32.append((pin(t["x"]), {h: pin(t[h]) for h in HEADS}))

    def float_step(k):
        x, y = ring_f32[k % 3]
        m.train_on_batch(x, y)

    def compact_step(k):
        x, y = ring_u8[k % 3]
        m.train_on_batch(x, y, norm_type=1)

    def resident_step(k):
        m._sync_lr()
        m.engine.train_step(None, None)

    def timed(fn):
        for k in range(args.warmup):
            fn(k)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(args.steps):
            fn(k)
        torch.cuda.synchronize()
        return round((time.perf_counter() - t0) * 1e3 / args.steps, 3)

    steps = {"float_upload": [], "compact": [], "resident": []}
    for _ in range(args.rounds):
        steps["float_upload"].append(timed(float_step))
        steps["compact"].append(timed(compact_step))
        steps["resident"].append(timed(resident_step))
    res["step_ms"] = {"shape": [B, S, S, 3], "classes": C, "dtype": "bf16", "path": "graph", "warmup": args.warmup, "steps": args.steps, **steps}
    res["upload_MB_per_step"] = {"float_upload": round(sum(t.numel() * t.element_size() for t in [ring_f32[0][0], *ring_f32[0][1].values()]) / 1e6, 2),
                                 "compact": round(sum(t.numel() for t in ring_u8[0]) / 1e6, 2)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
