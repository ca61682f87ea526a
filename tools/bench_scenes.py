#!/usr/bin/env python
"""Training from resident scenes: what cutting the patches on the GPU costs and what it replaces.  Prints one JSON line.

  windows_us     rua_scene_windows alone: a seeded 6000 x 6000 x 3 scene with its class map, B = 8 windows of 256 x 256 at random
                 origins, device events around `--reps` back-to-back calls after a warm-up, per call: one figure per code 0..7
                 (all eight windows under that code) and one for a uniform mix of codes, each with the bytes read + written and
                 the resulting GB/s; `pinned_copy` is the host-to-device copy of the same 2.1 MB batch (image + class map, pinned)
                 that the call replaces, timed the same way in the same run
  step_ms        train_on_batch on the single-GPU graph path, bf16, 256 x 256 x 3, 6 classes, multitask, B = 8, `--warmup` untimed
                 and `--steps` timed steps per variant, every step fetching its metrics like the training loop:
                   compact   uint8 image + uint8 class map (pinned, a ring of 3) copied up, the targets built on the GPU
                   scene     a SceneBatch: 8 table rows, the patches cut from the resident scene on the GPU, the targets built there
                   resident  no upload at all (train_step(None, None): the batch already on the device, as bench.py measures)
                 The variants alternate for `--rounds` rounds; every round's number is reported.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from _scene_bench import B, CIN, CLASSES, P, call_us, cfg3_model, clock_ms, make_scene  # noqa: E402


def windows_us(pool, size, reps):
    import torch
    from resunet_a_mltsk_keras_amd import _lib as L
    lib, st = L.lib(), torch.cuda.current_stream()
    rng = np.random.default_rng(1)
    img_out = torch.empty((B, P, P, CIN), dtype=torch.uint8, device="cuda")
    cls_out = torch.empty((B, P, P), dtype=torch.uint8, device="cuda")
    moved = 2 * (img_out.numel() + cls_out.numel())              # every byte is read once and written once

    timed = lambda fn: call_us(fn, reps)

    def figure(codes):
        t = np.array([[0, int(rng.integers(0, size - P + 1)), int(rng.integers(0, size - P + 1)), c] for c in codes], np.int32)
        us = timed(lambda: lib.call("rua_scene_windows", pool.img_ptrs, pool.cls_ptrs, pool.heights, pool.widths, 1, t.ctypes.data, B, P, P, CIN,
                                    img_out.data_ptr(), cls_out.data_ptr(), ctypes.c_void_p(st.cuda_stream)))
        return {"us_per_call": round(us, 2), "bytes_read_and_written": moved, "GBps": round(moved / us / 1e3, 1)}

    out = {f"code{c}": figure([c] * B) for c in range(8)}
    out["mixed"] = figure(list(range(8)))
    hi, hc = torch.empty(img_out.shape, dtype=torch.uint8).pin_memory(), torch.empty(cls_out.shape, dtype=torch.uint8).pin_memory()

    def copy():
        img_out.copy_(hi, non_blocking=True)
        cls_out.copy_(hc, non_blocking=True)
    us = timed(copy)
    out["pinned_copy"] = {"us_per_call": round(us, 2), "bytes": moved // 2, "GBps": round(moved / 2 / us / 1e3, 1)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--scene", type=int, default=6000, help="scene edge in pixels")
    args = ap.parse_args()
    import torch
    from multitasking_utils import Tanimoto_dual_loss
    from resunet_a_mltsk_keras_amd import scenes
    from resunet_a_mltsk_keras_amd.engine import HEADS
    from resunet_a_mltsk_keras_amd.keras_api import Adam
    if not torch.cuda.is_available():
        sys.exit("bench_scenes.py needs a GPU")
    img, cls = make_scene(args.scene)
    pool = scenes.ScenePool([img], [cls], patch=P)
    res = {"scene": [args.scene, args.scene, CIN], "windows_us": {"B": B, "patch": P, "reps": args.reps, **windows_us(pool, args.scene, args.reps)}}

    m = cfg3_model()
    loss = Tanimoto_dual_loss()
    m.compile(optimizer=Adam(lr=1e-3, beta_1=0.9), loss={h: loss for h in HEADS}, loss_weights={h: 1.0 for h in HEADS},
              metrics={"seg": ["accuracy"]})
    table = scenes.window_table([img.shape], P, 32, True)
    order = np.random.default_rng(2).permutation(len(table))
    batches = [pool.batch(table[order[k * B:(k + 1) * B]]) for k in range(3)]        # what a shuffled epoch of the CLI hands out
    pin = lambda a: torch.from_numpy(a).pin_memory()
    ring_u8 = [tuple(pin(a) for a in b.host()) for b in batches]                     # the same patches as files would deliver them

    def compact_step(k):
        x, y = ring_u8[k % 3]
        m.train_on_batch(x, y, norm_type=1)

    def scene_step(k):
        m.train_on_batch(batches[k % 3], norm_type=1)

    def resident_step(k):
        m._sync_lr()
        m.engine.train_step(None, None)

    timed = lambda fn: round(clock_ms(fn, args.warmup, args.steps, takes_index=True)[0], 3)

    steps = {"compact": [], "scene": [], "resident": []}
    for _ in range(args.rounds):
        steps["compact"].append(timed(compact_step))
        steps["scene"].append(timed(scene_step))
        steps["resident"].append(timed(resident_step))
    res["step_ms"] = {"shape": [B, P, P, CIN], "classes": CLASSES, "dtype": "bf16", "path": "graph", "warmup": args.warmup, "steps": args.steps, **steps}
    res["host_bytes_per_step"] = {"compact": sum(t.numel() for t in ring_u8[0]), "scene": int(batches[0].rows.nbytes)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
