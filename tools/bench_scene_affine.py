#!/usr/bin/env python
"""Random rotation, zoom and shift cut on the GPU: what rua_scene_windows_affine costs next to rua_scene_windows and next to the
copy a host-side augmentation would need.  Prints one JSON line.  The harness is tools/bench_scenes.py's (same scene, same timing
loops, same model and step variants); only the figures differ.

  windows_us     device events around `--reps` back-to-back calls after a warm-up, per call, B = 8 windows of 256 x 256 x 3 at random
                 origins of a seeded 6000 x 6000 x 3 scene with its class map:
                   scene_mixed     (a) rua_scene_windows, the eight codes mixed
                   affine_plain    (b) rua_scene_windows_affine on the same windows through affine_rows(...) with no jitter
                   affine_jitter   (c) ... with the CLI's default jitter (any angle, zoom 0.75 .. 1.33, shift up to 16 px)
                   affine_zoom025  (d) ... rotated 45 degrees at zoom 0.25 (zoom out: the taps of a tile spread over 181 x 181 px)
                   affine_zoom4    (d) ... rotated 45 degrees at zoom 4
                   pinned_copy     (e) the host-to-device copy of the same 2.1 MB batch (image + class map, pinned)
  step_ms        train_on_batch on the single-GPU graph path, bf16, 256 x 256 x 3, 6 classes, multitask, B = 8, `--warmup` untimed
                 and `--steps` timed steps per variant, every step fetching its metrics like the training loop:
                   scene     a SceneBatch: 8 table rows
                   affine    an AffineSceneBatch: the same rows under the default jitter
                   resident  no upload at all (train_step(None, None))
                 The variants alternate for `--rounds` rounds; every round's number is reported.
  conditions     kernel_time: (c) < (e).  step_time: in every round step_ms[affine] - step_ms[scene] <= (c) - (a) plus the largest
                 round-to-round spread of the scene variant - the new path adds its kernel time and nothing else.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _scene_bench import B, CIN, CLASSES, P, call_us, cfg3_model, clock_ms, make_scene  # noqa: E402

STRIDE = 32                                                    # the CLI's default: --aug_shift defaults to half of it


def windows_us(pool, size, reps):
    import torch
    from resunet_a_mltsk_keras_amd import _lib as L
    from resunet_a_mltsk_keras_amd import scenes
    lib, st = L.lib(), torch.cuda.current_stream()
    rng = np.random.default_rng(1)
    img_out = torch.empty((B, P, P, CIN), dtype=torch.uint8, device="cuda")
    cls_out = torch.empty((B, P, P), dtype=torch.uint8, device="cuda")
    nbytes = img_out.numel() + cls_out.numel()

    timed = lambda fn: call_us(fn, reps)

    def figure(name, t):
        t = np.ascontiguousarray(t, dtype=np.int32)
        us = timed(lambda: lib.call(name, pool.img_ptrs, pool.cls_ptrs, pool.heights, pool.widths, 1, t.ctypes.data, B, P, P, CIN,
                                    img_out.data_ptr(), cls_out.data_ptr(), ctypes.c_void_p(st.cuda_stream)))
        return {"us_per_call": round(us, 2), "bytes_written": nbytes}

    rows4 = np.array([[0, int(rng.integers(0, size - P + 1)), int(rng.integers(0, size - P + 1)), c] for c in range(8)], np.int32)
    angle, zoom, shift = scenes.Jitter(180.0, (0.75, 1.33), STRIDE / 2).draw(np.random.default_rng(2), B)
    out = {"scene_mixed": figure("rua_scene_windows", rows4),
           "affine_plain": figure("rua_scene_windows_affine", scenes.affine_rows(rows4, P)),
           "affine_jitter": figure("rua_scene_windows_affine", scenes.affine_rows(rows4, P, angle, zoom, shift)),
           "affine_zoom025": figure("rua_scene_windows_affine", scenes.affine_rows(rows4, P, 45.0, 0.25)),
           "affine_zoom4": figure("rua_scene_windows_affine", scenes.affine_rows(rows4, P, 45.0, 4.0))}
    hi, hc = torch.empty(img_out.shape, dtype=torch.uint8).pin_memory(), torch.empty(cls_out.shape, dtype=torch.uint8).pin_memory()

    def copy():
        img_out.copy_(hi, non_blocking=True)
        cls_out.copy_(hc, non_blocking=True)
    us = timed(copy)
    out["pinned_copy"] = {"us_per_call": round(us, 2), "bytes": nbytes, "GBps": round(nbytes / us / 1e3, 1)}
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
        sys.exit("bench_scene_affine.py needs a GPU")
    img, cls = make_scene(args.scene)
    pool = scenes.ScenePool([img], [cls], patch=P)
    wus = windows_us(pool, args.scene, args.reps)
    res = {"scene": [args.scene, args.scene, CIN], "windows_us": {"B": B, "patch": P, "reps": args.reps, **wus}}

    m = cfg3_model()
    loss = Tanimoto_dual_loss()
    m.compile(optimizer=Adam(lr=1e-3, beta_1=0.9), loss={h: loss for h in HEADS}, loss_weights={h: 1.0 for h in HEADS},
              metrics={"seg": ["accuracy"]})
    table = scenes.window_table([img.shape], P, STRIDE, True)
    order = np.random.default_rng(2).permutation(len(table))
    batches = [pool.batch(table[order[k * B:(k + 1) * B]]) for k in range(3)]        # what a shuffled epoch of the CLI hands out
    jittered = scenes.SceneLoader(pool, table, B, order=order[:3 * B], jitter=scenes.Jitter(180.0, (0.75, 1.33), STRIDE / 2), seed=0)
    affine = [b for b, _ in jittered]                                                # ... and what --random_aug yes makes of them

    def scene_step(k):
        m.train_on_batch(batches[k % 3], norm_type=1)

    def affine_step(k):
        m.train_on_batch(affine[k % 3], norm_type=1)

    def resident_step(k):
        m._sync_lr()
        m.engine.train_step(None, None)

    timed = lambda fn: round(clock_ms(fn, args.warmup, args.steps, takes_index=True)[0], 3)

    steps = {"scene": [], "affine": [], "resident": []}
    for _ in range(args.rounds):
        steps["scene"].append(timed(scene_step))
        steps["affine"].append(timed(affine_step))
        steps["resident"].append(timed(resident_step))
    res["step_ms"] = {"shape": [B, P, P, CIN], "classes": CLASSES, "dtype": "bf16", "path": "graph", "warmup": args.warmup, "steps": args.steps, **steps}
    res["host_bytes_per_step"] = {"scene": int(batches[0].rows.nbytes), "affine": int(affine[0].rows.nbytes)}

    a, c, e = (wus[k]["us_per_call"] for k in ("scene_mixed", "affine_jitter", "pinned_copy"))
    spread = max(steps["scene"]) - min(steps["scene"])
    added = [round(x - y, 3) for x, y in zip(steps["affine"], steps["scene"])]
    allowed = round((c - a) / 1e3 + spread, 3)
    res["conditions"] = {"kernel_time": {"affine_jitter_us": c, "pinned_copy_us": e, "holds": bool(c < e)},
                         "step_time": {"added_ms_per_round": added, "kernel_difference_ms": round((c - a) / 1e3, 4),
                                       "scene_spread_ms": round(spread, 3), "allowed_ms": allowed, "holds": bool(all(d <= allowed for d in added))}}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
