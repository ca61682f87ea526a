#!/usr/bin/env python
"""Colour, tone and noise jitter of the staged windows on the GPU: what rua_window_photometric costs next to the rua_scene_windows
call in front of it, and what it adds to a training step.  Prints one JSON line.  The harness is tools/bench_scenes.py's (same
scene, same timing loops, same model); only the figures differ.

  windows_us     device events around `--reps` back-to-back calls after a warm-up, per call, for B = 8 and B = 32 windows of
                 256 x 256 x 3 at random origins of a seeded 6000 x 6000 x 3 scene:
                   scene_mixed     rua_scene_windows, the eight codes mixed (image and class map)
                   photo_identity  rua_window_photometric in place, identity rows: the argument checks alone, nothing is launched
                   photo_colour    ... rows of PhotoJitter with the noise off: colour matrix and tone
                   photo_noise     ... rows of PhotoJitter as the CLI draws them: colour, tone and noise
                 GBps counts the bytes read plus the bytes written.
  step_ms        train_on_batch on the single-GPU graph path, bf16, 256 x 256 x 3, 6 classes, multitask, B = 8, `--warmup` untimed
                 and `--steps` timed steps per variant, every step fetching its metrics like the training loop:
                   off   SceneBatches without a photo table: the launches of a step as it was
                   on    the same batches with the tables SceneLoader(photo=PhotoJitter()) draws
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _scene_bench import B, CIN, CLASSES, P, call_us, cfg3_model, clock_ms, make_scene  # noqa: E402

STRIDE = 32


def windows_us(pool, size, reps, nb):
    import torch
    from resunet_a_mltsk_keras_amd import _lib as L
    from resunet_a_mltsk_keras_amd import scenes
    lib, st = L.lib(), torch.cuda.current_stream()
    rng = np.random.default_rng(1)
    img_out = torch.empty((nb, P, P, CIN), dtype=torch.uint8, device="cuda")
    cls_out = torch.empty((nb, P, P), dtype=torch.uint8, device="cuda")
    rows4 = np.array([[0, int(rng.integers(0, size - P + 1)), int(rng.integers(0, size - P + 1)), k % 8] for k in range(nb)], np.int32)

    def cut():
        lib.call("rua_scene_windows", pool.img_ptrs, pool.cls_ptrs, pool.heights, pool.widths, 1, rows4.ctypes.data, nb, P, P, CIN,
                 img_out.data_ptr(), cls_out.data_ptr(), ctypes.c_void_p(st.cuda_stream))

    out = {"scene_mixed": {"us_per_call": round(call_us(cut, reps), 2), "bytes_written": img_out.numel() + cls_out.numel()}}
    tables = {"photo_identity": scenes.photo_rows(nb),
              "photo_colour": scenes.PhotoJitter(noise_sigma=(0.0, 0.0)).draw(np.random.default_rng(2), nb, CIN),
              "photo_noise": scenes.PhotoJitter().draw(np.random.default_rng(2), nb, CIN)}
    for name, t in tables.items():
        t = np.ascontiguousarray(t, dtype=np.int32)
        us = call_us(lambda: lib.call("rua_window_photometric", img_out.data_ptr(), img_out.data_ptr(), nb, P, P, CIN, t.ctypes.data,
                                      ctypes.c_void_p(st.cuda_stream)), reps)
        moved = 0 if name == "photo_identity" else 2 * img_out.numel()
        out[name] = {"us_per_call": round(us, 2), "bytes_moved": moved, "GBps": round(moved / us / 1e3, 1)}
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
        sys.exit("bench_scene_photo.py needs a GPU")
    img, cls = make_scene(args.scene)
    pool = scenes.ScenePool([img], [cls], patch=P)
    res = {"scene": [args.scene, args.scene, CIN],
           "windows_us": {"patch": P, "reps": args.reps, **{f"B{nb}": windows_us(pool, args.scene, args.reps, nb) for nb in (8, 32)}}}

    m = cfg3_model()
    loss = Tanimoto_dual_loss()
    m.compile(optimizer=Adam(lr=1e-3, beta_1=0.9), loss={h: loss for h in HEADS}, loss_weights={h: 1.0 for h in HEADS},
              metrics={"seg": ["accuracy"]})
    table = scenes.window_table([img.shape], P, STRIDE, True)
    order = np.random.default_rng(2).permutation(len(table))
    off = [b for b, _ in scenes.SceneLoader(pool, table, B, order=order[:3 * B])]                    # what a shuffled epoch of the CLI hands out
    on = [b for b, _ in scenes.SceneLoader(pool, table, B, order=order[:3 * B], photo=scenes.PhotoJitter(), seed=0)]    # ... under --photo_aug yes

    timed = lambda batches: round(clock_ms(lambda k: m.train_on_batch(batches[k % 3], norm_type=1), args.warmup, args.steps, takes_index=True)[0], 3)
    steps = {"off": [], "on": []}
    for _ in range(args.rounds):
        steps["off"].append(timed(off))
        steps["on"].append(timed(on))
    res["step_ms"] = {"shape": [B, P, P, CIN], "classes": CLASSES, "dtype": "bf16", "path": "graph", "warmup": args.warmup, "steps": args.steps, **steps}
    res["host_bytes_per_step"] = {"off": int(off[0].rows.nbytes), "on": int(on[0].rows.nbytes + on[0].photo.nbytes)}
    res["added_ms_per_round"] = [round(a - b, 3) for a, b in zip(steps["on"], steps["off"])]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
