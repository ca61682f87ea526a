#!/usr/bin/env python
"""Copy-paste augmentation on the GPU: what rua_window_paste costs next to the rua_scene_windows call in front of it and next to the
pinned host-to-device copy a host-side paste would need, what ScenePool.object_bank costs once, and what the paste adds to a
training step.  Prints one JSON line.  The harness is tools/bench_scenes.py's (same scene, same timing loops, same model); the
class map gets 64 cars (12 x 24, class 4) and 16 buildings (150 x 150, class 5) stamped into its 16 x 16 blocks.

  windows_us     device events around `--reps` back-to-back calls after a warm-up, per call, for B = 8 and B = 32 windows of
                 256 x 256 x 3 at random origins of a seeded 6000 x 6000 x 3 scene:
                   scene_mixed        rua_scene_windows, the eight codes mixed (image and class map)
                   pinned_copy        the same batch's image and class bytes from pinned host memory to the device: the route a
                                      paste on the host would need
                   paste_0            rua_window_paste with no row: the argument checks alone, nothing is launched
                   paste_cars4/16     ... 4 / 16 cars per window, codes mixed, every class may be covered
                   paste_buildings2   ... 2 buildings per window, codes mixed
                   paste_cars16_plain / _transposing   ... 16 cars per window under the codes 0, 2, 3, 4 / 1, 5, 6, 7 only
  object_bank    ScenePool.object_bank of the scene (classes 4 and 5), by the host clock, `--rounds` times
  step_ms        train_on_batch on the single-GPU graph path, bf16, 256 x 256 x 3, 6 classes, multitask, B = 8, `--warmup` untimed
                 and `--steps` timed steps per variant, every step fetching its metrics like the training loop:
                   off   SceneBatches without a paste table: the launches of a step as it was
                   on    the same batches with the tables SceneLoader(paste=CopyPaste([4])) draws
                 The variants alternate for `--rounds` rounds; every round's number is reported.
  conditions     cars4_below_pinned_copy: paste_cars4 < pinned_copy at B = 8 and at B = 32;
                 step_within_kernel_plus_spread: in every round, on - off <= the kernel's time on the `on` tables + the largest
                 spread (max - min) among the off rounds.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _scene_bench import B, CIN, CLASSES, P, call_us, cfg3_model, clock_ms, make_scene  # noqa: E402

STRIDE = 32
CAR, BUILDING = (12, 24), (150, 150)
PLAIN, TRANSPOSING = (0, 2, 3, 4), (1, 5, 6, 7)


def stamp_objects(cls, size):
    """64 cars and 16 buildings at seeded places, each inside a frame of class 0 that keeps it an object of its own."""
    rng = np.random.default_rng(7)
    for (h, w), c, count in ((BUILDING, 5, 16), (CAR, 4, 64)):
        for _ in range(count):
            i, j = int(rng.integers(1, size - h - 1)), int(rng.integers(1, size - w - 1))
            cls[i - 1:i + h + 1, j - 1:j + w + 1] = 0
            cls[i:i + h, j:j + w] = c
    return cls


def table_of(bank_rows, bank, nb, per_window, codes, rng):
    """per_window objects of `bank_rows` in each of nb windows, fully inside, under the given codes."""
    M = nb * per_window
    k = rng.choice(bank_rows, M)
    code = rng.choice(np.asarray(codes), M)
    h, w = bank[k, 6] - bank[k, 4] + 1, bank[k, 7] - bank[k, 5] + 1
    tr = np.isin(code, TRANSPOSING)
    th, tw = np.where(tr, w, h), np.where(tr, h, w)
    from resunet_a_mltsk_keras_amd import scenes
    return scenes.paste_rows(bank, np.repeat(np.arange(nb), per_window), k, code, (rng.random(M) * (P - th + 1)).astype(np.int64),
                             (rng.random(M) * (P - tw + 1)).astype(np.int64))


def paste_call(lib, pool, img, cls, nb, table, st):
    t = np.ascontiguousarray(table, dtype=np.int32)
    return lambda: lib.call("rua_window_paste", img.data_ptr(), cls.data_ptr(), nb, P, P, CIN, CLASSES, pool.img_ptrs, pool.cls_ptrs, pool.inst_ptrs,
                            pool.heights, pool.widths, 1, t.ctypes.data if len(t) else None, len(t), ctypes.c_void_p(st.cuda_stream))


def windows_us(pool, size, reps, nb):
    import torch
    from resunet_a_mltsk_keras_amd import _lib as L
    lib, st = L.lib(), torch.cuda.current_stream()
    rng = np.random.default_rng(1)
    img_out = torch.empty((nb, P, P, CIN), dtype=torch.uint8, device="cuda")
    cls_out = torch.empty((nb, P, P), dtype=torch.uint8, device="cuda")
    rows4 = np.array([[0, int(rng.integers(0, size - P + 1)), int(rng.integers(0, size - P + 1)), k % 8] for k in range(nb)], np.int32)

    def cut():
        lib.call("rua_scene_windows", pool.img_ptrs, pool.cls_ptrs, pool.heights, pool.widths, 1, rows4.ctypes.data, nb, P, P, CIN,
                 img_out.data_ptr(), cls_out.data_ptr(), ctypes.c_void_p(st.cuda_stream))

    nbytes = img_out.numel() + cls_out.numel()
    out = {"scene_mixed": {"us_per_call": round(call_us(cut, reps), 2), "bytes_written": nbytes}}
    host_img, host_cls = img_out.cpu().pin_memory(), cls_out.cpu().pin_memory()

    def copy():
        img_out.copy_(host_img, non_blocking=True)
        cls_out.copy_(host_cls, non_blocking=True)

    us = call_us(copy, reps)
    out["pinned_copy"] = {"us_per_call": round(us, 2), "bytes_moved": nbytes, "GBps": round(nbytes / us / 1e3, 1)}
    bank = pool.bank
    h, w = bank[:, 6] - bank[:, 4] + 1, bank[:, 7] - bank[:, 5] + 1
    cars, buildings = np.flatnonzero((h == CAR[0]) & (w == CAR[1])), np.flatnonzero((h == BUILDING[0]) & (w == BUILDING[1]))
    every = PLAIN + TRANSPOSING
    tables = {"paste_0": np.zeros((0, 16), np.int32), "paste_cars4": table_of(cars, bank, nb, 4, every, rng), "paste_cars16": table_of(cars, bank, nb, 16, every, rng),
              "paste_buildings2": table_of(buildings, bank, nb, 2, every, rng), "paste_cars16_plain": table_of(cars, bank, nb, 16, PLAIN, rng),
              "paste_cars16_transposing": table_of(cars, bank, nb, 16, TRANSPOSING, rng)}
    for name, t in tables.items():
        cut()
        us = call_us(paste_call(lib, pool, img_out, cls_out, nb, t, st), reps)
        out[name] = {"us_per_call": round(us, 2), "rows": int(len(t)), "crop_pixels": int((t[:, 8].astype(np.int64) * t[:, 9]).sum())}
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
    from resunet_a_mltsk_keras_amd import _lib as L
    from resunet_a_mltsk_keras_amd import scenes
    from resunet_a_mltsk_keras_amd.engine import HEADS
    from resunet_a_mltsk_keras_amd.keras_api import Adam
    if not torch.cuda.is_available():
        sys.exit("bench_scene_paste.py needs a GPU")
    img, cls = make_scene(args.scene)
    cls = stamp_objects(cls, args.scene)
    pool = scenes.ScenePool([img], [cls], patch=P)
    bank_ms = []
    for _ in range(args.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        bank = pool.object_bank(CLASSES, [4, 5])
        torch.cuda.synchronize()
        bank_ms.append(round((time.perf_counter() - t0) * 1e3, 2))
    res = {"scene": [args.scene, args.scene, CIN],
           "object_bank": {"ms": bank_ms, "objects": int(len(bank)), "resident_bytes": int(sum(t.numel() * 4 for t in pool.inst_dev))},
           "windows_us": {"patch": P, "reps": args.reps, **{f"B{nb}": windows_us(pool, args.scene, args.reps, nb) for nb in (8, 32)}}}

    m = cfg3_model()
    loss = Tanimoto_dual_loss()
    m.compile(optimizer=Adam(lr=1e-3, beta_1=0.9), loss={h: loss for h in HEADS}, loss_weights={h: 1.0 for h in HEADS},
              metrics={"seg": ["accuracy"]})
    table = scenes.window_table([img.shape], P, STRIDE, True)
    order = np.random.default_rng(2).permutation(len(table))
    off = [b for b, _ in scenes.SceneLoader(pool, table, B, order=order[:3 * B])]                    # what a shuffled epoch of the CLI hands out
    on = [b for b, _ in scenes.SceneLoader(pool, table, B, order=order[:3 * B], paste=scenes.CopyPaste([4]), seed=0)]    # ... under --paste_aug yes --paste_classes 4

    timed = lambda batches: round(clock_ms(lambda k: m.train_on_batch(batches[k % 3], norm_type=1), args.warmup, args.steps, takes_index=True)[0], 3)
    steps = {"off": [], "on": []}
    for _ in range(args.rounds):
        steps["off"].append(timed(off))
        steps["on"].append(timed(on))
    st = torch.cuda.current_stream()
    buf_img, buf_cls = torch.zeros((B, P, P, CIN), dtype=torch.uint8, device="cuda"), torch.zeros((B, P, P), dtype=torch.uint8, device="cuda")
    kernel_ms = float(np.mean([call_us(paste_call(L.lib(), pool, buf_img, buf_cls, B, b.paste, st), args.reps) for b in on])) / 1e3
    res["step_ms"] = {"shape": [B, P, P, CIN], "classes": CLASSES, "dtype": "bf16", "path": "graph", "warmup": args.warmup, "steps": args.steps, **steps}
    res["host_bytes_per_step"] = {"off": int(off[0].rows.nbytes), "on": [int(b.rows.nbytes + b.paste.nbytes) for b in on]}
    res["added_ms_per_round"] = [round(a - b, 3) for a, b in zip(steps["on"], steps["off"])]
    res["paste_kernel_ms_on_tables"] = round(kernel_ms, 4)
    spread = max(steps["off"]) - min(steps["off"])
    w = res["windows_us"]
    res["conditions"] = {"cars4_below_pinned_copy": all(w[k]["paste_cars4"]["us_per_call"] < w[k]["pinned_copy"]["us_per_call"] for k in ("B8", "B32")),
                         "off_spread_ms": round(spread, 3),
                         "step_within_kernel_plus_spread": all(d <= kernel_ms + spread for d in res["added_ms_per_round"])}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
