#!/usr/bin/env python
"""Class counts of scene windows on the GPU: what rua_scene_class_counts costs and what it replaces.  Prints one JSON line and writes
it to `--out` (default profiles/scenes/bench_scene_counts.json).

Three seeded 6000 x 6000 class maps with 6 classes live in one pool: `blocky` (uniform 16 x 16 regions, as real references are
made of uniform regions of a few hundred pixels), `noise` (every pixel drawn on its own) and `uniform` (one class everywhere: every
count of a window lands in one cell).  Device events around `--reps` back-to-back calls after a warm-up, `--rounds` times; every
round's ms per call is reported, `ms` is their median and `spread_ms` their max - min.

  table_blocky    (a) the reference's distinct windows - patch 256, stride 32, 32 400 rows - with bytes read / time next to it
  table_noise     (b) the same table on the noise map ...
  table_uniform       ... and on the uniform map
  batch8          (c) a batch of 8 windows at random origins of the blocky map (us per call)
  host            (d) scenes.host_class_counts on the blocky map, timed on `--host_rows` evenly spaced rows of the table and scaled
                      to all of it (the time is linear in the rows: one bincount per window)
  conditions      gpu_faster_than_host: (a) < (d);  content_independent: uniform ms <= noise ms + the noise run's spread
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

from _scene_bench import CLASSES, P, make_maps, rounds_ms  # noqa: E402

STRIDE = 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="back-to-back calls per round on the whole table")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--kreps", type=int, default=200, help="back-to-back calls per round on the batch of 8")
    ap.add_argument("--host_rows", type=int, default=400)
    ap.add_argument("--scene", type=int, default=6000, help="scene edge in pixels")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scenes", "bench_scene_counts.json"))
    args = ap.parse_args()
    import torch
    from resunet_a_mltsk_keras_amd import _lib as L
    from resunet_a_mltsk_keras_amd import scenes
    if not torch.cuda.is_available():
        sys.exit("bench_scene_counts.py needs a GPU")
    maps = make_maps(args.scene)
    names = list(maps)
    one = np.zeros((args.scene, args.scene, 1), np.uint8)         # the images are not read
    pool = scenes.ScenePool([one] * len(names), [maps[n] for n in names], patch=P)
    lib, st = L.lib(), torch.cuda.current_stream()
    table = scenes.window_table([(args.scene, args.scene)], P, STRIDE, False)
    N = len(table)
    out = torch.empty((N, CLASSES + 1), dtype=torch.int32, device="cuda")

    def call(t):
        lib.call("rua_scene_class_counts", pool.cls_ptrs, pool.heights, pool.widths, len(pool), t.ctypes.data, len(t), P, P, CLASSES,
                 out.data_ptr(), ctypes.c_void_p(st.cuda_stream))

    timed = lambda t, reps: rounds_ms(lambda: call(t), args.rounds, reps)

    def on(name, rows):
        t = rows.copy()
        t[:, 0] = names.index(name)
        return np.ascontiguousarray(t)

    res = {"scene": [args.scene, args.scene], "patch": P, "stride": STRIDE, "classes": CLASSES, "rows": N, "reps": args.reps, "rounds": args.rounds}
    want = None
    for name in names:
        t = on(name, table)
        ms = timed(t, args.reps)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert (got.sum(1) == P * P).all()
        if name == "blocky":
            want = got
        res["table_" + name] = {"ms_per_call": [round(v, 3) for v in ms], "ms": round(float(np.median(ms)), 3), "spread_ms": round(max(ms) - min(ms), 3),
                                "bytes_read": N * P * P, "GBps": round(N * P * P / float(np.median(ms)) / 1e6, 1)}
    rng = np.random.default_rng(1)
    t8 = np.array([[0, int(rng.integers(0, args.scene - P + 1)), int(rng.integers(0, args.scene - P + 1)), 0] for _ in range(8)], np.int32)
    us = [v * 1e3 for v in timed(t8, args.kreps)]
    res["batch8"] = {"us_per_call": [round(v, 2) for v in us], "us": round(float(np.median(us)), 2), "kreps": args.kreps, "bytes_read": 8 * P * P}
    sub = table[np.linspace(0, N - 1, min(args.host_rows, N)).astype(np.int64)]
    t0 = time.perf_counter()
    host = scenes.host_class_counts([maps["blocky"]], sub, P, CLASSES)
    dt = time.perf_counter() - t0
    assert np.array_equal(host, want[np.linspace(0, N - 1, min(args.host_rows, N)).astype(np.int64)])       # the same numbers, while we are here
    res["host"] = {"rows_timed": len(sub), "ms_timed": round(dt * 1e3, 1), "ms_scaled_to_table": round(dt * 1e3 * N / len(sub), 1),
                   "note": "host_class_counts timed on rows_timed evenly spaced rows of the table, scaled linearly to all rows"}
    a, d = res["table_blocky"]["ms"], res["host"]["ms_scaled_to_table"]
    nz, un = res["table_noise"], res["table_uniform"]
    res["conditions"] = {"gpu_faster_than_host": bool(a < d), "host_over_gpu": round(d / a, 1),
                         "content_independent": bool(un["ms"] <= nz["ms"] + nz["spread_ms"]),
                         "uniform_ms": un["ms"], "noise_ms_plus_spread": round(nz["ms"] + nz["spread_ms"], 3)}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
