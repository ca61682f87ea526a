#!/usr/bin/env python
"""The eroded ground truth on the GPU: what rua_scene_erode costs and what it replaces.  Prints one JSON line and writes it to `--out`
(default profiles/scenes/bench_scene_erode.json).

Three seeded 6000 x 6000 class maps with 6 classes - `blocky` (uniform 16 x 16 regions, as real references are made of uniform
regions), `noise` (every pixel drawn on its own: everything erodes) and `uniform` (one class: nothing erodes, every count lands in one
cell) - and a seeded random prediction map.  Device events around `--reps` back-to-back calls after a warm-up, `--rounds` times; every
round's ms per call is reported, `ms` is their median and `spread_ms` their max - min.

  map_r3          the eroded map alone at radius 3 on the blocky map (reads cls, writes out)
  matrix_r3       the confusion matrix alone at radius 3 (reads cls and pred)
  both_r3         both in one pass (reads cls and pred, writes out), also on the noise and the uniform map
  both_r1 both_r16  the same at the smallest and the largest radius
  pool_both_r3    one call on all three maps, each with a prediction and an output of its own: 324 MB touched, more than the 256 MiB
                  Infinity Cache holds, where a single map's 108 MB may be served from it between back-to-back calls
  bytes, GBps, floor_ms, share_of_floor   next to the radius-3 figures: the bytes the row has to move (one read of cls, one of pred,
                  one write of out, as far as the row uses them), bytes / ms, the time those bytes take at the 6.3 TB/s a streaming
                  kernel reaches on this HBM (8 TB/s is its peak), and floor_ms / ms
  host            scenes.host_erode_confusion on the blocky map at radius 3, on this machine's CPU
  conditions      gpu_faster_than_host: both_r3 on the blocky map < host
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

from _scene_bench import CLASSES, make_maps, median_row, rounds_ms  # noqa: E402

HBM_BYTES_PER_MS = 6.3e9                                       # 6.3 TB/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200, help="back-to-back calls per round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scene", type=int, default=6000, help="scene edge in pixels")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scenes", "bench_scene_erode.json"))
    args = ap.parse_args()
    import torch
    from resunet_a_mltsk_keras_amd import _lib as L
    from resunet_a_mltsk_keras_amd import scenes
    if not torch.cuda.is_available():
        sys.exit("bench_scene_erode.py needs a GPU")
    S = args.scene
    maps = make_maps(S)
    names = list(maps)
    n = len(names)
    rng = np.random.default_rng(1)
    pred_host = rng.integers(0, CLASSES, (S, S), dtype=np.uint8)
    cls = [torch.from_numpy(maps[k]).cuda() for k in names]
    preds = [torch.from_numpy(pred_host).cuda() for _ in names]
    outs = [torch.empty((S, S), dtype=torch.uint8, device="cuda") for _ in names]
    conf = torch.zeros((CLASSES, CLASSES), dtype=torch.int64, device="cuda")
    lib, st = L.lib(), torch.cuda.current_stream()
    arr = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    size = lambda k: (ctypes.c_int32 * k)(*([S] * k))

    def call(which, r, with_out, with_pred):
        ts = range(n) if which is None else [names.index(which)]
        lib.call("rua_scene_erode", arr([cls[i] for i in ts]), size(len(ts)), size(len(ts)), len(ts), r,
                 arr([outs[i] for i in ts]) if with_out else None, arr([preds[i] for i in ts]) if with_pred else None,
                 CLASSES, conf.data_ptr() if with_pred else None, ctypes.c_void_p(st.cuda_stream))

    def timed(which, r, with_out, with_pred):
        per_call = rounds_ms(lambda: call(which, r, with_out, with_pred), args.rounds, args.reps)
        ms, row = float(np.median(per_call)), median_row(per_call)
        if r == 3:
            nbytes = (1 if which else n) * S * S * (1 + int(with_out) + int(with_pred))
            row.update(bytes=nbytes, GBps=round(nbytes / ms / 1e6, 1), floor_ms=round(nbytes / HBM_BYTES_PER_MS, 4),
                       share_of_floor=round(nbytes / HBM_BYTES_PER_MS / ms, 3))
        return row

    res = {"scene": [S, S], "classes": CLASSES, "reps": args.reps, "rounds": args.rounds, "hbm_TBps_for_floor": 6.3}
    res["map_r3"] = timed("blocky", 3, True, False)
    res["matrix_r3"] = timed("blocky", 3, False, True)
    res["both_r3"] = timed("blocky", 3, True, True)
    # the same numbers as the host's, while we are here: one call into a zeroed matrix
    conf.zero_()
    call("blocky", 3, True, True)
    torch.cuda.synchronize()
    got_cm, got_map = conf.cpu().numpy(), outs[0].cpu().numpy()
    res["both_r3_noise"] = timed("noise", 3, True, True)
    res["both_r3_uniform"] = timed("uniform", 3, True, True)
    res["both_r1"] = timed("blocky", 1, True, True)
    res["both_r16"] = timed("blocky", 16, True, True)
    res["pool_both_r3"] = timed(None, 3, True, True)
    t0 = time.perf_counter()
    want_cm = scenes.host_erode_confusion(maps["blocky"], pred_host, 3, CLASSES)
    dt = time.perf_counter() - t0
    assert np.array_equal(got_cm, want_cm) and np.array_equal(got_map, scenes.host_erode(maps["blocky"], 3))
    res["host"] = {"ms": round(dt * 1e3, 1), "note": "scenes.host_erode_confusion on the blocky map at radius 3, one run on this machine's CPU"}
    res["kept_fraction_r3"] = {k: round(float((scenes.host_erode(maps[k], 3) != 255).mean()), 4) for k in ("blocky",)}
    res["conditions"] = {"gpu_faster_than_host": bool(res["both_r3"]["ms"] < res["host"]["ms"]),
                         "host_over_gpu": round(res["host"]["ms"] / res["both_r3"]["ms"], 1)}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
