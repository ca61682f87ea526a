#!/usr/bin/env python
"""Test-time augmentation for whole-scene evaluation: what scoring a resident scene under K views of every window costs.  Prints one
JSON line.

The set-up of tools/bench_scene_predict.py: a seeded `--scene` x `--scene` x 3 scene (default 2048) with its class map, the cfg3 network
(256 x 256 x 3, 6 classes, multitask, bf16, graph path), windows of 256 at stride 256, batch 8.

  scene_ms       `--rounds` alternating rounds of `--reps` timed scenes after `--warmup` untimed ones, host clock around work that ends in
                 a device synchronise, ms per scene, for Model.predict_scene(views=) with `none` (one view: rua_scene_stitch, the path
                 without the argument), `flips` (3 views: forwards of 6 patches), `aug5` (5: forwards of 5) and `all` (8: forwards of 8);
                 `forwards` says how many forwards of how many patches a scene takes.  `all_over_none` is, per round, the `all` time
                 over the `none` time: both run forwards of 8 patches, `all` eight times as many, so only the stitch differs.
                 `agree_with_none` is the share of the scene's pixels a variant's map shares with the `none` map (random weights:
                 a figure, not a quality measure).
  stitch_us      rua_scene_stitch_views alone on 8 x 256 x 256 x 6 random probabilities, device events around `--kreps` back-to-back
                 calls after a warm-up, per call: K = 1, 3, 5 and 8 views (8 // K windows owned in full, so K = 8 reads the whole tensor
                 for one window's map), with the bytes read and written and the resulting GB/s; `scene_stitch` is rua_scene_stitch on
                 the same tensor (8 windows), `pinned_copy` the device-to-host copy of the tensor (pinned) that summing on the host
                 would pay first, timed the same way in the same run.
  conditions     the two bounds read from this run: the K = 8 call against the pinned copy, and `all` against 8 x `none` of the same
                 round plus 8 x the round-to-round spread of `none`.
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

VARIANTS = ("none", "flips", "aug5", "all")


def stitch_us(reps):
    import torch
    from resunet_a_mltsk_keras_amd import _lib as L
    from resunet_a_mltsk_keras_amd import scenes
    lib, st = L.lib(), torch.cuda.current_stream()
    size = 4 * P
    p = torch.rand((B, P, P, CLASSES), dtype=torch.float32, device="cuda")
    pred = torch.empty((size, size), dtype=torch.uint8, device="cuda")
    cls = torch.from_numpy(make_scene(size, 1)[1]).cuda()
    conf = torch.zeros((CLASSES, CLASSES), dtype=torch.int64, device="cuda")
    ptr1 = lambda t: (ctypes.c_void_p * 1)(t.data_ptr())
    pp, cp, hs, ws = ptr1(pred), ptr1(cls), (ctypes.c_int32 * 1)(size), (ctypes.c_int32 * 1)(size)
    rows = np.array([[0, (k // 4) * P, (k % 4) * P, 0] for k in range(B)], np.int32)
    own = np.array([[0, P, 0, P]] * B, np.int32)
    stream = ctypes.c_void_p(st.cuda_stream)

    timed = lambda fn: call_us(fn, reps)

    def figure(us, patches, windows):
        moved = patches * P * P * 4 * CLASSES + windows * P * P * 2          # the probabilities and the label read, the prediction written
        return {"us_per_call": round(us, 2), "patches_read": patches, "windows": windows, "bytes_read_and_written": moved,
                "GBps": round(moved / us / 1e3, 1)}

    out = {}
    for K in (1, 3, 5, 8):
        G = B // K
        codes = scenes.VIEW_SETS["all"][:K]
        vr = scenes.view_rows(rows[:G], codes)
        us = timed(lambda: lib.call("rua_scene_stitch_views", p.data_ptr(), G, K, P, P, CLASSES, vr.ctypes.data, own.ctypes.data, pp, cp, hs, ws, 1,
                                    conf.data_ptr(), stream))
        out[f"K{K}"] = {"codes": list(codes), **figure(us, G * K, G)}
    us = timed(lambda: lib.call("rua_scene_stitch", p.data_ptr(), B, P, P, CLASSES, rows.ctypes.data, own.ctypes.data, pp, cp, hs, ws, 1,
                                conf.data_ptr(), stream))
    out["scene_stitch"] = figure(us, B, B)
    host = torch.empty(p.shape, dtype=torch.float32).pin_memory()
    us = timed(lambda: host.copy_(p, non_blocking=True))
    nbytes = p.numel() * 4
    out["pinned_copy"] = {"us_per_call": round(us, 2), "bytes": nbytes, "GBps": round(nbytes / us / 1e3, 1)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3, help="timed scenes per round and variant")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kreps", type=int, default=200, help="timed calls of the kernel figures")
    ap.add_argument("--scene", type=int, default=2048, help="scene edge in pixels")
    args = ap.parse_args()
    import torch
    from resunet_a_mltsk_keras_amd import scenes
    if not torch.cuda.is_available():
        sys.exit("bench_scene_views.py needs a GPU")
    img, cls = make_scene(args.scene)
    pool = scenes.ScenePool([img], [cls], patch=P)
    m = cfg3_model()

    def timed(fn):
        ms, last = clock_ms(fn, args.warmup, args.reps)
        return round(ms, 2), last

    windows = len(pool.predict_table(0, P)[0])
    ms, maps = {v: [] for v in VARIANTS}, {}
    for _ in range(args.rounds):
        for v in VARIANTS:
            t, (maps[v], _) = timed(lambda: m.predict_scene(pool, 0, stride=P, batch=B, norm_type=1, views=v))
            ms[v].append(t)
    forwards = {}
    for v in VARIANTS:
        K = len(scenes.VIEW_SETS[v])
        G = B if v == "none" else max(1, B // K)
        forwards[v] = {"views": K, "forwards": -(-windows // G), "patches_per_forward": G if v == "none" else G * K}
    res = {"scene": [args.scene, args.scene, CIN], "model": {"shape": [B, P, P, CIN], "classes": CLASSES, "dtype": "bf16", "path": "graph"},
           "stride": P, "windows": windows, "warmup": args.warmup, "reps": args.reps, "rounds": args.rounds,
           "scene_ms": ms, "forwards": forwards,
           "all_over_none": [round(a / n, 3) for a, n in zip(ms["all"], ms["none"])],
           "agree_with_none": {v: round(float((maps[v] == maps["none"]).mean()), 4) for v in VARIANTS},
           "stitch_us": {"B": B, "patch": P, "classes": CLASSES, "reps": args.kreps, **stitch_us(args.kreps)}}
    spread = max(ms["none"]) - min(ms["none"])
    k8, copy = res["stitch_us"]["K8"]["us_per_call"], res["stitch_us"]["pinned_copy"]["us_per_call"]
    res["conditions"] = {
        "kernel_K8_below_pinned_copy": {"K8_us": k8, "pinned_copy_us": copy, "holds": bool(k8 < copy)},
        "all_within_8x_none": {"none_spread_ms": round(spread, 2), "bound_ms": [round(8 * n + 8 * spread, 2) for n in ms["none"]],
                               "all_ms": ms["all"], "holds": bool(all(a <= 8 * n + 8 * spread for a, n in zip(ms["all"], ms["none"])))}}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
