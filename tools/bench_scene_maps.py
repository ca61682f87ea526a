#!/usr/bin/env python
"""Whole-scene maps of every head: what rua_scene_stitch_maps and Model.predict_scene(heads=) cost.  Prints one JSON line.

The set-up of tools/bench_scene_views.py: a seeded `--scene` x `--scene` x 3 scene (default 2048) with its class map, the cfg3 network
(256 x 256 x 3, 6 classes, multitask, bf16, graph path), windows of 256 at stride 256, batch 8.

  stitch_us      rua_scene_stitch_maps alone, device events around `--kreps` back-to-back calls after a warm-up, per call: 8 x 256 x
                 256 x 6 random values at K = 1 (8 windows owned in full) and K = 8 (one window), and 8 x 256 x 256 x 3 in mode 1
                 (hsv_rgb, K = 1), with the bytes read and written and the resulting GB/s.  `pinned_copy_*` is the device-to-host copy
                 of the same floats (pinned), which the kernel replaces, and `stitch_views_*` rua_scene_stitch_views on the same
                 tensors, timed the same way in the same run.
  scene_ms       `--rounds` alternating rounds of `--reps` timed scenes after `--warmup` untimed ones, host clock around work that ends
                 in a device synchronise, ms per scene, for Model.predict_scene with heads=() and with all five heads, at views `none`
                 and `all`; `heads_minus_default` is their difference per round, `fetch_ms` the device-to-host copy of five maps of
                 the scene's size alone.  `host_route_ms` is the only alternative without the kernel: Model.predict per batch of 8
                 window rows (every head's floats to the host) and scenes.host_stitch_maps there, once per variant in the same run
                 (`--host_reps`), with `host_route_equal` saying whether its maps equal predict_scene's byte for byte.
  default_path   with --default_path only: predict_scene(heads=()) at views `none`, `--rounds` x `--reps` scenes, and the SHA-1 of the
                 map and the matrix - the figure two builds are compared by, each in a process of its own.
  conditions     the bounds read from this run: every kernel case below its pinned copy, and the full-heads call below the host
                 route at both view sets.
"""
import argparse
import ctypes
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from _scene_bench import B, CIN, CLASSES, P, call_us, cfg3_model, clock_ms, make_scene  # noqa: E402

ALL_HEADS = ("seg", "bound", "dist", "color", "color_rgb")
VIEWS = ("none", "all")


def stitch_us(reps):
    import torch
    from resunet_a_mltsk_keras_amd import _lib as L
    from resunet_a_mltsk_keras_amd import scenes
    lib, st = L.lib(), torch.cuda.current_stream()
    size = 4 * P
    ptr1 = lambda t: (ctypes.c_void_p * 1)(t.data_ptr())
    hs, ws = (ctypes.c_int32 * 1)(size), (ctypes.c_int32 * 1)(size)
    rows = np.array([[0, (k // 4) * P, (k % 4) * P, 0] for k in range(B)], np.int32)
    own = np.array([[0, P, 0, P]] * B, np.int32)
    stream = ctypes.c_void_p(st.cuda_stream)
    pred = torch.empty((size, size), dtype=torch.uint8, device="cuda")
    pp = ptr1(pred)

    timed = lambda fn: call_us(fn, reps)

    out = {}
    for name, ch, K, mode in (("plain_C6_K1", CLASSES, 1, 0), ("plain_C6_K8", CLASSES, 8, 0), ("hsv_rgb_C3_K1", 3, 1, 1)):
        G = B // K
        p = torch.rand((B, P, P, ch), dtype=torch.float32, device="cuda")
        m = torch.empty((size, size, ch), dtype=torch.uint8, device="cuda")
        mp = ptr1(m)
        vr = scenes.view_rows(rows[:G], scenes.VIEW_SETS["all"][:K])
        us = timed(lambda: lib.call("rua_scene_stitch_maps", p.data_ptr(), G, K, P, P, ch, vr.ctypes.data, own.ctypes.data, mp, hs, ws, 1, mode, stream))
        moved = B * P * P * 4 * ch + G * P * P * ch
        out[name] = {"us_per_call": round(us, 2), "patches_read": B, "windows": G, "bytes_read_and_written": moved, "GBps": round(moved / us / 1e3, 1)}
        us = timed(lambda: lib.call("rua_scene_stitch_views", p.data_ptr(), G, K, P, P, ch, vr.ctypes.data, own.ctypes.data, pp, None, hs, ws, 1,
                                    None, stream))
        out["stitch_views_" + name] = {"us_per_call": round(us, 2)}
        host = torch.empty(p.shape, dtype=torch.float32).pin_memory()
        us = timed(lambda: host.copy_(p, non_blocking=True))
        out["pinned_copy_" + name] = {"us_per_call": round(us, 2), "bytes": p.numel() * 4, "GBps": round(p.numel() * 4 / us / 1e3, 1)}
    return out


def host_route(m, pool, views, heads):
    """The route without the kernel: every head's floats of every batch to the host, host_stitch_maps there."""
    from resunet_a_mltsk_keras_amd import scenes
    codes = scenes.VIEW_SETS[views]
    K = len(codes)
    G = B if K == 1 else max(1, B // K)
    rows, own = pool.predict_table(0, P)
    maps = {h: [np.zeros(pool.shapes[0] + (3 if h.startswith("color") else CLASSES,), np.uint8)] for h in heads}
    for k0 in range(0, len(rows), G):
        vr = scenes.view_rows(rows[k0:k0 + G], codes)
        outs = m.predict(pool.batch(vr), batch_size=len(vr), norm_type=1)
        for h in heads:
            scenes.host_stitch_maps(outs["color" if h == "color_rgb" else h], vr, own[k0:k0 + G], pool.shapes, K,
                                    mode="hsv_rgb" if h == "color_rgb" else "plain", maps=maps[h])
    return {h: v[0] for h, v in maps.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3, help="timed scenes per round and variant")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kreps", type=int, default=200, help="timed calls of the kernel figures")
    ap.add_argument("--host_reps", type=int, default=1, help="timed runs of the host route per view set")
    ap.add_argument("--scene", type=int, default=2048, help="scene edge in pixels")
    ap.add_argument("--default_path", action="store_true", help="only predict_scene(heads=()) at views none, with hashes of its results")
    args = ap.parse_args()
    import torch
    from resunet_a_mltsk_keras_amd import scenes
    if not torch.cuda.is_available():
        sys.exit("bench_scene_maps.py needs a GPU")
    img, cls = make_scene(args.scene)
    pool = scenes.ScenePool([img], [cls], patch=P)
    m = cfg3_model()

    def timed(fn, warmup=args.warmup, reps=args.reps):
        ms, last = clock_ms(fn, warmup, reps)
        return round(ms, 2), last

    base = {"scene": [args.scene, args.scene, CIN], "model": {"shape": [B, P, P, CIN], "classes": CLASSES, "dtype": "bf16", "path": "graph"},
            "stride": P, "windows": len(pool.predict_table(0, P)[0]), "warmup": args.warmup, "reps": args.reps, "rounds": args.rounds}
    if args.default_path:
        ms = []
        for _ in range(args.rounds):
            t, (pred, cm) = timed(lambda: m.predict_scene(pool, 0, stride=P, batch=B, norm_type=1))
            ms.append(t)
        print(json.dumps({**base, "default_path": {"scene_ms": ms, "map_sha1": hashlib.sha1(pred.tobytes()).hexdigest(),
                                                   "matrix_sha1": hashlib.sha1(cm.tobytes()).hexdigest()}}))
        return
    ms = {v: {"default": [], "all_heads": []} for v in VIEWS}
    last = {}
    for _ in range(args.rounds):
        for v in VIEWS:
            t, _ = timed(lambda: m.predict_scene(pool, 0, stride=P, batch=B, norm_type=1, views=v))
            ms[v]["default"].append(t)
            t, last[v] = timed(lambda: m.predict_scene(pool, 0, stride=P, batch=B, norm_type=1, views=v, heads=ALL_HEADS))
            ms[v]["all_heads"].append(t)
    for v in VIEWS:
        ms[v]["heads_minus_default"] = [round(a - d, 2) for a, d in zip(ms[v]["all_heads"], ms[v]["default"])]
    resident = [torch.zeros((args.scene, args.scene, 3 if h.startswith("color") else CLASSES), dtype=torch.uint8, device="cuda") for h in ALL_HEADS]
    fetch_ms, _ = timed(lambda: [t.cpu().numpy() for t in resident])
    host_ms, host_equal = {}, {}
    for v in VIEWS:
        host_ms[v], maps = timed(lambda: host_route(m, pool, v, ALL_HEADS), warmup=0, reps=args.host_reps)
        host_equal[v] = {h: bool(np.array_equal(maps[h], last[v][2][h])) for h in ALL_HEADS}
    res = {**base, "heads": list(ALL_HEADS), "scene_ms": ms, "fetch_ms": fetch_ms, "fetch_bytes": int(sum(t.numel() for t in resident)),
           "host_route_ms": host_ms, "host_route_equal": host_equal,
           "stitch_us": {"B": B, "patch": P, "reps": args.kreps, **stitch_us(args.kreps)}}
    k = res["stitch_us"]
    res["conditions"] = {
        "kernel_below_pinned_copy": {n: {"kernel_us": k[n]["us_per_call"], "pinned_copy_us": k["pinned_copy_" + n]["us_per_call"],
                                         "holds": bool(k[n]["us_per_call"] < k["pinned_copy_" + n]["us_per_call"])}
                                     for n in ("plain_C6_K1", "plain_C6_K8", "hsv_rgb_C3_K1")},
        "all_heads_below_host_route": {v: {"all_heads_ms": ms[v]["all_heads"], "host_route_ms": host_ms[v],
                                           "holds": bool(max(ms[v]["all_heads"]) < host_ms[v])} for v in VIEWS}}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
