#!/usr/bin/env python
"""Whole-scene evaluation: what scoring a resident scene on the GPU costs and what it replaces.  Prints one JSON line.

A seeded `--scene` x `--scene` x 3 scene (default 2048) with its class map, the cfg3 network (256 x 256 x 3, 6 classes, multitask, bf16,
graph path), windows of 256 at stride 256 (non-overlapping) and stride 128 (every pixel from the central half of a window), 8 per batch.

  scene_ms       per stride, `--rounds` alternating rounds of `--reps` timed scenes after `--warmup` untimed ones, host clock around work
                 that ends in a device synchronise, ms per scene:
                   predict        the route there was: Model.predict(pool.batch(rows), batch_size=8, norm_type=1) - all four heads' float
                                  outputs copied to the host - then np.argmax of the seg head, the mosaic of the owned rectangles and the
                                  confusion matrix (np.bincount) on the host
                   predict_scene  Model.predict_scene: windows cut, predicted and stitched on the GPU, the uint8 map and the 6 x 6 matrix
                                  copied back once
                 `same_map` says whether the two routes' maps were equal in the last round; `host_bytes` what each copies to the host.
  stitch_us      rua_scene_stitch alone on a batch of 8 windows of random probabilities, device events around `--kreps` back-to-back calls
                 after a warm-up, per call: `full` (every window owned in full: stride 256) and `central` (the central 128 x 128:
                 stride 128), each with the bytes it reads and writes and the resulting GB/s; `pinned_copy` is the device-to-host copy
                 of the same seg probabilities (8 x 256 x 256 x 6 fp32, pinned) it replaces, timed the same way in the same run
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


def predict_route(m, pool, rows, own):
    """Today's route: every head's floats to the host, arg-max, mosaic and confusion matrix there."""
    H, W = pool.shapes[0]
    seg = m.predict(pool.batch(rows), batch_size=B, norm_type=1)["seg"]
    cls = np.argmax(seg, axis=-1).astype(np.uint8)
    out = np.empty((H, W), np.uint8)
    for k, ((_, r, c, _), (r0, r1, c0, c1)) in enumerate(zip(rows.tolist(), own.tolist())):
        out[r + r0:r + r1, c + c0:c + c1] = cls[k, r0:r1, c0:c1]
    true = pool.class_maps[0].astype(np.int64).ravel()
    keep = true < CLASSES
    cm = np.bincount(true[keep] * CLASSES + out.ravel()[keep], minlength=CLASSES * CLASSES).reshape(CLASSES, CLASSES)
    return out, cm


def stitch_us(reps):
    import torch
    from resunet_a_mltsk_keras_amd import _lib as L
    lib, st = L.lib(), torch.cuda.current_stream()
    size = 4 * P
    p = torch.rand((B, P, P, CLASSES), dtype=torch.float32, device="cuda")
    pred = torch.empty((size, size), dtype=torch.uint8, device="cuda")
    cls = torch.from_numpy(make_scene(size, 1)[1]).cuda()
    conf = torch.zeros((CLASSES, CLASSES), dtype=torch.int64, device="cuda")
    ptr1 = lambda t: (ctypes.c_void_p * 1)(t.data_ptr())
    pp, cp, hs, ws = ptr1(pred), ptr1(cls), (ctypes.c_int32 * 1)(size), (ctypes.c_int32 * 1)(size)
    rows = np.array([[0, (k // 4) * P, (k % 4) * P, 0] for k in range(B)], np.int32)

    timed = lambda fn: call_us(fn, reps)

    def figure(own_row):
        own = np.array([own_row] * B, np.int32)
        us = timed(lambda: lib.call("rua_scene_stitch", p.data_ptr(), B, P, P, CLASSES, rows.ctypes.data, own.ctypes.data, pp, cp, hs, ws, 1,
                                    conf.data_ptr(), ctypes.c_void_p(st.cuda_stream)))
        px = B * (own_row[1] - own_row[0]) * (own_row[3] - own_row[2])
        moved = px * (4 * CLASSES + 2)                              # the probabilities and the label read, the prediction written
        return {"us_per_call": round(us, 2), "pixels": px, "bytes_read_and_written": moved, "GBps": round(moved / us / 1e3, 1)}

    out = {"full": figure([0, P, 0, P]), "central": figure([P // 4, 3 * P // 4, P // 4, 3 * P // 4])}
    host = torch.empty(p.shape, dtype=torch.float32).pin_memory()
    us = timed(lambda: host.copy_(p, non_blocking=True))
    nbytes = p.numel() * 4
    out["pinned_copy"] = {"us_per_call": round(us, 2), "bytes": nbytes, "GBps": round(nbytes / us / 1e3, 1)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3, help="timed scenes per round and route")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kreps", type=int, default=200, help="timed calls of the kernel figure")
    ap.add_argument("--scene", type=int, default=2048, help="scene edge in pixels")
    args = ap.parse_args()
    import torch
    from resunet_a_mltsk_keras_amd import scenes
    if not torch.cuda.is_available():
        sys.exit("bench_scene_predict.py needs a GPU")
    img, cls = make_scene(args.scene)
    pool = scenes.ScenePool([img], [cls], patch=P)
    m = cfg3_model()

    def timed(fn):
        ms, last = clock_ms(fn, args.warmup, args.reps)
        return round(ms, 2), last

    res = {"scene": [args.scene, args.scene, CIN], "model": {"shape": [B, P, P, CIN], "classes": CLASSES, "dtype": "bf16", "path": "graph"},
           "warmup": args.warmup, "reps": args.reps, "scene_ms": {}}
    for stride in (P, P // 2):
        rows, own = pool.predict_table(0, stride)
        ms = {"predict": [], "predict_scene": []}
        for _ in range(args.rounds):
            t, a = timed(lambda: predict_route(m, pool, rows, own))
            ms["predict"].append(t)
            t, b = timed(lambda: m.predict_scene(pool, 0, stride=stride, batch=B, norm_type=1))
            ms["predict_scene"].append(t)
        heads = sum(CLASSES if h != "color" else 3 for h in ("seg", "bound", "dist", "color"))
        res["scene_ms"][f"stride{stride}"] = {
            "windows": len(rows), **ms, "same_map": bool(np.array_equal(a[0], b[0])), "same_confusion": bool(np.array_equal(a[1], b[1])),
            "differing_pixels": int((a[0] != b[0]).sum()),
            "host_bytes": {"predict": len(rows) * P * P * heads * 4, "predict_scene": args.scene * args.scene + CLASSES * CLASSES * 8}}
    res["stitch_us"] = {"B": B, "patch": P, "classes": CLASSES, "reps": args.kreps, **stitch_us(args.kreps)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
