#!/usr/bin/env python
"""Blended whole-scene prediction: what Model.predict_scene(blend="linear") and its kernel cost.  Prints one JSON line.

The set-up of tools/bench_scene_scales.py: a seeded `--scene` x `--scene` x 3 scene (default 2048) with its class map, the cfg3 network
(256 x 256 x 3, 6 classes, multitask, bf16, graph path), batch 8 - at stride 128, half the patch, where neighbouring windows overlap
by half and the blend has something to blend.

  scene_ms       `--rounds` alternating rounds of `--reps` timed scenes after `--warmup` untimed ones, host clock around work that ends in
                 a device synchronise, ms per scene (and the median over the rounds), for predict_scene with blend None - every pixel
                 from the window it is most central in, rua_scene_stitch / rua_scene_stitch_views - and "linear", each with views
                 `none` and `flips`; `forwards` says how many forwards of how many patches each setting takes (the same for both).
  forward_ms     the inference forward of 8 and of 6 patches alone (the captured graph), device events around `--kreps` replays.
  accumulate_us  rua_scene_accumulate_blend alone on 8 x 256 x 256 x 6 random probabilities, device events around `--kreps`
                 back-to-back calls after a warm-up, per call, for (G, K) = (8, 1) and (2, 3): the first G footprints of the scene's
                 blend_table (neighbours in a row, each overlapping the next by half), with the bytes it adds and the resulting GB/s of
                 added bytes; `accumulate` is rua_scene_accumulate on the same groups with the rectangles scale_table lets them own
                 (disjoint: about half the pixels of the interior footprints, plain read-add-write), timed the same way in the same run.
  conditions     scene_ms over (forwards x forward_ms) per setting, the blended scene over the unblended one, and the kernel over the
                 forward of its batch.
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

STRIDE = P // 2
BLENDS = {"cut": None, "linear": "linear"}
VIEWS = ("none", "flips")
ptr1 = lambda t: (ctypes.c_void_p * 1)(t.data_ptr())
int1 = lambda v: (ctypes.c_int32 * 1)(v)


def accumulate_us(reps, scene):
    import torch
    from resunet_a_mltsk_keras_amd import _lib as L
    from resunet_a_mltsk_keras_amd import scenes
    lib, stream = L.lib(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = torch.rand((B, P, P, CLASSES), dtype=torch.float32, device="cuda")
    acc = torch.zeros((scene, scene, CLASSES), dtype=torch.int32, device="cuda")
    ap, hs, ws = ptr1(acc), int1(scene), int1(scene)
    out = {}
    for G, K in ((8, 1), (2, 3)):
        codes = scenes.VIEW_SETS["flips"][:K]
        rows7, foot = scenes.blend_table((scene, scene), P, P, STRIDE, codes)
        _, own = scenes.scale_table((scene, scene), P, P, STRIDE, codes)
        rows7, foot, own = np.ascontiguousarray(rows7[:G * K]), np.ascontiguousarray(foot[:G]), np.ascontiguousarray(own[:G])
        row = {}
        for name, entry, rect in (("accumulate_blend", "rua_scene_accumulate_blend", foot), ("accumulate", "rua_scene_accumulate", own)):
            acc.zero_()
            us = call_us(lambda: lib.call(entry, p.data_ptr(), G, K, P, P, CLASSES, rows7.ctypes.data, rect.ctypes.data, ap, hs, ws, 1, stream), reps)
            added = int(((rect[:, 1] - rect[:, 0]) * (rect[:, 3] - rect[:, 2])).sum()) * CLASSES * 4
            row[name] = {"us_per_call": round(us, 2), "bytes_added": added, "GBps_added": round(added / us / 1e3, 1)}
        out[f"G{G}_K{K}"] = row
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2, help="timed scenes per round and setting")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kreps", type=int, default=100, help="timed calls of the kernel figures")
    ap.add_argument("--scene", type=int, default=2048, help="scene edge in pixels")
    args = ap.parse_args()
    import torch
    from resunet_a_mltsk_keras_amd import scenes
    if not torch.cuda.is_available():
        sys.exit("bench_scene_blend.py needs a GPU")
    img, cls = make_scene(args.scene)
    pool = scenes.ScenePool([img], [cls], patch=P)
    m = cfg3_model()
    settings = [(b, v) for b in BLENDS for v in VIEWS]
    name = lambda b, v: f"{b}_{v}"
    ms, maps = {name(b, v): [] for b, v in settings}, {}
    for _ in range(args.rounds):
        for b, v in settings:
            t, (maps[name(b, v)], _) = clock_ms(lambda: m.predict_scene(pool, 0, stride=STRIDE, batch=B, norm_type=1, views=v, blend=BLENDS[b]),
                                                args.warmup, args.reps)
            ms[name(b, v)].append(round(t, 2))
    med = {k: round(float(np.median(v)), 2) for k, v in ms.items()}
    eng = m.engine
    forward_ms = {}
    for n in (8, 6):
        g = eng.graph(n, False)
        forward_ms[f"patches{n}"] = round(call_us(lambda: eng._forward_eval(g), args.kreps) / 1e3, 3)
    acc_us = accumulate_us(args.kreps, args.scene)
    forwards = {}
    for b, v in settings:
        K = len(scenes.VIEW_SETS[v])
        G = max(1, B // K)
        n = len(scenes.blend_table((args.scene, args.scene), P, P, STRIDE, scenes.VIEW_SETS[v])[1])
        forwards[name(b, v)] = {"views": K, "groups": n, "forwards": -(-n // G), "patches_per_forward": G * K}
    res = {"scene": [args.scene, args.scene, CIN], "model": {"shape": [B, P, P, CIN], "classes": CLASSES, "dtype": "bf16", "path": "graph"},
           "stride": STRIDE, "warmup": args.warmup, "reps": args.reps, "rounds": args.rounds,
           "scene_ms": ms, "scene_ms_median": med, "forwards": forwards, "forward_ms": forward_ms,
           "agree_with_cut_none": {k: round(float((maps[k] == maps["cut_none"]).mean()), 4) for k in maps},
           "accumulate_us": {"B": B, "patch": P, "classes": CLASSES, "reps": args.kreps, **acc_us}}
    fwd_us = {"G8_K1": forward_ms["patches8"] * 1e3, "G2_K3": forward_ms["patches6"] * 1e3}
    res["conditions"] = {
        "scene_ms_over_its_forwards": {k: round(med[k] / (forwards[k]["forwards"] * forward_ms[f"patches{forwards[k]['patches_per_forward']}"]), 3)
                                       for k in med},
        "linear_over_cut": {v: round(med[name("linear", v)] / med[name("cut", v)], 3) for v in VIEWS},
        "blend_over_accumulate": {k: round(r["accumulate_blend"]["us_per_call"] / r["accumulate"]["us_per_call"], 3) for k, r in acc_us.items()},
        "blend_over_its_forward": {k: round(r["accumulate_blend"]["us_per_call"] / fwd_us[k], 4) for k, r in acc_us.items()}}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
