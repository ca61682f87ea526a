#!/usr/bin/env python
"""Multi-scale test-time augmentation for whole-scene evaluation: what Model.predict_scene(scales=) and its two kernels cost.  Prints
one JSON line.

The set-up of tools/bench_scene_views.py: a seeded `--scene` x `--scene` x 3 scene (default 2048) with its class map, the cfg3 network
(256 x 256 x 3, 6 classes, multitask, bf16, graph path), stride 256, batch 8.

  scene_ms       `--rounds` alternating rounds of `--reps` timed scenes after `--warmup` untimed ones, host clock around work that ends in
                 a device synchronise, ms per scene (and the median over the rounds), for predict_scene under scales (1,) - the path
                 without the argument - and (0.75, 1, 1.5), each with views `none` and `flips`; `forwards` says how many forwards of how
                 many patches each setting takes.
  forward_ms     the inference forward of 8 and of 6 patches alone (the captured graph), device events around `--kreps` replays.
  accumulate_us  rua_scene_accumulate alone on 8 x 256 x 256 x 6 random probabilities, device events around `--kreps` back-to-back
                 calls after a warm-up, per call, for (G, K) = (8, 1) and (2, 3) and the footprints of zoom 0.75, 1 and 1.5 (341, 256,
                 171; every footprint owned in full, so zoom 0.75 writes the most accumulator), with the bytes moved - the
                 probabilities read once, the accumulator read and written - and the resulting GB/s; `stitch_views` is
                 rua_scene_stitch_views at the same G and K on the same tensor, timed the same way in the same run.
  argmax_us      rua_scene_argmax on the int32 accumulator of a `--big` x `--big` scene (default 6000: 864 MB at 6 classes) with its
                 class map, and on the benchmark scene; `scene_stitch` is rua_scene_stitch on 8 windows of 256 owned in full and
                 `scene_stitch_whole_scene_us` that figure times the calls a `--big` scene takes at stride 256.
  share          the part of a multi-scale predict_scene that the two new kernels take: per setting, the accumulate figure of each
                 pass' (G, K, footprint) times the pass' batches plus one arg-max of the benchmark scene, over the median scene_ms.
  conditions     what this run says about the two expectations: rua_scene_accumulate costs less than the forward of the same batch,
                 and a multi-scale scene costs about its forwards - scene_ms over (forwards x forward_ms).
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

SCALES = {"one": (1.0,), "three": (0.75, 1.0, 1.5)}
VIEWS = ("none", "flips")
ptr1 = lambda t: (ctypes.c_void_p * 1)(t.data_ptr())
int1 = lambda v: (ctypes.c_int32 * 1)(v)


def accumulate_us(reps):
    """Per (G, K) and zoom: G footprints side by side in one scene, each owned in full, under the first K codes of `flips`."""
    import torch
    from resunet_a_mltsk_keras_amd import _lib as L
    from resunet_a_mltsk_keras_amd import scenes
    lib, stream = L.lib(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = torch.rand((B, P, P, CLASSES), dtype=torch.float32, device="cuda")
    out = {}
    for G, K in ((8, 1), (2, 3)):
        codes = scenes.VIEW_SETS["flips"][:K]
        row = {}
        for zoom in SCALES["three"]:
            F = scenes.scale_footprint(P, zoom)[0]
            rows7, own = scenes.scale_table((F, F * G), P, (F, F), P, codes)        # G footprints in a row, stride = footprint
            assert len(own) == G and (own[:, 1] - own[:, 0] == F).all() and (own[:, 3] - own[:, 2] == F).all()
            acc = torch.zeros((F, F * G, CLASSES), dtype=torch.int32, device="cuda")
            ap, hs, ws = ptr1(acc), int1(F), int1(F * G)
            us = call_us(lambda: lib.call("rua_scene_accumulate", p.data_ptr(), G, K, P, P, CLASSES, rows7.ctypes.data, own.ctypes.data, ap, hs, ws, 1,
                                          stream), reps)
            moved = G * K * P * P * CLASSES * 4 + 2 * G * F * F * CLASSES * 4
            row[f"zoom{zoom:g}"] = {"footprint": F, "us_per_call": round(us, 2), "bytes_moved": moved, "GBps": round(moved / us / 1e3, 1)}
        pred = torch.empty((P, P * G), dtype=torch.uint8, device="cuda")
        cls = torch.zeros((P, P * G), dtype=torch.uint8, device="cuda")
        conf = torch.zeros((CLASSES, CLASSES), dtype=torch.int64, device="cuda")
        rows4 = scenes.view_rows(np.array([[0, 0, g * P, 0] for g in range(G)], np.int32), codes)
        own4 = np.array([[0, P, 0, P]] * G, np.int32)
        pp, cp, hs, ws = ptr1(pred), ptr1(cls), int1(P), int1(P * G)
        us = call_us(lambda: lib.call("rua_scene_stitch_views", p.data_ptr(), G, K, P, P, CLASSES, rows4.ctypes.data, own4.ctypes.data, pp, cp, hs, ws,
                                      1, conf.data_ptr(), stream), reps)
        row["stitch_views"] = {"us_per_call": round(us, 2)}
        out[f"G{G}_K{K}"] = row
    return out


def argmax_us(reps, big, scene):
    import torch
    from resunet_a_mltsk_keras_amd import _lib as L
    lib, stream = L.lib(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    conf = torch.zeros((CLASSES, CLASSES), dtype=torch.int64, device="cuda")
    out = {}
    for name, size in (("big", big), ("scene", scene)):
        acc = torch.randint(0, 1 << 20, (size, size, CLASSES), dtype=torch.int32, device="cuda")
        pred = torch.empty((size, size), dtype=torch.uint8, device="cuda")
        cls = torch.from_numpy(make_scene(size, 1)[1]).cuda()
        ap, pp, cp, hs, ws = ptr1(acc), ptr1(pred), ptr1(cls), int1(size), int1(size)
        us = call_us(lambda: lib.call("rua_scene_argmax", ap, pp, cp, hs, ws, 1, CLASSES, conf.data_ptr(), stream), reps)
        moved = size * size * (4 * CLASSES + 2)
        out[name] = {"size": size, "us_per_call": round(us, 2), "bytes_moved": moved, "GBps": round(moved / us / 1e3, 1)}
        del acc, pred, cls
    p = torch.rand((B, P, P, CLASSES), dtype=torch.float32, device="cuda")
    pred = torch.empty((P, P * B), dtype=torch.uint8, device="cuda")
    cls = torch.zeros((P, P * B), dtype=torch.uint8, device="cuda")
    rows = np.array([[0, 0, g * P, 0] for g in range(B)], np.int32)
    own = np.array([[0, P, 0, P]] * B, np.int32)
    pp, cp, hs, ws = ptr1(pred), ptr1(cls), int1(P), int1(P * B)
    us = call_us(lambda: lib.call("rua_scene_stitch", p.data_ptr(), B, P, P, CLASSES, rows.ctypes.data, own.ctypes.data, pp, cp, hs, ws, 1,
                                  conf.data_ptr(), stream), reps)
    per_axis = -(-big // P)
    calls = -(-per_axis * per_axis // B)
    out["scene_stitch"] = {"us_per_call": round(us, 2), "windows": B}
    out["scene_stitch_whole_scene_us"] = {"calls": calls, "us": round(us * calls, 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2, help="timed scenes per round and setting")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kreps", type=int, default=100, help="timed calls of the kernel figures")
    ap.add_argument("--scene", type=int, default=2048, help="scene edge in pixels")
    ap.add_argument("--big", type=int, default=6000, help="edge of the scene of the arg-max figure")
    args = ap.parse_args()
    import torch
    from resunet_a_mltsk_keras_amd import scenes
    if not torch.cuda.is_available():
        sys.exit("bench_scene_scales.py needs a GPU")
    img, cls = make_scene(args.scene)
    pool = scenes.ScenePool([img], [cls], patch=P)
    m = cfg3_model()
    settings = [(s, v) for s in SCALES for v in VIEWS]
    name = lambda s, v: f"{s}_{v}"
    ms, maps = {name(s, v): [] for s, v in settings}, {}
    for _ in range(args.rounds):
        for s, v in settings:
            t, (maps[name(s, v)], _) = clock_ms(lambda: m.predict_scene(pool, 0, stride=P, batch=B, norm_type=1, views=v, scales=SCALES[s]),
                                                args.warmup, args.reps)
            ms[name(s, v)].append(round(t, 2))
    med = {k: round(float(np.median(v)), 2) for k, v in ms.items()}
    eng = m.engine
    forward_ms = {}
    for n in (8, 6):
        g = eng.graph(n, False)
        forward_ms[f"patches{n}"] = round(call_us(lambda: eng._forward_eval(g), args.kreps) / 1e3, 3)
    acc_us = accumulate_us(args.kreps)
    arg_us = argmax_us(max(3, args.kreps // 10), args.big, args.scene)
    forwards, share = {}, {}
    for s, v in settings:
        K = len(scenes.VIEW_SETS[v])
        G = max(1, B // K)
        passes = [len(scenes.scale_table((args.scene, args.scene), P, scenes.scale_footprint(P, z), P, scenes.VIEW_SETS[v])[1]) for z in SCALES[s]]
        batches = [-(-n // G) for n in passes]
        forwards[name(s, v)] = {"views": K, "groups_per_pass": passes, "forwards": sum(batches), "patches_per_forward": G * K}
        if s == "three":
            us = sum(b * acc_us[f"G{G}_K{K}"][f"zoom{z:g}"]["us_per_call"] for b, z in zip(batches, SCALES[s])) + arg_us["scene"]["us_per_call"]
            share[name(s, v)] = {"new_kernels_ms": round(us / 1e3, 3), "scene_ms": med[name(s, v)], "share": round(us / 1e3 / med[name(s, v)], 4)}
    res = {"scene": [args.scene, args.scene, CIN], "model": {"shape": [B, P, P, CIN], "classes": CLASSES, "dtype": "bf16", "path": "graph"},
           "stride": P, "warmup": args.warmup, "reps": args.reps, "rounds": args.rounds, "scales": {k: list(v) for k, v in SCALES.items()},
           "scene_ms": ms, "scene_ms_median": med, "forwards": forwards, "forward_ms": forward_ms,
           "agree_with_one_none": {k: round(float((maps[k] == maps["one_none"]).mean()), 4) for k in maps},
           "accumulate_us": {"B": B, "patch": P, "classes": CLASSES, "reps": args.kreps, **acc_us}, "argmax_us": arg_us, "share": share}
    worst = {k: max(v["us_per_call"] for z, v in row.items() if z.startswith("zoom")) for k, row in acc_us.items()}
    res["conditions"] = {
        "accumulate_below_its_forward": {"G8_K1": {"accumulate_us": worst["G8_K1"], "forward_us": round(forward_ms["patches8"] * 1e3, 1)},
                                         "G2_K3": {"accumulate_us": worst["G2_K3"], "forward_us": round(forward_ms["patches6"] * 1e3, 1)},
                                         "holds": bool(worst["G8_K1"] < forward_ms["patches8"] * 1e3 and worst["G2_K3"] < forward_ms["patches6"] * 1e3)},
        "scene_ms_over_its_forwards": {k: round(med[k] / (forwards[k]["forwards"] * forward_ms[f"patches{forwards[k]['patches_per_forward']}"]), 3)
                                       for k in med}}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
