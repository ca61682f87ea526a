#!/usr/bin/env python
"""The precision-recall sweep on the GPU: what rua_scene_area_open and rua_scene_sweep_hist cost, next to the per-level composition
of the entries that existed before them and to scipy on the host.  Prints one JSON line and writes it to `--out` (default
profiles/scenes/bench_scene_sweep.json).

Seeded 6000 x 6000 uint8 probability maps: `blocky` (16 x 16 blocks of one random byte each), `noise` (every pixel drawn on its
own), `uniform` (200 everywhere), `smooth` (noise under a 15 x 15 box filter, stretched to 0..255: the shape a network's
probabilities have) and, with --scene_net, `stitched` (class 1 of the seg map of Model.predict_scene(heads=("seg",)) of a
--net_scene scene by the cfg3 network, tiled to the map size).  The class map is the 16 x 16 blocks of tools/_scene_bench.py, class 1
positive.  Device events around `--reps` back-to-back calls after a warm-up, `--rounds` times; every round's ms per call is
reported, `ms` is their median and `spread_ms` their max - min.

  hist                      rua_scene_sweep_hist (probabilities and an opened map against the class map), per map
  open_a1_T51 open_a1_T255  rua_scene_area_open at min_area 1 (the table pass) with 51 and 255 levels
  open_a69_T{51,255}_c{4,8} rua_scene_area_open at min_area 69, 51 and 255 levels, 4- and 8-connected
  compose_T51 compose_T255  the same curve from the entries of before, level by level: torch binarises, rua_scene_regions labels the
                            whole binary map, rua_scene_sieve in void mode removes the small regions of class 1, torch counts TP
                            and FP; min_area 69, 4-connected, nothing read back before the end (`--compose_reps` calls per round);
                            its TP and FP are held against rua_scene_sweep_hist's on the way
  host                      scipy.ndimage.label of the map binarised at level 128 on this machine's CPU (where scipy imports), one
                            run, and that time multiplied by 51 and 255: an EXTRAPOLATION, not a measured curve
  scene                     with --scene_net: Model.predict_scene of the --net_scene scene with heads=("seg",) and with
                            sweep=dict(positive=1, min_area=69), wall clock in a device synchronise, ms per scene per round
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

from _scene_bench import B, CIN, CLASSES, P, cfg3_model, clock_ms, make_maps, median_row, rounds_ms  # noqa: E402

MIN_AREA = 69                                  # the reference's area opening
POSITIVE = 1


def box(a, r):
    """the (2 r + 1)^2 box sums of a, borders wrapped"""
    c = np.cumsum(np.concatenate([a[-r - 1:], a, a[:r]], 0), 0, dtype=np.float64)
    a = c[2 * r + 1:] - c[:-2 * r - 1]
    c = np.cumsum(np.concatenate([a[:, -r - 1:], a, a[:, :r]], 1), 1, dtype=np.float64)
    return c[:, 2 * r + 1:] - c[:, :-2 * r - 1]


def prob_maps(size, seed=0):
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 256, (size // 16 + 1, size // 16 + 1), dtype=np.uint8)
    blocky = np.ascontiguousarray(np.kron(f, np.ones((16, 16), np.uint8))[:size, :size])
    noise = rng.integers(0, 256, (size, size), dtype=np.uint8)
    s = box(rng.random((size, size)), 7)
    smooth = np.rint(255 * (s - s.min()) / (s.max() - s.min())).astype(np.uint8)
    return {"blocky": blocky, "noise": noise, "uniform": np.full((size, size), 200, np.uint8), "smooth": smooth}


def scipy_level(m, level=128):
    try:
        from scipy import ndimage
    except ImportError:
        return None
    t0 = time.perf_counter()
    n = int(ndimage.label(m >= level)[1])
    return n, time.perf_counter() - t0


def scene_rows(args, pool, model):
    seg, swept = [], []
    sweep = dict(positive=POSITIVE, min_area=MIN_AREA)
    for _ in range(args.rounds):
        t, _ = clock_ms(lambda: model.predict_scene(pool, 0, stride=P, batch=B, norm_type=1, heads=("seg",)), args.net_warmup, args.net_reps)
        seg.append(t)
        t, _ = clock_ms(lambda: model.predict_scene(pool, 0, stride=P, batch=B, norm_type=1, sweep=sweep), args.net_warmup, args.net_reps)
        swept.append(t)
    S = args.net_scene
    return {"scene": [S, S, CIN], "model": {"shape": [B, P, P, CIN], "classes": CLASSES, "dtype": "bf16"}, "warmup": args.net_warmup,
            "reps": args.net_reps, "heads_seg_ms": [round(v, 3) for v in seg], "sweep_ms": [round(v, 3) for v in swept],
            "extra_ms": [round(b - a, 3) for a, b in zip(seg, swept)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3, help="back-to-back calls per round")
    ap.add_argument("--compose_reps", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--scene", type=int, default=6000, help="map edge in pixels")
    ap.add_argument("--maps", nargs="*", default=None, help="only these maps")
    ap.add_argument("--scene_net", action="store_true", help="also time Model.predict_scene(sweep=) on a --net_scene scene, and add its map")
    ap.add_argument("--net_scene", type=int, default=2048)
    ap.add_argument("--net_reps", type=int, default=3)
    ap.add_argument("--net_warmup", type=int, default=3)
    ap.add_argument("--no_host", action="store_true", help="skip scipy on the host")
    ap.add_argument("--no_compose", action="store_true", help="skip the per-level composition")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scenes", "bench_scene_sweep.json"))
    args = ap.parse_args()
    import torch
    from resunet_a_mltsk_keras_amd import _lib as L
    from resunet_a_mltsk_keras_amd import scenes
    if not torch.cuda.is_available():
        sys.exit("bench_scene_sweep.py needs a GPU")
    S = args.scene
    maps = prob_maps(S)
    res = {"scene": [S, S], "classes": CLASSES, "positive": POSITIVE, "min_area": MIN_AREA, "reps": args.reps, "compose_reps": args.compose_reps,
           "rounds": args.rounds}
    if args.scene_net:
        rng = np.random.default_rng(0)
        N = args.net_scene
        pool = scenes.ScenePool([rng.integers(0, 256, (N, N, CIN), dtype=np.uint8)], [make_maps(N)["blocky"]], patch=P)
        model = cfg3_model()
        res["scene_net"] = scene_rows(args, pool, model)
        seg = model.predict_scene(pool, 0, stride=P, batch=B, norm_type=1, heads=("seg",))[-1]["seg"][..., POSITIVE]
        maps["stitched"] = np.ascontiguousarray(np.tile(seg, (S // N + 1, S // N + 1))[:S, :S])
        del pool, model
        torch.cuda.empty_cache()
    if args.maps:
        maps = {k: v for k, v in maps.items() if k in args.maps}
    lib = L.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr1 = lambda t: (ctypes.c_void_p * 1)(t.data_ptr())
    hs = (ctypes.c_int32 * 1)(S)
    labels, areas = (torch.empty((S, S), dtype=torch.int32, device="cuda") for _ in range(2))
    opened, out = (torch.empty((S, S), dtype=torch.uint8, device="cuda") for _ in range(2))
    hist = torch.zeros((2, 2, 256), dtype=torch.int64, device="cuda")
    cls = torch.from_numpy(make_maps(S)["blocky"]).cuda()
    pos, neg = cls == POSITIVE, (cls < CLASSES) & (cls != POSITIVE)
    level_sets = {51: scenes.sweep_levels(list(range(255, 0, -5))), 255: scenes.sweep_levels()}
    timed = lambda fn, reps=args.reps: median_row(rounds_ms(fn, args.rounds, reps, warmup=1))
    for name, m in maps.items():
        dev = torch.from_numpy(m).cuda()

        def area_open(T, min_area, conn):
            lv = level_sets[T]
            work = min_area > 1
            lib.call("rua_scene_area_open", ptr1(dev), hs, hs, 1, 1, lv.ctypes.data, len(lv), min_area, conn, ptr1(opened),
                     ptr1(labels) if work else None, ptr1(areas) if work else None, stream)

        def sweep_hist():
            lib.call("rua_scene_sweep_hist", ptr1(dev), ptr1(opened), ptr1(cls), hs, hs, 1, 1, POSITIVE, CLASSES, hist.data_ptr(), stream)

        def compose(T):
            tp, fp = [], []
            for t in level_sets[T].tolist():
                binary = (dev >= t).to(torch.uint8)
                lib.call("rua_scene_regions", ptr1(binary), hs, hs, 1, 4, ptr1(labels), ptr1(areas), MIN_AREA, 2, None, stream)
                lib.call("rua_scene_sieve", ptr1(binary), hs, hs, 1, 4, MIN_AREA, 2, 2, 0, ptr1(labels), ptr1(areas), ptr1(out), None, 0, None, stream)
                kept = out == 1
                tp.append((kept & pos).sum())
                fp.append((kept & neg).sum())
            return torch.stack(tp), torch.stack(fp)

        row = {}
        for T in (51, 255):
            row[f"open_a1_T{T}"] = timed(lambda: area_open(T, 1, 4))
            for conn in (4, 8):
                row[f"open_a{MIN_AREA}_T{T}_c{conn}"] = timed(lambda: area_open(T, MIN_AREA, conn))
        area_open(51, MIN_AREA, 4)                 # the opened map the histogram reads, and the curve the composition is held against
        row["hist"] = timed(sweep_hist)
        hist.zero_()
        sweep_hist()
        torch.cuda.synchronize()
        scores = scenes.sweep_scores(hist.cpu().numpy(), level_sets[51])
        row["settled_pixels"] = int((opened > 0).sum().item())
        row["average_precision"] = round(scores["average_precision"], 6)
        if not args.no_compose:
            tp, fp = compose(51)
            assert np.array_equal(tp.cpu().numpy(), scores["tp"]) and np.array_equal(fp.cpu().numpy(), scores["fp"]), name
            for T in (51, 255):
                row[f"compose_T{T}"] = timed(lambda: compose(T), args.compose_reps)
        host = None if args.no_host else scipy_level(m)
        if host is not None:
            ms = host[1] * 1e3
            row["host"] = {"level_128_ms": round(ms, 1), "components": host[0], "T51_ms_extrapolated": round(51 * ms, 1),
                           "T255_ms_extrapolated": round(255 * ms, 1),
                           "note": "scipy.ndimage.label of the map binarised at level 128, one run on this machine's CPU, times the number of levels"}
        res[name] = row
        del dev
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
