#!/usr/bin/env python
"""Connected regions and the sieve on the GPU: what rua_scene_regions and rua_scene_sieve cost, next to the one-pass kernels of the
scoring tail and to scipy on the host.  Prints one JSON line and writes it to `--out` (default
profiles/scenes/bench_scene_sieve.json).

Five seeded 6000 x 6000 maps with 6 classes: `blocky` (uniform 16 x 16 regions), `noise` (every pixel drawn on its own: 30 million
regions), `uniform` (one region across every tile seam), `serpentine` (a one-pixel path along every other row that turns at
alternating ends: one region, the longest chain of unions) and, with --scene_net, `stitched` (Model.predict_scene of a --net_scene
scene by the cfg3 network, tiled to the map size: the speckle a real arg-max map has).  Device events around `--reps` back-to-back
calls after a warm-up, `--rounds` times; every round's ms per call is reported, `ms` is their median and `spread_ms` their max - min.

  regions_c4 regions_c8     rua_scene_regions (labels, areas and the per-class counts) per map, 4- and 8-connected
  sieve_void sieve_fill     rua_scene_sieve alone (min_area 69, every class) on the labels of the 4-connected run, per map
  erode_r3 boundary_r3      rua_scene_erode (map and matrix) at radius 3 and rua_scene_boundary (counts) at tolerance 3 on the same map,
                            scored against itself rolled by (2, 1): the one-pass yardsticks of this path
  host                      scipy.ndimage.label of every class of the map on this machine's CPU (where scipy imports), one run per
                            map; the kernel's number of regions is held against scipy's on the way
  scene                     with --scene_net: Model.predict_scene of the --net_scene scene without and with sieve=69 (fill), wall clock
                            in a device synchronise, ms per scene per round, and their difference per round
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


def serpentine(size):
    m = np.zeros((size, size), np.uint8)
    m[::2] = 1
    for k, i in enumerate(range(1, size, 2)):
        m[i, size - 1 if k % 2 == 0 else 0] = 1
    return m


def scipy_regions(m):
    """(number of 4-connected regions over all byte values, seconds) by scipy.ndimage.label, or None where scipy is missing."""
    try:
        from scipy import ndimage
    except ImportError:
        return None
    t0 = time.perf_counter()
    n = sum(int(ndimage.label(m == v)[1]) for v in np.unique(m))
    return n, time.perf_counter() - t0


def scene_rows(args, pool, model):
    plain, sieved = [], []
    for _ in range(args.rounds):
        t, _ = clock_ms(lambda: model.predict_scene(pool, 0, stride=P, batch=B, norm_type=1), args.net_warmup, args.net_reps)
        plain.append(t)
        t, (_, _, report) = clock_ms(lambda: model.predict_scene(pool, 0, stride=P, batch=B, norm_type=1, sieve=MIN_AREA), args.net_warmup, args.net_reps)
        sieved.append(t)
    S = args.net_scene
    return {"scene": [S, S, CIN], "model": {"shape": [B, P, P, CIN], "classes": CLASSES, "dtype": "bf16"}, "warmup": args.net_warmup,
            "reps": args.net_reps, "plain_ms": [round(v, 3) for v in plain], "sieve_ms": [round(v, 3) for v in sieved],
            "extra_ms": [round(b - a, 3) for a, b in zip(plain, sieved)], "region_counts": report["counts"].tolist(), "changed": report["changed"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10, help="back-to-back calls per round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scene", type=int, default=6000, help="map edge in pixels")
    ap.add_argument("--scene_net", action="store_true", help="also time Model.predict_scene(sieve=69) on a --net_scene scene, and add its map")
    ap.add_argument("--net_scene", type=int, default=2048)
    ap.add_argument("--net_reps", type=int, default=3)
    ap.add_argument("--net_warmup", type=int, default=3)
    ap.add_argument("--no_host", action="store_true", help="skip scipy on the host")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scenes", "bench_scene_sieve.json"))
    args = ap.parse_args()
    import torch
    from resunet_a_mltsk_keras_amd import _lib as L
    from resunet_a_mltsk_keras_amd import scenes
    if not torch.cuda.is_available():
        sys.exit("bench_scene_sieve.py needs a GPU")
    S = args.scene
    maps = make_maps(S)
    maps["serpentine"] = serpentine(S)
    res = {"scene": [S, S], "classes": CLASSES, "min_area": MIN_AREA, "reps": args.reps, "rounds": args.rounds}
    if args.scene_net:
        rng = np.random.default_rng(0)
        N = args.net_scene
        pool = scenes.ScenePool([rng.integers(0, 256, (N, N, CIN), dtype=np.uint8)], [make_maps(N)["blocky"]], patch=P)
        model = cfg3_model()
        res["scene_net"] = scene_rows(args, pool, model)
        pred = model.predict_scene(pool, 0, stride=P, batch=B, norm_type=1)[0]
        maps["stitched"] = np.ascontiguousarray(np.tile(pred, (S // N + 1, S // N + 1))[:S, :S])
        del pool, model
        torch.cuda.empty_cache()
    lib = L.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr1 = lambda t: (ctypes.c_void_p * 1)(t.data_ptr())
    hs = (ctypes.c_int32 * 1)(S)
    labels, areas = (torch.empty((S, S), dtype=torch.int32, device="cuda") for _ in range(2))
    out = torch.empty((S, S), dtype=torch.uint8, device="cuda")
    work = torch.empty((int(lib.raw("rua_scene_sieve_work_bytes")(S, S, CLASSES)) // 4,), dtype=torch.int32, device="cuda")
    counts = torch.zeros((CLASSES, 3), dtype=torch.int64, device="cuda")
    changed = torch.zeros((1,), dtype=torch.int64, device="cuda")
    conf = torch.zeros((CLASSES, CLASSES), dtype=torch.int64, device="cuda")
    bcounts = torch.zeros((CLASSES, 4), dtype=torch.int64, device="cuda")
    timed = lambda fn: median_row(rounds_ms(fn, args.rounds, args.reps))
    for name, m in maps.items():
        dev = torch.from_numpy(m).cuda()
        rolled = torch.from_numpy(np.roll(m, (2, 1), (0, 1)).copy()).cuda()

        def regions(conn):
            lib.call("rua_scene_regions", ptr1(dev), hs, hs, 1, conn, ptr1(labels), ptr1(areas), MIN_AREA, CLASSES, counts.data_ptr(), stream)

        def sieve(mode):
            lib.call("rua_scene_sieve", ptr1(dev), hs, hs, 1, 4, MIN_AREA, CLASSES, (1 << CLASSES) - 1, mode, ptr1(labels), ptr1(areas), ptr1(out),
                     work.data_ptr(), work.numel() * 4, changed.data_ptr(), stream)

        row = {"regions_c8": timed(lambda: regions(8)), "regions_c4": timed(lambda: regions(4))}
        counts.zero_()
        regions(4)                               # the labels the sieve reads, and the counts of one call
        row["sieve_void"] = timed(lambda: sieve(0))
        row["sieve_fill"] = timed(lambda: sieve(1))
        changed.zero_()
        sieve(1)
        row["erode_r3"] = timed(lambda: lib.call("rua_scene_erode", ptr1(dev), hs, hs, 1, 3, ptr1(out), ptr1(rolled), CLASSES, conf.data_ptr(), stream))
        row["boundary_r3"] = timed(lambda: lib.call("rua_scene_boundary", ptr1(dev), ptr1(rolled), hs, hs, 1, 3, CLASSES, None, None, bcounts.data_ptr(), stream))
        torch.cuda.synchronize()
        row["region_counts"] = counts.cpu().numpy().tolist()
        row["fill_changed"] = int(changed.cpu().numpy()[0])
        row["regions"] = int((areas > 0).sum().item())
        host = None if args.no_host else scipy_regions(m)
        if host is not None:
            assert host[0] == row["regions"], (name, host[0], row["regions"])
            row["host"] = {"ms": round(host[1] * 1e3, 1), "note": "scipy.ndimage.label of every class, one run on this machine's CPU"}
        res[name] = row
        del dev, rolled
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
