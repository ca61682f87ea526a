#!/usr/bin/env python
"""Instances from whole-scene maps on the GPU: what rua_scene_seed_map, rua_scene_regions + rua_scene_instances and
rua_scene_instance_match cost, next to the host composition a user would write with scipy.  Prints one JSON line and writes it to
`--out` (default profiles/scenes/bench_scene_instances.json).

Seeded 6000 x 6000 maps with 6 classes, the families of tools/bench_scene_sieve.py: `blocky` (uniform 16 x 16 regions), `noise`
(every pixel drawn on its own), `uniform` (one region) and, with --scene_net, `stitched` (Model.predict_scene of a --net_scene scene
by the cfg3 network, tiled to the map size).  The boundary map is synthesised: 255 on scenes.host_boundaries of the map dilated by one
pixel, 40 elsewhere, in every channel; the seeds are the pixels of every class off that band.  Device events around `--reps`
back-to-back calls after a warm-up, `--rounds` times; every round's ms per call is reported, `ms` is their median and `spread_ms`
their max - min.

  seed_map                  rua_scene_seed_map with the boundary map, per map
  regions                   rua_scene_regions of the marker (4-connected): what rua_scene_instances reads
  instances_r0 _r4 _r16     rua_scene_instances alone (min_seed 8) at radius 0, 4 and 16, with `n` and `ungrown` of the radius-4 run
  match match_many          rua_scene_instance_match of the radius-4 instances against the 4-connected regions of two seeded block
                            maps: 256 x 256 blocks (a few hundred objects) and 8 x 8 blocks (more than 10^5 objects), with the
                            number of objects and of predictions that found one
  host                      scipy on this machine's CPU (where it imports), one run per map: ndimage.label of every class of the
                            marker, distance_transform_edt(return_indices=True) of the complement, the nearest seed's label within
                            4 pixels on the pixels of its class, and np.unique over the (predicted, true) pairs
  scene                     with --scene_net: Model.predict_scene of the --net_scene scene without and with instances= (every
                            class, boundary below 0.5, min_seed 8, radius 4), wall clock in a device synchronise, ms per scene per
                            round, and their difference per round
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

MIN_SEED, RADIUS = 8, 4
INSTANCES = {"classes": list(range(CLASSES)), "bound_below": 0.5, "min_seed": MIN_SEED, "radius": RADIUS}


def boundary_band(m):
    """True on the class boundaries of m (scenes.host_boundaries: a class pixel with a 4-neighbour of another byte), dilated by one pixel"""
    from resunet_a_mltsk_keras_amd import scenes
    edge = scenes.host_boundaries(m, CLASSES) != 255
    wide = edge.copy()
    wide[1:] |= edge[:-1]; wide[:-1] |= edge[1:]; wide[:, 1:] |= edge[:, :-1]; wide[:, :-1] |= edge[:, 1:]
    return wide


def scipy_pipeline(m, band, truth):
    """(predicted objects, seconds) of the host composition, or None where scipy is missing."""
    try:
        from scipy import ndimage
    except ImportError:
        return None
    t0 = time.perf_counter()
    seeds = np.zeros(m.shape, np.int32)
    n = 0
    for c in np.unique(m):
        lab, k = ndimage.label((m == c) & ~band)
        size = np.bincount(lab.ravel(), minlength=k + 1)
        lab[size[lab] < MIN_SEED] = 0
        seeds[lab > 0] = lab[lab > 0] + n
        n += k
    d, (ii, jj) = ndimage.distance_transform_edt(seeds == 0, return_indices=True)
    near = seeds[ii, jj]
    inst = np.where((d <= RADIUS) & (m[ii, jj] == m), near, 0)
    pairs = inst.astype(np.int64) * (int(truth.max()) + 1) + truth
    np.unique(pairs[(inst > 0) & (truth > 0)], return_counts=True)
    return int(len(np.unique(seeds)) - 1), time.perf_counter() - t0


def scene_rows(args, pool, model):
    plain, objects = [], []
    for _ in range(args.rounds):
        t, _ = clock_ms(lambda: model.predict_scene(pool, 0, stride=P, batch=B, norm_type=1), args.net_warmup, args.net_reps)
        plain.append(t)
        t, (_, _, report) = clock_ms(lambda: model.predict_scene(pool, 0, stride=P, batch=B, norm_type=1, instances=INSTANCES), args.net_warmup, args.net_reps)
        objects.append(t)
    S = args.net_scene
    return {"scene": [S, S, CIN], "model": {"shape": [B, P, P, CIN], "classes": CLASSES, "dtype": "bf16"}, "warmup": args.net_warmup,
            "reps": args.net_reps, "plain_ms": [round(v, 3) for v in plain], "instances_ms": [round(v, 3) for v in objects],
            "extra_ms": [round(b - a, 3) for a, b in zip(plain, objects)], "n": report["n"], "gt_n": report["gt_n"], "ungrown": report["ungrown"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10, help="back-to-back calls per round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scene", type=int, default=6000, help="map edge in pixels")
    ap.add_argument("--scene_net", action="store_true", help="also time Model.predict_scene(instances=) on a --net_scene scene, and add its map")
    ap.add_argument("--net_scene", type=int, default=2048)
    ap.add_argument("--net_reps", type=int, default=3)
    ap.add_argument("--net_warmup", type=int, default=3)
    ap.add_argument("--no_host", action="store_true", help="skip scipy on the host")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scenes", "bench_scene_instances.json"))
    args = ap.parse_args()
    import torch
    from resunet_a_mltsk_keras_amd import _lib as L
    from resunet_a_mltsk_keras_amd import scenes
    if not torch.cuda.is_available():
        sys.exit("bench_scene_instances.py needs a GPU")
    S = args.scene
    maps = make_maps(S)
    res = {"scene": [S, S], "classes": CLASSES, "min_seed": MIN_SEED, "reps": args.reps, "rounds": args.rounds}
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
    mask, cap = (1 << CLASSES) - 1, 1 << 20
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device="cuda")
    marker = torch.empty((S, S), dtype=torch.uint8, device="cuda")
    labels, areas, inst, inst_g = i32(S, S), i32(S, S), i32(S, S), i32(S, S)
    table, table_g, n = torch.zeros((cap, 8), dtype=torch.int32, device="cuda"), torch.zeros((cap, 8), dtype=torch.int32, device="cuda"), i32(2)
    work = i32(int(lib.raw("rua_scene_instances_work_bytes")(S, S)) // 4)
    mwork = i32(int(lib.raw("rua_scene_instance_match_work_bytes")(cap, cap)) // 4)
    match = i32(cap, 2)
    timed = lambda fn: median_row(rounds_ms(fn, args.rounds, args.reps))

    def objects_of(dev_map, into, tab):
        """the 4-connected regions of every class of a resident map as instances: (N, ungrown)"""
        lib.call("rua_scene_seed_map", dev_map.data_ptr(), None, None, S, S, CLASSES, mask, 256, 0, marker.data_ptr(), stream)
        lib.call("rua_scene_regions", ptr1(marker), hs, hs, 1, 4, ptr1(labels), ptr1(areas), 1, 1, None, stream)
        tab.zero_()
        lib.call("rua_scene_instances", dev_map.data_ptr(), marker.data_ptr(), labels.data_ptr(), areas.data_ptr(), S, S, CLASSES, mask, 1, 0,
                 work.data_ptr(), work.numel() * 4, into.data_ptr(), tab.data_ptr(), cap, n.data_ptr(), stream)
        return n.cpu().numpy().tolist()

    rng = np.random.default_rng(1)
    blocks = lambda k: torch.from_numpy(np.ascontiguousarray(np.kron(rng.integers(0, CLASSES, (S // k + 1, S // k + 1), dtype=np.uint8),
                                                                     np.ones((k, k), np.uint8))[:S, :S])).cuda()
    few, many = blocks(256), blocks(8)
    for name, m in maps.items():
        band = boundary_band(m)
        dev = torch.from_numpy(m).cuda()
        bound = torch.from_numpy(np.ascontiguousarray(np.where(band, 255, 40).astype(np.uint8)[..., None].repeat(CLASSES, 2))).cuda()

        def grow(radius):
            lib.call("rua_scene_instances", dev.data_ptr(), marker.data_ptr(), labels.data_ptr(), areas.data_ptr(), S, S, CLASSES, mask, MIN_SEED, radius,
                     work.data_ptr(), work.numel() * 4, inst.data_ptr(), table.data_ptr(), cap, n.data_ptr(), stream)

        def matched():
            lib.call("rua_scene_instance_match", inst.data_ptr(), table.data_ptr() + 8, cap, inst_g.data_ptr(), cap, S, S, mwork.data_ptr(), mwork.numel() * 4,
                     match.data_ptr(), stream)

        row = {}
        for key, other in (("match", few), ("match_many", many)):
            row[key + "_objects"] = objects_of(other, inst_g, table_g)[0]
            seed = lambda: lib.call("rua_scene_seed_map", dev.data_ptr(), bound.data_ptr(), None, S, S, CLASSES, mask, 128, 0, marker.data_ptr(), stream)
            regions = lambda: lib.call("rua_scene_regions", ptr1(marker), hs, hs, 1, 4, ptr1(labels), ptr1(areas), 1, 1, None, stream)
            if key == "match":
                row["seed_map"] = timed(seed)
                row["regions"] = timed(regions)
                for radius in (0, 16, 4):
                    table.zero_()
                    row[f"instances_r{radius}"] = timed(lambda: grow(radius))
                row["n"], row["ungrown"] = n.cpu().numpy().tolist()
            else:
                seed(); regions(); table.zero_(); grow(RADIUS)
            row[key] = timed(matched) if row["n"] <= cap and row[key + "_objects"] <= cap else None
            if row[key] is not None:
                row[key + "_matched"] = int((match[:row["n"], 0] >= 0).sum().item())
        host = None if args.no_host else scipy_pipeline(m, band, np.roll(m, (3, 2), (0, 1)).astype(np.int64) + 1)
        if host is not None:
            row["host"] = {"ms": round(host[1] * 1e3, 1), "seeds": host[0],
                           "note": "scipy.ndimage.label per class + distance_transform_edt(return_indices=True) + np.unique over pairs, one run on this machine's CPU"}
        res[name] = row
        del dev, bound
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
