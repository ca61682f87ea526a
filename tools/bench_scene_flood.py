#!/usr/bin/env python
"""The flood on the GPU: what rua_scene_flood costs on whole-scene maps, next to rua_scene_instances at radius 4 and 16, and what
predict_scene(instances=) costs with and without it.  Prints one JSON line and writes it to `--out` (default
profiles/scenes/bench_scene_flood.json).

Seeded 6000 x 6000 maps with 6 classes, the families of tools/bench_scene_instances.py - `blocky`, `noise`, `uniform` and, with
--scene_net, `stitched` - with the same synthetic boundary band (seeds are the pixels off it, min_seed 8), and `discs`: the two
touching discs of radius 34 of tests/test_scene_flood_host.py tiled over the map, class 1 on class 0, with the exact distance to the
other class as the height and the seeds at height >= 160.  The height of the other maps is synthetic, a pyramid of period 64 (255 at
the centre of each cell, 8 levels per pixel), [H][W].  Device events around `--reps` back-to-back calls after a warm-up, `--rounds`
times; every round's ms per call is reported, `ms` is their median and `spread_ms` their max - min.  rua_scene_flood works in place, so
every timed call first restores inst, the table and n from a copy on the device; `restore` is that copy alone and `flood_*` the
figure with it taken off.

  instances_r4 _r16         rua_scene_instances alone at radius 4 and 16
  restore                   the device copies in front of every flood call
  flood_r0 flood_r4         rua_scene_flood at rounds_per_level 1, floor 0, drain 0 (256 rounds, 32 launches) from the radius-0 and
                            the radius-4 instances, with the height; `settled`, `last_round` and `ungrown` before and after
  flood_r0_flat _r4_flat    the same without a height (a geodesic grow of reach 256)
  scene                     with --scene_net: Model.predict_scene of the --net_scene scene with instances= (class 1 .. 5, boundary
                            below 0.5, min_seed 8, radius 4) without and with flood=True, wall clock in a device synchronise, ms per
                            scene per round, alternating, and their difference per round
  parent                    with --parent_tree DIR, a built checkout of the parent commit (git worktree add DIR HEAD~1; python -c
                            "import __graft_entry__ as g; g.build()" there): the same predict_scene(instances=) call WITHOUT flood
                            in that tree and in this one, each in a fresh child process, alternating --ab_rounds times - the
                            reference for "flood off costs nothing".  Without the option this leg is not covered.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from _scene_bench import B, CIN, CLASSES, P, cfg3_model, clock_ms, make_maps, median_row, rounds_ms  # noqa: E402
from bench_scene_instances import boundary_band  # noqa: E402

MIN_SEED = 8
INSTANCES = {"classes": list(range(1, CLASSES)), "bound_below": 0.5, "min_seed": MIN_SEED, "radius": 4}


def disc_cell():
    """(class map, height) of one 96 x 160 cell: two discs of radius 34, centres 58 apart, and the exact distance to the background
    scaled to bytes"""
    H, W = 96, 160
    yy, xx = np.mgrid[:H, :W]
    inside = ((yy - 48) ** 2 + (xx - 51) ** 2 <= 34 * 34) | ((yy - 48) ** 2 + (xx - 109) ** 2 <= 34 * 34)
    oy, ox = np.nonzero(~inside)
    d2 = np.full((H, W), 1 << 30, np.int64)
    for k0 in range(0, len(oy), 512):
        d2 = np.minimum(d2, ((yy[..., None] - oy[k0:k0 + 512]) ** 2 + (xx[..., None] - ox[k0:k0 + 512]) ** 2).min(-1))
    d = np.sqrt(d2.astype(np.float64))
    return inside.astype(np.uint8), np.rint(255.0 * d / d.max()).astype(np.uint8)


def tiled(cell, S):
    return np.ascontiguousarray(np.tile(cell, (S // cell.shape[0] + 1, S // cell.shape[1] + 1))[:S, :S])


def pyramid(S):
    k = np.abs(np.arange(S) % 64 - 32)
    return np.ascontiguousarray((255 - 8 * np.minimum(31, np.maximum(k[:, None], k[None, :]))).astype(np.uint8))


def scene_rows(args, pool, model):
    plain, flooded = [], []
    for _ in range(args.rounds):
        t, _ = clock_ms(lambda: model.predict_scene(pool, 0, stride=P, batch=B, norm_type=1, instances=INSTANCES), args.net_warmup, args.net_reps)
        plain.append(t)
        t, (_, _, report) = clock_ms(lambda: model.predict_scene(pool, 0, stride=P, batch=B, norm_type=1, instances={**INSTANCES, "flood": True}),
                                     args.net_warmup, args.net_reps)
        flooded.append(t)
    S = args.net_scene
    return {"scene": [S, S, CIN], "model": {"shape": [B, P, P, CIN], "classes": CLASSES, "dtype": "bf16"}, "warmup": args.net_warmup,
            "reps": args.net_reps, "instances_ms": [round(v, 3) for v in plain], "flood_ms": [round(v, 3) for v in flooded],
            "extra_ms": [round(b - a, 3) for a, b in zip(plain, flooded)], "n": report["n"], "ungrown": report["ungrown"], "flood": report["flood"]}


CHILD = """
import json, os, sys
root = os.path.abspath(sys.argv[1])
sys.path[:0] = [root, os.path.join(root, "tools")]
import numpy as np
from _scene_bench import B, CIN, CLASSES, P, cfg3_model, clock_ms, make_maps
from resunet_a_mltsk_keras_amd import scenes
assert os.path.abspath(scenes.__file__).startswith(root + os.sep), scenes.__file__
N, warmup, reps, rounds = (int(v) for v in sys.argv[2:6])
instances = json.loads(sys.argv[6])
pool = scenes.ScenePool([np.random.default_rng(0).integers(0, 256, (N, N, CIN), dtype=np.uint8)], [make_maps(N)["blocky"]], patch=P)
model = cfg3_model()
ms = [round(clock_ms(lambda: model.predict_scene(pool, 0, stride=P, batch=B, norm_type=1, instances=instances), warmup, reps)[0], 3) for _ in range(rounds)]
print(json.dumps({"ms": ms, "has_flood": hasattr(scenes, "host_flood")}))
"""


def parent_rows(args):
    """predict_scene(instances=) without flood in the parent's tree and in this one, a fresh process each, alternating"""
    rows = {"parent": [], "this": []}
    for _ in range(args.ab_rounds):
        for key, tree in (("parent", os.path.abspath(args.parent_tree)), ("this", ROOT)):
            out = subprocess.run([sys.executable, "-c", CHILD, tree, str(args.net_scene), str(args.net_warmup), str(args.net_reps), str(args.rounds),
                                  json.dumps(INSTANCES)], capture_output=True, text=True, timeout=300, cwd=tree)
            if out.returncode != 0:
                sys.exit(f"bench_scene_flood.py: the child in {tree} failed:\n{out.stderr[-2000:]}")
            got = json.loads(out.stdout.strip().splitlines()[-1])
            if got["has_flood"] != (key == "this"):
                sys.exit(f"bench_scene_flood.py: {tree} is not the {key} tree")
            rows[key].append(got["ms"])
    med = {k: float(np.median(np.concatenate(v))) for k, v in rows.items()}
    return {"parent_ms": rows["parent"], "this_ms": rows["this"], "parent_median_ms": round(med["parent"], 3), "this_median_ms": round(med["this"], 3),
            "note": "predict_scene(instances=) without flood; one list per process, processes alternate"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="back-to-back calls per round")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--scene", type=int, default=6000, help="map edge in pixels")
    ap.add_argument("--scene_net", action="store_true", help="also time Model.predict_scene(instances=) with and without flood on a --net_scene scene, and add its map")
    ap.add_argument("--net_scene", type=int, default=2048)
    ap.add_argument("--net_reps", type=int, default=3)
    ap.add_argument("--net_warmup", type=int, default=3)
    ap.add_argument("--parent_tree", default=None, help="a built checkout of the parent commit: also time predict_scene(instances=) without flood there and here")
    ap.add_argument("--ab_rounds", type=int, default=2, help="processes per tree of the --parent_tree comparison")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scenes", "bench_scene_flood.json"))
    args = ap.parse_args()
    import torch
    from resunet_a_mltsk_keras_amd import _lib as L
    from resunet_a_mltsk_keras_amd import scenes
    if not torch.cuda.is_available():
        sys.exit("bench_scene_flood.py needs a GPU")
    S = args.scene
    maps = make_maps(S)
    res = {"scene": [S, S], "classes": CLASSES, "min_seed": MIN_SEED, "reps": args.reps, "rounds": args.rounds,
           "flood": {"rounds_per_level": 1, "floor": 0, "drain": 0, "rounds": 256}}
    if args.parent_tree:
        res["flood_off_vs_parent"] = parent_rows(args)                       # before this process opens the GPU: one process at a time
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
    cell_cls, cell_h = disc_cell()
    maps["discs"] = tiled(cell_cls, S)
    lib = L.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr1 = lambda t: (ctypes.c_void_p * 1)(t.data_ptr())
    hs = (ctypes.c_int32 * 1)(S)
    cap = 1 << 20
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device="cuda")
    labels, areas, inst, inst0 = i32(S, S), i32(S, S), i32(S, S), i32(S, S)
    table, table0, n, n0, stats = torch.zeros((cap, 8), dtype=torch.int32, device="cuda"), i32(cap, 8), i32(2), i32(2), i32(2)
    work = i32(int(lib.raw("rua_scene_instances_work_bytes")(S, S)) // 4)
    fwork = i32(int(lib.raw("rua_scene_flood_work_bytes")(S, S)) // 4)
    timed = lambda fn: median_row(rounds_ms(fn, args.rounds, args.reps))
    for name, m in maps.items():
        dev = torch.from_numpy(m).cuda()
        if name == "discs":
            mask, h = 2, tiled(cell_h, S)
            marker = torch.from_numpy(np.where((m == 1) & (h >= 160), 1, 255).astype(np.uint8)).cuda()
        else:
            mask, h = (1 << CLASSES) - 1, pyramid(S)
            marker = torch.from_numpy(np.where(boundary_band(m), 255, m).astype(np.uint8)).cuda()
        height = torch.from_numpy(h).cuda()
        lib.call("rua_scene_regions", ptr1(marker), hs, hs, 1, 4, ptr1(labels), ptr1(areas), 1, 1, None, stream)

        def grow(radius):
            lib.call("rua_scene_instances", dev.data_ptr(), marker.data_ptr(), labels.data_ptr(), areas.data_ptr(), S, S, CLASSES, mask, MIN_SEED, radius,
                     work.data_ptr(), work.numel() * 4, inst.data_ptr(), table.data_ptr(), cap, n.data_ptr(), stream)

        def restore():
            inst.copy_(inst0); table.copy_(table0); n.copy_(n0)

        def flood(hp):
            restore()
            lib.call("rua_scene_flood", dev.data_ptr(), hp, 1, 0, S, S, CLASSES, mask, 4, 1, 0, 0, fwork.data_ptr(), fwork.numel() * 4, inst.data_ptr(),
                     table.data_ptr(), cap, n.data_ptr(), stats.data_ptr(), stream)

        row = {}
        for radius in (16, 4):
            table.zero_()
            row[f"instances_r{radius}"] = timed(lambda: grow(radius))
        for radius in (0, 4):
            table.zero_()
            grow(radius)
            inst0.copy_(inst); table0.copy_(table); n0.copy_(n)
            row["n"], row[f"ungrown_r{radius}"] = n.cpu().numpy().tolist()
            if row["n"] > cap:
                row[f"flood_r{radius}"] = None                                  # more seeds than the table holds
                continue
            rest = timed(restore)
            row["restore"] = rest
            for key, hp in ((f"flood_r{radius}", height.data_ptr()), (f"flood_r{radius}_flat", None)):
                both = rounds_ms(lambda: flood(hp), args.rounds, args.reps)
                row[key] = median_row([b - rest["ms"] for b in both])
                settled, last = stats.cpu().numpy().tolist()
                row[key].update(settled=settled, last_round=last, ungrown=n.cpu().numpy().tolist()[1])
        res[name] = row
        del dev, marker, height
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
