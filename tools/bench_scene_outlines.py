#!/usr/bin/env python
"""Outlines of whole-scene instance maps on the GPU: what rua_scene_outline_count and rua_scene_outline_rings cost, next to
rua_scene_instances and to the host-side trace a user would otherwise write.  Prints one JSON line and writes it to `--out` (default
profiles/scenes/bench_scene_outlines.json).

Seeded 6000 x 6000 int32 id maps:
  blocky      the 4-connected regions of a 6-class map of 16 x 16 blocks, numbered by rua_scene_instances at radius 0
  uniform     one object that fills the map: four vertices, 24000 edges
  noise       every pixel its own draw out of 1000 ids: E near 4 H W, the worst case for memory (24 bytes of work per edge)
  serpentine  a one-pixel path through every other row: ONE ring of H W + 2 edges, the longest list to rank
  stitched    with --scene_net: the instance map Model.predict_scene(instances={..., "map": True}) leaves of a --net_scene scene by
              the cfg3 network, tiled to the map size
Device events around `--reps` back-to-back calls after a warm-up, `--rounds` times; every round's ms per call is reported, `ms` is
their median and `spread_ms` their max - min.

  count                     rua_scene_outline_count, with E, V
  rings                     rua_scene_outline_rings alone, with R, the rounds ceil(log2 E) and the work buffer's size
  instances_r0              blocky, uniform: rua_scene_instances at radius 0, the call that wrote the map
  fetch                     the copy of the int32 id map into pinned host memory that a host-side trace would start with
  host_jumping              scenes.host_outlines_jumping - the kernels' stages in numpy - on the top left --host_crop^2 pixels, one run
                            on this machine's CPU, and that time scaled by the pixel ratio to the full map
  host_walk                 scenes.host_outlines, the Python walk, on the top left 512 x 512 pixels, scaled alike
  scene                     with --scene_net: Model.predict_scene(instances=...) of the --net_scene scene without and with
                            "outlines", wall clock in a device synchronise, ms per scene per round, and their difference per round
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

INSTANCES = {"classes": list(range(CLASSES)), "bound_below": 256, "min_seed": 8, "radius": 4}


def serpentine(S):
    m = np.full((S, S), -1, np.int32)
    m[::2] = 0
    for k, i in enumerate(range(1, S - 1 if S % 2 else S, 2)):
        m[i, -1 if k % 2 == 0 else 0] = 0
    return m


def host_rows(m, crop):
    """the two host-side traces on crops of m, one run each, scaled to the whole map by pixels"""
    from resunet_a_mltsk_keras_amd import scenes
    out = {}
    for key, fn, c in (("host_jumping", scenes.host_outlines_jumping, crop), ("host_walk", scenes.host_outlines, 512)):
        part = np.ascontiguousarray(m[:c, :c])
        t0 = time.perf_counter()
        rings, _ = fn(part)
        ms = (time.perf_counter() - t0) * 1e3
        out[key] = {"crop": list(part.shape), "rings": len(rings), "ms": round(ms, 1), "scaled_ms": round(ms * m.size / part.size, 1),
                    "note": "one run on this machine's CPU; scaled_ms = ms x (map pixels / crop pixels)"}
    return out


def scene_rows(args, pool, model):
    plain, traced = [], []
    for _ in range(args.rounds):
        t, _ = clock_ms(lambda: model.predict_scene(pool, 0, stride=P, batch=B, norm_type=1, instances=INSTANCES), args.net_warmup, args.net_reps)
        plain.append(t)
        t, (_, _, report) = clock_ms(lambda: model.predict_scene(pool, 0, stride=P, batch=B, norm_type=1, instances={**INSTANCES, "outlines": True}),
                                     args.net_warmup, args.net_reps)
        traced.append(t)
    S = args.net_scene
    return {"scene": [S, S, CIN], "model": {"shape": [B, P, P, CIN], "classes": CLASSES, "dtype": "bf16"}, "warmup": args.net_warmup,
            "reps": args.net_reps, "instances_ms": [round(v, 3) for v in plain], "outlines_ms": [round(v, 3) for v in traced],
            "extra_ms": [round(b - a, 3) for a, b in zip(plain, traced)], "n": report["n"], "gt_n": report["gt_n"],
            "rings": len(report["outlines"][0]), "rings_true": len(report["outlines_true"][0])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="back-to-back calls per round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scene", type=int, default=6000, help="map edge in pixels")
    ap.add_argument("--scene_net", action="store_true", help="also time Model.predict_scene(instances=) with outlines on a --net_scene scene, and add its map")
    ap.add_argument("--net_scene", type=int, default=2048)
    ap.add_argument("--net_reps", type=int, default=3)
    ap.add_argument("--net_warmup", type=int, default=3)
    ap.add_argument("--host_crop", type=int, default=2048, help="edge of the crop scenes.host_outlines_jumping is timed on")
    ap.add_argument("--no_host", action="store_true", help="skip the host-side traces")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scenes", "bench_scene_outlines.json"))
    args = ap.parse_args()
    import torch
    from resunet_a_mltsk_keras_amd import _lib as L
    from resunet_a_mltsk_keras_amd import scenes
    if not torch.cuda.is_available():
        sys.exit("bench_scene_outlines.py needs a GPU")
    S = args.scene
    res = {"scene": [S, S], "reps": args.reps, "rounds": args.rounds}
    lib = L.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    timed = lambda fn: median_row(rounds_ms(fn, args.rounds, args.reps))
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device="cuda")
    class_maps = make_maps(S)
    families = {"blocky": class_maps["blocky"], "uniform": class_maps["uniform"],
                "noise": np.random.default_rng(2).integers(0, 1000, (S, S), dtype=np.int32), "serpentine": serpentine(S)}
    if args.scene_net:
        rng = np.random.default_rng(0)
        N = args.net_scene
        pool = scenes.ScenePool([rng.integers(0, 256, (N, N, CIN), dtype=np.uint8)], [make_maps(N)["blocky"]], patch=P)
        model = cfg3_model()
        res["scene_net"] = scene_rows(args, pool, model)
        inst = model.predict_scene(pool, 0, stride=P, batch=B, norm_type=1, instances={**INSTANCES, "map": True})[-1]["inst"]
        families["stitched"] = np.ascontiguousarray(np.tile(inst, (S // N + 1, S // N + 1))[:S, :S])
        del pool, model
        torch.cuda.empty_cache()
    pinned = torch.empty((S, S), dtype=torch.int32).pin_memory()
    base, n = i32(S, S), torch.empty((2,), dtype=torch.int64, device="cuda")
    cwork = i32(int(lib.raw("rua_scene_outline_work_bytes")(S, S, 0)) // 4)
    for name, m in families.items():
        row = {}
        if m.dtype == np.uint8:
            # the objects of a class map, as predict_scene builds them: seed map, regions, instances at radius 0
            cls = torch.from_numpy(m).cuda()
            marker = torch.empty((S, S), dtype=torch.uint8, device="cuda")
            labels, areas, inst = i32(S, S), i32(S, S), i32(S, S)
            cap = 1 << 20
            table, n2 = torch.zeros((cap, 8), dtype=torch.int32, device="cuda"), i32(2)
            iwork = i32(int(lib.raw("rua_scene_instances_work_bytes")(S, S)) // 4)
            one = lambda t: (ctypes.c_void_p * 1)(t.data_ptr())
            hs = (ctypes.c_int32 * 1)(S)
            mask = (1 << CLASSES) - 1
            lib.call("rua_scene_seed_map", cls.data_ptr(), None, None, S, S, CLASSES, mask, 256, 0, marker.data_ptr(), stream)
            lib.call("rua_scene_regions", one(marker), hs, hs, 1, 4, one(labels), one(areas), 1, 1, None, stream)

            def grow():
                table.zero_()
                lib.call("rua_scene_instances", cls.data_ptr(), marker.data_ptr(), labels.data_ptr(), areas.data_ptr(), S, S, CLASSES, mask, 1, 0,
                         iwork.data_ptr(), iwork.numel() * 4, inst.data_ptr(), table.data_ptr(), cap, n2.data_ptr(), stream)
            row["instances_r0"] = timed(grow)
            row["objects"] = int(n2.cpu().numpy()[0])
            host_map = inst.cpu().numpy()
            del cls, marker, labels, areas, table, iwork
        else:
            host_map = m
            inst = torch.from_numpy(m).cuda()
        count = lambda: lib.call("rua_scene_outline_count", inst.data_ptr(), S, S, 4, base.data_ptr(), cwork.data_ptr(), cwork.numel() * 4, n.data_ptr(), stream)
        row["count"] = timed(count)
        E, V = (int(v) for v in n.cpu().numpy())
        nwork = int(lib.raw("rua_scene_outline_work_bytes")(S, S, E))
        row.update(E=E, V=V, rounds_of_jumping=(E - 1).bit_length(), work_bytes=nwork)
        if E:
            work, rings, verts = torch.empty((nwork,), dtype=torch.uint8, device="cuda"), i32(V // 4, 6), i32(V, 2)
            trace = lambda: lib.call("rua_scene_outline_rings", inst.data_ptr(), base.data_ptr(), S, S, 4, E, V, work.data_ptr(), nwork, rings.data_ptr(),
                                     verts.data_ptr(), n.data_ptr(), stream)
            row["rings"] = timed(trace)
            row["R"] = int(n.cpu().numpy()[0])
            del work, rings, verts
        row["fetch"] = timed(lambda: pinned.copy_(inst, non_blocking=True))
        if not args.no_host:
            row.update(host_rows(host_map, args.host_crop))
        res[name] = row
        del inst
        torch.cuda.empty_cache()
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
