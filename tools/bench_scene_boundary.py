#!/usr/bin/env python
"""The boundary F1 on the GPU: what rua_scene_boundary costs and what it replaces.  Prints one JSON line and writes it to `--out`
(default profiles/scenes/bench_scene_boundary.json).

The set-up of tools/bench_scene_erode.py: three seeded 6000 x 6000 class maps with 6 classes - `blocky` (uniform 16 x 16 regions),
`noise` (every pixel drawn on its own: nearly every pixel is a boundary pixel) and `uniform` (one class: no boundary at all) - and
for each a prediction, the class map rolled by (2, 1) with 1 % of its pixels redrawn.  Device events around `--reps` back-to-back
calls after a warm-up, `--rounds` times; every round's ms per call is reported, `ms` is their median and `spread_ms` their max - min.

  counts_r0 counts_r1 counts_r3 counts_r16   the counts alone on the blocky map (reads cls and pred) at four tolerances
  counts_r3_noise counts_r3_uniform          the same at tolerance 3 on the other two maps
  maps            the two boundary maps alone (reads cls and pred, writes both)
  all_r3          maps and counts in one pass
  erode_both_r3   rua_scene_erode, eroded map and matrix in one pass, on the same maps: a kernel of the same kind, as context
  host            scenes.host_boundary_counts on the blocky map at tolerance 3, on this machine's CPU; the kernel's counts and maps
                  are held against the host's on the way
  scene           with --scene_net: Model.predict_scene of a 2048 x 2048 scene (cfg3 network, bf16, batch 8) without and with
                  boundary=3, wall clock in a device synchronise, ms per scene per round, their difference per round, and the host
                  definition's time on the fetched map
  conditions      kernel_faster_than_host: counts_r3 < host;  scene_extra_below_host: every round's difference < the host's time
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


def make_pred(m, seed):
    rng = np.random.default_rng(seed)
    p = np.roll(m, (2, 1), (0, 1)).copy()
    k = rng.random(p.shape) < 0.01
    p[k] = rng.integers(0, CLASSES, int(k.sum()), dtype=np.uint8)
    return p


def scene_rows(args):
    """predict_scene without and with boundary=3 on a seeded scene, and the host definition on the map it fetched."""
    import torch
    from resunet_a_mltsk_keras_amd import scenes
    S = args.net_scene
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (S, S, CIN), dtype=np.uint8)
    cls = make_maps(S)["blocky"]
    pool = scenes.ScenePool([img], [cls], patch=P)
    m = cfg3_model()

    timed = lambda fn: clock_ms(fn, args.net_warmup, args.net_reps)
    plain, with_b = [], []
    for _ in range(args.rounds):
        t, _ = timed(lambda: m.predict_scene(pool, 0, stride=P, batch=B, norm_type=1))
        plain.append(t)
        t, (pred, _, counts) = timed(lambda: m.predict_scene(pool, 0, stride=P, batch=B, norm_type=1, boundary=3))
        with_b.append(t)
    t0 = time.perf_counter()
    want = scenes.host_boundary_counts(cls, pred, 3, CLASSES)
    host_ms = (time.perf_counter() - t0) * 1e3
    assert np.array_equal(counts, want)
    extra = [b - a for a, b in zip(plain, with_b)]
    return {"scene": [S, S, CIN], "model": {"shape": [B, P, P, CIN], "classes": CLASSES, "dtype": "bf16"}, "warmup": args.net_warmup,
            "reps": args.net_reps, "plain_ms": [round(v, 3) for v in plain], "boundary_r3_ms": [round(v, 3) for v in with_b],
            "extra_ms": [round(v, 3) for v in extra], "host_counts_ms": round(host_ms, 1), "boundary_f1": scenes.boundary_scores(counts)["f1"].round(2).tolist()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50, help="back-to-back calls per round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scene", type=int, default=6000, help="map edge in pixels")
    ap.add_argument("--scene_net", action="store_true", help="also time Model.predict_scene(boundary=3) on a --net_scene scene")
    ap.add_argument("--net_scene", type=int, default=2048)
    ap.add_argument("--net_reps", type=int, default=3)
    ap.add_argument("--net_warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scenes", "bench_scene_boundary.json"))
    args = ap.parse_args()
    import torch
    from resunet_a_mltsk_keras_amd import _lib as L
    from resunet_a_mltsk_keras_amd import scenes
    if not torch.cuda.is_available():
        sys.exit("bench_scene_boundary.py needs a GPU")
    S = args.scene
    maps = make_maps(S)
    names = list(maps)
    pred_host = {k: make_pred(maps[k], 1 + i) for i, k in enumerate(names)}
    cls = {k: torch.from_numpy(maps[k]).cuda() for k in names}
    prd = {k: torch.from_numpy(pred_host[k]).cuda() for k in names}
    bc, bp = (torch.empty((S, S), dtype=torch.uint8, device="cuda") for _ in range(2))
    eroded = torch.empty((S, S), dtype=torch.uint8, device="cuda")
    counts = torch.zeros((CLASSES, 4), dtype=torch.int64, device="cuda")
    conf = torch.zeros((CLASSES, CLASSES), dtype=torch.int64, device="cuda")
    lib, st = L.lib(), torch.cuda.current_stream()
    ptr1 = lambda t: (ctypes.c_void_p * 1)(t.data_ptr())
    hs = (ctypes.c_int32 * 1)(S)
    stream = ctypes.c_void_p(st.cuda_stream)

    def boundary(which, r, with_maps, with_counts):
        lib.call("rua_scene_boundary", ptr1(cls[which]), ptr1(prd[which]), hs, hs, 1, r, CLASSES, ptr1(bc) if with_maps else None,
                 ptr1(bp) if with_maps else None, counts.data_ptr() if with_counts else None, stream)

    def erode(which):
        lib.call("rua_scene_erode", ptr1(cls[which]), hs, hs, 1, 3, ptr1(eroded), ptr1(prd[which]), CLASSES, conf.data_ptr(), stream)

    timed = lambda fn: median_row(rounds_ms(fn, args.rounds, args.reps))

    res = {"scene": [S, S], "classes": CLASSES, "reps": args.reps, "rounds": args.rounds}
    for r in (0, 1, 3, 16):
        res[f"counts_r{r}"] = timed(lambda: boundary("blocky", r, False, True))
    res["counts_r3_noise"] = timed(lambda: boundary("noise", 3, False, True))
    res["counts_r3_uniform"] = timed(lambda: boundary("uniform", 3, False, True))
    res["maps"] = timed(lambda: boundary("blocky", 3, True, False))
    res["all_r3"] = timed(lambda: boundary("blocky", 3, True, True))
    res["erode_both_r3"] = timed(lambda: erode("blocky"))
    # the same numbers as the host's, while we are here: one call into zeroed counts
    counts.zero_()
    boundary("blocky", 3, True, True)
    torch.cuda.synchronize()
    got, got_bc, got_bp = counts.cpu().numpy(), bc.cpu().numpy(), bp.cpu().numpy()
    t0 = time.perf_counter()
    want = scenes.host_boundary_counts(maps["blocky"], pred_host["blocky"], 3, CLASSES)
    dt = time.perf_counter() - t0
    assert np.array_equal(got, want), (got.tolist(), want.tolist())
    assert np.array_equal(got_bc, scenes.host_boundaries(maps["blocky"], CLASSES)) and np.array_equal(got_bp, scenes.host_boundaries(pred_host["blocky"], CLASSES))
    res["host"] = {"ms": round(dt * 1e3, 1), "note": "scenes.host_boundary_counts on the blocky map at tolerance 3, one run on this machine's CPU"}
    res["counts_blocky_r3"] = got.tolist()
    res["boundary_fraction"] = {k: round(float((scenes.host_boundaries(maps[k], CLASSES) != 255).mean()), 4) for k in ("blocky", "noise")}
    res["conditions"] = {"kernel_faster_than_host": bool(res["counts_r3"]["ms"] < res["host"]["ms"]),
                         "host_over_kernel": round(res["host"]["ms"] / res["counts_r3"]["ms"], 1)}
    if args.scene_net:
        del cls, prd, bc, bp, eroded
        res["scene_net"] = scene_rows(args)
        res["conditions"]["scene_extra_below_host"] = bool(max(res["scene_net"]["extra_ms"]) < res["scene_net"]["host_counts_ms"])
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
