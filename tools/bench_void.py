#!/usr/bin/env python
"""Training on partly labelled patches (LossSpec.ignore_void): what the void mask and the masked launches cost.  Prints one JSON line.

  void_mask_us   rua_void_mask alone at B x 256 x 256 (B = 8, 6 classes, ~30 % void) for margin 0 / 2 / 8: device events around `--reps`
                 back-to-back calls after a warm-up, per call
  head_fwd_us    the fused head forward (bf16, Cin = 32, 6 classes, softmax, B x 256 x 256) through rua_head_fwd_loss_void with a mask of ~30 % void
                 and with none (= rua_head_fwd_loss_rep), alternating for `--rounds` rounds
  step_ms        the cfg3 step (bf16, 256 x 256 x 3, 6 classes, multitask, B = 8, single-GPU graph path) on a resident batch
                 (train_step(None, None), as bench.py measures), `--warmup` untimed and `--steps` timed steps per variant:
                   off        compiled without the option
                   on_0       ignore_void = 2, a class map without a void byte
                   on_30      ignore_void = 2, ~30 % of the pixels void (blocks of 16 x 16, before the margin)
                 Three models in one process; the variants alternate for `--rounds` rounds and every round's number is reported.
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


def class_maps(rng, B, S, C, void_share):
    f = rng.integers(0, C, (B, S // 16 + 1, S // 16 + 1))
    f[rng.random(f.shape) < void_share] = 255
    return np.kron(f, np.ones((1, 16, 16), np.int64))[:, :S, :S].astype(np.uint8)


def events(fn, reps):
    import torch
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) * 1e3 / reps, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    import torch
    from multitasking_utils import Tanimoto_dual_loss
    from resunet_a_mltsk_keras_amd import _lib as L
    from resunet_a_mltsk_keras_amd.engine import HEADS, ModelConfig
    from resunet_a_mltsk_keras_amd.keras_api import Adam, Model
    if not torch.cuda.is_available():
        sys.exit("bench_void.py needs a GPU")
    lib, B, S, C = L.lib(), 8, 256, 6
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(0)
    res = {}

    cls30 = class_maps(rng, B, S, C, 0.3)
    cls_d = torch.from_numpy(cls30).cuda()
    mask_d = torch.empty_like(cls_d)
    res["void_mask_us"] = {"shape": [B, S, S], "void_share_of_class_map": round(float((cls30 >= C).mean()), 3)}
    for mg in (0, 2, 8):
        res["void_mask_us"][f"margin_{mg}"] = events(lambda: lib.call("rua_void_mask", cls_d.data_ptr(), B, S, S, C, mg, mask_d.data_ptr(), st()), args.reps)
    lib.call("rua_void_mask", cls_d.data_ptr(), B, S, S, C, 2, mask_d.data_ptr(), st())
    torch.cuda.synchronize()
    res["void_mask_us"]["void_share_at_margin_2"] = round(float((mask_d != 0).float().mean()), 3)

    HW, Cin = S * S, 32
    x = torch.randn((B * HW, Cin), device="cuda").to(torch.bfloat16)
    w, b = torch.randn((C, Cin), device="cuda") / 4, torch.randn((C,), device="cuda")
    y = torch.nn.functional.one_hot(torch.randint(0, C, (B * HW,), device="cuda"), C).float()
    z, p = torch.empty((B * HW, C), device="cuda"), torch.empty((B * HW, C), device="cuda")
    sums, met = torch.zeros(2 * B * C * 6, dtype=torch.float64, device="cuda"), torch.zeros(5, dtype=torch.float64, device="cuda")

    def head(vm):
        lib.call("rua_head_fwd_loss_void", x.data_ptr(), w.data_ptr(), b.data_ptr(), z.data_ptr(), p.data_ptr(), y.data_ptr(), sums.data_ptr(), 1, met.data_ptr(),
                 B, HW, Cin, C, L.ACT_SOFTMAX, L.RUA_BF16, vm, st())
    res["head_fwd_us"] = {"shape": [B, S, S, Cin], "classes": C, "unmasked": [], "masked": []}
    for _ in range(args.rounds):
        res["head_fwd_us"]["unmasked"].append(events(lambda: head(None), args.reps))
        res["head_fwd_us"]["masked"].append(events(lambda: head(mask_d.data_ptr()), args.reps))

    def model(ignore_void, cls):
        m = Model(ModelConfig(input_shape=(S, S, 3), num_classes=C, multitasking=True), dtype="bf16", seed=0)
        loss = Tanimoto_dual_loss()
        m.compile(optimizer=Adam(lr=1e-3, beta_1=0.9), loss={h: loss for h in HEADS}, loss_weights={h: 1.0 for h in HEADS},
                  metrics={"seg": ["accuracy"]}, ignore_void=ignore_void)
        m.train_on_batch(img, cls, norm_type=1)                 # the batch (and its void mask) is resident from here on
        return m
    img = rng.integers(0, 256, (B, S, S, 3)).astype(np.uint8)
    cls0 = class_maps(rng, B, S, C, 0.0)
    # without the option a class value >= C is an all-zero label row: "off" trains on the class map without void bytes
    models = {"off": model(None, cls0), "on_0": model(2, cls0), "on_30": model(2, cls30)}

    def timed(m):
        for _ in range(args.warmup):
            m.engine.train_step(None, None)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            m.engine.train_step(None, None)
        torch.cuda.synchronize()
        return round((time.perf_counter() - t0) * 1e3 / args.steps, 3)
    steps = {k: [] for k in models}
    for _ in range(args.rounds):
        for k, m in models.items():
            steps[k].append(timed(m))
    res["step_ms"] = {"shape": [B, S, S, 3], "classes": C, "dtype": "bf16", "path": "graph", "warmup": args.warmup, "steps": args.steps, **steps,
                      "dispatches_per_step": {k: m.engine.count_step_dispatches(B) for k, m in models.items()}}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
