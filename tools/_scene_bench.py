"""What the tools/bench_scene*.py share: the seeded scene and class maps of the cfg3 set-up (256 x 256 x 3 patches, 6 classes,
batch 8) and the three timing loops.  Each tool keeps its own command line and its own JSON."""
import time

import numpy as np

B, P, CIN, CLASSES = 8, 256, 3, 6


def make_scene(size, seed=0):
    """(uint8 image size x size x CIN of noise, uint8 class map of 16 x 16 blocks)."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (size, size, CIN), dtype=np.uint8)
    f = rng.integers(0, CLASSES, (size // 16 + 1, size // 16 + 1), dtype=np.uint8)
    return img, np.ascontiguousarray(np.kron(f, np.ones((16, 16), np.uint8))[:size, :size])


def make_maps(size, seed=0):
    """Three class maps: 16 x 16 blocks, per-pixel noise, one class everywhere."""
    rng = np.random.default_rng(seed)
    f = rng.integers(0, CLASSES, (size // 16 + 1, size // 16 + 1), dtype=np.uint8)
    blocky = np.ascontiguousarray(np.kron(f, np.ones((16, 16), np.uint8))[:size, :size])
    noise = rng.integers(0, CLASSES, (size, size), dtype=np.uint8)
    return {"blocky": blocky, "noise": noise, "uniform": np.full((size, size), 2, np.uint8)}


def cfg3_model():
    from resunet_a_mltsk_keras_amd.engine import ModelConfig
    from resunet_a_mltsk_keras_amd.keras_api import Model
    return Model(ModelConfig(input_shape=(P, P, CIN), num_classes=CLASSES, multitasking=True), dtype="bf16", seed=0)


def events_ms(fn, reps):
    """ms per call: device events around `reps` back-to-back calls."""
    import torch
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def call_us(fn, reps, warmup=5):
    """A kernel figure: us per call over `reps` calls after `warmup` untimed ones."""
    for _ in range(warmup):
        fn()
    return events_ms(fn, reps) * 1e3


def rounds_ms(fn, rounds, reps, warmup=2):
    """A kernel figure by rounds: [ms per call] of `rounds` rounds of `reps` calls after `warmup` untimed ones."""
    for _ in range(warmup):
        fn()
    return [events_ms(fn, reps) for _ in range(rounds)]


def median_row(per_call):
    return {"ms_per_call": [round(v, 4) for v in per_call], "ms": round(float(np.median(per_call)), 4),
            "spread_ms": round(max(per_call) - min(per_call), 4)}


def clock_ms(fn, warmup, reps, takes_index=False):
    """Work that ends in a device synchronise, by the host clock: (ms per call of `reps` calls after `warmup` untimed ones, what
    the last call returned).  takes_index: fn(k) with the call's index (training steps) instead of fn()."""
    import torch
    last = None
    for k in range(warmup):
        fn(k) if takes_index else fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(reps):
        last = fn(k) if takes_index else fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps, last
