"""Gradient accumulation (Keras 3's `gradient_accumulation_steps`): the host definition of what rua_accum_gate and rua_accum_step compute on
the GPU (csrc/loss_optim.hip), and the option's validation.

With K steps the optimizer applies the MEAN of K consecutive gradients once every K calls of train_on_batch.  A call is a micro-step: K - 1
HOLD steps add their gradient to an accumulator and leave weights, moments, the step counter, the rate and the weights' moving average alone;
the K-th, the UPDATE step, turns the gradient into the mean and runs the optimizer as always - clipping, decoupled decay and the non-finite
test act on the mean, and `optimizer.iterations` (Adam's bias correction, the schedules, the average's first step and overwrite period)
counts updates, not batches.  This follows recent Keras 3; Keras itself was never run against it.

The arithmetic is fp32 with every operation rounded on its own, and the mean is a correctly rounded DIVISION by K, not a product with 1 / K
(the two differ in the last bit for most K).  numpy's float32 `+` and `/` are exactly that, which makes host_accumulate the definition the
kernel is compared with bit for bit."""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np


def check_steps(k) -> Optional[int]:
    """None (off) or an integer >= 2, as Keras checks it; bool, float, 0, 1 and negatives are a ValueError.  Returns None or the int."""
    if k is None:
        return None
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 2:
        raise ValueError(f"gradient_accumulation_steps {k!r}: None (off) or an integer >= 2")
    if k > 1 << 24:
        raise ValueError(f"gradient_accumulation_steps {k!r}: at most 2^24 (the divisor must be exact in fp32)")
    return int(k)


def is_hold(micro: int, k: int) -> bool:
    """Whether the call that finds `micro` gradients in the accumulator is a hold step (rua_accum_gate's decision)."""
    return micro + 1 < k


def host_accumulate(a: np.ndarray, g: np.ndarray, micro: int, k: int) -> Tuple[np.ndarray, Optional[np.ndarray], int]:
    """One micro-step on fp32 arrays: (a2, g_out, micro2).  micro = gradients of the current cycle already in a (0 .. k - 1).
    Hold (micro + 1 < k): a2 = fadd(a, g), g_out None, micro2 = micro + 1.  Update: g_out = fdiv(fadd(g, a), float32(k)), a2 = 0, micro2 = 0."""
    if check_steps(k) is None or not 0 <= micro < k:
        raise ValueError(f"micro {micro!r} outside 0 .. k - 1 for k = {k!r}")
    a = np.asarray(a, dtype=np.float32)
    g = np.asarray(g, dtype=np.float32)
    if a.shape != g.shape:
        raise ValueError(f"accumulator {a.shape} and gradient {g.shape} differ in shape")
    with np.errstate(invalid="ignore", over="ignore"):
        if is_hold(micro, k):
            return (a + g).astype(np.float32), None, micro + 1
        return np.zeros_like(a), ((g + a).astype(np.float32) / np.float32(k)).astype(np.float32), 0
