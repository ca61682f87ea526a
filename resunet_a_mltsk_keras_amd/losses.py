"""Focal losses and label smoothing: the definitions.

Keras 3's CategoricalFocalCrossentropy, BinaryFocalCrossentropy and the `label_smoothing=` of its cross-entropies, written out as fp64 numpy
functions on channels-last arrays.  These functions are the specification; the kernels behind rua_pixel_loss_opts / rua_head_dz_opts /
rua_head_dz_multi_opts (csrc/loss_optim.hip) follow them in fp32, and the gradient passes a clip strictly inside it only.

With C classes, e = label_smoothing, g = gamma and the clip bounds KERAS_EPS, 1 - KERAS_EPS:

  smoothing           t = y (1 - e) + e / C under a softmax, t = y (1 - e) + e / 2 per sigmoid channel.  Weighted CE, CE on logits and BCE
                      on logits keep their formula with t in place of y; Tanimoto and MSE take none.
  categorical focal   u_c = clip(p_c / sum_k p_k);  L = - sum_c a_c t_c (1 - u_c)^g log u_c.  a is a per-class vector (Keras' scalar alpha
                      is that scalar in every class); the device takes it through class_w.
  binary focal        per channel: o = clip(p), bce = -(t log o + (1 - t) log(1 - o)), p_t = t p + (1 - t)(1 - p) on the unclipped p,
                      l_c = w_c (1 - p_t)^g bce with w_c = t alpha + (1 - t)(1 - alpha) under apply_class_balancing, else 1;  L = mean_c l_c.

Range (check_options): g = 0 or 1 <= g <= 8; 0 <= e < 1; a_c >= 0; 0 <= alpha <= 1; C <= 8.  0 < g < 1 is refused because the binary form's
derivative at p_t = 1 is not finite, and both kinds share the rule.  g = 0 is factor 1 exactly, by a branch (no pow(0, 0)).
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np

from . import _lib as L

KERAS_EPS = 1e-7
MAX_CLASSES = 8
SOFTMAX_KINDS = (L.LOSS_WCE, L.LOSS_CE_LOGITS, L.LOSS_FOCAL_CE)           # smoothing spreads e over the C classes
SIGMOID_KINDS = (L.LOSS_BCE_LOGITS, L.LOSS_FOCAL_BCE)                     # ... over the two outcomes of a channel
FOCAL_KINDS = (L.LOSS_FOCAL_CE, L.LOSS_FOCAL_BCE)
OPTION_KEYS = ("focal_gamma", "focal_alpha", "class_balance", "label_smoothing")      # LossSpec's per-head dicts, the checkpoint's keys


def host_smooth(y, label_smoothing: float, binary: bool = False):
    """The smoothed targets: y (1 - e) + e / C over the last axis, or y (1 - e) + e / 2 per channel with binary=True."""
    y = np.asarray(y, np.float64)
    e = float(label_smoothing)
    return y * (1.0 - e) + e / (2.0 if binary else y.shape[-1])


def _factor(q, gamma: float):
    return np.ones_like(q) if gamma == 0 else q ** float(gamma)


def host_categorical_focal(y_true, y_pred, alpha, gamma: float = 2.0, label_smoothing: float = 0.0):
    """The per-pixel map [...] of categorical focal cross-entropy on probabilities [..., C]; alpha: a scalar or C values."""
    y, p = np.asarray(y_true, np.float64), np.asarray(y_pred, np.float64)
    a = np.broadcast_to(np.asarray(alpha, np.float64), (p.shape[-1],))
    t = host_smooth(y, label_smoothing)
    u = np.clip(p / p.sum(-1, keepdims=True), KERAS_EPS, 1.0 - KERAS_EPS)
    return -(a * t * _factor(1.0 - u, gamma) * np.log(u)).sum(-1)


def host_binary_focal(y_true, y_pred, gamma: float = 2.0, alpha: float = 0.25, apply_class_balancing: bool = False, label_smoothing: float = 0.0):
    """The per-pixel map [...] of binary focal cross-entropy on sigmoid probabilities [..., C]: the mean over the channels."""
    y, p = np.asarray(y_true, np.float64), np.asarray(y_pred, np.float64)
    t = host_smooth(y, label_smoothing, binary=True)
    o = np.clip(p, KERAS_EPS, 1.0 - KERAS_EPS)
    bce = -(t * np.log(o) + (1.0 - t) * np.log(1.0 - o))
    p_t = t * p + (1.0 - t) * (1.0 - p)
    l = _factor(np.maximum(1.0 - p_t, 0.0), gamma) * bce      # (p_t <= 1 up to rounding; the device holds 1 - p_t at >= 0 too)
    if apply_class_balancing:
        l = (t * float(alpha) + (1.0 - t) * (1.0 - float(alpha))) * l
    return l.mean(-1)


def check_options(kind: int, num_classes: int, gamma: float = 0.0, alpha=None, class_balance: bool = False, label_smoothing: float = 0.0,
                  what: str = "loss"):
    """The range above for one head of loss kind `kind` with `num_classes` channels; raises ValueError.  alpha: the per-class vector of focal
    CE (None: not looked at), the scalar of binary focal."""
    e = float(label_smoothing)
    if not 0.0 <= e < 1.0:
        raise ValueError(f"{what}: label_smoothing {label_smoothing!r} must be in [0, 1)")
    if e != 0.0 and kind not in SOFTMAX_KINDS + SIGMOID_KINDS:
        raise ValueError(f"{what}: Tanimoto and MSE take no label smoothing")
    if kind not in FOCAL_KINDS:
        return
    g = float(gamma)
    if not (g == 0.0 or 1.0 <= g <= 8.0):
        raise ValueError(f"{what}: gamma {gamma!r} must be 0 or in [1, 8] (the derivative of (1 - p_t)^gamma at p_t = 1 is not finite for 0 < gamma < 1)")
    if num_classes > MAX_CLASSES:
        raise ValueError(f"{what}: {num_classes} classes, the focal kernels take at most {MAX_CLASSES}")
    if kind == L.LOSS_FOCAL_CE:
        if alpha is not None:
            a = np.asarray(alpha, np.float64).reshape(-1)
            if a.size != num_classes:
                raise ValueError(f"{what}: {a.size} alpha values for {num_classes} classes")
            if not (np.isfinite(a).all() and (a >= 0).all()):
                raise ValueError(f"{what}: the per-class alpha is finite and not negative")
    elif class_balance:
        if not 0.0 <= float(alpha) <= 1.0:
            raise ValueError(f"{what}: alpha {alpha!r} must be in [0, 1]")


def to_struct(gamma: float = 0.0, label_smoothing: float = 0.0, alpha: Optional[float] = None, class_balance: bool = False) -> "L.LossOpts":
    """rua_loss_opts of one head."""
    o = L.LossOpts()
    o.gamma, o.label_smoothing, o.alpha, o.class_balance = float(gamma), float(label_smoothing), float(alpha) if alpha is not None else 0.0, int(bool(class_balance))
    return o


def options_from_meta(lo: dict) -> Dict[str, dict]:
    """The four per-head dicts out of a checkpoint's `loss` metadata; a file written before the options existed has none: empty dicts."""
    return {k: dict(lo.get(k) or {}) for k in OPTION_KEYS}


def scalar_or_vector(alpha, num_classes: int) -> Sequence[float]:
    """Keras' scalar alpha as the per-class vector; a sequence stays (its length is check_options' business)."""
    a = np.asarray(alpha, np.float64).reshape(-1)
    return [float(a[0])] * num_classes if a.size == 1 else [float(v) for v in a]
