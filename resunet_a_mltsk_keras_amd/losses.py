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
    """The four per-head dicts out of a checkpoint's `loss` metadata; a file written before the options existed has none: empty dicts.  A file
    whose model mined hard examples carries a fifth, `ohem` (head -> ohem_options' dict); it is handed on only where the file has it."""
    out = {k: dict(lo.get(k) or {}) for k in OPTION_KEYS}
    if lo.get(OHEM_KEY):
        out[OHEM_KEY] = {h: ohem_options(**dict(o)) for h, o in lo[OHEM_KEY].items()}
    if lo.get(LOVASZ_KEY):                                # ... a sixth where a head is on the Lovasz loss
        out[LOVASZ_KEY] = {h: lovasz_options(**dict(o)) for h, o in lo[LOVASZ_KEY].items()}
    return out


# ---- online hard example mining (OHEM, bootstrapped cross-entropy) ----------------------------------------------------------------------------
# Per step and per head only the hardest pixels contribute: those whose loss lies above a threshold, but never fewer than a floor.  host_ohem is
# the definition; rua_ohem_select (csrc/ohem.hip) computes the same selection on the device bit for bit, and the head's gradient takes the mask and
# the normaliser from device memory (rua_head_dz_sel / rua_head_dz_multi_sel).  All parameters are integers or one float32, so that host and
# device agree exactly:
#   min_kept   int >= 0               the floor
#   keep_q16   int in 1..65536        the kept share of the valid pixels in Q16 (ohem_q16 turns a ratio into it)
#   thresh     a float32 or None      a loss value: every valid pixel at or above it is kept as well
#   warmup     int >= 0               optimizer updates over which the share falls linearly from 1 to keep_q16
# With thresh = -log(0.7), keep_q16 = 1 and min_kept = 100000 this is mmsegmentation's OHEMPixelSampler for plain cross-entropy; with no thresh and
# keep_q16 = 0.25 * 65536 it is bootstrapped cross-entropy at 25 %.
OHEM_KEY = "ohem"                                        # LossSpec's fifth per-head dict and the checkpoint's key
OHEM_FIELDS = ("keep_q16", "min_kept", "thresh", "prob_thresh", "warmup")
NO_KEY = 0xFFFFFFFF                                      # the key of a NaN, and tau_key's stand-in for "no valid pixel"


def ohem_key(values) -> np.ndarray:
    """The order-preserving uint32 key of float32 values: all bits of a negative flipped, the sign bit of a non-negative set (so -0 < +0);
    every NaN maps to 0xFFFFFFFF, the hardest key."""
    b = np.ascontiguousarray(values, np.float32).view(np.uint32)
    k = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    return np.where((b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000), np.uint32(NO_KEY), k).astype(np.uint32)


def ohem_unkey(key: int) -> np.float32:
    """The float32 a key stands for (0xFFFFFFFF: a NaN)."""
    k = int(key) & 0xFFFFFFFF
    b = (k ^ 0x80000000) if k & 0x80000000 else (~k & 0xFFFFFFFF)
    return np.array([b], np.uint32).view(np.float32)[0]


def ohem_q16(keep_ratio: float) -> int:
    """A kept share in (0, 1] as the Q16 integer the selection works with (rounded to nearest, at least 1)."""
    r = float(keep_ratio)
    if not 0.0 < r <= 1.0:
        raise ValueError(f"keep_ratio {keep_ratio!r} must be in (0, 1]")
    return min(65536, max(1, int(round(r * 65536.0))))


def ohem_share(keep_q16: int, warmup: int, t: int) -> int:
    """q(t): the share in Q16 after t optimizer updates - 65536 - ((65536 - keep_q16) * min(t, warmup)) // warmup, keep_q16 with no warm-up."""
    if int(warmup) <= 0:
        return int(keep_q16)
    return 65536 - ((65536 - int(keep_q16)) * min(max(int(t), 0), int(warmup))) // int(warmup)


def ohem_count(n_valid: int, q16: int, min_kept: int) -> int:
    """K = min(n_valid, max(min_kept, (n_valid * q + 65535) >> 16))."""
    return min(int(n_valid), max(int(min_kept), (int(n_valid) * int(q16) + 65535) >> 16))


def prob_to_thresh(prob_thresh: float) -> float:
    """mmsegmentation's probability threshold as a loss value of plain cross-entropy: float32(-log p)."""
    p = float(prob_thresh)
    if not 0.0 < p <= 1.0:
        raise ValueError(f"prob_thresh {prob_thresh!r} must be in (0, 1]")
    return float(np.float32(-np.log(p)))


def ohem_options(keep_q16: int = 16384, min_kept: int = 0, thresh: Optional[float] = None, prob_thresh: Optional[float] = None, warmup: int = 0) -> dict:
    """One head's options as the plain dict LossSpec.ohem and the checkpoint hold; prob_thresh = p stands for thresh = float32(-log p)."""
    if prob_thresh is not None:
        if thresh is not None and float(np.float32(thresh)) != prob_to_thresh(prob_thresh):
            raise ValueError("loss_thresh and prob_thresh: one of them")
        thresh = prob_to_thresh(prob_thresh)
    return dict(keep_q16=keep_q16, min_kept=min_kept, thresh=None if thresh is None else float(np.float32(thresh)),
                prob_thresh=None if prob_thresh is None else float(prob_thresh), warmup=warmup)


def check_ohem(o: dict, what: str = "ohem"):
    """The range of one head's options; raises ValueError."""
    unknown = [k for k in o if k not in OHEM_FIELDS]
    if unknown:
        raise ValueError(f"{what}: unknown option(s) {unknown}")
    isint = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, bool)
    q, mk, wu, th = o.get("keep_q16", 16384), o.get("min_kept", 0), o.get("warmup", 0), o.get("thresh")
    if not isint(q) or not 1 <= q <= 65536:
        raise ValueError(f"{what}: keep_q16 {q!r} must be an integer in 1..65536")
    if not isint(mk) or not 0 <= mk < 2 ** 62:
        raise ValueError(f"{what}: min_kept {mk!r} must be an integer >= 0")
    if not isint(wu) or not 0 <= wu < 2 ** 31:
        raise ValueError(f"{what}: warmup {wu!r} must be an integer >= 0")
    if th is not None and np.isnan(np.float32(th)):
        raise ValueError(f"{what}: thresh is NaN")
    if o.get("prob_thresh") is not None:
        if th is None or float(np.float32(th)) != prob_to_thresh(o["prob_thresh"]):
            raise ValueError(f"{what}: prob_thresh {o['prob_thresh']!r} and thresh {th!r} disagree")


def to_ohem_struct(o: dict) -> "L.OhemOpts":
    """rua_ohem_opts of one head."""
    s = L.OhemOpts()
    th = o.get("thresh")
    s.min_kept, s.keep_q16, s.warmup = int(o.get("min_kept", 0)), int(o.get("keep_q16", 16384)), int(o.get("warmup", 0))
    s.thresh, s.has_thresh = (float(np.float32(th)), 1) if th is not None else (0.0, 0)
    return s


def host_ohem(per_pixel, valid=None, keep_q16: int = 16384, min_kept: int = 0, thresh: Optional[float] = None, warmup: int = 0, t: int = 0,
              loss_weight: float = 1.0) -> dict:
    """The selection over one head's float32 per-pixel loss map L (any shape, as rua_pixel_loss* writes per_pixel) and valid (None: every pixel;
    else non-zero = valid, the void mask's "byte == 0"):

      n_valid = sum(valid);  q = ohem_share(keep_q16, warmup, t);  K = ohem_count(n_valid, q, min_kept)
      tau_key = the K-th largest valid key (0xFFFFFFFF with no valid pixel), with thresh: min(tau_key, key(thresh))
      kept    = valid and key(L) >= tau_key - ties at the threshold are all kept, so n_kept >= K and no order enters
      loss    = (fp64 sum of L over the kept pixels) / n_kept, 0 for n_kept = 0;  scale = float32(float64(loss_weight) / n_kept), or 0

    Returns dict(drop_mask uint8 of L's shape (0 kept, 1 dropped or void), tau_key, tau (float32), n_valid, n_kept, K, q16_used, kept_sum,
    loss, scale (float32))."""
    Lm = np.ascontiguousarray(per_pixel, np.float32)
    key = ohem_key(Lm).reshape(-1)
    v = np.ones(key.shape, bool) if valid is None else (np.asarray(valid).reshape(-1) != 0)
    n_valid = int(v.sum())
    q = ohem_share(keep_q16, warmup, t)
    K = ohem_count(n_valid, q, min_kept)
    tau_key = NO_KEY
    if K > 0:
        vk = key[v]
        tau_key = int(np.partition(vk, n_valid - K)[n_valid - K])          # the K-th largest = the (n_valid - K)-th smallest, 0-based
    if thresh is not None:
        th = np.float32(thresh)
        if np.isnan(th):
            raise ValueError("thresh is NaN")
        tau_key = min(tau_key, int(ohem_key(th).reshape(-1)[0]))
    kept = v & (key >= np.uint32(tau_key))
    n_kept = int(kept.sum())
    kept_sum = float(np.sum(Lm.reshape(-1)[kept].astype(np.float64))) if n_kept else 0.0
    return dict(drop_mask=(~kept).astype(np.uint8).reshape(Lm.shape), tau_key=tau_key, tau=ohem_unkey(tau_key), n_valid=n_valid, n_kept=n_kept, K=K,
                q16_used=q, kept_sum=kept_sum, loss=kept_sum / n_kept if n_kept else 0.0,
                scale=np.float32(np.float64(np.float32(loss_weight)) / np.float64(n_kept)) if n_kept else np.float32(0.0))     # (the C ABI takes loss_weight as a float32)


# ---- Lovasz-Softmax (Berman, Triki, Blaschko, CVPR 2018: lovasz_softmax) -----------------------------------------------------------------------
# The Lovasz extension of the Jaccard index: per class the valid pixels are ordered by their error and the error vector is weighted with the
# discrete gradient of the Jaccard loss along that order.  host_lovasz is the definition of the value and of d(loss)/d(probabilities),
# host_lovasz_dz of the step from there to the logits; rua_lovasz_grad / rua_lovasz_dz (csrc/lovasz.hip) compute the same bits on the device - the
# order, the weights and the gradient exactly, the fp64 sums up to their order.  One option:
#   classes    "present" (the paper's default): the classes with at least one foreground pixel among the valid ones count;  "all": every class
# Out of scope: per_image=True, the hinge form on logits, a built-in mix with cross-entropy on one head, sorting as a public utility.
LOVASZ_KEY = "lovasz"                                    # LossSpec's sixth per-head dict and the checkpoint's key
LOVASZ_FIELDS = ("classes",)
LOVASZ_CLASSES = ("present", "all")
LOVASZ_MAX_CLASSES = L.RUA_LOVASZ_MAX_C
LOVASZ_HEADS = {"seg": L.ACT_SOFTMAX, "bound": L.ACT_SIGMOID}          # the heads with binary targets; dist and color have continuous ones


def lovasz_options(classes: str = "present") -> dict:
    """One head's options as the plain dict LossSpec.lovasz and the checkpoint hold."""
    return dict(classes=classes)


def check_lovasz(o: dict, what: str = "lovasz", head: Optional[str] = None, num_classes: Optional[int] = None):
    """The range of one head's options, and (when given) the head and its channel count; raises ValueError."""
    if not isinstance(o, dict):
        raise ValueError(f"{what}: lovasz options are a dict (losses.lovasz_options), got {type(o).__name__}")
    unknown = [k for k in o if k not in LOVASZ_FIELDS]
    if unknown:
        raise ValueError(f"{what}: unknown option(s) {unknown}")
    if o.get("classes", "present") not in LOVASZ_CLASSES:
        raise ValueError(f"{what}: classes {o.get('classes')!r} must be one of {LOVASZ_CLASSES}")
    if head is not None and head not in LOVASZ_HEADS:
        raise ValueError(f"{what}: the Lovasz loss needs binary targets: heads {', '.join(LOVASZ_HEADS)} only, '{head}' has continuous ones")
    if num_classes is not None and not 1 <= int(num_classes) <= LOVASZ_MAX_CLASSES:
        raise ValueError(f"{what}: {num_classes} classes, the Lovasz kernels take 1..{LOVASZ_MAX_CLASSES}")


def lovasz_result(buf: bytes) -> dict:
    """rua_lovasz_result (the bytes read back from the device) as a dict: n_valid, n_cls, scale (float32), G and loss_c (16 entries), loss."""
    r = L.LovaszResult.from_buffer_copy(buf)
    return dict(n_valid=int(r.n_valid), n_cls=int(r.n_cls), scale=np.float32(r.scale), G=[int(v) for v in r.G], loss_c=[float(v) for v in r.loss_c],
                loss=float(r.loss))


def host_lovasz(y_pred, y_true, void=None, classes: str = "present", loss_weight: float = 1.0) -> dict:
    """The Lovasz-Softmax loss of probabilities p [..., C] (float32) against targets y [..., C], void [...] (non-zero = void) or None.  Per class c,
    over the n valid pixels in flat index order:

      fg = y > 0.5;  e = |float32(fg) - p| (one float32 subtraction);  G = sum fg
      order   = the valid pixels by ohem_key(e) DESCENDING (NaN first), ties in ascending pixel index
      F_r     = number of foreground pixels among the ranks 0..r;  J_r = 1 - (G - F_r) / (G + (r + 1) - F_r) in float64, J_-1 = 0
      w_r     = J_r - J_{r-1};  loss_c = sum_r float64(e_(r)) w_r
      dp      = float32(w_r) at a background pixel, -float32(w_r) at a foreground one; +0 at void pixels and in classes that are not counted

    counted = G > 0 ("present") or every class ("all"); loss = sum_counted loss_c / n_cls; scale = float32(float64(float32(loss_weight)) / n_cls);
    n = 0 or n_cls = 0: loss 0, scale 0, dp zero.  Returns dict(loss, loss_c [C] (0 where not counted), G [C], n_valid, n_cls, scale, dp (p's
    shape, float32), order (list of C arrays of n pixel indices), w (list of C float64 arrays, by rank))."""
    if classes not in LOVASZ_CLASSES:
        raise ValueError(f"classes {classes!r} must be one of {LOVASZ_CLASSES}")
    p = np.ascontiguousarray(y_pred, np.float32)
    Cc = p.shape[-1]
    p2 = p.reshape(-1, Cc)
    y2 = np.asarray(y_true).reshape(-1, Cc)
    M = p2.shape[0]
    valid = np.ones(M, bool) if void is None else (np.asarray(void).reshape(-1) == 0)
    idx = np.flatnonzero(valid)
    n = int(idx.size)
    dp = np.zeros((M, Cc), np.float32)
    G = [int((y2[idx, c] > 0.5).sum()) for c in range(Cc)]
    counted = [n > 0 and (classes == "all" or G[c] > 0) for c in range(Cc)]
    n_cls = int(sum(counted))
    loss_c, order, ws = [0.0] * Cc, [], []
    for c in range(Cc):
        fg = y2[idx, c] > 0.5
        e = np.abs(fg.astype(np.float32) - p2[idx, c]).astype(np.float32)
        key = ohem_key(e).astype(np.int64)
        perm = np.argsort(-key, kind="stable")             # descending key; stable: ties keep the ascending pixel index
        order.append(idx[perm].astype(np.int64))
        fgs = fg[perm].astype(np.int64)
        F = np.cumsum(fgs)
        r1 = np.arange(1, n + 1, dtype=np.int64)
        J = 1.0 - (G[c] - F).astype(np.float64) / (G[c] + r1 - F).astype(np.float64)
        w = J - np.concatenate([[0.0], J[:-1]])
        ws.append(w)
        if counted[c]:
            loss_c[c] = float(np.sum(e[perm].astype(np.float64) * w))
            wf = w.astype(np.float32)
            dp[idx[perm], c] = np.where(fgs == 1, -wf, wf)
    loss = float(sum(loss_c[c] for c in range(Cc) if counted[c]) / n_cls) if n_cls else 0.0
    scale = np.float32(np.float64(np.float32(loss_weight)) / np.float64(n_cls)) if n_cls else np.float32(0.0)
    return dict(loss=loss, loss_c=loss_c, G=G, n_valid=n, n_cls=n_cls, scale=scale, dp=dp.reshape(p.shape), order=order, w=ws)


def host_lovasz_dz(act: int, y_pred, dp, scale) -> np.ndarray:
    """d(total)/d(logits) from host_lovasz's dp, in float32 with every operation rounded on its own, in this order:

      softmax   s = (((g_0 p_0) + g_1 p_1) + ..) over c = 0..C-1;  dz_k = scale (p_k (g_k - s))
      sigmoid   dz_c = scale (g_c (p_c (1 - p_c)))

    A softmax pixel whose dp is zero in every class and a sigmoid element whose dp is zero - every void pixel - are +0.0f by a select, whatever p
    holds there (the formula gives the same zero for finite p and scale >= 0)."""
    p = np.ascontiguousarray(y_pred, np.float32)
    g = np.ascontiguousarray(dp, np.float32)
    sc = np.float32(scale)
    Cc = p.shape[-1]
    with np.errstate(invalid="ignore", over="ignore"):
        if act == L.ACT_SOFTMAX:
            s = (g[..., 0] * p[..., 0]).astype(np.float32)
            for c in range(1, Cc):
                s = (s + (g[..., c] * p[..., c]).astype(np.float32)).astype(np.float32)
            dz = (sc * (p * (g - s[..., None]).astype(np.float32)).astype(np.float32)).astype(np.float32)
            return np.where((g != 0).any(-1, keepdims=True), dz, np.float32(0.0)).astype(np.float32)
        if act == L.ACT_SIGMOID:
            dz = (sc * (g * (p * (np.float32(1.0) - p).astype(np.float32)).astype(np.float32)).astype(np.float32)).astype(np.float32)
            return np.where(g != 0, dz, np.float32(0.0)).astype(np.float32)
    raise ValueError("host_lovasz_dz: act is softmax or sigmoid")


def scalar_or_vector(alpha, num_classes: int) -> Sequence[float]:
    """Keras' scalar alpha as the per-class vector; a sequence stays (its length is check_options' business)."""
    a = np.asarray(alpha, np.float64).reshape(-1)
    return [float(a[0])] * num_classes if a.size == 1 else [float(v) for v in a]
