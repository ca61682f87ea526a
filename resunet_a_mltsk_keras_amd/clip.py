"""Host definitions of gradient clipping, decoupled weight decay and the non-finite step skip (include/rua_hip.h: rua_grad_sumsq,
rua_clip_finish, rua_adam_step_seg / rua_sgd_step_seg, rua_state_copy).

Two things live here, both pure numpy:
  * build_chunk_table: the (off, len, var) chunk table and the per-variable (chunk range, decay flag) table the kernels walk.  The product
    path (Engine.compile) uses this and nothing else of the module.
  * host_clipped_step: ONE optimizer step under these options, restated in float64.  Tests and tools compare the kernels with it.

Semantics (Keras' definitions; gs is the optimizer's grad_scale, 1 / world under data parallel):
  global_clipnorm=c   norm = gs * sqrt(sum of g^2 over all trainable elements); every gradient times coef = c / max(norm, c); norm 0: coef 1
  clipnorm=c          the same per VARIABLE - one Keras name: the cin segments ParamStore.conv splits a kernel into share one norm
  clipvalue=c         g * gs limited to [-c, c] by comparisons, so that a NaN stays a NaN
  weight_decay=wd     decoupled (Keras >= 2.11): theta -= theta * (wd * lr_base) before the gradient update, lr_base the BASE rate (not the
                      bias-corrected one); variables whose name contains one of the exclusion substrings do not decay
  skip_nonfinite      this project's own: if the sum of g^2 over all trainable elements is not finite the step leaves theta and the moments
                      alone (no decay either); the gradient is still zeroed, and the step counter still advances - a skipped step costs one t
                      of Adam's bias correction
Element order (Adam):  th1 = th - th * d, d = float32(wd * lr_base), for a decaying variable;  gg = clampv((g * gs) * coef[var]);  then the
plain Adam arithmetic on th1 and gg.  SGD: vel = mu * vel - lr * gg, th = th1 + vel."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

OPT_CHUNK = 8192                                            # RUA_OPT_CHUNK of include/rua_hip.h (tests/test_clip_host.py compares the two)
CLIP_NONE, CLIP_GLOBAL_NORM, CLIP_NORM, CLIP_VALUE = 0, 1, 2, 3

CHUNK_DTYPE = np.dtype([("off", "<i8"), ("len", "<i4"), ("var", "<i4")])                                # rua_opt_chunk
VAR_DTYPE = np.dtype([("chunk_begin", "<i4"), ("chunk_end", "<i4"), ("decay", "<i4"), ("pad", "<i4")])   # rua_opt_var
DEFAULT_DECAY_EXCLUDE = ("bias", "gamma", "beta")           # what train_ISPRS.py excludes unless --decay_all yes


def check_options(clipnorm=None, global_clipnorm=None, clipvalue=None, weight_decay=None) -> None:
    """Keras' rules: at most one clip option, each a positive number; the decay a non-negative one.  ValueError otherwise."""
    given = [(k, v) for k, v in (("clipnorm", clipnorm), ("global_clipnorm", global_clipnorm), ("clipvalue", clipvalue)) if v is not None]
    if len(given) > 1:
        raise ValueError(f"only one of clipnorm, global_clipnorm and clipvalue can be set (got {', '.join(k for k, _ in given)})")
    for k, v in given:
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or v <= 0:
            raise ValueError(f"{k}={v!r}: a positive number")
    if weight_decay is not None:
        v = weight_decay
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or v < 0:
            raise ValueError(f"weight_decay={v!r}: a non-negative number")


def clip_mode(clipnorm=None, global_clipnorm=None, clipvalue=None) -> Tuple[int, float]:
    """(mode of rua_clip_finish, c) of a checked option set."""
    check_options(clipnorm, global_clipnorm, clipvalue)
    if global_clipnorm is not None:
        return CLIP_GLOBAL_NORM, float(global_clipnorm)
    if clipnorm is not None:
        return CLIP_NORM, float(clipnorm)
    if clipvalue is not None:
        return CLIP_VALUE, float(clipvalue)
    return CLIP_NONE, 0.0


def build_chunk_table(entries: Sequence[dict], decay_exclude: Sequence[str] = (), chunk: int = OPT_CHUNK):
    """(chunks, vars, names) of a ParamStore's trainable entries (dicts with name, off, size, in buffer order).
    chunks: CHUNK_DTYPE rows - every entry cut into pieces of at most `chunk` elements; off a multiple of 16 (the entry's own off is, and
            chunk is a multiple of 16); no chunk spans entries, padding belongs to none.
    vars:   VAR_DTYPE rows - a variable is one name: its entries are adjacent (the segments of a split kernel) and so are its chunks,
            [chunk_begin, chunk_end); decay = 0 where the name contains one of the decay_exclude substrings, else 1.
    names:  the variables' names in order."""
    if chunk <= 0 or chunk % 16:
        raise ValueError(f"chunk {chunk}: a positive multiple of 16")
    if isinstance(decay_exclude, str):
        decay_exclude = (decay_exclude,)
    rows: List[Tuple[int, int, int]] = []
    vrows: List[List[int]] = []
    names: List[str] = []
    end = 0
    for e in entries:
        name, off, size = e["name"], int(e["off"]), int(e["size"])
        if off % 16 or off < end or size <= 0:
            raise ValueError(f"{name}: entry at {off} (+{size}) is misaligned, empty or overlaps the one before")
        end = off + size
        if not names or names[-1] != name:
            if name in names:
                raise ValueError(f"{name}: the entries of one variable must be adjacent")
            names.append(name)
            vrows.append([len(rows), len(rows), 0 if any(s in name for s in decay_exclude) else 1, 0])
        for a in range(0, size, chunk):
            rows.append((off + a, min(chunk, size - a), len(names) - 1))
        vrows[-1][1] = len(rows)
    chunks = np.array(rows, dtype=CHUNK_DTYPE) if rows else np.zeros(0, CHUNK_DTYPE)
    vars_ = np.array([tuple(v) for v in vrows], dtype=VAR_DTYPE) if vrows else np.zeros(0, VAR_DTYPE)
    return chunks, vars_, names


def covered(chunks: np.ndarray, n: int) -> np.ndarray:
    """How many chunks cover each of the n elements of the flat buffer (1 inside an entry, 0 on padding - anything else is a broken table)."""
    c = np.zeros(n, np.int32)
    for off, ln, _ in chunks.tolist():
        c[off:off + ln] += 1
    return c


def host_sumsq(g: np.ndarray, chunks: np.ndarray, vars_: np.ndarray) -> Tuple[np.ndarray, float]:
    """(per-variable, total) sums of g^2 in float64 over the chunk table."""
    g = np.asarray(g, np.float64)
    per = np.zeros(len(vars_), np.float64)
    for off, ln, v in chunks.tolist():
        x = g[off:off + ln]
        per[v] += float(np.dot(x, x))
    return per, float(per.sum())


def host_coef(per: np.ndarray, total: float, mode: int, c: float, grad_scale: float = 1.0) -> np.ndarray:
    """The finisher's float32 coefficient per variable, from float64 sums."""
    with np.errstate(invalid="ignore", over="ignore"):
        if mode == CLIP_GLOBAL_NORM:
            norm = grad_scale * np.sqrt(total)
            return np.full(len(per), np.float32(c / np.fmax(norm, c)), np.float32)
        if mode == CLIP_NORM:
            return (c / np.fmax(grad_scale * np.sqrt(per), c)).astype(np.float32)
    return np.ones(len(per), np.float32)


def host_clipped_step(theta, g, m, v, chunks, vars_, *, optimizer: str = "adam", lr: float, lr_base: Optional[float] = None,
                      beta_1: float = 0.9, beta_2: float = 0.999, eps: float = 1e-7, momentum: float = 0.0, grad_scale: float = 1.0,
                      clipnorm=None, global_clipnorm=None, clipvalue=None, weight_decay: float = 0.0, skip_nonfinite: bool = False) -> Dict[str, object]:
    """One optimizer step over the chunk table in float64.  theta, g, m, v: flat arrays (v ignored for "sgd", where m is the velocity).
    lr: the rate the update uses (Adam: the bias-corrected lr_t the rate kernel hands over); lr_base: the base rate the decay uses
    (default lr).  Scalars are used as given: a caller that compares with a kernel passes them float32-rounded, as the kernel receives them.
    The coefficient and d = wd * lr_base ARE rounded to float32 here, as the finisher and the optimizer round theirs.
    Returns dict(theta, m, v, g - all flat float64, padding untouched, g zeroed inside the chunks -, th1, gg (the decayed theta and the
    clipped gradient the update used), coef (float32 per variable), sumsq (per variable), norm (global), skipped)."""
    mode, c = clip_mode(clipnorm, global_clipnorm, clipvalue)
    check_options(weight_decay=weight_decay)
    th, gr, m1 = (np.array(a, np.float64) for a in (theta, g, m))
    v1 = np.array(v, np.float64) if optimizer == "adam" else None
    per, total = host_sumsq(gr, chunks, vars_)
    coef = host_coef(per, total, mode, c, grad_scale)
    with np.errstate(invalid="ignore", over="ignore"):
        norm = float(grad_scale * np.sqrt(total))
    skipped = bool(skip_nonfinite and not np.isfinite(total))
    d = float(np.float32(float(weight_decay) * float(lr if lr_base is None else lr_base)))
    th1_all, gg_all = th.copy(), np.zeros_like(gr)
    for off, ln, var in chunks.tolist():
        sl = slice(off, off + ln)
        if not skipped:
            t = th[sl]
            if weight_decay and vars_["decay"][var]:
                t = t - t * d
            th1_all[sl] = t
            with np.errstate(invalid="ignore", over="ignore"):
                gg = (gr[sl] * float(grad_scale)) * float(coef[var])
                if mode == CLIP_VALUE:
                    gg = np.where(gg < -c, -c, np.where(gg > c, c, gg))
                gg_all[sl] = gg
                if optimizer == "adam":
                    m1[sl] = beta_1 * m1[sl] + (1 - beta_1) * gg
                    v1[sl] = beta_2 * v1[sl] + (1 - beta_2) * gg * gg
                    th[sl] = t - lr * m1[sl] / (np.sqrt(v1[sl]) + eps)
                else:
                    m1[sl] = momentum * m1[sl] - lr * gg
                    th[sl] = t + m1[sl]
        gr[sl] = 0.0
    return dict(theta=th, m=m1, v=v1, g=gr, th1=th1_all, gg=gg_all, coef=coef, sumsq=per, norm=norm, skipped=skipped)
