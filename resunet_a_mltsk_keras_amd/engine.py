"""Static-plan execution engine for the ResUnet-a training path on MI355X.

The network is a fixed graph on fixed shapes, so instead of tracing or autograd the engine
RECORDS, once per (batch, mode), the exact list of librua_hip.so launches for forward,
backward and the optimizer, with every buffer pre-allocated; a step replays that list on one
HIP stream (optionally as a captured HIP graph).  PyTorch is used for device memory, streams
and torch.distributed only.  Reference call sites replaced: ResUnet_a/model2.py:14-193
(graph), train_ISPRS.py:131,148,167,186 (train_on_batch / test_on_batch), :404-407 (optimizers).
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib as L
from . import accum as AC
from . import clip as CL
from . import lamb as LB
from . import losses as LS
from . import schedules as SC
from .wgrad_queue import WgradQueue, WSpec
from .scenes import (BLEND_MODES, MAP_HEADS, AffineSceneBatch, SceneBatch, blend_table, check_blend_budget, check_photo_table, check_radius,
                     check_scales, check_tolerance, check_views, instance_params, instance_scores, scale_table, sieve_params, sweep_params,
                     view_rows)

BN_EPS, BN_MOMENTUM, KERAS_EPS = 1e-3, 0.99, 1e-7
HEADS = ["seg", "bound", "dist", "color"]
SUMS_REPLICAS = 1          # copies of a head's Tanimoto moments the blocks of rua_head_fwd_loss_rep spread their atomics over (measured: 8 copies take ~1 us off
                           # a head's forward and put ~8 us on the one-block finalisation that folds them - one copy it is)


@dataclass
class ModelConfig:
    input_shape: Tuple[int, int, int] = (256, 256, 3)
    num_classes: int = 5
    multitasking: bool = False
    variant: str = "model2"
    width: int = 32
    depth: int = 6

    def levels(self):
        dil = [[1, 3, 15, 31], [1, 3, 15, 31], [1, 3, 15], [1, 3, 15], [1], [1], [1]]
        return [(self.width * (2 ** i), dil[i]) for i in range(self.depth)]


@dataclass
class LossSpec:
    """What model.compile(...) received (train_ISPRS.py:411-461)."""
    kind: Dict[str, int] = field(default_factory=dict)       # head -> L.LOSS_*
    weight: Dict[str, float] = field(default_factory=dict)   # head -> loss weight
    class_weights: Optional[List[float]] = None
    optimizer: str = "adam"
    lr: float = 1e-3
    beta_1: float = 0.9
    beta_2: float = 0.999
    momentum: float = 0.8
    epsilon: float = 1e-7                                    # "lamb" only (lamb.py holds the definition): Adam's kernels are built with Keras' default
    ignore_void: Optional[int] = None                        # None: off.  An int (0..16): void pixels leave every loss and metric; the void mask of
                                                             # a class-map batch is cls >= num_classes dilated by this margin (labels.host_void_mask)
    # Gradient clipping, decoupled weight decay, non-finite step skip (clip.py holds the definitions).  All off: the optimizer issues the calls it always did.
    clipnorm: Optional[float] = None                         # per variable (one Keras name; the cin segments of a split kernel share one norm)
    global_clipnorm: Optional[float] = None                  # over all trainable elements; at most one of the three clip options
    clipvalue: Optional[float] = None
    weight_decay: Optional[float] = None                     # decoupled: theta -= theta * (weight_decay * base rate) in front of the gradient update
    decay_exclude: Optional[List[str]] = None                # substrings of variable names that do not decay
    skip_nonfinite: bool = False                             # a step whose gradient's sum of squares is not finite changes nothing but the step counter
                                                             # (it still advances: a skipped step costs one t of Adam's bias correction)

    # Learning-rate schedule and the weights' moving average (schedules.py holds the definitions).  Both off: the optimizer issues the calls it always did.
    lr_schedule: Optional[object] = None                     # a schedules.LearningRateSchedule: the rate of every step is computed on the device from
                                                             # the device's step counter (rua_lr_schedule_step); lr is then not looked at
    use_ema: bool = False                                    # E = momentum * E + (1 - momentum) * P behind every optimizer step (rua_ema_step)
    ema_momentum: float = 0.99
    ema_overwrite_frequency: Optional[int] = None            # every that many steps P takes E's values

    # Gradient accumulation (accum.py holds the definition).  Off: the optimizer issues the calls it always did.
    gradient_accumulation_steps: Optional[int] = None        # K >= 2: the optimizer applies the mean of K consecutive gradients once every K calls; the
                                                             # step counter, the schedules and the moving average count updates (rua_accum_gate, rua_accum_step)

    # Focal losses and label smoothing (losses.py holds the definitions), by head.  A head that is in none of them issues the calls it always did.
    focal_gamma: Dict[str, float] = field(default_factory=dict)       # heads of kind LOSS_FOCAL_CE / LOSS_FOCAL_BCE; focal CE's per-class alpha is class_weights
    focal_alpha: Dict[str, float] = field(default_factory=dict)       # binary focal: the scalar alpha of class balancing
    class_balance: Dict[str, bool] = field(default_factory=dict)      # binary focal: apply_class_balancing
    label_smoothing: Dict[str, float] = field(default_factory=dict)   # the three cross-entropies and the two focal kinds

    # Online hard example mining (losses.py holds the definition, host_ohem), by head: head -> losses.ohem_options(...).  A training step of such a
    # head keeps only its hardest pixels (rua_ohem_select) and takes the gradient's mask and normaliser from device memory; evaluation reports the
    # plain mean.  A head that is not in it issues the calls it always did.
    ohem: Dict[str, dict] = field(default_factory=dict)

    # Lovasz-Softmax (losses.py holds the definitions, host_lovasz / host_lovasz_dz), by head: head -> losses.lovasz_options(...) for the heads of
    # kind LOSS_LOVASZ ('seg', 'bound').  Such a head's loss and d(loss)/d(probabilities) come from rua_lovasz_grad (a device-wide sort), its
    # d(total)/d(logits) from a rua_lovasz_dz launch of its own.  With no head on it every plan issues the calls it always did.
    lovasz: Dict[str, dict] = field(default_factory=dict)

    def loss_options(self) -> Dict[str, object]:
        """The per-head dicts (checkpoint metadata); a spec without them gives {}: its file carries none."""
        d = dict(focal_gamma=dict(self.focal_gamma), focal_alpha=dict(self.focal_alpha), class_balance=dict(self.class_balance),
                 label_smoothing=dict(self.label_smoothing), ohem={h: dict(o) for h, o in self.ohem.items()},
                 lovasz={h: self.head_lovasz(h) for h, k in self.kind.items() if k == L.LOSS_LOVASZ})
        return {k: v for k, v in d.items() if v}

    def head_lovasz(self, head: str) -> Optional[dict]:
        """The options of a head on the Lovasz loss with every field filled in; None: the head is on another loss."""
        if self.kind.get(head) != L.LOSS_LOVASZ:
            return None
        return {**LS.lovasz_options(), **self.lovasz.get(head, {})}

    def head_ohem(self, head: str) -> Optional[dict]:
        """The head's mining options with every field filled in; None: the head does not mine."""
        o = self.ohem.get(head)
        return None if o is None else {**LS.ohem_options(), **o}

    def head_opts(self, head: str):
        """rua_loss_opts of a head whose kind is new or whose label_smoothing > 0; None: the head takes the entries without options."""
        kind, e = self.kind[head], float(self.label_smoothing.get(head, 0.0))
        if kind not in LS.FOCAL_KINDS and e == 0.0:
            return None
        return LS.to_struct(self.focal_gamma.get(head, 0.0), e, self.focal_alpha.get(head), self.class_balance.get(head, False))

    def accum_options(self) -> Dict[str, object]:
        """The accumulation option as a dict (checkpoint metadata, Model.compile)."""
        return dict(gradient_accumulation_steps=self.gradient_accumulation_steps)

    def sched_options(self) -> Dict[str, object]:
        """The schedule (as its get_config dict, or None) and the three EMA options as a dict (checkpoint metadata)."""
        return dict(lr_schedule=self.lr_schedule.get_config() if self.lr_schedule is not None else None, use_ema=bool(self.use_ema),
                    ema_momentum=float(self.ema_momentum), ema_overwrite_frequency=self.ema_overwrite_frequency)

    def clip_options(self) -> Dict[str, object]:
        """The six options as a dict (checkpoint metadata, Model.compile)."""
        return dict(clipnorm=self.clipnorm, global_clipnorm=self.global_clipnorm, clipvalue=self.clipvalue, weight_decay=self.weight_decay,
                    decay_exclude=list(self.decay_exclude) if self.decay_exclude else None, skip_nonfinite=bool(self.skip_nonfinite))

    def clip_on(self) -> bool:
        return (self.clipnorm is not None or self.global_clipnorm is not None or self.clipvalue is not None or bool(self.weight_decay)
                or bool(self.skip_nonfinite))


# ---------------------------------------------------------------------------------------
class ParamStore:
    """All trainable parameters in ONE flat fp32 buffer (Keras creation order), so the optimizer
    is one launch and gradient all-reduce buckets are contiguous slices.  BN moving statistics
    live in a second flat buffer.  Conv kernels are stored [tap][Cout][Cin_segment]."""

    def __init__(self):
        self.entries: List[dict] = []      # trainable entries in order
        self.state: List[dict] = []        # moving_mean / moving_variance
        self.n = 0
        self.ns = 0
        self.nw = 0                        # elements in the activation-dtype weight copies
        self.convs: Dict[str, dict] = {}
        self.bns: Dict[str, dict] = {}
        self.n_conv = 0
        self.n_bn = 0

    def _add(self, name, size, **kw):
        off = self.n
        self.entries.append(dict(name=name, off=off, size=size, **kw))
        self.n += (size + 15) // 16 * 16          # 64-byte aligned slices
        return off

    def conv(self, cins: List[int], cout: int, taps: int, name: Optional[str] = None, mfma: bool = True):
        if name is None:
            name = "conv2d" if self.n_conv == 0 else f"conv2d_{self.n_conv}"
            self.n_conv += 1
        segs = []
        c0 = 0
        for ci in cins:
            off = self._add(name + "/kernel", taps * cout * ci, kind="kernel", layer=name, taps=taps, cout=cout, cin=ci, cin_off=c0,
                            cin_total=sum(cins))
            dst = -1
            if mfma:
                dst = off                                  # the activation-dtype copies share the master's index space: the optimizer writes the forward
                self.nw = self.n                           # copy element for element (rua_adam_step_w), rua_weight_prep_dgrad builds the other from it
            segs.append(dict(off=off, dst=dst, C=ci))
            c0 += ci
        boff = self._add(name + "/bias", cout, kind="bias", layer=name)
        rec = dict(name=name, segs=segs, bias=boff, taps=taps, cout=cout, mfma=mfma)
        self.convs[name] = rec
        return rec

    def bn(self, c: int):
        name = "batch_normalization" if self.n_bn == 0 else f"batch_normalization_{self.n_bn}"
        self.n_bn += 1
        g = self._add(name + "/gamma", c, kind="gamma", layer=name)
        b = self._add(name + "/beta", c, kind="beta", layer=name)
        mm = self.ns
        self.state.append(dict(name=name + "/moving_mean", off=mm, size=c, init=0.0))
        self.ns += (c + 15) // 16 * 16
        mv = self.ns
        self.state.append(dict(name=name + "/moving_variance", off=mv, size=c, init=1.0))
        self.ns += (c + 15) // 16 * 16
        rec = dict(name=name, gamma=g, beta=b, mm=mm, mv=mv, C=c)
        self.bns[name] = rec
        return rec

    # -- host <-> device ------------------------------------------------------------------
    def init_host(self, seed: int) -> Tuple[np.ndarray, np.ndarray]:
        rng = np.random.default_rng(seed)
        P = np.zeros(self.n, np.float32)
        S = np.zeros(self.ns, np.float32)
        limits = {}
        for e in self.entries:
            if e["kind"] == "kernel":
                fan = e["taps"] * e["cin_total"] + e["taps"] * e["cout"]
                lim = math.sqrt(6.0 / fan)
                P[e["off"]:e["off"] + e["size"]] = rng.uniform(-lim, lim, e["size"]).astype(np.float32)
            elif e["kind"] == "gamma":
                P[e["off"]:e["off"] + e["size"]] = 1.0
        for s in self.state:
            S[s["off"]:s["off"] + s["size"]] = s["init"]
        return P, S

    def from_keras(self, weights: Dict[str, np.ndarray]) -> Tuple[np.ndarray, np.ndarray]:
        """Keras-layout dict (kernel HWIO, bias, gamma, beta, moving_*) -> flat host buffers."""
        P = np.zeros(self.n, np.float32)
        S = np.zeros(self.ns, np.float32)
        for e in self.entries:
            w = np.asarray(weights[e["name"]], np.float32)
            if e["kind"] == "kernel":
                kh, kw, cin, cout = w.shape
                assert kh * kw == e["taps"] and cout == e["cout"] and cin == e["cin_total"], (e["name"], w.shape)
                seg = w[:, :, e["cin_off"]:e["cin_off"] + e["cin"], :]                      # (kh,kw,ci,co)
                P[e["off"]:e["off"] + e["size"]] = seg.reshape(kh * kw, e["cin"], cout).transpose(0, 2, 1).reshape(-1)
            else:
                assert w.size == e["size"], (e["name"], w.shape)
                P[e["off"]:e["off"] + e["size"]] = w.reshape(-1)
        for s in self.state:
            S[s["off"]:s["off"] + s["size"]] = np.asarray(weights[s["name"]], np.float32).reshape(-1)
        return P, S

    def to_keras(self, P: np.ndarray, S: Optional[np.ndarray] = None) -> Dict[str, np.ndarray]:
        out: Dict[str, np.ndarray] = {}
        for e in self.entries:
            v = P[e["off"]:e["off"] + e["size"]]
            if e["kind"] == "kernel":
                k = int(round(math.sqrt(e["taps"])))
                seg = v.reshape(e["taps"], e["cout"], e["cin"]).transpose(0, 2, 1).reshape(k, k, e["cin"], e["cout"])
                if e["name"] not in out:
                    out[e["name"]] = np.zeros((k, k, e["cin_total"], e["cout"]), np.float32)
                out[e["name"]][:, :, e["cin_off"]:e["cin_off"] + e["cin"], :] = seg
            else:
                out[e["name"]] = v.copy()
        if S is not None:
            for s in self.state:
                out[s["name"]] = S[s["off"]:s["off"] + s["size"]].copy()
        return out

    def count(self) -> int:
        return sum(e["size"] for e in self.entries) + sum(s["size"] for s in self.state)


# ---------------------------------------------------------------------------------------
class Ten:
    """A device activation tensor [N][H][W][C] (storage owned by a torch tensor)."""
    __slots__ = ("N", "H", "W", "C", "t", "ptr", "grad", "gw", "stats", "f32", "relu_out", "masked_w", "plain_w", "bias_offs", "bias_done", "bn_src")

    def __init__(self, t: torch.Tensor, N, H, W, C, f32=False):
        self.t, self.N, self.H, self.W, self.C, self.f32 = t, N, H, W, C, f32
        self.ptr = t.data_ptr()
        self.grad: Optional["Ten"] = None
        self.gw = False
        self.stats: Optional[int] = None
        self.relu_out = False      # output of a fused ReLU: gradient writers that know how apply the (t > 0) mask themselves
        self.masked_w = 0          # gradient writers that applied it / that did not
        self.plain_w = 0
        self.bias_offs = None      # bias of the convolution that produced this tensor, if its gradient (the per-channel sum of this tensor's
        self.bias_done = False     # gradient) may be taken by the kernel that writes the gradient: done = it was
        self.bn_src = None         # bn_node record of the ReLU-less BatchNorm that produced this tensor: the kernel that writes its whole gradient may take the
                                   # BatchNorm backward's statistics (sum g, sum g * this tensor) on the way

    @property
    def M(self):
        return self.N * self.H * self.W


def stats_replicas(blocks: int) -> int:
    """Mirror of rua_stats_replicas(): replicas of a statistics buffer fed by `blocks` workgroups."""
    r = 1
    while r < 32 and r * 8 < blocks:
        r *= 2
    return r


def conv_stats_replicas(blocks: int) -> int:
    """Replicas for statistics produced by a convolution epilogue: its workgroups finish spread over the kernel's run
    time, so ~64 adds per address do not queue up (same-address fp64 atomics serialise at ~180 ns) - and every replica
    costs each consumer block of the fused BatchNorm kernels a dependent round trip per 4 replicas in its prologue."""
    r = 1
    while r < 32 and r * 64 < blocks:
        r *= 2
    return r


class Stat:
    """fp64 statistics buffer [R][2][C] in the per-step arena."""
    __slots__ = ("ptr", "R")

    def __init__(self, ptr, R):
        self.ptr, self.R = ptr, R


class _Dummy:
    """Stand-in for a device allocation during the dry (parameter-enumeration) pass."""

    def __init__(self, n=0):
        self._n = n

    def data_ptr(self):
        return 0

    def numel(self):
        return self._n

    def element_size(self):
        return 4

    def stride(self, i):
        return 0


class Plan:
    """Recorded launches, replayed in order on one stream.  calls[i] = (fn, name, args, grads): grads are the offsets of the
    parameters whose gradient that launch writes (in the flat buffer: Engine._bucket_marks fires an all-reduce bucket after the
    last launch that names one of its parameters)."""

    def __init__(self, dry=False):
        self.calls: List[tuple] = []
        self.keep: List[object] = []
        self.dry = dry
        self.scope: Optional[str] = None     # composite the next launches belong to (per-block timing in bench.py)
        self.scopes: List[Optional[str]] = []  # scope of calls[i]

    def add(self, name: str, *args, grads=()):
        if not self.dry:
            self.calls.append((L.lib().raw(name), name, args, tuple(grads)))
            self.scopes.append(self.scope)

    def run(self, stream_ptr: int, hooks=None, first=0, last=None):
        """Replay calls [first, last).  hooks: {call index -> python callable run right after that launch} (gradient buckets)."""
        lib = L.lib()
        s = C.c_void_p(stream_ptr)
        calls = self.calls if (first == 0 and last is None) else self.calls[first:last]
        for i, (fn, name, args, _) in enumerate(calls, start=first):
            rc = fn(*args, s)
            if rc != 0:
                lib.check(rc, name)
            if hooks:
                h = hooks.get(i)
                if h is not None:
                    h()


class Coef:
    """Per-channel fp32 vectors of one BN application (scale, shift, mean, rstd, A, B, C)."""

    def __init__(self, g: "Graph", C: int):
        t = g.alloc((7, (C + 15) // 16 * 16), torch.float32, zero=True)
        self.t = t
        p, st = t.data_ptr(), t.stride(0) * 4
        self.scale, self.shift, self.mean, self.rstd, self.A, self.B, self.Cc = [p + i * st for i in range(7)]


class _BackSteps(list):
    """The backward closures of a graph, in creation order.  A closure appended while a composite tag is set records its launches
    under that tag (unless it names a scope itself, as the ResBlocks do)."""

    def __init__(self, g):
        super().__init__()
        self.g = g

    def append(self, fn):
        tag = self.g.cur_tag
        if tag is None:
            return super().append(fn)

        def run():
            Bp = self.g.bwd
            prev = Bp.scope
            Bp.scope = tag
            fn()
            Bp.scope = prev
        super().append(run)


class Graph:
    """One recorded instance of the network for a fixed batch size and mode."""

    def __init__(self, eng: "Engine", batch: int, training: bool, dry: bool = False):
        self.e = eng
        self.dry = dry
        self.cfg = eng.cfg
        self.B = batch
        self.training = training
        self.dev = eng.dev
        self.dt = eng.dt
        self.tdt = torch.bfloat16 if eng.dt == L.RUA_BF16 else torch.float32
        self.vec = 8 if eng.dt == L.RUA_BF16 else 4
        self.fwd = Plan(dry)
        self.bwd = Plan(dry)
        self.loss_plan = Plan(dry)
        self.back_steps: List = _BackSteps(self)
        self.cur_tag: Optional[str] = None      # composite being recorded (stem, down, PSP, combine, heads): per-composite timing in bench.py
        self.block_tag = ""
        self.allocs: List[torch.Tensor] = []
        self.wq = WgradQueue(eng, self.bwd, self.dt, dry, self.alloc, self.allocs.append, self.G, self.issue)     # every weight gradient of the backward goes through it
        self.stats_used = 16                 # the first 16 doubles of the arena are the loss / metric scalars
        self.act_bytes = 0
        self.img_u8 = self.cls_u8 = self.tgt_scratch = None     # compact batches (Engine._upload_compact): allocated on first use
        # LossSpec.ignore_void: the batch's void mask [B,H,W] (non-zero: void).  The plans hold its address, so it exists before they are recorded and
        # stays where it is: a captured step reads whatever mask the latest batch put there
        self.void_u8 = None
        if not dry and eng.loss is not None and eng.loss.ignore_void is not None:
            self.void_u8 = torch.zeros((batch,) + tuple(eng.cfg.input_shape[:2]), dtype=torch.uint8, device=self.dev)
        self.void_ptr = self.void_u8.data_ptr() if self.void_u8 is not None else None
        self._build()

    def compact_buffers(self):
        """uint8 image [B,H,W,Cin] and class map [B,H,W] the compact batch is uploaded into, and the targets' scratch."""
        if self.img_u8 is None:
            H, W, Cin = self.cfg.input_shape
            self.img_u8 = torch.empty((self.B, H, W, Cin), dtype=torch.uint8, device=self.dev)
            self.cls_u8 = torch.empty((self.B, H, W), dtype=torch.uint8, device=self.dev)
            n = int(L.lib().raw("rua_targets_scratch_bytes")(self.B, self.cfg.num_classes))
            self.tgt_scratch = torch.empty((max(n, 4),), dtype=torch.uint8, device=self.dev)
        return self.img_u8, self.cls_u8, self.tgt_scratch

    # -- allocation -------------------------------------------------------------------------
    def alloc(self, shape, dtype, zero=False):
        if self.dry:
            return _Dummy(int(np.prod(shape)))
        t = (torch.zeros if zero else torch.empty)(shape, dtype=dtype, device=self.dev)
        self.act_bytes += t.numel() * t.element_size()
        self.allocs.append(t)          # the plan holds raw pointers: the graph owns every buffer for its lifetime
        return t

    def new(self, N, H, W, C, f32=False) -> Ten:
        return Ten(self.alloc((N, H, W, C), torch.float32 if f32 else self.tdt), N, H, W, C, f32)

    def like(self, x: Ten) -> Ten:
        return self.new(x.N, x.H, x.W, x.C, x.f32)

    def salloc(self, n: int) -> int:
        """n doubles from the per-step statistics arena (zeroed at the start of every step)."""
        off = self.stats_used
        self.stats_used += (n + 7) // 8 * 8
        if self.dry:
            return 0
        assert self.stats_used <= self.e.stats_arena.numel(), "statistics arena exhausted"
        return self.e.stats_arena.data_ptr() + off * 8

    def stat(self, C: int, blocks: int, burst: bool = False) -> Stat:
        """burst: the producer's workgroups all finish together (rua_col_stats*); else a convolution epilogue."""
        R = stats_replicas(blocks) if burst else conv_stats_replicas(blocks)
        return Stat(self.salloc(R * 2 * C), R)

    def gacc(self, x: Ten, masked: bool = False) -> Tuple[Ten, int]:
        """Gradient buffer of x and whether the next writer must accumulate.  masked: this writer applies x's ReLU mask to
        what it writes (the mask is idempotent on a masked sum, so it commutes with accumulation)."""
        assert not x.bias_done, "a gradient whose per-channel sums were already taken (bias gradient) gets another writer"
        if x.grad is None:
            x.grad = self.like(x)
        acc = 1 if x.gw else 0
        x.gw = True
        if masked:
            x.masked_w += 1
        else:
            x.plain_w += 1
        return x.grad, acc

    # -- primitive recorders ------------------------------------------------------------------
    def P(self, off):   # pointer into the flat fp32 parameter buffer
        return 0 if self.dry else self.e.P.data_ptr() + off * 4

    def G(self, off):   # pointer into the flat fp32 gradient buffer (the launch that writes there names `off`: Plan.add(grads=))
        return 0 if self.dry else self.e.G.data_ptr() + off * 4

    def S(self, off):
        return 0 if self.dry else self.e.S.data_ptr() + off * 4

    def Wf(self, dst):
        return 0 if self.dry else self.e.Wf.data_ptr() + dst * self.e.esize

    def Wd(self, dst):
        return 0 if self.dry else self.e.Wd.data_ptr() + dst * self.e.esize

    def stat_blocks(self, x: Ten) -> int:
        """Workgroups rua_col_stats / rua_col_stats2 launch for x (>= 8 pieces per thread, at most 1024)."""
        return max(1, min(1024, x.M * (x.C // self.vec) // 2048))

    def col_stats(self, plan: Plan, x: Ten) -> Stat:
        s = self.stat(x.C, self.stat_blocks(x), burst=True)
        plan.add("rua_col_stats", x.ptr, x.M, x.C, s.ptr, s.R, self.dt)
        return s

    def bn_finalize(self, plan: Plan, stats: Optional[Stat], count, bn, bessel=None) -> Coef:
        c = Coef(self, bn["C"])
        plan.keep.append(c)
        plan.add("rua_bn_finalize", stats.ptr if self.training else None, stats.R if self.training else 1, float(count), float(bessel or count),
                 self.P(bn["gamma"]), self.P(bn["beta"]), self.S(bn["mm"]), self.S(bn["mv"]), BN_MOMENTUM, BN_EPS,
                 1 if self.training else 0, c.scale, c.shift, c.mean, c.rstd, bn["C"])
        return c

    def bn_apply(self, plan: Plan, x: Ten, coefs: List[Coef], relu: bool) -> List[Ten]:
        outs = [self.like(x) for _ in coefs]
        sc = L.ptr_array([c.scale for c in coefs]); sh = L.ptr_array([c.shift for c in coefs]); ou = L.ptr_array([o.ptr for o in outs])
        plan.keep += [sc, sh, ou]
        plan.add("rua_bn_apply", x.ptr, len(coefs), sc, sh, 1 if relu else 0, ou, x.M, x.C, self.dt)
        return outs

    def bn_fwd(self, plan: Plan, x: Ten, bns: List[dict], relu: bool, stats: Optional[Stat], count, bessel=None, defer: Optional[List] = None,
               out_stats: bool = False):
        """[relu](BN_b(x)) for every branch b in ONE launch: coefficients from the statistics in the kernel prologue,
        published to `Coef` buffers (block 0) for the ReLU masks / backward; moving statistics updated in training."""
        outs = [self.like(x) for _ in bns]
        coefs = [Coef(self, bn["C"]) for bn in bns]
        d = L.BnFwdDesc()
        d.x, d.M, d.C, d.dtype, d.nb, d.relu = x.ptr, x.M, x.C, self.dt, len(bns), 1 if relu else 0
        d.training = 1 if self.training else 0
        if self.training:
            d.stats, d.replicas = stats.ptr, stats.R
        d.count, d.bessel_n, d.momentum, d.eps = float(count), float(bessel or count), BN_MOMENTUM, BN_EPS
        for i, (bn, c, o) in enumerate(zip(bns, coefs, outs)):
            b = d.br[i]
            b.gamma, b.beta, b.moving_mean, b.moving_var = self.P(bn["gamma"]), self.P(bn["beta"]), self.S(bn["mm"]), self.S(bn["mv"])
            b.scale, b.shift, b.mean, b.rstd, b.out = c.scale, c.shift, c.mean, c.rstd, o.ptr
            if out_stats and self.training and not relu and not self.dry and self.e.bn_out_stats:
                # the output's own statistics come out of the coefficients (sum = M beta, sum of squares = M (beta^2 + gamma^2 var / (var + eps))):
                # the BatchNorms of the ResBlock this tensor feeds need no rua_col_stats pass over it
                o.stats = Stat(self.salloc(2 * x.C), 1)
                b.out_stats = o.stats.ptr
        plan.keep += coefs
        if defer is not None:                                # the caller issues several as one rua_bn_fwd_group
            defer.append(d)
            return outs, coefs
        self.issue(plan, [d], "rua_bn_fwd")
        return outs, coefs

    def issue(self, plan: Plan, descs: List, one: str, group: Optional[str] = None):
        """Descriptors of one type as ONE launch: `one` on the descriptor itself, or `group` over a packed copy of them all.  The launch
        names the gradients its descriptors write (the `grads` that WgradQueue.desc / bn_bwd give them)."""
        grads = [o for d in descs for o in getattr(d, "grads", ())]
        if len(descs) == 1:
            plan.keep.append(descs[0])
            plan.add(one, C.byref(descs[0]), grads=grads)
        elif descs:
            arr = (type(descs[0]) * len(descs))(*descs)
            plan.keep.append(arr)
            plan.add(group, arr, len(descs), grads=grads)

    def bn_fwd_group(self, plan: Plan, items: List[tuple], relu: bool, count):
        """[relu](BN(x_i)) for several tensors of equal shape, each with its own BatchNorm and statistics, as ONE launch: items = (x, bn, stats);
        returns ([out_i], [coef_i])."""
        ds, outs, coefs = [], [], []
        for x, bn, st in items:
            o, c = self.bn_fwd(plan, x, [bn], relu, st, count, defer=ds)
            outs.append(o[0]); coefs.append(c[0])
        self.issue(plan, ds, "rua_bn_fwd", "rua_bn_fwd_group")
        return outs, coefs

    def bn_coefs(self, plan: Plan, like: Ten, bns: List[dict], stats: List[Optional[Stat]], count, bessel=None) -> List[Coef]:
        """Coefficients (scale, shift, mean, rstd; moving statistics updated in training) of several BatchNorms in ONE
        one-block launch, nothing applied: the consumers normalise on load.  stats[i]: branch i's own statistics."""
        coefs = [Coef(self, bn["C"]) for bn in bns]
        d = L.BnFwdDesc()
        d.x, d.M, d.C, d.dtype, d.nb, d.relu = None, like.M, like.C, self.dt, len(bns), 1
        d.training = 1 if self.training else 0
        d.count, d.bessel_n, d.momentum, d.eps = float(count), float(bessel or count), BN_MOMENTUM, BN_EPS
        for i, (bn, c, st) in enumerate(zip(bns, coefs, stats)):
            b = d.br[i]
            b.gamma, b.beta, b.moving_mean, b.moving_var = self.P(bn["gamma"]), self.P(bn["beta"]), self.S(bn["mm"]), self.S(bn["mv"])
            b.scale, b.shift, b.mean, b.rstd, b.out = c.scale, c.shift, c.mean, c.rstd, None
            if self.training:
                b.stats, b.replicas = st.ptr, st.R
        plan.keep += [d] + coefs
        plan.add("rua_bn_fwd", C.byref(d))
        return coefs

    def bn_bwd(self, plan: Plan, gs: List[Ten], coefs: List[Coef], bns: List[dict], stats2: List[Stat], x: Ten, out: Ten,
               accumulate: int, count, dskip: Optional[Ten] = None, masked=False, skip_bias: Optional[List[int]] = None, defer: Optional[List] = None,
               dx_bias: bool = False, stats2_out: Optional[List[bool]] = None):
        """dx (=|+=) [dskip] + sum_b BN-backward_b(g_b) in ONE launch; dgamma/dbeta added by block 0.
        skip_bias: bias offsets whose gradient is the per-channel sum of dskip - accumulated by this launch while it reads
        dskip anyway (instead of a col_stats pass over the same tensor), converted by one rua_stats_to_f32."""
        d = L.BnBwdDesc()
        d.x, d.dx, d.M, d.C, d.dtype, d.nb = x.ptr, out.ptr, x.M, x.C, self.dt, len(gs)
        d.dskip = dskip.ptr if dskip is not None else None
        d.masked, d.accumulate, d.count = 1 if masked else 0, accumulate, float(count)
        for i, (g, c, bn, s2) in enumerate(zip(gs, coefs, bns, stats2)):
            b = d.br[i]
            b.g, b.stats2, b.replicas = g.ptr, s2.ptr, s2.R
            b.stats2_out = 1 if (stats2_out and stats2_out[i]) else 0
            b.gamma, b.mean, b.rstd, b.scale, b.shift = self.P(bn["gamma"]), c.mean, c.rstd, c.scale, c.shift
            b.dgamma, b.dbeta = self.G(bn["gamma"]), self.G(bn["beta"])
        d.grads = [o for bn in bns for o in (bn["gamma"], bn["beta"])]
        st = None
        cg = x.C // self.vec
        if skip_bias and dskip is not None and not (cg <= 256 and 256 % cg == 0):
            self.bias_grad(plan, dskip, skip_bias)            # (d7 in fp32: 2048 channels = 512 pieces per pixel: its own pass)
            skip_bias = None
        if skip_bias and dskip is not None:
            blocks = max(1, min(1024, x.M * (x.C // self.vec) // 256))
            st = self.stat(x.C, blocks, burst=True)
            d.skip_stats, d.skip_replicas = st.ptr, st.R
        if defer is not None:                                # the caller issues several as one rua_bn_bwd_group
            assert st is None
            defer.append(d)
            return
        sx = None
        if (dx_bias and x.bn_src is not None and not x.bn_src["fused"] and not accumulate and not self.dry and self.e.bn_dx_bias and cg <= 256 and 256 % cg == 0):
            # x is the output of a ReLU-less BatchNorm (the combine BatchNorm in front of a decoder ResBlock, model2.py:86) and `out` its complete gradient g:
            # the sums of g and of g * x taken here are the statistics that BatchNorm's backward needs (it converts x back to its own input): no rua_col_stats2 pass
            blocks = max(1, min(1024, x.M * (x.C // self.vec) // 256))
            s2 = self.stat(x.C, blocks, burst=True)
            d.dx_stats, d.dx_replicas = s2.ptr, s2.R
            x.bn_src["s2"], x.bn_src["s2_out"] = s2, True
            x.bias_done = True                               # (no further writer of this gradient)
        elif (dx_bias and x.bias_offs and not accumulate and not self.dry and self.e.bn_dx_bias and cg <= 256 and 256 % cg == 0):
            # x is the output of a convolution with a bias and `out` its complete gradient: the per-channel sums of what this launch
            # writes ARE that bias gradient (no rua_col_stats pass over the gradient: the stride-2 convs in front of the encoder ResBlocks)
            blocks = max(1, min(1024, x.M * (x.C // self.vec) // 256))
            sx = self.stat(x.C, blocks, burst=True)
            d.dx_stats, d.dx_replicas = sx.ptr, sx.R
            x.bias_done = True
        self.issue(plan, [d], "rua_bn_bwd")
        if st is not None:
            self.stats_to_grads(plan, st, x.C, skip_bias)
        if sx is not None:
            self.stats_to_grads(plan, sx, x.C, x.bias_offs)

    def bn_bwd_group(self, plan: Plan, items: List[tuple]):
        """The one-branch BatchNorm backwards of a ResBlock's dilation branches (their second BatchNorms: own gradient, own input, own
        output) as ONE launch: items = (g, coef, bn, stats2, x, out, count)."""
        ds: List = []
        for g, c, bn, s2, x, out, cnt in items:
            self.bn_bwd(plan, [g], [c], [bn], [s2], x, out, 0, cnt, defer=ds)
        self.issue(plan, ds, "rua_bn_bwd", "rua_bn_bwd_group")

    def conv(self, plan: Plan, segs, layer_segs, cout, bias_ptr, out: Ten, stride=1, residual: Optional[Ten] = None,
             out_relu=False, stats=None, bias_more=(), in_bn: Optional["Coef"] = None, accumulate: int = 0, in_fold=None):
        """segs: [(Ten, up_shift, dil, taps)], layer_segs: [param seg dict] (same order).  in_bn: the (single) source is
        read as relu(scale * x + shift) - BatchNorm + ReLU applied by the kernel as the tile lands (normalise on load)."""
        d = self.conv_desc(segs, layer_segs, cout, bias_ptr, out, stride, residual, out_relu, stats, bias_more, in_bn, accumulate, in_fold)
        plan.keep.append(d)
        plan.add("rua_conv_fwd", C.byref(d))

    def bn_fold(self, plan: Plan, bn: dict, stats: Stat, count, bessel=None):
        """(Coef, rua_bn_fold) of a training-mode BatchNorm whose coefficients the consuming convolution derives in its own
        prologue from `stats` (no coefficient launch); the Coef buffers are filled by that convolution."""
        c = Coef(self, bn["C"])
        f = L.BnFold()
        f.stats, f.replicas = stats.ptr, stats.R
        f.count, f.bessel_n, f.eps, f.momentum = float(count), float(bessel or count), BN_EPS, BN_MOMENTUM
        f.gamma, f.beta, f.moving_mean, f.moving_var = self.P(bn["gamma"]), self.P(bn["beta"]), self.S(bn["mm"]), self.S(bn["mv"])
        f.scale, f.shift, f.mean, f.rstd = c.scale, c.shift, c.mean, c.rstd
        plan.keep += [c, f]
        return c, f

    def conv_desc(self, segs, layer_segs, cout, bias_ptr, out: Ten, stride=1, residual=None, out_relu=False, stats=None, bias_more=(),
                  in_bn=None, accumulate=0, in_fold=None):
        d = L.ConvDesc()
        d.nseg = len(segs)
        for i, ((t, up, dil, taps), ps) in enumerate(zip(segs, layer_segs)):
            assert t.C == ps["C"], (t.C, ps)
            s = d.seg[i]
            s.x, s.w, s.C, s.Hs, s.Ws, s.up_shift, s.dil, s.taps = t.ptr, self.Wf(ps["dst"]), t.C, t.H, t.W, up, dil, taps
        d.N, d.H, d.W, d.Cout, d.stride, d.dtype = out.N, out.H, out.W, cout, stride, self.dt
        d.bias = bias_ptr
        for i, b in enumerate(bias_more):                  # added after `bias` in this order (<= 3)
            d.bias_more[i] = b
        if residual is not None:
            d.aux, d.aux_mode = residual.ptr, 1
        d.out_relu = 1 if out_relu else 0
        d.y, d.out_stride, d.OH, d.OW = out.ptr, 1, out.H, out.W
        if stats is not None:
            d.stats, d.stats_mode, d.stats_replicas = stats.ptr, 1, stats.R
        d.accumulate = accumulate
        if in_fold is not None:                             # the kernel derives (and publishes) the coefficients itself
            d.in_fold, d.in_relu = C.addressof(in_fold), 1
        elif in_bn is not None:
            d.in_scale, d.in_shift, d.in_relu = in_bn.scale, in_bn.shift, 1
        self._ws(d)
        return d

    def fused_input_ok(self, x: Ten, nf: int, dil: int) -> bool:
        """Does a 3x3 conv x -> nf channels at this dilation run on a kernel that normalises on load (and its weight
        gradient on the all-taps kernel, which does too)?  Asked of the library, not guessed (rua_conv_fused_input_ok)."""
        if self.dry or self.dt != L.RUA_BF16 or not self.e.fuse_bn:
            return False
        d = L.ConvDesc()
        d.nseg = 1
        sg = d.seg[0]
        sg.x, sg.w, sg.C, sg.Hs, sg.Ws, sg.up_shift, sg.dil, sg.taps = x.ptr, x.ptr, x.C, x.H, x.W, 0, dil, 9
        d.N, d.H, d.W, d.Cout, d.stride, d.dtype = x.N, x.H, x.W, nf, 1, self.dt
        d.y, d.out_stride, d.OH, d.OW = x.ptr, 1, x.H, x.W
        return L.lib().raw("rua_conv_fused_input_ok")(C.byref(d)) == 1 and self.wgrad_all_taps(x, nf, [dil])

    def wgrad_all_taps(self, x: Ten, nf: int, dils: List[int]) -> bool:
        """Do the weight gradients of the 3x3 convs x -> nf channels at these dilations run on the all-taps kernel (rua_wgrad_kind 1)?  A throw-away
        descriptor: only its geometry is read."""
        w = L.WgradDesc()
        w.a, w.C, w.Hs, w.Ws, w.dy, w.Cout, w.H, w.W = x.ptr, x.C, x.H, x.W, x.ptr, nf, x.H, x.W
        w.N, w.stride, w.taps, w.dtype = x.N, 1, 9, self.dt
        w.workspace, w.workspace_bytes = self.e.scratch.data_ptr(), self.e.scratch.numel() * 4
        for dil in dils:
            w.dil = dil
            if L.lib().raw("rua_wgrad_kind")(C.byref(w)) != 1:
                return False
        return True

    def _ws(self, d):
        """Shared split-K scratch (launches are serialised on one stream, so one buffer serves every conv)."""
        if not self.dry and self.e.split_k and d.N * d.H * d.W * d.Cout * 4 <= self.e.workspace.numel() * 4:
            d.workspace, d.workspace_bytes = self.e.workspace.data_ptr(), self.e.workspace.numel() * 4

    def dgrad(self, plan: Plan, dy: Ten, wd_ptr, cin: int, dil: int, taps: int, out: Ten, accumulate: int,
              mask: Optional[Tuple[Ten, Optional[int], Optional[int]]] = None, stats2: Optional[int] = None,
              stat_aux: Optional[Ten] = None, out_stride: int = 1):
        """out (=|+=) conv(dy, W^T flipped) [* relu-mask(aux)], optional sum g / sum g*aux statistics."""
        d = self.dgrad_desc(dy, wd_ptr, cin, dil, taps, out, accumulate, mask, stats2, stat_aux, out_stride)
        plan.keep.append(d)
        plan.add("rua_conv_fwd", C.byref(d))

    def conv_group(self, plan: Plan, descs: List):
        """Independent convolutions (the dilation branches of a ResBlock) in one call: members on the same kernel share ONE grid."""
        if len(descs) > L.RUA_MAX_BRANCH:                      # (the five sources of a PSPPooling fuse conv: the library takes RUA_MAX_BRANCH members per call)
            self.conv_group(plan, descs[:L.RUA_MAX_BRANCH])
            self.conv_group(plan, descs[L.RUA_MAX_BRANCH:])
            return
        self.issue(plan, descs, "rua_conv_fwd", "rua_conv_fwd_group")

    def conv_sum(self, plan: Plan, descs: List):
        """Convolutions into ONE output, summed (member 0 writes, the others accumulate): rua_conv_fwd_sum."""
        self.issue(plan, descs, "rua_conv_fwd", "rua_conv_fwd_sum")

    def dgrad_desc(self, dy: Ten, wd_ptr, cin: int, dil: int, taps: int, out: Ten, accumulate: int, mask=None, stats2=None,
                   stat_aux=None, out_stride: int = 1):
        d = L.ConvDesc()
        d.nseg = 1
        s = d.seg[0]
        s.x, s.w, s.C, s.Hs, s.Ws, s.up_shift, s.dil, s.taps = dy.ptr, wd_ptr, dy.C, dy.H, dy.W, 0, dil, taps
        d.N, d.H, d.W, d.Cout, d.stride, d.dtype = dy.N, dy.H, dy.W, cin, 1, self.dt
        d.accumulate = accumulate
        d.y, d.out_stride, d.OH, d.OW = out.ptr, out_stride, out.H, out.W
        if mask is not None:
            d.aux, d.aux_mode, d.mscale, d.mshift = mask[0].ptr, 2, mask[1], mask[2]
        elif stat_aux is not None:
            d.aux, d.aux_mode = stat_aux.ptr, 3
        if stats2 is not None:
            d.stats, d.stats_mode, d.stats_replicas = stats2.ptr, 2, stats2.R
        self._ws(d)
        return d

    def bias_grad(self, plan: Plan, dy: Ten, bias_offs: List[int]):
        s = self.col_stats(plan, dy)
        self.stats_to_grads(plan, s, dy.C, bias_offs)

    def stats_to_grads(self, plan: Plan, s: Stat, Cc: int, offs: List[int]):
        """G[off .. off + C) += per-channel sums of `s` for every offset: its own small launch, or - deferred - records of the next
        batched reduction launch (WgradQueue.stats_records)."""
        if self.wq.defers(plan):
            return self.wq.stats_records(s, Cc, offs)
        dst = L.ptr_array([self.G(o) for o in offs])
        plan.keep.append(dst)
        plan.add("rua_stats_to_f32", s.ptr, s.R, Cc, dst, len(offs), grads=offs)

    def bn_bwd_finalize(self, plan: Plan, stats2, count, bn, coef: Coef):
        plan.add("rua_bn_bwd_finalize", stats2.ptr, stats2.R, float(count), self.P(bn["gamma"]), coef.mean, coef.rstd,
                 self.G(bn["gamma"]), self.G(bn["beta"]), coef.A, coef.B, coef.Cc, bn["C"], grads=(bn["gamma"], bn["beta"]))

    def bn_bwd_apply(self, plan: Plan, gs: List[Ten], coefs: List[Coef], x: Ten, out: Ten, accumulate: int,
                     dskip: Optional[Ten] = None, masked=False):
        g = L.ptr_array([t.ptr for t in gs]); A = L.ptr_array([c.A for c in coefs]); Bc = L.ptr_array([c.B for c in coefs])
        Cc = L.ptr_array([c.Cc for c in coefs]); ms = L.ptr_array([c.scale for c in coefs]); mt = L.ptr_array([c.shift for c in coefs])
        plan.keep += [g, A, Bc, Cc, ms, mt]
        plan.add("rua_bn_bwd_apply", len(gs), g, A, Bc, Cc, ms, mt, 1 if masked else 0, x.ptr,
                 dskip.ptr if dskip is not None else None, out.ptr, accumulate, x.M, x.C, self.dt)

    # -- layers: created on the first graph build, replayed (same order) on later builds ----------
    def Lconv(self, cins, cout, taps, name=None, mfma=True):
        return self.e.layer("conv", cins, cout, taps, name, mfma)

    def Lbn(self, c):
        return self.e.layer("bn", c)

    # -- composites -------------------------------------------------------------------------------
    def resblock(self, x: Ten, nf: int, dils: List[int]) -> Ten:
        """model2.py:15-34.  BN1 statistics are shared by all branches (same input)."""
        tr, F = self.training, self.fwd
        v2 = self.cfg.variant == "model2"
        scope = f"{self.block_tag}:ResBlock({nf},{dils})@{x.H}x{x.W}"
        F.scope = scope
        lay = [(self.Lbn(nf), self.Lconv([nf], nf, 9), self.Lbn(nf), self.Lconv([nf], nf, 9)) for _ in dils]
        cnt = x.M
        if tr and x.stats is None:
            x.stats = self.col_stats(F, x)
        if all(self.fused_input_ok(x, nf, d) for d in dils) or self.group_fused_ok(x, nf, dils):
            return self.resblock_fused(x, nf, dils, lay, scope)
        a1, coef1 = self.bn_fwd(F, x, [l[0] for l in lay], True, x.stats, cnt)
        y1 = [self.like(x) for _ in dils]
        st1 = [self.stat(nf, (cnt + 127) // 128) if tr else None for _ in dils]
        # the branches are independent until the final sum: their first convs go out as one grouped call
        self.conv_group(F, [self.conv_desc([(a, 0, d, 9)], l[1]["segs"], nf, self.P(l[1]["bias"]), y, stats=st)
                            for d, l, a, y, st in zip(dils, lay, a1, y1, st1)])
        out = self.like(x)
        # Second stage.  Where the library sums the branches on chip with every BatchNorm applied on load (rua_conv_fwd_sum ->
        # conv_band64 at the C = 64 level) no normalised copy of a first-conv output is written: ONE launch instead of a
        # rua_bn_fwd per branch + the concatenated conv; the weight gradients then normalise y1_b on load as well.
        sum2 = self.second_stage_sum_ok(x, y1, nf, dils, lay, out)
        if sum2:
            nb = len(dils)
            if tr and self.e.fold_bn:
                cf2 = [self.bn_fold(F, l[2], st, cnt) for l, st in zip(lay, st1)]
                coef2, fold2 = [c for c, _ in cf2], [f for _, f in cf2]
            else:
                coef2, fold2 = self.bn_coefs(F, x, [l[2] for l in lay], st1, cnt), [None] * nb
            a2 = [None] * nb
            self.conv_sum(F, [self.conv_desc([(y, 0, d, 9)], [l[3]["segs"][0]], nf, self.P(l[3]["bias"]), out, in_bn=c2, in_fold=f2,
                                             residual=x if (v2 and bi == 0) else None, accumulate=1 if bi > 0 else 0)
                              for bi, (d, l, y, c2, f2) in enumerate(zip(dils, lay, y1, coef2, fold2))])
        else:
            a2, coef2 = self.bn_fwd_group(F, [(y, l[2], st) for l, y, st in zip(lay, y1, st1)], True, cnt)
            biases = [self.P(l[3]["bias"]) for l in lay]        # the concatenated conv's bias = sum of the branches' biases
            self.conv(F, [(a, 0, d, 9) for a, d in zip(a2, dils)], [l[3]["segs"][0] for l in lay], nf, biases[0], out,
                      residual=x if v2 else None, bias_more=biases[1:])
        F.scope = None
        if not tr:
            return out

        in2 = list(zip(y1, coef2)) if sum2 else [(a, None) for a in a2]      # (sum2: y1_b normalised on load by the weight gradient too)
        self.resblock_back(x, out, nf, dils, lay, scope, y1, coef1, coef2, in2, [(a, None) for a in a1])
        return out

    def group_fused_ok(self, x: Ten, nf: int, dils: List[int]) -> bool:
        """The C = 64 level: no single convolution normalises on load there, but rua_conv_fwd_group runs the branches' first convs
        (and their data gradients) as ONE conv_band64m launch that does, rua_conv_fwd_sum the second convs (conv_band64), and the
        all-taps weight gradient normalises on load as well - then the whole ResBlock takes the normalise-on-load path."""
        if self.dry or self.dt != L.RUA_BF16 or not self.e.fuse_bn or len(dils) < 2:
            return False
        lib = L.lib()
        arr = (L.ConvDesc * len(dils))()
        dummy = L.BnFold()
        outs = [self.e.scratch.data_ptr() + 4096 * (i + 1) for i in range(len(dils))]       # distinct, never dereferenced
        for bi, d in enumerate(dils):
            q = arr[bi]
            q.nseg = 1
            sg = q.seg[0]
            sg.x, sg.w, sg.C, sg.Hs, sg.Ws, sg.up_shift, sg.dil, sg.taps = x.ptr, x.ptr, x.C, x.H, x.W, 0, d, 9
            q.N, q.H, q.W, q.Cout, q.stride, q.dtype = x.N, x.H, x.W, nf, 1, self.dt
            q.y, q.out_stride, q.OH, q.OW = outs[bi], 1, x.H, x.W
            q.in_fold, q.in_relu = C.addressof(dummy), 1
        if lib.raw("rua_conv_group_band_ok")(arr, len(dils)) != 1:
            return False
        for bi in range(len(dils)):                          # ... and the second convs as one summed launch
            arr[bi].y = outs[0]
            arr[bi].accumulate = 1 if bi > 0 else 0
        return lib.raw("rua_conv_sum_kernel")(arr, len(dils)) != 0 and self.wgrad_all_taps(x, nf, dils)

    def second_stage_sum_ok(self, x: Ten, y1: List[Ten], nf: int, dils: List[int], lay, out: Ten) -> bool:
        """Does the library run `out = x + sum_b conv(relu(BN2_b(y1_b)))` as ONE launch with the BatchNorms applied on load
        (rua_conv_sum_kernel), and the matching weight gradient with y1_b normalised on load (the all-taps kernel)?  Asked of the
        library, not guessed."""
        if self.dry or self.dt != L.RUA_BF16 or not self.e.fuse_bn or len(dils) < 1:
            return False
        arr = (L.ConvDesc * len(dils))()
        dummy = L.BnFold()
        for bi, (d, y) in enumerate(zip(dils, y1)):
            q = arr[bi]
            q.nseg = 1
            sg = q.seg[0]
            sg.x, sg.w, sg.C, sg.Hs, sg.Ws, sg.up_shift, sg.dil, sg.taps = y.ptr, y.ptr, y.C, y.H, y.W, 0, d, 9
            q.N, q.H, q.W, q.Cout, q.stride, q.dtype = x.N, x.H, x.W, nf, 1, self.dt
            q.y, q.out_stride, q.OH, q.OW = out.ptr, 1, x.H, x.W
            q.accumulate = 1 if bi > 0 else 0
            q.in_fold, q.in_relu = C.addressof(dummy), 1
        lib = L.lib()
        return lib.raw("rua_conv_sum_kernel")(arr, len(dils)) != 0 and self.wgrad_all_taps(x, nf, dils)

    def resblock_fused(self, x: Ten, nf: int, dils: List[int], lay, scope: str) -> Ten:
        """The same ResBlock (model2.py:15-34) with every BatchNorm + ReLU applied ON LOAD by the consuming kernel: no
        normalised copy of x or of a first-conv output is ever written.  Forward per branch: conv(relu(BN1_b(x))) -> y1_b
        (statistics in the epilogue) ; one coefficient launch for all BN2_b ; out = x + sum_b conv(relu(BN2_b(y1_b))) as one
        residual launch and accumulating launches (each reads its y1_b once).  Backward: the weight gradients read x / y1_b
        and normalise on load too; masks and BN-backward sums come out of the data-gradient epilogues as before."""
        tr, F = self.training, self.fwd
        v2 = self.cfg.variant == "model2"
        cnt = x.M
        nb = len(dils)
        fold = tr and self.e.fold_bn
        if fold:                                             # training: the convs derive the BN coefficients in their prologue
            cf1 = [self.bn_fold(F, l[0], x.stats, cnt) for l in lay]
            coef1, fold1 = [c for c, _ in cf1], [f for _, f in cf1]
        else:
            coef1, fold1 = self.bn_coefs(F, x, [l[0] for l in lay], [x.stats] * nb, cnt), [None] * nb
        y1 = [self.like(x) for _ in dils]
        st1 = [self.stat(nf, (cnt + 127) // 128) if tr else None for _ in dils]
        self.conv_group(F, [self.conv_desc([(x, 0, d, 9)], l[1]["segs"], nf, self.P(l[1]["bias"]), y, stats=st, in_bn=c1, in_fold=f1)
                            for d, l, c1, f1, y, st in zip(dils, lay, coef1, fold1, y1, st1)])       # all four dilations: ONE grid
        if fold:
            cf2 = [self.bn_fold(F, l[2], st, cnt) for l, st in zip(lay, st1)]
            coef2, fold2 = [c for c, _ in cf2], [f for _, f in cf2]
        else:
            coef2, fold2 = self.bn_coefs(F, x, [l[2] for l in lay], st1, cnt), [None] * nb
        out = self.like(x)
        # out = x + sum of the branches' second convs: ONE call, the sum kept on chip where the library has the kernel for it
        # (rua_conv_fwd_sum -> conv_band32: out written once); otherwise the members run one by one, member 0 with the residual
        self.conv_sum(F, [self.conv_desc([(y, 0, d, 9)], [l[3]["segs"][0]], nf, self.P(l[3]["bias"]), out, in_bn=c2, in_fold=f2,
                                         residual=x if (v2 and bi == 0) else None, accumulate=1 if bi > 0 else 0)
                          for bi, (d, l, y, c2, f2) in enumerate(zip(dils, lay, y1, coef2, fold2))])
        F.scope = None
        if not tr:
            return out

        self.resblock_back(x, out, nf, dils, lay, scope, y1, coef1, coef2, list(zip(y1, coef2)), [(x, c1) for c1 in coef1])
        return out

    def resblock_back(self, x: Ten, out: Ten, nf: int, dils: List[int], lay, scope: str, y1: List[Ten], coef1, coef2, in2: List[tuple], in1: List[tuple]):
        """The backward of both ResBlock forms.  in2 / in1: per branch, what its second / first convolution read - (tensor, the Coef it was normalised with
        on load, or None for a materialised BatchNorm + ReLU output) - and so what their weight gradients read."""
        v2, cnt = self.cfg.variant == "model2", x.M

        def back():
            Bp = self.bwd
            Bp.scope = scope
            dO = out.grad
            if not v2:
                self.bias_grad(Bp, dO, [l[3]["bias"] for l in lay])      # (model2: summed by the final bn_bwd, which reads dO as the skip gradient)
            w2 = self.wq.now_or_later(Bp, [WSpec(a, dO, l[3]["segs"][0]["off"], 1, d, 9, c) for d, l, (a, c) in zip(dils, lay, in2)])
            g2s = [self.like(x) for _ in dils]
            s2s = [self.stat(nf, (cnt + 127) // 128) for _ in dils]
            self.conv_group(Bp, [self.dgrad_desc(dO, self.Wd(l[3]["segs"][0]["dst"]), nf, d, 9, g2, 0, mask=(y, c2.scale, c2.shift), stats2=s2)
                                 for d, l, y, c2, g2, s2 in zip(dils, lay, y1, coef2, g2s, s2s)])
            dy1s = [self.like(x) for _ in dils]
            self.bn_bwd_group(Bp, [(g2, c2, l[2], s2, y, dy1, cnt) for l, y, c2, g2, s2, dy1 in zip(lay, y1, coef2, g2s, s2s, dy1s)])
            # no bias gradient launch: the output of a BN backward sums to zero per channel, so d b1 == 0 exactly
            self.wq.group(Bp, w2 + [WSpec(a, dy1, l[1]["segs"][0]["off"], 1, d, 9, c) for d, l, (a, c), dy1 in zip(dils, lay, in1, dy1s)])
            g1s = g2s                                          # g2 is dead after its bn_bwd: reuse the storage
            s1s = [self.stat(nf, (cnt + 127) // 128) for _ in dils]
            self.conv_group(Bp, [self.dgrad_desc(dy1, self.Wd(l[1]["segs"][0]["dst"]), nf, d, 9, g1, 0, mask=(x, c1.scale, c1.shift), stats2=s1)
                                 for d, l, dy1, c1, g1, s1 in zip(dils, lay, dy1s, coef1, g1s, s1s)])
            gx, acc = self.gacc(x)
            self.bn_bwd(Bp, g1s, coef1, [l[0] for l in lay], s1s, x, gx, acc, cnt, dskip=dO if v2 else None,
                        skip_bias=[l[3]["bias"] for l in lay] if v2 else None, dx_bias=True)
            Bp.scope = None
        self.back_steps.append(back)

    def down(self, x: Ten, nf: int) -> Ten:
        """Conv2D(nf,(1,1),strides=(2,2)) model2.py:103-111: samples pixels 0,2,4,..; no BN, no activation."""
        F, tr = self.fwd, self.training
        lay = self.Lconv([x.C], nf, 1)
        y = self.new(x.N, x.H // 2, x.W // 2, nf)
        st = self.stat(nf, (y.M + 127) // 128) if tr else None
        self.conv(F, [(x, 0, 1, 1)], lay["segs"], nf, self.P(lay["bias"]), y, stride=2, stats=st)
        y.stats = st
        y.bias_offs = [lay["bias"]]                          # the ResBlock behind it writes y's whole gradient: it may take the bias gradient on the way
        if tr:
            def back():
                Bp = self.bwd
                dy = y.grad
                if not y.bias_done:
                    self.bias_grad(Bp, dy, [lay["bias"]])
                self.wq.one(Bp, WSpec(x, dy, lay["segs"][0]["off"], 2, 1, 1))
                gx, acc = self.gacc(x)
                if not acc:
                    Bp.add("rua_fill_zero", gx.ptr, gx.t.numel() * gx.t.element_size())
                self.dgrad(Bp, dy, self.Wd(lay["segs"][0]["dst"]), x.C, 1, 1, gx, 1, out_stride=2)
            self.back_steps.append(back)
        return y

    def bn_node(self, x: Ten, bn, relu: bool, count=None, bessel=None, stats=None, defer: Optional[List] = None):
        """y = [relu](BN(x)) materialised; returns (y, coef, backward(fused: bool)).
        If the single consumer's dgrad wrote g (masked) and statistics itself, `fused` skips both."""
        F, tr = self.fwd, self.training
        cnt = count or x.M
        if tr and stats is None:
            stats = x.stats if x.stats is not None else self.col_stats(F, x)
        ys, coefs = self.bn_fwd(F, x, [bn], relu, stats, cnt, bessel, defer=defer, out_stats=True)     # defer: the caller issues several as one group launch
        y, coef = ys[0], coefs[0]
        node = dict(x=x, y=y, coef=coef, bn=bn, relu=relu, cnt=cnt, s2=None, fused=False, s2_out=False)
        if not relu and tr:
            y.bn_src = node

        def back(defer=None):
            Bp = self.bwd
            g = y.grad
            if not node["fused"] and not node["s2_out"]:
                node["s2"] = self.stat(x.C, self.stat_blocks(x), burst=True)
                Bp.add("rua_col_stats2", g.ptr, x.ptr, coef.scale, coef.shift, 1 if relu else 0, x.M, x.C, node["s2"].ptr, node["s2"].R, self.dt)
            gx, acc = self.gacc(x)
            self.bn_bwd(Bp, [g], [coef], [bn], [node["s2"]], x, gx, acc, cnt, masked=(relu and not node["fused"]), defer=defer,
                        stats2_out=[node["s2_out"]])
        node["back"] = back
        return y, node

    def fuse_target(self, node):
        """dgrad epilogue arguments that make `node`'s backward fused (single consumer only)."""
        node["fused"] = True
        node["s2"] = self.stat(node["x"].C, (node["x"].M + 127) // 128)
        g, _ = self.gacc(node["y"])
        if node["relu"]:
            return dict(out=g, mask=(node["x"], node["coef"].scale, node["coef"].shift), stats2=node["s2"])
        return dict(out=g, stat_aux=node["x"], stats2=node["s2"])

    def conv1x1_multi(self, segs, cout, out_hw, want_stats=True, defer: Optional[List] = None):
        """1x1 conv over concatenated sources [(Ten, up_shift)] -> raw output (with statistics).  defer: the descriptor is appended to this list
        instead of being launched (the caller issues independent convolutions as one group: Graph.conv_group)."""
        F, tr = self.fwd, self.training
        lay = self.Lconv([t.C for t, _ in segs], cout, 1)
        y = self.new(self.B, out_hw[0], out_hw[1], cout)
        st = self.stat(cout, (y.M + 127) // 128) if (tr and want_stats) else None
        if defer is not None:
            defer.append(self.conv_desc([(t, up, 1, 1) for t, up in segs], lay["segs"], cout, self.P(lay["bias"]), y, stats=st))
        else:
            self.conv(F, [(t, up, 1, 1) for t, up in segs], lay["segs"], cout, self.P(lay["bias"]), y, stats=st)
        y.stats = st
        return y, lay

    def conv1x1_multi_back(self, Bp, segs, lay, y: Ten, targets, bias: bool = False):
        """Backward of conv1x1_multi.  targets[i] = dict(out, mask/stat_aux/stats2) for a fused BN source,
        or None for a plain accumulate into the source's gradient.  In the model2 graph every conv1x1_multi is
        followed by a training-mode BatchNorm, so its bias gradient (the per-channel sum of a BN backward output) is
        exactly zero and no launch is spent on it; the model.py graph has no BN there and asks for it (bias=True)."""
        dy = y.grad
        if bias:
            self.bias_grad(Bp, dy, [lay["bias"]])
        pooled = {0: dy}
        ups = sorted({up for _, up in segs})
        if ups == [0, 1, 2, 3] and dy.H % 8 == 0 and dy.W % 8 == 0 and self.e.pool_pyramid:      # the PSP fuse conv: 2 / 4 / 8 in one pass over dy
            for up in (1, 2, 3):
                pooled[up] = self.new(dy.N, dy.H >> up, dy.W >> up, dy.C)
            Bp.add("rua_sumpool_pyramid", dy.ptr, pooled[1].ptr, pooled[2].ptr, pooled[3].ptr, dy.N, dy.H, dy.W, dy.C, self.dt)
        for (t, up), seg, tg in zip(segs, lay["segs"], targets):
            if up not in pooled:
                k = 1 << up
                pd = self.new(dy.N, dy.H // k, dy.W // k, dy.C)
                Bp.add("rua_sumpool", dy.ptr, pd.ptr, dy.N, dy.H, dy.W, dy.C, k, self.dt)
                pooled[up] = pd
        grouped = len(segs) > 1 and not self.dry and self.e.group_1x1 and self.dt == L.RUA_BF16
        ddescs = []
        # the per-source weight gradients: one grid where every member is a wgrad_pw launch (round 5), else one launch each (as a generic group these
        # unequal, tiny weight gradients measured slower - 18 vs 12 us)
        self.wq.pw_group(Bp, [WSpec(t, pooled[up], seg["off"], 1, 1, 1) for (t, up), seg in zip(segs, lay["segs"])])
        for (t, up), seg, tg in zip(segs, lay["segs"], targets):
            d = pooled[up]
            if tg is None:
                gx, acc = self.gacc(t)
                dd = self.dgrad_desc(d, self.Wd(seg["dst"]), t.C, 1, 1, gx, acc)
            else:
                dd = self.dgrad_desc(d, self.Wd(seg["dst"]), t.C, 1, 1, tg["out"], 0, tg.get("mask"), tg.get("stats2"), tg.get("stat_aux"))
            if grouped:
                ddescs.append(dd)
            else:
                Bp.keep.append(dd)
                Bp.add("rua_conv_fwd", C.byref(dd))
        if grouped:
            # the sources of a concatenating 1x1 conv have their own gradients: the data gradients of all sources as one group (members on the same
            # kernel share a grid: the pooled PSPPooling branches are ~10 us of latency apiece)
            self.conv_group(Bp, ddescs)

    def psp(self, x: Ten, nf: int) -> Ten:
        """PSPPooling + the ReLU the caller applies (model2.py:41-79,116,142): max-pool k -> [nearest up] ->
        1x1 conv + BN per branch, concat with the input, 1x1 conv + BN, ReLU.  The pooled branches are
        convolved and normalised at pooled resolution (conv and BN statistics commute with replication)
        and the upsample is folded into the fuse conv's read."""
        F, tr = self.fwd, self.training
        w_in = self.cfg.input_shape[1]
        ks = [1, 2] + ([4] if w_in >= 128 else []) + ([8] if w_in >= 256 else [])
        pooled, idxs = [], []
        pyramid = ks == [1, 2, 4, 8] and x.H % 8 == 0 and x.W % 8 == 0 and self.e.pool_pyramid     # one pass for the three poolings
        for k in ks:
            if k == 1:
                pooled.append(x); idxs.append(None)
            else:
                assert x.H % k == 0 and x.W % k == 0, f"PSP pool {k} does not divide {x.H}x{x.W}"
                p = self.new(x.N, x.H // k, x.W // k, x.C)
                idx = self.alloc((p.t.numel(),), torch.uint8)
                F.keep.append(idx)
                if not pyramid:
                    F.add("rua_maxpool_fwd", x.ptr, p.ptr, idx.data_ptr(), x.N, x.H, x.W, x.C, k, self.dt)
                pooled.append(p); idxs.append(idx)
        if pyramid:                                            # x is read once (k = 2); the 4- and 8-windows come from the level below
            F.add("rua_maxpool_fwd", x.ptr, pooled[1].ptr, idxs[1].data_ptr(), x.N, x.H, x.W, x.C, 2, self.dt)
            F.add("rua_maxpool_derive", pooled[1].ptr, idxs[1].data_ptr(), pooled[2].ptr, idxs[2].data_ptr(), x.N, x.H // 2, x.W // 2, x.C, 2, self.dt)
            F.add("rua_maxpool_derive", pooled[2].ptr, idxs[2].data_ptr(), pooled[3].ptr, idxs[3].data_ptr(), x.N, x.H // 4, x.W // 4, x.C, 4, self.dt)
        # Keras creates the branch Conv2DN layers (conv, bn) in order, then the fuse Conv2DN
        br, bds = [], []
        group_bn = not self.dry and self.dt == L.RUA_BF16      # the branches' BatchNorms (equal channels, unequal pixel counts) as ONE launch
        zs = []
        bdescs = [] if (not self.dry and self.e.group_1x1 and self.dt == L.RUA_BF16) else None       # the branch convolutions as ONE group
        for k, p in zip(ks, pooled):
            z, lay = self.conv1x1_multi([(p, 0)], nf // 4, (p.H, p.W), defer=bdescs)
            bn = self.Lbn(nf // 4)
            zs.append((k, p, z, lay, bn))
            if not group_bn:
                zb, node = self.bn_node(z, bn, False, count=z.M, bessel=z.M * k * k, stats=z.stats)
                br.append((k, p, z, lay, zb, node))
        if bdescs:                                             # (only with group_bn: the BatchNorms follow as one launch)
            self.conv_group(F, bdescs)
        if group_bn:
            for k, p, z, lay, bn in zs:
                zb, node = self.bn_node(z, bn, False, count=z.M, bessel=z.M * k * k, stats=z.stats, defer=bds)
                br.append((k, p, z, lay, zb, node))
            self.issue(F, bds, "rua_bn_fwd", "rua_bn_fwd_group")
        segs = [(b[4], int(math.log2(b[0]))) for b in br] + [(x, 0)]
        zf, layf = self.conv1x1_multi(segs, nf, (x.H, x.W))
        bnf = self.Lbn(nf)
        out, nodef = self.bn_node(zf, bnf, True, stats=zf.stats)
        if tr:
            def back():
                Bp = self.bwd
                nodef["back"]()                                    # out.grad -> zf.grad (unfused: several consumers)
                targets = [self.fuse_target(b[5]) for b in br] + [None]
                self.conv1x1_multi_back(Bp, segs, layf, zf, targets)
                bbs = [] if (group_bn and all(b_[5]["fused"] for b_ in br)) else None
                if bbs is not None:                                # every zb.grad is there: the four BatchNorm backwards as one launch
                    for b_ in br:
                        b_[5]["back"](defer=bbs)
                    self.issue(Bp, bbs, "rua_bn_bwd", "rua_bn_bwd_group")
                if bbs is not None and pyramid and bdescs is not None:
                    # the branch convolutions' data gradients as one group (independent: own source gradients)
                    self.wq.pw_group(Bp, [WSpec(p, z.grad, lay["segs"][0]["off"], 1, 1, 1) for (k, p, z, lay, zb, node) in br])
                    dd = []
                    for (k, p, z, lay, zb, node) in br:
                        gx, acc = self.gacc(p)
                        dd.append(self.dgrad_desc(z.grad, self.Wd(lay["segs"][0]["dst"]), p.C, 1, 1, gx, acc))
                    self.conv_group(Bp, dd)
                else:
                    for (k, p, z, lay, zb, node), idx in zip(br, idxs):
                        if bbs is None:
                            node["back"]()                             # zb.grad -> z.grad
                        self.conv1x1_multi_back(Bp, [(p, 0)], lay, z, [None])   # -> p.grad (p is x for k == 1)
                        if k > 1 and not pyramid:
                            gx, acc = self.gacc(x)
                            Bp.add("rua_maxpool_bwd", p.grad.ptr, idx.data_ptr(), gx.ptr, acc, x.N, x.H, x.W, x.C, k, self.dt)
                if pyramid:                                        # the three pooled gradients scattered in ONE pass over x.grad
                    gx, acc = self.gacc(x)
                    dys = L.ptr_array([b_[1].grad.ptr for b_ in br[1:]]); ixs = L.ptr_array([i.data_ptr() for i in idxs[1:]])
                    kk = (C.c_int32 * 3)(2, 4, 8)
                    Bp.keep += [dys, ixs, kk]
                    Bp.add("rua_maxpool_bwd_multi", 3, dys, ixs, kk, gx.ptr, acc, x.N, x.H, x.W, x.C, self.dt)
            self.back_steps.append(back)
        return out

    def up_combine(self, x: Ten, skip: Ten, nf: int) -> Ten:
        """UpSampling(x, nf/2) then combine(., skip, nf)  (model2.py:81-94): nearest x2 -> 1x1 conv -> BN, then
        ReLU || skip -> 1x1 conv -> BN.  The 1x1 conv and its BN run at LOW resolution (exact: conv and BN
        batch statistics commute with nearest replication) and the x2 is folded into the combine conv's read."""
        F, tr = self.fwd, self.training
        z, lay_u = self.conv1x1_multi([(x, 0)], nf // 2, (x.H, x.W))
        bn_u = self.Lbn(nf // 2)
        a, node_u = self.bn_node(z, bn_u, True, count=z.M, bessel=z.M * 4, stats=z.stats)
        segs = [(a, 1), (skip, 0)]
        zc, lay_c = self.conv1x1_multi(segs, nf, (skip.H, skip.W))
        bn_c = self.Lbn(nf)
        t, node_c = self.bn_node(zc, bn_c, False, stats=zc.stats)
        if tr:
            def back():
                Bp = self.bwd
                node_c["back"]()
                self.conv1x1_multi_back(Bp, segs, lay_c, zc, [self.fuse_target(node_u), None])
                node_u["back"]()
                self.conv1x1_multi_back(Bp, [(x, 0)], lay_u, z, [None])
            self.back_steps.append(back)
        return t

    def final_combine(self, x: Ten, c1: Ten, nf: int) -> Ten:
        """x_comb = combine(x, c1, 32)  (model2.py:140): ReLU(x) || c1 -> 1x1 conv -> BN."""
        F, tr = self.fwd, self.training
        r = self.like(x)
        F.add("rua_relu", x.ptr, r.ptr, x.t.numel(), self.dt)
        segs = [(r, 0), (c1, 0)]
        zc, lay = self.conv1x1_multi(segs, nf, (x.H, x.W))
        bn = self.Lbn(nf)
        t, node = self.bn_node(zc, bn, False, stats=zc.stats)
        if tr:
            def back():
                Bp = self.bwd
                node["back"]()
                gx, acc = self.gacc(x)
                assert acc == 0
                self.conv1x1_multi_back(Bp, segs, lay, zc, [dict(out=gx, mask=(x, None, None)), None])
            self.back_steps.append(back)
        return t

    # -- ResUnet_a/model.py graph: no BN around the 1x1 convs, no ReLU after PSP, no skip term in ResBlock ---------
    def psp_v1(self, x: Ten, nf: int) -> Ten:
        """PSPPooling of model.py:35-64: max-pool k -> 1x1 conv (bias, no BN) -> nearest up k; concat with the input;
        1x1 conv.  The convs already run at pooled resolution in the reference; the upsample is folded into the
        fuse conv's read."""
        F, tr = self.fwd, self.training
        w_in = self.cfg.input_shape[1]
        ks = [1, 2] + ([4] if w_in >= 128 else []) + ([8] if w_in >= 256 else [])
        br = []
        for k in ks:
            p, idx = x, None
            if k > 1:
                assert x.H % k == 0 and x.W % k == 0, f"PSP pool {k} does not divide {x.H}x{x.W}"
                p = self.new(x.N, x.H // k, x.W // k, x.C)
                idx = self.alloc((p.t.numel(),), torch.uint8)
                F.keep.append(idx)
                F.add("rua_maxpool_fwd", x.ptr, p.ptr, idx.data_ptr(), x.N, x.H, x.W, x.C, k, self.dt)
            br.append([k, p, idx])
        for b in br:                                             # Keras creates the branch convs after all the pools
            z, lay = self.conv1x1_multi([(b[1], 0)], nf // 4, (b[1].H, b[1].W), want_stats=False)
            b += [z, lay]
        segs = [(b[3], int(math.log2(b[0]))) for b in br] + [(x, 0)]
        zf, layf = self.conv1x1_multi(segs, nf, (x.H, x.W), want_stats=False)
        if tr:
            def back():
                Bp = self.bwd
                self.conv1x1_multi_back(Bp, segs, layf, zf, [None] * len(segs), bias=True)
                for k, p, idx, z, lay in br:
                    self.conv1x1_multi_back(Bp, [(p, 0)], lay, z, [None], bias=True)     # -> p.grad (p is x for k == 1)
                    if k > 1:
                        gx, acc = self.gacc(x)
                        Bp.add("rua_maxpool_bwd", p.grad.ptr, idx.data_ptr(), gx.ptr, acc, x.N, x.H, x.W, x.C, k, self.dt)
            self.back_steps.append(back)
        return zf

    def relu_cat_conv_v1(self, z: Ten, up: int, skip: Ten, nf: int, want_stats: bool) -> Ten:
        """combine() of model.py:66-70: ReLU(z) [nearest x2^up, folded into the read] || skip -> 1x1 conv (bias, no BN)."""
        F, tr = self.fwd, self.training
        r = self.like(z)
        F.add("rua_relu", z.ptr, r.ptr, z.t.numel(), self.dt)
        segs = [(r, up), (skip, 0)]
        zc, lay = self.conv1x1_multi(segs, nf, (skip.H, skip.W), want_stats=want_stats)
        if tr:
            def back():
                gz, acc = self.gacc(z)
                assert acc == 0
                self.conv1x1_multi_back(self.bwd, segs, lay, zc, [dict(out=gz, mask=(z, None, None)), None], bias=True)
            self.back_steps.append(back)
        return zc

    def up_combine_v1(self, x: Ten, skip: Ten, nf: int) -> Ten:
        """model.py:93-95: Conv2D(nf,(1,1)) at low resolution -> UpSampling2D -> combine(., skip, nf)."""
        z, lay_u = self.conv1x1_multi([(x, 0)], nf, (x.H, x.W), want_stats=False)
        if self.training:
            self.back_steps.append(lambda: self.conv1x1_multi_back(self.bwd, [(x, 0)], lay_u, z, [None], bias=True))
        return self.relu_cat_conv_v1(z, 1, skip, nf, want_stats=True)

    def conv3x3_relu(self, x: Ten, nf: int, name=None):
        """ZeroPadding2D(1)+Conv2D(32,(3,3),relu,valid) of the heads (model2.py:153-158) == same-pad 3x3 + ReLU.
        The ReLU's backward mask is applied by whoever writes y.grad (the next conv's data gradient or the head's), so no
        separate masking pass over dy runs; it is launched only if some writer could not."""
        F, tr = self.fwd, self.training
        lay = self.Lconv([x.C], nf, 9, name=name)
        y = self.new(x.N, x.H, x.W, nf)
        y.relu_out = True
        self.conv(F, [(x, 0, 1, 9)], lay["segs"], nf, self.P(lay["bias"]), y, out_relu=True)
        y.bias_offs = [lay["bias"]]                          # the single consumer writes y's whole (masked) gradient: it may take the bias gradient on the way
        if tr:
            def back():
                Bp = self.bwd
                dy = y.grad
                assert not (y.masked_w and y.plain_w), "mixed masked / unmasked writers of a ReLU output's gradient"
                if y.plain_w:
                    assert not y.bias_done
                    Bp.add("rua_relu_mask", dy.ptr, y.ptr, y.t.numel(), self.dt)
                if not y.bias_done:
                    self.bias_grad(Bp, dy, [lay["bias"]])
                self.wq.one(Bp, WSpec(x, dy, lay["segs"][0]["off"], 1, 1, 9))
                gx, acc = self.gacc(x, masked=x.relu_out)
                sx = None
                if x.bias_offs and x.relu_out and not acc and not self.dry and self.e.bn_dx_bias:
                    # x is the ReLU'ed output of a conv with a bias and this data gradient its only consumer: the epilogue's per-channel sums of the
                    # masked gradient are that bias gradient (no rua_col_stats pass)
                    sx = self.stat(x.C, (x.M + 127) // 128)
                self.dgrad(Bp, dy, self.Wd(lay["segs"][0]["dst"]), x.C, 1, 9, gx, acc, mask=(x, None, None) if x.relu_out else None, stats2=sx)
                if sx is not None:
                    self.stats_to_grads(Bp, sx, x.C, x.bias_offs)
                    x.bias_done = True
            self.back_steps.append(back)
        return y

    def head(self, x: Ten, cout: int, act: int, hname: str, name=None, lay=None):
        """Conv2D(C,(1,1)) + softmax/sigmoid, its loss and the gradient w.r.t. the logits."""
        F, tr = self.fwd, self.training
        lay = lay if lay is not None else self.Lconv([x.C], cout, 1, name=name, mfma=False)
        z = self.new(x.N, x.H, x.W, cout, f32=True)
        p = self.new(x.N, x.H, x.W, cout, f32=True)
        y = self.new(x.N, x.H, x.W, cout, f32=True)           # label buffer (host uploads into it)
        h = dict(name=hname, x=x, z=z, p=p, y=y, lay=lay, act=act, C=cout, slot=len(self.heads))
        sp = self.e.loss
        tani = sp is not None and sp.kind.get(hname) == L.LOSS_TANIMOTO
        if sp is not None and not self.dry and self.e.fuse_head_loss and (tani or hname == "seg"):
            # the Tanimoto moments (and the 'seg' head's accuracy / confusion counts) in the head's own epilogue: p is not read again
            if tani:
                # SUMS_REPLICAS copies of sums[B][C][6] (+ the slot rua_tanimoto_finalize_rep folds them into): a block of the head's forward adds
                # into one copy, so the ~64 blocks of a sample do not queue up on the same 36 fp64 addresses at the end of the launch
                h["sums_rep"] = SUMS_REPLICAS
                h["sums"] = self.salloc((SUMS_REPLICAS + 1) * x.N * cout * 6)
            if hname == "seg":
                h["metrics_done"] = True
            head_args = (x.ptr, self.P(lay["segs"][0]["off"]), self.P(lay["bias"]), z.ptr, p.ptr, y.ptr, h.get("sums"),
                         h.get("sums_rep", 1), self.e.scalars_ptr + 8 * 8 if hname == "seg" else None, x.N, x.H * x.W, x.C, cout, act, self.dt)
            if self.void_ptr is not None:
                F.add("rua_head_fwd_loss_void", *head_args, self.void_ptr)
            else:
                F.add("rua_head_fwd_loss_rep", *head_args)
        else:
            F.add("rua_head_fwd", x.ptr, self.P(lay["segs"][0]["off"]), self.P(lay["bias"]), z.ptr, p.ptr, x.M, x.C, cout, act, self.dt)
        self.heads.append(h)
        return h

    def heads_grouped(self, x_psp: Ten, x_comb: Ten, w0: int, Cc: int):
        """The multitask heads (model2.py:148-191) with their five 3x3 + ReLU convolutions issued as GROUPS across the heads - forward {seg1, bound1,
        dist1} and {seg2, dist2}, backward the weight gradients and the data gradients of {seg2, bound1, dist2}, then of {seg1, dist1} - instead of
        one launch per convolution: members on the same kernel form share one grid of persistent blocks (conv_strip32s_g / wgrad_rows32_g), which
        runs a 9.66 GFLOP member in ~14 us where a launch of its own takes 17 - 22.  Layers are created in the order of the head-by-head path
        (parameter layout and Keras names unchanged); same kernels, same arithmetic per convolution."""
        F, tr = self.fwd, self.training
        lay = {}
        lay["seg1"] = self.Lconv([x_psp.C], w0, 9, name="seg1"); lay["seg2"] = self.Lconv([w0], w0, 9, name="seg2")
        lay["seg3"] = self.Lconv([w0], Cc, 1, name="seg3", mfma=False)
        lay["bound1"] = self.Lconv([x_psp.C], w0, 9); lay["bound3"] = self.Lconv([w0], Cc, 1, mfma=False)
        lay["dist1"] = self.Lconv([x_comb.C], w0, 9); lay["dist2"] = self.Lconv([w0], w0, 9); lay["dist3"] = self.Lconv([w0], Cc, 1, mfma=False)
        lay["color"] = self.Lconv([x_comb.C], 3, 1, name="color", mfma=False)

        def out_of(x: Ten, ly) -> Ten:
            y = self.new(x.N, x.H, x.W, w0)
            y.relu_out = True
            y.bias_offs = [ly["bias"]]
            return y

        def fdesc(x: Ten, ly, y: Ten):
            return self.conv_desc([(x, 0, 1, 9)], ly["segs"], w0, self.P(ly["bias"]), y, out_relu=True)
        s1, b1, d1 = out_of(x_psp, lay["seg1"]), out_of(x_psp, lay["bound1"]), out_of(x_comb, lay["dist1"])
        self.cur_tag = F.scope = "heads_conv"
        self.conv_group(F, [fdesc(x_psp, lay["seg1"], s1), fdesc(x_psp, lay["bound1"], b1), fdesc(x_comb, lay["dist1"], d1)])
        s2, d2 = out_of(s1, lay["seg2"]), out_of(d1, lay["dist2"])
        self.conv_group(F, [fdesc(s1, lay["seg2"], s2), fdesc(d1, lay["dist2"], d2)])
        self.cur_tag = F.scope = None
        if tr:
            def phase(convs, carried=(), later=False):      # [(x, y, layer)]: weight gradients, then data gradients, of independent convolutions
                Bp = self.bwd
                for x, y, ly in convs:
                    assert not (y.masked_w and y.plain_w), "mixed masked / unmasked writers of a ReLU output's gradient"
                    if y.plain_w:
                        assert not y.bias_done
                        Bp.add("rua_relu_mask", y.grad.ptr, y.ptr, y.t.numel(), self.dt)
                    if not y.bias_done:
                        self.bias_grad(Bp, y.grad, [ly["bias"]])
                wg = list(carried) + [WSpec(x, y.grad, ly["segs"][0]["off"], 1, 1, 9) for x, y, ly in convs]
                if not later:                               # (later: these ride in the next phase's group - as the two groups of a ResBlock do, WgradQueue.now_or_later)
                    self.wq.group(Bp, wg)
                descs, sums = [], []
                for x, y, ly in convs:
                    gx, acc = self.gacc(x, masked=x.relu_out)
                    sx = None
                    if x.bias_offs and x.relu_out and not acc and not self.dry and self.e.bn_dx_bias:
                        sx = self.stat(x.C, (x.M + 127) // 128)     # the epilogue's sums of the masked gradient = the bias gradient of the conv behind x
                        sums.append((sx, x))
                    descs.append(self.dgrad_desc(y.grad, self.Wd(ly["segs"][0]["dst"]), x.C, 1, 9, gx, acc, mask=(x, None, None) if x.relu_out else None, stats2=sx))
                self.conv_group(Bp, descs)
                for sx, x in sums:
                    self.stats_to_grads(Bp, sx, x.C, x.bias_offs)
                    x.bias_done = True
                return wg if later else []

            def back():
                Bp = self.bwd
                Bp.scope = "heads_conv"
                merge = (not self.dry) and 1 in self.e.merge_wgrad            # (1: the heads)
                wg = phase([(s1, s2, lay["seg2"]), (x_psp, b1, lay["bound1"]), (d1, d2, lay["dist2"])], later=merge)
                phase([(x_psp, s1, lay["seg1"]), (x_comb, d1, lay["dist1"])], carried=wg)
                Bp.scope = None
            self.back_steps.append(back)
        self.tagged("head_seg", self.head, s2, Cc, L.ACT_SOFTMAX, "seg", "seg3", lay["seg3"])
        self.tagged("head_bound", self.head, b1, Cc, L.ACT_SIGMOID, "bound", None, lay["bound3"])
        self.tagged("head_dist", self.head, d2, Cc, L.ACT_SOFTMAX, "dist", None, lay["dist3"])
        self.tagged("head_color", self.head, x_comb, 3, L.ACT_SIGMOID, "color", "color", lay["color"])

    def head_loss(self, h):
        """Loss value (fp64 scalar slot) and, in training, d(total)/d(logits) -> head weights and x.grad."""
        sp, LP = self.e.loss, self.loss_plan
        kind, wgt = sp.kind[h["name"]], sp.weight[h["name"]]
        B, HW, Cc = self.B, h["x"].H * h["x"].W, h["C"]
        M = B * HW
        slot = self.e.scalars_ptr + h["slot"] * 8
        coef = None
        opts = sp.head_opts(h["name"])
        if kind == L.LOSS_TANIMOTO:
            coef = self.alloc((B * Cc * 3,), torch.float32, zero=True)
            LP.keep.append(coef)
            sums = h.get("sums")
            if sums is None:                                # (the head's forward did not take the moments itself)
                sums = self.salloc(B * Cc * 6)
                if self.void_ptr is not None:
                    LP.add("rua_tanimoto_sums_void", h["p"].ptr, h["y"].ptr, self.void_ptr, B, HW, Cc, sums)
                else:
                    LP.add("rua_tanimoto_sums", h["p"].ptr, h["y"].ptr, B, HW, Cc, sums)
            if self.multi_head:                             # one launch for all heads (_record_losses)
                th = L.TaniHead()
                th.sums, th.replicas, th.B, th.C, th.grad_scale, th.loss_out, th.coef, th.per_sample = sums, h.get("sums_rep", 1), B, Cc, wgt / B, slot, coef.data_ptr(), None
                self._tani_multi.append(th)
            else:
                LP.add("rua_tanimoto_finalize_rep", sums, h.get("sums_rep", 1), B, HW, Cc, wgt / B, slot, coef.data_ptr(), None)
            h["norm"] = 1.0
        elif kind == L.LOSS_LOVASZ:
            # the Lovasz extension of the Jaccard index: rua_lovasz_grad sorts every class's pixels by their error on the device, adds
            # weight * loss into the head's slot and leaves d(loss)/d(p) and the normaliser in device memory (training; evaluation takes the
            # value only).  Nothing is read back: a replay needs no host scalar
            lo = sp.head_lovasz(h["name"])
            nws = int(L.lib().raw("rua_lovasz_workspace_bytes")(M, Cc))
            if nws < 0:
                raise ValueError(f"{h['name']}: {M} pixels x {Cc} classes is out of the Lovasz kernels' range")
            res, ws = self.alloc((C.sizeof(L.LovaszResult) // 8,), torch.float64, zero=True), self.alloc((nws // 8 + 1,), torch.float64)
            dp = self.alloc((M * Cc,), torch.float32) if self.training else None
            LP.keep += [res, ws]
            LP.add("rua_lovasz_grad", h["p"].ptr, h["y"].ptr, self.void_ptr, M, Cc, 1 if lo["classes"] == "all" else 0, wgt, ws.data_ptr(), nws, slot,
                   dp.data_ptr() if dp is not None else None, None, res.data_ptr())
            w32 = float(np.float32(wgt))                  # the slot holds float32(weight) * loss: the norm takes the weight out again (1.0 exactly for a unit weight)
            h["norm"] = 1.0 / w32 if w32 != 0 else 1.0
            h["lovasz"] = dict(result=res, dp=dp, opts=lo)
        else:
            # online hard example mining (training plans only: evaluation reports the plain mean): the loss entry leaves the per-pixel map - its own sum
            # goes to a scratch slot nobody reads -, rua_ohem_select turns the map into the head's drop mask, its normaliser and the kept mean, which it
            # adds into the head's slot.  Everything stays on the device: a replay needs no host scalar
            oh = sp.head_ohem(h["name"]) if self.training else None
            pp, lslot = None, slot
            if oh is not None:
                pp = self.alloc((M,), torch.float32)
                lslot = self.salloc(1)
            if opts is not None:                            # a focal kind or label smoothing: the entry with options (mask optional)
                LP.keep.append(opts)
                LP.add("rua_pixel_loss_opts", kind, h["p"].ptr, h["z"].ptr, h["y"].ptr, self.e.class_w_ptr, self.void_ptr, C.byref(opts), M, Cc, lslot,
                       pp.data_ptr() if pp is not None else None)
            elif self.void_ptr is not None:                 # the sum over the valid pixels, still divided by M (Keras' sample_weight rule with 0 / 1 weights)
                LP.add("rua_pixel_loss_void", kind, h["p"].ptr, h["z"].ptr, h["y"].ptr, self.e.class_w_ptr, self.void_ptr, M, Cc, lslot,
                       pp.data_ptr() if pp is not None else None)
            else:
                LP.add("rua_pixel_loss", kind, h["p"].ptr, h["z"].ptr, h["y"].ptr, self.e.class_w_ptr, M, Cc, lslot, pp.data_ptr() if pp is not None else None)
            h["norm"] = 1.0 / M
            if oh is not None:
                nws = int(L.lib().raw("rua_ohem_workspace_bytes")(M))
                drop, res, ws = self.alloc((M,), torch.uint8), self.alloc((C.sizeof(L.OhemResult) // 8,), torch.float64, zero=True), self.alloc((nws // 8 + 1,), torch.float64)
                oo = LS.to_ohem_struct(oh)
                LP.keep.append(oo)
                LP.add("rua_ohem_select", pp.data_ptr(), self.void_ptr, M, C.byref(oo), self.e.lr_state.data_ptr() if oo.warmup > 0 else None, wgt,
                       ws.data_ptr(), nws, drop.data_ptr(), slot, res.data_ptr())
                h["norm"] = 1.0
                h["ohem"] = dict(per_pixel=pp, drop_mask=drop, result=res, opts=oh)
        if not self.training:
            return
        sel = h.get("ohem")
        lov = h.get("lovasz")

        dz = self.new(B, h["x"].H, h["x"].W, Cc, f32=True)
        h["dz"] = dz
        gs = wgt / B if kind == L.LOSS_TANIMOTO else wgt / M
        scale_ptr = sel["result"].data_ptr() + L.OhemResult.scale.offset if sel is not None else None
        if self.multi_head and lov is None:             # (a Lovasz head stays out of the heads' single launch: it has its own, below)
            dh = L.DzHead()
            dh.kind, dh.act, dh.p, dh.y, dh.coef, dh.class_w = kind, h["act"], h["p"].ptr, h["y"].ptr, coef.data_ptr() if coef is not None else None, self.e.class_w_ptr
            dh.grad_scale, dh.B, dh.HW, dh.C, dh.dz = gs, B, HW, Cc, dz.ptr
            self._dz_multi.append(dh)
            self._dz_multi_opts.append(opts)
            ds = L.DzSel()                                  # zeroed: the head takes no selection
            if sel is not None:
                ds.drop_mask, ds.scale_dev = sel["drop_mask"].data_ptr(), scale_ptr
            self._dz_multi_sel.append(ds)

        def back():
            Bp = self.bwd
            if lov is not None:
                Bp.add("rua_lovasz_dz", h["act"], h["p"].ptr, lov["dp"].data_ptr(), lov["result"].data_ptr() + L.LovaszResult.scale.offset, M, Cc, dz.ptr)
            if self.multi_head:
                if not self._dz_emitted and self._dz_multi:                    # the first backward step of the loss section: d(loss)/d(logits) of ALL heads in one launch
                    arr = (L.DzHead * len(self._dz_multi))(*self._dz_multi)
                    Bp.keep.append(arr)
                    if any(d.drop_mask for d in self._dz_multi_sel):         # a mining head: still one launch, its mask and normaliser read on the device
                        oarr = (L.LossOpts * len(self._dz_multi))(*[o if o is not None else L.LossOpts() for o in self._dz_multi_opts])
                        sarr = (L.DzSel * len(self._dz_multi))(*self._dz_multi_sel)
                        Bp.keep += [oarr, sarr]
                        Bp.add("rua_head_dz_multi_sel", arr, oarr, sarr, len(self._dz_multi), self.void_ptr)
                    elif any(o is not None for o in self._dz_multi_opts):      # still one launch: every head with its options, zeroed where it has none
                        oarr = (L.LossOpts * len(self._dz_multi))(*[o if o is not None else L.LossOpts() for o in self._dz_multi_opts])
                        Bp.keep.append(oarr)
                        Bp.add("rua_head_dz_multi_opts", arr, oarr, len(self._dz_multi), self.void_ptr)
                    elif self.void_ptr is not None:
                        Bp.add("rua_head_dz_multi_void", arr, len(self._dz_multi), self.void_ptr)
                    else:
                        Bp.add("rua_head_dz_multi", arr, len(self._dz_multi))
                    self._dz_emitted = True
            elif lov is not None:
                pass
            elif sel is not None:
                o = opts if opts is not None else L.LossOpts()
                Bp.keep.append(o)
                Bp.add("rua_head_dz_sel", kind, h["act"], h["p"].ptr, h["y"].ptr, coef.data_ptr() if coef is not None else None,
                       self.e.class_w_ptr, B, HW, Cc, C.byref(o), sel["drop_mask"].data_ptr(), scale_ptr, dz.ptr)
            elif opts is not None:
                Bp.keep.append(opts)
                Bp.add("rua_head_dz_opts", kind, h["act"], h["p"].ptr, h["y"].ptr, coef.data_ptr() if coef is not None else None,
                       self.e.class_w_ptr, gs, B, HW, Cc, self.void_ptr, C.byref(opts), dz.ptr)
            elif self.void_ptr is not None:
                Bp.add("rua_head_dz_void", kind, h["act"], h["p"].ptr, h["y"].ptr, coef.data_ptr() if coef is not None else None,
                       self.e.class_w_ptr, gs, B, HW, Cc, self.void_ptr, dz.ptr)
            else:
                Bp.add("rua_head_dz", kind, h["act"], h["p"].ptr, h["y"].ptr, coef.data_ptr() if coef is not None else None,
                       self.e.class_w_ptr, gs, B, HW, Cc, dz.ptr)
            hx = h["x"]
            gx, acc = self.gacc(hx, masked=hx.relu_out)
            lay = h["lay"]
            dxsum, grads = None, [lay["segs"][0]["off"], lay["bias"]]
            if hx.bias_offs and hx.relu_out and not acc and not self.dry and self.e.bn_dx_bias:
                dxsum = self.G(hx.bias_offs[0])            # the head's backward sums the masked gradient it writes: the bias gradient of the conv behind hx
                grads.append(hx.bias_offs[0])
                hx.bias_done = True
            Bp.add("rua_head_bwd_sums", hx.ptr, dz.ptr, self.P(lay["segs"][0]["off"]), gx.ptr, acc, self.G(lay["segs"][0]["off"]),
                   self.G(lay["bias"]), dxsum, self.e.scratch.data_ptr(), self.e.scratch.numel() * 4, M, hx.C, Cc, self.dt,
                   1 if hx.relu_out else 0, grads=grads)
        self.back_steps.append(back)

    # -- whole network ---------------------------------------------------------------------------------
    def tagged(self, tag: str, fn, *args):
        """Record fn(*args) - forward launches now, its backward closures later - under the composite name `tag`."""
        self.cur_tag = tag
        prev, self.fwd.scope = self.fwd.scope, tag
        out = fn(*args)
        self.fwd.scope = prev
        self.cur_tag = None
        return out

    def _build(self):
        cfg, F, tr = self.cfg, self.fwd, self.training
        if cfg.variant not in ("model2", "model"):
            raise ValueError(f"unknown graph variant {cfg.variant!r} (model2 = ResUnet_a/model2.py, model = ResUnet_a/model.py)")
        v2 = cfg.variant == "model2"
        H, W, Cin = cfg.input_shape
        lv = cfg.levels()
        w0 = lv[0][0]
        self.heads: List[dict] = []
        self.x_in = self.new(self.B, H, W, Cin, f32=True)
        stem = self.Lconv([Cin], w0, 1, mfma=False)
        c1 = self.new(self.B, H, W, w0)
        self.cur_tag, F.scope = "stem", "stem"
        # bf16 storage, <= 7 bands: the stem's weight gradient on the matrix pipe - the forward also writes the input as bf16 hi | lo | 1 (xpack), the backward is
        # the 1x1 weight gradient of dy against it + rua_stem_bwd_fold (include/rua_hip.h)
        pack = tr and not self.dry and self.e.stem_mfma and self.e.dtype == "bf16" and Cin <= 7 and w0 % 16 == 0 and c1.M >= 2048
        xpack = self.new(self.B, H, W, 16) if pack else None
        if tr and getattr(self.e, "stem_stats", True):
            # the statistics the first BatchNorm of the encoder needs, from the kernel that writes the tensor (no rua_col_stats pass over it)
            c1.stats = self.stat(w0, 2 * 256, burst=True)
        if pack:
            st = getattr(c1, "stats", None)
            F.add("rua_stem_fwd_pack", self.x_in.ptr, self.P(stem["segs"][0]["off"]), self.P(stem["bias"]), c1.ptr, c1.M, Cin, w0, self.dt,
                  st.ptr if st is not None else None, st.R if st is not None else 1, xpack.ptr)
        elif tr and getattr(self.e, "stem_stats", True):
            F.add("rua_stem_fwd_stats", self.x_in.ptr, self.P(stem["segs"][0]["off"]), self.P(stem["bias"]), c1.ptr, c1.M, Cin, w0, self.dt, c1.stats.ptr, c1.stats.R)
        else:
            F.add("rua_stem_fwd", self.x_in.ptr, self.P(stem["segs"][0]["off"]), self.P(stem["bias"]), c1.ptr, c1.M, Cin, w0, self.dt)
        if tr:
            def stem_back():
                Bp = self.bwd
                if pack:
                    tmp = self.alloc((w0 * 16,), torch.float32, zero=True)          # [Cout][16]: zero before every launch (the fold leaves it so)
                    d = self.wq.desc(WSpec(xpack, c1.grad, stem["segs"][0]["off"], 1, 1, 1))      # never deferred: the fold reads tmp right behind the call: its partials are summed by the call itself
                    d.dw, d.grads = tmp.data_ptr(), ()
                    self.issue(Bp, [d], "rua_conv_wgrad")
                    Bp.add("rua_stem_bwd_fold", tmp.data_ptr(), self.G(stem["segs"][0]["off"]), self.G(stem["bias"]), Cin, w0,
                           grads=(stem["segs"][0]["off"], stem["bias"]))
                else:
                    Bp.add("rua_stem_bwd", self.x_in.ptr, c1.grad.ptr, self.G(stem["segs"][0]["off"]), self.G(stem["bias"]),
                           c1.M, Cin, w0, self.dt, grads=(stem["segs"][0]["off"], stem["bias"]))
            self.back_steps.append(stem_back)
        self.cur_tag, F.scope = None, None
        x = c1
        skips = []
        for i, (nf, dils) in enumerate(lv):
            if i > 0:
                x = self.tagged(f"down{i + 1}", self.down, x, nf)
            self.block_tag = f"enc{i + 1}"
            x = self.resblock(x, nf, dils)
            skips.append(x)
        x = self.tagged("psp_mid", self.psp if v2 else self.psp_v1, x, lv[-1][0])
        for i in range(len(lv) - 2, -1, -1):
            nf, dils = lv[i]
            x = self.tagged(f"up{i + 1}", self.up_combine if v2 else self.up_combine_v1, x, skips[i], nf)
            self.block_tag = f"dec{i + 1}"
            x = self.resblock(x, nf, dils)
        x_comb = self.tagged("combine_top", self.final_combine, x, c1, w0) if v2 else self.tagged("combine_top", self.relu_cat_conv_v1, x, 0, c1, w0, False)
        x_psp = self.tagged("psp_top", self.psp if v2 else self.psp_v1, x_comb, w0)
        Cc = cfg.num_classes
        if not cfg.multitasking:
            self.tagged("head_seg", self.head, x_psp, Cc, L.ACT_SOFTMAX, "seg")
        elif not self.dry and self.e.group_heads and self.e.dtype == "bf16":
            self.heads_grouped(x_psp, x_comb, w0, Cc)
        else:
            def seg_head():
                s = self.conv3x3_relu(x_psp, w0, "seg1")
                s = self.conv3x3_relu(s, w0, "seg2")
                self.head(s, Cc, L.ACT_SOFTMAX, "seg", "seg3")

            def dist_head():
                d = self.conv3x3_relu(x_comb, w0)
                d = self.conv3x3_relu(d, w0)
                self.head(d, Cc, L.ACT_SOFTMAX, "dist")
            self.tagged("head_seg", seg_head)
            self.tagged("head_bound", lambda: self.head(self.conv3x3_relu(x_psp, w0), Cc, L.ACT_SIGMOID, "bound"))
            self.tagged("head_dist", dist_head)
            self.tagged("head_color", self.head, x_comb, 3, L.ACT_SIGMOID, "color", "color")
        self.outputs = {h["name"]: h for h in self.heads}
        if self.e.loss is not None and not self.dry:
            self._record_losses()

    def _record_losses(self):
        """Loss / metric launches and (training) the whole backward plan, in reverse creation order."""
        # multitask: the heads' Tanimoto finalisations and their d(loss)/d(logits) as one launch each (rua_tanimoto_finalize_multi, rua_head_dz_multi)
        self.multi_head = len(self.heads) > 1 and self.e.multi_head
        self._tani_multi, self._dz_multi, self._dz_multi_opts, self._dz_multi_sel, self._dz_emitted = [], [], [], [], False
        for h in self.heads:
            self.cur_tag = self.loss_plan.scope = "loss_" + h["name"]
            self.head_loss(h)
        if self._tani_multi:
            self.loss_plan.scope = "loss_finalize"
            arr = (L.TaniHead * len(self._tani_multi))(*self._tani_multi)
            self.loss_plan.keep.append(arr)
            self.loss_plan.add("rua_tanimoto_finalize_multi", arr, len(self._tani_multi))
        self.cur_tag = self.loss_plan.scope = None
        seg = self.outputs["seg"]
        if not seg.get("metrics_done"):
            if self.void_ptr is not None:
                self.loss_plan.add("rua_seg_metrics_void", seg["p"].ptr, seg["y"].ptr, self.void_ptr, seg["x"].M, seg["C"], self.e.scalars_ptr + 8 * 8)
            else:
                self.loss_plan.add("rua_seg_metrics", seg["p"].ptr, seg["y"].ptr, seg["x"].M, seg["C"], self.e.scalars_ptr + 8 * 8)
        if self.training:
            for step in reversed(self.back_steps):
                step()
            self.back_steps = []
            self.wq.flush()


# ---------------------------------------------------------------------------------------
class Engine:
    """Owns parameters, optimizer state and the recorded graphs; one instance per process (= per GPU)."""

    def __init__(self, cfg: ModelConfig, dtype: str = "bf16", device: Optional[torch.device] = None, seed: int = 0,
                 split_k: bool = True, _layout_only: bool = False):
        assert dtype in ("bf16", "f32")
        self.cfg = cfg
        self.dt = L.RUA_BF16 if dtype == "bf16" else L.RUA_F32
        self.dtype = dtype
        self.esize = 2 if dtype == "bf16" else 4
        if cfg.width % 32 != 0:
            raise ValueError(f"width={cfg.width}: the first-stage width must be a multiple of 32 (PSP branches are width/4 "
                             "channels and the MFMA epilogue stores 8-channel pieces)")
        self.dev = None
        self.fuse_bn = os.environ.get("RUA_FUSE_BN", "1") != "0"     # normalise-on-load ResBlocks where the library offers it
        self.fuse_head_loss = os.environ.get("RUA_FUSE_HEAD_LOSS", "1") != "0"   # Tanimoto moments / seg metrics in the heads' forward epilogue
        self.bn_out_stats = os.environ.get("RUA_BN_OUT_STATS", "1") != "0"       # statistics of a ReLU-less BatchNorm's output from its coefficients
        self.bn_dx_bias = os.environ.get("RUA_BN_DX_BIAS", "1") != "0"           # bias gradients of the stride-2 convs from the sums of the BatchNorm backward that writes their output's gradient
        self.pool_pyramid = os.environ.get("RUA_POOL_PYRAMID", "1") != "0"   # PSPPooling: the 2 / 4 / 8 poolings (and their adjoints) in single passes
        self.fold_bn = os.environ.get("RUA_FOLD_BN", "1") != "0"     # ... and their coefficient launches folded into the convs' prologues
        self.defer_reduce = os.environ.get("RUA_DEFER_REDUCE", "1") != "0"     # weight-gradient partials summed by batched launches
        # ... flushed whenever more than this many bytes of partials are pending: the K-slice slabs of levels 3 - 5 are then still in the 256 MB
        # Infinity Cache when the reduction reads them (one reduction at the end of the backward read all 0.6 GB from HBM)
        self.flush_bytes = int(float(os.environ.get("RUA_FLUSH_MB", "1e9")) * (1 << 20))
        self.cu_count = 256
        self.split_k = split_k       # False: bit-reproducible convolutions (no fp32-atomic K slices); parity tests on tiny
                                     # inputs use it because a BatchNorm over 2 samples amplifies atomic-order noise ~1e4x
        self.params = ParamStore()
        self.layers: List[dict] = []
        self.cursor = 0
        self.built = False
        self.loss: Optional[LossSpec] = None
        self.clip: Optional[dict] = None                    # device tables of clip.py's options (_setup_clip); None: every option off
        self._s_backed = False
        self.E: Optional[torch.Tensor] = None               # use_ema: the moving average of P (fp32, P's layout), allocated by compile()
        self._sched = None                                  # lr_schedule: the rua_lr_schedule the rate kernel takes by value
        self._in_ema = False                                # inside ema_weights(): P and E have swapped contents
        self.A: Optional[torch.Tensor] = None               # gradient_accumulation_steps: the accumulator (fp32, P's layout), allocated by compile()
        self.acc_state: Optional[torch.Tensor] = None       # ... int32 [0] gradients of the current cycle in A, [1] this step's hold flag (rua_accum_gate)
        self.micro, self._micro_dev = 0, -1                 # ... the host's mirror of acc_state[0] and what the device copy holds (as t / _t_dev)
        self.graphs: Dict[Tuple[int, bool], Graph] = {}
        self.class_w_ptr = None
        self.scalars_ptr = 0
        Graph(self, 1, True, dry=True)                      # enumerate layers / parameters (no device needed)
        self.built = True
        ps = self.params
        if _layout_only:
            return
        L.lib()                                             # raises if librua_hip.so is missing
        if not torch.cuda.is_available():
            raise L.RuaError("no HIP device visible: the ResUnet-a training path runs on MI355X only (there is no CPU fallback)")
        self.dev = device or torch.device("cuda", torch.cuda.current_device())
        cu = C.c_int32(0)
        if L.lib().raw("rua_device_info")(C.byref(cu), None, None, 0) == 0 and cu.value > 0:
            self.cu_count = cu.value
        z = lambda n, dt=torch.float32: torch.zeros(max(n, 16), dtype=dt, device=self.dev)
        self.P, self.G, self.M1, self.V1, self.S = z(ps.n), z(ps.n + ps.ns + 16), z(ps.n), z(ps.n), z(ps.ns)      # G: room behind the last gradient for the BatchNorm state's ride in the first all-reduce bucket (dist.py)
        tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
        self.Wf, self.Wd = z(ps.n, tdt), z(ps.n, tdt)
        # first-writer overwrite of the gradient arena: in a whole step every weight gradient has ONE producer and the optimizer left the arena zero, so the kernels
        # that end in a read-modify-write of dW store instead (a device flag, include/rua_hip.h: forward_backward() called on its own still ACCUMULATES)
        self.wgrad_overwrite = os.environ.get("RUA_WGRAD_OVERWRITE", "1") != "0"
        self.ow_flag = torch.zeros(4, dtype=torch.int32, device=self.dev)
        self._ow = 0
        self._g_pending = False                             # G holds gradients no optimizer step has consumed (forward_backward() on its own)
        self.opt_wcopy = dtype == "bf16" and os.environ.get("RUA_OPT_WCOPY", "1") != "0"   # the optimizer writes the forward-layout bf16 copy itself
        self.wf_fresh = False                               # the forward copy holds bf16(P): written by the optimizer (or a full rua_weight_prep) since P last changed
        items = np.zeros(0, dtype=[("src", "<i8"), ("dst", "<i8"), ("taps", "<i4"), ("cout", "<i4"), ("c", "<i4"), ("pad", "<i4")])
        rows, mx = [], 1
        for lay in self.layers:
            if "segs" in lay and lay["mfma"]:
                for sg in lay["segs"]:
                    rows.append((sg["off"], sg["dst"], lay["taps"], lay["cout"], sg["C"], 0))
                    mx = max(mx, lay["taps"] * lay["cout"] * sg["C"])
        items = np.array(rows, dtype=items.dtype)
        self.wprep_items = torch.from_numpy(np.frombuffer(items.tobytes(), dtype=np.uint8).copy()).to(self.dev)
        self.wprep_n, self.wprep_max = len(rows), mx
        bm = []                                              # block map of rua_weight_prep_dgrad: (item, first tile) per block
        for i, (_, _, taps, cout, ci, _) in enumerate(rows):
            for b in range(L.lib().raw("rua_wprep_blocks")(taps, cout, ci)):
                bm += [i, 8 * b]
        self.wprep_map = torch.tensor(bm if bm else [0, 0], dtype=torch.int32, device=self.dev)
        self.wprep_map_n = len(bm) // 2
        self.stats_arena = torch.zeros(1 << 22, dtype=torch.float64, device=self.dev)
        # the split-K slab workspace of the convolutions and the weight gradients' partial scratch: launches are serialised on one stream, so
        # one of each serves every launch (the scratch has room for the fp32 K-slice slabs of the deterministic weight gradients: 128 MB)
        self.workspace = torch.zeros(8 << 20, dtype=torch.float32, device=self.dev)
        self.scratch = torch.zeros(32 << 20, dtype=torch.float32, device=self.dev)
        self.lr_dev = torch.zeros(16, dtype=torch.float32, device=self.dev)               # step-dependent optimizer scalars
        self.lr_state = torch.zeros(2, dtype=torch.float64, device=self.dev)              # [steps taken, base learning rate]
        self._t_dev, self._lr_base_dev = -1, None                                         # what lr_state holds (host shadow)
        self._dp_fence = torch.zeros(16, dtype=torch.float32, device=self.dev)            # see _graph_step_dp
        self.use_graph = os.environ.get("RUA_USE_GRAPH", "1") != "0"                      # 0 (experiments): the single-GPU step as eager launches too
        self.group_1x1 = os.environ.get("RUA_GROUP_1X1", "1") != "0"       # PSPPooling's branch convolutions and the per-source gradients of concatenating 1x1 convolutions as groups
        self.group_heads = os.environ.get("RUA_GROUP_HEADS", "1") != "0"   # the heads' 3x3 convolutions (and their gradients) grouped across the heads
        self.multi_head = os.environ.get("RUA_MULTI_HEAD", "1") != "0"     # the heads' loss finalisation / d(loss)/d(logits) as one launch each
        self.merge_wgrad = {int(v) for v in os.environ.get("RUA_MERGE_WGRAD", "1,32,64,128,256").split(",") if v}     # channel counts whose ResBlocks issue both weight-gradient groups as one (WgradQueue.now_or_later)
        self.group_wgrad_pw = os.environ.get("RUA_GROUP_WGRAD_PW", "1") != "0"   # the narrow 1x1 weight gradients of a composite as one grid (WgradQueue.pw_group)
        self.batch_wgrad = os.environ.get("RUA_BATCH_WGRAD", "1") != "0"         # bf16: a step's generic-tile weight gradients as one batched launch in front of each flush (WgradQueue.hold_back)
        self.stem_mfma = os.environ.get("RUA_STEM_MFMA", "1") != "0"       # bf16: the stem's weight gradient through rua_stem_fwd_pack / rua_conv_wgrad / rua_stem_bwd_fold
        self.stem_stats = os.environ.get("RUA_STEM_STATS", "1") != "0"     # rua_stem_fwd_stats instead of a rua_col_stats pass over the stem's output
        self._captured: Dict[int, object] = {}
        self._captured_eval: Dict[int, object] = {}        # batch -> graph of the inference forward (False: capture failed)
        self._eval_seen = set()
        self._captured_dp: Dict[int, list] = {}
        # Data-parallel step: eager launches by default (2.4 ms of host time per 10.4 ms step; measured as fast as the
        # HIP-graph pieces and immune to the graph-launch / stream-event hazard described in _graph_step_dp); RUA_DP_GRAPH=1
        # selects the pieces.
        self.dp_graph = os.environ.get("RUA_DP_GRAPH", "0") == "1"
        self.dp_fence = os.environ.get("RUA_DP_FENCE", "0") == "1"      # experiments only (tools/dp_graph_check.py): an eager kernel behind every piece replay
        self.scalars_ptr = self.stats_arena.data_ptr()
        self.t = 0
        self.weights_dirty = True
        self.world = 1
        self.dist = None
        P, S = ps.init_host(seed)
        self.P.copy_(torch.from_numpy(P)); self.S.copy_(torch.from_numpy(S))

    @classmethod
    def param_layout(cls, cfg: ModelConfig, dtype: str = "f32") -> ParamStore:
        """Parameter table (names, shapes, flat offsets) without touching a device."""
        return cls(cfg, dtype, _layout_only=True).params

    # -- layer registry ------------------------------------------------------------------------------
    def layer(self, kind, *args):
        if not self.built:
            rec = self.params.conv(*args) if kind == "conv" else self.params.bn(*args)
            self.layers.append(rec)
            return rec
        rec = self.layers[self.cursor]
        self.cursor += 1
        return rec

    def graph(self, batch: int, training: bool) -> Graph:
        key = (batch, training)
        if key not in self.graphs:
            assert self.loss is not None, "compile() first"
            self.cursor = 0
            self.graphs[key] = Graph(self, batch, training)
            assert self.cursor == len(self.layers)
        return self.graphs[key]

    def compile(self, spec: LossSpec):
        if self.dev is not None and (self.graphs or self._captured or self._captured_eval or self._captured_dp):
            # a re-compile (Keras fine-tune pattern, or predict()'s auto-compile followed by compile): the captured HIP graphs
            # hold raw pointers into the old plan's buffers and bake in the old loss / optimizer - drop them with the plan
            torch.cuda.synchronize()
        self._captured, self._captured_eval, self._captured_dp = {}, {}, {}
        self._eval_seen = set()
        self._opt_graph = None
        iv = spec.ignore_void
        if iv is not None and (isinstance(iv, bool) or not isinstance(iv, (int, np.integer)) or not 0 <= iv <= 16):
            raise ValueError(f"ignore_void {iv!r}: None (off) or a margin in 0..16")
        CL.check_options(spec.clipnorm, spec.global_clipnorm, spec.clipvalue, spec.weight_decay)
        SC.check_ema_options(spec.use_ema, spec.ema_momentum, spec.ema_overwrite_frequency)
        if spec.lr_schedule is not None and not isinstance(spec.lr_schedule, SC.LearningRateSchedule):
            raise ValueError(f"lr_schedule {spec.lr_schedule!r}: None or a schedule of resunet_a_mltsk_keras_amd.schedules")
        AC.check_steps(spec.gradient_accumulation_steps)
        if spec.optimizer not in ("adam", "sgd", "lamb"):
            raise ValueError(f"optimizer {spec.optimizer!r}: 'adam', 'sgd' or 'lamb'")
        if spec.optimizer == "lamb":
            LB.check_options(spec.beta_1, spec.beta_2, spec.epsilon)
        self._check_loss_options(spec)
        if self._in_ema:
            raise RuntimeError("compile() inside ema_weights(): leave the block first")
        if self.loss is not None and (self.loss.optimizer != spec.optimizer):
            self._t_dev, self._lr_base_dev = -1, None          # device-side step counter / base rate are pushed again
        self.loss = spec
        self.graphs = {}
        if spec.class_weights is not None:
            self.class_w = torch.tensor(list(spec.class_weights) + [0.0] * 8, dtype=torch.float32, device=self.dev)
            self.class_w_ptr = self.class_w.data_ptr()
        else:
            self.class_w_ptr = None
        self._setup_clip(spec)
        self._sched = SC.to_struct(spec.lr_schedule) if spec.lr_schedule is not None else None
        self.E = None
        if spec.use_ema and self.dev is not None:
            self.E = torch.empty_like(self.P)
            self.reset_ema()
        # gradient accumulation: a re-compile drops accumulator and counter (an open cycle is lost with the optimizer it belonged to)
        self.A, self.acc_state = None, None
        self.micro, self._micro_dev = 0, -1
        if spec.gradient_accumulation_steps is not None and self.dev is not None:
            self.A = torch.zeros_like(self.P)
            self.acc_state = torch.zeros(4, dtype=torch.int32, device=self.dev)

    def _check_loss_options(self, spec: LossSpec):
        """The focal kinds and the per-head options against the heads (activation, channels) and losses.py's range: ValueError before any launch."""
        acts = dict(seg=L.ACT_SOFTMAX, bound=L.ACT_SIGMOID, dist=L.ACT_SOFTMAX, color=L.ACT_SIGMOID)
        for name in LS.OPTION_KEYS:
            for h in getattr(spec, name):
                if h not in spec.kind:
                    raise ValueError(f"{name}: '{h}' is not a head of this model ({', '.join(spec.kind)})")
        # the Lovasz loss: binary targets only ('seg' under its softmax, 'bound' per sigmoid channel), and none of the per-pixel options
        for h in spec.lovasz:
            if h not in spec.kind:
                raise ValueError(f"lovasz: '{h}' is not a head of this model ({', '.join(spec.kind)})")
            if spec.kind[h] != L.LOSS_LOVASZ:
                raise ValueError(f"{h}: lovasz options belong to a head on the Lovasz loss")
        for h, kind in spec.kind.items():
            if kind != L.LOSS_LOVASZ:
                continue
            LS.check_lovasz(spec.lovasz.get(h, {}), what=f"{h}: lovasz", head=h, num_classes=3 if h == "color" else self.cfg.num_classes)
            if h in spec.ohem:
                raise ValueError(f"{h}: the Lovasz loss has no per-pixel map, online hard example mining does not combine with it")
            if float(spec.label_smoothing.get(h, 0.0)) != 0.0:
                raise ValueError(f"{h}: the Lovasz loss takes no label smoothing")
        for h, kind in spec.kind.items():
            if kind == L.LOSS_FOCAL_CE and acts[h] != L.ACT_SOFTMAX:
                raise ValueError(f"{h}: categorical focal cross-entropy needs a softmax head")
            if kind == L.LOSS_FOCAL_BCE and acts[h] != L.ACT_SIGMOID:
                raise ValueError(f"{h}: binary focal cross-entropy needs a sigmoid head")
            if kind not in LS.FOCAL_KINDS and (h in spec.focal_gamma or h in spec.focal_alpha or h in spec.class_balance):
                raise ValueError(f"{h}: focal_gamma / focal_alpha / class_balance belong to the focal losses")
            if kind == L.LOSS_FOCAL_CE and spec.class_weights is None:
                raise ValueError(f"{h}: categorical focal cross-entropy needs its per-class alpha (class_weights)")
            nc = 3 if h == "color" else self.cfg.num_classes
            LS.check_options(kind, nc, spec.focal_gamma.get(h, 0.0), spec.class_weights if kind == L.LOSS_FOCAL_CE else spec.focal_alpha.get(h, 0.0),
                             spec.class_balance.get(h, False), spec.label_smoothing.get(h, 0.0), what=h)
        # online hard example mining: per-pixel losses only (Tanimoto has no per-pixel map); a probability threshold means -log p only where the
        # per-pixel loss IS -log p of the true class: plain CE, or weighted CE with unit weights, without smoothing
        for h, o in spec.ohem.items():
            if h not in spec.kind:
                raise ValueError(f"ohem: '{h}' is not a head of this model ({', '.join(spec.kind)})")
            if spec.kind[h] == L.LOSS_TANIMOTO:
                raise ValueError(f"{h}: online hard example mining needs a per-pixel loss, the Tanimoto loss has none")
            if not isinstance(o, dict):
                raise ValueError(f"{h}: ohem options are a dict (losses.ohem_options), got {type(o).__name__}")
            LS.check_ohem(o, what=f"{h}: ohem")
            if o.get("prob_thresh") is not None:
                unit = spec.kind[h] == L.LOSS_WCE and spec.class_weights is not None and all(float(w) == 1.0 for w in spec.class_weights)
                if not (spec.kind[h] == L.LOSS_CE_LOGITS or unit) or float(spec.label_smoothing.get(h, 0.0)) != 0.0:
                    raise ValueError(f"{h}: prob_thresh goes with plain categorical cross-entropy (or weighted CE with unit weights) without label "
                                     "smoothing only; give loss_thresh for the other losses")

    def accumulation_state(self) -> Optional[Dict[str, int]]:
        """gradient_accumulation_steps: dict(steps=K, micro=gradients of the current cycle already accumulated, 0 .. K - 1); None with the
        option off.  The host's mirror: no device read."""
        k = self.loss.gradient_accumulation_steps if self.loss is not None else None
        return None if k is None else dict(steps=int(k), micro=int(self.micro))

    def reset_ema(self):
        """use_ema: E = P (compile(), weights from a file without an average, a broadcast): padding stays zero and the average starts sane."""
        if self.E is not None:
            self.E.copy_(self.P)

    @contextlib.contextmanager
    def ema_weights(self):
        """Run the block under the averaged weights: the CONTENTS of P and E are swapped on the device (the recorded plans hold P's
        pointer, so the buffers stay), the weight copies are marked stale, and everything is swapped back on exit.  A training step inside
        the block raises.  BatchNorm moving statistics are not averaged: the block runs with the current ones."""
        if self.E is None:
            raise RuntimeError("ema_weights(): the model was compiled without use_ema")
        if self._in_ema:
            raise RuntimeError("ema_weights() blocks do not nest")
        self._swap_ema()
        self._in_ema = True
        try:
            yield self
        finally:
            self._in_ema = False
            self._swap_ema()

    def _swap_ema(self):
        tmp = self.P.clone()
        self.P.copy_(self.E); self.E.copy_(tmp)
        self.params_changed()

    def finalize_ema(self):
        """P = E for good (Keras' optimizer.finalize_variable_values); E keeps its values."""
        if self.E is None:
            raise RuntimeError("finalize_ema(): the model was compiled without use_ema")
        if self._in_ema:
            raise RuntimeError("finalize_ema() inside ema_weights(): leave the block first")
        self.P.copy_(self.E)
        self.params_changed()

    def current_lr(self) -> float:
        """The base rate of the NEXT optimizer step: schedules.host_lr at the step counter under a schedule, loss.lr otherwise."""
        sp = self.loss
        return SC.host_lr(sp.lr_schedule, self.t) if sp.lr_schedule is not None else float(sp.lr)

    def _setup_clip(self, spec: LossSpec):
        """The device side of clip.py's options: chunk and variable tables (built once, here), the per-chunk partials, the per-variable sums and
        coefficients, the skip flag, the report and the BatchNorm state's backup.  Nothing is allocated and self.clip is None with every option off."""
        self.clip = None
        self._s_backed = False
        # gradient accumulation takes the chunk-table route too (mode RUA_CLIP_NONE with no clip option): its optimizers honour the hold flag.
        # So does LAMB, always: its trust ratio is per variable
        lamb = spec.optimizer == "lamb"
        if not (spec.clip_on() or spec.gradient_accumulation_steps is not None or lamb) or self.dev is None:
            return
        chunks, vars_, names = CL.build_chunk_table(self.params.entries, spec.decay_exclude or ())
        mode, c = CL.clip_mode(spec.clipnorm, spec.global_clipnorm, spec.clipvalue)
        raw = lambda a: torch.from_numpy(np.frombuffer(a.tobytes(), dtype=np.uint8).copy()).to(self.dev)
        zd = lambda n, dt: torch.zeros(max(n, 4), dtype=dt, device=self.dev)
        self.clip = dict(chunks=raw(chunks), vars=raw(vars_), names=names, n_chunks=len(chunks), n_vars=len(vars_), mode=mode, c=c,
                         cv=c if mode == CL.CLIP_VALUE else 0.0, wd=float(spec.weight_decay or 0.0), skip=1 if spec.skip_nonfinite else 0,
                         partials=zd(len(chunks), torch.float64), var_sumsq=zd(len(vars_), torch.float64), coef=zd(len(vars_), torch.float32),
                         flag=zd(4, torch.int32), report=zd(4, torch.float64),
                         s_backup=zd(self.params.ns, torch.float32) if spec.skip_nonfinite and self.params.ns > 0 else None)
        if lamb:
            # pass 1's per-chunk sums, the finisher's per-variable sums (W then U), ratios and report.  With no clip option, no decay, no skip and
            # no accumulation the sum of squares and the clip finisher are not launched: the coefficients are ones for good
            self.clip["plain"] = not spec.clip_on() and spec.gradient_accumulation_steps is None
            if self.clip["plain"]:
                self.clip["coef"].fill_(1.0)
            self.clip.update(pw=zd(len(chunks), torch.float64), pu=zd(len(chunks), torch.float64), var_wu=zd(2 * len(vars_), torch.float64),
                             ratio=zd(len(vars_), torch.float32), trust=zd(4, torch.float64))

    def trust_report(self) -> Optional[Dict[str, object]]:
        """LAMB: what the last update's finisher wrote (None for the other optimizers) - min_ratio, max_ratio: the smallest and largest trust
        ratio ||w|| / ||update|| it applied; forced: the variables whose ratio a zero or non-finite norm set to 1; updates: updates taken since
        compile() (a skipped or a hold step is none); ratios: {variable name: ratio}.  Synchronises the device."""
        if self.clip is None or "ratio" not in self.clip:
            return None
        torch.cuda.synchronize()
        r = self.clip["trust"].cpu().numpy()
        ratios = self.clip["ratio"].cpu().numpy()[:self.clip["n_vars"]]
        return dict(min_ratio=float(r[0]), max_ratio=float(r[1]), forced=int(r[2]), updates=int(r[3]),
                    ratios={n: float(x) for n, x in zip(self.clip["names"], ratios)})

    def _launch_lamb(self, flag, grad_scale, wc, sv):
        """The three LAMB launches where rua_adam_step_seg stands (lamb.py): moments and direction with the per-chunk sums, the one-block
        finisher (ratios, report), the update.  flag: the flag rua_adam_step_seg would take."""
        sp, ck, lib = self.loss, self.clip, L.lib()
        lib.call("rua_lamb_moments", self.P.data_ptr(), self.G.data_ptr(), self.M1.data_ptr(), self.V1.data_ptr(), ck["chunks"].data_ptr(), ck["n_chunks"],
                 ck["vars"].data_ptr(), ck["coef"].data_ptr(), flag, self.lr_state.data_ptr(), sp.beta_1, sp.beta_2, sp.epsilon, grad_scale, ck["cv"], ck["wd"],
                 ck["pw"].data_ptr(), ck["pu"].data_ptr(), sv)
        lib.call("rua_lamb_finish", ck["pw"].data_ptr(), ck["pu"].data_ptr(), ck["n_chunks"], ck["vars"].data_ptr(), ck["n_vars"], flag, ck["var_wu"].data_ptr(),
                 ck["ratio"].data_ptr(), ck["trust"].data_ptr(), sv)
        lib.call("rua_lamb_apply", self.P.data_ptr(), self.G.data_ptr(), ck["chunks"].data_ptr(), ck["n_chunks"], ck["vars"].data_ptr(), ck["ratio"].data_ptr(), flag,
                 self.lr_dev.data_ptr(), self.lr_state.data_ptr(), ck["wd"], 1, wc, sv)

    def clip_report(self) -> Optional[Dict[str, float]]:
        """What the last optimizer step's finisher wrote (None with every clip / decay / skip option off): norm - that step's global gradient norm
        (grad_scale included) -, min_coef - the smallest coefficient it applied (1 when nothing was clipped; clipvalue does not show here) -, and the
        counts since compile() of steps skipped and of steps a norm clipped.  Synchronises the device: the only host read of the whole feature.
        Under gradient accumulation the four describe and count UPDATE steps (the norm is the mean gradient's); a hold step changes none."""
        if self.clip is None or not self.loss.clip_on():      # gradient accumulation alone walks the chunk table too, but has nothing to report
            return None
        torch.cuda.synchronize()
        r = self.clip["report"].cpu().numpy()
        return dict(norm=float(r[0]), min_coef=float(r[1]), skipped=int(r[2]), clipped=int(r[3]))

    def ohem_report(self) -> Optional[Dict[str, dict]]:
        """Online hard example mining: what rua_ohem_select left for the last training step, per mining head - kept (n_kept / n_valid, 0 with no
        valid pixel), tau (the loss value of the threshold key), tau_key, K, n_kept, n_valid, q16_used, kept_sum, scale.  None when no head mines
        or no training step has run.  Under data parallel and accumulation these are this rank's, this micro-batch's.  Synchronises the device."""
        if self.loss is None or not self.loss.ohem:
            return None
        g = self.graphs.get((getattr(self, "_last_B", None), True))
        if g is None:
            return None
        torch.cuda.synchronize()
        out = {}
        for h in g.heads:
            if "ohem" not in h:
                continue
            r = L.OhemResult.from_buffer_copy(h["ohem"]["result"].cpu().numpy().tobytes())
            out[h["name"]] = dict(kept=r.n_kept / r.n_valid if r.n_valid else 0.0, tau=float(r.tau), tau_key=int(r.tau_key), K=int(r.K), n_kept=int(r.n_kept),
                                  n_valid=int(r.n_valid), q16_used=int(r.q16_used), kept_sum=float(r.kept_sum), scale=float(r.scale))
        return out

    def lovasz_report(self) -> Optional[Dict[str, dict]]:
        """The Lovasz loss: what rua_lovasz_grad left for the last step, per head on it - n_valid, n_cls, G and loss_c per class, loss, scale.
        None when no head is on the loss or no step has run; the last training step's, or an evaluation step's while none has run.  Under data parallel and accumulation these are this rank's, this micro-batch's.
        Synchronises the device."""
        if self.loss is None or L.LOSS_LOVASZ not in self.loss.kind.values():
            return None
        B = getattr(self, "_last_B", None)                  # the last training step's plan; with none yet, an evaluation plan
        g = self.graphs.get((B, True)) or self.graphs.get((B, False)) or next(iter(reversed(list(self.graphs.values()))), None)
        if g is None:
            return None
        torch.cuda.synchronize()
        out = {}
        for h in g.heads:
            if "lovasz" not in h:
                continue
            r = LS.lovasz_result(h["lovasz"]["result"].cpu().numpy().tobytes())
            Cc = h["C"]
            out[h["name"]] = dict(n_valid=r["n_valid"], n_cls=r["n_cls"], G=r["G"][:Cc], loss_c=r["loss_c"][:Cc], loss=r["loss"], scale=float(r["scale"]))
        return out

    def _backup_state(self, s):
        """skip_nonfinite: the BatchNorm moving statistics as the step finds them (the forward folds the batch into them before anyone knows
        whether the gradient is finite); rua_state_copy puts them back behind a skipped step (_launch_optimizer)."""
        ck = self.clip
        if ck is not None and ck["s_backup"] is not None:
            L.lib().call("rua_state_copy", ck["s_backup"].data_ptr(), self.S.data_ptr(), self.params.ns, None, C.c_void_p(s))

    def drop_plans(self):
        """Forget every recorded plan and captured graph (they are rebuilt on the next step): a launch heuristic that is read when a plan
        is RECORDED - the CU count behind the weight gradients' partial counts - has changed (rua_set_tuning(cu_reserve))."""
        if self.dev is not None and (self.graphs or self._captured or self._captured_eval or self._captured_dp):
            torch.cuda.synchronize()
        self._captured, self._captured_eval, self._captured_dp = {}, {}, {}
        self._eval_seen = set()
        self._opt_graph = None
        self.graphs = {}
        cu = C.c_int32(0)
        if self.dev is not None and L.lib().raw("rua_device_info")(C.byref(cu), None, None, 0) == 0 and cu.value > 0:
            self.cu_count = cu.value

    # -- weights ---------------------------------------------------------------------------------------
    def set_weights(self, keras_dict: Dict[str, np.ndarray]):
        P, S = self.params.from_keras(keras_dict)
        self.P.copy_(torch.from_numpy(P)); self.S.copy_(torch.from_numpy(S))
        self.params_changed()

    def params_changed(self):
        """P was written from outside the optimizer (set_weights, a checkpoint, a broadcast): both weight copies are rebuilt from it."""
        self.weights_dirty = True
        self.wf_fresh = False

    def get_weights(self) -> Dict[str, np.ndarray]:
        return self.params.to_keras(self.P.cpu().numpy(), self.S.cpu().numpy())

    def grads_keras(self) -> Dict[str, np.ndarray]:
        return self.params.to_keras(self.G.cpu().numpy())

    def count_params(self) -> int:
        return self.params.count()

    # -- execution ---------------------------------------------------------------------------------------
    def _stream(self) -> int:
        return torch.cuda.current_stream(self.dev).cuda_stream

    def _prep_weights(self, s):
        if self.weights_dirty:
            if self.opt_wcopy and self.wf_fresh:            # the optimizer left the forward copy: only the data-gradient layout is built, from it
                L.lib().call("rua_weight_prep_dgrad", self.Wf.data_ptr(), self.Wd.data_ptr(), self.wprep_items.data_ptr(), self.wprep_n, self.wprep_max,
                             self.wprep_map.data_ptr() if self.wprep_map_n else None, self.wprep_map_n, self.dt, C.c_void_p(s))
            else:
                L.lib().call("rua_weight_prep", self.P.data_ptr(), self.Wf.data_ptr(), self.Wd.data_ptr(), self.wprep_items.data_ptr(),
                             self.wprep_n, self.wprep_max, self.dt, C.c_void_p(s))
                self.wf_fresh = True
            self.weights_dirty = False

    def _ensure_forward_copy(self):
        """Before a captured step is replayed (its weight refresh is the data-gradient-only one): if P changed from outside, rebuild both copies now."""
        if self.opt_wcopy and not self.wf_fresh:
            self.weights_dirty = True
            self._prep_weights(self._stream())

    def _check_void(self, x, norm_type, void_mask):
        """The host-side conditions of a caller-supplied void mask (no-op for None): the public entry points call it before they build or
        launch anything."""
        if void_mask is None:
            return
        if self.loss is None or self.loss.ignore_void is None:
            raise ValueError("void_mask needs a model compiled with ignore_void")
        if isinstance(x, SceneBatch) or norm_type is not None:
            raise ValueError("void_mask goes with float batches only: class-map and scene batches derive their own mask from the class map")
        if x is None:
            raise ValueError("void_mask without a batch")
        want = (x.shape[0],) + tuple(self.cfg.input_shape[:2])
        ok = (isinstance(void_mask, np.ndarray) and void_mask.dtype in (np.dtype(np.uint8), np.dtype(np.bool_))) or \
             (isinstance(void_mask, torch.Tensor) and void_mask.dtype in (torch.uint8, torch.bool))
        if not ok:
            raise ValueError(f"void_mask must be a uint8 or bool array, got {getattr(void_mask, 'dtype', type(void_mask))}")
        if tuple(void_mask.shape) != want:
            raise ValueError(f"void_mask must have shape {want}, got {tuple(void_mask.shape)}")

    def _check_photo(self, x, norm_type, photo):
        """The host-side conditions of a caller-supplied photo table (None for None): the checked int32 [B][16] table of a compact uint8
        batch.  A float batch has no bytes to jitter and a scene batch carries its own (SceneBatch.with_photo): ValueError, before
        anything is uploaded or launched."""
        if photo is None:
            return None
        if isinstance(x, SceneBatch):
            raise ValueError("photo goes with compact uint8 batches only: a scene batch carries its own table (SceneBatch.with_photo)")
        if norm_type is None:
            raise ValueError("photo goes with compact uint8 batches only: a float batch (norm_type None) has no bytes to jitter")
        if x is None:
            raise ValueError("photo without a batch")
        t = check_photo_table(photo, int(self.cfg.input_shape[2]))
        if len(t) != x.shape[0]:
            raise ValueError(f"{len(t)} photo rows for a batch of {x.shape[0]} patches")
        return t

    def _apply_photo(self, g: Graph, table: np.ndarray):
        """rua_window_photometric in place on the staged image of g.compact_buffers(): on the compute stream, behind whatever put
        the bytes there and in front of _compact_targets, outside any captured graph.  The host passes B * 16 integers."""
        img = g.compact_buffers()[0]
        H, W, Cin = self.cfg.input_shape
        t = np.ascontiguousarray(table, dtype=np.int32)
        if t.shape != (g.B, 16):
            raise ValueError(f"photo table of shape {t.shape} for a graph of batch {g.B}")
        L.lib().call("rua_window_photometric", img.data_ptr(), img.data_ptr(), g.B, H, W, Cin, t.ctypes.data, C.c_void_p(self._stream()))

    def _upload(self, g: Graph, x, y, void_mask=None):
        if g.void_u8 is not None and x is not None:
            # float batches: the caller's mask, or none.  (Uploaded with the batch: x None replays the batch - and the mask - already there.)
            if void_mask is None:
                g.void_u8.zero_()
            else:
                m = torch.from_numpy(np.ascontiguousarray(void_mask)) if isinstance(void_mask, np.ndarray) else void_mask
                g.void_u8.copy_(m.to(torch.uint8) if m.dtype == torch.bool else m, non_blocking=bool(m.is_pinned()) and m.dtype == torch.uint8)

        def put(dst: torch.Tensor, src):
            if src is None:
                return
            if isinstance(src, np.ndarray):
                src = torch.from_numpy(np.ascontiguousarray(src, dtype=np.float32))
            if tuple(src.shape) != tuple(dst.shape):
                raise ValueError(f"expected shape {tuple(dst.shape)}, got {tuple(src.shape)}")
            # pageable sources may be temporaries: blocking copy.  Pinned tensors (loader.PrefetchLoader slots, which stay
            # alive and untouched until the step has returned its metrics) go up asynchronously on the compute stream.
            dst.copy_(src, non_blocking=bool(src.is_pinned()) if isinstance(src, torch.Tensor) else False)
        put(g.x_in.t, x)
        if y is not None:
            if isinstance(y, dict):
                for h in g.heads:
                    put(h["y"].t, y[h["name"]])
            else:
                put(g.heads[0]["y"].t, y)

    def _upload_compact(self, g: Graph, x, y, norm_type: int, photo=None):
        """Compact batch: x uint8 [B,H,W,Cin], y uint8 class map [B,H,W] (None: x only).  The bytes go up like _upload's (photo, a
        checked photo table: then rua_window_photometric jitters the image in place), then rua_multitask_targets writes x (normalised) into g.x_in and seg / bound / dist / color into the heads' label buffers on the
        compute stream - in front of the recorded plans, outside any captured graph."""
        img, cls, scratch = g.compact_buffers()

        def put(dst: torch.Tensor, src):
            if isinstance(src, np.ndarray):
                if src.dtype != np.uint8:
                    raise ValueError(f"compact batches are uint8, got {src.dtype}")
                src = torch.from_numpy(np.ascontiguousarray(src))
            if src.dtype != torch.uint8:
                raise ValueError(f"compact batches are uint8, got {src.dtype}")
            if tuple(src.shape) != tuple(dst.shape):
                raise ValueError(f"expected shape {tuple(dst.shape)}, got {tuple(src.shape)}")
            dst.copy_(src, non_blocking=bool(src.is_pinned()))
        put(img, x)
        if y is not None:
            put(cls, y)
        if photo is not None:
            self._apply_photo(g, photo)
        self._compact_targets(g, y is not None, norm_type)

    def _compact_targets(self, g: Graph, with_labels: bool, norm_type: int):
        """rua_multitask_targets from g.compact_buffers() into g.x_in and (with_labels) the heads' label buffers, on the compute stream."""
        img, cls, scratch = g.compact_buffers()
        H, W, Cin = self.cfg.input_shape
        ptr = lambda name: g.outputs[name]["y"].ptr
        if not with_labels:
            labels = (None, None, None, None, None)
        else:
            mt = self.cfg.multitasking
            labels = (cls.data_ptr(), ptr("seg")) + ((ptr("bound"), ptr("dist"), ptr("color")) if mt else (None, None, None))
        L.lib().call("rua_multitask_targets", img.data_ptr(), labels[0], g.B, H, W, Cin, self.cfg.num_classes, int(norm_type), g.x_in.ptr,
                     labels[1], labels[2], labels[3], labels[4], scratch.data_ptr(), scratch.numel(), C.c_void_p(self._stream()))
        if with_labels and g.void_u8 is not None:           # the batch's void mask, from the class map the targets were made of
            L.lib().call("rua_void_mask", cls.data_ptr(), g.B, H, W, self.cfg.num_classes, int(self.loss.ignore_void), g.void_ptr,
                         C.c_void_p(self._stream()))

    def _check_scene(self, x, y, norm_type, with_labels: bool = True):
        """The host-side conditions of a scene batch (no-op for any other x): the public entry points call it before they build or
        launch anything."""
        if not isinstance(x, SceneBatch):
            return
        pool = x.pool
        H, W, Cin = self.cfg.input_shape
        if y is not None:
            raise ValueError("a scene batch carries its own labels: y must be None")
        if isinstance(norm_type, bool) or not isinstance(norm_type, (int, np.integer)) or norm_type not in (1, 2):
            raise ValueError(f"norm_type {norm_type!r}: scene batches support 1 (/255) and 2 (/126.5)")
        if tuple(x.patch) != (H, W) or pool.channels != Cin:
            raise ValueError(f"scene batch of {x.patch[0]} x {x.patch[1]} x {pool.channels} patches for a model whose input is {H} x {W} x {Cin}")
        if with_labels and pool.cls_ptrs is None:
            raise ValueError("this scene pool holds no class maps: it serves predict() only")
        dev = torch.device(self.dev)
        if pool.device.type != dev.type or (dev.index is not None and pool.device.index != dev.index):
            raise ValueError(f"the scene pool lives on {pool.device}, the engine on {self.dev}")
        if x.paste is not None:
            if not with_labels:
                raise ValueError("a paste table changes the labels with the image: it does not go with windows cut without labels")
            if pool.inst_ptrs is None or pool.bank_classes != self.cfg.num_classes:
                raise ValueError(f"the pool's object bank was built for {pool.bank_classes} classes, the model has {self.cfg.num_classes}")

    def _check_paste(self, x, paste):
        """A paste table as a keyword (no-op for None): there is no such thing - the objects live in a scene pool, so only a scene
        batch can carry a table (SceneBatch.with_paste); ValueError, before anything is uploaded or launched."""
        if paste is None:
            return
        if isinstance(x, SceneBatch):
            raise ValueError("paste: a scene batch carries its own table (SceneBatch.with_paste)")
        raise ValueError("paste goes with scene batches only (SceneBatch.with_paste): a compact or float batch has no scene pool to take objects from")

    def _upload_scene(self, g: Graph, batch: SceneBatch, norm_type: int, with_labels: bool = True):
        """Scene batch (scenes.SceneBatch: resident scenes + a window table): rua_scene_windows cuts and augments the windows into
        g.compact_buffers(), then the targets call of _upload_compact - both on the compute stream, in front of the recorded plans,
        outside any captured graph.  The host passes B * 4 integers; nothing is copied.  with_labels False: images only (inference).
        An AffineSceneBatch (B * 7 integers: rotation, zoom and shift) goes through rua_scene_windows_affine in the same place.
        A batch with a photo table (batch.photo, B * 16 integers) gets one in-place rua_window_photometric call between the two.
        A batch with a paste table (batch.paste, M * 16 integers) gets one rua_window_paste call between the cut and the photo call:
        the photometric jitter lights a pasted object together with its new background, and the void mask, made from the staged
        class map, follows the pasted labels.  Objects are pasted at the scene's native resolution, into a zoomed affine window too.
        A batch without a table issues no call for it."""
        self._check_scene(batch, None, norm_type, with_labels)
        pool = batch.pool
        H, W, Cin = self.cfg.input_shape
        if len(batch) != g.B:
            raise ValueError(f"scene batch of {len(batch)} windows for a graph of batch {g.B}")
        img, cls, _ = g.compact_buffers()
        rows = np.ascontiguousarray(batch.rows, dtype=np.int32)
        L.lib().call("rua_scene_windows_affine" if isinstance(batch, AffineSceneBatch) else "rua_scene_windows", pool.img_ptrs, pool.cls_ptrs if with_labels else None, pool.heights, pool.widths, len(pool),
                     rows.ctypes.data, g.B, H, W, Cin, img.data_ptr(), cls.data_ptr() if with_labels else None, C.c_void_p(self._stream()))
        if batch.paste is not None:
            self._apply_paste(g, batch)
        if batch.photo is not None:
            self._apply_photo(g, batch.photo)
        self._compact_targets(g, with_labels, int(norm_type))

    def _apply_paste(self, g: Graph, batch: SceneBatch):
        """rua_window_paste on the staged image and class map of g.compact_buffers(): on the compute stream, behind the cut and in
        front of the photo and targets calls, outside any captured graph.  The host passes M * 16 integers; the objects come from
        the pool's resident scenes and id maps (ScenePool.object_bank)."""
        pool = batch.pool
        img, cls, _ = g.compact_buffers()
        H, W, Cin = self.cfg.input_shape
        t = np.ascontiguousarray(batch.paste, dtype=np.int32)
        L.lib().call("rua_window_paste", img.data_ptr(), cls.data_ptr(), g.B, H, W, Cin, self.cfg.num_classes, pool.img_ptrs, pool.cls_ptrs,
                     pool.inst_ptrs, pool.heights, pool.widths, len(pool), t.ctypes.data if len(t) else None, len(t), C.c_void_p(self._stream()))

    def _put_batch(self, g: Graph, x, y, norm_type: Optional[int], with_labels: bool = True, void_mask=None, photo=None):
        """norm_type None: float batch (_upload); 1 or 2: compact uint8 batch (_upload_compact).  x a SceneBatch: _upload_scene
        (y is None: the labels are the pool's class maps; with_labels False: predict)."""
        if isinstance(x, SceneBatch):
            if y is not None:
                raise ValueError("a scene batch carries its own labels: y must be None")
            self._upload_scene(g, x, norm_type, with_labels)
        elif norm_type is None:
            self._upload(g, x, y, void_mask)
        elif x is not None:
            self._upload_compact(g, x, y, norm_type, photo)

    def _zero_arena(self, g: Graph, s):
        L.lib().call("rua_fill_zero", self.stats_arena.data_ptr(), g.stats_used * 8, C.c_void_p(s))

    def _results(self, g: Graph):
        """Metric list of the step in the reference's order.  Under data parallel the scalars are summed over the replicas
        first (one all-reduce of 16 doubles), so every rank returns the SAME numbers, aggregated the way
        MirroredStrategy reports them (train_ISPRS.py:347,432): losses = mean of the replicas' means, accuracy over all
        replicas' pixels, TP/FP/TN/FN summed.  Every rank must therefore fetch results in the same steps."""
        sc, w = self.stats_arena[:16], 1
        if self.dist is not None and self.world > 1:
            sc, w = self.dist.reduce_scalars(sc), self.world
        sc = sc.cpu().numpy()
        per = [float(sc[h["slot"]] * h["norm"] / w) for h in g.heads]
        total = sum(self.loss.weight[h["name"]] * v for h, v in zip(g.heads, per))
        M = g.outputs["seg"]["x"].M * w
        if g.void_u8 is not None:                           # every valid pixel is counted once per class in TP + FP + TN + FN; no valid pixel: accuracy 0
            M = float(sc[9] + sc[10] + sc[11] + sc[12]) / g.outputs["seg"]["C"]
        mets = [float(sc[8] / M) if M > 0 else 0.0, float(sc[9]), float(sc[10]), float(sc[11]), float(sc[12])]
        if self.cfg.multitasking:
            return [total] + per + mets
        return [total] + mets

    def _set_overwrite(self, v: int):
        if self._ow != v:
            self.ow_flag.fill_(v)
            self._ow = v

    def forward_backward(self, x=None, y=None, _whole_step: bool = False, norm_type: Optional[int] = None, void_mask=None, photo=None, paste=None):
        """forward + losses + backward on the current stream; gradients are ADDED to self.G (several calls before one optimizer_step accumulate, e.g. the
        replicas of a data-parallel step played one after the other); _whole_step (train_step): the arena is zero and this is the step's only backward.
        norm_type 1 / 2: x, y are a compact batch (uint8 image, uint8 class map; _upload_compact); photo: as train_step."""
        self._check_scene(x, y, norm_type)
        self._check_void(x, norm_type, void_mask)
        photo = self._check_photo(x, norm_type, photo)
        self._check_paste(x, paste)
        # first-writer overwrite needs a ZERO gradient arena: after a standalone forward_backward() (which accumulates) the arena holds
        # unapplied gradients, and the next whole step must accumulate on top of them too (mixing the two calls keeps its old meaning)
        self._set_overwrite(1 if (_whole_step and self.wgrad_overwrite and not self._g_pending) else 0)
        if not _whole_step:
            self._g_pending = True
        B = x.shape[0] if x is not None else self._last_B
        self._last_B = B
        g = self.graph(B, True)
        s = self._stream()
        self._put_batch(g, x, y, norm_type, void_mask=void_mask, photo=photo)
        if any(o.get("warmup") for o in self.loss.ohem.values()):      # rua_ohem_select reads the step counter in front of the optimizer launch
            self._sync_lr_state()
        self._zero_arena(g, s)
        if not self._s_backed:                              # the first forward since an optimizer step: the state this step begins with
            self._backup_state(s)
            self._s_backed = True
        self._prep_weights(s)
        g.fwd.run(s)
        g.loss_plan.run(s)
        hooks = None
        if self.dist is not None:
            self.dist.start_state_reduce(self)
            self.dist.reducer.begin()
            if self.dist.overlap:
                hooks = self._bucket_hooks(g)
        g.bwd.run(s, hooks)
        return g

    def _bucket_marks(self, g: Graph) -> Dict[int, List[int]]:
        """{backward launch index -> gradient buckets that are complete after that launch}: a bucket is complete after the last launch
        that names one of its parameters' gradients."""
        if getattr(g, "_marks", None) is None:
            last: Dict[int, int] = {}
            for idx, (_, _, _, grads) in enumerate(g.bwd.calls):
                for off in grads:
                    last[self.dist.bucket_of(off)] = idx
            by_idx: Dict[int, List[int]] = {}
            for b, idx in sorted(last.items()):
                by_idx.setdefault(idx, []).append(b)
            g._marks = by_idx
        return g._marks

    def _bucket_hooks(self, g: Graph):
        """{backward launch index -> fire the all-reduce of every gradient bucket that is complete after it}."""
        if getattr(g, "_hooks", None) is None:
            red = self.dist.reducer
            g._hooks = {idx: (lambda bs=bs: [red.ready(b) for b in bs]) for idx, bs in self._bucket_marks(g).items()}
        return g._hooks

    def _set_lr(self):
        """Advance the step counter.  The step-dependent learning rate is produced on the device by the optimizer launch
        (`rua_lr_step`), so a captured step replays with no host-side scalar update in between; the host only pushes the
        base rate / the counter when they were changed from outside (K.set_value(optimizer.lr), a loaded checkpoint)."""
        sp = self.loss
        if self._in_ema:
            raise RuntimeError("a training step inside ema_weights(): P holds the averaged weights; leave the block first")
        self._sync_lr_state()
        k = sp.gradient_accumulation_steps
        if k is not None:
            # gradient accumulation: the gate of this step's optimizer launch advances the device's micro counter and decides hold / update from
            # it; the host mirrors it the way it mirrors t, and a hold step advances neither t nor the device's step counter
            if self._micro_dev != self.micro:
                self.acc_state.copy_(torch.tensor([self.micro, 0, 0, 0], dtype=torch.int32))
            hold = AC.is_hold(self.micro, k)
            self.micro = self.micro + 1 if hold else 0
            self._micro_dev = self.micro
            if hold:
                return
        self.t += 1
        self._t_dev += 1                                    # the optimizer launch of this step advances the device counter

    def _sync_lr_state(self):
        """The device pair [steps taken, base rate] brought up to the host's, where they were changed from outside.  _set_lr's first half; a
        forward_backward() of a model that mines hard examples under a warm-up calls it too, since rua_ohem_select reads the counter in front of
        the optimizer launch."""
        sp = self.loss
        if sp.lr_schedule is not None:
            # the rate kernel writes the base rate itself (lr_state[1]) from the counter: only a counter changed from outside (a checkpoint) is pushed
            if self._t_dev != self.t:
                self.lr_state.copy_(torch.tensor([float(self.t), SC.host_lr(sp.lr_schedule, self.t)], dtype=torch.float64))
                self._t_dev, self._lr_base_dev = self.t, None
        elif self._t_dev != self.t or self._lr_base_dev != sp.lr:
            self.lr_state.copy_(torch.tensor([float(self.t), float(sp.lr)], dtype=torch.float64))
            self._t_dev, self._lr_base_dev = self.t, sp.lr

    def _launch_optimizer(self, grad_scale, s):
        sp = self.loss
        if self.A is not None:
            return self._launch_optimizer_accum(grad_scale, s)
        if self._sched is not None:                         # the same one-thread launch, with the schedule's constants by value
            L.lib().call("rua_lr_schedule_step", self.lr_state.data_ptr(), self.lr_dev.data_ptr(), self._sched, 1 if sp.optimizer == "adam" else 0,
                         float(sp.beta_1), float(sp.beta_2), C.c_void_p(s))
        else:
            L.lib().call("rua_lr_step", self.lr_state.data_ptr(), self.lr_dev.data_ptr(), 1 if sp.optimizer == "adam" else 0,
                         float(sp.beta_1), float(sp.beta_2), C.c_void_p(s))
        wc = self.Wf.data_ptr() if self.opt_wcopy else None    # bf16 storage: the updated weights leave as the forward-layout copy in the same pass
        ck = self.clip
        if ck is not None:
            # clip.py's options: sum of squares per chunk, the one-block finisher (coefficients, skip flag, report), the optimizer over the chunk table
            # and - skip_nonfinite - the BatchNorm state put back behind a skipped step.  Everything is decided on the device: a replay needs no host
            # scalar.  Under data parallel this runs on the REDUCED gradient (dist.reduce_gradients comes first and has already copied the reduced
            # state out of G's tail into S, so the restore is the last writer of S): every rank takes the same decision.
            lib, sv = L.lib(), C.c_void_p(s)
            if not ck.get("plain"):                         # plain LAMB: nothing to clip, decay or skip - the coefficients are ones
                lib.call("rua_grad_sumsq", self.G.data_ptr(), ck["chunks"].data_ptr(), ck["n_chunks"], ck["partials"].data_ptr(), sv)
                lib.call("rua_clip_finish", ck["partials"].data_ptr(), ck["n_chunks"], ck["vars"].data_ptr(), ck["n_vars"], ck["mode"], ck["c"], float(grad_scale),
                         ck["skip"], ck["var_sumsq"].data_ptr(), ck["coef"].data_ptr(), ck["flag"].data_ptr(), ck["report"].data_ptr(), sv)
            flag = ck["flag"].data_ptr() if ck["skip"] else None
            if sp.optimizer == "lamb":
                self._launch_lamb(flag, grad_scale, wc, sv)
            elif sp.optimizer == "adam":
                lib.call("rua_adam_step_seg", self.P.data_ptr(), self.G.data_ptr(), self.M1.data_ptr(), self.V1.data_ptr(), ck["chunks"].data_ptr(),
                         ck["n_chunks"], ck["vars"].data_ptr(), ck["coef"].data_ptr(), flag, self.lr_dev.data_ptr(), self.lr_state.data_ptr(),
                         sp.beta_1, sp.beta_2, KERAS_EPS, grad_scale, ck["cv"], ck["wd"], 1, wc, sv)
            else:
                lib.call("rua_sgd_step_seg", self.P.data_ptr(), self.G.data_ptr(), self.M1.data_ptr(), ck["chunks"].data_ptr(), ck["n_chunks"],
                         ck["vars"].data_ptr(), ck["coef"].data_ptr(), flag, self.lr_dev.data_ptr(), self.lr_state.data_ptr(), sp.momentum,
                         grad_scale, ck["cv"], ck["wd"], 1, wc, sv)
            self._launch_ema(wc, flag, s)
            if ck["s_backup"] is not None:
                lib.call("rua_state_copy", self.S.data_ptr(), ck["s_backup"].data_ptr(), self.params.ns, flag, sv)
            return
        if sp.optimizer == "adam":
            L.lib().call("rua_adam_step_w", self.P.data_ptr(), self.G.data_ptr(), self.M1.data_ptr(), self.V1.data_ptr(), self.params.n,
                         0.0, self.lr_dev.data_ptr(), sp.beta_1, sp.beta_2, KERAS_EPS, grad_scale, 1, wc, C.c_void_p(s))
        else:
            L.lib().call("rua_sgd_step_w", self.P.data_ptr(), self.G.data_ptr(), self.M1.data_ptr(), self.params.n, 0.0,
                         self.lr_dev.data_ptr(), sp.momentum, grad_scale, 1, wc, C.c_void_p(s))
        self._launch_ema(wc, None, s)

    def _launch_optimizer_accum(self, grad_scale, s):
        """gradient_accumulation_steps: the optimizer tail of a micro-step, the same launches on a hold and on an update step (a captured step
        replays either): the gate decides from the device's micro counter, rua_accum_step adds G[:n] to the accumulator (hold) or turns it into
        the cycle's mean (update), and the chunk-table route of clip.py follows in its gated forms - rate kernel, sum of squares and finisher
        keep every bit on a hold step; the finisher writes flag[0] = skipped, which only the BatchNorm restore reads, and flag[1] = hold or
        skipped, which the optimizer (it then only zeroes G and rewrites the bf16 copy of the unchanged weights) and the moving average read.
        Two launches more than the chunk-table route, four more than the flat one.  Under data parallel G is the reduced gradient, and its
        tail - the BatchNorm state - is not accumulated."""
        sp, ck, lib, sv = self.loss, self.clip, L.lib(), C.c_void_p(s)
        k, adam = int(sp.gradient_accumulation_steps), 1 if sp.optimizer == "adam" else 0
        hold = self.acc_state.data_ptr() + 4
        flag = ck["flag"].data_ptr()
        both = flag + 4
        wc = self.Wf.data_ptr() if self.opt_wcopy else None
        lib.call("rua_accum_gate", self.acc_state.data_ptr(), k, hold, sv)
        lib.call("rua_accum_step", self.G.data_ptr(), self.A.data_ptr(), self.params.n, k, hold, sv)
        if self._sched is not None:
            lib.call("rua_lr_schedule_step_gated", self.lr_state.data_ptr(), self.lr_dev.data_ptr(), self._sched, adam, float(sp.beta_1), float(sp.beta_2), hold, sv)
        else:
            lib.call("rua_lr_step_gated", self.lr_state.data_ptr(), self.lr_dev.data_ptr(), adam, float(sp.beta_1), float(sp.beta_2), hold, sv)
        lib.call("rua_grad_sumsq_gated", self.G.data_ptr(), ck["chunks"].data_ptr(), ck["n_chunks"], ck["partials"].data_ptr(), hold, sv)
        lib.call("rua_clip_finish_gated", ck["partials"].data_ptr(), ck["n_chunks"], ck["vars"].data_ptr(), ck["n_vars"], ck["mode"], ck["c"], float(grad_scale),
                 ck["skip"], ck["var_sumsq"].data_ptr(), ck["coef"].data_ptr(), flag, ck["report"].data_ptr(), hold, sv)
        if sp.optimizer == "lamb":
            self._launch_lamb(both, grad_scale, wc, sv)
        elif adam:
            lib.call("rua_adam_step_seg", self.P.data_ptr(), self.G.data_ptr(), self.M1.data_ptr(), self.V1.data_ptr(), ck["chunks"].data_ptr(),
                     ck["n_chunks"], ck["vars"].data_ptr(), ck["coef"].data_ptr(), both, self.lr_dev.data_ptr(), self.lr_state.data_ptr(),
                     sp.beta_1, sp.beta_2, KERAS_EPS, grad_scale, ck["cv"], ck["wd"], 1, wc, sv)
        else:
            lib.call("rua_sgd_step_seg", self.P.data_ptr(), self.G.data_ptr(), self.M1.data_ptr(), ck["chunks"].data_ptr(), ck["n_chunks"],
                     ck["vars"].data_ptr(), ck["coef"].data_ptr(), both, self.lr_dev.data_ptr(), self.lr_state.data_ptr(), sp.momentum,
                     grad_scale, ck["cv"], ck["wd"], 1, wc, sv)
        self._launch_ema(wc, both, s)
        if ck["s_backup"] is not None:
            lib.call("rua_state_copy", self.S.data_ptr(), ck["s_backup"].data_ptr(), self.params.ns, flag, sv)

    def _launch_ema(self, wc, flag, s):
        """use_ema: the moving average right behind the optimizer kernel, inside the same capture.  The step counter (first-step copy, overwrite
        period) and the skip flag are read on the device; an overwrite refreshes the forward-layout copy the optimizer wrote (wc) as well."""
        if self.E is None:
            return
        sp = self.loss
        L.lib().call("rua_ema_step", self.E.data_ptr(), self.P.data_ptr(), wc, self.params.n, float(sp.ema_momentum), self.lr_state.data_ptr(),
                     int(sp.ema_overwrite_frequency or 0), flag, C.c_void_p(s))

    def optimizer_step(self, grad_scale: float = 1.0):
        self._set_lr()
        self._launch_optimizer(grad_scale, self._stream())
        self.weights_dirty = True
        self._g_pending = False                             # the optimizer zeroed the arena as it consumed it
        self._s_backed = False                              # skip_nonfinite: the next forward_backward opens a new step

    def _issue_step(self, g: Graph):
        """The whole training step on the current stream: arena fill, weight refresh (forced), forward, losses, backward, optimizer -
        what _graph_step runs and captures and count_step_dispatches counts."""
        s = self._stream()
        self._zero_arena(g, s)
        self._backup_state(s)
        self.weights_dirty = True
        self._prep_weights(s)
        g.fwd.run(s)
        g.loss_plan.run(s)
        g.bwd.run(s)
        self._launch_optimizer(1.0, s)

    def _graph_step(self, x, y, norm_type: Optional[int] = None, void_mask=None, photo=None):
        """Single-GPU fast path: the whole step (arena zeroing, weight refresh, forward, losses, backward, optimizer)
        captured once into a HIP graph and replayed; only the input upload and the lr scalar stay outside."""
        B = x.shape[0] if x is not None else self._last_B
        self._last_B = B
        g = self.graph(B, True)
        self._put_batch(g, x, y, norm_type, void_mask=void_mask, photo=photo)
        self._set_lr()
        self._set_overwrite(1 if (self.wgrad_overwrite and not self._g_pending) else 0)
        self._g_pending = False                             # the step's optimizer launch zeroes the arena
        cap = self._captured.get(B)
        if cap is None:
            # warm-up run outside capture (sets kernel attributes, pays first-launch costs), then capture
            self._issue_step(g)
            torch.cuda.synchronize()
            cap = torch.cuda.CUDAGraph()
            with torch.cuda.graph(cap):
                self._issue_step(g)
            self._captured[B] = cap
            self.weights_dirty = True
            # the warm-up consumed this step's update; the capture itself launched nothing
            return g
        self._ensure_forward_copy()
        cap.replay()
        self.weights_dirty = True
        return g

    def count_step_dispatches(self, batch: int) -> Optional[int]:
        """Kernel nodes of the whole training step (arena fill, weight refresh, forward, losses, backward, optimizer) captured
        into a throw-away HIP graph: the number of dispatches a step costs, counted rather than read off a profile.  The step must
        have run at least once (kernel attributes set); the capture launches nothing."""
        try:
            g = self.graph(batch, True)
            torch.cuda.synchronize()
            cap = torch.cuda.CUDAGraph(keep_graph=True)
            dirty, fresh = self.weights_dirty, self.wf_fresh
            with torch.cuda.graph(cap):
                self._issue_step(g)
            self.weights_dirty, self.wf_fresh = dirty, fresh
            k = C.c_int32(0)
            L.lib().call("rua_graph_kernel_nodes", C.c_void_p(cap.raw_cuda_graph()), C.byref(k), None)
            del cap
            return int(k.value)
        except Exception:                                   # diagnostics only
            torch.cuda.synchronize()
            return None

    def _graph_step_dp(self, x, y, norm_type: Optional[int] = None, void_mask=None, photo=None):
        """Data-parallel fast path: the step is cut at the launches after which a gradient bucket is complete; every
        piece is its own HIP graph, the bucket all-reduces are issued eagerly between the replays on the reducer's side
        stream (RCCL stays outside the captures), so they overlap the next pieces exactly like in the eager path."""
        B = x.shape[0] if x is not None else self._last_B
        self._last_B = B
        g = self.graph(B, True)
        self._put_batch(g, x, y, norm_type, void_mask=void_mask, photo=photo)
        red = self.dist.reducer
        pieces = self._captured_dp.get(B)
        if pieces is None:
            # one eager step (first-launch costs, kernel attributes, RCCL channel set-up), then capture the pieces
            self.forward_backward(None, None, _whole_step=True)
            self.dist.reduce_gradients(self)
            self.optimizer_step(1.0 / self.world)
            torch.cuda.synchronize()
            marks = self._bucket_marks(g) if self.dist.overlap else {}
            cuts = sorted(marks)
            nb = len(g.bwd.calls)
            pieces, first = [], 0
            try:
                for ci, idx in enumerate(cuts + [nb - 1]):
                    if ci == len(cuts) and first >= nb:
                        break
                    cap = torch.cuda.CUDAGraph()
                    # thread_local: the process group's watchdog thread may query events while we capture
                    with torch.cuda.graph(cap, capture_error_mode="thread_local"):
                        s = self._stream()
                        if first == 0:
                            self._zero_arena(g, s); self._backup_state(s); self.weights_dirty = True; self._prep_weights(s)
                            g.fwd.run(s); g.loss_plan.run(s)
                        g.bwd.run(s, first=first, last=idx + 1)
                    pieces.append((cap, marks.get(idx, []) if ci < len(cuts) else []))
                    first = idx + 1
                opt = torch.cuda.CUDAGraph()
                with torch.cuda.graph(opt, capture_error_mode="thread_local"):
                    self._launch_optimizer(1.0 / self.world, self._stream())
                ok = 1
            except RuntimeError as exc:
                # Capture is an optimisation: the eager launch sequence issues the same kernels and the same collectives
                # (BN state first, then the buckets in the same order - see the replay below).  Say so loudly and carry on.
                import sys
                print(f"[resunet_a] HIP-graph capture of the data-parallel step failed ({exc}); running it eagerly", file=sys.stderr, flush=True)
                torch.cuda.synchronize()
                ok = 0
            # the ranks switch TOGETHER: the fallback is decided by a MIN over the ranks' capture results
            if self.dist.all_ranks_ok(ok) == 0:
                self.dp_graph = False
                self.weights_dirty = True
                return g
            self._captured_dp[B] = pieces
            self._opt_graph = opt
            self.weights_dirty = True
            return g
        self._set_lr()
        self._set_overwrite(1 if (self.wgrad_overwrite and not self._g_pending) else 0)
        self._g_pending = False
        self._ensure_forward_copy()
        red.begin()
        for pi, (cap, buckets) in enumerate(pieces):
            cap.replay()
            # (History, DESIGN.md section 6: with hipMemsetAsync captured as memset NODES - the statistics-arena fill at the head of the
            # first piece, the gradient fills of the stride-2 convolutions - these back-to-back piece replays corrupted the step on
            # some boxes of the pool, deterministically per process and NOT as an ordering problem: a device synchronise between the
            # replays did not help, an eager kernel launch between them did, and so does what is in place now - rua_fill_zero is an
            # ordinary kernel, no graph holds a memset node.  tools/dp_graph_check.py reproduces all of it; RUA_DP_FENCE=1 brings the
            # eager kernel back for experiments.)
            if self.dp_fence:
                self._dp_fence.zero_()
            elif os.environ.get("RUA_DP_SYNC") == "1":          # experiment (tools/dp_graph_check.py): a device synchronise instead
                torch.cuda.synchronize()
            if pi == 0:
                # same collective order as the eager path (forward_backward): BN moving statistics first - they are final
                # once the forward (inside the first piece) has run - then the gradient buckets
                self.dist.start_state_reduce(self)
            for b in buckets:
                red.ready(b)
        self.dist.reduce_gradients(self)
        self._opt_graph.replay()
        self.weights_dirty = True
        return g

    def train_step(self, x=None, y=None, fetch: bool = True, norm_type: Optional[int] = None, void_mask=None, photo=None, paste=None):
        """One Keras train_on_batch (train_ISPRS.py:131,148): returns the metric list in the reference's order.
        norm_type 1 / 2: x, y are a compact batch - uint8 image [B,H,W,Cin], uint8 class map [B,H,W] - whose float input and targets
        are built on the device (_upload_compact) before the step.  x a scenes.SceneBatch (y None, norm_type 1 / 2): the patches are cut
        from the resident scenes on the device (_upload_scene).  void_mask (float batches of a model compiled with ignore_void): uint8 or bool
        [B,H,W], non-zero = void; class-map and scene batches derive theirs from the class map (rua_void_mask).  photo (compact uint8
        batches): an int32 [B][16] photo table (scenes.check_photo_table) - the uploaded image is jittered in place
        (rua_window_photometric) before the targets are built; a scene batch carries its own, a float batch has none: ValueError.
        paste: always a ValueError - pasted objects come from a scene pool, so only a scene batch carries a paste table
        (SceneBatch.with_paste), which _upload_scene applies between the cut and the photo call."""
        self._check_scene(x, y, norm_type)
        self._check_void(x, norm_type, void_mask)
        photo = self._check_photo(x, norm_type, photo)
        self._check_paste(x, paste)
        if self.use_graph and self.dist is None:
            g = self._graph_step(x, y, norm_type, void_mask, photo)
            return self._results(g) if fetch else None
        if self.use_graph and self.dp_graph and not self.dist.host_staged:
            g = self._graph_step_dp(x, y, norm_type, void_mask, photo)
            return self._results(g) if fetch else None
        g = self.forward_backward(x, y, _whole_step=True, norm_type=norm_type, void_mask=void_mask, photo=photo)
        if self.dist is not None:
            self.dist.reduce_gradients(self)
        self.optimizer_step(1.0 / self.world)
        return self._results(g) if fetch else None

    def test_step(self, x, y, norm_type: Optional[int] = None, void_mask=None, photo=None, paste=None):
        """Keras test_on_batch (train_ISPRS.py:167,186): BN uses moving statistics, nothing is updated.  norm_type, void_mask, photo: as train_step."""
        self._check_scene(x, y, norm_type)
        self._check_void(x, norm_type, void_mask)
        photo = self._check_photo(x, norm_type, photo)
        self._check_paste(x, paste)
        g = self.graph(x.shape[0], False)
        s = self._stream()
        self._put_batch(g, x, y, norm_type, void_mask=void_mask, photo=photo)
        self._zero_arena(g, s)
        self._prep_weights(s)
        g.fwd.run(s)
        g.loss_plan.run(s)
        return self._results(g)

    def predict(self, x, norm_type: Optional[int] = None):
        """Inference forward (moving BN statistics).  The forward launch list of a batch size is captured into a HIP graph
        on its second use (the reference's evaluation calls predict(batch_size=1) per patch, test_ISPRS.py:28: ~250
        launches of host time per patch otherwise).  norm_type 1 / 2: x is uint8 and normalised on the device."""
        self._check_scene(x, None, norm_type, with_labels=False)
        B = x.shape[0]
        g = self.graph(B, False)
        self._put_batch(g, x, None, norm_type, with_labels=False)
        self._forward_eval(g)
        outs = {h["name"]: h["p"].t.cpu().numpy() for h in g.heads}
        return outs if self.cfg.multitasking else outs["seg"]

    def _forward_eval(self, g: Graph):
        """The inference forward of the batch already in g.x_in, on the compute stream: the recorded launch list, or its captured HIP
        graph from the second use of a batch size on (predict and predict_scene share the captures)."""
        B = g.B
        s = self._stream()
        self._prep_weights(s)
        cap = self._captured_eval.get(B) if self.use_graph else None
        if cap is None:
            g.fwd.run(s)
            if self.use_graph and B in self._eval_seen:
                try:
                    torch.cuda.synchronize()
                    cap = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(cap):
                        g.fwd.run(self._stream())
                    self._captured_eval[B] = cap           # capture launched nothing: this call's results are the eager run's
                except RuntimeError as exc:
                    import sys
                    print(f"[resunet_a] HIP-graph capture of the inference forward failed ({exc}); staying eager", file=sys.stderr, flush=True)
                    torch.cuda.synchronize()
                    self._captured_eval[B] = False
            self._eval_seen.add(B)
        elif cap is False:
            g.fwd.run(s)
        else:
            cap.replay()

    def predict_scene(self, pool, scene: int, stride: Optional[int] = None, batch: int = 8, norm_type: int = 1, on_batch=None, views=(0,),
                      erode: int = 0, heads=(), on_heads=None, boundary: Optional[int] = None, scales=None, blend=None, sieve=None, sweep=None,
                      instances=None):
        """The class map of a whole resident scene: (uint8 [H][W] prediction, int64 [C][C] confusion matrix indexed [true][pred], None
        for a pool without class maps).  scenes.predict_table covers the scene with windows `stride` apart (None: the patch) and gives
        every pixel to the window it is most central in; the windows go through the forward `batch` at a time - rua_scene_windows,
        the plan or captured graph of predict(), then rua_scene_stitch on the seg head's probabilities, all on the compute stream -
        and only the map and the matrix come back, once, at the end.  The last batch is padded with repeats of its last window that
        own nothing, so one batch size (one graph, one capture) serves the scene.  A label >= C is not counted.
        on_batch(rows, own, p): called after each batch's stitch has been issued with the batch's tables and the seg head's device
        tensor [batch][H][W][C], which the next batch overwrites (clone it to keep it).
        views: test-time augmentation - a tuple of symmetry codes (scenes.transform) or a scenes.VIEW_SETS name.  (0,) is the path
        above, call for call.  Otherwise every window is predicted under its K views in ONE forward: G = max(1, batch // K) windows
        make a forward of G * K patches (scenes.view_rows, cut by rua_scene_windows), and rua_scene_stitch_views turns the views
        back, sums each pixel's K probability vectors in view order and takes the arg-max of the sum (scenes.host_stitch_views is
        its definition).  Ownership is unchanged; the last batch is padded with repeats of its last group that own nothing;
        on_batch sees rows [G * K][4], own [G][4] and p [G * K][H][W][C].
        erode: 0 is the path and the return value above.  A radius 1..16 also scores the finished map on the eroded ground truth
        (scenes.host_erode: class-map pixels within that radius of another value become "no class"; the ISPRS benchmark uses 3):
        after the window loop one rua_scene_erode call counts the stitched prediction against the eroded class map into a second
        matrix, on the compute stream, and the return value is (prediction, confusion matrix, confusion matrix on the eroded ground
        truth).  It scores the stitched map, so it works under any views.  ValueError for a pool without class maps.
        heads: () is the path and the return value above.  Otherwise a tuple out of "seg", "bound", "dist", "color" and "color_rgb":
        after each forward one rua_scene_stitch_maps call per requested head follows the seg stitch on the compute stream, with the
        batch's same rows and own (K = 1 for views (0,)), into a uint8 [H][W][Ch] map of the head on the device - the K views turned
        back, quantised and averaged in integers (scenes.host_stitch_maps is the definition): the seg probabilities, the boundary
        and distance maps, the colour head's HSV, each times 255 and rounded; "color_rgb" is the colour head turned into an RGB
        picture (mode "hsv_rgb"), which needs norm_type 1 (under 2 the colour target is not HSV / (179, 255, 255): labels.color_label).
        The maps come back once, at the end, as a last element of the return tuple: {head: uint8 [H][W][Ch]}.  ValueError for a head
        the model does not have (single task: only "seg").  on_heads(rows, own, {head: device tensor [batch][H][W][Ch]}): called
        after the batch's stitches have been issued, with the head outputs the next batch overwrites ("color_rgb" is "color"'s).
        boundary: None is the path and the return value above, call for call.  A tolerance 0..16 (0: exact coincidence) also counts
        the boundary pixels of the finished map against those of the pool's un-eroded class map (scenes.host_boundary_counts: per
        class n_pred, m_pred, n_true, m_true - what scenes.boundary_scores turns into the boundary precision, recall and F1): one
        rua_scene_boundary call after the window loop, on the compute stream, into a zeroed int64 [C][4] buffer that is fetched at
        the end.  It scores the stitched map, so it works under any views and together with erode and heads; the return value is
        (prediction, confusion matrix[, matrix on the eroded ground truth][, boundary counts][, head maps]).  ValueError for a pool
        without class maps.
        scales: None or (1.0,) is the path and the return value above, call for call.  Otherwise multi-scale test-time augmentation,
        a tuple of 1 to 8 distinct zooms (> 1 zooms in; scenes.check_scales): an int32 [H][W][C] accumulator (4 H W C bytes) is zeroed
        on the compute stream and, scale after scale in the order given, the scene is covered by scenes.scale_table - footprints of
        patch / zoom scene pixels, the stride scaled with them, every pixel owned by the footprint it is most central in -, batches
        of G = max(1, batch // K) footprints under the K views are cut by rua_scene_windows_affine (pool.affine_batch), go through the
        same forward plan / captured graph and are resampled onto the scene grid and added by one rua_scene_accumulate call each
        (scenes.host_accumulate is the definition; nothing is blended between neighbouring windows of a pass, only the passes are
        summed); the last batch of a pass is padded with repeats of its last group that own an empty rectangle.  One
        rua_scene_argmax call then writes the class map and the confusion matrix (scenes.host_argmax); erode and boundary score that
        map as above.  on_batch(rows7, own, p) sees the [G * K][7] affine rows, the [G][4] rectangles in scene coordinates and the
        device tensor.  ValueError, before any GPU work, with heads (multi-scale maps of the other heads are not built), for a
        footprint larger than the scene, a transposing view with a non-square patch or a malformed `scales`.
        blend: None is every path above, call for call.  "linear" blends overlapping windows instead of giving each pixel to one of
        them, always through the accumulator: scales None or (1.0,) is one pass with the patch as its footprint, and stride None
        then means patch // 2 per axis (blending windows that do not overlap does nothing).  Per pass scenes.blend_table hands out
        scale_table's rows and, in place of an owned rectangle, each group's FULL footprint; batches of G = max(1, batch // K) groups
        go through pool.affine_batch and the same forward plan / captured graph, and one rua_scene_accumulate_blend per batch adds
        (wy wx v + 32768) >> 16 of the K views' sum v under the footprint's linear taper (scenes.blend_weight, out of 256, flat
        towards the scene's border, never below 16) with integer atomics - scenes.host_accumulate_blend is the definition, and the
        sums do not depend on the order.  The last batch of a pass is padded with groups whose rectangle is empty; one
        rua_scene_argmax follows, erode and boundary score its map; on_batch(rows7, foot, p).  scenes.check_blend_budget keeps the
        int32 sums in range (K times the footprints over one pixel, summed over the passes, below 32768).  ValueError, before any
        GPU work, for another value, over the budget, and with heads (blended maps of the other heads are not built).
        sieve: None is every path and return value above, call for call.  Otherwise a minimum mapping unit for the finished map: a
        minimum area in pixels, or a dict {min_area, mode="fill", connectivity=4, classes=None, rounds=1} (scenes.check_sieve;
        scenes.host_sieve is the definition).  After the window loop or rua_scene_argmax, on the compute stream, rua_scene_regions
        labels the connected regions of the map and rua_scene_sieve removes those of fewer than min_area pixels - "fill" gives each
        the class most of its kept 4-neighbours have, "void" turns them into 255, which no score counts (the reference's area
        opening) - `rounds` times, from one resident map into a second and back; one rua_scene_erode call at radius 0 then counts the
        sieved map into a fresh matrix.  The returned prediction, the confusion matrix, the matrix on the eroded ground truth and the
        boundary counts are those of the SIEVED map, and a region report is inserted in the tuple in front of the head maps:
        {"confusion_raw": the matrix of the un-sieved map (None without class maps), "counts": int64 [C][3], per class the regions
        of the un-sieved map, the small ones among them and their pixels (scenes.host_region_counts), "changed": the bytes changed,
        summed over the rounds}, fetched once at the end.  It works under any views, scales, blend, erode, boundary and heads, and
        on a pool without class maps (only the scores need them).  ValueError, before any GPU work, for a malformed `sieve`.
        sweep: None is every path and return value above, call for call.  Otherwise the precision-recall sweep of one class's
        probabilities (the reference's second protocol, matrics_AA_recall): a class index, or a dict {positive, thresholds=None,
        min_area=1, connectivity=4, opened=False} (scenes.sweep_params; thresholds as scenes.sweep_levels takes them).  The seg head's
        uint8 [H][W][C] map is stitched as heads=("seg",) stitches it, whether or not the caller asked for it (it is returned only if
        asked for).  After the window loop, on the compute stream, rua_scene_area_open builds the opened map of channel `positive`
        of that resident map, read where it lies (min_area > 1, or opened=True: scenes.host_area_open is the definition), and
        rua_scene_sweep_hist counts probabilities and opened bytes against the pool's class map into a zeroed int64 [2][2][256]
        histogram (scenes.host_sweep_hist; min_area 1 opens nothing, hist[1] is hist[0]).  A report {"hist", "levels": uint8 [T],
        "opened": uint8 [H][W] or None} is added after the sieve report and in front of the head maps, fetched once at the end;
        scenes.sweep_scores(hist, levels) is the curve.  The sweep reads probabilities, not the sieved class map; it composes with
        views, erode, boundary, sieve and heads.  ValueError, before any GPU work, for a malformed `sweep`, a pool without class
        maps, and with scales or blend (the probabilities then live in an int32 accumulator: no maps of the heads are built).
        instances: None is every path and return value above, call for call.  Otherwise the objects of the finished map: a class
        index, a list of classes, or a dict {classes, bound_below=128, dist_at_least=0, min_seed=1, radius=4, connectivity=4,
        iou_percent=(50, 55 .. 95), max_instances=2^20, map=False, outlines=False, flood=None} (scenes.instance_params; the two
        thresholds are byte levels, or floats in 0..1 that are quantised as the maps are).  The "bound" map is stitched when
        bound_below < 256 and the "dist" map when dist_at_least > 0, as heads= stitches them, whether or not the caller asked for
        them (they are returned only if asked for).  After the sieve - the instances are those of the SIEVED map when sieve= is given
        - and before any fetch, on the compute stream: rua_scene_seed_map keeps the pixels of the chosen classes that lie off the
        predicted boundaries and deep enough in the distance map, rua_scene_regions labels that marker and rua_scene_instances
        numbers the seeds and grows them back over their class within `radius` pixels (scenes.host_seed_map and
        scenes.host_instances are the definitions).  On a pool with class maps the same three calls, without head maps and at radius
        0, turn the pool's class map into the true objects - the connected regions of the chosen classes - and
        rua_scene_instance_match finds for every predicted instance the object that holds more than half of it
        (scenes.host_instance_match).  A report {"n", "ungrown", "table": int32 [n][8] (scenes.TABLE_COLUMNS), "inst": int32 [H][W]
        (only with map=True), "gt_n", "gt_table", "match": int32 [n][2], "scores": scenes.instance_scores at iou_percent} is added
        after the sweep report and in front of the head maps, fetched once at the end; the last four entries are None without class
        maps.  With flood=True or a dict {rounds_per_level=1, floor=0, drain=0} (scenes.flood_params) the grown instances of the
        PREDICTION are flooded over their class before the match and the outlines read them - rua_scene_flood, scenes.host_flood the
        definition; the ground truth is untouched.  On a multitask model without scales= and blend= the distance map is stitched,
        asked for or not, and is the per-class height; elsewhere the flood runs without a height.  "ungrown", "table" and "inst" are
        then the flooded ones and the report gains "flood": {"height": "dist" | None, "rounds", "settled", "last_round"}.  With
        outlines=True the report gains "outlines" and "outlines_true", each a (rings int32 [R][6], verts int32 [V][2]) pair
        (scenes.host_outlines; outline_polygons and write_geojson turn them into a vector layer): rua_scene_outline_count and
        rua_scene_outline_rings trace the predicted instance map, and the true objects' map on a pool with class maps (None
        without), where they lie, after everything else was issued - only rings and vertices leave the GPU.  Without the key the
        calls are what they were.  ValueError, before any GPU work, for a malformed value, a head threshold on a single-task model
        (give bound_below=256 there: with both head tests off only the class map is read, and it works everywhere) and a head
        threshold together with scales or blend (no maps of the heads are built there); ValueError after the fetch if the scene
        holds more than max_instances seeds or objects."""
        H, W, _ = self.cfg.input_shape
        Cn = self.cfg.num_classes
        if instances is not None:
            instances = instance_params(instances, Cn)
            inst_heads = (("bound",) if instances["bound_below"] < 256 else ()) + (("dist",) if instances["dist_at_least"] > 0 else ())
            if inst_heads and not self.cfg.multitasking:
                raise ValueError(f"predict_scene(instances=): this model has no {inst_heads[0]!r} head; give bound_below=256 and dist_at_least=0")
            if inst_heads and (blend is not None or (scales is not None and check_scales(scales, (H, W)) is not None)):
                raise ValueError("predict_scene(instances=) with a head threshold and scales or blend: maps of the heads are not built there; "
                                 "give bound_below=256 and dist_at_least=0, or one of the two")
        if sieve is not None:
            sieve = sieve_params(sieve, Cn)
        if sweep is not None:
            sweep = sweep_params(sweep, Cn)
            if pool.cls_ptrs is None:
                raise ValueError("predict_scene(sweep=) needs the pool's class maps: there is no ground truth to count against")
        views = check_views(views, (H, W))
        erode = check_radius(erode)
        heads = self._check_map_heads(heads, norm_type)
        boundary = check_tolerance(boundary)
        if scales is not None:
            if not 0 <= int(scene) < len(pool):
                raise ValueError(f"scene {scene} outside 0..{len(pool) - 1}")
            scales = check_scales(scales, (H, W), pool.shapes[int(scene)])           # None for (1.0,): the single-scale path
            if scales is not None and heads:
                raise ValueError(f"predict_scene(scales=, heads={heads}): multi-scale maps of the heads are not built; give one of the two")
            if scales is not None and sweep is not None:
                raise ValueError("predict_scene(scales=, sweep=): multi-scale maps of the heads are not built; give one of the two")
        if blend is not None:
            if not isinstance(blend, str) or blend not in BLEND_MODES:
                raise ValueError(f"blend {blend!r}: None or one of {BLEND_MODES}")
            if heads:
                raise ValueError(f"predict_scene(blend=, heads={heads}): blended maps of the heads are not built; give one of the two")
            if sweep is not None:
                raise ValueError("predict_scene(blend=, sweep=): blended maps of the heads are not built; give one of the two")
            if not 0 <= int(scene) < len(pool):
                raise ValueError(f"scene {scene} outside 0..{len(pool) - 1}")
            if scales is None:
                scales = ((H, W),)                                                   # one pass, the patch its footprint
            if stride is None:
                stride = (max(1, H // 2), max(1, W // 2))
        if erode and pool.cls_ptrs is None:
            raise ValueError(f"predict_scene(erode={erode}) needs the pool's class maps: there is no ground truth to erode")
        if boundary is not None and pool.cls_ptrs is None:
            raise ValueError(f"predict_scene(boundary={boundary}) needs the pool's class maps: there are no true boundaries to match")
        if isinstance(batch, bool) or not isinstance(batch, (int, np.integer)) or batch < 1:
            raise ValueError(f"batch {batch!r} must be a positive integer")
        if pool.patch is None or tuple(pool.patch) != (H, W):
            raise ValueError(f"the scene pool's patch is {pool.patch}, the model's input {H} x {W}")
        rows, own = pool.predict_table(scene, stride)
        if blend is not None:
            check_blend_budget(pool.shapes[int(scene)], (H, W), scales, stride, len(views))
        self._check_scene(pool.batch(rows[:1]), None, norm_type, with_labels=False)
        K = len(views)
        tta = views != (0,)
        G = max(1, int(batch) // K) if tta else int(batch)          # windows per forward
        B, SH, SW = G * K, *pool.shapes[int(scene)]
        g = self.graph(B, False)
        seg = g.outputs["seg"]["p"]
        pred = torch.empty((SH, SW), dtype=torch.uint8, device=self.dev)
        counted = pool.cls_ptrs is not None
        conf = torch.zeros((Cn, Cn), dtype=torch.int64, device=self.dev) if counted else None
        # rua_scene_stitch addresses scenes through host arrays of device pointers, like the pool's own: here one scene, index 0
        sc = int(scene)
        pred_ptr, cls_ptr = (C.c_void_p * 1)(pred.data_ptr()), (C.c_void_p * 1)(pool.cls_dev[sc].data_ptr()) if counted else None
        sh, sw = (C.c_int32 * 1)(SH), (C.c_int32 * 1)(SW)
        # one resident map per requested head: (source tensor, channels, mode, map, its one-entry pointer array)
        head_maps = {}
        extra = ("seg",) if sweep is not None and "seg" not in heads else ()                  # the sweep reads the seg map, asked for or not
        if instances is not None:
            extra += tuple(h for h in inst_heads if h not in heads)                           # ... and the seed map the head maps it tests
            flood = instances.get("flood")
            flood_dist = flood is not None and self.cfg.multitasking and scales is None       # blend= sets scales: no head maps there
            if flood_dist and "dist" not in heads + extra:
                extra += ("dist",)                                                            # ... and the flood its height
        for h in heads + extra:
            src = g.outputs["color" if h == "color_rgb" else h]["p"]
            m = torch.zeros((SH, SW, src.C), dtype=torch.uint8, device=self.dev)
            head_maps[h] = (src, src.C, 1 if h == "color_rgb" else 0, m, (C.c_void_p * 1)(m.data_ptr()))
        nothing = np.zeros((1, 4), np.int32)
        if scales is not None:
            if stride is None:
                stride = (H, W)
            table, entry = (scale_table, "rua_scene_accumulate") if blend is None else (blend_table, "rua_scene_accumulate_blend")
            acc = torch.zeros((SH, SW, Cn), dtype=torch.int32, device=self.dev)
            acc_ptr = (C.c_void_p * 1)(acc.data_ptr())
            for fp in scales:
                rows7, own7 = table((SH, SW), (H, W), fp, stride, views)
                rows7[:, 0] = sc
                for g0 in range(0, len(own7), G):
                    r, o = rows7[g0 * K:(g0 + G) * K], own7[g0:g0 + G]
                    if len(o) < G:
                        r = np.concatenate([r, np.tile(r[-K:], (G - len(o), 1))])
                        o = np.concatenate([o, np.repeat(nothing, G - len(o), 0)])
                    r, o = np.ascontiguousarray(r, dtype=np.int32), np.ascontiguousarray(o, dtype=np.int32)
                    self._upload_scene(g, pool.affine_batch(r), norm_type, with_labels=False)
                    self._forward_eval(g)
                    r0 = r.copy()
                    r0[:, 0] = 0
                    L.lib().call(entry, seg.ptr, G, K, H, W, Cn, r0.ctypes.data, o.ctypes.data, acc_ptr, sh, sw, 1,
                                 C.c_void_p(self._stream()))
                    if on_batch is not None:
                        on_batch(r, o, seg.t)
            L.lib().call("rua_scene_argmax", acc_ptr, pred_ptr, cls_ptr, sh, sw, 1, Cn, conf.data_ptr() if counted else None,
                         C.c_void_p(self._stream()))
        for k0 in range(0, len(rows), G) if scales is None else ():       # the single-scale window loop
            r, o = rows[k0:k0 + G], own[k0:k0 + G]
            if len(r) < G:
                r = np.concatenate([r, np.repeat(r[-1:], G - len(r), 0)])
                o = np.concatenate([o, np.repeat(nothing, G - len(o), 0)])
            if tta:
                r = view_rows(r, views)
            r, o = np.ascontiguousarray(r, dtype=np.int32), np.ascontiguousarray(o, dtype=np.int32)
            self._upload_scene(g, pool.batch(r), norm_type, with_labels=False)
            self._forward_eval(g)
            r0 = r.copy()
            r0[:, 0] = 0
            if tta:
                L.lib().call("rua_scene_stitch_views", seg.ptr, G, K, H, W, Cn, r0.ctypes.data, o.ctypes.data, pred_ptr, cls_ptr, sh, sw, 1,
                             conf.data_ptr() if counted else None, C.c_void_p(self._stream()))
            else:
                L.lib().call("rua_scene_stitch", seg.ptr, B, H, W, Cn, r0.ctypes.data, o.ctypes.data, pred_ptr, cls_ptr, sh, sw, 1,
                             conf.data_ptr() if counted else None, C.c_void_p(self._stream()))
            for src, ch, mode, _, ptr in head_maps.values():
                L.lib().call("rua_scene_stitch_maps", src.ptr, G, K, H, W, ch, r0.ctypes.data, o.ctypes.data, ptr, sh, sw, 1, mode,
                             C.c_void_p(self._stream()))
            if on_batch is not None:
                on_batch(r, o, seg.t)
            if on_heads is not None:
                on_heads(r, o, {h: head_maps[h][0].t for h in heads})
        if sieve is not None:
            # the stitched map is sieved before anything scores it: regions, then sieve, round after round between two resident maps
            mn, _, mode, conn, mask, rounds = sieve
            st = C.c_void_p(self._stream())
            conf_raw = conf
            labels, areas = (torch.empty((SH, SW), dtype=torch.int32, device=self.dev) for _ in range(2))
            lab_ptr, area_ptr = (C.c_void_p * 1)(labels.data_ptr()), (C.c_void_p * 1)(areas.data_ptr())
            rcounts = torch.zeros((Cn, 3), dtype=torch.int64, device=self.dev)
            changed = torch.zeros((1,), dtype=torch.int64, device=self.dev)
            nwork = int(L.lib().raw("rua_scene_sieve_work_bytes")(SH, SW, Cn)) if mode == 1 else 0
            work = torch.empty((nwork // 4,), dtype=torch.int32, device=self.dev) if nwork else None
            other = torch.empty_like(pred)
            for k in range(rounds):
                src_ptr, dst_ptr = (C.c_void_p * 1)(pred.data_ptr()), (C.c_void_p * 1)(other.data_ptr())
                L.lib().call("rua_scene_regions", src_ptr, sh, sw, 1, conn, lab_ptr, area_ptr, mn, Cn, rcounts.data_ptr() if k == 0 else None, st)
                L.lib().call("rua_scene_sieve", src_ptr, sh, sw, 1, conn, mn, Cn, mask, mode, lab_ptr, area_ptr, dst_ptr,
                             work.data_ptr() if nwork else None, nwork, changed.data_ptr(), st)
                pred, other = other, pred
            pred_ptr = (C.c_void_p * 1)(pred.data_ptr())
            if counted:
                conf = torch.zeros((Cn, Cn), dtype=torch.int64, device=self.dev)
                L.lib().call("rua_scene_erode", cls_ptr, sh, sw, 1, 0, None, pred_ptr, Cn, conf.data_ptr(), st)
        if sweep is not None:
            # the sweep reads the stitched probabilities of one class where they lie: channel `positive` of the seg map
            positive, levels, mn, conn, want_opened = sweep
            st = C.c_void_p(self._stream())
            _, seg_ch, _, seg_map, _ = head_maps["seg"]
            prob_ptr = (C.c_void_p * 1)(seg_map.data_ptr() + positive)
            shist = torch.zeros((2, 2, 256), dtype=torch.int64, device=self.dev)
            opened = torch.empty((SH, SW), dtype=torch.uint8, device=self.dev) if mn > 1 or want_opened else None
            open_ptr = (C.c_void_p * 1)(opened.data_ptr()) if opened is not None else None
            if opened is not None:
                slab, sarea = (torch.empty((SH, SW), dtype=torch.int32, device=self.dev) for _ in range(2)) if mn > 1 else (None, None)
                L.lib().call("rua_scene_area_open", prob_ptr, sh, sw, 1, seg_ch, levels.ctypes.data, len(levels), mn, conn, open_ptr,
                             (C.c_void_p * 1)(slab.data_ptr()) if mn > 1 else None, (C.c_void_p * 1)(sarea.data_ptr()) if mn > 1 else None, st)
            L.lib().call("rua_scene_sweep_hist", prob_ptr, open_ptr if mn > 1 else None, (C.c_void_p * 1)(pool.cls_dev[sc].data_ptr()), sh, sw, 1,
                         seg_ch, positive, Cn, shist.data_ptr(), st)
        if instances is not None:
            # seeds, regions, grow - and the same on the ground truth, then the match: all resident, nothing fetched yet
            ip, st, inst_keep = instances, C.c_void_p(self._stream()), []
            cap = min(ip["max_instances"], SH * SW)
            head_ptr = lambda h: head_maps[h][3].data_ptr() if h in inst_heads else None
            inst_p, table_p, n_p = pool._device_instances(pred.data_ptr(), head_ptr("bound"), head_ptr("dist"), (SH, SW), Cn, ip["mask"],
                                                          ip["bound_below"], ip["dist_at_least"], ip["min_seed"], ip["radius"], ip["connectivity"],
                                                          cap, st, inst_keep)
            if flood is not None:
                # the grown instances flood down the distance map, in place, before anything reads them
                fstats = pool._device_flood(pred.data_ptr(), head_maps["dist"][3].data_ptr() if flood_dist else None,
                                            head_maps["dist"][1] if flood_dist else 1, 1 if flood_dist else 0, (SH, SW), Cn, ip["mask"],
                                            ip["connectivity"], flood, inst_p, table_p, cap, n_p, st, inst_keep)
            if counted:
                inst_g, table_g, n_g = pool._device_instances(pool.cls_dev[sc].data_ptr(), None, None, (SH, SW), Cn, ip["mask"], 256, 0, 1, 0,
                                                              ip["connectivity"], cap, st, inst_keep)
                imatch = pool._device_match(inst_p, table_p, inst_g, cap, (SH, SW), st, inst_keep)
        # what scores the stitched map is issued first, kernel after kernel on the compute stream; every fetch comes after
        if boundary is not None:
            bcounts = torch.zeros((Cn, 4), dtype=torch.int64, device=self.dev)
            L.lib().call("rua_scene_boundary", cls_ptr, pred_ptr, sh, sw, 1, boundary, Cn, None, None, bcounts.data_ptr(), C.c_void_p(self._stream()))
        if erode:
            conf_e = torch.zeros((Cn, Cn), dtype=torch.int64, device=self.dev)
            L.lib().call("rua_scene_erode", cls_ptr, sh, sw, 1, erode, None, pred_ptr, Cn, conf_e.data_ptr(), C.c_void_p(self._stream()))
        more = ({h: head_maps[h][3].cpu().numpy() for h in heads},) if heads else ()
        if instances is not None:
            N, ungrown = (int(v) for v in n_p.cpu().numpy())
            if N > cap:
                raise ValueError(f"rua_scene_instances: the scene holds {N} seeds, max_instances is {ip['max_instances']}")
            report = {"n": N, "ungrown": ungrown, "table": table_p[:N].cpu().numpy(), "gt_n": None, "gt_table": None, "match": None, "scores": None}
            if flood is not None:
                settled, last = (int(v) for v in fstats.cpu().numpy())
                report["flood"] = {"height": "dist" if flood_dist else None, "rounds": flood["rounds"], "settled": settled, "last_round": last}
            if ip["map"]:
                report["inst"] = inst_p.cpu().numpy()
            if counted:
                Ng = int(n_g.cpu().numpy()[0])
                if Ng > cap:
                    raise ValueError(f"rua_scene_instances: the class map holds {Ng} objects, max_instances is {ip['max_instances']}")
                report.update(gt_n=Ng, gt_table=table_g[:Ng].cpu().numpy(), match=imatch[:N].cpu().numpy())
                report["scores"] = instance_scores(report["table"], report["gt_table"], report["match"], Cn, ip["iou_percent"])
            if ip.get("outlines"):
                # the instance maps are traced where they lie; each costs one fetch of 16 bytes between its two calls, so they come last
                report["outlines"] = pool._device_outlines(inst_p, (SH, SW), ip["connectivity"], st)
                report["outlines_true"] = pool._device_outlines(inst_g, (SH, SW), ip["connectivity"], st) if counted else None
            more = (report,) + more
        if sweep is not None:
            more = ({"hist": shist.cpu().numpy(), "levels": levels, "opened": opened.cpu().numpy() if want_opened else None},) + more
        if sieve is not None:
            more = ({"confusion_raw": conf_raw.cpu().numpy() if counted else None, "counts": rcounts.cpu().numpy(),
                     "changed": int(changed.cpu().numpy()[0])},) + more
        if boundary is not None:
            more = (bcounts.cpu().numpy(),) + more
        if erode:
            more = (conf_e.cpu().numpy(),) + more
        return (pred.cpu().numpy(), (conf.cpu().numpy() if counted else None)) + more

    def _check_map_heads(self, heads, norm_type) -> Tuple[str, ...]:
        """predict_scene's heads as a tuple of distinct names out of scenes.MAP_HEADS that this model and norm_type can give."""
        if isinstance(heads, str):
            heads = (heads,)
        try:
            heads = tuple(heads)
        except TypeError:
            raise ValueError(f"heads {heads!r}: a tuple out of {MAP_HEADS}") from None
        have = ("seg", "bound", "dist", "color") if self.cfg.multitasking else ("seg",)
        for k, h in enumerate(heads):
            if h not in MAP_HEADS:
                raise ValueError(f"heads: {h!r} is not one of {MAP_HEADS}")
            if h in heads[:k]:
                raise ValueError(f"heads {heads}: {h!r} occurs twice")
            if ("color" if h == "color_rgb" else h) not in have:
                raise ValueError(f"heads: this model has no {h!r} head (it has {have})")
            if h == "color_rgb" and norm_type != 1:
                raise ValueError(f"heads: 'color_rgb' needs norm_type 1: under norm_type {norm_type!r} the colour head's target is not HSV / (179, 255, 255)")
        return heads

    def logits(self, training: bool, batch: int) -> Dict[str, np.ndarray]:
        g = self.graph(batch, training)
        return {h["name"]: h["z"].t.cpu().numpy() for h in g.heads}
