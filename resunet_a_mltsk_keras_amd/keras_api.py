"""Drop-in Python surface of the reference's training path, backed by the HIP engine.

Mirrors exactly what the reference's callers touch:
  * `Resunet_a(input_shape, num_classes, args, inputs=None).model`      ResUnet_a/model.py:6-12, model2.py:6-12
  * Keras-Model duck type: summary / compile / train_on_batch / test_on_batch / predict / save / output_names /
    optimizer.lr                                                          train_ISPRS.py:95,131,148,167,186,292,445-461,478-480
  * `Adam(lr=, beta_1=)`, `SGD(lr=, momentum=)`, `K.get_value/set_value`, `load_model`          utils.py imports, train_ISPRS.py:404-407,474
  * loss factories `Tanimoto_dual_loss()` and `weighted_categorical_crossentropy(weights)`     multitasking_utils.py:71-85, utils.py:466-491
x / y cross this boundary as host numpy float32 NHWC arrays (dict of arrays for the multitask heads), like in
the reference, or as a compact batch - uint8 image [B,H,W,Cin] and integer class map [B,H,W] - whose float input and targets
are built on the GPU (rua_multitask_targets).  Everything numerical runs in librua_hip.so; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import json
import os
from typing import Dict, List, Optional

import numpy as np
import torch

from . import _lib as L
from . import losses as LS
from .engine import HEADS, Engine, LossSpec, ModelConfig
from .scenes import SceneBatch


# ---- optimizers / backend shims -------------------------------------------------------------------
class _Var:
    """Stands in for a Keras backend variable (optimizer.lr)."""

    def __init__(self, v):
        self.value = float(v)

    def numpy(self):
        return self.value

    def __float__(self):
        return self.value


class _SchedVar(_Var):
    """optimizer.lr under a learning-rate schedule: K.get_value gives schedules.host_lr at the engine's step counter (step 0 before the
    optimizer is compiled into a model); K.set_value raises, as Keras does for an optimizer built with a schedule."""

    def __init__(self, schedule):
        self.schedule = schedule
        self.engine = None

    @property
    def value(self):
        from .schedules import host_lr
        return host_lr(self.schedule, self.engine.t if self.engine is not None else 0)

    @value.setter
    def value(self, x):
        raise TypeError("this optimizer was created with a learning-rate schedule as its learning_rate, hence its learning rate is not settable")


def _lr_var(learning_rate, lr, default):
    from .schedules import LearningRateSchedule
    v = learning_rate if learning_rate is not None else (lr if lr is not None else default)
    return _SchedVar(v) if isinstance(v, LearningRateSchedule) else _Var(v)


class _ClipOptions:
    """Keras' clipnorm / global_clipnorm / clipvalue / weight_decay (clip.py has the definitions) and this package's skip_nonfinite, shared by
    Adam and SGD: at most one clip option, each positive; exclude_from_weight_decay takes substrings of variable names, as Keras does.
    Also the two optimizers' share of the learning-rate schedule and of use_ema / ema_momentum / ema_overwrite_frequency (schedules.py)."""

    def _set_clip(self, clipnorm, global_clipnorm, clipvalue, weight_decay, skip_nonfinite):
        from .clip import check_options
        check_options(clipnorm, global_clipnorm, clipvalue, weight_decay)
        self.clipnorm, self.global_clipnorm, self.clipvalue = clipnorm, global_clipnorm, clipvalue
        self.weight_decay, self.skip_nonfinite = weight_decay, bool(skip_nonfinite)
        self.decay_exclude: List[str] = []

    def _set_ema(self, use_ema, ema_momentum, ema_overwrite_frequency):
        """Keras' use_ema / ema_momentum / ema_overwrite_frequency (schedules.py has the definition), validated as Keras validates them."""
        from .schedules import check_ema_options
        check_ema_options(use_ema, ema_momentum, ema_overwrite_frequency)
        self.use_ema, self.ema_momentum, self.ema_overwrite_frequency = bool(use_ema), float(ema_momentum), ema_overwrite_frequency
        self._model = None

    def _set_accum(self, gradient_accumulation_steps):
        """Keras 3's gradient_accumulation_steps (accum.py has the definition): None or an integer >= 2, checked as Keras checks it."""
        from .accum import check_steps
        self.gradient_accumulation_steps = check_steps(gradient_accumulation_steps)

    def accum_options(self):
        return dict(gradient_accumulation_steps=self.gradient_accumulation_steps)

    @property
    def lr_schedule(self):
        return self.lr.schedule if isinstance(self.lr, _SchedVar) else None

    def sched_options(self):
        return dict(lr_schedule=self.lr_schedule, use_ema=self.use_ema, ema_momentum=self.ema_momentum,
                    ema_overwrite_frequency=self.ema_overwrite_frequency)

    def finalize_variable_values(self, var_list=None):
        """Keras' name for Model.finalize_ema: the averaged weights become the model's weights for good (use_ema only)."""
        if self._model is None:
            raise RuntimeError("finalize_variable_values: compile the optimizer into a model first")
        self._model.finalize_ema()

    def exclude_from_weight_decay(self, var_list=None, var_names=None):
        """Variables whose name contains one of var_names do not decay (call before compile).  var_list - Keras' list of variable objects -
        has no meaning here: the variables live in one flat buffer."""
        if var_list:
            raise ValueError("exclude_from_weight_decay: pass var_names (substrings of variable names); there are no variable objects to list")
        names = [var_names] if isinstance(var_names, str) else list(var_names or [])
        if not all(isinstance(n, str) and n for n in names):
            raise ValueError("exclude_from_weight_decay: var_names is a list of non-empty strings")
        self.decay_exclude = names

    def clip_options(self):
        return dict(clipnorm=self.clipnorm, global_clipnorm=self.global_clipnorm, clipvalue=self.clipvalue, weight_decay=self.weight_decay,
                    decay_exclude=list(self.decay_exclude) or None, skip_nonfinite=self.skip_nonfinite)


class Adam(_ClipOptions):
    def __init__(self, lr=None, learning_rate=None, beta_1=0.9, beta_2=0.999, epsilon=1e-7, clipnorm=None, global_clipnorm=None, clipvalue=None,
                 weight_decay=None, skip_nonfinite=False, use_ema=False, ema_momentum=0.99, ema_overwrite_frequency=None,
                 gradient_accumulation_steps=None, **_):
        self._set_clip(clipnorm, global_clipnorm, clipvalue, weight_decay, skip_nonfinite)
        self._set_accum(gradient_accumulation_steps)
        self._set_ema(use_ema, ema_momentum, ema_overwrite_frequency)
        self.lr = _lr_var(learning_rate, lr, 1e-3)
        self.learning_rate = self.lr
        self.beta_1, self.beta_2, self.epsilon, self.kind = beta_1, beta_2, epsilon, "adam"
        if abs(epsilon - 1e-7) > 1e-12:
            raise ValueError("the HIP Adam kernel is built with Keras' default epsilon 1e-7")


class Lamb(_ClipOptions):
    """Keras 3's Lamb (lamb.py has the definition): Adam's direction, each variable's step scaled by ||w|| / ||update|| on the GPU.  Every
    keyword Adam takes from _ClipOptions composes with it; epsilon is free (Adam's is built in).  Model.trust_report() shows the ratios."""

    def __init__(self, learning_rate=None, beta_1=0.9, beta_2=0.999, epsilon=1e-7, lr=None, clipnorm=None, global_clipnorm=None, clipvalue=None,
                 weight_decay=None, skip_nonfinite=False, use_ema=False, ema_momentum=0.99, ema_overwrite_frequency=None,
                 gradient_accumulation_steps=None, **_):
        from .lamb import check_options
        check_options(beta_1, beta_2, epsilon)
        self._set_clip(clipnorm, global_clipnorm, clipvalue, weight_decay, skip_nonfinite)
        self._set_accum(gradient_accumulation_steps)
        self._set_ema(use_ema, ema_momentum, ema_overwrite_frequency)
        self.lr = _lr_var(learning_rate, lr, 1e-3)
        self.learning_rate = self.lr
        self.beta_1, self.beta_2, self.epsilon, self.kind = float(beta_1), float(beta_2), float(epsilon), "lamb"


class SGD(_ClipOptions):
    def __init__(self, lr=None, learning_rate=None, momentum=0.0, nesterov=False, clipnorm=None, global_clipnorm=None, clipvalue=None,
                 weight_decay=None, skip_nonfinite=False, use_ema=False, ema_momentum=0.99, ema_overwrite_frequency=None,
                 gradient_accumulation_steps=None, **_):
        self._set_clip(clipnorm, global_clipnorm, clipvalue, weight_decay, skip_nonfinite)
        self._set_accum(gradient_accumulation_steps)
        self._set_ema(use_ema, ema_momentum, ema_overwrite_frequency)
        self.lr = _lr_var(learning_rate, lr, 1e-2)
        self.learning_rate = self.lr
        self.momentum, self.kind = momentum, "sgd"
        if nesterov:
            raise ValueError("Nesterov momentum is not part of the reference path")


class _Backend:
    """`K` as train_ISPRS.py:478-480 uses it."""

    @staticmethod
    def get_value(v):
        return float(v.value) if isinstance(v, _Var) else v

    @staticmethod
    def set_value(v, x):
        v.value = float(x)                                     # raises under a learning-rate schedule (_SchedVar)

    @staticmethod
    def epsilon():
        return 1e-7


K = _Backend()


# ---- losses ------------------------------------------------------------------------------------------
def _dev_f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


class TanimotoDualLoss:
    """Returned by Tanimoto_dual_loss(): a tag `compile` recognises; calling it evaluates the (B,) loss vector
    of multitasking_utils.py:71-85 on the GPU (rua_tanimoto_sums / rua_tanimoto_finalize)."""
    kind = L.LOSS_TANIMOTO
    __name__ = "loss"

    def __call__(self, label, pred):
        label, pred = np.asarray(label, np.float32), np.asarray(pred, np.float32)
        B, Cc = label.shape[0], label.shape[-1]
        HW = int(np.prod(label.shape[1:-1]))
        lib = L.lib()
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        p, y = _dev_f32(pred), _dev_f32(label)
        sums = torch.zeros(B * Cc * 6, dtype=torch.float64, device="cuda")
        out = torch.zeros(1, dtype=torch.float64, device="cuda")
        per = torch.zeros(B, dtype=torch.float32, device="cuda")
        lib.call("rua_tanimoto_sums", p.data_ptr(), y.data_ptr(), B, HW, Cc, sums.data_ptr(), s)
        lib.call("rua_tanimoto_finalize", sums.data_ptr(), B, HW, Cc, 1.0, out.data_ptr(), None, per.data_ptr(), s)
        return per.cpu().numpy()


def Tanimoto_dual_loss():
    return TanimotoDualLoss()


def Tanimoto_loss(label, pred):
    """multitasking_utils.py:38-68: the (B,) Tanimoto ratio with class weights 1/V^2 from the volumes of `label`
    (inf -> largest finite weight), on the GPU: the moments kernel of the training path with the arguments in the
    reference's order, finished by rua_tanimoto_ratio."""
    label, pred = np.asarray(label, np.float32), np.asarray(pred, np.float32)
    if label.shape != pred.shape:
        raise ValueError(f"label {label.shape} and pred {pred.shape} differ")
    B, Cc = label.shape[0], label.shape[-1]
    HW = int(np.prod(label.shape[1:-1]))
    lib = L.lib()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    a, b = _dev_f32(label), _dev_f32(pred)
    sums = torch.zeros(B * Cc * 6, dtype=torch.float64, device="cuda")
    out = torch.zeros(1, dtype=torch.float64, device="cuda")
    per = torch.zeros(B, dtype=torch.float32, device="cuda")
    lib.call("rua_tanimoto_sums", a.data_ptr(), b.data_ptr(), B, HW, Cc, sums.data_ptr(), s)      # p := label, y := pred
    lib.call("rua_tanimoto_ratio", sums.data_ptr(), B, Cc, out.data_ptr(), per.data_ptr(), s)
    return per.cpu().numpy()


class WeightedCategoricalCrossentropy:
    """Returned by weighted_categorical_crossentropy(weights) (utils.py:466-491); calling it gives the (B,H,W) map."""
    kind = L.LOSS_WCE
    __name__ = "loss"

    def __init__(self, weights, label_smoothing=0.0):
        self.weights = [float(w) for w in np.asarray(weights).reshape(-1)]
        self.label_smoothing = float(label_smoothing)

    def __call__(self, y_true, y_pred):
        y_true, y_pred = np.asarray(y_true, np.float32), np.asarray(y_pred, np.float32)
        Cc = y_true.shape[-1]
        if Cc != len(self.weights):
            raise ValueError(f"{len(self.weights)} class weights for {Cc} classes")
        M = int(np.prod(y_true.shape[:-1]))
        lib = L.lib()
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        p, y, w = _dev_f32(y_pred), _dev_f32(y_true), _dev_f32(self.weights + [0.0] * 8)
        out = torch.zeros(1, dtype=torch.float64, device="cuda")
        per = torch.zeros(M, dtype=torch.float32, device="cuda")
        if self.label_smoothing:
            LS.check_options(self.kind, Cc, label_smoothing=self.label_smoothing, what="weighted_categorical_crossentropy")
            lib.call("rua_pixel_loss_opts", L.LOSS_WCE, p.data_ptr(), None, y.data_ptr(), w.data_ptr(), None, C.byref(LS.to_struct(0.0, self.label_smoothing)),
                     M, Cc, out.data_ptr(), per.data_ptr(), s)
        else:
            lib.call("rua_pixel_loss", L.LOSS_WCE, p.data_ptr(), None, y.data_ptr(), w.data_ptr(), M, Cc, out.data_ptr(), per.data_ptr(), s)
        return per.cpu().numpy().reshape(y_true.shape[:-1])


def weighted_categorical_crossentropy(weights, label_smoothing=0.0):
    return WeightedCategoricalCrossentropy(weights, label_smoothing=label_smoothing)


class CategoricalCrossentropy:      # tf.keras.losses.* as train_ISPRS.py:414-416,427-428 instantiates them
    kind = L.LOSS_CE_LOGITS

    def __init__(self, label_smoothing=0.0):
        self.label_smoothing = float(label_smoothing)


class BinaryCrossentropy:
    kind = L.LOSS_BCE_LOGITS

    def __init__(self, label_smoothing=0.0):
        self.label_smoothing = float(label_smoothing)


def _focal_map(kind, y_true, y_pred, class_w, opts):
    """The (B,H,W) map of a focal loss from the GPU (rua_pixel_loss_opts)."""
    y_true, y_pred = np.asarray(y_true, np.float32), np.asarray(y_pred, np.float32)
    if y_true.shape != y_pred.shape:
        raise ValueError(f"y_true {y_true.shape} and y_pred {y_pred.shape} differ")
    Cc = y_true.shape[-1]
    M = int(np.prod(y_true.shape[:-1]))
    lib = L.lib()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p, y = _dev_f32(y_pred), _dev_f32(y_true)
    w = _dev_f32(list(class_w) + [0.0] * 8) if class_w is not None else None
    out = torch.zeros(1, dtype=torch.float64, device="cuda")
    per = torch.zeros(M, dtype=torch.float32, device="cuda")
    lib.call("rua_pixel_loss_opts", kind, p.data_ptr(), None, y.data_ptr(), w.data_ptr() if w is not None else None, None, C.byref(opts), M, Cc,
             out.data_ptr(), per.data_ptr(), s)
    return per.cpu().numpy().reshape(y_true.shape[:-1])


class CategoricalFocalCrossentropy:
    """Keras' CategoricalFocalCrossentropy on a softmax head (losses.host_categorical_focal is the definition).  alpha: Keras' scalar, or - this
    package's extension - one value per class.  Calling it gives the (B,H,W) map."""
    kind = L.LOSS_FOCAL_CE
    __name__ = "loss"

    def __init__(self, alpha=0.25, gamma=2.0, label_smoothing=0.0):
        a = np.asarray(alpha, np.float64).reshape(-1)
        self.alpha = float(a[0]) if a.size == 1 and np.ndim(alpha) == 0 else [float(v) for v in a]
        self.gamma, self.label_smoothing = float(gamma), float(label_smoothing)

    def alpha_vector(self, num_classes):
        return [self.alpha] * num_classes if isinstance(self.alpha, float) else list(self.alpha)

    def __call__(self, y_true, y_pred):
        Cc = np.shape(y_true)[-1]
        a = self.alpha_vector(Cc)
        LS.check_options(self.kind, Cc, self.gamma, a, False, self.label_smoothing, what="CategoricalFocalCrossentropy")
        return _focal_map(self.kind, y_true, y_pred, a, LS.to_struct(self.gamma, self.label_smoothing))


class BinaryFocalCrossentropy:
    """Keras' BinaryFocalCrossentropy on a sigmoid head (losses.host_binary_focal is the definition).  Calling it gives the (B,H,W) map."""
    kind = L.LOSS_FOCAL_BCE
    __name__ = "loss"

    def __init__(self, apply_class_balancing=False, alpha=0.25, gamma=2.0, label_smoothing=0.0):
        self.apply_class_balancing, self.alpha = bool(apply_class_balancing), float(alpha)
        self.gamma, self.label_smoothing = float(gamma), float(label_smoothing)

    def __call__(self, y_true, y_pred):
        LS.check_options(self.kind, np.shape(y_true)[-1], self.gamma, self.alpha, self.apply_class_balancing, self.label_smoothing, what="BinaryFocalCrossentropy")
        return _focal_map(self.kind, y_true, y_pred, None, LS.to_struct(self.gamma, self.label_smoothing, self.alpha, self.apply_class_balancing))


class MeanSquaredError:
    kind = L.LOSS_MSE


def lovasz_on_gpu(y_true, y_pred, void_mask=None, classes="present", loss_weight=1.0, want_dp=False):
    """rua_lovasz_grad on host arrays [..., C]: dict(loss, n_valid, n_cls, scale, G, loss_c[, dp]) as losses.lovasz_result gives them."""
    y_true, y_pred = np.asarray(y_true, np.float32), np.asarray(y_pred, np.float32)
    if y_true.shape != y_pred.shape:
        raise ValueError(f"y_true {y_true.shape} and y_pred {y_pred.shape} differ")
    Cc = y_true.shape[-1]
    M = int(np.prod(y_true.shape[:-1]))
    LS.check_lovasz(LS.lovasz_options(classes), what="LovaszSoftmax", num_classes=Cc)
    lib = L.lib()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p, y = _dev_f32(y_pred.reshape(-1)), _dev_f32(y_true.reshape(-1))
    vm = torch.from_numpy(np.ascontiguousarray(np.asarray(void_mask).reshape(-1) != 0, np.uint8)).to("cuda") if void_mask is not None else None
    nws = int(lib.raw("rua_lovasz_workspace_bytes")(M, Cc))
    if nws < 0:
        raise ValueError(f"LovaszSoftmax: {M} pixels x {Cc} classes is out of the kernels' range")
    ws = torch.empty(nws // 8 + 1, dtype=torch.float64, device="cuda")
    out = torch.zeros(1, dtype=torch.float64, device="cuda")
    res = torch.zeros(C.sizeof(L.LovaszResult) // 8, dtype=torch.float64, device="cuda")
    dp = torch.empty(M * Cc, dtype=torch.float32, device="cuda") if want_dp else None
    lib.call("rua_lovasz_grad", p.data_ptr(), y.data_ptr(), vm.data_ptr() if vm is not None else None, M, Cc, int(classes == "all"), float(loss_weight),
             ws.data_ptr(), nws, out.data_ptr(), dp.data_ptr() if dp is not None else None, None, res.data_ptr(), s)
    r = LS.lovasz_result(res.cpu().numpy().tobytes())
    if want_dp:
        r["dp"] = dp.cpu().numpy().reshape(y_pred.shape)
    return r


class LovaszSoftmax:
    """The Lovasz-Softmax loss (Berman, Triki, Blaschko, CVPR 2018) on the softmax 'seg' head or - per channel, the binary Lovasz loss on
    probabilities - the sigmoid 'bound' head: the Lovasz extension of the Jaccard index, the loss to fine-tune directly for mean IoU.
    classes: "present" (classes with foreground in the batch count, the paper's default) or "all".  losses.host_lovasz is the definition; the
    sort and the gradient run on the GPU (rua_lovasz_grad, rua_lovasz_dz) inside the training step.  Calling the object on (y_true, y_pred)
    returns the scalar from the GPU.  Not offered: per_image=True, the hinge form on logits, a built-in mix with cross-entropy on one head."""
    kind = L.LOSS_LOVASZ
    __name__ = "loss"

    def __init__(self, classes="present"):
        self.options = LS.lovasz_options(classes)
        LS.check_lovasz(self.options, what="LovaszSoftmax")
        self.classes = classes

    def __call__(self, y_true, y_pred):
        return lovasz_on_gpu(y_true, y_pred, classes=self.classes)["loss"]


class OnlineHardExampleMining:
    """Online hard example mining (bootstrapped cross-entropy) around any per-pixel loss object or name the package accepts: per training step
    only the head's hardest pixels contribute - the keep_ratio share of the valid pixels with the largest loss, never fewer than min_kept, and
    every pixel whose loss is at least loss_thresh (prob_thresh = p: loss_thresh = float32(-log p), mmsegmentation's OHEMPixelSampler for plain
    cross-entropy).  warmup_steps: optimizer updates over which the share falls from 1 to keep_ratio.  losses.host_ohem is the definition; the
    selection runs on the GPU (rua_ohem_select) inside the training step; evaluation reports the plain mean.  Calling the object on
    (y_true, y_pred) returns the (B,H,W) keep map (1 = kept) of that batch from the GPU, taken with the final share (no warm-up)."""

    def __init__(self, loss, keep_ratio=0.25, min_kept=0, loss_thresh=None, prob_thresh=None, warmup_steps=0):
        if loss_thresh is not None and prob_thresh is not None:
            raise ValueError("loss_thresh and prob_thresh: one of them")
        self.loss = _named_loss(loss)
        if isinstance(self.loss, OnlineHardExampleMining):
            raise ValueError("OnlineHardExampleMining does not nest")
        self.keep_ratio, self.min_kept, self.warmup_steps = float(keep_ratio), min_kept, warmup_steps
        self.loss_thresh, self.prob_thresh = loss_thresh, prob_thresh
        self.options = LS.ohem_options(LS.ohem_q16(keep_ratio), min_kept, loss_thresh, prob_thresh, warmup_steps)
        LS.check_ohem(self.options, what="OnlineHardExampleMining")

    @property
    def kind(self):
        if isinstance(self.loss, str):
            if self.loss not in _LOSS_NAMES:
                raise ValueError(f"unknown loss '{self.loss}'")
            return _LOSS_NAMES[self.loss]
        return getattr(self.loss, "kind", None)

    @property
    def weights(self):
        return getattr(self.loss, "weights", None)

    def __getattr__(self, name):                         # label_smoothing, gamma, alpha, ...: the wrapped loss's
        if name in ("loss", "options"):
            raise AttributeError(name)
        return getattr(self.loss, name)

    def __call__(self, y_true, y_pred):
        if not callable(self.loss):
            raise TypeError("the keep map needs a loss object that returns its (B,H,W) map when called")
        per = np.ascontiguousarray(self.loss(y_true, y_pred), np.float32)
        M = per.size
        lib = L.lib()
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        pp = _dev_f32(per.reshape(-1))
        nws = int(lib.raw("rua_ohem_workspace_bytes")(M))
        ws = torch.empty(nws // 8 + 1, dtype=torch.float64, device="cuda")
        drop = torch.empty(M, dtype=torch.uint8, device="cuda")
        out = torch.zeros(1, dtype=torch.float64, device="cuda")
        res = torch.zeros(C.sizeof(L.OhemResult) // 8, dtype=torch.float64, device="cuda")
        o = LS.to_ohem_struct(self.options)
        lib.call("rua_ohem_select", pp.data_ptr(), None, M, C.byref(o), None, 1.0, ws.data_ptr(), nws, drop.data_ptr(), out.data_ptr(), res.data_ptr(), s)
        return (1 - drop.cpu().numpy()).astype(np.uint8).reshape(per.shape)


_LOSS_NAMES = {"categorical_crossentropy": L.LOSS_CE_LOGITS, "binary_crossentropy": L.LOSS_BCE_LOGITS,
               "mse": L.LOSS_MSE, "mean_squared_error": L.LOSS_MSE, "tanimoto": L.LOSS_TANIMOTO,
               "categorical_focal_crossentropy": L.LOSS_FOCAL_CE, "binary_focal_crossentropy": L.LOSS_FOCAL_BCE,
               "lovasz": L.LOSS_LOVASZ, "lovasz_softmax": L.LOSS_LOVASZ}


def _named_loss(loss):
    """A focal loss given by its Keras name: the object with Keras' defaults; "lovasz" / "lovasz_softmax": LovaszSoftmax().  Other names and objects pass."""
    if isinstance(loss, str) and _LOSS_NAMES.get(loss) == L.LOSS_LOVASZ:
        return LovaszSoftmax()
    if isinstance(loss, str) and _LOSS_NAMES.get(loss) in LS.FOCAL_KINDS:
        return CategoricalFocalCrossentropy() if _LOSS_NAMES[loss] == L.LOSS_FOCAL_CE else BinaryFocalCrossentropy()
    return loss


def _loss_kind(loss, head):
    loss = _named_loss(loss)
    if isinstance(loss, str):
        if loss not in _LOSS_NAMES:
            raise ValueError(f"unknown loss '{loss}'")
        return _LOSS_NAMES[loss], None
    kind = getattr(loss, "kind", None)
    if kind is None:
        raise TypeError(f"loss for output '{head}' must come from this package's factories (got {type(loss).__name__}); "
                        "arbitrary Python loss callables cannot run on the HIP path")
    if kind == L.LOSS_CE_LOGITS and head in ("bound", "color"):
        raise ValueError("categorical cross-entropy needs a softmax head")
    if kind == L.LOSS_BCE_LOGITS and head in ("seg", "dist"):
        raise ValueError("binary cross-entropy needs a sigmoid head")
    if kind == L.LOSS_FOCAL_CE and head in ("bound", "color"):
        raise ValueError("categorical focal cross-entropy needs a softmax head")
    if kind == L.LOSS_FOCAL_BCE and head in ("seg", "dist"):
        raise ValueError("binary focal cross-entropy needs a sigmoid head")
    if kind == L.LOSS_LOVASZ and head not in LS.LOVASZ_HEADS:
        raise ValueError(f"the Lovasz loss needs binary targets: heads {', '.join(LS.LOVASZ_HEADS)} only, '{head}' has continuous ones")
    return kind, getattr(loss, "weights", None)


def _loss_head_options(loss, head, spec_opts):
    """The options a loss object carries (label_smoothing, and the focal ones) into LossSpec's per-head dicts."""
    loss = _named_loss(loss)
    e = float(getattr(loss, "label_smoothing", 0.0) or 0.0)
    if e != 0.0:
        spec_opts["label_smoothing"][head] = e
    if getattr(loss, "kind", None) in LS.FOCAL_KINDS:
        spec_opts["focal_gamma"][head] = loss.gamma
    if getattr(loss, "kind", None) == L.LOSS_FOCAL_BCE and loss.apply_class_balancing:
        spec_opts["class_balance"][head] = True
        spec_opts["focal_alpha"][head] = loss.alpha


# ---- compact batches ---------------------------------------------------------------------------------
def _is_int(a) -> bool:
    if isinstance(a, torch.Tensor):
        return not (a.dtype.is_floating_point or a.dtype.is_complex or a.dtype == torch.bool)
    return isinstance(a, np.ndarray) and np.issubdtype(a.dtype, np.integer)


def compact_batch(x, y):
    """(x, y) of the compact path - uint8 image [B,H,W,Cin], uint8 class map [B,H,W] - or None when y is not an integer array of
    shape [B,H,W] (then the batch is the float one).  A class map of a wider integer type must lie in [0, 255]."""
    if y is None or isinstance(y, dict) or getattr(y, "ndim", None) != 3 or not _is_int(y):
        return None
    is_u8 = (y.dtype == torch.uint8) if isinstance(y, torch.Tensor) else (y.dtype == np.uint8)
    if not is_u8:
        lo, hi = int(y.min()), int(y.max())
        if lo < 0 or hi > 255:
            raise ValueError(f"class map values must lie in [0, 255], got [{lo}, {hi}]")
        y = y.to(torch.uint8) if isinstance(y, torch.Tensor) else y.astype(np.uint8)
    x_u8 = (x.dtype == torch.uint8) if isinstance(x, torch.Tensor) else (isinstance(x, np.ndarray) and x.dtype == np.uint8)
    if not x_u8 or x.ndim != 4 or tuple(x.shape[:3]) != tuple(y.shape):
        raise ValueError(f"with a class map y {tuple(y.shape)}, x must be uint8 [B,H,W,Cin] of the same B, H, W "
                         f"(got {getattr(x, 'dtype', type(x))} {tuple(getattr(x, 'shape', ()))})")
    return x, y


def void_margin(ignore_void) -> Optional[int]:
    """compile(ignore_void=...) as LossSpec.ignore_void: None / False -> None (off), True -> labels.VOID_MARGIN, an int 0..16 -> itself."""
    from .labels import VOID_MARGIN
    if ignore_void is None or ignore_void is False:
        return None
    if ignore_void is True:
        return VOID_MARGIN
    if not isinstance(ignore_void, (int, np.integer)) or not 0 <= ignore_void <= 16:
        raise ValueError(f"ignore_void {ignore_void!r}: None, True (margin {VOID_MARGIN}) or a margin in 0..16")
    return int(ignore_void)


# ---- the model ---------------------------------------------------------------------------------------
class Model:
    """Keras-Model duck type over the recorded HIP plan."""

    def __init__(self, cfg: ModelConfig, dtype: str = "bf16", seed: int = 0):
        self.cfg = cfg
        self.engine = Engine(cfg, dtype=dtype, seed=seed)
        self.optimizer = None
        self.output_names = list(HEADS) if cfg.multitasking else ["softmax"]
        self.metrics_names: List[str] = []
        self._compiled = False

    # -- Keras surface ---------------------------------------------------------------------------------
    def summary(self, print_fn=print):
        ps = self.engine.params
        print_fn(f'Model: "resunet_a_{self.cfg.variant}"  (HIP/gfx950 plan, activations {self.engine.dtype})')
        print_fn("_" * 78)
        print_fn(f"{'Layer (Keras name)':38s}{'Param shape':26s}{'Param #':>12s}")
        print_fn("=" * 78)
        shown = {}
        for e in ps.entries:
            if e["kind"] == "kernel":
                k = int(round(e["taps"] ** 0.5))
                shown.setdefault(e["name"], [(k, k, e["cin_total"], e["cout"]), 0])
                shown[e["name"]][1] += e["size"]
            else:
                shown[e["name"]] = [(e["size"],), e["size"]]
        for name, (shape, n) in shown.items():
            print_fn(f"{name:38s}{str(shape):26s}{n:12d}")
        train = sum(e["size"] for e in ps.entries)
        total = ps.count()
        print_fn("=" * 78)
        print_fn(f"Total params: {total:,}\nTrainable params: {train:,}\nNon-trainable params: {total - train:,}")

    def count_params(self):
        return self.engine.count_params()

    def compile(self, optimizer=None, loss=None, loss_weights=None, metrics=None, ignore_void=None, **_):
        """ignore_void None: off.  True or a margin 0..16 (True = labels.VOID_MARGIN, 2): void pixels - a class value >= num_classes in a
        class-map or scene batch, dilated by the margin; the void_mask of a float batch - leave every head's loss, the gradients and the
        metrics.  The option is NOT stored in .h5 files: a loaded model is compiled without it, compile() again to set it.
        The optimizer's clipnorm / global_clipnorm / clipvalue / weight_decay (and exclude_from_weight_decay) / skip_nonfinite go into the
        LossSpec as they are (clip.py has the definitions; they ARE stored in .h5 files).  skip_nonfinite: a step whose gradient is not finite
        changes neither weights nor moments nor BatchNorm statistics, but still advances the step counter - it costs one t of Adam's bias
        correction.  clip_report() tells how many steps were skipped and clipped.
        A schedules.LearningRateSchedule as the optimizer's learning_rate and use_ema / ema_momentum / ema_overwrite_frequency go the same
        way (schedules.py has the definitions; stored in .h5 files, the averaged weights with them).
        gradient_accumulation_steps=K on the optimizer (accum.py has the definition): train_on_batch changes the weights on every K-th call
        only, with the mean of the K gradients; iterations, schedules and the average count those updates.  accumulation_state() tells where
        the cycle stands; the .h5 file holds the option and an open cycle.
        Losses: CategoricalFocalCrossentropy / BinaryFocalCrossentropy (or their Keras names as strings) and label_smoothing= on the
        cross-entropies go into LossSpec's per-head dicts (losses.py has the definitions; stored in .h5 files).  Focal CE's per-class alpha
        travels as the class weights: one vector per model.
        LovaszSoftmax(classes=) (or "lovasz" / "lovasz_softmax") on 'seg' and 'bound' goes into LossSpec.lovasz (stored in .h5 files); it combines
        with no OnlineHardExampleMining, label smoothing or focal option on the same head.  lovasz_report() gives the last step's class counts."""
        margin = void_margin(ignore_void)
        if optimizer is None or isinstance(optimizer, str):
            optimizer = {"adam": Adam, "sgd": SGD, "lamb": Lamb}[optimizer or "adam"]()
        self.optimizer = optimizer
        heads = HEADS if self.cfg.multitasking else ["seg"]
        kinds, cw = {}, None
        lopts = {k: {} for k in LS.OPTION_KEYS}
        mining, lovasz = {}, {}
        for h in heads:
            l = _named_loss(loss[h] if isinstance(loss, dict) else loss)
            kinds[h], w = _loss_kind(l, h)
            _loss_head_options(l, h, lopts)
            if isinstance(l, OnlineHardExampleMining):
                mining[h] = dict(l.options)
            if kinds[h] == L.LOSS_LOVASZ:
                lovasz[h] = dict((l.loss if isinstance(l, OnlineHardExampleMining) else l).options)
            if kinds[h] == L.LOSS_FOCAL_CE:                  # the per-class alpha travels as the class weights (one vector per model, as weighted CE's)
                w = l.alpha_vector(self.cfg.num_classes)
                if len(w) != self.cfg.num_classes:
                    raise ValueError(f"{len(w)} alpha values for {self.cfg.num_classes} classes")
                if cw is not None and list(cw) != list(w):
                    raise ValueError("one per-class vector per model: the weighted / focal CE heads must agree in it")
            if w is not None:
                if len(w) != self.cfg.num_classes:
                    raise ValueError(f"{len(w)} class weights for {self.cfg.num_classes} classes")
                cw = w
        weights = {h: 1.0 for h in heads}
        if loss_weights:
            weights.update({h: float(loss_weights[h]) for h in heads if h in loss_weights})
        spec = LossSpec(kind=kinds, weight=weights, class_weights=cw, optimizer=optimizer.kind, lr=optimizer.lr.value,
                        beta_1=getattr(optimizer, "beta_1", 0.9), beta_2=getattr(optimizer, "beta_2", 0.999),
                        momentum=getattr(optimizer, "momentum", 0.0), epsilon=getattr(optimizer, "epsilon", 1e-7), ignore_void=margin, **lopts, ohem=mining, lovasz=lovasz,
                        **(optimizer.clip_options() if hasattr(optimizer, "clip_options") else {}),
                        **(optimizer.sched_options() if hasattr(optimizer, "sched_options") else {}),
                        **(optimizer.accum_options() if hasattr(optimizer, "accum_options") else {}))
        self.engine.compile(spec)
        self._attach_optimizer()
        self._finish_compile()

    def _finish_compile(self, restored_optimizer_state: bool = False):
        """Shared tail of compile() and load_model(compile=True): attach data parallel when the process is one rank of a
        torch.distributed job (MirroredStrategy scope of train_ISPRS.py:347,432), name the returned metrics."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            from .dist import DataParallel
            dp = DataParallel(self.engine)                   # broadcasts rank 0's weights and BN state
            if restored_optimizer_state:
                dp.broadcast_optimizer_state()               # ... and rank 0's Adam moments / step count / weight average on resume
            else:
                self.engine.reset_ema()                      # use_ema: the average starts from the broadcast weights
        m = ["accuracy", "true_positives", "false_positives", "true_negatives", "false_negatives"]
        if self.cfg.multitasking:
            self.metrics_names = ["loss"] + [h + "_loss" for h in HEADS] + ["seg_" + x for x in m]
        else:
            self.metrics_names = ["loss"] + m
        self._compiled = True

    def clip_report(self):
        """Engine.clip_report: dict(norm, min_coef, skipped, clipped) of the last step and the counts since compile(), or None when the optimizer
        was given no clipnorm / global_clipnorm / clipvalue / weight_decay / skip_nonfinite.  Synchronises the device."""
        return self.engine.clip_report()

    def trust_report(self):
        """Engine.trust_report: dict(min_ratio, max_ratio, forced, updates, ratios={variable name: ratio}) of the last LAMB update, or None when
        the optimizer is not Lamb.  Synchronises the device."""
        return self.engine.trust_report()

    def ohem_report(self):
        """Engine.ohem_report: per mining head dict(kept - the kept share of the last training step's valid pixels -, tau, tau_key, K, n_kept,
        n_valid, q16_used, kept_sum, scale), or None when no head was compiled with OnlineHardExampleMining.  Synchronises the device."""
        return self.engine.ohem_report()

    def lovasz_report(self):
        """Engine.lovasz_report: per head on the Lovasz loss dict(n_valid, n_cls, G, loss_c, loss, scale) of the last step, or None when no head
        was compiled with LovaszSoftmax.  Synchronises the device."""
        return self.engine.lovasz_report()

    def accumulation_state(self):
        """Adam / SGD(gradient_accumulation_steps=K): dict(steps=K, micro=calls of train_on_batch since the last update, 0 .. K - 1); None with
        the option off.  An incomplete cycle at the end of an epoch carries over into the next one."""
        return self.engine.accumulation_state()

    def _attach_optimizer(self):
        """The optimizer's way back to the model: K.get_value(optimizer.lr) under a schedule reads the engine's step counter, and
        optimizer.finalize_variable_values() is Model.finalize_ema."""
        if isinstance(self.optimizer.lr, _SchedVar):
            self.optimizer.lr.engine = self.engine
        if hasattr(self.optimizer, "_model"):
            self.optimizer._model = self

    def _sync_lr(self):
        if self.engine.loss.lr_schedule is None:               # under a schedule the rate is the device's business (and set_value raises)
            self.engine.loss.lr = self.optimizer.lr.value      # K.set_value(model.optimizer.lr, ...) takes effect

    def ema_weights(self):
        """`with model.ema_weights(): ...` - the block (predict, test_on_batch, predict_scene, evaluate_scenes, save_weights) runs under the
        moving average of the weights (Adam / SGD(use_ema=True)); the trained weights are back on exit.  train_on_batch inside raises.
        BatchNorm moving statistics are not averaged."""
        return self.engine.ema_weights()

    def finalize_ema(self):
        """The averaged weights become the model's weights for good (Keras: optimizer.finalize_variable_values)."""
        self.engine.finalize_ema()

    def _local_batch(self, x, y, local_shard=False):
        """Under DP `-bs` is the GLOBAL batch (train_ISPRS.py:314,347): each rank takes its contiguous shard.
        local_shard=True: the caller already holds only this rank's shard (loader.PrefetchLoader(rank=, world=))."""
        w = self.engine.world
        if w == 1 or local_shard:
            return x, y
        import torch.distributed as dist
        r, B = dist.get_rank(), x.shape[0]
        if B % w:
            raise ValueError(f"global batch {B} not divisible by {w} replicas")
        sl = slice(r * (B // w), (r + 1) * (B // w))
        return x[sl], ({k: v[sl] for k, v in y.items()} if isinstance(y, dict) else (None if y is None else y[sl]))

    def _batch(self, x, y, norm_type, local_shard):
        """This rank's (x, y, norm_type for the engine): norm_type only for a compact batch (compact_batch), None for the float one.
        A scenes.SceneBatch (y None) is checked against the model (Engine._check_scene) and sharded by its rows: every rank holds the pool."""
        if isinstance(x, SceneBatch):
            self.engine._check_scene(x, y, norm_type)
            if self.engine.world > 1 and not local_shard:
                import torch.distributed as dist
                x = x.shard(dist.get_rank(), self.engine.world)
            return x, None, int(norm_type)
        cb = compact_batch(x, y)
        if cb is not None:
            if norm_type not in (1, 2):
                raise ValueError(f"norm_type {norm_type!r}: compact batches support 1 (/255) and 2 (/126.5)")
            x, y = cb
        x, y = self._local_batch(x, y, local_shard)
        return x, y, (int(norm_type) if cb is not None else None)

    def _void(self, x, y, void_mask, local_shard):
        """This rank's void mask (None: none), refused - before anything is uploaded or launched - where it has no meaning: a model compiled
        without ignore_void, a class-map or scene batch (those derive their own mask), a wrong shape or dtype."""
        if void_mask is None:
            return None
        cb = None if isinstance(x, SceneBatch) else compact_batch(x, y)
        self.engine._check_void(x, 1 if (cb is not None or isinstance(x, SceneBatch)) else None, void_mask)
        return self._local_batch(void_mask, None, local_shard)[0]

    def _photo(self, x, y, photo, local_shard):
        """This rank's photo table (None: none), refused - before anything is uploaded or launched - where it has no meaning: a scene
        batch (it carries its own, SceneBatch.with_photo) and a float batch (no bytes to jitter)."""
        if photo is None:
            return None
        cb = None if isinstance(x, SceneBatch) else compact_batch(x, y)
        t = self.engine._check_photo(x, 1 if cb is not None else None, photo)
        return self._local_batch(t, None, local_shard)[0]

    def train_on_batch(self, x, y=None, return_dict=False, local_shard=False, norm_type=1, void_mask=None, photo=None, paste=None, **_):
        """y an integer class map [B,H,W] (x then uint8 [B,H,W,Cin]): the compact path - x / norm_type and the targets seg, bound, dist
        and color (labels.py) are built on the GPU.  void_mask (float batches, compile(ignore_void=...)): uint8 or bool [B,H,W], non-zero =
        void; sharded like y under data parallel.  photo (compact batches): an int32 [B][16] photo table (scenes.photo_rows,
        PhotoJitter.draw) - the image is jittered on the GPU before x and the targets are built; sharded like y.  paste: refused
        (ValueError) - copy-paste takes its objects from a scene pool, so a scene batch carries the table (SceneBatch.with_paste)."""
        assert self._compiled, "compile() first"
        self.engine._check_paste(x, paste)
        self._sync_lr()
        vm = self._void(x, y, void_mask, local_shard)
        ph = self._photo(x, y, photo, local_shard)
        x, y, nt = self._batch(x, y, norm_type, local_shard)
        res = self.engine.train_step(x, y, norm_type=nt, void_mask=vm, photo=ph)
        return dict(zip(self.metrics_names, res)) if return_dict else res

    def test_on_batch(self, x, y=None, return_dict=False, local_shard=False, norm_type=1, void_mask=None, photo=None, paste=None, **_):
        assert self._compiled, "compile() first"
        self.engine._check_paste(x, paste)
        vm = self._void(x, y, void_mask, local_shard)
        ph = self._photo(x, y, photo, local_shard)
        x, y, nt = self._batch(x, y, norm_type, local_shard)
        res = self.engine.test_step(x, y, norm_type=nt, void_mask=vm, photo=ph)
        return dict(zip(self.metrics_names, res)) if return_dict else res

    def predict(self, x, batch_size=1, norm_type=None, **_):
        """norm_type None: x is cast to float32 as it is.  1 / 2: x is uint8 and divided by 255 / 126.5 on the GPU."""
        if isinstance(x, SceneBatch):                      # windows of resident scenes (images only): cut and normalised on the GPU
            self.engine._check_scene(x, None, norm_type, with_labels=False)
        elif norm_type is None:
            x = np.asarray(x, np.float32)
        else:
            if norm_type not in (1, 2):
                raise ValueError(f"norm_type {norm_type!r}: 1 (/255), 2 (/126.5) or None (x as given)")
            if not isinstance(x, torch.Tensor):
                x = np.asarray(x)
            if x.dtype != (torch.uint8 if isinstance(x, torch.Tensor) else np.uint8):
                raise ValueError(f"predict(norm_type={norm_type}) takes uint8 images, got {x.dtype}")
        if self.engine.loss is None:                      # load_model(..., compile=False) then predict (test_ISPRS.py:278,28)
            self.engine.compile(LossSpec(kind={h: L.LOSS_TANIMOTO for h in HEADS}, weight={h: 1.0 for h in HEADS}))
        outs = [self.engine.predict(x[i:i + batch_size], norm_type=norm_type) for i in range(0, x.shape[0], batch_size)]
        if self.cfg.multitasking:
            return {h: np.concatenate([o[h] for o in outs], axis=0) for h in HEADS}
        return np.concatenate(outs, axis=0)

    def predict_scene(self, pool, scene, stride=None, batch=8, norm_type=1, on_batch=None, views=(0,), erode=0, heads=(), on_heads=None,
                      boundary=None, scales=None, blend=None, sieve=None, sweep=None, instances=None):
        """Engine.predict_scene: (uint8 [H][W] class map of the pool's scene `scene`, int64 [C][C] confusion matrix [true][pred] or None
        without class maps), the windows cut, predicted and stitched on the GPU; only these two arrays come back.  views: test-time
        augmentation, a tuple of symmetry codes or a scenes.VIEW_SETS name ("none", "flips", "aug5", "all").  erode: a radius 1..16
        adds a third value, the confusion matrix on the eroded ground truth (scenes.host_erode; the ISPRS benchmark uses 3).  heads: a
        tuple out of "seg", "bound", "dist", "color", "color_rgb" adds a last value, {head: uint8 [H][W][Ch] map} - the head's output
        over the whole scene, averaged over the views and quantised on the GPU (scenes.host_stitch_maps); () adds nothing.  boundary: a
        tolerance 0..16 adds, after the matrices and before the head maps, the int64 [C][4] boundary counts of the map against the
        class map (scenes.host_boundary_counts; scenes.boundary_scores gives the boundary F1); None adds nothing.  scales: multi-scale
        test-time augmentation, a tuple of 1 to 8 distinct zooms such as (0.75, 1.0, 1.5) - the scene is covered once per zoom under
        all views and the resampled probabilities are summed on the GPU (scenes.host_accumulate, scenes.host_argmax); not together
        with heads; None or (1.0,) is the single-scale path.  blend: "linear" blends overlapping windows under a linear taper instead
        of giving each pixel to one window (scenes.host_accumulate_blend; stride None then means half the patch; not together with
        heads); None changes nothing.  sieve: a minimum area in pixels, or a dict {min_area, mode="fill" | "void", connectivity=4 | 8,
        classes=None, rounds=1}, removes the connected regions below that area from the finished map on the GPU before anything
        scores it (scenes.host_sieve); every returned score is then the sieved map's, and a report {"confusion_raw", "counts",
        "changed"} is added in front of the head maps; None changes nothing.  sweep: a class index, or a dict {positive,
        thresholds=None, min_area=1, connectivity=4 | 8, opened=False}: the precision-recall sweep of that class's stitched
        probabilities against the class map, area-opened on the GPU (scenes.host_area_open, scenes.host_sweep_hist); a report
        {"hist": int64 [2][2][256], "levels", "opened": the opened map or None} is added after the sieve report and before the head
        maps, and scenes.sweep_scores(hist, levels) is the curve; needs class maps, not together with scales or blend; None changes
        nothing.  instances: a class index, a list of classes, or a dict {classes, bound_below=128, dist_at_least=0, min_seed=1,
        radius=4, connectivity=4 | 8, iou_percent, max_instances, map=False, outlines=False, flood=None}: the objects of the
        finished (sieved) map - seeds off the predicted boundaries, grown back over their class on the GPU (scenes.host_seed_map,
        scenes.host_instances) - and, with class maps, their match against the connected regions of the ground truth
        (scenes.host_instance_match, scenes.instance_scores); a report {"n", "ungrown", "table", "inst" (with map=True), "gt_n",
        "gt_table", "match", "scores"} is added after the sweep report and before the head maps; a head threshold needs a multitask
        model and neither scales nor blend (bound_below=256 reads the class map only); outlines=True adds "outlines" and
        "outlines_true", the (rings, verts) of the predicted and the true instance map traced on the GPU (scenes.host_outlines;
        scenes.outline_polygons and scenes.write_geojson make the vector layer); flood=True or {rounds_per_level=1, floor=0,
        drain=0} floods the grown instances of the prediction over their class, down the stitched distance map on a multitask model
        without scales and blend and without a height elsewhere (scenes.host_flood), before match and outlines read them, and adds
        "flood": {"height", "rounds", "settled", "last_round"}; None changes nothing."""
        if self.engine.loss is None:                      # load_model(..., compile=False), as predict
            self.engine.compile(LossSpec(kind={h: L.LOSS_TANIMOTO for h in HEADS}, weight={h: 1.0 for h in HEADS}))
        return self.engine.predict_scene(pool, scene, stride=stride, batch=batch, norm_type=norm_type, on_batch=on_batch, views=views, erode=erode,
                                         heads=heads, on_heads=on_heads, boundary=boundary, scales=scales, blend=blend, sieve=sieve, sweep=sweep,
                                         instances=instances)

    def evaluate_scenes(self, pool, stride=None, batch_size=8, norm_type=1, views=(0,), erode=0, heads=(), boundary=None, scales=None, blend=None,
                        sieve=None, sweep=None, instances=None):
        """predict_scene of every scene of the pool: (list of uint8 class maps, the confusion matrices summed - None without class maps);
        with erode >= 1 a third value, the matrices on the eroded ground truth summed; with boundary (a tolerance 0..16) a next
        value, the int64 [C][4] boundary counts summed over the scenes; with heads a last value, the list of the scenes'
        {head: uint8 [H][W][Ch] map} dicts.  scales, blend: predict_scene's, for every scene.  sieve: predict_scene's; the maps and
        every score are then the sieved maps', and in front of the head maps comes the region report summed over the scenes
        ({"confusion_raw": None without class maps, "counts", "changed"}).  sweep: predict_scene's; after the region report comes
        {"hist": the scenes' histograms summed, "levels", "opened": the list of the scenes' opened maps, or None}.  instances:
        predict_scene's; after the sweep report comes {"scenes": the list of the scenes' reports (ids and tables are per scene),
        "scores": scenes.sum_instance_scores of their scores, None without class maps}."""
        heads = (heads,) if isinstance(heads, str) else tuple(heads)
        maps, total, total_e, total_b, head_maps, report, swept, objects = [], None, None, None, [], None, None, []
        for s in range(len(pool)):
            m, cm, *more = self.predict_scene(pool, s, stride=stride, batch=batch_size, norm_type=norm_type, views=views, erode=erode, heads=heads,
                                              boundary=boundary, scales=scales, blend=blend, sieve=sieve, sweep=sweep, instances=instances)
            maps.append(m)
            if cm is not None:
                total = cm if total is None else total + cm
            if heads:
                head_maps.append(more.pop())
            if instances is not None:
                objects.append(more.pop())
            if sweep is not None:
                r = more.pop()
                if swept is None:
                    swept = {"hist": np.zeros_like(r["hist"]), "levels": r["levels"], "opened": None if r["opened"] is None else []}
                swept["hist"] = swept["hist"] + r["hist"]
                if r["opened"] is not None:
                    swept["opened"].append(r["opened"])
            if sieve is not None:
                r = more.pop()
                report = r if report is None else {k: (None if r[k] is None else report[k] + r[k]) for k in r}
            if boundary is not None:
                b = more.pop()
                total_b = b if total_b is None else total_b + b
            if more:
                total_e = more[0] if total_e is None else total_e + more[0]
        res = (maps, total, total_e) if erode else (maps, total)
        if boundary is not None:
            res += (total_b,)
        if sieve is not None:
            res += (report,)
        if sweep is not None:
            res += (swept,)
        if instances is not None:
            from .scenes import sum_instance_scores
            scored = [r["scores"] for r in objects if r["scores"] is not None]
            res += ({"scenes": objects, "scores": sum_instance_scores(scored) if scored else None},)
        return res + (head_maps,) if heads else res

    # -- checkpoints (train_ISPRS.py:292,474-480): real HDF5 in the Keras layout, written / read by h5lite (no h5py needed) --
    def save(self, path):
        """`model.save('best_model.h5')` (train_ISPRS.py:292): an HDF5 file whose `model_weights` group is exactly what Keras'
        save_weights writes (layer_names / weight_names attributes, HWIO kernels, BN gamma, beta, moving_mean,
        moving_variance) - so Keras' `load_weights` reads it - plus this package's own metadata (root attribute
        `rua_checkpoint`: graph configuration, compile arguments, step count) and optimizer moments (`optimizer_weights`)."""
        from . import h5lite
        e = self.engine
        meta = dict(format="rua-checkpoint-2", cfg=dict(input_shape=list(self.cfg.input_shape), num_classes=self.cfg.num_classes,
                                                        multitasking=self.cfg.multitasking, variant=self.cfg.variant, width=self.cfg.width,
                                                        depth=self.cfg.depth), dtype=e.dtype, t=e.t)
        root = h5lite.Group()
        if e.loss is not None:
            sp = e.loss
            meta["loss"] = dict(kind=sp.kind, weight=sp.weight, class_weights=sp.class_weights, optimizer=sp.optimizer, lr=sp.lr,
                                beta_1=sp.beta_1, beta_2=sp.beta_2, momentum=sp.momentum, **sp.clip_options(), **sp.sched_options(), **sp.accum_options(),
                                **sp.loss_options())
            if sp.optimizer == "lamb":                       # the one optimizer whose epsilon is an option
                meta["loss"]["epsilon"] = float(sp.epsilon)
            og = root.require_group("optimizer_weights")
            og.set("rua/m:0", e.M1.cpu().numpy()); og.set("rua/v:0", e.V1.cpu().numpy())
            og.set("rua/iterations:0", np.array(e.t, np.int64))
            names = [b"rua/iterations:0", b"rua/m:0", b"rua/v:0"]
            if e.E is not None:
                if e._in_ema:
                    raise RuntimeError("save() inside ema_weights(): leave the block first (the file holds both sets of weights)")
                og.set("rua/ema:0", e.E.cpu().numpy())
                names.append(b"rua/ema:0")
            if e.A is not None:                              # gradient accumulation: an open cycle continues bit for bit after a resume
                og.set("rua/accum:0", e.A.cpu().numpy()); og.set("rua/accum_micro:0", np.array(e.micro, np.int64))
                names += [b"rua/accum:0", b"rua/accum_micro:0"]
            og.attrs["weight_names"] = np.array(names)
        root.attrs["keras_version"] = b"2.4.0"
        root.attrs["backend"] = b"tensorflow"
        root.attrs["rua_checkpoint"] = json.dumps(meta).encode("utf8")
        root.children["model_weights"] = h5lite.keras_group_from_weights(e.get_weights(), self._keras_layer_order())
        h5lite.write_h5(path, root)

    def _keras_layer_order(self):
        """The weighted layers in the order of Keras' `model.layers` (graph depth, keras_graph.py): what a topological
        `load_weights` on the TensorFlow side zips the file's `layer_names` with."""
        from . import keras_graph
        c = self.cfg
        return keras_graph.weighted_layer_order(c.input_shape[1], c.multitasking, c.variant, c.depth)

    def get_weights_dict(self) -> Dict[str, np.ndarray]:
        return self.engine.get_weights()

    def set_weights_dict(self, w: Dict[str, np.ndarray]):
        self.engine.set_weights(w)

    # -- weight exchange with the reference: Keras' own HDF5 layout (`model.save_weights('w.h5')` on the
    #    TensorFlow side, or the `model_weights` group of a full `model.save`), kernels HWIO, BN gamma / beta / moving_mean /
    #    moving_variance, layers matched by order within a type (canonical_keras_names).  `.npz` (Keras variable name ->
    #    array) stays as a second carrier.
    def save_weights(self, path):
        if str(path).endswith(".npz"):
            np.savez(path, **{k + ":0": v for k, v in self.engine.get_weights().items()})
            return
        from . import h5lite
        h5lite.write_h5(path, h5lite.keras_group_from_weights(self.engine.get_weights(), self._keras_layer_order()))

    def load_weights(self, path):
        if str(path).endswith(".npz"):
            with np.load(path) as z:
                given = {k: z[k] for k in z.files}
        else:
            from . import h5lite
            given = h5lite.keras_weights_from_group(h5lite.read_h5(path))
        self.engine.set_weights(canonical_keras_names(given, self.engine.get_weights()))
        self.engine.reset_ema()                                # a weights file holds no average: it starts again from these weights


def canonical_keras_names(given: Dict[str, np.ndarray], want: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """Maps a dict of Keras variables onto this model's names.  Keras numbers layers per process (`conv2d_85/kernel:0`
    if other models were built before), so layers are matched by their ORDER within a layer type, not by the absolute
    index; a `:0` suffix is dropped.  Any missing / extra variable or shape mismatch is an error naming the variable."""
    def split(name):
        layer, _, var = name.split(":")[0].rpartition("/")
        base, _, idx = layer.rpartition("_")
        return (base, int(idx), var) if base and idx.isdigit() else (layer, 0, var)

    def ranked(names):
        seen: Dict[str, list] = {}
        for n in names:
            b, i, _ = split(n)
            if i not in seen.setdefault(b, []):
                seen[b].append(i)
        rank = {b: {i: r for r, i in enumerate(sorted(v))} for b, v in seen.items()}
        return {(split(n)[0], rank[split(n)[0]][split(n)[1]], split(n)[2]): n for n in names}

    g, w = ranked(given), ranked(want)
    missing = [w[k] for k in w if k not in g]
    extra = [g[k] for k in g if k not in w]
    if missing or extra:
        raise ValueError(f"weights do not match the model: missing {missing[:4]}{'...' if len(missing) > 4 else ''}, "
                         f"unexpected {extra[:4]}{'...' if len(extra) > 4 else ''}")
    out = {}
    for k, name in w.items():
        a = np.asarray(given[g[k]], np.float32)
        if a.shape != want[name].shape:
            raise ValueError(f"{g[k]}: shape {a.shape}, the model's {name} is {want[name].shape}")
        out[name] = a
    return out


def _cfg_from_keras_file(root, weights, input_shape):
    """Graph configuration of a file Keras itself wrote (no `rua_checkpoint` attribute): channels / width / classes / heads /
    depth from the variable shapes (file order = Keras layer order), the graph variant (model2.py or model.py) by which
    parameter layout the variables fit, the patch size from `model_config` (InputLayer batch_input_shape) or the caller."""
    kernels = [(k, v) for k, v in weights.items() if k.split(":")[0].endswith("/kernel") and v.ndim == 4]
    if not kernels:
        raise ValueError("no convolution kernels in the file")
    stem = kernels[0][1]
    cin, width = int(stem.shape[2]), int(stem.shape[3])
    names = {k.split(":")[0] for k in weights}
    multitask = any(n.startswith(("seg3", "color")) for n in names)             # the multitask heads carry explicit layer names (model2.py:153-188)
    ncls = int(next(v for k, v in kernels if k.startswith("seg3")).shape[-1]) if multitask else int(kernels[-1][1].shape[-1])
    depth = 7 if max(int(v.shape[-1]) for _, v in kernels) >= width * 64 else 6
    if input_shape is None:
        cfgs = root.attrs.get("model_config")
        try:
            mc = json.loads(cfgs.decode("utf8") if isinstance(cfgs, bytes) else cfgs)
            shp = next(l["config"]["batch_input_shape"] for l in mc["config"]["layers"] if l["class_name"] == "InputLayer")
            input_shape = (int(shp[1]), int(shp[2]), cin)
        except Exception:
            raise ValueError("this Keras file does not say the patch size (no usable model_config): pass load_model(path, input_shape=(H, W, C))") from None
    err = None
    for variant in ("model2", "model"):
        cfg = ModelConfig(tuple(input_shape), ncls, multitask, variant, width, depth)
        ps = Engine.param_layout(cfg)
        want = ps.to_keras(np.zeros(ps.n, np.float32), np.zeros(ps.ns, np.float32))
        try:
            canonical_keras_names(weights, want)
            return cfg
        except ValueError as exc:
            err = exc
    raise ValueError(f"the variables fit neither ResUnet_a/model2.py nor ResUnet_a/model.py ({err})")


def loss_clip_options(lo: dict) -> dict:
    """The clip / decay / skip options out of a checkpoint's `loss` metadata; a file written before they existed has none of the keys: all off."""
    ex = lo.get("decay_exclude")
    return dict(clipnorm=lo.get("clipnorm"), global_clipnorm=lo.get("global_clipnorm"), clipvalue=lo.get("clipvalue"),
                weight_decay=lo.get("weight_decay"), decay_exclude=[str(x) for x in ex] if ex else None,
                skip_nonfinite=bool(lo.get("skip_nonfinite", False)))


def loss_sched_options(lo: dict) -> dict:
    """The learning-rate schedule and the EMA options out of a checkpoint's `loss` metadata; a file written before they existed has none of
    the keys: a constant rate, no average."""
    from .schedules import schedule_from_config
    q = lo.get("ema_overwrite_frequency")
    return dict(lr_schedule=schedule_from_config(lo.get("lr_schedule")), use_ema=bool(lo.get("use_ema", False)),
                ema_momentum=float(lo.get("ema_momentum", 0.99)), ema_overwrite_frequency=None if q is None else int(q))


def loss_accum_options(lo: dict) -> dict:
    """gradient_accumulation_steps out of a checkpoint's `loss` metadata; a file written before the option existed has no such key: off."""
    k = lo.get("gradient_accumulation_steps")
    return dict(gradient_accumulation_steps=None if k is None else int(k))


def load_model(path, compile=True, custom_objects=None, dtype=None, input_shape=None, weights="model", **_):
    """`load_model('best_model.h5')` (train_ISPRS.py:474, test_ISPRS.py:278).  Reads HDF5 only - nothing is unpickled, so a
    checkpoint cannot run code.  A file written by Model.save() restores graph, compile arguments and optimizer state; a file
    written by Keras itself (`model.save` / `save_weights` of the reference) is loaded as weights into a model whose
    configuration is read off the variable shapes (compile it yourself afterwards).
    weights="ema": the model's weights are the file's moving average (`optimizer_weights/rua/ema:0`, written by a model trained with
    use_ema) instead of the trained ones; a file without one is a ValueError."""
    from . import h5lite
    if weights not in ("model", "ema"):
        raise ValueError(f"weights {weights!r}: 'model' or 'ema'")
    if not h5lite.is_hdf5(path):
        raise ValueError(f"{path} is not an HDF5 file (checkpoints of this package and of Keras are HDF5; nothing else is read)")
    root = h5lite.read_h5(path)
    ema = None
    if weights == "ema":
        if "optimizer_weights" not in root or "rua/ema:0" not in root["optimizer_weights"]:
            raise ValueError(f"{path} holds no averaged weights (it was not saved by a model trained with use_ema)")
        ema = np.ascontiguousarray(root["optimizer_weights"]["rua/ema:0"], dtype=np.float32)
    weights = h5lite.keras_weights_from_group(root)
    meta_raw = root.attrs.get("rua_checkpoint")
    if meta_raw is None:
        m = Model(_cfg_from_keras_file(root, weights, input_shape), dtype=dtype or "bf16")
        m.engine.set_weights(canonical_keras_names(weights, m.engine.get_weights()))
        return m
    meta = json.loads(meta_raw.decode("utf8") if isinstance(meta_raw, bytes) else meta_raw)
    if meta.get("format") != "rua-checkpoint-2":
        raise ValueError(f"{path}: unknown checkpoint format {meta.get('format')!r}")
    c = meta["cfg"]
    cfg = ModelConfig(tuple(c["input_shape"]), c["num_classes"], c["multitasking"], c["variant"], c["width"], c["depth"])
    m = Model(cfg, dtype=dtype or meta["dtype"])
    m.engine.set_weights(canonical_keras_names(weights, m.engine.get_weights()))
    if compile and "loss" in meta:
        lo = meta["loss"]
        co = loss_clip_options(lo)
        so = loss_sched_options(lo)
        ko = {k: v for k, v in co.items() if k != "decay_exclude"}
        ko.update({k: v for k, v in so.items() if k != "lr_schedule"})
        ao = loss_accum_options(lo)
        ko.update(ao)
        rate = so["lr_schedule"] if so["lr_schedule"] is not None else lo["lr"]
        eo = {}
        if lo["optimizer"] == "lamb":
            eo = dict(epsilon=float(lo.get("epsilon", 1e-7)))
            opt = Lamb(learning_rate=rate, beta_1=lo["beta_1"], beta_2=lo["beta_2"], **eo, **ko)
        else:
            opt = Adam(lr=rate, beta_1=lo["beta_1"], beta_2=lo["beta_2"], **ko) if lo["optimizer"] == "adam" else SGD(lr=rate, momentum=lo["momentum"], **ko)
        if co["decay_exclude"]:
            opt.exclude_from_weight_decay(var_names=co["decay_exclude"])
        m.optimizer = opt
        m.engine.compile(LossSpec(kind={k: int(v) for k, v in lo["kind"].items()}, weight=lo["weight"], class_weights=lo["class_weights"],
                                  optimizer=lo["optimizer"], lr=lo["lr"], beta_1=lo["beta_1"], beta_2=lo["beta_2"], momentum=lo["momentum"], **eo, **co, **so, **ao,
                                  **LS.options_from_meta(lo)))
        m._attach_optimizer()
        og = root["optimizer_weights"]
        m.engine.M1.copy_(torch.from_numpy(np.ascontiguousarray(og["rua/m:0"]))); m.engine.V1.copy_(torch.from_numpy(np.ascontiguousarray(og["rua/v:0"])))
        m.engine.t = int(og["rua/iterations:0"])
        if m.engine.E is not None and "rua/ema:0" in og:      # a file without an average: compile() left E = P
            m.engine.E.copy_(torch.from_numpy(np.ascontiguousarray(og["rua/ema:0"])))
        if m.engine.A is not None and "rua/accum:0" in og:    # a file without an accumulator: compile() left it zero, the cycle starts over
            m.engine.A.copy_(torch.from_numpy(np.ascontiguousarray(og["rua/accum:0"], dtype=np.float32)))
            m.engine.micro, m.engine._micro_dev = int(og["rua/accum_micro:0"]), -1
        m._finish_compile(restored_optimizer_state=True)
    if ema is not None:
        if ema.shape != tuple(m.engine.P.shape):
            raise ValueError(f"{path}: the averaged weights have {ema.size} elements, the model's parameter buffer {m.engine.P.numel()}")
        m.engine.P.copy_(torch.from_numpy(ema))
        m.engine.params_changed()
    return m


class Resunet_a(object):
    """Same constructor as the reference (ResUnet_a/model2.py:6-12): builds `.model`."""
    variant = "model2"

    def __init__(self, input_shape, num_classes, args, inputs=None):
        self.num_classes = num_classes
        self.img_height, self.img_width, self.img_channel = input_shape
        self.args = args
        self.inputs = inputs
        self.model = self.build_model_ResUneta()

    def build_model_ResUneta(self):
        cfg = ModelConfig(input_shape=(self.img_height, self.img_width, self.img_channel), num_classes=self.num_classes,
                          multitasking=bool(getattr(self.args, "multitasking", False)), variant=self.variant,
                          width=int(getattr(self.args, "width", 32)), depth=int(getattr(self.args, "depth", 6)))
        return Model(cfg, dtype=getattr(self.args, "dtype", "bf16"), seed=int(getattr(self.args, "seed", 0)))


class Resunet_a_v1(Resunet_a):
    """ResUnet_a/model.py graph (no skip in the ResBlock sum, no BN on the 1x1 convs, conv-then-upsample)."""
    variant = "model"
