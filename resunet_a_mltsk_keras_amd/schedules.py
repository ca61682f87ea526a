"""Learning-rate schedules and the exponential moving average of the weights: the host definitions of what rua_lr_schedule_step and
rua_ema_step compute on the GPU (csrc/loss_optim.hip), and the Keras-shaped classes Adam / SGD take as `learning_rate`.

`host_lr(schedule, step)` in fp64 numpy IS the definition of a schedule; `step` counts the optimizer steps already taken (0 for the first
update), as Keras' `optimizer.iterations` does.  The formulas are the ones of keras.optimizers.schedules as its documentation and source
state them; no Keras is installed next to this package, so they have been compared against the text, never against a run of Keras.

`host_ema(ema, theta, momentum, t, overwrite_every)` in fp32 numpy is the definition of the weight average, Keras 3's
`use_ema` / `ema_momentum` / `ema_overwrite_frequency` with its first-step rule (the average starts as a copy of the weights).
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np

from ._lib import LrSchedule as RuaLrSchedule

f64 = np.float64
MAX_BOUNDARIES = 16                                        # RUA_SCHED_MAX_BOUNDARIES of include/rua_hip.h
KIND_CONSTANT, KIND_COSINE, KIND_EXPONENTIAL, KIND_POLYNOMIAL, KIND_PIECEWISE, KIND_INVERSE_TIME = range(6)   # RUA_SCHED_*
KIND_NAMES = ("constant", "cosine", "exponential", "polynomial", "piecewise", "inverse_time")


def _positive_int(name, v, least=1):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < least:
        raise ValueError(f"{name} {v!r}: an integer >= {least}")
    return int(v)


def _finite(name, v, least=None):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or (least is not None and v < least):
        raise ValueError(f"{name} {v!r}: a finite number" + (f" >= {least}" if least is not None else ""))
    return float(v)


class LearningRateSchedule:
    """Base of the five schedules.  Calling one gives host_lr (fp64); get_config / schedule_from_config carry it through a checkpoint."""
    kind = KIND_CONSTANT

    def __call__(self, step):
        return host_lr(self, step)

    def get_config(self) -> Dict[str, object]:
        raise NotImplementedError

    def max_rate(self) -> float:
        """The largest rate the schedule can give (the scale of the kernel tests' bound)."""
        raise NotImplementedError

    def __eq__(self, other):
        return isinstance(other, LearningRateSchedule) and self.get_config() == other.get_config()

    def __repr__(self):
        c = self.get_config()
        return f"{type(self).__name__}({', '.join(f'{k}={v!r}' for k, v in c.items() if k != 'kind')})"


class CosineDecay(LearningRateSchedule):
    """Keras' CosineDecay.  Without warmup_target:
        s = min(step, decay_steps);  lr = initial * ((1 - alpha) * 0.5 * (1 + cos(pi * s / decay_steps)) + alpha)
    With warmup_target (warmup_steps >= 0):
        step <  warmup_steps:  lr = (warmup_target - initial) * (step / warmup_steps) + initial
        otherwise:             s = min(step, warmup_steps + decay_steps) - warmup_steps
                               lr = warmup_target * ((1 - alpha) * 0.5 * (1 + cos(pi * s / decay_steps)) + alpha)"""
    kind = KIND_COSINE

    def __init__(self, initial_learning_rate, decay_steps, alpha=0.0, warmup_target=None, warmup_steps=0):
        self.initial_learning_rate = _finite("initial_learning_rate", initial_learning_rate, 0.0)
        self.decay_steps = _positive_int("decay_steps", decay_steps)
        self.alpha = _finite("alpha", alpha, 0.0)
        self.warmup_target = None if warmup_target is None else _finite("warmup_target", warmup_target, 0.0)
        self.warmup_steps = _positive_int("warmup_steps", warmup_steps, 0)

    def get_config(self):
        return dict(kind="cosine", initial_learning_rate=self.initial_learning_rate, decay_steps=self.decay_steps, alpha=self.alpha,
                    warmup_target=self.warmup_target, warmup_steps=self.warmup_steps)

    def max_rate(self):
        return max(self.initial_learning_rate, self.warmup_target or 0.0) * max(1.0, self.alpha)


class ExponentialDecay(LearningRateSchedule):
    """Keras' ExponentialDecay:  p = step / decay_steps (staircase: floor(p));  lr = initial * decay_rate ** p"""
    kind = KIND_EXPONENTIAL

    def __init__(self, initial_learning_rate, decay_steps, decay_rate, staircase=False):
        self.initial_learning_rate = _finite("initial_learning_rate", initial_learning_rate, 0.0)
        self.decay_steps = _positive_int("decay_steps", decay_steps)
        self.decay_rate = _finite("decay_rate", decay_rate, 0.0)
        self.staircase = bool(staircase)

    def get_config(self):
        return dict(kind="exponential", initial_learning_rate=self.initial_learning_rate, decay_steps=self.decay_steps, decay_rate=self.decay_rate,
                    staircase=self.staircase)

    def max_rate(self):
        return self.initial_learning_rate if self.decay_rate <= 1.0 else float("inf")


class PolynomialDecay(LearningRateSchedule):
    """Keras' PolynomialDecay.
        cycle:      d = decay_steps * (1 if step == 0 else ceil(step / decay_steps)),  s = step
        otherwise:  d = decay_steps,                                                    s = min(step, decay_steps)
        lr = (initial - end) * (1 - s / d) ** power + end"""
    kind = KIND_POLYNOMIAL

    def __init__(self, initial_learning_rate, decay_steps, end_learning_rate=1e-4, power=1.0, cycle=False):
        self.initial_learning_rate = _finite("initial_learning_rate", initial_learning_rate, 0.0)
        self.decay_steps = _positive_int("decay_steps", decay_steps)
        self.end_learning_rate = _finite("end_learning_rate", end_learning_rate, 0.0)
        self.power = _finite("power", power)
        if self.power <= 0.0:
            raise ValueError(f"power {power!r}: a positive number")
        self.cycle = bool(cycle)

    def get_config(self):
        return dict(kind="polynomial", initial_learning_rate=self.initial_learning_rate, decay_steps=self.decay_steps,
                    end_learning_rate=self.end_learning_rate, power=self.power, cycle=self.cycle)

    def max_rate(self):
        return max(self.initial_learning_rate, self.end_learning_rate)


class PiecewiseConstantDecay(LearningRateSchedule):
    """Keras' PiecewiseConstantDecay:  lr = values[i] for the first i with step <= boundaries[i], values[-1] beyond the last boundary.
    At most 16 boundaries (the table travels to the kernel by value), strictly increasing, len(values) = len(boundaries) + 1."""
    kind = KIND_PIECEWISE

    def __init__(self, boundaries, values):
        b, v = list(boundaries), list(values)
        if not 1 <= len(b) <= MAX_BOUNDARIES:
            raise ValueError(f"{len(b)} boundaries: 1 to {MAX_BOUNDARIES}")
        if len(v) != len(b) + 1:
            raise ValueError(f"{len(v)} values for {len(b)} boundaries: one more value than boundaries")
        self.boundaries = [_positive_int("boundary", x, 0) for x in b]
        if any(y <= x for x, y in zip(self.boundaries, self.boundaries[1:])):
            raise ValueError(f"boundaries {self.boundaries}: strictly increasing")
        self.values = [_finite("value", x, 0.0) for x in v]

    def get_config(self):
        return dict(kind="piecewise", boundaries=list(self.boundaries), values=list(self.values))

    def max_rate(self):
        return max(self.values)


class InverseTimeDecay(LearningRateSchedule):
    """Keras' InverseTimeDecay:  p = step / decay_steps (staircase: floor(p));  lr = initial / (1 + decay_rate * p)"""
    kind = KIND_INVERSE_TIME

    def __init__(self, initial_learning_rate, decay_steps, decay_rate, staircase=False):
        self.initial_learning_rate = _finite("initial_learning_rate", initial_learning_rate, 0.0)
        self.decay_steps = _positive_int("decay_steps", decay_steps)
        self.decay_rate = _finite("decay_rate", decay_rate, 0.0)
        self.staircase = bool(staircase)

    def get_config(self):
        return dict(kind="inverse_time", initial_learning_rate=self.initial_learning_rate, decay_steps=self.decay_steps, decay_rate=self.decay_rate,
                    staircase=self.staircase)

    def max_rate(self):
        return self.initial_learning_rate


class Constant(LearningRateSchedule):
    """lr = initial: what the step computes without a schedule, as a schedule (the kernel tests compare it with rua_lr_step's bits)."""
    kind = KIND_CONSTANT

    def __init__(self, initial_learning_rate):
        self.initial_learning_rate = _finite("initial_learning_rate", initial_learning_rate, 0.0)

    def get_config(self):
        return dict(kind="constant", initial_learning_rate=self.initial_learning_rate)

    def max_rate(self):
        return self.initial_learning_rate


_CLASSES = {"constant": Constant, "cosine": CosineDecay, "exponential": ExponentialDecay, "polynomial": PolynomialDecay,
            "piecewise": PiecewiseConstantDecay, "inverse_time": InverseTimeDecay}


def schedule_from_config(cfg: Optional[dict]) -> Optional[LearningRateSchedule]:
    """get_config()'s dict back into a schedule; None (a checkpoint without one) stays None."""
    if cfg is None:
        return None
    kw = dict(cfg)
    kind = kw.pop("kind", None)
    if kind not in _CLASSES:
        raise ValueError(f"learning-rate schedule kind {kind!r}: one of {sorted(_CLASSES)}")
    return _CLASSES[kind](**kw)


def host_lr(schedule: LearningRateSchedule, step) -> float:
    """THE definition of the rate of the optimizer step that follows `step` completed ones, in fp64 (the classes' docstrings hold the
    formulas, Keras' as its documentation states them - not checked against a run of Keras, which is not installed here)."""
    s = f64(step)
    if s < 0:
        raise ValueError(f"step {step!r}: not negative")
    k = schedule
    if isinstance(k, Constant):
        return float(f64(k.initial_learning_rate))
    if isinstance(k, CosineDecay):
        d, a = f64(k.decay_steps), f64(k.alpha)
        base = f64(k.initial_learning_rate)
        if k.warmup_target is not None:
            w, tgt = f64(k.warmup_steps), f64(k.warmup_target)
            if s < w:
                return float((tgt - base) * (s / w) + base)
            s, base = np.minimum(s, w + d) - w, tgt
        else:
            s = np.minimum(s, d)
        cosine = f64(0.5) * (f64(1.0) + np.cos(f64(np.pi) * (s / d)))
        return float(base * ((f64(1.0) - a) * cosine + a))
    if isinstance(k, ExponentialDecay):
        p = s / f64(k.decay_steps)
        if k.staircase:
            p = np.floor(p)
        return float(f64(k.initial_learning_rate) * np.power(f64(k.decay_rate), p))
    if isinstance(k, PolynomialDecay):
        d = f64(k.decay_steps)
        if k.cycle:
            d = d * (f64(1.0) if s == 0 else np.ceil(s / d))
        else:
            s = np.minimum(s, d)
        end = f64(k.end_learning_rate)
        return float((f64(k.initial_learning_rate) - end) * np.power(f64(1.0) - s / d, f64(k.power)) + end)
    if isinstance(k, PiecewiseConstantDecay):
        for b, v in zip(k.boundaries, k.values):
            if s <= b:
                return float(f64(v))
        return float(f64(k.values[-1]))
    if isinstance(k, InverseTimeDecay):
        p = s / f64(k.decay_steps)
        if k.staircase:
            p = np.floor(p)
        return float(f64(k.initial_learning_rate) / (f64(1.0) + f64(k.decay_rate) * p))
    raise TypeError(f"{schedule!r} is no learning-rate schedule of this package")


def to_struct(schedule: LearningRateSchedule) -> RuaLrSchedule:
    """The schedule as the by-value argument of rua_lr_schedule_step."""
    st = RuaLrSchedule()
    k = schedule
    st.kind = k.kind
    st.initial = float(getattr(k, "initial_learning_rate", 0.0))
    st.decay_steps = float(getattr(k, "decay_steps", 1))
    st.decay_rate = float(getattr(k, "decay_rate", 0.0))
    st.alpha = float(getattr(k, "alpha", 0.0))
    st.end = float(getattr(k, "end_learning_rate", 0.0))
    st.power = float(getattr(k, "power", 1.0))
    st.staircase = 1 if getattr(k, "staircase", False) else 0
    st.cycle = 1 if getattr(k, "cycle", False) else 0
    if getattr(k, "warmup_target", None) is not None:
        st.warmup, st.warmup_target, st.warmup_steps = 1, float(k.warmup_target), float(k.warmup_steps)
    if isinstance(k, PiecewiseConstantDecay):
        st.n_boundaries = len(k.boundaries)
        for i, b in enumerate(k.boundaries):
            st.boundaries[i] = float(b)
        for i, v in enumerate(k.values):
            st.values[i] = float(v)
    return st


# ---- exponential moving average of the weights -----------------------------------------------------------------------------------------
def check_ema_options(use_ema, ema_momentum, ema_overwrite_frequency):
    """Keras' validation: momentum in [0, 1]; the overwrite frequency None or an integer >= 1 (both only looked at when use_ema)."""
    if not use_ema:
        return
    m = ema_momentum
    if isinstance(m, bool) or not isinstance(m, (int, float, np.integer, np.floating)) or not 0.0 <= m <= 1.0:
        raise ValueError(f"ema_momentum {m!r}: a number in [0, 1]")
    q = ema_overwrite_frequency
    if q is not None and (isinstance(q, bool) or not isinstance(q, (int, np.integer)) or q < 1):
        raise ValueError(f"ema_overwrite_frequency {q!r}: None or an integer >= 1")


def host_ema(ema, theta, momentum, t, overwrite_every=0, skipped=False):
    """One rua_ema_step on the host, in fp32: returns (ema', theta').  t = optimizer steps taken INCLUDING this one.
        skipped:  nothing changes
        t == 1:   ema' = theta                                   (Keras 3's first-step rule)
        else:     ema' = m * ema + (1 - m) * theta                every operation rounded to fp32 on its own
        overwrite_every > 0 and t % overwrite_every == 0:  theta' = ema'"""
    e, th = np.asarray(ema, np.float32), np.asarray(theta, np.float32)
    if skipped:
        return e.copy(), th.copy()
    m = np.float32(momentum)
    if int(t) == 1:
        e1 = th.copy()
    else:
        e1 = (m * e + (np.float32(1.0) - m) * th).astype(np.float32)
    th1 = e1.copy() if overwrite_every and overwrite_every > 0 and int(t) % int(overwrite_every) == 0 else th.copy()
    return e1, th1
