#!/usr/bin/env python
"""Training CLI of the ResUnet-a path on MI355X — same flags, defaults and results-directory roles as the
reference's train_ISPRS.py (reference train_ISPRS.py:297-338 flags, :55-292 epoch loop, :354-380 dataset listing).

Deviations, all additive or forced by the reference's hard-coded values:
  * `--channels` (default: read from the first patch) replaces the hard-coded `channels = 3` (reference :401) and
    the label buffers take their class count from `--num_classes` instead of the hard-coded 5 (reference :491).
  * patches and labels are paired BY FILE NAME; the reference relies on os.listdir returning the same order in
    every directory (reference :354-374).
  * the default weighted-CE class weights are the reference's five values (reference :424) only when
    --num_classes is 5; otherwise uniform weights.
  * scalars go to `<results_path>/logs/{train,val}/scalars.jsonl` with the reference's TensorBoard tag names
    (tensorboard is not available); the best model is `<results_path>/best_model.h5`: real HDF5 whose `model_weights` group is
    Keras' own weight layout (plus this package's metadata and optimizer state, written without h5py by h5lite).
  * `--compact_dataset yes --norm_type {1,2}`: read the compact layout (uint8 images/ and labels/classes/, written by
    `python -m resunet_a_mltsk_keras_amd.compact`); x and the seg / bound / dist / color targets are built on the GPU.
  * `--scene_dataset yes --stride S --data_aug {yes,no}` (with `-ps`, `--norm_type`): `-dp` is a scene directory (scenes/ and
    labels/scenes/, written by `python -m resunet_a_mltsk_keras_amd.scenes`).  The scenes stay on the GPU and every step cuts and
    augments its patches there; the patch set, its split and its order are those of a `--compact_dataset yes` run on the
    directory `scenes.materialize` writes from the same arguments.
  * `--random_aug yes --aug_rotate DEG --aug_zoom LO HI --aug_shift PX` (with `--scene_dataset yes`): every training window is
    rotated by a random angle in [-DEG, DEG], zoomed by a log-uniform factor in [LO, HI] and shifted by up to PX pixels (default
    `--stride` / 2), with reflect padding at the scene border, drawn afresh every epoch from `--seed` (scenes.SceneLoader(jitter=)).
    The validation windows and the split are untouched, so validation numbers compare between runs with and without the flag.
  * `--photo_aug yes --photo_brightness V --photo_contrast LO HI --photo_saturation LO HI --photo_hue DEG --photo_tone V
    --photo_noise LO HI` (with `--scene_dataset yes`): every training window gets a random brightness offset in [-V, V] of full
    scale, a log-uniform contrast and saturation, a hue rotation in [-DEG, DEG], a tone-curve strength in [-V, V] and hashed noise
    of a sigma in [LO, HI] levels, applied to the cut uint8 window on the GPU (rua_window_photometric) before the input and the
    targets are built from it - the colour head's HSV target follows the jittered image.  Drawn afresh every epoch from `--seed`
    (scenes.SceneLoader(photo=)), in a random stream of its own: `--random_aug` draws what it draws without it.  The validation
    windows and the split are untouched.  The option is not stored in a checkpoint.
  * `--paste_aug yes --paste_classes K [K ...] [--paste_per_window LO HI] [--paste_onto SRC:DST[,DST] ...] [--paste_over_void yes]
    [--paste_min_area A] [--paste_max_area A]` (with `--scene_dataset yes`): copy-paste augmentation (Ghiasi et al., CVPR 2021).
    The ground-truth objects of the classes K - their connected regions in the class maps, found once on the GPU after the scenes
    are uploaded (ScenePool.object_bank; the bank's size per class is printed) - are pasted, pixels and labels together, into the
    cut training windows (rua_window_paste) before the photometric jitter and before the input and the targets are built, so all
    four heads follow.  Per window LO..HI pastes; per paste the class is drawn uniformly from K (a rare class is seen as often as a
    common one), then an object of it, one of the eight symmetries and a place inside the window; `--paste_onto 4:0` lets class 4
    cover class 0 only.  Drawn afresh every epoch from `--seed` in a random stream of its own (scenes.SceneLoader(paste=)).  The
    objects come from the scenes the training windows are cut from (the split is by windows, which overlap, as in the reference);
    the validation windows are never pasted into.  The id maps cost 4 bytes per scene pixel of GPU memory.  Not stored in a checkpoint.
  * `--class_weights auto` (with `--scene_dataset yes --loss weighted_cross_entropy`): the weighted-CE class weights are total /
    pixels of the class over the training windows (scenes.class_weights; the reference's five numbers are that rule on its own
    patch set), counted on the GPU from the resident class maps (ScenePool.class_counts).  `--class_weights w0 ... wC-1` gives
    them explicitly, for any layout.  Without the flag: the reference's five values at 5 classes, uniform weights otherwise.
  * `--balance_class K --balance_percent P` (with `--scene_dataset yes`): only the training windows in which class K covers at
    least P percent of the pixels are trained on (the reference's bal_aug_patches, utils.py:383, with the class a parameter;
    scenes.balance_rows).  The validation windows and the split are untouched.
  * `--clipnorm C` / `--global_clipnorm C` / `--clipvalue C` (at most one), `--weight_decay WD [--decay_all yes]`, `--skip_nonfinite yes`:
    Keras' gradient clipping and decoupled weight decay (kernels only unless --decay_all yes: names with bias / gamma / beta are
    excluded) and a guard that leaves weights, moments and BatchNorm statistics alone in a step whose gradient holds an Inf or a NaN,
    all decided on the GPU (resunet_a_mltsk_keras_amd/clip.py).  After each epoch the counts of skipped and clipped steps and the last
    gradient norm are printed.  With `-cp` the options come from the checkpoint.
  * `--lr_schedule {constant,cosine,exponential,polynomial,piecewise,inverse_time}` with `--lr_decay_steps`, `--lr_warmup_steps`,
    `--lr_warmup_target`, `--lr_alpha`, `--lr_decay_rate`, `--lr_end`, `--lr_power`, `--lr_staircase`, `--lr_cycle`, `--lr_boundaries`,
    `--lr_values`: Keras' learning-rate schedules with `-lr` as the initial rate, computed on the GPU from the device's step counter
    (resunet_a_mltsk_keras_amd/schedules.py).  The current rate is printed once per epoch.  With `-cp` the schedule comes from the
    checkpoint and continues at its iteration; `-lr` is then not applied.
  * `--ema yes --ema_momentum M --ema_overwrite_frequency N`: Keras' moving average of the weights (use_ema), updated on the GPU behind
    every optimizer step.  Each epoch's validation and the best-model criterion then run under the averaged weights; the saved file
    holds both sets (eval_scenes_ISPRS.py --weights ema evaluates the averaged one).
  * `--grad_accum K`: Keras 3's gradient_accumulation_steps - the optimizer applies the mean of K consecutive batches' gradients once every
    K batches, decided on the GPU (resunet_a_mltsk_keras_amd/accum.py).  `--lr_decay_steps`, `--lr_warmup_steps`, `--lr_boundaries` and
    `--ema_overwrite_frequency` then count updates, not batches; an incomplete cycle at the end of an epoch carries over into the next.
    The per-epoch line prints the updates taken next to the batches seen.  `--grad_accum 1` is off.  With `-cp` the option comes from
    the checkpoint, an open cycle with it.
  * `-optm lamb [--lamb_epsilon E]`: the LAMB optimizer (resunet_a_mltsk_keras_amd/lamb.py) - Adam's direction with each variable's step scaled
    by ||w|| / ||update|| on the GPU, so that one `-lr` carries across `-bs` x GPUs x `--grad_accum`.  Every option above composes with it; the
    per-epoch line prints the smallest and largest trust ratio of the last update.
  * `--loss focal` with `--focal_gamma G` (default 2; 0 or 1..8), `--focal_alpha A [A ...]` (one value or one per class, default 0.25)
    and `--bound_alpha A` (default: no class balancing): Keras' categorical focal cross-entropy on the seg head and, with
    `--multitasking yes`, the binary focal cross-entropy on the boundary head; dist and color get MSE, as with the two cross-entropy
    choices.  `--class_weights` (a list, or `auto`) is accepted with it and becomes the per-class alpha as given; with `--focal_gamma 0`
    that is weighted cross entropy.  `--label_smoothing E` smooths the targets of the cross-entropy and focal losses (not `--loss
    tanimoto`; the MSE heads take none).  All on the GPU (resunet_a_mltsk_keras_amd/losses.py); with `-cp` the loss and its options come
    from the checkpoint.
  * `--loss lovasz [--lovasz_classes present|all]`: the Lovasz-Softmax loss (the Lovasz extension of the Jaccard index; Berman, Triki,
    Blaschko, CVPR 2018) on the seg head and, with `--multitasking yes`, on the boundary head; dist and color get MSE.  The sort it needs
    runs on the GPU inside the captured step (resunet_a_mltsk_keras_amd/losses.py, csrc/lovasz.hip).  It is the loss to fine-tune for mean
    IoU: with `-cp` the checkpoint gives the weights and the optimizer's moments and step count, the command line this loss and the optimizer's settings.  `--ignore_void`
    composes; `--ohem`, `--label_smoothing` and the focal flags do not.  Not offered: per-image averaging, the hinge form on logits, a
    built-in mix with cross-entropy on one head.
  * `--ohem yes [--ohem_keep 0.25] [--ohem_min_kept N] [--ohem_thresh T | --ohem_prob P] [--ohem_warmup N] [--ohem_heads seg bound]`: online
    hard example mining (bootstrapped cross-entropy) - per step only the hardest pixels of the mining heads (default: seg) contribute to
    loss and gradient: the `--ohem_keep` share of the valid pixels, never fewer than N, and every pixel whose loss is at least T
    (`--ohem_prob P`, `--loss cross_entropy` only: T = -log P).  The exact selection runs on the GPU inside the captured step
    (resunet_a_mltsk_keras_amd/losses.py, csrc/ohem.hip); validation reports the plain mean.  Not with `--loss tanimoto`.  The per-epoch
    line prints the kept share and the threshold of the last step.
  * `--dtype {bf16,f32}`, `--seed`: engine options.  Launch with torch.distributed.run for multi-GPU data
    parallel (`-bs` is then the GLOBAL batch, as under MirroredStrategy).
"""
import argparse
import contextlib
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

REFERENCE_WCE_WEIGHTS = [4.34558461, 2.97682037, 3.92124661, 5.67350328, 374.0300152]   # reference train_ISPRS.py:424
TASKS = [("seg", "Segmentation"), ("bound", "Boundary"), ("dist", "Distance"), ("color", "Color")]


def str2bool(v):
    if isinstance(v, bool):
        return v
    s = str(v).lower()
    if s in ("yes", "true", "t", "y", "1"):
        return True
    if s in ("no", "false", "f", "n", "0"):
        return False
    raise argparse.ArgumentTypeError("Boolean value expected.")


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--resunet_a", help="choose resunet-a model or not", type=str2bool, default=False)
    p.add_argument("--multitasking", help="choose resunet-a multitasking or not", type=str2bool, default=False)
    p.add_argument("--gpu_parallel", help="choose 1 to train one multiple gpu", type=str2bool, default=False)
    p.add_argument("-rp", "--results_path", type=str, default="./results/results_run1",
                   help="Path where to save logs and model checkpoint.")
    p.add_argument("-cp", "--checkpoint_path", type=str, default=None, help="Path where to load model checkpoint to continue training")
    p.add_argument("-dp", "--dataset_path", type=str, default="./DATASETS/patch_size=256_stride=32", help="Path where to load dataset")
    p.add_argument("-bs", "--batch_size", type=int, default=4, help="Batch size on training")
    p.add_argument("-lr", "--learning_rate", type=float, default=1e-3, help="Learning rate on training")
    p.add_argument("--loss", type=str, default="weighted_cross_entropy", choices=["weighted_cross_entropy", "cross_entropy", "tanimoto", "focal", "lovasz"])
    p.add_argument("--lovasz_classes", type=str, default="present", choices=["present", "all"],
                   help="--loss lovasz: the classes that count in a batch - those with foreground among its valid pixels (the paper's default) or all")
    p.add_argument("-optm", "--optimizer", type=str, choices=["adam", "sgd", "lamb"], default="adam")
    p.add_argument("--lamb_epsilon", type=float, default=1e-7, metavar="E", help="-optm lamb: the epsilon of the Adam direction (default 1e-7, as the Adam of this package)")
    p.add_argument("--num_classes", type=int, default=5)
    p.add_argument("--epochs", type=int, default=500)
    p.add_argument("-ps", "--patch_size", type=int, default=256)
    p.add_argument("--bound_weight", type=float, default=1.0)
    p.add_argument("--dist_weight", type=float, default=1.0)
    p.add_argument("--color_weight", type=float, default=1.0)
    # additive
    p.add_argument("--channels", type=int, default=0, help="input bands (0 = read from the first patch)")
    p.add_argument("--dtype", type=str, default="bf16", choices=["bf16", "f32"])
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--compact_dataset", type=str2bool, default=False,
                   help="dataset in the compact layout: images/<name>.npy (uint8 HxWxC) + labels/classes/<name>.npy (uint8 HxW)")
    p.add_argument("--norm_type", type=int, default=1, choices=[1, 2], help="compact layout: x = u8 / 255 (1) or u8 / 126.5 (2)")
    p.add_argument("--scene_dataset", type=str2bool, default=False,
                   help="dataset is a scene directory: scenes/<name>.npy (uint8 HxWxC) + labels/scenes/<name>.npy (uint8 HxW); patches are cut on the GPU")
    p.add_argument("--stride", type=int, default=32, help="scene directory: window stride")
    p.add_argument("--data_aug", type=str2bool, default=True, help="scene directory: every window five times (as is, rot90, rot180, flipped rows, flipped columns)")
    p.add_argument("--random_aug", type=str2bool, default=False,
                   help="scene directory: random rotation, zoom and shift of every training window, resampled on the GPU")
    p.add_argument("--aug_rotate", type=float, default=180.0, metavar="DEG", help="random_aug: the angle is uniform in [-DEG, DEG]")
    p.add_argument("--aug_zoom", type=float, nargs=2, default=[0.75, 1.33], metavar=("LO", "HI"), help="random_aug: the zoom is log-uniform in [LO, HI]")
    p.add_argument("--aug_shift", type=float, default=None, metavar="PX", help="random_aug: shift of up to PX pixels per axis (default: stride / 2)")
    p.add_argument("--photo_aug", type=str2bool, default=False,
                   help="scene directory: random brightness, contrast, saturation, hue, tone and noise of every training window, applied on the GPU")
    p.add_argument("--photo_brightness", type=float, default=0.1, metavar="V", help="photo_aug: the offset is uniform in [-V, V] of full scale")
    p.add_argument("--photo_contrast", type=float, nargs=2, default=[0.8, 1.25], metavar=("LO", "HI"), help="photo_aug: the contrast is log-uniform in [LO, HI]")
    p.add_argument("--photo_saturation", type=float, nargs=2, default=[0.8, 1.25], metavar=("LO", "HI"), help="photo_aug: the saturation is log-uniform in [LO, HI] (3 channels)")
    p.add_argument("--photo_hue", type=float, default=8.0, metavar="DEG", help="photo_aug: the hue turns by an angle uniform in [-DEG, DEG] (3 channels)")
    p.add_argument("--photo_tone", type=float, default=0.4, metavar="V", help="photo_aug: the tone-curve strength is uniform in [-V, V], V <= 1")
    p.add_argument("--photo_noise", type=float, nargs=2, default=[0.0, 3.0], metavar=("LO", "HI"), help="photo_aug: the noise sigma, in levels, is uniform in [LO, HI]")
    p.add_argument("--paste_aug", type=str2bool, default=False,
                   help="scene directory: copy-paste augmentation - ground-truth objects of --paste_classes pasted into the training windows on the GPU")
    p.add_argument("--paste_classes", type=int, nargs="+", default=None, metavar="K", help="paste_aug: the classes whose objects are pasted; each is drawn equally often")
    p.add_argument("--paste_per_window", type=int, nargs=2, default=[0, 3], metavar=("LO", "HI"), help="paste_aug: the number of pastes per window is uniform in LO..HI")
    p.add_argument("--paste_onto", type=str, nargs="+", default=None, metavar="SRC:DST[,DST]",
                   help="paste_aug: class SRC may cover the classes DST only (default: every class), e.g. 4:0 - cars on impervious surface")
    p.add_argument("--paste_over_void", type=str2bool, default=False, help="paste_aug: objects may also cover pixels that carry no class")
    p.add_argument("--paste_min_area", type=int, default=1, metavar="A", help="paste_aug: objects of at least A pixels")
    p.add_argument("--paste_max_area", type=int, default=None, metavar="A", help="paste_aug: objects of at most A pixels (default: no limit)")
    p.add_argument("--class_weights", type=str, nargs="+", default=None, metavar="W",
                   help="weighted_cross_entropy (class weights) / focal (per-class alpha): `auto` (scene directory: total / pixels of the class over the training windows) or one weight per class")
    p.add_argument("--focal_gamma", type=float, default=2.0, metavar="G", help="--loss focal: the focusing exponent, 0 or 1..8 (0 with --class_weights is weighted cross entropy)")
    p.add_argument("--focal_alpha", type=float, nargs="+", default=None, metavar="A",
                   help="--loss focal: the seg head's alpha, one value or one per class (default 0.25; --class_weights gives it instead)")
    p.add_argument("--bound_alpha", type=float, default=None, metavar="A",
                   help="--loss focal, multitasking: class balancing of the boundary head's binary focal loss with this alpha (default: none)")
    p.add_argument("--label_smoothing", type=float, default=0.0, metavar="E",
                   help="label smoothing of the cross-entropy and focal losses, in [0, 1) (not --loss tanimoto; the MSE heads take none)")
    p.add_argument("--ohem", type=str2bool, default=False,
                   help="online hard example mining: per step only the hardest pixels of the --ohem_heads contribute to loss and gradient, selected on the GPU")
    p.add_argument("--ohem_keep", type=float, default=0.25, metavar="R", help="ohem: the kept share of the valid pixels, in (0, 1]")
    p.add_argument("--ohem_min_kept", type=int, default=0, metavar="N", help="ohem: never fewer than N pixels per step (and head)")
    p.add_argument("--ohem_thresh", type=float, default=None, metavar="T", help="ohem: keep every pixel whose loss is at least T as well")
    p.add_argument("--ohem_prob", type=float, default=None, metavar="P",
                   help="ohem, --loss cross_entropy: the threshold as a probability of the true class, T = -log P (mmsegmentation's OHEMPixelSampler)")
    p.add_argument("--ohem_warmup", type=int, default=0, metavar="N", help="ohem: the kept share falls from 1 to --ohem_keep over the first N optimizer updates")
    p.add_argument("--ohem_heads", nargs="+", choices=["seg", "bound"], default=["seg"], help="ohem: the mining heads (bound needs --multitasking yes)")
    p.add_argument("--balance_class", type=int, default=None, metavar="K",
                   help="scene directory: train only on windows in which class K covers at least --balance_percent of the pixels")
    p.add_argument("--balance_percent", type=float, default=None, metavar="P", help="balance_class: the share of the window, in percent")
    p.add_argument("--ignore_void", type=str2bool, default=False,
                   help="class-map layouts (--compact_dataset / --scene_dataset yes): pixels whose class value is >= --num_classes are no label; they leave every loss, gradient and metric")
    p.add_argument("--void_margin", type=int, default=2, metavar="N",
                   help="ignore_void: pixels within N (Chebyshev, 0..16) of a void pixel are void too; 2 covers the boundary target's reach across a class / void interface")
    p.add_argument("--clipnorm", type=float, default=None, metavar="C", help="clip every variable's gradient to the norm C (Keras' clipnorm)")
    p.add_argument("--global_clipnorm", type=float, default=None, metavar="C", help="clip the whole gradient to the norm C (Keras' global_clipnorm)")
    p.add_argument("--clipvalue", type=float, default=None, metavar="C", help="limit every gradient element to [-C, C] (Keras' clipvalue); at most one clip flag")
    p.add_argument("--weight_decay", type=float, default=None, metavar="WD", help="decoupled weight decay: theta -= theta * WD * learning rate before every update")
    p.add_argument("--decay_all", type=str2bool, default=False, help="weight_decay: decay biases and BatchNorm gamma / beta too (default: kernels only)")
    p.add_argument("--skip_nonfinite", type=str2bool, default=False,
                   help="leave weights, moments and BatchNorm statistics alone in a step whose gradient holds an Inf or a NaN")
    p.add_argument("--lr_schedule", choices=["constant", "cosine", "exponential", "polynomial", "piecewise", "inverse_time"], default="constant",
                   help="learning-rate schedule (Keras' formulas, computed on the GPU); -lr is the initial rate")
    p.add_argument("--lr_decay_steps", type=int, default=None, metavar="N", help="lr_schedule: optimizer steps of one decay (every kind but piecewise); under --grad_accum these are updates, not batches")
    p.add_argument("--lr_warmup_steps", type=int, default=0, metavar="N", help="cosine: linear warm-up from -lr to --lr_warmup_target over N steps (under --grad_accum: updates, not batches)")
    p.add_argument("--lr_warmup_target", type=float, default=None, metavar="LR", help="cosine: the rate the warm-up ends at and the cosine starts from")
    p.add_argument("--lr_alpha", type=float, default=0.0, metavar="A", help="cosine: the final rate as a fraction of the start of the decay")
    p.add_argument("--lr_decay_rate", type=float, default=None, metavar="R", help="exponential / inverse_time: the decay rate")
    p.add_argument("--lr_staircase", type=str2bool, default=False, help="exponential / inverse_time: decay in whole multiples of --lr_decay_steps")
    p.add_argument("--lr_end", type=float, default=1e-4, metavar="LR", help="polynomial: the final rate")
    p.add_argument("--lr_power", type=float, default=1.0, metavar="P", help="polynomial: the power")
    p.add_argument("--lr_cycle", type=str2bool, default=False, help="polynomial: start a new, longer decay when one ends")
    p.add_argument("--lr_boundaries", type=str, default=None, metavar="S1,S2,..", help="piecewise: at most 16 increasing step counts")
    p.add_argument("--lr_values", type=str, default=None, metavar="LR0,LR1,..", help="piecewise: one rate more than boundaries; LRi holds while step <= Si")
    p.add_argument("--ema", type=str2bool, default=False, help="keep a moving average of the weights; validation and the best-model criterion use it")
    p.add_argument("--ema_momentum", type=float, default=0.99, metavar="M", help="ema: average = M * average + (1 - M) * weights after every step")
    p.add_argument("--ema_overwrite_frequency", type=int, default=None, metavar="N", help="ema: every N steps the weights take the average's values (under --grad_accum: updates, not batches)")
    p.add_argument("--grad_accum", type=int, default=1, metavar="K",
                   help="apply the mean of K consecutive batches' gradients once every K batches (1: off); schedules, Adam's bias correction and the "
                        "moving average then count updates, not batches")
    return p


def schedule_options(args):
    """--lr_schedule and its numeric flags as the optimizer's learning_rate (a float for `constant`), --ema* as its keywords; checked before
    anything is built (resunet_a_mltsk_keras_amd/schedules.py has the definitions)."""
    from resunet_a_mltsk_keras_amd import schedules as SC
    kind, lr = args.lr_schedule, args.learning_rate
    need = lambda flag, v: sys.exit(f"--lr_schedule {kind} needs {flag}") if v is None else v
    try:
        if kind == "constant":
            rate = lr
        elif kind == "piecewise":
            b = [int(v) for v in need("--lr_boundaries", args.lr_boundaries).split(",")]
            rate = SC.PiecewiseConstantDecay(b, [float(v) for v in need("--lr_values", args.lr_values).split(",")])
        else:
            steps = need("--lr_decay_steps", args.lr_decay_steps)
            if kind == "cosine":
                rate = SC.CosineDecay(lr, steps, alpha=args.lr_alpha, warmup_target=args.lr_warmup_target, warmup_steps=args.lr_warmup_steps)
            elif kind == "polynomial":
                rate = SC.PolynomialDecay(lr, steps, end_learning_rate=args.lr_end, power=args.lr_power, cycle=args.lr_cycle)
            else:
                cls = SC.ExponentialDecay if kind == "exponential" else SC.InverseTimeDecay
                rate = cls(lr, steps, need("--lr_decay_rate", args.lr_decay_rate), staircase=args.lr_staircase)
        kw = dict(use_ema=bool(args.ema), ema_momentum=args.ema_momentum, ema_overwrite_frequency=args.ema_overwrite_frequency)
        SC.check_ema_options(**kw)
    except ValueError as exc:
        sys.exit(f"learning-rate schedule / ema flags: {exc}")
    return rate, kw


def optimizer_options(args):
    """--clipnorm / --global_clipnorm / --clipvalue / --weight_decay / --skip_nonfinite as the optimizer's keywords, checked before anything is
    built (resunet_a_mltsk_keras_amd/clip.py has the definitions): at most one clip flag, each positive."""
    from resunet_a_mltsk_keras_amd.clip import check_options
    kw = dict(clipnorm=args.clipnorm, global_clipnorm=args.global_clipnorm, clipvalue=args.clipvalue, weight_decay=args.weight_decay)
    try:
        check_options(**kw)
    except ValueError as exc:
        sys.exit(f"optimizer flags: {exc}")
    return dict(kw, skip_nonfinite=bool(args.skip_nonfinite))


def accum_options(args):
    """--grad_accum as the optimizer's keyword (1 is off), checked before anything is built (resunet_a_mltsk_keras_amd/accum.py)."""
    from resunet_a_mltsk_keras_amd.accum import check_steps
    try:
        return dict(gradient_accumulation_steps=check_steps(None if args.grad_accum == 1 else args.grad_accum))
    except ValueError as exc:
        sys.exit(f"--grad_accum: {exc}")


def check_void_flags(args):
    """--ignore_void / --void_margin checked against the rest of the command line, before anything is loaded: returns the margin, or None (off)."""
    if not args.ignore_void:
        return None
    if not (args.compact_dataset or args.scene_dataset):
        sys.exit("--ignore_void yes reads the void pixels off a class map: it needs --compact_dataset yes or --scene_dataset yes (the float layout has none)")
    if args.checkpoint_path is not None and args.loss != "lovasz":      # (--loss lovasz -cp compiles the loaded model from the command line)
        sys.exit("--ignore_void: the option is not stored in a checkpoint, and --checkpoint_path compiles the model from the checkpoint")
    if not 0 <= args.void_margin <= 16:
        sys.exit(f"--void_margin {args.void_margin} outside 0..16")
    return args.void_margin


def check_photo_flags(args):
    """--photo_aug and its ranges checked against the rest of the command line, before anything is loaded: returns the PhotoJitter, or
    None (off); SystemExit with a message otherwise."""
    if not args.photo_aug:
        return None
    if not args.scene_dataset:
        sys.exit("--photo_aug yes jitters windows of resident scenes: it needs --scene_dataset yes")
    from resunet_a_mltsk_keras_amd.scenes import PhotoJitter
    try:
        return PhotoJitter(args.photo_brightness, tuple(args.photo_contrast), tuple(args.photo_saturation), args.photo_hue, args.photo_tone,
                           tuple(args.photo_noise))
    except ValueError as exc:
        sys.exit(f"--photo_aug: {exc}")


def check_paste_flags(args):
    """--paste_aug and its options checked against the rest of the command line, before anything is loaded: returns the CopyPaste, or
    None (off); SystemExit with a message otherwise."""
    if not args.paste_aug:
        return None
    if not args.scene_dataset:
        sys.exit("--paste_aug yes pastes objects of resident scenes: it needs --scene_dataset yes")
    if not args.paste_classes:
        sys.exit("--paste_aug yes needs --paste_classes K [K ...]: the classes whose objects are pasted")
    C = args.num_classes
    bad = [c for c in args.paste_classes if not 0 <= c < C]
    if bad:
        sys.exit(f"--paste_classes {bad[0]} outside 0..{C - 1}")
    onto = None
    for item in args.paste_onto or []:
        try:
            src, dst = item.split(":")
            src, dst = int(src), [int(d) for d in dst.split(",")]
        except ValueError:
            sys.exit(f"--paste_onto {item!r}: SRC:DST[,DST...] with class indices, as in 4:0,1")
        if src not in args.paste_classes:
            sys.exit(f"--paste_onto {item!r}: class {src} is not one of --paste_classes {args.paste_classes}")
        if any(not 0 <= d < C for d in dst):
            sys.exit(f"--paste_onto {item!r}: a destination class outside 0..{C - 1}")
        onto = {**(onto or {}), src: dst}
    if args.paste_min_area < 1 or (args.paste_max_area is not None and args.paste_max_area < args.paste_min_area):
        sys.exit(f"--paste_min_area {args.paste_min_area}, --paste_max_area {args.paste_max_area}: 1 <= min <= max")
    from resunet_a_mltsk_keras_amd.scenes import CopyPaste
    try:
        return CopyPaste(args.paste_classes, tuple(args.paste_per_window), onto, args.paste_over_void)
    except ValueError as exc:
        sys.exit(f"--paste_aug: {exc}")


def build_object_bank(args, pool, table, x_tr, say):
    """--paste_aug yes: the pool's object bank (ScenePool.object_bank: ground-truth objects of --paste_classes, found on the GPU, the
    id maps resident), built once and restricted to the scenes that training windows are cut from; prints its size per class."""
    from resunet_a_mltsk_keras_amd.scenes import patch_index
    bank = pool.object_bank(args.num_classes, args.paste_classes, min_area=args.paste_min_area, max_area=args.paste_max_area)
    train_scenes = np.unique(table[[patch_index(n) for n in x_tr], 0])
    pool.bank = bank = np.ascontiguousarray(bank[np.isin(bank[:, 0], train_scenes)])
    per_class = ", ".join(f"class {c}: {int((bank[:, 2] == c).sum())}" for c in sorted(set(args.paste_classes)))
    say(f"Object bank: {len(bank)} objects of {len(train_scenes)} training scenes ({per_class}); area >= {args.paste_min_area}"
        + (f", <= {args.paste_max_area}" if args.paste_max_area is not None else "") + f", box <= {min(pool.patch)} pixels")
    if not len(bank):
        sys.exit(f"--paste_aug yes: the training scenes hold no object of --paste_classes {args.paste_classes} within the area and size limits")
    return bank


def scene_loaders(args, pool, table, x_tr, x_va, batch_size, rank=0, world=1):
    """(training SceneLoader, validation SceneLoader) of a scene run: x_tr / x_va are patch_{k}.npy names of table rows k.
    --random_aug, --photo_aug and --paste_aug reach the training loader alone: it draws a rotation, zoom and shift, a photo row per
    window and the paste rows of a batch per pass (the same on every rank); the validation loader is the same with and without them."""
    from resunet_a_mltsk_keras_amd.scenes import Jitter, SceneLoader, patch_index
    jitter = None
    if getattr(args, "random_aug", False):
        jitter = Jitter(args.aug_rotate, tuple(args.aug_zoom), args.stride / 2 if args.aug_shift is None else args.aug_shift)
    photo = check_photo_flags(args) if getattr(args, "photo_aug", False) else None
    paste = check_paste_flags(args) if getattr(args, "paste_aug", False) else None
    ld_tr = SceneLoader(pool, table[[patch_index(n) for n in x_tr]], batch_size, args.patch_size, rank=rank, world=world,
                        jitter=jitter, seed=args.seed, photo=photo, paste=paste)
    ld_va = SceneLoader(pool, table[[patch_index(n) for n in x_va]], batch_size, args.patch_size, rank=rank, world=world)
    return ld_tr, ld_va


def check_class_flags(args):
    """The --class_weights / --balance_* flags checked against the rest of the command line, before anything is loaded: returns
    None (no flag: today's weights), "auto" or the explicit weights as a list of floats; SystemExit with a message otherwise."""
    cw = args.class_weights
    if (args.balance_class is None) != (args.balance_percent is None):
        sys.exit("--balance_class K and --balance_percent P go together")
    if args.balance_class is not None:
        if not args.scene_dataset:
            sys.exit("--balance_class filters the windows of resident scenes: it needs --scene_dataset yes")
        if not 0 <= args.balance_class < args.num_classes:
            sys.exit(f"--balance_class {args.balance_class} outside 0..{args.num_classes - 1} (--num_classes {args.num_classes})")
        if not 0 <= args.balance_percent <= 100:
            sys.exit(f"--balance_percent {args.balance_percent} outside 0..100")
    if cw is None:
        return None
    if args.checkpoint_path is not None:
        sys.exit("--class_weights: with --checkpoint_path the loss, its class weights included, comes from the checkpoint")
    if args.loss not in ("weighted_cross_entropy", "focal"):
        sys.exit(f"--class_weights are the weights of --loss weighted_cross_entropy or the per-class alpha of --loss focal, not of --loss {args.loss}")
    if len(cw) == 1 and cw[0].lower() == "auto":
        if not args.scene_dataset:
            sys.exit("--class_weights auto counts the classes of resident scenes: it needs --scene_dataset yes")
        return "auto"
    try:
        w = [float(v) for v in cw]
    except ValueError:
        sys.exit(f"--class_weights {' '.join(cw)}: `auto` or one number per class")
    if len(w) != args.num_classes:
        sys.exit(f"--class_weights: {len(w)} weights for --num_classes {args.num_classes}")
    if not all(math.isfinite(v) and v >= 0 for v in w):
        sys.exit(f"--class_weights {' '.join(cw)}: the weights are finite and not negative")
    return w


def check_loss_flags(args):
    """--focal_* / --bound_alpha / --label_smoothing checked against --loss and the rest of the command line, before anything is loaded:
    returns the seg head's explicit alpha vector (None: --class_weights or the default 0.25); SystemExit with a message otherwise."""
    from resunet_a_mltsk_keras_amd import _lib as L
    from resunet_a_mltsk_keras_amd import losses as LS
    focal = args.loss == "focal"
    given = [n for n, v, d in (("--focal_gamma", args.focal_gamma, 2.0), ("--focal_alpha", args.focal_alpha, None), ("--bound_alpha", args.bound_alpha, None),
                               ("--label_smoothing", args.label_smoothing, 0.0)) if v != d]
    if given and args.checkpoint_path is not None:
        sys.exit(f"{given[0]}: with --checkpoint_path the loss, its options included, comes from the checkpoint")
    if not focal:
        for n in given:
            if n != "--label_smoothing":
                sys.exit(f"{n} belongs to --loss focal, not to --loss {args.loss}")
    if args.label_smoothing and args.loss == "tanimoto":
        sys.exit("--label_smoothing: the Tanimoto loss takes no label smoothing")
    if args.label_smoothing and args.loss == "lovasz":
        sys.exit("--label_smoothing: the Lovasz loss takes no label smoothing")
    if args.lovasz_classes != "present" and args.loss != "lovasz":
        sys.exit(f"--lovasz_classes belongs to --loss lovasz, not to --loss {args.loss}")
    if args.loss == "lovasz" and not 1 <= args.num_classes <= LS.LOVASZ_MAX_CLASSES:
        sys.exit(f"--loss lovasz: --num_classes {args.num_classes}, the Lovasz kernels take 1..{LS.LOVASZ_MAX_CLASSES}")
    alpha = None
    if args.focal_alpha is not None:
        if args.class_weights is not None:
            sys.exit("--focal_alpha and --class_weights both name the seg head's per-class alpha: give one of them")
        if len(args.focal_alpha) not in (1, args.num_classes):
            sys.exit(f"--focal_alpha: {len(args.focal_alpha)} values; one, or one per class (--num_classes {args.num_classes})")
        alpha = LS.scalar_or_vector(args.focal_alpha, args.num_classes)
    if args.bound_alpha is not None and not args.multitasking:
        sys.exit("--bound_alpha balances the boundary head's loss: it needs --multitasking yes")
    try:
        kind = {"focal": L.LOSS_FOCAL_CE, "tanimoto": L.LOSS_TANIMOTO, "cross_entropy": L.LOSS_CE_LOGITS}.get(args.loss, L.LOSS_WCE)
        LS.check_options(kind, args.num_classes, args.focal_gamma, alpha, False, args.label_smoothing, what="--loss " + args.loss)
        if focal and args.bound_alpha is not None:
            LS.check_options(L.LOSS_FOCAL_BCE, args.num_classes, args.focal_gamma, args.bound_alpha, True, args.label_smoothing, what="--bound_alpha")
    except ValueError as exc:
        sys.exit(str(exc))
    return alpha


def check_ohem_flags(args):
    """--ohem and its flags checked against --loss and the rest of the command line, before anything is loaded: returns the keyword arguments of
    keras_api.OnlineHardExampleMining (None: off); SystemExit with a message otherwise."""
    from resunet_a_mltsk_keras_amd import losses as LS
    given = [n for n, v, d in (("--ohem_keep", args.ohem_keep, 0.25), ("--ohem_min_kept", args.ohem_min_kept, 0), ("--ohem_thresh", args.ohem_thresh, None),
                               ("--ohem_prob", args.ohem_prob, None), ("--ohem_warmup", args.ohem_warmup, 0), ("--ohem_heads", args.ohem_heads, ["seg"])) if v != d]
    if not args.ohem:
        if given:
            sys.exit(f"{given[0]} belongs to --ohem yes")
        return None
    if args.checkpoint_path is not None:
        sys.exit("--ohem: with --checkpoint_path the loss, its options included, comes from the checkpoint")
    if args.loss == "tanimoto":
        sys.exit("--ohem needs a per-pixel loss: the Tanimoto loss has none")
    if args.loss == "lovasz":
        sys.exit("--ohem needs a per-pixel loss: the Lovasz loss has none")
    if "bound" in args.ohem_heads and not args.multitasking:
        sys.exit("--ohem_heads bound: the boundary head needs --multitasking yes")
    if args.ohem_thresh is not None and args.ohem_prob is not None:
        sys.exit("--ohem_thresh and --ohem_prob both name the threshold: give one of them")
    if args.ohem_prob is not None and (args.loss != "cross_entropy" or args.label_smoothing or args.ohem_heads != ["seg"]):
        sys.exit("--ohem_prob means -log P of the true class: --loss cross_entropy without --label_smoothing, on the seg head; give --ohem_thresh otherwise")
    try:
        kw = dict(keep_ratio=args.ohem_keep, min_kept=args.ohem_min_kept, loss_thresh=args.ohem_thresh, prob_thresh=args.ohem_prob, warmup_steps=args.ohem_warmup)
        LS.check_ohem(LS.ohem_options(LS.ohem_q16(kw["keep_ratio"]), kw["min_kept"], kw["loss_thresh"], kw["prob_thresh"], kw["warmup_steps"]), what="--ohem")
    except ValueError as exc:
        sys.exit(f"--ohem: {exc}")
    return kw


def print_class_histogram(say, counts, num_classes):
    """Pixels and share per class of int64 [N][C + 1] window counts, and the share of pixels that carry no class (>= C)."""
    n = counts.sum(0)
    total = max(int(n.sum()), 1)
    say(f"Class histogram of the {len(counts)} training windows:")
    for c in range(num_classes):
        say(f"  class {c}: {int(n[c])} pixels ({100.0 * int(n[c]) / total:.4f} %)")
    say(f"  no class (>= {num_classes}): {int(n[num_classes])} pixels ({100.0 * int(n[num_classes]) / total:.4f} %)")


def compute_mcc(tp, tn, fp, fn):
    den = math.sqrt((tp + fp) * (tp + fn) * (tn + fp) * (tn + fn))
    return (tp * tn - fp * fn) / den if den > 0 else float("nan")


def list_dataset(root, multitasking):
    """Name-paired patch paths: <root>/train/x.npy with <root>/labels/{seg,bound,dist,color}/x.npy."""
    tdir = os.path.join(root, "train")
    names = sorted(n for n in os.listdir(tdir) if n.endswith(".npy"))
    heads = ["seg", "bound", "dist", "color"] if multitasking else ["seg"]
    for h in heads:
        have = set(os.listdir(os.path.join(root, "labels", h)))
        missing = [n for n in names if n not in have]
        if missing:
            raise FileNotFoundError(f"labels/{h} lacks {len(missing)} patches, e.g. {missing[0]}")
    xs = [os.path.join(tdir, n) for n in names]
    ys = {h: [os.path.join(root, "labels", h, n) for n in names] for h in heads}
    return xs, ys


def list_compact_dataset(root):
    """Name-paired compact patches: <root>/images/x.npy with <root>/labels/classes/x.npy."""
    names = sorted(n for n in os.listdir(os.path.join(root, "images")) if n.endswith(".npy"))
    have = set(os.listdir(os.path.join(root, "labels", "classes")))
    missing = [n for n in names if n not in have]
    if missing:
        raise FileNotFoundError(f"labels/classes lacks {len(missing)} patches, e.g. {missing[0]}")
    return [os.path.join(root, "images", n) for n in names], {"classes": [os.path.join(root, "labels", "classes", n) for n in names]}


def list_scene_dataset(n_patches):
    """The listing list_compact_dataset would give for the materialised dataset of an n-row window table (scenes.materialize
    writes row k as patch_{k}.npy): the file names in lexicographic order, as the images and as the labels."""
    from resunet_a_mltsk_keras_amd.scenes import patch_name
    names = sorted(patch_name(k) for k in range(n_patches))
    return names, {"classes": list(names)}


def split_dataset(xs, ys):
    """train_test_split(test_size=0.2, random_state=42) applied to every list jointly (reference :377-380)."""
    from sklearn.model_selection import train_test_split
    heads = list(ys)
    parts = train_test_split(xs, *[ys[h] for h in heads], test_size=0.2, random_state=42)
    x_tr, x_va = parts[0], parts[1]
    y_tr = {h: parts[2 + 2 * i] for i, h in enumerate(heads)}
    y_va = {h: parts[3 + 2 * i] for i, h in enumerate(heads)}
    return x_tr, y_tr, x_va, y_va


class ScalarLog:
    def __init__(self, path):
        os.makedirs(path, exist_ok=True)
        self.f = open(os.path.join(path, "scalars.jsonl"), "a")

    def scalar(self, tag, value, step):
        self.f.write(json.dumps({"tag": tag, "value": float(value), "step": int(step)}) + "\n")
        self.f.flush()



def agree_from_rank0(value, world):
    """Rank 0's value on every rank.  The metrics are already replica-aggregated inside train_on_batch / test_on_batch
    (identical on all ranks); the stop / save decision still goes through one broadcast per epoch, so that no rank can
    ever leave the epoch loop while the others wait in the next gradient all-reduce (reference :280-292 takes ONE
    decision for all replicas)."""
    if world <= 1:
        return float(value)
    import torch
    import torch.distributed as dist
    t = torch.tensor([float(value)], dtype=torch.float64)
    if dist.get_backend() == "nccl":
        t = t.cuda()
    dist.broadcast(t, 0)
    return float(t.item())


def train_model(args, net, x_tr, y_tr, x_va, y_va, batch_size, epochs, x_shape, n_classes, patience=10, delta=0.001,
                metrics_names=None, rank=0, world=1, scenes=None):
    say = print if rank == 0 else (lambda *a, **k: None)
    say("Start training...\n" + "=" * 60)
    say(f"Training on {len(x_tr)} images\nValidating on {len(x_va)} images\n" + "=" * 60 + f"\nTotal Epochs: {epochs}")
    tw = ScalarLog(os.path.join(args.results_path, "logs", "train")) if rank == 0 else None
    vw = ScalarLog(os.path.join(args.results_path, "logs", "val")) if rank == 0 else None
    from resunet_a_mltsk_keras_amd.loader import PrefetchLoader
    # the reference loads 5*B .npy files serially before every step (train_ISPRS.py:115-141); here worker threads read
    # two batches ahead into pinned buffers
    # under data parallel `batch_size` is the global batch and every rank reads only its own shard of it
    # compact layout: uint8 slots, and the targets are built on the GPU from the class map
    compact = bool(getattr(args, "compact_dataset", False))
    if scenes is None:
        ld_tr = PrefetchLoader(x_tr, y_tr, batch_size, rank=rank, world=world, keep_dtype=compact)
        ld_va = PrefetchLoader(x_va, y_va, batch_size, rank=rank, world=world, keep_dtype=compact)
    else:
        # scenes = (ScenePool, window table): x_tr / x_va are patch_{k}.npy names of table rows k; no files, no loader threads - a
        # batch is its rows of the table, and every rank holds the pool and takes its own rows
        pool, table = scenes
        ld_tr, ld_va = scene_loaders(args, pool, table, x_tr, x_va, batch_size, rank, world)
    shard = dict(local_shard=True) if world > 1 else {}
    if compact or scenes is not None:
        shard["norm_type"] = args.norm_type
    labels = (lambda yb: None) if scenes is not None else (lambda yb: yb["classes"]) if compact else (lambda yb: yb if args.multitasking else yb["seg"])
    min_loss, cont = float("inf"), 0
    use_ema = bool(getattr(getattr(net, "optimizer", None), "use_ema", False))
    from resunet_a_mltsk_keras_amd.keras_api import K
    rng = np.random.default_rng(args.seed)
    say(net.output_names)
    for epoch in range(epochs):
        acc_tr = np.zeros(len(metrics_names)); acc_va = np.zeros(len(metrics_names))
        ld_tr.set_order(rng.permutation(len(x_tr)))
        n_tr, n_va = len(ld_tr), len(ld_va)
        t_before = getattr(getattr(net, "engine", None), "t", None)
        for xb, yb in ld_tr:
            acc_tr += np.asarray(net.train_on_batch(x=xb, y=labels(yb), return_dict=False, **shard))
        acc_tr /= max(n_tr, 1)
        # --ema yes: the validation - and with it the best-model criterion - runs under the averaged weights (the trained ones are back after it)
        with (net.ema_weights() if use_ema else contextlib.nullcontext()):
            for xb, yb in ld_va:
                acc_va += np.asarray(net.test_on_batch(x=xb, y=labels(yb), **shard))
        acc_va /= max(n_va, 1)
        tm, vm = dict(zip(metrics_names, acc_tr)), dict(zip(metrics_names, acc_va))
        pre = "seg_" if args.multitasking else ""
        mcc = compute_mcc(vm[pre + "true_positives"], vm[pre + "true_negatives"], vm[pre + "false_positives"], vm[pre + "false_negatives"])
        if rank == 0:
            if not args.multitasking:
                print(f"Epoch: {epoch} Training loss: {tm['loss']:.5f} Train acc.: {100 * tm['accuracy']:.5f}% "
                      f"Validation loss: {vm['loss']:.5f} Validation acc.: {100 * vm['accuracy']:.5f}%")
                tw.scalar("Total/Loss", tm["loss"], epoch); tw.scalar("Total/Accuracy", tm["accuracy"], epoch)
                vw.scalar("Total/Loss", vm["loss"], epoch); vw.scalar("Total/Accuracy", vm["accuracy"], epoch); vw.scalar("Total/MCC", mcc, epoch)
            else:
                print(f"+{'-' * 62}+\n| Epoch: {epoch:<53d}|\n| {'Task':8s}{'Loss':>13s}{'Val Loss':>13s}{'Acc %':>13s}{'Val Acc %':>13s} |")
                for key, tag in TASKS:
                    a = (100 * tm["seg_accuracy"], 100 * vm["seg_accuracy"]) if key == "seg" else (0, 0)
                    print(f"| {key.capitalize():8s}{tm[key + '_loss']:13.5f}{vm[key + '_loss']:13.5f}{a[0]:13.5f}{a[1]:13.5f} |")
                    tw.scalar(tag + "/Loss", tm[key + "_loss"], epoch); vw.scalar(tag + "/Loss", vm[key + "_loss"], epoch)
                tw.scalar("Segmentation/Accuracy", tm["seg_accuracy"], epoch); vw.scalar("Segmentation/Accuracy", vm["seg_accuracy"], epoch)
                vw.scalar("Segmentation/MCC", mcc, epoch)
                print(f"| {'Total':8s}{tm['loss']:13.5f}{vm['loss']:13.5f}{0:13d}{0:13d} |\n+{'-' * 62}+")
                tw.scalar("Total/Loss", tm["loss"], epoch); vw.scalar("Total/Loss", vm["loss"], epoch)
        acc = net.accumulation_state() if hasattr(net, "accumulation_state") else None
        if acc is not None:                                     # --grad_accum: updates taken next to batches seen; an open cycle carries over
            say(f"Gradient accumulation: {net.engine.t - t_before} updates from {n_tr} batches (K = {acc['steps']}; {acc['micro']} batches wait in the accumulator)")
        if getattr(net, "optimizer", None) is not None:
            say(f"Learning rate: {K.get_value(net.optimizer.lr):.6g}" + (" (validated under the averaged weights)" if use_ema else ""))
        rep = net.clip_report() if hasattr(net, "clip_report") else None        # None: no clip / decay / skip option is on
        if rep is not None:
            say(f"Optimizer: {rep['skipped']} steps skipped (non-finite gradient), {rep['clipped']} clipped by a norm so far; last gradient norm {rep['norm']:.6g}")
        trust = net.trust_report() if hasattr(net, "trust_report") else None   # None: the optimizer is not LAMB
        if trust is not None:
            say(f"LAMB trust ratio: {trust['min_ratio']:.6g} .. {trust['max_ratio']:.6g} over {len(trust['ratios'])} variables "
                f"({trust['forced']} forced to 1; {trust['updates']} updates so far)")
        lov = net.lovasz_report() if hasattr(net, "lovasz_report") else None   # None: no head is on the Lovasz loss
        if lov:
            say("Lovasz loss (last step): " + "; ".join(f"{h} {r['loss']:.6g} over {r['n_cls']} classes, {r['n_valid']} valid pixels" for h, r in lov.items()))
        mined = net.ohem_report() if hasattr(net, "ohem_report") else None     # None: no head mines hard examples
        if mined:
            say("Hard example mining (last step): " + "; ".join(f"{h} kept {r['kept']:.4f} of {r['n_valid']} valid pixels, tau {r['tau']:.6g}" for h, r in mined.items()))
        val_loss = agree_from_rank0(vm["loss"], world)
        if val_loss >= min_loss + delta:
            cont += 1
            say(f"EarlyStopping counter: {cont} out of {patience}")
            if cont >= patience:
                say("Early Stopping! \t Training Stopped")
                return net
        else:
            cont, min_loss = 0, val_loss
            say("Saving best model...")
            if rank == 0:
                net.save(os.path.join(args.results_path, "best_model.h5"))
    return None            # like the reference: the model is returned only on early stop (reference :287)


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.random_aug and not args.scene_dataset:
        sys.exit("--random_aug yes resamples windows of resident scenes: it needs --scene_dataset yes")
    check_photo_flags(args)
    check_paste_flags(args)
    class_weights = check_class_flags(args)
    focal_alpha = check_loss_flags(args)
    ohem_kw = check_ohem_flags(args)
    void_margin = check_void_flags(args)
    import torch
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        import torch.distributed as dist
        local = int(os.environ.get("LOCAL_RANK", "0"))
        torch.cuda.set_device(local)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    say = print if rank == 0 else (lambda *a, **k: None)
    say("=" * 30 + "INITIALIZING" + "=" * 30)
    say(f"GPUS DEVICES: {[torch.cuda.get_device_name(i) for i in range(torch.cuda.device_count())]}")
    say(f"Number of devices: {world}")
    if not args.resunet_a:
        sys.exit("--resunet_a False selects the reference's baseline U-Net, which is outside the accelerated path")

    from ResUnet_a.model2 import Resunet_a
    from multitasking_utils import Tanimoto_dual_loss
    from resunet_a_mltsk_keras_amd.keras_api import (SGD, Adam, Lamb, BinaryCrossentropy, BinaryFocalCrossentropy, CategoricalCrossentropy,
                                                   CategoricalFocalCrossentropy, K, MeanSquaredError, load_model, weighted_categorical_crossentropy)

    scenes = None
    if args.scene_dataset:
        if args.compact_dataset:
            sys.exit("--scene_dataset and --compact_dataset name two different layouts of -dp: give one of them")
        from resunet_a_mltsk_keras_amd.scenes import ScenePool, load_scene_dir, window_table
        _, images, class_maps = load_scene_dir(args.dataset_path)
        table = window_table([im.shape for im in images], args.patch_size, args.stride, args.data_aug)
        scenes = (ScenePool(images, class_maps, patch=args.patch_size), table)
        xs, ys = list_scene_dataset(len(table))
    else:
        xs, ys = list_compact_dataset(args.dataset_path) if args.compact_dataset else list_dataset(args.dataset_path, args.multitasking)
    x_tr, y_tr, x_va, y_va = split_dataset(xs, ys)
    if class_weights == "auto" or args.balance_class is not None:
        # class counts of the training windows, from the resident class maps: every rank computes the same integers itself
        from resunet_a_mltsk_keras_amd.scenes import balance_rows, patch_index
        from resunet_a_mltsk_keras_amd.scenes import class_weights as weights_of_counts
        pool, table = scenes
        counts = pool.class_counts(table[[patch_index(n) for n in x_tr]], args.num_classes)
        if args.balance_class is not None:
            keep = balance_rows(counts, args.balance_class, args.balance_percent, args.patch_size)
            if not keep.any():
                sys.exit(f"--balance_class {args.balance_class} --balance_percent {args.balance_percent:g}: none of the {len(keep)} training windows passes")
            say(f"Balance filter: class {args.balance_class} >= {args.balance_percent:g} % keeps {int(keep.sum())} of {len(keep)} training windows")
            x_tr = [n for n, k in zip(x_tr, keep) if k]
            y_tr = {h: [n for n, k in zip(v, keep) if k] for h, v in y_tr.items()}
            counts = counts[keep]
        print_class_histogram(say, counts, args.num_classes)
        if class_weights == "auto":
            try:
                class_weights = [float(w) for w in weights_of_counts(counts)]
            except ValueError as exc:
                sys.exit(f"--class_weights auto: {exc}")
    if args.paste_aug:
        build_object_bank(args, scenes[0], scenes[1], x_tr, say)
    rows = cols = args.patch_size
    channels = args.channels or (int(images[0].shape[-1]) if scenes is not None else int(np.load(xs[0]).shape[-1]))
    opt_kw = optimizer_options(args)
    rate, ema_kw = schedule_options(args)
    opt_kw.update(ema_kw)
    opt_kw.update(accum_options(args))
    if args.optimizer == "lamb":
        try:
            optm = Lamb(learning_rate=rate, beta_1=0.9, epsilon=args.lamb_epsilon, **opt_kw)
        except ValueError as exc:
            sys.exit(f"--lamb_epsilon: {exc}")
    else:
        optm = Adam(lr=rate, beta_1=0.9, **opt_kw) if args.optimizer == "adam" else SGD(lr=rate, momentum=0.8, **opt_kw)
    if args.weight_decay and not args.decay_all:
        from resunet_a_mltsk_keras_amd.clip import DEFAULT_DECAY_EXCLUDE
        optm.exclude_from_weight_decay(var_names=list(DEFAULT_DECAY_EXCLUDE))
    say("=" * 60)
    ls = args.label_smoothing
    if args.loss == "cross_entropy":
        say("Using Cross Entropy")
        loss, loss_bound, loss_reg = CategoricalCrossentropy(label_smoothing=ls), BinaryCrossentropy(label_smoothing=ls), MeanSquaredError()
    elif args.loss == "focal":
        alpha = class_weights if class_weights is not None else focal_alpha if focal_alpha is not None else 0.25
        say(f"Using Focal loss (gamma {args.focal_gamma:g}, alpha {alpha}, boundary alpha {args.bound_alpha}, label smoothing {ls:g})")
        loss = CategoricalFocalCrossentropy(alpha=alpha, gamma=args.focal_gamma, label_smoothing=ls)
        loss_bound = BinaryFocalCrossentropy(apply_class_balancing=args.bound_alpha is not None, alpha=args.bound_alpha if args.bound_alpha is not None else 0.25,
                                             gamma=args.focal_gamma, label_smoothing=ls)
        loss_reg = MeanSquaredError()
    elif args.loss == "tanimoto":
        say("Using Tanimoto Dual Loss")
        loss = loss_bound = loss_reg = Tanimoto_dual_loss()
    elif args.loss == "lovasz":
        from resunet_a_mltsk_keras_amd.keras_api import LovaszSoftmax
        say(f"Using Lovasz-Softmax loss (classes {args.lovasz_classes}) on seg and, multitasking, bound; MSE on dist and color")
        loss, loss_bound, loss_reg = LovaszSoftmax(args.lovasz_classes), LovaszSoftmax(args.lovasz_classes), MeanSquaredError()
    else:
        say("Using Weighted cross entropy")
        weights = class_weights if class_weights is not None else REFERENCE_WCE_WEIGHTS if args.num_classes == 5 else [1.0] * args.num_classes
        say(weights)
        loss, loss_bound, loss_reg = weighted_categorical_crossentropy(weights, label_smoothing=ls), BinaryCrossentropy(label_smoothing=ls), MeanSquaredError()
    if ohem_kw is not None:
        from resunet_a_mltsk_keras_amd.keras_api import OnlineHardExampleMining
        say(f"Online hard example mining on {', '.join(args.ohem_heads)}: keep {args.ohem_keep:g} of the valid pixels, at least {args.ohem_min_kept}, "
            f"loss threshold {args.ohem_thresh if args.ohem_prob is None else f'-log {args.ohem_prob:g}'}, warm-up {args.ohem_warmup} updates")
        if "seg" in args.ohem_heads:
            loss = OnlineHardExampleMining(loss, **ohem_kw)
        if "bound" in args.ohem_heads:
            loss_bound = OnlineHardExampleMining(loss_bound, **ohem_kw)
    say("=" * 60)

    # --loss lovasz with --checkpoint_path fine-tunes: the checkpoint gives the weights, the BatchNorm statistics, the moments and the step count,
    # the command line the loss and the optimizer's settings (every other --loss keeps the checkpoint's loss and optimizer)
    finetune = args.checkpoint_path is not None and args.loss == "lovasz"
    if args.checkpoint_path is None or finetune:
        if finetune:
            say(f"[INFO] loading {args.checkpoint_path} to fine-tune under the Lovasz loss (the command line's optimizer settings, -lr {args.learning_rate})...")
            model = load_model(args.checkpoint_path)
            if bool(model.cfg.multitasking) != bool(args.multitasking):
                sys.exit(f"--multitasking {'yes' if args.multitasking else 'no'}: the checkpoint's model is {'' if model.cfg.multitasking else 'not '}multitasking")
        else:
            resuneta = Resunet_a((rows, cols, channels), args.num_classes, args)
            model = resuneta.model
        if rank == 0:
            model.summary()
        if args.multitasking:
            say("Multitasking enabled!")
            lw = {"seg": 1.0, "bound": args.bound_weight, "dist": args.dist_weight, "color": args.color_weight}
            say(f"Loss Weights: {lw}")
            model.compile(optimizer=optm, loss={"seg": loss, "bound": loss_bound, "dist": loss_reg, "color": loss_reg},
                          loss_weights=lw, metrics={"seg": ["accuracy"]}, ignore_void=void_margin)
        else:
            say("Using simple ResUnet-a")
            model.compile(optimizer=optm, loss=loss, metrics=["accuracy"], ignore_void=void_margin)
        if void_margin is not None:
            say(f"Void pixels (class value >= {args.num_classes}, margin {void_margin}) are ignored")
        say("ResUnet-a compiled!")
    else:
        say(f"[INFO] loading {args.checkpoint_path}...")
        model = load_model(args.checkpoint_path)
        say(f"[INFO] old learning rate: {K.get_value(model.optimizer.lr)}")
        if model.optimizer.lr_schedule is not None:
            say(f"[INFO] the checkpoint trains under {model.optimizer.lr_schedule!r}: -lr is not applied, the schedule continues at its iteration")
        else:
            K.set_value(model.optimizer.lr, args.learning_rate)
            say(f"[INFO] new learning rate: {K.get_value(model.optimizer.lr)}")

    if rank == 0:
        os.makedirs(args.results_path, exist_ok=True)
    if world > 1 and args.batch_size % world:
        sys.exit(f"-bs {args.batch_size} is the GLOBAL batch and must divide by the {world} replicas")
    x_shape = (args.batch_size, rows, cols, channels)
    t0 = time.time()
    train_model(args, model, x_tr, y_tr, x_va, y_va, args.batch_size, args.epochs, x_shape, args.num_classes,
                metrics_names=model.metrics_names, rank=rank, world=world, scenes=scenes)
    say(f"\nTraining took: {(time.time() - t0) / 3600} \n")
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
