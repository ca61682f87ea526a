"""Compact dataset layout: a patch is its uint8 image and its uint8 class map; the float input x and the targets seg, bound, dist
and color are built on the GPU at every step (rua_multitask_targets, Engine._upload_compact) instead of being read as five float32
files.  At 256 x 256 x 3 with 6 classes that is 256 KB per patch instead of 6.3 MB.

    <root>/images/<name>.npy           uint8 H x W x C
    <root>/labels/classes/<name>.npy   uint8 H x W

`python -m resunet_a_mltsk_keras_amd.compact --src DIR --dst DIR --norm_type 1` converts the reference's layout
(<src>/train/<name>.npy, the normalised float32 image; <src>/labels/seg/<name>.npy, one-hot): the image becomes
rint(x * 255) (norm_type 2: rint(x * 126.5)) and is kept only if float32(u8) / 255 gives back every value exactly; the one-hot
label becomes its argmax.  labels/bound, dist and color are not copied - they are functions of the two (labels.py).
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import Dict

import numpy as np

NORM_DIV = {1: 255.0, 2: 126.5}        # the reference's normalize_rgb: img /= 255. (1), img /= 127.5 - 1. (2)


def normalize_u8(img_u8: np.ndarray, norm_type: int) -> np.ndarray:
    """x of a compact patch: float32(u8) / 255 or / 126.5 (float32 division, as the reference's float32 `img /= ...`)."""
    if norm_type not in NORM_DIV:
        raise ValueError(f"norm_type {norm_type!r}: the compact layout supports 1 and 2")
    return img_u8.astype(np.float32) / np.float32(NORM_DIV[norm_type])


def onehot(cls_u8: np.ndarray, num_classes: int) -> np.ndarray:
    """float32 one-hot of a class map; a class value >= num_classes gives an all-zero row."""
    return (cls_u8[..., None] == np.arange(num_classes, dtype=cls_u8.dtype)).astype(np.float32)


def host_targets(img_u8: np.ndarray, cls_u8: np.ndarray, num_classes: int, norm_type: int, multitask: bool = True) -> Dict[str, np.ndarray]:
    """The host definition of what rua_multitask_targets writes, per patch through labels.py: x and seg (+ bound, dist, color)
    for a batch img [B,H,W,Cin], cls [B,H,W]."""
    from .labels import multitask_labels
    out = {"x": normalize_u8(img_u8, norm_type), "seg": onehot(cls_u8, num_classes)}
    if multitask:
        per = [multitask_labels(out["seg"][b], img_u8[b], norm_type) for b in range(img_u8.shape[0])]
        for h in ("bound", "dist", "color"):
            out[h] = np.stack([p[h] for p in per])
    return out


def image_to_u8(img: np.ndarray, norm_type: int) -> np.ndarray:
    """The uint8 image whose normalisation is exactly `img`; ValueError if there is none."""
    if norm_type not in NORM_DIV:
        raise ValueError(f"norm_type {norm_type!r}: the compact layout supports 1 and 2")
    q = np.rint(np.asarray(img, np.float64) * NORM_DIV[norm_type])
    if not np.isfinite(q).all() or q.min() < 0 or q.max() > 255:
        raise ValueError(f"image values outside [0, 255 / {NORM_DIV[norm_type]}]: not a norm_type {norm_type} image")
    u8 = q.astype(np.uint8)
    back = normalize_u8(u8, norm_type)
    if back.shape != img.shape or not np.array_equal(back, img):
        raise ValueError(f"image is not float32(u8) / {NORM_DIV[norm_type]:g} exactly: not a norm_type {norm_type} image")
    return u8


def seg_to_classes(seg: np.ndarray, zero_rows_void: bool = False) -> np.ndarray:
    """argmax of a one-hot label (ValueError if it is not one-hot).  zero_rows_void: an all-zero row - a pixel without a class - is
    accepted and becomes 255 (C <= 255 then)."""
    if seg.ndim != 3 or seg.shape[-1] > (255 if zero_rows_void else 256) or not ((seg == 0) | (seg == 1)).all():
        raise ValueError("labels/seg must be one-hot H x W x C with C <= 256")
    rows = seg.sum(-1)
    if not ((rows == 1) | (rows == 0)).all() if zero_rows_void else not (rows == 1).all():
        raise ValueError("labels/seg must be one-hot H x W x C with C <= 256")
    cls = seg.argmax(-1).astype(np.uint8)
    if zero_rows_void:
        cls[rows == 0] = 255
    return cls


def convert(src: str, dst: str, norm_type: int, zero_rows_void: bool = False) -> int:
    """Reference layout -> compact layout, paired by file name; returns the number of patches written."""
    names = sorted(n for n in os.listdir(os.path.join(src, "train")) if n.endswith(".npy"))
    have = set(os.listdir(os.path.join(src, "labels", "seg")))
    missing = [n for n in names if n not in have]
    if missing:
        raise FileNotFoundError(f"labels/seg lacks {len(missing)} patches, e.g. {missing[0]}")
    os.makedirs(os.path.join(dst, "images"), exist_ok=True)
    os.makedirs(os.path.join(dst, "labels", "classes"), exist_ok=True)
    for n in names:
        try:
            img = image_to_u8(np.load(os.path.join(src, "train", n)), norm_type)
            cls = seg_to_classes(np.load(os.path.join(src, "labels", "seg", n)), zero_rows_void)
        except ValueError as exc:
            raise ValueError(f"{n}: {exc}") from None
        np.save(os.path.join(dst, "images", n), img)
        np.save(os.path.join(dst, "labels", "classes", n), cls)
    return len(names)


def main(argv=None) -> int:
    p = argparse.ArgumentParser(description="convert a reference-layout patch dataset to the compact uint8 layout")
    p.add_argument("--src", required=True, help="dataset with train/ and labels/seg/")
    p.add_argument("--dst", required=True, help="output: images/ and labels/classes/")
    p.add_argument("--norm_type", type=int, default=1, choices=[1, 2])
    p.add_argument("--zero_rows_void", action="store_true", help="accept all-zero label rows as class 255, 'no class' (default: refuse them)")
    a = p.parse_args(argv)
    n = convert(a.src, a.dst, a.norm_type, a.zero_rows_void)
    print(f"{n} patches written to {a.dst}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
