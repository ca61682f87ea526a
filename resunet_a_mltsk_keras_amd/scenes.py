"""Training from whole scenes: the scenes stay resident on the GPU and a step names its patches by index; rua_scene_windows
(csrc/scene.hip) cuts and augments them straight into the uint8 buffers rua_multitask_targets reads (Engine._upload_scene).
The reference does this offline (preprocess_save_patches_ISPRS.py): a 256 x 256 window slid at stride 32, every window written
five times (as it is, rot90 once, rot90 twice, flipped on axis 0, flipped on axis 1) - 64 windows x 5 copies per scene pixel.

    <root>/scenes/<name>.npy          uint8 H x W x C
    <root>/labels/scenes/<name>.npy   uint8 H x W

A batch is a window table, int32 [N][4] rows (scene, row, col, code): the window scene[row:row+PH, col:col+PW] transformed by

    code  numpy                              out[i, j] =
    0     w                                  w[i, j]
    1     np.rot90(w, 1)                     w[j, P-1-i]
    2     np.rot90(w, 2)                     w[PH-1-i, PW-1-j]
    3     np.flip(w, 0)                      w[PH-1-i, j]
    4     np.flip(w, 1)                      w[i, PW-1-j]
    5     np.rot90(w, 3)                     w[P-1-j, i]
    6     w.transpose(1, 0, 2)               w[j, i]
    7     np.rot90(w, 2).transpose(1, 0, 2)  w[P-1-j, P-1-i]

0 - 4 are the reference's five copies in its order, 5 - 7 complete the symmetries of the square; 1, 5, 6 and 7 need PH == PW.
window_table() enumerates the reference's patch set: patch k of a written-out dataset (`patch_{k}.npy`) is row k.

Random rotation, zoom and shift (the ResUNet-a paper's augmentation) go through a second table, int32 [N][7] rows
(scene, y0, x0, a_yy, a_yx, a_xy, a_xx) in Q16 fixed point: destination pixel (i, j) samples the scene at
sy = y0 + i * a_yy + j * a_yx, sx = x0 + i * a_xy + j * a_xx, the image bilinearly, the class map at the nearest pixel, with
reflect padding at the scene border (host_windows_affine is the definition, rua_scene_windows_affine its kernel).  affine_rows()
makes such rows from [N][4] rows and a rotation / zoom / shift, AffineSceneBatch carries them, SceneLoader(jitter=) draws them.

Colour, tone and noise jitter is a second pass over the cut bytes: an int32 [N][16] photo table, one row per window - a 3 x 3
colour matrix and offsets, a tone value, a noise amplitude and seed, all Q16 - (host_photometric is the definition,
rua_window_photometric, csrc/photo.hip, its kernel).  photo_rows() makes rows from brightness, contrast, saturation, hue, tone and
noise sigma, SceneBatch.with_photo() carries them, PhotoJitter draws them and SceneLoader(photo=) hands them out.

Copy-paste augmentation (Ghiasi et al., CVPR 2021) sits between the two: an int32 [M][16] paste table whose rows drop ground-truth
objects of the scenes - hard mask and label together - into the cut windows (host_paste is the definition, rua_window_paste,
csrc/paste.hip, its kernel).  host_object_bank() / ScenePool.object_bank() find the objects (the connected regions of chosen classes,
as int32 id maps and a table of class, area and bounding box), paste_rows() makes rows from bank entries, SceneBatch.with_paste()
carries them, CopyPaste draws them - the class uniformly, so a rare class is seen more often - and SceneLoader(paste=) hands them out.

Whole-scene evaluation goes the other way: predict_table() covers a scene with windows (the last one flush with the border) and
gives every scene pixel to exactly one of them, an int32 [N][4] ownership table of (r0, r1, c0, c1) rectangles in window
coordinates next to the window rows; rua_scene_stitch writes the arg-max of each owned pixel's class probabilities into a uint8
scene map and counts (true, predicted) pairs into a confusion matrix (host_stitch is its definition, Engine.predict_scene its user).

Test-time augmentation keeps that ownership and predicts every window under K of the eight codes, its views: view_rows() repeats a
code-0 table K times with the codes of VIEW_SETS (or any distinct codes), the K views of a window sit next to each other in one
forward batch, and rua_scene_stitch_views turns them back (INVERSE), sums each pixel's K probability vectors in float32 in view
order and takes the arg-max of the sum (host_stitch_views is its definition, Engine.predict_scene(views=) its user).

Whole-scene maps of every head use the same tables: rua_scene_stitch_maps takes any head's float32 window outputs under K views,
turns them back, quantises each value to Q16 (quantise_q16), averages in integers and writes a resident uint8 [H][W][Ch] map - the
seg probabilities, the boundary and distance maps, the colour head's HSV, or that HSV turned into an RGB picture (hsv_to_rgb_u8,
averaged over the views in RGB); host_stitch_maps is its definition, Engine.predict_scene(heads=) its user.

Multi-scale test-time augmentation is the evaluation side of the zoom jitter: scale_footprint() says how many scene pixels a window
covers at a zoom, scale_table() covers the scene with such footprints - predict_table's ownership, in scene coordinates - and makes
the affine rows that cut each footprint into a patch under K views (rua_scene_windows_affine), and rua_scene_accumulate brings the
class probabilities back: every owned scene pixel samples its window bilinearly at an exact fixed-point coordinate, in Q16 integers,
and the K views' sum is added to a scene-sized int32 accumulator, pass after pass (host_accumulate is its definition); nothing is
blended between the windows of a pass.  rua_scene_argmax then writes the class map and the confusion matrix (host_argmax);
check_scales() reads predict_scene's `scales`, Engine.predict_scene(scales=) is their user.

Blending is the one path on which neighbouring windows share pixels: blend_table() hands out each group's full footprint in place
of an owned rectangle, blend_weight() is a linear taper per axis in 1/256 (flat towards a scene border, never below 16), and
rua_scene_accumulate_blend adds (wy wx v + 32768) >> 16 of the K views' sum v to the same accumulator with integer atomics
(host_accumulate_blend is its definition: integer sums do not depend on the order); check_blend_budget() keeps the int32 sums in
range, Engine.predict_scene(blend="linear") is their user.

Class counts close the loop on the dataset: host_class_counts() says how many pixels of each class (and how many of none, a
value >= C) lie in each window of a table, rua_scene_class_counts is its kernel on the resident class maps and
ScenePool.class_counts() its user; class_weights() turns the counts of the training rows into the reference's weighted-CE weights
(total / pixels of the class - its five hard-coded numbers are exactly that for its own patch set) and balance_rows() is the test
of the reference's bal_aug_patches (keep a window only if a chosen class covers at least `percent` of it) on a window table.

The eroded ground truth is what the ISPRS benchmark publishes numbers on: host_erode() replaces every pixel that has a pixel of
another value within a disc of `radius` (3 there) by 255, "no class" for every C, because the reference labels are uncertain at
class boundaries; the scene border is no boundary.  rua_scene_erode is its kernel on resident maps - one pass writes the eroded
map, counts a prediction map against it into a confusion matrix (host_erode_confusion), or both -, ScenePool.eroded_maps() and
Engine.predict_scene(erode=) are its users.

The boundary F1 (BF score, Csurka et al. 2013) says whether the predicted class edges are where the true ones are, which no area
score does and the eroded protocol leaves out on purpose: host_boundaries() marks the inner 4-connected boundary pixels of every
class of a map, host_boundary_counts() counts, per class, the boundary pixels of the prediction that have one of the ground truth
within `radius` pixels and the other way round, and boundary_scores() turns such counts into precision, recall and F1.
rua_scene_boundary is the kernel of the first two on resident maps, ScenePool.boundary_counts() / boundary_maps() and
Engine.predict_scene(boundary=) are its users.  Radius 0 is exact coincidence, a real tolerance: "off" is None (check_tolerance).

A minimum mapping unit cleans a class map of speckle, as the reference's `prediction` does with an area opening before it scores:
host_regions() labels the connected regions of equal bytes of a map (4- or 8-connected) with their smallest row-major index and
gives each region's pixel count at that root, host_region_counts() counts per class the regions and the small ones among them, and
host_sieve() removes the regions below `min_area` pixels - mode "void" turns them into 255, which every score leaves out (the
reference's protocol), mode "fill" gives each the class most of its kept 4-neighbours have.  rua_scene_regions and
rua_scene_sieve (csrc/regions.hip) are their kernels on resident maps, ScenePool.region_counts() / sieved_maps() and
Engine.predict_scene(sieve=) their users; check_sieve() checks the parameters in the kernels' words.

A precision-recall sweep judges one class's probability instead of the arg-max map, as the reference's matrics_AA_recall does:
at every threshold the probability is binarised and area-opened, removed and "no class" pixels leave the count.  Thresholding
commutes with the area opening and the kept sets are nested, so host_area_open() builds ONE opened map per scene for all levels
(sweep_levels()), host_sweep_hist() one histogram of probabilities and opened bytes against the class map, and sweep_scores()
reads recall, precision, F1, alarm area and the average precision at every level from its suffix sums.  rua_scene_area_open and
rua_scene_sweep_hist (csrc/sweep.hip) are their kernels on resident maps, ScenePool.opened_maps() / sweep_hist() and
Engine.predict_scene(sweep=) their users.

Outlines: host_outlines() is the definition of the rings of an int32 id map - the directed pixel edges between an object and
anything else, each with one successor, their cycles, and every cycle's corners in walking order from its smallest edge -, in
integers; rua_scene_outline_count and rua_scene_outline_rings (csrc/outlines.hip) are its kernels on resident maps (list ranking by
pointer jumping), ScenePool.outlines() and Engine.predict_scene(instances={..., "outlines": True}) their users; outline_polygons()
gives the holes to their rings, simplify_ring() is an exact-integer Douglas-Peucker and write_geojson() writes the vector layer.

Flooding: host_flood() is the definition of a bounded, marker-controlled watershed of a height map in synchronous rounds - the
levels 255 .. floor let down one by one, an unsettled pixel that has reached the level taking the smallest id among its settled
neighbours of its own class -, flood_table() of the instance table afterwards; rua_scene_flood (csrc/flood.hip) is its kernel on
resident maps, ScenePool.instances(flood=) and Engine.predict_scene(instances={..., "flood": True}) its users: the grow step that
brings the small seed cores of touching buildings back to their outlines, which the bounded disc of host_instances cannot.

`python -m resunet_a_mltsk_keras_amd.scenes --image Image_Train.npy --reference Reference_Train.npy --dst DIR` writes a scene
directory from the reference's two inputs (C x H x W arrays, the reference colour-coded); `--materialize DST` also writes the
compact patch layout (compact.py) of its window table, for users who want files.
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import sys
from typing import List, Optional, Sequence, Tuple

import numpy as np

TRANSPOSING = (1, 5, 6, 7)
NUM_CODES = 8
MAX_PATCH, MAX_CHANNELS = 512, 16
# the five ISPRS label colours and their class values (the reference's label_dict)
ISPRS_COLOURS = {(255, 255, 255): 0, (0, 255, 0): 1, (0, 255, 255): 2, (0, 0, 255): 3, (255, 255, 0): 4}


def _patch2(patch) -> Tuple[int, int]:
    if isinstance(patch, (int, np.integer)):
        return int(patch), int(patch)
    ph, pw = patch
    return int(ph), int(pw)


def transform(w: np.ndarray, code: int) -> np.ndarray:
    """Window w (H x W or H x W x C) under `code` (the table in the module docstring)."""
    if code == 0:
        return w
    if code == 1:
        return np.rot90(w, 1)
    if code == 2:
        return np.rot90(w, 2)
    if code == 3:
        return np.flip(w, 0)
    if code == 4:
        return np.flip(w, 1)
    if code == 5:
        return np.rot90(w, 3)
    if code == 6:
        return np.swapaxes(w, 0, 1)
    if code == 7:
        return np.swapaxes(np.rot90(w, 2), 0, 1)
    raise ValueError(f"code {code} outside 0..7")


def window_table(shapes: Sequence[Sequence[int]], patch, stride: int, data_aug: bool) -> np.ndarray:
    """The reference's patch set as a window table: scene after scene the origins row = 0, stride, ... while row + patch <= H,
    the same for columns, row-major (the order view_as_windows(..., step=stride) reshapes to); with data_aug patch 5 * i + j is
    window i under code j, without it patch i is window i under code 0."""
    ph, pw = _patch2(patch)
    if stride < 1:
        raise ValueError(f"stride {stride} must be at least 1")
    parts = []
    codes = np.arange(5 if data_aug else 1, dtype=np.int32)
    for s, shp in enumerate(shapes):
        H, W = int(shp[0]), int(shp[1])
        if H < ph or W < pw:
            raise ValueError(f"scene {s} is {H} x {W}: smaller than the {ph} x {pw} patch")
        rows, cols = np.arange(0, H - ph + 1, stride, dtype=np.int32), np.arange(0, W - pw + 1, stride, dtype=np.int32)
        t = np.empty((len(rows), len(cols), len(codes), 4), np.int32)
        t[..., 0] = s
        t[..., 1] = rows[:, None, None]
        t[..., 2] = cols[None, :, None]
        t[..., 3] = codes[None, None, :]
        parts.append(t.reshape(-1, 4))
    return np.concatenate(parts) if parts else np.zeros((0, 4), np.int32)


def _is_table4(a: np.ndarray) -> bool:
    return a.ndim == 2 and a.shape[1] == 4 and bool(np.issubdtype(a.dtype, np.integer))


def _window_table(table) -> np.ndarray:
    t = np.asarray(table)
    if not _is_table4(t):
        raise ValueError(f"a window table is an integer [N][4] array of (scene, row, col, code) rows, got {t.dtype} {t.shape}")
    return t


def _two_tables(fn: str, rows, own, code: str):
    t, o = np.asarray(rows), np.asarray(own)
    for a, what in ((t, f"(scene, row, col, {code})"), (o, "(r0, r1, c0, c1)")):
        if not _is_table4(a):
            raise ValueError(f"{fn} takes integer [N][4] arrays of {what} rows, got {a.dtype} {a.shape}")
    return t, o


def _check_rows(fn: str, shapes, rows: list, ph: int, pw: int, own: Optional[list] = None, K: int = 1, views=None, code0: bool = False):
    """csrc/scene.hip's row checks (check_window_rows, check_groups) in their order and words, spoken as `fn`: `rows` in groups of K
    views with an `own` row each (None: none).  code0: rua_scene_stitch's rule, its groups are "rows"; views: the codes of a group."""
    n = len(shapes)
    for g in range(len(rows) // K):
        s0, ra, ca, _ = rows[g * K]
        for v in range(K):
            k = g * K + v
            s, r, c, code = rows[k]
            if not 0 <= s < n:
                raise ValueError(f"{fn}: row {k}: scene {s} outside 0..{n - 1}")
            H, W = int(shapes[s][0]), int(shapes[s][1])
            if r < 0 or c < 0 or r + ph > H or c + pw > W:
                raise ValueError(f"{fn}: row {k}: window ({r}, {c}) + {ph} x {pw} leaves its {H} x {W} scene")
            if (s, r, c) != (s0, ra, ca):
                raise ValueError(f"{fn}: row {k}: scene {s}, window ({r}, {c}), but its group {g} is scene {s0}, window ({ra}, {ca})")
            if code0:
                if code != 0:
                    raise ValueError(f"{fn}: row {k}: code {code} (a prediction window is cut as it is: code 0)")
                continue
            if not 0 <= code < NUM_CODES:
                raise ValueError(f"{fn}: row {k}: code {code} outside 0..7")
            if ph != pw and code in TRANSPOSING:
                raise ValueError(f"{fn}: row {k}: code {code} transposes and needs a square patch (got {ph} x {pw})")
            if views is not None and code != views[v]:
                raise ValueError(f"{fn}: row {k}: code {code}, but view {v} of {views} is code {views[v]}")
        if own is not None:
            r0, r1, c0, c1 = own[g]
            if not (0 <= r0 <= r1 <= ph and 0 <= c0 <= c1 <= pw):
                raise ValueError(f"{fn}: {'row' if code0 else 'group'} {g}: owned rows {r0}..{r1}, columns {c0}..{c1} outside the {ph} x {pw} window")


def check_table(shapes: Sequence[Sequence[int]], table: np.ndarray, patch) -> np.ndarray:
    """The table as a contiguous int32 [N][4] array; ValueError, in rua_scene_windows' own words, for the first bad row."""
    ph, pw = _patch2(patch)
    t = _window_table(table)
    n = len(shapes)
    if n < 1 or t.shape[0] < 1:
        raise ValueError(f"rua_scene_windows: nscenes {n}, N {t.shape[0]} (both >= 1)")
    if not (1 <= ph <= MAX_PATCH and 1 <= pw <= MAX_PATCH):
        raise ValueError(f"rua_scene_windows: PH {ph}, PW {pw} (1 <= PH, PW <= 512)")
    _check_rows("rua_scene_windows", shapes, t.tolist(), ph, pw)
    return np.ascontiguousarray(t, dtype=np.int32)


def host_windows(images: Sequence[np.ndarray], class_maps: Optional[Sequence[np.ndarray]], table: np.ndarray, patch):
    """The numpy definition of what rua_scene_windows writes: (img uint8 [N][PH][PW][C], cls uint8 [N][PH][PW] or None)."""
    ph, pw = _patch2(patch)
    t = check_table([im.shape for im in images], table, patch)
    img = np.empty((len(t), ph, pw, images[0].shape[2]), np.uint8)
    cls = np.empty((len(t), ph, pw), np.uint8) if class_maps is not None else None
    for k, (s, r, c, code) in enumerate(t.tolist()):
        img[k] = transform(images[s][r:r + ph, c:c + pw], code)
        if cls is not None:
            cls[k] = transform(class_maps[s][r:r + ph, c:c + pw], code)
    return img, cls


# ---- affine windows: rotation, zoom and shift, reflect-padded -------------------------------------------------------------------
Q16 = 65536
MAX_SCENE, MAX_COEF, MAX_ORIGIN = 16384, 4 * Q16, 1 << 30
# out[i, j] = w[S (i, j) + offset] for the eight codes: the rows (a_yy, a_yx), (a_xy, a_xx) of S
SYMMETRY = np.array([[[1, 0], [0, 1]], [[0, 1], [-1, 0]], [[-1, 0], [0, -1]], [[-1, 0], [0, 1]],
                     [[1, 0], [0, -1]], [[0, -1], [1, 0]], [[0, 1], [1, 0]], [[0, -1], [-1, 0]]], np.int64)


def check_affine_table(shapes: Sequence[Sequence[int]], table7: np.ndarray, patch, channels: int = 1) -> np.ndarray:
    """The table as a contiguous int32 [N][7] array; ValueError, in rua_scene_windows_affine's own words, for the first violation."""
    ph, pw = _patch2(patch)
    t = np.asarray(table7)
    if t.ndim != 2 or t.shape[1] != 7 or not np.issubdtype(t.dtype, np.integer):
        raise ValueError(f"an affine window table is an integer [N][7] array of (scene, y0, x0, a_yy, a_yx, a_xy, a_xx) rows, got {t.dtype} {t.shape}")
    n = len(shapes)
    if n < 1 or t.shape[0] < 1:
        raise ValueError(f"rua_scene_windows_affine: nscenes {n}, N {t.shape[0]} (both >= 1)")
    if not 1 <= channels <= MAX_CHANNELS:
        raise ValueError(f"rua_scene_windows_affine: Cin {channels} outside 1..16")
    if not (1 <= ph <= MAX_PATCH and 1 <= pw <= MAX_PATCH):
        raise ValueError(f"rua_scene_windows_affine: PH {ph}, PW {pw} (1 <= PH, PW <= 512)")
    for s, shp in enumerate(shapes):
        H, W = int(shp[0]), int(shp[1])
        if not (2 <= H <= MAX_SCENE and 2 <= W <= MAX_SCENE):
            raise ValueError(f"rua_scene_windows_affine: scene {s}: size {H} x {W} (2 <= H, W <= 16384)")
    t64 = t.astype(np.int64)
    bad = (t64[:, 0] < 0) | (t64[:, 0] >= n) | (np.abs(t64[:, 1:3]) > MAX_ORIGIN).any(1) | (np.abs(t64[:, 3:]) > MAX_COEF).any(1)
    if bad.any():
        k = int(np.argmax(bad))
        row = [int(v) for v in t64[k]]
        if not 0 <= row[0] < n:
            raise ValueError(f"rua_scene_windows_affine: row {k}: scene {row[0]} outside 0..{n - 1}")
        if abs(row[1]) > MAX_ORIGIN or abs(row[2]) > MAX_ORIGIN:
            raise ValueError(f"rua_scene_windows_affine: row {k}: origin ({row[1]}, {row[2]}) outside -2^30..2^30 (Q16)")
        a = next(v for v in row[3:] if abs(v) > MAX_COEF)
        raise ValueError(f"rua_scene_windows_affine: row {k}: coefficient {a} outside -262144..262144 (4 in Q16)")
    return np.ascontiguousarray(t, dtype=np.int32)


def _reflect(t: np.ndarray, n: int) -> np.ndarray:
    """numpy's 'reflect' padding as an index map: no edge repeat, any number of reflections."""
    m = 2 * (n - 1)
    u = np.mod(t, m)
    return np.where(u < n, u, m - u)


def host_windows_affine(images: Sequence[np.ndarray], class_maps: Optional[Sequence[np.ndarray]], table7: np.ndarray, patch):
    """The numpy definition of what rua_scene_windows_affine writes (include/rua_hip.h spells the same arithmetic out), in int64:
    (img uint8 [N][PH][PW][C], cls uint8 [N][PH][PW] or None)."""
    ph, pw = _patch2(patch)
    t = check_affine_table([im.shape for im in images], table7, patch, images[0].shape[2])
    img = np.empty((len(t), ph, pw, images[0].shape[2]), np.uint8)
    cls = np.empty((len(t), ph, pw), np.uint8) if class_maps is not None else None
    i, j = np.arange(ph, dtype=np.int64)[:, None], np.arange(pw, dtype=np.int64)[None, :]
    for k, (s, y0, x0, ayy, ayx, axy, axx) in enumerate(t.tolist()):
        im = images[s]
        H, W = im.shape[:2]
        sy, sx = y0 + i * ayy + j * ayx, x0 + i * axy + j * axx
        iy, ix, fy, fx = sy >> 16, sx >> 16, ((sy & 0xFFFF) >> 8)[..., None], ((sx & 0xFFFF) >> 8)[..., None]
        r0, r1, c0, c1 = _reflect(iy, H), _reflect(iy + 1, H), _reflect(ix, W), _reflect(ix + 1, W)
        p = lambda r, c: im[r, c].astype(np.int64)
        top, bot = (256 - fx) * p(r0, c0) + fx * p(r0, c1), (256 - fx) * p(r1, c0) + fx * p(r1, c1)
        img[k] = ((256 - fy) * top + fy * bot + 32768) >> 16
        if cls is not None:
            cls[k] = class_maps[s][_reflect((sy + 32768) >> 16, H), _reflect((sx + 32768) >> 16, W)]
    return img, cls


def affine_rows(rows4: np.ndarray, patch, rotate_deg=0.0, zoom=1.0, shift_q16=(0, 0)) -> np.ndarray:
    """[N][7] affine rows of [N][4] (scene, row, col, code) rows rotated by rotate_deg about the window centre, zoomed (> 1: in)
    and shifted by shift_q16 = (y, x) in Q16 pixels; the arguments broadcast per row ([N], [N], [N][2]).  The matrix is
    M = (1 / zoom) R(theta) S(code), a = rint(65536 M); the origin puts the patch centre on the window centre (+ shift).  With no
    rotation, zoom 1 and no shift host_windows_affine of the result is host_windows of rows4, bit for bit."""
    ph, pw = _patch2(patch)
    r4 = _window_table(rows4).astype(np.int64)
    N, code = len(r4), r4[:, 3]
    bad = np.flatnonzero((code < 0) | (code >= NUM_CODES))
    if bad.size:
        raise ValueError(f"affine_rows: row {int(bad[0])}: code {int(code[bad[0]])} outside 0..7")
    if ph != pw:
        bad = np.flatnonzero(np.isin(code, TRANSPOSING))
        if bad.size:
            raise ValueError(f"affine_rows: row {int(bad[0])}: code {int(code[bad[0]])} transposes and needs a square patch (got {ph} x {pw})")
    theta = np.deg2rad(np.broadcast_to(np.asarray(rotate_deg, np.float64), (N,)))
    z = np.broadcast_to(np.asarray(zoom, np.float64), (N,))
    if not (z > 0).all():
        raise ValueError("affine_rows: zoom must be positive")
    shift = np.broadcast_to(np.asarray(shift_q16, np.int64), (N, 2))
    R = np.empty((N, 2, 2), np.float64)
    R[:, 0, 0], R[:, 0, 1], R[:, 1, 0], R[:, 1, 1] = np.cos(theta), -np.sin(theta), np.sin(theta), np.cos(theta)
    a = np.rint(Q16 * (R @ SYMMETRY[code].astype(np.float64)) / z[:, None, None]).astype(np.int64)
    out = np.empty((N, 7), np.int64)
    out[:, 0] = r4[:, 0]
    out[:, 3:] = a.reshape(N, 4)
    # window centre in half pixels, minus half the patch's extent under the map
    out[:, 1] = (2 * r4[:, 1] + ph - 1) * (Q16 // 2) + shift[:, 0] - ((a[:, 0, 0] * (ph - 1) + a[:, 0, 1] * (pw - 1)) >> 1)
    out[:, 2] = (2 * r4[:, 2] + pw - 1) * (Q16 // 2) + shift[:, 1] - ((a[:, 1, 0] * (ph - 1) + a[:, 1, 1] * (pw - 1)) >> 1)
    if (np.abs(out) > 2 ** 31 - 1).any():
        raise ValueError("affine_rows: a row leaves the int32 range")
    return out.astype(np.int32)


# ---- photometric jitter: a colour matrix, a tone curve and hashed noise on the staged uint8 windows -------------------------------
PHOTO_MAX_M, PHOTO_MAX_B, PHOTO_MAX_T, PHOTO_MAX_A = 1 << 20, 1 << 29, Q16, Q16
SIGMA_Z = float(np.sqrt((256.0 ** 2 - 1.0) / 3.0))            # of z, the sum of four independent uniform bytes minus 510
_PHOTO_LIKE = (0, -1, -1, -1, 0, -1, -1, -1, 0, 9, 9, 9)       # a scalar row: the word each of words 0..11 must equal; -1: zero


def check_photo_table(table16, channels: int) -> np.ndarray:
    """The photo table as a contiguous int32 [N][16] array (word 14, the seed, is taken mod 2^32); ValueError, in
    rua_window_photometric's own words, for the first violation."""
    t = np.asarray(table16)
    if t.ndim != 2 or t.shape[1] != 16 or not np.issubdtype(t.dtype, np.integer):
        raise ValueError(f"a photo table is an integer [N][16] array of (M[3][3], b[3], tone, noise, seed, 0) rows, got {t.dtype} {t.shape}")
    fn = "rua_window_photometric"
    if t.shape[0] < 1:
        raise ValueError(f"{fn}: N {t.shape[0]} (>= 1)")
    if isinstance(channels, bool) or not isinstance(channels, (int, np.integer)) or not 1 <= channels <= MAX_CHANNELS:
        raise ValueError(f"{fn}: Cin {channels} outside 1..16")
    t64 = t.astype(np.int64)
    t64[:, 14] = ((t64[:, 14] + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)
    bad = (np.abs(t64[:, :9]) > PHOTO_MAX_M).any(1) | (np.abs(t64[:, 9:12]) > PHOTO_MAX_B).any(1) | (np.abs(t64[:, 12]) > PHOTO_MAX_T)
    bad |= (t64[:, 13] < 0) | (t64[:, 13] > PHOTO_MAX_A) | (t64[:, 15] != 0)
    if channels != 3:
        like = np.where(np.array(_PHOTO_LIKE)[None, :] < 0, 0, t64[:, [max(q, 0) for q in _PHOTO_LIKE]])
        bad |= (t64[:, :12] != like).any(1)
    if bad.any():
        k = int(np.argmax(bad))
        r = [int(v) for v in t64[k]]
        for q in range(9):
            if abs(r[q]) > PHOTO_MAX_M:
                raise ValueError(f"{fn}: row {k}: word {q}: matrix entry {r[q]} outside -1048576..1048576 (16 in Q16)")
        for q in range(9, 12):
            if abs(r[q]) > PHOTO_MAX_B:
                raise ValueError(f"{fn}: row {k}: word {q}: offset {r[q]} outside -536870912..536870912 (8192 levels in Q16)")
        if abs(r[12]) > PHOTO_MAX_T:
            raise ValueError(f"{fn}: row {k}: word 12: tone {r[12]} outside -65536..65536 (1 in Q16)")
        if not 0 <= r[13] <= PHOTO_MAX_A:
            raise ValueError(f"{fn}: row {k}: word 13: noise amplitude {r[13]} outside 0..65536")
        if r[15] != 0:
            raise ValueError(f"{fn}: row {k}: word 15: reserved, must be 0, got {r[15]}")
        q = next(q for q in range(12) if r[q] != (0 if _PHOTO_LIKE[q] < 0 else r[_PHOTO_LIKE[q]]))
        raise ValueError(f"{fn}: row {k}: word {q}: {r[q]}, but Cin {channels} != 3 takes scalar rows (off-diagonals 0, one gain, one offset)")
    return np.ascontiguousarray(t64, dtype=np.int32)


def host_photometric(img_u8: np.ndarray, table16) -> np.ndarray:
    """The numpy definition of what rua_window_photometric writes (include/rua_hip.h spells the same arithmetic out), in int64:
    uint8 [N][PH][PW][Cin] from uint8 [N][PH][PW][Cin] and an int32 [N][16] photo table - colour matrix and offsets, the tone curve,
    then noise hashed from the row's seed and the byte's position inside its window."""
    img = np.asarray(img_u8)
    if img.dtype != np.uint8 or img.ndim != 4:
        raise ValueError(f"windows are uint8 [N][PH][PW][Cin], got {img.dtype} {img.shape}")
    N, PH, PW, Cin = img.shape
    R = check_photo_table(table16, Cin).astype(np.int64)
    if len(R) != N:
        raise ValueError(f"{len(R)} photo rows for {N} windows")
    row = lambda q: R[:, q][:, None, None, None]
    p = img.astype(np.int64)
    if Cin == 3:
        u = np.einsum("ncd,nijd->nijc", R[:, :9].reshape(N, 3, 3), p) + R[:, 9:12][:, None, None, :]
    else:
        u = row(0) * p + row(9)
    u = np.clip((u + 32768) >> 16, 0, 255)
    v = np.clip(u + ((row(12) * u * (255 - u) + (1 << 23)) >> 24), 0, 255)
    idx = np.arange(PH * PW * Cin, dtype=np.uint32).reshape(1, PH, PW, Cin)
    x = R[:, 14].astype(np.uint32)[:, None, None, None] + (idx + np.uint32(1)) * np.uint32(0x9E3779B9)      # uint32 arrays wrap
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7FEB352D)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846CA68B)
    x ^= x >> np.uint32(16)
    x = x.astype(np.int64)
    z = (x & 255) + ((x >> 8) & 255) + ((x >> 16) & 255) + (x >> 24) - 510
    return np.clip(v + ((row(13) * z + 32768) >> 16), 0, 255).astype(np.uint8)       # A == 0 adds (32768 >> 16) = 0


def photo_rows(n: int, brightness=0.0, contrast=1.0, saturation=1.0, hue_deg=0.0, tone=0.0, noise_sigma=0.0, seeds=0) -> np.ndarray:
    """int32 [n][16] photo rows; every argument a scalar or a length-n array.  In float64 M = contrast * Sat(saturation) * Hue(hue_deg)
    with Sat(s) = s I + (1 - s) 1 w^T, w = (0.299, 0.587, 0.114), and Hue the rotation by hue_deg about the grey axis (1, 1, 1) / sqrt 3
    - both fix the grey axis, so grey stays grey; b = brightness * 255 + (1 - contrast) * 127.5 on every channel (contrast turns about
    mid-grey), t = tone, A = noise_sigma / SIGMA_Z (noise_sigma in levels); each times 65536 and rounded with np.rint.  The defaults
    give the identity row exactly.  ValueError (check_photo_table's) for a row beyond the kernel's limits."""
    n = int(n)
    per = lambda v: np.broadcast_to(np.asarray(v, np.float64), (n,))
    br, co, sa, th, to, sg = per(brightness), per(contrast), per(saturation), np.deg2rad(per(hue_deg)), per(tone), per(noise_sigma)
    I, w = np.eye(3), np.array([0.299, 0.587, 0.114])
    sat = sa[:, None, None] * I + (1.0 - sa)[:, None, None] * np.broadcast_to(w, (3, 3))
    K = np.array([[0.0, -1.0, 1.0], [1.0, 0.0, -1.0], [-1.0, 1.0, 0.0]]) / np.sqrt(3.0)          # the cross product with the grey axis
    hue = np.cos(th)[:, None, None] * I + (1.0 - np.cos(th))[:, None, None] * np.full((3, 3), 1.0 / 3.0) + np.sin(th)[:, None, None] * K
    out = np.zeros((n, 16), np.int64)
    out[:, :9] = np.rint(Q16 * (co[:, None, None] * (sat @ hue))).reshape(n, 9)
    out[:, 9:12] = np.rint(Q16 * (br * 255.0 + (1.0 - co) * 127.5))[:, None]
    out[:, 12] = np.rint(Q16 * to)
    out[:, 13] = np.rint(Q16 * sg / SIGMA_Z)
    out[:, 14] = np.broadcast_to(np.asarray(seeds, np.int64), (n,))
    return check_photo_table(out, 3)


class PhotoJitter:
    """The random part of SceneLoader's photometric augmentation: brightness uniform in [-brightness, brightness] (of full scale),
    contrast and saturation log-uniform in their (lo, hi), the hue angle uniform in [-hue_deg, hue_deg], the tone uniform in
    [-tone, tone], the noise sigma (in levels) uniform in its (lo, hi), one noise seed per window."""

    def __init__(self, brightness: float = 0.1, contrast: Tuple[float, float] = (0.8, 1.25), saturation: Tuple[float, float] = (0.8, 1.25),
                 hue_deg: float = 8.0, tone: float = 0.4, noise_sigma: Tuple[float, float] = (0.0, 3.0)):
        for name, (lo, hi) in (("contrast", contrast), ("saturation", saturation)):
            if not 0 < float(lo) <= float(hi):
                raise ValueError(f"{name} range ({lo}, {hi}): 0 < lo <= hi")
        if not 0 <= float(noise_sigma[0]) <= float(noise_sigma[1]):
            raise ValueError(f"noise_sigma range ({noise_sigma[0]}, {noise_sigma[1]}): 0 <= lo <= hi")
        if brightness < 0 or hue_deg < 0 or tone < 0:
            raise ValueError(f"brightness {brightness}, hue_deg {hue_deg} and tone {tone} are magnitudes (>= 0)")
        if tone > 1:
            raise ValueError(f"tone {tone} above 1: the curve is monotone only up to 1")
        self.brightness, self.hue_deg, self.tone = float(brightness), float(hue_deg), float(tone)
        self.contrast, self.saturation = (float(contrast[0]), float(contrast[1])), (float(saturation[0]), float(saturation[1]))
        self.noise_sigma = (float(noise_sigma[0]), float(noise_sigma[1]))

    def draw(self, rng: np.random.Generator, n: int, channels: int = 3) -> np.ndarray:
        """The int32 [n][16] photo table of n windows: brightness, contrast, saturation, hue, tone, sigma and seeds - drawn in this
        order from rng, whatever `channels` is.  channels != 3: saturation and hue stay out of the rows, which are scalar then."""
        log_uniform = lambda r: np.exp(rng.uniform(np.log(r[0]), np.log(r[1]), n))
        br = rng.uniform(-self.brightness, self.brightness, n)
        co, sa = log_uniform(self.contrast), log_uniform(self.saturation)
        hue = rng.uniform(-self.hue_deg, self.hue_deg, n)
        tone = rng.uniform(-self.tone, self.tone, n)
        sigma = rng.uniform(self.noise_sigma[0], self.noise_sigma[1], n)
        seeds = rng.integers(0, 1 << 31, n, dtype=np.int64)
        if channels != 3:
            sa, hue = 1.0, 0.0
        return check_photo_table(photo_rows(n, br, co, sa, hue, tone, sigma, seeds), channels)


# ---- whole-scene prediction: windows that cover a scene, every pixel owned by one of them -----------------------------------------
MAX_CLASSES = 64


def _axis_cover(L: int, P: int, S: int):
    """One axis of predict_table: (origins [K], owned intervals [K][2] in scene coordinates)."""
    K = -(-(L - P) // S) + 1
    o = np.minimum(np.arange(K, dtype=np.int64) * S, L - P)
    b = np.empty(K + 1, np.int64)
    b[0], b[K] = 0, L
    b[1:K] = (o[:-1] + P + o[1:]) // 2                          # half way through the overlap of windows k and k + 1
    return o, np.stack([b[:-1], b[1:]], 1)


def predict_table(shape_hw: Sequence[int], patch, stride: int):
    """(rows, own), both int32 [N][4]: windows that cover an H x W scene and the part of each that is predicted from it.
    Per axis of length L (patch P, stride S, 1 <= S <= P <= L): origins o_k = min(k S, L - P) for k < K = ceil((L - P) / S) + 1 - the
    last window is flush with the border -, cuts b_-1 = 0, b_k = (o_k + P + o_{k+1}) // 2, b_{K-1} = L; window k owns [b_{k-1}, b_k),
    which lies inside [o_k, o_k + P) since S <= P.  Every scene pixel is owned exactly once, by the window it is most central in.
    rows: (0, row, col, 0), row-major over (row index, column index) - what rua_scene_windows reads; own: (r0, r1, c0, c1) in
    window coordinates.  With S == P and L % P == 0 these are the non-overlapping tiles in row-major order, each owned in full.
    patch and stride may be (rows, columns) pairs."""
    ph, pw = _patch2(patch)
    H, W = int(shape_hw[0]), int(shape_hw[1])
    pair = stride if isinstance(stride, (tuple, list)) and len(stride) == 2 else (stride, stride)     # (rows, columns), as patch
    if any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in pair):
        raise ValueError(f"stride {stride!r} must be an integer (or a pair of them: rows, columns)")
    sh, sw = int(pair[0]), int(pair[1])
    for L, P, S, what in ((H, ph, sh, "rows"), (W, pw, sw, "columns")):
        if not 1 <= S <= P <= L:
            raise ValueError(f"predict_table: {what}: stride {S}, patch {P}, scene {L} (1 <= stride <= patch <= scene)")
    (orow, brow), (ocol, bcol) = _axis_cover(H, ph, sh), _axis_cover(W, pw, sw)
    rows = np.zeros((len(orow), len(ocol), 4), np.int32)
    own = np.empty((len(orow), len(ocol), 4), np.int32)
    rows[..., 1], rows[..., 2] = orow[:, None], ocol[None, :]
    own[..., 0:2] = (brow - orow[:, None])[:, None, :]
    own[..., 2:4] = (bcol - ocol[:, None])[None, :, :]
    return rows.reshape(-1, 4), own.reshape(-1, 4)


def check_own(shapes: Sequence[Sequence[int]], rows: np.ndarray, own: np.ndarray, patch, num_classes: int = 1):
    """(rows, own) as contiguous int32 [N][4] arrays; ValueError, in rua_scene_stitch's own words, for the first violation."""
    ph, pw = _patch2(patch)
    t, o = _two_tables("rua_scene_stitch", rows, own, "0")
    n = len(shapes)
    if n < 1 or t.shape[0] < 1 or o.shape[0] != t.shape[0]:
        raise ValueError(f"rua_scene_stitch: nscenes {n}, N {t.shape[0]} windows, {o.shape[0]} ownership rows (both >= 1, one per window)")
    if not (1 <= ph <= MAX_PATCH and 1 <= pw <= MAX_PATCH):
        raise ValueError(f"rua_scene_stitch: PH {ph}, PW {pw} (1 <= PH, PW <= 512)")
    if not 1 <= num_classes <= MAX_CLASSES:
        raise ValueError(f"rua_scene_stitch: C {num_classes} outside 1..64")
    _check_rows("rua_scene_stitch", shapes, t.tolist(), ph, pw, own=o.tolist(), code0=True)
    return np.ascontiguousarray(t, dtype=np.int32), np.ascontiguousarray(o, dtype=np.int32)


def host_stitch(p: np.ndarray, rows: np.ndarray, own: np.ndarray, shapes: Sequence[Sequence[int]],
                class_maps: Optional[Sequence[np.ndarray]] = None, num_classes: Optional[int] = None, fill: int = 0):
    """The numpy definition of what rua_scene_stitch writes.  p: [N][PH][PW][C] class probabilities of the windows `rows`; for every
    (i, j) of window n's owned rectangle pred = np.argmax(p[n, i, j]) (the first index of the maximum) goes to
    maps[scene][row + i, col + j] and, where class maps are given and the label t there is < C, confusion[t, pred] += 1.
    Returns (uint8 [H][W] map per scene of `shapes`, unowned pixels holding `fill`; int64 [C][C] confusion matrix indexed
    [true][pred], None without class maps)."""
    p = np.asarray(p)
    if p.ndim != 4 or len(p) != len(np.asarray(rows)):
        raise ValueError(f"p is [N][PH][PW][C] with one window per table row, got {p.shape} for {len(np.asarray(rows))} rows")
    C = int(p.shape[3]) if num_classes is None else int(num_classes)
    if C != p.shape[3]:
        raise ValueError(f"p holds {p.shape[3]} classes, num_classes is {C}")
    t, o = check_own(shapes, rows, own, p.shape[1:3], C)
    return _score_groups(t, o, 1, shapes, class_maps, C, fill, lambda k, r0, r1, c0, c1: p[k, r0:r1, c0:c1])


def _score_groups(t, o, K: int, shapes, class_maps, C: int, fill: int, values):
    """The map-and-matrix half of host_stitch and host_stitch_views: the arg-max of values(g, r0, r1, c0, c1), group g's
    [r1 - r0][c1 - c0][C] array, goes to the scene maps (unowned: `fill`) and into the confusion matrix (None without class maps)."""
    maps = [np.full((int(h), int(w)), fill, np.uint8) for h, w in shapes]
    cm = None if class_maps is None else np.zeros((C, C), np.int64)
    for g, (r0, r1, c0, c1) in enumerate(o.tolist()):
        if r0 == r1 or c0 == c1:
            continue
        s, row, col, _ = t[g * K].tolist()
        pred = np.argmax(values(g, r0, r1, c0, c1), axis=-1)
        maps[s][row + r0:row + r1, col + c0:col + c1] = pred
        if cm is not None:
            true = np.asarray(class_maps[s])[row + r0:row + r1, col + c0:col + c1].astype(np.int64)
            keep = true < C
            cm += np.bincount(true[keep] * C + pred[keep], minlength=C * C).reshape(C, C)
    return maps, cm


# ---- test-time augmentation: a window predicted under K symmetries (its views), the probabilities summed ------------------------
INVERSE = (0, 5, 2, 3, 4, 1, 6, 7)            # transform(transform(w, c), INVERSE[c]) is w
VIEW_SETS = {"none": (0,), "flips": (0, 3, 4), "aug5": (0, 1, 2, 3, 4), "all": (0, 1, 2, 3, 4, 5, 6, 7)}
MAX_VIEWS = 8


def check_views(views, patch=None) -> Tuple[int, ...]:
    """The views as a tuple of codes: a VIEW_SETS name or 1 to 8 distinct codes in 0..7, a transposing one only with a square patch
    (patch None: not checked).  ValueError, in rua_scene_stitch_views' own words where it has any."""
    if isinstance(views, str):
        if views not in VIEW_SETS:
            raise ValueError(f"views {views!r}: not one of {sorted(VIEW_SETS)} (or a list of codes 0..7)")
        views = VIEW_SETS[views]
    try:
        v = tuple(views)
    except TypeError:
        raise ValueError(f"views {views!r}: a name of {sorted(VIEW_SETS)} or a sequence of codes 0..7") from None
    if any(isinstance(c, bool) or not isinstance(c, (int, np.integer)) for c in v):
        raise ValueError(f"views {views!r}: the codes are integers 0..7")
    v = tuple(int(c) for c in v)
    if not 1 <= len(v) <= MAX_VIEWS:
        raise ValueError(f"rua_scene_stitch_views: K {len(v)} outside 1..8")
    for k, c in enumerate(v):
        if not 0 <= c < NUM_CODES:
            raise ValueError(f"rua_scene_stitch_views: row {k}: code {c} outside 0..7")
        if c in v[:k]:
            raise ValueError(f"views {v}: code {c} occurs twice")
    if patch is not None:
        ph, pw = _patch2(patch)
        for k, c in enumerate(v):
            if ph != pw and c in TRANSPOSING:
                raise ValueError(f"rua_scene_stitch_views: row {k}: code {c} transposes and needs a square patch (got {ph} x {pw})")
    return v


def view_rows(rows: np.ndarray, views) -> np.ndarray:
    """int32 [G*K][4]: rows g*K .. g*K+K-1 repeat row g of the code-0 table `rows` [G][4] with the codes of `views`, in that order."""
    v = check_views(views)
    r = _window_table(rows)
    out = np.repeat(r.astype(np.int32), len(v), axis=0)
    out[:, 3] = np.tile(np.asarray(v, np.int32), len(r))
    return out


def check_view_table(shapes: Sequence[Sequence[int]], rows: np.ndarray, own: np.ndarray, views_or_K, patch, num_classes: int = 1):
    """(rows [G*K][4], own [G][4], K) as contiguous int32 arrays; ValueError, in rua_scene_stitch_views' own words, for the first
    violation.  views_or_K: K, or the views every group must carry in order (then check_views applies to them too)."""
    ph, pw = _patch2(patch)
    t, o = _two_tables("rua_scene_stitch_views", rows, own, "code")
    views = None
    if isinstance(views_or_K, (int, np.integer)) and not isinstance(views_or_K, bool):
        K = int(views_or_K)
    else:
        views = check_views(views_or_K, patch)
        K = len(views)
    n, G = len(shapes), o.shape[0]
    if n < 1 or G < 1:
        raise ValueError(f"rua_scene_stitch_views: nscenes {n}, G {G} (both >= 1)")
    if not 1 <= K <= MAX_VIEWS:
        raise ValueError(f"rua_scene_stitch_views: K {K} outside 1..8")
    if t.shape[0] != G * K:
        raise ValueError(f"rua_scene_stitch_views: {t.shape[0]} window rows for {G} groups of K {K} views (K rows per ownership row)")
    if not 1 <= num_classes <= MAX_CLASSES:
        raise ValueError(f"rua_scene_stitch_views: C {num_classes} outside 1..64")
    if not (1 <= ph <= MAX_PATCH and 1 <= pw <= MAX_PATCH):
        raise ValueError(f"rua_scene_stitch_views: PH {ph}, PW {pw} (1 <= PH, PW <= 512)")
    _check_rows("rua_scene_stitch_views", shapes, t.tolist(), ph, pw, own=o.tolist(), K=K, views=views)
    return np.ascontiguousarray(t, dtype=np.int32), np.ascontiguousarray(o, dtype=np.int32), K


def host_stitch_views(p: np.ndarray, rows: np.ndarray, own: np.ndarray, shapes: Sequence[Sequence[int]],
                      class_maps: Optional[Sequence[np.ndarray]] = None, num_classes: Optional[int] = None, fill: int = 0):
    """The numpy definition of what rua_scene_stitch_views writes.  p: [G*K][PH][PW][C] float32, the class probabilities of the K
    views of G windows (rows [G*K][4], view_rows' layout; own [G][4]; K = len(rows) // len(own)).  For group g the views are turned
    back, q_k = transform(p[g*K + k], INVERSE[code_k]), and summed in float32 strictly in view order: s = q_0, then s = s + q_k - no
    pairwise sum, no wider accumulator, no division.  pred = np.argmax(s[i, j]) for every (i, j) of the owned rectangle; the map and
    the confusion matrix follow as in host_stitch, whose result this is for K = 1 and code 0."""
    p = np.asarray(p)
    r, o = np.asarray(rows), np.asarray(own)
    if o.ndim != 2 or len(o) < 1 or r.ndim != 2 or len(r) % len(o):
        raise ValueError(f"rows is [G*K][4] and own [G][4]: {len(r)} rows are no multiple of {len(o)} ownership rows")
    if p.ndim != 4 or len(p) != len(r):
        raise ValueError(f"p is [G*K][PH][PW][C] with one view per table row, got {p.shape} for {len(r)} rows")
    if p.dtype != np.float32:
        raise ValueError(f"p is float32 (the sums are defined in it), got {p.dtype}")
    C = int(p.shape[3]) if num_classes is None else int(num_classes)
    if C != p.shape[3]:
        raise ValueError(f"p holds {p.shape[3]} classes, num_classes is {C}")
    t, o, K = check_view_table(shapes, r, o, len(r) // len(o), p.shape[1:3], C)

    def summed(g, r0, r1, c0, c1):
        acc = None
        for k in range(K):
            q = transform(p[g * K + k], INVERSE[int(t[g * K + k, 3])])[r0:r1, c0:c1]
            acc = q.astype(np.float32, copy=True) if acc is None else acc + q
        assert acc.dtype == np.float32
        return acc

    return _score_groups(t, o, K, shapes, class_maps, C, fill, summed)


# ---- whole-scene maps of any head: the window outputs under K views, turned back, averaged and quantised to uint8 ---------------
MAP_MODES = {"plain": 0, "hsv_rgb": 1}
MAP_HEADS = ("seg", "bound", "dist", "color", "color_rgb")     # what predict_scene(heads=) takes; color_rgb is the colour head in mode 1


def quantise_q16(x) -> np.ndarray:
    """float32 of any shape -> int64 a = rint(min(max(x, 0), 1) * 65536), ties to even; NaN and -inf give 0, +inf 65536.  The
    multiply is by a power of two and exact, so from here on a map is a function of integers (rua_scene_stitch_maps: sm_q16)."""
    x = np.asarray(x)
    if x.dtype != np.float32:
        raise ValueError(f"quantise_q16 is defined on float32, got {x.dtype}")
    y = np.where(x > 0, x, np.float32(0))                       # NaN > 0 is False
    y = np.minimum(y, np.float32(1))
    a = np.rint(y * np.float32(65536))
    assert a.dtype == np.float32
    return a.astype(np.int64)


def hsv_to_rgb_u8(hsv) -> np.ndarray:
    """uint8 [..., 3] HSV with H in 0..179 (degrees / 2, as labels.rgb_to_hsv_u8 gives it), S and V in 0..255 -> uint8 [..., 3] RGB:
    the textbook sector formula rounded exactly, in integers.  sec = h // 30, f = h % 30, p = (v (255 - s) + 127) // 255,
    q = (v (7650 - s f) + 3825) // 7650, t = (v (7650 - s (30 - f)) + 3825) // 7650 and (r, g, b) = (v,t,p), (q,v,p), (p,v,t),
    (p,q,v), (t,p,v), (v,p,q) for sec 0..5.  ValueError for an H above 179."""
    a = np.asarray(hsv)
    if a.dtype != np.uint8 or a.ndim < 1 or a.shape[-1] != 3:
        raise ValueError(f"hsv_to_rgb_u8 takes uint8 [..., 3], got {a.dtype} {a.shape}")
    h, s, v = (a[..., k].astype(np.int64) for k in range(3))
    if h.size and int(h.max()) > 179:
        raise ValueError(f"hsv_to_rgb_u8: H {int(h.max())} above 179 (H is degrees / 2)")
    sec, f = h // 30, h % 30
    p = (v * (255 - s) + 127) // 255
    q = (v * (7650 - s * f) + 3825) // 7650
    t = (v * (7650 - s * (30 - f)) + 3825) // 7650
    r = np.choose(sec, [v, q, p, p, t, v])
    g = np.choose(sec, [t, v, v, q, p, p])
    b = np.choose(sec, [p, p, t, v, v, q])
    return np.stack([r, g, b], axis=-1).astype(np.uint8)


def host_stitch_maps(p: np.ndarray, rows: np.ndarray, own: np.ndarray, shapes: Sequence[Sequence[int]], K: int, mode: str = "plain",
                     maps: Optional[Sequence[np.ndarray]] = None, patch=None) -> List[np.ndarray]:
    """The numpy definition of what rua_scene_stitch_maps writes.  p: float32 [G*K][PH][PW][Ch], any head's outputs for the K views
    of G windows (rows [G*K][4], view_rows' layout; own [G][4]; the checks are check_view_table's).  Returns one uint8 [H][W][Ch] map
    per scene of `shapes`: `maps` (written in place, only inside the owned rectangles) or fresh ones that start at 0.  With q_k view
    k turned back (INVERSE) and a_k = quantise_q16(q_k[i][j][c]):
      mode "plain":    A = sum of a_k;  out = (255 A + K 32768) // (K 65536), the rounded mean in 0..255;
      mode "hsv_rgb":  (Ch = 3) per view h = 179 a_k[0] >> 16, s = 255 a_k[1] >> 16, v = 255 a_k[2] >> 16 (truncation, as the
                       reference's (hsv * [179, 255, 255]).astype(uint8)), rgb_k = hsv_to_rgb_u8; out = (2 sum of rgb_k + K) // (2 K).
                       The views are averaged in RGB: hue is circular, and the mean of two reds at 0.005 and 0.995 would be cyan.
    Integers from the first step on: the order of the views cannot matter.  patch: (PH, PW) to hold p against (None: p's own)."""
    p = np.asarray(p)
    if mode not in MAP_MODES:
        raise ValueError(f"rua_scene_stitch_maps: mode {mode!r} (one of {sorted(MAP_MODES)})")
    if p.ndim != 4 or p.dtype != np.float32:
        raise ValueError(f"p is float32 [G*K][PH][PW][Ch], got {p.dtype} {p.shape}")
    ph, pw = _patch2(p.shape[1:3] if patch is None else patch)
    if (ph, pw) != tuple(p.shape[1:3]):
        raise ValueError(f"p holds {p.shape[1]} x {p.shape[2]} windows, the patch is {ph} x {pw}")
    Ch = int(p.shape[3])
    if mode == "hsv_rgb" and Ch != 3:
        raise ValueError(f"rua_scene_stitch_maps: mode 1 (hsv_rgb) reads H, S, V: Ch 3, got {Ch}")
    if isinstance(K, bool) or not isinstance(K, (int, np.integer)):
        raise ValueError(f"K {K!r} must be an integer")
    t, o, K = check_view_table(shapes, rows, own, int(K), (ph, pw), Ch)
    if len(p) != len(t):
        raise ValueError(f"p is [G*K][PH][PW][Ch] with one view per table row, got {p.shape} for {len(t)} rows")
    if maps is None:
        maps = [np.zeros((int(h), int(w), Ch), np.uint8) for h, w in shapes]
    else:
        maps = list(maps)
        for m, (h, w) in zip(maps, shapes):
            if not isinstance(m, np.ndarray) or m.dtype != np.uint8 or m.shape != (int(h), int(w), Ch):
                raise ValueError(f"a given map is a uint8 array [{h}][{w}][{Ch}], got {getattr(m, 'dtype', type(m))} {getattr(m, 'shape', '')}")
        if len(maps) != len(shapes):
            raise ValueError(f"{len(maps)} maps for {len(shapes)} scenes")
    for g, (r0, r1, c0, c1) in enumerate(o.tolist()):
        if r0 == r1 or c0 == c1:
            continue
        s, row, col, _ = t[g * K].tolist()
        acc = np.zeros((r1 - r0, c1 - c0, Ch), np.int64)
        for k in range(K):
            a = quantise_q16(transform(p[g * K + k], INVERSE[int(t[g * K + k, 3])])[r0:r1, c0:c1])
            if mode == "plain":
                acc += a
            else:
                hsv = np.stack([(179 * a[..., 0]) >> 16, (255 * a[..., 1]) >> 16, (255 * a[..., 2]) >> 16], axis=-1)
                acc += hsv_to_rgb_u8(hsv.astype(np.uint8))
        out = (255 * acc + K * 32768) // (K * 65536) if mode == "plain" else (2 * acc + K) // (2 * K)
        maps[s][row + r0:row + r1, col + c0:col + c1] = out
    return maps


# ---- multi-scale test-time augmentation: a scene covered at several zooms, the passes summed in a scene-sized accumulator --------
MAX_SCALES = 8
_ACC = "rua_scene_accumulate"


def scale_footprint(patch, zoom) -> Tuple[int, int]:
    """The footprint F = (FH, FW) of a scale: the scene pixels per axis that one PH x PW window covers at `zoom` (> 1 zooms in, as in
    affine_rows), F = floor(P / zoom + 1/2).  ValueError unless 1 <= F, P <= 4 F and F <= 4 P on both axes: 4 is
    rua_scene_windows_affine's coefficient limit (Q16), and a window that covers less than a quarter of its pixels says little."""
    ph, pw = _patch2(patch)
    if isinstance(zoom, bool) or not isinstance(zoom, (int, float, np.integer, np.floating)) or not np.isfinite(zoom) or not zoom > 0:
        raise ValueError(f"scale_footprint: zoom {zoom!r} must be a positive number")
    f = tuple(int(np.floor(p / float(zoom) + 0.5)) for p in (ph, pw))
    for P, F, what in ((ph, f[0], "rows"), (pw, f[1], "columns")):
        if not (1 <= F and P <= 4 * F and F <= 4 * P):
            raise ValueError(f"scale_footprint: {what}: zoom {zoom} gives a footprint of {F} for a patch of {P} (1 <= F, P <= 4 F, F <= 4 P)")
    return f


def scale_table(shape_hw: Sequence[int], patch, footprint, stride, views=(0,)):
    """One pass of a multi-scale prediction: (rows7 int32 [G*K][7], own int32 [G][4]).  The cover is predict_table(shape_hw, F, SF) with
    the stride scaled to the footprint, SF = clamp(rint(stride F / P), 1, F) per axis; group g is footprint g of the cover, `own` its
    owned rectangle (r0, r1, c0, c1) in ABSOLUTE scene coordinates, and its K rows - consecutive, in the order of `views`, view_rows'
    layout - are the affine rows (scene 0) that cut the footprint into a PH x PW window under view code c:
    A = diag(a_y, a_x) SYMMETRY[c], a_y = rint(65536 FH / PH), a_x likewise, the origin by affine_rows' rule with the footprint's
    centre in place of the window's.  All integers.  With F == P and code 0 host_windows_affine of the rows is host_windows of the cover."""
    ph, pw, fh, fw, rows4, own4 = _scale_cover(shape_hw, patch, footprint, stride)
    v = check_views(views, (ph, pw))
    G, K = len(rows4), len(v)
    r, c = rows4[:, 1].astype(np.int64), rows4[:, 2].astype(np.int64)
    own = own4.astype(np.int64)
    own[:, 0:2] += r[:, None]
    own[:, 2:4] += c[:, None]
    ay, ax = (2 * Q16 * fh + ph) // (2 * ph), (2 * Q16 * fw + pw) // (2 * pw)
    A = SYMMETRY[list(v)] * np.array([[ay], [ax]], np.int64)                    # [K][2][2]: diag(a_y, a_x) S
    rows7 = np.zeros((G, K, 7), np.int64)
    rows7[:, :, 3:] = A.reshape(K, 4)[None]
    rows7[:, :, 1] = ((2 * r + fh - 1) * (Q16 // 2))[:, None] - ((A[:, 0, 0] * (ph - 1) + A[:, 0, 1] * (pw - 1)) >> 1)[None, :]
    rows7[:, :, 2] = ((2 * c + fw - 1) * (Q16 // 2))[:, None] - ((A[:, 1, 0] * (ph - 1) + A[:, 1, 1] * (pw - 1)) >> 1)[None, :]
    if (np.abs(rows7) > 2 ** 31 - 1).any():
        raise ValueError("scale_table: a row leaves the int32 range")
    return rows7.reshape(G * K, 7).astype(np.int32), own.astype(np.int32)


def _scaled_stride(patch, footprint, stride, fn: str = "scale_table"):
    """(PH, PW, FH, FW, (SFH, SFW)): scale_table's arguments read, and the stride scaled to the footprint, SF = clamp(rint(stride F / P), 1, F)."""
    ph, pw = _patch2(patch)
    fh, fw = _patch2(footprint)
    pair = stride if isinstance(stride, (tuple, list)) and len(stride) == 2 else (stride, stride)
    if any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in pair):
        raise ValueError(f"stride {stride!r} must be an integer (or a pair of them: rows, columns)")
    for P, F, S, what in ((ph, fh, int(pair[0]), "rows"), (pw, fw, int(pair[1]), "columns")):
        if not (1 <= F and P <= 4 * F and F <= 4 * P):
            raise ValueError(f"{fn}: {what}: footprint {F}, patch {P} (1 <= F, P <= 4 F, F <= 4 P)")
        if not 1 <= S <= P:
            raise ValueError(f"{fn}: {what}: stride {S}, patch {P} (1 <= stride <= patch)")
    sf = tuple(min(max((2 * int(S) * F + P) // (2 * P), 1), F) for S, F, P in ((pair[0], fh, ph), (pair[1], fw, pw)))
    return ph, pw, fh, fw, sf


def _scale_cover(shape_hw, patch, footprint, stride):
    """(PH, PW, FH, FW, rows4, own4): the cover predict_table(shape_hw, F, SF) of one pass, the stride scaled to the footprint."""
    ph, pw, fh, fw, sf = _scaled_stride(patch, footprint, stride)
    rows4, own4 = predict_table(shape_hw, (fh, fw), sf)
    return ph, pw, fh, fw, rows4, own4


def check_scales(scales, patch, shape_hw=None) -> Optional[Tuple[Tuple[int, int], ...]]:
    """predict_scene's scales as footprints: None for None or (1.0,) - the single-scale path -, otherwise one scale_footprint per zoom
    of a tuple of 1 to 8 distinct positive zooms with distinct footprints, each no larger than the scene (shape_hw None: not checked)."""
    if scales is None:
        return None
    if isinstance(scales, (str, bytes)):
        raise ValueError(f"scales {scales!r}: a tuple of 1 to {MAX_SCALES} distinct positive zooms")
    try:
        z = tuple(scales)
    except TypeError:
        raise ValueError(f"scales {scales!r}: a tuple of 1 to {MAX_SCALES} distinct positive zooms") from None
    if not 1 <= len(z) <= MAX_SCALES:
        raise ValueError(f"scales {scales!r}: a tuple of 1 to {MAX_SCALES} distinct positive zooms")
    fps = tuple(scale_footprint(patch, zoom) for zoom in z)
    for k, zoom in enumerate(z):
        if any(float(zoom) == float(y) for y in z[:k]):
            raise ValueError(f"scales {z}: zoom {zoom} occurs twice")
        if fps[k] in fps[:k]:
            raise ValueError(f"scales {z}: zooms {z[fps.index(fps[k])]} and {zoom} give the same footprint {fps[k][0]} x {fps[k][1]}")
        if shape_hw is not None and (fps[k][0] > int(shape_hw[0]) or fps[k][1] > int(shape_hw[1])):
            raise ValueError(f"scales {z}: zoom {zoom} gives a footprint of {fps[k][0]} x {fps[k][1]}, larger than the "
                             f"{int(shape_hw[0])} x {int(shape_hw[1])} scene")
    if len(z) == 1 and float(z[0]) == 1.0:
        return None
    return fps


def _axis_w(y: int, o: int, a: int) -> int:
    """The unclamped window coordinate, in 1/256 pixels, of scene coordinate y on an axis with origin o and coefficient a != 0 (Q16)."""
    t = y * Q16 - o
    if a < 0:
        t, a = -t, -a
    return (t * 256 + (a >> 1)) // a


def _axis_taps(lo: int, hi: int, o: int, a: int, n: int):
    """(i0, i1, f), int64 [hi - lo] each: the two window indices and the weight of the second, in 1/256, for scene coordinates lo..hi-1."""
    w = np.array([_axis_w(y, o, a) for y in range(lo, hi)], np.int64).reshape(-1)
    w = np.clip(w, 0, (n - 1) * 256)
    i0 = w >> 8
    return i0, np.minimum(i0 + 1, n - 1), w & 255


def _check_accumulate(fn: str, shapes, rows7, own, K, patch, num_classes: int, one_size: bool):
    """check_accumulate and check_accumulate_blend under the entry point's name `fn`; one_size: the non-empty rectangles have one size."""
    ph, pw = _patch2(patch)
    size, first = None, 0
    t, o = np.asarray(rows7), np.asarray(own)
    if t.ndim != 2 or t.shape[1] != 7 or not np.issubdtype(t.dtype, np.integer) or not _is_table4(o):
        raise ValueError(f"{fn} takes integer [G*K][7] rows (scene, y0, x0, a_yy, a_yx, a_xy, a_xx) and [G][4] rows (r0, r1, c0, c1), "
                         f"got {t.dtype} {t.shape} and {o.dtype} {o.shape}")
    if isinstance(K, bool) or not isinstance(K, (int, np.integer)):
        raise ValueError(f"K {K!r} must be an integer")
    K, n, G = int(K), len(shapes), o.shape[0]
    if n < 1 or G < 1:
        raise ValueError(f"{fn}: nscenes {n}, G {G} (both >= 1)")
    if not 1 <= K <= MAX_VIEWS:
        raise ValueError(f"{fn}: K {K} outside 1..8")
    if t.shape[0] != G * K:
        raise ValueError(f"{fn}: {t.shape[0]} window rows for {G} groups of K {K} views (K rows per ownership row)")
    if not 1 <= num_classes <= MAX_CLASSES:
        raise ValueError(f"{fn}: C {num_classes} outside 1..64")
    if not (1 <= ph <= MAX_PATCH and 1 <= pw <= MAX_PATCH):
        raise ValueError(f"{fn}: PH {ph}, PW {pw} (1 <= PH, PW <= 512)")
    for s, shp in enumerate(shapes):
        if not (1 <= int(shp[0]) <= MAX_SCENE and 1 <= int(shp[1]) <= MAX_SCENE):
            raise ValueError(f"{fn}: scene {s}: size {int(shp[0])} x {int(shp[1])} (1 <= H, W <= 16384)")
    rows, owns = t.tolist(), o.tolist()
    for g in range(G):
        s0 = rows[g * K][0]
        for v in range(K):
            k = g * K + v
            s, _, _, ayy, ayx, axy, axx = rows[k]
            if not 0 <= s < n:
                raise ValueError(f"{fn}: row {k}: scene {s} outside 0..{n - 1}")
            if s != s0:
                raise ValueError(f"{fn}: row {k}: scene {s}, but its group {g} is scene {s0}")
            keeps, turns = ayx == 0 and axy == 0 and ayy != 0 and axx != 0, ayy == 0 and axx == 0 and ayx != 0 and axy != 0
            if not (keeps or turns):
                raise ValueError(f"{fn}: row {k}: matrix ({ayy}, {ayx}, {axy}, {axx}) is not axis-aligned "
                                 "(a_yx = a_xy = 0 or a_yy = a_xx = 0, the other two nonzero)")
            if turns and ph != pw:
                raise ValueError(f"{fn}: row {k}: matrix ({ayy}, {ayx}, {axy}, {axx}) transposes and needs a square patch (got {ph} x {pw})")
        H, W = int(shapes[s0][0]), int(shapes[s0][1])
        r0, r1, c0, c1 = owns[g]
        if not (0 <= r0 <= r1 <= H and 0 <= c0 <= c1 <= W):
            raise ValueError(f"{fn}: group {g}: rectangle rows {r0}..{r1}, columns {c0}..{c1} outside its {H} x {W} scene")
        if r0 == r1 or c0 == c1:
            continue
        if one_size and size is None:
            size, first = (r1 - r0, c1 - c0), g
        if one_size and (r1 - r0, c1 - c0) != size:
            raise ValueError(f"{fn}: group {g}: rectangle of {r1 - r0} x {c1 - c0}, but group {first} has {size[0]} x {size[1]} (the footprints of one call have one size)")
        for v in range(K):
            k = g * K + v
            _, y0, x0, ayy, ayx, axy, axx = rows[k]
            ay, ny, ax, nx = (ayy, ph, axx, pw) if ayx == 0 else (ayx, pw, axy, ph)
            ends = [(_axis_w(y, y0, ay), ny) for y in (r0, r1 - 1)] + [(_axis_w(x, x0, ax), nx) for x in (c0, c1 - 1)]
            if any(not -256 <= w <= m * 256 for w, m in ends):
                raise ValueError(f"{fn}: row {k}: rectangle rows {r0}..{r1}, columns {c0}..{c1} of group {g} leaves the window's footprint")
    return np.ascontiguousarray(t, dtype=np.int32), np.ascontiguousarray(o, dtype=np.int32)


def check_accumulate(shapes: Sequence[Sequence[int]], rows7, own, K, patch, num_classes: int = 1):
    """(rows7 [G*K][7], own [G][4]) as contiguous int32 arrays; ValueError, in rua_scene_accumulate's own words, for the first violation."""
    return _check_accumulate(_ACC, shapes, rows7, own, K, patch, num_classes, False)


def host_accumulate(p: np.ndarray, rows7, own, shapes: Sequence[Sequence[int]], K: int, acc: Optional[Sequence[np.ndarray]] = None) -> List[np.ndarray]:
    """The numpy definition of what rua_scene_accumulate adds: the way back of scale_table.  p: float32 [G*K][PH][PW][C], the class
    probabilities of the K views of G windows cut by the affine rows rows7 [G*K][7]; own [G][4]: each group's rectangle in scene
    coordinates.  acc: one int32 [H][W][C] array per scene of `shapes`, added into in place (None: fresh zeros); returned.
    Every row is axis-aligned: a_yx = a_xy = 0 (scene y follows the window's row index through a_yy, x its column index through
    a_xx) or a_yy = a_xx = 0 (y follows the column index through a_yx, x the row index through a_xy; square patches only).  For
    a scene coordinate y on an axis with origin o, coefficient a and n window pixels along the index it feeds:
        t = y 65536 - o;  a < 0: t, a = -t, -a;   w = floor((256 t + (a >> 1)) / a), the window coordinate in 1/256 pixels;
        w = clamp(w, 0, 256 (n - 1));  i0 = w >> 8;  f = w & 255;  i1 = min(i0 + 1, n - 1)
    and with q = quantise_q16(p[g K + k]) at the four index pairs, fy and fx the weights from the y and the x axis,
        val = ((256 - fy) ((256 - fx) q00 + fx q01) + fy ((256 - fx) q10 + fx q11) + 32768) >> 16
    acc[scene][y, x, c] += the sum of val over the K views, for every (y, x) of the rectangle and every channel.  Integers from the
    first step on: the order of views, groups and passes cannot matter.  An empty rectangle adds nothing; a rectangle must lie in
    its scene and in every view's footprint (the unclamped w of its first and last row and column in [-256, 256 n])."""
    return _accumulate(p, rows7, own, shapes, K, acc, False)


def _accumulate(p, rows7, own, shapes, K, acc, blend: bool):
    """host_accumulate (blend False) and host_accumulate_blend (blend True): the K views' sums of every group, weighted or not, added to acc."""
    p = np.asarray(p)
    if p.ndim != 4 or p.dtype != np.float32:
        raise ValueError(f"p is float32 [G*K][PH][PW][C], got {p.dtype} {p.shape}")
    PH, PW, Cn = (int(v) for v in p.shape[1:])
    t, o = _check_accumulate(_ACCB if blend else _ACC, shapes, rows7, own, K, (PH, PW), Cn, blend)
    K = int(K)
    if len(p) != len(t):
        raise ValueError(f"p is [G*K][PH][PW][C] with one view per table row, got {p.shape} for {len(t)} rows")
    if acc is None:
        acc = [np.zeros((int(h), int(w), Cn), np.int32) for h, w in shapes]
    else:
        acc = list(acc)
        if len(acc) != len(shapes):
            raise ValueError(f"{len(acc)} accumulators for {len(shapes)} scenes")
        for m, (h, w) in zip(acc, shapes):
            if not isinstance(m, np.ndarray) or m.dtype != np.int32 or m.shape != (int(h), int(w), Cn):
                raise ValueError(f"an accumulator is an int32 array [{h}][{w}][{Cn}], got {getattr(m, 'dtype', type(m))} {getattr(m, 'shape', '')}")
    rows = t.tolist()
    for g, (r0, r1, c0, c1) in enumerate(o.tolist()):
        if r0 == r1 or c0 == c1:
            continue
        total = np.zeros((r1 - r0, c1 - c0, Cn), np.int64)
        for k in range(g * K, g * K + K):
            _, y0, x0, ayy, ayx, axy, axx = rows[k]
            q = quantise_q16(p[k])
            if ayx == 0:
                u0, u1, fy = _axis_taps(r0, r1, y0, ayy, PH)
                v0, v1, fx = _axis_taps(c0, c1, x0, axx, PW)
            else:                                                              # y feeds the column index, x the row index
                u0, u1, fy = _axis_taps(r0, r1, y0, ayx, PW)
                v0, v1, fx = _axis_taps(c0, c1, x0, axy, PH)
                q = q.swapaxes(0, 1)
            fy, fx = fy[:, None, None], fx[None, :, None]
            at = lambda u, v: q[u[:, None], v[None, :]]
            top, bot = (256 - fx) * at(u0, v0) + fx * at(u0, v1), (256 - fx) * at(u1, v0) + fx * at(u1, v1)
            total += ((256 - fy) * top + fy * bot + 32768) >> 16
        if blend:
            H, W = int(shapes[rows[g * K][0]][0]), int(shapes[rows[g * K][0]][1])
            wy, wx = _blend_axis(0, r1 - r0, r1 - r0, r0 == 0, r1 == H), _blend_axis(0, c1 - c0, c1 - c0, c0 == 0, c1 == W)
            total = ((wy[:, None] * wx[None, :])[:, :, None] * total + 32768) >> 16
        acc[rows[g * K][0]][r0:r1, c0:c1] += total.astype(np.int32)
    return acc


def host_argmax(acc: Sequence[np.ndarray], class_maps: Optional[Sequence[np.ndarray]] = None, num_classes: Optional[int] = None):
    """The numpy definition of what rua_scene_argmax writes: (uint8 [H][W] map per scene, int64 [C][C] confusion matrix indexed
    [true][pred], None without class maps).  pred is the first index of the maximum of acc[y, x, :]; a label >= C is not counted."""
    acc = [np.asarray(a) for a in acc]
    if len(acc) < 1:
        raise ValueError("rua_scene_argmax: nscenes 0 (>= 1)")
    for s, a in enumerate(acc):
        if a.ndim != 3 or a.dtype != np.int32 or a.shape[2] != acc[0].shape[2] or a.shape[0] < 1 or a.shape[1] < 1:
            raise ValueError(f"scene {s}: an accumulator is an int32 array [H][W][C] with one C for all, got {a.dtype} {a.shape}")
    Cn = int(acc[0].shape[2]) if num_classes is None else int(num_classes)
    if Cn != acc[0].shape[2]:
        raise ValueError(f"the accumulators hold {acc[0].shape[2]} classes, num_classes is {Cn}")
    if not 1 <= Cn <= MAX_CLASSES:
        raise ValueError(f"rua_scene_argmax: C {Cn} outside 1..64")
    if class_maps is not None and len(class_maps) != len(acc):
        raise ValueError(f"{len(class_maps)} class maps for {len(acc)} scenes")
    maps = [np.argmax(a, axis=-1).astype(np.uint8) for a in acc]
    if class_maps is None:
        return maps, None
    cm = np.zeros((Cn, Cn), np.int64)
    for s, (m, c) in enumerate(zip(maps, class_maps)):
        true = np.asarray(c)
        if true.shape != m.shape:
            raise ValueError(f"scene {s}: its class map is {m.shape[0]} x {m.shape[1]}, got {true.shape}")
        true = true.astype(np.int64)
        keep = true < Cn
        cm += np.bincount(true[keep] * Cn + m[keep].astype(np.int64), minlength=Cn * Cn).reshape(Cn, Cn)
    return maps, cm


# ---- blended whole-scene prediction: overlapping footprints added under a linear taper, in integers ----------------------------------
_ACCB = "rua_scene_accumulate_blend"
BLEND_MODES = ("linear",)
BLEND_ONE, BLEND_FLOOR = 256, 16
BLEND_BUDGET = 32768                            # K * footprints per pixel stay below it: a contribution is at most K * 65536, the sum int32


def blend_weight(t: int, F: int, flat_lo: bool, flat_hi: bool) -> int:
    """The weight, out of 256, of position t (0 <= t < F) along one axis of a footprint of F scene pixels: a linear taper
    max(16, (256 (2 min(t, F - 1 - t) + 1)) // F), and 256 on the half that touches the scene's low (flat_lo: 2 t + 1 <= F) or high
    (flat_hi: 2 t + 1 >= F) border, where no other footprint covers the pixel better.  With a stride of F / 2 and even F the tapers of
    neighbouring footprints sum to 256 wherever the floor does not bind; the floor keeps 8 bits of a probability at a footprint's corner."""
    t, F = int(t), int(F)
    if not 0 <= t < F:
        raise ValueError(f"blend_weight: position {t} outside 0..{F - 1}")
    if (flat_lo and 2 * t + 1 <= F) or (flat_hi and 2 * t + 1 >= F):
        return BLEND_ONE
    return max(BLEND_FLOOR, (BLEND_ONE * (2 * min(t, F - 1 - t) + 1)) // F)


def _blend_axis(lo: int, hi: int, F: int, flat_lo: bool, flat_hi: bool) -> np.ndarray:
    """blend_weight of the positions lo..hi-1, int64 [hi - lo]."""
    t = np.arange(lo, hi, dtype=np.int64)
    w = np.maximum(BLEND_FLOOR, (BLEND_ONE * (2 * np.minimum(t, F - 1 - t) + 1)) // F)
    flat = np.zeros(len(t), bool)
    if flat_lo:
        flat |= 2 * t + 1 <= F
    if flat_hi:
        flat |= 2 * t + 1 >= F
    return np.where(flat, BLEND_ONE, w)


def blend_table(shape_hw: Sequence[int], patch, footprint, stride, views=(0,)):
    """One pass of a blended prediction: (rows7 int32 [G*K][7], foot int32 [G][4]).  rows7 is scale_table's; foot takes the place of its
    owned rectangle: the FULL footprint (r, r + FH, c, c + FW) of each group in absolute scene coordinates.  Footprints never leave
    the scene, and they overlap: host_accumulate_blend weights them."""
    rows7, _ = scale_table(shape_hw, patch, footprint, stride, views)
    _, _, fh, fw, rows4, _ = _scale_cover(shape_hw, patch, footprint, stride)
    r, c = rows4[:, 1].astype(np.int64), rows4[:, 2].astype(np.int64)
    return rows7, np.stack([r, r + fh, c, c + fw], 1).astype(np.int32)


def check_accumulate_blend(shapes: Sequence[Sequence[int]], rows7, foot, K, patch, num_classes: int = 1):
    """(rows7 [G*K][7], foot [G][4]) as contiguous int32 arrays; ValueError, in rua_scene_accumulate_blend's own words, for the first
    violation: everything check_accumulate refuses, and non-empty rectangles of two sizes in one call (a call is one pass)."""
    return _check_accumulate(_ACCB, shapes, rows7, foot, K, patch, num_classes, True)


def host_accumulate_blend(p: np.ndarray, rows7, foot, shapes: Sequence[Sequence[int]], K: int, acc: Optional[Sequence[np.ndarray]] = None) -> List[np.ndarray]:
    """The numpy definition of what rua_scene_accumulate_blend adds: host_accumulate's arguments, but foot [G][4] holds each group's
    FULL footprint (r0, r1, c0, c1), and footprints of one call overlap.  For each group and each scene pixel (y, x) of its footprint
    v[c] is the sum over the K views of host_accumulate's bilinear Q16 sample (the same coordinate, taps and (.. + 32768) >> 16 per
    view), and
        acc[scene][y, x, c] += (wy wx v[c] + 32768) >> 16,   wy = blend_weight(y - r0, r1 - r0, r0 == 0, r1 == H), wx likewise for columns.
    The weight lives in scene space: the K views of a group share it, flips and transpositions do not touch it.  A contribution is
    at most K 65536 (check_blend_budget keeps the int32 sums in range); integer sums are the same in any order of groups and calls."""
    return _accumulate(p, rows7, foot, shapes, K, acc, True)


def _axis_depth(L: int, F: int, S: int) -> int:
    """The greatest number of footprints of _axis_cover(L, F, S) that cover one pixel of the axis."""
    o, _ = _axis_cover(L, F, S)
    d = np.zeros(L + 1, np.int64)
    np.add.at(d, o, 1)
    np.add.at(d, o + F, -1)
    return int(np.cumsum(d).max())


def check_blend_budget(shape_hw: Sequence[int], patch, footprints, stride, K) -> int:
    """K * the sum over the passes (one per footprint of `footprints`, covered as blend_table covers) of cover_y * cover_x, the greatest
    number of footprints per axis over one pixel; ValueError unless it is below 32768: the accumulator is int32 and a contribution
    reaches K * 65536."""
    H, W = int(shape_hw[0]), int(shape_hw[1])
    total = 0
    for fp in footprints:
        _, _, fh, fw, sf = _scaled_stride(patch, fp, stride, "check_blend_budget")
        if fh > H or fw > W:
            raise ValueError(f"check_blend_budget: footprint {fh} x {fw} is larger than the {H} x {W} scene")
        total += _axis_depth(H, fh, sf[0]) * _axis_depth(W, fw, sf[1])
    if not int(K) * total < BLEND_BUDGET:
        raise ValueError(f"check_blend_budget: K {int(K)} views times {total} footprints over one pixel (cover_y * cover_x, summed over the passes) "
                         f"is {int(K) * total}: the int32 accumulator takes fewer than {BLEND_BUDGET}; use a larger stride")
    return int(K) * total


# ---- class counts of windows: what class weights and a balance filter are functions of ------------------------------------------
def _check_classes(num_classes) -> int:
    if isinstance(num_classes, bool) or not isinstance(num_classes, (int, np.integer)) or not 1 <= int(num_classes) <= MAX_CLASSES:
        raise ValueError(f"rua_scene_class_counts: C {num_classes} outside 1..64")
    return int(num_classes)


def host_class_counts(class_maps: Sequence[np.ndarray], table: np.ndarray, patch, num_classes: int) -> np.ndarray:
    """The numpy definition of what rua_scene_class_counts writes, as int64 [N][C + 1]: for row n = (scene, row, col, code) and the
    window cm[row:row+PH, col:col+PW], counts[n][c] is the number of pixels equal to c for c < C and counts[n][C] the number with a
    value >= C.  Every row sums to PH * PW.  The code is checked as check_table checks it and does not change the counts: a
    symmetry permutes pixels."""
    ph, pw = _patch2(patch)
    C_ = _check_classes(num_classes)
    t = check_table([cm.shape for cm in class_maps], table, patch)
    out = np.empty((len(t), C_ + 1), np.int64)
    for k, (s, r, c, _) in enumerate(t.tolist()):
        w = np.minimum(np.asarray(class_maps[s])[r:r + ph, c:c + pw], C_)
        out[k] = np.bincount(w.ravel(), minlength=C_ + 1)
    return out


def class_weights(counts: np.ndarray) -> np.ndarray:
    """float64 [C] weighted-CE class weights of int [N][C + 1] window counts, the reference's rule: with n_c the column sums over
    c < C (the >= C column is ignored), w_c = sum(n) / n_c.  A class with n_c = 0 gets the largest weight among the classes that
    are present - it is rare, not free.  ValueError if no pixel carries a class."""
    a = np.asarray(counts)
    if a.ndim != 2 or a.shape[1] < 2 or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"class counts are an integer [N][C + 1] array, got {a.dtype} {a.shape}")
    n = a[:, :-1].astype(np.int64).sum(0)
    total = int(n.sum())
    if total == 0:
        raise ValueError("class_weights: no pixel of the counted windows carries a class below C: there is nothing to weigh")
    w = np.zeros(len(n), np.float64)
    w[n > 0] = float(total) / n[n > 0]
    w[n == 0] = w.max()
    return w


def balance_rows(counts: np.ndarray, cls: int, percent: float, patch) -> np.ndarray:
    """bool [N]: counts[:, cls] >= int(PH * PW * percent / 100) - the test of the reference's bal_aug_patches (utils.py:383), which
    keeps a patch when class 1 covers at least `percent` of it, with the class a parameter."""
    ph, pw = _patch2(patch)
    a = np.asarray(counts)
    if a.ndim != 2 or a.shape[1] < 2 or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"class counts are an integer [N][C + 1] array, got {a.dtype} {a.shape}")
    if isinstance(cls, bool) or not isinstance(cls, (int, np.integer)) or not 0 <= int(cls) < a.shape[1] - 1:
        raise ValueError(f"balance_rows: class {cls} outside 0..{a.shape[1] - 2}")
    if not 0 <= percent <= 100:
        raise ValueError(f"balance_rows: percent {percent} outside 0..100")
    return a[:, int(cls)] >= int(ph * pw * percent / 100)


# ---- the eroded ground truth: pixels near a class boundary become "no class" ------------------------------------------------------
MAX_RADIUS = 16


def check_radius(radius) -> int:
    """The erosion radius as an int; ValueError, in rua_scene_erode's own words, unless it is an integer in 0..16."""
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)):
        raise ValueError(f"rua_scene_erode: radius {radius!r} is no integer")
    if not 0 <= int(radius) <= MAX_RADIUS:
        raise ValueError(f"rua_scene_erode: radius {int(radius)} outside 0..16")
    return int(radius)


def _check_map(a, what: str) -> np.ndarray:
    a = np.asarray(a)
    if a.dtype != np.uint8 or a.ndim != 2 or a.size == 0:
        raise ValueError(f"{what} is a non-empty uint8 H x W array, got {a.dtype} {a.shape}")
    return a


def host_erode(class_map: np.ndarray, radius: int) -> np.ndarray:
    """The numpy definition of what rua_scene_erode writes, uint8 [H][W]: out[i, j] = 255 if some offset (dy, dx) with
    dy^2 + dx^2 <= radius^2 has (i + dy, j + dx) inside the map and class_map[i + dy, j + dx] != class_map[i, j], otherwise
    class_map[i, j].  Bytes are compared raw (a value >= C beside a class pixel erodes it and stays what it is - no class - itself),
    pixels outside the map do not exist (the border is no boundary), radius 0 is the identity, and no class count is involved: 255
    is "no class" for every C <= 64."""
    cm = _check_map(class_map, "a class map")
    r = check_radius(radius)
    H, W = cm.shape
    eroded = np.zeros((H, W), bool)
    for dy in range(-min(r, H - 1), min(r, H - 1) + 1):
        lim = min(int(np.sqrt(r * r - dy * dy) + 1e-9), W - 1)               # isqrt: the argument is an integer below 2^9
        for dx in range(-lim, lim + 1):
            if dy == 0 and dx == 0:
                continue
            i0, i1, j0, j1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)    # the pixels whose neighbour exists
            eroded[i0:i1, j0:j1] |= cm[i0 + dy:i1 + dy, j0 + dx:j1 + dx] != cm[i0:i1, j0:j1]
    out = cm.copy()
    out[eroded] = 255
    return out


def host_erode_confusion(class_map: np.ndarray, pred: np.ndarray, radius: int, num_classes: int) -> np.ndarray:
    """int64 [C][C] indexed [true][pred]: the (t, pred) pairs over the pixels with t = host_erode(class_map, radius)[i, j] < C and
    pred[i, j] < C - what rua_scene_erode adds to its confusion matrix."""
    if isinstance(num_classes, bool) or not isinstance(num_classes, (int, np.integer)) or not 1 <= int(num_classes) <= MAX_CLASSES:
        raise ValueError(f"rua_scene_erode: C {num_classes} outside 1..64")
    C_ = int(num_classes)
    t = host_erode(class_map, radius).astype(np.int64)
    p = _check_map(pred, "a prediction map")
    if p.shape != t.shape:
        raise ValueError(f"the prediction map is {p.shape}, the class map {t.shape}")
    keep = (t < C_) & (p < C_)
    return np.bincount(t[keep] * C_ + p[keep].astype(np.int64), minlength=C_ * C_).reshape(C_, C_)


# ---- boundary F1: are the predicted class edges where the true ones are ------------------------------------------------------------
def check_tolerance(radius) -> Optional[int]:
    """The boundary tolerance as an int, or None for None ("off": 0 is a real tolerance, exact coincidence); ValueError, in
    rua_scene_boundary's own words, unless it is an integer in 0..16."""
    if radius is None:
        return None
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)):
        raise ValueError(f"rua_scene_boundary: radius {radius!r} is no integer")
    if not 0 <= int(radius) <= MAX_RADIUS:
        raise ValueError(f"rua_scene_boundary: radius {int(radius)} outside 0..16")
    return int(radius)


def _check_boundary_classes(num_classes) -> int:
    if isinstance(num_classes, bool) or not isinstance(num_classes, (int, np.integer)) or not 1 <= int(num_classes) <= MAX_CLASSES:
        raise ValueError(f"rua_scene_boundary: C {num_classes} outside 1..64")
    return int(num_classes)


def _check_boundary_map(a, what: str) -> np.ndarray:
    a = np.asarray(a)
    if a.dtype != np.uint8 or a.ndim != 2 or a.size == 0:
        raise ValueError(f"rua_scene_boundary: {what} is a non-empty uint8 H x W array, got {a.dtype} {a.shape}")
    return a


def host_boundaries(m: np.ndarray, num_classes: int) -> np.ndarray:
    """The numpy definition of the boundary image rua_scene_boundary writes, uint8 [H][W]: out[i, j] = m[i, j] if m[i, j] < C and
    one of the 4-neighbours of (i, j) that lie inside the map holds another byte, otherwise 255.  Bytes are compared raw: a value
    >= C is never a boundary pixel itself and makes its class neighbours boundary pixels; pixels outside the map do not exist (the
    scene border is no boundary, as in host_erode).  B_c(m), the pixels where the result equals c, is the inner boundary of class c
    with 4-connectivity."""
    m = _check_boundary_map(m, "a map")
    C_ = _check_boundary_classes(num_classes)
    edge = np.zeros(m.shape, bool)
    v, h = m[1:] != m[:-1], m[:, 1:] != m[:, :-1]
    edge[1:] |= v
    edge[:-1] |= v
    edge[:, 1:] |= h
    edge[:, :-1] |= h
    return np.where(edge & (m < C_), m, np.uint8(255)).astype(np.uint8)


def host_boundary_counts(class_map: np.ndarray, pred: np.ndarray, radius: int, num_classes: int) -> np.ndarray:
    """The numpy definition of what rua_scene_boundary adds to its counts, int64 [C][4]: row c is (n_pred, m_pred, n_true, m_true)
    with n_pred = |B_c(pred)| (host_boundaries), m_pred the number of x in B_c(pred) for which some y in B_c(class_map) has
    (x - y) . (x - y) <= radius^2, and n_true, m_true the same with the two maps exchanged.  radius is an integer 0..16, 0 exact
    coincidence.  100 m_pred / n_pred is the boundary precision of class c, 100 m_true / n_true its recall (boundary_scores)."""
    t = _check_boundary_map(class_map, "the class map")
    p = _check_boundary_map(pred, "the prediction map")
    r = check_tolerance(radius)
    if r is None:
        raise ValueError("rua_scene_boundary: radius None is no integer")
    C_ = _check_boundary_classes(num_classes)
    if p.shape != t.shape:
        raise ValueError(f"rua_scene_boundary: the prediction map is {p.shape}, the class map {t.shape}")
    H, W = t.shape
    bt, bp = host_boundaries(t, C_), host_boundaries(p, C_)
    hit_t, hit_p = np.zeros((H, W), bool), np.zeros((H, W), bool)
    for dy in range(-min(r, H - 1), min(r, H - 1) + 1):
        lim = min(int(np.sqrt(r * r - dy * dy) + 1e-9), W - 1)               # isqrt: the argument is an integer below 2^9
        for dx in range(-lim, lim + 1):
            i0, i1, j0, j1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)    # the pixels whose partner exists
            hit_p[i0:i1, j0:j1] |= bp[i0:i1, j0:j1] == bt[i0 + dy:i1 + dy, j0 + dx:j1 + dx]
            hit_t[i0:i1, j0:j1] |= bt[i0:i1, j0:j1] == bp[i0 + dy:i1 + dy, j0 + dx:j1 + dx]
    out = np.empty((C_, 4), np.int64)
    for col, (b, hit) in enumerate(((bp, hit_p), (bt, hit_t))):                 # 255 == 255 "hits" too: only class bytes are counted
        out[:, 2 * col] = np.bincount(b[b < C_], minlength=C_)
        out[:, 2 * col + 1] = np.bincount(b[(b < C_) & hit], minlength=C_)
    return out


def boundary_scores(counts) -> dict:
    """Boundary precision, recall and F1 in percent (as eval_scenes_ISPRS.metrics_from_confusion gives its scores) from int [C][4]
    counts of (n_pred, m_pred, n_true, m_true) rows; [n][C][4] counts of several scenes are SUMMED first.  The published BF score
    averages per image instead; Engine.predict_scene and ScenePool.boundary_counts return the per-scene counts, so a user can do
    that by scoring each and averaging.  {"precision": float64 [C] = 100 m_pred / n_pred, nan where n_pred == 0; "recall":
    100 m_true / n_true, nan where n_true == 0; "f1": 2 P R / (P + R) - nan where both n are 0 (the class has no boundary in either
    map), 0 where exactly one n is 0 and 0 where P + R == 0; "f1_mean": the mean of the f1 that are not nan, nan if there is none}."""
    a = np.asarray(counts)
    if a.ndim == 3 and a.shape[0] >= 1:
        a = a.astype(np.int64).sum(0) if np.issubdtype(a.dtype, np.integer) else a
    if a.ndim != 2 or a.shape[1] != 4 or a.shape[0] < 1 or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"boundary counts are an integer [C][4] (or [n][C][4]) array of (n_pred, m_pred, n_true, m_true) rows, got {a.dtype} {a.shape}")
    a = a.astype(np.int64)
    if (a < 0).any() or (a[:, 1] > a[:, 0]).any() or (a[:, 3] > a[:, 2]).any():
        raise ValueError("boundary counts: 0 <= m_pred <= n_pred and 0 <= m_true <= n_true in every row")
    n_p, m_p, n_t, m_t = (a[:, k].astype(np.float64) for k in range(4))
    nan = np.full(len(a), np.nan)
    prec = np.divide(100 * m_p, n_p, out=nan.copy(), where=n_p > 0)
    rec = np.divide(100 * m_t, n_t, out=nan.copy(), where=n_t > 0)
    f1 = np.zeros(len(a), np.float64)
    both = (n_p > 0) & (n_t > 0) & (np.nan_to_num(prec) + np.nan_to_num(rec) > 0)
    f1[both] = 2 * prec[both] * rec[both] / (prec[both] + rec[both])
    f1[(n_p == 0) & (n_t == 0)] = np.nan
    have = ~np.isnan(f1)
    return {"precision": prec, "recall": rec, "f1": f1, "f1_mean": float(f1[have].mean()) if have.any() else float("nan")}


# ---- connected regions and the sieve: a minimum mapping unit for class maps -------------------------------------------------------
SIEVE_MODES = ("void", "fill")                 # the C ABI's mode 0 and 1
MAX_ROUNDS = 4


def _is_int(v) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, np.integer))


def _check_connectivity(fn: str, connectivity) -> int:
    if not _is_int(connectivity) or int(connectivity) not in (4, 8):
        raise ValueError(f"{fn}: connectivity {connectivity!r} is neither 4 nor 8")
    return int(connectivity)


def _check_region_map(fn: str, a, what: str = "a map") -> np.ndarray:
    a = np.asarray(a)
    if a.dtype != np.uint8 or a.ndim != 2 or a.size == 0:
        raise ValueError(f"{fn}: {what} is a non-empty uint8 H x W array, got {a.dtype} {a.shape}")
    if a.size >= 1 << 31:
        raise ValueError(f"{fn}: {what}: size {a.shape[0]} x {a.shape[1]} (H * W < 2^31: a label is an int32 pixel index)")
    return a


def check_sieve(min_area, num_classes, mode="fill", connectivity=4, classes=None, rounds=1, fn: str = "rua_scene_sieve"):
    """The parameters of a sieve as (min_area, C, mode number, connectivity, class mask, rounds) - mode 0 is "void", 1 "fill", bit c
    of the mask is set if class c is sieved (classes None: every class below C); ValueError, in rua_scene_sieve's own words, unless
    1 <= min_area < 2^31, 1 <= C <= 64, the mode is one of SIEVE_MODES, the connectivity 4 or 8, every class an integer in 0..C-1
    and rounds in 1..4."""
    if not _is_int(min_area) or not 1 <= int(min_area) < 1 << 31:
        raise ValueError(f"{fn}: min_area {min_area!r} outside 1..2147483647")
    if not _is_int(num_classes) or not 1 <= int(num_classes) <= MAX_CLASSES:
        raise ValueError(f"{fn}: C {num_classes} outside 1..64")
    C_ = int(num_classes)
    if not isinstance(mode, str) or mode not in SIEVE_MODES:
        raise ValueError(f"{fn}: mode {mode!r} is neither void (0) nor fill (1)")
    conn = _check_connectivity(fn, connectivity)
    if classes is None:
        mask = (1 << C_) - 1
    else:
        if isinstance(classes, (str, bytes)) or _is_int(classes):
            classes = (classes,)
        mask = 0
        for c in classes:
            if not _is_int(c) or not 0 <= int(c) < C_:
                raise ValueError(f"{fn}: class_mask names class {c!r}, outside 0..{C_ - 1}")
            mask |= 1 << int(c)
    if not _is_int(rounds) or not 1 <= int(rounds) <= MAX_ROUNDS:
        raise ValueError(f"{fn}: rounds {rounds!r} outside 1..{MAX_ROUNDS}")
    return int(min_area), C_, SIEVE_MODES.index(mode), conn, mask, int(rounds)


def sieve_params(sieve, num_classes):
    """Engine.predict_scene's `sieve` as check_sieve's tuple: an integer is min_area with mode "fill", connectivity 4, every class
    and one round; a dict may hold min_area (required), mode, connectivity, classes and rounds.  ValueError for anything else."""
    if _is_int(sieve):
        return check_sieve(sieve, num_classes)
    if not isinstance(sieve, dict):
        raise ValueError(f"sieve {sieve!r}: None, a minimum area in pixels or a dict of min_area, mode, connectivity, classes, rounds")
    unknown = sorted(set(sieve) - {"min_area", "mode", "connectivity", "classes", "rounds"})
    if unknown:
        raise ValueError(f"sieve: unknown key {unknown[0]!r} (min_area, mode, connectivity, classes, rounds)")
    if "min_area" not in sieve:
        raise ValueError("sieve: the dict needs min_area")
    return check_sieve(sieve["min_area"], num_classes, sieve.get("mode", "fill"), sieve.get("connectivity", 4), sieve.get("classes"),
                       sieve.get("rounds", 1))


def host_regions(class_map: np.ndarray, connectivity: int = 4):
    """The numpy definition of what rua_scene_regions writes: (labels int32 [H][W], areas int32 [H][W]).  A region is a maximal set
    of pixels of equal byte value connected through 4-neighbours (connectivity 4) or 8-neighbours (8); bytes are compared raw, so
    "no class" bytes form regions like any other, and pixels outside the map do not exist.  labels[i, j] is the smallest row-major
    index i' * W + j' of the pixel's region - its root, canonical, so label maps compare bit for bit -, areas holds the region's
    pixel count at the root and 0 everywhere else.  H * W < 2^31.
    Rows are cut into runs of equal bytes; a union-find over the runs (the larger root always points to the smaller) joins the
    runs of neighbouring rows that touch, and a run's root is the first pixel of the first run of its set."""
    m = _check_region_map("rua_scene_regions", class_map)
    conn = _check_connectivity("rua_scene_regions", connectivity)
    H, W = m.shape
    start = np.ones((H, W), bool)
    start[:, 1:] = m[:, 1:] != m[:, :-1]
    run = (np.cumsum(start.ravel()) - 1).reshape(H, W)                   # the run of every pixel, numbered in row-major order
    first = np.flatnonzero(start.ravel())                                 # ... and the first pixel of every run: ascending
    pairs = [np.stack([run[1:][m[1:] == m[:-1]], run[:-1][m[1:] == m[:-1]]], 1)]
    if conn == 8:
        d = m[1:, 1:] == m[:-1, :-1]
        pairs.append(np.stack([run[1:, 1:][d], run[:-1, :-1][d]], 1))
        d = m[1:, :-1] == m[:-1, 1:]
        pairs.append(np.stack([run[1:, :-1][d], run[:-1, 1:][d]], 1))
    parent = list(range(len(first)))

    def find(a: int) -> int:
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for a, b in np.unique(np.concatenate(pairs), axis=0).tolist():
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    root = np.fromiter((find(a) for a in range(len(first))), np.int64, len(first))
    labels = first[root][run]
    areas = np.bincount(labels.ravel(), minlength=H * W).reshape(H, W)
    return labels.astype(np.int32), areas.astype(np.int32)


def host_region_counts(class_map: np.ndarray, min_area: int, num_classes: int, connectivity: int = 4) -> np.ndarray:
    """The numpy definition of what rua_scene_regions adds to its counts, int64 [C][3]: per class c < C the regions of byte c
    (host_regions), how many of them have fewer than min_area pixels, and how many pixels those small regions hold."""
    mn, C_, _, conn, _, _ = check_sieve(min_area, num_classes, connectivity=connectivity, fn="rua_scene_regions")
    m = _check_region_map("rua_scene_regions", class_map)
    _, areas = host_regions(m, conn)
    at = areas > 0
    byte, area = m[at].astype(np.int64), areas[at].astype(np.int64)
    keep = byte < C_
    byte, area = byte[keep], area[keep]
    small = area < mn
    out = np.zeros((C_, 3), np.int64)
    out[:, 0] = np.bincount(byte, minlength=C_)
    out[:, 1] = np.bincount(byte[small], minlength=C_)
    out[:, 2] = np.bincount(byte[small], weights=area[small], minlength=C_).astype(np.int64)
    return out


def _sieve_round(m: np.ndarray, mn: int, C_: int, mode: int, conn: int, mask: int) -> np.ndarray:
    H, W = m.shape
    labels, areas = host_regions(m, conn)
    sieved = np.array([(mask >> c) & 1 for c in range(256)], bool)       # bits >= C are never set
    small = sieved[m] & (areas.ravel()[labels] < mn)
    out = m.copy()
    if mode == 0:
        out[small] = 255
        return out
    kept = (m < C_) & ~small
    roots, slot = np.unique(labels[small], return_inverse=True)          # the small regions, and the region of every small pixel
    if not len(roots):
        return out
    votes = np.zeros((len(roots), C_), np.int64)
    slot_of = np.full((H, W), -1, np.int64)
    slot_of[small] = np.asarray(slot).reshape(-1)
    for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)):                    # x at [i0:i1, j0:j1], its neighbour y at the same plus (dy, dx)
        i0, i1, j0, j1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
        pair = small[i0:i1, j0:j1] & kept[i0 + dy:i1 + dy, j0 + dx:j1 + dx]
        np.add.at(votes, (slot_of[i0:i1, j0:j1][pair], m[i0 + dy:i1 + dy, j0 + dx:j1 + dx][pair].astype(np.int64)), 1)
    winner = votes.argmax(1).astype(np.uint8)                            # the first maximum: a tie goes to the lowest class
    voted = votes.sum(1) > 0
    s = slot_of[small]
    out[small] = np.where(voted[s], winner[s], m[small])
    return out


def host_sieve(class_map: np.ndarray, min_area: int, num_classes: int, mode: str, connectivity: int = 4, classes=None,
               rounds: int = 1) -> np.ndarray:
    """The numpy definition of what `rounds` rounds of rua_scene_regions and rua_scene_sieve leave, uint8 [H][W].  A region
    (host_regions) is SMALL if its byte c is < C, c is in `classes` (None: every class) and it has fewer than min_area pixels -
    min_area 1 is the identity, and a region of exactly min_area pixels stays, as under skimage's area_opening.  Every other
    region with a byte < C is KEPT, those of a class outside `classes` too; regions of bytes >= C are never changed and never
    donate.  mode "void": the pixels of small regions become 255, so they drop out of every score through the p < C rule of the
    confusion and boundary counts (the reference's protocol; restricted to class 1 of a binary map it is area_opening followed by
    the exclusion).  mode "fill": every small region R takes one class for all its pixels - one vote is cast for the byte of y per
    ordered pair (x in R, y a 4-neighbour of x inside the map and in a kept region), also under connectivity 8; the class with the
    most votes wins, a tie goes to the lowest class, and a region with no vote stays as it is.  All small regions decide at once,
    from the input map.  rounds (1..4) applies the whole operation again to its own output: a second round removes speckle nested
    inside speckle, which after round 1 lies inside a kept region; further rounds on a stable map change nothing."""
    mn, C_, md, conn, mask, n = check_sieve(min_area, num_classes, mode, connectivity, classes, rounds)
    out = _check_region_map("rua_scene_sieve", class_map)
    for _ in range(n):
        out = _sieve_round(out, mn, C_, md, conn, mask)
    return out


def sweep_levels(thresholds=None) -> np.ndarray:
    """The levels of a precision-recall sweep as rua_scene_area_open takes them: a uint8 array of distinct levels in 1..255, strictly
    descending.  Level t means "byte >= t", the byte being what rua_scene_stitch_maps mode 0 wrote: the rounded 255 p.  None gives
    all 255 levels; a float threshold thr in (0, 1] gives the level max(1, rint(255 thr)); an integer is taken as a level;
    duplicates are dropped.  ValueError, in rua_scene_area_open's own words, for an empty list, a level 0 or a level above 255."""
    fn = "rua_scene_area_open"
    if thresholds is None:
        return np.arange(255, 0, -1).astype(np.uint8)
    if isinstance(thresholds, (str, bytes)):
        raise ValueError(f"{fn}: thresholds {thresholds!r}: None or a list of levels 1..255 or of thresholds in (0, 1]")
    if np.ndim(thresholds) == 0:
        thresholds = (thresholds,)
    out = []
    for k, thr in enumerate(np.asarray(thresholds).ravel().tolist() if isinstance(thresholds, np.ndarray) else list(thresholds)):
        if _is_int(thr):
            v = int(thr)
        elif isinstance(thr, (float, np.floating)) and not isinstance(thr, bool):
            if not 0.0 < float(thr) <= 1.0:
                raise ValueError(f"{fn}: thresholds[{k}] = {thr!r} outside (0, 1] (an integer is taken as a level 1..255)")
            v = max(1, int(np.rint(255.0 * float(thr))))
        else:
            raise ValueError(f"{fn}: thresholds[{k}] = {thr!r} is neither an integer level nor a float threshold")
        if not 1 <= v <= 255:
            raise ValueError(f"{fn}: levels[{k}] = {v} outside 1..255")
        out.append(v)
    if not out:
        raise ValueError(f"{fn}: T 0 outside 1..255")
    return np.array(sorted(set(out), reverse=True), np.uint8)


def _check_min_area(fn: str, min_area) -> int:
    if not _is_int(min_area) or not 1 <= int(min_area) < 1 << 31:
        raise ValueError(f"{fn}: min_area {min_area!r} outside 1..2147483647")
    return int(min_area)


def host_area_open(prob: np.ndarray, levels, min_area: int, connectivity: int = 4) -> np.ndarray:
    """The numpy definition of what rua_scene_area_open writes, the OPENED map G, uint8 [H][W], of the uint8 probability map prob:
    G[x] is the largest listed level t (sweep_levels) such that x lies in a connected component of {prob >= t} - 4- or 8-connected -
    with at least min_area pixels, and 0 if there is none.  {G >= t} is then, for every listed t, exactly the binary map the
    reference's protocol scores at that threshold: {prob >= t} after skimage's area_opening(area_threshold=min_area) (a component of
    exactly min_area pixels stays).  One map serves every threshold because thresholding commutes with the opening and the kept sets
    are nested: a component of at least min_area pixels at level t lies inside one at every lower level.
    Written from scratch per level: host_regions of the binarised map, nothing carried from one level to the next.  min_area 1:
    G[x] is the largest listed level <= prob[x]."""
    fn = "rua_scene_area_open"
    p = _check_region_map(fn, prob, "the probability map")
    lv = sweep_levels(levels)
    mn = _check_min_area(fn, min_area)
    conn = _check_connectivity(fn, connectivity)
    out = np.zeros(p.shape, np.uint8)
    for t in lv.tolist():
        binary = (p >= t).astype(np.uint8)
        labels, areas = host_regions(binary, conn)
        kept = (binary == 1) & (areas.ravel()[labels] >= mn)
        out[kept & (out == 0)] = t
    return out


def host_sweep_hist(prob: np.ndarray, opened: Optional[np.ndarray], cls: np.ndarray, positive: int, num_classes: int) -> np.ndarray:
    """The numpy definition of what rua_scene_sweep_hist adds to its histogram, int64 [2][2][256]: hist[0][k][l] counts the pixels
    with prob == l, hist[1][k][l] those with opened == l (opened None stands for prob: no area opening); k = 1 where cls ==
    positive, k = 0 where cls < num_classes and cls != positive.  Pixels with cls >= num_classes - the project's "no class", which is
    how a user encodes the reference's "past deforestation / buffer = 2" and the outside of its mask - are counted nowhere."""
    fn = "rua_scene_sweep_hist"
    p = _check_region_map(fn, prob, "the probability map")
    o = p if opened is None else _check_region_map(fn, opened, "the opened map")
    c = _check_region_map(fn, cls, "the class map")
    if o.shape != p.shape or c.shape != p.shape:
        raise ValueError(f"{fn}: the probability map is {p.shape}, the opened map {o.shape}, the class map {c.shape}")
    if not _is_int(num_classes) or not 1 <= int(num_classes) <= MAX_CLASSES:
        raise ValueError(f"{fn}: C {num_classes} outside 1..64")
    if not _is_int(positive) or not 0 <= int(positive) < int(num_classes):
        raise ValueError(f"{fn}: positive {positive!r} outside 0..{int(num_classes) - 1}")
    out = np.zeros((2, 2, 256), np.int64)
    for k, sel in enumerate(((c < int(num_classes)) & (c != int(positive)), c == int(positive))):
        out[0, k] = np.bincount(p[sel], minlength=256)
        out[1, k] = np.bincount(o[sel], minlength=256)
    return out


def sweep_scores(hist, levels=None) -> dict:
    """The precision-recall curve of a histogram of host_sweep_hist / rua_scene_sweep_hist (int64 [2][2][256], or a sum of such over
    scenes) at these levels (sweep_levels; they must be levels the opened map was built with, or any levels if it was not opened).
    A dict of arrays over the descending levels, with S_t(a) = sum of a[l] over l >= t:
      tp = S_t(hist[1][1])    fp = S_t(hist[1][0])    fn = sum of hist[0][1][l] over l < t
      removed = S_t(hist[0][0] + hist[0][1]) - S_t(hist[1][0] + hist[1][1]): predicted pixels that sit in a region below min_area;
                they are left out of tp, fp and fn, as the reference leaves them out
      recall = tp / (tp + fn)    precision = tp / (tp + fp)    f1 = 2 tp / (2 tp + fp + fn)    alarm_area = (tp + fp) / valid
    each 0 where it would be 0 / 0; "levels" the levels, "valid" (an int) the total of hist[0], and "average_precision" (a float)
    the sum over k of (recall_k - recall_{k-1}) precision_k along the descending levels with recall_{-1} = 0.
    Recall is non-decreasing along the descending levels because the kept sets are nested: tp only grows as t falls and fn only
    shrinks, with or without an opening.  One deliberate difference from the reference's
    matrics_AA_recall: the denominator of its alarm area also counts its "not considered" pixels, ours counts only valid ones."""
    h = np.asarray(hist)
    if h.shape != (2, 2, 256) or h.dtype.kind not in "iu":
        raise ValueError(f"sweep_scores: hist is an integer [2][2][256] array, got {h.dtype} {h.shape}")
    h = h.astype(np.int64)
    lv = sweep_levels(levels)
    at = lv.astype(np.int64)
    suffix = lambda a: np.cumsum(a[::-1])[::-1][at]
    tp, fp = suffix(h[1, 1]), suffix(h[1, 0])
    fn_ = int(h[0, 1].sum()) - suffix(h[0, 1])
    removed = suffix(h[0, 0] + h[0, 1]) - suffix(h[1, 0] + h[1, 1])
    valid = int(h[0].sum())

    def ratio(a, b):
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        return np.divide(a, b, out=np.zeros_like(a), where=b != 0)

    recall, precision = ratio(tp, tp + fn_), ratio(tp, tp + fp)
    ap = float(np.sum(np.diff(np.concatenate([[0.0], recall])) * precision))
    return {"levels": lv, "tp": tp, "fp": fp, "fn": fn_, "removed": removed, "valid": valid, "recall": recall, "precision": precision,
            "f1": ratio(2 * tp, 2 * tp + fp + fn_), "alarm_area": ratio(tp + fp, np.full(len(lv), valid)), "average_precision": ap}


def sweep_params(sweep, num_classes):
    """Engine.predict_scene's `sweep` as (positive, levels, min_area, connectivity, opened): an integer is the positive class with
    all 255 levels, min_area 1, connectivity 4 and no opened map returned; a dict may hold positive (required), thresholds,
    min_area, connectivity and opened.  ValueError, in the C entries' words, for anything else."""
    fn = "rua_scene_sweep_hist"
    if _is_int(sweep):
        sweep = {"positive": sweep}
    if not isinstance(sweep, dict):
        raise ValueError(f"sweep {sweep!r}: None, a class index or a dict of positive, thresholds, min_area, connectivity, opened")
    unknown = sorted(set(sweep) - {"positive", "thresholds", "min_area", "connectivity", "opened"})
    if unknown:
        raise ValueError(f"sweep: unknown key {unknown[0]!r} (positive, thresholds, min_area, connectivity, opened)")
    if "positive" not in sweep:
        raise ValueError("sweep: the dict needs positive")
    if not _is_int(num_classes) or not 1 <= int(num_classes) <= MAX_CLASSES:
        raise ValueError(f"{fn}: C {num_classes} outside 1..64")
    pos = sweep["positive"]
    if not _is_int(pos) or not 0 <= int(pos) < int(num_classes):
        raise ValueError(f"{fn}: positive {pos!r} outside 0..{int(num_classes) - 1}")
    return (int(pos), sweep_levels(sweep.get("thresholds")), _check_min_area("rua_scene_area_open", sweep.get("min_area", 1)),
            _check_connectivity("rua_scene_area_open", sweep.get("connectivity", 4)), bool(sweep.get("opened", False)))


# ---- instances: seeds from the class, boundary and distance maps, grown, and matched against the true objects ---------------------
MAX_INSTANCES = 1 << 20
IOU_PERCENT = tuple(range(50, 100, 5))
TABLE_COLUMNS = ("root", "class", "area", "seed_area", "i_min", "j_min", "i_max", "j_max")
_SEED, _INST, _MATCH = "rua_scene_seed_map", "rua_scene_instances", "rua_scene_instance_match"


def _class_mask(fn: str, classes, C_: int) -> int:
    if isinstance(classes, (str, bytes)):
        raise ValueError(f"{fn}: classes {classes!r}: a class index or a list of them")
    if _is_int(classes):
        classes = (classes,)
    mask = 0
    for c in classes:
        if not _is_int(c) or not 0 <= int(c) < C_:
            raise ValueError(f"{fn}: class_mask names class {c!r}, outside 0..{C_ - 1}")
        mask |= 1 << int(c)
    return mask


def _check_num_classes(fn: str, num_classes) -> int:
    if not _is_int(num_classes) or not 1 <= int(num_classes) <= MAX_CLASSES:
        raise ValueError(f"{fn}: C {num_classes} outside 1..64")
    return int(num_classes)


def _check_head_map(fn: str, a, what: str, shape, C_: int):
    if a is None:
        return None
    a = np.asarray(a)
    if a.dtype != np.uint8 or a.shape != tuple(shape) + (C_,):
        raise ValueError(f"{fn}: {what} is a uint8 [{shape[0]}][{shape[1]}][{C_}] map, got {a.dtype} {a.shape}")
    return a


def check_seed_map(num_classes, classes, bound_below=128, dist_at_least=0, fn: str = _SEED):
    """(C, class mask, bound_below, dist_at_least) of a seed map; ValueError, in rua_scene_seed_map's own words, unless
    1 <= C <= 64, every class is an integer in 0..C-1, bound_below an integer in 1..256 and dist_at_least one in 0..255."""
    C_ = _check_num_classes(fn, num_classes)
    mask = _class_mask(fn, classes, C_)
    if not _is_int(bound_below) or not 1 <= int(bound_below) <= 256:
        raise ValueError(f"{fn}: bound_below {bound_below!r} outside 1..256")
    if not _is_int(dist_at_least) or not 0 <= int(dist_at_least) <= 255:
        raise ValueError(f"{fn}: dist_at_least {dist_at_least!r} outside 0..255")
    return C_, mask, int(bound_below), int(dist_at_least)


def check_instances(num_classes, classes, min_seed=1, radius=4, connectivity=4, max_instances=MAX_INSTANCES, fn: str = _INST):
    """(C, class mask, min_seed, radius, connectivity, max_instances) of rua_scene_instances; ValueError in its own words."""
    C_ = _check_num_classes(fn, num_classes)
    mask = _class_mask(fn, classes, C_)
    if not _is_int(min_seed) or not 1 <= int(min_seed) < 1 << 31:
        raise ValueError(f"{fn}: min_seed {min_seed!r} outside 1..2147483647")
    if not _is_int(radius) or not 0 <= int(radius) <= MAX_RADIUS:
        raise ValueError(f"{fn}: radius {radius!r} outside 0..16")
    conn = _check_connectivity(fn, connectivity)
    if not _is_int(max_instances) or not 1 <= int(max_instances) < 1 << 31:
        raise ValueError(f"{fn}: max_instances {max_instances!r} outside 1..2147483647")
    return C_, mask, int(min_seed), int(radius), conn, int(max_instances)


def host_seed_map(cls: np.ndarray, bound=None, dist=None, *, num_classes, classes, bound_below=128, dist_at_least=0) -> np.ndarray:
    """The numpy definition of what rua_scene_seed_map writes, uint8 [H][W].  cls is a uint8 [H][W] class map, bound and dist (each
    may be None) uint8 [H][W][C] maps in the layout predict_scene(heads=) returns.  marker[x] = c = cls[x] where c < C, c is in
    `classes`, (bound is None or bound[x][c] < bound_below) and (dist is None or dist[x][c] >= dist_at_least); 255 elsewhere.
    bound_below 1..256 (256 switches the test off), dist_at_least 0..255."""
    C_, mask, bb, da = check_seed_map(num_classes, classes, bound_below, dist_at_least)
    m = _check_region_map(_SEED, cls, "the class map")
    b = _check_head_map(_SEED, bound, "the boundary map", m.shape, C_)
    d = _check_head_map(_SEED, dist, "the distance map", m.shape, C_)
    chosen = np.array([(mask >> c) & 1 if c < C_ else 0 for c in range(256)], bool)
    keep = chosen[m]
    c = np.minimum(m, C_ - 1).astype(np.int64)[..., None]               # the channel read where the pixel is kept at all
    if b is not None:
        keep &= np.take_along_axis(b, c, 2)[..., 0].astype(np.int64) < bb
    if d is not None:
        keep &= np.take_along_axis(d, c, 2)[..., 0].astype(np.int64) >= da
    return np.where(keep, m, np.uint8(255)).astype(np.uint8)


def host_instances(cls: np.ndarray, marker: np.ndarray, *, num_classes, classes, min_seed=1, radius=4, connectivity=4,
                   max_instances=MAX_INSTANCES):
    """The numpy definition of what rua_scene_regions and rua_scene_instances leave: (inst int32 [H][W], table int32
    [min(N, max_instances)][8], n, ungrown).  A SEED is a region (host_regions under `connectivity`) of `marker` with a byte c < C and
    at least min_seed pixels; seeds are numbered 0..N-1 in ascending order of their root, the region's smallest row-major index.
    A pixel x is ELIGIBLE if c = cls[x] < C and c is in `classes`; its candidates are the seed pixels y with marker[y] == c and
    (x - y) . (x - y) <= radius^2, and inst[x] is the id of the candidate that minimises the pair (squared distance, id), compared
    lexicographically; -1 if there is none and on every pixel that is not eligible.  Pixels outside the map do not exist.  The search
    is EUCLIDEAN, not geodesic: a seed may claim a pixel of its class across a gap of other classes that is narrower than the
    radius - the bounded disc of host_erode and host_boundary_counts, exact in integers and free of any iteration to a fixed point.
    A seed pixel whose class map byte equals its marker byte takes its own id, at distance 0.  Table row k is (root, class, area,
    seed_area, i_min, j_min, i_max, j_max) - TABLE_COLUMNS -, area and bounding box over the pixels with inst == k (an instance
    without a pixel: area 0 and the box H, W, -1, -1); inst always holds the true ids, only the table is capped.  n = N, the
    uncapped seed count; ungrown counts the eligible pixels with inst == -1.  radius 0..16; radius 0 leaves the seeds themselves.
    With marker = host_seed_map(cls, num_classes=C, classes=...) and radius 0 the instances are exactly the connected regions of
    those classes: ground-truth objects are obtained this way."""
    C_, mask, ms, r, conn, cap = check_instances(num_classes, classes, min_seed, radius, connectivity, max_instances)
    cm = _check_region_map(_INST, cls, "the class map")
    mk = _check_region_map(_INST, marker, "the marker map")
    if mk.shape != cm.shape:
        raise ValueError(f"{_INST}: the marker map is {mk.shape}, the class map {cm.shape}")
    H, W = cm.shape
    labels, areas = host_regions(mk, conn)
    flat_area = areas.ravel().astype(np.int64)
    roots = np.flatnonzero((flat_area >= ms) & (mk.ravel() < C_) & (flat_area > 0))      # ascending: the ids
    N = len(roots)
    id_of_root = np.full(H * W, -1, np.int64)
    id_of_root[roots] = np.arange(N)
    sid = id_of_root[labels]                                              # the seed id of every pixel, -1 off the seeds
    chosen = np.array([(mask >> c) & 1 if c < C_ else 0 for c in range(256)], bool)
    eligible = chosen[cm]
    none = np.int64(1) << 62
    best = np.full((H, W), none, np.int64)
    for dy in range(-min(r, H - 1), min(r, H - 1) + 1):
        lim = min(int(np.sqrt(r * r - dy * dy) + 1e-9), W - 1)           # isqrt: the argument is an integer below 2^9
        for dx in range(-lim, lim + 1):
            i0, i1, j0, j1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)    # the pixels whose partner exists
            s = sid[i0 + dy:i1 + dy, j0 + dx:j1 + dx]
            ok = (s >= 0) & (mk[i0 + dy:i1 + dy, j0 + dx:j1 + dx] == cm[i0:i1, j0:j1])
            key = np.where(ok, (np.int64(dy * dy + dx * dx) << 32) | s, none)
            np.minimum(best[i0:i1, j0:j1], key, out=best[i0:i1, j0:j1])
    found = eligible & (best != none)
    inst = np.where(found, best & 0xFFFFFFFF, -1).astype(np.int32)
    rows = min(N, cap)
    table = np.zeros((rows, 8), np.int32)
    if rows:
        table[:, 0] = roots[:rows]
        table[:, 1] = mk.ravel()[roots[:rows]]
        table[:, 3] = flat_area[roots[:rows]]
        table[:, 4], table[:, 5], table[:, 6], table[:, 7] = H, W, -1, -1
        ii, jj = np.nonzero((inst >= 0) & (inst < rows))
        k = inst[ii, jj].astype(np.int64)
        table[:, 2] = np.bincount(k, minlength=rows)
        np.minimum.at(table[:, 4], k, ii.astype(np.int32))
        np.minimum.at(table[:, 5], k, jj.astype(np.int32))
        np.maximum.at(table[:, 6], k, ii.astype(np.int32))
        np.maximum.at(table[:, 7], k, jj.astype(np.int32))
    return inst, table, int(N), int((eligible & ~found).sum())


def _check_inst_map(fn: str, a, what: str) -> np.ndarray:
    a = np.asarray(a)
    if a.dtype != np.int32 or a.ndim != 2 or a.size == 0 or a.size >= 1 << 31:
        raise ValueError(f"{fn}: {what} is a non-empty int32 H x W array of fewer than 2^31 pixels, got {a.dtype} {a.shape}")
    return a


def _check_table(fn: str, a, what: str) -> np.ndarray:
    a = np.asarray(a)
    if a.dtype != np.int32 or a.ndim != 2 or a.shape[1] != 8:
        raise ValueError(f"{fn}: {what} is an int32 [N][8] array, got {a.dtype} {a.shape}")
    return a


def host_instance_match(inst_p: np.ndarray, table_p: np.ndarray, inst_g: np.ndarray, n_g: int) -> np.ndarray:
    """The numpy definition of what rua_scene_instance_match writes, int32 [Np][2] with Np = len(table_p): row P is (g, inter) if
    some ground-truth id 0 <= g < n_g has 2 |{x : inst_p[x] == P and inst_g[x] == g}| > area_P (table_p[P][2]), inter being that
    count; (-1, 0) otherwise.  Two sets with IoU > 1/2 share more than half of each, so every match at an IoU threshold >= 0.5 has
    such a g, and it is unique: the table is all that object scoring at those thresholds needs."""
    p, g = _check_inst_map(_MATCH, inst_p, "inst_p"), _check_inst_map(_MATCH, inst_g, "inst_g")
    t = _check_table(_MATCH, table_p, "table_p")
    if p.shape != g.shape:
        raise ValueError(f"{_MATCH}: inst_p is {p.shape}, inst_g {g.shape}")
    if not _is_int(n_g) or not 0 <= int(n_g) < 1 << 31:
        raise ValueError(f"{_MATCH}: Ng {n_g!r} outside 0..2147483647")
    Np, Ng = len(t), int(n_g)
    out = np.zeros((Np, 2), np.int32)
    out[:, 0] = -1
    both = (p >= 0) & (p < Np) & (g >= 0) & (g < Ng)
    if Np and both.any():
        pair, count = np.unique(p[both].astype(np.int64) * max(Ng, 1) + g[both].astype(np.int64), return_counts=True)
        P = pair // max(Ng, 1)
        won = 2 * count > t[P, 2].astype(np.int64)
        out[P[won], 0] = (pair[won] % max(Ng, 1)).astype(np.int32)
        out[P[won], 1] = count[won].astype(np.int32)
    return out


def instance_scores(table_p, table_g, match, num_classes, iou_percent=IOU_PERCENT) -> dict:
    """Object scores from the two instance tables and host_instance_match's table.  A predicted instance P with match row (g, inter)
    is a true positive at the threshold t (percent) if g >= 0, the classes of P and g are equal and
    100 inter > t (area_P + area_g - inter) - strict and in integers, and t >= 50, so no two predictions can claim one object.  A
    dict: "iou_percent" int64 [T]; "tp", "fp" = Np_c - tp and "fn" = Ng_c - tp, int64 [C][T]; "n_pred", "n_true" int64 [C];
    "precision", "recall" and "f1" float64 [C][T] in percent (precision nan where the class has no prediction, recall nan where it
    has no object, f1 = 200 tp / (2 tp + fp + fn), nan where it has neither); "f1_50" float64 [C], the column of threshold 50 (nan
    if 50 is not listed) and "f1_mean" float64 [C], the mean over the thresholds."""
    fn = "instance_scores"
    tp_, tg_ = _check_table(fn, table_p, "table_p"), _check_table(fn, table_g, "table_g")
    C_ = _check_num_classes(fn, num_classes)
    m = np.asarray(match)
    if m.dtype.kind not in "iu" or m.shape != (len(tp_), 2):
        raise ValueError(f"{fn}: match is an integer [{len(tp_)}][2] array, got {m.dtype} {m.shape}")
    if np.ndim(iou_percent) == 0:
        iou_percent = (iou_percent,)
    thr = list(iou_percent)
    for t in thr:
        if not _is_int(t) or not 50 <= int(t) <= 99:
            raise ValueError(f"{fn}: iou_percent {t!r} outside 50..99 (a match below one half is not unique)")
    if not thr or len(set(int(t) for t in thr)) != len(thr):
        raise ValueError(f"{fn}: iou_percent {iou_percent!r}: a non-empty list of distinct thresholds")
    thr = np.array([int(t) for t in thr], np.int64)
    g, inter = m[:, 0].astype(np.int64), m[:, 1].astype(np.int64)
    if ((g < -1) | (g >= len(tg_))).any():
        raise ValueError(f"{fn}: match names an object outside 0..{len(tg_) - 1}")
    cp, ap = tp_[:, 1].astype(np.int64), tp_[:, 2].astype(np.int64)
    cg, ag = tg_[:, 1].astype(np.int64), tg_[:, 2].astype(np.int64)
    has = g >= 0
    gs = np.where(has, g, 0)
    same = has & (cp < C_) & (cg[gs] == cp) if len(tg_) else np.zeros(len(tp_), bool)
    union = ap + (ag[gs] if len(tg_) else 0) - inter
    hit = same[:, None] & (100 * inter[:, None] > thr[None, :] * union[:, None])                   # [Np][T]
    tp = np.zeros((C_, len(thr)), np.int64)
    np.add.at(tp, np.minimum(cp, C_ - 1)[hit.any(1)], hit[hit.any(1)].astype(np.int64))
    n_pred = np.bincount(cp[cp < C_], minlength=C_).astype(np.int64)
    n_true = np.bincount(cg[cg < C_], minlength=C_).astype(np.int64)
    return _object_scores(thr, tp, n_pred, n_true)


def _object_scores(thr: np.ndarray, tp: np.ndarray, n_pred: np.ndarray, n_true: np.ndarray) -> dict:
    fp, fn_ = n_pred[:, None] - tp, n_true[:, None] - tp

    def ratio(a, b):
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        return np.divide(100.0 * a, b, out=np.full(a.shape, np.nan), where=b != 0)

    f1 = ratio(2 * tp, 2 * tp + fp + fn_)
    at50 = np.flatnonzero(thr == 50)
    return {"iou_percent": thr, "tp": tp, "fp": fp, "fn": fn_, "n_pred": n_pred, "n_true": n_true,
            "precision": ratio(tp, np.broadcast_to(n_pred[:, None], tp.shape)), "recall": ratio(tp, np.broadcast_to(n_true[:, None], tp.shape)),
            "f1": f1, "f1_50": f1[:, at50[0]] if len(at50) else np.full(len(tp), np.nan), "f1_mean": f1.mean(1)}


def sum_instance_scores(scores: Sequence[dict]) -> dict:
    """instance_scores of several scenes as one: the true positives and the object counts are summed per class and threshold (ids
    are per scene, counts are not) and the ratios are taken of the sums.  ValueError unless all were scored at the same thresholds."""
    scores = list(scores)
    if not scores:
        raise ValueError("sum_instance_scores: no scores")
    thr = np.asarray(scores[0]["iou_percent"], np.int64)
    for s in scores[1:]:
        if not np.array_equal(s["iou_percent"], thr) or s["tp"].shape != scores[0]["tp"].shape:
            raise ValueError("sum_instance_scores: the scores differ in their thresholds or classes")
    return _object_scores(thr, *(sum(np.asarray(s[k], np.int64) for s in scores) for k in ("tp", "n_pred", "n_true")))


def _byte_threshold(fn: str, key: str, v, lo: int, hi: int) -> int:
    """An integer is a byte level; a float in 0..1 is quantised as the maps are: rint(255 v)."""
    if isinstance(v, (float, np.floating)):
        if not 0.0 <= float(v) <= 1.0:
            raise ValueError(f"{fn}: {key} {v!r} outside 0..1 (an integer is taken as a byte level {lo}..{hi})")
        v = min(max(int(np.rint(255.0 * float(v))), lo), hi)
    if not _is_int(v) or not lo <= int(v) <= hi:
        raise ValueError(f"{fn}: {key} {v!r} outside {lo}..{hi}")
    return int(v)


INSTANCE_KEYS = ("classes", "bound_below", "dist_at_least", "min_seed", "radius", "connectivity", "iou_percent", "max_instances", "map", "outlines", "flood")


def instance_params(value, C) -> dict:
    """Engine.predict_scene's `instances` as a dict of every key of INSTANCE_KEYS, checked: a class index or a list of classes takes
    the defaults (bound_below 128, dist_at_least 0, min_seed 1, radius 4, connectivity 4, iou_percent 50, 55 .. 95, max_instances
    2^20, map False); a dict may hold any of the keys, `classes` is required.  bound_below and dist_at_least may be floats in 0..1:
    they are quantised with the rounding the maps use, rint(255 v) (bound_below at least 1).  "mask" is added: bit c set for every
    chosen class.  "outlines" (trace the instance maps: host_outlines) is in the result only if it was given, and so is "flood"
    (flood the grown instances down the distance map: host_flood), as flood_params returns it.  ValueError, in the C entries' words,
    for anything else."""
    C_ = _check_num_classes(_INST, C)
    if _is_int(value) or isinstance(value, (list, tuple, np.ndarray)):
        value = {"classes": value}
    if not isinstance(value, dict):
        raise ValueError(f"instances {value!r}: None, a class index, a list of classes or a dict of {', '.join(INSTANCE_KEYS)}")
    unknown = sorted(set(value) - set(INSTANCE_KEYS))
    if unknown:
        raise ValueError(f"instances: unknown key {unknown[0]!r} ({', '.join(INSTANCE_KEYS)})")
    if "classes" not in value:
        raise ValueError("instances: the dict needs classes")
    classes = value["classes"]
    if isinstance(classes, np.ndarray):
        classes = classes.tolist()
    bb = _byte_threshold(_SEED, "bound_below", value.get("bound_below", 128), 1, 256)
    da = _byte_threshold(_SEED, "dist_at_least", value.get("dist_at_least", 0), 0, 255)
    check_seed_map(C_, classes, bb, da)
    _, mask, ms, r, conn, cap = check_instances(C_, classes, value.get("min_seed", 1), value.get("radius", 4), value.get("connectivity", 4),
                                                value.get("max_instances", MAX_INSTANCES))
    iou = value.get("iou_percent", IOU_PERCENT)
    iou = (iou,) if np.ndim(iou) == 0 else tuple(iou)
    empty = np.zeros((0, 8), np.int32)
    instance_scores(empty, empty, np.zeros((0, 2), np.int32), C_, iou)             # its checks
    out = {"classes": tuple(c for c in range(C_) if (mask >> c) & 1), "mask": mask, "bound_below": bb, "dist_at_least": da, "min_seed": ms,
           "radius": r, "connectivity": conn, "iou_percent": tuple(int(t) for t in iou), "max_instances": cap, "map": bool(value.get("map", False))}
    if "outlines" in value:
        out["outlines"] = bool(value["outlines"])
    if "flood" in value:
        out["flood"] = flood_params(value["flood"])
    return out


# ---- flooding: a bounded, marker-controlled watershed of a height map in synchronous rounds ----------------------------------------
_FLOOD = "rua_scene_flood"
FLOOD_KEYS = ("rounds_per_level", "floor", "drain")
MAX_FLOOD_ROUNDS_PER_LEVEL, MAX_FLOOD_DRAIN = 16, 4096


def check_flood(num_classes, classes, connectivity=4, rounds_per_level=1, floor=0, drain=0, fn: str = _FLOOD):
    """(C, class mask, connectivity, rounds_per_level, floor, drain) of rua_scene_flood; ValueError in its own words unless
    1 <= C <= 64, every class is an integer in 0..C-1, connectivity is 4 or 8, rounds_per_level an integer in 1..16, floor one in
    0..255 and drain one in 0..4096."""
    C_ = _check_num_classes(fn, num_classes)
    mask = _class_mask(fn, classes, C_)
    conn = _check_connectivity(fn, connectivity)
    if not _is_int(rounds_per_level) or not 1 <= int(rounds_per_level) <= MAX_FLOOD_ROUNDS_PER_LEVEL:
        raise ValueError(f"{fn}: rounds_per_level {rounds_per_level!r} outside 1..16")
    if not _is_int(floor) or not 0 <= int(floor) <= 255:
        raise ValueError(f"{fn}: floor {floor!r} outside 0..255")
    if not _is_int(drain) or not 0 <= int(drain) <= MAX_FLOOD_DRAIN:
        raise ValueError(f"{fn}: drain {drain!r} outside 0..4096")
    return C_, mask, conn, int(rounds_per_level), int(floor), int(drain)


def flood_rounds(rounds_per_level=1, floor=0, drain=0) -> int:
    """R, the length of the schedule: (256 - floor) rounds_per_level + drain."""
    return (256 - int(floor)) * int(rounds_per_level) + int(drain)


def flood_params(value):
    """The `flood` of ScenePool.instances and of predict_scene's `instances` as a checked dict {rounds_per_level, floor, drain,
    rounds}: True takes the defaults (1, 0, 0); a dict may hold any of FLOOD_KEYS, and its floor may be a float in 0..1, quantised
    with the rounding the maps use, rint(255 v); None and False are None, no flood.  "rounds" is R, the length of the schedule.
    ValueError, in rua_scene_flood's words, for anything else."""
    if value is None or value is False:
        return None
    if value is True:
        value = {}
    if not isinstance(value, dict):
        raise ValueError(f"flood {value!r}: None, True or a dict of {', '.join(FLOOD_KEYS)}")
    unknown = sorted(set(value) - set(FLOOD_KEYS))
    if unknown:
        raise ValueError(f"flood: unknown key {unknown[0]!r} ({', '.join(FLOOD_KEYS)})")
    fl = _byte_threshold(_FLOOD, "floor", value.get("floor", 0), 0, 255)
    _, _, _, J, fl, D = check_flood(1, 0, 4, value.get("rounds_per_level", 1), fl, value.get("drain", 0))
    return {"rounds_per_level": J, "floor": fl, "drain": D, "rounds": flood_rounds(J, fl, D)}


def _flood_height(fn: str, height, cm: np.ndarray, C_: int):
    """The height of every pixel as a uint8 [H][W] array (None stays None), from None, a [H][W] or a [H][W][C] map."""
    if height is None:
        return None
    h = np.asarray(height)
    if h.dtype != np.uint8 or h.shape not in (cm.shape, cm.shape + (C_,)):
        raise ValueError(f"{fn}: the height is None or a uint8 [{cm.shape[0]}][{cm.shape[1]}] or [{cm.shape[0]}][{cm.shape[1]}][{C_}] map, "
                         f"got {h.dtype} {h.shape}")
    if h.ndim == 3:
        h = np.take_along_axis(h, np.minimum(cm, C_ - 1).astype(np.int64)[..., None], 2)[..., 0]    # read where the pixel is eligible
    return h


def host_flood(cls: np.ndarray, height, inst: np.ndarray, *, num_classes, classes, connectivity=4, rounds_per_level=1, floor=0, drain=0):
    """The numpy definition of what rua_scene_flood leaves: (inst_out int32 [H][W], settled, last_round).  cls is the uint8 [H][W]
    class map, inst the int32 id map host_instances left (any radius; -1: no instance).  height is None - every pixel has height
    255 -, a uint8 [H][W] map, or a uint8 [H][W][C] map in the layout predict_scene(heads=("dist",)) returns, the height of x then
    being height[x][cls[x]].  A pixel is ELIGIBLE as in host_instances - cls[x] < C and cls[x] chosen - and SETTLED if inst[x] >= 0.
    The schedule is a list of R = (256 - floor) rounds_per_level + drain rounds: the levels t = 255, 254, .., floor, each
    rounds_per_level times, then `drain` more rounds at level floor.  One round at level t is synchronous, every decision reads the
    state at the start of the round: an eligible, unsettled pixel x with height(x) >= t that has at least one settled neighbour y
    under `connectivity` with cls[y] == cls[x] takes the smallest id among those neighbours (pixels outside the map do not exist);
    nothing else changes, and a settled pixel never changes again.  `settled` is the number of pixels the flood settled,
    `last_round` 1 + the index of the last round that settled one, 0 if none did: last_round == R says that the schedule may have
    cut the flood short.  Meyer's flooding with the priority queue replaced by rounds: breadth-first within a level, a plateau
    wider than rounds_per_level finishes at later levels; with height None a geodesic grow of reach R.  The loop stops early
    where every later round is provably idle; the result is that of the full schedule."""
    C_, mask, conn, J, fl, D = check_flood(num_classes, classes, connectivity, rounds_per_level, floor, drain)
    cm = _check_region_map(_FLOOD, cls, "the class map")
    cur = _check_inst_map(_FLOOD, inst, "inst").copy()
    if cur.shape != cm.shape:
        raise ValueError(f"{_FLOOD}: inst is {cur.shape}, the class map {cm.shape}")
    h = _flood_height(_FLOOD, height, cm, C_)
    H, W = cm.shape
    chosen = np.array([(mask >> c) & 1 if c < C_ else 0 for c in range(256)], bool)
    eligible = chosen[cm]
    key = np.where(eligible, cm, np.uint8(255))
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if conn == 8 else [])
    none = np.int64(1) << 40
    levels, R = (256 - fl) * J, flood_rounds(J, fl, D)
    settled = last = r = 0
    while r < R:
        t = max(255 - r // J, fl)
        open_ = eligible & (cur < 0)
        if not open_.any():
            break
        cand = open_ if h is None else open_ & (h >= t)
        k = 0
        if cand.any():
            best = np.full((H, W), none, np.int64)
            for dy, dx in steps:
                i0, i1, j0, j1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)    # the pixels whose neighbour exists
                if i0 >= i1 or j0 >= j1:
                    continue
                nb = cur[i0 + dy:i1 + dy, j0 + dx:j1 + dx]
                ok = (nb >= 0) & (key[i0 + dy:i1 + dy, j0 + dx:j1 + dx] == key[i0:i1, j0:j1])
                np.minimum(best[i0:i1, j0:j1], np.where(ok, nb.astype(np.int64), none), out=best[i0:i1, j0:j1])
            take = cand & (best != none)
            k = int(take.sum())
            if k:
                cur[take] = best[take].astype(np.int32)
                settled, last = settled + k, r + 1
        if k:
            r += 1
        elif r >= levels:
            break                                                          # the drain: every later round is this one again
        else:
            r = (r // J + 1) * J                                           # so are the rounds left at this level
    return cur, int(settled), int(last)


def flood_table(inst: np.ndarray, table: np.ndarray, cls: np.ndarray, *, num_classes, classes):
    """What rua_scene_flood's last pass makes of host_instances' table and count: (table, ungrown).  The columns area, i_min,
    j_min, i_max and j_max of every row are those of the pixels with inst == row (none: area 0 and the box H, W, -1, -1; an id from
    len(table) on has no row), root, class and seed area stay; ungrown counts the eligible pixels with inst < 0."""
    a, t = _check_inst_map(_FLOOD, inst, "inst"), _check_table(_FLOOD, table, "table").copy()
    cm = _check_region_map(_FLOOD, cls, "the class map")
    C_ = _check_num_classes(_FLOOD, num_classes)
    mask = _class_mask(_FLOOD, classes, C_)
    if a.shape != cm.shape:
        raise ValueError(f"{_FLOOD}: inst is {a.shape}, the class map {cm.shape}")
    H, W = a.shape
    rows = len(t)
    if rows:
        t[:, 2], t[:, 4], t[:, 5], t[:, 6], t[:, 7] = 0, H, W, -1, -1
        ii, jj = np.nonzero((a >= 0) & (a < rows))
        k = a[ii, jj].astype(np.int64)
        t[:, 2] = np.bincount(k, minlength=rows)
        np.minimum.at(t[:, 4], k, ii.astype(np.int32))
        np.minimum.at(t[:, 5], k, jj.astype(np.int32))
        np.maximum.at(t[:, 6], k, ii.astype(np.int32))
        np.maximum.at(t[:, 7], k, jj.astype(np.int32))
    chosen = np.array([(mask >> c) & 1 if c < C_ else 0 for c in range(256)], bool)
    return t, int((chosen[cm] & (a < 0)).sum())


# ---- outlines: the rings of an instance map, their polygons with holes, and a GeoJSON layer --------------------------------------
_OL_COUNT, _OL_RINGS = "rua_scene_outline_count", "rua_scene_outline_rings"
MAX_OUTLINE_PIXELS = 1 << 29                     # keys 4 (H W - 1) + 3 and areas fit an int32
RING_COLUMNS = ("id", "leader_key", "vertex_offset", "vertex_count", "area", "length")
_OL_ACROSS = ((-1, 0), (0, 1), (1, 0), (0, -1))  # the pixel across side s (top, right, bottom, left); the heading of side s is _OL_ACROSS[s + 1]
_OL_END = ((0, 1), (1, 1), (1, 0), (0, 0))       # the end point of side s, from the pixel's corner (i, j)


def check_outlines(shape, connectivity=4, fn: str = _OL_COUNT) -> Tuple[int, int, int]:
    """(H, W, connectivity) of the outline entries; ValueError in their own words."""
    if len(shape) != 2 or not all(_is_int(v) for v in shape) or min(shape) < 1 or int(shape[0]) * int(shape[1]) > MAX_OUTLINE_PIXELS:
        raise ValueError(f"{fn}: size {' x '.join(str(v) for v in shape)} (1 <= H, W and H * W <= 2^29: keys and areas are int32)")
    return int(shape[0]), int(shape[1]), _check_connectivity(fn, connectivity)


def _outline_edges(inst: np.ndarray, conn: int):
    """(exists bool [4 H W], successor key int64 [4 H W]) by edge key, straight from the edge and successor rules."""
    H, W = inst.shape
    P = np.full((H + 2, W + 2), -1, np.int64)
    P[1:-1, 1:-1] = np.where(inst < 0, -1, inst)
    at = lambda di, dj: P[1 + di:1 + di + H, 1 + dj:1 + dj + W]
    k, p = at(0, 0), np.arange(H * W, dtype=np.int64).reshape(H, W)
    exists, succ = np.zeros((H, W, 4), bool), np.zeros((H, W, 4), np.int64)
    for s in range(4):
        (ni, nj), (fi, fj) = _OL_ACROSS[s], _OL_ACROSS[(s + 1) % 4]
        li, lj = fi + ni, fj + nj
        exists[..., s] = (k >= 0) & (at(ni, nj) != k)
        f, l = at(fi, fj) == k, at(li, lj) == k
        left = l & (f | (conn == 8))                                                     # rules 1 and 3
        succ[..., s] = np.where(left, 4 * (p + li * W + lj) + (s + 3) % 4, np.where(f, 4 * (p + fi * W + fj) + s, 4 * p + (s + 1) % 4))
    return exists.reshape(-1), succ.reshape(-1)


def host_outlines(inst: np.ndarray, connectivity: int = 4):
    """The numpy definition of what rua_scene_outline_count and rua_scene_outline_rings leave: (rings int32 [R][6], verts int32 [V][2]).
    An id >= 0 is an object, a negative id none.  A vertex is a grid corner (y, x), 0 <= y <= H, 0 <= x <= W; pixel (i, j) is the
    square between (i, j) and (i+1, j+1).  Pixel p with id k owns a directed edge on side s (0 top, 1 right, 2 bottom, 3 left) if the
    pixel across that side lies outside the map or has another id; the pixel is on the right of the direction of travel, rows
    pointing down: top runs east (i, j) -> (i, j+1), right south, bottom west, left north.  The edge's key is 4 (i W + j) + s.  With F
    the pixel one step along the heading and L the pixel across side s from F, the successor of (p, s) is (L, s+3 mod 4) if F and L
    have id k (a left turn), else (F, s) if F has (straight on), else (L, s+3 mod 4) if connectivity is 8 and L has (across the
    diagonal), else (p, s+1 mod 4) (a right turn).  The cycles are the rings: one outer ring per connected piece of an id, one per
    hole.  A corner edge is one whose successor has another side; its vertex is its end point.  A ring's leader is its edge of smallest
    key; its vertices are those of its corner edges in walking order from the leader (no collinear points: an even number, at least
    4); rings are ordered by leader key and verts is their concatenation.  A ring's row is RING_COLUMNS: id, leader key, vertex
    offset, vertex count, area, length - length the number of unit edges, area the signed enclosed area in pixels (the sum of i + 1
    over the side-2 edges minus the sum of i over the side-0 edges), positive for an outer ring, which runs clockwise on screen,
    negative for a hole."""
    a = _check_inst_map(_OL_COUNT, inst, "inst")
    H, W, conn = check_outlines(a.shape, connectivity)
    exists, succ = _outline_edges(a, conn)
    nxt, flat, seen = succ.tolist(), a.ravel(), bytearray(4 * H * W)
    rings, verts = [], []
    for lead in np.flatnonzero(exists).tolist():                                         # ascending keys: a ring is met first at its leader
        if seen[lead]:
            continue
        e, area, length, first = lead, 0, 0, len(verts)
        while True:
            seen[e] = 1
            (i, j), s = divmod(e >> 2, W), e & 3
            length += 1
            area += i + 1 if s == 2 else -i if s == 0 else 0
            if nxt[e] & 3 != s:
                verts.append((i + _OL_END[s][0], j + _OL_END[s][1]))
            e = nxt[e]
            if e == lead:
                break
        rings.append((int(flat[lead >> 2]), lead, first, len(verts) - first, area, length))
    return np.array(rings, np.int32).reshape(-1, 6), np.array(verts, np.int32).reshape(-1, 2)


def host_outlines_jumping(inst: np.ndarray, connectivity: int = 4):
    """host_outlines by the stages of csrc/outlines.hip, in numpy arrays over the compacted edges: leaders by pointer jumping on
    (min, hop), ranks by the same jumping on (sum, hop) after every cycle was cut in front of its leader (the terminal entry E points
    at itself with weight 0), ceil(log2 E) rounds each, ring numbers and offsets by prefix sums.  The same arrays, without a walk."""
    a = _check_inst_map(_OL_COUNT, inst, "inst")
    H, W, conn = check_outlines(a.shape, connectivity)
    exists, succ = _outline_edges(a, conn)
    keys = np.flatnonzero(exists)
    E = len(keys)
    if E == 0:
        return np.zeros((0, 6), np.int32), np.zeros((0, 2), np.int32)
    nxt = (np.cumsum(exists) - 1)[succ[keys]]                                            # compaction keeps key order
    side, row = keys & 3, (keys >> 2) // W
    corner = ((succ[keys] & 3) != side).astype(np.int64)
    rounds = int(E - 1).bit_length()                                                     # ceil(log2 E)
    lead, hop = np.arange(E), nxt
    for _ in range(rounds):
        lead, hop = np.minimum(lead, lead[hop]), hop[hop]
    tail, hop = np.append(corner, 0), np.append(np.where(nxt == lead, E, nxt), E)
    for _ in range(rounds):
        tail, hop = tail + tail[hop], hop[hop]
    is_lead = lead == np.arange(E)
    ring = (np.cumsum(is_lead) - 1)[lead]
    R = int(is_lead.sum())
    count = np.bincount(ring, corner, R).astype(np.int64)
    area = np.bincount(ring, np.where(side == 2, row + 1, np.where(side == 0, -row, 0)), R).astype(np.int64)
    offset = np.cumsum(count) - count
    rings = np.stack([a.ravel()[keys[is_lead] >> 2], keys[is_lead], offset, count, area, np.bincount(ring, minlength=R)], 1).astype(np.int32)
    c = corner == 1
    verts = np.zeros((int(count.sum()), 2), np.int32)
    end = np.array(_OL_END)[side[c]]
    verts[offset[ring[c]] + count[ring[c]] - tail[:E][c]] = np.stack([row[c] + end[:, 0], (keys[c] >> 2) % W + end[:, 1]], 1)
    return rings, verts


def _check_rings(fn: str, rings, verts):
    r, v = np.asarray(rings), np.asarray(verts)
    if r.ndim != 2 or r.shape[1] != 6 or v.ndim != 2 or v.shape[1] != 2 or r.dtype.kind != "i" or v.dtype.kind != "i":
        raise ValueError(f"{fn}: rings is an integer [R][6] array and verts an integer [V][2] array, got {r.dtype} {r.shape} and {v.dtype} {v.shape}")
    if len(r) and (int(r[:, 3].sum()) != len(v) or (r[:, 2] != np.cumsum(r[:, 3]) - r[:, 3]).any()):
        raise ValueError(f"{fn}: the rings' offsets and counts do not tile the {len(v)} vertices")
    return r.astype(np.int64), v.astype(np.int64)


def _ring_holds(ring: np.ndarray, i: int, j: int) -> bool:
    """Even-odd: does the ring enclose the centre of pixel (i, j)?  The ray runs east; only vertical edges can cross it."""
    y0, x0, y1 = ring[:, 0], ring[:, 1], np.roll(ring[:, 0], -1)
    vertical = (x0 == np.roll(ring[:, 1], -1)) & (x0 > j) & (np.minimum(y0, y1) <= i) & (i < np.maximum(y0, y1))
    return bool(vertical.sum() & 1)


def outline_polygons(rings, verts, table=None, min_area: int = 0) -> List[dict]:
    """The polygons of host_outlines' (rings, verts): a list of dicts {id, class, area, exterior, holes}, one per outer ring, in ring
    order.  exterior is the ring's int [n][2] vertices (y, x), holes a list of such arrays.  A hole goes to the outer ring of the same id
    with the smallest area that contains the pixel owning the hole's leader edge (even-odd; rings of one id never cross, so that ring
    is unique); an id in several pieces gives several polygons.  area is the exterior's area plus the (negative) areas of its holes:
    the pixels of that piece.  class is column 1 of row `id` of `table` (an instance table) or None without one.  Polygons of fewer than
    min_area pixels are left out, with their holes."""
    r, v = _check_rings("outline_polygons", rings, verts)
    if table is not None:
        table = _check_table("outline_polygons", table, "table")
    take = lambda q: v[q[2]:q[2] + q[3]]
    outer = [k for k in range(len(r)) if r[k, 4] > 0]
    polys = {k: {"id": int(r[k, 0]), "class": None if table is None else int(table[r[k, 0], 1]), "area": int(r[k, 4]),
                 "exterior": take(r[k]).astype(np.int32), "holes": []} for k in outer}
    by_id = {}
    for k in outer:
        by_id.setdefault(int(r[k, 0]), []).append(k)
    box = {k: (polys[k]["exterior"].min(0), polys[k]["exterior"].max(0)) for k in outer}
    for q in r[r[:, 4] < 0]:
        hole = take(q)
        # The edges from the leader to the first vertex share its side s, so the one that ends at that vertex is owned by the pixel at
        # vertex - _OL_END[s]: a pixel of the same piece as the leader's (the key alone does not give the pixel without W).
        end = _OL_END[int(q[1]) & 3]
        pi, pj = int(hole[0, 0]) - end[0], int(hole[0, 1]) - end[1]
        best = None
        for k in by_id.get(int(q[0]), ()):
            lo, hi = box[k]
            if lo[0] <= pi < hi[0] and lo[1] <= pj < hi[1] and (best is None or r[k, 4] < r[best, 4]) and _ring_holds(polys[k]["exterior"], pi, pj):
                best = k
        if best is None:
            raise ValueError(f"outline_polygons: the hole with leader key {int(q[1])} lies in no outer ring of id {int(q[0])}")
        polys[best]["holes"].append(hole.astype(np.int32))
        polys[best]["area"] += int(q[4])
    return [polys[k] for k in outer if polys[k]["area"] >= min_area]


def _simplify_chain(pts: np.ndarray, lo: int, hi: int, q: int, keep: np.ndarray) -> None:
    """Douglas-Peucker between the kept vertices lo < hi of pts (int64 [n][2]): the vertex farthest from the chord stays, and both
    halves are treated alike, unless it lies within the tolerance: 256 cross^2 <= q^2 len^2, exact in integers."""
    stack = [(lo, hi)]
    while stack:
        lo, hi = stack.pop()
        if hi - lo < 2:
            continue
        d, rel = pts[hi] - pts[lo], pts[lo + 1:hi] - pts[lo]
        len2 = int(d[0]) * int(d[0]) + int(d[1]) * int(d[1])
        # a chord of length 0 (a ring that touches itself at a corner): the distance from that point
        far2 = (rel[:, 0] * d[1] - rel[:, 1] * d[0]) ** 2 if len2 else (rel ** 2).sum(1)
        k = int(far2.argmax())
        if 256 * int(far2[k]) > q * q * (len2 or 1):
            keep[lo + 1 + k] = True
            stack += [(lo, lo + 1 + k), (lo + 1 + k, hi)]


def simplify_ring(ring, tolerance: float) -> np.ndarray:
    """Douglas-Peucker on a closed ring of vertices (y, x), int [n][2], first vertex not repeated: the ring is anchored at its first
    vertex and at the vertex farthest from it, and both chains between the anchors are simplified with the exact integer test
    256 cross^2 <= q^2 len^2, q = round(16 tolerance), in int64 (coordinates below 2^14 cannot overflow it).  Tolerance 0 returns the
    input, and so does a ring that would be left with fewer than 4 vertices.  The anchors always stay: a ring whose first vertex sits on
    a small notch keeps it.  Known limit: neighbouring polygons are simplified independently and may then overlap, or leave a gap, by up
    to the tolerance."""
    pts = np.asarray(ring)
    if pts.ndim != 2 or pts.shape[1] != 2 or len(pts) < 4 or pts.dtype.kind != "i":
        raise ValueError(f"simplify_ring: a ring is an integer [n][2] array of at least 4 vertices, got {pts.dtype} {pts.shape}")
    if not tolerance >= 0:
        raise ValueError(f"simplify_ring: tolerance {tolerance!r} is negative")
    q = int(round(16 * float(tolerance)))
    if q == 0:
        return pts
    p = pts.astype(np.int64)
    far = int(((p - p[0]) ** 2).sum(1).argmax())
    closed = np.concatenate([p, p[:1]])                                                 # the second chain ends at the first vertex again
    keep = np.zeros(len(closed), bool)
    keep[[0, far]] = True
    _simplify_chain(closed, 0, far, q, keep)
    _simplify_chain(closed, far, len(p), q, keep)
    return pts[keep[:-1]] if keep[:-1].sum() >= 4 else pts


def _shoelace2(xy) -> float:
    """twice the signed area of a closed ring of (X, Y): positive counter-clockwise, Y pointing up"""
    return sum(a[0] * b[1] - b[0] * a[1] for a, b in zip(xy, xy[1:] + xy[:1]))


def write_geojson(path: str, polygons: Sequence[dict], transform=(0.0, 1.0, 0.0, 0.0, 0.0, -1.0), properties=None) -> int:
    """outline_polygons' dicts as a GeoJSON FeatureCollection of Polygon features (the json module only); the number of features.
    transform = (x0, dx, rx, y0, ry, dy) maps a vertex (y, x) to X = x0 + dx x + rx y, Y = y0 + ry x + dy y - the six numbers of a
    world file in GDAL's order; the default maps (y, x) to (x, -y).  Rings are closed (first point repeated), the exterior
    counter-clockwise and the holes clockwise in OUTPUT coordinates, as RFC 7946 asks: the orientation is decided from the signed area
    after the transform.  A feature's properties are id, class and area, updated by `properties` (a dict for every feature, or a
    function of the polygon dict that returns one)."""
    import json
    t = [float(v) for v in transform]
    if len(t) != 6:
        raise ValueError(f"write_geojson: transform {transform!r} is not six numbers (x0, dx, rx, y0, ry, dy)")

    def ring_of(vertices, ccw: bool):
        xy = [[t[0] + t[1] * float(x) + t[2] * float(y), t[3] + t[4] * float(x) + t[5] * float(y)] for y, x in np.asarray(vertices).tolist()]
        if (_shoelace2(xy) > 0) != ccw:
            xy.reverse()
        return xy + [xy[0]]

    features = []
    for poly in polygons:
        props = {"id": poly["id"], "class": poly["class"], "area": poly["area"]}
        if properties is not None:
            props.update(properties(poly) if callable(properties) else properties)
        features.append({"type": "Feature", "properties": props,
                         "geometry": {"type": "Polygon", "coordinates": [ring_of(poly["exterior"], True)] + [ring_of(h, False) for h in poly["holes"]]}})
    with open(path, "w") as f:
        json.dump({"type": "FeatureCollection", "features": features}, f)
    return len(features)

_PASTE = "rua_window_paste"
MAX_PASTE_OFFSET = 1024
BANK_COLUMNS = ("scene", "id", "class", "area", "i_min", "j_min", "i_max", "j_max")
PASTE_WORDS = ("window", "scene", "id", "code", "top", "left", "i0", "j0", "h", "w", "onto_lo", "onto_hi", "flags")


def check_paste_table(shapes: Sequence[Sequence[int]], pastes, N: int, patch, num_classes: int, channels: int = 1) -> np.ndarray:
    """The paste table as a contiguous int32 [M][16] array (M may be 0); ValueError, in rua_window_paste's own words and order, for
    the first violation.  shapes: the (H, W) of every scene; N windows of `patch`; words 10 and 11, the onto mask, are taken mod 2^32."""
    fn = _PASTE
    ph, pw = _patch2(patch)
    t = np.asarray(pastes)
    if t.ndim != 2 or t.shape[1] != 16 or not (np.issubdtype(t.dtype, np.integer) or t.size == 0):
        raise ValueError(f"a paste table is an integer [M][16] array of (window, scene, id, code, top, left, i0, j0, h, w, onto_lo, onto_hi, "
                         f"flags, 0, 0, 0) rows, got {t.dtype} {t.shape}")
    if not _is_int(N) or N < 1:
        raise ValueError(f"{fn}: N {N} (>= 1)")
    if not _is_int(channels) or not 1 <= channels <= MAX_CHANNELS:
        raise ValueError(f"{fn}: Cin {channels} outside 1..16")
    if not (1 <= ph <= MAX_PATCH and 1 <= pw <= MAX_PATCH):
        raise ValueError(f"{fn}: PH {ph}, PW {pw} (1 <= PH, PW <= 512)")
    if not _is_int(num_classes) or not 1 <= int(num_classes) <= MAX_CLASSES:
        raise ValueError(f"{fn}: C {num_classes} outside 1..64")
    if int(N) * ph * pw * int(channels) >= 1 << 31:
        raise ValueError(f"{fn}: N*PH*PW*Cin is {int(N) * ph * pw * int(channels)} (must stay below 2^31)")
    t64 = t.astype(np.int64).reshape(-1, 16)
    t64[:, 10:12] = ((t64[:, 10:12] + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)
    if ((t64 < -(1 << 31)) | (t64 >= 1 << 31)).any():
        raise ValueError(f"{fn}: a word leaves the int32 range")
    n = len(shapes)
    if len(t64) and n < 1:
        raise ValueError(f"{fn}: nscenes {n} (>= 1)")
    prev = 0
    for k, R in enumerate(t64.tolist()):
        if not 0 <= R[0] < N:
            raise ValueError(f"{fn}: row {k}: word 0: window {R[0]} outside 0..{N - 1}")
        if k and R[0] < prev:
            raise ValueError(f"{fn}: row {k}: word 0: window {R[0]} after window {prev} (rows are sorted by window)")
        prev = R[0]
        if not 0 <= R[1] < n:
            raise ValueError(f"{fn}: row {k}: word 1: scene {R[1]} outside 0..{n - 1}")
        if R[2] < 0:
            raise ValueError(f"{fn}: row {k}: word 2: id {R[2]} is negative")
        if not 0 <= R[3] < NUM_CODES:
            raise ValueError(f"{fn}: row {k}: word 3: code {R[3]} outside 0..7")
        for q, what in ((4, "top"), (5, "left")):
            if abs(R[q]) > MAX_PASTE_OFFSET:
                raise ValueError(f"{fn}: row {k}: word {q}: {what} {R[q]} outside -1024..1024")
        for q, what in ((8, "h"), (9, "w")):
            if not 1 <= R[q] <= MAX_PATCH:
                raise ValueError(f"{fn}: row {k}: word {q}: {what} {R[q]} outside 1..512")
        H, W = int(shapes[R[1]][0]), int(shapes[R[1]][1])
        if R[6] < 0 or R[6] + R[8] > H:
            raise ValueError(f"{fn}: row {k}: word 6: rows {R[6]} + {R[8]} leave the {H} x {W} scene")
        if R[7] < 0 or R[7] + R[9] > W:
            raise ValueError(f"{fn}: row {k}: word 7: columns {R[7]} + {R[9]} leave the {H} x {W} scene")
        if R[12] not in (0, 1):
            raise ValueError(f"{fn}: row {k}: word 12: flags {R[12]} (0, or 1: paste over pixels of no class)")
        for q in (13, 14, 15):
            if R[q] != 0:
                raise ValueError(f"{fn}: row {k}: word {q}: reserved, must be 0, got {R[q]}")
    return np.ascontiguousarray(t64, dtype=np.int32)


def host_paste(img: np.ndarray, cls: np.ndarray, images: Sequence[np.ndarray], class_maps: Sequence[np.ndarray],
               inst_maps: Sequence[np.ndarray], pastes, num_classes: int):
    """The numpy definition of what rua_window_paste leaves: (img uint8 [N][PH][PW][Cin], cls uint8 [N][PH][PW]), copies of the
    arguments with the int [M][16] rows of `pastes` applied IN TABLE ORDER.  Row (window, scene, id, code, top, left, i0, j0, h, w,
    onto_lo, onto_hi, flags, 0, 0, 0): the crop is scene[i0:i0+h, j0:j0+w], T = transform(crop, code) lies with its first pixel at
    (top, left) of the window, clipped to it; a destination pixel inside T is pasted iff its source pixel's inst_maps[scene] value
    is `id` and its CURRENT class byte d (after every earlier row) is allowed - d < num_classes: bit d of the 64-bit mask
    onto_lo | onto_hi << 32; otherwise: flags & 1.  A pasted pixel takes its source's image bytes and class byte."""
    img, cls = np.array(img, copy=True), np.array(cls, copy=True)
    if img.dtype != np.uint8 or img.ndim != 4 or cls.dtype != np.uint8 or cls.shape != img.shape[:3]:
        raise ValueError(f"windows are uint8 [N][PH][PW][Cin] with a uint8 [N][PH][PW] class map, got {img.dtype} {img.shape} and {cls.dtype} {cls.shape}")
    N, PH, PW, Cin = img.shape
    t = check_paste_table([im.shape for im in images], pastes, N, (PH, PW), num_classes, Cin)
    for n, s, id_, code, top, left, i0, j0, h, w, lo, hi, flags in t[:, :13].tolist():
        mask = (lo & 0xFFFFFFFF) | ((hi & 0xFFFFFFFF) << 32)
        crop = np.s_[i0:i0 + h, j0:j0 + w]
        Ti, Tc, Tm = transform(images[s][crop], code), transform(class_maps[s][crop], code), transform(np.asarray(inst_maps[s])[crop] == id_, code)
        th, tw = Tm.shape
        y0, y1, x0, x1 = max(top, 0), min(top + th, PH), max(left, 0), min(left + tw, PW)
        if y0 >= y1 or x0 >= x1:
            continue
        allowed = np.array([(mask >> d) & 1 if d < num_classes else flags & 1 for d in range(256)], bool)
        src = np.s_[y0 - top:y1 - top, x0 - left:x1 - left]
        m = Tm[src] & allowed[cls[n, y0:y1, x0:x1]]
        img[n, y0:y1, x0:x1][m] = Ti[src][m]
        cls[n, y0:y1, x0:x1][m] = Tc[src][m]
    return img, cls


def _bank_rows(s: int, table: np.ndarray, max_area, max_extent) -> np.ndarray:
    """The bank rows of scene s from its complete instance table: the area and extent filters of host_object_bank."""
    t = np.asarray(table, np.int64).reshape(-1, 8)
    keep = (t[:, 2] >= 1) & (t[:, 6] - t[:, 4] < max_extent) & (t[:, 7] - t[:, 5] < max_extent)
    if max_area is not None:
        keep &= t[:, 2] <= max_area
    k = np.flatnonzero(keep)
    out = np.empty((len(k), 8), np.int32)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3], out[:, 4:] = s, k, t[k, 1], t[k, 2], t[k, 4:]
    return out


def _check_bank_filters(min_area, max_area, max_extent, default_extent: int):
    if not _is_int(min_area) or not 1 <= int(min_area) < 1 << 31:
        raise ValueError(f"object bank: min_area {min_area!r} outside 1..2147483647")
    if max_area is not None and (not _is_int(max_area) or int(max_area) < int(min_area)):
        raise ValueError(f"object bank: max_area {max_area!r} below min_area {min_area}")
    if max_extent is None:
        max_extent = default_extent
    if not _is_int(max_extent) or not 1 <= int(max_extent) <= MAX_PATCH:
        raise ValueError(f"object bank: max_extent {max_extent!r} outside 1..512 (what rua_window_paste takes)")
    return int(min_area), None if max_area is None else int(max_area), int(max_extent)


def host_object_bank(class_maps: Sequence[np.ndarray], num_classes: int, classes, min_area: int = 1, max_area: Optional[int] = None,
                     max_extent: Optional[int] = None, connectivity: int = 4):
    """The ground-truth objects of uint8 [H][W] class maps, to paste: (inst_maps, bank).  inst_maps[s] is int32 [H][W], host_instances
    at radius 0 of host_seed_map (no heads) with min_seed = min_area: the connected regions (under `connectivity`) of the chosen
    `classes` with at least min_area pixels, numbered per scene from 0 in ascending order of their root (smallest row-major index);
    -1 elsewhere.  bank is int32 [K][8], rows (scene, id, class, area, i_min, j_min, i_max, j_max) - BANK_COLUMNS - in (scene, id)
    order, of the objects with area <= max_area (None: no limit) whose bounding box is at most max_extent high and wide (None: 512,
    the largest crop rua_window_paste takes)."""
    mn, mx, ext = _check_bank_filters(min_area, max_area, max_extent, MAX_PATCH)
    inst_maps, parts = [], []
    for s, cm in enumerate(class_maps):
        marker = host_seed_map(cm, num_classes=num_classes, classes=classes)
        cap = min(MAX_INSTANCES, marker.size)
        inst, table, n, _ = host_instances(cm, marker, num_classes=num_classes, classes=classes, min_seed=mn, radius=0, connectivity=connectivity,
                                           max_instances=cap)
        if n > cap:
            raise ValueError(f"object bank: scene {s} holds {n} objects, more than {cap}")
        inst_maps.append(inst)
        parts.append(_bank_rows(s, table, mx, ext))
    return inst_maps, (np.concatenate(parts) if parts else np.zeros((0, 8), np.int32))


def _onto_masks(onto, classes: np.ndarray) -> np.ndarray:
    """The uint64 onto mask of rows that paste `classes` [M]: None - every class; a sequence of classes - those, for every row; a dict
    pasted class -> classes it may cover (a class without an entry: every class)."""
    every = np.uint64(0xFFFFFFFFFFFFFFFF)
    out = np.full(len(classes), every, np.uint64)
    if onto is None:
        return out
    if isinstance(onto, dict):
        for src, dst in onto.items():
            out[classes == int(src)] = np.uint64(_class_mask("paste onto", dst, MAX_CLASSES))
        return out
    out[:] = np.uint64(_class_mask("paste onto", onto, MAX_CLASSES))
    return out


def paste_rows(bank: np.ndarray, window, bank_index, code, top, left, onto=None, over_void: bool = False) -> np.ndarray:
    """int32 [M][16] paste rows from rows of an object bank: row m pastes object bank[bank_index[m]] - its bounding box is the crop -
    under code[m] with its first pixel at (top[m], left[m]) of window[m]; every argument a scalar or a length-M array.  onto: None
    (the object may cover every class), a sequence of classes, or a dict {pasted class: classes it may cover}; over_void: it may also
    cover pixels that hold no class (a byte >= num_classes).  The rows come back in the order given: a table is sorted by window."""
    b = _check_table("paste_rows", np.asarray(bank, np.int32), "the bank").astype(np.int64)
    args = np.broadcast_arrays(*(np.asarray(v, np.int64) for v in (window, bank_index, code, top, left)))
    win, idx, code, top, left = (a.reshape(-1) for a in args)
    if len(idx) and (idx.min() < 0 or idx.max() >= len(b)):
        raise ValueError(f"paste_rows: bank_index outside 0..{len(b) - 1}")
    o = b[idx]
    out = np.zeros((len(idx), 16), np.int64)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3], out[:, 4], out[:, 5] = win, o[:, 0], o[:, 1], code, top, left
    out[:, 6], out[:, 7], out[:, 8], out[:, 9] = o[:, 4], o[:, 5], o[:, 6] - o[:, 4] + 1, o[:, 7] - o[:, 5] + 1
    masks = _onto_masks(onto, o[:, 2])
    out[:, 10] = (masks & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)
    out[:, 11] = (masks >> np.uint64(32)).astype(np.uint32).view(np.int32)
    out[:, 12] = 1 if over_void else 0
    return out.astype(np.int32)


class CopyPaste:
    """The random part of SceneLoader's copy-paste augmentation (Ghiasi et al., CVPR 2021): per window a number of pastes uniform in
    per_window = (lo, hi), both included; per paste the class uniform over those of `classes` that have objects in the bank - not
    over the objects, so a rare class is pasted as often as a common one -, the object uniform within its class, the code uniform
    in 0..7 and the position uniform over the placements that lie fully inside the window.  onto, over_void: as paste_rows."""

    def __init__(self, classes, per_window: Tuple[int, int] = (0, 3), onto=None, over_void: bool = False):
        self.classes = tuple(sorted({int(c) for c in ((classes,) if _is_int(classes) else classes)}))
        if not self.classes or min(self.classes) < 0 or max(self.classes) >= MAX_CLASSES:
            raise ValueError(f"classes {classes!r}: one or more class indices in 0..63")
        lo, hi = int(per_window[0]), int(per_window[1])
        if not 0 <= lo <= hi:
            raise ValueError(f"per_window range ({lo}, {hi}): 0 <= lo <= hi")
        self.per_window, self.over_void = (lo, hi), bool(over_void)
        _onto_masks(onto, np.zeros(0, np.int64))
        self.onto = onto

    def draw(self, rng: np.random.Generator, bank: np.ndarray, n: int, patch, num_classes: int) -> np.ndarray:
        """The int32 [M][16] paste table of n windows of `patch`, sorted by window - drawn from rng in this order: the n counts, then
        for all M pastes at once the classes, the objects, the codes, the tops, the lefts.  Objects whose bounding box does not fit
        into the patch under every code (a side above the smaller patch side) are never drawn."""
        ph, pw = _patch2(patch)
        b = _check_table("CopyPaste.draw", np.asarray(bank, np.int32), "the bank").astype(np.int64)
        if any(c >= num_classes for c in self.classes):
            raise ValueError(f"CopyPaste: classes {self.classes} for a model of {num_classes} classes")
        h, w = b[:, 6] - b[:, 4] + 1, b[:, 7] - b[:, 5] + 1
        fits = np.maximum(h, w) <= min(ph, pw)
        members = [np.flatnonzero(fits & (b[:, 2] == c)) for c in self.classes]
        members = [m for m in members if len(m)]
        counts = rng.integers(self.per_window[0], self.per_window[1] + 1, int(n))
        M = int(counts.sum())
        if not members or M == 0:
            return np.zeros((0, 16), np.int32)
        which = rng.integers(0, len(members), M)
        size = np.array([len(m) for m in members], np.int64)[which]
        pick = np.minimum((rng.random(M) * size).astype(np.int64), size - 1)
        idx = np.array([members[c][p] for c, p in zip(which.tolist(), pick.tolist())], np.int64)
        code = rng.integers(0, NUM_CODES, M)
        tr = np.isin(code, TRANSPOSING)
        th, tw = np.where(tr, w[idx], h[idx]), np.where(tr, h[idx], w[idx])
        top = np.minimum((rng.random(M) * (ph - th + 1)).astype(np.int64), ph - th)
        left = np.minimum((rng.random(M) * (pw - tw + 1)).astype(np.int64), pw - tw)
        return paste_rows(b, np.repeat(np.arange(int(n)), counts), idx, code, top, left, self.onto, self.over_void)


def _paste_take(table: np.ndarray, windows: np.ndarray) -> np.ndarray:
    """The rows of a paste table whose window is one of `windows` (old indices, in their new order), renumbered and sorted."""
    new = {int(old): k for k, old in enumerate(windows.tolist())}
    keep = [k for k, wdw in enumerate(table[:, 0].tolist()) if wdw in new]
    out = table[keep].copy()
    out[:, 0] = [new[int(wdw)] for wdw in out[:, 0]]
    return np.ascontiguousarray(out[np.argsort(out[:, 0], kind="stable")])


def check_scenes(images: Sequence[np.ndarray], class_maps: Optional[Sequence[np.ndarray]]) -> int:
    """Scenes are uint8 H x W x C with one C for all, class maps uint8 H x W of their image's size.  Returns C."""
    if len(images) < 1:
        raise ValueError("no scenes")
    if class_maps is not None and len(class_maps) != len(images):
        raise ValueError(f"{len(images)} scenes but {len(class_maps)} class maps")
    ch = None
    for s, im in enumerate(images):
        if im.dtype != np.uint8 or im.ndim != 3:
            raise ValueError(f"scene {s}: images are uint8 H x W x C, got {im.dtype} {im.shape}")
        ch = im.shape[2] if ch is None else ch
        if im.shape[2] != ch or not 1 <= ch <= MAX_CHANNELS:
            raise ValueError(f"scene {s}: {im.shape[2]} channels (scene 0 has {ch}; 1..{MAX_CHANNELS} supported)")
        if class_maps is not None:
            cm = class_maps[s]
            if cm.dtype != np.uint8 or cm.shape != im.shape[:2]:
                raise ValueError(f"scene {s}: its class map is uint8 {im.shape[0]} x {im.shape[1]}, got {cm.dtype} {cm.shape}")
    return int(ch)


class SceneBatch:
    """A batch named by index: a pool, int32 [B][4] table rows and the patch size.  Takes the place of x in Engine.train_step /
    test_step / predict and Model.train_on_batch / test_on_batch / predict (y is None: the class maps are the pool's).
    photo: None, or the checked int32 [B][16] photo table (check_photo_table) whose row k jitters window k after it is cut.
    paste: None, or the checked int32 [M][16] paste table (check_paste_table) whose rows drop objects of the pool's bank into the
    cut windows, before the photo table lights them."""

    def __init__(self, pool: "ScenePool", rows: np.ndarray, patch: Tuple[int, int], photo: Optional[np.ndarray] = None,
                 paste: Optional[np.ndarray] = None):
        self.pool, self.rows, self.patch, self.photo, self.paste = pool, rows, patch, photo, paste

    @property
    def shape(self):
        return (self.rows.shape[0], self.patch[0], self.patch[1], self.pool.channels)

    def __len__(self):
        return self.rows.shape[0]

    def __getitem__(self, sl):
        """The windows of a slice, with their photo rows and their paste rows (renumbered to the slice's windows)."""
        if not isinstance(sl, slice):
            raise TypeError("a SceneBatch is sliced, not indexed")
        return type(self)(self.pool, np.ascontiguousarray(self.rows[sl]), self.patch,
                          None if self.photo is None else np.ascontiguousarray(self.photo[sl]),
                          None if self.paste is None else _paste_take(self.paste, np.arange(len(self))[sl]))

    def with_photo(self, table16) -> "SceneBatch":
        """A batch of the same class and rows that carries this photo table, one row per window (None: none)."""
        if table16 is None:
            return type(self)(self.pool, self.rows, self.patch, None, self.paste)
        t = check_photo_table(table16, self.pool.channels)
        if len(t) != len(self):
            raise ValueError(f"{len(t)} photo rows for a batch of {len(self)} windows")
        return type(self)(self.pool, self.rows, self.patch, t, self.paste)

    def with_paste(self, table) -> "SceneBatch":
        """A batch of the same class, rows and photo table that carries this paste table (None: none), checked against the pool in
        rua_window_paste's words.  The ids are those of the pool's resident id maps: ValueError before ScenePool.object_bank()."""
        if table is None:
            return type(self)(self.pool, self.rows, self.patch, self.photo, None)
        if self.pool.bank is None:
            raise ValueError("with_paste: this pool has no object bank yet (ScenePool.object_bank() builds the id maps a paste row names)")
        t = check_paste_table(self.pool.shapes, table, len(self), self.patch, self.pool.bank_classes, self.pool.channels)
        return type(self)(self.pool, self.rows, self.patch, self.photo, t)

    def shard(self, rank: int, world: int) -> "SceneBatch":
        """This rank's contiguous share of a global batch (the split Model._local_batch makes)."""
        B = len(self)
        if B % world:
            raise ValueError(f"global batch {B} not divisible by {world} replicas")
        return self[rank * (B // world):(rank + 1) * (B // world)]

    def _cut(self):
        return host_windows(self.pool.images, self.pool.class_maps, self.rows, self.patch)

    def host(self):
        """host_windows of this batch; with a paste table, host_paste of both; with a photo table, host_photometric of the image
        after that (the class map is untouched by it): cut, then paste, then photo."""
        img, cls = self._cut()
        if self.paste is not None:
            if cls is None:
                raise ValueError("a paste table needs class maps: this pool holds none")
            img, cls = host_paste(img, cls, self.pool.images, self.pool.class_maps, self.pool.inst_maps, self.paste, self.pool.bank_classes)
        return (img if self.photo is None else host_photometric(img, self.photo)), cls


class AffineSceneBatch(SceneBatch):
    """A SceneBatch whose rows are the int32 [B][7] affine table (check_affine_table): rua_scene_windows_affine cuts it;
    host() is host_windows_affine of it (and host_photometric of that, with a photo table)."""

    def _cut(self):
        return host_windows_affine(self.pool.images, self.pool.class_maps, self.rows, self.patch)


class Jitter:
    """The random part of SceneLoader's augmentation: the angle uniform in [-rotate_deg, rotate_deg], the zoom log-uniform in
    zoom = (lo, hi), the shift uniform in whole Q16 units within [-shift, shift] pixels on either axis."""

    def __init__(self, rotate_deg: float = 180.0, zoom: Tuple[float, float] = (0.75, 1.33), shift: float = 16.0):
        lo, hi = float(zoom[0]), float(zoom[1])
        if not 0 < lo <= hi:
            raise ValueError(f"zoom range ({lo}, {hi}): 0 < lo <= hi")
        if rotate_deg < 0 or shift < 0:
            raise ValueError(f"rotate_deg {rotate_deg} and shift {shift} are magnitudes (>= 0)")
        self.rotate_deg, self.zoom, self.shift = float(rotate_deg), (lo, hi), float(shift)

    def draw(self, rng: np.random.Generator, n: int):
        """(angles in degrees [n], zooms [n], Q16 shifts int64 [n][2]) - in this order from rng."""
        angle = rng.uniform(-self.rotate_deg, self.rotate_deg, n)
        zoom = np.exp(rng.uniform(np.log(self.zoom[0]), np.log(self.zoom[1]), n))
        s = int(round(self.shift * Q16))
        return angle, zoom, rng.integers(-s, s + 1, (n, 2), dtype=np.int64)


class ScenePool:
    """Scenes uploaded once: uint8 H x W x C images (one C for all) and, for training, their uint8 H x W class maps.  Keeps the
    host arrays of device pointers and sizes rua_scene_windows takes.  patch: checked against every scene, and the default of
    batch().  device "cpu" keeps the scenes in host memory: table checks and host_windows work, the engine refuses it."""

    def __init__(self, images: Sequence[np.ndarray], class_maps: Optional[Sequence[np.ndarray]] = None, patch=None, device="cuda"):
        import torch
        self.images = [np.ascontiguousarray(im) for im in images]
        self.class_maps = None if class_maps is None else [np.ascontiguousarray(cm) for cm in class_maps]
        self.channels = check_scenes(self.images, self.class_maps)
        self.shapes: List[Tuple[int, int]] = [(im.shape[0], im.shape[1]) for im in self.images]
        self.patch = None if patch is None else _patch2(patch)
        if self.patch is not None:
            for s, (H, W) in enumerate(self.shapes):
                if H < self.patch[0] or W < self.patch[1]:
                    raise ValueError(f"scene {s} is {H} x {W}: smaller than the {self.patch[0]} x {self.patch[1]} patch")
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.img_dev = [torch.from_numpy(im).to(self.device) for im in self.images]
        self.cls_dev = None if self.class_maps is None else [torch.from_numpy(cm).to(self.device) for cm in self.class_maps]
        n = len(self.images)
        self.img_ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in self.img_dev])
        self.cls_ptrs = None if self.cls_dev is None else (C.c_void_p * n)(*[t.data_ptr() for t in self.cls_dev])
        self.heights = (C.c_int32 * n)(*[h for h, _ in self.shapes])
        self.widths = (C.c_int32 * n)(*[w for _, w in self.shapes])
        # object_bank(): the objects to paste (host, int32 [K][8]), the class count they were made under, the resident id maps
        self.bank = self.bank_classes = self.inst_dev = self.inst_ptrs = self._inst_host = None

    def __len__(self):
        return len(self.images)

    def object_bank(self, num_classes: int, classes, min_area: int = 1, max_area: Optional[int] = None, max_extent: Optional[int] = None,
                    connectivity: int = 4) -> np.ndarray:
        """host_object_bank of the pool's class maps, on the device: per scene rua_scene_seed_map, rua_scene_regions and
        rua_scene_instances at radius 0 with min_seed = min_area (the ground-truth objects), one fetch of the object table, and the
        marker, labels, areas and work buffers are freed before the next scene.  The int32 id maps STAY RESIDENT - self.inst_dev,
        self.inst_ptrs, what rua_window_paste reads -: 4 bytes per scene pixel, 144 MB for a 6000 x 6000 tile, next to the 4 bytes
        per pixel of its image and class map.  self.bank is the host table, int32 [K][8] (BANK_COLUMNS), and is returned;
        self.bank_classes is num_classes.  max_extent None: the smaller side of the pool's patch (512 without one).  A "cpu" pool
        holds the host definition's maps.  Calling it again replaces all of it."""
        if self.class_maps is None:
            raise ValueError("object_bank: this scene pool holds no class maps")
        default = MAX_PATCH if self.patch is None else min(min(self.patch), MAX_PATCH)
        mn, mx, ext = _check_bank_filters(min_area, max_area, max_extent, default)
        C_, mask, bb, da = check_seed_map(num_classes, classes)
        _, _, _, _, conn, _ = check_instances(C_, classes, mn, 0, connectivity)
        self.inst_dev = self.inst_ptrs = self._inst_host = None
        if self.device.type != "cuda":
            self._inst_host, self.bank = host_object_bank(self.class_maps, C_, [c for c in range(C_) if (mask >> c) & 1], mn, mx, ext, conn)
        else:
            import torch
            inst_dev, parts = [], []
            with torch.cuda.device(self.device):
                st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
                for s, (H, W) in enumerate(self.shapes):
                    keep, cap = [], min(MAX_INSTANCES, H * W)
                    inst, table, n = self._device_instances(self.cls_dev[s].data_ptr(), None, None, (H, W), C_, mask, bb, da, mn, 0, conn, cap, st, keep)
                    N = int(n.cpu().numpy()[0])                         # the fetch waits for the scene's calls
                    del keep                                             # marker, labels, areas, work: scratch
                    if N > cap:
                        raise ValueError(f"object bank: scene {s} holds {N} objects, more than {cap}")
                    parts.append(_bank_rows(s, table[:N].cpu().numpy(), mx, ext))
                    inst_dev.append(inst)
                    del table, n
            self.inst_dev = inst_dev
            self.inst_ptrs = (C.c_void_p * len(inst_dev))(*[t.data_ptr() for t in inst_dev])
            self.bank = np.concatenate(parts)
        self.bank_classes = C_
        return self.bank

    @property
    def inst_maps(self) -> List[np.ndarray]:
        """The id maps of object_bank() on the host, int32 [H][W] per scene (a device pool fetches them once, on first use)."""
        if self.bank is None:
            raise ValueError("no object bank yet: ScenePool.object_bank() builds the id maps")
        if self._inst_host is None:
            self._inst_host = [t.cpu().numpy() for t in self.inst_dev]
        return self._inst_host

    def batch(self, rows, patch=None) -> SceneBatch:
        """The batch of these table rows; ValueError (rua_scene_windows' wording) for a row the kernel would refuse."""
        p = self.patch if patch is None else _patch2(patch)
        if p is None:
            raise ValueError("no patch size: give ScenePool(patch=) or batch(rows, patch)")
        return SceneBatch(self, check_table(self.shapes, rows, p), p)

    def affine_batch(self, table7, patch=None) -> AffineSceneBatch:
        """The batch of these [N][7] affine rows; ValueError (rua_scene_windows_affine's wording) for what the kernel would refuse."""
        p = self.patch if patch is None else _patch2(patch)
        if p is None:
            raise ValueError("no patch size: give ScenePool(patch=) or affine_batch(table7, patch)")
        return AffineSceneBatch(self, check_affine_table(self.shapes, table7, p, self.channels), p)

    def class_counts(self, rows, num_classes: int, patch=None) -> np.ndarray:
        """int64 [N][C + 1] class counts of these table rows (host_class_counts is the definition).  The distinct (scene, row,
        col) windows - the reference's five copies of a window are one - are counted in one rua_scene_class_counts call on the
        resident class maps, fetched once and scattered back to the rows; a "cpu" pool returns host_class_counts."""
        p = self.patch if patch is None else _patch2(patch)
        if p is None:
            raise ValueError("no patch size: give ScenePool(patch=) or class_counts(rows, num_classes, patch)")
        if self.class_maps is None:
            raise ValueError("class_counts needs the pool's class maps")
        C_ = _check_classes(num_classes)
        t = check_table(self.shapes, rows, p)
        if self.device.type != "cuda":
            return host_class_counts(self.class_maps, t, p, C_)
        import torch
        from . import _lib as L
        uniq, inverse = np.unique(t[:, :3], axis=0, return_inverse=True)
        win = np.zeros((len(uniq), 4), np.int32)                            # code 0: a symmetry does not change the counts
        win[:, :3] = uniq
        with torch.cuda.device(self.device):
            out = torch.empty((len(win), C_ + 1), dtype=torch.int32, device=self.device)
            L.lib().call("rua_scene_class_counts", self.cls_ptrs, self.heights, self.widths, len(self), win.ctypes.data, len(win), p[0], p[1], C_,
                         out.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
            got = out.cpu().numpy()
        return got.astype(np.int64)[np.asarray(inverse).reshape(-1)]

    def eroded_maps(self, radius: int) -> List[np.ndarray]:
        """host_erode of every class map of the pool, a list of uint8 [H][W] arrays: one rua_scene_erode call over all resident
        class maps into one device buffer, fetched once; a "cpu" pool returns host_erode of each map."""
        if self.class_maps is None:
            raise ValueError("eroded_maps needs the pool's class maps")
        r = check_radius(radius)
        if self.device.type != "cuda":
            return [host_erode(cm, r) for cm in self.class_maps]
        import torch
        from . import _lib as L
        sizes = [h * w for h, w in self.shapes]
        first = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        with torch.cuda.device(self.device):
            out = torch.empty((int(first[-1]),), dtype=torch.uint8, device=self.device)
            out_ptrs = (C.c_void_p * len(self))(*[out.data_ptr() + int(o) for o in first[:-1]])
            L.lib().call("rua_scene_erode", self.cls_ptrs, self.heights, self.widths, len(self), r, out_ptrs, None, 0, None,
                         C.c_void_p(torch.cuda.current_stream().cuda_stream))
            got = out.cpu().numpy()
        return [got[first[s]:first[s + 1]].reshape(self.shapes[s]).copy() for s in range(len(self))]

    def _check_preds(self, preds) -> list:
        preds = list(preds)
        if len(preds) != len(self):
            raise ValueError(f"rua_scene_boundary: {len(preds)} prediction maps for {len(self)} scenes (one per scene, None to skip one)")
        out = []
        for s, p in enumerate(preds):
            if p is not None:
                p = np.ascontiguousarray(_check_boundary_map(p, f"scene {s}: the prediction map"))
                if p.shape != self.shapes[s]:
                    raise ValueError(f"rua_scene_boundary: scene {s}: the prediction map is {p.shape}, the class map {self.shapes[s]}")
            out.append(p)
        return out

    def boundary_counts(self, preds, radius: int, num_classes: int) -> np.ndarray:
        """int64 [n][C][4], host_boundary_counts of every scene's class map and preds[s], a uint8 [H][W] map per scene of the pool
        (a None entry skips its scene: its rows stay 0) - the boundary F1 of maps that come from files, without a model
        (boundary_scores of the result, or of one scene's rows).  The maps are uploaded in one copy, rua_scene_boundary is called once per scored
        scene into that scene's [C][4] cells of one device buffer (the call sums its scenes into one set of counts), and the buffer
        is fetched once; a "cpu" pool returns the host definition."""
        if self.class_maps is None:
            raise ValueError("boundary_counts needs the pool's class maps")
        r = check_tolerance(radius)
        if r is None:
            raise ValueError("rua_scene_boundary: radius None is no integer")
        C_ = _check_boundary_classes(num_classes)
        preds = self._check_preds(preds)
        if self.device.type != "cuda":
            out = np.zeros((len(self), C_, 4), np.int64)
            for s, p in enumerate(preds):
                if p is not None:
                    out[s] = host_boundary_counts(self.class_maps[s], p, r, C_)
            return out
        import torch
        from . import _lib as L
        with torch.cuda.device(self.device):
            counts = torch.zeros((len(self), C_, 4), dtype=torch.int64, device=self.device)
            st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            scored = [s for s, p in enumerate(preds) if p is not None]
            if not scored:
                return counts.cpu().numpy()
            first = np.concatenate([[0], np.cumsum([preds[s].size for s in scored])]).astype(np.int64)
            dev = torch.from_numpy(np.concatenate([preds[s].ravel() for s in scored])).to(self.device)      # one upload for all maps
            for k, s in enumerate(scored):
                H, W = self.shapes[s]
                L.lib().call("rua_scene_boundary", (C.c_void_p * 1)(self.cls_dev[s].data_ptr()), (C.c_void_p * 1)(dev.data_ptr() + int(first[k])),
                             (C.c_int32 * 1)(H), (C.c_int32 * 1)(W), 1, r, C_, None, None, counts[s].data_ptr(), st)
            return counts.cpu().numpy()

    def boundary_maps(self, num_classes: int) -> List[np.ndarray]:
        """host_boundaries of every class map of the pool, a list of uint8 [H][W] arrays: one rua_scene_boundary call over all
        resident class maps into one device buffer, fetched once; a "cpu" pool returns host_boundaries of each map."""
        if self.class_maps is None:
            raise ValueError("boundary_maps needs the pool's class maps")
        C_ = _check_boundary_classes(num_classes)
        if self.device.type != "cuda":
            return [host_boundaries(cm, C_) for cm in self.class_maps]
        import torch
        from . import _lib as L
        sizes = [h * w for h, w in self.shapes]
        first = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        with torch.cuda.device(self.device):
            out = torch.empty((int(first[-1]),), dtype=torch.uint8, device=self.device)
            out_ptrs = (C.c_void_p * len(self))(*[out.data_ptr() + int(o) for o in first[:-1]])
            L.lib().call("rua_scene_boundary", self.cls_ptrs, self.cls_ptrs, self.heights, self.widths, len(self), 0, C_, out_ptrs, None, None,
                         C.c_void_p(torch.cuda.current_stream().cuda_stream))
            got = out.cpu().numpy()
        return [got[first[s]:first[s + 1]].reshape(self.shapes[s]).copy() for s in range(len(self))]

    def _check_region_maps(self, fn: str, maps) -> list:
        maps = list(maps)
        if len(maps) != len(self):
            raise ValueError(f"{fn}: {len(maps)} maps for {len(self)} scenes (one per scene, None to skip one)")
        out = []
        for s, m in enumerate(maps):
            if m is not None:
                m = np.ascontiguousarray(_check_region_map(fn, m, f"scene {s}: the map"))
                if m.shape != self.shapes[s]:
                    raise ValueError(f"{fn}: scene {s}: the map is {m.shape}, the scene {self.shapes[s]}")
            out.append(m)
        return out

    def _region_buffers(self, maps):
        """One upload of these maps, and int32 labels and areas beside them: (scenes given, device tensors map / labels / areas, the
        ctypes arrays of per-scene pointers map / labels / areas / heights / widths, the first pixel of every scene in the buffers)."""
        import torch
        given = [s for s, m in enumerate(maps) if m is not None]
        first = np.concatenate([[0], np.cumsum([maps[s].size for s in given])]).astype(np.int64)
        dev = torch.from_numpy(np.concatenate([maps[s].ravel() for s in given])).to(self.device)
        labels, areas = (torch.empty((int(first[-1]),), dtype=torch.int32, device=self.device) for _ in range(2))
        n = len(given)
        ptrs = lambda t, unit: (C.c_void_p * n)(*[t.data_ptr() + unit * int(o) for o in first[:-1]])
        hs, ws = (C.c_int32 * n)(*[self.shapes[s][0] for s in given]), (C.c_int32 * n)(*[self.shapes[s][1] for s in given])
        return given, (dev, labels, areas), (ptrs(dev, 1), ptrs(labels, 4), ptrs(areas, 4), hs, ws), first

    def region_counts(self, maps=None, *, min_area: int, num_classes: int, connectivity: int = 4) -> np.ndarray:
        """int64 [n][C][3], host_region_counts of every scene: per class the connected regions, those of fewer than min_area pixels and
        the pixels these hold - of the pool's class maps (maps None), or of maps[s], a uint8 [H][W] map per scene of the pool that
        came from a file (a None entry skips its scene: its rows stay 0).  The maps are uploaded in one copy, rua_scene_regions is
        called once per counted scene into that scene's [C][3] cells of one device buffer (a call sums its scenes into one set of
        counts), and the buffer is fetched once; a "cpu" pool returns the host definition."""
        fn = "rua_scene_regions"
        mn, C_, _, conn, _, _ = check_sieve(min_area, num_classes, connectivity=connectivity, fn=fn)
        if maps is None:
            if self.class_maps is None:
                raise ValueError("region_counts needs maps, or the pool's class maps")
            maps = self.class_maps
        maps = self._check_region_maps(fn, maps)
        if self.device.type != "cuda":
            out = np.zeros((len(self), C_, 3), np.int64)
            for s, m in enumerate(maps):
                if m is not None:
                    out[s] = host_region_counts(m, mn, C_, conn)
            return out
        import torch
        from . import _lib as L
        with torch.cuda.device(self.device):
            counts = torch.zeros((len(self), C_, 3), dtype=torch.int64, device=self.device)
            if all(m is None for m in maps):
                return counts.cpu().numpy()
            st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            given, keep, (mp, lp, ap, hs, ws), _ = self._region_buffers(maps)
            one = lambda a, k, t: (t * 1)(a[k])
            for k, s in enumerate(given):
                L.lib().call(fn, one(mp, k, C.c_void_p), one(hs, k, C.c_int32), one(ws, k, C.c_int32), 1, conn, one(lp, k, C.c_void_p),
                             one(ap, k, C.c_void_p), mn, C_, counts[s].data_ptr(), st)
            return counts.cpu().numpy()

    def sieved_maps(self, maps, min_area: int, num_classes: int, mode: str, connectivity: int = 4, classes=None, rounds: int = 1) -> List[np.ndarray]:
        """host_sieve of maps[s], a uint8 [H][W] map per scene of the pool (a None entry skips its scene and gives None), as a list of
        uint8 maps: one upload of all maps, `rounds` times one rua_scene_regions and one rua_scene_sieve call over all of them
        between two device buffers, and one fetch; a "cpu" pool returns the host definition."""
        fn = "rua_scene_sieve"
        mn, C_, md, conn, mask, n = check_sieve(min_area, num_classes, mode, connectivity, classes, rounds)
        maps = self._check_region_maps(fn, maps)
        if self.device.type != "cuda":
            return [None if m is None else host_sieve(m, mn, C_, mode, conn, classes, n) for m in maps]
        if all(m is None for m in maps):
            return [None] * len(maps)
        import torch
        from . import _lib as L
        with torch.cuda.device(self.device):
            st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            given, (dev, labels, areas), (mp, lp, ap, hs, ws), first = self._region_buffers(maps)
            other = torch.empty_like(dev)
            op = (C.c_void_p * len(given))(*[other.data_ptr() + int(o) for o in first[:-1]])
            nwork = sum(int(L.lib().raw("rua_scene_sieve_work_bytes")(*self.shapes[s], C_)) for s in given) if md == 1 else 0
            work = torch.empty((nwork // 4,), dtype=torch.int32, device=self.device) if nwork else None
            for _ in range(n):
                L.lib().call("rua_scene_regions", mp, hs, ws, len(given), conn, lp, ap, mn, C_, None, st)
                L.lib().call(fn, mp, hs, ws, len(given), conn, mn, C_, mask, md, lp, ap, op, work.data_ptr() if nwork else None, nwork, None, st)
                dev, other, mp, op = other, dev, op, mp
            got = dev.cpu().numpy()
        out = [None] * len(maps)
        for k, s in enumerate(given):
            out[s] = got[first[k]:first[k + 1]].reshape(self.shapes[s]).copy()
        return out

    def _device_instances(self, cls_ptr: int, bound_ptr, dist_ptr, shape, C_, mask, bb, da, ms, r, conn, cap, st, keep: list, marker=None):
        """The three calls that turn resident maps into instances, issued on stream `st`: rua_scene_seed_map (unless `marker`, a
        device tensor, is given), rua_scene_regions of the marker, rua_scene_instances.  Returns the device tensors (inst int32
        [H][W], table int32 [cap][8] - zeroed first, so rows from N on hold area 0 -, n int32 [2]); every buffer the calls use is
        appended to `keep`, which the caller holds until the stream has run them."""
        import torch
        from . import _lib as L
        H, W = shape
        dev = self.device
        if marker is None:
            marker = torch.empty((H, W), dtype=torch.uint8, device=dev)
            L.lib().call(_SEED, cls_ptr, bound_ptr, dist_ptr, H, W, C_, mask, bb, da, marker.data_ptr(), st)
        labels, areas, inst = (torch.empty((H, W), dtype=torch.int32, device=dev) for _ in range(3))
        one = lambda v, t=C.c_void_p: (t * 1)(v)
        L.lib().call("rua_scene_regions", one(marker.data_ptr()), one(H, C.c_int32), one(W, C.c_int32), 1, conn, one(labels.data_ptr()),
                     one(areas.data_ptr()), 1, 1, None, st)
        nwork = int(L.lib().raw("rua_scene_instances_work_bytes")(H, W))
        work = torch.empty((nwork // 4,), dtype=torch.int32, device=dev)
        table = torch.zeros((cap, 8), dtype=torch.int32, device=dev)
        n = torch.zeros((2,), dtype=torch.int32, device=dev)
        L.lib().call(_INST, cls_ptr, marker.data_ptr(), labels.data_ptr(), areas.data_ptr(), H, W, C_, mask, ms, r, work.data_ptr(), nwork,
                     inst.data_ptr(), table.data_ptr(), cap, n.data_ptr(), st)
        keep += [marker, labels, areas, work]
        return inst, table, n

    def _device_flood(self, cls_ptr: int, height_ptr, pix_stride: int, per_class: int, shape, C_, mask, conn, fp: dict, inst, table, cap, n,
                      st, keep: list):
        """rua_scene_flood of a resident instance map on stream `st`, in place: inst, and with them table and n (both may be
        None), are the flooded ones afterwards.  fp is flood_params' dict.  Returns the device tensor stats int32 [2] (settled,
        last_round); the work buffer is appended to `keep`."""
        import torch
        from . import _lib as L
        H, W = shape
        nwork = int(L.lib().raw("rua_scene_flood_work_bytes")(H, W))
        work = torch.empty((nwork // 4,), dtype=torch.int32, device=self.device)
        stats = torch.zeros((2,), dtype=torch.int32, device=self.device)
        L.lib().call(_FLOOD, cls_ptr, height_ptr, pix_stride, per_class, H, W, C_, mask, conn, fp["rounds_per_level"], fp["floor"], fp["drain"],
                     work.data_ptr(), nwork, inst.data_ptr(), None if table is None else table.data_ptr(), cap,
                     None if table is None else n.data_ptr(), stats.data_ptr(), st)
        keep.append(work)
        return stats

    def _device_match(self, inst_p, table_p, inst_g, Ng: int, shape, st, keep: list):
        """rua_scene_instance_match of two resident instance maps on stream `st`: the device tensor int32 [rows of table_p][2]."""
        import torch
        from . import _lib as L
        Np = int(table_p.shape[0])
        nwork = int(L.lib().raw("rua_scene_instance_match_work_bytes")(Np, Ng))
        work = torch.empty((max(nwork // 4, 1),), dtype=torch.int32, device=self.device)
        match = torch.empty((Np, 2), dtype=torch.int32, device=self.device)
        L.lib().call(_MATCH, inst_p.data_ptr(), table_p.data_ptr() + 8 if Np else None, Np, inst_g.data_ptr(), Ng, shape[0], shape[1],
                     work.data_ptr(), nwork, match.data_ptr() if Np else None, st)
        keep.append(work)
        return match

    def instances(self, maps, bound=None, dist=None, *, num_classes, classes, bound_below=128, dist_at_least=0, min_seed=1, radius=4,
                  connectivity=4, max_instances=MAX_INSTANCES, want_map=True, flood=None):
        """host_seed_map and host_instances of maps[s], a uint8 [H][W] class map per scene of the pool that came from a file (a None
        entry skips its scene and gives None), with bound[s] and dist[s], uint8 [H][W][C] maps or None, as a list of
        (inst int32 [H][W] or None without want_map, table int32 [n][8], n, ungrown): per scene one upload, rua_scene_seed_map,
        rua_scene_regions and rua_scene_instances on the current stream, and one fetch after all scenes were issued; a "cpu" pool
        returns the host definitions.  flood (True or a dict, flood_params): the grown instances are then flooded over their class
        (host_flood; rua_scene_flood on the same stream) with dist[s] as the per-class height, without a height where it is None;
        inst, table and ungrown are the flooded ones (flood_table), and each tuple gains a fifth element {"settled", "last_round",
        "rounds"}.  ValueError naming both numbers if a scene holds more than max_instances seeds."""
        C_, mask, bb, da = check_seed_map(num_classes, classes, bound_below, dist_at_least)
        _, _, ms, r, conn, cap = check_instances(C_, classes, min_seed, radius, connectivity, max_instances)
        fp = flood_params(flood)
        chosen = [c for c in range(C_) if (mask >> c) & 1]
        maps = self._check_region_maps(_INST, maps)
        heads = []
        for what, given in (("boundary", bound), ("distance", dist)):
            given = [None] * len(self) if given is None else list(given)
            if len(given) != len(self):
                raise ValueError(f"{_SEED}: {len(given)} {what} maps for {len(self)} scenes (one per scene, or None)")
            heads.append([None if a is None or maps[s] is None else np.ascontiguousarray(_check_head_map(_SEED, a, f"scene {s}: the {what} map", self.shapes[s], C_))
                          for s, a in enumerate(given)])
        out = [None] * len(self)
        if self.device.type != "cuda":
            for s, m in enumerate(maps):
                if m is not None:
                    marker = host_seed_map(m, heads[0][s], heads[1][s], num_classes=C_, classes=chosen, bound_below=bb, dist_at_least=da)
                    out[s] = host_instances(m, marker, num_classes=C_, classes=chosen, min_seed=ms, radius=r, connectivity=conn, max_instances=cap)
                    if fp is not None:
                        inst, settled, last = host_flood(m, heads[1][s], out[s][0], num_classes=C_, classes=chosen, connectivity=conn,
                                                         rounds_per_level=fp["rounds_per_level"], floor=fp["floor"], drain=fp["drain"])
                        table, ungrown = flood_table(inst, out[s][1], m, num_classes=C_, classes=chosen)
                        out[s] = (inst, table, out[s][2], ungrown, {"settled": settled, "last_round": last, "rounds": fp["rounds"]})
        else:
            import torch
            with torch.cuda.device(self.device):
                st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
                keep, issued = [], {}
                for s, m in enumerate(maps):
                    if m is None:
                        continue
                    H, W = self.shapes[s]
                    dev = [None if a is None else torch.from_numpy(a).to(self.device) for a in (m, heads[0][s], heads[1][s])]
                    keep += dev
                    issued[s] = self._device_instances(dev[0].data_ptr(), None if dev[1] is None else dev[1].data_ptr(),
                                                       None if dev[2] is None else dev[2].data_ptr(), (H, W), C_, mask, bb, da, ms, r, conn,
                                                       min(cap, H * W), st, keep)
                    if fp is not None:
                        inst, table, n = issued[s]
                        stats = self._device_flood(dev[0].data_ptr(), None if dev[2] is None else dev[2].data_ptr(), C_, 1, (H, W), C_, mask, conn,
                                                   fp, inst, table, min(cap, H * W), n, st, keep)
                        issued[s] += (stats,)
                for s, (inst, table, n, *stats) in issued.items():
                    N, ungrown = (int(v) for v in n.cpu().numpy())
                    out[s] = (inst.cpu().numpy(), table[:min(N, cap)].cpu().numpy(), N, ungrown)
                    if stats:
                        settled, last = (int(v) for v in stats[0].cpu().numpy())
                        out[s] += ({"settled": settled, "last_round": last, "rounds": fp["rounds"]},)
        for s, res in enumerate(out):
            if res is not None:
                if res[2] > cap:
                    raise ValueError(f"{_INST}: scene {s} holds {res[2]} seeds, max_instances is {cap}")
                if not want_map:
                    out[s] = (None,) + tuple(res[1:])
        return out

    def instance_match(self, inst_p, table_p, inst_g, table_g) -> np.ndarray:
        """host_instance_match(inst_p, table_p, inst_g, len(table_g)), int32 [Np][2], of two instance maps of one size with their
        complete tables: one upload, one rua_scene_instance_match call and one fetch; a "cpu" pool returns the host definition."""
        p, g = _check_inst_map(_MATCH, inst_p, "inst_p"), _check_inst_map(_MATCH, inst_g, "inst_g")
        tp, tg = _check_table(_MATCH, table_p, "table_p"), _check_table(_MATCH, table_g, "table_g")
        if p.shape != g.shape:
            raise ValueError(f"{_MATCH}: inst_p is {p.shape}, inst_g {g.shape}")
        if self.device.type != "cuda" or len(tp) == 0:
            return host_instance_match(p, tp, g, len(tg))
        import torch
        with torch.cuda.device(self.device):
            st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            keep = []
            dp, dg, dt = (torch.from_numpy(np.ascontiguousarray(a)).to(self.device) for a in (p, g, tp))
            return self._device_match(dp, dt, dg, len(tg), p.shape, st, keep).cpu().numpy()

    def _device_outlines(self, inst, shape, conn: int, st):
        """host_outlines of a resident int32 [H][W] id map, as numpy arrays: rua_scene_outline_count on stream `st`, one fetch of its
        16 bytes (E, V) - the outputs are sized by them -, rua_scene_outline_rings, one fetch of rings, vertices and R."""
        import torch
        from . import _lib as L
        H, W = shape
        dev = self.device
        i32 = lambda n: torch.empty((max(n, 1),), dtype=torch.int32, device=dev)
        base, n = i32(H * W), torch.empty((2,), dtype=torch.int64, device=dev)
        nwork = int(L.lib().raw("rua_scene_outline_work_bytes")(H, W, 0))
        work = i32(nwork // 4)
        L.lib().call(_OL_COUNT, inst.data_ptr(), H, W, conn, base.data_ptr(), work.data_ptr(), nwork, n.data_ptr(), st)
        E, V = (int(v) for v in n.cpu().numpy())                                         # the one readback between the two calls
        if E == 0:
            return np.zeros((0, 6), np.int32), np.zeros((0, 2), np.int32)
        nwork = int(L.lib().raw("rua_scene_outline_work_bytes")(H, W, E))
        work = i32(nwork // 4)
        rings, verts = i32(V // 4 * 6).view(-1, 6), i32(V * 2).view(-1, 2)
        L.lib().call(_OL_RINGS, inst.data_ptr(), base.data_ptr(), H, W, conn, E, V, work.data_ptr(), nwork, rings.data_ptr(), verts.data_ptr(),
                     n.data_ptr(), st)
        R = int(n.cpu().numpy()[0])
        return rings[:R].cpu().numpy(), verts.cpu().numpy()

    def outlines(self, inst_maps=None, connectivity: int = 4):
        """host_outlines of one int32 [H][W] id map per scene, as a list of (rings int32 [R][6], verts int32 [V][2]) (a None entry
        skips its scene and gives None).  inst_maps None: the pool's own ground-truth id maps, where object_bank() left them resident.
        Maps given as numpy arrays are uploaded; per scene rua_scene_outline_count, a fetch of 16 bytes, rua_scene_outline_rings and
        the fetch of the result, on the current stream.  A "cpu" pool returns the host definition."""
        if inst_maps is None:
            if self.bank is None:
                raise ValueError("no object bank yet: ScenePool.object_bank() builds the id maps")
            maps = self.inst_dev if self.device.type == "cuda" else self._inst_host
        else:
            maps = list(inst_maps)
            if len(maps) != len(self):
                raise ValueError(f"{_OL_COUNT}: {len(maps)} maps for {len(self)} scenes (one per scene, None to skip one)")
            maps = [None if m is None else np.ascontiguousarray(_check_inst_map(_OL_COUNT, m, f"scene {s}: the map")) for s, m in enumerate(maps)]
        conn = _check_connectivity(_OL_COUNT, connectivity)
        for s, m in enumerate(maps):
            if m is not None:
                check_outlines(tuple(m.shape), conn)
                if tuple(m.shape) != self.shapes[s]:
                    raise ValueError(f"{_OL_COUNT}: scene {s}: the map is {tuple(m.shape)}, the scene {self.shapes[s]}")
        if self.device.type != "cuda":
            return [None if m is None else host_outlines(m, conn) for m in maps]
        import torch
        with torch.cuda.device(self.device):
            st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            return [None if m is None else self._device_outlines(torch.from_numpy(m).to(self.device) if isinstance(m, np.ndarray) else m,
                                                                 self.shapes[s], conn, st) for s, m in enumerate(maps)]

    def _area_open(self, given, dev, first, lv, mn, conn, st):
        """rua_scene_area_open of the dense maps of the scenes `given` that lie in `dev` from first[k] on: the opened maps in one
        device buffer of the same layout, and the ctypes arrays of per-scene pointers map / opened / heights / widths."""
        import torch
        from . import _lib as L
        n = len(given)
        ptrs = lambda t, unit: (C.c_void_p * n)(*[t.data_ptr() + unit * int(o) for o in first[:-1]])
        hs, ws = (C.c_int32 * n)(*[self.shapes[s][0] for s in given]), (C.c_int32 * n)(*[self.shapes[s][1] for s in given])
        opened = torch.empty_like(dev)
        mp, op = ptrs(dev, 1), ptrs(opened, 1)
        lp = ap = None
        if mn > 1:
            labels, areas = (torch.empty((int(first[-1]),), dtype=torch.int32, device=self.device) for _ in range(2))
            lp, ap = ptrs(labels, 4), ptrs(areas, 4)
        L.lib().call("rua_scene_area_open", mp, hs, ws, n, 1, lv.ctypes.data, len(lv), mn, conn, op, lp, ap, st)
        return opened, (mp, op, hs, ws)

    def opened_maps(self, probs, thresholds=None, min_area: int = 1, connectivity: int = 4) -> List[np.ndarray]:
        """host_area_open of probs[s], a uint8 [H][W] probability map per scene of the pool (a None entry skips its scene and gives
        None), as a list of uint8 maps: one upload of all maps, one rua_scene_area_open call over all of them and one fetch; a "cpu"
        pool returns the host definition."""
        fn = "rua_scene_area_open"
        lv, mn, conn = sweep_levels(thresholds), _check_min_area(fn, min_area), _check_connectivity(fn, connectivity)
        probs = self._check_region_maps(fn, probs)
        if self.device.type != "cuda":
            return [None if p is None else host_area_open(p, lv, mn, conn) for p in probs]
        given = [s for s, p in enumerate(probs) if p is not None]
        if not given:
            return [None] * len(probs)
        import torch
        with torch.cuda.device(self.device):
            st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            first = np.concatenate([[0], np.cumsum([probs[s].size for s in given])]).astype(np.int64)
            dev = torch.from_numpy(np.concatenate([probs[s].ravel() for s in given])).to(self.device)
            opened, _ = self._area_open(given, dev, first, lv, mn, conn, st)
            got = opened.cpu().numpy()
        out = [None] * len(probs)
        for k, s in enumerate(given):
            out[s] = got[first[k]:first[k + 1]].reshape(self.shapes[s]).copy()
        return out

    def sweep_hist(self, probs, positive: int, num_classes: int, thresholds=None, min_area: int = 1, connectivity: int = 4) -> np.ndarray:
        """int64 [n][2][2][256], host_sweep_hist of probs[s] - a uint8 [H][W] map of class `positive`'s probability per scene of the
        pool, None to skip a scene (its cells stay 0) - against the pool's class maps; sweep_scores of a scene's cells, or of their
        sum, is the precision-recall curve.  min_area 1 opens nothing: hist[1] is hist[0].  Otherwise the opened map is
        host_area_open at these thresholds (sweep_levels), and the curve is read at those levels.  One upload of all maps, one
        rua_scene_area_open call over all of them (min_area > 1), one rua_scene_sweep_hist call per scene into that scene's cells
        of one device buffer (a call sums its scenes into one histogram) and one fetch; a "cpu" pool returns the host definition."""
        fn = "rua_scene_sweep_hist"
        if self.class_maps is None:
            raise ValueError("sweep_hist needs the pool's class maps")
        pos, lv, mn, conn, _ = sweep_params({"positive": positive, "thresholds": thresholds, "min_area": min_area, "connectivity": connectivity},
                                            num_classes)
        C_ = int(num_classes)
        probs = self._check_region_maps(fn, probs)
        given = [s for s, p in enumerate(probs) if p is not None]
        if self.device.type != "cuda":
            out = np.zeros((len(self), 2, 2, 256), np.int64)
            for s in given:
                out[s] = host_sweep_hist(probs[s], host_area_open(probs[s], lv, mn, conn) if mn > 1 else None, self.class_maps[s], pos, C_)
            return out
        import torch
        from . import _lib as L
        with torch.cuda.device(self.device):
            hist = torch.zeros((len(self), 2, 2, 256), dtype=torch.int64, device=self.device)
            if not given:
                return hist.cpu().numpy()
            st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            first = np.concatenate([[0], np.cumsum([probs[s].size for s in given])]).astype(np.int64)
            dev = torch.from_numpy(np.concatenate([probs[s].ravel() for s in given])).to(self.device)
            opened = None
            if mn > 1:
                opened, _ = self._area_open(given, dev, first, lv, mn, conn, st)
            one = lambda v, t=C.c_void_p: (t * 1)(v)
            for k, s in enumerate(given):
                H, W = self.shapes[s]
                L.lib().call(fn, one(dev.data_ptr() + int(first[k])), None if opened is None else one(opened.data_ptr() + int(first[k])),
                             one(self.cls_dev[s].data_ptr()), one(H, C.c_int32), one(W, C.c_int32), 1, 1, pos, C_, hist[s].data_ptr(), st)
            return hist.cpu().numpy()

    def predict_table(self, scene: int, stride: Optional[int] = None):
        """predict_table of scene `scene` with the pool's patch (stride None: the patch, non-overlapping windows), rows naming it."""
        if self.patch is None:
            raise ValueError("no patch size: give ScenePool(patch=)")
        if not 0 <= int(scene) < len(self):
            raise ValueError(f"scene {scene} outside 0..{len(self) - 1}")
        if stride is None:
            stride = self.patch
        rows, own = predict_table(self.shapes[int(scene)], self.patch, stride)
        rows[:, 0] = int(scene)
        return rows, own


class SceneLoader:
    """loader.PrefetchLoader's iteration over a window table instead of files: `len(order) // batch_size` batches per pass, the
    last partial batch dropped, `batch_size` the GLOBAL batch of which rank r yields rows [r * B / world, (r + 1) * B / world).
    Yields (SceneBatch, None); order: indices into `table` (default: all of it, in order).
    jitter (a Jitter): batch k of pass e (e counts __iter__ calls from 0) draws one rotation, zoom and shift per row of the GLOBAL
    batch from np.random.default_rng([seed, e, k]), turns its rows into affine rows (affine_rows) and every rank takes its own:
    a world of 2 sees exactly the windows a world of 1 sees.  Yields (AffineSceneBatch, None) then.
    photo (a PhotoJitter): batch k of pass e draws the GLOBAL batch's photo table from np.random.default_rng([seed, e, k, 1]) - a
    stream of its own: the draws of jitter= are what they are without it -, every rank takes its own rows, and the batches carry
    them (SceneBatch.photo).  Passes are counted with photo alone as with jitter.
    paste (a CopyPaste; the pool has its object_bank()): batch k of pass e draws the GLOBAL batch's paste table from
    np.random.default_rng([seed, e, k, 2]) - again a stream of its own -, every rank takes the rows of its windows, renumbered, and
    the batches carry them (SceneBatch.paste).  Passes are counted with paste alone too."""

    def __init__(self, pool: ScenePool, table: np.ndarray, batch_size: int, patch=None, order: Optional[Sequence[int]] = None,
                 rank: int = 0, world: int = 1, jitter: Optional[Jitter] = None, seed: int = 0, photo: Optional[PhotoJitter] = None,
                 paste: Optional[CopyPaste] = None):
        if batch_size < 1:
            raise ValueError("batch_size must be >= 1")
        if world < 1 or not (0 <= rank < world):
            raise ValueError(f"rank {rank} outside world {world}")
        if batch_size % world:
            raise ValueError(f"global batch {batch_size} not divisible by {world} replicas")
        self.pool, self.table, self.patch = pool, np.asarray(table), patch
        self.B, self.rank, self.local_B = int(batch_size), int(rank), int(batch_size) // int(world)
        self.order = np.arange(len(self.table)) if order is None else np.asarray(order, dtype=np.int64)
        self.jitter, self.photo, self.seed, self.passes = jitter, photo, int(seed), 0
        if paste is not None and pool.bank is None:
            raise ValueError("SceneLoader(paste=): this pool has no object bank yet (ScenePool.object_bank())")
        self.paste = paste

    def __len__(self) -> int:
        return len(self.order) // self.B

    def set_order(self, order: Sequence[int]) -> None:
        self.order = np.asarray(order, dtype=np.int64)

    def __iter__(self):
        if self.jitter is None and self.photo is None and self.paste is None:
            return self._plain(None)
        e, self.passes = self.passes, self.passes + 1
        return self._jittered(e) if self.jitter is not None else self._plain(e)

    def _with_photo(self, batch: SceneBatch, e: Optional[int], k: int) -> SceneBatch:
        """The rank's batch with its rows of the global batch's photo and paste tables."""
        if self.paste is not None:
            table = self.paste.draw(np.random.default_rng([self.seed, e, k, 2]), self.pool.bank, self.B, batch.patch, self.pool.bank_classes)
            batch = batch.with_paste(_paste_take(table, np.arange(self.rank * self.local_B, (self.rank + 1) * self.local_B)))
        if self.photo is None:
            return batch
        table = self.photo.draw(np.random.default_rng([self.seed, e, k, 1]), self.B, self.pool.channels)
        return batch.with_photo(table[self.rank * self.local_B:(self.rank + 1) * self.local_B])

    def _plain(self, e: Optional[int]):
        for k in range(len(self)):
            first = k * self.B + self.rank * self.local_B
            yield self._with_photo(self.pool.batch(self.table[self.order[first:first + self.local_B]], self.patch), e, k), None

    def _jittered(self, e: int):
        patch = self.pool.patch if self.patch is None else _patch2(self.patch)
        if patch is None:
            raise ValueError("no patch size: give ScenePool(patch=) or SceneLoader(patch=)")
        for k in range(len(self)):
            angle, zoom, shift = self.jitter.draw(np.random.default_rng([self.seed, e, k]), self.B)
            rows = affine_rows(self.table[self.order[k * self.B:(k + 1) * self.B]], patch, angle, zoom, shift)
            yield self._with_photo(self.pool.affine_batch(rows[self.rank * self.local_B:(self.rank + 1) * self.local_B], patch), e, k), None


# ---- scene directories ------------------------------------------------------------------------------------------------------
def save_scene_dir(root: str, names: Sequence[str], images: Sequence[np.ndarray], class_maps: Sequence[np.ndarray]) -> None:
    check_scenes(images, class_maps)
    os.makedirs(os.path.join(root, "scenes"), exist_ok=True)
    os.makedirs(os.path.join(root, "labels", "scenes"), exist_ok=True)
    for n, im, cm in zip(names, images, class_maps):
        np.save(os.path.join(root, "scenes", n + ".npy"), im)
        np.save(os.path.join(root, "labels", "scenes", n + ".npy"), cm)


def load_scene_dir(root: str):
    """(names, images, class maps) of a scene directory, sorted by name and paired by file name."""
    files = sorted(n for n in os.listdir(os.path.join(root, "scenes")) if n.endswith(".npy"))
    if not files:
        raise FileNotFoundError(f"{os.path.join(root, 'scenes')} holds no .npy scene")
    have = set(os.listdir(os.path.join(root, "labels", "scenes")))
    missing = [n for n in files if n not in have]
    if missing:
        raise FileNotFoundError(f"labels/scenes lacks {len(missing)} scenes, e.g. {missing[0]}")
    images = [np.load(os.path.join(root, "scenes", n)) for n in files]
    class_maps = [np.load(os.path.join(root, "labels", "scenes", n)) for n in files]
    try:
        check_scenes(images, class_maps)
    except ValueError as exc:
        raise ValueError(f"{root}: {exc} (scenes in name order: {files})") from None
    return [n[:-4] for n in files], images, class_maps


def patch_name(k: int) -> str:
    return f"patch_{k}.npy"


def patch_index(name: str) -> int:
    """k of `patch_{k}.npy` (a bare name or a path)."""
    base = os.path.basename(name)
    if not (base.startswith("patch_") and base.endswith(".npy") and base[6:-4].isdigit()):
        raise ValueError(f"{name}: not a patch_<k>.npy name")
    return int(base[6:-4])


def materialize(root: str, dst: str, patch, stride: int, data_aug: bool, chunk: int = 256) -> int:
    """Writes the compact patch layout of a scene directory's window table: <dst>/images/patch_{k}.npy and
    <dst>/labels/classes/patch_{k}.npy for table row k.  Returns the number of patches."""
    _, images, class_maps = load_scene_dir(root)
    table = window_table([im.shape for im in images], patch, stride, data_aug)
    os.makedirs(os.path.join(dst, "images"), exist_ok=True)
    os.makedirs(os.path.join(dst, "labels", "classes"), exist_ok=True)
    for k0 in range(0, len(table), chunk):
        img, cls = host_windows(images, class_maps, table[k0:k0 + chunk], patch)
        for k in range(len(img)):
            np.save(os.path.join(dst, "images", patch_name(k0 + k)), img[k])
            np.save(os.path.join(dst, "labels", "classes", patch_name(k0 + k)), cls[k])
    return len(table)


# ---- the reference's inputs -------------------------------------------------------------------------------------------------
def colours_to_classes(ref_hwc: np.ndarray, colours=None, unknown: str = "error") -> np.ndarray:
    """uint8 class map of a colour-coded H x W x 3 label image.  unknown "error": ValueError naming the first (row-major) pixel of an
    unknown colour; "void": such pixels become 255, "no class" (the ISPRS benchmark's clutter (255, 0, 0) is in neither colour table)."""
    if unknown not in ("error", "void"):
        raise ValueError(f"unknown={unknown!r}: 'error' or 'void'")
    colours = ISPRS_COLOURS if colours is None else colours
    a = np.asarray(ref_hwc)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"a colour-coded reference is H x W x 3, got {a.shape}")
    key = (a[..., 0].astype(np.int64) << 16) | (a[..., 1].astype(np.int64) << 8) | a[..., 2].astype(np.int64)
    out = np.zeros(a.shape[:2], np.uint8)
    known = np.zeros(a.shape[:2], bool)
    for (r, g, b), v in colours.items():
        m = key == ((r << 16) | (g << 8) | b)
        out[m] = v
        known |= m
    if unknown == "void":
        out[~known] = 255
    elif not known.all():
        i, j = np.unravel_index(int(np.argmin(known)), known.shape)
        raise ValueError(f"unknown colour {tuple(int(v) for v in a[i, j])} at row {i}, column {j}: not one of {sorted(colours)}")
    return out


def convert_reference_inputs(image_chw: np.ndarray, reference_chw: np.ndarray, unknown: str = "error"):
    """(uint8 H x W x C image, uint8 H x W class map) from the reference's C x H x W Image_Train / Reference_Train arrays
    (unknown: colours_to_classes)."""
    if image_chw.ndim != 3 or reference_chw.ndim != 3:
        raise ValueError(f"C x H x W arrays expected, got {image_chw.shape} and {reference_chw.shape}")
    if image_chw.dtype != np.uint8:
        raise ValueError(f"the image must be uint8, got {image_chw.dtype}")
    if image_chw.shape[1:] != reference_chw.shape[1:]:
        raise ValueError(f"image is {image_chw.shape[1:]}, reference {reference_chw.shape[1:]}")
    img = np.ascontiguousarray(image_chw.transpose(1, 2, 0))
    return img, colours_to_classes(reference_chw.transpose(1, 2, 0), unknown=unknown)


def _yes(v) -> bool:
    s = str(v).lower()
    if s in ("yes", "true", "t", "y", "1"):
        return True
    if s in ("no", "false", "f", "n", "0"):
        return False
    raise argparse.ArgumentTypeError("Boolean value expected.")


def main(argv=None) -> int:
    p = argparse.ArgumentParser(description="write a scene directory from the reference's Image_Train.npy / Reference_Train.npy")
    p.add_argument("--image", required=True, help="C x H x W uint8 image (.npy)")
    p.add_argument("--reference", required=True, help="3 x H x W colour-coded labels (.npy)")
    p.add_argument("--dst", required=True, help="output scene directory: scenes/ and labels/scenes/")
    p.add_argument("--name", default="scene", help="file name of the scene")
    p.add_argument("--materialize", default=None, metavar="DST", help="also write the compact patch layout of the window table there")
    p.add_argument("-ps", "--patch_size", type=int, default=256)
    p.add_argument("--stride", type=int, default=32)
    p.add_argument("--data_aug", type=_yes, default=True)
    p.add_argument("--unknown_colour", choices=["error", "void"], default="error",
                   help="a label colour outside the table: refuse it (error), or write class 255, 'no class' (void; train with --ignore_void yes)")
    a = p.parse_args(argv)
    img, cls = convert_reference_inputs(np.load(a.image), np.load(a.reference), unknown=a.unknown_colour)
    save_scene_dir(a.dst, [a.name], [img], [cls])
    print(f"scene {a.name}: {img.shape[0]} x {img.shape[1]} x {img.shape[2]} written to {a.dst}")
    if a.materialize:
        n = materialize(a.dst, a.materialize, a.patch_size, a.stride, a.data_aug)
        print(f"{n} patches written to {a.materialize}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
