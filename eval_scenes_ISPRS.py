"""Evaluation of a trained model on whole scenes, on the GPU: what test_ISPRS.py does for the reference's test tile (patches,
predict, arg-max, metrics, mosaic), for a scene directory (resunet_a_mltsk_keras_amd.scenes: scenes/<name>.npy,
labels/scenes/<name>.npy) as `train_ISPRS.py --scene_dataset yes` trains from.  test_ISPRS.py's flags, plus --stride, --views, --scales, --blend, --erode_boundary,
--boundary_f1, --sieve, --pr_curve, --instances, --polygons and --head_maps.

Every scene stays on the GPU, is covered by windows --stride apart (default: the patch; the last window flush with the border, so
nothing is left unpredicted), every pixel is predicted from the window it is most central in, and Model.predict_scene brings back
only the uint8 class map and the C x C confusion matrix.  metrics_from_confusion turns the matrix into the accuracy / F1 / recall /
precision of test_ISPRS.compute_metrics_hw.  Per scene it writes `pred_seg_reconstructed_<name>.npy/.ppm` and
`confusion_matrix_<name>.npy`; the printed and returned metrics are those of the summed matrix.

--views is test-time augmentation: every window is predicted under the named symmetries (`none`, `flips`, `aug5` - the five copies
`--data_aug` trains on -, `all`, or a list of codes 0..7 of scenes.transform) in one forward, and the arg-max is taken of the sum of
the turned-back probabilities (scenes.host_stitch_views).  The output files are the same.

--scales Z [Z ...] is multi-scale test-time augmentation, the evaluation side of `train_ISPRS.py --aug_zoom`: the scene is covered once
per zoom Z (> 1 zooms in; a window covers patch / Z scene pixels per axis, scenes.scale_footprint), every cover under all --views, the
probabilities are resampled back onto the scene grid and summed in an int32 accumulator on the GPU (scenes.host_accumulate), and the
arg-max of the sums is the class map (scenes.host_argmax).  `--scales 1` is the single-scale path; --scales and --head_maps exclude
each other.  The output files are the same.

--blend linear blends overlapping windows instead of giving every pixel to the window it is most central in: each window's
probabilities enter an int32 accumulator on the GPU under a linear taper (scenes.blend_weight: full weight in the middle and towards
the scene's border, 1/16 at least), summed over the --views and the --scales, and the arg-max of the sums is the class map
(scenes.host_accumulate_blend, scenes.host_argmax).  --stride then defaults to half the patch; --blend and --head_maps exclude each
other.  The output files are the same, plus `eval_settings.json` with the views, scales, stride and blend of the run.

--erode_boundary R also scores on the eroded ground truth, the one the ISPRS benchmark and the ResUNet-a paper publish numbers on
(R = 3 there): class-map pixels within a disc of radius R of a pixel of another value are left out (scenes.host_erode), on the GPU,
against the same stitched map.  After the full block a second one follows, `Eroded ground truth (radius R)` and the same five
entries; per scene `confusion_matrix_eroded_<name>.npy` is written, and the returned dict gains the `*_eroded` keys.

--boundary_f1 R also scores the class edges themselves, which the area scores above do not and the eroded protocol leaves out: the
boundary F1 (BF score, Csurka et al. 2013) with a tolerance of R pixels (0..16; 0 is exact coincidence) - per class the share of
the predicted boundary pixels that have a true one of their class within R pixels (precision), the share of the true ones that
have a predicted one (recall), and their F1 (scenes.host_boundary_counts, scenes.boundary_scores), counted on the GPU against the
un-eroded class map.  Per scene `boundary_counts_<name>.npy` (int64 C x 4: n_pred, m_pred, n_true, m_true) is written; after the
blocks above a block `Boundary F1 (tolerance R px)` follows, scored on the counts summed over the scenes (the published BF score
averages per image: the per-scene files allow that); the returned dict gains `boundary_counts`, `boundary_precision`,
`boundary_recall`, `boundary_f1` and `boundary_f1_mean`.

--sieve N [--sieve_mode fill|void] [--sieve_connectivity 4|8] [--sieve_classes c ...] [--sieve_rounds R] cleans the finished map
with a minimum mapping unit before anything scores it: the connected regions (of equal class, 4- or 8-connected) of fewer than N
pixels are removed on the GPU (scenes.host_sieve) - `fill` gives each the class most of its kept 4-neighbours have, `void` turns
them into 255, which no score counts -, only those of the classes --sieve_classes names (default: all), --sieve_rounds times.
`--sieve 69 --sieve_mode void --sieve_classes 1` is the reference's `prediction` protocol (an area opening of 69 pixels, the removed
pixels left out of the score).  The written map and every block of scores are then the sieved map's; per scene the region counts of
the un-sieved map (per class: regions, regions below N pixels, their pixels) and the pixels changed are printed and
`region_counts_<name>.npy` (int64 C x 3) is written; after the sieved scores a block `Before the sieve` prints those of the raw map;
the returned dict gains `confusion_matrix_raw`, `region_counts` and `sieve_changed`.

--pr_curve C [--pr_thresholds T ...] [--pr_min_area A] [--pr_connectivity 4|8] [--pr_opened yes] also sweeps a threshold over the
stitched probability of class C instead of judging the arg-max map at one operating point - the reference's second protocol
(matrics_AA_recall): at every level (all 255 bytes, or --pr_thresholds as probabilities in (0, 1] or bytes 1..255) the probability
is binarised, the connected regions of fewer than A pixels are removed and left out of the count (an area opening; A = 1: none),
and class-map bytes >= --num_classes are counted nowhere.  One opened map and one histogram per scene, built on the GPU
(scenes.host_area_open, scenes.host_sweep_hist), give every level at once.  Per scene and summed, a table of threshold, recall,
precision, F1 and alarm area at up to ten evenly spaced levels and the average precision are printed; `pr_hist_<name>.npy` (int64
2 x 2 x 256), `pr_curve.npy` (float64 9 x T of the sum: level, tp, fp, fn, removed, recall, precision, f1, alarm area) and, with
--pr_opened yes, `pr_opened_<name>.npy` (uint8 H x W) are written; the returned dict gains `pr_hist`, `pr_levels`, `pr_scores` and
`average_precision`.  Not together with --scales or --blend.

--instances C [C ...] [--inst_bound 0.5] [--inst_dist 0] [--inst_min_seed 8] [--inst_radius 4] [--inst_connectivity 4|8]
[--inst_map yes] also counts and scores OBJECTS of the classes C (buildings, cars): a row of touching cars predicted as one blob is
almost perfect per pixel and one object instead of five.  Seeds are the pixels of the finished (sieved) map of those classes whose
predicted boundary probability is below --inst_bound and whose distance-map value is at least --inst_dist (probabilities in 0..1,
quantised as the head maps are; --inst_bound 1.0 and --inst_dist 0 switch the tests off, which a single-task model, --scales and
--blend need); seed regions of at least --inst_min_seed pixels are numbered and grown back over their class within --inst_radius
pixels (0..16), all on the GPU (scenes.host_seed_map, scenes.host_instances).  The true objects are the connected regions of the
same classes of the class map; a predicted object is a true positive at an IoU threshold t if it and a true object of its class
overlap with IoU > t (scenes.host_instance_match, scenes.instance_scores).  Per class the predicted and true object counts, the
object precision, recall and F1 at IoU 0.5 and the mean F1 over 0.5:0.05:0.95 are printed, summed over the scenes;
`instances_<name>.npy` (int32 n x 8: root, class, area, seed_area, i_min, j_min, i_max, j_max), `instance_scores.npy` (float64
C x 6: n_pred, n_true, precision, recall, F1 at 0.5, mean F1) and, with --inst_map yes, `inst_map_<name>.npy` (int32 H x W, -1
off the objects) are written; the returned dict gains `instance_scores` and `instance_counts`.

--inst_flood yes [--inst_flood_rounds J] [--inst_flood_floor F] [--inst_flood_drain D], with --instances, floods the grown objects of
the prediction over the rest of their class before they are matched, traced and written: a bounded watershed on the GPU
(scenes.host_flood) that lets the distance map's levels 255 .. F down one by one, J rounds each, and D rounds more at the last
level; in a round a pixel of the class that has reached the level joins the smallest object beside it.  The height is the
predicted distance map on a multitask model without --scales and --blend, and absent elsewhere (a geodesic grow).  F is a
probability in 0..1, quantised as the head maps are.  Buildings need it: a seed threshold high enough to split two touching
buildings leaves cores that --inst_radius cannot grow back to the outline.  Per scene the settled pixels are printed, and a warning
where the last round still settled some (the schedule may have cut the flood short); the returned dict gains `flood_settled`.

--polygons yes [--poly_simplify T] [--poly_min_area A] [--poly_truth yes], with --instances, also writes the objects as a vector
layer: the predicted instance map is traced on the GPU into closed rings of pixel corners, outer rings and holes
(scenes.host_outlines; only rings and vertices leave the GPU), every hole is given to the ring round it (scenes.outline_polygons),
polygons of fewer than A pixels are dropped, every ring is simplified with Douglas-Peucker at a tolerance of T pixels (default 0:
the exact pixel outline; neighbouring polygons are simplified independently and may then overlap by up to T), and
`polygons_<name>.geojson` is written: a FeatureCollection of Polygon features with the properties id, class and area, in pixel
coordinates (x, -y), exteriors counter-clockwise (RFC 7946).  --poly_truth yes writes the true objects alike, as
`polygons_true_<name>.geojson`.  The polygon and hole counts per class are printed; the returned dict gains `polygon_counts`
(int64 C x 2).

--head_maps HEAD [HEAD ...] also writes whole-scene maps of the named heads (`seg`, `bound`, `dist`, `color`, `color_rgb`; what
test_ISPRS.py:285-414 displays per patch): `pred_<head>_<name>.npy`, uint8 H x W x Ch - the head's output averaged over the views,
times 255, rounded (scenes.host_stitch_maps), stitched on the GPU by the same windows and ownership as the class map.  `color_rgb`
is the colour head's HSV turned into an RGB picture; it is also written as `pred_color_rgb_<name>.ppm`, and its mean absolute
difference from the scene image is printed.  The returned dict gains `head_maps` (per scene {head: map}) and `color_mae`.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

from test_ISPRS import LABEL_DICT, build_parser as _patch_parser, convert_preds2rgb


def metrics_from_confusion(cm):
    """compute_metrics_hw from a C x C confusion matrix [true][pred]: accuracy and per-class F1 / recall / precision in percent,
    (accuracy, f1score, recall, precision).  A class without support (or never predicted) gives 0, sklearn's default apart from its
    warning; unlike sklearn, which drops a class that occurs in neither array, the vectors always have C entries."""
    cm = np.asarray(cm, np.float64)
    if cm.ndim != 2 or cm.shape[0] != cm.shape[1]:
        raise ValueError(f"a confusion matrix is C x C, got {cm.shape}")
    tp, support, predicted, total = np.diag(cm), cm.sum(1), cm.sum(0), cm.sum()
    ratio = lambda num, den: np.divide(num, den, out=np.zeros_like(num), where=den > 0)
    accuracy = 100 * float(tp.sum() / total) if total > 0 else 0.0
    return accuracy, 100 * ratio(2 * tp, support + predicted), 100 * ratio(tp, support), 100 * ratio(tp, predicted)


def _yes(v):
    s = str(v).lower()
    if s in ("yes", "true", "t", "y", "1"):
        return True
    if s in ("no", "false", "f", "n", "0"):
        return False
    raise argparse.ArgumentTypeError("Boolean value expected.")


def build_parser():
    parser = _patch_parser()                                   # test_ISPRS.py's flags; --dataset_path is the scene directory
    parser.add_argument("--scene_dataset", type=_yes, default=True, help="as train_ISPRS.py names the layout; this script reads no other")
    parser.add_argument("--stride", type=int, default=None, help="distance between windows (default: the patch size)")
    parser.add_argument("--weights", choices=["model", "ema"], default="model",
                        help="model: the trained weights; ema: their moving average (a file saved by train_ISPRS.py --ema yes)")
    parser.add_argument("--views", nargs="+", default=["none"], metavar="SET|CODE",
                        help="test-time augmentation: none, flips, aug5, all, or symmetry codes 0..7 (e.g. --views 0 3 4)")
    parser.add_argument("--scales", nargs="+", type=float, default=None, metavar="Z",
                        help="multi-scale test-time augmentation: 1 to 8 distinct zooms, e.g. --scales 0.75 1 1.5 (default: the scene's own scale only)")
    parser.add_argument("--blend", choices=["linear"], default=None,
                        help="blend overlapping windows under a linear taper instead of cutting between them (--stride then defaults to half the patch)")
    parser.add_argument("--erode_boundary", type=int, default=0, metavar="R",
                        help="also score on the ground truth eroded by a disc of radius R (0..16; the ISPRS benchmark uses 3); 0: off")
    parser.add_argument("--boundary_f1", type=int, default=None, metavar="R",
                        help="also print the boundary F1 (BF score) with a tolerance of R pixels (0..16; 0: exact coincidence); default: off")
    parser.add_argument("--sieve", type=int, default=None, metavar="N",
                        help="remove connected regions of fewer than N pixels from the class map before it is scored; default: off")
    parser.add_argument("--sieve_mode", choices=["fill", "void"], default="fill",
                        help="fill: a removed region takes the class most of its kept 4-neighbours have; void: it becomes 255 and leaves every score")
    parser.add_argument("--sieve_connectivity", type=int, default=4, metavar="4|8", help="what connects the pixels of a region: 4- or 8-neighbours")
    parser.add_argument("--sieve_classes", nargs="+", type=int, default=None, metavar="c", help="sieve only regions of these classes (default: all)")
    parser.add_argument("--sieve_rounds", type=int, default=1, metavar="R", help="apply the sieve R times (1..4): a second round removes speckle nested in speckle")
    parser.add_argument("--pr_curve", type=int, default=None, metavar="C",
                        help="also sweep a threshold over the probability of class C: recall, precision, F1, alarm area, average precision; default: off")
    parser.add_argument("--pr_thresholds", nargs="+", type=float, default=None, metavar="T",
                        help="the thresholds of --pr_curve: probabilities in (0, 1], or bytes 1..255 (default: all 255 bytes)")
    parser.add_argument("--pr_min_area", type=int, default=1, metavar="A", help="area opening of every binarised map: regions below A pixels leave the count")
    parser.add_argument("--pr_connectivity", type=int, default=4, metavar="4|8", help="what connects the pixels of a region: 4- or 8-neighbours")
    parser.add_argument("--pr_opened", type=_yes, default=False, help="also write the opened map of every scene")
    parser.add_argument("--instances", nargs="+", type=int, default=None, metavar="C",
                        help="also count and score the objects of these classes (seeds off the predicted boundaries, grown back); default: off")
    parser.add_argument("--inst_bound", type=float, default=0.5, metavar="P", help="a seed pixel's boundary probability lies below P (1.0: no test)")
    parser.add_argument("--inst_dist", type=float, default=0.0, metavar="P", help="a seed pixel's distance-map value is at least P (0: no test)")
    parser.add_argument("--inst_min_seed", type=int, default=8, metavar="N", help="seed regions of fewer than N pixels are no objects")
    parser.add_argument("--inst_radius", type=int, default=4, metavar="R", help="seeds are grown back over their class within R pixels (0..16)")
    parser.add_argument("--inst_connectivity", type=int, default=4, metavar="4|8", help="what connects the pixels of a seed: 4- or 8-neighbours")
    parser.add_argument("--inst_map", type=_yes, default=False, help="also write the instance map of every scene")
    parser.add_argument("--inst_flood", type=_yes, default=False, help="with --instances: flood the grown objects over their class, down the distance map")
    parser.add_argument("--inst_flood_rounds", type=int, default=1, metavar="J", help="rounds per level of the flood (1..16)")
    parser.add_argument("--inst_flood_floor", type=float, default=0.0, metavar="F", help="the lowest distance-map value the flood lets down (0..1)")
    parser.add_argument("--inst_flood_drain", type=int, default=0, metavar="D", help="further rounds at the lowest level (0..4096)")
    parser.add_argument("--polygons", type=_yes, default=False, help="with --instances: also write the objects of every scene as GeoJSON polygons")
    parser.add_argument("--poly_simplify", type=float, default=0.0, metavar="T", help="Douglas-Peucker tolerance in pixels for every ring (0: the exact outline)")
    parser.add_argument("--poly_min_area", type=int, default=0, metavar="A", help="polygons of fewer than A pixels are left out")
    parser.add_argument("--poly_truth", type=_yes, default=False, help="also write the polygons of the true objects")
    parser.add_argument("--head_maps", nargs="+", default=[], metavar="HEAD",
                        help="also write uint8 whole-scene maps of these heads: seg, bound, dist, color, color_rgb (default: none)")
    return parser


def parse_views(words):
    """--views' words as a tuple of codes: one set name, or codes separated by blanks or commas."""
    from resunet_a_mltsk_keras_amd import scenes
    words = [w for word in words for w in str(word).split(",") if w]
    if len(words) == 1 and words[0] in scenes.VIEW_SETS:
        return scenes.check_views(words[0])
    if not words or not all(w.isdigit() for w in words):
        raise SystemExit(f"--views {' '.join(words)}: one of {', '.join(scenes.VIEW_SETS)}, or symmetry codes 0..7")
    try:
        return scenes.check_views(tuple(int(w) for w in words))
    except ValueError as exc:
        raise SystemExit(f"--views: {exc}") from None


def parse_scales(zooms, patch, head_maps=()):
    """--scales' zooms as a tuple (None: absent), refused together with --head_maps and for what scenes.check_scales refuses."""
    from resunet_a_mltsk_keras_amd import scenes
    if zooms is None:
        return None
    if head_maps:
        raise SystemExit("--scales and --head_maps exclude each other: multi-scale maps of the other heads are not built")
    try:
        scenes.check_scales(tuple(zooms), patch)
    except ValueError as exc:
        raise SystemExit(f"--scales: {exc}") from None
    return tuple(zooms)


def parse_sweep(args):
    """--pr_curve and its companions as predict_scene's `sweep` dict (None: absent); thresholds above 1 are bytes."""
    from resunet_a_mltsk_keras_amd import scenes
    if args.pr_curve is None:
        return None
    if args.scales is not None or args.blend is not None:
        raise SystemExit("--pr_curve excludes --scales and --blend: the probabilities then live in an int32 accumulator, no maps of the heads are built")
    thr = args.pr_thresholds
    if thr is not None:
        thr = [int(t) if t > 1 and float(t).is_integer() else float(t) for t in thr]
    sweep = dict(positive=args.pr_curve, thresholds=thr, min_area=args.pr_min_area, connectivity=args.pr_connectivity, opened=bool(args.pr_opened))
    try:
        scenes.sweep_params(sweep, args.num_classes)
    except ValueError as exc:
        raise SystemExit(f"--pr_curve: {exc}") from None
    return sweep


def parse_instances(args):
    """--instances and its companions as predict_scene's `instances` dict (None: absent); a bound of 1.0 switches that test off."""
    from resunet_a_mltsk_keras_amd import scenes
    if args.instances is None:
        if args.polygons:
            raise SystemExit("--polygons needs --instances: the polygons are the outlines of its objects")
        if args.inst_flood:
            raise SystemExit("--inst_flood needs --instances: the flood grows its objects")
        return None
    if args.polygons and (not args.poly_simplify >= 0 or args.poly_min_area < 0):
        raise SystemExit(f"--polygons: --poly_simplify {args.poly_simplify:g} and --poly_min_area {args.poly_min_area} must not be negative")
    inst = dict(classes=args.instances, bound_below=256 if args.inst_bound == 1.0 else float(args.inst_bound), dist_at_least=float(args.inst_dist),
                min_seed=args.inst_min_seed, radius=args.inst_radius, connectivity=args.inst_connectivity, map=bool(args.inst_map))
    if args.inst_flood:
        inst["flood"] = dict(rounds_per_level=args.inst_flood_rounds, floor=float(args.inst_flood_floor), drain=args.inst_flood_drain)
    try:
        p = scenes.instance_params(inst, args.num_classes)
    except ValueError as exc:
        raise SystemExit(f"--instances: {exc}") from None
    if (p["bound_below"] < 256 or p["dist_at_least"] > 0) and (args.scales is not None or args.blend is not None):
        raise SystemExit("--instances with --inst_bound below 1 or --inst_dist above 0 excludes --scales and --blend: no maps of the heads are built there")
    if args.polygons:
        inst["outlines"] = True
    return inst


def write_polygons(path, outlines, table, args, counts):
    """One GeoJSON layer from a (rings, verts) pair and its instance table; counts int64 [C][2] gains the polygons and holes per class."""
    from resunet_a_mltsk_keras_amd import scenes
    polys = scenes.outline_polygons(outlines[0], outlines[1], table, args.poly_min_area)
    for p in polys:
        p["exterior"] = scenes.simplify_ring(p["exterior"], args.poly_simplify)
        p["holes"] = [scenes.simplify_ring(h, args.poly_simplify) for h in p["holes"]]
        counts[p["class"]] += (1, len(p["holes"]))
    scenes.write_geojson(path, polys)


def print_curve(title, scores):
    """threshold / recall / precision / F1 / alarm area at up to ten evenly spaced levels of the curve, and the average precision"""
    n = len(scores["levels"])
    rows = sorted(set(np.rint(np.linspace(0, n - 1, min(n, 10))).astype(int).tolist()))
    print(f'{title}: average precision {scores["average_precision"]:.6f}')
    print('  threshold   recall  precision       F1  alarm area')
    for k in rows:
        print(f'  {int(scores["levels"][k]):3d} ({int(scores["levels"][k]) / 255:.3f}) {scores["recall"][k]:8.4f} {scores["precision"][k]:10.4f} '
              f'{scores["f1"][k]:8.4f} {scores["alarm_area"][k]:11.6f}')


def write_ppm(path, rgb):
    h, w = rgb.shape[:2]
    with open(path, 'wb') as f:                                                               # dependency-free image
        f.write(f"P6\n{w} {h}\n255\n".encode() + np.ascontiguousarray(rgb, dtype=np.uint8).tobytes())


def main(argv=None):
    args = build_parser().parse_args(argv)
    from resunet_a_mltsk_keras_amd import scenes
    from resunet_a_mltsk_keras_amd.keras_api import load_model
    if not args.scene_dataset:
        raise SystemExit("--scene_dataset no: test_ISPRS.py evaluates Image_Test.npy / Reference_Test.npy")
    if args.norm_type not in (1, 2):
        raise SystemExit("scenes are normalised on the GPU: --norm_type 1 or 2")
    try:
        boundary = scenes.check_tolerance(args.boundary_f1)
    except ValueError as exc:
        raise SystemExit(f"--boundary_f1: {exc}") from None
    sieve = None
    if args.sieve is not None:
        sieve = dict(min_area=args.sieve, mode=args.sieve_mode, connectivity=args.sieve_connectivity, classes=args.sieve_classes, rounds=args.sieve_rounds)
        try:
            scenes.sieve_params(sieve, args.num_classes)
        except ValueError as exc:
            raise SystemExit(f"--sieve: {exc}") from None
    sweep = parse_sweep(args)
    instances = parse_instances(args)
    heads = tuple(args.head_maps)
    scales = parse_scales(args.scales, args.patch_size, heads)
    if args.blend is not None and heads:
        raise SystemExit("--blend and --head_maps exclude each other: blended maps of the other heads are not built")
    for k, h in enumerate(heads):
        if h not in scenes.MAP_HEADS or h in heads[:k]:
            raise SystemExit(f"--head_maps {' '.join(heads)}: distinct names out of {', '.join(scenes.MAP_HEADS)}")
    if "color_rgb" in heads and args.norm_type != 1:
        raise SystemExit("--head_maps color_rgb needs --norm_type 1 (the colour target is HSV / (179, 255, 255) only there)")
    names, images, class_maps = scenes.load_scene_dir(args.dataset_path)
    try:
        model = load_model(args.model_path, compile=False, weights=args.weights)
    except ValueError as exc:
        if args.weights != "ema":
            raise
        raise SystemExit(f"--weights ema: {exc}")
    model.summary()
    if model.cfg.num_classes != args.num_classes:
        raise SystemExit(f"--num_classes {args.num_classes}, but the model predicts {model.cfg.num_classes} classes")
    pool = scenes.ScenePool(images, class_maps, patch=args.patch_size)
    views = parse_views(args.views)
    try:
        erode = scenes.check_radius(args.erode_boundary)
    except ValueError as exc:
        raise SystemExit(f"--erode_boundary: {exc}") from None
    if heads and not (model.cfg.multitasking or heads == ("seg",)):
        raise SystemExit(f"--head_maps {' '.join(heads)}: a single-task model has only the seg head")
    if instances is not None and not model.cfg.multitasking and (instances["bound_below"] != 256 or instances["dist_at_least"] > 0):
        raise SystemExit("--instances: a single-task model has no boundary and distance heads; give --inst_bound 1 --inst_dist 0")
    os.makedirs(args.output_path, exist_ok=True)
    lut = {k: v for k, v in LABEL_DICT.items() if v < args.num_classes}
    for extra in range(len(lut), args.num_classes):                                              # classes beyond the ISPRS colours: greys
        lut[str((40 * extra % 256,) * 3)] = extra
    if sieve is not None and args.sieve_mode == "void":
        lut[str((0, 0, 0))] = 255                                                                # the removed regions: black in the .ppm
    total = np.zeros((args.num_classes, args.num_classes), np.int64)
    total_eroded = np.zeros_like(total)
    total_boundary = np.zeros((args.num_classes, 4), np.int64)
    total_raw, total_regions, total_changed = np.zeros_like(total), np.zeros((args.num_classes, 3), np.int64), 0
    all_head_maps, mae_sum, mae_n = [], 0.0, 0
    total_hist = np.zeros((2, 2, 256), np.int64)
    object_scores, flood_settled = [], 0
    polygon_counts, polygon_counts_true = (np.zeros((args.num_classes, 2), np.int64) for _ in range(2))
    print('=' * 40)
    print('[TEST]')
    print(f'views: {" ".join(str(c) for c in views)} ({len(views)} per window)')
    if scales is not None:
        print(f'scales: {" ".join(f"{z:g}" for z in scales)} ({len(scales)} passes per view)')
        for name, shape in zip(names, pool.shapes):
            try:
                scenes.check_scales(scales, args.patch_size, shape)
            except ValueError as exc:
                raise SystemExit(f"--scales: scene {name}: {exc}") from None
    if args.blend is not None:
        print(f'blend: {args.blend}')
        with open(os.path.join(args.output_path, 'eval_settings.json'), 'w') as f:
            json.dump({"views": list(views), "scales": None if scales is None else list(scales), "stride": args.stride, "blend": args.blend}, f)
    for s, name in enumerate(names):
        pred, cm, *more = model.predict_scene(pool, s, stride=args.stride, batch=max(1, args.batch_size), norm_type=args.norm_type, views=views,
                                              erode=erode, heads=heads, boundary=boundary, scales=scales, blend=args.blend, sieve=sieve, sweep=sweep,
                                              instances=instances)
        head_maps = more.pop() if heads else {}
        if instances is not None:
            objects = more.pop()
            np.save(os.path.join(args.output_path, f'instances_{name}.npy'), objects["table"])
            if "inst" in objects:
                np.save(os.path.join(args.output_path, f'inst_map_{name}.npy'), objects["inst"])
            object_scores.append(objects["scores"])
            if args.polygons:
                write_polygons(os.path.join(args.output_path, f'polygons_{name}.geojson'), objects["outlines"], objects["table"], args, polygon_counts)
                if args.poly_truth and objects["outlines_true"] is not None:
                    write_polygons(os.path.join(args.output_path, f'polygons_true_{name}.geojson'), objects["outlines_true"], objects["gt_table"], args,
                                   polygon_counts_true)
            print(f'scene {name}: {objects["n"]} predicted objects, {objects["gt_n"]} true objects, {objects["ungrown"]} pixels of the classes outside every object')
            if "flood" in objects:
                fl = objects["flood"]
                flood_settled += fl["settled"]
                cut = ' - the last round still settled pixels: the schedule may have cut the flood short' if fl["last_round"] == fl["rounds"] else ''
                print(f'scene {name}: the flood settled {fl["settled"]} pixels ({"down the distance map" if fl["height"] else "without a height"}, '
                      f'last round {fl["last_round"]} of {fl["rounds"]}){cut}')
        if sweep is not None:
            swept = more.pop()
            total_hist += swept["hist"]
            np.save(os.path.join(args.output_path, f'pr_hist_{name}.npy'), swept["hist"])
            if swept["opened"] is not None:
                np.save(os.path.join(args.output_path, f'pr_opened_{name}.npy'), swept["opened"])
            print_curve(f'scene {name}: class {args.pr_curve}, min_area {args.pr_min_area}', scenes.sweep_scores(swept["hist"], swept["levels"]))
        if sieve is not None:
            report = more.pop()
            total_raw += report["confusion_raw"]
            total_regions += report["counts"]
            total_changed += report["changed"]
            np.save(os.path.join(args.output_path, f'region_counts_{name}.npy'), report["counts"])
            print(f'scene {name}: regions per class (all, below {args.sieve} px, their pixels) {report["counts"].tolist()}, {report["changed"]} pixels changed')
        if boundary is not None:
            counts = more.pop()
            total_boundary += counts
            np.save(os.path.join(args.output_path, f'boundary_counts_{name}.npy'), counts)
        total += cm
        print(f'scene {name}: {pred.shape[0]} x {pred.shape[1]}, accuracy {metrics_from_confusion(cm)[0]:.4f}')
        np.save(os.path.join(args.output_path, f'pred_seg_reconstructed_{name}.npy'), pred)
        write_ppm(os.path.join(args.output_path, f'pred_seg_reconstructed_{name}.ppm'), convert_preds2rgb(pred, lut))
        np.save(os.path.join(args.output_path, f'confusion_matrix_{name}.npy'), cm)
        if erode:
            total_eroded += more[0]
            np.save(os.path.join(args.output_path, f'confusion_matrix_eroded_{name}.npy'), more[0])
        for h, m in head_maps.items():
            np.save(os.path.join(args.output_path, f'pred_{h}_{name}.npy'), m)
        if "color_rgb" in head_maps:
            rgb = head_maps["color_rgb"]
            write_ppm(os.path.join(args.output_path, f'pred_color_rgb_{name}.ppm'), rgb)
            diff = np.abs(rgb.astype(np.int16) - images[s][..., :3].astype(np.int16))
            mae_sum, mae_n = mae_sum + float(diff.sum()), mae_n + diff.size
            print(f'scene {name}: colour reconstruction, mean absolute difference from the image {diff.mean():.4f}')
        if heads:
            all_head_maps.append(head_maps)
    metrics = metrics_from_confusion(total)
    print('Confusion  matrix \n', total)
    print()
    print('Accuracy: ', metrics[0])
    print('F1score: ', metrics[1])
    print('Recall: ', metrics[2])
    print('Precision: ', metrics[3])
    res = {"accuracy": metrics[0], "f1": metrics[1], "recall": metrics[2], "precision": metrics[3], "confusion_matrix": total}
    if args.blend is not None:
        res["blend"] = args.blend
    if sieve is not None:
        m = metrics_from_confusion(total_raw)
        print()
        print(f'Before the sieve (--sieve {args.sieve}, {args.sieve_mode}: {total_changed} pixels changed)')
        print('Region counts (regions, small regions, their pixels) \n', total_regions)
        print('Confusion  matrix \n', total_raw)
        print()
        print('Accuracy: ', m[0])
        print('F1score: ', m[1])
        print('Recall: ', m[2])
        print('Precision: ', m[3])
        res.update(confusion_matrix_raw=total_raw, region_counts=total_regions, sieve_changed=total_changed)
    if erode:
        m = metrics_from_confusion(total_eroded)
        print()
        print(f'Eroded ground truth (radius {erode})')
        print('Confusion  matrix \n', total_eroded)
        print()
        print('Accuracy: ', m[0])
        print('F1score: ', m[1])
        print('Recall: ', m[2])
        print('Precision: ', m[3])
        res.update(confusion_matrix_eroded=total_eroded, accuracy_eroded=m[0], f1_eroded=m[1], recall_eroded=m[2], precision_eroded=m[3])
    if boundary is not None:
        b = scenes.boundary_scores(total_boundary)
        print()
        print(f'Boundary F1 (tolerance {boundary} px)')
        print('Boundary counts (n_pred, m_pred, n_true, m_true) \n', total_boundary)
        print()
        print('Precision: ', b["precision"])
        print('Recall: ', b["recall"])
        print('F1score: ', b["f1"])
        print('Mean F1score: ', b["f1_mean"])
        res.update(boundary_counts=total_boundary, boundary_precision=b["precision"], boundary_recall=b["recall"], boundary_f1=b["f1"],
                   boundary_f1_mean=b["f1_mean"])
    if sweep is not None:
        sc = scenes.sweep_scores(total_hist, swept["levels"])
        print()
        print_curve(f'Precision-recall sweep of class {args.pr_curve} (min_area {args.pr_min_area}, connectivity {args.pr_connectivity}, {len(sc["levels"])} levels)', sc)
        np.save(os.path.join(args.output_path, 'pr_curve.npy'),
                np.stack([np.asarray(sc[k], np.float64) for k in ("levels", "tp", "fp", "fn", "removed", "recall", "precision", "f1", "alarm_area")]))
        res.update(pr_hist=total_hist, pr_levels=sc["levels"], pr_scores=sc, average_precision=sc["average_precision"])
    if instances is not None:
        sc = scenes.sum_instance_scores(object_scores)
        at50 = int(np.flatnonzero(sc["iou_percent"] == 50)[0])
        print()
        print(f'Objects of the classes {" ".join(str(c) for c in args.instances)} (seeds: boundary below {args.inst_bound:g}, distance at least {args.inst_dist:g}, '
              f'{args.inst_min_seed} px; grown {args.inst_radius} px)')
        print('  class  predicted     true  precision   recall       F1  mean F1 (IoU 0.5:0.05:0.95)')
        table = np.stack([sc["n_pred"].astype(np.float64), sc["n_true"].astype(np.float64), sc["precision"][:, at50], sc["recall"][:, at50],
                          sc["f1_50"], sc["f1_mean"]], 1)
        for c in sorted(set(args.instances)):
            print(f'  {c:5d} {int(table[c, 0]):10d} {int(table[c, 1]):8d} {table[c, 2]:10.4f} {table[c, 3]:8.4f} {table[c, 4]:8.4f} {table[c, 5]:8.4f}')
        np.save(os.path.join(args.output_path, 'instance_scores.npy'), table)
        res.update(instance_scores=sc, instance_counts=np.stack([sc["n_pred"], sc["n_true"]], 1))
        if args.inst_flood:
            res["flood_settled"] = flood_settled
        if args.polygons:
            print()
            print(f'Polygons (simplified at {args.poly_simplify:g} px, at least {args.poly_min_area} px)' + (', predicted / true' if args.poly_truth else ''))
            print('  class   polygons      holes')
            for c in sorted(set(args.instances)):
                true = f'   / {polygon_counts_true[c, 0]:8d} {polygon_counts_true[c, 1]:10d}' if args.poly_truth else ''
                print(f'  {c:5d} {polygon_counts[c, 0]:10d} {polygon_counts[c, 1]:10d}{true}')
            res["polygon_counts"] = polygon_counts
    if heads:
        res["head_maps"] = all_head_maps
        res["color_mae"] = mae_sum / mae_n if mae_n else None
        if mae_n:
            print()
            print('Colour reconstruction, mean absolute difference: ', res["color_mae"])
    return res


if __name__ == "__main__":
    main(sys.argv[1:])
