"""Host side of the eroded ground truth (scenes.py: host_erode, host_erode_confusion, check_radius, ScenePool.eroded_maps on a cpu
pool; eval_scenes_ISPRS.py: --erode_boundary): the numpy definition against scipy's binary erosion per value, against the same scan
over an edge-replicated pad and against the O(radius) form the kernel uses, the lattice disc a single pixel erodes, the scene border,
and the confusion matrix on the eroded map.  Everything is bytes and integers: every comparison is exact."""
import os
import sys

import numpy as np
import pytest

from resunet_a_mltsk_keras_amd import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = [(1, 1), (1, 300), (300, 1), (5, 300), (67, 45), (130, 257)]
RADII = [0, 1, 2, 3, 7, 16]
C = 5


def blocky(seed, H, W, C=C, region=16):
    """Uniform region x region blocks of classes 0..C-1 with a sprinkle of 255 and of the value C (both "no class")."""
    rng = np.random.default_rng(seed)
    f = rng.integers(0, C, (H // region + 1, W // region + 1)).astype(np.uint8)
    m = np.ascontiguousarray(np.kron(f, np.ones((region, region), np.uint8))[:H, :W])
    m[rng.random(m.shape) < 0.003] = 255
    m[rng.random(m.shape) < 0.003] = C
    return m


def disc(r):
    yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
    return yy * yy + xx * xx <= r * r


def scipy_erode(cm, r):
    """A pixel keeps its value v iff the binary erosion of (cm == v) by the disc keeps it, the outside counting as v."""
    from scipy import ndimage
    out = np.full(cm.shape, 255, np.uint8)
    for v in np.unique(cm):
        out[ndimage.binary_erosion(cm == v, structure=disc(r), border_value=1)] = v
    return out


def pad_erode(cm, r):
    """The same scan over np.pad(mode="edge"): clamping a coordinate moves an offset towards the centre, so it stays in the disc."""
    H, W = cm.shape
    p = np.pad(cm, r, mode="edge")
    er = np.zeros(cm.shape, bool)
    for dy, dx in np.argwhere(disc(r)) - r:
        er |= p[r + dy:r + dy + H, r + dx:r + dx + W] != cm
    out = cm.copy()
    out[er] = 255
    return out


def rows_erode(cm, r):
    """The O(radius) form: hd(i, j) the distance along row i to the nearest other value; (i, j) erodes iff for some |dy| <= r, rows
    clamped, cm[i + dy, j] != cm[i, j] or hd(i + dy, j)^2 <= r^2 - dy^2."""
    H, W = cm.shape
    hd = np.full((H, W), 255, np.int64)
    for d in range(min(r, W - 1), 0, -1):
        near = np.zeros((H, W), bool)
        near[:, d:] |= cm[:, d:] != cm[:, :-d]
        near[:, :-d] |= cm[:, :-d] != cm[:, d:]
        hd[near] = d
    er = np.zeros((H, W), bool)
    for dy in range(-r, r + 1):
        at = np.clip(np.arange(H) + dy, 0, H - 1)
        er |= (cm[at] != cm) | (hd[at] ** 2 <= r * r - dy * dy)
    out = cm.copy()
    out[er] = 255
    return out


@pytest.mark.parametrize("r", RADII)
@pytest.mark.parametrize("shape", SHAPES)
def test_host_erode_is_the_erosion_per_value(shape, r):
    cm = blocky(shape[0] * 1000 + shape[1], *shape)
    got = scenes.host_erode(cm, r)
    assert got.dtype == np.uint8 and got.shape == cm.shape
    assert np.array_equal(got, scipy_erode(cm, r))
    assert np.array_equal(got, pad_erode(cm, r))
    assert np.array_equal(got, rows_erode(cm, r))
    assert ((got == cm) | (got == 255)).all()
    if r == 0:
        assert np.array_equal(got, cm)


def test_maps_smaller_than_the_radius():
    for shape in [(1, 1), (2, 3), (5, 4), (9, 2)]:
        assert max(shape) < 16
        cm = np.random.default_rng(shape[0]).integers(0, 3, shape).astype(np.uint8)
        for r in (7, 16):
            assert np.array_equal(scenes.host_erode(cm, r), scipy_erode(cm, r))
    two = np.array([[1, 1], [1, 2]], np.uint8)
    assert (scenes.host_erode(two, 16) == 255).all() and np.array_equal(scenes.host_erode(two[:1], 16), two[:1])


def test_one_pixel_erodes_the_lattice_disc():
    cm = np.full((41, 41), 2, np.uint8)
    cm[20, 20] = 4
    got = scenes.host_erode(cm, 3)
    assert int((got == 255).sum()) == 29
    assert np.array_equal(got == 255, np.pad(disc(3), 17))
    for dy, dx, eroded in [(3, 0, True), (2, 2, True), (3, 1, False), (1, 3, False), (-3, 0, True), (0, -3, True), (-2, -2, True)]:
        assert (got[20 + dy, 20 + dx] == 255) == eroded, (dy, dx)
    assert got[20, 20] == 255                                   # the odd pixel has other values all around it
    for r in RADII:
        assert int((scenes.host_erode(cm, r) == 255).sum()) == (int(disc(r).sum()) if r else 0)


@pytest.mark.parametrize("value", [0, 4, 5, 255])
def test_a_uniform_map_comes_back_unchanged(value):
    for shape in [(1, 1), (7, 40), (41, 41)]:
        cm = np.full(shape, value, np.uint8)
        for r in RADII:
            assert np.array_equal(scenes.host_erode(cm, r), cm)


def test_a_class_edge_in_the_outermost_row_or_column():
    cm = np.zeros((20, 30), np.uint8)
    cm[0, :] = 1                                                # the first row is another class
    got = scenes.host_erode(cm, 3)
    assert (got[:4] == 255).all() and (got[4:] == 0).all()      # rows 0 (its neighbours below) and 1..3; row 4 is 4 > 3 away
    cm = np.zeros((20, 30), np.uint8)
    cm[:, 29] = 3                                               # the last column
    got = scenes.host_erode(cm, 2)
    assert (got[:, 27:] == 255).all() and (got[:, :27] == 0).all()
    cm = np.zeros((20, 30), np.uint8)
    cm[19, 29] = 1                                              # one corner pixel: a quarter disc
    got = scenes.host_erode(cm, 3)
    assert int((got == 255).sum()) == 11 and got[16, 29] == 255 and got[19, 26] == 255 and got[17, 27] == 255 and got[16, 28] == 0


def plain_confusion(cm, pred, C):
    t, p = cm.astype(np.int64), pred.astype(np.int64)
    keep = (t < C) & (p < C)
    return np.bincount(t[keep] * C + p[keep], minlength=C * C).reshape(C, C)


def test_host_erode_confusion():
    rng = np.random.default_rng(3)
    cm = blocky(9, 67, 45)
    pred = rng.integers(0, C + 1, cm.shape).astype(np.uint8)    # the value C: a prediction that is skipped
    pred[rng.random(cm.shape) < 0.01] = 255
    plain = plain_confusion(cm, pred, C)
    got0 = scenes.host_erode_confusion(cm, pred, 0, C)
    assert got0.dtype == np.int64 and got0.shape == (C, C) and np.array_equal(got0, plain)
    assert plain.sum() == int(((cm < C) & (pred < C)).sum()) < cm.size      # pred >= C and t >= C are skipped
    last = plain
    for r in RADII[1:]:
        got = scenes.host_erode_confusion(cm, pred, r, C)
        assert (got <= last).all() and np.array_equal(got, plain_confusion(scenes.host_erode(cm, r), pred, C))
        last = got
    assert 0 < scenes.host_erode_confusion(cm, pred, 3, C).sum() < plain.sum()
    # t >= C: with C = 3 the classes 3 and 4 are no class, and they still erode their neighbours
    small = scenes.host_erode_confusion(cm, np.minimum(pred, 2), 2, 3)
    assert np.array_equal(small, plain_confusion(scenes.host_erode(cm, 2), np.minimum(pred, 2), 3))
    with pytest.raises(ValueError, match="C 0 outside 1..64"):
        scenes.host_erode_confusion(cm, pred, 1, 0)
    with pytest.raises(ValueError, match="C 65 outside 1..64"):
        scenes.host_erode_confusion(cm, pred, 1, 65)
    with pytest.raises(ValueError, match="prediction map"):
        scenes.host_erode_confusion(cm, pred[:-1], 1, C)


def test_check_radius():
    assert scenes.check_radius(0) == 0 and scenes.check_radius(np.int32(16)) == 16
    for bad in (-1, 17, 255):
        with pytest.raises(ValueError, match=f"rua_scene_erode: radius {bad} outside 0..16"):
            scenes.check_radius(bad)
    for bad in (3.0, "3", None, True):
        with pytest.raises(ValueError, match="rua_scene_erode: radius"):
            scenes.check_radius(bad)
    with pytest.raises(ValueError, match="radius 17"):
        scenes.host_erode(np.zeros((4, 4), np.uint8), 17)
    with pytest.raises(ValueError, match="uint8"):
        scenes.host_erode(np.zeros((4, 4), np.int32), 1)


def test_cpu_pool_eroded_maps():
    maps = [blocky(1, 40, 57), blocky(2, 33, 20)]
    images = [np.zeros(m.shape + (1,), np.uint8) for m in maps]
    pool = scenes.ScenePool(images, maps, device="cpu")
    for r in (0, 3):
        got = pool.eroded_maps(r)
        assert len(got) == 2 and all(np.array_equal(g, scenes.host_erode(m, r)) for g, m in zip(got, maps))
    with pytest.raises(ValueError, match="radius 17"):
        pool.eroded_maps(17)
    with pytest.raises(ValueError, match="class maps"):
        scenes.ScenePool(images, None, device="cpu").eroded_maps(3)


def test_cli_knows_erode_boundary():
    import eval_scenes_ISPRS
    parser = eval_scenes_ISPRS.build_parser()
    assert parser.get_default("erode_boundary") == 0
    args = parser.parse_args(["--model_path", "m.h5", "--dataset_path", "d", "--erode_boundary", "3"])
    assert args.erode_boundary == 3
