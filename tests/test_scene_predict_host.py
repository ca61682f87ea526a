"""Host side of whole-scene evaluation: scenes.predict_table (windows that cover a scene, every pixel owned by exactly one),
scenes.host_stitch (the numpy definition of rua_scene_stitch) and eval_scenes_ISPRS.metrics_from_confusion."""
import json
import os

import numpy as np
import pytest

import eval_scenes_ISPRS
import test_ISPRS
from resunet_a_mltsk_keras_amd import scenes

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

CASES = [((96, 160), 32, 32), ((300, 260), 256, 128), ((150, 171), 64, 24), ((150, 171), 64, 64), ((64, 64), 64, 64), ((64, 64), 64, 17),
         ((40, 35), 32, 1)]


@pytest.mark.parametrize("shape,P,S", CASES)
def test_predict_table_owns_every_pixel_once(shape, P, S):
    H, W = shape
    rows, own = scenes.predict_table(shape, P, S)
    assert rows.dtype == np.int32 and own.dtype == np.int32 and rows.shape == own.shape and rows.shape[1] == 4
    assert (rows[:, 0] == 0).all() and (rows[:, 3] == 0).all()
    count = np.zeros(shape, np.int64)
    for (_, r, c, _), (r0, r1, c0, c1) in zip(rows.tolist(), own.tolist()):
        assert 0 <= r and r + P <= H and 0 <= c and c + P <= W                      # the window inside the scene
        assert 0 <= r0 < r1 <= P and 0 <= c0 < c1 <= P                               # the rectangle inside the window, never empty
        count[r + r0:r + r1, c + c0:c + c1] += 1
    assert (count == 1).all()
    # per axis: K = ceil((L - P) / S) + 1 origins min(k S, L - P), row-major, the last one flush with the border
    for L, col in ((H, 1), (W, 2)):
        K = -(-(L - P) // S) + 1
        want = np.minimum(np.arange(K) * S, L - P)
        assert np.array_equal(np.unique(rows[:, col]), np.unique(want)) and rows[:, col].max() == L - P
    KH, KW = -(-(H - P) // S) + 1, -(-(W - P) // S) + 1
    assert len(rows) == KH * KW
    grid = rows.reshape(KH, KW, 4)
    assert (grid[:, :, 1] == grid[:, :1, 1]).all() and (grid[:, :, 2] == grid[:1, :, 2]).all()   # row-major over (row index, col index)
    assert tuple(rows[-1, 1:3]) == (H - P, W - P)
    # the cuts: half way through the overlap of neighbouring windows
    o = np.minimum(np.arange(KW) * S, W - P)
    cuts = [0] + [(o[k] + P + o[k + 1]) // 2 for k in range(KW - 1)] + [W]
    assert [int(c + c0) for (_, _, c, _), (_, _, c0, _) in zip(grid[0].tolist(), own.reshape(KH, KW, 4)[0].tolist())] == cuts[:-1]
    if S == P and H % P == 0 and W % P == 0:
        index = np.arange(H * W).reshape(H, W)
        first = test_ISPRS._tiles(index, P)[:, 0, 0]                                # the scene pixel each reference tile starts at
        assert np.array_equal(rows[:, 1] * W + rows[:, 2], first)
        assert (own == np.array([0, P, 0, P])).all()


def test_predict_table_rectangular_patch():
    assert all(np.array_equal(a, b) for a, b in zip(scenes.predict_table((50, 90), (16, 48), (12, 12)), scenes.predict_table((50, 90), (16, 48), 12)))
    with pytest.raises(ValueError, match="rows: stride 24, patch 16"):
        scenes.predict_table((50, 90), (16, 48), 24)
    rows, own = scenes.predict_table((50, 90), (16, 48), (12, 24))
    assert sorted(set(rows[:, 1].tolist())) == [0, 12, 24, 34] and sorted(set(rows[:, 2].tolist())) == [0, 24, 42]
    count = np.zeros((50, 90), np.int64)
    for (_, r, c, _), (r0, r1, c0, c1) in zip(rows.tolist(), own.tolist()):
        assert r + 16 <= 50 and c + 48 <= 90 and r1 <= 16 and c1 <= 48
        count[r + r0:r + r1, c + c0:c + c1] += 1
    assert (count == 1).all()


@pytest.mark.parametrize("shape,P,S", [((64, 64), 32, 33), ((64, 64), 32, 0), ((64, 64), 32, -4), ((64, 31), 32, 16), ((20, 64), 32, 16)])
def test_predict_table_refuses(shape, P, S):
    with pytest.raises(ValueError, match="stride"):
        scenes.predict_table(shape, P, S)


def test_pool_predict_table_names_its_scene():
    pool = scenes.ScenePool([np.zeros((40, 40, 3), np.uint8), np.zeros((70, 50, 3), np.uint8)], None, patch=32, device="cpu")
    rows, own = pool.predict_table(1, 20)
    want_rows, want_own = scenes.predict_table((70, 50), 32, 20)
    assert (rows[:, 0] == 1).all() and np.array_equal(rows[:, 1:], want_rows[:, 1:]) and np.array_equal(own, want_own)
    assert np.array_equal(pool.predict_table(0)[0], scenes.predict_table((40, 40), 32, 32)[0])       # stride None: the patch
    with pytest.raises(ValueError, match="scene 2"):
        pool.predict_table(2, 20)


def test_host_stitch_by_hand():
    """Two classes, 2 x 2 windows on a 2 x 4 scene: a tie (lowest index wins), a label of 255 (not counted), an empty rectangle (no write)."""
    p = np.array([[[[0.2, 0.8], [0.5, 0.5]],            # window 0 at (0, 0): classes 1, 0 (tie)
                   [[0.9, 0.1], [0.3, 0.7]]],           #                     0, 1
                  [[[0.1, 0.9], [0.1, 0.9]],            # window 1 at (0, 2): owns only its right column: 1 / 0
                   [[0.1, 0.9], [0.6, 0.4]]],
                  [[[0.0, 1.0], [0.0, 1.0]],            # window 2 at (0, 1): owns column 1 of itself = scene column 2
                   [[0.0, 1.0], [1.0, 0.0]]],
                  [[[0.0, 1.0], [0.0, 1.0]],            # window 3 at (0, 0): empty rectangle
                   [[0.0, 1.0], [0.0, 1.0]]]], np.float32)
    rows = np.array([[0, 0, 0, 0], [0, 0, 2, 0], [0, 0, 1, 0], [0, 0, 0, 0]], np.int32)
    own = np.array([[0, 2, 0, 2], [0, 2, 1, 2], [0, 2, 1, 2], [1, 1, 0, 2]], np.int32)
    cls = np.array([[1, 1, 255, 1], [0, 0, 0, 0]], np.uint8)
    maps, cm = scenes.host_stitch(p, rows, own, [(2, 4)], [cls])
    assert maps[0].dtype == np.uint8 and np.array_equal(maps[0], [[1, 0, 1, 1], [0, 1, 0, 0]])
    assert cm.dtype == np.int64 and np.array_equal(cm, [[3, 1], [1, 2]])            # [true][pred]; the 255 pixel is in neither row
    maps, none = scenes.host_stitch(p[:1], rows[:1], own[:1], [(2, 4)], fill=0xEE)
    assert none is None and np.array_equal(maps[0], [[1, 0, 0xEE, 0xEE], [0, 1, 0xEE, 0xEE]])
    for bad_rows, bad_own, msg in [(np.array([[0, 0, 3, 0]]), own[:1], "row 0: window"), (np.array([[1, 0, 0, 0]]), own[:1], "row 0: scene 1"),
                                   (np.array([[0, 0, 0, 2]]), own[:1], "row 0: code 2"), (rows[:1], np.array([[0, 3, 0, 2]]), "row 0: owned rows")]:
        with pytest.raises(ValueError, match=msg):
            scenes.host_stitch(p[:1], bad_rows, bad_own, [(2, 4)])


def test_host_stitch_of_predict_table_is_the_mosaic():
    """With stride == patch on a scene of whole tiles host_stitch is the reference's arg-max + pred_recostruction."""
    rng = np.random.default_rng(0)
    H, W, P, C = 64, 96, 32, 5
    rows, own = scenes.predict_table((H, W), P, P)
    p = rng.random((len(rows), P, P, C), dtype=np.float32)
    cls = rng.integers(0, C, (H, W)).astype(np.uint8)
    maps, cm = scenes.host_stitch(p, rows, own, [(H, W)], [cls])
    mosaic = test_ISPRS.pred_recostruction(P, np.argmax(p, -1), cls)
    assert np.array_equal(maps[0], mosaic.astype(np.uint8))
    want = np.zeros((C, C), np.int64)
    np.add.at(want, (cls.ravel(), maps[0].ravel()), 1)
    assert np.array_equal(cm, want)


# ---- metrics_from_confusion ---------------------------------------------------------------------------------------------------
def test_metrics_from_confusion_reference_runs():
    """The confusion matrices the reference printed, and the accuracy / F1 / recall / precision it printed with them (8 decimals)."""
    with open(os.path.join(GOLDEN, "reference_confusion.json")) as f:
        runs = json.load(f)["runs"]
    assert runs
    for run in runs:
        acc, f1, rec, prec = eval_scenes_ISPRS.metrics_from_confusion(np.array(run["confusion"]))
        assert abs(acc - run["accuracy"]) < 1e-9, run["name"]
        for got, key in ((f1, "f1score"), (rec, "recall"), (prec, "precision")):
            assert np.allclose(got, run[key], rtol=0, atol=1e-8), (run["name"], key)


def test_metrics_from_confusion_by_hand():
    """3 x 3 with an empty class: class 2 has no support and is never predicted -> 0 everywhere, the vectors keep three entries."""
    cm = np.array([[6, 2, 0], [1, 3, 0], [0, 0, 0]])
    acc, f1, rec, prec = eval_scenes_ISPRS.metrics_from_confusion(cm)
    assert acc == pytest.approx(100 * 9 / 12)
    assert np.allclose(rec, [75.0, 75.0, 0.0]) and np.allclose(prec, [100 * 6 / 7, 60.0, 0.0])
    assert np.allclose(f1, [100 * 12 / 15, 100 * 6 / 9, 0.0])
    # a class with support that is never predicted: recall 0, precision 0 (no prediction), F1 0
    acc, f1, rec, prec = eval_scenes_ISPRS.metrics_from_confusion(np.array([[2, 0], [3, 0]]))
    assert acc == pytest.approx(40.0) and np.allclose(rec, [100.0, 0.0]) and np.allclose(prec, [40.0, 0.0]) and np.allclose(f1, [100 * 4 / 7, 0.0])
    assert eval_scenes_ISPRS.metrics_from_confusion(np.zeros((2, 2)))[0] == 0.0
    with pytest.raises(ValueError):
        eval_scenes_ISPRS.metrics_from_confusion(np.zeros((2, 3)))


def test_metrics_from_confusion_against_sklearn():
    pytest.importorskip("sklearn")
    from sklearn.metrics import confusion_matrix
    rng = np.random.default_rng(1)
    C = 5
    true, pred = rng.integers(0, C, 5000), rng.integers(0, C, 5000)
    agree = rng.random(5000) < 0.6
    pred[agree] = true[agree]
    cm = confusion_matrix(true, pred, labels=np.arange(C))
    want = test_ISPRS.compute_metrics_hw(true, pred)
    got = eval_scenes_ISPRS.metrics_from_confusion(cm)
    assert got[0] == pytest.approx(want[0], abs=1e-9)
    for g, w in zip(got[1:], want[1:]):
        assert np.allclose(g, w, rtol=0, atol=1e-9)
