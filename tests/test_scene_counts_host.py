"""Host side of the class counts of scene windows (scenes.py: host_class_counts, class_weights, balance_rows, ScenePool.class_counts
on a cpu pool; train_ISPRS.py: --class_weights / --balance_class / --balance_percent): the numpy definition against a pixel loop,
the weights against the reference's five numbers, the balance test against a restatement of the reference's loop,
rua_scene_class_counts' refusals (no launch: safe without a GPU) and the CLI's."""
import ctypes
import os
import sys

import numpy as np
import pytest

from resunet_a_mltsk_keras_amd import _lib as L
from resunet_a_mltsk_keras_amd import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def loop_counts(class_maps, table, PH, PW, C):
    """counts[n][c] pixel by pixel, in plain Python."""
    out = np.zeros((len(table), C + 1), np.int64)
    for n, (s, r, c, _) in enumerate(np.asarray(table).tolist()):
        for i in range(PH):
            for j in range(PW):
                v = int(class_maps[s][r + i, c + j])
                out[n, v if v < C else C] += 1
    return out


# ---- 1. host_class_counts -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("PH,PW,C", [(5, 5, 3), (4, 7, 5), (6, 6, 1), (3, 8, 64)])
def test_host_class_counts_against_a_pixel_loop(PH, PW, C):
    rng = np.random.default_rng(PH * 100 + PW * 10 + C)
    shapes = [(9, 11), (PH, PW), (12, 8)]                      # the second scene is exactly one patch large
    maps = [rng.integers(0, C + 3, s).astype(np.uint8) for s in shapes]
    maps[0][0, :3] = (C, 255, 0)
    table = np.array([[0, 0, 0, 0], [0, 9 - PH, 11 - PW, 2], [1, 0, 0, 3], [2, 12 - PH, 0, 4], [2, 1, 8 - PW, 0], [0, 2, 1, 0]], np.int32)
    got = scenes.host_class_counts(maps, table, (PH, PW), C)
    assert got.dtype == np.int64 and got.shape == (len(table), C + 1)
    assert np.array_equal(got, loop_counts(maps, table, PH, PW, C))
    assert (got.sum(1) == PH * PW).all()


def test_rows_sum_to_the_patch_and_codes_share_one_row():
    rng = np.random.default_rng(3)
    cm = rng.integers(0, 7, (20, 23)).astype(np.uint8)
    table = np.array([[0, 4, 6, code] for code in range(8)], np.int32)
    got = scenes.host_class_counts([cm], table, 12, 5)
    assert (got.sum(1) == 144).all()
    assert (got == got[0]).all()                               # a symmetry permutes pixels
    # ... and they are the counts of the transformed window the training step sees
    _, cls = scenes.host_windows([np.zeros((20, 23, 1), np.uint8)], [cm], table, 12)
    for k in range(8):
        assert np.array_equal(got[k], np.bincount(np.minimum(cls[k], 5).ravel(), minlength=6))


def test_last_column_catches_c_and_255():
    cm = np.zeros((8, 8), np.uint8)
    cm[0, 0], cm[0, 1], cm[1, 0], cm[7, 7], cm[3, 3] = 4, 255, 3, 200, 5
    got = scenes.host_class_counts([cm], np.array([[0, 0, 0, 0]], np.int32), 8, 4)
    assert got.tolist() == [[59, 0, 0, 1, 4]]                  # 4, 255, 200 and 5 are "no class" at C = 4; 3 is a class
    got = scenes.host_class_counts([cm], np.array([[0, 0, 0, 0]], np.int32), 8, 5)
    assert got.tolist() == [[59, 0, 0, 1, 1, 3]]


def test_check_table_errors_are_reached_through_it():
    maps = [np.zeros((40, 50), np.uint8), np.zeros((64, 33), np.uint8)]
    for row, patch, msg in [([2, 0, 0, 0], 32, "rua_scene_windows: row 1: scene 2 outside 0..1"),
                            ([0, 9, 18, 0], 32, r"row 1: window \(9, 18\) \+ 32 x 32 leaves its 40 x 50 scene"),
                            ([0, 0, 0, 8], 32, "row 1: code 8 outside 0..7"),
                            ([0, 0, 0, 6], (16, 48), r"row 1: code 6 transposes and needs a square patch \(got 16 x 48\)")]:
        with pytest.raises(ValueError, match=msg):
            scenes.host_class_counts(maps, np.array([[0, 0, 0, 0], row], np.int32), patch, 5)
    with pytest.raises(ValueError, match="N 0"):
        scenes.host_class_counts(maps, np.zeros((0, 4), np.int32), 32, 5)
    with pytest.raises(ValueError, match="PH 513"):
        scenes.host_class_counts(maps, np.array([[0, 0, 0, 0]], np.int32), (513, 32), 5)
    for C in (0, 65):
        with pytest.raises(ValueError, match=f"rua_scene_class_counts: C {C} outside 1..64"):
            scenes.host_class_counts(maps, np.array([[0, 0, 0, 0]], np.int32), 32, C)


# ---- 2. class_weights ---------------------------------------------------------------------------------------------------------
def test_class_weights_reproduce_the_reference_numbers():
    """The reference's five weights are 1 / frequency: counts in the proportions 1 / w give them back."""
    import train_ISPRS as cli
    w = np.array(cli.REFERENCE_WCE_WEIGHTS, np.float64)
    assert abs((1.0 / w).sum() - 1.0) < 1e-8
    total = 10 ** 12
    n = np.rint(total / w).astype(np.int64)                    # rounding to whole pixels: 1e-9 relative at most (n >= 2.6e9)
    counts = np.zeros((3, 6), np.int64)
    counts[0, :5] = n // 2
    counts[1, :5] = n - n // 2
    counts[:, 5] = (12345, 0, 99)                              # the >= C column is ignored
    got = scenes.class_weights(counts)
    assert got.dtype == np.float64 and got.shape == (5,)
    assert np.allclose(got, w, rtol=1e-6, atol=0)


def test_class_weights_absent_class_and_all_zero():
    counts = np.array([[30, 0, 10, 7], [30, 0, 10, 0]], np.int64)
    got = scenes.class_weights(counts)
    assert got.tolist() == [80 / 60, 4.0, 4.0]                 # the absent class: the largest weight among the present, not 0 or inf
    assert scenes.class_weights(np.array([[5, 9]], np.int64)).tolist() == [1.0]
    with pytest.raises(ValueError, match="no pixel"):
        scenes.class_weights(np.array([[0, 0, 64], [0, 0, 64]], np.int64))
    with pytest.raises(ValueError, match=r"\[N\]\[C \+ 1\]"):
        scenes.class_weights(np.zeros((4,), np.int64))


# ---- 3. balance_rows ----------------------------------------------------------------------------------------------------------
def reference_balance(percent, patch_size, patches_ref, cls=1):
    """The test of the reference's bal_aug_patches loop (utils.py:383), the class a parameter: indices of the patches it keeps."""
    kept = []
    for i in range(0, len(patches_ref)):
        patch = patches_ref[i]
        class1 = patch[patch == cls]
        if len(class1) >= int((patch_size ** 2) * (percent / 100)):
            kept.append(i)
    return kept


@pytest.mark.parametrize("cls,percent", [(1, 10), (1, 25), (2, 50), (0, 0), (1, 100)])
def test_balance_rows_against_the_reference_loop(cls, percent):
    P = 8
    rng = np.random.default_rng(cls * 1000 + percent)
    patches = [rng.integers(0, 4, (P, P)).astype(np.uint8) for _ in range(12)]
    thr = int(P * P * percent / 100)
    assert thr == int((P ** 2) * (percent / 100))              # the two ways of writing the threshold agree on these cases
    for k, n in enumerate((thr - 1, thr, thr + 1)):             # one below, exactly on and one above the threshold
        p = np.full(P * P, 3 if cls != 3 else 0, np.uint8)
        p[:max(0, min(P * P, n))] = cls
        patches[k] = rng.permutation(p).reshape(P, P)
    cm = np.concatenate(patches, axis=1)                       # one scene, the patches side by side
    table = np.array([[0, 0, P * k, k % 5] for k in range(12)], np.int32)
    counts = scenes.host_class_counts([cm], table, P, 4)
    keep = scenes.balance_rows(counts, cls, percent, P)
    assert keep.dtype == bool and keep.shape == (12,)
    assert np.flatnonzero(keep).tolist() == reference_balance(percent, P, patches, cls)
    if 0 < thr < P * P:
        assert keep[:3].tolist() == [False, True, True]
    with pytest.raises(ValueError, match="class 4 outside 0..3"):
        scenes.balance_rows(counts, 4, percent, P)
    with pytest.raises(ValueError, match="percent"):
        scenes.balance_rows(counts, 1, 101, P)


# ---- 4. ScenePool.class_counts on a cpu pool ------------------------------------------------------------------------------------
def test_cpu_pool_class_counts_with_repeated_windows_in_shuffled_order():
    rng = np.random.default_rng(7)
    shapes = [(40, 57), (33, 36)]
    images = [rng.integers(0, 256, s + (3,)).astype(np.uint8) for s in shapes]
    maps = [rng.integers(0, 8, s).astype(np.uint8) for s in shapes]
    table = scenes.window_table(shapes, 32, 4, True)           # every window five times
    table = np.concatenate([table, table[::3]])[rng.permutation(len(table) + len(table[::3]))]
    pool = scenes.ScenePool(images, maps, patch=32, device="cpu")
    got = pool.class_counts(table, 6)
    assert got.dtype == np.int64 and got.shape == (len(table), 7)
    assert np.array_equal(got, scenes.host_class_counts(maps, table, 32, 6))
    assert np.array_equal(got[:5], loop_counts(maps, table[:5], 32, 32, 6))
    rect = table[np.isin(table[:, 3], (0, 2, 3, 4))][:6]        # a patch of its own: the codes that keep a rectangle's shape
    assert np.array_equal(pool.class_counts(rect, 3, patch=(16, 20)), scenes.host_class_counts(maps, rect, (16, 20), 3))
    with pytest.raises(ValueError, match="row 1: scene 2 outside 0..1"):
        pool.class_counts(np.array([[0, 0, 0, 0], [2, 0, 0, 0]], np.int32), 6)
    with pytest.raises(ValueError, match="C 65 outside 1..64"):
        pool.class_counts(table, 65)
    with pytest.raises(ValueError, match="class maps"):
        scenes.ScenePool(images, None, patch=32, device="cpu").class_counts(table, 6)
    with pytest.raises(ValueError, match="no patch size"):
        scenes.ScenePool(images, maps, device="cpu").class_counts(table, 6)


# ---- 5. rua_scene_class_counts' refusals: nothing is launched -------------------------------------------------------------------
def test_class_counts_argument_validation_without_launch():
    lib = L.lib()
    fn = lib.raw("rua_scene_class_counts")
    A = 1 << 24                                               # fake, suitably aligned addresses: never dereferenced on the host
    shapes = [(40, 50), (64, 33)]
    n = len(shapes)
    ptrs = (ctypes.c_void_p * n)(A, A)
    hs, ws = (ctypes.c_int32 * n)(*[s[0] for s in shapes]), (ctypes.c_int32 * n)(*[s[1] for s in shapes])
    good = np.array([[0, 8, 18, 0], [1, 32, 1, 7], [0, 0, 0, 4]], np.int32)

    def call(table, PH=32, PW=32, C=5, N=None, counts=A, scene_cls=ptrs):
        t = np.ascontiguousarray(table, dtype=np.int32)
        return fn(scene_cls, hs, ws, n, t.ctypes.data, len(t) if N is None else N, PH, PW, C, counts, None)

    for change, msg in [(dict(counts=None), b"required"), (dict(scene_cls=None), b"required"), (dict(N=0), b"N 0"), (dict(C=0), b"C 0 outside 1..64"),
                        (dict(C=65), b"C 65 outside 1..64"), (dict(PH=513), b"PH 513"), (dict(PW=0), b"512"), (dict(counts=A + 2), b"4-byte")]:
        assert call(good, **change) == -1, change
        assert msg in lib.dll.rua_last_error() and b"rua_scene_class_counts: " in lib.dll.rua_last_error(), (change, lib.dll.rua_last_error())
    maps = [np.zeros(s, np.uint8) for s in shapes]
    rows = [([2, 0, 0, 0], "scene 2 outside 0..1"), ([0, 9, 18, 0], "window (9, 18) + 32 x 32 leaves its 40 x 50 scene"),
            ([1, 32, 2, 0], "leaves its 64 x 33 scene"), ([0, 0, -1, 0], "leaves its"), ([0, 0, 0, 8], "code 8 outside 0..7")]
    for at in (0, 2):
        for row, msg in rows:
            table = np.concatenate([good[:at], np.array([row], np.int32)])
            assert call(table) == -1, row
            err = lib.dll.rua_last_error().decode()
            assert err.startswith(f"rua_scene_class_counts: row {at}: ") and msg in err, (row, err)
            with pytest.raises(ValueError) as exc:             # check_table's wording is the same behind the function's name
                scenes.host_class_counts(maps, table, 32, 5)
            assert str(exc.value).split(": ", 1)[1] == err.split(": ", 1)[1]
    assert call(np.array([[0, 0, 0, 0], [0, 0, 0, 5]], np.int32), PH=16, PW=48) == -1
    assert b"row 1: code 5 transposes and needs a square patch (got 16 x 48)" in lib.dll.rua_last_error()


# ---- 6. the CLI ---------------------------------------------------------------------------------------------------------------
def test_cli_parser_and_refusals(tmp_path):
    import train_ISPRS as cli
    base = ["--resunet_a", "yes", "--multitasking", "yes", "-dp", str(tmp_path), "-rp", str(tmp_path / "run")]
    a = cli.build_parser().parse_args(base)
    assert a.class_weights is None and a.balance_class is None and a.balance_percent is None
    assert cli.check_class_flags(a) is None                    # no flag: today's weights
    a = cli.build_parser().parse_args(base + ["--scene_dataset", "yes", "--class_weights", "auto", "--balance_class", "1", "--balance_percent", "10"])
    assert cli.check_class_flags(a) == "auto" and a.balance_class == 1 and a.balance_percent == 10.0
    a = cli.build_parser().parse_args(base + ["--num_classes", "3", "--class_weights", "1", "2.5", "4e1"])
    assert cli.check_class_flags(a) == [1.0, 2.5, 40.0]       # explicit weights: any layout
    refusals = [(["--class_weights", "auto"], "needs --scene_dataset yes"),
                (["--class_weights", "1", "2", "3"], "3 weights for --num_classes 5"),
                (["--num_classes", "6", "--class_weights", "1", "2", "3", "4", "5"], "5 weights for --num_classes 6"),
                (["--scene_dataset", "yes", "--class_weights", "auto", "-cp", str(tmp_path / "m.h5")], "comes from the checkpoint"),
                (["--class_weights", "1", "2", "3", "4", "5", "-cp", str(tmp_path / "m.h5")], "comes from the checkpoint"),
                (["--scene_dataset", "yes", "--class_weights", "auto", "--loss", "tanimoto"], "weighted_cross_entropy"),
                (["--class_weights", "1", "2", "x", "4", "5"], "one number per class"),
                (["--scene_dataset", "yes", "--balance_class", "1"], "go together"),
                (["--balance_class", "1", "--balance_percent", "10"], "needs --scene_dataset yes"),
                (["--scene_dataset", "yes", "--balance_class", "5", "--balance_percent", "10"], "outside 0..4"),
                (["--scene_dataset", "yes", "--balance_class", "1", "--balance_percent", "150"], "outside 0..100")]
    for extra, msg in refusals:
        with pytest.raises(SystemExit) as exc:                 # main refuses before it loads anything
            cli.main(base + extra)
        assert isinstance(exc.value.code, str) and msg in exc.value.code, (extra, exc.value.code)
