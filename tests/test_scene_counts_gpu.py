"""GPU tests of the class counts of scene windows: rua_scene_class_counts (csrc/scene.hip) through the C ABI with exact integer equality
against scenes.host_class_counts - every byte phase of a window row, odd scene widths, windows flush with the borders, uniform maps
(one cell takes every pixel of a window), values equal to C and 255, more windows than one launch carries, overwrite semantics and
the refusals - then ScenePool.class_counts against the cpu pool's and train_ISPRS.main with --class_weights auto and the balance
filter."""
import ast
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from resunet_a_mltsk_keras_amd import _lib as L
from resunet_a_mltsk_keras_amd import scenes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 1024                                                 # int32 cells behind counts that must come back untouched
FILL = 0x5A5A5A5A                                            # what counts holds before a call: not zero
SQUARE_CODES, RECT_CODES = list(range(8)), [0, 2, 3, 4]


def class_pool(maps):
    """A pool of these class maps (the images are not read: one zero channel)."""
    return scenes.ScenePool([np.zeros(m.shape + (1,), np.uint8) for m in maps], maps)


def run_counts(maps, table, PH, PW, C, expect_error=None, N=None):
    """rua_scene_class_counts into a buffer pre-filled with FILL, a guard region behind it; twice into the same buffer.  Returns
    int64 [N][C + 1].  With expect_error: the call must fail with RUA_ERR_ARG and that message and leave the buffer as it was."""
    pool = class_pool(maps)
    t = np.ascontiguousarray(table, dtype=np.int32)
    n = len(t) if N is None else N
    cells = max(n, 1) * (max(C, 0) + 1)
    buf = torch.full((cells + GUARD,), FILL, dtype=torch.int32, device="cuda")
    args = (pool.cls_ptrs, pool.heights, pool.widths, len(pool), t.ctypes.data, n, PH, PW, C, buf.data_ptr(),
            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    if expect_error is not None:
        assert L.lib().raw("rua_scene_class_counts")(*args) == -1
        err = L.lib().dll.rua_last_error().decode()
        assert err.startswith("rua_scene_class_counts: ") and expect_error in err, err
        torch.cuda.synchronize()
        assert (buf.cpu().numpy() == FILL).all(), "a refused call wrote into counts"
        return None
    L.lib().call("rua_scene_class_counts", *args)
    torch.cuda.synchronize()
    first = buf.cpu().numpy()
    assert (first[cells:] == FILL).all(), "cells behind counts were written"
    L.lib().call("rua_scene_class_counts", *args)              # into what the first call left: overwritten, not accumulated
    torch.cuda.synchronize()
    second = buf.cpu().numpy()
    assert np.array_equal(first, second), "a second call into the same buffer gave other counts"
    return first[:cells].reshape(n, C + 1).astype(np.int64)


def assert_counts(got, want, table):
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (len(bad), "first at", tuple(bad[0]), "table row", np.asarray(table)[bad[0][0]].tolist(),
                           "got", got[bad[0][0]].tolist(), "want", want[bad[0][0]].tolist())


def phase_table(shapes, PH, PW, codes):
    """Per scene: the four corners, a window on each border, and windows at columns 0 .. 15 (every byte phase of a row modulo 16, on
    two different rows) as far as the scene allows; codes dealt round robin."""
    rows = []
    for s, (H, W) in enumerate(shapes):
        r1, c1 = H - PH, W - PW
        spots = [(0, 0), (0, c1), (r1, 0), (r1, c1), (0, c1 // 2), (r1, c1 // 3), (r1 // 2, 0), (r1 // 3, c1)]
        spots += [(r, c) for c in range(min(16, c1 + 1)) for r in (min(1, r1), r1 // 2)]
        spots += [(r1 // 2, c1 - c) for c in range(min(16, c1 + 1))]
        rows += [(s, r, c) for r, c in dict.fromkeys(spots)]
    return np.array([[s, r, c, codes[k % len(codes)]] for k, (s, r, c) in enumerate(rows)], np.int32)


def noise_maps(rng, shapes, C):
    """Values 0 .. C + 1 (C and C + 1 are "no class") with a sprinkle of 255, every class present."""
    maps = [rng.integers(0, C + 2, s).astype(np.uint8) for s in shapes]
    for m in maps:
        m[rng.random(m.shape) < 0.02] = 255
    return maps


# ---- 1. exact counts: patches x class counts, odd widths, every phase, borders, three scenes in one call --------------------------
@pytest.mark.parametrize("C", [1, 3, 5, 6, 64])
@pytest.mark.parametrize("PH,PW", [(32, 32), (16, 48), (37, 37)])
def test_class_counts_exact_on_noise(PH, PW, C):
    rng = np.random.default_rng(PH * 1000 + PW * 10 + C)
    shapes = [(PH + 9, 101), (PH + 30, 77), (PH, PW)]           # odd widths: the row pitch moves the phase from row to row; one scene exactly a patch
    maps = noise_maps(rng, shapes, C)
    table = phase_table(shapes, PH, PW, SQUARE_CODES if PH == PW else RECT_CODES)
    assert len(table) > 60 and {int(c) % 16 for c in table[:, 2]} == set(range(16))
    got = run_counts(maps, table, PH, PW, C)
    want = scenes.host_class_counts(maps, table, (PH, PW), C)
    assert_counts(got, want, table)
    assert (got.sum(1) == PH * PW).all()


def test_codes_share_one_row():
    rng = np.random.default_rng(5)
    maps = noise_maps(rng, [(50, 77)], 5)
    table = np.array([[0, 7, 13, code] for code in range(8)], np.int32)
    got = run_counts(maps, table, 37, 37, 5)
    assert_counts(got, scenes.host_class_counts(maps, table, 37, 5), table)
    assert (got == got[0]).all()


# ---- 2. large patches --------------------------------------------------------------------------------------------------------
def test_class_counts_256():
    rng = np.random.default_rng(11)
    shapes = [(300, 333)]
    f = rng.integers(0, 8, (300 // 16 + 1, 333 // 16 + 1)).astype(np.uint8)          # blocky, as real class maps are; 6 and 7: no class
    maps = [np.ascontiguousarray(np.kron(f, np.ones((16, 16), np.uint8))[:300, :333])]
    table = np.array([[0, 0, 0, 0], [0, 44, 77, 1], [0, 44, 76, 5], [0, 0, 77, 2], [0, 44, 0, 3], [0, 13, 35, 6], [0, 30, 16, 7], [0, 1, 1, 4]], np.int32)
    got = run_counts(maps, table, 256, 256, 6)
    assert_counts(got, scenes.host_class_counts(maps, table, 256, 6), table)


@pytest.mark.parametrize("value,C", [(2, 5), (5, 5), (255, 6), (0, 1)])
def test_uniform_512_window_fills_one_cell(value, C):
    """Every pixel of a 512 x 512 window in one cell: 262 144, far beyond any 8- or 16-bit partial counter."""
    maps = [np.full((512, 512), value, np.uint8)]
    table = np.array([[0, 0, 0, 0]], np.int32)
    got = run_counts(maps, table, 512, 512, C)
    want = np.zeros((1, C + 1), np.int64)
    want[0, min(value, C)] = 512 * 512
    assert_counts(got, want, table)
    assert_counts(got, scenes.host_class_counts(maps, table, 512, C), table)


def test_noise_512_window():
    rng = np.random.default_rng(13)
    maps = noise_maps(rng, [(512, 512)], 6)
    table = np.array([[0, 0, 0, 3]], np.int32)
    assert_counts(run_counts(maps, table, 512, 512, 6), scenes.host_class_counts(maps, table, 512, 6), table)


# ---- 3. uniform maps: the contended case --------------------------------------------------------------------------------------
@pytest.mark.parametrize("PH,PW", [(32, 32), (16, 48), (37, 37)])
@pytest.mark.parametrize("value,C", [(0, 5), (4, 5), (5, 5), (255, 5), (63, 64), (64, 64)])
def test_uniform_maps(PH, PW, value, C):
    shapes = [(PH + 9, 101), (PH, PW)]
    maps = [np.full(s, value, np.uint8) for s in shapes]
    table = phase_table(shapes, PH, PW, [0])
    got = run_counts(maps, table, PH, PW, C)
    want = np.zeros((len(table), C + 1), np.int64)
    want[:, min(value, C)] = PH * PW
    assert_counts(got, want, table)


# ---- 4. N = 1, 8, 300 (more than one launch) ------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 8, 300])
def test_batch_sizes(N):
    rng = np.random.default_rng(N)
    shapes = [(70, 101), (64, 77), (45, 40)]
    maps = noise_maps(rng, shapes, 6)
    t = np.empty((N, 4), np.int32)
    t[:, 0] = rng.integers(0, 3, N)
    t[:, 1] = [rng.integers(0, shapes[s][0] - 32 + 1) for s in t[:, 0]]
    t[:, 2] = [rng.integers(0, shapes[s][1] - 32 + 1) for s in t[:, 0]]
    t[:, 3] = np.arange(N) % 8
    got = run_counts(maps, t, 32, 32, 6)
    assert_counts(got, scenes.host_class_counts(maps, t, 32, 6), t)


# ---- 5. refusals: RUA_ERR_ARG naming the row, the buffer left as it was ---------------------------------------------------------
def test_refusals_leave_the_buffer_alone():
    rng = np.random.default_rng(17)
    shapes = [(40, 57), (64, 50)]
    maps = noise_maps(rng, shapes, 5)
    good = np.array([[0, 8, 18, 0], [1, 32, 1, 7], [0, 0, 0, 4]], np.int32)

    def with_row(at, row):
        t = good.copy()
        t[at] = row
        return t
    run_counts(maps, with_row(2, [2, 0, 0, 0]), 32, 32, 5, expect_error="row 2: scene 2 outside 0..1")
    run_counts(maps, with_row(1, [0, 9, 18, 0]), 32, 32, 5, expect_error="row 1: window (9, 18) + 32 x 32 leaves its 40 x 57 scene")
    run_counts(maps, with_row(0, [1, 32, 19, 0]), 32, 32, 5, expect_error="row 0: window (32, 19) + 32 x 32 leaves its 64 x 50 scene")
    run_counts(maps, np.array([[0, 24, 9, 0], [1, 48, 2, 2], [0, 0, 0, 6]], np.int32), 16, 48, 5, expect_error="row 2: code 6 transposes and needs a square patch (got 16 x 48)")
    run_counts(maps, good, 32, 32, 0, expect_error="C 0 outside 1..64")
    run_counts(maps, good, 32, 32, 65, expect_error="C 65 outside 1..64")
    run_counts(maps, good, 513, 32, 5, expect_error="PH 513")
    run_counts(maps, good, 32, 32, 5, N=0, expect_error="N 0")
    got = run_counts(maps, good, 32, 32, 5)                     # and the same rows, unbroken, are counted
    assert_counts(got, scenes.host_class_counts(maps, good, 32, 5), good)


# ---- 6. ScenePool.class_counts -------------------------------------------------------------------------------------------------
def test_pool_class_counts_equal_the_cpu_pools():
    rng = np.random.default_rng(19)
    shapes = [(70, 101), (64, 77)]
    images = [rng.integers(0, 256, s + (3,)).astype(np.uint8) for s in shapes]
    maps = noise_maps(rng, shapes, 5)
    table = scenes.window_table(shapes, 32, 8, True)             # every window five times: one row of counts each on the device
    table = table[rng.permutation(len(table))]
    gpu, cpu = scenes.ScenePool(images, maps, patch=32), scenes.ScenePool(images, maps, patch=32, device="cpu")
    got = gpu.class_counts(table, 5)
    assert got.dtype == np.int64 and got.shape == (len(table), 6)
    assert_counts(got, cpu.class_counts(table, 5), table)
    rect = scenes.window_table(shapes, (16, 48), 8, False)[::3]   # a patch of its own
    assert_counts(gpu.class_counts(rect, 7, patch=(16, 48)), cpu.class_counts(rect, 7, patch=(16, 48)), rect)
    with pytest.raises(ValueError, match="row 1: scene 2 outside 0..1"):
        gpu.class_counts(np.array([[0, 0, 0, 0], [2, 0, 0, 0]], np.int32), 5)


# ---- 7. the CLI ------------------------------------------------------------------------------------------------------------------
def cli_scene(seed, H=96, W=128, C=4):
    """Class 1 fills the columns left of 41 (with holes of other classes and a few "no class" pixels), so of the windows at columns
    0, 32 and 64 the first two hold at least 10 % of it and the third holds none."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    f = rng.choice([0, 2, 3], (H // 8, W // 8))
    cls = np.kron(f, np.ones((8, 8), np.int64))[:H, :W]
    cls[:, :41] = 1
    cls[10:20, 5:15] = 2
    cls[50:53, 90:100] = 255
    cls[70:72, 0:30] = C
    return img, cls.astype(np.uint8)


def test_cli_auto_weights_and_balance_filter(tmp_path, capsys):
    """train_ISPRS.main --class_weights auto --balance_class 1 --balance_percent 10 on a 96 x 128 scene, one epoch: the printed
    weights are class_weights of the kept training rows, it trains on exactly the kept count, and a second run gives the same
    weights.  -ps 64, as every CLI test of this suite: five stride-2 levels and the 2 x 2 pooling of the middle PSPPooling make 64
    the smallest input the network accepts (at 32 its deepest level is 1 x 1 and the pooling does not divide it)."""
    sys.path.insert(0, ROOT)
    import train_ISPRS as cli
    P, S, C = 64, 32, 4
    img, cls = cli_scene(23)
    root = str(tmp_path / "scenes")
    scenes.save_scene_dir(root, ["tile"], [img], [cls])
    # what the run must arrive at, from the definitions alone
    table = scenes.window_table([img.shape], P, S, True)
    xs, ys = cli.list_scene_dataset(len(table))
    x_tr, _, x_va, _ = cli.split_dataset(xs, ys)
    tr_rows = table[[scenes.patch_index(n) for n in x_tr]]
    counts = scenes.host_class_counts([cls], tr_rows, P, C)
    keep = scenes.balance_rows(counts, 1, 10, P)
    assert 4 <= keep.sum() < len(keep)                          # the filter takes some rows and leaves a batch at least
    want = scenes.class_weights(counts[keep])

    def run(name):
        cli.main(["--resunet_a", "yes", "--multitasking", "yes", "--loss", "weighted_cross_entropy", "-rp", str(tmp_path / name), "-dp", root,
                  "-bs", "4", "-ps", str(P), "--num_classes", str(C), "--epochs", "1", "--dtype", "f32", "--norm_type", "1", "--seed", "5",
                  "--scene_dataset", "yes", "--stride", str(S), "--data_aug", "yes",
                  "--class_weights", "auto", "--balance_class", "1", "--balance_percent", "10"])
        out = capsys.readouterr().out
        lines = out.splitlines()
        at = lines.index("Using Weighted cross entropy")
        assert f"Balance filter: class 1 >= 10 % keeps {int(keep.sum())} of {len(keep)} training windows" in out, out[:3000]
        assert f"Training on {int(keep.sum())} images" in lines and f"Validating on {len(x_va)} images" in lines, out[:3000]
        assert f"Class histogram of the {int(keep.sum())} training windows:" in lines
        assert os.path.exists(tmp_path / name / "best_model.h5")
        return ast.literal_eval(lines[at + 1])

    first = run("a")
    assert first == [float(w) for w in want], (first, want.tolist())
    assert run("b") == first
