"""GPU tests of training from whole scenes: rua_scene_windows (csrc/scene.hip) bit for bit against scenes.host_windows, the engine's
buffers after _upload_scene against _upload_compact fed with host_windows' arrays, the Keras-style surface and the CLI against the
compact path on the same patches."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from resunet_a_mltsk_keras_amd import _lib as L
from resunet_a_mltsk_keras_amd import scenes

from _scene_util import GUARD, HEADS, NCLS as C, assert_same, blob_pool, blob_scene, make_scenes, new_engine, new_training_model, read_scalars, state

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def border_windows(shapes, PH, PW, codes, rng, extra=0):
    """Per scene: the four corners, a window on each border, and `extra` random ones; codes dealt round robin."""
    rows = []
    for s, (H, W) in enumerate(shapes):
        r1, c1 = H - PH, W - PW
        spots = [(0, 0), (0, c1), (r1, 0), (r1, c1), (0, c1 // 2), (r1, c1 // 3), (r1 // 2, 0), (r1 // 3, c1)]
        spots += [(int(rng.integers(0, r1 + 1)), int(rng.integers(0, c1 + 1))) for _ in range(extra)]
        rows += [(s, r, c) for r, c in spots]
    return np.array([[s, r, c, codes[k % len(codes)]] for k, (s, r, c) in enumerate(rows)], np.int32)


def run_windows(images, maps, table, PH, PW, image_only=False):
    """rua_scene_windows into pattern-filled outputs with a guard region behind each; returns (img, cls) and checks the guards."""
    dev = torch.device("cuda")
    pool = scenes.ScenePool(images, None if image_only else maps)
    Cin, N = pool.channels, len(table)
    ni, nc = N * PH * PW * Cin, N * PH * PW
    img_out = torch.full((ni + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    cls_out = torch.full((nc + GUARD,), 0x5A, dtype=torch.uint8, device=dev)
    t = np.ascontiguousarray(table, dtype=np.int32)
    L.lib().call("rua_scene_windows", pool.img_ptrs, pool.cls_ptrs, pool.heights, pool.widths, len(pool), t.ctypes.data, N, PH, PW, Cin,
                 img_out.data_ptr(), None if image_only else cls_out.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    gi, gc = img_out.cpu().numpy(), cls_out.cpu().numpy()
    assert (gi[ni:] == 0xA5).all(), "bytes behind img_out were written"
    assert (gc[nc if not image_only else 0:] == 0x5A).all(), "bytes behind cls_out were written (or cls_out in the image-only form)"
    return gi[:ni].reshape(N, PH, PW, Cin), (None if image_only else gc[:nc].reshape(N, PH, PW))


ALL_CODES = list(range(8))
RECT_CODES = [0, 2, 3, 4]


# odd scene widths: window rows start at every alignment (col * Cin) % 4 and the row pitch W * Cin shifts it from row to row
@pytest.mark.parametrize("PH,PW,codes", [(256, 256, ALL_CODES), (128, 128, ALL_CODES), (64, 64, ALL_CODES), (37, 37, ALL_CODES),
                                         (48, 80, RECT_CODES)])
@pytest.mark.parametrize("Cin", [1, 3, 4, 7])
def test_scene_windows_bitwise(PH, PW, codes, Cin):
    rng = np.random.default_rng(PH * 31 + PW + Cin)
    shapes = [(PH + 41, (PW + 67) | 1), (PH, (PW + 5) | 1), (PH + 3, PW)]  # three scenes of different sizes, two odd widths, two tight fits
    images, maps = make_scenes(rng, shapes, Cin)
    table = border_windows(shapes, PH, PW, codes, rng, extra=4)
    # four consecutive columns: every start alignment (col * Cin) % 4 this Cin can give, under every code
    table = np.concatenate([table] + [np.array([[0, 7 + c, 9 + c, code] for code in codes], np.int32) for c in range(4)])
    assert {(int(c) * Cin) % 4 for c in table[:, 2]} == {(c * Cin) % 4 for c in range(4)}
    gi, gc = run_windows(images, maps, table, PH, PW)
    wi, wc = scenes.host_windows(images, maps, table, (PH, PW))
    assert_same(gi, wi, table, "image")
    assert_same(gc, wc, table, "class map")
    assert set(table[:, 3].tolist()) == set(codes)                         # all of them in the one batch


@pytest.mark.parametrize("N", [1, 8, 300])
def test_scene_windows_batch_sizes_and_image_only(N):
    """N = 1, a training batch, and more windows than one launch carries (128); then the image-only form on the same table."""
    rng = np.random.default_rng(N)
    P, Cin = 64, 3
    shapes = [(97, 131), (64, 64), (150, 75)]
    images, maps = make_scenes(rng, shapes, Cin)
    table = np.array([[s, int(rng.integers(0, shapes[s][0] - P + 1)), int(rng.integers(0, shapes[s][1] - P + 1)), int(rng.integers(0, 8))]
                      for s in rng.integers(0, 3, N)], np.int32)
    wi, wc = scenes.host_windows(images, maps, table, P)
    gi, gc = run_windows(images, maps, table, P, P)
    assert_same(gi, wi, table, "image")
    assert_same(gc, wc, table, "class map")
    oi, oc = run_windows(images, maps, table, P, P, image_only=True)
    assert oc is None
    assert_same(oi, wi, table, "image-only form")


def test_two_calls_are_bitwise_identical():
    rng = np.random.default_rng(9)
    images, maps = make_scenes(rng, [(300, 333)], 3)
    table = border_windows([(300, 333)], 256, 256, ALL_CODES, rng)
    a, b = run_windows(images, maps, table, 256, 256), run_windows(images, maps, table, 256, 256)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- engine / model level -------------------------------------------------------------------------------------------------
def batch_rows(seed, B=2, nscenes=2):
    rng = np.random.default_rng(seed)
    return np.array([[int(rng.integers(0, nscenes)), int(rng.integers(0, 150 - 64 + 1)), int(rng.integers(0, 171 - 64 + 1)), int(rng.integers(0, 8))]
                     for _ in range(B)], np.int32)


@pytest.fixture(scope="module")
def pool():
    return blob_pool()


@pytest.mark.parametrize("multitask", [True, False])
def test_engine_buffers_hold_the_compact_paths_bytes(pool, multitask):
    """host_windows' arrays through _upload_compact vs the same rows through _upload_scene: g.x_in and every head's y hold identical bytes."""
    eng = new_engine(multitask)
    batch = pool.batch(batch_rows(1))
    img, cls = batch.host()
    for training in (True, False):
        g = eng.graph(2, training)
        for norm_type in (1, 2):
            eng._upload_compact(g, torch.from_numpy(img).pin_memory(), torch.from_numpy(cls).pin_memory(), norm_type)
            torch.cuda.synchronize()
            want = [g.x_in.t.clone()] + [h["y"].t.clone() for h in g.heads]
            for t in [g.x_in.t] + [h["y"].t for h in g.heads]:
                t.fill_(float("nan"))
            for t in g.compact_buffers()[:2]:
                t.fill_(0xEE)
            eng._upload_scene(g, batch, norm_type)
            torch.cuda.synchronize()
            got = [g.x_in.t] + [h["y"].t for h in g.heads]
            for w, v in zip(want, got):
                assert torch.equal(w.view(torch.int32), v.view(torch.int32)), (training, norm_type)


def run_sequence(m, pool, scene_input):
    """Two training steps, an evaluation and a prediction: from SceneBatches, or from the compact batches host_windows gives for the same rows."""
    out = {"train metrics": []}
    for s in (11, 12):
        b = pool.batch(batch_rows(s))
        out["train metrics"].append(m.train_on_batch(b, norm_type=1) if scene_input else m.train_on_batch(*b.host(), norm_type=1))
    b = pool.batch(batch_rows(13))
    out["test metrics"] = m.test_on_batch(b, norm_type=1) if scene_input else m.test_on_batch(*b.host(), norm_type=1)
    p = m.predict(b, batch_size=2, norm_type=1) if scene_input else m.predict(b.host()[0], batch_size=2, norm_type=1)
    out["predict"] = np.concatenate([p[h].ravel() for h in HEADS])
    out["weights after two steps"] = state(m)
    return {k: np.asarray(v, np.float64) for k, v in out.items()}


def compare_with_twins(twins, cand, what):
    """The rule of test_model_compact_batches_train_like_float_batches, with its constants: if the twins of the baseline agree exactly
    the candidate must match bit for bit, else deviate at most ten times the twins' own spread plus 1e-6 of scale."""
    deterministic = all(np.array_equal(f[k], twins[0][k]) for f in twins[1:] for k in cand)
    print(f"{what}: the compact-path baseline is {'deterministic: bitwise comparison' if deterministic else 'not deterministic: spread comparison'}")
    for k in cand:
        assert np.isfinite(cand[k]).all(), k
        if deterministic:
            assert np.array_equal(cand[k], twins[0][k]), k
        else:
            spread = max(np.abs(f[k] - g[k]).max() for i, f in enumerate(twins) for g in twins[i + 1:])
            dev = np.abs(cand[k] - twins[0][k]).max()
            print(f"  {k}: scene vs compact {dev:.3g}, compact vs compact up to {spread:.3g}")
            assert dev <= 10 * spread + 1e-6 * max(1.0, np.abs(twins[0][k]).max()), (k, dev, spread)


@pytest.mark.parametrize("use_graph", [True, False])
def test_model_scene_batches_train_like_compact_batches(pool, use_graph):
    twins = [run_sequence(new_training_model(use_graph), pool, False) for _ in range(3)]
    cand = run_sequence(new_training_model(use_graph), pool, True)
    compare_with_twins(twins, cand, f"use_graph={use_graph}")


def test_model_rejects_bad_scene_batches(pool):
    """Each refusal comes before any launch: the model's buffers are never touched (no graph is even built for these batch sizes)."""
    m = new_training_model(True)
    b = pool.batch(batch_rows(2, B=3))
    for nt in (3, 1.0, 0, None, True):
        with pytest.raises(ValueError, match="norm_type"):
            m.train_on_batch(b, norm_type=nt)
        with pytest.raises(ValueError, match="norm_type"):
            m.engine.test_step(b, None, norm_type=nt)
        with pytest.raises(ValueError, match="norm_type"):
            m.predict(b, batch_size=3, norm_type=nt)
    with pytest.raises(ValueError, match=r"32 x 32 x 3 patches .* 64 x 64 x 3"):
        m.train_on_batch(pool.batch(np.array([[0, 0, 0, 0]] * 3, np.int32), 32), norm_type=1)
    four = scenes.ScenePool([np.zeros((70, 70, 4), np.uint8)], [np.zeros((70, 70), np.uint8)], patch=64)
    with pytest.raises(ValueError, match=r"64 x 64 x 4 patches .* 64 x 64 x 3"):
        m.test_on_batch(four.batch(np.array([[0, 0, 0, 0]] * 3, np.int32)), norm_type=1)
    with pytest.raises(ValueError, match="y must be None"):
        m.train_on_batch(b, np.zeros((3, 64, 64), np.uint8), norm_type=1)
    unlabeled = scenes.ScenePool(pool.images, None, patch=64)
    with pytest.raises(ValueError, match="no class maps"):
        m.train_on_batch(unlabeled.batch(batch_rows(2, B=3)), norm_type=1)
    assert not m.engine.graphs                                 # nothing was built, let alone launched


# ---- CLI --------------------------------------------------------------------------------------------------------------------
def run_cli(results, dataset, extra):
    cmd = [sys.executable, os.path.join(ROOT, "train_ISPRS.py"), "--resunet_a", "yes", "--multitasking", "yes", "--loss", "tanimoto", "-rp", results,
           "-dp", dataset, "-bs", "4", "-ps", "64", "--num_classes", str(C), "--epochs", "2", "--dtype", "f32", "--norm_type", "1", "--seed", "5"] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert os.path.exists(os.path.join(results, "best_model.h5"))
    tr, va = read_scalars(os.path.join(results, "logs", "train", "scalars.jsonl")), read_scalars(os.path.join(results, "logs", "val", "scalars.jsonl"))
    assert tr and va and all(np.isfinite(s["value"]) for s in tr + va if s["tag"] != "Segmentation/MCC")
    return {k: np.array([s["value"] for s in tr if s["step"] == 0 and s["tag"] == k], np.float64) for k in sorted({s["tag"] for s in tr})}


def test_cli_scene_directory_trains_like_the_materialised_dataset(tmp_path):
    """A seeded 160 x 192 scene, -ps 64 --stride 32 --data_aug yes, two epochs, f32: the first epoch's training metrics against
    --compact_dataset yes runs on the directory materialize() writes (three of them: the baseline's own spread)."""
    img, cls = blob_scene(200, 160, 192)
    root, dst = str(tmp_path / "scenes"), str(tmp_path / "patches")
    scenes.save_scene_dir(root, ["tile"], [img], [cls])
    assert scenes.materialize(root, dst, 64, 32, True) == 4 * 5 * 5
    twins = [run_cli(str(tmp_path / f"compact{i}"), dst, ["--compact_dataset", "yes"]) for i in range(3)]
    cand = run_cli(str(tmp_path / "scene"), root, ["--scene_dataset", "yes", "--stride", "32", "--data_aug", "yes"])
    assert set(cand) == set(twins[0]) and all(len(v) == 1 for v in cand.values())
    compare_with_twins(twins, cand, "CLI, first epoch")
