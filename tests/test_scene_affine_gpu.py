"""GPU tests of the affine scene windows: rua_scene_windows_affine (csrc/scene.hip) bit for bit against scenes.host_windows_affine
and, without a jitter, against rua_scene_windows; the engine's buffers after _upload_scene with an AffineSceneBatch against
_upload_compact fed with its host() arrays; the Keras-style surface against the compact path on the same patches; the CLI with
--random_aug yes."""
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
Q = 65536


def run_windows(name, images, maps, table, PH, PW, image_only=False):
    """`name` (rua_scene_windows or rua_scene_windows_affine) into pattern-filled outputs with a guard region behind each; returns
    (img, cls) and checks the guards."""
    dev = torch.device("cuda")
    pool = scenes.ScenePool(images, None if image_only else maps)
    Cin, N = pool.channels, len(table)
    ni, nc = N * PH * PW * Cin, N * PH * PW
    img_out = torch.full((ni + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    cls_out = torch.full((nc + GUARD,), 0x5A, dtype=torch.uint8, device=dev)
    t = np.ascontiguousarray(table, dtype=np.int32)
    L.lib().call(name, pool.img_ptrs, pool.cls_ptrs, pool.heights, pool.widths, len(pool), t.ctypes.data, N, PH, PW, Cin,
                 img_out.data_ptr(), None if image_only else cls_out.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    gi, gc = img_out.cpu().numpy(), cls_out.cpu().numpy()
    assert (gi[ni:] == 0xA5).all(), "bytes behind img_out were written"
    assert (gc[nc if not image_only else 0:] == 0x5A).all(), "bytes behind cls_out were written (or cls_out in the image-only form)"
    return gi[:ni].reshape(N, PH, PW, Cin), (None if image_only else gc[:nc].reshape(N, PH, PW))


def affine_table(rng, shapes, PH, PW, N):
    """N rows over all scenes: patch centres on every border, in every corner, up to a patch outside the scene and anywhere inside;
    random angles; zoom 0.25, 1 and 4 and log-uniform in between; the symmetry codes the patch shape allows."""
    codes = list(range(8)) if PH == PW else [0, 2, 3, 4]
    rows4 = np.zeros((N, 4), np.int32)
    rows4[:, 0] = np.arange(N) % len(shapes)
    rows4[:, 3] = [codes[k % len(codes)] for k in range(N)]
    zoom = np.exp(rng.uniform(np.log(0.25), np.log(4.0), N))
    zoom[0:9:3], zoom[1:9:3], zoom[2:9:3] = 0.25, 1.0, 4.0     # the extremes and 1 on each scene
    angle = rng.uniform(-180, 180, N)
    cy, cx = np.empty(N), np.empty(N)
    for k in range(N):
        H, W = shapes[rows4[k, 0]]
        ys = [0, H - 1, (H - 1) / 2, -PH, H - 1 + PH, rng.uniform(-PH, H - 1 + PH)]
        xs = [0, W - 1, (W - 1) / 2, -PW, W - 1 + PW, rng.uniform(-PW, W - 1 + PW)]
        q = k // len(shapes)                                   # every (y, x) pair of the first five on every scene, then random ones
        cy[k], cx[k] = (ys[q // 5], xs[q % 5]) if q < 25 else (ys[5], xs[5])
    shift = np.stack([np.rint((cy - (PH - 1) / 2) * Q), np.rint((cx - (PW - 1) / 2) * Q)], 1).astype(np.int64)
    return scenes.affine_rows(rows4, (PH, PW), angle, zoom, shift)


# ---- 1. the kernel against its numpy definition -----------------------------------------------------------------------------------
@pytest.mark.parametrize("PH,PW,N", [(256, 256, 84), (128, 128, 90), (37, 37, 300), (48, 80, 300)])
@pytest.mark.parametrize("Cin", [1, 3, 4, 7])
def test_affine_windows_bitwise(PH, PW, N, Cin):
    """Three scenes per call (two odd widths, one of them 2 x 2); 300 windows are more than three launches' worth (80 each), 84 and
    90 more than one."""
    rng = np.random.default_rng(PH * 31 + PW + Cin)
    shapes = [(PH + 41, (PW + 67) | 1), (2, 2), (PH // 2 + 3, (PW + 5) | 1)]
    images, maps = make_scenes(rng, shapes, Cin)
    table = affine_table(rng, shapes, PH, PW, N)
    wi, wc = scenes.host_windows_affine(images, maps, table, (PH, PW))
    gi, gc = run_windows("rua_scene_windows_affine", images, maps, table, PH, PW)
    assert_same(gi, wi, table, "image")
    assert_same(gc, wc, table, "class map")
    oi, oc = run_windows("rua_scene_windows_affine", images, maps, table, PH, PW, image_only=True)
    assert oc is None
    assert_same(oi, wi, table, "image-only form")


# ---- 2. without a jitter: the existing kernel's bytes -----------------------------------------------------------------------------
@pytest.mark.parametrize("PH,PW,codes", [(256, 256, list(range(8))), (37, 37, list(range(8))), (48, 80, [0, 2, 3, 4])])
@pytest.mark.parametrize("Cin", [1, 3, 4, 7])
def test_affine_rows_without_jitter_equal_scene_windows(PH, PW, codes, Cin):
    rng = np.random.default_rng(PH + PW * 7 + Cin)
    shapes = [(PH + 41, (PW + 67) | 1), (PH, (PW + 5) | 1), (PH + 3, PW)]
    images, maps = make_scenes(rng, shapes, Cin)
    rows = []
    for s, (H, W) in enumerate(shapes):
        r1, c1 = H - PH, W - PW
        spots = [(0, 0), (0, c1), (r1, 0), (r1, c1), (r1 // 2, c1 // 3), (int(rng.integers(0, r1 + 1)), int(rng.integers(0, c1 + 1)))]
        rows += [[s, r, c, code] for r, c in spots for code in codes]
    rows4 = np.array(rows, np.int32)
    ki, kc = run_windows("rua_scene_windows", images, maps, rows4, PH, PW)
    ai, ac = run_windows("rua_scene_windows_affine", images, maps, scenes.affine_rows(rows4, (PH, PW)), PH, PW)
    assert_same(ai, ki, rows4, "image")
    assert_same(ac, kc, rows4, "class map")


# ---- engine / model level -----------------------------------------------------------------------------------------------------
def affine_batch(pool, seed, B=2, nscenes=2):
    """B windows anywhere in the scenes (borders included), each under its own rotation, zoom in [0.5, 2] and shift of up to 20 px."""
    rng = np.random.default_rng(seed)
    rows4 = np.array([[int(rng.integers(0, nscenes)), int(rng.integers(0, 150 - 64 + 1)), int(rng.integers(0, 171 - 64 + 1)), int(rng.integers(0, 8))]
                      for _ in range(B)], np.int32)
    t7 = scenes.affine_rows(rows4, 64, rng.uniform(-180, 180, B), np.exp(rng.uniform(np.log(0.5), np.log(2.0), B)),
                            rng.integers(-20 * Q, 20 * Q + 1, (B, 2)))
    return pool.affine_batch(t7)


@pytest.fixture(scope="module")
def pool():
    return blob_pool()


@pytest.mark.parametrize("multitask", [True, False])
def test_engine_buffers_hold_the_compact_paths_bytes(pool, multitask):
    """host()'s arrays through _upload_compact vs the same affine rows through _upload_scene: g.x_in and every head's y hold identical bytes."""
    eng = new_engine(multitask)
    batch = affine_batch(pool, 1)
    assert isinstance(batch, scenes.AffineSceneBatch)
    img, cls = batch.host()
    assert not np.array_equal(img, pool.batch(np.array([[0, 0, 0, 0]] * 2, np.int32)).host()[0])
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
    """Two training steps, an evaluation and a prediction: from AffineSceneBatches, or from the compact batches host() gives for the same rows."""
    out = {"train metrics": []}
    for s in (11, 12):
        b = affine_batch(pool, s)
        out["train metrics"].append(m.train_on_batch(b, norm_type=1) if scene_input else m.train_on_batch(*b.host(), norm_type=1))
    b = affine_batch(pool, 13)
    out["test metrics"] = m.test_on_batch(b, norm_type=1) if scene_input else m.test_on_batch(*b.host(), norm_type=1)
    p = m.predict(b, batch_size=2, norm_type=1) if scene_input else m.predict(b.host()[0], batch_size=2, norm_type=1)
    out["predict"] = np.concatenate([p[h].ravel() for h in HEADS])
    out["weights after two steps"] = state(m)
    return {k: np.asarray(v, np.float64) for k, v in out.items()}


def compare_with_twins(twins, cand, what):
    """The rule of tests/test_scenes_gpu.py, with its constants: if the twins of the baseline agree exactly the candidate must match
    bit for bit, else deviate at most ten times the twins' own spread plus 1e-6 of scale."""
    deterministic = all(np.array_equal(f[k], twins[0][k]) for f in twins[1:] for k in cand)
    print(f"{what}: the compact-path baseline is {'deterministic: bitwise comparison' if deterministic else 'not deterministic: spread comparison'}")
    for k in cand:
        assert np.isfinite(cand[k]).all(), k
        if deterministic:
            assert np.array_equal(cand[k], twins[0][k]), k
        else:
            spread = max(np.abs(f[k] - g[k]).max() for i, f in enumerate(twins) for g in twins[i + 1:])
            dev = np.abs(cand[k] - twins[0][k]).max()
            print(f"  {k}: affine scene vs compact {dev:.3g}, compact vs compact up to {spread:.3g}")
            assert dev <= 10 * spread + 1e-6 * max(1.0, np.abs(twins[0][k]).max()), (k, dev, spread)


@pytest.mark.parametrize("use_graph", [True, False])
def test_model_affine_batches_train_like_compact_batches(pool, use_graph):
    twins = [run_sequence(new_training_model(use_graph), pool, False) for _ in range(3)]
    cand = run_sequence(new_training_model(use_graph), pool, True)
    compare_with_twins(twins, cand, f"use_graph={use_graph}")


# ---- CLI --------------------------------------------------------------------------------------------------------------------------
def run_cli(results, dataset, extra):
    cmd = [sys.executable, os.path.join(ROOT, "train_ISPRS.py"), "--resunet_a", "yes", "--multitasking", "yes", "--loss", "tanimoto", "-rp", results,
           "-dp", dataset, "-bs", "4", "-ps", "64", "--num_classes", str(C), "--epochs", "2", "--dtype", "f32", "--norm_type", "1", "--seed", "5",
           "--scene_dataset", "yes", "--stride", "32", "--data_aug", "yes"] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert os.path.exists(os.path.join(results, "best_model.h5"))
    tr, va = read_scalars(os.path.join(results, "logs", "train", "scalars.jsonl")), read_scalars(os.path.join(results, "logs", "val", "scalars.jsonl"))
    assert tr and va and all(np.isfinite(s["value"]) for s in tr + va if s["tag"] != "Segmentation/MCC")
    return {k: np.array([s["value"] for s in tr if s["tag"] == k], np.float64) for k in sorted({s["tag"] for s in tr if s["tag"].endswith("/Loss")})}


def test_cli_random_aug_trains_and_is_live(tmp_path):
    """A seeded 160 x 192 scene, -ps 64, two epochs, f32: --random_aug yes runs to the end with finite losses and a checkpoint, and
    logs other training losses than --random_aug no from the same seed."""
    img, cls = blob_scene(200, 160, 192)
    root = str(tmp_path / "scenes")
    scenes.save_scene_dir(root, ["tile"], [img], [cls])
    aug = run_cli(str(tmp_path / "aug"), root, ["--random_aug", "yes"])
    plain = run_cli(str(tmp_path / "plain"), root, ["--random_aug", "no"])
    assert set(aug) == set(plain) and all(len(v) == 2 and np.isfinite(v).all() for v in aug.values())
    print({k: (aug[k].tolist(), plain[k].tolist()) for k in aug})
    assert all(not np.array_equal(aug[k], plain[k]) for k in aug)
