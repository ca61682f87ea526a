"""GPU tests of the photometric jitter: rua_window_photometric (csrc/photo.hip) bit for bit against scenes.host_photometric, in place
and out of place; the engine's buffers after _upload_scene with a photo table against _upload_compact fed with batch.host(); the
Keras-style surface against the compact path on the same bytes; the CLI with --photo_aug yes."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from resunet_a_mltsk_keras_amd import _lib as L
from resunet_a_mltsk_keras_amd import scenes

from _scene_util import GUARD, NCLS as C, blob_pool, blob_scene, new_engine, new_training_model, read_scalars, state

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = 65536
IDENT = np.array([Q, 0, 0, 0, Q, 0, 0, 0, Q, 0, 0, 0, 0, 0, 0, 0], np.int64)


def rows_within_limits(rng, n, scalar, first=0):
    """n rows: random within the limits, every second one moderate (a matrix at the limits saturates nearly every byte); the first
    ones are, from number `first` of them on: two rows AT each limit (both signs), an identity row, a row with A = 0, a row with t = 0."""
    t = np.zeros((n, 16), np.int64)
    t[:, :9] = rng.integers(-(1 << 20), (1 << 20) + 1, (n, 9))
    t[:, 9:12] = rng.integers(-(1 << 29), (1 << 29) + 1, (n, 3))
    t[:, 12] = rng.integers(-Q, Q + 1, n)
    t[:, 13] = rng.integers(0, Q + 1, n)
    t[:, 14] = rng.integers(-(1 << 31), 1 << 31, n)
    for k in range(0, n, 2):
        t[k, :9] = IDENT[:9] + rng.integers(-20000, 20001, 9)
        t[k, 9:12] = rng.integers(-40 * Q, 40 * Q + 1, 3)
        t[k, 13] = rng.integers(0, 4000)
    M, B = 1 << 20, 1 << 29
    special = [[M, M, M, -M, -M, M, M, -M, M, B, -B, B, Q, Q, -1, 0], [-M, M, -M, M, M, -M, -M, M, -M, -B, B, -B, -Q, Q, (1 << 31) - 1, 0],
               IDENT.tolist(), [70000, 900, -800, 0, 60000, 5000, -3000, 0, 65000, -5 * Q, 3 * Q, 0, 30000, 0, 77, 0],
               [Q, 0, 0, 0, 50000, 0, 0, 2000, Q, 0, 9 * Q, -Q, 0, 3000, -(1 << 31), 0]]
    for k, r in enumerate(special[first:first + n]):
        t[k] = r
    if scalar:
        t[:, 1:4] = t[:, 5:8] = 0
        t[:, 4] = t[:, 8] = t[:, 0]
        t[:, 10] = t[:, 11] = t[:, 9]
    return t.astype(np.int32)


def run_photometric(img, table, in_place):
    """rua_window_photometric on a device copy of img: into itself, or into a pattern-filled output; GUARD bytes behind either buffer
    must come back untouched and, out of place, the input too."""
    dev = torch.device("cuda")
    N, PH, PW, Cin = img.shape
    n = img.size
    src = torch.full((n + GUARD,), 0x5A, dtype=torch.uint8, device=dev)
    src[:n] = torch.from_numpy(img.ravel()).to(dev)
    dst = src if in_place else torch.full((n + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    t = np.ascontiguousarray(table, dtype=np.int32)
    L.lib().call("rua_window_photometric", src.data_ptr(), dst.data_ptr(), N, PH, PW, Cin, t.ctypes.data,
                 ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    s, d = src.cpu().numpy(), dst.cpu().numpy()
    assert (s[n:] == 0x5A).all(), "bytes behind img_in were written"
    if not in_place:
        assert (d[n:] == 0xA5).all(), "bytes behind img_out were written"
        assert np.array_equal(s[:n], img.ravel()), "the input of an out-of-place call changed"
    return d[:n].reshape(img.shape)


# ---- 1. the kernel against its numpy definition -----------------------------------------------------------------------------------
@pytest.mark.parametrize("PH,PW,N,Cin", [(5, 7, 3, 3), (8, 8, 50, 3), (33, 31, 4, 1), (16, 16, 5, 4), (9, 9, 3, 7), (64, 64, 4, 3),
                                         (5, 7, 5, 3), (1, 1, 9, 3), (1, 2, 6, 1), (1, 1, 5, 16)])
def test_photometric_bitwise(PH, PW, N, Cin):
    """105-byte windows start at byte phases 0, 1, 2 (and 3 with five of them); 50 windows are more than one launch's 48; 33 x 31 x 1
    and 9 x 9 x 7 windows are odd too; 64 x 64 x 3 has several blocks' worth of whole runs; one-pixel and two-byte windows are shorter
    than the bytes in front of their first dword boundary.  With fewer than five windows a second table holds the special rows the
    first has no room for."""
    rng = np.random.default_rng(PH * 131 + PW * 7 + N + Cin)
    img = rng.integers(0, 256, (N, PH, PW, Cin)).astype(np.uint8)
    img[0, 0, 0], img[-1, -1, -1] = 255, 0
    for first in ((0, 2) if N < 5 else (0,)):
        table = rows_within_limits(rng, N, Cin != 3, first)
        want = scenes.host_photometric(img, table)
        assert not np.array_equal(want, img)
        for in_place in (True, False):
            got = run_photometric(img, table, in_place)
            bad = np.argwhere(got != want)
            assert bad.size == 0, ("in place" if in_place else "out of place", len(bad), "first at", tuple(bad[0]), "row", table[bad[0][0]].tolist())
    ident = np.tile(IDENT.astype(np.int32), (N, 1))             # identity rows: left alone in place, copied out of place
    for in_place in (True, False):
        assert np.array_equal(run_photometric(img, ident, in_place), img)


# ---- 2. engine --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pool():
    return blob_pool()


def photo_batch(pool, seed, affine, B=2):
    """B windows anywhere in the two scenes, plain (any code) or under a rotation, zoom and shift, with a drawn photo table."""
    rng = np.random.default_rng(seed)
    rows4 = np.array([[int(rng.integers(0, 2)), int(rng.integers(0, 150 - 64 + 1)), int(rng.integers(0, 171 - 64 + 1)), int(rng.integers(0, 8))]
                      for _ in range(B)], np.int32)
    if affine:
        b = pool.affine_batch(scenes.affine_rows(rows4, 64, rng.uniform(-180, 180, B), np.exp(rng.uniform(np.log(0.5), np.log(2.0), B)),
                                                 rng.integers(-20 * Q, 20 * Q + 1, (B, 2))))
    else:
        b = pool.batch(rows4)
    return b.with_photo(scenes.PhotoJitter(noise_sigma=(1.0, 3.0)).draw(rng, B, 3))


@pytest.mark.parametrize("affine", [False, True])
def test_engine_buffers_hold_the_compact_paths_bytes(pool, affine):
    """A scene batch with a photo table through _upload_scene leaves batch.host()'s bytes in g.compact_buffers(); g.x_in and every
    head's y are what _upload_compact makes from those host bytes."""
    eng = new_engine(True)
    batch = photo_batch(pool, 1, affine)
    assert type(batch) is (scenes.AffineSceneBatch if affine else scenes.SceneBatch)
    img, cls = batch.host()
    assert not np.array_equal(img, batch.with_photo(None).host()[0])
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
            bi, bc = g.compact_buffers()[:2]
            assert np.array_equal(bi.cpu().numpy().reshape(img.shape), img) and np.array_equal(bc.cpu().numpy().reshape(cls.shape), cls)
            got = [g.x_in.t] + [h["y"].t for h in g.heads]
            for w, v in zip(want, got):
                assert torch.equal(w.view(torch.int32), v.view(torch.int32)), (training, norm_type)
            # the keyword on a compact batch: the unjittered bytes and the table give the same buffers
            raw = batch.with_photo(None).host()[0]
            for t in got:
                t.fill_(float("nan"))
            eng._upload_compact(g, torch.from_numpy(raw), torch.from_numpy(cls), norm_type, eng._check_photo(raw, norm_type, batch.photo))
            torch.cuda.synchronize()
            assert np.array_equal(g.compact_buffers()[0].cpu().numpy().reshape(img.shape), img)
            for w, v in zip(want, got):
                assert torch.equal(w.view(torch.int32), v.view(torch.int32)), ("photo=", training, norm_type)


def test_photo_keyword_is_refused_where_it_has_no_meaning(pool):
    eng = new_engine(False)
    batch = photo_batch(pool, 2, False)
    table = batch.photo
    x = np.zeros((2, 64, 64, 3), np.float32)
    y = np.zeros((2, 64, 64, C), np.float32)
    for step in (eng.train_step, eng.test_step, eng.forward_backward):
        with pytest.raises(ValueError, match="float batch"):
            step(x, y, photo=table)
        with pytest.raises(ValueError, match="carries its own"):
            step(batch, None, norm_type=1, photo=table)
    u8 = np.zeros((2, 64, 64, 3), np.uint8)
    with pytest.raises(ValueError, match="photo rows for a batch"):
        eng.train_step(u8, np.zeros((2, 64, 64), np.uint8), norm_type=1, photo=table[:1])
    bad = table.copy()
    bad[1, 13] = -1
    with pytest.raises(ValueError, match="row 1: word 13"):
        eng.test_step(u8, np.zeros((2, 64, 64), np.uint8), norm_type=1, photo=bad)
    m = new_training_model(False)
    with pytest.raises(ValueError, match="carries its own"):
        m.train_on_batch(batch, norm_type=1, photo=table)
    with pytest.raises(ValueError, match="float batch"):
        m.test_on_batch(x, {h: y for h in ("seg",)}, photo=table)


# ---- 3. model ---------------------------------------------------------------------------------------------------------------------
def run_steps(m, pool, how):
    """Three training steps on the same jittered windows: from scene batches that carry their photo tables ("scene"), from the
    compact batches their host() gives ("host"), or from the unjittered compact batches and photo= ("keyword")."""
    out = []
    for k, (seed, affine) in enumerate([(21, False), (22, True), (23, False)]):
        b = photo_batch(pool, seed, affine)
        if how == "scene":
            out.append(m.train_on_batch(b, norm_type=1))
        elif how == "host":
            out.append(m.train_on_batch(*b.host(), norm_type=1))
        else:
            raw = b.with_photo(None).host()
            out.append(m.train_on_batch(raw[0], raw[1], norm_type=1, photo=b.photo))
    return np.asarray(out, np.float64), state(m)


@pytest.fixture
def one_block_stem():
    """Of the 346 gradient tensors of this model's step, 344 are the same bits in every run; the stem's kernel and bias are not: every
    block of rua_stem_bwd ends in one float atomic per weight, and the order the blocks arrive in is the hardware's (measured: two
    runs of the compact path on the same bytes differ by 7e-9 there, and by 7e-4 in the weights three Adam steps later).  With the
    tuning key stem_blocks = 1 that kernel is one block, and the whole step is a function of its inputs - on both sides alike."""
    lib = L.lib()
    before = lib.get_tuning("stem_blocks")
    lib.set_tuning(stem_blocks=1)
    yield
    lib.set_tuning(stem_blocks=before)


@pytest.mark.parametrize("use_graph", [True, False])
def test_model_photo_batches_train_like_compact_batches(pool, one_block_stem, use_graph):
    """Three training steps from scene batches that carry photo tables, and from compact batches with photo=, against the compact
    batches of batch.host(): the same metrics and the same weights and BatchNorm state, bit for bit."""
    want_metrics, want_state = run_steps(new_training_model(use_graph), pool, "host")
    assert np.isfinite(want_metrics).all()
    twin_metrics, twin_state = run_steps(new_training_model(use_graph), pool, "host")
    assert np.array_equal(twin_metrics, want_metrics) and np.array_equal(twin_state, want_state), "the compact path does not reproduce itself"
    for how in ("scene", "keyword"):
        metrics, st = run_steps(new_training_model(use_graph), pool, how)
        print(how, "metrics deviate by", np.abs(metrics - want_metrics).max(), "state by", np.abs(st - want_state).max())
        assert np.array_equal(metrics, want_metrics), how
        assert np.array_equal(st, want_state), how


# ---- 4. CLI -----------------------------------------------------------------------------------------------------------------------
def run_cli(results, dataset, extra, expect_ok=True):
    cmd = [sys.executable, os.path.join(ROOT, "train_ISPRS.py"), "--resunet_a", "yes", "--multitasking", "yes", "--loss", "tanimoto", "-rp", results,
           "-dp", dataset, "-bs", "4", "-ps", "64", "--num_classes", str(C), "--epochs", "1", "--dtype", "f32", "--norm_type", "1", "--seed", "5",
           "--stride", "32", "--data_aug", "no"] + extra
    # two runs write the same scalars only if the step is a function of its inputs: the stem's weight gradient as one block (one_block_stem)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ, RUA_TUNE_STEM_BLOCKS="1"))
    if not expect_ok:
        return r
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    tr, va = read_scalars(os.path.join(results, "logs", "train", "scalars.jsonl")), read_scalars(os.path.join(results, "logs", "val", "scalars.jsonl"))
    assert tr and va and all(np.isfinite(s["value"]) for s in tr + va if s["tag"] != "Segmentation/MCC")
    return [(s["tag"], s["step"], s["value"]) for s in tr]


def test_cli_photo_aug_trains_is_seeded_and_live(tmp_path):
    """A seeded 160 x 192 scene, -ps 64, stride 32 without the five copies: 20 windows, 16 of them trained on in four steps of one
    epoch.  --photo_aug yes runs to the end; twice with one seed it logs identical training scalars, and other ones than without
    the flag; the validation loader of the flagged run holds the windows of the unflagged one and no photo table."""
    img, cls = blob_scene(200, 160, 192)
    root = str(tmp_path / "scenes")
    scenes.save_scene_dir(root, ["tile"], [img], [cls])
    on = ["--scene_dataset", "yes", "--photo_aug", "yes"]
    first = run_cli(str(tmp_path / "a"), root, on)
    second = run_cli(str(tmp_path / "b"), root, on)
    plain = run_cli(str(tmp_path / "c"), root, ["--scene_dataset", "yes"])
    assert first == second
    assert [t[:2] for t in first] == [t[:2] for t in plain]
    losses = [k for k, t in enumerate(first) if t[0].endswith("/Loss")]
    assert losses and all(first[k][2] != plain[k][2] for k in losses), (first, plain)

    refused = run_cli(str(tmp_path / "d"), root, ["--photo_aug", "yes"], expect_ok=False)
    assert refused.returncode != 0 and "--photo_aug yes jitters windows of resident scenes: it needs --scene_dataset yes" in refused.stderr

    import train_ISPRS as cli
    cpu = scenes.ScenePool([img], [cls], patch=64, device="cpu")
    table = scenes.window_table(cpu.shapes, 64, 32, False)
    names, _ = cli.list_scene_dataset(len(table))
    x_tr, x_va = names[:16], names[16:]
    loaders = {}
    for flag in ("yes", "no"):
        args = cli.build_parser().parse_args(["--scene_dataset", "yes", "--photo_aug", flag, "-ps", "64", "--seed", "5"])
        loaders[flag] = cli.scene_loaders(args, cpu, table, x_tr, x_va, 4)
    for (a, _), (b, _) in zip(loaders["yes"][1], loaders["no"][1]):
        assert a.photo is None and b.photo is None and np.array_equal(a.rows, b.rows)
    for (a, _), (b, _) in zip(loaders["yes"][0], loaders["no"][0]):
        assert a.photo is not None and b.photo is None and np.array_equal(a.rows, b.rows)
