"""GPU tests of the drop-in surface: committed goldens (no oracle at run time), the Keras-style API, checkpoints,
the CLI end to end on a synthetic dataset in the reference's on-disk format, and data-parallel semantics
(one GPU emulating two MirroredStrategy replicas) against the oracle."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADS = ["seg", "bound", "dist", "color"]


def rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-12))


def test_golden_tiny_multitask_fp32():
    """HIP path vs tests/golden/tiny_multitask.npz.  The golden holds the oracle's weights seed, not the weights;
    the weights are regenerated with the same glorot/numpy recipe (oracle/make_golden.py)."""
    from oracle import resuneta_ref as ref            # only for the seeded initial weights
    from resunet_a_mltsk_keras_amd import _lib as L
    from resunet_a_mltsk_keras_amd.engine import Engine, LossSpec, ModelConfig
    g = np.load(os.path.join(ROOT, "tests", "golden", "tiny_multitask.npz"))
    params, _ = ref.init_params(ref.RefConfig(input_shape=(64, 64, 6), num_classes=6, multitasking=True), int(g["seed"]))
    eng = Engine(ModelConfig(input_shape=(64, 64, 6), num_classes=6, multitasking=True), dtype="f32", split_k=False)
    eng.compile(LossSpec(kind={h: L.LOSS_TANIMOTO for h in HEADS}, weight=dict(zip(HEADS, g["loss_weights"].tolist()))))
    eng.set_weights({k: v.numpy() for k, v in params.items()})
    pred = eng.predict(g["x"])
    for h in HEADS:
        assert np.abs(pred[h] - g["pred_eval_" + h]).max() < 1e-4, h
    gr = eng.forward_backward(g["x"], {h: g["y_" + h] for h in HEADS})
    torch.cuda.synchronize()
    res = eng._results(gr)
    assert np.allclose(res[:5], g["losses"], rtol=1e-3, atol=1e-5)
    for h, z in eng.logits(True, 2).items():
        assert rel(z, g["logits_" + h]) < 1e-3, h
    grads = eng.grads_keras()
    for name, s in zip(g["grad_names"], g["grad_abs_sums"]):
        assert abs(float(np.abs(grads[str(name)]).sum()) - s) < 5e-3 * s, name


def test_loss_factories_evaluate_on_gpu():
    from multitasking_utils import Tanimoto_dual_loss
    from utils import weighted_categorical_crossentropy
    k = np.load(os.path.join(ROOT, "tests", "golden", "tanimoto_kat.npz"))
    f = Tanimoto_dual_loss()
    assert np.allclose(f(k["y_swap"], k["p_swap"]), k["l_swap"], rtol=1e-5)
    assert np.allclose(f(k["y_rand"], k["p_rand"]), k["l_rand"], rtol=1e-5)
    y = np.eye(3, dtype=np.float32)[np.array([[[0, 1], [2, 0]]])]
    p = np.full_like(y, 1 / 3)
    w = [0.5, 2.0, 10.0]
    out = weighted_categorical_crossentropy(w)(y, p)
    assert out.shape == (1, 2, 2) and np.allclose(out, (y * w).sum(-1) * np.log(3), rtol=1e-6)


def test_standalone_tanimoto_loss_matches_reference_definition():
    """multitasking_utils.py:38-68 `Tanimoto_loss(label, pred)` -> (B,), weights from the LABEL volumes, inf -> largest finite
    weight (:46-53), all-inf -> 1e-5/1e-5; on the GPU through rua_tanimoto_sums + rua_tanimoto_ratio, against both CPU
    restatements and the hand computation of tests/test_oracle_kat.py."""
    from multitasking_utils import Tanimoto_dual_loss, Tanimoto_loss
    from oracle import naive_ops as nv
    rng = np.random.default_rng(4)
    ids = rng.integers(0, 2, size=(3, 16, 16))
    y = np.eye(3, dtype=np.float32)[ids]                       # class 2 absent everywhere -> its weight = max finite weight
    p = rng.uniform(0.05, 0.95, y.shape).astype(np.float32)
    got = Tanimoto_loss(y, p)
    assert got.shape == (3,) and np.allclose(got, nv.tanimoto_loss(y, p), rtol=1e-5)
    v = y.sum(axis=(1, 2)).mean(axis=0)
    w = np.array([1 / v[0] ** 2, 1 / v[1] ** 2, 0]); w[2] = w[:2].max()
    sp, ss = (p * y).sum(axis=(1, 2)), (p ** 2 + y ** 2).sum(axis=(1, 2))
    assert np.allclose(got, ((w * sp).sum(-1) + 1e-5) / ((w * (ss - sp)).sum(-1) + 1e-5), rtol=1e-5)
    z = np.zeros((2, 8, 8, 3), np.float32)
    assert np.allclose(Tanimoto_loss(z, z), 1.0)
    # the dual is built from it exactly as the reference does (:79-84), with the swapped first term
    dual = 1.0 - 0.5 * (Tanimoto_loss(p, y) + Tanimoto_loss(1 - y, 1 - p))
    assert np.allclose(Tanimoto_dual_loss()(y, p), dual, rtol=1e-5, atol=1e-6)


class Args:
    multitasking = True
    gpu_parallel = False
    dtype = "f32"


def test_keras_style_model_roundtrip(tmp_path):
    from ResUnet_a.model2 import Resunet_a
    from multitasking_utils import Tanimoto_dual_loss
    from utils import Adam, K, load_model
    from resunet_a_mltsk_keras_amd.synthetic import make_batch
    net = Resunet_a((64, 64, 3), 4, Args())
    assert (net.num_classes, net.img_height, net.img_width, net.img_channel) == (4, 64, 64, 3)
    model = net.model
    lines = []
    model.summary(print_fn=lines.append)
    assert any("conv2d_1/kernel" in l for l in lines) and "Total params" in lines[-1]
    loss = Tanimoto_dual_loss()
    model.compile(optimizer=Adam(lr=1e-3, beta_1=0.9), loss={h: loss for h in HEADS},
                  loss_weights={"seg": 1.0, "bound": 1.0, "dist": 1.0, "color": 1.0}, metrics={"seg": ["accuracy"]})
    assert model.metrics_names[:5] == ["loss", "seg_loss", "bound_loss", "dist_loss", "color_loss"] and len(model.metrics_names) == 10
    assert model.output_names == HEADS
    x, y = make_batch(2, 64, 3, 4, True, seed=2, block=16)
    first = model.train_on_batch(x=x, y=y, return_dict=False)
    assert len(first) == 10 and all(np.isfinite(first))
    for _ in range(5):
        last = model.train_on_batch(x, y)
    assert last[0] < first[0]                                  # the same batch gets easier
    ev = model.test_on_batch(x=x, y=y)
    assert len(ev) == 10
    pred = model.predict(x, batch_size=1)
    assert set(pred) == set(HEADS) and pred["seg"].shape == (2, 64, 64, 4) and pred["color"].shape == (2, 64, 64, 3)
    assert np.allclose(pred["seg"].sum(-1), 1.0, atol=1e-5)
    for _ in range(2):                                         # later calls replay the captured inference forward
        again = model.predict(x, batch_size=1)
        assert all(np.array_equal(again[h], pred[h]) for h in HEADS)
    assert model.engine._captured_eval.get(1) not in (None, False)
    path = str(tmp_path / "best_model.h5")
    model.save(path)
    m2 = load_model(path)
    assert K.get_value(m2.optimizer.lr) == pytest.approx(1e-3)
    K.set_value(m2.optimizer.lr, 5e-4)
    p2 = m2.predict(x, batch_size=2)
    assert np.abs(p2["seg"] - pred["seg"]).max() < 1e-6
    a = m2.train_on_batch(x, y)
    b = model.train_on_batch(x, y)
    assert abs(a[0] - b[0]) < 1e-4                             # same state (weights, Adam moments, step count) continues
    m3 = load_model(path, compile=False)
    assert np.abs(m3.predict(x)["dist"] - pred["dist"]).max() < 1e-6
    # weight exchange with the reference: .npz of Keras variable names, layer numbers shifted as in a
    # Keras process that built another model first
    w = m3.get_weights_dict()
    shifted = {}
    for k, v in w.items():
        layer, var = k.rsplit("/", 1)
        base, _, idx = layer.rpartition("_")
        n = int(idx) if base and idx.isdigit() else 0
        base = base if base and idx.isdigit() else layer
        shifted[f"{base}_{n + 7}/{var}:0"] = v
    np.savez(str(tmp_path / "from_keras.npz"), **shifted)
    net4 = Resunet_a((64, 64, 3), 4, Args())
    net4.model.load_weights(str(tmp_path / "from_keras.npz"))
    assert np.abs(net4.model.predict(x)["seg"] - m3.predict(x)["seg"]).max() < 1e-6
    net4.model.save_weights(str(tmp_path / "to_keras.npz"))
    with np.load(str(tmp_path / "to_keras.npz")) as z:
        assert set(z.files) == {k + ":0" for k in w} and all(np.array_equal(z[k + ":0"], w[k]) for k in w)
    # the same exchange through real HDF5 in Keras' own layout (h5lite, no h5py): a file "Keras wrote" (shifted layer
    # numbers, no metadata of ours) -> load_model reads the configuration off the variables; save_weights -> Keras layout
    from resunet_a_mltsk_keras_amd import h5lite
    root = h5lite.Group({"keras_version": b"2.4.0", "backend": b"tensorflow"})
    root.children["model_weights"] = h5lite.keras_group_from_weights(shifted)
    h5lite.write_h5(str(tmp_path / "from_keras.h5"), root)
    m5 = load_model(str(tmp_path / "from_keras.h5"), compile=False, input_shape=(64, 64, 3), dtype="f32")
    assert (m5.cfg.num_classes, m5.cfg.multitasking, m5.cfg.variant) == (4, True, "model2")
    assert np.abs(m5.predict(x)["seg"] - m3.predict(x)["seg"]).max() < 1e-6
    net4.model.save_weights(str(tmp_path / "to_keras.h5"))
    back = h5lite.keras_weights_from_group(h5lite.read_h5(str(tmp_path / "to_keras.h5")))
    assert set(back) == {k + ":0" for k in w} and all(np.array_equal(back[k + ":0"], w[k]) for k in w)
    ck = h5lite.read_h5(path)                                  # model.save(): Keras weight layout + our metadata + optimizer moments
    assert "rua_checkpoint" in ck.attrs and "model_weights" in ck and ck["optimizer_weights/rua/m:0"].dtype == np.float32
    import pickle
    bad = str(tmp_path / "pickled.h5")
    pickle.dump({"weights": 1}, open(bad, "wb"))
    with pytest.raises(ValueError, match="not an HDF5 file"):  # nothing is ever unpickled
        load_model(bad)


def test_cli_end_to_end_on_synthetic_dataset(tmp_path):
    sys.path.insert(0, ROOT)
    import train_ISPRS as cli
    from resunet_a_mltsk_keras_amd.synthetic import make_batch
    x, y = make_batch(10, 64, 3, 4, True, seed=3, block=16)
    ds = tmp_path / "ds"
    os.makedirs(ds / "train")
    for h in HEADS:
        os.makedirs(ds / "labels" / h)
    for i in range(10):
        np.save(ds / "train" / f"patch_{i}.npy", x[i])
        for h in HEADS:
            np.save(ds / "labels" / h / f"patch_{i}.npy", y[h][i])
    rp = tmp_path / "run"
    cli.main(["--resunet_a", "True", "--multitasking", "True", "--loss", "tanimoto", "-dp", str(ds), "-rp", str(rp), "-bs", "2",
              "--epochs", "2", "-ps", "64", "--num_classes", "4", "--dtype", "f32"])
    assert os.path.exists(rp / "best_model.h5")
    lines = open(rp / "logs" / "val" / "scalars.jsonl").read().strip().splitlines()
    tags = {__import__("json").loads(l)["tag"] for l in lines}
    assert {"Segmentation/Loss", "Boundary/Loss", "Distance/Loss", "Color/Loss", "Total/Loss", "Segmentation/MCC"} <= tags
    from utils import load_model
    m = load_model(str(rp / "best_model.h5"), compile=False)
    assert m.predict(x[:1])["seg"].shape == (1, 64, 64, 4)


def test_two_replica_semantics_on_one_gpu():
    """MirroredStrategy semantics (train_ISPRS.py:347,432): every replica normalises with its OWN batch statistics
    and its OWN Tanimoto class volumes; gradients are summed and divided by the replica count.  One GPU plays both
    replicas (gradients accumulate in the flat buffer) and is compared with the oracle doing the same on the CPU."""
    from oracle import resuneta_ref as ref
    from resunet_a_mltsk_keras_amd import _lib as L
    from resunet_a_mltsk_keras_amd.engine import Engine, LossSpec, ModelConfig
    from resunet_a_mltsk_keras_amd.synthetic import make_batch
    shape, C = (64, 64, 3), 4
    rcfg = ref.RefConfig(input_shape=shape, num_classes=C, multitasking=True)
    params, order = ref.init_params(rcfg, 11)
    lw = {h: 1.0 for h in HEADS}
    eng = Engine(ModelConfig(input_shape=shape, num_classes=C, multitasking=True), dtype="f32", split_k=False)
    eng.compile(LossSpec(kind={h: L.LOSS_TANIMOTO for h in HEADS}, weight=lw, optimizer="sgd", lr=0.05, momentum=0.8))
    eng.set_weights({k: v.numpy() for k, v in params.items()})
    x, y = make_batch(4, 64, 3, C, True, seed=21, block=16)
    shards = [(x[:2], {h: v[:2] for h, v in y.items()}), (x[2:], {h: v[2:] for h, v in y.items()})]
    losses = []
    for xs, ys in shards:                                   # replica r: local forward/backward, G accumulates
        g = eng.forward_backward(xs, ys)
        torch.cuda.synchronize()
        losses.append(eng._results(g)[0])
    eng.optimizer_step(grad_scale=0.5)
    torch.cuda.synchronize()
    # oracle: mean of the two replica losses, each from its own training-mode forward
    p = {k: v.clone() for k, v in params.items()}
    for k in order:
        p[k].requires_grad_(True)
    tot, exp_losses = 0, []
    for xs, ys in shards:
        tr = ref.RefTrainer(rcfg, p, order, ref.CompileSpec(loss="tanimoto", loss_weights=lw))
        total, vals, _, _ = tr._losses(xs, ys, training=True)
        tot = tot + 0.5 * total
        exp_losses.append(float(total.detach()))
    tot.backward()
    assert np.allclose(losses, exp_losses, rtol=1e-3)
    w = eng.get_weights()
    worst = 0.0
    for k in order:
        e = (p[k].detach() - 0.05 * p[k].grad).numpy()        # first SGD-momentum step: v = -lr*g
        worst = max(worst, float((np.abs(w[k] - e).max() - 1e-6) / (np.abs(e).max() + 1e-6)))
    assert worst < 2e-3, worst


def _run_ranks(tmp_path, tag, extra=()):
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    out = tmp_path / tag
    os.makedirs(out)
    worker = os.path.join(ROOT, "tests", "_dp_rank_worker.py")
    procs = [subprocess.Popen([sys.executable, worker, str(r), "2", str(port), str(out), *extra], stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT) for r in range(2)]
    logs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=420)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        logs.append(o.decode(errors="replace"))
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)
    return [np.load(out / f"rank{r}.npz") for r in range(2)]


def test_two_process_data_parallel_engine(tmp_path):
    """Two real ranks (two processes sharing cuda:0, gloo host-staged collectives) against one process playing both
    MirroredStrategy replicas (train_ISPRS.py:347,432): rank-0 weights broadcast, local BN statistics / Tanimoto volumes,
    gradients summed / world, BN moving statistics averaged, and the returned metrics replica-aggregated and IDENTICAL on
    both ranks (reference :280-292 takes one decision from them).  Then resume from a checkpoint under DP (-cp path)."""
    from resunet_a_mltsk_keras_amd import _lib as L
    from resunet_a_mltsk_keras_amd.engine import Engine, LossSpec, ModelConfig
    from resunet_a_mltsk_keras_amd.synthetic import make_batch
    r0, r1 = _run_ranks(tmp_path, "fresh")
    assert np.array_equal(r0["res"], r1["res"]) and np.array_equal(r0["ev"], r1["ev"])        # same numbers on every rank
    assert np.array_equal(r0["P"], r1["P"]) and np.array_equal(r0["S"], r1["S"])              # replicas stay in lock-step
    # single process emulating the two replicas, from rank 0's initial weights (seed 11)
    C = 4
    lw = {h: 1.0 for h in HEADS}
    eng = Engine(ModelConfig(input_shape=(64, 64, 3), num_classes=C, multitasking=True), dtype="f32", seed=11, split_k=False)
    eng.compile(LossSpec(kind={h: L.LOSS_TANIMOTO for h in HEADS}, weight=lw, optimizer="sgd", lr=0.05, momentum=0.8))
    x, y = make_batch(4, 64, 3, C, True, seed=21, block=16)
    shards = [(x[:2], {h: v[:2] for h, v in y.items()}), (x[2:], {h: v[2:] for h, v in y.items()})]
    exp = []
    for _ in range(2):
        S0, Ss, rs = eng.S.clone(), [], []
        for xs, ys in shards:
            eng.S.copy_(S0)
            g = eng.forward_backward(xs, ys)
            torch.cuda.synchronize()
            rs.append(eng._results(g)); Ss.append(eng.S.clone())
        eng.S.copy_((Ss[0] + Ss[1]) / 2)
        eng.optimizer_step(grad_scale=0.5)
        rs = np.asarray(rs)
        exp.append(np.concatenate([rs[:, :6].mean(0), rs[:, 6:].sum(0)]))     # losses + accuracy: mean; TP/FP/TN/FN: summed
    torch.cuda.synchronize()
    assert np.allclose(r0["res"], np.asarray(exp), rtol=2e-5, atol=1e-6), (r0["res"], exp)
    P = eng.P.cpu().numpy()
    assert np.abs(P - r0["P"]).max() < 1e-5 * max(1.0, np.abs(P).max())
    assert np.abs(eng.S.cpu().numpy() - r0["S"]).max() < 1e-5
    ev = [eng.test_step(xs, ys) for xs, ys in shards]
    ev = np.asarray(ev)
    assert np.allclose(r0["ev"], np.concatenate([ev[:, :6].mean(0), ev[:, 6:].sum(0)]), rtol=2e-5, atol=1e-6)
    # resume: only the file is shared; every rank restores it, attaches DP, rank 0's state wins, training continues in step
    from resunet_a_mltsk_keras_amd import keras_api as ka
    m = ka.Model(ModelConfig(input_shape=(64, 64, 3), num_classes=C, multitasking=True), dtype="f32", seed=11)
    m.compile(optimizer=ka.SGD(lr=0.05, momentum=0.8), loss={h: ka.Tanimoto_dual_loss() for h in HEADS}, loss_weights=lw)
    m.engine.split_k = False
    m.engine.P.copy_(torch.from_numpy(r0["P"])); m.engine.S.copy_(torch.from_numpy(r0["S"]))
    m.engine.M1.copy_(torch.from_numpy(r0["M1"])); m.engine.t = int(r0["t"])
    ck = str(tmp_path / "resume.h5")
    m.save(ck)
    q0, q1 = _run_ranks(tmp_path, "resumed", extra=(ck,))
    assert np.array_equal(q0["res"], q1["res"]) and np.array_equal(q0["P"], q1["P"])
    assert int(q0["t"]) == int(r0["t"]) + 2
    assert q0["res"][0][0] < r0["res"][0][0]                   # continues from the trained state, not from a fresh init


def test_data_parallel_graph_pieces_match_single_process_step():
    """The N>1 fast path (backward cut into HIP graphs at gradient-bucket boundaries, RCCL all-reduces issued between
    the replays) must compute the same steps as the whole-step graph.  A one-rank RCCL group exercises the real
    collectives and stream fences on the single GPU of the test box."""
    import torch.distributed as dist
    from resunet_a_mltsk_keras_amd import _lib as L
    from resunet_a_mltsk_keras_amd.dist import DataParallel
    from resunet_a_mltsk_keras_amd.engine import Engine, LossSpec, ModelConfig
    from resunet_a_mltsk_keras_amd.synthetic import make_batch
    shape, C = (64, 64, 3), 4
    lw = {h: 1.0 for h in HEADS}
    spec = lambda: LossSpec(kind={h: L.LOSS_TANIMOTO for h in HEADS}, weight=lw, optimizer="sgd", lr=0.02, momentum=0.8)
    x, y = make_batch(4, 64, 3, C, True, seed=5, block=16)
    a = Engine(ModelConfig(input_shape=shape, num_classes=C, multitasking=True), dtype="f32", seed=3, split_k=False)
    a.compile(spec())
    la = [a.train_step(x, y)[0] for _ in range(4)]
    created = not dist.is_initialized()
    if created:
        dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29541", rank=0, world_size=1)
    try:
        b = Engine(ModelConfig(input_shape=shape, num_classes=C, multitasking=True), dtype="f32", seed=3, split_k=False)
        b.compile(spec())
        b.dp_graph = True                                         # opt-in path (default: eager launches)
        dp = DataParallel(b, bucket_mb=4.0)                       # small buckets => several pieces
        assert len(dp.buckets) > 3
        lb = [b.train_step(x, y)[0] for _ in range(4)]
        assert len(b._captured_dp[4]) > 2                         # really went through the piecewise path
        torch.cuda.synchronize()
        assert np.allclose(la, lb, rtol=2e-4), (la, lb)
        pa, pb = a.P.cpu().numpy(), b.P.cpu().numpy()          # same bar as test_graph_replay_equals_eager_launches:
        d = np.abs(pa - pb)                                      # atomic-order noise only, no systematic difference
        assert d.mean() < 1e-4 * np.abs(pa).mean() and d.max() < 2e-3, (float(d.mean()), float(d.max()))
        # back-to-back replays with nothing fetched in between (what bench.py and a fed training loop do): graph launches
        # directly followed by the collectives' stream events corrupted steps on this stack until an eager kernel was put
        # between them (engine._graph_step_dp); the parameters must stay finite and the loss must keep falling
        for _ in range(24):
            b.train_step(None, None, fetch=False)
        torch.cuda.synchronize()
        last = b._results(b.graph(4, True))[0]
        assert bool(torch.isfinite(b.P).all()) and bool(torch.isfinite(b.S).all()) and np.isfinite(last) and last < lb[-1]
    finally:
        if created:
            dist.destroy_process_group()


def _ints(v):
    """Every integer reachable from a recorded launch argument: plain ints, ctypes structs (passed by reference) and arrays."""
    import ctypes
    if isinstance(v, int):
        yield v
    elif isinstance(v, (tuple, ctypes.Array)):
        for e in v:
            yield from _ints(e)
    elif isinstance(v, ctypes.Structure):
        for f in v._fields_:
            yield from _ints(getattr(v, f[0]))
    elif hasattr(v, "_obj"):                                     # ctypes.byref(struct)
        yield from _ints(v._obj)


def test_data_parallel_bucket_hooks_follow_the_last_gradient_writer():
    """Under data parallel a bucket's all-reduce is issued right after the last backward launch that writes into it: not earlier (it would
    read unwritten gradients), not later (overlap lost).  Which launch writes which gradient is read off the recorded arguments themselves -
    every pointer into the gradient arena a launch passes, its descriptors and the batched reductions' tables included - not off the
    recorder's bookkeeping.  Buckets of the default size, and one bucket per parameter entry; the cfg3 layout in bf16 and the cfg4 layout
    (depth 7, C = 2048) in fp32.  Nothing runs: the plans are only recorded."""
    import gc
    import torch.distributed as dist
    from resunet_a_mltsk_keras_amd import _lib as L
    from resunet_a_mltsk_keras_amd.dist import DataParallel
    from resunet_a_mltsk_keras_amd.engine import Engine, LossSpec, ModelConfig
    created = not dist.is_initialized()
    if created:
        dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29543", rank=0, world_size=1)
    try:
        for size, depth, dtype, B in ((256, 6, "bf16", 8), (512, 7, "f32", 1)):
            eng = Engine(ModelConfig(input_shape=(size, size, 6), num_classes=6, multitasking=True, depth=depth), dtype=dtype)
            eng.compile(LossSpec(kind={h: L.LOSS_TANIMOTO for h in HEADS}, weight={h: 1.0 for h in HEADS}))
            g0, g1 = eng.G.data_ptr(), eng.G.data_ptr() + 4 * eng.params.n
            for kw in ({}, {"bucket_mb": 1e-5}):                   # 1e-5 MB: every parameter entry is a bucket of its own
                dp = DataParallel(eng, **kw)
                eng.drop_plans()
                g = eng.graph(B, True)
                last = {}
                for i, (_, name, args, _) in enumerate(g.bwd.calls):
                    vals = list(_ints(args))
                    if name == "rua_wgrad_reduce_batch":         # the records of the batched reduction live in a device table
                        table = next(t for t in g.allocs if t.data_ptr() == args[0])
                        vals += list(_ints((L.WgradPending * args[1]).from_buffer_copy(table.cpu().numpy().tobytes())))
                    for v in vals:
                        if g0 <= v < g1:
                            last[dp.bucket_of((v - g0) // 4)] = i
                hook = {b: i for i, bs in eng._bucket_marks(g).items() for b in bs}
                bad = {b: (hook.get(b), last.get(b)) for b in set(hook) | set(last) if hook.get(b) != last.get(b)}
                assert not bad, (size, dtype, kw, sorted(bad.items())[:8])
                # every bucket gets its hook, except one that holds nothing but the bias of a convolution followed by a training-mode
                # BatchNorm: that gradient is exactly zero and no launch writes it (the arena's zeros are reduced at the end of the step)
                unwritten = [e["name"] for e in eng.params.entries if dp.bucket_of(e["off"]) not in hook]
                assert all(n.endswith("/bias") for n in unwritten), (size, dtype, kw, unwritten[:8])
                if not kw:
                    assert not unwritten, (size, dtype, unwritten[:8])
            del eng, g, dp
            gc.collect()
            torch.cuda.empty_cache()
    finally:
        if created:
            dist.destroy_process_group()


def test_evaluation_script_end_to_end(tmp_path):
    """test_ISPRS.py: tile -> predict -> argmax -> metrics -> mosaic on a synthetic test tile; the numbers must
    equal what the same model gives through predict() directly."""
    import importlib.util
    from ResUnet_a.model2 import Resunet_a
    spec = importlib.util.spec_from_file_location("eval_isprs", os.path.join(ROOT, "test_ISPRS.py"))
    ev = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ev)

    class A:
        multitasking = True
        gpu_parallel = False
    ps, ncls = 64, 5
    net = Resunet_a((ps, ps, 3), ncls, A()).model
    path = str(tmp_path / "m.h5")
    net.save(path)
    rng = np.random.default_rng(0)
    colours = np.array([eval(k) for k in ev.LABEL_DICT], np.uint8)
    cls = rng.integers(0, 5, size=(2 * ps + 10, 3 * ps))                       # 2 x 3 patches + a border that is dropped
    os.makedirs(tmp_path / "data")
    np.save(tmp_path / "data" / "Image_Test.npy", rng.integers(0, 256, size=(3,) + cls.shape).astype(np.uint8))
    np.save(tmp_path / "data" / "Reference_Test.npy", colours[cls].transpose(2, 0, 1))
    out = ev.main(["--use_multitasking", "--model_path", path, "--dataset_path", str(tmp_path / "data"), "-ps", str(ps),
                   "--num_classes", str(ncls), "--output_path", str(tmp_path / "preds")])
    img = np.load(tmp_path / "data" / "Image_Test.npy").astype(np.float32).transpose(1, 2, 0) / 255.0
    patches = ev.extract_patches_train(img, ps)
    direct = np.argmax(net.predict(patches, batch_size=2)["seg"], axis=-1)
    ref = ev.extract_patches_test(cls.astype(np.uint8), ps)
    assert out["accuracy"] == pytest.approx(100.0 * (direct.reshape(-1) == ref.reshape(-1)).mean(), abs=1e-9)
    mosaic = np.load(tmp_path / "preds" / "pred_seg_reconstructed.npy")
    assert mosaic.shape == cls.shape and np.array_equal(mosaic[:ps, ps:2 * ps], direct[1])
    assert out["confusion_matrix"].sum() == 6 * ps * ps
    assert os.path.getsize(tmp_path / "preds" / "pred_seg_reconstructed.ppm") > 3 * cls.size
    assert np.load(tmp_path / "preds" / "pred_color.npy").shape == (6, ps, ps, 3)


def test_bench_plain_line_and_dumped_outputs(tmp_path):
    """bench.py without --full: the headline fields only, exactly --steps timed steps, and --dump-outputs writes the last
    timed step's arrays (float32 / float64, under 64 MB); two runs with the same arguments see the same inputs."""
    import json
    import subprocess
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    dumps = []
    for run in ("a", "b"):
        d = tmp_path / run
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "2",
                            "--dump-outputs", str(d)], env=env, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-3000:]
        lines = [l for l in p.stdout.splitlines() if l.strip()]
        assert len(lines) == 1, lines
        got = json.loads(lines[0])
        for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert k in got, k
        assert got["steps"] == 3 and got["timed_blocks"] == 1 and got["ms_per_step"] > 0 and got["value"] > 0
        assert not {"roofline", "also", "cpu_baseline", "dp"} & set(got)
        files = sorted(os.listdir(d))
        assert files == sorted(["metrics.npy", "params.npy", "bn_state.npy"] + [f"head_{h}.npy" for h in HEADS]), files
        arrs = {f[:-4]: np.load(d / f) for f in files}
        assert sum(os.path.getsize(d / f) for f in files) <= 64 << 20
        assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in arrs.values())
        assert arrs["metrics"].dtype == np.float64 and np.isclose(arrs["metrics"][0], got["config"]["loss_last_step"], atol=1e-5)
        dumps.append(arrs)
    # same inputs, and the dumped step starts from the initial training state in both runs (bench.py TrainState): the runs agree
    # to the rounding of one step (measured: bit-identical but for a few updated parameters whose gradient is a sum that
    # cancels to ~1e-9, where Adam's normalisation leaves ~1e-8 of atomic-order noise)
    a, b = dumps
    for k in a:
        scale = max(1.0, float(np.abs(a[k]).max()))
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and float(np.abs(a[k] - b[k]).max()) <= 1e-6 * scale, k
