"""Gradient accumulation under data parallel: a one-rank RCCL group (the set-up of tests/test_api_gpu.py's graph-pieces test) runs the real
reduction, the eager data-parallel step and the HIP-graph pieces with their captured optimizer tail.  One K = 2 cycle there - the hold step, then
the update step, which under the pieces is all replays, the captured optimizer tail included - equals the non-parallel engine bit for bit:
with one rank the all-reduce is the identity and grad_scale is 1.  rua_stem_bwd is pinned to one block so that the step is a function of its
inputs (tests/test_sched_engine_gpu.py explains)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from _kernel_util import bits_of  # noqa: E402
from resunet_a_mltsk_keras_amd import _lib as L  # noqa: E402
from resunet_a_mltsk_keras_amd.engine import HEADS, Engine, LossSpec, ModelConfig  # noqa: E402
from resunet_a_mltsk_keras_amd.synthetic import make_batch  # noqa: E402

SHAPE, NCLS, BATCH = (64, 64, 3), 4, 2


def engine():
    eng = Engine(ModelConfig(input_shape=SHAPE, num_classes=NCLS, multitasking=True, width=32), dtype="f32", seed=4, split_k=False)
    eng.compile(LossSpec(kind={h: L.LOSS_TANIMOTO for h in HEADS}, weight={h: 1.0 for h in HEADS}, lr=1e-3, gradient_accumulation_steps=2,
                         global_clipnorm=1.0))
    return eng


def bits(eng):
    torch.cuda.synchronize()
    return [bits_of(t).copy() for t in (eng.P, eng.M1, eng.V1, eng.S, eng.A)]


@pytest.fixture
def one_block_stem():
    lib = L.lib()
    before = lib.get_tuning("stem_blocks")
    lib.set_tuning(stem_blocks=1)
    yield
    lib.set_tuning(stem_blocks=before)


@pytest.mark.parametrize("pieces", [False, True], ids=["eager", "graph_pieces"])
def test_one_cycle_under_a_one_rank_group_equals_the_single_engine(pieces, one_block_stem):
    import torch.distributed as dist
    from resunet_a_mltsk_keras_amd.dist import DataParallel
    batches = [make_batch(BATCH, SHAPE[0], SHAPE[2], NCLS, True, seed=300 + k, block=16) for k in range(2)]
    a = engine()
    ref = []
    for x, y in batches:
        a.train_step(x, y, fetch=False)
        ref.append(bits(a))
    assert a.t == 1
    created = not dist.is_initialized()
    if created:
        dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29547", rank=0, world_size=1)
    try:
        b = engine()
        b.dp_graph = pieces
        DataParallel(b, bucket_mb=4.0)
        for k, (x, y) in enumerate(batches):                                       # with the pieces: an eager step and the captures, then replays
            before = bits(b)
            b.train_step(x, y, fetch=False)
            got = bits(b)
            for name, u, v in zip(("P", "M1", "V1", "S", "A"), got, ref[k]):
                assert (u == v).all(), (pieces, k, name)
            if k % 2 == 0:
                assert all((u == v).all() for u, v in zip(got[:3], before[:3]))    # the hold step
        assert b.t == 1 and b.accumulation_state() == dict(steps=2, micro=0)
        assert (not pieces) or (BATCH in b._captured_dp and b._opt_graph is not None)
        rep = b.clip_report()
        assert rep == a.clip_report() and rep["skipped"] == 0 and rep["norm"] > 0  # the same bits went into the same finisher
    finally:
        if created:
            dist.destroy_process_group()
