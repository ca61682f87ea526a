"""The batched form of rua_conv_wgrad_group (rua_wgrad_desc.batch) and the engine's deferral of a step's generic-tile weight
gradients to ONE launch in front of each flush (WgradQueue.hold_back).

Library level: the member shapes are read off the recorded cfg3 bf16 backward plan.  With bit 5 of the tuning key wgrad_group
(every member keeps the K split it would take alone) a batch equals the single launches bit for bit; with the default split
(one block budget dealt by work) each dW is held to the bound test_kernels_gpu.py::test_conv_wgrad holds this kernel to:
2e-2 of the output scale against a float64 host product of the bf16-rounded operands.

Model level: deferral on against deferral off.  With bit 5 the flat gradient buffer after forward_backward() is bitwise equal -
the liveness proof: an operand overwritten between the recorded position and the batch would show here.  One exception, which is
the parent's and not the deferral's: the stem's weight and bias gradient (rua_stem_bwd_fold behind a ticketed wgrad_pw launch, or
rua_stem_bwd) is added with float atomics and is not reproducible between two runs of the SAME engine - measured on cfg2, two
runs with the deferral off: 197 of its 224 elements differ, by at most 5.8e-10 (scale 2e-4), every other element of the 42 M is
bit-identical.  Nothing reads the stem's gradient during the backward, so those 224 elements are held to fp32 summation noise (1e-5
of the buffer's scale, the bound of test_first_writer_overwrite_step_equals_the_accumulating_backward) and every other element
to bitwise equality.  With the default split one training step agrees like the fused / materialised twins of test_model_gpu.py
(losses 2e-3, logits 5e-2 of scale)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from resunet_a_mltsk_keras_amd import _lib as L  # noqa: E402
from resunet_a_mltsk_keras_amd.engine import Engine, LossSpec, ModelConfig  # noqa: E402
from resunet_a_mltsk_keras_amd.synthetic import make_batch  # noqa: E402

HEADS = ["seg", "bound", "dist", "color"]
KEEP_OWN_SPLIT = 32                                          # bit 5 of the tuning key wgrad_group
TOL_BF16 = 2e-2                                              # tests/test_kernels_gpu.py: tol(RUA_BF16)
STEP_DISPATCHES_BEFORE, MEMBERS_BEFORE = 266, 23             # the cfg3 bf16 step with one launch per generic-tile weight gradient

# name -> (input shape, classes, multitask, batch, depth, variant)
MODELS = {
    "cfg3": ((256, 256, 6), 6, True, 8, 6, "model2"),
    "cfg2": ((256, 256, 6), 6, False, 8, 6, "model2"),
    "cfg5": ((128, 128, 7), 2, False, 32, 6, "model2"),
    "d7_small": ((512, 512, 6), 6, True, 1, 7, "model2"),      # depth 7 needs 512-pixel patches (the 8-window of the PSPPooling on the bottleneck): small = batch 1
    "model_py": ((128, 128, 7), 6, False, 4, 6, "model"),
}


def dev():
    return torch.device("cuda", 0)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def rel_err(got, exp):
    got = np.asarray(got, np.float64); exp = np.asarray(exp, np.float64)
    return float(np.abs(got - exp).max() / (np.abs(exp).max() + 1e-12))


class tuning:
    """wgrad_group with / without the keep-own-split bit for the length of a block (read when a plan is recorded AND when it runs)."""

    def __init__(self, keep_own: bool):
        self.keep_own = keep_own

    def __enter__(self):
        self.old = L.lib().get_tuning("wgrad_group")
        L.lib().set_tuning(wgrad_group=(self.old | KEEP_OWN_SPLIT) if self.keep_own else (self.old & ~KEEP_OWN_SPLIT))

    def __exit__(self, *exc):
        L.lib().set_tuning(wgrad_group=self.old)


def engine(name, batch_wgrad: bool, flush_mb=None, optimizer="sgd", lr=1e-3):
    shape, ncls, mt, B, depth, variant = MODELS[name]
    eng = Engine(ModelConfig(input_shape=shape, num_classes=ncls, multitasking=mt, depth=depth, variant=variant), dtype="bf16", seed=0)
    eng.batch_wgrad = batch_wgrad
    if flush_mb is not None:
        eng.flush_bytes = int(flush_mb * (1 << 20))
    heads = HEADS if mt else ["seg"]
    eng.compile(LossSpec(kind={h: L.LOSS_TANIMOTO for h in heads}, weight={h: 1.0 for h in heads}, optimizer=optimizer, lr=lr))
    x, y = make_batch(B, shape[0], shape[2], ncls, mt, seed=11)
    return eng, x, y, B


def batch_calls(g):
    """(index, descriptor array, members) of the batched launches on a recorded backward plan."""
    return [(i, c[2][0], c[2][1]) for i, c in enumerate(g.bwd.calls) if c[1] == "rua_conv_wgrad_group" and g.bwd.scopes[i] == "wgrad_batch"]


def stem_mask(eng, g):
    """True on the stem's weight and bias gradient: the one float-atomic, run-to-run irreproducible writer of the backward plan."""
    m = torch.zeros(eng.params.n, dtype=torch.bool, device=eng.G.device)
    for (_, name, args, grads) in g.bwd.calls:
        if name in ("rua_stem_bwd_fold", "rua_stem_bwd"):
            cin, cout = (args[3], args[4]) if name == "rua_stem_bwd_fold" else (args[5], args[6])
            m[grads[0]:grads[0] + cin * cout] = True
            m[grads[1]:grads[1] + cout] = True
    assert 0 < int(m.sum()) <= 16 * 256 + 256
    return m


def same_but_stem_noise(a, b, mask, what):
    assert torch.isfinite(a).all() and torch.isfinite(b).all(), what
    assert torch.equal(a[~mask], b[~mask]), (what, int((a != b)[~mask].sum()), float((a - b)[~mask].abs().max()))
    scale = float(b.abs().max())
    assert float((a - b)[mask].abs().max()) <= 1e-5 * scale, (what, "stem", float((a - b)[mask].abs().max()), scale)


def release(*engs):
    for e in engs:
        e._captured = {}
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# ---- library level ---------------------------------------------------------------------------------------------------------
_SHAPES = []


def cfg3_member_shapes():
    """(N, Hs, Ws, C, H, W, Cout, stride, dil, taps) of every member of the cfg3 bf16 step's batched launch, from the recorded plan."""
    if not _SHAPES:
        eng, x, y, B = engine("cfg3", True)
        g = eng.graph(B, True)
        calls = batch_calls(g)
        assert len(calls) == 1, [c[0] for c in calls]
        _, arr, n = calls[0]
        for i in range(n):
            d = arr[i]
            assert d.batch == 1 and d.defer == 1 and d.dtype == L.RUA_BF16
            _SHAPES.append((d.N, d.Hs, d.Ws, d.C, d.H, d.W, d.Cout, d.stride, d.dil, d.taps))
        del g
        release(eng)
    return list(_SHAPES)


def host_product(a, dy, shape):
    """float64 dW [taps][Cout][C] of the bf16-rounded operands (a NHWC, dy NHWC)."""
    N, Hs, Ws, Cs, H, W, Cout, stride, dil, taps = shape
    k = 3 if taps == 9 else 1
    w = torch.zeros((Cout, Cs, k, k), dtype=torch.float64, requires_grad=True)
    yy = F.conv2d(a.float().cpu().double().permute(0, 3, 1, 2), w, None, stride=stride, padding=dil * (k // 2), dilation=dil)
    yy = yy[:, :, :H, :W]
    yy.backward(dy.float().cpu().double().permute(0, 3, 1, 2))
    return w.grad.permute(2, 3, 0, 1).reshape(taps, Cout, Cs).numpy()


class Members:
    def __init__(self, shapes, seed=0):
        lib = L.lib()
        g = torch.Generator(device="cpu").manual_seed(seed)
        self.shapes, self.keep, self.descs, self.dws = shapes, [], [], []
        for (N, Hs, Ws, Cs, H, W, Cout, stride, dil, taps) in shapes:
            a = torch.randn((N, Hs, Ws, Cs), generator=g).to(dev()).to(torch.bfloat16).contiguous()
            dy = torch.randn((N, H, W, Cout), generator=g).to(dev()).to(torch.bfloat16).contiguous()
            dw = torch.zeros((taps, Cout, Cs), dtype=torch.float32, device=dev())
            ws = torch.zeros((16 << 20) // 4, dtype=torch.float32, device=dev())
            d = L.WgradDesc()
            d.a, d.C, d.Hs, d.Ws, d.dy, d.Cout, d.H, d.W = a.data_ptr(), Cs, Hs, Ws, dy.data_ptr(), Cout, H, W
            d.N, d.stride, d.dil, d.taps, d.dtype = N, stride, dil, taps, L.RUA_BF16
            d.dw, d.workspace, d.workspace_bytes = dw.data_ptr(), ws.data_ptr(), ws.numel() * 4
            assert lib.raw("rua_wgrad_kind")(C.byref(d)) == 0 and lib.raw("rua_wgrad_img_kind")(C.byref(d)) == 0, (N, Hs, Ws, Cs, Cout)
            self.keep += [a, dy, ws]
            self.descs.append(d)
            self.dws.append(dw)

    def array(self, batch, defer=0):
        arr = (L.WgradDesc * len(self.descs))()
        for i, d in enumerate(self.descs):
            C.memmove(C.byref(arr, i * C.sizeof(L.WgradDesc)), C.byref(d), C.sizeof(L.WgradDesc))
            arr[i].batch, arr[i].defer = batch, defer
        return arr

    def take(self):
        torch.cuda.synchronize()
        out = [dw.clone() for dw in self.dws]
        for dw in self.dws:
            dw.zero_()
        return out

    def alone(self):
        for d in self.descs:
            L.lib().call("rua_conv_wgrad", C.byref(d), stream())
        return self.take()


@pytest.mark.parametrize("which", ["step", "one", "cap", "two_grids"])
def test_batch_equals_single_launches_and_the_host_product(which):
    """The members of a cfg3 step (`step`), a batch of one, a batch at the cap of one grid and one beyond it (two grids)."""
    lib = L.lib()
    shapes = cfg3_member_shapes()
    assert len(shapes) >= 1
    cap = L.RUA_MAX_WGRAD_BATCH
    assert len(shapes) <= cap                                 # a whole step fits one grid, with headroom
    if which == "one":
        shapes = shapes[:1]
    elif which == "cap":
        shapes = [shapes[i % len(shapes)] for i in range(cap)]
    elif which == "two_grids":
        shapes = [shapes[i % len(shapes)] for i in range(cap + 5)]
    m = Members(shapes)
    n = len(shapes)
    grids = (n + cap - 1) // cap
    sep = m.alone()
    # every member keeps its own K split: bit for bit the single launches
    with tuning(keep_own=True):
        lib.call("rua_conv_wgrad_group", m.array(1), n, stream())
        assert lib.raw("rua_wgrad_group_last_grids")() == grids
        got = m.take()
    for i in range(n):
        assert torch.equal(got[i], sep[i]), ("keep own split", i, shapes[i])
    # one block budget dealt by work: the kernel's own bound against the float64 host product, no looser than for the single launch
    with tuning(keep_own=False):
        lib.call("rua_conv_wgrad_group", m.array(1), n, stream())
        assert lib.raw("rua_wgrad_group_last_grids")() == grids
        got = m.take()
        lib.call("rua_conv_wgrad_group", m.array(1), n, stream())
        again = m.take()
        # deferred: the records of rua_wgrad_group_plan describe exactly the slabs the batch leaves
        arr = m.array(1, defer=1)
        recs = (L.WgradPending * n)()
        lib.call("rua_wgrad_group_plan", arr, n, recs)
        lib.call("rua_conv_wgrad_group", arr, n, stream())
        items, blocks = [], 0
        for i in range(n):
            if recs[i].kind != 0:
                assert recs[i].kind == 2 and recs[i].parts >= 2
                r = L.WgradPending.from_buffer_copy(recs[i])
                r.block_begin = blocks
                blocks += r.blocks
                items.append(r)
        if items:
            table = (L.WgradPending * len(items))(*items)
            tdev = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(dev())
            lib.call("rua_wgrad_reduce_batch", tdev.data_ptr(), len(items), blocks, stream())
        deferred = m.take()
    seen = {}
    for i in range(n):
        assert torch.equal(got[i], again[i]), ("deterministic", i, shapes[i])
        assert torch.equal(got[i], deferred[i]), ("deferred", i, shapes[i])
        if shapes[i] not in seen:                                # (repeated shapes hold other random operands, but the host product of one is enough)
            seen[shapes[i]] = True
            exp = host_product(m.keep[3 * i], m.keep[3 * i + 1], shapes[i])
            e_batch, e_alone = rel_err(got[i].cpu().numpy(), exp), rel_err(sep[i].cpu().numpy(), exp)
            print("member %2d %s: batch %.3g, alone %.3g of the output scale" % (i, shapes[i], e_batch, e_alone))
            assert e_batch < TOL_BF16, (i, shapes[i], e_batch)


def test_batch_flag_is_ignored_outside_the_batched_form():
    """rua_conv_wgrad ignores the flag, and rua_wgrad_group_plan with the keep-own-split bit is rua_wgrad_plan per member."""
    lib = L.lib()
    m = Members(cfg3_member_shapes()[:4])
    arr = m.array(1, defer=1)
    with tuning(keep_own=True):
        recs = (L.WgradPending * 4)()
        lib.call("rua_wgrad_group_plan", arr, 4, recs)
        for i in range(4):
            r = L.WgradPending()
            lib.call("rua_wgrad_plan", C.byref(arr[i]), C.byref(r))
            assert (r.kind, r.parts, r.n, r.partials, r.dw, r.blocks) == (recs[i].kind, recs[i].parts, recs[i].n, recs[i].partials, recs[i].dw, recs[i].blocks)


# ---- model level: deferral on against deferral off -----------------------------------------------------------------------------
def grads_after_backward(name, batch_wgrad, flush_mb=None):
    eng, x, y, B = engine(name, batch_wgrad, flush_mb)
    g = eng.forward_backward(x, y)
    torch.cuda.synchronize()
    G = eng.G[:eng.params.n].clone()
    calls = batch_calls(g)
    flushes = [c[1] for c in g.bwd.calls].count("rua_wgrad_reduce_batch")
    members = sum(c[2] for c in calls)
    mask = stem_mask(eng, g)
    for _, arr, n in calls:                                  # (no held-back member writes where the stem does)
        for i in range(n):
            off = (arr[i].dw - eng.G.data_ptr()) // 4
            assert not bool(mask[off:off + arr[i].taps * arr[i].Cout * arr[i].C].any())
    del g
    release(eng)
    return G, len(calls), members, flushes, mask


@pytest.mark.parametrize("name", sorted(MODELS))
def test_deferral_leaves_the_gradients_bitwise_equal_with_own_splits(name):
    with tuning(keep_own=True):
        G_on, ncalls, members, _, mask = grads_after_backward(name, True)
        G_off, ncalls_off, _, _, _ = grads_after_backward(name, False)
    assert ncalls >= 1 and members >= 1 and ncalls_off == 0, (ncalls, members, ncalls_off)
    print("%s: %d weight gradients held back for %d batched launch(es)" % (name, members, ncalls))
    assert float(G_on.abs().max()) > 0
    same_but_stem_noise(G_on, G_off, mask, name)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_one_train_step_with_the_shared_budget_matches_single_launches(name):
    res = []
    with tuning(keep_own=False):
        for on in (True, False):
            eng, x, y, B = engine(name, on)
            losses = eng.train_step(x, y)
            g = eng.forward_backward(x, y)                   # the logits after the update
            torch.cuda.synchronize()
            res.append((np.array(losses, np.float64), eng._results(g), {h: np.asarray(z, np.float64) for h, z in eng.logits(True, B).items()}))
            del g
            release(eng)
    (l_on, r_on, z_on), (l_off, r_off, z_off) = res
    nl = 5 if MODELS[name][2] else 1
    for i in range(nl):
        assert abs(l_on[i] - l_off[i]) <= 2e-3 * max(1.0, abs(l_off[i])), (i, l_on[i], l_off[i])
        assert abs(r_on[i] - r_off[i]) <= 2e-3 * max(1.0, abs(r_off[i])), (i, r_on[i], r_off[i])
    for h in z_on:
        assert rel_err(z_on[h], z_off[h]) < 5e-2, (h, rel_err(z_on[h], z_off[h]))


@pytest.mark.parametrize("path", ["eager", "graph"])
def test_a_flush_between_record_and_end_of_backward_keeps_the_order(path):
    """flush_bytes so small that flushes land between a held-back member's record and the end of backward: every flush is preceded
    by the batch of what was held back until then, on the eager path and in the captured step."""
    name = "cfg3"
    with tuning(keep_own=True):
        if path == "eager":
            G_on, ncalls, members, flushes, mask = grads_after_backward(name, True, flush_mb=4)
            G_off, _, _, flushes_off, _ = grads_after_backward(name, False, flush_mb=4)
            _, _, members_one, _, _ = grads_after_backward(name, True)
            assert ncalls >= 2 and flushes >= 2 and members == members_one, (ncalls, flushes, members, members_one)
            same_but_stem_noise(G_on, G_off, mask, "eager")
            return
        # the captured step zeroes the gradient arena behind the optimizer: Adam's first moment is what it leaves of the gradients.  Learning rate 0: the
        # weights stay, every replay sees the same gradients (the stem's irreproducible bits never reach a forward pass), M1 accumulates them in a fixed order
        M1 = []
        for on in (True, False):
            eng, x, y, B = engine(name, on, flush_mb=4, optimizer="adam", lr=0.0)
            assert eng.use_graph
            P0 = eng.P.clone()
            for _ in range(3):                               # warm-up + capture, then replays
                eng.train_step(x, y)
            torch.cuda.synchronize()
            assert B in eng._captured and torch.equal(eng.P, P0)
            g = eng.graph(B, True)
            if on:
                assert len(batch_calls(g)) >= 2
            mask = stem_mask(eng, g)
            M1.append(eng.M1[:eng.params.n].clone())
            del g
            release(eng)
        assert float(M1[0].abs().max()) > 0
        same_but_stem_noise(M1[0], M1[1], mask, "graph")


_COUNT_CHILD = """
import json, torch
import tests_wgrad_batch_child as T
from resunet_a_mltsk_keras_amd import _lib as L
eng, x, y, B = T.engine("cfg3", True, optimizer="adam")
eng.train_step(x, y)
eng.train_step(x, y)
torch.cuda.synchronize()
grids = L.lib().raw("rua_wgrad_group_last_grids")()     # the batch is the step's last rua_conv_wgrad_group call
calls = T.batch_calls(eng.graph(B, True))
print("RESULT " + json.dumps(dict(grids=grids, calls=[c[2] for c in calls], nodes=eng.count_step_dispatches(B))))
"""


def test_dispatch_count_of_the_captured_cfg3_step():
    """Kernel nodes of the captured cfg3 bf16 step: at most 266 - 23 + G.  Counted in a fresh process: the tuning keys are global to
    the library, and tests that ran before in this one leave some at other values than a step starts with (wgd_mintiles for one)."""
    import importlib.util
    import json
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import importlib.util, sys\nspec = importlib.util.spec_from_file_location('tests_wgrad_batch_child', %r)\n"
            "m = importlib.util.module_from_spec(spec); sys.modules['tests_wgrad_batch_child'] = m; spec.loader.exec_module(m)\n" % os.path.abspath(__file__)) + _COUNT_CHILD
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(here)] + [p for p in os.environ.get("PYTHONPATH", "").split(os.pathsep) if p]))
    flags = ["-s"] if sys.flags.no_user_site else []
    out = subprocess.run([sys.executable] + flags + ["-c", code], cwd=os.path.dirname(here), env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    r = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    print("cfg3 bf16 step: %s kernel nodes, members %s in %d grid(s)" % (r["nodes"], r["calls"], r["grids"]))
    assert r["calls"] == [MEMBERS_BEFORE], r
    assert 1 <= r["grids"] <= 2
    assert r["nodes"] is not None and r["nodes"] <= STEP_DISPATCHES_BEFORE - MEMBERS_BEFORE + r["grids"], r
