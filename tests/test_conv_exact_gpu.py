"""Every convolution and weight-gradient route, bit for bit against a float64 reference.

The data of tests/_exact_util.py are small integers (ternary operands, integer biases / residuals / bases): no product and no partial sum rounds, in bf16, fp32 or
the fp64 statistics, whatever the summation order - so y, both halves of the statistics and dW must EQUAL the reference, and one misplaced element anywhere fails.
(tests/test_kernels_gpu.py bounds the same kernels by 2e-2 of the output scale on Gaussian data: a column left out of the statistics or a pixel left out of dW
passes there - tests/test_conv_exact_host.py shows both.)  Every case asserts the route the planner gives it BEFORE it launches and its preconditions as plain
asserts; a mismatch reports how many elements differ, the first index, got / expected and the route."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from resunet_a_mltsk_keras_amd import _lib as L  # noqa: E402

import _exact_util as X  # noqa: E402

DT = {X.BF16: L.RUA_BF16, X.F32: L.RUA_F32}
KERNELS = ["conv_igemm", "conv_dma", "conv_dmap", "conv_halo", "conv_pw", "conv_strip", "conv_small", "conv_img", "conv_img2", "conv_band128m (sum)"]
WG_KINDS = ["wgrad_kernel", "all-taps", "wgrad_dmap", "wgrad_pw"]
WG_IMG = ["", " / wgrad_img", " / wgrad_imgs"]
PW_TAIL = 264 << 10                                          # wgrad_pw: replica accumulators + tickets at the end of the workspace (include/rua_hip.h)


def dev():
    return torch.device("cuda", 0)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def sdev(a, dt):
    """exact small values -> the storage type on the device"""
    t = torch.from_numpy(np.array(a, dtype=np.float32, order="C")).to(dev())
    return (t.to(torch.bfloat16) if dt == X.BF16 else t).contiguous()


def fdev(a):
    return torch.from_numpy(np.array(a, dtype=np.float32, order="C")).to(dev())


def host(t):
    return t.float().cpu().numpy() if t.dtype == torch.bfloat16 else t.cpu().numpy()


class tuned:
    """tuning keys set for the plan and the launch, the defaults back whatever happens"""

    def __init__(self, keys):
        self.keys = keys

    def __enter__(self):
        for k, v, _ in self.keys:
            L.lib().set_tuning(**{k: v})

    def __exit__(self, *exc):
        for k, _, dflt in self.keys:
            L.lib().set_tuning(**{k: dflt})


def as_array(cls, descs):
    arr = (cls * len(descs))()
    for i, d in enumerate(descs):
        C.memmove(C.byref(arr, i * C.sizeof(cls)), C.byref(d), C.sizeof(cls))
    return arr


def route_of(info):
    name = KERNELS[info.kernel_id] if 0 <= info.kernel_id < len(KERNELS) else "band launcher"
    return (f"{name} (kernel_id {info.kernel_id}, form {info.form}, grid {info.grid_x} x {info.grid_y}, tile {info.bm} x {info.bn}, K slices {info.ksplit}, "
            f"finisher {info.finisher}, band {info.band}, chain {info.chain})")


def stats_sum(stats, R, Cout):
    return stats.cpu().numpy().reshape(R, 2, Cout).sum(0)


# ------------------------------------------------------------------------------------------------------------------------------- forward, one launch
def fwd_desc(c, t):
    """the descriptor of a forward case over the device tensors t (name -> tensor, lists for x / w / more)"""
    d = L.ConvDesc()
    d.nseg = len(c.segs)
    for i, (Cs, up, dil, taps) in enumerate(c.segs):
        s = d.seg[i]
        s.x, s.w, s.C, s.Hs, s.Ws, s.up_shift, s.dil, s.taps = t["x"][i].data_ptr(), t["w"][i].data_ptr(), Cs, (c.H * c.stride) >> up, (c.W * c.stride) >> up, up, dil, taps
    d.N, d.H, d.W, d.Cout, d.stride, d.dtype = c.N, c.H, c.W, c.Cout, c.stride, DT[c.dt]
    d.y, d.out_stride, d.OH, d.OW = t["y"].data_ptr(), 1, c.H, c.W
    if c.epi in ("res", "resp", "relu") or c.mask_bias:
        d.bias = t["bias"].data_ptr()
        for i, m in enumerate(t["more"]):
            d.bias_more[i] = m.data_ptr()
    if c.epi in ("res", "resp"):
        d.aux, d.aux_mode = t["aux"].data_ptr(), 1
    elif c.epi in ("mask", "macc"):
        d.aux, d.aux_mode, d.mscale, d.mshift = t["aux"].data_ptr(), 2, t["mscale"].data_ptr(), t["mshift"].data_ptr()
        d.accumulate = 1 if c.epi == "macc" else 0
    elif c.epi == "aux3":
        d.aux, d.aux_mode = t["aux"].data_ptr(), 3
    elif c.epi == "relu":
        d.out_relu = 1
    elif c.epi == "acc":
        d.accumulate, d.out_stride, d.OH, d.OW = 1, 2, 2 * c.H, 2 * c.W
    if c.epi in ("res", "mask", "macc", "aux3"):
        d.stats, d.stats_mode, d.stats_replicas = t["stats"].data_ptr(), (1 if c.epi == "res" else 2), X.STAT_R
    if c.norm:
        d.in_scale, d.in_shift, d.in_relu = t["in_scale"].data_ptr(), t["in_shift"].data_ptr(), int(c.norm == 2)
    if "ws" in t:
        d.workspace, d.workspace_bytes = t["ws"].data_ptr(), t["ws"].numel() * 4
    return d


@pytest.mark.parametrize("c", X.FWD_CASES, ids=[c.name for c in X.FWD_CASES])
def test_conv_fwd_exact(c):
    lib = L.lib()
    r = X.fwd_case(c)
    X.check_fwd_preconditions(c, r)
    t = {"x": [sdev(a, c.dt) for a in r["x"]], "w": [sdev(a, c.dt) for a in r["w"]], "bias": fdev(r["bias"]), "more": [fdev(m) for m in r["more"]]}
    for k in ("mscale", "mshift", "in_scale", "in_shift"):
        if k in r:
            t[k] = fdev(r[k])
    if "aux" in r:
        t["aux"] = sdev(r["aux"], c.dt)
    # an output that does not accumulate starts from a value no result takes: every element has to be written
    t["y"] = sdev(r["y0"], c.dt) if "y0" in r else sdev(np.full(r["y"].shape, 300.0, np.float32), c.dt)
    t["stats"] = torch.zeros(X.STAT_R * 2 * c.Cout, dtype=torch.float64, device=dev())
    with tuned(c.tune):
        if c.ws:
            probe = fwd_desc(c, t)
            slab = lib.raw("rua_conv_workspace_bytes")(C.byref(probe))
            t["ws"] = torch.zeros((32 * slab + 4096) // 4, dtype=torch.float32, device=dev())      # (the last 4 KiB: ticket counters, zero once)
        d = fwd_desc(c, t)
        info = L.ConvLaunchInfo()
        lib.call("rua_conv_plan", C.byref(d), C.byref(info))
        route = route_of(info)
        assert info.kernel_id == c.kid == lib.raw("rua_conv_kernel_id")(C.byref(d)), (c.name, "planned on another kernel", route)
        assert not c.split or info.ksplit > 1, (c.name, "no K slices", route)
        assert not c.norm or lib.raw("rua_conv_fused_input_ok")(C.byref(d)) == 1, (c.name, route)
        lib.call("rua_conv_fwd", C.byref(d), stream())
        torch.cuda.synchronize()
        assert lib.raw("rua_conv_last_ksplit")() == info.ksplit
    X.assert_exact(host(t["y"]), r["y"], f"{c.name}: y", route, "(n, h, w, c)")
    if r["stats"] is not None:
        st = stats_sum(t["stats"], X.STAT_R, c.Cout)
        X.assert_exact(st[0], r["stats"][0], f"{c.name}: statistics, sum v", route, "(c,)")
        X.assert_exact(st[1], r["stats"][1], f"{c.name}: statistics, " + ("sum v^2" if c.epi == "res" else "sum v * aux"), route, "(c,)")
    if c.ws:
        assert int(t["ws"][-1024:].view(torch.int32).abs().max()) == 0, (c.name, "ticket counters left non-zero", route)


# ------------------------------------------------------------------------------------------------------------------------------- forward, band forms
def band_descs(c, r, t):
    nb = len(c.dils)
    arr = (L.ConvDesc * nb)()
    for b in range(nb):
        d = arr[b]
        d.nseg = 1
        s = d.seg[0]
        x = t["x"][0 if len(t["x"]) == 1 else b]
        s.x, s.w, s.C, s.Hs, s.Ws, s.up_shift, s.dil, s.taps = x.data_ptr(), t["w"][b].data_ptr(), c.C, c.H, c.W, 0, c.dils[b], 9
        d.N, d.H, d.W, d.Cout, d.stride, d.dtype = c.N, c.H, c.W, c.C, 1, L.RUA_BF16
        d.out_stride, d.OH, d.OW = 1, c.H, c.W
        if c.kind in ("norm", "first"):
            d.in_scale, d.in_shift, d.in_relu = t["in_scale"][b].data_ptr(), t["in_shift"][b].data_ptr(), 1
        if c.form == "sum":
            d.y, d.bias, d.accumulate = t["y"][0].data_ptr(), t["bias"][b].data_ptr(), (1 if b > 0 else 0)
            if b == 0:
                d.aux, d.aux_mode = t["aux"].data_ptr(), 1
        else:
            d.y = t["y"][b].data_ptr()
            d.stats, d.stats_replicas = t["stats"][b].data_ptr(), X.STAT_R
            if c.kind == "first":
                d.bias, d.stats_mode = t["bias"][b].data_ptr(), 1
            else:
                d.aux, d.aux_mode, d.mscale, d.mshift, d.stats_mode = t["aux"][b].data_ptr(), 2, t["mscale"][b].data_ptr(), t["mshift"][b].data_ptr(), 2
    return arr


def band_tensors(c, r):
    t = {"x": [sdev(a, X.BF16) for a in r["x"]], "w": [sdev(a, X.BF16) for a in r["w"]], "bias": [fdev(a) for a in r["bias"]]}
    for k in ("in_scale", "in_shift", "mscale", "mshift"):
        if k in r:
            t[k] = [fdev(a) for a in r[k]]
    if "aux" in r:
        t["aux"] = sdev(r["aux"], X.BF16) if c.form == "sum" else [sdev(a, X.BF16) for a in r["aux"]]
    t["y"] = [sdev(np.full(y.shape, 300.0, np.float32), X.BF16) for y in r["y"]]
    t["stats"] = [torch.zeros(X.STAT_R * 2 * c.C, dtype=torch.float64, device=dev()) for _ in r["y"]]
    return t


@pytest.mark.parametrize("c", X.SUM_CASES, ids=[c.name for c in X.SUM_CASES])
def test_conv_fwd_sum_exact(c):
    """rua_conv_fwd_sum on conv_band32 / conv_band64: the branches' sum kept on chip, the output written once"""
    lib = L.lib()
    r = X.band_case(c)
    X.check_band_preconditions(c, r)
    t = band_tensors(c, r)
    arr = band_descs(c, r, t)
    nb = len(c.dils)
    route = f"rua_conv_fwd_sum, rua_conv_sum_kernel {lib.raw('rua_conv_sum_kernel')(arr, nb)} (1 conv_band32, 2 conv_band64, 0 member by member)"
    assert lib.raw("rua_conv_sum_kernel")(arr, nb) == c.expect, (c.name, route)
    lib.call("rua_conv_fwd_sum", arr, nb, stream())
    torch.cuda.synchronize()
    assert lib.raw("rua_conv_sum_last_kernel")() == c.expect
    X.assert_exact(host(t["y"][0]), r["y"][0], f"{c.name}: y", route, "(n, h, w, c)")


@pytest.mark.parametrize("c", X.GROUP_CASES, ids=[c.name for c in X.GROUP_CASES])
def test_conv_fwd_group_band_exact(c):
    """rua_conv_fwd_group on conv_band64m / conv_band128m: independent members in one launch, each with its own normalise-on-load, bias / mask and statistics"""
    lib = L.lib()
    r = X.band_case(c)
    X.check_band_preconditions(c, r)
    t = band_tensors(c, r)
    arr = band_descs(c, r, t)
    nb = len(c.dils)
    out, n_out = (L.ConvLaunchInfo * nb)(), C.c_int32(-1)
    lib.call("rua_conv_group_plan", arr, nb, out, C.byref(n_out))
    route = "rua_conv_fwd_group: " + route_of(out[0])
    assert lib.raw("rua_conv_group_band_ok")(arr, nb) == 1 and n_out.value == 1 and out[0].band == c.expect and out[0].members == (1 << nb) - 1, (c.name, route)
    lib.call("rua_conv_fwd_group", arr, nb, stream())
    torch.cuda.synchronize()
    assert lib.raw("rua_conv_group_last_band")() == c.expect and lib.raw("rua_conv_group_last_grids")() == 1
    for b in range(nb):
        what = f"{c.name}: member {b} (dilation {c.dils[b]})"
        X.assert_exact(host(t["y"][b]), r["y"][b], what + ": y", route, "(n, h, w, c)")
        st = stats_sum(t["stats"][b], X.STAT_R, c.C)
        X.assert_exact(st[0], r["stats"][b][0], what + ": statistics, sum v", route, "(c,)")
        X.assert_exact(st[1], r["stats"][b][1], what + ": statistics, " + ("sum v^2" if c.kind == "first" else "sum v * aux"), route, "(c,)")


def test_conv_fwd_group_dmap_chain_exact():
    """conv_dmap members walking back to back through one grid (tuning key dmap_chain, on the burst-issue form): three dilation branches at 8 x 32 x 32 x 256"""
    lib = L.lib()
    cases = X.CHAIN_CASES
    keep, descs, refs = [], [], []
    for c in cases:
        r = X.fwd_case(c)
        X.check_fwd_preconditions(c, r)
        t = {"x": [sdev(a, c.dt) for a in r["x"]], "w": [sdev(a, c.dt) for a in r["w"]], "bias": fdev(r["bias"]), "more": [], "aux": sdev(r["aux"], c.dt),
             "mscale": fdev(r["mscale"]), "mshift": fdev(r["mshift"]), "y": sdev(np.full(r["y"].shape, 300.0, np.float32), c.dt),
             "stats": torch.zeros(X.STAT_R * 2 * c.Cout, dtype=torch.float64, device=dev())}
        keep.append(t); descs.append(fwd_desc(c, t)); refs.append((r["y"], r["stats"]))
    arr = as_array(L.ConvDesc, descs)
    n = len(cases)
    with tuned((("dmap_chain", 3, 0), ("dmap_spread", 0, 1))):
        out, n_out = (L.ConvLaunchInfo * n)(), C.c_int32(-1)
        lib.call("rua_conv_group_plan", arr, n, out, C.byref(n_out))
        route = "rua_conv_fwd_group: " + route_of(out[0])
        assert n_out.value == 1 and out[0].kernel_id == 2 and out[0].chain == n, route
        lib.call("rua_conv_fwd_group", arr, n, stream())
        torch.cuda.synchronize()
        assert lib.raw("rua_conv_group_last_chain")() == n and lib.raw("rua_conv_group_last_grids")() == 1
    for i, (t, (y, st)) in enumerate(zip(keep, refs)):
        X.assert_exact(host(t["y"]), y, f"{cases[i].name}: y", route, "(n, h, w, c)")
        got = stats_sum(t["stats"], X.STAT_R, cases[i].Cout)
        X.assert_exact(got[0], st[0], f"{cases[i].name}: statistics, sum v", route, "(c,)")
        X.assert_exact(got[1], st[1], f"{cases[i].name}: statistics, sum v * aux", route, "(c,)")


# ------------------------------------------------------------------------------------------------------------------------------- weight gradients
class WgRun:
    """device tensors and descriptor of one weight-gradient case; the workspace is what rua_wgrad_workspace_bytes asks for, zero-filled (wgrad_pw needs its tail zero)"""

    def __init__(self, c):
        lib = L.lib()
        self.c, self.r = c, X.wg_case(c)
        X.check_wg_preconditions(c, self.r)
        r = self.r
        self.a, self.dy = sdev(r["a"], c.dt), sdev(r["dy"], c.dt)
        self.dw = fdev(r["base"])
        self.flag = torch.zeros(4, dtype=torch.int32, device=dev())
        d = self.d = L.WgradDesc()
        d.a, d.C, d.Hs, d.Ws = self.a.data_ptr(), c.C, c.Hs, c.Ws
        d.dy, d.Cout, d.H, d.W = self.dy.data_ptr(), c.Cout, c.H, c.W
        d.N, d.stride, d.dil, d.taps, d.dtype = c.N, c.stride, c.dil, c.taps, DT[c.dt]
        d.dw = self.dw.data_ptr()
        if c.norm:
            self.sc, self.sh = fdev(r["in_scale"]), fdev(r["in_shift"])
            d.in_scale, d.in_shift, d.in_relu = self.sc.data_ptr(), self.sh.data_ptr(), int(c.norm == 2)
        self.ws = None
        if c.ws:
            nbytes = lib.raw("rua_wgrad_workspace_bytes")(C.byref(d))
            assert nbytes >= PW_TAIL
            self.ws = torch.zeros(nbytes // 4, dtype=torch.float32, device=dev())
            d.workspace, d.workspace_bytes = self.ws.data_ptr(), nbytes

    def route(self):
        lib = L.lib()
        kind, img = lib.raw("rua_wgrad_kind")(C.byref(self.d)), lib.raw("rua_wgrad_img_kind")(C.byref(self.d))
        p = L.WgradPending()
        lib.call("rua_wgrad_plan", C.byref(self.d), C.byref(p))
        return kind, img, p, (f"{WG_KINDS[kind]}{WG_IMG[img]} (rua_wgrad_kind {kind}, rua_wgrad_img_kind {img}, pending kind {p.kind}, partial buffers {p.parts}, "
                              f"workspace {'yes' if self.ws is not None else 'no'})")

    def tail_is_zero(self):
        return self.ws is None or float(self.ws[-(PW_TAIL // 4):].abs().max()) == 0.0


@pytest.mark.parametrize("c", X.WG_CASES, ids=[c.name for c in X.WG_CASES])
def test_conv_wgrad_exact(c):
    lib = L.lib()
    with tuned(c.tune):
        g = WgRun(c)
        kind, img, p, route = g.route()
        assert (kind, img) == (c.kind, c.img), (c.name, "planned on another kernel", route)
        if c.kind == 0 and c.img == 0:
            assert (p.kind == 2) == c.ws, (c.name, "K slices go through slabs exactly when there is a workspace", route)
        lib.call("rua_conv_wgrad", C.byref(g.d), stream())               # dw += sum, on the integer base
        torch.cuda.synchronize()
        X.assert_exact(g.dw.cpu().numpy(), g.r["dw"], f"{c.name}: dW (added to the base)", route, "(tap, co, c)")
        assert g.tail_is_zero(), (c.name, "the tail of the workspace is not zero again", route)
        # the first-writer flag: dw holds zeros and the device flag is up - kernels that end in a read-modify-write of dW store instead, those that add with atomics
        # or replicas ignore it: the gradient alone either way
        g.dw.zero_()
        g.flag.fill_(1)
        g.d.overwrite_dev = g.flag.data_ptr()
        lib.call("rua_conv_wgrad", C.byref(g.d), stream())
        torch.cuda.synchronize()
        X.assert_exact(g.dw.cpu().numpy(), g.r["grad"], f"{c.name}: dW (overwrite_dev -> 1, dW zeroed)", route, "(tap, co, c)")
        assert g.tail_is_zero(), (c.name, route)


def reduce_pending(recs):
    lib = L.lib()
    items, blocks = [], 0
    for rec in recs:
        if rec.kind != 0:
            q = L.WgradPending.from_buffer_copy(rec)
            q.block_begin = blocks
            blocks += q.blocks
            items.append(q)
    if items:
        table = (L.WgradPending * len(items))(*items)
        tdev = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(dev())
        lib.call("rua_wgrad_reduce_batch", tdev.data_ptr(), len(items), blocks, stream())
    return len(items)


@pytest.mark.parametrize("grp", X.WG_GROUPS, ids=[g.name for g in X.WG_GROUPS])
def test_conv_wgrad_group_exact(grp):
    """Four all-taps members sharing one round of blocks (group_members), three unequal generic members in the batched grid (one block budget: K splits other
    than a lone launch's - irrelevant to exact sums), and a deferred pair finished by one rua_wgrad_reduce_batch: each member against its own float64 reference."""
    lib = L.lib()
    runs = [WgRun(c) for c in grp.members]
    n = len(runs)
    for g in runs:
        if grp.form == "group":
            g.d.group_members = n
        elif grp.form == "batch":
            g.d.batch = 1
        else:
            g.d.defer = 1
    routes = []
    for g in runs:
        kind, img, p, route = g.route()
        assert (kind, img) == (g.c.kind, g.c.img), (g.c.name, route)
        routes.append(f"{grp.form}: {route}")
    if grp.form == "deferred":
        recs = []
        for g in runs:
            p = L.WgradPending()
            lib.call("rua_wgrad_plan", C.byref(g.d), C.byref(p))
            assert p.kind in (1, 2), (g.c.name, "nothing to defer")
            recs.append(p)
            lib.call("rua_conv_wgrad", C.byref(g.d), stream())
        assert reduce_pending(recs) == n
    else:
        arr = as_array(L.WgradDesc, [g.d for g in runs])
        recs = (L.WgradPending * n)()
        lib.call("rua_wgrad_group_plan", arr, n, recs)
        if grp.form == "group":
            assert all(recs[i].kind == 1 for i in range(n)), [recs[i].kind for i in range(n)]
        lib.call("rua_conv_wgrad_group", arr, n, stream())
        assert lib.raw("rua_wgrad_group_last_grids")() == 1, (grp.name, "the members did not share a grid")
    torch.cuda.synchronize()
    for g, route in zip(runs, routes):
        X.assert_exact(g.dw.cpu().numpy(), g.r["dw"], f"{g.c.name}: dW (added to the base)", route, "(tap, co, c)")
