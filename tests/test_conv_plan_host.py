"""The forward-convolution planner, pinned on the CPU: rua_conv_kernel_id, rua_conv_tile_bm / _bn, rua_conv_smem_bytes, rua_conv_fused_input_ok,
rua_conv_workspace_bytes, rua_conv_group_band_ok, rua_conv_plan and rua_conv_group_plan answer what tests/golden/conv_plans.json recorded
(tools/record_conv_plans.py) for every descriptor and tuning of the file - the query exports' column was recorded before the planner existed - and a plan is
consistent with the queries and with itself.  No GPU: nothing is launched, no pointer is followed."""
import importlib.util
import json
import os

from resunet_a_mltsk_keras_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KID, FORM, GX, GY, BLOCK, LDS, BM, BN, KSPLIT, FIN, MEMBERS = range(11)


def _recorder():
    spec = importlib.util.spec_from_file_location("record_conv_plans", os.path.join(ROOT, "tools", "record_conv_plans.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_conv_plans_equal_the_recorded_ones():
    with open(os.path.join(ROOT, "tests", "golden", "conv_plans.json")) as f:
        want = json.load(f)
    lib = L.lib()
    keys = sorted({k for t in want["tunings"] for k in t} | {k for g in want["groups"] for k in g["tune"]})
    before = {k: lib.get_tuning(k) for k in keys}
    try:
        got = _recorder().replay(lib, want)
    finally:
        lib.set_tuning(**before)
    got = json.loads(json.dumps(got))
    assert len(want["descs"]) == 291 and len(want["plans"]) == 1811 and len(want["groups"]) == 45 and len(want["fwd_errors"]) == 21
    for g, w in zip(got["plans"], want["plans"]):
        assert g == w, (want["tunings"][w[0]], want["descs"][w[1]], "got", g[2:], "recorded", w[2:])
    for g, w in zip(got["groups"], want["groups"]):
        assert g == w, (w["name"], "got", g["band_ok"], g["result"], "recorded", w["band_ok"], w["result"])
    assert {k: lib.get_tuning(k) for k in keys} == before

    # a plan agrees with the queries: the kernel id, and the tile where the kernel has one
    planned = 0
    for ti, di, (kid, bm, bn, smem, fused, slab), (rc, err, info) in want["plans"]:
        if rc != 0:
            assert rc == -1 and err and info is None
            continue
        planned += 1
        assert info[KID] == kid, (want["tunings"][ti], want["descs"][di])
        if kid in (0, 1, 2):
            assert (info[BM], info[BN]) == (bm, bn), (want["tunings"][ti], want["descs"][di])
        else:
            assert (info[BM], info[BN]) == (0, 0)
        assert info[FIN] == (1 if info[KSPLIT] > 1 and kid != 9 else 0) and info[MEMBERS] == 1
        assert (info[FORM] >= 0 and info[GX] >= 1 and info[GY] == 1 and info[BLOCK] in (256, 512)) or kid == 9
        if kid == 0:
            assert info[LDS] <= smem                      # rua_conv_smem_bytes: the unit table at its capacity
    assert planned == 1338                                # the rest are the rejected descriptors, under every tuning
    # what rua_conv_fwd rejected before the planner existed, rua_conv_plan rejects with the same code and text
    by_desc = {di: plan for ti, di, _, plan in want["plans"] if ti == 0}
    for di, rc, err in want["fwd_errors"]:
        assert by_desc[di][:2] == [rc, err]
    # every member of a group is in exactly one launch
    for g in want["groups"]:
        rc, err, band, chain, launches = g["result"]
        if rc != 0:
            assert launches == [] and err
            continue
        masks = [r[MEMBERS] for r in launches]
        assert sum(masks) == (1 << len(g["members"])) - 1 and all(m > 0 for m in masks), g["name"]
        for i, m in enumerate(masks):
            assert all(m & o == 0 for o in masks[i + 1:]), g["name"]
        assert (band != 0) == bool(g["band_ok"]) and (not band or len(launches) == 1), g["name"]
        assert chain in [0] + [bin(m).count("1") for m in masks], g["name"]
