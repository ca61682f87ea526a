"""The weight-gradient planner, pinned on the CPU: rua_wgrad_kind, rua_wgrad_img_kind, rua_wgrad_workspace_bytes, rua_wgrad_plan and rua_wgrad_group_plan
answer what tests/golden/wgrad_plans.json recorded (tools/record_wgrad_plans.py) for every descriptor and tuning of the file.  No GPU: nothing is launched,
no pointer is followed."""
import importlib.util
import json
import os

from resunet_a_mltsk_keras_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _recorder():
    spec = importlib.util.spec_from_file_location("record_wgrad_plans", os.path.join(ROOT, "tools", "record_wgrad_plans.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_wgrad_plans_equal_the_recorded_ones():
    with open(os.path.join(ROOT, "tests", "golden", "wgrad_plans.json")) as f:
        want = json.load(f)
    lib = L.lib()
    keys = sorted({k for t in want["tunings"] for k in t} | {"wgrad_group"})
    before = {k: lib.get_tuning(k) for k in keys}
    try:
        got = _recorder().replay(lib, want)
    finally:
        lib.set_tuning(**before)
    got = json.loads(json.dumps(got))
    assert len(want["plans"]) >= 400 and len(want["groups"]) == 5
    assert got["groups"] == want["groups"]
    for g, w in zip(got["plans"], want["plans"]):
        assert g == w, (want["tunings"][w[0]], want["descs"][w[1]], "got", g[2], "recorded", w[2])
    assert {k: lib.get_tuning(k) for k in keys} == before
