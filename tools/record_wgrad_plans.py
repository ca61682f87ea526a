"""Record what the weight-gradient planner decides for a sweep of descriptors and tunings: tests/golden/wgrad_plans.json.

    python tools/record_wgrad_plans.py [--out tests/golden/wgrad_plans.json]

Needs no GPU: rua_wgrad_kind, rua_wgrad_img_kind, rua_wgrad_workspace_bytes, rua_wgrad_plan and rua_wgrad_group_plan only compute, the pointers of the
descriptors are made up and never followed (without a device rua_cu_count() is 256, the MI355X's own count).  A pointer is written as "<role><member>+<offset>"
(role: a, dy, dw, ws, sc(ale), sh(ift), ow = overwrite_dev).  tests/test_wgrad_plan_host.py replays the descriptors of the file (replay() below) and asserts
that the library still answers the same - record the file with the library of the commit whose decisions are to be kept."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from resunet_a_mltsk_keras_amd import _lib as L  # noqa: E402

ROLES = ["a", "dy", "dw", "ws", "sc", "sh", "ow"]
FIELD_OF = {"a": "a", "dy": "dy", "dw": "dw", "ws": "workspace", "sc": "in_scale", "sh": "in_shift", "ow": "overwrite_dev"}
INTS = ["C", "Hs", "Ws", "Cout", "H", "W", "N", "stride", "dil", "taps", "dtype", "workspace_bytes", "in_relu", "defer", "group_members", "batch"]
TUNINGS = [{}, {"wgrad_rows": 0}, {"wgrad_slabs": 0}, {"wgrad_taps_share": 0}, {"wgrad_pw": 7}, {"cu_reserve": 8}]


def fake(role, member):
    return (1 << 52) + (member << 44) + ((ROLES.index(role) + 1) << 40)


def name_of(p):
    if not p:
        return None
    role, member, off = ((p >> 40) & 15) - 1, (p >> 44) & 255, p & ((1 << 40) - 1)
    assert p >> 52 == 1 and 0 <= role < len(ROLES), hex(p)
    return "%s%d+%d" % (ROLES[role], member, off)


def to_desc(spec, member=0):
    d = L.WgradDesc()
    for k in INTS:
        setattr(d, k, spec.get(k, 0))
    for role in spec["ptrs"]:
        setattr(d, FIELD_OF[role], fake(role, member))
    return d


def pending(r):
    return [r.kind, r.parts, r.n, name_of(r.partials), name_of(r.dw), r.CC, r.blocks, r.block_begin, r.pad, name_of(r.overwrite_dev)]


def plan_one(lib, spec):
    """[return code, error text, kind, img_kind, workspace bytes, pending record] of one descriptor"""
    d, r = to_desc(spec), L.WgradPending()
    rc = lib.raw("rua_wgrad_plan")(C.byref(d), C.byref(r))
    err = lib.dll.rua_last_error().decode() if rc else ""
    return [rc, err, lib.raw("rua_wgrad_kind")(C.byref(d)), lib.raw("rua_wgrad_img_kind")(C.byref(d)), lib.raw("rua_wgrad_workspace_bytes")(C.byref(d)), pending(r)]


def plan_group(lib, specs):
    arr, out = (L.WgradDesc * len(specs))(), (L.WgradPending * len(specs))()
    for i, s in enumerate(specs):
        d = to_desc(s, i)
        C.memmove(C.byref(arr, i * C.sizeof(L.WgradDesc)), C.byref(d), C.sizeof(L.WgradDesc))
    rc = lib.raw("rua_wgrad_group_plan")(arr, len(specs), out)
    return [rc, lib.dll.rua_last_error().decode() if rc else "", [pending(r) for r in out]]


def replay(lib, fix):
    """What the library answers today for the descriptors and tunings of a recorded file, in the file's own layout.  Tuning is restored."""
    keys = sorted({k for t in fix["tunings"] for k in t} | {k for g in fix["groups"] for k in g["tune"]})
    old = {k: lib.get_tuning(k) for k in keys}
    plans, groups = [], []
    try:
        for ti, di, _ in fix["plans"]:
            lib.set_tuning(**old)
            lib.set_tuning(**fix["tunings"][ti])
            plans.append([ti, di, plan_one(lib, fix["descs"][di])])
        for g in fix["groups"]:
            lib.set_tuning(**old)
            lib.set_tuning(**g["tune"])
            groups.append({"name": g["name"], "tune": g["tune"], "members": g["members"], "result": plan_group(lib, g["members"])})
    finally:
        lib.set_tuning(**old)
    return {"tunings": fix["tunings"], "descs": fix["descs"], "plans": plans, "groups": groups}


def conv(N, H, C, Cout=None, taps=9, dil=1, dtype=L.RUA_BF16, ws=True, bn=False, stride=1, W=None, **more):
    W, Cout = W or H, Cout or C
    s = dict(N=N, H=H, W=W, Hs=H * stride, Ws=W * stride, C=C, Cout=Cout, taps=taps, dil=dil, stride=stride, dtype=dtype)
    s["ptrs"] = ["a", "dy", "dw"] + (["ws"] if ws else []) + (["sc", "sh"] if bn else [])
    if bn:
        s["in_relu"] = 1
    s.update(more)
    return s


def sweep():
    """(descriptors, indices of the subset that every non-default tuning runs too)"""
    descs, core = [], []
    levels = [(256, 32), (128, 64), (64, 128), (32, 256), (16, 512), (8, 1024)]           # cfg3 at batch 8
    for H, Cc in levels:
        for taps, dil in [(9, 1), (9, 3), (9, 15), (9, 31), (1, 1)]:
            for ws in (True, False):
                descs.append(conv(8, H, Cc, taps=taps, dil=dil, ws=ws))
            core.append(len(descs) - 2)
            descs.append(conv(8, H, Cc, taps=taps, dil=dil, defer=1))
            descs.append(conv(8, H, Cc, taps=taps, dil=dil, group_members=4, defer=1, ptrs=["a", "dy", "dw", "ws", "ow"]))
            core.append(len(descs) - 1)
            if taps == 9 and Cc <= 256:                                                      # BatchNorm + ReLU on load: the all-taps levels, and one that rejects it
                descs.append(conv(8, H, Cc, dil=dil, bn=True))
                core.append(len(descs) - 1)
                descs.append(conv(8, H, Cc, dil=dil, bn=True, group_members=4, defer=1))
        descs.append(conv(8, H, Cc, Cout=max(32, Cc // 2), taps=1))                          # the narrowing 1x1 of a level
        core.append(len(descs) - 1)
    core.append(len(descs)); descs.append(conv(8, 128, 32, Cout=64, taps=1, stride=2))       # a stride-2 1x1
    descs.append(conv(8, 128, 32, Cout=64, taps=1, stride=2, defer=1))
    core.append(len(descs)); descs.append(conv(3, 20, 24, Cout=40, dil=2))                   # the odd shape
    descs.append(conv(3, 20, 24, Cout=40, dil=2, ws=False))
    core.append(len(descs)); descs.append(conv(8, 16, 16, Cout=32, taps=1))                  # the stem's 1x1 on the packed input (too few pixels for wgrad_pw)
    descs.append(conv(8, 256, 16, Cout=32, taps=1, defer=1))
    core.append(len(descs)); descs.append(conv(2, 64, 32, dtype=L.RUA_F32))                  # fp32
    descs.append(conv(3, 20, 24, Cout=40, dil=2, dtype=L.RUA_F32, ws=False))
    core.append(len(descs)); descs.append(conv(2, 8, 64))                                    # whole-image kernels at their smallest
    descs.append(conv(4, 16, 64, Cout=128))
    # descriptors the library must reject
    bad = [conv(8, 64, 32, ptrs=["dy", "dw"]), conv(8, 64, 32, dtype=7), conv(8, 64, 12), conv(8, 64, 32, dtype=L.RUA_F32, Cout=30), conv(8, 64, 32, taps=3),
           conv(3, 20, 24, Cout=40, dil=2, bn=True), conv(8, 64, 32, Cout=64, taps=1, ws=False, Hs=32, Ws=32, stride=2), conv(64, 256, 40, Cout=136)]
    core += list(range(len(descs), len(descs) + len(bad)))
    return descs + bad, core


def group_cases():
    small = [conv(8, 16, 512, Cout=256, taps=1, defer=1, batch=1), conv(3, 20, 24, Cout=40, dil=2, defer=1, batch=1), conv(8, 8, 1024, Cout=256, taps=1, defer=1, batch=1)]
    many = [conv(1 + i % 3, 16 + 4 * (i % 5), 24 + 8 * (i % 4), Cout=40 + 8 * (i % 7), taps=(9 if i % 2 else 1), dil=1 + i % 3, defer=i % 2, batch=1) for i in range(33)]
    for s in small + many:
        s["workspace_bytes"] = 4 << 20
    mixed = [dict(s) for s in small]
    mixed[1]["batch"] = 0
    out = []
    for wg in (23, 55):
        out.append({"name": "three unequal members, wgrad_group=%d" % wg, "tune": {"wgrad_group": wg}, "members": small})
        out.append({"name": "a member without batch falls back, wgrad_group=%d" % wg, "tune": {"wgrad_group": wg}, "members": mixed})
    out.append({"name": "33 members take two grids", "tune": {}, "members": many})
    return out


def record(lib):
    descs, core = sweep()
    for s in descs:                                                                           # the workspace a caller would allocate (default tuning)
        if "ws" in s["ptrs"] and "workspace_bytes" not in s:
            d = to_desc(s)
            s["workspace_bytes"] = lib.raw("rua_wgrad_workspace_bytes")(C.byref(d))
    plans = [[ti, di, None] for ti in range(len(TUNINGS)) for di in (range(len(descs)) if ti == 0 else core)]
    return replay(lib, {"tunings": TUNINGS, "descs": descs, "plans": plans, "groups": [dict(g, result=None) for g in group_cases()]})


def dump(fix, path):
    row = lambda v: json.dumps(v, separators=(",", ":"))
    with open(path, "w") as f:
        f.write('{"tunings":%s,\n"descs":[\n%s],\n"plans":[\n%s],\n"groups":[\n%s]}\n' % (
            row(fix["tunings"]), ",\n".join(row(d) for d in fix["descs"]), ",\n".join(row(p) for p in fix["plans"]), ",\n".join(row(g) for g in fix["groups"])))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "wgrad_plans.json"))
    a = ap.parse_args()
    fix = record(L.lib())
    dump(fix, a.out)
    print("%s: %d descriptors, %d plans, %d group plans, %d bytes" % (a.out, len(fix["descs"]), len(fix["plans"]), len(fix["groups"]), os.path.getsize(a.out)))
