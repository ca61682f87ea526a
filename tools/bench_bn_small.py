"""The fused BatchNorm launches of cfg3's deep levels (levels 4 - 6, psp_mid, up5, up4), each alone, in the pixel-major and in the channel-sliced form
(tuning key bn_sliced; csrc/elementwise.hip, bn_route).  The descriptors are the ones the engine records for a cfg3 train step (bf16, batch 8), replayed through the
C ABI: nb, options and replica counts as the engine issues them.

  launches   every deep launch: pixel-major, the chooser's route, S = 4, and four times the chooser's parts (P above the replica count of a statistics output)
  sweep-M    one launch per channel count with its pixel count cut down: where the forms cross
  replicas   the same launch reading 1 / 8 / 32 replicas of its input statistics: the price of the prologue

warm: 20 launches back to back behind a blocker that keeps the stream busy while they are enqueued, per launch.  cold: one launch behind a 512 MB sweep, HIP events
around it, the median bracket of an empty pair subtracted.  Microseconds.

usage (GPU box): python tools/bench_bn_small.py [launches] [sweep-M] [replicas] > profiles/bn_sliced/bench_bn_small.txt"""
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from resunet_a_mltsk_keras_amd import _lib as L                     # noqa: E402
from resunet_a_mltsk_keras_amd.engine import Engine, LossSpec, ModelConfig   # noqa: E402
from resunet_a_mltsk_keras_amd.synthetic import make_batch          # noqa: E402

NAMES = ("rua_bn_fwd", "rua_bn_fwd_group", "rua_bn_bwd", "rua_bn_bwd_group")
DEEP_PIECES = 8192 * 32                                             # level 4: M = 8192, C = 256 in bf16
BURST = 20


def members(name, args):
    """The descriptors of one recorded call."""
    return [args[0][i] for i in range(args[1])] if name.endswith("_group") else [args[0]._obj]


def describe(name, ds):
    d = ds[0]
    if "fwd" in name:
        rin = max([d.replicas if d.stats else 0] + [d.br[b].replicas for b in range(d.nb) if d.br[b].stats])
        opt = f"relu{d.relu} train{d.training}" + (" out_stats" if d.br[0].out_stats else "")
        rout = 0
    else:
        rin = max(d.br[b].replicas for b in range(d.nb))
        rout = min([r for r, on in ((d.skip_replicas, d.skip_stats), (d.dx_replicas, d.dx_stats)) if on] or [0])
        opt = (f"mask{d.masked} acc{d.accumulate}" + (" dskip" if d.dskip else "") + (f" skip_stats/{d.skip_replicas}" if d.skip_stats else "")
               + (f" dx_stats/{d.dx_replicas}" if d.dx_stats else "") + (" s2out" if any(d.br[b].stats2_out for b in range(d.nb)) else ""))
    ms = "/".join(str(m.M) for m in ds)
    return f"{name[4:]:13s} M {ms:>16s} C {d.C:4d} nb {d.nb} Rin {rin:2d} Rout {rout:2d} {opt}"


def route(name, d):
    r = L.lib().raw("rua_bn_fwd_route" if "fwd" in name else "rua_bn_bwd_route")(C.byref(d))
    return f"S{r & 255} P{r >> 8}" if r else "pixel"


class Timer:
    def __init__(self):
        self.big = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")
        self.sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        pairs = [self.bracket(lambda: None) for _ in range(30)]
        self.empty = sorted(pairs)[len(pairs) // 2]

    def bracket(self, f):
        self.big.add_(1)                                            # 512 MB read and written: the caches hold nothing of the launch's tensors
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); f(); b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3

    def run(self, fn, args, reps=9):
        def go():
            rc = fn(*args, self.sp)
            if rc != 0:
                L.lib().check(rc, "launch")
        go()
        torch.cuda.synchronize()
        warm = []
        for _ in range(reps):
            for _ in range(6):
                self.big.add_(1)                                    # the blocker: the burst is enqueued while it runs
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(BURST):
                go()
            b.record()
            torch.cuda.synchronize()
            warm.append(a.elapsed_time(b) * 1e3 / BURST)
        cold = sorted(self.bracket(go) for _ in range(reps))[reps // 2] - self.empty
        return sorted(warm)[reps // 2], max(cold, 0.0)


def variants(t, fn, args, kinds):
    lib, out = L.lib(), []
    for label, kv in kinds:
        lib.set_tuning(**kv)
        try:
            w, c = t.run(fn, args)
        finally:
            lib.set_tuning(bn_sliced=1, bn_sliced_s=0, bn_sliced_parts=0)
        out.append(f"{label} {w:6.2f} / {c:6.2f}")
    return " | ".join(out)


def main():
    what = set(sys.argv[1:]) or {"launches", "sweep-M", "replicas"}
    torch.cuda.set_device(0)
    eng = Engine(ModelConfig(input_shape=(256, 256, 6), num_classes=6, multitasking=True, depth=6), dtype="bf16", seed=0)
    heads = ["seg", "bound", "dist", "color"]
    eng.compile(LossSpec(kind={h: L.LOSS_TANIMOTO for h in heads}, weight={h: 1.0 for h in heads}, optimizer="adam", lr=1e-3))
    x, y = make_batch(8, 256, 6, 6, True, seed=1234)
    for _ in range(2):
        eng.train_step(x, y, fetch=False)
    torch.cuda.synchronize()
    g = eng.graph(8, True)
    calls = [(pn, plan.scopes[i] or "-", name, fn, args) for pn, plan in (("fwd", g.fwd), ("bwd", g.bwd))
             for i, (fn, name, args, _) in enumerate(plan.calls) if name in NAMES]
    t = Timer()
    lib = L.lib()
    print(f"# warm / cold us per launch; empty event bracket {t.empty:.2f} us subtracted from cold")
    if "launches" in what:
        tot = {}
        for pn, scope, name, fn, args in calls:
            ds = members(name, args)
            applies = ds[0].br[0].g if "bwd" in name else ds[0].br[0].out              # (coefficient-only launches stay one block)
            if max(m.M * (m.C // 8) for m in ds) > DEEP_PIECES or not applies:
                continue
            lib.set_tuning(bn_sliced=2)
            rt = [route(name, m) for m in ds]
            lib.set_tuning(bn_sliced=1)
            p4 = max(int(r.split("P")[1]) for r in rt if r != "pixel") * 4 if any(r != "pixel" for r in rt) else 0
            kinds = [("pixel", dict(bn_sliced=0)), ("sliced", dict(bn_sliced=2)), ("S4", dict(bn_sliced=2, bn_sliced_s=4))]
            if len(ds) == 1 and p4:
                kinds.append((f"P{p4}", dict(bn_sliced=2, bn_sliced_parts=p4)))
            print(f"{pn} {scope.split(':')[0]:8s} {describe(name, ds)} route {','.join(rt)} :: {variants(t, fn, args, kinds)}", flush=True)
    singles = [(name, fn, args) for pn, scope, name, fn, args in calls if not name.endswith("_group")
               and (members(name, args)[0].br[0].g if "bwd" in name else members(name, args)[0].br[0].out)]
    if "sweep-M" in what:
        print("# sweep over M (the recorded launch with its pixel count cut down): pixel vs sliced, warm / cold")
        for Cc in (64, 128, 256, 512, 1024):
            for kind in ("rua_bn_fwd", "rua_bn_bwd"):
                cand = [(members(n, a)[0].M * members(n, a)[0].nb, n, f, a) for n, f, a in singles if n == kind and members(n, a)[0].C == Cc]
                if not cand:
                    continue
                _, name, fn, args = max(cand, key=lambda c: c[0])
                d = members(name, args)[0]
                full = d.M
                m = 256
                while m <= min(full, 131072):
                    d.M = m
                    lib.set_tuning(bn_sliced=2)
                    rt = route(name, d)
                    lib.set_tuning(bn_sliced=1)
                    print(f"{describe(name, [d])} route {rt} :: {variants(t, fn, args, [('pixel', dict(bn_sliced=0)), ('sliced', dict(bn_sliced=2))])}", flush=True)
                    m *= 2
                d.M = full
    if "replicas" in what:
        print("# input statistics read from 1 / 8 / 32 replicas (the launches that read 32): pixel vs sliced, warm / cold")
        for name, fn, args in singles:
            d = members(name, args)[0]
            if d.M * (d.C // 8) > DEEP_PIECES:
                continue
            fields = [(d, "replicas")] if "fwd" in name else [(d.br[b], "replicas") for b in range(d.nb)]
            before = [getattr(o, f) for o, f in fields]
            if max(before) < 32:
                continue
            for r in (1, 8, 32):
                for (o, f), was in zip(fields, before):
                    setattr(o, f, min(r, was))
                print(f"{describe(name, [d])} :: {variants(t, fn, args, [('pixel', dict(bn_sliced=0)), ('sliced', dict(bn_sliced=2))])}", flush=True)
            for (o, f), was in zip(fields, before):
                setattr(o, f, was)


if __name__ == "__main__":
    main()
