"""Print the recorded plans of a training graph, one line per launch of fwd, loss_plan and bwd: name, scope, the gradient offsets it names and its
arguments, descriptors field by field.  Every address is printed as the rank of its first appearance in the dump (p0, p1, ...): the text does not depend on
where the allocator put things but still shows which launches share a buffer - two checkouts record the same step exactly when their dumps are equal.

    python tools/plan_dump.py cfg3 [--dtype f32] [--buckets 4] [--sha]

The model is a row of MODELS in tests/test_wgrad_batch_gpu.py; the engine's switches come from the environment (RUA_FLUSH_MB=4 ...).  --buckets K: the
gradients are cut into K equal all-reduce buckets as under data parallel (a stub: no process group, no step is run).  Needs a GPU (graphs allocate)."""
import argparse
import ast
import ctypes as C
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from resunet_a_mltsk_keras_amd import _lib as L  # noqa: E402
from resunet_a_mltsk_keras_amd.engine import Engine, LossSpec, ModelConfig  # noqa: E402

HEADS = ["seg", "bound", "dist", "color"]


def models():
    tree = ast.parse(open(os.path.join(ROOT, "tests", "test_wgrad_batch_gpu.py")).read())
    node = next(n for n in tree.body if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", "") == "MODELS")
    return ast.literal_eval(node.value)


class Buckets:
    """Engine.dist for recording only: K equal ranges of the flat parameter buffer."""

    def __init__(self, k, n):
        self.k, self.n = k, n

    def bucket_of(self, off):
        return min(self.k - 1, off * self.k // self.n)


class Dump:
    def __init__(self):
        self.rank, self.lines = {}, []

    def addr(self, p):
        return "null" if not p else "p%d" % self.rank.setdefault(int(p), len(self.rank))

    def value(self, v, ctype=None):
        if isinstance(v, C.Structure):
            return "{" + " ".join("%s=%s" % (f, self.value(getattr(v, f), t)) for f, t in v._fields_) + "}"
        if isinstance(v, C.Array):
            return "[" + " ".join(self.value(x, v._type_) for x in v) + "]"
        if ctype is C.c_void_p or isinstance(v, C.c_void_p):
            return self.addr(v.value if isinstance(v, C.c_void_p) else v)
        if type(v).__name__ == "CArgObject":                   # ctypes.byref(descriptor)
            return self.value(v._obj)
        if isinstance(v, int) and v >= 1 << 40:
            return self.addr(v)
        return "null" if v is None else repr(v)

    def plan(self, tag, plan, g):
        for (_, name, args, grads), scope in zip(plan.calls, plan.scopes):
            self.lines.append("%s %s scope=%s grads=%s %s" % (tag, name, scope, list(grads), " ".join(self.value(a) for a in args)))
            if name == "rua_wgrad_reduce_batch":               # its table lives on the device: the records, in order
                table = next(t for t in g.allocs if t.data_ptr() == args[0])
                recs = (L.WgradPending * args[1]).from_buffer_copy(table.cpu().numpy().tobytes())
                self.lines += ["%s   record %s" % (tag, self.value(r)) for r in recs]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("model", choices=sorted(models()))
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--buckets", type=int, default=0)
    ap.add_argument("--sha", action="store_true", help="print only the SHA-256 of the dump and the three launch counts")
    a = ap.parse_args()
    shape, ncls, mt, B, depth, variant = models()[a.model]
    eng = Engine(ModelConfig(input_shape=shape, num_classes=ncls, multitasking=mt, depth=depth, variant=variant), dtype=a.dtype, seed=0)
    heads = HEADS if mt else ["seg"]
    eng.compile(LossSpec(kind={h: L.LOSS_TANIMOTO for h in heads}, weight={h: 1.0 for h in heads}))
    if a.buckets:
        eng.dist = Buckets(a.buckets, eng.params.n)
    g = eng.graph(B, True)
    d = Dump()
    for tag, plan in (("fwd", g.fwd), ("loss", g.loss_plan), ("bwd", g.bwd)):
        d.plan(tag, plan, g)
    d.lines += ["alloc %d %s %s" % (i, tuple(t.shape), t.dtype) for i, t in enumerate(g.allocs)]
    text = "\n".join(d.lines) + "\n"
    if a.sha:
        print("%s fwd %d loss %d bwd %d" % (hashlib.sha256(text.encode()).hexdigest(), len(g.fwd.calls), len(g.loss_plan.calls), len(g.bwd.calls)))
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
