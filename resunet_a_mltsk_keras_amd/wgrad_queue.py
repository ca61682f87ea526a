"""When the weight gradients of a training graph are launched and when their partial sums are reduced: one owner (WgradQueue) for the deferred reductions, the
launches held back in front of each flush, and the gradient offsets (`grads=`) every such launch names for the data-parallel bucket marks."""
import ctypes as C
from collections import namedtuple
from typing import List

import torch

from . import _lib as L

WS_TAIL_BYTES = 264 << 10        # the LAST 264 KiB of a workspace: replica accumulators and ticket counters (include/rua_hip.h: zeroed once, left zero by every call)


# One weight gradient: dW[dw_off] of the convolution (stride, dil, taps) from its input `a` (a Ten) and its output's gradient `dy`; in_bn (a Coef): `a` is read
# as relu(scale * a + shift) (normalise on load)
WSpec = namedtuple("WSpec", "a dy dw_off stride dil taps in_bn", defaults=(None,))


def chunks(items: List, n: int) -> List[List]:
    return [items[i:i + n] for i in range(0, len(items), n)]


class WgradQueue:
    """The weight-gradient schedule of one training Graph.  `e` is the Engine, read for its settings only (defer_reduce, batch_wgrad, group_wgrad_pw,
    merge_wgrad, flush_bytes, cu_count, wgrad_overwrite / ow_flag, scratch, dist, dev); bwd the backward Plan - launches recorded into another plan, or by a dry
    graph, are never deferred, never held back and never ask the library; alloc / keep / G / issue are the Graph's own (keep: allocs.append)."""

    def __init__(self, e, bwd, dt: int, dry: bool, alloc, keep, G, issue):
        self.e, self.bwd, self.dt, self.dry, self.alloc, self.keep, self.G, self.issue = e, bwd, dt, dry, alloc, keep, G, issue
        self.pending: List[tuple] = []          # deferred weight-gradient reductions (record, dW offset)
        self.pending_bytes = 0                  # ... and the bytes of partials they will read (Engine.flush_bytes)
        self.pending_bucket = 0
        self.later: List[tuple] = []            # generic-tile weight gradients held back for ONE batched launch in front of the next flush (descriptor, dW offset)

    def desc(self, sp: WSpec, group: int = 0):
        """The descriptor of one weight gradient, reducing in the shared scratch - and nothing else: no flush, no allocation, no record."""
        d = L.WgradDesc()
        d.group_members = group                            # members of the rua_conv_wgrad_group call this descriptor belongs to
        d.a, d.C, d.Hs, d.Ws = sp.a.ptr, sp.a.C, sp.a.H, sp.a.W
        if sp.in_bn is not None:                            # a is read as relu(scale * a + shift) (normalise on load)
            d.in_scale, d.in_shift, d.in_relu = sp.in_bn.scale, sp.in_bn.shift, 1
        d.dy, d.Cout, d.H, d.W = sp.dy.ptr, sp.dy.C, sp.dy.H, sp.dy.W
        d.N, d.stride, d.dil, d.taps, d.dtype = sp.dy.N, sp.stride, sp.dil, sp.taps, self.dt
        d.dw, d.grads = self.G(sp.dw_off), (sp.dw_off,)     # (grads: the offsets Graph.issue names on the launch)
        if not self.dry:
            if self.e.wgrad_overwrite:
                d.overwrite_dev = self.e.ow_flag.data_ptr()    # whole steps store dW instead of adding to the zeroed arena (Engine._set_overwrite)
            d.workspace, d.workspace_bytes = self.e.scratch.data_ptr(), self.e.scratch.numel() * 4
        return d

    def defers(self, plan) -> bool:
        return (not self.dry) and self.e.defer_reduce and plan is self.bwd

    def admit(self, plan, dw_off: int, byte_cap: bool = True) -> bool:
        """THE flush rule, in front of a launch (or record) that writes dW[dw_off]: what is queued goes out first when this gradient belongs to another
        all-reduce bucket or - byte_cap - more than Engine.flush_bytes of partials are pending.  False (and nothing done): `plan` does not defer.
        stats_records passes byte_cap=False: statistics records add no pending bytes, so the cap is never their reason to flush (a bucket change is)."""
        if not self.defers(plan):
            return False
        bucket = self.e.dist.bucket_of(dw_off) if self.e.dist is not None else 0
        if (self.pending or self.later) and (bucket != self.pending_bucket or (byte_cap and self.pending_bytes > self.e.flush_bytes)):
            self.flush()
        self.pending_bucket = bucket
        return True

    def private_ws(self, d, nbytes: int):        # d reduces in a zeroed fp32 workspace of its own (private until the flush; zeroed: the tail convention)
        ws = self.alloc(((nbytes + 3) // 4,), torch.float32, zero=True)
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel() * 4

    # -- deferred weight-gradient reductions: the partial sums of many weight gradients (all-taps block partials, K-slice slabs)
    #    are added into dW by ONE batched launch instead of one small launch each (80 of them per cfg3 step).  Under data
    #    parallel the batch is flushed whenever the next weight gradient belongs to another all-reduce bucket, so a bucket's
    #    gradients are final - and its all-reduce starts - as early as before.
    def defer(self, d, dw_off: int):
        lib = L.lib()
        rec = L.WgradPending()
        d.defer = 1
        lib.call("rua_wgrad_plan", C.byref(d), C.byref(rec))           # with the shared scratch: which kind of partials, if any
        if rec.kind == 0:
            d.defer = 0
            return
        # exactly the partials this call writes (all-taps: one per CU and output-channel half; slabs: one dW per K slice) + the tail
        nbytes = (self.e.cu_count * 9 * 32 * rec.CC * 4 if rec.kind == 1 else rec.parts * rec.n * 4) + WS_TAIL_BYTES
        self.private_ws(d, nbytes)
        lib.call("rua_wgrad_plan", C.byref(d), C.byref(rec))           # the record for the private workspace
        assert rec.kind != 0
        self.pending.append((rec, dw_off))
        self.pending_bytes += nbytes

    def one(self, plan, sp: WSpec, d=None):
        """One weight gradient (d: its descriptor, where the caller has built it already): launched here, or held back."""
        d = self.desc(sp) if d is None else d
        if not self.hold_back(plan, sp, d):
            if self.admit(plan, sp.dw_off):
                self.defer(d, sp.dw_off)
            self.issue(plan, [d], "rua_conv_wgrad")

    # -- batched weight gradients: the generic-tile weight gradients of a step (the wide 1x1 convolutions on small maps: 2 - 13 us apiece, each a launch that
    #    splits its K range to fill the chip alone) are not launched where they are recorded.  They wait in `later` and go out as ONE rua_conv_wgrad_group call
    #    (its batched form: one compact grid, one block budget) IMMEDIATELY IN FRONT OF every flush - a bucket change, Engine.flush_bytes, the end of
    #    backward.  The flush invariant: the pending records of a held-back member are created by that call's recording (issue_later), so they can never be
    #    reduced before their slabs are written, and under data parallel a bucket's gradients are final at the same flush as with one launch each.
    def hold_back(self, plan, sp: WSpec, d) -> bool:
        """Hold this weight gradient back for the batched launch in front of the next flush; False: the caller launches it here.  Candidates: bf16 backward
        plans with deferred reductions, rua_wgrad_kind() == 0 and no whole-image kernel.  Holding a launch back is sound only while nothing writes its operands
        between the recorded position and the flush: `a` is a forward activation (or its pooled / normalised copy) and `dy` the finished gradient of the
        convolution's output; the graph owns every buffer for its lifetime (alloc) and the backward rewrites neither.  The one explicit storage reuse of the
        backward, the ResBlocks' g1s = g2s, holds gradients of 3x3 branch convolutions: all-taps / wgrad_dmap / whole-image launches, never candidates here."""
        if not self.defers(plan) or sp.in_bn is not None or self.dt != L.RUA_BF16 or not self.e.batch_wgrad:
            return False
        lib = L.lib()
        if lib.raw("rua_wgrad_kind")(C.byref(d)) != 0 or lib.raw("rua_wgrad_img_kind")(C.byref(d)) != 0:
            return False
        self.admit(plan, sp.dw_off)
        d.batch, d.defer = 1, 1
        self.later.append((d, sp.dw_off))
        return True

    def issue_later(self):
        """The held-back weight gradients as one rua_conv_wgrad_group call, and the pending records of the slabs it leaves."""
        if not self.later:
            return
        lib, plan = L.lib(), self.bwd
        n = len(self.later)
        arr = (L.WgradDesc * n)(*[d for d, _ in self.later])
        recs = (L.WgradPending * n)()
        lib.call("rua_wgrad_group_plan", arr, n, recs)                   # with the shared scratch: which members leave slabs, and how many
        for i in range(n):
            if recs[i].kind != 0:
                nbytes = recs[i].parts * recs[i].n * 4 + WS_TAIL_BYTES
                self.private_ws(arr[i], nbytes)                          # as in defer
                self.pending_bytes += nbytes
        first = [(recs[i].kind, recs[i].parts) for i in range(n)]
        lib.call("rua_wgrad_group_plan", arr, n, recs)                   # the records for the private workspaces
        assert first == [(recs[i].kind, recs[i].parts) for i in range(n)]
        for i, (_, off) in enumerate(self.later):
            if recs[i].kind != 0:
                self.pending.append((L.WgradPending.from_buffer_copy(recs[i]), off))
        plan.keep.append(arr)
        prev, plan.scope = plan.scope, "wgrad_batch"
        plan.add("rua_conv_wgrad_group", arr, n, grads=[off for _, off in self.later])
        plan.scope = prev
        self.later = []

    def group(self, plan, specs: List[WSpec]):
        """Independent weight gradients (the dilation branches of a ResBlock) in one call: members on the same kernel share ONE
        grid.  specs: (a, dy, dw_off, stride, dil, taps, in_bn).  Under data parallel the group counts as one launch of the
        bucket of its first member (a pending-reduction flush can only come in front of the whole group)."""
        for part in chunks(specs, 1 if self.dry else L.RUA_MAX_WGRAD_GROUP):
            if len(part) == 1:
                self.one(plan, part[0])
                continue
            descs = [self.desc(sp, group=len(part)) for sp in part]
            if self.admit(plan, part[0].dw_off):               # only the first member may flush or move the current bucket
                for d, sp in zip(descs, part):
                    self.defer(d, sp.dw_off)
            self.issue(plan, descs, "rua_conv_wgrad", "rua_conv_wgrad_group")

    def now_or_later(self, plan, specs: List[WSpec]) -> List[WSpec]:
        """The weight gradients of a ResBlock's SECOND convolutions: issued here - or returned, to ride in ONE group with the first convolutions' (whose
        dy exists three launches later).  Twice the members per grid = half the blocks per member: half the block partials to write and to reduce
        (levels 3 - 4: 24 MB per member) and half the ring fills per row of work.  Engine.merge_wgrad holds the channel counts that do."""
        if self.dry or len(specs) < 2 or 2 * len(specs) > L.RUA_MAX_WGRAD_GROUP or specs[0].a.C not in self.e.merge_wgrad:
            self.group(plan, specs)
            return []
        return specs

    def pw_group(self, plan, specs: List[WSpec]):
        """The narrow 1x1 weight gradients of one composite (the sources of a concatenating conv, the branch convs of a PSPPooling: independent, 2 - 15 us
        apiece and mostly launch ramp + drain) as ONE rua_conv_wgrad_group call.  The library runs them as one grid when every member is a wgrad_pw launch with
        replicas / tickets of its own - so each member gets a private (zeroed) workspace here; anything else falls back to one launch each, as before."""
        grouped = not self.dry and self.dt == L.RUA_BF16 and self.e.group_wgrad_pw
        for part in chunks(specs, L.RUA_MAX_BRANCH if grouped else 1):
            descs = [self.desc(sp) for sp in part]             # built once: probed here, then launched as they are
            if len(part) < 2 or not all(L.lib().raw("rua_wgrad_kind")(C.byref(d)) == 3 for d in descs):
                for sp, d in zip(part, descs):                 # one launch each - or, generic tiles, held back for the step's batched launch (hold_back)
                    self.one(plan, sp, d)
                continue
            if self.admit(plan, part[0].dw_off):               # as in group: the first member's bucket
                for d, sp in zip(descs, part):
                    self.defer(d, sp.dw_off)
            for d in descs:
                if not d.defer:                                # (d.defer: block partials, summed by the next rua_wgrad_reduce_batch: defer gave it a private workspace)
                    self.private_ws(d, int(L.lib().raw("rua_wgrad_workspace_bytes")(C.byref(d))))
            self.issue(plan, descs, "rua_conv_wgrad", "rua_conv_wgrad_group")

    def stats_records(self, s, Cc: int, offs: List[int]):
        """G[off .. off + Cc) += the per-channel sums of `s`, for every offset, as records of the next batched reduction launch (the plan defers: Graph.stats_to_grads)."""
        for o in offs:
            self.admit(self.bwd, o, byte_cap=False)
            rec = L.WgradPending()
            rec.kind, rec.parts, rec.n, rec.partials, rec.dw, rec.blocks = 3, s.R, Cc, s.ptr, self.G(o), (Cc + 255) // 256
            self.pending.append((rec, o))

    def flush(self):
        """What was held back goes out, then ONE rua_wgrad_reduce_batch over everything pending: behind it the gradients of every launch recorded so far are final."""
        self.issue_later()
        self.pending_bytes = 0
        if not self.pending:
            return
        blocks = 0
        for r, _ in self.pending:
            r.block_begin = blocks
            blocks += r.blocks
        recs = (L.WgradPending * len(self.pending))(*[r for r, _ in self.pending])
        table = torch.frombuffer(bytearray(bytes(recs)), dtype=torch.uint8).to(self.e.dev)
        self.keep(table)
        self.bwd.add("rua_wgrad_reduce_batch", table.data_ptr(), len(self.pending), blocks, grads=[off for _, off in self.pending])
        self.pending = []
