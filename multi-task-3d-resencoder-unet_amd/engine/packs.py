"""Packed weights of a plan and the zero-padded shadows of its padded parameters.

No conv kernel reads a parameter: each reads a packed copy ([tap][Co][Ci] forward, [tap][Ci][Co] backward, compute dtype) that
`WeightPacks` refreshes when it went stale.  `Pack.stale` / `Pack.mark_fresh` are the ONLY definition of freshness: the plan's
re-pack, a replayed program or graph that re-packed, and the optimizers whose update kernel rewrites the packs all go through
them."""
import contextlib
from dataclasses import dataclass
from typing import List, Optional

import torch

from . import ops
from .replay import as_f32


@dataclass(eq=False)
class Pack:
    """the packed copies of one conv / transposed-conv weight (`param`: the parameter, or its padded shadow)"""
    param: torch.Tensor
    kind: str                           # "conv" | "convT"
    w_fwd: torch.Tensor
    w_bwd: Optional[torch.Tensor]       # None in an inference plan
    version: int = -1                   # param._version, param.data_ptr() and the model's weight epoch when last packed
    ptr: Optional[int] = None
    epoch: Optional[int] = None
    event: Optional[int] = None         # numbered event of the pack launch still in flight: the first consumer waits for it
    group: Optional[list] = None        # the entries packed by that launch (one event per group)
    deferred: bool = False              # held back by WeightPacks.refresh until the forward list reaches `issue_deferred`

    def stale(self, epoch):
        """Staleness: tensor version / address AND the model's weight epoch.  torch's FUSED optimizers (fused=True
        Adam/AdamW/SGD: `_fused_adamw_` ...) update parameters WITHOUT bumping `Tensor._version`, so a version check alone
        would keep the initial packed weights for a whole training run.  Every backward pass through the engine
        therefore starts a new weight epoch (an optimizer step is what normally follows it) and all plans of the model
        re-pack on their next forward; pure inference (no backward) keeps its packs."""
        p = self.param
        return self.epoch != epoch or self.version != p._version or self.ptr != p.data_ptr()

    def mark_fresh(self, epoch, event=None):
        """the packed copies hold the parameter as it is now (`event`: once that numbered event has passed)"""
        p = self.param
        self.version, self.ptr, self.epoch, self.event = p._version, p.data_ptr(), epoch, event


@dataclass(eq=False)
class Shadow:
    """Channel counts that are not a multiple of the kernels' K tile (features_per_stage is free in the reference,
    build_network_from_config.py:85-148): every activation buffer is PADDED to the next multiple, and each parameter that
    touches a padded extent gets a zero-padded fp32 SHADOW that the kernels read instead (refreshed from the real
    parameter in Plan._forward_pre; zero weights / bias keep the padding channels exactly 0 through conv, InstanceNorm,
    LeakyReLU, pool, transposed conv and head); its gradient is produced padded and sliced back in Plan._backward_finish.
    No kernel knows about it.  (Cost: the padded FLOPs and ~3 small torch copies per padded parameter and step.)"""
    param: torch.Tensor
    sh: torch.Tensor                    # the persistent zero tensor of the padded shape
    pairs: list                         # [(index into sh, index into param)]: the ranges of sh that mirror param
    seen: Optional[tuple] = None        # (version, address, weight epoch) of param when sh was last refreshed
    gpad: Optional[torch.Tensor] = None    # the padded gradient the kernels write (allocated by the first backward)

    def refresh(self, epoch):
        q = self.param
        tag = (q._version, q.data_ptr(), epoch)
        if self.seen != tag:
            src = q.detach()
            for dst, sidx in self.pairs:
                self.sh[dst].copy_(src[sidx])
            self.seen = tag


class WeightPacks:
    """The packs of one plan, in first-use order, and their refresh.  The packs are pure HBM traffic (1.7 GB at cfg2) while the
    first stages of the forward pass are MFMA/LDS bound: they run on the side stream in first-use order, in a few table
    launches (rx_pack_multi, 40 tensors each) in GROUPS of ~`limit` bytes of parameters with one numbered event per group.  The
    first convs of the forward wait for the first (small) group only; the other groups (the 512-channel stages: 80 % of the
    bytes) are DEFERRED: issued from inside the forward list, behind the full-resolution stage, where the packing competes with
    the 64^3 / 32^3 convolutions instead of the HBM-bound full-resolution InstanceNorm passes.  (Was: one launch + one event
    per tensor, 66 launches of 17 us on average per cfg2 step.)

    Of its plan it uses the side stream (`_pack_stream()`, `_side`), the fork event (`_ev_fork`) and the `_unstable_params` flag."""

    def __init__(self, plan, dtype, two_d):
        self.plan = plan
        self.dtype = dtype
        self.two_d = two_d
        self.entries: List[Pack] = []
        self.limit = 96 << 20           # fp32 parameter bytes per pack group
        self.slots: List[int] = []      # numbered event of pack group i (allocated on first use, handed back by release)
        self.deferred = None            # (groups, side stream, weight epoch) held back by refresh

    def __iter__(self):
        return iter(self.entries)

    def __len__(self):
        return len(self.entries)

    @staticmethod
    def groups(entries, limit, max_groups=4):
        """`entries` in order, split where the next tensor would pass `limit` fp32 bytes: [first ~limit] [next] [next] [rest]"""
        out, cur, cur_bytes = [], [], 0
        for ent in entries:
            nb = ent.param.numel() * 4
            if cur and cur_bytes + nb > limit and len(out) < max_groups - 1:
                out.append(cur)
                cur, cur_bytes = [], 0
            cur.append(ent)
            cur_bytes += nb
        if cur:
            out.append(cur)
        return out

    def by_param(self, wait_side=True):
        """the optimizers' preamble: {id(parameter): Pack}.  `wait_side`: the current stream first waits for the side stream
        (nobody may still read the packs / gradients that an update rewrites)"""
        if wait_side and self.plan._side is not None:
            torch.cuda.current_stream().wait_stream(self.plan._side)
        return {id(e.param): e for e in self.entries}

    def stale(self, epoch, force=False):
        return [e for e in self.entries if force or e.stale(epoch)]

    def mark_fresh(self, epoch):
        """a replayed program or graph re-packed every parameter"""
        for ent in self.entries:
            ent.mark_fresh(epoch)

    def refresh(self, epoch, force=False, defer=False):
        """re-pack every stale entry (all of them with `force`: inside a captured graph or a recorded program); `defer`: the
        forward list will call `issue_deferred`, all groups but the first wait for that"""
        stale = self.stale(epoch, force)
        if not stale:
            return
        side = self.plan._pack_stream()
        if side is not None:
            ops.event_record(self.plan._ev_fork)               # the optimizer's writes are on the main stream
            ops.stream_wait(self.plan._ev_fork, side)
        self._pack(stale, side, epoch, defer)

    def repack(self, entries, epoch):
        """re-pack `entries` on the side stream NOW (called from inside a `torch.cuda.stream(side)` block by the streamed
        optimizer step, right after the update of those parameters) and mark them fresh"""
        self._pack(entries, self.plan._side, epoch)

    def _pack(self, entries, side, epoch, defer=False):
        groups = self.groups(entries, self.limit)
        self.deferred = None
        if defer and side is not None and len(groups) > 1:
            self.deferred = (groups[1:], side, epoch)
            for grp in groups[1:]:
                for ent in grp:
                    ent.deferred = True       # a consumer that comes earlier than expected issues them itself (wait)
            groups = groups[:1]
        self._issue(groups, side, 0, epoch)

    def issue_deferred(self):
        """(from inside the forward list) the pack groups that refresh held back: ordered after the optimizer's writes by the
        fork event recorded there (the side stream executes in order), and before their first consumer by position in the list"""
        d, self.deferred = self.deferred, None
        if d is not None:
            groups, side, epoch = d
            ops.event_record(self.plan._ev_fork)               # main stream: everything up to here
            ops.stream_wait(self.plan._ev_fork, side)
            self._issue(groups, side, 1, epoch)

    def _issue(self, groups, side, gi0, epoch):
        with torch.cuda.stream(side) if side is not None else contextlib.nullcontext():
            for gi, grp in enumerate(groups, gi0):
                items = []
                for ent in grp:
                    w, copied = as_f32(ent.param)
                    if copied:
                        self.plan._unstable_params = True      # a temporary: its address is not replayable
                    if self.two_d:
                        w = w.unsqueeze(2)
                    items.append((w, 0 if ent.kind == "conv" else 1, ent.w_fwd, ent.w_bwd))
                ops.pack_weights_multi(items, self.dtype)
                slot = None
                if side is not None:
                    while len(self.slots) <= gi:
                        self.slots.append(ops.event_new())
                    slot = self.slots[gi]
                    ops.event_record(slot)
                for ent in grp:
                    ent.deferred, ent.group = False, grp
                    ent.mark_fresh(epoch, slot)

    def wait(self, ent):
        """the current stream waits for `ent`'s pack launch (the step of every consumer conv starts with this)"""
        if ent.deferred and self.deferred is not None:
            self.issue_deferred()
        if ent.event is not None:
            ops.stream_wait(ent.event)
            for e in ent.group:          # one event per pack group: the first consumer's wait covers them all (stream order)
                e.event = None

    def finish(self):
        """issue the pack groups still held back, then wait for every pack (parameters of unused branches included: never leave
        a pack in flight)"""
        self.issue_deferred()
        for ent in self.entries:
            self.wait(ent)

    def release(self):
        """forget the event slots; returns them (the plan hands them back to the library)"""
        slots, self.slots = self.slots, []
        for ent in self.entries:
            ent.event = None
        return slots
