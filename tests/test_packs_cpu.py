"""CPU: the weight packs of a plan (engine/packs.py) without a plan -- the grouping rule, the one definition of freshness, and
a `WeightPacks` over CPU tensors with a stand-in `ops` and no side stream: what is packed, when, and in which order."""
import types

import pytest
import torch

import mt3d_amd  # noqa: F401
from mt3d_amd.engine import packs as P
from mt3d_amd.engine.packs import Pack, WeightPacks


def entry(numel=8, kind="conv"):
    return Pack(param=torch.zeros(numel), kind=kind, w_fwd=torch.zeros(numel), w_bwd=torch.zeros(numel))


def sizes(groups):
    return [[e.param.numel() for e in g] for g in groups]


def test_groups_of_nothing():
    assert WeightPacks.groups([], 100) == []


def test_groups_keep_one_tensor_over_the_limit_whole():
    e = entry(1000)
    assert WeightPacks.groups([e], 16) == [[e]]
    assert sizes(WeightPacks.groups([entry(1000), entry(2)], 16)) == [[1000], [2]]


def test_groups_split_where_the_next_tensor_would_pass_the_limit():
    ents = [entry(4), entry(4), entry(4)]           # 16 fp32 bytes each
    assert sizes(WeightPacks.groups(ents, 32)) == [[4, 4], [4]]          # exactly at the limit: no split yet
    assert sizes(WeightPacks.groups(ents, 31)) == [[4], [4], [4]]
    assert sizes(WeightPacks.groups(ents, 48)) == [[4, 4, 4]]


def test_groups_fourth_takes_the_rest_and_order_is_kept():
    ents = [entry(n) for n in (1, 2, 3, 4, 5, 6, 7)]
    got = WeightPacks.groups(ents, 1)
    assert sizes(got) == [[1], [2], [3], [4, 5, 6, 7]]
    assert [e for g in got for e in g] == ents                            # the same objects, in order
    assert sizes(WeightPacks.groups(ents, 1, max_groups=2)) == [[1], [2, 3, 4, 5, 6, 7]]


def test_pack_is_stale_until_marked_and_by_each_criterion_alone():
    e = entry()
    assert e.stale(0)                               # never packed
    e.mark_fresh(0)
    assert not e.stale(0) and e.event is None
    e.param.add_(1)                                 # version
    assert e.stale(0)
    e.mark_fresh(0, event=5)
    assert not e.stale(0) and e.event == 5
    assert e.stale(1)                               # weight epoch
    e.mark_fresh(1)
    assert not e.stale(1)
    moved = torch.zeros(8)
    while moved._version < e.param._version:
        moved.add_(0)
    e.param = moved                                # address: same version, same epoch, other storage
    assert e.version == moved._version and e.stale(1)
    e.mark_fresh(1)
    assert not e.stale(1)


class FakeOps:
    def __init__(self):
        self.calls = []

    def pack_weights_multi(self, items, dtype):
        self.calls.append([w for w, _, _, _ in items])

    def __getattr__(self, name):                    # no side stream: no event may be made, recorded or waited for
        raise AssertionError(f"ops.{name} called without a side stream")


@pytest.fixture
def packs(monkeypatch):
    ops = FakeOps()
    monkeypatch.setattr(P, "ops", ops)
    plan = types.SimpleNamespace(_side=None, _ev_fork=None, _unstable_params=False, _pack_stream=lambda: None)
    wp = WeightPacks(plan, torch.bfloat16, two_d=False)
    wp.entries += [entry(n, kind) for n, kind in ((8, "conv"), (16, "convT"), (24, "conv"))]
    return wp, ops, plan


def packed(ops):
    """numel of every tensor packed since the last look, in launch order"""
    out = [w.numel() for call in ops.calls for w in call]
    del ops.calls[:]
    return out


def test_refresh_packs_what_is_stale_once_and_in_order(packs):
    wp, ops, plan = packs
    assert len(wp) == 3 and list(wp) == wp.entries and len(wp.stale(0)) == 3
    wp.refresh(0, defer=True)                       # (nothing is deferred without a side stream)
    assert packed(ops) == [8, 16, 24] and wp.deferred is None and not wp.stale(0)
    wp.finish()
    assert all(e.event is None and not e.deferred for e in wp) and wp.slots == []
    wp.refresh(0)
    assert packed(ops) == []                        # fresh: nothing
    wp.entries[1].param.add_(1)
    assert wp.stale(0) == [wp.entries[1]]
    wp.refresh(0)
    assert packed(ops) == [16]                      # a version bump: that entry alone
    wp.refresh(1)
    assert packed(ops) == [8, 16, 24]               # a new weight epoch: all
    assert len(wp.stale(1, force=True)) == 3 and not wp.stale(1)
    wp.refresh(1, force=True)
    assert packed(ops) == [8, 16, 24]
    assert not plan._unstable_params


def test_groups_follow_the_limit_and_a_copied_parameter_is_flagged(packs):
    wp, ops, plan = packs
    wp.limit = 1
    wp.refresh(0)
    assert [len(c) for c in ops.calls] == [1, 1, 1] and packed(ops) == [8, 16, 24]
    wp.entries[0].param = torch.zeros(8, dtype=torch.float64)            # the pack launch reads an fp32 temporary
    wp.repack(wp.entries[:1], 0)
    assert ops.calls[0][0].dtype == torch.float32 and plan._unstable_params
    assert wp.by_param() == {id(e.param): e for e in wp.entries}
    wp.mark_fresh(3)
    assert not wp.stale(3) and wp.release() == []
