"""CPU: every draw of the randomized GPU tests (tests/test_fuzz_gpu.py) builds its execution plan on the meta device -- forward and
backward launch lists, padded buffers, shadow parameters -- in both compute types; structural invariants only (no kernel runs)."""
import pytest
import torch

import mt3d_amd  # noqa: F401
import resenc_oracle as oracle
import test_fuzz_gpu as fz
from mt3d_amd.builders.build_network_from_config import NetworkFromConfig
from mt3d_amd.engine.plan import Plan, UnsupportedConfig


def _all_draws():
    return ([("small", i, c) for i, c in enumerate(fz.configs())] + [("medium", i, c) for i, c in enumerate(fz.medium_configs())]
            + [("large", i, c) for i, c in enumerate(fz.large_configs())])


_BUILT = {}


def _plans(dtype):
    """(draw kind, draw index, draw, net, training plan, inference plan) of every draw the engine supports; built once per dtype"""
    if dtype not in _BUILT:
        rows = []
        for kind, i, c in _all_draws():
            mgr = oracle.make_mgr(c["patch"], c["tasks"], c["cin"], c["batch"], False, c["mc"])
            net = NetworkFromConfig(mgr)
            shape = (c["batch"], c["cin"], *c["patch"])
            try:
                plan = Plan(net.to("meta"), shape, dtype, "meta", needs_grad=True)
            except UnsupportedConfig:
                continue
            rows.append((kind, i, c, net, plan, Plan(net, shape, dtype, "meta", needs_grad=False)))
        _BUILT[dtype] = rows
    return _BUILT[dtype]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_every_fuzz_draw_plans_on_the_meta_device(dtype):
    built = 0
    for kind, i, c, net, plan, ev in _plans(dtype):
        built += 1
        assert set(plan.outputs) == set(c["tasks"]), (kind, i)
        for name, info in c["tasks"].items():
            out = plan.outputs[name]
            assert out.shape[0] == c["batch"] and out.shape[1] == info["channels"], (kind, i, name)
        assert len(plan.fwd) > 0 and len(plan.bwd) > 0
        used = {id(p) for p in plan.params}
        # every parameter except the unused deep-supervision heads is an engine input
        for n, p in net.named_parameters():
            assert (id(p) in used) or ".seg_layers." in n, (kind, i, n)
        for e in plan._shadows:              # a shadow is at least as large as its parameter in every dimension
            assert all(a >= b for a, b in zip(e.sh.shape, e.param.shape)), (kind, i)
        assert len(ev.bwd) == 0
    assert built >= 55, built


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fusion_links_are_mutual(dtype):
    """every fusion link of a plan has its counterpart on the record it points at, and an inference plan carries no backward-only link"""
    seen = dict(stats=0, pool=0, head=0, head_src=0, head_dw=0, instats=0)
    for kind, i, c, net, plan, ev in _plans(dtype):
        for pl in (plan, ev):
            for tape in [pl.enc_tape] + pl.dec_tapes:
                where = (kind, i, pl.needs_grad)
                inacts = [r for r in tape if r.kind == "inact"]
                # statistics out of the conv / stem epilogue: the giver is that inact's producer of y, the inact knows
                givers = [r for r in tape if r.kind in ("conv", "stem") and r.stats_to is not None]
                for r in givers:
                    assert r.stats_to in inacts and r.stats_to.y is r.y and r.stats_to.stats_done, where
                assert sorted(map(id, (r.stats_to for r in givers))) == sorted(id(r) for r in inacts if r.stats_done), where
                # fused pools: exactly one producer points at each, and only fused pools are pointed at
                pooled = [r.pool_to for r in inacts if r.pool_to is not None]
                assert sorted(map(id, pooled)) == sorted(id(r) for r in tape if r.kind == "pool" and r.fused), where
                assert all(r.pool_to.x is r.out for r in inacts if r.pool_to is not None), where
                # heads computed by the layer below: exactly one inact points at each
                headed = [r.head_to for r in inacts if r.head_to is not None]
                assert sorted(map(id, headed)) == sorted(id(r) for r in tape if r.kind == "head" and r.fwd_fused), where
                assert all(r.head_to.x is r.out for r in inacts if r.head_to is not None), where
                for r in inacts:
                    assert not r.head_dw_fused or r.head_src is not None, where
                    if r.head_src is not None:
                        assert r.head_src.x is r.out and r.head_src.dx_fused and r.head_src.dw_fused == r.head_dw_fused, where
                    assert (r.m12 is not None) == any(q.kind == "conv" and q.instats_for is r for t in [pl.enc_tape] + pl.dec_tapes
                                                      for q in t), where
                for r in tape:
                    if r.kind == "head" and (r.dx_fused or r.dw_fused):
                        assert sum(q.head_src is r for q in inacts) == 1, where
                if not pl.needs_grad:        # the backward-only links
                    assert all(r.head_src is None and not r.head_dw_fused and r.m12 is None and r.m12x is None for r in inacts), where
                    assert all(r.instats_for is None for r in tape if r.kind == "conv"), where
                    assert all(not r.dx_fused and not r.dw_fused for r in tape if r.kind == "head"), where
                    assert all(at.last_writer is None and at.pool_pending is None and at.gact is None
                               for r in tape for at in (getattr(r, "x", None), getattr(r, "y", None), getattr(r, "out", None))
                               if at is not None and not isinstance(at, torch.Tensor)), where
                seen["stats"] += len(givers)
                seen["pool"] += len(pooled)
                seen["head"] += len(headed)
                seen["head_src"] += sum(r.head_src is not None for r in inacts)
                seen["head_dw"] += sum(r.head_dw_fused for r in inacts)
                seen["instats"] += sum(r.m12 is not None for r in inacts)
    if dtype == torch.float32:      # every fusion needs a 16-bit compute type, except the block-output pool
        assert all(v == 0 for k, v in seen.items() if k != "pool"), seen
    else:                           # the draws reach every link (or the conditions above check nothing)
        assert all(v > 0 for v in seen.values()), seen
