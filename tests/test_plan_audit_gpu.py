"""GPU (-m gpu): the wiring of engine/plan.py in the 16-bit compute types, audited launch by launch (tests/plan_audit.py).

Two training steps of a small network run through a recording proxy of `ops`.  Step 1 holds every launch to the per-element bound
of its op test, given the bytes it read; before each pass of step 2 everything the same pass wrote in step 1 is NaN, and every
launch must read and leave finite values only -- a stale m12, an accumulate into an unwritten gradient view, an output that was not
stored but is still read each name their launch.  Both losses must equal, bit for bit, those of the same two steps (an SGD step
between them) without the proxy and without the poison.  Each case ends with its launch ledger: the fused entry points and
variants it is there for must have been seen.

Shapes: patch (8, 16, 16), batch 2, two stages.  Stage 0 (2048 voxels, x extent 16, 32 channel buffers) meets every condition of
the dtype-gated fusions (`_above_single_launch`, `_halo_x_ok`, c % 32, the fused head's widths); stage 1 (256 voxels) takes the
single-launch InstanceNorm path.  Two blocks in stage 0: the first block's output is not pooled (bwd_res without pool_dy), the second
one's is (pool_fwd, bwd_res with pool_dy).

A conv3d_bwd_data_instats that DELIVERS m12 needs the persistent halo kernel: 32 -> 32 channels from 512 tiles of 4 x 4 x 16
voxels (csrc/rx_conv_halo_plan.h), batch 2 of (32, 32, 64).  fp64 references of every convolution of such a step take minutes,
so test_instats_chain audits by reference only the launches it is there for -- conv3d_bwd_data_instats (dx, and check_m12 on the
delivered sums) and instnorm_act_bwd_apply, which must read an m12 that a fused launch of the same pass left -- and holds every
other launch of that plan to the stale-state check alone; their references are the business of the small configurations.

The image and the stem weights are rounded to values representable in bf16 and fp16, as
the stem op test's are, because the 16-bit stem kernels convert both."""
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

import resenc_oracle as oracle
from golden_cases import TASKS_2HEAD, _manual
from plan_audit import install

PATCH, BATCH = (8, 16, 16), 2


def _mc(**kw):
    return _manual(features_per_stage=[32, 64], num_stages=2, n_blocks_per_stage=[2, 1], kernel_sizes=[3, 3],
                   n_conv_per_stage_decoder=[1], strides=[1, 2], conv_bias=True, **kw)


# name -> (model config, tasks in the loss, what the ledger must hold in a 16-bit type)
CONFIGS = {
    "plain": (_mc(), ("sheet", "normals"),
              {"stem_conv_fwd_stats", "conv3d_fwd_stats", "instnorm_act_head_fwd:out=None", "instnorm_act_pool_fwd",
               "conv3d_bwd_data_instats", "instnorm_act_bwd_head:dw", "instnorm_act_bwd_res:pool",
               "instnorm_act_bwd_res:nopool"}),
    # 24 / 48 features in 32 / 64 channel buffers: the head reads a padded shadow of its weight, so its dw / db stay with head_bwd
    "padded": (dict(_mc(), features_per_stage=[24, 48]), ("sheet", "normals"),
               {"stem_conv_fwd_stats", "conv3d_fwd_stats", "instnorm_act_head_fwd:out=stored", "instnorm_act_bwd_head:nodw",
                "head_bwd:dx=None", "conv3d_bwd_data_instats", "instnorm_act_pool_fwd"}),
    # channel dropout, and one task outside the loss
    "dropout_task_out": (_mc(dropout_op_kwargs={"p": 0.2}), ("sheet",),
                         {"conv3d_fwd_stats", "stem_conv_fwd_stats", "fused_stats->mask", "instnorm_stats_mask",
                          "head_src:dlogits=None", "instnorm_act_bwd_head:dw"}),
}
FP32_LEDGER = {"instnorm_act_bwd_res:pool", "instnorm_act_bwd_res:nopool", "instnorm_act_pool_fwd", "head_fwd", "head_bwd",
               "conv3d_bwd_data", "instnorm_act_bwd"}


@pytest.fixture(scope="module")
def NetworkFromConfig():
    import mt3d_amd  # noqa: F401
    from mt3d_amd.builders.build_network_from_config import NetworkFromConfig as N
    from mt3d_amd.engine import lib
    lib.require_device()
    return N


def rnd16_(t):
    """in place: round to values representable in bf16, fp16 and fp32 (tests/test_stem_head_gpu.py::rnd16)"""
    with torch.no_grad():
        r = t.to(torch.bfloat16).to(t.dtype)
        t.copy_(torch.where(r.abs() < 2.0 ** -14, torch.zeros_like(r), r))
    return t


def round_stem(net):
    for m in net.shared_encoder.stem.convs:
        rnd16_(m.spec()["conv"].weight)


def make_net(N, monkeypatch, mc, patch=PATCH, tasks=TASKS_2HEAD):
    monkeypatch.setenv("RX_PROGRAMS", "0")          # one host call per launch
    mgr = oracle.make_mgr(patch, tasks, 1, BATCH, False, mc)
    torch.manual_seed(4)
    net = N(mgr).cuda()
    round_stem(net)
    return net


def batch(seed, patch=PATCH, tasks=TASKS_2HEAD):
    x, targets = oracle.synthetic_batch(BATCH, 1, patch, tasks, seed)
    return rnd16_(x).cuda(), {k: v.cuda() for k, v in targets.items()}


def two_steps(N, monkeypatch, mc, dtype, in_loss, audited, patch=PATCH, tasks=TASKS_2HEAD, only=None):
    net = make_net(N, monkeypatch, mc, patch, tasks)
    A = install(monkeypatch, net, only) if audited else None
    opt = torch.optim.SGD(list(net.parameters()), lr=0.05)
    losses = []
    for step in range(2):
        x, targets = batch(100 + step, patch, tasks)
        net.train()
        if A:
            A.begin("fwd", strict=step == 1)
        with torch.autocast("cuda", dtype=dtype, enabled=dtype != torch.float32):
            out = net(x)
        if A:
            A.check()
        loss = oracle.train_loss({k: out[k] for k in in_loss}, {k: targets[k] for k in in_loss}, tasks)
        if A:
            A.begin("bwd", strict=step == 1)
        loss.backward()
        if A:
            A.check()
        losses.append(loss.item())
        assert all(torch.isfinite(v).all() for v in out.values()), "a logit is not finite"
        for n, p in net.named_parameters():
            if any(n.startswith(f"task_decoders.{t}.") for t in tasks if t not in in_loss):
                # (its head gets no gradient; the decoder under it runs its backward on a zeroed output gradient)
                assert p.grad is None or (p.grad == 0).all(), f"{n} belongs to a task outside the loss and has a gradient"
            else:
                assert p.grad is not None and torch.isfinite(p.grad).all(), f"gradient of {n} is missing or not finite"
        if A and step == 1:      # the stale-state check had something to bite on, in both passes
            assert A.poisoned["fwd"] > 0 and A.poisoned["bwd"] > 0, (A.poisoned, A.kept_live)
        opt.step()
        round_stem(net)
        opt.zero_grad(set_to_none=True)
    return losses, A


def audit_case(N, monkeypatch, mc, dtype, in_loss, ledger, **kw):
    t0 = time.time()
    plain, _ = two_steps(N, monkeypatch, mc, dtype, in_loss, audited=False, **{k: v for k, v in kw.items() if k != "only"})
    monkeypatch.undo()
    t1 = time.time()
    audited, A = two_steps(N, monkeypatch, mc, dtype, in_loss, audited=True, **kw)
    print(f"\nplan audit: {len(A.calls)} launches audited, {time.time() - t1:.1f} s (plain run {t1 - t0:.1f} s); poisoned ranges "
          f"{A.poisoned}, kept as live activations {A.kept_live}; ops seen: {sorted(A.ledger)}")
    assert audited == plain, f"losses with the proxy and the poison {audited} differ from those without {plain}"
    missing = ledger - A.ledger
    assert not missing, f"the audit never reached {sorted(missing)}; saw {sorted(A.ledger)}"
    return A


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_training_plan_audit(NetworkFromConfig, monkeypatch, config, dtype):
    mc, in_loss, ledger = CONFIGS[config]
    A = audit_case(NetworkFromConfig, monkeypatch, mc, dtype, in_loss, ledger)
    if config == "dropout_task_out":
        plan = next(p for p in A.net._plans.values() if p.needs_grad)
        assert plan._drops and all(d.p == 0.2 for d in plan._drops)


SHEET = {"sheet": TASKS_2HEAD["sheet"]}


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_instats_chain(NetworkFromConfig, monkeypatch, dtype):
    """the backward-data launch that completes a layer's output gradient leaves that layer's two backward means, and the layer's
    apply pass consumes them: one block at full resolution (stem -> conv1 -> conv2), one task, 512 tiles"""
    mc = _manual(features_per_stage=[32, 64], num_stages=2, n_blocks_per_stage=[1, 1], kernel_sizes=[3, 3],
                 n_conv_per_stage_decoder=[1], strides=[1, 2])
    A = audit_case(NetworkFromConfig, monkeypatch, mc, dtype, ("sheet",), {"conv3d_bwd_data_instats", "instats->apply"},
                   patch=(32, 32, 64), tasks=SHEET, only={"conv3d_bwd_data_instats", "instnorm_act_bwd_apply"})
    assert A.names("bwd").count("instnorm_act_bwd_apply") >= 2      # once per step at least


def test_training_plan_audit_fp32(NetworkFromConfig, monkeypatch):
    """the auditors are dtype-generic: the branches that are not dtype-gated (`_bwd_inact_res`, `pool_pending`, `_fuse_block_pool`)
    under the same stale-state check"""
    mc, in_loss, _ = CONFIGS["plain"]
    A = audit_case(NetworkFromConfig, monkeypatch, mc, torch.float32, in_loss, FP32_LEDGER)
    gated = {"conv3d_fwd_stats", "stem_conv_fwd_stats", "instnorm_act_head_fwd", "conv3d_bwd_data_instats", "instnorm_act_bwd_head"}
    assert not (gated & A.ledger), f"fp32 plan took a 16-bit fusion: {sorted(gated & A.ledger)}"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_inference_plan_audit(NetworkFromConfig, monkeypatch, dtype):
    """needs_grad=False: `keep` is False in `with_head`, nobody stores the activated output under the head"""
    t0 = time.time()
    net = make_net(NetworkFromConfig, monkeypatch, CONFIGS["plain"][0])
    A = install(monkeypatch, net)
    net.eval()
    outs = []
    for step in range(2):
        x, _ = batch(100 + step)
        A.begin("fwd", strict=step == 1)
        with torch.no_grad(), torch.autocast("cuda", dtype=dtype):
            outs.append(net(x))
        A.check()
        assert all(torch.isfinite(v).all() for v in outs[-1].values())
    monkeypatch.undo()
    monkeypatch.setenv("RX_PROGRAMS", "0")
    with torch.no_grad(), torch.autocast("cuda", dtype=dtype):
        again = net(batch(101)[0])
    assert all(torch.equal(again[k], outs[1][k]) for k in again), "logits with the proxy and the poison differ from those without"
    plan, = net._plans.values()
    assert not plan.needs_grad
    want = {"instnorm_act_head_fwd:out=None", "conv3d_fwd_stats", "stem_conv_fwd_stats", "instnorm_act_pool_fwd"}
    print(f"\nplan audit (inference): {len(A.calls)} launches audited, {time.time() - t0:.1f} s; ops seen: {sorted(A.ledger)}")
    assert not (want - A.ledger), f"the audit never reached {sorted(want - A.ledger)}; saw {sorted(A.ledger)}"
