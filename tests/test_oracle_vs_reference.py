"""CPU: the oracle against what the REAL reference computed (tests/golden/parity/, made by
oracle/make_golden_parity.py where the reference tree exists): same state_dict bit for bit, same train-mode
outputs, same loss, same gradients, same autoconfigured topology."""
import json
import os

import numpy as np
import pytest
import torch

import resenc_oracle as oracle
from golden_cases import CASES
from make_golden_parity import AUTOCONFIG_PATCHES, GRAD_SAMPLE, THREADS, grad_sample_index, tensor_digest

PARITY = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "parity")


@pytest.fixture
def threads():
    n = torch.get_num_threads()
    torch.set_num_threads(THREADS)          # the fixture's thread count: the same summation order in every reduction
    yield
    torch.set_num_threads(n)


@pytest.mark.parametrize("case", list(CASES))
def test_state_dict_and_forward_backward_equal(case, threads):
    ref = np.load(os.path.join(PARITY, f"{case}.npz"), allow_pickle=False)
    c = CASES[case]
    mgr = oracle.make_mgr(c["patch"], c["tasks"], c["in_channels"], 1, c["autoconfigure"], c["model_config"])
    torch.manual_seed(c["seed"])
    mine = oracle.NetworkFromConfig(mgr)
    sm = mine.state_dict()
    assert list(sm.keys()) == json.loads(str(ref["state_dict_keys"]))      # same keys in the same order
    for k, digest in zip(sm, json.loads(str(ref["state_dict_sha256"]))):
        assert tensor_digest(sm[k]) == digest, k                                     # same seeded init, bit for bit
    x, targets = oracle.synthetic_batch(c["batch"], c["in_channels"], c["patch"], c["tasks"], c["data_seed"])
    mine.train()
    torch.manual_seed(77)                              # (channel dropout draws its masks from the global generator)
    o_m = mine(x)
    assert list(o_m) == json.loads(str(ref["out_keys"]))
    for k in o_m:
        # identical op sequence -> identical bits on the machine that made the fixture; another CPU may pick other oneDNN
        # convolution kernels (other fp32 summation orders), so the stored outputs are matched to fp32 round-off
        assert torch.allclose(torch.from_numpy(ref[f"out.{k}"]), o_m[k], rtol=1e-4, atol=1e-5), k
    l_m = oracle.train_loss(o_m, targets, c["tasks"])
    assert abs(float(ref["loss"]) - l_m.item()) < 1e-6
    l_m.backward()
    names = json.loads(str(ref["param_names"]))
    has_grad = ref["param_has_grad"]
    assert [n for n, _ in mine.named_parameters()] == names
    for (n, p), hg in zip(mine.named_parameters(), has_grad):
        assert (p.grad is None) == (not hg), n
        if p.grad is None:
            continue
        g = p.grad.flatten()
        if g.numel() > GRAD_SAMPLE:
            # the whole tensor through sums that the element-wise bound below implies, the elements through a fixed sample
            s, sa, l2 = ref[f"grad_sums.{n}"]
            gd = p.grad.double()
            bound = 1e-4 * gd.abs().sum().item() + 1e-7 * g.numel()
            assert abs(gd.sum().item() - s) <= bound and abs(gd.abs().sum().item() - sa) <= bound, n
            assert abs(gd.norm().item() - l2) <= 1e-4 * gd.norm().item() + 1e-7 * g.numel() ** 0.5, n
            g = g[grad_sample_index(g.numel())]
        assert torch.allclose(torch.from_numpy(ref[f"grad.{n}"]), g, rtol=1e-4, atol=1e-7), n


def test_autoconfig_topology_matches_reference_for_baseline_patches():
    with open(os.path.join(PARITY, "autoconfig.json")) as f:
        rows = json.load(f)
    assert [tuple(r["patch"]) for r in rows] == AUTOCONFIG_PATCHES
    for r in rows:
        patch = tuple(r["patch"])
        _, s_m, k_m = oracle.plan_pooling(patch, 4, (1.0,) * len(patch), 999999)
        assert [list(s) for s in s_m] == r["strides"] and [list(k) for k in k_m] == r["kernels"], patch
        assert oracle.blocks_per_stage(len(s_m)) == r["n_blocks_per_stage"]
