"""GPU (-m gpu): randomized differential test over the reference's config surface -- 36 small networks drawn from a fixed
generator (encoder block type, decoder block type, feature counts on and off the 32-channel tile, blocks per stage, per-axis
kernels / strides, conv_bias, SqueezeExcite, do_stem, 2-D / 3-D, 1-16 input channels, 1-20 output classes with and without
softmax, batch 1-3, ReLU / LeakyReLU, decoder convs per stage) against the CPU oracle in fp32 mode.  Logits carry the 2e-4 bar;
the data seeds are not curated for LeakyReLU mask margin, so gradients are checked by magnitude and direction (a mask flip moves a
tensor by 1e-3..2e-2, a wiring bug by O(1)): cosine > 0.99 and norm ratio within 3 % (0.9971 seen on a 4-stage BottleneckD draw), for every parameter that has a gradient --
and exactly the same set of parameters must have one."""
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

import resenc_oracle as oracle
from helpers import rel_l2


def draw(rng):
    two_d = rng.random() < 0.25
    nd = 2 if two_d else 3
    n_st = rng.choice([2, 3, 3, 4])
    base = rng.choice([16, 24, 32, 32, 40, 48])
    feats = [min(base * 2 ** i, rng.choice([96, 128, 160])) for i in range(n_st)]
    enc = rng.choice(["BasicBlockD", "BasicBlockD", "BottleneckBlockD", "ResidualBlock"])      # "ResidualBlock": the plain-conv quirk
    dec = rng.choice(["ConvBlock", "ConvBlock", "ResidualBlock"])
    aniso = (not two_d) and rng.random() < 0.3
    kernels, strides = [], []
    for s in range(n_st):
        k = [rng.choice([1, 3]) if aniso and s == 0 else 3 for _ in range(nd)]
        if all(v == 1 for v in k):
            k[-1] = 3          # (a 1x1x1 first layer on one input channel makes every channel the same affine map: ill-conditioned in 16 bits)
        st = ([2] * nd if rng.random() < 0.15 else [1] * nd) if s == 0 else [rng.choice([1, 2]) if aniso else 2 for _ in range(nd)]
        if s > 0 and all(v == 1 for v in st):
            st[-1] = 2
        kernels.append(k), strides.append(st)
    total = [1] * nd
    for st in strides:
        total = [a * b for a, b in zip(total, st)]
    patch = tuple(t * rng.choice([2, 3] if t >= 8 else [2, 4]) for t in total)
    if two_d:
        patch = tuple(max(p, 16) // t * t if False else p for p, t in zip(patch, total))
    mc = {"basic_encoder_block": enc, "basic_decoder_block": dec,
          "bottleneck_block": "BottleneckBlockD" if enc == "BottleneckBlockD" else "BasicBlockD",
          "features_per_stage": feats, "num_stages": n_st, "n_blocks_per_stage": [rng.choice([1, 2]) for _ in range(n_st)],
          "kernel_sizes": kernels, "n_conv_per_stage_decoder": [rng.choice([1, 2]) for _ in range(n_st - 1)], "strides": strides,
          "conv_bias": rng.random() < 0.5, "nonlin": rng.choice(["nn.LeakyReLU", "nn.LeakyReLU", "nn.ReLU"])}
    if enc != "ResidualBlock" and rng.random() < 0.35:
        mc["squeeze_excitation"] = True
    if rng.random() < 0.25:
        mc["do_stem"] = False
    classes = rng.choice([1, 1, 2, 3, 5, 12, 20])
    act = "softmax" if classes > 1 and rng.random() < 0.6 else ("sigmoid" if rng.random() < 0.5 else "none")
    tasks = {"t": {"channels": classes, "activation": act, "weight": 1, "loss_fn": "BCEDiceLoss", "loss_kwargs": {"alpha": 0.5, "beta": 0.5}}}
    if rng.random() < 0.3:
        tasks["n"] = {"channels": 3, "activation": "none", "weight": 0.5, "loss_fn": "MaskedCosineLoss"}
    return dict(patch=patch, cin=rng.choice([1, 1, 2, 3, 6, 8, 12, 16]), batch=rng.choice([1, 2, 3]), mc=mc, tasks=tasks)


def targets_for(c, outputs, seed):
    """targets at the OUTPUT extent (a strided first stage shrinks it: the reference's heads then live on the coarser grid)"""
    osp = tuple(next(iter(outputs.values())).shape[2:])
    return oracle.synthetic_batch(c["batch"], c["cin"], osp, c["tasks"], seed)[1]


def configs(n=36, seed=20260):
    seed = int(__import__("os").environ.get("RX_FUZZ_SEED", seed))      # (bug hunting: other draws than the committed ones)
    rng = random.Random(seed)
    return [draw(rng) for _ in range(n)]


@pytest.fixture(scope="module")
def NetworkFromConfig():
    import mt3d_amd  # noqa: F401
    from mt3d_amd.builders.build_network_from_config import NetworkFromConfig as N
    return N


def draw_geometry(rng):
    """round 3: the conv geometries and widths the engine used to refuse -- kernel sizes 1 / 3 / 5 / 7, strides 1..4 per axis and
    stage, 1..40 input channels, wide stems, heads beyond 64 classes, with the block / decoder variety of `draw`"""
    two_d = rng.random() < 0.2
    nd = 2 if two_d else 3
    n_st = rng.choice([2, 2, 3])
    base = rng.choice([16, 32, 32])
    feats = [min(base * 2 ** i, 64) for i in range(n_st)]
    enc = rng.choice(["BasicBlockD", "BasicBlockD", "BottleneckBlockD", "ResidualBlock"])
    dec = rng.choice(["ConvBlock", "ConvBlock", "ResidualBlock"])
    kernels, strides = [], []
    for s in range(n_st):
        k = [rng.choice([1, 3, 3, 5, 5, 7]) for _ in range(nd)]      # (odd: an even kernel shrinks the map under pad (k-1)//2 and the
        if all(v == 1 for v in k):                                   #  reference's own residual adds / concats then fail; op-level tests cover them)
            k[-1] = 5
        if s == 0:
            st = [rng.choice([1, 1, 1, 2, 3]) for _ in range(nd)] if rng.random() < 0.3 else [1] * nd
        else:
            st = [rng.choice([1, 2, 2, 3, 4]) for _ in range(nd)]
            if all(v == 1 for v in st):
                st[-1] = rng.choice([2, 3, 4])
        kernels.append(k), strides.append(st)
    total = [1] * nd
    for st in strides:
        total = [a * b for a, b in zip(total, st)]
    patch = tuple(t * rng.choice([2, 3] if t >= 6 else [3, 4, 6]) for t in total)
    mc = {"basic_encoder_block": enc, "basic_decoder_block": dec,
          "bottleneck_block": "BottleneckBlockD" if enc == "BottleneckBlockD" else "BasicBlockD",
          "features_per_stage": feats, "num_stages": n_st, "n_blocks_per_stage": [rng.choice([1, 2]) for _ in range(n_st)],
          "kernel_sizes": kernels, "n_conv_per_stage_decoder": [1] * (n_st - 1), "strides": strides,
          "conv_bias": rng.random() < 0.5, "nonlin": "nn.LeakyReLU"}
    if rng.random() < 0.25:
        mc["do_stem"] = False
    elif rng.random() < 0.3:
        mc["stem_channels"] = rng.choice([72, 96])
    classes = rng.choice([1, 2, 3, 70, 100])
    act = "softmax" if classes > 1 and rng.random() < 0.6 else ("sigmoid" if rng.random() < 0.5 else "none")
    tasks = {"t": {"channels": classes, "activation": act, "weight": 1, "loss_fn": "BCEDiceLoss", "loss_kwargs": {"alpha": 0.5, "beta": 0.5}}}
    return dict(patch=patch, cin=rng.choice([1, 2, 5, 17, 24, 33, 40]), batch=rng.choice([1, 2]), mc=mc, tasks=tasks)


def geometry_configs(n=24, seed=30303):
    seed = int(__import__("os").environ.get("RX_FUZZ_SEED", seed))
    rng = random.Random(seed)
    return [draw_geometry(rng) for _ in range(n)]


@pytest.mark.parametrize("i", range(24))
def test_random_geometry_matches_the_oracle(NetworkFromConfig, i):
    """24 draws of `draw_geometry` against the CPU oracle evaluated in fp64, same bars as test_random_config_matches_the_oracle.
    (fp64: torch's fp32 CPU convolution backward is not a usable reference for some of these geometries -- draw 22, a [7, 1, 3]
    kernel at stride [2, 2, 4], comes out uncorrelated with the fp64 evaluation at 1-32 threads (cosine 0.001-0.01) and right at
    128; the engine agrees with fp64 to 1 - 4e-13.  scripts/probes/geom22_probe.py)"""
    _check_against_oracle(NetworkFromConfig, geometry_configs()[i], i, oracle_dtype=torch.float64)


@pytest.mark.parametrize("i", range(36))
def test_random_config_matches_the_oracle(NetworkFromConfig, i):
    _check_against_oracle(NetworkFromConfig, configs()[i], i)


def _check_against_oracle(NetworkFromConfig, c, i, oracle_dtype=torch.float32):
    from mt3d_amd.engine.plan import UnsupportedConfig
    mgr = oracle.make_mgr(c["patch"], c["tasks"], c["cin"], c["batch"], False, c["mc"])
    torch.manual_seed(100 + i)
    try:
        ref = oracle.NetworkFromConfig(mgr).to(oracle_dtype)
    except (ValueError, AssertionError, RuntimeError, IndexError) as e:       # a topology the reference itself cannot build
        pytest.skip(f"oracle refuses: {type(e).__name__}: {e}")
    torch.manual_seed(100 + i)
    net = NetworkFromConfig(mgr).cuda()
    net.compute_dtype = torch.float32
    assert list(ref.state_dict().keys()) == list(net.state_dict().keys())
    x, t = oracle.synthetic_batch(c["batch"], c["cin"], c["patch"], c["tasks"], 7 + i)
    try:
        o_r = ref(x.to(oracle_dtype))
    except (RuntimeError, ValueError) as e:                                   # e.g. concat size mismatch of an odd topology
        pytest.skip(f"oracle forward fails: {e}")
    try:
        o_n = net(x.cuda())
    except UnsupportedConfig as e:
        pytest.skip(f"loudly rejected: {e}")
    for k in o_r:
        assert rel_l2(o_n[k].cpu(), o_r[k].detach()) < 2e-4, (c, k)
    t = targets_for(c, o_r, 7 + i)
    l_r = oracle.train_loss(o_r, {k: v.to(oracle_dtype) for k, v in t.items()}, c["tasks"])
    l_n = oracle.train_loss(o_n, {k: v.cuda() for k, v in t.items()}, c["tasks"])
    assert abs(l_r.item() - l_n.item()) < 1e-4 * max(1.0, abs(l_r.item()))
    l_r.backward()
    l_n.backward()
    pr, pn = dict(ref.named_parameters()), dict(net.named_parameters())
    for n in pr:
        assert (pr[n].grad is None) == (pn[n].grad is None), (c, n)
        if pr[n].grad is None or pr[n].grad.norm() < 1e-6:
            continue
        if n.endswith(".conv.weight") and pr[n][0].numel() == 1:
            continue                      # a 1x1x1 conv of ONE channel under an InstanceNorm: the norm removes its scale, d/dw is an eps-sized residue
        if n.endswith(".conv.bias"):      # in front of an InstanceNorm: analytically zero, both sides hold round-off
            wn = pr[n[:-len("bias")] + "weight"].grad.norm().item()
            assert pn[n].grad.norm().item() <= 1e-3 * wn + 1e-5, (c, n)
            continue
        a, b = pn[n].grad.double().flatten().cpu(), pr[n].grad.double().flatten()
        cos = (a @ b / (a.norm() * b.norm())).item()
        assert cos > 0.99 and abs(a.norm().item() / b.norm().item() - 1) < 3e-2, (c, n, cos, a.norm().item() / b.norm().item())
    ref.eval(); net.eval()
    with torch.no_grad():
        e_r, e_n = ref(x.to(oracle_dtype)), net(x.cuda())
    for k in e_r:
        assert rel_l2(e_n[k].cpu(), e_r[k]) < 2e-4, (c, k)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("i", range(0, 36, 2))
def test_random_config_low_precision_modes(NetworkFromConfig, i, dtype):
    """the same draw in the 16-bit throughput modes (other kernel instantiations: MFMA K tile 32, 16-byte vectors of 8): logits
    within the drift the reference's own autocast shows (4e-2 bf16 / 8e-3 fp16 of the fp32 oracle, x1.5 for the tiny extents
    drawn here), the loss within 3e-2, finite gradients for exactly the parameters the oracle gives one, two steps bit-identical."""
    c = configs()[i]
    mgr = oracle.make_mgr(c["patch"], c["tasks"], c["cin"], c["batch"], False, c["mc"])
    torch.manual_seed(100 + i)
    ref = oracle.NetworkFromConfig(mgr)
    torch.manual_seed(100 + i)
    net = NetworkFromConfig(mgr).cuda()
    net.compute_dtype = dtype
    x, t = oracle.synthetic_batch(c["batch"], c["cin"], c["patch"], c["tasks"], 7 + i)
    o_r = ref(x)
    t = targets_for(c, o_r, 7 + i)
    l_r = oracle.train_loss(o_r, t, c["tasks"])
    l_r.backward()
    runs = []
    from mt3d_amd.engine.plan import UnsupportedConfig
    for _ in range(2):
        net.zero_grad(set_to_none=True)
        try:
            o_n = net(x.cuda())
        except UnsupportedConfig as e:
            pytest.skip(f"loudly rejected: {e}")
        l_n = oracle.train_loss(o_n, {k: v.cuda() for k, v in t.items()}, c["tasks"])
        l_n.backward()
        runs.append(({k: v.detach().clone() for k, v in o_n.items()}, {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}))
    for k in o_r:
        assert torch.equal(runs[0][0][k], runs[1][0][k])
        tol = (7e-2 if dtype == torch.bfloat16 else 1.2e-2)
        vox = 1
        for d in c["patch"]:
            vox *= d
        if vox <= 256:
            tol *= 3            # (InstanceNorm over the 1-16 voxels of the deepest stage amplifies the 16-bit rounding: 2.6e-2 seen in fp16)
        assert rel_l2(runs[0][0][k].cpu(), o_r[k].detach()) < tol, (c, k, rel_l2(runs[0][0][k].cpu(), o_r[k].detach()))
    assert abs(l_r.item() - l_n.item()) < 3e-2 * max(1.0, abs(l_r.item()))
    have = {n for n, p in ref.named_parameters() if p.grad is not None}
    assert set(runs[0][1]) == have
    for n, g in runs[0][1].items():
        assert torch.isfinite(g).all(), n
        assert torch.equal(g, runs[1][1][n]), n


# ---- medium sizes: the persistent / halo / parity-class kernels only run above a few hundred tiles -------------------------------
def draw_medium(rng):
    n_st = rng.choice([3, 4, 4, 5])
    base = rng.choice([32, 32, 32, 24, 64])
    feats = [min(base * 2 ** i, 256) for i in range(n_st)]
    aniso = rng.random() < 0.4
    kernels, strides = [], []
    for s in range(n_st):
        k = [rng.choice([1, 3]) if aniso and s < 2 else 3 for _ in range(3)]
        if s == 0 and all(v == 1 for v in k):
            k[-1] = 3
        st = [1, 1, 1] if s == 0 else [rng.choice([1, 2]) if aniso and s < 3 else 2 for _ in range(3)]
        if s > 0 and all(v == 1 for v in st):
            st[rng.randrange(3)] = 2
        kernels.append(k), strides.append(st)
    total = [1, 1, 1]
    for st in strides:
        total = [a * b for a, b in zip(total, st)]
    patch = tuple(t * rng.choice([2, 3, 4, 5, 6, 8]) for t in total)
    while patch[0] * patch[1] * patch[2] > 96 ** 3 // 2:
        patch = tuple(max(t, p // 2 // t * t) for p, t in zip(patch, total))
    mc = {"basic_encoder_block": rng.choice(["BasicBlockD", "BasicBlockD", "BasicBlockD", "ResidualBlock", "BottleneckBlockD"]),
          "basic_decoder_block": rng.choice(["ConvBlock", "ConvBlock", "ResidualBlock"]),
          "features_per_stage": feats, "num_stages": n_st, "n_blocks_per_stage": [rng.choice([1, 2]) for _ in range(n_st)],
          "kernel_sizes": kernels, "n_conv_per_stage_decoder": [1] * (n_st - 1), "strides": strides,
          "conv_bias": rng.random() < 0.5, "squeeze_excitation": rng.random() < 0.3}
    mc["bottleneck_block"] = "BottleneckBlockD" if mc["basic_encoder_block"] == "BottleneckBlockD" else "BasicBlockD"
    if mc["basic_encoder_block"] == "ResidualBlock":
        mc["squeeze_excitation"] = False
    tasks = {"t": {"channels": rng.choice([1, 1, 2, 4]), "activation": "none", "weight": 1, "loss_fn": "BCEDiceLoss",
                   "loss_kwargs": {"alpha": 0.5, "beta": 0.5}}}
    if rng.random() < 0.3:
        tasks["n"] = {"channels": 3, "activation": "none", "weight": 1, "loss_fn": "MaskedCosineLoss"}
    return dict(patch=patch, cin=rng.choice([1, 1, 2, 4]), batch=rng.choice([1, 2, 2, 3]), mc=mc, tasks=tasks)


def medium_configs(n=16, seed=778):
    seed = int(__import__("os").environ.get("RX_FUZZ_SEED", seed))
    rng = random.Random(seed)
    return [draw_medium(rng) for _ in range(n)]


@pytest.mark.parametrize("i", range(16))
def test_random_medium_config_16bit_paths_agree_with_fp32(NetworkFromConfig, i):
    """draws with up to ~0.4 M voxels per sample, where the dispatch picks the LDS-halo, persistent, parity-class and split-K kernels
    (ragged tiles, per-axis kernels and strides, odd batch): the fp32 engine against the CPU oracle (logits 2e-4, loss), then the
    bf16 and fp16 engines against the fp32 engine (logits within the 16-bit drift, every gradient finite and pointing the same
    way for the tensors that carry most of the gradient mass), each 16-bit step bit-reproducible."""
    c = medium_configs()[i]
    mgr = oracle.make_mgr(c["patch"], c["tasks"], c["cin"], c["batch"], False, c["mc"])
    torch.manual_seed(300 + i)
    ref = oracle.NetworkFromConfig(mgr)
    torch.manual_seed(300 + i)
    net = NetworkFromConfig(mgr).cuda()
    x, t = oracle.synthetic_batch(c["batch"], c["cin"], c["patch"], c["tasks"], 40 + i)
    tc = {k: v.cuda() for k, v in t.items()}
    with torch.no_grad():
        o_r = ref(x)
    res = {}
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        net.compute_dtype = dt
        runs = []
        for _ in range(2 if dt != torch.float32 else 1):
            net.zero_grad(set_to_none=True)
            o = net(x.cuda())
            loss = oracle.train_loss(o, tc, c["tasks"])
            # fp16: per-voxel loss gradients of 1e-6 sit below the format's normal range -- scaled as the reference's GradScaler
            # does (train.py:94-97,224), un-scaled before comparing
            scale = 4096.0 if dt == torch.float16 else 1.0
            (loss * scale).backward()
            runs.append(({k: v.detach().clone() for k, v in o.items()}, loss.item(),
                         {n: p.grad / scale for n, p in net.named_parameters() if p.grad is not None}))
        if len(runs) == 2:
            assert all(torch.equal(runs[0][0][k], runs[1][0][k]) for k in runs[0][0]), (c, dt)
            assert all(torch.equal(runs[0][2][n], runs[1][2][n]) for n in runs[0][2]), (c, dt)
        res[dt] = runs[0]
    for k in o_r:
        assert rel_l2(res[torch.float32][0][k].cpu(), o_r[k]) < 2e-4, (c, k)
    g32 = res[torch.float32][2]
    top = sorted(g32, key=lambda n: -g32[n].norm().item())[:max(4, len(g32) // 4)]
    for dt, ltol in ((torch.bfloat16, 6e-2), (torch.float16, 1.2e-2)):
        for k in o_r:
            assert rel_l2(res[dt][0][k], res[torch.float32][0][k]) < ltol, (c, dt, k, rel_l2(res[dt][0][k], res[torch.float32][0][k]))
        assert abs(res[dt][1] - res[torch.float32][1]) < 3e-2 * max(1.0, abs(res[torch.float32][1]))
        assert set(res[dt][2]) == set(g32)
        for n, g in res[dt][2].items():
            assert torch.isfinite(g).all(), (c, dt, n)
        for n in top:
            a, b = res[dt][2][n].double().flatten(), g32[n].double().flatten()
            cos = (a @ b / (a.norm() * b.norm()).clamp_min(1e-30)).item()
            # (bf16 flips ~1 % of the LeakyReLU masks per layer: 0.78-0.9 seen on BottleneckD stacks, 0.98 in fp16; a wiring bug gives ~0)
            assert cos > (0.7 if dt == torch.bfloat16 else 0.95), (c, dt, n, cos)


# ---- channel dropout on random topologies: the same kept planes on both sides ---------------------------------------------------
@pytest.mark.parametrize("i", range(0, 36, 3))
def test_random_config_with_channel_dropout(NetworkFromConfig, i):
    """the draw of test_random_config_matches_the_oracle with `dropout_op_kwargs: {p: 0.3}`: the engine's masks (forced from a
    CPU generator, one per dropout layer in forward order) are handed to the oracle's nn.Dropout modules in their execution
    order; fp32 logits 2e-4, gradients by direction / magnitude, eval mode identical to the run without dropout."""
    from mt3d_amd.engine import plan as plan_mod
    c = configs()[i]
    p = 0.3
    mc = dict(c["mc"], dropout_op_kwargs={"p": p})
    mgr = oracle.make_mgr(c["patch"], c["tasks"], c["cin"], c["batch"], False, mc)
    torch.manual_seed(100 + i)
    ref = oracle.NetworkFromConfig(mgr)
    torch.manual_seed(100 + i)
    net = NetworkFromConfig(mgr).cuda()
    net.compute_dtype = torch.float32
    x, t = oracle.synthetic_batch(c["batch"], c["cin"], c["patch"], c["tasks"], 7 + i)
    gen = torch.Generator().manual_seed(900 + i)
    masks = {}

    def draw_mask(self, d):
        j = next(k for k, e in enumerate(self._drops) if e is d)
        if j not in masks:
            masks[j] = torch.bernoulli(torch.full(tuple(d.keep.shape), 1 - p), generator=gen)
        d.keep.copy_(masks[j])
    orig = plan_mod.Plan._draw_dropout
    plan_mod.Plan._draw_dropout = draw_mask
    try:
        try:
            o_n = net(x.cuda())
        except plan_mod.UnsupportedConfig as e:
            pytest.skip(f"loudly rejected: {e}")
        plan = next(iter(net._plans.values()))
        # the oracle's dropout modules in execution order; module k multiplies by mask k / (1 - p) on its real channels
        mods = []
        hooks = [m.register_forward_pre_hook(lambda mod, inp: mods.append(mod))
                 for m in ref.modules() if isinstance(m, (torch.nn.Dropout3d, torch.nn.Dropout2d))]
        with torch.no_grad():
            ref(x)
        for h in hooks:
            h.remove()
        assert len(mods) == len(plan._drops) == len(masks) > 0

        def forced(mk):
            def fwd(inp):
                cr = inp.shape[1]
                return inp * (mk[:, :cr] / (1 - p)).view(inp.shape[0], cr, *([1] * (inp.dim() - 2))).to(inp.dtype)
            return fwd
        for k, m in enumerate(mods):
            m.forward = forced(masks[k])
        o_r = ref(x)
        for k in o_r:
            assert rel_l2(o_n[k].cpu(), o_r[k].detach()) < 2e-4, (c, k, rel_l2(o_n[k].cpu(), o_r[k].detach()))
        t = targets_for(c, o_r, 7 + i)
        l_r = oracle.train_loss(o_r, t, c["tasks"])
        l_n = oracle.train_loss(o_n, {k: v.cuda() for k, v in t.items()}, c["tasks"])
        l_r.backward()
        l_n.backward()
    finally:
        plan_mod.Plan._draw_dropout = orig
    pr, pn = dict(ref.named_parameters()), dict(net.named_parameters())
    for n in pr:
        assert (pr[n].grad is None) == (pn[n].grad is None), (c, n)
        if pr[n].grad is None or pr[n].grad.norm() < 1e-6 or n.endswith(".conv.bias"):
            continue
        a, b = pn[n].grad.double().flatten().cpu(), pr[n].grad.double().flatten()
        cos = (a @ b / (a.norm() * b.norm())).item()
        assert cos > 0.99 and abs(a.norm().item() / b.norm().item() - 1) < 3e-2, (c, n, cos, a.norm().item() / b.norm().item())


# ---- launch programs on random launch lists ----------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [1, 5, 9, 13])
def test_random_medium_config_program_replay_is_bit_identical(NetworkFromConfig, monkeypatch, i):
    """recorded launch programs replay exactly what an eager pass issues, whatever the launch list: 5 bf16 training steps of a
    random medium draw with RX_PROGRAMS=1 and =0 end in identical losses and parameters"""
    c = medium_configs()[i]

    def run(programs):
        monkeypatch.setenv("RX_PROGRAMS", "1" if programs else "0")
        mgr = oracle.make_mgr(c["patch"], c["tasks"], c["cin"], c["batch"], False, c["mc"])
        torch.manual_seed(300 + i)
        net = NetworkFromConfig(mgr).cuda()
        net.compute_dtype = torch.bfloat16
        opt = torch.optim.SGD(net.parameters(), lr=0.05)
        losses = []
        for step in range(5):
            x, t = oracle.synthetic_batch(c["batch"], c["cin"], c["patch"], c["tasks"], 500 + step)
            out = net(x.cuda())
            loss = oracle.train_loss(out, {k: v.cuda() for k, v in t.items()}, c["tasks"])
            loss.backward()
            losses.append(loss.item())
            opt.step()
            opt.zero_grad(set_to_none=True)
        return losses, {n: p.detach().clone() for n, p in net.named_parameters()}
    l0, p0 = run(False)
    l1, p1 = run(True)
    assert l0 == l1
    for n in p0:
        assert torch.equal(p0[n], p1[n]), n


# ---- large irregular shapes: the full-resolution kernel instantiations (planar concat, fused statistics, fused head) ----------
def large_configs(n=6, seed=4242):
    seed = int(__import__("os").environ.get("RX_FUZZ_SEED", seed))
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        n_st = rng.choice([4, 5, 5, 6])
        total = 2 ** (n_st - 1)
        patch = tuple(total * rng.choice([3, 4, 5, 6, 7, 8]) for _ in range(3))
        while patch[0] * patch[1] * patch[2] > 2_400_000:
            patch = tuple(sorted(patch))
            patch = (patch[0], patch[1], patch[2] - total)
        mc = {"basic_encoder_block": "BasicBlockD", "basic_decoder_block": rng.choice(["ConvBlock", "ConvBlock", "ResidualBlock"]),
              "bottleneck_block": "BasicBlockD", "features_per_stage": [min(32 * 2 ** i, 256) for i in range(n_st)], "num_stages": n_st,
              "n_blocks_per_stage": [1] + [rng.choice([1, 2]) for _ in range(n_st - 1)], "kernel_sizes": [[3, 3, 3]] * n_st,
              "n_conv_per_stage_decoder": [1] * (n_st - 1), "strides": [[1, 1, 1]] + [[2, 2, 2]] * (n_st - 1),
              "conv_bias": rng.random() < 0.5, "squeeze_excitation": rng.random() < 0.4}
        tasks = {"t": {"channels": rng.choice([1, 2, 3]), "activation": "none", "weight": 1, "loss_fn": "BCEDiceLoss",
                       "loss_kwargs": {"alpha": 0.5, "beta": 0.5}}}
        if rng.random() < 0.4:
            tasks["n"] = {"channels": 3, "activation": "none", "weight": 1, "loss_fn": "MaskedCosineLoss"}
        out.append(dict(patch=patch, cin=rng.choice([1, 1, 2]), batch=rng.choice([1, 2, 3]), mc=mc, tasks=tasks))
    return out


@pytest.mark.parametrize("i", range(6))
def test_random_large_config_bf16_agrees_with_fp32_engine(NetworkFromConfig, i):
    """1-2.4 M voxels per sample with extents that are multiples of the total stride only (e.g. 96 x 112 x 80): the bf16 engine
    (persistent halo kernels, planar concat, statistics from conv epilogues, fused head, InstanceNorm-backward sums from
    data-gradient epilogues) against the fp32 engine (generic kernels): logits within the bf16 drift, loss, gradient direction of
    the heaviest tensors, two bf16 steps bit-identical.  (The fp32 engine is pinned to the oracle at the smaller sizes above.)"""
    c = large_configs()[i]
    mgr = oracle.make_mgr(c["patch"], c["tasks"], c["cin"], c["batch"], False, c["mc"])
    torch.manual_seed(700 + i)
    net = NetworkFromConfig(mgr).cuda()
    x, t = oracle.synthetic_batch(c["batch"], c["cin"], c["patch"], c["tasks"], 70 + i)
    x, t = x.cuda(), {k: v.cuda() for k, v in t.items()}
    res = {}
    for dt in (torch.float32, torch.bfloat16):
        net.compute_dtype = dt
        runs = []
        for _ in range(2 if dt == torch.bfloat16 else 1):
            net.zero_grad(set_to_none=True)
            o = net(x)
            loss = oracle.train_loss(o, t, c["tasks"])
            loss.backward()
            runs.append(({k: v.detach().clone() for k, v in o.items()}, loss.item(),
                         {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}))
        if len(runs) == 2:
            assert all(torch.equal(runs[0][0][k], runs[1][0][k]) for k in runs[0][0]), c
            assert all(torch.equal(runs[0][2][n], runs[1][2][n]) for n in runs[0][2]), c
        res[dt] = runs[0]
        net._plans = {k: v for k, v in net._plans.items() if v.dtype != torch.float32}      # free the fp32 buffers
        torch.cuda.empty_cache()
    lo, hi = res[torch.bfloat16], res[torch.float32]
    for k in hi[0]:
        assert rel_l2(lo[0][k], hi[0][k]) < 6e-2, (c, k, rel_l2(lo[0][k], hi[0][k]))
    assert abs(lo[1] - hi[1]) < 3e-2 * max(1.0, abs(hi[1]))
    assert set(lo[2]) == set(hi[2])
    top = sorted(hi[2], key=lambda n: -hi[2][n].norm().item())[:6]
    for n in top:
        a, b = lo[2][n].double().flatten(), hi[2][n].double().flatten()
        cos = (a @ b / (a.norm() * b.norm()).clamp_min(1e-30)).item()
        assert torch.isfinite(lo[2][n]).all() and cos > 0.7, (c, n, cos)
