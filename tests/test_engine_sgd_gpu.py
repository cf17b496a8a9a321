"""GPU (-m gpu): `EngineSGD` (training/optim/engine_sgd.py) step by step against the fp64 SGD of tests/sgd_ref.py, its state-dict
interchange with torch.optim.SGD, its fused update-and-pack on a model's training plan, the GradScaler protocol of both engine
optimizers, and the trainer's `engine_optimizer: true` wiring for SGD and for amp_dtype fp16."""
import copy
import os

import pytest
import torch

import adamw_ref
import sgd_ref
from sgd_ref import next_grad

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "tasks", "synthetic_sheet.yaml")
SHAPES = [(40, 24, 3, 3, 3), (5,), (16, 8, 1, 1, 1)]
HYPER = (1e-2, 0.9, 0.0, 0.01, True)                      # (lr, momentum, dampening, weight_decay, nesterov): what the trainer builds
KW = dict(lr=HYPER[0], momentum=HYPER[1], dampening=HYPER[2], weight_decay=HYPER[3], nesterov=HYPER[4])
ADAM = adamw_ref.HYPERS[0]
ADAM_KW = dict(lr=ADAM[0], betas=ADAM[1:3], eps=ADAM[3], weight_decay=ADAM[4])


@pytest.fixture(scope="module")
def opt_mod():
    import mt3d_amd  # noqa: F401
    from mt3d_amd.engine import lib
    from mt3d_amd.training import optim
    lib.require_device()
    return optim


def _params(seed, shapes=SHAPES):
    torch.manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, device="cuda")) for s in shapes]


def _set_grads(ps, seed, k, scale=1.0):
    for j, p in enumerate(ps):
        p.grad = (next_grad(p.numel(), seed + j, k).view(p.shape) * scale).cuda()


def _bits(t):
    return t.detach().contiguous().view(torch.int32).clone()


def _sgd_snap(opt, ps):
    return [(p.detach().flatten().cpu(), opt.state[p]["momentum_buffer"].flatten().cpu() if opt.state.get(p) else None) for p in ps]


def _sgd_check(opt, ps, before, clip, what, hyper=HYPER):
    torch.cuda.synchronize()
    for j, p in enumerate(ps):
        first = before[j][1] is None
        sgd_ref.check_step((p.detach().flatten(), opt.state[p]["momentum_buffer"].flatten()), before[j], p.grad.flatten().cpu(), clip,
                           sgd_ref.sgd_args(*hyper, first), f"{what}: parameter {j}")


def _adam_snap(opt, ps):
    return [(p.detach().flatten().cpu(), opt.state[p]["exp_avg"].flatten().cpu(), opt.state[p]["exp_avg_sq"].flatten().cpu()) if opt.state.get(p)
            else (p.detach().flatten().cpu(), torch.zeros(p.numel()), torch.zeros(p.numel())) for p in ps]


def _capture_scalar(opt):
    """records the device scalar the optimizer hands to its kernels (read back on the host after the step)"""
    seen = []
    inner = opt._flat_update

    def spy(group, items, clip):
        seen.append(clip)
        return inner(group, items, clip)
    opt._flat_update = spy
    return seen


# ---- per-step check -------------------------------------------------------------------------------------------------------------
def test_engine_sgd_five_steps_with_clipping(opt_mod):
    """five steps with clip_grad_norm(3), each inside the bound from a snapshot taken before it; the returned norm is
    torch.nn.utils.clip_grad_norm_'s on a clone"""
    ps = _params(21)
    opt = opt_mod.EngineSGD(ps, model=None, **KW)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=5)
    for k in range(5):
        _set_grads(ps, 1200, k, scale=10.0 if k % 2 == 0 else 0.001)         # alternately clipped and not
        clones = [torch.nn.Parameter(p.detach().clone()) for p in ps]
        for c, p in zip(clones, ps):
            c.grad = p.grad.clone()
        want = torch.nn.utils.clip_grad_norm_(clones, 3).item()
        before = _sgd_snap(opt, ps)
        gbits = [_bits(p.grad) for p in ps]
        total = opt.clip_grad_norm(3)
        clip = opt._clip.item()
        assert abs(total.item() - want) <= 1e-6 * want
        assert (clip < 1.0) == (k % 2 == 0)
        lr = opt.param_groups[0]["lr"]
        opt.step()
        _sgd_check(opt, ps, before, clip, f"engine_sgd: step {k}", hyper=(lr,) + HYPER[1:])
        assert all(torch.equal(_bits(p.grad), b) for p, b in zip(ps, gbits)), "grad written"
        assert opt._clip is None
        sched.step()
    sd = opt.state_dict()
    assert set(sd["state"][0]) == {"momentum_buffer"}
    # every key torch.optim.SGD writes (`initial_lr` is the scheduler's)
    assert set(sd["param_groups"][0]) - {"initial_lr"} == set(torch.optim.SGD(_params(0), lr=0.1).state_dict()["param_groups"][0])


def test_engine_sgd_constructor_and_parameter_checks(opt_mod):
    from mt3d_amd.engine.lib import RxError
    ps = _params(22)
    for kw, msg in ((dict(lr=-1.0), "Invalid learning rate"), (dict(momentum=-0.1), "Invalid momentum value"),
                    (dict(weight_decay=-0.1), "Invalid weight_decay value"), (dict(nesterov=True), "Nesterov momentum requires"),
                    (dict(nesterov=True, momentum=0.9, dampening=0.1), "Nesterov momentum requires")):
        with pytest.raises(ValueError, match=msg):
            opt_mod.EngineSGD(ps, **kw)
    opt = opt_mod.EngineSGD(ps, **KW)
    _set_grads(ps, 1250, 0)
    opt.param_groups[0]["maximize"] = True
    with pytest.raises(ValueError, match="maximize"):
        opt.step()
    assert not opt.state.get(ps[0])
    for bad in (torch.nn.Parameter(torch.randn(8)), torch.nn.Parameter(torch.randn(8, device="cuda", dtype=torch.float64)),
                torch.nn.Parameter(torch.randn(8, 6, device="cuda").t())):
        bad.grad = torch.zeros_like(bad)
        with pytest.raises(RxError):
            opt_mod.EngineSGD([bad], **KW).step()


# ---- state-dict interchange ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["engine", "torch"])
def test_engine_sgd_state_dict_interchanges_with_torch_sgd(opt_mod, source):
    """two steps of one class, state_dict() into the other, whose next step stays inside the bound of the fp64 continuation of the
    state it was given"""
    pa = _params(23)
    mk = {"engine": lambda ps: opt_mod.EngineSGD(ps, model=None, **KW), "torch": lambda ps: torch.optim.SGD(ps, **KW)}
    other = "torch" if source == "engine" else "engine"
    oa = mk[source](pa)
    for k in range(2):
        _set_grads(pa, 1300, k)
        oa.step()
    sd = copy.deepcopy(oa.state_dict())
    pb = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    ob = mk[other](pb)
    ob.load_state_dict(sd)
    for a, b in zip(pa, pb):
        assert torch.equal(_bits(oa.state[a]["momentum_buffer"]), _bits(ob.state[b]["momentum_buffer"]))
    _set_grads(pb, 1300, 2)
    before = _sgd_snap(ob, pb)
    assert all(b[1] is not None for b in before)
    ob.step()
    _sgd_check(ob, pb, before, None, f"engine_sgd: {other} continues {source}")


# ---- with a model: fused update-and-pack ------------------------------------------------------------------------------------------
def test_engine_sgd_rewrites_the_plans_packs(opt_mod):
    """a golden-case network at 16^3 with model= given: after step() every pack entry is fresh and the next forward equals, bit for
    bit, that of a twin whose packs are rebuilt from the fp32 weights; every parameter inside the bound of the fp64 step"""
    from test_optim_gpu import _setup, _train
    net, c, mgr, x, targets, N = _setup()
    ps = [p for p in net.parameters()]
    opt = opt_mod.EngineSGD(ps, model=net, **KW)
    clips = []

    def clip(o):
        o.clip_grad_norm(0.05)
        clips.append(o._clip.item())
        clip.before = [(p.detach().flatten().cpu(), None) for p in ps]
        clip.grads = [None if p.grad is None else p.grad.flatten().cpu() for p in ps]
    _train(net, c, x, targets, opt, 1, clip)
    torch.cuda.synchronize()
    plan = [p for p in net._plans.values() if p.needs_grad][0]
    assert opt._plan() is plan and not plan._packs_stale() and all(e.event is None for e in plan.packs)
    assert clips[0] < 1.0
    args = sgd_ref.sgd_args(*HYPER, True)
    for (name, p), before, g in zip(net.named_parameters(), clip.before, clip.grads):
        if g is None:
            assert torch.equal(p.detach().flatten().cpu(), before[0]) and not opt.state.get(p), name
            continue
        sgd_ref.check_step((p.detach().flatten(), opt.state[p]["momentum_buffer"].flatten()), before, g, clips[0], args, f"engine_sgd plan: {name}")
    twin = N(mgr).cuda()
    twin.load_state_dict(net.state_dict())

    def fwd(m):
        m.train()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            return m(x)
    o1, o2 = fwd(net), fwd(twin)
    for k in o1:
        assert torch.equal(o1[k], o2[k]), k


# ---- GradScaler -------------------------------------------------------------------------------------------------------------------
def _scaler():
    s = torch.amp.GradScaler("cuda", init_scale=1024.)
    s.scale(torch.ones((), device="cuda"))                # (the scale tensor is created by the first scale() call)
    return s


def _make(opt_mod, which, ps):
    return opt_mod.EngineSGD(ps, model=None, **KW) if which == "sgd" else opt_mod.EngineAdamW(ps, model=None, **ADAM_KW)


def _state_bits(opt, ps):
    return [{k: (_bits(v) if torch.is_tensor(v) else v) for k, v in opt.state[p].items()} if opt.state.get(p) else None for p in ps]


def _same_state(a, b):
    if (a is None) != (b is None) or (a is not None and set(a) != set(b)):
        return False
    return a is None or all(torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k] for k in a)


@pytest.mark.parametrize("which", ["sgd", "adamw"])
def test_scaler_finite_step_matches_the_reference(opt_mod, which):
    """two steps under GradScaler(init_scale=1024) on gradients scaled by 1024: each equals the per-element reference with the
    combined scalar clip * (1 / 1024) read back from the device; the scale stays"""
    ps = _params(24)
    opt = _make(opt_mod, which, ps)
    seen = _capture_scalar(opt)
    scaler = _scaler()
    for k in range(2):
        _set_grads(ps, 1400, k, scale=1024.0 * (10.0 if k == 0 else 0.01))
        before = _sgd_snap(opt, ps) if which == "sgd" else _adam_snap(opt, ps)
        total = opt_mod.clip_and_step(opt, ps, 3, scaler)
        scaler.update()
        torch.cuda.synchronize()
        comb = seen[-1].item()
        want = min(1.0, 3.0 / (total.item() + 1e-6)) / 1024.0
        assert abs(comb - want) <= 4 * 2.0 ** -24 * want, (comb, want)          # norm taken on the scaled gradients, then 1 / scale
        assert not hasattr(opt, "grad_scale") and not hasattr(opt, "found_inf") and opt._clip is None
        if which == "sgd":
            _sgd_check(opt, ps, before, comb, f"engine_sgd scaler: step {k}")
        else:
            for j, p in enumerate(ps):
                st = opt.state[p]
                assert st["step"] == k + 1
                adamw_ref.check_step((p.detach().flatten(), st["exp_avg"].flatten(), st["exp_avg_sq"].flatten()), before[j],
                                     p.grad.flatten().cpu(), comb, adamw_ref.adam_args(*ADAM, k + 1), f"engine_adamw scaler: step {k} parameter {j}")
        assert scaler.get_scale() == 1024.0
    # without clip_grad_norm the scalar is 1 / grad_scale alone
    _set_grads(ps, 1400, 2, scale=1024.0)
    scaler.step(opt)
    scaler.update()
    assert seen[-1].item() == 1.0 / 1024.0


@pytest.mark.parametrize("which", ["sgd", "adamw"])
@pytest.mark.parametrize("fresh", [True, False], ids=["no_state_yet", "after_a_step"])
def test_scaler_inf_step_is_skipped(opt_mod, which, fresh):
    """one gradient element inf: p, every state tensor and state[p] bitwise unchanged (no state created on a fresh optimizer), the
    clip scalar dropped, and the scale halved by update()"""
    ps = _params(25)
    opt = _make(opt_mod, which, ps)
    scaler = _scaler()
    if not fresh:
        _set_grads(ps, 1500, 0, scale=1024.0)
        opt_mod.clip_and_step(opt, ps, 3, scaler)
        scaler.update()
    _set_grads(ps, 1500, 1, scale=1024.0)
    ps[0].grad.view(-1)[7] = float("inf")
    pbits, sbits = [_bits(p) for p in ps], _state_bits(opt, ps)
    opt_mod.clip_and_step(opt, ps, 3, scaler)
    scaler.update()
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(p), b) for p, b in zip(ps, pbits))
    assert all(_same_state(a, b) for a, b in zip(_state_bits(opt, ps), sbits))
    if fresh:
        assert all(not opt.state.get(p) for p in ps)
    assert opt._clip is None and not hasattr(opt, "found_inf")
    assert scaler.get_scale() == 512.0


@pytest.mark.parametrize("which", ["sgd", "adamw"])
def test_disabled_scaler_is_the_no_scaler_call(opt_mod, which):
    pa = _params(26)
    pb = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    oa, ob = _make(opt_mod, which, pa), _make(opt_mod, which, pb)
    off = torch.amp.GradScaler("cuda", enabled=False)
    for k in range(2):
        _set_grads(pa, 1600, k, scale=10.0)
        _set_grads(pb, 1600, k, scale=10.0)
        na, nb = opt_mod.clip_and_step(oa, pa, 3, off), opt_mod.clip_and_step(ob, pb, 3, None)
        assert na.item() == nb.item()
    for a, b in zip(pa, pb):
        assert torch.equal(_bits(a), _bits(b))
        assert _same_state(_state_bits(oa, [a])[0], _state_bits(ob, [b])[0])


# ---- trainer ----------------------------------------------------------------------------------------------------------------------
def _trainer_cfg(tmp_path, name, **tr_config):
    import yaml
    cfg = yaml.safe_load(open(CFG))
    cfg["tr_setup"].update(model_name=name, ckpt_out_base=str(tmp_path / f"ckpt_{name}"), tensorboard_log_dir=str(tmp_path / f"tb_{name}"))
    cfg["tr_config"].update(max_epoch=1, max_steps_per_epoch=2, max_val_steps_per_epoch=1, **tr_config)
    p = tmp_path / f"{name}.yaml"
    yaml.safe_dump(cfg, open(p, "w"))
    return cfg, p


@pytest.mark.parametrize("name,tr_config,cls", [("sgd", dict(optimizer="SGD", engine_optimizer=True), "EngineSGD"),
                                                ("adamw_fp16", dict(amp_dtype="fp16", engine_optimizer=True), "EngineAdamW"),
                                                ("sgd_fp16", dict(optimizer="SGD", amp_dtype="fp16", engine_optimizer=True), "EngineSGD")])
def test_trainer_runs_the_engine_optimizers(opt_mod, tmp_path, name, tr_config, cls):
    """BaseTrainer on the synthetic dataset at 32^3, two steps: the optimizer's class, finite losses, changed parameters, and a
    checkpoint that torch.load()s and that a second trainer resumes from"""
    import yaml
    from mt3d_amd.train import BaseTrainer
    cfg, p = _trainer_cfg(tmp_path, name, **tr_config)
    os.chdir(tmp_path)

    class Rec(BaseTrainer):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.losses, self.opt, self.initial = [], None, None

        def _log(self, *a):
            s = " ".join(str(x) for x in a)
            if s.startswith("[Train]"):
                self.losses.append(float(s.split("sheet: ")[1].split(" ")[0]))

        def _get_optimizer(self, model):
            self.opt = super()._get_optimizer(model)
            self.initial = {k: v.detach().clone() for k, v in model.state_dict().items()}
            return self.opt

    tr = Rec(str(p), verbose=False)
    model = tr.train()
    assert type(tr.opt) is getattr(opt_mod, cls)
    assert len(tr.losses) == 1 and all(x == x and abs(x) != float("inf") for x in tr.losses)
    sd = BaseTrainer._strip_compile_prefix(model.state_dict())
    changed = [k for k, v in sd.items() if v.dtype.is_floating_point and not torch.equal(v.cpu(), tr.initial[k].cpu())]
    assert "shared_encoder.stages.0.blocks.0.conv1.conv.weight" in changed, changed[:5]
    assert all(torch.isfinite(v).all().item() for v in sd.values() if v.dtype.is_floating_point)
    path = tmp_path / f"ckpt_{name}" / f"{name}_1.pth"
    ck = torch.load(path, weights_only=True)
    assert set(ck) == {"model", "optimizer", "scheduler", "epoch"}
    key = "momentum_buffer" if cls == "EngineSGD" else "exp_avg"
    assert ck["optimizer"]["state"] and all(key in s for s in ck["optimizer"]["state"].values())
    cfg["tr_setup"]["checkpoint_path"] = str(path)
    yaml.safe_dump(cfg, open(p, "w"))
    tr2 = Rec(str(p), verbose=False)
    m2 = tr2.train()                                          # start_epoch == max_epoch: the state loads, no step
    assert type(tr2.opt) is type(tr.opt)
    for (k, a), (_, b) in zip(model.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a.cpu(), b.cpu()), k
    s1, s2 = tr.opt.state_dict()["state"], tr2.opt.state_dict()["state"]
    assert set(s1) == set(s2) and all(torch.equal(s1[i][key].cpu(), s2[i][key].cpu()) for i in s1)


def test_trainer_without_the_flag_builds_torchs_optimizers(opt_mod, tmp_path):
    from mt3d_amd.train import BaseTrainer
    for name, tr_config, cls in (("plain_sgd", dict(optimizer="SGD"), torch.optim.SGD), ("plain_adamw", dict(), torch.optim.AdamW),
                                 ("plain_fp16", dict(amp_dtype="fp16"), torch.optim.AdamW),
                                 ("off_sgd", dict(optimizer="SGD", engine_optimizer=False), torch.optim.SGD)):
        _, p = _trainer_cfg(tmp_path, name, **tr_config)
        tr = BaseTrainer(str(p), verbose=False)
        assert type(tr._get_optimizer(tr._build_model())) is cls, name
