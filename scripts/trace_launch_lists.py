"""Launch lists of the engine plan, traced on the CPU: every public function of `engine.ops` is replaced by a logger, a plan is
built on the meta device, and every step of `plan.fwd` and `plan.bwd` is called.  Prints one canonical trace per configuration
(every fuzz draw, the golden cases, the cfg2 bench workload; both compute types, training and inference plans, both `apply_act`
settings, one task absent from the loss, training / eval setting of DropPath and channel dropout).

A refactor of engine/plan.py must leave the output byte-identical: run this same file against both trees and diff,
    python scripts/trace_launch_lists.py --root <checkout of the parent> > a.txt
    python scripts/trace_launch_lists.py > b.txt
(`--digest`: one sha256 per configuration instead of the full trace).  It uses only names a plan keeps:
fwd / bwd / outputs / params / packs / grad_order / _drops / _gates / _x / _apply_act / _dlogits / _grads.

`--run` traces the RUN side instead: `run_forward` / `run_backward` are driven for whole steps, weight packing included
(`pack_weights_multi` is logged with its items).  On the meta device (default; single stream) over every configuration:
a training plan's step 1, step 2 behind a fused optimizer step (every pack marked fresh: nothing is packed), step 3 behind a
plain backward (new weight epoch: everything is packed), step 4 with one parameter's version bumped (that entry alone), and
an inference plan's two forwards, encoder and decoders.  `--run --device cuda` (needs the GPU) runs `--steps` SGD training
steps of the golden case `--only` (default auto16_2head) on the real `ops`, each wrapped by the logger: the host-call order
on two streams, event slots numbered by first appearance.  `--pack-limit BYTES` lowers `plan.packs.limit` there."""
import argparse
import hashlib
import os
import sys
import types

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--digest", action="store_true")
ap.add_argument("--only", default=None, help="substring of the configuration names to run")
ap.add_argument("--run", action="store_true", help="trace run_forward / run_backward instead of the launch lists")
ap.add_argument("--device", default="meta", choices=("meta", "cuda"), help="--run only: cuda = the real ops, logged")
ap.add_argument("--steps", type=int, default=3, help="--run --device cuda: training steps")
ap.add_argument("--pack-limit", type=int, default=None, help="--run --device cuda: plan.packs.limit")
args = ap.parse_args()
ROOT = os.path.abspath(args.root)
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import bench  # noqa: E402
import mt3d_amd  # noqa: E402,F401
import resenc_oracle as oracle  # noqa: E402
import test_fuzz_gpu as fz  # noqa: E402
from golden_cases import CASES  # noqa: E402
from mt3d_amd.builders.build_network_from_config import NetworkFromConfig  # noqa: E402
from mt3d_amd.engine import ops  # noqa: E402
from mt3d_amd.engine.plan import Plan, UnsupportedConfig  # noqa: E402

LOG = []
_ids, _alive = {}, []


def _ordinal(obj):
    if id(obj) not in _ids:
        _ids[id(obj)] = len(_ids)
        _alive.append(obj)          # ids stay unique while the trace runs
    return _ids[id(obj)]


def canon(v):
    if isinstance(v, ops.Act):
        return (f"Act(#{_ordinal(v.root if v.root is not None else v.t)} c0={v.c0} c={v.c} plane={v.plane} "
                f"{tuple(v.t.shape)})")
    if isinstance(v, torch.Tensor):
        return f"T(#{_ordinal(v._base if v._base is not None else v)} {tuple(v.shape)} {v.dtype})"
    if isinstance(v, dict):
        return "{" + ", ".join(f"{k}: {canon(v[k])}" for k in sorted(v)) + "}"
    if isinstance(v, (list, tuple)):
        return "[" + ", ".join(canon(e) for e in v) + "]"
    if REAL and isinstance(v, torch.cuda.Stream):
        return "main" if v == torch.cuda.default_stream() else "side"
    if callable(v):
        return "<fn>"
    return repr(v)


RETURNS = {"workspace": lambda: torch.empty(1, dtype=torch.uint8, device="meta"), "event_new": lambda: 7,
           "conv3d_bwd_data_instats": lambda: True}
REAL = args.run and args.device == "cuda"       # the real ops run; the logger only listens
EVENT_OPS = ("event_record", "stream_wait", "event_free")
_slots = {}


def _slot(s):
    """numbered events of the library, renumbered by first appearance"""
    return f"ev{_slots.setdefault(s, len(_slots))}"


def _logger(name, real=None):
    def call(*a, **k):
        if name != "workspace":
            shown = [_slot(a[0])] + [canon(e) for e in a[1:]] if REAL and name in EVENT_OPS else [canon(e) for e in a]
            on = f" @{canon(torch.cuda.current_stream())}" if REAL else ""
            LOG.append(name + "(" + ", ".join(shown + [f"{n}={canon(k[n])}" for n in sorted(k)]) + ")" + on)
        if real is not None:
            out = real(*a, **k)
            if name == "event_new":
                LOG[-1] += f" -> {_slot(out)}"
            return out
        return RETURNS[name]() if name in RETURNS else None
    return call


for _n, _f in list(vars(ops).items()):
    if isinstance(_f, types.FunctionType) and not _n.startswith("_"):
        setattr(ops, _n, _logger(_n, _f if REAL else None))


def _get(o, k):
    return o[k] if isinstance(o, dict) else getattr(o, k)


def _set(o, k, v):
    if isinstance(o, dict):
        o[k] = v
    else:
        setattr(o, k, v)


def set_mode(plan, training):
    """the per-step fields of DropPath / channel dropout, as Plan._forward_pre leaves them"""
    for g in plan._gates:
        sc = _get(g, "scale")
        _set(g, "scale_now", sc if (sc is not None and training) else None)
    for d in plan._drops:
        _set(d, "active", training)
        _set(d, "eps_now", _get(d, "eps") * (1.0 - _get(d, "p")) ** 2 if training else _get(d, "eps"))


def emit(title, lines):
    if args.digest:
        print(f"{title}: {len(lines)} lines {hashlib.sha256(chr(10).join(lines).encode()).hexdigest()}")
    else:
        print(f"== {title}")
        for ln in lines:
            print("  " + ln)


def trace(name, mgr, shape):
    for dtype in (torch.float32, torch.bfloat16):
        for needs_grad in (True, False):
            title = f"{name} {str(dtype)[6:]} grad={int(needs_grad)}"
            net = NetworkFromConfig(mgr).to("meta")
            try:
                plan = Plan(net, shape, dtype, "meta", needs_grad=needs_grad)
            except UnsupportedConfig as e:
                emit(title, [f"UnsupportedConfig: {e}"])
                continue
            _ids.clear()
            _alive.clear()
            emit(title + " plan", [f"grad_order={plan.grad_order}", f"bytes_alloc={plan.bytes_alloc}", f"packs={len(plan.packs)}",
                                   f"pack_delay_at={plan._pack_delay_at}", f"n_fwd_enc={plan.n_fwd_enc}",
                                   f"fwd_dec_start={plan.fwd_dec_start}", f"fwd={len(plan.fwd)} bwd={len(plan.bwd)}"])
            x = torch.empty(shape, dtype=torch.float32, device="meta")
            plan._x = x.unsqueeze(2) if plan.two_d else x
            modes = (True, False) if (plan._gates or plan._drops) else (False,)
            tasks = list(plan.outputs)
            for training in modes:
                set_mode(plan, training)
                for apply_act in (False, True):
                    plan._apply_act = apply_act
                    del LOG[:]
                    for step in plan.fwd:
                        step()
                    emit(f"{title} fwd train={int(training)} act={int(apply_act)}", list(LOG))
                for absent in ((None, tasks[0]) if needs_grad else ()):
                    plan._dlogits = {k: torch.empty(tuple(v.shape), dtype=torch.float32, device="meta")
                                     for k, v in plan.outputs.items() if k != absent}
                    plan._grads = [None] * len(plan.params)
                    del LOG[:]
                    for step in plan.bwd:
                        step()
                    emit(f"{title} bwd train={int(training)} absent={absent}", list(LOG))
            plan.release()


def trace_run(name, mgr, shape):
    """whole steps through run_forward / run_backward on the meta device (see the module docstring)"""
    for dtype in (torch.float32, torch.bfloat16):
        title = f"{name} {str(dtype)[6:]} run"
        net = NetworkFromConfig(mgr).to("meta")
        try:
            plan = Plan(net, shape, dtype, "meta", needs_grad=True)
            infer = Plan(net, shape, dtype, "meta", needs_grad=False)
        except UnsupportedConfig as e:
            emit(title, [f"UnsupportedConfig: {e}"])
            continue
        _ids.clear()
        _alive.clear()
        x = torch.empty(shape, dtype=torch.float32, device="meta")

        def step(label):
            del LOG[:]
            outs = plan.run_forward(x, apply_act=False)
            emit(f"{title} {label} forward", LOG + [f"outputs={canon(outs)}"])
            del LOG[:]
            grads = plan.run_backward({k: torch.empty(tuple(v.shape), dtype=torch.float32, device="meta") for k, v in outs.items()})
            emit(f"{title} {label} backward", LOG + [f"grads={canon(grads)}", f"stale={len(plan._packs_stale())}"])

        net.train()
        step("step 1")
        plan._mark_packs_fresh()            # what a fused engine optimizer step leaves behind
        step("step 2 (packs fresh)")
        step("step 3 (new weight epoch)")
        plan._mark_packs_fresh()
        packs = list(plan.packs)
        with torch.no_grad():
            _get(packs[len(packs) // 2], "param").zero_()
        step("step 4 (one version bumped)")
        net.eval()
        for label in ("forward 1", "forward 2"):
            del LOG[:]
            outs = infer.run_forward(x, apply_act=True)
            emit(f"{title} inference {label}", LOG + [f"outputs={canon(outs)}"])
        del LOG[:]
        skips = infer.run_encoder(x)
        emit(f"{title} inference encoder", LOG + [f"skips={canon(skips)}"])
        for d, task in enumerate(infer.outputs):
            del LOG[:]
            out = infer.run_decoder(d, task, skips)
            emit(f"{title} inference decoder {task}", LOG + [f"out={canon(out)}"])
        plan.release()
        infer.release()


def trace_cuda():
    """the host-call order of `--steps` SGD training steps on the GPU, two streams (see the module docstring)"""
    case = args.only or "auto16_2head"
    c = CASES[case]
    mgr = oracle.make_mgr(c["patch"], c["tasks"], c["in_channels"], c["batch"], c["autoconfigure"], c["model_config"])
    torch.manual_seed(c["seed"])
    net = NetworkFromConfig(mgr).cuda()
    net.compute_dtype = torch.bfloat16
    net.train()
    opt = torch.optim.SGD(list(net.parameters()), lr=0.05)
    shape = (c["batch"], c["in_channels"], *c["patch"])
    plan = net.plan_for(shape, torch.bfloat16, torch.device("cuda", torch.cuda.current_device()), True)
    if args.pack_limit is not None:
        plan.packs.limit = args.pack_limit
    print(f"== {case} bf16 programs={int(plan.use_programs)} pack_limit={args.pack_limit}")
    for step in range(args.steps):
        x, targets = oracle.synthetic_batch(c["batch"], c["in_channels"], c["patch"], c["tasks"], 100 + step)
        x, targets = x.cuda(), {k: v.cuda() for k, v in targets.items()}
        del LOG[:]
        out = net(x)
        emit(f"step {step + 1} forward", list(LOG))
        loss = oracle.train_loss(out, targets, c["tasks"])
        del LOG[:]
        loss.backward()
        emit(f"step {step + 1} backward", LOG + [f"loss={loss.item()!r}"])
        opt.step()
        opt.zero_grad(set_to_none=True)
    assert list(net._plans.values()) == [plan]
    torch.cuda.synchronize()


def main():
    if REAL:
        trace_cuda()
        return
    jobs = []
    for kind, gen in (("small", fz.configs), ("medium", fz.medium_configs), ("large", fz.large_configs)):
        for i, c in enumerate(gen()):
            jobs.append((f"fuzz-{kind}{i}", oracle.make_mgr(c["patch"], c["tasks"], c["cin"], c["batch"], False, c["mc"]),
                         (c["batch"], c["cin"], *c["patch"])))
    for case, c in CASES.items():
        jobs.append((f"golden-{case}", oracle.make_mgr(c["patch"], c["tasks"], c["in_channels"], c["batch"], c["autoconfigure"],
                                                       c["model_config"]), (c["batch"], c["in_channels"], *c["patch"])))
    w = bench.WORKLOADS["cfg2"]
    jobs.append(("bench-cfg2", bench.make_mgr(w), (w["batch"], w["in_channels"], *w["patch"])))
    n = 0
    for name, mgr, shape in jobs:
        if args.only is None or args.only in name:
            (trace_run if args.run else trace)(name, mgr, shape)
            n += 1
    print(f"{n} configurations traced", file=sys.stderr)


main()
