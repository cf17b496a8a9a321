"""The end of a training step (clip_grad_norm(3) + optimizer update [+ weight re-pack]) on the cfg2 parameter set, per optimizer path:
device time between two events around the tail (median and range over the repeats, cases interleaved) and, from one profiled tail,
the number of kernel launches and their summed kernel time.  The torch rows are what the trainer runs without `engine_optimizer`.
   usage: python scripts/bench_optim.py [--repeats N] [--warmup N] [--out FILE.json]"""
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import torch
import bench
import mt3d_amd  # noqa: F401
from mt3d_amd.builders.build_network_from_config import NetworkFromConfig
from mt3d_amd.engine import lib
from mt3d_amd.training.optim import EngineAdamW, EngineSGD, clip_and_step


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


repeats, warmup = arg("--repeats", 20), arg("--warmup", 3)
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
lib.require_device()
dev = torch.device("cuda", 0)
w = dict(bench.WORKLOADS["cfg2"], batch=1)
torch.manual_seed(0)
net = NetworkFromConfig(bench.make_mgr(w)).to(dev)
net.train()
x, targets = bench.synthetic_batch(w, 1, 1234, dev)
with torch.autocast("cuda", dtype=torch.bfloat16):          # one real step: builds the training plan (its packs) and real gradients
    out = net(x)
    loss = sum(torch.nn.functional.binary_cross_entropy_with_logits(out[k].float(), targets[k]) for k in targets)
loss.backward()
params = [p for p in net.parameters() if p.grad is not None]
plan = [p for p in net._plans.values() if p.needs_grad][0]
n_par = sum(p.numel() for p in params)
print(f"cfg2: {len(params)} parameters with gradients, {n_par / 1e6:.1f} M elements, {len(plan.packs)} packed weights", flush=True)


def repack():
    """every packed weight of the plan from its fp32 parameter (rx_pack_multi: 40 tensors per launch), on the current stream"""
    ents = [e for e in plan.packs if e.param[0, 0].numel() <= 27]
    n = len(ents)
    VP, IP = ctypes.c_void_p * n, ctypes.c_int * n
    lib.check(lib.load().rx_pack_multi(lib.DTYPE_CODE[plan.dtype], n, VP(*[e.param.data_ptr() for e in ents]),
                                       IP(*[0 if e.kind == "conv" else 1 for e in ents]), IP(*[e.param.shape[0] for e in ents]),
                                       IP(*[e.param.shape[1] for e in ents]), IP(*[e.param[0, 0].numel() for e in ents]),
                                       VP(*[e.w_fwd.data_ptr() if e.w_fwd is not None else 0 for e in ents]),
                                       VP(*[e.w_bwd.data_ptr() if e.w_bwd is not None else 0 for e in ents]), lib.stream_ptr()),
              "rx_pack_multi")


LR = 1e-6                                                    # the tails run hundreds of times on the same gradients
SGD_KW = dict(lr=LR, momentum=0.9, nesterov=True, weight_decay=0.0)
t_sgd = torch.optim.SGD(params, **SGD_KW)
e_sgd, e_sgd_pack = EngineSGD(params, model=None, **SGD_KW), EngineSGD(params, model=net, **SGD_KW)
t_adam = torch.optim.AdamW(params, lr=LR, weight_decay=0.0)
e_adam, e_adam_pack = EngineAdamW(params, model=None, lr=LR, weight_decay=0.0), EngineAdamW(params, model=net, lr=LR, weight_decay=0.0)
scalers = {k: torch.amp.GradScaler("cuda", init_scale=1024.) for k in ("t", "e", "p")}
for s in scalers.values():
    s.scale(torch.ones((), device=dev))


def scaled(opt, key):
    def run():
        clip_and_step(opt, params, 3, scalers[key])
        scalers[key].update()
    return run


def torch_sgd():
    torch.nn.utils.clip_grad_norm_(params, 3)                # scales the gradients in place: coefficient 1 from the second run on
    t_sgd.step()


CASES = [
    ("torch SGD + clip_grad_norm_", torch_sgd),
    ("EngineSGD flat", lambda: clip_and_step(e_sgd, params, 3)),
    ("EngineSGD with packs", lambda: clip_and_step(e_sgd_pack, params, 3)),
    ("weight re-pack alone (rx_pack_multi)", repack),
    ("torch AdamW + clip_grad_norm_ under GradScaler", scaled(t_adam, "t")),
    ("EngineAdamW flat under GradScaler", scaled(e_adam, "e")),
    ("EngineAdamW with packs under GradScaler", scaled(e_adam_pack, "p")),
]


def profile(fn):
    """(launches, summed kernel time in us) of one tail, or (None, None) where the profiler gives no device events"""
    try:
        from torch.profiler import ProfilerActivity, profile as prof
        with prof(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as p:
            fn()
            torch.cuda.synchronize()
        ks = [e for e in p.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]
        return (len(ks), sum(e.device_time for e in ks)) if ks else (None, None)
    except Exception as exc:                                 # noqa: BLE001
        print(f"profiler unavailable: {exc}", flush=True)
        return None, None


times = {name: [] for name, _ in CASES}
for name, fn in CASES:
    for _ in range(warmup):
        fn()
torch.cuda.synchronize()
for _ in range(repeats):                                     # interleaved: every case sees the same drift of the clocks
    for name, fn in CASES:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times[name].append(e0.elapsed_time(e1) * 1e3)
rows = []
for name, fn in CASES:
    launches, kernel_us = profile(fn)
    t = sorted(times[name])
    row = dict(case=name, median_us=statistics.median(t), min_us=t[0], max_us=t[-1], repeats=repeats, launches=launches, kernel_us=kernel_us)
    rows.append(row)
    k = "not measured" if launches is None else f"{launches:4d} launches {kernel_us:8.1f} us kernel time"
    print(f"{name:48s} {row['median_us']:8.1f} us  [{t[0]:8.1f} .. {t[-1]:8.1f}]  {k}", flush=True)
if out_path:
    with open(out_path, "w") as f:
        json.dump(dict(parameters=len(params), elements=n_par, packed=len(plan.packs), rows=rows), f, indent=1)
