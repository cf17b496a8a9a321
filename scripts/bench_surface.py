"""Surface-distance kernels: time per call of `ops.edt_sq` and of a full `ops.surface_hist` on a synthetic sheet, against
a plain device copy of the same bytes (the floor), the numpy statement and scipy's distance transform on the host, and what the
`surface` block adds to one validation step next to that step's eval forward.  Prints ONE JSON line.

    python scripts/bench_surface.py [--sizes 64 128 192] [--batch 2] [--rounds 9] [--no-model]

Per size: a `--batch` x 1 x size^3 target sheet, two voxels thick and gently bent, and a prediction that is the same sheet one
voxel off with 0.1 % of the voxels flipped.  Every result is compared with its numpy statement first (size 64 only: the statement
takes seconds per volume beyond that).  Timing: HIP events around regions of one call on each of SETS distinct batches, the arms
ALTERNATED round by round after two warm-up rounds, median [min, max] over the rounds, microseconds per CALL through `engine.ops`
(wrapper included).  The copy arms move the call's algorithmic bytes with `Tensor.copy_` (half of them read, half written).
Host references are timed once, on ONE volume, with a wall clock.
The validation step: `ValidationMetrics.update` on cfg2's batch (2 x 1 x 128^3, one binary task) with and without the `surface`
block, and the eval-mode forward of bench.py's cfg2 network (bf16) on the same batch, all in this process."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SETS = 4


def sheet_pair(size, batch, seed):
    """(prediction logits, target) float32 (batch, 1, size, size, size): a bent two-voxel sheet and a shifted, speckled copy"""
    r = np.random.default_rng(seed)
    zz, yy, xx = np.meshgrid(*(np.arange(size, dtype=np.float32),) * 3, indexing="ij")
    pred, targ = [], []
    for n in range(batch):
        mid = size / 2 + (size / 16) * np.sin(xx * (6.0 / size) + n + seed) * np.cos(yy * (5.0 / size))
        t = (zz >= mid) & (zz < mid + 2)
        p = ((zz >= mid + 1) & (zz < mid + 3)) ^ (r.random(t.shape) < 0.001)
        targ.append(t.astype(np.float32)), pred.append(p.astype(np.float32) * 4.0 - 2.0)
    return np.stack(pred)[:, None], np.stack(targ)[:, None]


def regions(fns, rounds, sets=SETS, warmup=2):
    """every fn of `fns` over all its sets once per region, the fns ALTERNATED round by round; microseconds per call, per fn"""
    import torch
    times = {k: [] for k in fns}
    for rnd in range(warmup + rounds):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(sets):
                fn(i)
            b.record()
            b.synchronize()
            if rnd >= warmup:
                times[k].append(1e3 * a.elapsed_time(b) / sets)
    return {k: {"us": round(float(np.median(v)), 1), "us_min_max": [round(min(v), 1), round(max(v), 1)]} for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 128, 192])
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--no-model", action="store_true", help="skip the validation-step block (no network is built)")
    a = ap.parse_args()
    import torch
    import mt3d_amd  # noqa: F401
    from mt3d_amd.engine import ops as E
    from mt3d_amd.training import metrics as M
    from mt3d_amd.training.metrics import surface as S
    if not torch.cuda.is_available():
        raise SystemExit("bench_surface: needs the GPU (there is no host path to time)")
    try:
        from scipy import ndimage as ndi
    except ImportError:
        ndi = None
    res = {"batch": a.batch, "sets": SETS, "rounds": a.rounds, "scipy": "present" if ndi is not None else "absent", "sizes": {}}
    for size in a.sizes:
        vox = a.batch * size ** 3
        host = [sheet_pair(size, a.batch, s) for s in range(SETS)]
        pred = [torch.from_numpy(p).cuda() for p, _ in host]
        targ = [torch.from_numpy(t).cuda() for _, t in host]
        feat = [E.mask_edges(t, 0.5) for t in targ]
        dist = torch.empty(feat[0].shape, dtype=torch.int32, device="cuda")
        bins = S.default_bins((size,) * 3)
        hist = torch.zeros((2, bins), dtype=torch.int64, device="cuda")
        counts = torch.zeros(4, dtype=torch.int64, device="cuda")
        scratch = E.surface_scratch(pred[0].shape, "cuda")
        out = {"voxels": vox, "edge_share_of_target": round(float(feat[0].float().mean()), 4)}
        if size <= 64:
            want_d = np.stack([S.edt_sq_numpy(v) for v in feat[0][:, 0].cpu().numpy()])[:, None]
            out["edt_sq_equals_statement"] = bool(np.array_equal(E.edt_sq(feat[0]).cpu().numpy(), want_d))
            wh = [S.surface_hist_numpy(host[0][0][n, 0], host[0][1][n, 0], 0.0, 0.5) for n in range(a.batch)]
            h, c = E.surface_hist(pred[0], targ[0], 0.0, 0.5)
            out["surface_hist_equals_statement"] = bool(np.array_equal(h.cpu().numpy(), sum(w[0] for w in wh))
                                                        and np.array_equal(c.cpu().numpy(), sum(w[1] for w in wh)))
        edt_bytes = vox * 5
        hist_bytes = vox * (4 + 4 + 6 + 16)      # the wrapper's accounting for a float32 prediction
        src = torch.empty(hist_bytes // 2, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        t = regions({"edt_sq": lambda i: E.edt_sq(feat[i], out=dist),
                     "copy_edt_bytes": lambda i: dst[:edt_bytes // 2].copy_(src[:edt_bytes // 2]),
                     "surface_hist": lambda i: E.surface_hist(pred[i], targ[i], 0.0, 0.5, hist=hist, counts=counts, scratch=scratch),
                     "copy_hist_bytes": lambda i: dst.copy_(src)}, a.rounds)
        out.update(t)
        out["edt_sq"]["bytes"], out["surface_hist"]["bytes"] = edt_bytes, hist_bytes
        out["edt_sq"]["GBps"] = round(edt_bytes / out["edt_sq"]["us"] / 1e3, 1)
        out["surface_hist"]["GBps"] = round(hist_bytes / out["surface_hist"]["us"] / 1e3, 1)
        out["edt_sq"]["over_copy"] = round(out["edt_sq"]["us"] / out["copy_edt_bytes"]["us"], 1)
        out["surface_hist"]["over_copy"] = round(out["surface_hist"]["us"] / out["copy_hist_bytes"]["us"], 1)
        # host references: ONE volume, once
        one = feat[0][0, 0].cpu().numpy().astype(bool)
        if size <= 128:
            t0 = time.perf_counter()
            S.edt_sq_numpy(one)
            out["numpy_statement_s_per_volume"] = round(time.perf_counter() - t0, 3)
        else:
            out["numpy_statement_s_per_volume"] = "not run"
        if ndi is not None:
            t0 = time.perf_counter()
            ndi.distance_transform_edt(~one)
            out["scipy_edt_s_per_volume"] = round(time.perf_counter() - t0, 3)
        else:
            out["scipy_edt_s_per_volume"] = "absent"
        res["sizes"][str(size)] = out
        del pred, targ, feat, dist, hist, scratch, src, dst
        torch.cuda.empty_cache()

    if not a.no_model:
        # one validation step of cfg2: what update() costs with and without the block, next to the eval forward of the same batch
        from types import SimpleNamespace
        from mt3d_amd.builders.build_network_from_config import NetworkFromConfig
        tasks = {"sheet": {"channels": 1, "activation": "none", "weight": 1, "loss_fn": "BCEDiceLoss", "loss_kwargs": {"alpha": 0.5, "beta": 0.5}}}
        size, batch = 128, 2
        host = [sheet_pair(size, batch, 10 + s) for s in range(SETS)]
        outs = [{"sheet": torch.from_numpy(p).cuda()} for p, _ in host]
        tgts = [{"sheet": torch.from_numpy(t).cuda()} for _, t in host]
        plain, surf = M.ValidationMetrics(tasks, True), M.ValidationMetrics(tasks, {"surface": True})
        torch.manual_seed(0)
        net = NetworkFromConfig(SimpleNamespace(tasks=tasks, train_patch_size=(size,) * 3, train_batch_size=batch, in_channels=1, vram_max=16.0,
                                                autoconfigure=True, model_config={}, verbose=False)).cuda()
        net.compute_dtype = torch.bfloat16
        net.eval()
        xs = [torch.rand((batch, 1) + (size,) * 3, device="cuda") for _ in range(SETS)]

        def forward(i):
            with torch.no_grad():
                return net(xs[i])
        t = regions({"update_plain": lambda i: plain.update(outs[i], tgts[i]), "update_surface": lambda i: surf.update(outs[i], tgts[i]),
                     "eval_forward": forward}, a.rounds)
        added = t["update_surface"]["us"] - t["update_plain"]["us"]
        t["added_us_per_validation_batch"] = round(added, 1)
        t["added_over_eval_forward"] = round(added / t["eval_forward"]["us"], 3)
        t["scores"] = {k: round(v, 4) for k, v in surf.compute()["sheet"].items()}
        res["validation_step_cfg2"] = t
    try:
        res["device"] = torch.cuda.get_device_name()
        res["sclk_mhz_after"] = int(torch.cuda.clock_rate())          # the clock is left to the governor; read, never set
    except Exception as e:      # (an optional reading: pynvml / amdsmi may be absent)
        res["sclk_mhz_after"] = f"not read ({type(e).__name__})"
    print(json.dumps(res))


if __name__ == "__main__":
    main()
