"""Connected-component kernels: time per call of `ops.cc_label`, `ops.cc_sizes` and `ops.cc_filter` on a synthetic sheet
volume and on the serpentine, against a plain device copy of the same bytes (the floor) and `scipy.ndimage.label` on the host, and
the two-pass `ComponentFilter` against the one-slab one on one store.  Prints ONE JSON line.

    python scripts/bench_components.py [--size 512] [--rounds 7] [--driver-size 256] [--no-host]

Sheet volume: `--size`^3 uint8, three curved slabs four voxels thick at 255 plus speckle (2 % of the voxels at 200), level 127,
connectivity 26.  Serpentine: full-x rows on every second y joined alternately at either end, on every z: one component, the
spiral case.  The labels of volume 0 of each kind are compared with `label_numpy` at the timed size before anything is timed.
`launches_per_volume` is worked out from the shape the way `rx_cc_label` decides it (a tile pass, a seam pass per axis that has more
than one tile, a flatten pass if there is more than one tile); it is not counted on the device.  Timing: HIP events around regions of one call on each of SETS distinct volumes, the arms ALTERNATED round by round
after two warm-up rounds, median [min, max] over the rounds, microseconds per CALL through `engine.ops` (wrapper included).  The
copy arm moves the three calls' algorithmic bytes (5 + 8 + 6 per voxel) with `Tensor.copy_`, half read and half written.  The host
reference is timed once, on ONE volume, with a wall clock.  The driver is timed with a wall clock, reads and writes included."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SETS = 3


def sheet_volume(size, seed):
    r = np.random.default_rng(seed)
    zz, yy, xx = np.meshgrid(*(np.arange(size, dtype=np.float32),) * 3, indexing="ij")
    v = np.zeros((size,) * 3, np.uint8)
    for k in range(3):
        mid = size * (k + 1) / 4 + (size / 16) * np.sin(xx * (6.0 / size) + k + seed) * np.cos(yy * (5.0 / size))
        v[(zz >= mid) & (zz < mid + 4)] = 255
    v[r.random(v.shape) < 0.02] = 200
    return v


def serpentine(size):
    m = np.zeros((size,) * 3, np.uint8)
    m[:, ::2, :] = 255
    for y in range(1, size, 2):
        m[:, y, size - 1 if (y // 2) % 2 == 0 else 0] = 255
    return m


def regions(fns, rounds, sets, warmup=2):
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
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--driver-size", type=int, default=256)
    ap.add_argument("--no-host", action="store_true", help="skip scipy.ndimage.label")
    a = ap.parse_args()
    import torch
    import mt3d_amd  # noqa: F401
    import mt3d_amd.postprocess as pp
    from mt3d_amd.dataloading import zarr_lite
    from mt3d_amd.engine import ops as E
    if not torch.cuda.is_available():
        raise SystemExit("bench_components: needs the GPU (the host path is postprocess.label_numpy)")
    try:
        from scipy import ndimage as ndi
    except ImportError:
        ndi = None
    res = {"size": a.size, "sets": SETS, "rounds": a.rounds, "level": 127, "connectivity": 26, "tile": [8, 8, 64]}
    tiles = [-(-a.size // t) for t in (8, 8, 64)]
    label_launches = 1 + sum(n > 1 for n in tiles) + (tiles[0] * tiles[1] * tiles[2] > 1)

    vox = a.size ** 3
    for name, host in (("sheet", [sheet_volume(a.size, s) for s in range(SETS)]), ("serpentine", [serpentine(a.size)])):
        sets = len(host)
        vals = [torch.from_numpy(h).cuda()[None, None] for h in host]
        labels = torch.empty(vals[0].shape, dtype=torch.int32, device="cuda")
        sizes = torch.empty((1, 1, vox), dtype=torch.int32, device="cuda")
        outv = torch.empty_like(vals[0])
        nbytes = vox * (5 + 8 + 6)
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        got = E.cc_label(vals[0], 127, 26, out=labels)[0, 0].cpu().numpy()
        equal = bool(np.array_equal(got, pp.label_numpy(host[0] > 127, 26)))
        del got

        def all_three(i):
            E.cc_label(vals[i], 127, 26, out=labels)
            E.cc_sizes(labels, out=sizes)
            E.cc_filter(vals[i], labels, sizes, 20000, out=outv)
        t = regions({"cc_label": lambda i: E.cc_label(vals[i], 127, 26, out=labels), "cc_sizes": lambda i: E.cc_sizes(labels, out=sizes),
                     "cc_filter": lambda i: E.cc_filter(vals[i], labels, sizes, 20000, out=outv), "label_sizes_filter": all_three,
                     "copy_same_bytes": lambda i: dst.copy_(src)}, a.rounds, sets)
        all_three(0)      # the tables below describe volume 0, the one the host reference labels
        s = sizes.reshape(-1)
        out = {"voxels": vox, "foreground_share": round(float((vals[0] > 127).float().mean()), 4), "components": int((s > 0).sum()),
               "largest": int(s.max()), "equals_statement": equal,
               "launches_per_volume": {"cc_label": label_launches, "cc_sizes_memset_and_kernel": 2, "cc_filter": 1},
               "label_pass_bytes_per_voxel": 5, "bytes": nbytes}
        out.update(t)
        out["label_sizes_filter"]["GBps"] = round(nbytes / out["label_sizes_filter"]["us"] / 1e3, 1)
        out["label_sizes_filter"]["over_copy"] = round(out["label_sizes_filter"]["us"] / out["copy_same_bytes"]["us"], 1)
        if ndi is not None and not a.no_host:
            t0 = time.perf_counter()
            _, n = ndi.label(host[0] > 127, ndi.generate_binary_structure(3, 3))
            out["scipy_label_s"] = round(time.perf_counter() - t0, 3)
            out["scipy_components"] = int(n)
            out["device_over_scipy"] = round(out["label_sizes_filter"]["us"] / 1e6 / out["scipy_label_s"], 5)
        else:
            out["scipy_label_s"] = "absent" if ndi is None else "not run"
        res[name] = out
        del vals, labels, sizes, outv, src, dst
        torch.cuda.empty_cache()

    # the driver: one slab against four, on one store (wall clock: reads, device work, the host merge and the writes)
    d = a.driver_size
    with tempfile.TemporaryDirectory() as tmp:
        zarr_lite.write_array(os.path.join(tmp, "sheet_final"), sheet_volume(d, 9), (64, 64, 64), compressor="zlib")
        drv = {"size": d}
        for name, slab in (("warm_up", None), ("one_slab", None), ("four_slabs", -(-d // 4))):
            shutil.rmtree(os.path.join(tmp, "sheet_filtered"), ignore_errors=True)
            t0 = time.perf_counter()
            summary = pp.ComponentFilter(127, 26, 20000, slab=slab).run(tmp, "sheet")
            torch.cuda.synchronize()
            if name != "warm_up":
                drv[name + "_s"] = round(time.perf_counter() - t0, 3)
                drv[name + "_kept"] = [summary["components"], summary["kept"]]
        res["driver"] = drv
    try:
        res["device"] = torch.cuda.get_device_name()
    except Exception as e:
        res["device"] = f"not read ({type(e).__name__})"
    print(json.dumps(res))


if __name__ == "__main__":
    main()
