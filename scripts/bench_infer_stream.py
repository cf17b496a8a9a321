"""Streaming sliding-window inference (inference.StreamingInferer) against the HBM-resident SlidingWindowInferer on the same volume:
the cfg2 network, bf16, 128^3 patches, overlap 0.5, a synthetic uint8 zarr of 256 x 768 x 768 (default) on local disk.

    python scripts/bench_infer_stream.py [--z 256 --yx 768] [--runs 3] [--modes raw,zlib,resident] [--tta SPEC ...]
                                         [--tile TY,TX ...] [--skip-empty] [--keep DIR]

Alternates the modes run by run and prints one JSON line per run and a summary line: patches/s and Mvoxel/s of volume, and for the
streaming runs where the host time went (slab reads, waits for the chunk writers).  `--modes raw --runs 1` under
`rocprofv3 --kernel-trace --stats` gives the per-kernel times of rx_sw_gather / rx_sw_accumulate / rx_sw_finalize.

`--tta SPEC` (repeatable) runs the streaming modes with test-time augmentation as well: SPEC is `off`, `flip` or a JSON mapping such
as '{"flip":["z","y","x"],"rot90":["z"]}'.  Every (mode, SPEC) pair is a variant of its own, alternated run by run with the others;
a variant with V views also reports view-forwards/s = V x patches / seconds.  Without the option only `off` runs.

`--tile TY,TX` (repeatable) adds, per streaming mode, a variant run in Y/X tiles of TY x TX owned voxels; it reports the tiles, the
recompute factor and the forwards really made.  `--skip-empty` adds, per streaming mode, a variant with `skip_empty=True` on a copy
of the volume whose half x >= YX / 2 is zero (written next to the volume); it reports the positions skipped.  patches/s and
Mvoxel/s are always those of the volume: positions of the untiled grid and voxels of the whole array per second."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench as B  # noqa: E402
import mt3d_amd  # noqa: E402,F401
from mt3d_amd.builders.build_network_from_config import NetworkFromConfig  # noqa: E402
from mt3d_amd.dataloading import zarr_lite  # noqa: E402
from mt3d_amd.inference import SlidingWindowInferer, StreamingInferer, all_positions  # noqa: E402


def synthetic_volume(path, Z, YX, patch):
    """smooth uint8 structure plus noise (compresses like a real scan would, roughly), written chunk row by chunk row"""
    from concurrent.futures import ThreadPoolExecutor
    rng = np.random.default_rng(0)
    w = zarr_lite.ChunkedWriter(path, (Z, YX, YX), patch, np.uint8, "zlib")
    yy, xx = np.meshgrid(np.arange(YX), np.arange(YX), indexing="ij")
    with ThreadPoolExecutor(16) as pool:
        futs = []
        for z0 in range(0, Z, patch[0]):
            z1 = min(Z, z0 + patch[0])
            zz = np.arange(z0, z1)[:, None, None]
            base = 128 + 60 * np.sin(zz / 23.0 + yy / 31.0) * np.cos(xx / 17.0)
            blk = np.clip(base + rng.normal(0, 12, size=base.shape), 0, 255).astype(np.uint8)
            futs += w.write_rows(z0, blk, pool)
        for f in futs:
            f.result()
    return zarr_lite.open(path)


def half_zeroed_copy(arr, path, patch):
    """the volume with its half x >= X / 2 zeroed, chunk row by chunk row"""
    Z, Y, X = arr.shape
    w = zarr_lite.ChunkedWriter(path, (Z, Y, X), patch, np.uint8, "zlib")
    for z0 in range(0, Z, patch[0]):
        blk = arr[z0:min(Z, z0 + patch[0])].copy()
        blk[:, :, X // 2:] = 0
        w.write_rows(z0, blk)
    return zarr_lite.open(path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--z", type=int, default=256)
    ap.add_argument("--yx", type=int, default=768)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--modes", default="raw,zlib,resident")
    ap.add_argument("--tta", action="append", default=None, metavar="SPEC",
                    help="off, flip or a JSON mapping {flip: [axes], rot90: [axes]}; repeatable, each is run alternated with the others")
    ap.add_argument("--tile", action="append", default=None, metavar="TY,TX", help="owned tile extents; repeatable")
    ap.add_argument("--skip-empty", action="store_true", help="also run with skip_empty=True on a half-zeroed copy of the volume")
    ap.add_argument("--keep", default=None, help="work directory to use (default: a temporary one, removed at the end)")
    a = ap.parse_args()
    patch = (128, 128, 128)
    work = a.keep or tempfile.mkdtemp(prefix="infer_stream_")
    os.makedirs(work, exist_ok=True)
    try:
        t0 = time.perf_counter()
        src = os.path.join(work, "vol.zarr")
        arr = zarr_lite.open(src) if os.path.exists(src) else synthetic_volume(src, a.z, a.yx, patch)
        print(json.dumps({"setup": "volume", "shape": arr.shape, "seconds": round(time.perf_counter() - t0, 2)}), flush=True)
        w = dict(B.WORKLOADS["cfg2"])
        torch.manual_seed(0)
        net = NetworkFromConfig(B.make_mgr(w)).cuda()
        targets = {"sheet": {"channels": 1, "activation": "sigmoid"}}
        shape = tuple(arr.shape)
        n_pos = len(all_positions(shape, patch, 0.5))
        vox = float(np.prod(shape))
        resident = None
        specs = [(t, None if t == "off" else (json.loads(t) if t.lstrip().startswith("{") else t)) for t in (a.tta or ["off"])]
        # a variant: (label, mode, tta, extra StreamingInferer arguments, source); the resident inferer has no views
        modes = [(m if t == "off" else f"{m}+tta:{t}", m, spec, {}, src) for m in a.modes.split(",")
                 for t, spec in (specs if m != "resident" else [("off", None)])]
        for m in [m for m in a.modes.split(",") if m != "resident"]:
            for t in a.tile or []:
                ty, tx = (int(v) for v in t.split(","))
                modes.append((f"{m}+tile:{ty}x{tx}", m, None, {"tile": (ty, tx)}, src))
            if a.skip_empty:
                half = os.path.join(work, "vol_half.zarr")
                if not os.path.exists(half):
                    half_zeroed_copy(arr, half, patch)
                modes.append((f"{m}+skip", m, None, {"skip_empty": True}, half))
        results = {label: [] for label, *_ in modes}
        views = {label: 1 for label, *_ in modes}
        # run 0 of each mode is a warm-up (plan build, lazy buffers, program recording); the modes alternate run by run
        order = [(r, v) for r in range(a.runs + 1) for v in modes]
        for r, (label, m, spec, extra_args, source) in order:
            torch.cuda.synchronize()
            if m == "resident":
                if resident is None:
                    resident = torch.from_numpy(arr[...].astype(np.float32) / np.float32(255.0)).cuda()[None]
                inf = SlidingWindowInferer(net, targets, patch, batch_size=a.batch, overlap=0.5, compute_dtype=torch.bfloat16)
                t = time.perf_counter()
                out = inf(resident)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t
                del out
                extra = {}
            else:
                out_dir = os.path.join(work, f"out_{r}")
                inf = StreamingInferer(net, targets, patch, batch_size=a.batch, overlap=0.5, compute_dtype=torch.bfloat16, tta=spec,
                                       **extra_args)
                t = time.perf_counter()
                inf.run(source, out_dir, compressor=None if m == "raw" else "zlib")
                torch.cuda.synchronize()
                dt = time.perf_counter() - t
                tm = inf.last_timing
                views[label] = tm["views"]
                extra = {"read_s": round(tm["read_s"], 3), "write_wait_s": round(tm["write_wait_s"], 3),
                         "device_MiB": round(inf.last_schedule["device_bytes"] / 2**20, 1), "views": tm["views"],
                         "view_forwards_per_s": round(tm["views"] * n_pos / dt, 2), "forwards": tm["forwards"],
                         "tiles": tm["tiles"], "recompute": round(inf.last_schedule["recompute"], 4), "skipped": tm["skipped"]}
                shutil.rmtree(out_dir, ignore_errors=True)
            rec = dict(mode=label, run=r, warmup=r == 0, seconds=round(dt, 3), patches_per_s=round(n_pos / dt, 2),
                       mvoxel_per_s=round(vox / dt / 1e6, 2), **extra)
            print(json.dumps(rec), flush=True)
            if r > 0:
                results[label].append(dt)
        summ = {m: dict(median_s=round(float(np.median(v)), 3), min_s=round(min(v), 3), max_s=round(max(v), 3),
                        patches_per_s=round(n_pos / float(np.median(v)), 2),
                        view_forwards_per_s=round(views[m] * n_pos / float(np.median(v)), 2),
                        mvoxel_per_s=round(vox / float(np.median(v)) / 1e6, 2)) for m, v in results.items() if v}
        if "resident" in summ:
            for m in summ:
                summ[m]["vs_resident"] = round(summ["resident"]["median_s"] / summ[m]["median_s"], 3)
        print(json.dumps({"summary": summ, "patches": n_pos, "shape": shape, "batch": a.batch}), flush=True)
    finally:
        if not a.keep:
            shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
