"""Times the surface-nets passes (csrc/rx_isosurface.hip) on a synthetic sheet volume against their HBM floor, and the numpy statement on
a crop.  The floor of a pass: one byte read per voxel plus the bytes it writes (classify: the bits and the row counts; emit: the
vertices and triangles, and the bits and offsets it reads), at the measured HBM copy rate.

    python scripts/bench_isosurface.py [--size 512] [--crop 128] [--reps 20]
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HBM_BYTES_PER_S = 6.29e12      # float4 copy, measured; the spec is 8.0e12


def sheet_volume(n, seed=0):
    """a wavy sheet about four voxels thick with a linear ramp across it, plus sparse speckle: what a filtered prediction looks like"""
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(np.arange(n, dtype=np.float32), np.arange(n, dtype=np.float32), np.arange(n, dtype=np.float32), indexing="ij", sparse=True)
    d = np.abs(z - (n / 2 + n / 16 * np.sin(y * (6.28 / n)) * np.cos(x * (6.28 / n))))
    v = np.clip(np.rint(127.5 + 48 * (2.0 - d)), 0, 255).astype(np.uint8)
    v[rng.random(v.shape, dtype=np.float32) < 1e-4] = 255
    return v


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--crop", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args(argv)
    import torch
    import mt3d_amd  # noqa: F401
    import mt3d_amd.postprocess as pp
    from mt3d_amd.engine import lib as L
    from mt3d_amd.engine import ops
    from mt3d_amd.engine.ops.core import _ptr
    L.require_device()
    n = a.size
    host = sheet_volume(n)
    v = torch.from_numpy(host).cuda()
    so, sp = L.load(), L.stream_ptr
    rows, words = (n + 1) * (n + 1), (n + 1 + 63) // 64
    bits = torch.empty((rows, words), dtype=torch.int64, device="cuda")
    counts = torch.empty((rows, 2), dtype=torch.int32, device="cuda")
    offs = torch.empty((rows, 2), dtype=torch.int64, device="cuda")
    totals = torch.empty(2, dtype=torch.int64, device="cuda")
    nv, nt = ops.iso_counts(v, 127)
    vert = torch.empty((nv, 3), dtype=torch.float32, device="cuda")
    tri = torch.empty((nt, 3), dtype=torch.int64, device="cuda")
    passes = {
        "classify": (lambda: L.check(so.rx_iso_classify(_ptr(v), 127, n, n, n, 0, n + 1, _ptr(bits), _ptr(counts), sp()), "classify"),
                     v.numel() + bits.numel() * 8 + counts.numel() * 4),
        "scan": (lambda: L.check(so.rx_iso_scan(_ptr(counts), rows, _ptr(offs), _ptr(totals), sp()), "scan"), counts.numel() * 4 + offs.numel() * 8),
        "emit": (lambda: L.check(so.rx_iso_emit(_ptr(v), 127, n, n, n, 0, _ptr(bits), _ptr(offs), 0, 0, 0, 0, nv, nt // 2, _ptr(vert), _ptr(tri), sp()),
                                 "emit"), v.numel() + bits.numel() * 8 + offs.numel() * 8 + vert.numel() * 4 + tri.numel() * 8),
    }
    out = dict(size=n, vertices=nv, triangles=nt, hbm_bytes_per_s=HBM_BYTES_PER_S, passes={})
    for name, (fn, nbytes) in passes.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / a.reps
        floor_ms = nbytes / HBM_BYTES_PER_S * 1e3
        out["passes"][name] = dict(ms=round(ms, 4), bytes=int(nbytes), gb_per_s=round(nbytes / ms / 1e6, 1), floor_ms=round(floor_ms, 4),
                                   ratio_to_floor=round(ms / floor_ms, 2))
    t = time.perf_counter()
    gv, gt = ops.iso_mesh(v, 127)
    torch.cuda.synchronize()
    out["iso_mesh_ms"] = round((time.perf_counter() - t) * 1e3, 3)
    out["megavoxels_per_s"] = round(n**3 / (sum(p["ms"] for p in out["passes"].values()) * 1e-3) / 1e6, 1)
    c = a.crop
    lo = (n - c) // 2
    crop = np.ascontiguousarray(host[lo:lo + c, lo:lo + c, lo:lo + c])
    t = time.perf_counter()
    sv, st = pp.surface_nets_numpy(crop, 127)
    out["numpy_crop"] = dict(size=c, s=round(time.perf_counter() - t, 3), vertices=len(sv), triangles=len(st))
    dv, dt = ops.iso_mesh(torch.from_numpy(crop).cuda(), 127)
    out["crop_equal"] = bool(np.array_equal(dv.cpu().numpy().view(np.int32), sv.view(np.int32)) and np.array_equal(dt.cpu().numpy(), st))
    print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    main()
