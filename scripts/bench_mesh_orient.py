"""Times mesh orientation (csrc/rx_meshsample.hip, through ops.mesh_sample / mesh_face_cos / mesh_select) on one stated synthetic
case -- the surface-nets mesh of the synthetic sheet of scripts/bench_isosurface.py under a random (3, Z, Y, X) uint16 field --
against a torch formulation on the same device (`grid_sample` on the volume decoded to float32, index ops for the cosine and the
selection) and against the numpy statements on the host of the same machine, and checks that kernels and statements give the same
bytes (the torch formulation rounds differently and is only timed).  Each device time is the median over --reps calls, every call
between two events after three warm-up calls; the host time is one call.

    python scripts/bench_mesh_orient.py [--size 256] [--reps 20]
Prints one JSON line."""
import argparse
import json
import os
import runpy
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def _median_ms(torch, fn, reps):
    times = []
    for rep in range(reps + 3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        if rep >= 3:      # three warm-up calls
            times.append(e0.elapsed_time(e1))
    return round(float(np.median(times)), 4), out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args(argv)
    import torch
    import mt3d_amd  # noqa: F401
    import mt3d_amd.postprocess as pp
    from mt3d_amd.engine import lib as L
    from mt3d_amd.engine import ops
    L.require_device()
    sheet_volume = runpy.run_path(os.path.join(HERE, "bench_isosurface.py"))["sheet_volume"]
    dv, dt = ops.iso_mesh(torch.from_numpy(sheet_volume(a.size)).cuda(), 127)
    hv, ht = dv.cpu().numpy(), dt.cpu().numpy()
    n = a.size
    field = np.random.default_rng(0).integers(0, 65536, (3, n, n, n)).astype(np.uint16)
    field[2] |= 0x8000      # the z component mostly positive: a front and a back
    dfield = torch.from_numpy(field.view(np.int16)).cuda()
    V, T = len(hv), len(ht)

    sample_ms, unit = _median_ms(torch, lambda: ops.mesh_sample(dfield, dv, "normal_u16", unit=True), a.reps)
    cos_ms, (cos, side, used) = _median_ms(torch, lambda: ops.mesh_face_cos(dv, dt, unit, 0.2, "front"), a.reps)
    select_ms, sel = _median_ms(torch, lambda: ops.mesh_select(dv, dt, side == 1, (unit,), used=used), a.reps)

    # the torch formulation: decode once (not timed: a user would keep the decoded volume, 12 bytes per voxel), then sample
    decoded = ((dfield.view(torch.uint16).to(torch.float32) / 65535) * 2 - 1)[None]
    scale = torch.tensor([2.0 / (n - 1)] * 3, device="cuda")

    def torch_sample():
        grid = (dv * scale - 1).view(1, 1, 1, V, 3)
        s = torch.nn.functional.grid_sample(decoded, grid, mode="bilinear", padding_mode="border", align_corners=True).view(3, V).t()
        length = s.norm(dim=1, keepdim=True)
        return torch.where(length > 0, s / length, torch.zeros_like(s))

    def torch_cos(u):
        p = dv[dt]
        g = torch.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0], dim=1)
        m = u[dt].sum(1)
        c = (g * m).sum(1) / torch.sqrt((g * g).sum(1) * (m * m).sum(1))
        return c, (c > 0.2).to(torch.int8) - (c < -0.2).to(torch.int8)

    def torch_select(u, s):
        kept = dt[s == 1]
        ids = torch.unique(kept)
        row = torch.full((V,), -1, dtype=torch.int64, device="cuda")
        row[ids] = torch.arange(len(ids), device="cuda")
        return dv[ids], row[kept], u[ids], row

    torch_sample_ms, tu = _median_ms(torch, torch_sample, a.reps)
    torch_cos_ms, (tc, ts) = _median_ms(torch, lambda: torch_cos(tu), a.reps)
    torch_select_ms, _ = _median_ms(torch, lambda: torch_select(tu, ts), a.reps)
    del decoded

    t0 = time.perf_counter()
    hunit = pp.unit_numpy(pp.sample_points_numpy(field, hv, "normal_u16")[0])
    host_sample_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    hcos = pp.face_cos_numpy(hv, ht, hunit)
    hside = pp.side_numpy(hcos, 0.2)
    host_cos_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    want = pp.select_numpy(hv, ht, hside == 1, hunit)
    host_select_s = time.perf_counter() - t0
    bits = lambda x: np.ascontiguousarray(x.cpu().numpy() if hasattr(x, "cpu") else x, np.float32).view(np.int32)      # noqa: E731
    same = (np.array_equal(bits(unit), bits(hunit)) and np.array_equal(bits(cos), bits(hcos)) and np.array_equal(side.cpu().numpy(), hside)
            and np.array_equal(bits(sel[0]), bits(want[0])) and np.array_equal(sel[1].cpu().numpy(), want[1])
            and np.array_equal(bits(sel[2][0]), bits(want[2][0])) and np.array_equal(sel[3].cpu().numpy(), want[3]))
    # bytes per vertex of the sampling pass: 12 in, 12 out, and 8 corners x 3 channels x 2 bytes gathered (mostly from cache)
    moved = V * (12 + 12 + 8 * 3 * 2)
    res = dict(size=a.size, vertices=V, triangles=T, reps=a.reps, front=int((hside == 1).sum()), back=int((hside == -1).sum()),
               rim=int((hside == 0).sum()), out_vertices=len(want[0]), equal=bool(same),
               sample=dict(device_ms=sample_ms, torch_ms=torch_sample_ms, host_s=round(host_sample_s, 3), bytes_per_vertex=72,
                           gather_gb_s=round(moved / sample_ms / 1e6, 1)),
               face_cos=dict(device_ms=cos_ms, torch_ms=torch_cos_ms, host_s=round(host_cos_s, 3)),
               select=dict(device_ms=select_ms, torch_ms=torch_select_ms, host_s=round(host_select_s, 3)))
    print(json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    main()
