"""Times mesh decimation (csrc/rx_meshdecimate.hip, through ops.mesh_decimate) on one stated synthetic mesh -- the surface-nets mesh
of the synthetic sheet of scripts/bench_isosurface.py -- against the numpy statement `decimate_numpy` on the host of the same
machine, for both representatives, and checks that the two give the same bytes.  The device time is the mean over --reps whole
calls between two events after three warm-up calls (the call allocates, launches about twenty kernels and reads two small results
back, all of which a user pays); the host time is one call.

    python scripts/bench_mesh_decimate.py [--size 256] [--cell 4.0] [--reps 10]
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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--cell", type=float, default=4.0)
    ap.add_argument("--reps", type=int, default=10)
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
    res = dict(size=a.size, cell=a.cell, vertices=len(hv), triangles=len(ht), reps=a.reps)
    for representative in ("mean", "nearest"):
        total = 0.0
        for rep in range(a.reps + 3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            got = ops.mesh_decimate(dv, dt, a.cell, representative)
            e1.record()
            torch.cuda.synchronize()
            if rep >= 3:      # three warm-up calls
                total += e0.elapsed_time(e1)
        t0 = time.perf_counter()
        want = pp.decimate_numpy(hv, ht, a.cell, representative)
        host_s = time.perf_counter() - t0
        same = (np.array_equal(got[0].cpu().numpy().view(np.int32), want[0].view(np.int32)) and np.array_equal(got[1].cpu().numpy(), want[1])
                and np.array_equal(got[2].cpu().numpy(), want[2]))
        res[representative] = dict(device_ms=round(total / a.reps, 3), host_s=round(host_s, 3), out_vertices=len(want[0]), out_triangles=len(want[1]),
                                   clusters=int(want[2].max()) + 1, equal=bool(same))
    print(json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    main()
