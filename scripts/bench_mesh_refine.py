"""Times the mesh-refinement passes (csrc/rx_meshrefine.hip) on the surface-nets mesh of the synthetic sheet of
scripts/bench_isosurface.py against their algorithmic-byte floor at the measured HBM copy rate, and the numpy statement on the mesh of
a crop.  The floor of a pass counts every array it must read or write once: a gathered array (positions, face vectors) once, not
once per use.

    python scripts/bench_mesh_refine.py [--size 512] [--crop 128] [--reps 20]
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
HBM_BYTES_PER_S = 6.29e12      # float4 copy, measured; the spec is 8.0e12


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
    sheet_volume = runpy.run_path(os.path.join(HERE, "bench_isosurface.py"))["sheet_volume"]
    host = sheet_volume(a.size)
    dv, dt = ops.iso_mesh(torch.from_numpy(host).cuda(), 127)
    V, T = dv.shape[0], dt.shape[0]
    t0 = time.perf_counter()
    adj = ops.mesh_adjacency(V, dt)
    torch.cuda.synchronize()
    first_adjacency_ms = (time.perf_counter() - t0) * 1e3
    E = adj.neighbours.shape[0]
    so, sp = L.load(), L.stream_ptr
    i32 = lambda n: torch.empty(n, dtype=torch.int32, device="cuda")      # noqa: E731
    counts, flag, cursor, deg = i32(V), torch.zeros(1, dtype=torch.int32, device="cuda"), i32(V), i32(V)
    foff, offs = torch.empty(V + 1, dtype=torch.int64, device="cuda"), torch.empty(V + 1, dtype=torch.int64, device="cuda")
    faces, raw, nbr, bnd = i32(3 * T), i32(6 * T), i32(E), torch.empty(V, dtype=torch.uint8, device="cuda")
    out, fvec, nrm = torch.empty_like(dv), torch.empty((T, 3), device="cuda"), torch.empty_like(dv)

    def fill():
        L.check(so.rx_mesh_fill(_ptr(dt), T, V, _ptr(foff), _ptr(cursor), 3 * T, _ptr(faces), _ptr(raw), sp()), "fill")
    # (launch, algorithmic bytes, what has to run before every timed launch)
    passes = {
        "count": (lambda: L.check(so.rx_mesh_count(_ptr(dt), T, V, _ptr(counts), _ptr(flag), sp()), "count"), 24 * T + 4 * V, None),
        "scan": (lambda: L.check(so.rx_mesh_scan(_ptr(counts), V, _ptr(foff), sp()), "scan"), 12 * V, None),
        "fill": (fill, 24 * T + 3 * T * 12 + 12 * V, None),
        "canonical": (lambda: L.check(so.rx_mesh_canonical(V, _ptr(foff), 3 * T, _ptr(faces), _ptr(raw), _ptr(deg), _ptr(bnd), sp()), "canonical"),
                      2 * 3 * T * 12 + 13 * V, fill),      # it sorts in place: every timed launch gets freshly filled slots
        "scan_degrees": (lambda: L.check(so.rx_mesh_scan(_ptr(deg), V, _ptr(offs), sp()), "scan"), 12 * V, None),
        "compact": (lambda: L.check(so.rx_mesh_compact(V, _ptr(foff), _ptr(raw), 3 * T, _ptr(offs), E, _ptr(nbr), sp()), "compact"), 8 * E + 16 * V, None),
        "smooth_pass": (lambda: L.check(so.rx_mesh_smooth_pass(_ptr(dv), _ptr(dv), V, _ptr(adj.offsets), _ptr(adj.neighbours), E, _ptr(adj.boundary), 0.5, 1.0,
                                                                _ptr(out), sp()), "smooth"), V * (12 + 12 + 12 + 8 + 1) + 4 * E, None),
        "face_vectors": (lambda: L.check(so.rx_mesh_face_vectors(_ptr(dv), V, _ptr(dt), T, _ptr(fvec), sp()), "faces"), 24 * T + 12 * V + 12 * T, None),
        "vertex_normals": (lambda: L.check(so.rx_mesh_vertex_normals(V, _ptr(adj.face_offsets), _ptr(adj.faces), 3 * T, _ptr(fvec), T, _ptr(nrm), sp()),
                                           "normals"), V * (8 + 12) + 3 * T * 4 + 12 * T, None),
    }
    res = dict(size=a.size, vertices=V, triangles=T, neighbours=E, max_degree=int((adj.offsets[1:] - adj.offsets[:-1]).max().item()),
               hbm_bytes_per_s=HBM_BYTES_PER_S, passes={})
    for name, (fn, nbytes, before) in passes.items():
        total = 0.0
        for rep in range(a.reps + 3):
            if before is not None:
                before()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if rep >= 3:      # three warm-up launches
                total += e0.elapsed_time(e1)
        ms, floor_ms = total / a.reps, nbytes / HBM_BYTES_PER_S * 1e3
        res["passes"][name] = dict(ms=round(ms, 4), bytes=int(nbytes), gb_per_s=round(nbytes / ms / 1e6, 1), floor_ms=round(floor_ms, 4),
                                   ratio_to_floor=round(ms / floor_ms, 2))
    same = all(torch.equal(x, y) for x, y in zip((offs, nbr, bnd, foff, faces), adj))
    res["adjacency_equal"], res["first_adjacency_ms"] = bool(same), round(first_adjacency_ms, 3)
    t0 = time.perf_counter()
    q = ops.mesh_smooth(dv, dt, 10, clamp=1.0, adjacency=adj)
    n = ops.mesh_vertex_normals(q, dt, adjacency=adj)
    torch.cuda.synchronize()
    res["refine_10_iterations_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    c = a.crop
    lo = (a.size - c) // 2
    cv, ct = pp.surface_nets_numpy(np.ascontiguousarray(host[lo:lo + c, lo:lo + c, lo:lo + c]), 127)
    t0 = time.perf_counter()
    sv, sn = pp.refine_numpy(cv, ct)
    res["numpy_crop"] = dict(size=c, s=round(time.perf_counter() - t0, 3), vertices=len(cv), triangles=len(ct))
    gv = ops.mesh_smooth(torch.from_numpy(cv).cuda(), torch.from_numpy(ct).cuda(), 10, clamp=1.0)
    gn = ops.mesh_vertex_normals(gv, torch.from_numpy(ct).cuda())
    res["crop_equal"] = bool(np.array_equal(gv.cpu().numpy().view(np.int32), sv.view(np.int32))
                             and np.array_equal(gn.cpu().numpy().view(np.int32), sn.view(np.int32)))
    print(json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    main()
