"""Times the mesh slicing pass (csrc/rx_meshslice.hip) on a synthetic sheet of about 200k triangles cut by a 128-slice slab of
1024 x 1024 images: key scatter plus resolve for normals and for labels, the key-buffer clear, and the numpy statement on a
subsample of the triangles, scaled by the triangle count (the statement's cost is linear in the triangles that reach a slice).

    python scripts/bench_meshslice.py [--grid 317] [--size 1024] [--slices 128] [--iters 5] [--host-triangles 200]

The atomics issued are counted on the host subsample (every in-image paint of the statement is one atomic of the device pass) and
scaled the same way.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def sheet(grid, size, slices, seed=0):
    rng = np.random.default_rng(seed)
    u, v = np.meshgrid(np.arange(grid), np.arange(grid), indexing="ij")
    x = 8 + (size - 16) * u / (grid - 1) + rng.uniform(-0.3, 0.3, u.shape)
    y = size / 2 + size / 4 * np.sin(6.0 * u / grid + 2.0 * v / grid) + rng.uniform(-0.3, 0.3, u.shape)
    z = -0.5 + slices * v / (grid - 1) + rng.uniform(-0.1, 0.1, u.shape)
    verts = np.stack([x, y, z], axis=-1).reshape(-1, 3).astype(np.float32)
    idx = (u * grid + v)[:-1, :-1].reshape(-1)
    a, b, c, d = idx, idx + grid, idx + grid + 1, idx + 1
    tris = np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)]).astype(np.int64)
    return verts, tris


def timed(fn, iters):
    import torch
    fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=317)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--slices", type=int, default=128)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--host-triangles", type=int, default=200)
    args = ap.parse_args()
    import torch
    import mt3d_amd  # noqa: F401
    from mt3d_amd.engine import lib as L
    from mt3d_amd.engine import ops
    from mt3d_amd.tasks.normals import mesh_targets as M
    verts, tris = sheet(args.grid, args.size, args.slices)
    normals = M.vertex_normals_numpy(verts, tris)
    labels = np.ones(len(tris), np.int32)
    w = h = args.size
    nz = args.slices
    dv, dt, dn, dl = (torch.from_numpy(a).cuda() for a in (verts, tris.astype(np.int32), normals, labels))
    keys64 = torch.zeros((nz, h, w), dtype=torch.int64, device="cuda")
    keys32 = torch.zeros((nz, h, w), dtype=torch.int32, device="cuda")
    out_n = {"normals": torch.empty((nz, h, w, 3), dtype=ops._U16, device="cuda")}
    out_l = {"labels": torch.empty((nz, h, w), dtype=ops._U16, device="cuda")}
    lib, geom = L.load(), (w, h, 0, nz, 0, 0, h, w)
    p = lambda t: t.data_ptr()      # noqa: E731

    def keys_normals():
        L.check(lib.rx_mesh_slice_keys(0, p(dv), len(verts), p(dt), len(tris), p(dn), *geom, 1.5, p(keys64), L.stream_ptr()), "keys")

    def keys_labels():
        L.check(lib.rx_mesh_slice_keys(1, p(dv), len(verts), p(dt), len(tris), None, *geom, 0.0, p(keys32), L.stream_ptr()), "keys")

    res = {"triangles": len(tris), "size": args.size, "slices": nz}
    res["normals_total_ms"] = timed(lambda: ops.mesh_slice_normals(dv, dt, dn, w, h, 0, nz, keys=keys64, out=out_n), args.iters)
    res["labels_total_ms"] = timed(lambda: ops.mesh_slice_labels(dv, dt, dl, w, h, 0, nz, keys=keys32, out=out_l), args.iters)
    res["clear_keys64_ms"] = timed(keys64.zero_, args.iters)
    res["clear_keys32_ms"] = timed(keys32.zero_, args.iters)
    res["keys_normals_ms"] = timed(keys_normals, args.iters)          # (onto keys already holding the maxima: the same atomics are issued)
    res["keys_labels_ms"] = timed(keys_labels, args.iters)
    res["painted_normals_voxels"] = int((keys64 != 0).sum())
    res["painted_label_voxels"] = int((keys32 != 0).sum())

    # the statement on a subsample of triangles, all slices each reaches
    rng = np.random.default_rng(1)
    pick = np.sort(rng.choice(len(tris), size=min(args.host_triangles, len(tris)), replace=False))
    sub = tris[pick]
    t0 = time.perf_counter()
    atomics = 0
    for z in range(nz):
        reach = sub[(verts[sub, 2].min(axis=1) <= z) & (z <= verts[sub, 2].max(axis=1))]
        if len(reach):
            atomics += sum(1 for _ in M._normals_events(verts, reach, normals, z, w, h, 1.5))
    t_n = time.perf_counter() - t0
    t0 = time.perf_counter()
    latomics = 0
    for z in range(nz):
        reach = sub[(verts[sub, 2].min(axis=1) <= z) & (z <= verts[sub, 2].max(axis=1))]
        if len(reach):
            latomics += sum(1 for _ in M._labels_events(verts, reach, np.int64(z), w, h))
    t_l = time.perf_counter() - t0
    scale = len(tris) / len(pick)
    res["host_normals_s_scaled"] = t_n * scale
    res["host_labels_s_scaled"] = t_l * scale
    res["normals_atomics"] = int(atomics * scale)
    res["label_atomics"] = int(latomics * scale)
    res["normals_atomics_per_s"] = res["normals_atomics"] / (res["keys_normals_ms"] * 1e-3)
    res["label_atomics_per_s"] = res["label_atomics"] / (res["keys_labels_ms"] * 1e-3)
    res["normals_speedup_vs_host"] = res["host_normals_s_scaled"] / (res["normals_total_ms"] * 1e-3)
    res["labels_speedup_vs_host"] = res["host_labels_s_scaled"] / (res["labels_total_ms"] * 1e-3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
