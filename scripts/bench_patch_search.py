"""The valid-patch search of the dataset constructor: `find_valid_patches` (host, one process) against
`find_valid_patches_device` (HIP box statistics) on the same synthetic label store.  Prints ONE JSON line.

    python scripts/bench_patch_search.py [--size 512] [--patch 128] [--chunk 128] [--stores raw,zlib] [--no-host] [--streamed-div 4]

The label is size^3 uint8 written with zarr_lite under a temporary directory, once raw and once zlib: wavy sheets about 3 voxels
thick every 16 voxels of y (19 % on) inside a box that leaves an empty margin and with one empty slab cut out of it, so candidates
are kept and rejected for every reason.  Per store:

  host      seconds of `find_valid_patches(store, ...)`: every candidate sliced out of the store (each voxel read and decompressed
            up to eight times), np.argwhere and np.count_nonzero per candidate, on this machine's CPU
  device    seconds of `find_valid_patches_device(store, ...)` end to end, and its `last_timing`: read_s (store reads the caller
            waited for), upload_s, kernel_s (launches up to their synchronise, outputs copied back), host_s (the three tests)
  streamed  the same with max_device_bytes = label bytes / --streamed-div, which forces the two-pass streamed path
  kernel    the candidate launch alone on the resident label: HIP events around one `rx_box_stats` call per round, median of
            `--rounds`; GB/s against what the launch reads, candidates x patch voxels x 1 byte (each voxel up to eight times)

The two lists are compared first; a difference is an error, not a number."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sheets(n):
    """n^3 uint8 0 / 255, built slab by slab (no n^3 float temporaries beyond one slab)"""
    lab = np.zeros((n, n, n), np.uint8)
    y = np.arange(n, dtype=np.float32)[None, :, None]
    x = np.arange(n, dtype=np.float32)[None, None, :]
    m = max(n // 16, 1)
    for z0 in range(0, n, 32):
        z = np.arange(z0, min(z0 + 32, n), dtype=np.float32)[:, None, None]
        on = np.abs(((y + 6 * np.sin(x / 9.0) + 4 * np.cos(z / 7.0)) % 16) - 8) < 1.5
        lab[z0:z0 + 32] = on * np.uint8(255)
    lab[:m], lab[n - m - 3:] = 0, 0
    lab[:, :m + 1], lab[:, n - m:] = 0, 0
    lab[:, :, :m + 2], lab[:, :, n - m - 1:] = 0, 0
    lab[n // 2:n // 2 + n // 5, :, n // 3:] = 0
    return lab


def note(msg):
    print(f"[bench_patch_search] {msg}", file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--patch", type=int, default=128)
    ap.add_argument("--chunk", type=int, default=128)
    ap.add_argument("--stores", default="raw,zlib")
    ap.add_argument("--no-host", action="store_true", help="skip the host search (the lists are then not compared)")
    ap.add_argument("--streamed-div", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--bbox-threshold", type=float, default=0.97)
    ap.add_argument("--label-threshold", type=float, default=0.10)
    args = ap.parse_args()
    import torch

    import mt3d_amd  # noqa: F401
    from mt3d_amd.dataloading import patch_search_device as P
    from mt3d_amd.dataloading import zarr_lite
    from mt3d_amd.dataloading.dataset import find_valid_patches
    from mt3d_amd.engine import lib as L
    from mt3d_amd.engine import ops as E
    L.require_device()
    patch = (args.patch,) * 3
    lab = sheets(args.size)
    res = {"bench": "patch_search", "device": torch.cuda.get_device_name(0), "size": args.size, "patch": args.patch, "chunk": args.chunk,
           "dtype": "uint8", "label_on": round(float(np.count_nonzero(lab)) / lab.size, 4), "cpus": len(os.sched_getaffinity(0))}
    with tempfile.TemporaryDirectory() as tmp:
        for kind in [s for s in args.stores.split(",") if s]:
            t0 = time.perf_counter()
            store = zarr_lite.write_array(os.path.join(tmp, f"label_{kind}.zarr"), lab, (args.chunk,) * 3,
                                          compressor=None if kind == "raw" else "zlib")
            r = {"write_s": round(time.perf_counter() - t0, 3),
                 "store_bytes": sum(os.path.getsize(os.path.join(store.path, f)) for f in os.listdir(store.path))}
            note(f"{kind}: store written in {r['write_s']} s; device search")
            P.find_valid_patches_device(store, patch, args.bbox_threshold, args.label_threshold)      # warm-up: code objects, page cache
            t0 = time.perf_counter()
            dev = P.find_valid_patches_device(store, patch, args.bbox_threshold, args.label_threshold)
            r["device_s"] = round(time.perf_counter() - t0, 4)
            r["device"] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in P.last_timing.items()}
            t0 = time.perf_counter()
            streamed = P.find_valid_patches_device(store, patch, args.bbox_threshold, args.label_threshold,
                                                   max_device_bytes=max(lab.nbytes // args.streamed_div, args.patch * args.size * args.size))
            r["streamed_s"] = round(time.perf_counter() - t0, 4)
            r["streamed"] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in P.last_timing.items()}
            if streamed != dev:
                sys.exit(f"{kind}: the streamed and the resident device searches differ")
            r["patches"], r["candidates"] = len(dev), r["device"]["candidates"]
            if not args.no_host:
                note(f"{kind}: device {r['device_s']} s, streamed {r['streamed_s']} s, {len(dev)} patches; host search")
                t0 = time.perf_counter()
                host = find_valid_patches(store, patch, args.bbox_threshold, args.label_threshold)
                r["host_s"] = round(time.perf_counter() - t0, 3)
                if host != dev:
                    sys.exit(f"{kind}: the device search and the host search differ ({len(dev)} and {len(host)} patches)")
                r["lists_equal"] = True
                r["speedup"] = round(r["host_s"] / r["device_s"], 1)
            res[kind] = r
    note("the candidate launch alone")
    # the candidate launch alone, on the resident label
    vol = torch.from_numpy(lab).cuda()
    _, e = E.box_stats(vol, np.array([[0, 0, 0, *lab.shape]], np.int32))
    zs, ys, xs = P.candidate_starts([int(v) for v in e[0]], patch)
    boxes = np.array([[z, y, x, *patch] for z in zs for y in ys for x in xs], np.int32)
    if len(boxes):
        lib = L.load()
        n = len(boxes)
        nbytes = lib.rx_box_stats_workspace(n)
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        count = torch.empty(n, dtype=torch.int64, device="cuda")
        ext = torch.empty((n, 6), dtype=torch.int32, device="cuda")
        us = []
        for rnd in range(2 + args.rounds):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            L.check(lib.rx_box_stats(vol.data_ptr(), L.RX_SW_U8, *lab.shape, boxes.ctypes.data, n, ws.data_ptr(), nbytes, count.data_ptr(),
                                     ext.data_ptr(), L.stream_ptr()), "rx_box_stats")
            b.record()
            b.synchronize()
            if rnd >= 2:
                us.append(1e3 * a.elapsed_time(b))
        read = n * args.patch ** 3
        res["kernel"] = {"boxes": n, "us_median": round(float(np.median(us)), 1), "us_min": round(min(us), 1), "us_max": round(max(us), 1),
                         "bytes_read": read, "gbps": round(read / (float(np.median(us)) * 1e-6) / 1e9, 1)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
