"""Per-kernel times of the test-time-augmentation ends of streaming inference, split by what the view does to x, at the shapes of
scripts/bench_infer_stream.py: a uint8 ring slab of 128 x 768 x 768, batch 2 of 128^3 patches, one sigmoid channel.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o kt -- python scripts/bench_infer_tta_kernels.py [--reps 20]
    python scripts/bench_infer_tta_kernels.py --parse DIR

The run launches, group after group, `warmup + reps` gathers and as many accumulates with both slots on the same record: the plain
entry points (rx_sw_gather / rx_sw_accumulate), then rx_sw_gather_geom / rx_sw_accumulate_geom with the identity, a z flip, an x
flip, a quarter turn about z (x and y trade places) and one about y (x and z trade places).  `--parse` reads the kernel trace, cuts
the dispatches of each kind into those groups by launch order and prints the median and the spread per group."""
import argparse
import csv
import ctypes
import glob
import json
import os
import sys

sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]

GROUPS = ["plain", "identity", "flip_z", "flip_x", "rot_z (x<->y)", "rot_y (x<->z)"]
WARMUP = 3


def parse(trace_dir, reps):
    rows = []
    for f in glob.glob(trace_dir + "/**/*kernel_trace.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            rows.append((int(r["Start_Timestamp"]), r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    rows.sort()
    per = WARMUP + reps
    for kind in ("sw_gather", "sw_accumulate"):
        d = [(n, us) for _, n, us in rows if kind in n]
        if len(d) != per * len(GROUPS):
            raise SystemExit(f"{kind}: {len(d)} dispatches in the trace, expected {per * len(GROUPS)} (was --reps the same?)")
        for i, g in enumerate(GROUPS):
            part = d[i * per + WARMUP:(i + 1) * per]
            us = sorted(u for _, u in part)
            print(json.dumps({"kernel": part[0][0].split("(")[0][:48], "group": g, "calls": len(us), "median_us": round(us[len(us) // 2], 1),
                              "min_us": round(us[0], 1), "max_us": round(us[-1], 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--parse", default=None, metavar="DIR", help="summarise the kernel trace under DIR instead of running")
    a = ap.parse_args()
    if a.parse:
        return parse(a.parse, a.reps)
    import torch
    import mt3d_amd  # noqa: F401
    from mt3d_amd.dataloading.geometry_device import GeomOp, flip_op, rot90_op
    from mt3d_amd.engine import lib as L
    L.require_device()
    lib = L.load()
    R, Y, X, P, B = 128, 768, 768, 128, 2
    torch.manual_seed(0)
    slab = torch.randint(0, 256, (1, R, Y, X), dtype=torch.uint8, device="cuda")
    xb = torch.empty((B, 1, P, P, P), dtype=torch.float32, device="cuda")
    logits = torch.randn((B, 1, P, P, P), dtype=torch.float32, device="cuda")
    weight = torch.ones((P, P, P), dtype=torch.float32, device="cuda")
    acc = torch.zeros((1, R, Y, X), dtype=torch.float32, device="cuda")
    wsum = torch.zeros((R, Y, X), dtype=torch.float32, device="cuda")
    org = (ctypes.c_int32 * 6)(0, 64, 64, 0, 64, 128)            # two neighbours of a row of positions, overlapping by half
    ops = {"identity": GeomOp(), "flip_z": flip_op(0), "flip_x": flip_op(2), "rot_z (x<->y)": rot90_op("z", 1), "rot_y (x<->z)": rot90_op("y", 1)}
    sp = L.stream_ptr()
    for g in GROUPS:
        for _ in range(WARMUP + a.reps):
            if g == "plain":
                L.check(lib.rx_sw_gather(L.RX_SW_U8, slab.data_ptr(), 1, R, Y, X, B, org, P, P, P, L.RX_SW_SCALE, xb.data_ptr(), None, 0, sp),
                        "rx_sw_gather")
                L.check(lib.rx_sw_accumulate(logits.data_ptr(), B, B, 1, P, P, P, org, L.RX_ACT_SIGMOID, weight.data_ptr(), acc.data_ptr(),
                                             wsum.data_ptr(), R, Y, X, sp), "rx_sw_accumulate")
            else:
                fwd = (ctypes.c_int32 * 24)(*(ops[g].row() * 2))
                inv = (ctypes.c_int32 * 24)(*(ops[g].inverse().row() * 2))
                L.check(lib.rx_sw_gather_geom(L.RX_SW_U8, slab.data_ptr(), 1, R, Y, X, B, org, fwd, P, P, P, L.RX_SW_SCALE, xb.data_ptr(),
                                              None, 0, sp), "rx_sw_gather_geom")
                L.check(lib.rx_sw_accumulate_geom(logits.data_ptr(), B, B, 1, P, P, P, org, inv, 0, L.RX_ACT_SIGMOID, weight.data_ptr(),
                                                  acc.data_ptr(), wsum.data_ptr(), R, Y, X, sp), "rx_sw_accumulate_geom")
        torch.cuda.synchronize()
    print(json.dumps({"groups": GROUPS, "warmup": WARMUP, "reps": a.reps}), flush=True)


if __name__ == "__main__":
    main()
