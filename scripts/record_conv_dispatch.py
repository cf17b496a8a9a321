"""Records what every conv entry point dispatches and computes for the shapes of the dispatch ledger (tests/conv_dispatch_cases.py,
through tests/test_conv_dispatch_gpu.py::test_ledger_row itself) and for the pinned cases of tests/test_ops_gpu.py
(tests/conv_dispatch_record.py: PINNED):

    python scripts/record_conv_dispatch.py [--out tests/data/conv_dispatch.json] [--check]

Per case and entry point: rx_last_conv_kernel() and a SHA-256 of the output.  Run it at the commit whose behaviour is to be pinned,
TWICE: when the file exists already, the second run keeps only what both runs agree on -- a digest that differs becomes null and is
reported; a kernel name that differs is an error.  Delete the file to record afresh.  --check writes nothing: it replays every case
against the file, the pinned ones included (test_ledger_row replays the ledger's on every run of the suite)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import conv_dispatch_record as REC  # noqa: E402
import test_conv_dispatch_gpu as T  # noqa: E402
from test_ops_gpu import out_dim  # noqa: E402


def pinned_pass(ops, case, s, dtn):
    """the random pass of test_ledger_row on a pinned case: the same operands and calls, no reference"""
    half = dtn != "float32"
    x, w, b = T.operands(s, half)
    if s.kind == "convT":
        odims = tuple(d * ss for d, ss in zip(s.dims, s.s))
    else:
        odims = tuple(out_dim(d, kk, ss) for d, kk, ss in zip(s.dims, s.k, s.s))
    r = dict(x=x, w=w, b=b, gy=T.rnd((s.n, s.co, *odims), half, 4, 0.25), base=T.rnd(tuple(x.shape), half, 5, 0.25), odims=odims)
    T.run_entries(ops, s, getattr(torch, dtn), r, f"{case}-{dtn}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=REC.JSON_PATH)
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    import mt3d_amd  # noqa: F401
    from mt3d_amd.engine import lib, ops
    lib.require_device()
    REC.JSON_PATH = args.out
    REC.RECORDING = None if args.check else {}
    for key, dtn in T.CASES:
        T.test_ledger_row(ops, key, dtn)
    for case, s in REC.PINNED.items():
        for dtn in s.dtypes:
            pinned_pass(ops, case, s, dtn)
    if args.check:
        n = sum(len(v) for v in REC.recorded().values())
        nulls = sum(e["sha"] is None for v in REC.recorded().values() for e in v.values())
        print(f"{n} calls replayed against {args.out}: every kernel name and {n - nulls} digests equal ({nulls} null)")
        return
    cases = REC.RECORDING
    if os.path.exists(args.out):
        with open(args.out) as f:
            first = json.load(f)["cases"]
        assert sorted(first) == sorted(cases), "the case list changed between the two runs"
        for case, entries in cases.items():
            assert sorted(entries) == sorted(first[case]), case
            for e, rec in entries.items():
                was = first[case][e]
                assert rec["kernel"] == was["kernel"], f"{case} {e}: {was} then {rec}"
                if was["sha"] != rec["sha"]:
                    print(f"{case} {e}: the output differs between the two runs -> null")
                    rec["sha"] = None
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"cases": cases}, f, indent=0, sort_keys=True)
        f.write("\n")
    n = sum(len(v) for v in cases.values())
    nulls = sum(e["sha"] is None for v in cases.values() for e in v.values())
    names = sorted({e["kernel"] for v in cases.values() for e in v.values()})
    print(f"{n} calls recorded into {args.out} ({nulls} null digests); kernels: {', '.join(names)}")


if __name__ == "__main__":
    main()
