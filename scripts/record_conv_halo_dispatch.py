"""Records what the stride-1 3x3x3 conv entry points dispatch and compute for the calls of tests/conv_halo_cases.py:

    python scripts/record_conv_halo_dispatch.py [--out tests/data/conv_halo_dispatch.json]

Per call: rx_last_conv_kernel(), the `fused` return where there is one, the message of a refused call, and a SHA-256 of every
output.  Run it at the commit whose behaviour is to be pinned, TWICE: when the file exists already, the second run keeps only
what both runs agree on -- a digest that differs becomes null (that output is not reproducible run to run and is pinned by name and
flag only); a kernel name, flag or message that differs is an error.  Delete the file to record afresh."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import conv_halo_cases as C  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=C.JSON_PATH)
    args = ap.parse_args()
    import mt3d_amd  # noqa: F401
    from mt3d_amd.engine import lib, ops
    lib.require_device()
    cases = {cid: C.run(ops, cid) for cid in C.case_ids()}
    if os.path.exists(args.out):
        with open(args.out) as f:
            first = json.load(f)["cases"]
        assert sorted(first) == sorted(cases), "the case list changed between the two runs"
        for cid, rec in cases.items():
            was = first[cid]
            same = {k: v for k, v in rec.items() if k != "sha"} == {k: v for k, v in was.items() if k != "sha"}
            assert same, f"{cid}: {was} then {rec}"
            for name, digest in rec["sha"].items():
                if was["sha"][name] != digest:
                    print(f"{cid}: {name} differs between the two runs -> null")
                    rec["sha"][name] = None
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"cases": cases}, f, indent=0, sort_keys=True)
        f.write("\n")
    names = sorted({rec["kernel"] for rec in cases.values() if rec["kernel"]})
    print(f"{len(cases)} calls recorded into {args.out}; kernels: {', '.join(names)}")


if __name__ == "__main__":
    main()
