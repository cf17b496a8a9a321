"""`python -m mt3d_amd.postprocess --store PATH --task sheet ...`: connected-component filtering of an existing prediction store."""
import argparse
import json

from .components import ComponentFilter


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m mt3d_amd.postprocess",
                                 description="Remove the small connected components of <store>/<task>_final (HIP engine).")
    ap.add_argument("--store", required=True, help="the prediction store (the directory that holds <task>_final)")
    ap.add_argument("--task", required=True)
    ap.add_argument("--level", type=int, default=127, help="the mask is _final > level")
    ap.add_argument("--connectivity", type=int, default=26, choices=[6, 18, 26])
    ap.add_argument("--min-voxels", type=int, required=True, help="components with fewer voxels are removed")
    ap.add_argument("--write-labels", action="store_true", help="also write <task>_labels (uint32, kept components 1 .. K)")
    ap.add_argument("--max-device-gb", type=float, default=None, help="device budget (default: half of the free memory)")
    ap.add_argument("--slab", type=int, default=None, help="rows per slab (default: from the budget)")
    a = ap.parse_args(argv)
    gb = a.max_device_gb
    summary = ComponentFilter(a.level, a.connectivity, a.min_voxels, a.write_labels, None if gb is None else int(gb * 2**30),
                              a.slab).run(a.store, a.task)
    print(json.dumps(summary), flush=True)
    return summary


if __name__ == "__main__":
    main()
