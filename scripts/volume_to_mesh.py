"""A prediction volume -> a triangle mesh: the counterpart of scripts/mesh_to_targets.py.

    python scripts/volume_to_mesh.py --store PATH --task sheet [--source filtered|final] [--level 127] [--format obj|ply]
                                     [--out FILE] [--max-device-gb G] [--slab N] [--where device|host]

Reads `<store>/<task>_<source>` (a single-channel (Z, Y, X) uint8 array), extracts the surface `value > level` by surface nets and
writes `<store>/<task>_<source>.obj` (or .ply, or --out).  Vertices are (x, y, z) in voxel coordinates, what `read_obj` and
`MeshTargetBuilder` take.  A volume beyond the device budget runs in slabs of cell planes and gives the same file.  --where device
needs an MI355X and the built library; --where host runs the numpy statement.  Prints the summary as one JSON line."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--store", required=True, help="the prediction store (the directory that holds <task>_<source>)")
    ap.add_argument("--task", required=True)
    ap.add_argument("--source", choices=("filtered", "final"), default="filtered")
    ap.add_argument("--level", type=int, default=127, help="inside is value > level")
    ap.add_argument("--format", choices=("obj", "ply"), default="obj")
    ap.add_argument("--out", default=None, help="the file to write (default: <store>/<task>_<source>.<format>)")
    ap.add_argument("--max-device-gb", type=float, default=None, help="device budget (default: half of the free memory)")
    ap.add_argument("--slab", type=int, default=None, help="cell planes per slab (default: from the budget)")
    ap.add_argument("--where", choices=("device", "host"), default="device")
    a = ap.parse_args(argv)
    import mt3d_amd  # noqa: F401
    from mt3d_amd.postprocess import SurfaceMesher, surface_nets_numpy
    gb = a.max_device_gb
    mesher = SurfaceMesher(a.level, a.format, None if gb is None else int(gb * 2**30), a.slab, surface_nets_numpy if a.where == "host" else None)
    summary = mesher.run(a.store, a.task, a.source, a.out)
    print(json.dumps(summary), flush=True)
    return summary


if __name__ == "__main__":
    main()
