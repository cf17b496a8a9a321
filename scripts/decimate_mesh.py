"""A triangle mesh -> the same surface with far fewer triangles: what follows scripts/refine_mesh.py.

    python scripts/decimate_mesh.py --mesh PATH --cell C [--representative mean|nearest] [--no-normals] [--out FILE]
                                    [--max-device-gb G] [--where device|host]

Reads an OBJ or a PLY as `write_obj` / `write_ply` / `write_refined` write them, clusters its vertices on a grid of cubes with edge
--cell (in the mesh's units: voxels), replaces every cluster by one representative (the mean of its members, or the member nearest
the cube's centre), drops the triangles that collapse or repeat, takes the area-weighted normals of the result and writes
`<stem>_decimated.<ext>` (or --out).  The whole mesh is resident on the device.  --where device needs an MI355X and the built
library; --where host runs the numpy statement.  Prints the summary as one JSON line."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--mesh", required=True, help="the .obj or .ply file to decimate")
    ap.add_argument("--cell", type=float, required=True, help="the edge of a grid cell, in the mesh's units")
    ap.add_argument("--representative", choices=("mean", "nearest"), default="mean")
    ap.add_argument("--no-normals", action="store_true", help="write positions only")
    ap.add_argument("--out", default=None, help="the file to write (default: <stem>_decimated.<ext> next to --mesh)")
    ap.add_argument("--max-device-gb", type=float, default=None, help="device budget (default: half of the free memory)")
    ap.add_argument("--where", choices=("device", "host"), default="device")
    a = ap.parse_args(argv)
    import mt3d_amd  # noqa: F401
    from mt3d_amd.postprocess import MeshDecimator, decimate_numpy
    gb = a.max_device_gb
    fmt = None if a.out is None else os.path.splitext(a.out)[1][1:].lower() or None
    decimator = MeshDecimator(a.cell, a.representative, not a.no_normals, fmt, None if gb is None else int(gb * 2**30),
                              decimate_numpy if a.where == "host" else None)
    summary = decimator.run(a.mesh, a.out)
    print(json.dumps(summary), flush=True)
    return summary


if __name__ == "__main__":
    main()
