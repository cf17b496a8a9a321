"""A triangle mesh and a predicted normal field -> one face of the mesh, with predicted normals: what follows
scripts/decimate_mesh.py.

    python scripts/orient_mesh.py --mesh PATH --store PATH [--normals-name normals_final] [--side front|back|both] [--min-cos 0.2]
                                  [--normals predicted|mesh] [--out FILE] [--max-device-gb G] [--where device|host]

Reads an OBJ or a PLY as `write_obj` / `write_ply` / `write_refined` write them and the (3, Z, Y, X) uint16 array
`<store>/<normals-name>` that streaming inference writes, samples the array at the vertices, classifies every triangle as front,
back or rim by the cosine between its face vector and the sampled vectors, and writes `<stem>_<side>.<ext>` (`_oriented` for both;
or --out) with the sampled unit vectors, or with the output mesh's own normals, as vertex normals.  An array that does not fit the
device budget beside the mesh goes in z-slabs.  --where device needs an MI355X and the built library; --where host runs the numpy
statements.  Prints the summary as one JSON line."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--mesh", required=True, help="the .obj or .ply file to orient")
    ap.add_argument("--store", required=True, help="the zarr store that holds the predicted normals")
    ap.add_argument("--normals-name", default="normals_final", help="the (3, Z, Y, X) uint16 array in --store")
    ap.add_argument("--side", choices=("front", "back", "both"), default="front")
    ap.add_argument("--min-cos", type=float, default=0.2, help="|cos| at or below this is the rim")
    ap.add_argument("--normals", choices=("predicted", "mesh"), default="predicted")
    ap.add_argument("--out", default=None, help="the file to write (default: <stem>_<side>.<ext> next to --mesh)")
    ap.add_argument("--max-device-gb", type=float, default=None, help="device budget (default: half of the free memory)")
    ap.add_argument("--where", choices=("device", "host"), default="device")
    a = ap.parse_args(argv)
    import mt3d_amd  # noqa: F401
    from mt3d_amd.postprocess import MeshOrienter
    gb = a.max_device_gb
    fmt = None if a.out is None else os.path.splitext(a.out)[1][1:].lower() or None
    summary = MeshOrienter(a.side, a.min_cos, a.normals, fmt, None if gb is None else int(gb * 2**30), a.where).run(
        a.mesh, a.store, a.normals_name, a.out)
    print(json.dumps(summary), flush=True)
    return summary


if __name__ == "__main__":
    main()
