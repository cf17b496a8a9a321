"""A triangle mesh -> the same mesh smoothed, with vertex normals: what follows scripts/volume_to_mesh.py.

    python scripts/refine_mesh.py --mesh PATH [--iterations 10] [--lambda 0.5] [--mu -0.53 | --mu none] [--clamp 1.0 | --clamp none]
                                  [--no-pin-boundary] [--no-normals] [--out FILE] [--max-device-gb G] [--where device|host]

Reads an OBJ or a PLY as `write_obj` / `write_ply` write them, runs Taubin smoothing (a pass with --lambda, then one with --mu, per
iteration; --mu none is the plain Laplacian; --clamp bounds every coordinate's distance from the input), takes the area-weighted
normals of the smoothed mesh and writes `<stem>_refined.<ext>` (or --out).  The whole mesh is resident on the device.  --where
device needs an MI355X and the built library; --where host runs the numpy statement.  Prints the summary as one JSON line."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _number_or_none(s):
    return None if s.lower() in ("none", "null") else float(s)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--mesh", required=True, help="the .obj or .ply file to refine")
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--lambda", dest="lam", type=float, default=0.5)
    ap.add_argument("--mu", type=_number_or_none, default=-0.53)
    ap.add_argument("--clamp", type=_number_or_none, default=1.0)
    ap.add_argument("--no-pin-boundary", action="store_true", help="let boundary vertices move")
    ap.add_argument("--no-normals", action="store_true", help="write positions only")
    ap.add_argument("--out", default=None, help="the file to write (default: <stem>_refined.<ext> next to --mesh)")
    ap.add_argument("--max-device-gb", type=float, default=None, help="device budget (default: half of the free memory)")
    ap.add_argument("--where", choices=("device", "host"), default="device")
    a = ap.parse_args(argv)
    import mt3d_amd  # noqa: F401
    from mt3d_amd.postprocess import MeshRefiner, refine_numpy
    gb = a.max_device_gb
    fmt = None if a.out is None else os.path.splitext(a.out)[1][1:].lower() or None
    refiner = MeshRefiner(a.iterations, a.lam, a.mu, a.clamp, not a.no_pin_boundary, not a.no_normals, fmt,
                          None if gb is None else int(gb * 2**30), refine_numpy if a.where == "host" else None)
    summary = refiner.run(a.mesh, a.out)
    print(json.dumps(summary), flush=True)
    return summary


if __name__ == "__main__":
    main()
