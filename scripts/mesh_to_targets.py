"""Meshes -> training targets: the reference's write_face_normals_final.py / write_mesh_labels.py / slices_to_zarr.py in one step.

    python scripts/mesh_to_targets.py 'meshes/*.obj' --out normals.zarr --shape Z H W [--min-z Z0]
                                      [--labels | --binary] [--exp-factor 1.5] [--slab 128] [--where device|host]

Writes a zarr v2 group at --out with the array `volume`: by default the (Z, H, W, 3) uint16 normals volume; --labels the (Z, H, W)
uint16 instance labels (mesh i, in sorted path order, paints i + 1); --binary the uint8 sheet mask (255 where a normal was painted).
Volume slice k is the plane z = min_z + k.  Vertex normals are area-weighted (see tasks/normals/mesh_targets.py for what is pinned to
the reference and what is not).  --where device needs an MI355X and the built library; --where host runs the numpy statement."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("meshes", nargs="+", help="OBJ files or glob patterns")
    ap.add_argument("--out", required=True, help="path of the zarr group to create")
    ap.add_argument("--shape", nargs=3, type=int, required=True, metavar=("Z", "H", "W"))
    ap.add_argument("--min-z", type=int, default=0)
    kind = ap.add_mutually_exclusive_group()
    kind.add_argument("--labels", action="store_true", help="instance labels instead of normals")
    kind.add_argument("--binary", action="store_true", help="the uint8 sheet mask instead of normals")
    ap.add_argument("--exp-factor", type=float, default=1.5)
    ap.add_argument("--slab", type=int, default=None, help="slices per device pass (default: one chunk row, 128)")
    ap.add_argument("--where", choices=("device", "host"), default="device")
    ap.add_argument("--zlib", action="store_true", help="compress the chunks")
    args = ap.parse_args(argv)
    import mt3d_amd  # noqa: F401
    from mt3d_amd.tasks.normals.mesh_targets import MeshTargetBuilder, expand_mesh_args
    paths = expand_mesh_args(args.meshes)
    b = MeshTargetBuilder(paths, args.shape, slab=args.slab, min_z=args.min_z, exp_factor=args.exp_factor, where=args.where,
                          compressor="zlib" if args.zlib else None)
    print(f"{len(paths)} meshes, {len(b.triangles)} triangles, {len(b.vertices)} vertices -> {args.out}")
    arr = b.labels_volume(args.out) if args.labels else b.sheet_mask(args.out) if args.binary else b.normals_volume(args.out)
    print(arr)


if __name__ == "__main__":
    main()
