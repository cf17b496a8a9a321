"""The mesh chain end to end, shared by tests/test_mesh_chain_cpu.py and tests/test_mesh_chain_gpu.py: extract -> refine -> decimate ->
orient on the slab sheet of mesh_orient_cases (with a normals volume that varies) and extract -> refine -> decimate on the graded
ball of mesh_refine_cases, in both formats, with and without normals.  `run` returns, per combination, the SHA-256 of every mesh
file written and every summary dict returned; tests/data/mesh_chain_digests.json holds what the host statements gave.  The device is
the statements bit for bit, so the one recording serves both.

    python tests/mesh_chain.py      # records the digests again, on the host"""
import hashlib
import json
import os

import numpy as np

import mesh_orient_cases as O
import mesh_refine_cases as R

DIGESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "mesh_chain_digests.json")
COMBINATIONS = [(fmt, normals) for fmt in ("obj", "ply") for normals in (True, False)]
CELL = 2.0


def run(tmp, device):
    """-> {"<fmt>-<normals|plain>": {"files": {name: sha256}, "summaries": {"<task>.<stage>": dict}}}"""
    import mt3d_amd  # noqa: F401
    import mt3d_amd.postprocess as pp
    from mt3d_amd.dataloading import zarr_lite
    host = (lambda f: None) if device else (lambda f: f)
    rng = np.random.default_rng(8)
    field = O.constant_field(O.SHEET["shape"]).astype(np.int64) + rng.integers(-3000, 3000, (3,) + O.SHEET["shape"])
    out = {}
    for fmt, normals in COMBINATIONS:
        name = f"{fmt}-{'normals' if normals else 'plain'}"
        store = os.path.join(str(tmp), name)
        zarr_lite.write_array(os.path.join(store, "normals_final"), np.clip(field, 0, 65535).astype(np.uint16), (3, 4, 8, 8), compressor="zlib")
        zarr_lite.write_array(os.path.join(store, "sheet_filtered"), O.sheet_volume(), (4, 8, 8))
        zarr_lite.write_array(os.path.join(store, "ball_filtered"), R.I.ball(R.BALL["shape"], R.BALL["R"], R.BALL["centre"]), (8, 8, 8))
        summaries = {}
        for task in ("sheet", "ball"):
            summaries[f"{task}.mesh"] = pp.SurfaceMesher(127, fmt, mesher=host(pp.surface_nets_numpy)).run(store, task, "filtered")
            path = os.path.join(store, f"{task}_filtered.{fmt}")
            summaries[f"{task}.refine"] = pp.MeshRefiner(normals=normals, refiner=host(pp.refine_numpy)).run(path)
            path = os.path.join(store, f"{task}_filtered_refined.{fmt}")
            summaries[f"{task}.decimate"] = pp.MeshDecimator(CELL, normals=normals, decimator=host(pp.decimate_numpy)).run(path)
        path = os.path.join(store, f"sheet_filtered_refined_decimated.{fmt}")
        orienter = pp.MeshOrienter(normals="predicted" if normals else "mesh", where="device" if device else "host")
        summaries["sheet.orient"] = orienter.run(path, store)
        files = {f: hashlib.sha256(open(os.path.join(store, f), "rb").read()).hexdigest() for f in sorted(os.listdir(store))
                 if f.endswith("." + fmt)}
        out[name] = json.loads(json.dumps(dict(files=files, summaries=summaries)))      # as the recording reads back
    return out


def recorded():
    with open(DIGESTS) as f:
        return json.load(f)


if __name__ == "__main__":
    import sys
    import tempfile
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    with tempfile.TemporaryDirectory() as tmp, open(DIGESTS, "w") as f:
        json.dump(run(tmp, device=False), f, indent=1, sort_keys=True)
        f.write("\n")
