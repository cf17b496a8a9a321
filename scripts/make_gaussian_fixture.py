"""Regenerate tests/golden/gaussian_maps.npz: Gaussian importance maps computed by the REFERENCE's own `compute_gaussian_3d`
(inference/helpers.py:8-68, scipy.ndimage.gaussian_filter) for a few small tiles, pinning `inference.gaussian_importance_map`.

    RX_REFERENCE_ROOT=<reference checkout> python scripts/make_gaussian_fixture.py

Needs the reference tree, scipy and torch at generation time only; the tests read the .npz alone."""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "gaussian_maps.npz")
TILES = [(16, 16, 16), (24, 20, 16), (17, 33, 40), (32, 32, 32), (1, 64, 64), (8, 48, 64)]


def main():
    ref = os.environ.get("RX_REFERENCE_ROOT")
    if not ref:
        sys.exit("set RX_REFERENCE_ROOT to the reference checkout")
    sys.dont_write_bytecode = True
    spec = importlib.util.spec_from_file_location("ref_inference_helpers", os.path.join(ref, "inference", "helpers.py"))
    helpers = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(helpers)
    maps = {}
    for t in TILES:
        g = helpers.compute_gaussian_3d(t).numpy()
        assert g.dtype == np.float32 and g.shape == t
        maps["x".join(str(d) for d in t)] = g
    np.savez_compressed(OUT, **maps)
    print(OUT, os.path.getsize(OUT), "bytes", sorted(maps))


if __name__ == "__main__":
    main()
