"""Regenerate tests/golden/patch_search.npz: what the REFERENCE's own `find_label_bounding_box` and `_find_valid_patches`
(helpers.py) return on small in-memory label arrays, pinning dataloading/dataset.py: find_label_bounding_box / find_valid_patches
and, through them, the device search.

    RX_REFERENCE_ROOT=<reference checkout> python scripts/make_patch_search_fixture.py

The reference's helpers.py imports `zarr`, `fsspec` and `tqdm` at module level; none of them touches the two functions beyond
tqdm's progress bar, so whichever is not installed is stubbed (`load_reference_helpers`).  `_find_valid_patches` runs as it is,
its 4-process Pool included.  Recorded per case i: `label_i` (uint8 or uint16, at most 40^3), `patch_i` (3), `thr_i` (bbox
threshold, label threshold), `bbox_i` (6: the reference's bounding box, (D, -1, H, -1, W, -1) for an empty label) and `starts_i`
(n, 3: the start positions in the reference's order).  Cases: seeded blobs over two thresholds pairs with a cubic, an odd and an
anisotropic (8, 12, 16) patch; an all-zero label; a label whose bounding box is thinner than the patch along one axis (both
give no patches).  Needs the reference tree at generation time only."""
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "patch_search.npz")


class _Bar:
    """what helpers.py uses of tqdm: a context manager with update(), and a pass-through iterator"""

    def __init__(self, iterable=None, **kw):
        self.iterable = iterable

    def __iter__(self):
        return iter(self.iterable)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def update(self, n=1):
        pass


def load_reference_helpers(ref_root):
    """the reference's helpers.py as a module, with its absent third-party imports stubbed"""
    sys.dont_write_bytecode = True
    for name in ("zarr", "fsspec", "tqdm"):
        if name in sys.modules:
            continue
        try:
            importlib.import_module(name)
        except ImportError:
            stub = types.ModuleType(name)
            if name == "tqdm":
                stub.tqdm = _Bar
            sys.modules[name] = stub
    spec = importlib.util.spec_from_file_location("ref_patch_helpers", os.path.join(ref_root, "helpers.py"))
    ref = importlib.util.module_from_spec(spec)
    sys.modules["ref_patch_helpers"] = ref      # the Pool's workers unpickle _check_patch_chunk by module name
    spec.loader.exec_module(ref)
    return ref


def run_reference(ref, label, patch, bbox_threshold, label_threshold):
    """(bbox (6,) int64, starts (n, 3) int64) from the reference's two functions, progress output swallowed"""
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        bbox = ref.find_label_bounding_box(label)
        found = ref._find_valid_patches(label, tuple(patch), bbox_threshold=bbox_threshold, label_threshold=label_threshold)
    assert all(p["volume_idx"] == 0 for p in found)
    starts = np.array([p["start_pos"] for p in found], np.int64).reshape(-1, 3)
    return np.array([int(v) for v in bbox], np.int64), starts


def blobs(shape, seed, dtype, density):
    """a label with structure at the patch scale: a box of seeded noise inside an empty margin, with a hole and a sparse corner, so
    that candidates fail for each of the three reasons"""
    rng = np.random.default_rng(seed)
    D, H, W = shape
    lab = np.zeros(shape, dtype)
    top = np.iinfo(dtype).max
    lab[3:D - 2, 2:H - 3, 4:W - 1] = (rng.random((D - 5, H - 5, W - 5)) < density) * top
    lab[D // 3:D // 3 + D // 4, H // 4:H // 4 + H // 3, W // 2:W // 2 + W // 4] = 0          # an empty hole
    sparse = rng.random((D // 3, H // 3, W // 3)) < 0.01
    lab[D - D // 3 - 2:D - 2, 2:2 + H // 3, 4:4 + W // 3] = sparse * top                       # a thinly labelled corner
    return lab


def cases():
    """(label, patch, bbox_threshold, label_threshold)"""
    out = []
    a = blobs((40, 40, 40), 1, np.uint8, 0.4)
    b = blobs((36, 40, 33), 2, np.uint16, 0.3)
    b[b > 0] = np.random.default_rng(3).integers(1, 65536, size=int((b > 0).sum()), dtype=np.uint16)     # any positive value is a label
    for lab in (a, b):
        for patch in ((16, 16, 16), (9, 11, 13), (8, 12, 16)):
            for thr in ((0.9, 0.1), (0.5, 0.3), (0.97, 0.02)):
                out.append((lab, patch, *thr))
    out.append((np.zeros((24, 20, 28), np.uint8), (8, 8, 8), 0.5, 0.05))                       # nothing labelled
    thin = np.zeros((32, 32, 32), np.uint16)
    thin[4:30, 10:15, 3:29] = 1000                                                              # 5 voxels thick in y, patch 8
    out.append((thin, (8, 8, 8), 0.1, 0.01))
    out.append((thin, (8, 4, 8), 0.1, 0.01))                                                    # ... and a patch that does fit
    return out


def main():
    ref_root = os.environ.get("RX_REFERENCE_ROOT")
    if not ref_root:
        sys.exit("set RX_REFERENCE_ROOT to the reference checkout")
    ref = load_reference_helpers(ref_root)
    arrays = {}
    stored = {}
    n_found = []
    for i, (lab, patch, bt, lt) in enumerate(cases()):
        bbox, starts = run_reference(ref, lab, patch, bt, lt)
        key = id(lab)
        if key not in stored:
            stored[key] = i
            arrays[f"label_{i}"] = lab
        arrays[f"label_of_{i}"] = np.array(stored[key], np.int64)      # labels are stored once
        arrays[f"patch_{i}"] = np.array(patch, np.int64)
        arrays[f"thr_{i}"] = np.array([bt, lt], np.float64)
        arrays[f"bbox_{i}"] = bbox
        arrays[f"starts_{i}"] = starts
        n_found.append(len(starts))
    arrays["n_cases"] = np.array(len(n_found), np.int64)
    print("patches per case:", n_found)
    assert n_found[-3] == 0 and n_found[-2] == 0 and n_found[-1] > 0 and sum(n > 0 for n in n_found) >= 12
    np.savez_compressed(OUT, **arrays)
    size = os.path.getsize(OUT)
    print(OUT, size, "bytes")
    assert size < 512 * 1024


if __name__ == "__main__":
    main()
