"""CPU: the numpy statements of the connected-component pass against scipy.ndimage.label, the host half of the out-of-core run and the
whole two-pass `ComponentFilter` with `label_numpy` in place of the kernels, the config block, and the kernels' own find / union /
tile-merge logic (csrc/rx_components_core.h) run serially under the address and undefined-behaviour sanitizers."""
import json
import os
import subprocess

import numpy as np
import pytest

import components_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pp():
    import mt3d_amd  # noqa: F401
    import mt3d_amd.postprocess as pp
    return pp


def _scipy_labels(mask, connectivity):
    """scipy numbers components in raster order of first encounter, so label k's first voxel is its smallest index: the oracle is
    1 + first[k - 1] gathered by label, 0 on background"""
    ndi = pytest.importorskip("scipy.ndimage")
    lab, n = ndi.label(mask, ndi.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[connectivity]))
    flat = lab.reshape(-1)
    idx = np.nonzero(flat)[0]
    first = np.zeros(n + 1, np.int64)
    k, where = np.unique(flat[idx], return_index=True)
    first[k] = idx[where] + 1
    return first[lab].astype(np.int32), lab, n


CASES = C.cases()


@pytest.mark.parametrize("connectivity", C.CONNECTIVITIES)
def test_statements_against_scipy(connectivity):
    pp = _pp()
    for name, mask in CASES:
        want, lab, n = _scipy_labels(mask, connectivity)
        got = pp.label_numpy(mask, connectivity)
        assert got.dtype == np.int32 and np.array_equal(got, want), (name, connectivity)
        counts = np.bincount(lab.reshape(-1), minlength=n + 1)[1:]      # by scipy's numbering
        sizes = pp.component_sizes_numpy(got)
        assert sizes.dtype == np.int32 and sizes.shape == (mask.size,)
        roots = np.unique(want[want > 0]) - 1
        assert np.array_equal(np.nonzero(sizes)[0], roots) and np.array_equal(np.sort(sizes[roots]), np.sort(counts)), name
        assert np.array_equal(sizes[want[mask] - 1], counts[lab[mask] - 1]), name
        if n:
            values = np.where(mask, 200, 5).astype(np.uint8)
            cut = int(np.sort(counts)[len(counts) // 2])      # exactly a component's size: it is kept, one more drops it
            for mv in (cut, cut + 1):
                f, labels = pp.filter_numpy(values, 127, connectivity, mv)
                keep = mask & (np.concatenate([[0], counts])[lab] >= mv)
                assert np.array_equal(labels, want) and np.array_equal(f, np.where(keep, values, 0)), (name, mv)


def test_the_cases_are_what_they_claim():
    pp = _pp()

    def count(mask, c):
        lab = pp.label_numpy(mask, c)
        return len(np.unique(lab[lab > 0]))
    assert count(C.serpentine((6, 40, 40)), 6) == 1
    cb = dict(C.masks((9, 10, 12)))["checkerboard"]
    assert (count(cb, 26), count(cb, 18), count(cb, 6)) == (1, 1, int(cb.sum()))
    big = dict(C.masks((40, 40, 130)))
    assert [count(big["corner_pair"], c) for c in (6, 18, 26)] == [2, 2, 1]
    assert [count(big["edge_pair"], c) for c in (6, 18, 26)] == [2, 1, 1]
    lab = pp.label_numpy(big["backward_root"], 6)
    assert lab[-1, -1, -1] == 2 and count(big["backward_root"], 6) == 1      # the root is voxel (0, 0, 1)
    mid = dict(C.masks((33, 17, 70)))
    n = [count(mid[k], c) for k in ("random10", "random30", "random60") for c in (6, 18, 26)]
    assert min(n) == 1 and max(n) > 2000      # both the one-giant and the many-tiny regime occur


def test_union_find_terminates_on_a_long_serpentine():
    pp = _pp()
    lab = pp.label_numpy(C.serpentine((2, 400, 300)), 6)      # diameter ~ 60000: whole-volume min-propagation would need that many sweeps
    assert np.array_equal(np.unique(lab), [0, 1])


# ---- the out-of-core run on the host ---------------------------------------------------------------------------------------------------
def _store(tmp_path, name, values, chunks=(8, 16, 16)):
    from mt3d_amd.dataloading import zarr_lite
    store = tmp_path / name
    os.makedirs(store)
    zarr_lite.write_array(str(store / "sheet_final"), values, chunks, compressor="zlib")
    return str(store)


def _read(store, name):
    from mt3d_amd.dataloading import zarr_lite
    return zarr_lite.open(os.path.join(store, name))[...]


def _compact(labels, sizes, min_voxels):
    kept = np.nonzero(sizes >= min_voxels)[0]
    table = np.zeros(sizes.size + 1, np.uint32)
    table[kept + 1] = np.arange(1, kept.size + 1)
    return table[labels]


@pytest.mark.parametrize("connectivity", C.CONNECTIVITIES)
@pytest.mark.parametrize("kind", ["random", "serpentine"])
def test_component_filter_is_the_same_at_every_slab_depth(tmp_path, kind, connectivity):
    pp = _pp()
    shape = (20, 24, 40)
    values = C.sheet_values(shape) if kind == "random" else np.where(C.serpentine(shape), 255, 0).astype(np.uint8)
    sizes_all = pp.component_sizes_numpy(pp.label_numpy(values > 127, connectivity))
    big = np.sort(sizes_all[sizes_all > 0])[::-1]
    min_voxels = 40 if kind == "random" else 1
    want, labels = pp.filter_numpy(values, 127, connectivity, min_voxels)
    if kind == "random":      # the plate spans every slab and survives; the blob lies inside one slab and survives; speckle goes
        assert want[:, 2, 3].all() and want[12, 15, 21] == 255 and (want != values).any()
        assert labels[12, 15, 21] - 1 == 12 * 24 * 40 + 15 * 40 + 21
    summary = dict(level=127, connectivity=connectivity, min_voxels=min_voxels, components=int((sizes_all > 0).sum()),
                   kept=int((sizes_all >= min_voxels).sum()), voxels=int(sizes_all.sum()),
                   kept_voxels=int(sizes_all[sizes_all >= min_voxels].sum()), largest=[int(s) for s in big[:10]])
    for s in (2, 3, 7, 20):
        store = _store(tmp_path, f"{kind}{connectivity}_{s}", values)
        f = pp.ComponentFilter(127, connectivity, min_voxels, write_labels=True, slab=s, labeler=pp.label_values_numpy)
        got = f.run(store, "sheet")
        assert f.last_slab == s
        assert got == summary and json.load(open(os.path.join(store, "sheet_filtered", ".zattrs"))) == summary, s
        out, lab = _read(store, "sheet_filtered"), _read(store, "sheet_labels")
        assert out.dtype == np.uint8 and np.array_equal(out, want), s
        assert lab.dtype == np.uint32 and np.array_equal(lab, _compact(labels, sizes_all, min_voxels)), s
        meta, src = (json.load(open(os.path.join(store, n, ".zarray"))) for n in ("sheet_filtered", "sheet_final"))
        assert meta["chunks"] == src["chunks"] and meta["compressor"] == src["compressor"]


def test_merge_slabs_links_the_larger_id_under_the_smaller():
    pp = _pp()
    # two slabs of one row each, 1 x 4 planes: slab 0 holds voxels 1 and 3 (two components), slab 1 voxels 0, 1, 2 (one component)
    t0 = (np.array([1, 3], np.int32), np.array([1, 1], np.int32))
    t1 = (np.array([0], np.int32), np.array([3], np.int32))
    seam = (np.array([[0, 2, 0, 4]], np.int32), np.array([[1, 1, 1, 0]], np.int32))
    (r0, s0), (r1, s1) = pp.merge_slabs([t0, t1], [seam], 6, [0, 1])
    assert r0.dtype == np.int64 and s0.dtype == np.int64
    assert r0.tolist() == [1, 3] and s0.tolist() == [4, 1] and r1.tolist() == [1] and s1.tolist() == [4]      # 6: only (0, 1) touches
    (r0, s0), (r1, s1) = pp.merge_slabs([t0, t1], [seam], 18, [0, 1])
    assert r0.tolist() == [1, 1] and s0.tolist() == [5, 5] and r1.tolist() == [1] and s1.tolist() == [5]      # 18: (0, 3) - (1, 2) too
    assert r1[0] < 4 + 0      # the id of slab 1's root, 1 * 4 + 0, went under the smaller one


def test_refusals(tmp_path):
    pp = _pp()
    values = C.sheet_values((4, 8, 8))
    store = _store(tmp_path, "a", values, chunks=(4, 8, 8))
    f = pp.ComponentFilter(127, 26, 3, labeler=pp.label_values_numpy)
    f.run(store, "sheet")
    with pytest.raises(FileExistsError, match="sheet_filtered"):
        f.run(store, "sheet")
    with pytest.raises(ValueError, match="ink"):
        f.run(store, "ink")
    from mt3d_amd.dataloading import zarr_lite
    zarr_lite.write_array(os.path.join(store, "normals_final"), np.zeros((3, 4, 8, 8), np.uint8), (3, 4, 8, 8))
    zarr_lite.write_array(os.path.join(store, "wide_final"), np.zeros((4, 8, 8), np.uint16), (4, 8, 8))
    for task in ("normals", "wide"):
        with pytest.raises(ValueError, match=task):
            f.run(store, task)
    # a budget below two slices: 2 * 9 * 8 * 8 = 1152 bytes
    with pytest.raises(MemoryError, match=r"two slices of a 8 x 8 plane need 1152 bytes"):
        pp.ComponentFilter(127, 26, 3, max_device_bytes=1151, labeler=pp.label_values_numpy).run(_store(tmp_path, "b", values), "sheet")
    g = pp.ComponentFilter(127, 26, 3, max_device_bytes=1152, labeler=pp.label_values_numpy)
    g.run(_store(tmp_path, "c", values), "sheet")
    assert g.last_slab == 2
    g = pp.ComponentFilter(127, 26, 3, max_device_bytes=4 * 9 * 64 - 1, labeler=pp.label_values_numpy)      # just under the whole volume
    g.run(_store(tmp_path, "d", values), "sheet")
    assert g.last_slab == 3
    for kw, key in ((dict(level=255), "level"), (dict(level=-1), "level"), (dict(connectivity=8), "connectivity"),
                    (dict(min_voxels=0), "min_voxels")):
        with pytest.raises(ValueError, match=key):
            pp.ComponentFilter(**{**dict(level=127, connectivity=26, min_voxels=1), **kw})


TARGETS = {"sheet": {"channels": 1, "activation": "sigmoid"}, "normals": {"channels": 3}}


def test_parse_config():
    pp = _pp()
    assert pp.parse_config(None, TARGETS) is None
    ok = {"tasks": ["sheet"], "min_voxels": 20000}
    assert pp.parse_config({"components": ok}, TARGETS)["components"] == dict(
        tasks=("sheet",), level=127, connectivity=26, min_voxels=20000, write_labels=False, max_device_gb=None)
    full = {"tasks": ["sheet"], "level": 100, "connectivity": 6, "min_voxels": 5, "write_labels": True, "max_device_gb": 8}
    assert pp.parse_config({"components": full}, TARGETS, (16, 16, 16))["components"] == dict(
        tasks=("sheet",), level=100, connectivity=6, min_voxels=5, write_labels=True, max_device_gb=8.0)
    bad = [({"holes": {}}, "holes"), ({"components": {**ok, "colour": 1}}, "colour"), ({"components": {**ok, "tasks": ["ink"]}}, "ink"),
           ({"components": {**ok, "tasks": ["normals"]}}, "normals"), ({"components": {**ok, "level": 255}}, "level"),
           ({"components": {**ok, "level": -1}}, "level"), ({"components": {**ok, "connectivity": 8}}, "connectivity"),
           ({"components": {**ok, "min_voxels": 0}}, "min_voxels"), ({"components": {"tasks": ["sheet"]}}, "min_voxels"),
           ({"components": {**ok, "write_labels": "yes"}}, "write_labels"), ({"components": {**ok, "max_device_gb": 0}}, "max_device_gb"),
           ({"components": {"min_voxels": 3}}, "tasks")]
    for block, key in bad:
        with pytest.raises(ValueError, match=key):
            pp.parse_config(block, TARGETS)
    with pytest.raises(ValueError, match="patch_size"):
        pp.parse_config({"components": ok}, TARGETS, (64, 64))


def test_config_manager_key(tmp_path):
    import yaml
    import mt3d_amd  # noqa: F401
    from mt3d_amd.configuration.config_manager import ConfigManager

    def cfg(ic):
        p = tmp_path / "cfg.yaml"
        p.write_text(yaml.safe_dump({"tr_setup": {}, "tr_config": {"patch_size": [16, 16, 16]}, "model_config": {},
                                     "dataset_config": {"targets": {"sheet": {"channels": 1, "activation": "sigmoid"}}},
                                     "inference_config": ic}))
        return str(p)
    assert ConfigManager(cfg({}), verbose=False).infer_postprocess is None
    m = ConfigManager(cfg({"postprocess": {"components": {"tasks": ["sheet"], "min_voxels": 7}}}), verbose=False)
    assert m.infer_postprocess["components"]["min_voxels"] == 7 and m.infer_postprocess["components"]["tasks"] == ("sheet",)
    with pytest.raises(ValueError, match="inference_config.postprocess.components.connectivity"):
        ConfigManager(cfg({"postprocess": {"components": {"tasks": ["sheet"], "min_voxels": 7, "connectivity": 4}}}), verbose=False)


def test_command_line(tmp_path, capsys):
    pp = _pp()
    from mt3d_amd.postprocess.__main__ import main
    values = C.sheet_values((20, 24, 40))
    store = _store(tmp_path, "cli", values)
    orig = pp.components.ComponentFilter.__init__

    def host_init(self, *a, **k):      # the command line has no `labeler`: give it the host one, there is no device here
        orig(self, *a, **k)
        self.labeler = pp.label_values_numpy
    pp.components.ComponentFilter.__init__ = host_init
    try:
        got = main(["--store", store, "--task", "sheet", "--min-voxels", "40", "--connectivity", "18", "--slab", "7", "--write-labels"])
    finally:
        pp.components.ComponentFilter.__init__ = orig
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == got and got["connectivity"] == 18
    assert np.array_equal(_read(store, "sheet_filtered"), pp.filter_numpy(values, 127, 18, 40)[0])
    assert os.path.exists(os.path.join(store, "sheet_labels"))


# ---- the kernels' own logic on the CPU, under the sanitizers ------------------------------------------------------------------------------
def test_host_check_program(tmp_path):
    """csrc/rx_components_core.h is what the kernels call.  A stand-alone C++ program runs it serially over this file's shapes and
    mask kinds, in three visiting orders, against a breadth-first search of its own, compiled with -fsanitize=address,undefined."""
    csrc = os.path.join(ROOT, "multi-task-3d-resencoder-unet_amd", "csrc")
    exe = str(tmp_path / "components_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wno-unknown-pragmas", os.path.join(csrc, "tools", "components_host_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    n = len(C.SHAPES) * len(C.masks((2, 2, 2))) * len(C.CONNECTIVITIES) * 3
    assert r.returncode == 0 and f"{n} cases, 0 differ from the breadth-first search" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_a_failed_run_leaves_nothing_and_the_store_convention_is_kept(tmp_path):
    pp = _pp()
    from mt3d_amd.dataloading import zarr_lite
    values = C.sheet_values((20, 24, 40))
    store = tmp_path / "s"
    os.makedirs(store)
    zarr_lite.write_array(str(store / "sheet_final"), values, (8, 16, 16), compressor=None, dimension_separator="/")
    calls = []

    def failing(v, level, connectivity):      # fails in pass 2, after rows have been written
        calls.append(1)
        if len(calls) == 5:
            raise RuntimeError("labeler gave up")
        return pp.label_values_numpy(v, level, connectivity)
    with pytest.raises(RuntimeError, match="gave up"):
        pp.ComponentFilter(127, 26, 40, write_labels=True, slab=7, labeler=failing).run(str(store), "sheet")
    assert sorted(os.listdir(store)) == ["sheet_final"]
    pp.ComponentFilter(127, 26, 40, write_labels=True, slab=7, labeler=pp.label_values_numpy).run(str(store), "sheet")      # the rerun is not blocked
    assert sorted(os.listdir(store)) == ["sheet_filtered", "sheet_final", "sheet_labels"]
    assert np.array_equal(_read(str(store), "sheet_filtered"), pp.filter_numpy(values, 127, 26, 40)[0])
    for n in ("sheet_filtered", "sheet_labels"):
        meta = json.load(open(store / n / ".zarray"))
        assert meta["dimension_separator"] == "/" and meta["compressor"] is None and meta["chunks"] == [8, 16, 16]


def test_a_slab_never_exceeds_the_label_range():
    pp = _pp()
    host = dict(labeler=pp.label_values_numpy)
    plane = (1 << 14, 1 << 14)      # 2^28 voxels: 7 rows are the most whose index + 1 fits int32
    assert pp.ComponentFilter(min_voxels=1, **host).slab_depth((10,) + plane) == 7
    assert pp.ComponentFilter(min_voxels=1, max_device_bytes=1 << 50).slab_depth((10,) + plane) == 7
    assert pp.ComponentFilter(min_voxels=1, slab=7, **host).slab_depth((10,) + plane) == 7
    with pytest.raises(ValueError, match="slab 8.*at most 7 rows"):
        pp.ComponentFilter(min_voxels=1, slab=8, **host).slab_depth((10,) + plane)
    with pytest.raises(ValueError, match="more than 2\\^31 - 2 voxels"):      # not a matter of the budget
        pp.ComponentFilter(min_voxels=1, max_device_bytes=1 << 50).slab_depth((4, 1 << 15, 1 << 15))
