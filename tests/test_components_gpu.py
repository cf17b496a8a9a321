"""Connected components on the device: ops.cc_label / cc_sizes / cc_filter (csrc/rx_components.hip) against the numpy statements of
postprocess/components.py over the shared case list, and `ComponentFilter` resident and in slabs.  Everything is an integer and every
comparison is array_equal."""
import json
import os

import numpy as np
import pytest
import torch

import components_cases as C

pytestmark = pytest.mark.gpu


def _mods():
    import mt3d_amd  # noqa: F401
    import mt3d_amd.postprocess as pp
    from mt3d_amd.engine import lib as L
    from mt3d_amd.engine import ops
    L.require_device()
    return L, ops, pp


_WANT = {}


def _want(pp, name, mask, connectivity):
    """label_numpy of a case, computed once and shared"""
    key = (name, connectivity)
    if key not in _WANT:
        _WANT[key] = pp.label_numpy(mask, connectivity)
        _WANT[key].setflags(write=False)
    return _WANT[key]


@pytest.mark.parametrize("connectivity", C.CONNECTIVITIES)
def test_label_every_case(connectivity):
    _, ops, pp = _mods()
    cases = C.cases()
    got = [(name, mask, ops.cc_label(torch.from_numpy(mask).cuda()[None, None], connectivity=connectivity)) for name, mask in cases]
    torch.cuda.synchronize()
    for name, mask, g in got:
        assert g.dtype == torch.int32 and tuple(g.shape) == (1, 1) + mask.shape
        assert np.array_equal(g[0, 0].cpu().numpy(), _want(pp, name, mask, connectivity)), (name, connectivity)


def test_label_batches_storage_level_and_out():
    _, ops, pp = _mods()
    shape = (33, 17, 70)
    named = dict(C.masks(shape))
    four = [named[k] for k in ("random30", "serpentine", "corner_pair", "random60")]      # four different volumes: a volume index bug shows
    batch = np.stack(four).reshape((2, 2) + shape)
    want = np.stack([pp.label_numpy(m, 18) for m in four]).reshape(batch.shape)
    assert np.array_equal(ops.cc_label(torch.from_numpy(batch).cuda(), connectivity=18).cpu().numpy(), want)      # bool storage
    u8 = torch.from_numpy(batch.astype(np.uint8) * 9).cuda()
    out = torch.full(batch.shape, -7, dtype=torch.int32, device="cuda")
    assert ops.cc_label(u8, 0, 18, out=out) is out and np.array_equal(out.cpu().numpy(), want)                    # uint8 storage, out=
    noise = np.random.default_rng(3).integers(0, 256, (1, 2) + shape).astype(np.uint8)
    for level in (0, 127):
        got = ops.cc_label(torch.from_numpy(noise).cuda(), level, 26).cpu().numpy()
        for c in range(2):
            assert np.array_equal(got[0, c], pp.label_numpy(noise[0, c] > level, 26)), (level, c)


def test_sizes_and_filter():
    _, ops, pp = _mods()
    shape = (33, 17, 70)
    rng = np.random.default_rng(8)
    vols = [np.where(rng.random(shape) < p, rng.integers(128, 256, shape), rng.integers(0, 128, shape)).astype(np.uint8) for p in (0.2, 0.45)]
    vols.append(np.where(C.serpentine(shape), 255, 0).astype(np.uint8))      # one component of whole rows: the run aggregation
    vols.append(np.full(shape, 200, np.uint8))
    batch = np.stack(vols).reshape((2, 2) + shape)
    v = torch.from_numpy(batch).cuda()
    labels = ops.cc_label(v, 127, 6)
    sizes = torch.full((2, 2, batch[0, 0].size), -3, dtype=torch.int32, device="cuda")
    assert ops.cc_sizes(labels, out=sizes) is sizes      # zeroes it itself
    want_sizes = [pp.component_sizes_numpy(pp.label_numpy(x > 127, 6)) for x in vols]
    assert np.array_equal(sizes.cpu().numpy().reshape(4, -1), np.stack(want_sizes))
    s0 = want_sizes[0]
    cut = int(np.sort(s0[s0 > 0])[-3])      # exactly a component's size: kept; one more: dropped
    for mv in (1, cut, cut + 1):
        want = np.stack([pp.filter_numpy(x, 127, 6, mv)[0] for x in vols]).reshape(batch.shape)
        assert np.array_equal(ops.cc_filter(v, labels, sizes, mv).cpu().numpy(), want), mv
    kept_at = [(pp.filter_numpy(vols[0], 127, 6, mv)[0] > 0).sum() for mv in (cut, cut + 1)]
    assert kept_at[0] - kept_at[1] >= cut      # the component of exactly `cut` voxels went
    inplace = v.clone()
    assert ops.cc_filter(inplace, labels, sizes, cut, out=inplace) is inplace
    assert np.array_equal(inplace.cpu().numpy(), np.stack([pp.filter_numpy(x, 127, 6, cut)[0] for x in vols]).reshape(batch.shape))
    odd = v.reshape(-1)[1:1 + 4 * 1000 + 3]      # a base that is not 4-byte aligned and a length that is no multiple of 4: the scalar path
    lab = labels.reshape(-1)[1:1 + 4003].clone().clamp(max=4003)
    sz = torch.randint(0, 3, (4003,), dtype=torch.int32, device="cuda")
    got = ops.cc_filter(odd.reshape(1, 1, 1, 1, -1), lab.reshape(1, 1, 1, 1, -1), sz.reshape(1, 1, -1), 2).cpu().numpy().reshape(-1)
    ln, sn, on = lab.cpu().numpy(), sz.cpu().numpy(), odd.cpu().numpy()
    assert np.array_equal(got, np.where((ln > 0) & (sn[np.maximum(ln, 1) - 1] >= 2), on, 0))


def test_two_runs_are_identical():
    _, ops, _ = _mods()
    mask = torch.from_numpy(dict(C.masks((40, 40, 130)))["random30"]).cuda()[None, None]
    a, b = ops.cc_label(mask, connectivity=26), ops.cc_label(mask, connectivity=26)
    assert torch.equal(a, b)


def test_refusals():
    L, ops, _ = _mods()
    v = torch.zeros((1, 1, 4, 5, 6), dtype=torch.uint8, device="cuda")
    for bad in (v.cpu(), v.float(), v[0]):
        with pytest.raises(L.RxError):
            ops.cc_label(bad)
    with pytest.raises(L.RxError, match="connectivity"):
        ops.cc_label(v, connectivity=8)
    with pytest.raises(L.RxError, match="level"):
        ops.cc_label(v, level=255)
    labels = ops.cc_label(v)
    for bad in (labels.cpu(), labels.float(), labels[0]):
        with pytest.raises(L.RxError):
            ops.cc_sizes(bad)
    sizes = ops.cc_sizes(labels)
    with pytest.raises(L.RxError, match="min_voxels"):
        ops.cc_filter(v, labels, sizes, 0)
    with pytest.raises(L.RxError, match="sizes"):
        ops.cc_filter(v, labels, sizes[..., :-1], 1)
    with pytest.raises(L.RxError, match="labels"):
        ops.cc_filter(v, labels.float(), sizes, 1)
    # the library's own limits, refused with a status before any launch (no device memory is touched: the pointers are never read)
    so, p = L.load(), v.data_ptr()
    from ctypes import c_void_p
    for args in ((2, 1, 1 << 11, 1 << 10, 1 << 10), (1, 1, 0, 4, 4)):      # 2^31 voxels; an extent of 0
        level, n, z, y, x = args
        assert so.rx_cc_label(c_void_p(p), level, n, z, y, x, 26, c_void_p(labels.data_ptr()), None) != 0
    assert so.rx_cc_label(c_void_p(p), 0, 1, 4, 5, 6, 8, c_void_p(labels.data_ptr()), None) != 0 and b"connectivity" in so.rx_last_error()


def _store(tmp_path, name, values):
    from mt3d_amd.dataloading import zarr_lite
    store = tmp_path / name
    os.makedirs(store)
    zarr_lite.write_array(str(store / "sheet_final"), values, (8, 16, 16), compressor="zlib")
    return str(store)


def test_component_filter_resident_and_in_slabs(tmp_path):
    _, _, pp = _mods()
    from mt3d_amd.dataloading import zarr_lite
    shape = (20, 24, 40)
    values = C.sheet_values(shape)
    want, labels = pp.filter_numpy(values, 127, 26, 40)
    sizes = pp.component_sizes_numpy(labels)
    kept = np.nonzero(sizes >= 40)[0]
    table = np.zeros(sizes.size + 1, np.uint32)
    table[kept + 1] = np.arange(1, kept.size + 1)
    runs = {}
    for name, kw in (("resident", dict(slab=None)), ("slabs", dict(slab=7)), ("budget", dict(max_device_bytes=9 * values.size - 1))):
        store = _store(tmp_path, name, values)
        f = pp.ComponentFilter(127, 26, 40, write_labels=True, **kw)
        summary = f.run(store, "sheet")
        runs[name] = (summary, f.last_slab)
        assert np.array_equal(zarr_lite.open(os.path.join(store, "sheet_filtered"))[...], want), name
        assert np.array_equal(zarr_lite.open(os.path.join(store, "sheet_labels"))[...], table[labels]), name
        assert json.load(open(os.path.join(store, "sheet_filtered", ".zattrs"))) == summary
    assert runs["resident"][1] == 20 and runs["slabs"][1] == 7 and runs["budget"][1] == 19      # one slab, four, two
    assert runs["resident"][0] == runs["slabs"][0] == runs["budget"][0]
    assert runs["resident"][0]["kept"] == kept.size and runs["resident"][0]["components"] == int((sizes > 0).sum())


def test_component_filter_stays_within_nine_bytes_per_slab_voxel(tmp_path):
    """the three slab buffers are allocated once (9 B per voxel of a slab) and everything else -- table compaction, the scatter of
    global sizes, the compact-id gather of `write_labels` -- works on SCRATCH_ELEMENTS at a time: at most 32 MiB on the side.  The
    slab here holds more voxels than one such piece, so the piecewise paths run, and two slabs, so buffers are reused."""
    _, _, pp = _mods()
    from mt3d_amd.dataloading import zarr_lite
    from mt3d_amd.postprocess import components as M
    shape, slab = (48, 256, 256), 24
    assert slab * shape[1] * shape[2] > M.SCRATCH_ELEMENTS
    values = C.sheet_values(shape)
    store = tmp_path / "big"
    os.makedirs(store)
    zarr_lite.write_array(str(store / "sheet_final"), values, (24, 128, 128))
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    pp.ComponentFilter(127, 26, 40, write_labels=True, slab=slab).run(str(store), "sheet")
    peak = torch.cuda.max_memory_allocated() - before
    print("peak bytes", peak, "slab bytes", M.BYTES_PER_VOXEL * slab * shape[1] * shape[2])
    assert peak <= M.BYTES_PER_VOXEL * slab * shape[1] * shape[2] + (32 << 20)
    want, labels = pp.filter_numpy(values, 127, 26, 40)
    sizes = pp.component_sizes_numpy(labels)
    kept = np.nonzero(sizes >= 40)[0]
    table = np.zeros(sizes.size + 1, np.uint32)
    table[kept + 1] = np.arange(1, kept.size + 1)
    assert np.array_equal(zarr_lite.open(str(store / "sheet_filtered"))[...], want)
    assert np.array_equal(zarr_lite.open(str(store / "sheet_labels"))[...], table[labels])
