"""Streaming sliding-window inference, CPU side: the Gaussian importance map against maps the reference's own
`compute_gaussian_3d` produced (tests/golden/gaussian_maps.npz, scripts/make_gaussian_fixture.py), the chunked zarr writer, the
pure streaming schedule, and the new config keys / command-line refusals."""
import itertools
import os

import numpy as np
import pytest

import mt3d_amd  # noqa: F401
from mt3d_amd import inference as inf
from mt3d_amd.dataloading import zarr_lite

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gaussian_map_matches_the_reference_bit_for_bit():
    """bit-exact: the restatement performs the reference's float operations in the same order (see the docstring)"""
    fx = np.load(os.path.join(ROOT, "tests", "golden", "gaussian_maps.npz"))
    assert len(fx.files) >= 5
    for key in fx.files:
        tile = tuple(int(v) for v in key.split("x"))
        got = inf.gaussian_importance_map(tile)
        want = fx[key]
        assert got.dtype == np.float32 and got.shape == want.shape == tile, key
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), key
        assert got.max() == 1.0 and got.min() > 0


@pytest.mark.parametrize("sep,comp", list(itertools.product([".", "/"], [None, "zlib"])))
def test_chunked_writer_round_trip(tmp_path, sep, comp):
    rng = np.random.default_rng(7)
    Z, Y, X = 37, 20, 18
    vol3 = rng.integers(0, 255, size=(Z, Y, X), dtype=np.uint8)
    vol3[16:32] = 0                                    # an all-fill chunk row: skipped on disk, read back as fill
    vol4 = rng.normal(size=(3, Z, Y, X)).astype(np.float32)
    w3 = zarr_lite.ChunkedWriter(tmp_path / "a3", (Z, Y, X), (16, 8, 8), np.uint8, comp, dimension_separator=sep)
    w4 = zarr_lite.ChunkedWriter(tmp_path / "a4", (3, Z, Y, X), (3, 16, 8, 8), np.float32, comp, dimension_separator=sep)
    for z0, z1 in ((0, 16), (16, 32), (32, 37)):       # the last block is a partial edge chunk row
        assert w3.write_rows(z0, vol3[z0:z1]) == []
        w4.write_rows(z0, vol4[:, z0:z1])
    a3, a4 = zarr_lite.open(str(tmp_path / "a3")), zarr_lite.open(str(tmp_path / "a4"))
    assert a3.shape == (Z, Y, X) and a3.chunks == (16, 8, 8) and a3.dtype == np.uint8
    assert np.array_equal(a3[:, :, :], vol3) and np.array_equal(a4[...], vol4)
    assert np.array_equal(a4[1, 30:37, 3:19, 17], vol4[1, 30:37, 3:19, 17])
    name = sep.join(["2", "2", "2"])
    assert os.path.exists(os.path.join(str(tmp_path / "a3"), *name.split("/")))   # edge chunk stored (at full size: _chunk checks)
    with pytest.raises(FileExistsError):
        zarr_lite.ChunkedWriter(tmp_path / "a3", (Z, Y, X), (16, 8, 8), np.uint8, comp)
    w5 = zarr_lite.ChunkedWriter(tmp_path / "a5", (Z, Y, X), (16, 8, 8), np.uint8, comp)
    with pytest.raises(zarr_lite.ZarrLiteError):
        w5.write_rows(8, vol3[8:24])                   # not on a chunk boundary
    with pytest.raises(zarr_lite.ZarrLiteError):
        w5.write_rows(0, vol3[0:10])                   # not whole chunk rows
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(4) as pool:
        futs = w5.write_rows(0, vol3[0:32], pool) + w5.write_rows(32, vol3[32:], pool)
        for f in futs:
            f.result()
    assert np.array_equal(zarr_lite.open(str(tmp_path / "a5"))[...], vol3)


CASES = [((40, 36, 44), (16, 16, 16), 0.5, 2), ((37, 20, 24), (16, 8, 8), 0.25, 3), ((16, 16, 16), (16, 16, 16), 0.5, 2),
         ((100, 24, 24), (32, 16, 16), 0.75, 4), ((65, 17, 19), (8, 8, 8), 0.0, 1), ((129, 16, 16), (64, 16, 16), 0.5, 2)]


@pytest.mark.parametrize("shape,patch,overlap,bs", CASES)
def test_schedule_invariants(shape, patch, overlap, bs):
    Z = shape[0]
    pz = patch[0]
    s = inf.stream_schedule(shape, patch, overlap, bs)
    pos = inf.all_positions(shape, patch, overlap)
    assert s["positions"] == pos and s["ring"] == pz
    # every position runs exactly once, in the order of all_positions; padding repeats a patch and is not counted
    ran = [p for st in s["steps"] for chunk, valid in st["batches"] for p in chunk[:valid]]
    assert ran == pos
    for st in s["steps"]:
        for chunk, valid in st["batches"]:
            assert len(chunk) == s["batch"] and 1 <= valid <= s["batch"]
            assert all(p == chunk[valid - 1] for p in chunk[valid:])
            assert all(p[0] == st["z"] for p in chunk)
    # loads: contiguous, new rows only, each step's patches inside the rows loaded so far, ring never overrun
    loaded = 0
    for st in s["steps"]:
        lo, hi = st["load"]
        assert lo == loaded and hi == st["z"] + pz and hi - st["z"] <= s["ring"]
        loaded = hi
    assert loaded == Z
    # finalize ranges partition [0, Z) in order, and a row is finalized only when no later patch touches it
    fins = [st["finalize"] for st in s["steps"]]
    assert fins[0][0] == 0 and fins[-1][1] == Z and all(a[1] == b[0] for a, b in zip(fins, fins[1:]))
    for k, st in enumerate(s["steps"]):
        later = [p[0] for nxt in s["steps"][k + 1:] for chunk, v in nxt["batches"] for p in chunk[:v]]
        assert all(z >= st["finalize"][1] for z in later)
        assert st["finalize"][0] >= st["z"] or k == 0          # live rows of step k fit the ring: [z_k, z_k + pz)
    # chunk rows: each written once, only when all its rows are finalized, in order, covering [0, Z)
    writes = [st["write"] for st in s["steps"] if st["write"][1] > st["write"][0]]
    assert writes[0][0] == 0 and writes[-1][1] == Z and all(a[1] == b[0] for a, b in zip(writes, writes[1:]))
    for st in s["steps"]:
        lo, hi = st["write"]
        if hi > lo:
            assert lo % pz == 0 and (hi % pz == 0 or hi == Z) and hi <= st["finalize"][1]
    assert s["max_finalize_rows"] <= pz


def test_schedule_device_bytes_do_not_grow_with_z():
    base = inf.stream_schedule((64, 96, 80), (32, 32, 32), 0.5, 2, cin=1, in_itemsize=1, acc_channels=4, out_bytes_per_voxel=30)
    for Z in (65, 200, 1000, 4096):
        s = inf.stream_schedule((Z, 96, 80), (32, 32, 32), 0.5, 2, cin=1, in_itemsize=1, acc_channels=4, out_bytes_per_voxel=30)
        for k in ("accumulator_bytes", "input_bytes", "staging_bytes", "patch_bytes", "device_bytes"):
            assert s[k] == base[k], (Z, k)
    assert base["accumulator_bytes"] == 32 * 96 * 80 * 4 * 5


def test_streaming_inferer_refuses_bad_options_and_an_existing_store(tmp_path):
    targets = {"sheet": {"channels": 1, "activation": "sigmoid"}}
    with pytest.raises(ValueError):
        inf.StreamingInferer(None, targets, (16, 16, 16), blend="median")
    with pytest.raises(ValueError):
        inf.StreamingInferer(None, targets, (16, 16, 16), normalization="minmax")
    os.makedirs(tmp_path / "predictions.zarr")
    with pytest.raises(FileExistsError):
        inf.StreamingInferer(None, targets, (16, 16, 16)).run(np.zeros((16, 16, 16), np.uint8), str(tmp_path))
    with pytest.raises(ValueError):
        inf.StreamingInferer(None, targets, (16, 16, 16)).run(np.zeros((16, 16, 16), np.int32), str(tmp_path / "o"))


def _cfg(tmp_path, ic):
    import yaml
    cfg = {"tr_setup": {}, "tr_config": {"patch_size": [16, 16, 16]}, "model_config": {},
           "dataset_config": {"targets": {"sheet": {"channels": 1, "activation": "sigmoid"}}}, "inference_config": ic}
    p = tmp_path / "cfg.yaml"
    p.write_text(yaml.safe_dump(cfg))
    return str(p)


def test_config_keys_and_cli_refusals(tmp_path):
    from mt3d_amd.configuration.config_manager import ConfigManager
    m = ConfigManager(_cfg(tmp_path, {}), verbose=False)
    assert (m.infer_input_path, m.infer_overlap, m.infer_blend, m.infer_normalization, m.infer_max_device_gb) == \
        (None, 0.5, "uniform", "scale", None)
    assert m.infer_targets == {"sheet": {"channels": 1, "activation": "sigmoid"}}
    m = ConfigManager(_cfg(tmp_path, {"input_path": "v.zarr", "overlap": 0.25, "blend": "Gaussian", "normalization": "zscore",
                                      "max_device_gb": 12, "targets": {"a": {"channels": 2}}}), verbose=False)
    assert (m.infer_input_path, m.infer_overlap, m.infer_blend, m.infer_normalization, m.infer_max_device_gb) == \
        ("v.zarr", 0.25, "gaussian", "zscore", 12.0)
    assert m.infer_targets == {"a": {"channels": 2}}
    m = ConfigManager(_cfg(tmp_path, {"targets": [{"ink": {"channels": 1}}, {"b": {"channels": 3}}]}), verbose=False)
    assert m.infer_targets == {"ink": {"channels": 1}, "b": {"channels": 3}}     # the reference task files' list form
    with pytest.raises(SystemExit, match="cv2"):
        inf.main(["--config_path", _cfg(tmp_path, {}), "--write_layers"])
    with pytest.raises(SystemExit, match="no input"):
        inf.main(["--config_path", _cfg(tmp_path, {})])
