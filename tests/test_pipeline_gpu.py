"""GPU: every device stage of the training input side at once (`stages.DevicePipeline`), behind `DeviceFeeder` and inline as
`forward_loss` applies it to a batch the feeder did not stage: the two paths agree bit for bit, and both are the host oracles
chained in the documented order -- `ingest_numpy` -> `dilate_numpy` -> `apply_op_numpy` -> `affine_numpy` -> `elastic_numpy` ->
`apply_params_numpy` -- on the draws the stages made.  Every stage up to the deformation is compared bit for bit, as its own GPU
test compares it; the intensity stack within `test_augment_device_gpu._tolerance` of its draw (0 for the exact members)."""
import numpy as np
import pytest
import torch

import mt3d_amd  # noqa: F401
from mt3d_amd.dataloading import augment_device as A
from mt3d_amd.dataloading import dilate_device as D
from mt3d_amd.dataloading import elastic_device as M
from mt3d_amd.dataloading import geometry_device as G
from mt3d_amd.dataloading import ingest_device as I
from mt3d_amd.dataloading import spatial_device as S
from mt3d_amd.dataloading.stages import DevicePipeline

# x unequal: only the rotation about x (the plane of z and y) keeps the shape; spacing 8, the kernel's minimum: a 5 x 5 x 6 node grid
PATCH, BATCH, BATCHES = (16, 16, 24), 2, 2
RULES = {"image": "div255", "sheet": "div255", "normals": "normal_u16"}
RADIUS, SPACING, SEED = 2, 8, 11


def raw_items():
    """what a `where: device` ingest dataset hands out: uint8 image, uint8 label (a voxel in the corner: the ball clips at three
    faces), uint16 channels-last normals"""
    rng = np.random.default_rng(3)
    items = []
    for _ in range(BATCH * BATCHES):
        sheet = (rng.random(PATCH) < 0.004).astype(np.uint8) * 255
        sheet[0, 0, 0] = 255
        items.append({"image": torch.from_numpy(rng.integers(0, 256, PATCH, dtype=np.uint8)), "sheet": torch.from_numpy(sheet),
                      "normals": torch.from_numpy(rng.integers(0, 65536, PATCH + (3,), dtype=np.uint16))})
    return items


def make_pipeline():
    return DevicePipeline(
        ingest=I.DeviceIngest(RULES), dilate=D.DeviceDilate(["sheet"], RADIUS),
        geometry=G.DeviceGeometry(flip={"p": 1.0, "p_transform": 1.0}, rot90={"axes": ("x",), "p": 1.0, "p_transform": 1.0}, seed=SEED),
        spatial=S.DeviceSpatial(rotation={"axes": ("z", "y", "x"), "max_degrees": 30.0, "p": 1.0}, scale={"range": (0.8, 1.25), "p": 1.0},
                                seed=SEED),
        elastic=M.DeviceElastic(spacing=SPACING, magnitude=(0.5, 1.25), p=1.0, seed=SEED), augmenter=A.DeviceAugmenter(seed=SEED))


def draws_of(pipe):
    """the draws of the pipeline's last call, per sample: (GeomOp, AffineOp, ElasticField, AugmentParams)"""
    return list(zip(pipe.geometry.last_ops, pipe.spatial.last_ops, pipe.elastic.last_fields, pipe.augmenter.last_params))


def oracle_chain(item, draws):
    """one raw item through the numpy statement of every stage, in `DevicePipeline`'s order -> ({key: float32 (C, Z, Y, X)}, the
    image before the intensity stack)"""
    op, aff, field, params = draws
    out = {k: I.ingest_numpy(v.numpy(), RULES[k]) for k, v in item.items()}
    out["sheet"] = D.dilate_numpy(out["sheet"], RADIUS)
    out = {k: G.apply_op_numpy(op, v, k == "normals") for k, v in out.items()}
    out = S.apply_item_numpy(aff, out)
    out = M.apply_item_numpy(field, out)
    before = out["image"]
    out["image"] = A.apply_params_numpy(before, params)
    return out, before


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and bool((a.view(np.int32) == b.view(np.int32)).all())


@pytest.mark.gpu
def test_feeder_and_inline_paths_agree_and_are_the_chained_oracles():
    from torch.utils.data import DataLoader
    from test_augment_device_gpu import _tolerance
    from mt3d_amd.train import DeviceFeeder, PinnedRingCollate
    items = raw_items()
    device = torch.device("cuda", torch.cuda.current_device())
    behind, inline = make_pipeline(), make_pipeline()
    fed, fed_draws = [], []
    for batch in DeviceFeeder(DataLoader(items, batch_size=BATCH, shuffle=False, collate_fn=PinnedRingCollate()), device, behind):
        torch.cuda.synchronize()
        fed.append({k: v.cpu().numpy() for k, v in batch.items()})
        fed_draws.append(draws_of(behind))          # (the feeder stages the next batch only when it is asked for it)
    moved = {"geometry": 0, "spatial": 0}
    assert len(fed) == BATCHES
    for b, host in enumerate(DataLoader(items, batch_size=BATCH, shuffle=False)):
        assert host["image"].dtype == torch.uint8 and host["normals"].dtype == torch.uint16 and not host["image"].is_cuda
        dev = inline.to_device(host, device)          # as `forward_loss` does for a batch the feeder did not stage
        assert dev["image"].dtype == torch.uint8 and dev["normals"].shape == (BATCH,) + PATCH + (3,)
        got = inline(dev)
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in got.items()}
        draws = draws_of(inline)
        assert [d[:3] for d in draws] == [d[:3] for d in fed_draws[b]]          # identically seeded: the same draws ...
        assert set(got) == set(fed[b]) == set(RULES)
        for k in RULES:
            assert got[k].shape == (BATCH, 3 if k == "normals" else 1) + PATCH and same_bits(got[k], fed[b][k]), (b, k)      # ... and bits
        for j, d in enumerate(draws):
            moved["geometry"] += not d[0].is_identity()
            moved["spatial"] += not d[1].is_identity()
            assert d[0].preserves(PATCH) and not d[2].is_identity()
            want, before = oracle_chain(items[BATCH * b + j], d)
            assert 0 < want["sheet"].sum() < want["sheet"].size and set(np.unique(want["sheet"])) <= {0.0, 1.0}
            assert np.count_nonzero(want["normals"]) > 0 and 0 < np.count_nonzero(before) < before.size
            for k in ("sheet", "normals"):
                assert same_bits(got[k][j], want[k]), (b, j, k)
            tol = _tolerance(d[3])
            err = np.abs(got["image"][j].astype(np.float64) - want["image"]).max()
            print(f"batch {b} sample {j}: image max err {err:.3e} (allowed {tol:.3e})")
            assert err <= tol, (b, j, err, tol)
    assert moved["geometry"] > 0 and moved["spatial"] > 0          # not a comparison of untouched batches
