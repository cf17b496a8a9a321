"""CPU: the host half of the device augmentation stack (dataloading/augment_device.py) -- parameter draws, the numpy statement of
what the kernels compute, the restated Philox4x32-10 generator, the table of the C ABI and the `augment: "device"` config value.
The kernels themselves: tests/test_augment_device_gpu.py."""
import warnings

import numpy as np
import pytest
import torch

import mt3d_amd  # noqa: F401
from mt3d_amd.dataloading import augment as A
from mt3d_amd.dataloading import augment_device as D

SHAPE = (14, 18, 10)          # small, non-cubic


def _patch(seed=99, shape=SHAPE):
    return np.random.default_rng(seed).random(shape, dtype=np.float32)


def _is_noise(p):
    return p.g2 is not None and p.g2[0] == "noise"


def test_draw_order_matches_the_host_stack_bit_for_bit():
    """seeds 0..199: draw_params + apply_params_numpy == augment_image, bit for bit, for every seed whose draw does not select
    GaussNoise (after its `rng.normal(size=...)` the two generator streams legitimately diverge).  Those seeds (expected
    0.35 / 2 = 17.5 %; 31 of these 200) may be at most 30 %, and must still agree through group 1."""
    x = _patch()
    left_out = 0
    for s in range(200):
        p = D.draw_params(np.random.default_rng(s), x.shape)
        if _is_noise(p):
            left_out += 1
            rng = np.random.default_rng(s)          # the host stack up to and including group 1
            want = x.copy()
            prob, members = A.GROUPS[0]
            if rng.random() < prob:
                want = members[int(rng.integers(len(members)))](want, rng)
            assert np.array_equal(D.apply_params_numpy(x, D.AugmentParams(g1=p.g1)), want), s
            continue
        got, want = D.apply_params_numpy(x, p), A.augment_image(x, np.random.default_rng(s))
        assert got.dtype == np.float32 and np.array_equal(got, want), (s, p)
    assert 0 < left_out <= 60


def test_multi_channel_patch_is_one_draw_and_leaves_the_generator_where_the_host_stack_does():
    x = np.stack([_patch(1), _patch(2)])
    for s in range(40):
        r1, r2 = np.random.default_rng(s), np.random.default_rng(s)
        p = D.draw_params(r1, x.shape)
        if _is_noise(p):
            continue
        assert np.array_equal(D.apply_params_numpy(x, p), A.augment_image(x, r2))
        assert r1.random() == r2.random()


# Philox4x32-10 known answers: produced once by running the host-compilable engine that ships with torch
# (torch/include/ATen/core/PhiloxRNGEngine.h, at::philox_engine(seed = key, subsequence = 0, offset = counter), four outputs);
# the first row is also the counter 0 / key 0 vector of Random123's kat_vectors.
KAT = [
    (0x0, 0x0, (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    (0x0, 0x1, (0xf8e4cca4, 0x5cb200db, 0xb1a574eb, 0x097eff67)),
    (0x0, 0x100000000, (0x6ad0c5ec, 0xea236249, 0x73a459f5, 0x074944b3)),
    (0x0123456789abcdef, 0x0, (0xb850222e, 0xc58cb04b, 0x14a7a020, 0x7a84fff9)),
    (0x0123456789abcdef, 0x75bcd15, (0xec684f00, 0x53c06e7f, 0x9ee3668c, 0xdf26d1f4)),
    (0xffffffffffffffff, 0x1, (0x19fed511, 0x4b67e034, 0x9d2c02e2, 0x9fe857b4)),
    (0xffffffffffffffff, 0x100000000, (0x85af3999, 0xf0ea2a5e, 0x1c58f27c, 0x402bd930)),
    (0x2a, 0x75bcd15, (0x5f01aba0, 0xb67f0d70, 0xf25e8d57, 0xfda7c468)),
]


def test_philox_restatement_reproduces_known_answers():
    for key, ctr, want in KAT:
        assert tuple(int(v) for v in D.philox4x32_10([ctr], key)[0]) == want, (hex(key), hex(ctr))
    many = D.philox4x32_10([c for _, c, _ in KAT], 0x2a)          # vectorised over counters
    assert tuple(int(v) for v in many[-1]) == KAT[-1][2]


def test_noise_statistics_of_the_restatement():
    """2 M samples of a unit normal: |mean| <= 5 / sqrt(N) and |std - 1| <= 5 / sqrt(2 N) (five standard errors of either
    estimate) -- a wrong uniform -> normal mapping cannot pass; all four outputs of a counter are used and are uncorrelated"""
    N = 2_000_000
    n = D.philox_normals(0x5eed5eed5eed, N)
    assert n.shape == (N,) and np.isfinite(n).all()
    assert abs(n.mean()) <= 5.0 / np.sqrt(N) and abs(n.std() - 1.0) <= 5.0 / np.sqrt(2 * N)
    assert np.abs(n).max() <= np.sqrt(2 * 24 * np.log(2.0)) + 1e-9          # 24-bit uniforms in (0, 1]
    q = n.reshape(-1, 4)
    for a in range(4):
        for b in range(a + 1, 4):
            assert abs(np.mean(q[:, a] * q[:, b])) <= 5.0 / np.sqrt(N / 4)
    assert not np.array_equal(n[:1000], D.philox_normals(0x5eed5eed5eee, 1000))
    # the noise reaches an image as clip(img + sigma * n)
    x = np.full((20, 20, 20), 0.5, np.float32)
    out = D.apply_params_numpy(x, D.AugmentParams(g2=("noise", np.float32(0.3), 7)))
    inner = out[(out > 0) & (out < 1)]
    assert 0.0 <= out.min() and out.max() <= 1.0 and 0.2 < inner.std() < 0.3


def test_draw_params_ranges_and_frequencies():
    N = 4000
    rng = np.random.default_rng(11)
    cnt = {"bc": 0, "illum": 0, "mult": 0, "noise": 0, "filter": 0, "down": 0, "boxes": 0, "g1": 0, "g2": 0, "g3": 0}
    Z, Y, X = 40, 50, 60
    for _ in range(N):
        p = D.draw_params(rng, (Z, Y, X))
        if p.g1 is not None:
            cnt["g1"] += 1
            kind, F, b = p.g1
            assert kind == "affine"
            if np.ndim(F) == 0:
                cnt["bc"] += 1
                assert 0.8 - 1e-6 <= F <= 1.2 + 1e-6 and -0.2 - 1e-6 <= b <= 0.2 + 1e-6
            else:
                cnt["illum"] += 1
                assert F.shape == (Z, Y) and F.dtype == np.float32 and b == 0 and 0.8 - 1e-6 <= F.min() and F.max() <= 1.2 + 1e-6
        if p.g2 is not None:
            cnt["g2"] += 1
            if p.g2[0] == "noise":
                cnt["noise"] += 1
                assert 0.2 <= p.g2[1] <= 0.44 + 1e-6 and 0 <= p.g2[2] < 2 ** 64
            else:
                cnt["mult"] += 1
                assert 0.9 - 1e-6 <= p.g2[1] <= 1.1 + 1e-6 and p.g2[2] == 0
        if p.g3 is not None:
            cnt["g3"] += 1
            if p.g3[0] == "filter":
                cnt["filter"] += 1
                kern = p.g3[1]
                k = kern.shape[0]
                assert kern.shape == (k, k) and kern.dtype == np.float32 and k % 2 == 1
                assert k in (3, 5, 7) or 7 <= k <= 21          # the blurs; defocus: radius 3..10 -> k = 2 r + 1
                assert kern.min() >= 0 and kern.sum() == pytest.approx(1.0, abs=1e-5)
            else:
                cnt["down"] += 1
                zi, yi = p.g3[1], p.g3[2]
                assert zi.shape == (Z,) and yi.shape == (Y,) and 0 <= zi.min() and zi.max() < Z and 0 <= yi.min() and yi.max() < Y
        if p.boxes:
            cnt["boxes"] += 1
            assert 1 <= len(p.boxes) <= 4 and p.fill == 0.5
            for z0, y0, x0, d, h, w in p.boxes:
                assert z0 >= 0 and y0 >= 0 and x0 >= 0 and z0 + d <= Z and y0 + h <= Y and x0 + w <= X
                assert int(Z * 0.1) <= d <= int(Z * 0.4) and int(Y * 0.1) <= h <= int(Y * 0.4) and int(X * 0.1) <= w <= int(X * 0.4)
    for key, want in (("g1", 0.30), ("g2", 0.35), ("g3", 0.40), ("bc", 0.15), ("illum", 0.15), ("mult", 0.175), ("noise", 0.175),
                      ("filter", 0.30), ("down", 0.10), ("boxes", 0.25)):
        assert abs(cnt[key] / N - want) < 0.03, (key, cnt)
    ks = set()
    for s in range(300):
        r = np.random.default_rng(s)
        ks.add(A.defocus_kernel(r).shape[0])
        assert A.motion_blur_kernel(r).shape[0] in (3, 5, 7) and A.advanced_blur_kernel(r).shape[0] in (3, 5, 7)
    assert ks == {7, 9, 11, 13, 15, 17, 19, 21}


def test_table_layout_matches_the_c_struct():
    p = [D.AugmentParams(g1=("affine", np.full((6, 5), 1.5, np.float32), np.float32(0.25)), g2=("noise", np.float32(0.3), (7 << 32) | 9),
                         g3=("filter", np.arange(9, dtype=np.float32).reshape(3, 3)), boxes=[(1, 2, 3, 2, 2, 2)]),
         D.AugmentParams(g2=("affine", np.float32(1.1), np.float32(0.0)), g3=("downscale", np.arange(6), np.arange(5))),
         D.AugmentParams()]
    buf, words = D.pack_table(p, (6, 5, 8))
    rec = buf[:3 * 160].view(D.SAMPLE_DTYPE)
    pool = buf[3 * 160:].view(np.float32)
    assert words % 4 == 0 and 0 < words <= D.table_words(3, 6, 5)
    assert list(rec["pw_mode"][0]) == [D.PW_PLANE, D.PW_NOISE] and rec["key_lo"][0] == 9 and rec["key_hi"][0] == 7
    assert np.all(pool[rec["pw_off"][0][0]:][:30] == 1.5) and rec["pw_b"][0][0] == 0.25 and rec["pw_a"][0][1] == np.float32(0.3)
    assert rec["g3_mode"][0] == D.G3_FILTER and rec["k"][0] == 3 and np.array_equal(pool[rec["g3_off"][0]:][:9], np.arange(9))
    assert rec["nbox"][0] == 1 and list(rec["box"][0][0]) == [1, 2, 3, 2, 2, 2] and rec["fill"][0] == 0.5
    assert rec["g3_mode"][1] == D.G3_DOWNSCALE
    assert list(pool.view(np.int32)[rec["g3_off"][1]:][:11]) == [0, 1, 2, 3, 4, 5, 0, 1, 2, 3, 4]
    assert list(rec["pw_mode"][2]) == [0, 0] and rec["g3_mode"][2] == 0 and rec["nbox"][2] == 0 and p[2].identity()


def test_cpu_tensors_are_refused():
    from mt3d_amd.engine.lib import RxError
    with pytest.raises(RxError):
        D.DeviceAugmenter(seed=1)(torch.zeros(1, 1, 4, 4, 4))


def test_config_value_device_gives_raw_items_without_a_warning(tmp_path):
    from types import SimpleNamespace
    from mt3d_amd.dataloading import zarr_lite
    from mt3d_amd.dataloading.dataset import ZarrSegmentationDataset3D
    rng = np.random.default_rng(1)
    img = rng.integers(0, 255, size=(32, 32, 32), dtype=np.uint8)
    lab = (rng.random((32, 32, 32)) > 0.5).astype(np.uint8) * 255
    paths = {}
    for name, arr in (("img", img), ("sheet", lab)):
        paths[name] = str(tmp_path / f"{name}.zarr")
        zarr_lite.write_array(paths[name], arr, (16, 16, 16), compressor="zlib")
    mgr = SimpleNamespace(model_name="m", tasks={"sheet": {"channels": 1}}, train_patch_size=(16, 16, 16), min_labeled_ratio=0.1,
                          min_bbox_percent=0.5, dilate_label=False, use_cache=False, cache_folder=str(tmp_path),
                          volume_paths=[{"input": paths["img"], "sheet": paths["sheet"], "ref_label": "sheet"}],
                          dataset_config={"augment": "device"})
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        dev = ZarrSegmentationDataset3D(mgr)
    assert dev.device_augment is True and dev.augment is False
    mgr.dataset_config = {"augment": False}
    raw = ZarrSegmentationDataset3D(mgr)
    assert raw.device_augment is False and raw.augment is False
    assert len(dev) == len(raw) > 0
    for i in range(len(dev)):
        a, r = dev[i], raw[i]
        assert torch.equal(a["image"], r["image"]) and torch.equal(a["sheet"], r["sheet"])
    for mode, aug in (("restated", True), ("true", True), ("false", False), (True, True)):
        mgr.dataset_config = {"augment": mode}
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ds = ZarrSegmentationDataset3D(mgr)
        assert ds.augment is aug and ds.device_augment is False
    mgr.dataset_config = {"augment": "sometimes"}
    with pytest.raises(ValueError):
        ZarrSegmentationDataset3D(mgr)
