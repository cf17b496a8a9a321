"""The augmentation stack of `augment.py` with the voxels touched ON THE DEVICE (`dataset_config.augment: "device"`).

Parameters are drawn on the host, per patch, by `draw_params`: it walks the stack exactly as `augment.augment_image` does and makes
the same generator calls in the same order, with one exception -- where `gauss_noise` draws a patch-sized `rng.normal`, it draws
one 64-bit key for the device's counter-based generator (Philox4x32-10 + Box-Muller, a pure function of (key, voxel)).  What the
kernels then compute (csrc/rx_augment.hip: rx_aug_pointwise, rx_aug_filter_zy) is stated in numpy by `apply_params_numpy`, built
from `augment.py`'s own pieces; it is the oracle of the GPU tests and the CPU side of scripts/bench_augment.py.  For every draw
that does not select GaussNoise, `apply_params_numpy(x, draw_params(rng))` equals `augment_image(x, rng)` bit for bit
(tests/test_augment_device_cpu.py), so the device stack inherits exactly the standing of the restatement (parity with
albumentations unpinned, see `augment.py`).

`DeviceAugmenter` draws one parameter set per item of a batch, packs them into the table the C ABI takes and launches the kernels
on the current stream.  Targets are never touched."""
from dataclasses import dataclass, field

import numpy as np
import torch

from . import augment as A

PW_NONE, PW_AFFINE, PW_PLANE, PW_NOISE = 0, 1, 2, 3
G3_NONE, G3_FILTER, G3_DOWNSCALE = 0, 1, 2
MAX_K, MAX_BOXES = 21, 4

# mirror of `rx_aug_sample` (include/rxunet.h), 160 bytes
SAMPLE_DTYPE = np.dtype([("pw_mode", "<i4", (2,)), ("pw_a", "<f4", (2,)), ("pw_b", "<f4", (2,)), ("pw_off", "<i4", (2,)),
                         ("key_lo", "<u4"), ("key_hi", "<u4"), ("g3_mode", "<i4"), ("k", "<i4"), ("g3_off", "<i4"),
                         ("nbox", "<i4"), ("box", "<i4", (MAX_BOXES, 6)), ("fill", "<f4"), ("pad_", "<i4")])
assert SAMPLE_DTYPE.itemsize == 160


@dataclass
class AugmentParams:
    """one patch's draw.  `g1` / `g2`: None, ("affine", F, b) with F an fp32 scalar or a (Z, Y) fp32 plane -> clip(img * F + b),
    or ("noise", sigma, key) -> clip(img + sigma * n(key, voxel)).  `g3`: None, ("filter", (k, k) fp32 kernel) or
    ("downscale", z source rows, y source columns).  `boxes`: (z0, y0, x0, d, h, w), filled with `fill`."""
    g1: tuple = None
    g2: tuple = None
    g3: tuple = None
    boxes: list = field(default_factory=list)
    fill: float = 0.5

    def identity(self):
        return self.g1 is None and self.g2 is None and self.g3 is None and not self.boxes


def _illumination_factor(rng, h, w):
    """the (Z, Y) factor of `augment.illumination`: the same draws and the same statements"""
    intensity = rng.uniform(0.01, 0.2) * (1.0 if rng.random() < 0.5 else -1.0)
    ang = np.deg2rad(rng.uniform(0.0, 360.0))
    yy, xx = np.meshgrid(np.linspace(0.0, 1.0, h), np.linspace(0.0, 1.0, w), indexing="ij")
    g = xx * np.cos(ang) + yy * np.sin(ang)
    g = (g - g.min()) / max(g.max() - g.min(), 1e-12)
    return (1.0 + intensity * g).astype(np.float32)


def _downscale_tables(h, w):
    """`augment.downscale`'s index arithmetic, composed: output row z reads source row down_r[up_r[z]]"""
    hs, ws = max(1, int(round(h * 0.25))), max(1, int(round(w * 0.25)))
    down_r = np.minimum((np.arange(hs) * (h / hs)).astype(np.int64), h - 1)
    down_c = np.minimum((np.arange(ws) * (w / ws)).astype(np.int64), w - 1)
    up_r = np.minimum((np.arange(h) * (hs / h)).astype(np.int64), hs - 1)
    up_c = np.minimum((np.arange(w) * (ws / w)).astype(np.int64), ws - 1)
    return down_r[up_r].astype(np.int32), down_c[up_c].astype(np.int32)


def _draw_boxes(rng, shape, num_holes_range=(1, 4), depth_range=(0.1, 0.4), height_range=(0.1, 0.4), width_range=(0.1, 0.4)):
    """the draws of `augment.coarse_dropout_3d` with its default arguments"""
    D, H, W = shape
    boxes = []
    for _ in range(int(rng.integers(num_holes_range[0], num_holes_range[1] + 1))):
        d = max(1, int(D * rng.uniform(*depth_range)))
        h = max(1, int(H * rng.uniform(*height_range)))
        w = max(1, int(W * rng.uniform(*width_range)))
        z0, y0, x0 = (int(rng.integers(0, D - d + 1)), int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1)))
        boxes.append((z0, y0, x0, d, h, w))
    return boxes


def draw_params(rng, patch_shape):
    """the parameters of one patch (Z, Y, X) -- a leading channel axis is ignored: one draw per patch, every channel alike"""
    Z, Y, X = (int(v) for v in tuple(patch_shape)[-3:])
    p = AugmentParams()
    (p1, m1), (p2, m2), (p3, m3) = A.GROUPS
    if rng.random() < p1:
        if int(rng.integers(len(m1))) == 0:                  # random_brightness_contrast
            alpha = 1.0 + rng.uniform(-0.2, 0.2)
            beta = rng.uniform(-0.2, 0.2)
            p.g1 = ("affine", np.float32(alpha), np.float32(beta))
        else:                                                # illumination
            p.g1 = ("affine", _illumination_factor(rng, Z, Y), np.float32(0.0))
    if rng.random() < p2:
        if int(rng.integers(len(m2))) == 0:                  # multiplicative_noise
            p.g2 = ("affine", np.float32(rng.uniform(0.9, 1.1)), np.float32(0.0))
        else:                                                # gauss_noise: sigma, then a key instead of rng.normal(size=...)
            sigma = rng.uniform(0.2, 0.44)
            p.g2 = ("noise", np.float32(sigma), int(rng.integers(0, 2 ** 64, dtype=np.uint64)))
    if rng.random() < p3:
        which = int(rng.integers(len(m3)))
        if which == 2:
            p.g3 = ("downscale", *_downscale_tables(Z, Y))
        else:
            kern = (A.motion_blur_kernel, A.defocus_kernel, None, A.advanced_blur_kernel)[which](rng)
            p.g3 = ("filter", np.ascontiguousarray(kern, dtype=np.float32))
    if rng.random() < A.P_VOLUME_COMPOSE and rng.random() < A.P_COARSE_DROPOUT:
        p.boxes = _draw_boxes(rng, (Z, Y, X))
    return p


# ---- the device generator, restated -------------------------------------------------------------------------------------------
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def philox4x32_10(counter, key):
    """Philox4x32-10 for an array of 64-bit counters (counter words (lo, hi, 0, 0)) and one 64-bit key -> (n, 4) uint32"""
    ctr = np.asarray(counter, dtype=np.uint64).reshape(-1)
    mask = np.uint64(0xFFFFFFFF)
    c0, c1 = ctr & mask, ctr >> np.uint64(32)
    c2, c3 = np.zeros_like(c0), np.zeros_like(c0)
    k0, k1 = int(key) & 0xFFFFFFFF, (int(key) >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c0, np.uint64(_M1) * c2          # 32 x 32 -> 64 bit products (operands < 2^32: no overflow)
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & mask, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & mask
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=1).astype(np.uint32)


def philox_normals(key, n, dtype=np.float64):
    """the standard normals of voxels 0..n-1 of a patch, as the kernels form them: voxel i takes output i % 4 of counter i // 4;
    the top 24 bits + 1, scaled by 2^-24, are uniforms in (0, 1]; (u0, u1) and (u2, u3) are Box-Muller pairs (cos first).
    `dtype` float64: the exact-arithmetic statement the device's fp32 evaluation is held against; float32: the same operations in
    fp32 (scripts and the derivation of the tolerance)."""
    r = philox4x32_10(np.arange((n + 3) // 4, dtype=np.uint64), key)
    u = ((r >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24          # exact in fp32 as well
    u = u.astype(dtype)
    two_pi = dtype(6.28318530717958647692)
    out = np.empty((u.shape[0], 4), dtype)
    for pr in range(2):
        rad = np.sqrt(dtype(-2.0) * np.log(u[:, 2 * pr]))
        ang = two_pi * u[:, 2 * pr + 1]
        out[:, 2 * pr], out[:, 2 * pr + 1] = rad * np.cos(ang), rad * np.sin(ang)
    return out.reshape(-1)[:n]


def apply_params_numpy(img, params):
    """what the kernels compute, in numpy: (Z, Y, X) or (C, Z, Y, X) float32 in, a new float32 array out"""
    img = np.asarray(img, dtype=np.float32)
    if img.ndim == 4:
        return np.stack([apply_params_numpy(img[c], params) for c in range(img.shape[0])])
    out = img.copy()
    for st in (params.g1, params.g2):
        if st is None:
            continue
        if st[0] == "affine":
            F = st[1] if np.ndim(st[1]) == 0 else np.asarray(st[1], np.float32)[:, :, None]
            out = A._clip(out * F + np.float32(st[2]))
        else:
            n = philox_normals(st[2], out.size).reshape(out.shape)
            out = A._clip(out.astype(np.float64) + float(np.float32(st[1])) * n).astype(np.float32)
    if params.g3 is not None:
        if params.g3[0] == "filter":
            out = A._clip(A._filter_plane(out, params.g3[1]))
        else:
            out = np.ascontiguousarray(out[params.g3[1]][:, params.g3[2]])
    if params.boxes:
        out = out.copy()
        for z0, y0, x0, d, h, w in params.boxes:
            out[z0:z0 + d, y0:y0 + h, x0:x0 + w] = np.float32(params.fill)
    return np.ascontiguousarray(out, dtype=np.float32)


# ---- the table of the C ABI ----------------------------------------------------------------------------------------------------
def table_words(batch, z, y):
    """upper bound of the pool (4-byte words) of a batch: per sample a (Z, Y) plane per pointwise stage and the larger of 21 x 21
    weights / Z + Y indices, each piece rounded up to 4 words"""
    per = 2 * ((z * y + 3) // 4 * 4) + (max(MAX_K * MAX_K, z + y) + 3) // 4 * 4
    return batch * per


def pack_table(params, shape, buf=None):
    """`params` (one AugmentParams per sample) -> (table bytes as a uint8 array: len(params) records + pool, pool words used).
    `buf`: a uint8 array to fill (e.g. the numpy view of a pinned tensor) of at least 160 * B + 4 * table_words(B, Z, Y) bytes."""
    Z, Y, X = (int(v) for v in tuple(shape)[-3:])
    B = len(params)
    nbytes = SAMPLE_DTYPE.itemsize * B + 4 * table_words(B, Z, Y)
    if buf is None:
        buf = np.zeros(nbytes, np.uint8)
    rec = buf[:SAMPLE_DTYPE.itemsize * B].view(SAMPLE_DTYPE)
    rec[:] = np.zeros((), SAMPLE_DTYPE)
    pool_f = buf[SAMPLE_DTYPE.itemsize * B:nbytes].view(np.float32)
    pool_i = pool_f.view(np.int32)
    used = 0

    def put(arr, as_int=False):
        nonlocal used
        off, n = used, arr.size
        (pool_i if as_int else pool_f)[off:off + n] = arr.reshape(-1)
        used = (off + n + 3) // 4 * 4
        return off
    for i, p in enumerate(params):
        r = rec[i]
        for st, g in enumerate((p.g1, p.g2)):
            if g is None:
                continue
            if g[0] == "noise":
                r["pw_mode"][st], r["pw_a"][st] = PW_NOISE, g[1]
                r["key_lo"], r["key_hi"] = int(g[2]) & 0xFFFFFFFF, (int(g[2]) >> 32) & 0xFFFFFFFF
            elif np.ndim(g[1]) == 0:
                r["pw_mode"][st], r["pw_a"][st], r["pw_b"][st] = PW_AFFINE, g[1], g[2]
            else:
                plane = np.ascontiguousarray(g[1], np.float32)
                if plane.shape != (Z, Y):
                    raise ValueError(f"factor plane {plane.shape} for a patch of (Z, Y) = {(Z, Y)}")
                r["pw_mode"][st], r["pw_b"][st], r["pw_off"][st] = PW_PLANE, g[2], put(plane)
        if p.g3 is not None:
            if p.g3[0] == "filter":
                kern = np.ascontiguousarray(p.g3[1], np.float32)
                r["g3_mode"], r["k"] = G3_FILTER, kern.shape[0]
                if kern.ndim == 2 and kern.shape[0] == kern.shape[1] and kern.size <= MAX_K * MAX_K:
                    r["g3_off"] = put(kern)          # (anything else is refused by the library, which names the reason)
            else:
                r["g3_mode"] = G3_DOWNSCALE
                r["g3_off"] = put(np.concatenate([np.asarray(p.g3[1], np.int32), np.asarray(p.g3[2], np.int32)]), as_int=True)
        r["nbox"] = len(p.boxes)
        for j, bx in enumerate(p.boxes[:MAX_BOXES]):
            r["box"][j] = bx
        r["fill"] = p.fill
    return buf[:nbytes], used


class DeviceAugmenter:
    """`augmenter(image_batch) -> image_batch`: (B, C, Z, Y, X) fp32 on the device, augmented on the CURRENT stream.  Draws B
    parameter sets from its own generator, seeded from `torch.initial_seed()` and the rank (ranks differ, a seeded run repeats).
    The output (and the scratch batch of the out-of-place stage) comes from torch's caching allocator on the current stream, so a
    batch that a step on another stream still reads is never overwritten as long as that consumer calls `record_stream`, as
    `DeviceFeeder` does for everything it hands over.  The parameter table goes through two pinned host buffers in turn."""

    def __init__(self, seed=None, rank=0):
        seed = torch.initial_seed() if seed is None else int(seed)
        self.rng = np.random.default_rng([seed % (1 << 63), int(rank)])
        self._pinned = [None, None]
        self._events = [None, None]
        self._turn = 0
        self.last_params = None          # the draws of the last call (tests, debugging)

    def _host_table(self, nbytes):
        slot = self._turn % 2
        self._turn += 1
        if self._events[slot] is not None:
            self._events[slot].synchronize()          # the copy that read this buffer two calls ago
        t = self._pinned[slot]
        if t is None or t.numel() < nbytes:
            t = self._pinned[slot] = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        return slot, t

    def __call__(self, image, params=None):
        from ..engine import ops
        from ..engine.lib import RxError
        if not isinstance(image, torch.Tensor) or not image.is_cuda:
            raise RxError("DeviceAugmenter: the image batch must be a device tensor (the host stack is dataloading/augment.py)")
        if image.dim() != 5 or image.dtype != torch.float32:
            raise RxError(f"DeviceAugmenter: expected a float32 (B, C, Z, Y, X) batch, got {image.dtype} {tuple(image.shape)}")
        image = image.contiguous()
        B, _, Z, Y, X = image.shape
        if params is None:
            params = [draw_params(self.rng, (Z, Y, X)) for _ in range(B)]
        self.last_params = params
        nbytes = SAMPLE_DTYPE.itemsize * B + 4 * table_words(B, Z, Y)
        slot, host = self._host_table(nbytes)
        _, words = pack_table(params, (Z, Y, X), host.numpy())
        used = SAMPLE_DTYPE.itemsize * B + 4 * words
        dev = torch.empty(used, dtype=torch.uint8, device=image.device)
        dev.copy_(host[:used], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._events[slot] = ev
        return ops.augment_batch(image, host, dev, words, any(p.g3 is not None for p in params))
