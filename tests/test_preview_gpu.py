"""GPU: rx_preview_panel (csrc/rx_preview.hip) through engine.ops.preview_panel / preview_frames against the numpy statement
training.visualization.panel_numpy / minmax_numpy / frames_numpy.  Without the sigmoid every byte and every (lo, hi) is exact.

Shapes (h x w), the smallest that reach each path of the kernel, whose tile is 256 lanes x one 16-byte unit (4 fp32 or 8 16-bit
pixels): 1x1 and 3x5 (no unit at all, or one: heads and tails only), 7x9 (a few units), 33x31 = 1023 and 37x29 = 1073 (just under
and just over 256 lanes x 4), 64x65 (several tiles, a row length that is no multiple of 4).  Every shape also runs on a sample
whose base is one element past an aligned address, so that the scalar head is not empty."""
import ctypes

import numpy as np
import pytest
import torch

import mt3d_amd  # noqa: F401
from mt3d_amd.engine import lib, ops
from mt3d_amd.training import visualization as V

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1), (3, 5), (7, 9), (33, 31), (37, 29), (64, 65)]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
FILL = 0xAA


def _sample(host, dtype, offset=0):
    """a (C, Z, H, W) host float32 array -> the device tensor of `dtype`, its base `offset` elements past an aligned allocation"""
    flat = torch.empty(host.size + offset, dtype=dtype, device="cuda")
    vol = flat[offset:].view(host.shape)
    vol.copy_(torch.from_numpy(host))
    assert vol.is_contiguous() and vol.data_ptr() == flat.data_ptr() + offset * flat.element_size()
    return vol


def _draw(vol, y0=0, x0=0, z_step=1, sigmoid=False, with_minmax=True):
    """-> (panel bytes (Zk, h, w, 3), minmax, the whole frame buffer), after checking that nothing outside the panel was written"""
    c, z, h, w = vol.shape
    zk = -(-z // z_step)
    wf = x0 + w + 1
    wf += wf % 4 == 0                                   # a row stride (3 * wf) that is no multiple of 4
    frames = torch.full((zk, y0 + h + 2, wf, 3), FILL, dtype=torch.uint8, device="cuda")
    assert frames.stride(1) % 4 != 0
    mm = torch.full((3 if c == 3 else 1, zk, 2), -7.0, device="cuda") if with_minmax else None
    assert ops.preview_panel(vol, frames, y0, x0, z_step=z_step, sigmoid=sigmoid, minmax=mm) is frames
    torch.cuda.synchronize()
    full = frames.cpu().numpy()
    outside = np.ones(full.shape, bool)
    outside[:, y0:y0 + h, x0:x0 + w] = False
    assert (full[outside] == FILL).all(), "a byte outside the panel was written"
    return full[:, y0:y0 + h, x0:x0 + w], None if mm is None else mm.cpu().numpy(), full


def _check_exact(vol, **kw):
    z_step = kw.get("z_step", 1)
    got, mm, _ = _draw(vol, **kw)
    want = V.panel_numpy(vol)[::z_step]
    assert np.array_equal(got, want), f"{int((got != want).sum())} bytes differ, shape {tuple(vol.shape)} {vol.dtype} {kw}"
    if mm is not None:
        assert np.array_equal(mm, V.minmax_numpy(vol)[:, ::z_step], equal_nan=True)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_panel_is_the_statement(hw, dtype):
    rng = np.random.default_rng(100 * hw[0] + hw[1])
    for z in (1, 2, 5):
        for c in (1, 2, 3):
            host = (rng.standard_normal((c, z) + hw) * rng.uniform(0.1, 30)).astype(np.float32)
            for offset in (0, 1):
                vol = _sample(host, dtype, offset)
                for z_step in (1, 2, 3):
                    _check_exact(vol, z_step=z_step, y0=z_step - 1, x0=c - 1)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_flat_tiny_and_non_finite_slices(dtype):
    h, w = 37, 29
    rng = np.random.default_rng(7)
    host = rng.standard_normal((3, 6, h, w)).astype(np.float32)
    host[0, 0] = 0.25                                                        # constant
    host[1, 1] = rng.random((h, w)).astype(np.float32) * np.float32(5e-7)    # range 5e-7: flat
    host[1, 1, 0, 0], host[1, 1, -1, -1] = 0.0, 5e-7
    host[2, 2] = rng.random((h, w)).astype(np.float32) * np.float32(2e-6)    # range 2e-6: scaled
    host[2, 2, 0, 0], host[2, 2, -1, -1] = 0.0, 2e-6
    host[0, 3, 17, 5] = np.nan
    host[1, 4, 0, 0] = np.inf
    host[2, 5, -1, -1] = -np.inf
    host[1, 0, 36, 28] = np.nan                                              # (in a tail)
    vol = _sample(host, dtype, 1)
    want = V.panel_numpy(vol)
    if dtype == torch.float32:      # (in 16 bits the tiny ranges round to other values; the statement follows, whatever they become)
        assert (want[0, :, :, 0] == 127).all() and (want[1, :, :, 1] == 127).all() and want[2, :, :, 2].max() == 255
    for ch, s in ((0, 3), (1, 4), (2, 5), (1, 0)):
        assert (want[s, :, :, ch] == 127).all()
    _check_exact(vol)
    _check_exact(_sample(host[:1], dtype, 0))                                # the same slices of channel 0 as a grey panel


def test_extremes_in_the_first_head_element_and_the_last_tail_element():
    h, w = 7, 10
    host = np.random.default_rng(8).standard_normal((3, 2, h, w)).astype(np.float32)
    vol = _sample(host, torch.float32, 1)
    v = h * w
    for k in range(3):
        for s in range(2):
            head = (-(vol.data_ptr() + 4 * (k * 2 + s) * v) % 16) // 4
            if k == 0:
                assert head > 0 and (v - head) % 4 > 0                       # a scalar head and a scalar tail
    host[:, :, 0, 0], host[:, :, -1, -1] = -100.0, 100.0                     # the minimum first, the maximum last
    _check_exact(_sample(host, torch.float32, 1))
    host[:, :, 0, 0], host[:, :, -1, -1] = 100.0, -100.0
    _check_exact(_sample(host, torch.float32, 1))


@pytest.mark.parametrize("y0", [0, 3])
@pytest.mark.parametrize("x0", [0, 1, 5])
def test_placement(x0, y0):
    rng = np.random.default_rng(10 * x0 + y0)
    for c, hw, dtype in ((1, (9, 11), torch.float32), (3, (9, 11), torch.bfloat16), (3, (37, 29), torch.float32), (1, (33, 31), torch.float16)):
        _check_exact(_sample(rng.standard_normal((c, 2) + hw).astype(np.float32), dtype, 1), x0=x0, y0=y0, with_minmax=False)


def test_preview_frames_is_frames_numpy_and_reuses_its_buffer():
    g = torch.Generator().manual_seed(12)
    b, z, h, w = 2, 5, 10, 13
    image = torch.randn(b, 1, z, h, w, generator=g).cuda()
    targets = {"sheet": (torch.randn(b, 1, z, h, w, generator=g) > 0).float().cuda(), "normals": torch.randn(b, 3, z, h, w, generator=g).cuda()}
    preds = {"normals": torch.randn(b, 3, z, h, w, generator=g).cuda().to(torch.bfloat16), "sheet": torch.randn(b, 1, z, h, w, generator=g).cuda()}
    for every in (1, 2):
        want = V.frames_numpy(image[1].cpu(), {k: v[1].cpu() for k, v in targets.items()}, {k: v[1].cpu() for k, v in preds.items()}, every=every)
        out = ops.preview_frames(image, targets, preds, sample=1, every=every)
        assert out.dtype == torch.uint8 and tuple(out.shape) == (-(-z // every), 2 * h, 3 * w, 3)
        first = out.cpu().numpy()
        assert np.array_equal(first, want)
        assert not first[:, h:, :w].any()
        again = ops.preview_frames(image, targets, preds, sample=1, every=every, out=out)
        assert again is out and np.array_equal(again.cpu().numpy(), want)
    # a sigmoid task: the one-channel prediction only, within the cap of the sigmoid test below
    out = ops.preview_frames(image, targets, preds, sample=0, sigmoid_tasks=("sheet", "normals")).cpu().numpy()
    want = V.frames_numpy(image[0].cpu(), {k: v[0].cpu() for k, v in targets.items()}, {k: v[0].cpu() for k, v in preds.items()},
                          sigmoid_tasks=("sheet", "normals"))
    assert np.array_equal(out[:, :h], want[:, :h]) and np.array_equal(out[:, h:, :2 * w], want[:, h:, :2 * w])
    assert np.abs(out.astype(np.int32) - want.astype(np.int32)).max() <= 1


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_sigmoid_within_one_grey_level(dtype):
    """device expf is not numpy's exp: at most one grey level, on at most 1 % of the bytes, for slices that span at least 0.1 after
    the sigmoid (a rounding difference of a few ulp in v moves ((v - lo) / r) * 255 across an integer only when it lies within
    ~1e-4 of one)"""
    h, w = 37, 29
    host = (np.random.default_rng(13).standard_normal((1, 3, h, w)) * 2).astype(np.float32)
    host[0, :, 0, 0], host[0, :, -1, -1] = -2.0, 2.0
    vol = _sample(host, dtype, 1)
    s = 1.0 / (1.0 + np.exp(-vol.float().cpu().numpy().astype(np.float64))).reshape(3, -1)
    assert (s.max(1) - s.min(1)).min() >= 0.1
    got, mm, _ = _draw(vol, sigmoid=True)
    want = V.panel_numpy(vol, sigmoid=True)
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    print(f"sigmoid {dtype}: max byte difference {d.max()}, share of differing bytes {(d > 0).mean():.5f}")
    assert d.max() <= 1 and (d > 0).mean() <= 0.01
    assert np.allclose(mm, V.minmax_numpy(vol, sigmoid=True), rtol=1e-6, atol=0)


def test_argument_errors_are_refused_before_launch():
    so = lib.load()
    src_buf = torch.zeros(1 << 14, dtype=torch.float32, device="cuda")
    frames_buf = torch.full((1 << 16,), FILL, dtype=torch.uint8, device="cuda")
    mm_buf = torch.full((64,), -7.0, device="cuda")
    # every pointer sits in the middle of a buffer far larger than anything these arguments could address
    src, frames, mm = src_buf.data_ptr() + (1 << 15), frames_buf.data_ptr() + (1 << 15), mm_buf.data_ptr() + 64
    good = dict(src=src, dtype=lib.RX_F32, c=1, z=2, h=3, w=4, z_step=1, sigmoid=0, frames=frames, frame_stride=100, row_stride=20, y0=1,
                x0=1, minmax=mm)
    order = ("src", "dtype", "c", "z", "h", "w", "z_step", "sigmoid", "frames", "frame_stride", "row_stride", "y0", "x0", "minmax")

    def call(**kw):
        a = {**good, **kw}
        return so.rx_preview_panel(*[ctypes.c_void_p(a[k]) if k in ("src", "frames", "minmax") else a[k] for k in order], lib.stream_ptr())
    bad = [dict(src=0), dict(frames=0), dict(c=0), dict(c=-3), dict(z=0), dict(h=0), dict(w=0), dict(w=-1), dict(z_step=0), dict(z_step=-1),
           dict(dtype=3), dict(dtype=-1), dict(src=src + 2), dict(src=src + 1, dtype=lib.RX_BF16), dict(minmax=mm + 2), dict(y0=-1),
           dict(x0=-1), dict(row_stride=14), dict(frame_stride=79), dict(frame_stride=-100), dict(row_stride=-20)]
    for kw in bad:
        assert call(**kw) == -1, kw                                          # RX_EINVAL
        assert b"rx_preview_panel" in so.rx_last_error()
    torch.cuda.synchronize()
    assert (frames_buf == FILL).all() and (mm_buf == -7.0).all()             # nothing ran
    assert call() == 0 and call(row_stride=15, frame_stride=60, minmax=0) == 0      # the limits themselves are fine
    torch.cuda.synchronize()
    assert int((frames_buf != FILL).sum()) > 0


def test_wrappers_refuse_what_the_kernel_does_not_take():
    vol = torch.zeros(1, 2, 3, 4, device="cuda")
    frames = torch.zeros(2, 3, 4, 3, dtype=torch.uint8, device="cuda")
    ops.preview_panel(vol, frames, 0, 0)
    for bad_vol in (vol.cpu(), vol.double(), vol.to(torch.int32), vol[0], torch.zeros(1, 2, 3, 8, device="cuda")[..., ::2], "x"):
        with pytest.raises(lib.RxError):
            ops.preview_panel(bad_vol, frames, 0, 0)
    for bad_frames in (frames.cpu(), frames.float(), frames[:1], frames[..., :2], torch.zeros(2, 3, 8, 3, dtype=torch.uint8, device="cuda")[:, :, ::2]):
        with pytest.raises(lib.RxError):
            ops.preview_panel(vol, bad_frames, 0, 0)
    for kw in (dict(y0=1), dict(x0=1), dict(y0=-1), dict(z_step=0), dict(minmax=torch.zeros(1, 2, 3, device="cuda")),
               dict(minmax=torch.zeros(1, 2, 2))):
        with pytest.raises(lib.RxError):
            ops.preview_panel(vol, frames, **{"y0": 0, "x0": 0, **kw})
    img = torch.zeros(2, 1, 2, 3, 4, device="cuda")
    t, p = {"a": img.clone()}, {"a": img.clone()}
    ops.preview_frames(img, t, p)
    for args in ((img.cpu(), t, p), (img, {"a": img.cpu()}, p), (img.double(), t, p), (img[:, :, 0], {"a": img[:, :, 0]}, {"a": img[:, :, 0]}),
                 (img, t, {"b": img}), (img, t, {"a": torch.zeros(2, 1, 2, 3, 5, device="cuda")}),
                 (torch.zeros(2, 1, 2, 3, 8, device="cuda")[..., ::2], t, p)):
        with pytest.raises(lib.RxError):
            ops.preview_frames(*args)
    for kw in (dict(sample=2), dict(sample=-1), dict(every=0), dict(out=torch.zeros(2, 6, 8, 3, dtype=torch.uint8)),
               dict(out=torch.zeros(2, 6, 9, 3, dtype=torch.uint8, device="cuda"))):
        with pytest.raises(lib.RxError):
            ops.preview_frames(img, t, p, **kw)
