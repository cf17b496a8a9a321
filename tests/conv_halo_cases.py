"""The calls whose halo-kernel dispatch is pinned by tests/data/conv_halo_dispatch.json: what scripts/record_conv_halo_dispatch.py
recorded (kernel name, `fused` flag, SHA-256 of every output) and what test_conv_halo_dispatch_gpu.py replays.  `queries()` states
the same calls as the selector's input (csrc/rx_conv_halo_plan.h) for test_conv_halo_plan_cpu.py, without a GPU.

n = 2, kernel 3x3x3, stride 1.  Inputs are seeded random floats: integer data would make the fused sums independent of the order in
which the persistent grid adds them, and a changed grid would go unseen."""
import functools
import hashlib
import json
import os

import torch

JSON_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "conv_halo_dispatch.json")
N, K, S = 2, (3, 3, 3), (1, 1, 1)
HALF = ("bfloat16", "float16")
ALL = HALF + ("float32",)
# (label, Ci, Co, (Z, Y, X), dtypes): each the smallest shape that reaches its branch; tiles = n * ceil(Z/4) ceil(Y/4) ceil(X/16)
SHAPES = [
    ("A", 32, 32, (30, 36, 64), ALL),        # conv_halo32p: 576 tiles >= 512, ragged z / y
    ("B1", 64, 64, (14, 32, 64), HALF),      # conv_halo64ws, one channel block: 256 tiles
    ("B2", 64, 128, (14, 32, 64), HALF),     # conv_halo64ws, two channel blocks forward
    ("C", 64, 96, (14, 32, 32), HALF),       # conv_halo32ws: 128 tiles x 3 blocks forward, x 2 backward
    ("D1", 32, 32, (16, 32, 48), ALL),       # conv_halo32: 192 tiles, below 512 and Ci < 64
    ("D2", 128, 32, (16, 32, 48), ALL),      # conv_halo32 with epilogue statistics: 192 pairs < 256 keeps it off 32ws
    ("E1", 32, 64, (48, 32, 8), ALL),        # conv_halo_kernel<32>: tile 4x8x8, 96 tiles x 2 blocks = 192
    ("E2", 32, 256, (32, 32, 8), ALL),       # conv_halo_kernel<64>: 64 tiles x 4 = 256
    ("F1", 256, 256, (4, 4, 4), HALF),       # no 256-voxel tile: the gather kernels
    ("F2", 32, 32, (16, 16, 32), HALF),      # 64 pairs < 192: the gather kernels
]
ENTRIES = ("fwd", "fwd_stats", "bwd_data_acc0", "bwd_data_acc1", "bwd_data_instats_acc0", "bwd_data_instats_acc1")
# planar concat (the calls of test_planar_concat_convs_equal_interleaved): 64 channels as two dense 32-channel planes
PLANAR_DIMS = (16, 32, 64)
PLANAR_ENTRIES = ("planar_fwd", "planar_fwd_stats", "plane_out_fwd", "planar_dx_acc0", "planar_dx_acc1", "planar_too_small")
WS_BYTES = 192 << 20                         # ops.workspace(): what the statistics entry points offer


def case_ids():
    ids = [f"{lab}/{dt}/{e}" for lab, _, _, _, dts in SHAPES for dt in dts for e in ENTRIES]
    return ids + [f"G/{dt}/{e}" for dt in HALF for e in PLANAR_ENTRIES]


@functools.lru_cache(maxsize=8)          # the entry points of one shape share their host tensors; callers never write to them
def _rnd(shape, dtype, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def _act(ops, ncdhw):
    return ops.Act(ncdhw.permute(0, 2, 3, 4, 1).contiguous().cuda())


def _sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def _planes(t):
    """(n, z, y, x, 64) -> the (2, n, z, y, x, 32) root of a planar concat"""
    return torch.stack([t[..., :32].contiguous(), t[..., 32:].contiguous()], 0)


def run(ops, cid):
    """one recorded call -> {"kernel", "fused" (entry points that return it), "raises" (refused calls), "sha": {output: digest}}"""
    from mt3d_amd.engine.lib import RxError
    lab, dtn, entry = cid.split("/")
    dtype = getattr(torch, dtn)
    if lab == "G":
        ci, co, dims = 64, 32, PLANAR_DIMS
    else:
        ci, co, dims = next((a, b, d) for l, a, b, d, _ in SHAPES if l == lab)
    w = _rnd((co, ci, *K), torch.float32, 2, (27 * ci) ** -0.5).cuda()
    wf, wb = ops.pack_conv_weight(w, dtype)
    bias = _rnd((co,), torch.float32, 3).cuda()
    out, sha = {}, {}
    if entry == "planar_too_small":
        small = ops.Act.planar(torch.zeros((2, 1, 4, 4, 16, 32), dtype=dtype, device="cuda"))
        try:
            ops.conv3d_fwd(small, wf, None, ops.Act.empty(1, 4, 4, 16, 32, dtype), K, S)
            out["raises"] = None
        except RxError as e:
            out["raises"] = str(e)
    elif entry in ("fwd", "fwd_stats", "planar_fwd", "planar_fwd_stats", "plane_out_fwd"):
        x = _act(ops, _rnd((N, ci, *dims), dtype, 1))
        if entry.startswith("planar"):
            x = ops.Act.planar(_planes(x.t))
        y = ops.Act(torch.full((N, *dims, co), float("nan"), dtype=dtype, device="cuda"))
        if entry == "plane_out_fwd":         # written into the middle plane of a three-plane concat
            root3 = torch.full((3, N, *dims, 32), -97.0, dtype=dtype, device="cuda")
            y = ops.Act.planar(root3, 1)
        if entry.endswith("stats"):
            stats = torch.full((N, co, 2), float("nan"), device="cuda")
            ops.conv3d_fwd_stats(x, wf, bias, y, K, S, stats)
            sha["stats"] = stats
        else:
            ops.conv3d_fwd(x, wf, bias, y, K, S)
        sha["y"] = root3 if entry == "plane_out_fwd" else y.t
    else:
        acc = entry.endswith("acc1")
        dy = _act(ops, _rnd((N, co, *dims), dtype, 4, 0.2))
        dx = _act(ops, _rnd((N, ci, *dims), dtype, 5, 0.1))
        if entry.startswith("planar"):
            root = _planes(dx.t)
            dx = ops.Act.planar(root)
        if "instats" in entry:
            yv = _act(ops, _rnd((N, ci, *dims), dtype, 6) + 0.3)
            stats = torch.empty((N, ci, 2), device="cuda")
            ops.instnorm_stats(yv, stats)
            m12 = torch.full((N, ci, 2), -3.0, device="cuda")
            out["fused"] = ops.conv3d_bwd_data_instats(dy, wb, dx, K, S, acc, yv, stats, 0.01, m12)
            sha["m12"] = m12
        else:
            ops.conv3d_bwd_data(dy, wb, dx, K, S, acc)
        sha["dx"] = root if entry.startswith("planar") else dx.t
    # (a refused call notes no kernel of its own: the name would be the previous call's)
    out["kernel"] = None if out.get("raises") else ops.load().rx_last_conv_kernel().decode()
    torch.cuda.synchronize()
    out["sha"] = {k: _sha(v) for k, v in sha.items()}
    return out


def recorded():
    with open(JSON_PATH) as f:
        return json.load(f)["cases"]


# ---- the same calls as rx_ch_choose queries ----------------------------------------------------------------------------------
QUERY_FIELDS = ("dt", "N", "Z", "Y", "X", "Ci", "Co", "ldi", "ldo", "in_cs", "out_cs", "in_lo", "out_lo", "w_lo", "bsy_lo", "bs_ldy",
                "flip", "accumulate", "stat_offered", "stat_bytes", "want_bs")
DT_CODE = {"float32": 0, "bfloat16": 1, "float16": 2}


def query(dt, n, dims, ci, co, **kw):
    """a query with dense, 16-byte aligned operands (what torch allocates); `ci` / `co` are the launch's input / output channels"""
    q = dict.fromkeys(QUERY_FIELDS, 0)
    q.update(dt=DT_CODE.get(dt, dt), N=n, Z=dims[0], Y=dims[1], X=dims[2], Ci=ci, Co=co, ldi=ci, ldo=co)
    q.update(kw)
    return q


def query_of(cid):
    """the rx_ch_choose query behind a recorded call (None: the call is refused before the selector, or is not a halo candidate)"""
    lab, dtn, entry = cid.split("/")
    if lab == "G":
        ci, co, dims = 64, 32, PLANAR_DIMS
        plane = N * dims[0] * dims[1] * dims[2] * 32
        if entry == "planar_too_small":
            return query(dtn, 1, (4, 4, 16), 64, 32, ldi=32, in_cs=4 * 4 * 16 * 32)
        if entry in ("planar_fwd", "planar_fwd_stats"):
            stat = entry.endswith("stats")
            return query(dtn, N, dims, 64, 32, ldi=32, in_cs=plane, stat_offered=int(stat), stat_bytes=WS_BYTES if stat else 0)
        if entry == "plane_out_fwd":
            return query(dtn, N, dims, 64, 32)
        return query(dtn, N, dims, 32, 64, ldo=32, out_cs=plane, flip=1, accumulate=int(entry.endswith("acc1")))
    ci, co, dims = next((a, b, d) for l, a, b, d, _ in SHAPES if l == lab)
    if entry == "fwd":
        return query(dtn, N, dims, ci, co)
    if entry == "fwd_stats":
        return query(dtn, N, dims, ci, co, stat_offered=1, stat_bytes=WS_BYTES)
    acc = int(entry.endswith("acc1"))
    if "instats" in entry:
        return query(dtn, N, dims, co, ci, flip=1, accumulate=acc, stat_offered=1, stat_bytes=WS_BYTES, want_bs=1, bs_ldy=ci)
    return query(dtn, N, dims, co, ci, flip=1, accumulate=acc)
