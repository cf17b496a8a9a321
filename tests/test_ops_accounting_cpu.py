"""CPU: the profiler accounting of engine.ops -- which label, how many algorithmic bytes (bench.py's `hbm` block) and which kernel
name with how many FLOPs (its `kernels` block) every accounted wrapper hands to the profiler.  A recording stand-in is installed
through `ops.set_profiler`; it notes its arguments and never calls the launch, so nothing here needs a device.

TABLE was MEASURED, not derived: this file was run against the commit before `engine/ops` became a package and the values it
recorded were pasted in; it is carried unchanged across that split.  Operands have pairwise different channel counts, sliced out of
wider buffers, so that a formula that counts the wrong operand, or the buffer's channels instead of the addressed ones, shows."""
import os

import pytest
import torch

import mt3d_amd  # noqa: F401
from mt3d_amd.engine import lib, ops

N, SMALL, BIG = 2, (2, 3, 4), (4, 6, 8)          # 24 voxels (<= 128) and 192 (> 128): the two tile buckets of igemm_name
F16 = torch.float16


class Recorder:
    def __init__(self):
        self.log = []

    def run(self, name, flops, launches, fn):
        self.log.append((name, flops, launches))

    def run_bytes(self, name, nbytes, fn):
        self.log.append((name, nbytes))


class OnDevice(torch.Tensor):
    """a host tensor that answers `is_cuda` like a device tensor: the wrappers that refuse host batches get as far as the profiler"""
    is_cuda = property(lambda self: True)


def dev(*shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype).as_subclass(OnDevice)


def act(c, dims=SMALL, dtype=F16):
    """`c` channels from channel 8 of a buffer 16 wider"""
    return ops.Act(torch.zeros((N, *dims, c + 16), dtype=dtype), 8, c)


def calls():
    g, y, out, dy, dres, res, pool, big = act(32), act(24), act(16), act(8), act(40), act(4), act(12), act(64, BIG)
    y32 = act(20, dtype=torch.float32)
    ncdhw, x_in = torch.zeros(N, 3, *SMALL), torch.zeros(N, 1, *SMALL)
    w, wt = torch.zeros(4, 3, 3, 3, 3), torch.zeros(6, 5, 2, 2, 2)
    wf, wb = torch.zeros(27, 4, 3, dtype=F16), torch.zeros(8, 6, 5, dtype=F16)
    ws = torch.zeros(8, dtype=torch.uint8)
    k3, s1, s2 = (3, 3, 3), (1, 1, 1), (2, 2, 2)
    o = ops
    yield "instnorm_stats", lambda: o.instnorm_stats(y, None)
    yield "instnorm_stats fp32", lambda: o.instnorm_stats(y32, None, 1e-5, ws)
    yield "instnorm_act_fwd", lambda: o.instnorm_act_fwd(y, None, out)
    yield "instnorm_act_fwd residual", lambda: o.instnorm_act_fwd(y, None, out, 0.01, res)
    yield "instnorm_fwd", lambda: o.instnorm_fwd(y, None, out)
    yield "instnorm_fwd residual", lambda: o.instnorm_fwd(y, None, out, residual=res, ws=ws)
    yield "instnorm_act_bwd", lambda: o.instnorm_act_bwd(g, y, None, out, dy)
    yield "instnorm_act_bwd no out", lambda: o.instnorm_act_bwd(g, y, None, None, dy, 0.01)
    yield "instnorm_act_bwd d_residual", lambda: o.instnorm_act_bwd(g, y, None, out, dy, d_residual=dres)
    yield "instnorm_act_bwd d_residual accumulated", lambda: o.instnorm_act_bwd(g, y, None, out, dy, 0.01, dres, True, ws)
    yield "instnorm_act_bwd_res", lambda: o.instnorm_act_bwd_res(g, y, None, out, dy, dres)
    yield "instnorm_act_bwd_res pool_dy", lambda: o.instnorm_act_bwd_res(g, y, None, out, dy, dres, 0.01, pool, s2)
    yield "instnorm_act_bwd_apply", lambda: o.instnorm_act_bwd_apply(g, y, None, out, dy, None)
    yield "instnorm_act_bwd_apply d_residual", lambda: o.instnorm_act_bwd_apply(g, y, None, out, dy, None, d_residual=dres)
    yield "instnorm_act_bwd_apply d_residual accumulated", lambda: o.instnorm_act_bwd_apply(g, y, None, None, dy, None, 0.01, dres,
                                                                                           accumulate_residual=True)
    yield "se_gate_fwd", lambda: o.se_gate_fwd(y, None, None, None, None, None, None, path_scale=None, ws=ws)
    yield "instnorm_gate_act_fwd", lambda: o.instnorm_gate_act_fwd(y, None, None, 1, out)
    yield "instnorm_gate_act_fwd residual", lambda: o.instnorm_gate_act_fwd(y, None, None, 0, out, residual=res)
    yield "se_gate_bwd", lambda: o.se_gate_bwd(g, y, None, out, 0.01, None, None, None, None, None, None, None, ws=ws)
    yield "se_gate_bwd no out", lambda: o.se_gate_bwd(g, y, None, None, 0.01, None, None, None, None, None, None, None, dw1=None)
    yield "instnorm_gate_act_bwd", lambda: o.instnorm_gate_act_bwd(g, y, None, out, 0.01, None, None, None, 1, dy)
    yield "instnorm_gate_act_bwd d_residual", lambda: o.instnorm_gate_act_bwd(g, y, None, out, 0.01, None, None, None, 1, dy, dres)
    yield "instnorm_gate_act_bwd d_residual accumulated", lambda: o.instnorm_gate_act_bwd(g, y, None, out, 0.01, None, None, None, 1,
                                                                                         dy, dres, True)
    yield "avgpool_fwd", lambda: o.avgpool_fwd(y, pool, s2)
    yield "instnorm_act_pool_fwd", lambda: o.instnorm_act_pool_fwd(y, None, out, pool, s2)
    yield "instnorm_act_pool_fwd residual", lambda: o.instnorm_act_pool_fwd(y, None, out, pool, s2, 0.01, res)
    yield "avgpool_bwd", lambda: o.avgpool_bwd(dy, g, s2)
    yield "avgpool_bwd accumulated", lambda: o.avgpool_bwd(dy, g, s2, accumulate=True)
    yield "head_fwd", lambda: o.head_fwd(y, w, None, ncdhw)
    yield "head_bwd", lambda: o.head_bwd(ncdhw, y, w, dy, None, None)
    yield "head_bwd no dx", lambda: o.head_bwd(ncdhw, y, w, None, None, None, ws=ws)
    yield "instnorm_act_head_fwd", lambda: o.instnorm_act_head_fwd(y, None, out, w, None, ncdhw, 1)
    yield "instnorm_act_head_fwd no out", lambda: o.instnorm_act_head_fwd(y, None, None, w, None, ncdhw, 0, slope=0.2)
    yield "instnorm_act_bwd_head", lambda: o.instnorm_act_bwd_head(ncdhw, w, y, None, dy, dw=None, db=None)
    yield "channel_sum", lambda: o.channel_sum(g, None)
    yield "pack_conv_weight", lambda: o.pack_conv_weight(w, F16)
    yield "pack_conv_weight fwd only", lambda: o.pack_conv_weight(w, F16, wf, None, True, False)
    yield "pack_conv_weight bwd only fp32", lambda: o.pack_conv_weight(w, torch.float32, want_fwd=False)
    yield "pack_convT_weight", lambda: o.pack_convT_weight(wt, F16)
    yield "pack_convT_weight bwd only", lambda: o.pack_convT_weight(wt, F16, None, wb, want_fwd=False, want_bwd=True)
    yield "pack_convT_weight neither", lambda: o.pack_convT_weight(wt, F16, want_fwd=False, want_bwd=False)
    yield "pack_weights_multi", lambda: o.pack_weights_multi([(w, 0, wf, None), (wt, 1, wf, wb), (wt, 1, None, None)], F16)
    yield "stem_conv_fwd", lambda: o.stem_conv_fwd(x_in, None, None, out, k3)
    yield "stem_conv_fwd_stats", lambda: o.stem_conv_fwd_stats(x_in, None, None, out, k3, None, ws=ws)
    yield "stem_conv_bwd_weight", lambda: o.stem_conv_bwd_weight(x_in, dy, None, k3)
    yield "convT3d_fwd", lambda: o.convT3d_fwd(y, None, None, big, s2)
    yield "convT3d_bwd_data", lambda: o.convT3d_bwd_data(big, None, dy, s2)
    yield "convT3d_bwd_data accumulated", lambda: o.convT3d_bwd_data(big, None, dy, s2, True, ws)
    yield "convT3d_bwd_weight", lambda: o.convT3d_bwd_weight(y, big, None, s2, ws=ws)
    # the MFMA convolutions: kernel names by tile bucket (voxels <= 128 / > 128) and channel bucket (co % 64 == 0 or not)
    big32, small64 = act(32, BIG), act(64)
    yield "conv3d_fwd <256,64>", lambda: o.conv3d_fwd(big32, None, None, big, k3, s1, ws)
    yield "conv3d_fwd <128,32>", lambda: o.conv3d_fwd(y, None, None, g, (1, 3, 3), s1, ws=ws)
    yield "conv3d_fwd_stats <128,64>", lambda: o.conv3d_fwd_stats(y, None, None, small64, k3, s1, None, ws=ws)
    yield "conv3d_fwd_stats <256,32>", lambda: o.conv3d_fwd_stats(big, None, None, big32, (1, 1, 1), s1, None, 1e-5, ws)
    yield "conv3d_bwd_data <256,64>", lambda: o.conv3d_bwd_data(big32, None, big, k3, s1, ws=ws)
    yield "conv3d_bwd_data <128,32> from stride 2", lambda: o.conv3d_bwd_data(dy, None, g, k3, s2, True, ws)
    yield "conv3d_bwd_data_instats <128,64>", lambda: o.conv3d_bwd_data_instats(y, None, small64, k3, s1, False, small64, None, 0.01,
                                                                               None, ws)
    yield "conv3d_bwd_data_instats <256,32>", lambda: o.conv3d_bwd_data_instats(big, None, big32, k3, s1, False, big32, None, 0.01,
                                                                               None, ws=ws)
    # validation and pipeline passes that refuse host tensors
    pred, tgt = dev(N, 3, *SMALL, dtype=F16), dev(N, 3, *SMALL)
    yield "seg_counts", lambda: o.seg_counts(pred, tgt)
    yield "class_counts probabilities", lambda: o.class_counts(pred, tgt)
    yield "class_counts indices", lambda: o.class_counts(pred, dev(N, *SMALL, dtype=torch.int64))
    tables = [(dev(n, dtype=torch.int32), dev(n, 4), dev(n, 4)) for n in SMALL]
    yield "elastic_apply", lambda: o.elastic_apply(tgt, dev(N, 3, 4, 4, 4), tables, (8, 8, 8), "linear", "clamp")
    frames = dev(2, 3, 4, 3, dtype=torch.uint8)
    yield "preview_panel", lambda: o.preview_panel(pred[0], frames, 0, 0)
    yield "preview_panel one channel, every other slice", lambda: o.preview_panel(tgt[1, :1], frames, 0, 0, z_step=2)
    yield "preview_frames", lambda: o.preview_frames(tgt[:, :1], {"a": tgt[:, :1], "n": pred}, {"a": pred[:, :2], "n": pred},
                                                     sample=1, every=2)


def wgrad_calls():
    """these ask the built library for their workspace before they reach the profiler"""
    ws = torch.zeros(8, dtype=torch.uint8)
    yield "conv3d_bwd_weight <64,32>", lambda: ops.conv3d_bwd_weight(act(32), act(64), None, (3, 3, 3), (1, 1, 1), ws)
    yield "conv3d_bwd_weight <32,64>", lambda: ops.conv3d_bwd_weight(act(64, BIG), act(32, BIG), None, (1, 3, 3), (1, 1, 1), ws=ws)
    yield "normal_stats", lambda: ops.normal_stats(dev(N, 3, *SMALL, dtype=F16), dev(N, 3, *SMALL))


TABLE = {
    'instnorm_stats': ('in_stats(colreduce)', 2304),
    'instnorm_stats fp32': ('in_stats(colreduce)', 3840),
    'instnorm_act_fwd': ('in_act_fwd', 3840),
    'instnorm_act_fwd residual': ('in_act_fwd', 4224),
    'instnorm_fwd': ('in_fwd(stats+apply)', 3840),
    'instnorm_fwd residual': ('in_fwd(stats+apply)', 4224),
    'instnorm_act_bwd': ('in_act_bwd(colreduce+apply)', 7680),
    'instnorm_act_bwd no out': ('in_act_bwd(colreduce+apply)', 6144),
    'instnorm_act_bwd d_residual': ('in_act_bwd(colreduce+apply)', 11520),
    'instnorm_act_bwd d_residual accumulated': ('in_act_bwd(colreduce+apply)', 15360),
    'instnorm_act_bwd_res': ('in_act_bwd_res(colreduce+apply)', 11520),
    'instnorm_act_bwd_res pool_dy': ('in_act_bwd_res(colreduce+apply)', 12672),
    'instnorm_act_bwd_apply': ('in_act_bwd_apply', 7680),
    'instnorm_act_bwd_apply d_residual': ('in_act_bwd_apply', 11520),
    'instnorm_act_bwd_apply d_residual accumulated': ('in_act_bwd_apply', 13824),
    'se_gate_fwd': ('se_gate_fwd(linesum+gate)', 2304),
    'instnorm_gate_act_fwd': ('in_gate_act_fwd', 3840),
    'instnorm_gate_act_fwd residual': ('in_gate_act_fwd', 4224),
    'se_gate_bwd': ('se_gate_bwd(linesums+gate)', 6912),
    'se_gate_bwd no out': ('se_gate_bwd(linesums+gate)', 5376),
    'instnorm_gate_act_bwd': ('in_gate_act_bwd', 7680),
    'instnorm_gate_act_bwd d_residual': ('in_gate_act_bwd', 11520),
    'instnorm_gate_act_bwd d_residual accumulated': ('in_gate_act_bwd', 15360),
    'avgpool_fwd': ('avgpool_fwd', 3456),
    'instnorm_act_pool_fwd': ('in_act_pool_fwd', 4992),
    'instnorm_act_pool_fwd residual': ('in_act_pool_fwd', 5376),
    'avgpool_bwd': ('avgpool_bwd', 3840),
    'avgpool_bwd accumulated': ('avgpool_bwd', 6912),
    'head_fwd': ('head_fwd', 2880),
    'head_bwd': ('head_bwd', 3648),
    'head_bwd no dx': ('head_bwd', 2880),
    'instnorm_act_head_fwd': ('in_act_head_fwd', 4416),
    'instnorm_act_head_fwd no out': ('in_act_head_fwd', 2880),
    'instnorm_act_bwd_head': ('in_act_bwd_head(colreduce+apply)', 3648),
    'channel_sum': ('channel_sum', 3072),
    'pack_conv_weight': ('pack', 2592),
    'pack_conv_weight fwd only': ('pack', 1944),
    'pack_conv_weight bwd only fp32': ('pack', 2592),
    'pack_convT_weight': ('pack', 1920),
    'pack_convT_weight bwd only': ('pack', 1440),
    'pack_convT_weight neither': ('pack', 960),
    'pack_weights_multi': ('pack', 4824),
    'stem_conv_fwd': ('stem_conv_fwd', 1728),
    'stem_conv_fwd_stats': ('stem_conv_fwd', 1728),
    'stem_conv_bwd_weight': ('stem_conv_bwd_weight', 960),
    'convT3d_fwd': ('convT_fwd', 51456),
    'convT3d_bwd_data': ('convT_bwd_data', 49920),
    'convT3d_bwd_data accumulated': ('convT_bwd_data', 50688),
    'convT3d_bwd_weight': ('convT_bwd_weight', 51456),
    'conv3d_fwd <256,64>': ('fwd:igemm_kernel<256,64>', 42467328.0, 1),
    'conv3d_fwd <128,32>': ('fwd:igemm_kernel<128,32>', 663552.0, 1),
    'conv3d_fwd_stats <128,64>': ('fwd:igemm_kernel<128,64>', 3981312.0, 1),
    'conv3d_fwd_stats <256,32>': ('fwd:igemm_kernel<256,32>', 1572864.0, 1),
    'conv3d_bwd_data <256,64>': ('dgrad:igemm_kernel<256,64>', 42467328.0, 1),
    'conv3d_bwd_data <128,32> from stride 2': ('dgrad:igemm_kernel<128,32>', 663552.0, 1),
    'conv3d_bwd_data_instats <128,64>': ('dgrad:igemm_kernel<128,64>', 3981312.0, 1),
    'conv3d_bwd_data_instats <256,32>': ('dgrad:igemm_kernel<256,32>', 42467328.0, 1),
    'seg_counts': ('seg_counts', 864),
    'class_counts probabilities': ('class_counts', 864),
    'class_counts indices': ('class_counts', 672),
    'elastic_apply': ('elastic_apply', 1152),
    'preview_panel': ('preview_panel', 216),
    'preview_panel one channel, every other slice': ('preview_panel', 84),
    'preview_frames': ('preview_frames', 444),
}

WGRAD_TABLE = {
    'conv3d_bwd_weight <64,32>': ('wgrad:wgrad_kernel<64,32>', 5308416.0, 1),
    'conv3d_bwd_weight <32,64>': ('wgrad:wgrad_kernel<32,64>', 14155776.0, 1),
    'normal_stats': ('normal_stats', 864),
}


def record(cases):
    rec, got = Recorder(), {}
    ops.set_profiler(rec)
    try:
        for case, call in cases:
            del rec.log[:]
            call()
            assert len(rec.log) == 1, f"{case}: {len(rec.log)} profiler entries"
            got[case] = rec.log[0]
    finally:
        ops.set_profiler(None)
    return got


def test_every_accounted_wrapper_reports_its_label_and_cost():
    got = record(calls())
    assert got.keys() == TABLE.keys()
    wrong = {case: (got[case], TABLE[case]) for case in TABLE if got[case] != TABLE[case]}
    assert not wrong, wrong


@pytest.mark.skipif(not os.path.exists(lib.LIB_PATH), reason="the workspace queries need the built library")
def test_wrappers_that_ask_the_library_first():
    assert record(wgrad_calls()) == WGRAD_TABLE


def test_profiling_reports_the_installed_profiler():
    assert ops.profiling() is None
    rec = Recorder()
    ops.set_profiler(rec)
    try:
        assert ops.profiling() is rec
        ops.avgpool_fwd(act(8), act(8), (2, 2, 2))
        assert rec.log == [("avgpool_fwd", 2 * N * 24 * 8 * 2)]
    finally:
        ops.set_profiler(None)
    assert ops.profiling() is None
