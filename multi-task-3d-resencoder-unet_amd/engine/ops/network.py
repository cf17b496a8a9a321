"""The network's launches: weight packing, the MFMA convolutions and transposed convolutions, the InstanceNorm family, SqueezeExcite
and DropPath gates, pooling, stem and task heads.  Each accounted launch carries its `hbm` label and byte formula, or its `flops`
kernel name and count, as a decorator (see core)."""
import ctypes
from ctypes import byref, c_int

import torch

from .. import lib as _l
from ..lib import I3, check, load, stream_ptr
from .core import LaunchProfiler, _code, _desc, _ptr, _tb, _ws_args, flops, hbm, timed_bytes, workspace


# ---- parameter packing ------------------------------------------------------------------------
def _pack_bytes(w, dtype, want_fwd, want_bwd):
    e = torch.empty((), dtype=dtype).element_size()
    return w.numel() * (4 + (e if want_fwd else 0) + (e if want_bwd else 0))


def _pack(entry, w, co, ci, dtype, w_fwd, w_bwd, want_fwd, want_bwd):
    taps = w[0, 0].numel()
    if want_fwd and w_fwd is None:
        w_fwd = torch.empty((taps, co, ci), dtype=dtype, device=w.device)
    if want_bwd and w_bwd is None:
        w_bwd = torch.empty((taps, ci, co), dtype=dtype, device=w.device)
    check(getattr(load(), entry)(_code(dtype), _ptr(w), w.shape[0], w.shape[1], taps, _ptr(w_fwd if want_fwd else None),
                                 _ptr(w_bwd if want_bwd else None), stream_ptr()), entry)
    return w_fwd, w_bwd


@hbm("pack", _pack_bytes)
def pack_conv_weight(w, dtype, w_fwd=None, w_bwd=None, want_fwd=True, want_bwd=True):
    """w: (Co, Ci, kz, ky, kx) fp32 -> (w_fwd [T][Co][Ci], w_bwd [T][Ci][Co]) in `dtype`."""
    return _pack("rx_pack_conv_weight", w, w.shape[0], w.shape[1], dtype, w_fwd, w_bwd, want_fwd, want_bwd)


@hbm("pack", _pack_bytes)
def pack_convT_weight(w, dtype, w_fwd=None, w_bwd=None, want_fwd=True, want_bwd=True):
    """w: (Ci, Co, kz, ky, kx) fp32 -> (w_fwd [T][Co][Ci], w_bwd [T][Ci][Co])."""
    return _pack("rx_pack_convT_weight", w, w.shape[1], w.shape[0], dtype, w_fwd, w_bwd, want_fwd, want_bwd)


def pack_weights_multi(items, dtype):
    """items: [(w fp32 contiguous, kind 0 conv / 1 convT, w_fwd or None, w_bwd or None)] -> ONE launch per 40 tensors
    (rx_pack_multi).  5-D weights (a 2-D net's are unsqueezed by the caller)."""
    n = len(items)
    if n == 0:
        return
    VP, IA = ctypes.c_void_p * n, c_int * n
    wp = VP(*[w.data_ptr() for w, _, _, _ in items])
    kind = IA(*[k for _, k, _, _ in items])
    A = IA(*[w.shape[0] for w, _, _, _ in items])
    B = IA(*[w.shape[1] for w, _, _, _ in items])
    T = IA(*[w[0, 0].numel() for w, _, _, _ in items])
    fw = VP(*[(f.data_ptr() if f is not None else None) for _, _, f, _ in items])
    bw = VP(*[(b.data_ptr() if b is not None else None) for _, _, _, b in items])
    esz = torch.empty((), dtype=dtype).element_size()
    nbytes = sum(w.numel() * (4 + (esz if f is not None else 0) + (esz if b is not None else 0)) for w, _, f, b in items)
    timed_bytes("pack", nbytes, lambda: check(load().rx_pack_multi(_code(dtype), n, wp, kind, A, B, T, fw, bw, stream_ptr()),
                                             "rx_pack_multi"))


# ---- convolutions -----------------------------------------------------------------------------
def _igemm(kind, tile, full, other, kernel):
    """("kind:igemm_kernel<..>" by the voxels and channels of `tile`, the FLOPs of a conv between `full` (all its voxels) and `other`)"""
    return kind + ":" + LaunchProfiler.igemm_name(tile.voxels, tile.c), _conv_flops(full, other, kernel)


def _conv_flops(full, other, kernel):
    return 2.0 * full.dims[0] * full.voxels * full.c * other.c * (kernel[0] * kernel[1] * kernel[2])


@flops(lambda x, y, kernel: _igemm("fwd", y, y, x, kernel))
def conv3d_fwd(x, w_fwd, bias, y, kernel, stride, ws=None):
    check(load().rx_conv3d_fwd(_code(x.dtype), byref(x.desc()), _ptr(w_fwd), _ptr(bias), byref(y.desc()),
                               I3(*kernel), I3(*stride), *_ws_args(ws), stream_ptr()), "rx_conv3d_fwd")


@flops(lambda x, y, kernel: _igemm("fwd", y, y, x, kernel))
def conv3d_fwd_stats(x, w_fwd, bias, y, kernel, stride, stats, eps=1e-5, ws=None):
    """conv + InstanceNorm statistics of its output (fused into the conv epilogue on the persistent halo kernels)"""
    check(load().rx_conv3d_fwd_stats(_code(x.dtype), byref(x.desc()), _ptr(w_fwd), _ptr(bias), byref(y.desc()), I3(*kernel),
                                     I3(*stride), float(eps), _ptr(stats), *_ws_args(ws), stream_ptr()), "rx_conv3d_fwd_stats")


@flops(lambda dy, dx, kernel: _igemm("dgrad", dx, dy, dx, kernel))
def conv3d_bwd_data(dy, w_bwd, dx, kernel, stride, accumulate=False, ws=None):
    check(load().rx_conv3d_bwd_data(_code(dy.dtype), byref(dy.desc()), _ptr(w_bwd), byref(dx.desc()), I3(*kernel), I3(*stride),
                                    int(accumulate), *_ws_args(ws), stream_ptr()), "rx_conv3d_bwd_data")


@flops(lambda dy, dx, kernel: _igemm("dgrad", dx, dx, dy, kernel))
def conv3d_bwd_data_instats(dy, w_bwd, dx, kernel, stride, accumulate, in_y, in_stats, slope, m12, ws=None):
    """backward-data that completes dx = dL/d(out of an InstanceNorm layer without residual) and, on the persistent kernel,
    leaves that layer's two backward means in m12.  Returns True when m12 was written (continue with instnorm_act_bwd_apply)."""
    fused = c_int(0)
    check(load().rx_conv3d_bwd_data_instats(_code(dy.dtype), byref(dy.desc()), _ptr(w_bwd), byref(dx.desc()), I3(*kernel),
                                            I3(*stride), int(accumulate), byref(in_y.desc()), _ptr(in_stats), float(slope),
                                            _ptr(m12), byref(fused), *_ws_args(ws), stream_ptr()), "rx_conv3d_bwd_data_instats")
    return bool(fused.value)


def _bwd_bytes(g, y, out, dy, d_residual, accumulate_residual):
    return _tb(g) + _tb(y) + _tb(dy) + _tb(out) + _tb(d_residual) * (2 if accumulate_residual else 1)


@hbm("in_act_bwd_apply", _bwd_bytes)
def instnorm_act_bwd_apply(g, y, stats, out, dy, m12, slope=0.01, d_residual=None, accumulate_residual=False):
    check(load().rx_instnorm_act_bwd_apply(_code(y.dtype), byref(g.desc()), byref(y.desc()), _ptr(stats), _desc(out), float(slope),
                                           _ptr(m12), byref(dy.desc()), _desc(d_residual), int(accumulate_residual), stream_ptr()),
          "rx_instnorm_act_bwd_apply")


@flops(lambda x, dy, kernel: (f"wgrad:wgrad_kernel<{64 if dy.c % 64 == 0 else 32},{64 if x.c % 64 == 0 else 32}>",
                              _conv_flops(dy, x, kernel)))
def conv3d_bwd_weight(x, dy, dw, kernel, stride, ws=None):
    need = load().rx_conv3d_bwd_weight_workspace(byref(x.desc()), byref(dy.desc()), I3(*kernel))
    ws = workspace(need) if ws is None else ws
    check(load().rx_conv3d_bwd_weight(_code(x.dtype), byref(x.desc()), byref(dy.desc()), _ptr(dw), I3(*kernel),
                                      I3(*stride), *_ws_args(ws), stream_ptr()), "rx_conv3d_bwd_weight")


@hbm("convT_fwd", lambda x, y: _tb(x) + _tb(y))
def convT3d_fwd(x, w_fwd, bias, y, stride, ws=None):
    check(load().rx_convT3d_fwd(_code(x.dtype), byref(x.desc()), _ptr(w_fwd), _ptr(bias), byref(y.desc()),
                                I3(*stride), *_ws_args(ws), stream_ptr()), "rx_convT3d_fwd")


@hbm("convT_bwd_data", lambda dy, dx, accumulate: _tb(dy) + _tb(dx) * (2 if accumulate else 1))
def convT3d_bwd_data(dy, w_bwd, dx, stride, accumulate=False, ws=None):
    check(load().rx_convT3d_bwd_data(_code(dy.dtype), byref(dy.desc()), _ptr(w_bwd), byref(dx.desc()), I3(*stride),
                                     int(accumulate), *_ws_args(ws), stream_ptr()), "rx_convT3d_bwd_data")


@hbm("convT_bwd_weight", lambda x, dy: _tb(x) + _tb(dy))
def convT3d_bwd_weight(x, dy, dw, stride, ws=None):
    need = load().rx_convT3d_bwd_weight_workspace(byref(x.desc()), byref(dy.desc()), I3(*stride))
    ws = workspace(need) if ws is None else ws
    check(load().rx_convT3d_bwd_weight(_code(x.dtype), byref(x.desc()), byref(dy.desc()), _ptr(dw), I3(*stride),
                                       *_ws_args(ws), stream_ptr()), "rx_convT3d_bwd_weight")


# ---- InstanceNorm + LeakyReLU + residual -------------------------------------------------------
@hbm("in_stats(colreduce)", lambda y: _tb(y))
def instnorm_stats(y, stats, eps=1e-5, ws=None):
    check(load().rx_instnorm_stats(_code(y.dtype), byref(y.desc()), eps, _ptr(stats), *_ws_args(ws), stream_ptr()), "rx_instnorm_stats")


def instnorm_stats_mask(stats, keep):
    """channel dropout in front of an InstanceNorm: rstd = 0 for the dropped (n, c) planes (see rx_instnorm_stats_mask)"""
    check(load().rx_instnorm_stats_mask(_ptr(stats), _ptr(keep), int(keep.numel()), stream_ptr()), "rx_instnorm_stats_mask")


@hbm("in_act_fwd", lambda y, out, residual: _tb(y) + _tb(out) + _tb(residual))
def instnorm_act_fwd(y, stats, out, slope=0.01, residual=None):
    check(load().rx_instnorm_act_fwd(_code(y.dtype), byref(y.desc()), _ptr(stats), _desc(residual), byref(out.desc()),
                                     float(slope), stream_ptr()), "rx_instnorm_act_fwd")


@hbm("in_fwd(stats+apply)", lambda y, out, residual: _tb(y) + _tb(out) + _tb(residual))
def instnorm_fwd(y, stats, out, slope=0.01, residual=None, eps=1e-5, ws=None):
    """stats + apply; a single launch for the low-resolution stages."""
    check(load().rx_instnorm_fwd(_code(y.dtype), byref(y.desc()), eps, _ptr(stats), _desc(residual), byref(out.desc()),
                                 float(slope), *_ws_args(ws), stream_ptr()), "rx_instnorm_fwd")


@hbm("in_act_bwd(colreduce+apply)", _bwd_bytes)
def instnorm_act_bwd(g, y, stats, out, dy, slope=0.01, d_residual=None, accumulate_residual=False, ws=None):
    check(load().rx_instnorm_act_bwd(_code(y.dtype), byref(g.desc()), byref(y.desc()), _ptr(stats), _desc(out), float(slope),
                                     byref(dy.desc()), _desc(d_residual), int(accumulate_residual), *_ws_args(ws), stream_ptr()),
          "rx_instnorm_act_bwd")


@hbm("in_act_bwd_res(colreduce+apply)",
     lambda g, y, out, dy, d_residual, pool_dy: _tb(g) + _tb(y) + _tb(out) + _tb(dy) + _tb(d_residual) + _tb(pool_dy))
def instnorm_act_bwd_res(g, y, stats, out, dy, d_residual, slope=0.01, pool_dy=None, pool_stride=(1, 1, 1), ws=None):
    """residual-block epilogue backward with the masked gradient written once into `d_residual` (rx_instnorm_act_bwd_res);
    pool_dy: gradient of the next stage's skip-path AvgPool, added on the fly"""
    check(load().rx_instnorm_act_bwd_res(_code(y.dtype), byref(g.desc()), byref(y.desc()), _ptr(stats), byref(out.desc()),
                                         float(slope), _desc(pool_dy), I3(*pool_stride), byref(d_residual.desc()),
                                         byref(dy.desc()), *_ws_args(ws), stream_ptr()), "rx_instnorm_act_bwd_res")


# ---- SqueezeExcite / DropPath fused with InstanceNorm + residual + LeakyReLU ----------------------
def _se_params(se):
    """se: dict(w1, b1, w2, b2, rd, keep_x) of fp32 device tensors, or None (DropPath only)"""
    if se is None:
        return None
    return byref(_l.RxSeParams(se["w1"].data_ptr(), se["b1"].data_ptr(), se["w2"].data_ptr(), se["b2"].data_ptr(),
                               int(se["rd"]), int(se["keep_x"])))


def se_workspace_bytes(y):
    return load().rx_se_workspace(byref(y.desc()))


@hbm("se_gate_fwd(linesum+gate)", lambda y: _tb(y))
def se_gate_fwd(y, stats, se, pooled, hidden, gate, mult, path_scale=None, ws=None):
    ws = workspace(se_workspace_bytes(y)) if ws is None else ws
    check(load().rx_se_gate_fwd(_code(y.dtype), byref(y.desc()), _ptr(stats), _ptr(path_scale), _se_params(se), _ptr(pooled),
                                _ptr(hidden), _ptr(gate), _ptr(mult), *_ws_args(ws), stream_ptr()), "rx_se_gate_fwd")


@hbm("in_gate_act_fwd", lambda y, out, residual: _tb(y) + _tb(out) + _tb(residual))
def instnorm_gate_act_fwd(y, stats, mult, keep_x, out, slope=0.01, residual=None):
    check(load().rx_instnorm_gate_act_fwd(_code(y.dtype), byref(y.desc()), _ptr(stats), _ptr(mult), int(keep_x), _desc(residual),
                                          byref(out.desc()), float(slope), stream_ptr()), "rx_instnorm_gate_act_fwd")


@hbm("se_gate_bwd(linesums+gate)", lambda g, y, out: _tb(g) + _tb(y) + _tb(out))
def se_gate_bwd(g, y, stats, out, slope, se, pooled, hidden, gate, mult, dadd, m12, dw1=None, db1=None, dw2=None, db2=None,
                path_scale=None, ws=None):
    ws = workspace(se_workspace_bytes(y)) if ws is None else ws
    check(load().rx_se_gate_bwd(_code(y.dtype), byref(g.desc()), byref(y.desc()), _ptr(stats), _desc(out), float(slope),
                                _ptr(path_scale), _se_params(se), _ptr(pooled), _ptr(hidden), _ptr(gate), _ptr(mult), _ptr(dadd),
                                _ptr(m12), _ptr(dw1), _ptr(db1), _ptr(dw2), _ptr(db2), *_ws_args(ws), stream_ptr()), "rx_se_gate_bwd")


@hbm("in_gate_act_bwd", _bwd_bytes)
def instnorm_gate_act_bwd(g, y, stats, out, slope, mult, dadd, m12, keep_x, dy, d_residual=None, accumulate_residual=False):
    check(load().rx_instnorm_gate_act_bwd(_code(y.dtype), byref(g.desc()), byref(y.desc()), _ptr(stats), _desc(out), float(slope),
                                          _ptr(mult), _ptr(dadd), _ptr(m12), int(keep_x), byref(dy.desc()), _desc(d_residual),
                                          int(accumulate_residual), stream_ptr()), "rx_instnorm_gate_act_bwd")


# ---- pooling ------------------------------------------------------------------------------------
@hbm("avgpool_fwd", lambda x, y: _tb(x) + _tb(y))
def avgpool_fwd(x, y, stride):
    check(load().rx_avgpool_fwd(_code(x.dtype), byref(x.desc()), byref(y.desc()), I3(*stride), stream_ptr()), "rx_avgpool_fwd")


@hbm("in_act_pool_fwd", lambda y, out, pooled, residual: _tb(y) + _tb(out) + _tb(pooled) + _tb(residual))
def instnorm_act_pool_fwd(y, stats, out, pooled, stride, slope=0.01, residual=None):
    check(load().rx_instnorm_act_pool_fwd(_code(y.dtype), byref(y.desc()), _ptr(stats), _desc(residual), byref(out.desc()),
                                          byref(pooled.desc()), I3(*stride), float(slope), stream_ptr()), "rx_instnorm_act_pool_fwd")


@hbm("avgpool_bwd", lambda dy, dx, accumulate: _tb(dy) + _tb(dx) * (2 if accumulate else 1))
def avgpool_bwd(dy, dx, stride, accumulate=False):
    check(load().rx_avgpool_bwd(_code(dy.dtype), byref(dy.desc()), byref(dx.desc()), I3(*stride), int(accumulate),
                                stream_ptr()), "rx_avgpool_bwd")


# ---- stem / head --------------------------------------------------------------------------------
@hbm("stem_conv_fwd", lambda x_ncdhw, out: x_ncdhw.numel() * 4 + _tb(out))
def stem_conv_fwd(x_ncdhw, w, bias, out, kernel):
    n, cin, z, y, x = x_ncdhw.shape
    assert x_ncdhw.dtype == torch.float32 and x_ncdhw.is_contiguous()
    check(load().rx_stem_conv_fwd(_code(out.dtype), _ptr(x_ncdhw), n, cin, z, y, x, _ptr(w), _ptr(bias),
                                  byref(out.desc()), I3(*kernel), stream_ptr()), "rx_stem_conv_fwd")


@hbm("stem_conv_fwd", lambda x_ncdhw, out: x_ncdhw.numel() * 4 + _tb(out))
def stem_conv_fwd_stats(x_ncdhw, w, bias, out, kernel, stats, eps=1e-5, ws=None):
    """stem conv + InstanceNorm statistics of its output (one pass on the MFMA kernel)"""
    n, cin, z, y, x = x_ncdhw.shape
    assert x_ncdhw.dtype == torch.float32 and x_ncdhw.is_contiguous()
    check(load().rx_stem_conv_fwd_stats(_code(out.dtype), _ptr(x_ncdhw), n, cin, z, y, x, _ptr(w), _ptr(bias),
                                        byref(out.desc()), I3(*kernel), float(eps), _ptr(stats), *_ws_args(ws), stream_ptr()),
          "rx_stem_conv_fwd_stats")


@hbm("stem_conv_bwd_weight", lambda x_ncdhw, dy: x_ncdhw.numel() * 4 + _tb(dy))
def stem_conv_bwd_weight(x_ncdhw, dy, dw, kernel, ws=None):
    n, cin, z, y, x = x_ncdhw.shape
    need = load().rx_stem_conv_bwd_weight_workspace(cin, dy.c, 27)
    ws = workspace(need) if ws is None else ws
    check(load().rx_stem_conv_bwd_weight(_code(dy.dtype), _ptr(x_ncdhw), n, cin, z, y, x, byref(dy.desc()), _ptr(dw),
                                         I3(*kernel), *_ws_args(ws), stream_ptr()), "rx_stem_conv_bwd_weight")


@hbm("head_fwd", lambda x, out_ncdhw: _tb(x) + out_ncdhw.numel() * 4)
def head_fwd(x, w, b, out_ncdhw, act=_l.RX_ACT_NONE):
    k = w.shape[0]
    check(load().rx_head_fwd(_code(x.dtype), byref(x.desc()), _ptr(w), _ptr(b), k, _ptr(out_ncdhw), int(act),
                             stream_ptr()), "rx_head_fwd")


@hbm("head_bwd", lambda dout_ncdhw, x, dx: dout_ncdhw.numel() * 4 + _tb(x) + _tb(dx))
def head_bwd(dout_ncdhw, x, w, dx, dw, db, ws=None):
    k = w.shape[0]
    need = load().rx_head_bwd_workspace(byref(x.desc()), k)
    ws = workspace(need) if ws is None else ws
    check(load().rx_head_bwd(_code(x.dtype), _ptr(dout_ncdhw), byref(x.desc()), _ptr(w), k, _desc(dx), _ptr(dw), _ptr(db),
                             *_ws_args(ws), stream_ptr()), "rx_head_bwd")


@hbm("in_act_head_fwd", lambda y, out, out_ncdhw: _tb(y) + _tb(out) + out_ncdhw.numel() * 4)
def instnorm_act_head_fwd(y, stats, out, w, b, out_ncdhw, act, slope=0.01):
    """InstanceNorm apply + LeakyReLU + the task head's 1x1x1 conv (+ eval activation) in one pass over y"""
    check(load().rx_instnorm_act_head_fwd(_code(y.dtype), byref(y.desc()), _ptr(stats), _desc(out), float(slope), _ptr(w), _ptr(b),
                                          w.shape[0], _ptr(out_ncdhw), int(act), stream_ptr()), "rx_instnorm_act_head_fwd")


@hbm("in_act_bwd_head(colreduce+apply)", lambda dout_ncdhw, y, dy: dout_ncdhw.numel() * 4 + _tb(y) + _tb(dy))
def instnorm_act_bwd_head(dout_ncdhw, w, y, stats, dy, slope=0.01, ws=None, dw=None, db=None):
    """InstanceNorm + LeakyReLU backward of the layer under a task head; the head's data gradient dout x w is formed on the fly.
    dw / db (optional, together): the head's own parameter gradients out of the same reduce pass (the activation is recomputed
    from y) -- head_bwd is then not called at all and the forward need not store the activated output; without them head_bwd is
    called with dx=None"""
    check(load().rx_instnorm_act_bwd_head(_code(y.dtype), _ptr(dout_ncdhw), w.shape[0], _ptr(w), byref(y.desc()), _ptr(stats),
                                          float(slope), byref(dy.desc()), _ptr(dw), _ptr(db), *_ws_args(ws), stream_ptr()),
          "rx_instnorm_act_bwd_head")


@hbm("channel_sum", lambda x: _tb(x))
def channel_sum(x, out, ws=None):
    check(load().rx_channel_sum(_code(x.dtype), byref(x.desc()), _ptr(out), *_ws_args(ws), stream_ptr()), "rx_channel_sum")
