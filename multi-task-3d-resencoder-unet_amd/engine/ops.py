"""Thin Python wrappers over the C ABI (one function per entry point of include/rxunet.h).

`Act` is the host-side handle of a channels-last activation `(n, z, y, x, c)` living in a torch
tensor of shape `(n, z, y, x, ld)`; `Act.slice(c0, c)` addresses a channel range of the same
buffer (how the decoder's `torch.cat((up, skip), 1)` -- decoder.py:147 -- is eliminated).
Nothing here computes on the host or with torch ops: every function enqueues HIP kernels on
torch's current stream.
"""
from ctypes import byref, c_int32, c_void_p

import numpy as np
import torch

from . import lib as _l
from .lib import I3, RxAct, check, load, stream_ptr

_WS = {}
_PROF = None      # optional launch profiler (bench.py): times the conv launches with HIP events on the
                  # stream they are enqueued on and attributes algorithmic FLOPs to kernel instantiations


def set_profiler(p):
    global _PROF
    _PROF = p


class LaunchProfiler:
    """HIP-event timing of the MFMA conv launches, grouped by kernel instantiation.  Used only by bench.py;
    costs two event records per launch."""

    def __init__(self):
        self.pending = []
        self.groups = {}
        self.pending_hbm = []
        self.hbm = {}

    @staticmethod
    def igemm_name(vq, co):
        return f"igemm_kernel<{256 if vq > 128 else 128},{64 if co % 64 == 0 else 32}>"

    def run(self, name, flops, launches, fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        kind = name.split(":")[0]
        if launches == 1:      # the library tells which instantiation it actually dispatched
            name = kind + ":" + load().rx_last_conv_kernel().decode()
        self.pending.append((name, flops, launches, e0, e1))

    def run_bytes(self, name, nbytes, fn):
        """an HBM-bound launch (or launch pair): `nbytes` = ALGORITHMIC bytes (every operand tensor touched once at its storage
        type); timed like the convs, on the stream it is enqueued on"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        self.pending_hbm.append((name, float(nbytes), e0, e1))
        return r

    def collect(self):
        torch.cuda.synchronize()
        for name, flops, launches, e0, e1 in self.pending:
            g = self.groups.setdefault(name, dict(ms=0.0, flops=0.0, calls=0, launches=0))
            g["ms"] += e0.elapsed_time(e1)
            g["flops"] += flops
            g["calls"] += 1
            g["launches"] += launches
        self.pending = []
        for name, nbytes, e0, e1 in self.pending_hbm:
            g = self.hbm.setdefault(name, dict(ms=0.0, bytes=0.0, calls=0))
            g["ms"] += e0.elapsed_time(e1)
            g["bytes"] += nbytes
            g["calls"] += 1
        self.pending_hbm = []
        return self.groups


# ---- numbered events + launch programs (include/rxunet.h "launch programs") -------------------------------------------
def event_new():
    return int(load().rx_event_new())


def event_free(slot):
    """hand a numbered event back to the library (programs that mention it must be gone first)"""
    check(load().rx_event_free(int(slot)), "rx_event_free")


def _sp(stream):
    return stream_ptr() if stream is None else c_void_p(stream.cuda_stream)


def event_record(slot, stream=None):
    """record numbered event `slot` on `stream` (default: torch's current stream)"""
    check(load().rx_event_record(slot, _sp(stream)), "rx_event_record")


def stream_wait(slot, stream=None):
    """make `stream` (default: current) wait for the last record of event `slot`"""
    check(load().rx_stream_wait(slot, _sp(stream)), "rx_stream_wait")


class Program:
    """a recorded launch list (rx_prog): `with prog.recording(streams): <ordinary ops calls>` executes AND records them;
    `prog.run(streams)` replays them from C"""

    def __init__(self):
        self.h = c_void_p(load().rx_prog_create())
        self.n = 0

    def __del__(self):
        try:
            if self.h:
                load().rx_prog_destroy(self.h)
        except Exception:
            pass

    @staticmethod
    def _table(streams):
        import ctypes
        return (ctypes.c_void_p * len(streams))(*[s.cuda_stream for s in streams])

    def begin(self, streams):
        check(load().rx_prog_begin(self.h, self._table(streams), len(streams)), "rx_prog_begin")

    def end(self):
        check(load().rx_prog_end(self.h), "rx_prog_end")
        self.n = int(load().rx_prog_len(self.h))

    def __len__(self):
        return int(load().rx_prog_len(self.h))

    def run(self, streams, first=0, last=-1):
        check(load().rx_prog_run(self.h, first, last, self._table(streams), len(streams), None), "rx_prog_run")

    def run_timed(self, streams):
        """profiling replay: per-command milliseconds (HIP events on each command's stream; synchronises)"""
        import ctypes
        ms = (ctypes.c_float * max(self.n, 1))()
        check(load().rx_prog_run(self.h, 0, -1, self._table(streams), len(streams), ms), "rx_prog_run")
        lib = load()
        return [(lib.rx_prog_cmd_name(self.h, i).decode(), lib.rx_prog_cmd_kernel(self.h, i).decode(),
                 int(lib.rx_prog_cmd_stream(self.h, i)), float(ms[i])) for i in range(self.n)]


def workspace(nbytes=None, device=None):
    """One scratch buffer per device, grown on demand (never inside a graph capture)."""
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    need = int(nbytes or 0)
    cur = _WS.get(device)
    if cur is None or cur.numel() < need:
        size = max(need, 192 << 20)
        cur = torch.empty(size, dtype=torch.uint8, device=device)
        _WS[device] = cur
    return cur


class Act:
    __slots__ = ("t", "c0", "c", "root", "plane", "_d")

    def __init__(self, t, c0=0, c=None):
        assert t.dim() == 5 and t.is_contiguous(), "Act wraps a contiguous (n,z,y,x,ld) tensor"
        self.t, self.c0 = t, c0
        self.c = t.shape[4] - c0 if c is None else c
        assert 0 < self.c and c0 + self.c <= t.shape[4]
        self.root, self.plane = None, None      # set for planar concats and their planes (see `planar`)
        self._d = None                          # cached rx_act descriptor (the wrapped storage never moves)

    @staticmethod
    def planar(root, plane=None):
        """`root`: (G, n, z, y, x, 32) contiguous -- a concat of G 32-channel groups kept as G DENSE tensors (rx_act.cs).
        plane=None: the whole concat (c = 32*G; only the 3x3x3 stride-1 conv entry points take it);
        plane=j: group j, an ordinary dense activation that remembers where it lives."""
        assert root.dim() == 6 and root.is_contiguous() and root.shape[5] == 32
        a = Act(root[0 if plane is None else plane])
        a.root, a.plane = root, plane
        if plane is None:
            a.c = 32 * root.shape[0]
        return a

    @property
    def key(self):
        """identity of the underlying buffer (gradient buffers are allocated per buffer, not per view)"""
        return id(self.root) if self.root is not None else id(self.t)

    @property
    def is_planar_cat(self):
        return self.root is not None and self.plane is None

    @property
    def full_buffer(self):
        """does this view address every channel of its buffer?"""
        return self.is_planar_cat or (self.root is None and self.c0 == 0 and self.c == self.t.shape[4])

    @staticmethod
    def empty(n, z, y, x, c, dtype, device="cuda"):
        return Act(torch.empty((n, z, y, x, c), dtype=dtype, device=device))

    @staticmethod
    def zeros(n, z, y, x, c, dtype, device="cuda"):
        return Act(torch.zeros((n, z, y, x, c), dtype=dtype, device=device))

    def slice(self, c0, c):
        if self.is_planar_cat:
            assert c == 32 and c0 % 32 == 0, "a planar concat is sliced plane by plane"
            return Act.planar(self.root, c0 // 32)
        a = Act(self.t, self.c0 + c0, c)
        a.root, a.plane = self.root, self.plane
        return a

    @property
    def dtype(self):
        return self.t.dtype

    @property
    def dims(self):
        return tuple(self.t.shape[:4])

    @property
    def voxels(self):
        s = self.t.shape
        return s[1] * s[2] * s[3]

    def desc(self):
        d = self._d
        if d is None:       # built once: ~2 us of ctypes work per call otherwise, on ~2000 calls per train step
            s = self.t.shape
            if self.is_planar_cat:
                d = RxAct(self.root.data_ptr(), s[0], s[1], s[2], s[3], self.c, 32, self.root.stride(0))
            else:
                d = RxAct(self.t.data_ptr() + self.c0 * self.t.element_size(), s[0], s[1], s[2], s[3], self.c, s[4], 0)
            self._d = d
        return d

    def like(self, root_or_t):
        """the same view (channel range / plane) of another buffer of the same shape (gradient buffers)"""
        if self.root is not None:
            return Act.planar(root_or_t, self.plane)
        return Act(root_or_t, self.c0, self.c)

    def tensor(self):
        """(n, z, y, x, c) view of the addressed channels (for tests / debugging)."""
        if self.is_planar_cat:
            return torch.cat(list(self.root), dim=-1)
        return self.t[..., self.c0:self.c0 + self.c]

    def to_ncdhw(self):
        return self.tensor().permute(0, 4, 1, 2, 3).contiguous()

    @staticmethod
    def from_ncdhw(x, dtype=None):
        return Act(x.permute(0, 2, 3, 4, 1).contiguous().to(dtype or x.dtype))


def _code(dtype):
    return _l.DTYPE_CODE[dtype]


def _ptr(t):
    return c_void_p(t.data_ptr()) if t is not None else c_void_p(0)


def _ws_args(ws):
    return c_void_p(ws.data_ptr()), ws.numel()


# ---- parameter packing ------------------------------------------------------------------------
def pack_conv_weight(w, dtype, w_fwd=None, w_bwd=None, want_fwd=True, want_bwd=True):
    """w: (Co, Ci, kz, ky, kx) fp32 -> (w_fwd [T][Co][Ci], w_bwd [T][Ci][Co]) in `dtype`."""
    co, ci = w.shape[0], w.shape[1]
    taps = w[0, 0].numel()
    if want_fwd and w_fwd is None:
        w_fwd = torch.empty((taps, co, ci), dtype=dtype, device=w.device)
    if want_bwd and w_bwd is None:
        w_bwd = torch.empty((taps, ci, co), dtype=dtype, device=w.device)
    check(load().rx_pack_conv_weight(_code(dtype), _ptr(w), co, ci, taps, _ptr(w_fwd if want_fwd else None),
                                     _ptr(w_bwd if want_bwd else None), stream_ptr()), "rx_pack_conv_weight")
    return w_fwd, w_bwd


def pack_convT_weight(w, dtype, w_fwd=None, w_bwd=None, want_fwd=True, want_bwd=True):
    """w: (Ci, Co, kz, ky, kx) fp32 -> (w_fwd [T][Co][Ci], w_bwd [T][Ci][Co])."""
    ci, co = w.shape[0], w.shape[1]
    taps = w[0, 0].numel()
    if want_fwd and w_fwd is None:
        w_fwd = torch.empty((taps, co, ci), dtype=dtype, device=w.device)
    if want_bwd and w_bwd is None:
        w_bwd = torch.empty((taps, ci, co), dtype=dtype, device=w.device)
    check(load().rx_pack_convT_weight(_code(dtype), _ptr(w), ci, co, taps, _ptr(w_fwd if want_fwd else None),
                                      _ptr(w_bwd if want_bwd else None), stream_ptr()), "rx_pack_convT_weight")
    return w_fwd, w_bwd


def pack_weights_multi(items, dtype):
    """items: [(w fp32 contiguous, kind 0 conv / 1 convT, w_fwd or None, w_bwd or None)] -> ONE launch per 40 tensors
    (rx_pack_multi).  5-D weights (a 2-D net's are unsqueezed by the caller)."""
    import ctypes
    n = len(items)
    if n == 0:
        return
    VP, IA = ctypes.c_void_p * n, ctypes.c_int * n
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
def _taps(kernel):
    return kernel[0] * kernel[1] * kernel[2]


def conv3d_fwd(x, w_fwd, bias, y, kernel, stride, ws=None):
    ws = workspace() if ws is None else ws

    def go():
        check(load().rx_conv3d_fwd(_code(x.dtype), byref(x.desc()), _ptr(w_fwd), _ptr(bias), byref(y.desc()),
                                   I3(*kernel), I3(*stride), *_ws_args(ws), stream_ptr()), "rx_conv3d_fwd")
    if _PROF is None:
        return go()
    n = y.dims[0]
    _PROF.run("fwd:" + LaunchProfiler.igemm_name(y.voxels, y.c), 2.0 * n * y.voxels * y.c * x.c * _taps(kernel), 1, go)


def conv3d_fwd_stats(x, w_fwd, bias, y, kernel, stride, stats, eps=1e-5, ws=None):
    """conv + InstanceNorm statistics of its output (fused into the conv epilogue on the persistent halo kernels)"""
    ws = workspace() if ws is None else ws

    def go():
        check(load().rx_conv3d_fwd_stats(_code(x.dtype), byref(x.desc()), _ptr(w_fwd), _ptr(bias), byref(y.desc()),
                                         I3(*kernel), I3(*stride), float(eps), _ptr(stats), *_ws_args(ws), stream_ptr()),
              "rx_conv3d_fwd_stats")
    if _PROF is None:
        return go()
    n = y.dims[0]
    _PROF.run("fwd:" + LaunchProfiler.igemm_name(y.voxels, y.c), 2.0 * n * y.voxels * y.c * x.c * _taps(kernel), 1, go)


def conv3d_bwd_data(dy, w_bwd, dx, kernel, stride, accumulate=False, ws=None):
    ws = workspace() if ws is None else ws

    def go():
        check(load().rx_conv3d_bwd_data(_code(dy.dtype), byref(dy.desc()), _ptr(w_bwd), byref(dx.desc()), I3(*kernel),
                                        I3(*stride), int(accumulate), *_ws_args(ws), stream_ptr()),
              "rx_conv3d_bwd_data")
    if _PROF is None:
        return go()
    n = dy.dims[0]
    _PROF.run("dgrad:" + LaunchProfiler.igemm_name(dx.voxels, dx.c), 2.0 * n * dy.voxels * dy.c * dx.c * _taps(kernel), 1, go)


def conv3d_bwd_data_instats(dy, w_bwd, dx, kernel, stride, accumulate, in_y, in_stats, slope, m12, ws=None):
    """backward-data that completes dx = dL/d(out of an InstanceNorm layer without residual) and, on the persistent kernel,
    leaves that layer's two backward means in m12.  Returns True when m12 was written (continue with instnorm_act_bwd_apply)."""
    from ctypes import c_int
    ws = workspace() if ws is None else ws
    fused = c_int(0)

    def go():
        check(load().rx_conv3d_bwd_data_instats(_code(dy.dtype), byref(dy.desc()), _ptr(w_bwd), byref(dx.desc()), I3(*kernel),
                                                I3(*stride), int(accumulate), byref(in_y.desc()), _ptr(in_stats), float(slope),
                                                _ptr(m12), byref(fused), *_ws_args(ws), stream_ptr()), "rx_conv3d_bwd_data_instats")
    if _PROF is None:
        go()
    else:
        n = dx.dims[0]
        _PROF.run("dgrad:" + LaunchProfiler.igemm_name(dx.voxels, dx.c), 2.0 * n * dx.voxels * dx.c * dy.c * _taps(kernel), 1, go)
    return bool(fused.value)


def instnorm_act_bwd_apply(g, y, stats, out, dy, m12, slope=0.01, d_residual=None, accumulate_residual=False):
    check(load().rx_instnorm_act_bwd_apply(_code(y.dtype), byref(g.desc()), byref(y.desc()), _ptr(stats),
                                           byref(out.desc()) if out is not None else None, float(slope), _ptr(m12),
                                           byref(dy.desc()),
                                           byref(d_residual.desc()) if d_residual is not None else None,
                                           int(accumulate_residual), stream_ptr()), "rx_instnorm_act_bwd_apply")


def conv3d_bwd_weight(x, dy, dw, kernel, stride, ws=None):
    need = load().rx_conv3d_bwd_weight_workspace(byref(x.desc()), byref(dy.desc()), I3(*kernel))
    ws = workspace(need) if ws is None else ws

    def go():
        check(load().rx_conv3d_bwd_weight(_code(x.dtype), byref(x.desc()), byref(dy.desc()), _ptr(dw), I3(*kernel),
                                          I3(*stride), *_ws_args(ws), stream_ptr()), "rx_conv3d_bwd_weight")
    if _PROF is None:
        return go()
    n = dy.dims[0]
    name = f"wgrad:wgrad_kernel<{64 if dy.c % 64 == 0 else 32},{64 if x.c % 64 == 0 else 32}>"
    _PROF.run(name, 2.0 * n * dy.voxels * dy.c * x.c * _taps(kernel), 1, go)


def convT3d_fwd(x, w_fwd, bias, y, stride, ws=None):
    ws = workspace() if ws is None else ws
    check(load().rx_convT3d_fwd(_code(x.dtype), byref(x.desc()), _ptr(w_fwd), _ptr(bias), byref(y.desc()),
                                I3(*stride), *_ws_args(ws), stream_ptr()), "rx_convT3d_fwd")


def convT3d_bwd_data(dy, w_bwd, dx, stride, accumulate=False, ws=None):
    ws = workspace() if ws is None else ws
    check(load().rx_convT3d_bwd_data(_code(dy.dtype), byref(dy.desc()), _ptr(w_bwd), byref(dx.desc()), I3(*stride),
                                     int(accumulate), *_ws_args(ws), stream_ptr()), "rx_convT3d_bwd_data")


def convT3d_bwd_weight(x, dy, dw, stride, ws=None):
    need = load().rx_convT3d_bwd_weight_workspace(byref(x.desc()), byref(dy.desc()), I3(*stride))
    ws = workspace(need) if ws is None else ws
    check(load().rx_convT3d_bwd_weight(_code(x.dtype), byref(x.desc()), byref(dy.desc()), _ptr(dw), I3(*stride),
                                       *_ws_args(ws), stream_ptr()), "rx_convT3d_bwd_weight")


# ---- InstanceNorm + LeakyReLU + residual -------------------------------------------------------
def instnorm_stats(y, stats, eps=1e-5, ws=None):
    ws = workspace() if ws is None else ws
    check(load().rx_instnorm_stats(_code(y.dtype), byref(y.desc()), eps, _ptr(stats), *_ws_args(ws), stream_ptr()),
          "rx_instnorm_stats")


def instnorm_stats_mask(stats, keep):
    """channel dropout in front of an InstanceNorm: rstd = 0 for the dropped (n, c) planes (see rx_instnorm_stats_mask)"""
    check(load().rx_instnorm_stats_mask(_ptr(stats), _ptr(keep), int(keep.numel()), stream_ptr()), "rx_instnorm_stats_mask")


def instnorm_act_fwd(y, stats, out, slope=0.01, residual=None):
    check(load().rx_instnorm_act_fwd(_code(y.dtype), byref(y.desc()), _ptr(stats),
                                     byref(residual.desc()) if residual is not None else None, byref(out.desc()),
                                     float(slope), stream_ptr()), "rx_instnorm_act_fwd")


def instnorm_fwd(y, stats, out, slope=0.01, residual=None, eps=1e-5, ws=None):
    """stats + apply; a single launch for the low-resolution stages."""
    ws = workspace() if ws is None else ws
    check(load().rx_instnorm_fwd(_code(y.dtype), byref(y.desc()), eps, _ptr(stats),
                                 byref(residual.desc()) if residual is not None else None, byref(out.desc()),
                                 float(slope), *_ws_args(ws), stream_ptr()), "rx_instnorm_fwd")


def instnorm_act_bwd(g, y, stats, out, dy, slope=0.01, d_residual=None, accumulate_residual=False, ws=None):
    ws = workspace() if ws is None else ws
    check(load().rx_instnorm_act_bwd(_code(y.dtype), byref(g.desc()), byref(y.desc()), _ptr(stats),
                                     byref(out.desc()) if out is not None else None, float(slope), byref(dy.desc()),
                                     byref(d_residual.desc()) if d_residual is not None else None,
                                     int(accumulate_residual), *_ws_args(ws), stream_ptr()), "rx_instnorm_act_bwd")


def instnorm_act_bwd_res(g, y, stats, out, dy, d_residual, slope=0.01, pool_dy=None, pool_stride=(1, 1, 1), ws=None):
    """residual-block epilogue backward with the masked gradient written once into `d_residual` (rx_instnorm_act_bwd_res);
    pool_dy: gradient of the next stage's skip-path AvgPool, added on the fly"""
    ws = workspace() if ws is None else ws
    check(load().rx_instnorm_act_bwd_res(_code(y.dtype), byref(g.desc()), byref(y.desc()), _ptr(stats), byref(out.desc()),
                                         float(slope), byref(pool_dy.desc()) if pool_dy is not None else None, I3(*pool_stride),
                                         byref(d_residual.desc()), byref(dy.desc()), *_ws_args(ws), stream_ptr()),
          "rx_instnorm_act_bwd_res")


# ---- SqueezeExcite / DropPath fused with InstanceNorm + residual + LeakyReLU ----------------------
def _se_params(se):
    """se: dict(w1, b1, w2, b2, rd, keep_x) of fp32 device tensors, or None (DropPath only)"""
    if se is None:
        return None
    return byref(_l.RxSeParams(se["w1"].data_ptr(), se["b1"].data_ptr(), se["w2"].data_ptr(), se["b2"].data_ptr(),
                               int(se["rd"]), int(se["keep_x"])))


def se_workspace_bytes(y):
    return load().rx_se_workspace(byref(y.desc()))


def se_gate_fwd(y, stats, se, pooled, hidden, gate, mult, path_scale=None, ws=None):
    ws = workspace(se_workspace_bytes(y)) if ws is None else ws
    check(load().rx_se_gate_fwd(_code(y.dtype), byref(y.desc()), _ptr(stats), _ptr(path_scale), _se_params(se), _ptr(pooled),
                                _ptr(hidden), _ptr(gate), _ptr(mult), *_ws_args(ws), stream_ptr()), "rx_se_gate_fwd")


def instnorm_gate_act_fwd(y, stats, mult, keep_x, out, slope=0.01, residual=None):
    check(load().rx_instnorm_gate_act_fwd(_code(y.dtype), byref(y.desc()), _ptr(stats), _ptr(mult), int(keep_x),
                                          byref(residual.desc()) if residual is not None else None, byref(out.desc()),
                                          float(slope), stream_ptr()), "rx_instnorm_gate_act_fwd")


def se_gate_bwd(g, y, stats, out, slope, se, pooled, hidden, gate, mult, dadd, m12, dw1=None, db1=None, dw2=None, db2=None,
                path_scale=None, ws=None):
    ws = workspace(se_workspace_bytes(y)) if ws is None else ws
    check(load().rx_se_gate_bwd(_code(y.dtype), byref(g.desc()), byref(y.desc()), _ptr(stats),
                                byref(out.desc()) if out is not None else None, float(slope), _ptr(path_scale), _se_params(se),
                                _ptr(pooled), _ptr(hidden), _ptr(gate), _ptr(mult), _ptr(dadd), _ptr(m12), _ptr(dw1), _ptr(db1),
                                _ptr(dw2), _ptr(db2), *_ws_args(ws), stream_ptr()), "rx_se_gate_bwd")


def instnorm_gate_act_bwd(g, y, stats, out, slope, mult, dadd, m12, keep_x, dy, d_residual=None, accumulate_residual=False):
    check(load().rx_instnorm_gate_act_bwd(_code(y.dtype), byref(g.desc()), byref(y.desc()), _ptr(stats),
                                          byref(out.desc()) if out is not None else None, float(slope), _ptr(mult), _ptr(dadd),
                                          _ptr(m12), int(keep_x), byref(dy.desc()),
                                          byref(d_residual.desc()) if d_residual is not None else None,
                                          int(accumulate_residual), stream_ptr()), "rx_instnorm_gate_act_bwd")


# ---- pooling ------------------------------------------------------------------------------------
def avgpool_fwd(x, y, stride):
    check(load().rx_avgpool_fwd(_code(x.dtype), byref(x.desc()), byref(y.desc()), I3(*stride), stream_ptr()),
          "rx_avgpool_fwd")


def instnorm_act_pool_fwd(y, stats, out, pooled, stride, slope=0.01, residual=None):
    check(load().rx_instnorm_act_pool_fwd(_code(y.dtype), byref(y.desc()), _ptr(stats),
                                          byref(residual.desc()) if residual is not None else None, byref(out.desc()),
                                          byref(pooled.desc()), I3(*stride), float(slope), stream_ptr()), "rx_instnorm_act_pool_fwd")


def avgpool_bwd(dy, dx, stride, accumulate=False):
    check(load().rx_avgpool_bwd(_code(dy.dtype), byref(dy.desc()), byref(dx.desc()), I3(*stride), int(accumulate),
                                stream_ptr()), "rx_avgpool_bwd")


# ---- stem / head --------------------------------------------------------------------------------
def stem_conv_fwd(x_ncdhw, w, bias, out, kernel):
    n, cin, z, y, x = x_ncdhw.shape
    assert x_ncdhw.dtype == torch.float32 and x_ncdhw.is_contiguous()
    check(load().rx_stem_conv_fwd(_code(out.dtype), _ptr(x_ncdhw), n, cin, z, y, x, _ptr(w), _ptr(bias),
                                  byref(out.desc()), I3(*kernel), stream_ptr()), "rx_stem_conv_fwd")


def stem_conv_fwd_stats(x_ncdhw, w, bias, out, kernel, stats, eps=1e-5, ws=None):
    """stem conv + InstanceNorm statistics of its output (one pass on the MFMA kernel)"""
    n, cin, z, y, x = x_ncdhw.shape
    assert x_ncdhw.dtype == torch.float32 and x_ncdhw.is_contiguous()
    ws = workspace() if ws is None else ws
    check(load().rx_stem_conv_fwd_stats(_code(out.dtype), _ptr(x_ncdhw), n, cin, z, y, x, _ptr(w), _ptr(bias),
                                        byref(out.desc()), I3(*kernel), float(eps), _ptr(stats), *_ws_args(ws), stream_ptr()),
          "rx_stem_conv_fwd_stats")


def stem_conv_bwd_weight(x_ncdhw, dy, dw, kernel, ws=None):
    n, cin, z, y, x = x_ncdhw.shape
    need = load().rx_stem_conv_bwd_weight_workspace(cin, dy.c, 27)
    ws = workspace(need) if ws is None else ws
    check(load().rx_stem_conv_bwd_weight(_code(dy.dtype), _ptr(x_ncdhw), n, cin, z, y, x, byref(dy.desc()), _ptr(dw),
                                         I3(*kernel), *_ws_args(ws), stream_ptr()), "rx_stem_conv_bwd_weight")


def head_fwd(x, w, b, out_ncdhw, act=_l.RX_ACT_NONE):
    k = w.shape[0]
    check(load().rx_head_fwd(_code(x.dtype), byref(x.desc()), _ptr(w), _ptr(b), k, _ptr(out_ncdhw), int(act),
                             stream_ptr()), "rx_head_fwd")


def head_bwd(dout_ncdhw, x, w, dx, dw, db, ws=None):
    k = w.shape[0]
    need = load().rx_head_bwd_workspace(byref(x.desc()), k)
    ws = workspace(need) if ws is None else ws
    check(load().rx_head_bwd(_code(x.dtype), _ptr(dout_ncdhw), byref(x.desc()), _ptr(w), k,
                             byref(dx.desc()) if dx is not None else None, _ptr(dw), _ptr(db), *_ws_args(ws),
                             stream_ptr()), "rx_head_bwd")


def instnorm_act_head_fwd(y, stats, out, w, b, out_ncdhw, act, slope=0.01):
    """InstanceNorm apply + LeakyReLU + the task head's 1x1x1 conv (+ eval activation) in one pass over y"""
    check(load().rx_instnorm_act_head_fwd(_code(y.dtype), byref(y.desc()), _ptr(stats), byref(out.desc()) if out is not None else None,
                                          float(slope), _ptr(w), _ptr(b), w.shape[0], _ptr(out_ncdhw), int(act), stream_ptr()),
          "rx_instnorm_act_head_fwd")


def instnorm_act_bwd_head(dout_ncdhw, w, y, stats, dy, slope=0.01, ws=None, dw=None, db=None):
    """InstanceNorm + LeakyReLU backward of the layer under a task head; the head's data gradient dout x w is formed on the fly.
    dw / db (optional, together): the head's own parameter gradients out of the same reduce pass (the activation is recomputed
    from y) -- head_bwd is then not called at all and the forward need not store the activated output; without them head_bwd is
    called with dx=None"""
    ws = workspace() if ws is None else ws
    check(load().rx_instnorm_act_bwd_head(_code(y.dtype), _ptr(dout_ncdhw), w.shape[0], _ptr(w), byref(y.desc()), _ptr(stats),
                                          float(slope), byref(dy.desc()), _ptr(dw), _ptr(db), *_ws_args(ws), stream_ptr()),
          "rx_instnorm_act_bwd_head")


def channel_sum(x, out, ws=None):
    ws = workspace() if ws is None else ws
    check(load().rx_channel_sum(_code(x.dtype), byref(x.desc()), _ptr(out), *_ws_args(ws), stream_ptr()),
          "rx_channel_sum")


# ---- task losses (single-pass kernels; loss value and upstream gradient stay on the device) ------
def _ncv(t):
    n, c = t.shape[0], t.shape[1]
    return n, c, t.numel() // (n * c)


def bce_dice_loss_fwd(logits, target, alpha, beta, smoothing=0.1, eps=1e-6):
    """-> (loss: 0-dim fp32 device tensor, coef: (2*C,) fp32 for the backward)"""
    n, c, v = _ncv(logits)
    loss = torch.empty((), dtype=torch.float32, device=logits.device)
    coef = torch.empty(2 * c, dtype=torch.float32, device=logits.device)
    ws = workspace(load().rx_loss_workspace(n, c, v))
    check(load().rx_bce_dice_loss_fwd(_ptr(logits), _ptr(target), n, c, v, alpha, beta, smoothing, eps, _ptr(loss), _ptr(coef),
                                      *_ws_args(ws), stream_ptr()), "rx_bce_dice_loss_fwd")
    return loss, coef


def bce_dice_loss_bwd(logits, target, coef, grad_loss, alpha, beta, smoothing=0.1):
    n, c, v = _ncv(logits)
    dlogits = torch.empty_like(logits)
    check(load().rx_bce_dice_loss_bwd(_ptr(logits), _ptr(target), n, c, v, alpha, beta, smoothing, _ptr(coef), _ptr(grad_loss),
                                      _ptr(dlogits), stream_ptr()), "rx_bce_dice_loss_bwd")
    return dlogits


def masked_cosine_loss_fwd(pred, target):
    n, c, v = _ncv(pred)
    loss = torch.empty((), dtype=torch.float32, device=pred.device)
    coef = torch.empty(1, dtype=torch.float32, device=pred.device)
    ws = workspace(load().rx_loss_workspace(n, c, v))
    check(load().rx_masked_cosine_loss_fwd(_ptr(pred), _ptr(target), n, c, v, _ptr(loss), _ptr(coef), *_ws_args(ws), stream_ptr()),
          "rx_masked_cosine_loss_fwd")
    return loss, coef


def masked_cosine_loss_bwd(pred, target, coef, grad_loss):
    n, c, v = _ncv(pred)
    dpred = torch.empty_like(pred)
    check(load().rx_masked_cosine_loss_bwd(_ptr(pred), _ptr(target), n, c, v, _ptr(coef), _ptr(grad_loss), _ptr(dpred),
                                           stream_ptr()), "rx_masked_cosine_loss_bwd")
    return dpred


_REDUCTION = {"mean": _l.RX_REDUCE_MEAN, "sum": _l.RX_REDUCE_SUM}


def elem_loss_fwd(kind, x, target, reduction="mean", smoothing=0.0, alpha_z=None):
    """element-wise family (kind: lib.RX_LOSS_*) on contiguous fp32 (N, C, *spatial); `alpha_z`: optional (Z,) fp32 device table of
    per-slice smoothing, Z = x.shape[2].  -> loss: 0-dim fp32 device tensor"""
    n, c, v = _ncv(x)
    loss = torch.empty((), dtype=torch.float32, device=x.device)
    ws = workspace(load().rx_loss_workspace(n, c, v))
    check(load().rx_elem_loss_fwd(kind, _ptr(x), _ptr(target), n, c, v, smoothing, _ptr(alpha_z), alpha_z.numel() if alpha_z is not None else 0,
                                  _REDUCTION[reduction], _ptr(loss), *_ws_args(ws), stream_ptr()), "rx_elem_loss_fwd")
    return loss


def elem_loss_bwd(kind, x, target, grad_loss, reduction="mean", smoothing=0.0, alpha_z=None):
    n, c, v = _ncv(x)
    dx = torch.empty_like(x)
    check(load().rx_elem_loss_bwd(kind, _ptr(x), _ptr(target), n, c, v, smoothing, _ptr(alpha_z), alpha_z.numel() if alpha_z is not None else 0,
                                  _REDUCTION[reduction], _ptr(grad_loss), _ptr(dx), stream_ptr()), "rx_elem_loss_bwd")
    return dx


def _ce_targets(target):
    """(target_prob, target_index): float targets are class probabilities, int64 targets class indices"""
    return (None, target) if target.dtype == torch.int64 else (target, None)


def cross_entropy_loss_fwd(logits, target, reduction="mean", ignore_index=-100):
    """logits: contiguous fp32 (N, C, *spatial); target: fp32 of the same shape, or int64 (N, *spatial).
    -> (loss: 0-dim fp32 device tensor, coef: (1,) backward scale, saved: per-voxel lse [and target sum] for the backward)"""
    n, c, v = _ncv(logits)
    tp, ti = _ce_targets(target)
    loss = torch.empty((), dtype=torch.float32, device=logits.device)
    coef = torch.empty(1, dtype=torch.float32, device=logits.device)
    saved = torch.empty((1 if tp is None else 2, n, v), dtype=torch.float32, device=logits.device)
    ws = workspace(load().rx_cross_entropy_loss_workspace(n, c, v))
    check(load().rx_cross_entropy_loss_fwd(_ptr(logits), _ptr(tp), _ptr(ti), ignore_index, n, c, v, _REDUCTION[reduction], _ptr(loss),
                                           _ptr(coef), _ptr(saved), *_ws_args(ws), stream_ptr()), "rx_cross_entropy_loss_fwd")
    return loss, coef, saved


def cross_entropy_loss_bwd(logits, target, coef, saved, grad_loss, ignore_index=-100):
    n, c, v = _ncv(logits)
    tp, ti = _ce_targets(target)
    dlogits = torch.empty_like(logits)
    check(load().rx_cross_entropy_loss_bwd(_ptr(logits), _ptr(tp), _ptr(ti), ignore_index, n, c, v, _ptr(coef), _ptr(saved),
                                           _ptr(grad_loss), _ptr(dlogits), stream_ptr()), "rx_cross_entropy_loss_bwd")
    return dlogits


# ---- training augmentation on the device (dataloading/augment_device.py draws the parameters and packs the table) -------------
def aug_pointwise(image, out, scratch, host_table, table, pool_words):
    """pass 1 on a contiguous fp32 (B, C, Z, Y, X) batch; `host_table`: the pinned / host uint8 tensor holding the same bytes as the
    device tensor `table`; `scratch` None when no sample has a group-3 member"""
    b, c, z, y, x = image.shape
    check(load().rx_aug_pointwise(_ptr(image), _ptr(out), _ptr(scratch) if scratch is not None else None,
                                  scratch.numel() * scratch.element_size() if scratch is not None else 0, b, c, z, y, x,
                                  c_void_p(host_table.data_ptr()), _ptr(table), pool_words, stream_ptr()), "rx_aug_pointwise")


def aug_filter_zy(scratch, out, host_table, table, pool_words):
    """pass 2: the k x k (Z, Y) correlation or the downscale gather, then the dropout boxes, scratch -> out"""
    b, c, z, y, x = out.shape
    check(load().rx_aug_filter_zy(_ptr(scratch), _ptr(out), b, c, z, y, x, c_void_p(host_table.data_ptr()), _ptr(table), pool_words,
                                  stream_ptr()), "rx_aug_filter_zy")


def augment_batch(image, host_table, table, pool_words, any_group3):
    """both passes -> a new batch (allocated on the current stream)"""
    if not image.is_cuda:
        raise _l.RxError("augment_batch: the image batch must be a device tensor")
    out = torch.empty_like(image)
    scratch = None
    if any_group3:
        b, c, z, y, x = image.shape
        assert load().rx_aug_workspace(b, c, z, y, x) == image.numel() * 4
        scratch = torch.empty_like(image)
    aug_pointwise(image, out, scratch, host_table, table, pool_words)
    if any_group3:
        aug_filter_zy(scratch, out, host_table, table, pool_words)
    return out


def geom_table(geom_ops):
    """`geom_ops`: one record per sample -- objects with `.row()` (dataloading.geometry_device.GeomOp) or 12 integers
    (src_axis, flip, ch_src, ch_neg) -> the (B, 12) int32 host image of `rx_geom_sample`"""
    rows = [o.row() if hasattr(o, "row") else o for o in geom_ops]
    table = np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(len(rows), 12))
    return table


def geom_apply(tensor, geom_ops, vector):
    """flips / 90-degree rotations of a float32 (B, C, Z, Y, X) device batch, one record of `geom_ops` per sample -> a new batch
    (allocated on the current stream).  `vector`: the three channels are a vector field and follow the records' component rule."""
    if not isinstance(tensor, torch.Tensor) or not tensor.is_cuda:
        raise _l.RxError("geom_apply: the batch must be a device tensor (the host classes are training/transforms/geometric)")
    if tensor.dim() != 5 or tensor.dtype != torch.float32:
        raise _l.RxError(f"geom_apply: expected a float32 (B, C, Z, Y, X) batch, got {tensor.dtype} {tuple(tensor.shape)}")
    tensor = tensor.contiguous()
    table = geom_table(geom_ops)
    b, c, z, y, x = tensor.shape
    if table.shape[0] != b:
        raise _l.RxError(f"geom_apply: {table.shape[0]} records for a batch of {b}")
    out = torch.empty_like(tensor)
    check(load().rx_geom_apply(_ptr(tensor), _ptr(out), b, c, z, y, x, table.ctypes.data, 1 if vector else 0, stream_ptr()),
          "rx_geom_apply")
    return out


def affine_table(affine_ops):
    """`affine_ops`: one record per sample -- objects with `.row()` (dataloading.spatial_device.AffineOp) or 18 numbers (point,
    then vector, row-major), or a (B, 18) array -> the (B, 18) float32 host image of `rx_affine_sample`"""
    if isinstance(affine_ops, np.ndarray):
        rows = affine_ops
    else:
        rows = [o.row() if hasattr(o, "row") else o for o in affine_ops]
    return np.ascontiguousarray(np.asarray(rows, dtype=np.float32).reshape(len(rows), 18))


def affine_apply(tensor, table, interp, border, fill=0.0, vector=False, out=None):
    """rotation / scaling of a float32 (B, C, Z, Y, X) device batch, one record of `table` (`affine_table`, or what it takes) per
    sample -> a new batch on the current stream, or `out` (a distinct contiguous float32 tensor of the same shape).  `interp`:
    "linear" | "nearest"; `border`: "constant" (outside voxels are `fill`) | "clamp"; `vector`: the three channels are a vector
    field and are turned by the records' `vector` matrices.  dataloading.spatial_device.affine_numpy is the statement."""
    from ..dataloading.spatial_device import BORDER, INTERP
    if not isinstance(tensor, torch.Tensor) or not tensor.is_cuda:
        raise _l.RxError("affine_apply: the batch must be a device tensor (the host path is spatial_device.affine_numpy)")
    if tensor.dim() != 5 or tensor.dtype != torch.float32:
        raise _l.RxError(f"affine_apply: expected a float32 (B, C, Z, Y, X) batch, got {tensor.dtype} {tuple(tensor.shape)}")
    if interp not in INTERP or border not in BORDER:
        raise _l.RxError(f"affine_apply: interp {interp!r} (linear, nearest), border {border!r} (constant, clamp)")
    src = tensor.contiguous()
    table = affine_table(table)
    b, c, z, y, x = src.shape
    if table.shape[0] != b:
        raise _l.RxError(f"affine_apply: {table.shape[0]} records for a batch of {b}")
    if out is None:
        out = torch.empty_like(src)
    elif (not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != torch.float32 or out.shape != src.shape
          or not out.is_contiguous()):
        raise _l.RxError(f"affine_apply: `out` must be a contiguous float32 device tensor of shape {tuple(src.shape)}")
    check(load().rx_affine_apply(_ptr(src), _ptr(out), b, c, z, y, x, table.ctypes.data, INTERP[interp], BORDER[border], float(fill),
                                 1 if vector else 0, stream_ptr()), "rx_affine_apply")
    return out


_ELASTIC_TABLES = {}


def elastic_tables(shape, spacing, device=None):
    """the per-axis B-spline tables of a (Z, Y, X) patch at `spacing` = (sz, sy, sx) (dataloading.elastic_device.bspline_tables) on
    the device: ((idx_z, w_z, dw_z), (idx_y, ...), (idx_x, ...)), int32 [n] and float32 [n, 4] tensors.  Cached per (shape, spacing,
    device): a trainer uploads them once."""
    from ..dataloading.elastic_device import bspline_tables
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if device.type != "cuda":
        raise _l.RxError(f"elastic_tables: {device} is not a device (the host path is elastic_device.elastic_numpy)")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    shape, spacing = tuple(int(v) for v in shape), tuple(int(v) for v in spacing)
    if len(shape) != 3 or len(spacing) != 3 or min(shape) < 1 or min(spacing) < 1:
        raise _l.RxError(f"elastic_tables: shape {shape}, spacing {spacing} (three positive extents, three positive spacings)")
    key = (shape, spacing, device)
    if key not in _ELASTIC_TABLES:
        _ELASTIC_TABLES[key] = tuple(tuple(torch.from_numpy(t).to(device) for t in bspline_tables(n, s)) for n, s in zip(shape, spacing))
    return _ELASTIC_TABLES[key]


def elastic_nodes(fields, device=None):
    """`fields`: one `dataloading.elastic_device.ElasticField` per sample, all with one spacing and one lattice -> the
    (B, 3, Gz, Gy, Gx) float32 device tensor of their nodes: staged in pinned host memory and uploaded with ONE non-blocking copy
    on the current stream, no synchronisation.  Nodes that are not finite are refused here (the device cannot refuse them)."""
    fields = list(fields)
    if not fields or any(not hasattr(f, "nodes") or not hasattr(f, "spacing") for f in fields):
        raise _l.RxError("elastic_nodes: expected a non-empty list of ElasticField")
    sp, shp = tuple(fields[0].spacing), tuple(fields[0].nodes.shape)
    for i, f in enumerate(fields):
        if tuple(f.spacing) != sp or tuple(f.nodes.shape) != shp:
            raise _l.RxError(f"elastic_nodes: field {i} has spacing {tuple(f.spacing)} and nodes {tuple(f.nodes.shape)}, field 0 has "
                             f"{sp} and {shp}: one batch, one lattice")
        if not np.isfinite(f.nodes).all():
            raise _l.RxError(f"elastic_nodes: field {i} has nodes that are not finite")
    host = torch.empty((len(fields),) + shp, dtype=torch.float32, pin_memory=True)
    stage = host.numpy()
    for i, f in enumerate(fields):
        stage[i] = f.nodes
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    return host.to(device, non_blocking=True)


def elastic_apply(tensor, nodes, tables, spacing, interp, border, fill=0.0, vector=False, out=None):
    """B-spline deformation of a float32 (B, C, Z, Y, X) device batch: `nodes` (`elastic_nodes`) the (B, 3, Gz, Gy, Gx) float32
    device lattice, `tables` (`elastic_tables`) for (Z, Y, X) at `spacing` = (sz, sy, sx), each >= 8 -> a new batch on the current
    stream, or `out` (a distinct contiguous float32 tensor of the same shape).  `interp`: "linear" | "nearest"; `border`: "constant"
    (outside voxels are `fill`) | "clamp"; `vector`: the three channels are a normal field (Nx, Ny, Nz) and take the covector
    rule.  dataloading.elastic_device.elastic_numpy is the statement.  The fold guard is the config parser's: nodes of any finite
    size are served, and no load leaves a sample."""
    from ..dataloading.spatial_device import BORDER, INTERP
    if not isinstance(tensor, torch.Tensor) or not tensor.is_cuda:
        raise _l.RxError("elastic_apply: the batch must be a device tensor (the host path is elastic_device.elastic_numpy)")
    if tensor.dim() != 5 or tensor.dtype != torch.float32:
        raise _l.RxError(f"elastic_apply: expected a float32 (B, C, Z, Y, X) batch, got {tensor.dtype} {tuple(tensor.shape)}")
    if interp not in INTERP or border not in BORDER:
        raise _l.RxError(f"elastic_apply: interp {interp!r} (linear, nearest), border {border!r} (constant, clamp)")
    src = tensor.contiguous()
    b, c, z, y, x = src.shape
    try:
        sp = tuple(int(v) for v in spacing)
    except (TypeError, ValueError):
        sp = ()
    if len(sp) != 3 or min(sp) < 1:
        raise _l.RxError(f"elastic_apply: spacing {spacing!r} (three positive ints)")
    want = (b, 3) + tuple((n - 1) // s + 4 for n, s in zip((z, y, x), sp))
    if (not isinstance(nodes, torch.Tensor) or nodes.device != src.device or nodes.dtype != torch.float32 or tuple(nodes.shape) != want
            or not nodes.is_contiguous()):
        got = (nodes.dtype, tuple(nodes.shape), nodes.device) if isinstance(nodes, torch.Tensor) else type(nodes)
        raise _l.RxError(f"elastic_apply: `nodes` must be a contiguous float32 tensor of shape {want} on {src.device}, got {got}")
    ok = isinstance(tables, (tuple, list)) and len(tables) == 3
    for n, ax in zip((z, y, x), tables if ok else ()):
        ok = ok and isinstance(ax, (tuple, list)) and len(ax) == 3 and all(isinstance(t, torch.Tensor) and t.device == src.device
                                                                            and t.is_contiguous() for t in ax)
        ok = ok and ax[0].dtype == torch.int32 and tuple(ax[0].shape) == (n,) and all(t.dtype == torch.float32 and tuple(t.shape) == (n, 4)
                                                                                      for t in ax[1:])
    if not ok:
        raise _l.RxError(f"elastic_apply: `tables` must be elastic_tables(({z}, {y}, {x}), spacing) on {src.device}")
    if out is None:
        out = torch.empty_like(src)
    elif (not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != torch.float32 or out.shape != src.shape
          or not out.is_contiguous()):
        raise _l.RxError(f"elastic_apply: `out` must be a contiguous float32 device tensor of shape {tuple(src.shape)}")
    rec = _l.RxElasticTables(*[t.data_ptr() for ax in tables for t in ax])
    timed_bytes("elastic_apply", 2 * src.numel() * 4,
                lambda: check(load().rx_elastic_apply(_ptr(src), _ptr(out), b, c, z, y, x, _ptr(nodes), I3(*sp), byref(rec), INTERP[interp],
                                                      BORDER[border], float(fill), 1 if vector else 0, stream_ptr()), "rx_elastic_apply"))
    return out


def label_dilate(tensor, radius=5, out=None):
    """binary dilation with the ball of `radius` (1..8) of a float32 (B, C, Z, Y, X) device batch, every (sample, channel) volume
    on its own: 1.0 where a voxel > 0 lies within the radius, else 0.0 (dataloading.dilate_device.dilate_numpy is the statement).
    `out=None`: in place, returns `tensor`; the bit scratch comes from the caching allocator on the current stream."""
    if not isinstance(tensor, torch.Tensor) or not tensor.is_cuda:
        raise _l.RxError("label_dilate: the batch must be a device tensor (the host path is scipy's binary_dilation in the dataset)")
    if tensor.dim() != 5 or tensor.dtype != torch.float32:
        raise _l.RxError(f"label_dilate: expected a float32 (B, C, Z, Y, X) batch, got {tensor.dtype} {tuple(tensor.shape)}")
    src = tensor.contiguous()
    if out is None:
        out = src
    elif (not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != torch.float32 or out.shape != src.shape
          or not out.is_contiguous()):
        raise _l.RxError(f"label_dilate: `out` must be a contiguous float32 device tensor of shape {tuple(src.shape)}")
    b, c, z, y, x = src.shape
    nbytes = load().rx_dilate_workspace(b, c, z, y, x)
    scratch = torch.empty(max(nbytes // 8, 1), dtype=torch.int64, device=src.device)
    check(load().rx_label_dilate(_ptr(src), _ptr(out), _ptr(scratch), nbytes, b, c, z, y, x, int(radius), stream_ptr()),
          "rx_label_dilate")
    if out is src and src is not tensor:      # a non-contiguous batch dilated "in place": hand the values back to its own storage
        tensor.copy_(src)
        return tensor
    return out


def box_stats(vol, boxes):
    """per box (z0, y0, x0, dz, dy, dx) of a contiguous (Z, Y, X) device tensor -- uint8, float32, or uint16 (int16 is read as the
    uint16 bits it holds) -- the count of voxels != 0 and the box-local (minz, maxz, miny, maxy, minx, maxx) of the voxels > 0,
    (dz, -1, dy, -1, dx, -1) where there is none (dataloading.patch_search_device.box_stats_numpy is the statement).  Returns
    (count np.uint64 [N], ext np.int32 [N, 6]) after synchronising the current stream."""
    codes = {torch.uint8: _l.RX_SW_U8, torch.int16: _l.RX_SW_U16, torch.float32: _l.RX_SW_F32}
    if hasattr(torch, "uint16"):
        codes[torch.uint16] = _l.RX_SW_U16
    if not isinstance(vol, torch.Tensor) or not vol.is_cuda:
        raise _l.RxError("box_stats: the volume must be a device tensor (the host statement is patch_search_device.box_stats_numpy)")
    if vol.dtype not in codes:
        raise _l.RxError(f"box_stats: dtype {vol.dtype} (uint8, uint16 / int16 or float32)")
    if vol.dim() != 3 or not vol.is_contiguous():
        raise _l.RxError(f"box_stats: expected a contiguous (Z, Y, X) tensor, got {tuple(vol.shape)} with strides {tuple(vol.stride())}")
    if max(vol.shape) >= (1 << 31):
        raise _l.RxError(f"box_stats: an extent of {tuple(vol.shape)} is beyond int32 (only z * y * x may exceed 2^31)")
    table = np.asarray(boxes)
    if table.ndim != 2 or table.shape[1] != 6 or table.shape[0] < 1 or table.dtype.kind not in "iu":
        raise _l.RxError(f"box_stats: boxes must be an (N, 6) integer array with N >= 1, got {table.dtype} {table.shape}")
    if table.min() < -(1 << 31) or table.max() >= (1 << 31):
        raise _l.RxError("box_stats: a box entry is beyond int32")
    table = np.ascontiguousarray(table, dtype=np.int32)      # read by the copy engine until the synchronise below
    n = len(table)
    z, y, x = vol.shape
    with torch.cuda.device(vol.device):
        nbytes = load().rx_box_stats_workspace(n)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=vol.device)
        count = torch.empty(n, dtype=torch.int64, device=vol.device)
        ext = torch.empty((n, 6), dtype=torch.int32, device=vol.device)
        check(load().rx_box_stats(_ptr(vol), codes[vol.dtype], z, y, x, table.ctypes.data, n, _ptr(ws), nbytes, _ptr(count), _ptr(ext),
                                  stream_ptr()), "rx_box_stats")
        torch.cuda.current_stream().synchronize()
        return count.cpu().numpy().view(np.uint64), ext.cpu().numpy()


def ingest(tensor, rule, out=None):
    """raw patches -> the float32 channel-first batch: a uint8, uint16 or float32 device tensor, (B, Z, Y, X) or channels-last
    (B, Z, Y, X, C) with C <= 8, scaled by `rule` (a name of dataloading.ingest_device.RULES or its code; `ingest_numpy` is the
    statement) into a new (B, C, Z, Y, X) float32 tensor on the current stream (C = 1 for a 4-D input), or into `out`.  A
    non-contiguous input is made contiguous first."""
    from ..dataloading.ingest_device import RULES, rule_code
    codes = {torch.uint8: _l.RX_SW_U8, torch.float32: _l.RX_SW_F32}
    if hasattr(torch, "uint16"):
        codes[torch.uint16] = _l.RX_SW_U16
    if not isinstance(tensor, torch.Tensor) or not tensor.is_cuda:
        raise _l.RxError("ingest: the batch must be a device tensor (the host statement is ingest_device.ingest_numpy)")
    if tensor.dtype not in codes:
        raise _l.RxError(f"ingest: dtype {tensor.dtype} (uint8, uint16 or float32)")
    if tensor.dim() not in (4, 5):
        raise _l.RxError(f"ingest: expected (B, Z, Y, X) or channels-last (B, Z, Y, X, C), got {tuple(tensor.shape)}")
    try:
        code = rule_code(rule)
    except ValueError as e:
        raise _l.RxError(str(e)) from None
    src = tensor.contiguous()
    b, z, y, x = src.shape[:4]
    c = src.shape[4] if src.dim() == 5 else 1
    shape = (b, c, z, y, x)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=src.device)
    elif (not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != torch.float32 or tuple(out.shape) != shape
          or not out.is_contiguous()):
        raise _l.RxError(f"ingest: `out` must be a contiguous float32 device tensor of shape {shape}")
    check(load().rx_ingest(_ptr(src), codes[src.dtype], _ptr(out), b, z, y, x, c, code, stream_ptr()), f"rx_ingest ({RULES[code]})")
    return out


# ---- streaming sliding-window inference (csrc/rx_infer.hip; inference.StreamingInferer is the caller) -----------------------------
# A slab is a contiguous (C, ring, Y, X) device tensor whose ring row r holds the volume row z with z % ring == r.  `origins` is a
# Python list of (z, y, x) patch origins, z an absolute volume row; `views` a list of `GeomOp.row()` records, one per origin.  The
# tables go to the kernels by value: nothing here allocates, copies to the device or synchronises, except `sw_occupancy`'s read.
SW_NORM = {"scale": _l.RX_SW_SCALE, "zscore": _l.RX_SW_ZSCORE}
SW_BLEND = {"average": _l.RX_SW_BLEND_AVERAGE, "unit": _l.RX_SW_BLEND_UNIT, "none": _l.RX_SW_BLEND_NONE}
SW_CAST = {"u8": _l.RX_SW_CAST_U8, "u16": _l.RX_SW_CAST_U16}
SW_ACT = {"none": _l.RX_ACT_NONE, "sigmoid": _l.RX_ACT_SIGMOID, "softmax": _l.RX_ACT_SOFTMAX}
_SW_IN = {torch.uint8: _l.RX_SW_U8, torch.int16: _l.RX_SW_U16, torch.float32: _l.RX_SW_F32}      # int16: the uint16 bits it holds


def _sw_table(fn, rows, n, width):
    flat = [v for r in rows for v in r]
    if len(flat) != n * width:
        raise _l.RxError(f"{fn}: expected {n} records of {width} integers, got {len(flat)} integers")
    return (c_int32 * len(flat))(*flat)


def _sw_slab(fn, slab, dtypes=_SW_IN):
    if not isinstance(slab, torch.Tensor) or not slab.is_cuda or slab.dim() != 4 or not slab.is_contiguous() or slab.dtype not in dtypes:
        raise _l.RxError(f"{fn}: a slab is a contiguous (C, ring, Y, X) device tensor of {[str(d) for d in dtypes]}")
    return slab.shape


def sw_gather_workspace(batch, cin, patch):
    """bytes of fp64 scratch that `sw_gather(norm="zscore")` needs for (batch, cin, *patch) patches"""
    return load().rx_sw_gather_workspace(int(batch), int(cin), *(int(p) for p in patch))


def sw_gather(slab, origins, out, norm, workspace, views=None):
    """the patches at `origins` of an input slab (uint8, int16 holding uint16 bits, float32) -> `out` (B, cin, pz, py, px)
    float32, scaled to [0, 1] (`norm` "scale") and then standardised per patch ("zscore"; `workspace`: a float64 tensor of
    `sw_gather_workspace` bytes).  `views` None: rx_sw_gather; a list of B rows: patch b as its view sees it (rx_sw_gather_geom)."""
    fn = "rx_sw_gather" if views is None else "rx_sw_gather_geom"
    cin, ring, y, x = _sw_slab(fn, slab)
    b, pz, py, px = len(origins), out.shape[2], out.shape[3], out.shape[4]
    if out.dtype != torch.float32 or tuple(out.shape[:2]) != (b, cin) or not out.is_contiguous():
        raise _l.RxError(f"{fn}: `out` must be a contiguous float32 ({b}, {cin}, pz, py, px) tensor, got {out.dtype} {tuple(out.shape)}")
    ws_bytes = workspace.numel() * workspace.element_size() if norm == "zscore" else 0
    head = (_SW_IN[slab.dtype], _ptr(slab), cin, ring, y, x, b, _sw_table(fn, origins, b, 3))
    tail = (pz, py, px, SW_NORM[norm], _ptr(out), _ptr(workspace), ws_bytes, stream_ptr())
    if views is None:
        check(load().rx_sw_gather(*head, *tail), fn)
    else:
        check(load().rx_sw_gather_geom(*head, _sw_table(fn, views, b, 12), *tail), fn)


def sw_accumulate(logits, valid, origins, act, weights, acc, wsum=None, views=None, vector=False):
    """one task's logits (B, c, pz, py, px) float32 -> activation `act` (an RX_ACT code) -> for the first `valid` patches, in
    order: acc (c, ring, Y, X) += weights * p and, where `wsum` (ring, Y, X) is given, wsum += weights.  `views` None:
    rx_sw_accumulate; a list of B rows: each prediction is first moved by its row -- the inverse of the view it was gathered
    with -- and a `vector` task follows the component and sign rule (rx_sw_accumulate_geom)."""
    fn = "rx_sw_accumulate" if views is None else "rx_sw_accumulate_geom"
    c, ring, y, x = _sw_slab(fn, acc, (torch.float32,))
    b, (pz, py, px) = len(origins), weights.shape
    if logits.dtype != torch.float32 or logits.numel() != b * c * pz * py * px or not logits.is_contiguous():
        raise _l.RxError(f"{fn}: expected contiguous float32 logits of ({b}, {c}, {pz}, {py}, {px}), "
                         f"got {logits.dtype} {tuple(logits.shape)}")
    org = _sw_table(fn, origins, b, 3)
    tail = (_ptr(weights), _ptr(acc), _ptr(wsum) if wsum is not None else None, ring, y, x, stream_ptr())
    if views is None:
        check(load().rx_sw_accumulate(_ptr(logits), b, int(valid), c, pz, py, px, org, int(act), *tail), fn)
    else:
        check(load().rx_sw_accumulate_geom(_ptr(logits), b, int(valid), c, pz, py, px, org, _sw_table(fn, views, b, 12),
                                           1 if vector else 0, int(act), *tail), fn)


def sw_finalize(acc, wsum, z0, rows, blend, cast, blended, final, wsum_out=None, reset_wsum=False):
    """volume rows [z0, z0 + rows) of the ring accumulators -> `blended` (c, rows, Y, X) float32 by the rule `blend` ("average",
    "unit", "none") and `final`, its integer cast ("u8" into uint8, "u16" into int16 storage); `wsum_out`: the weight sum of those
    rows.  The rows of `acc` are zeroed after reading, and with `reset_wsum` (the last task that shares `wsum`) those of `wsum`."""
    c, ring, y, x = _sw_slab("rx_sw_finalize", acc, (torch.float32,))
    check(load().rx_sw_finalize(_ptr(acc), _ptr(wsum), c, ring, y, x, int(z0), int(rows), SW_BLEND[blend], SW_CAST[cast],
                                2 if reset_wsum else 1, _ptr(blended), _ptr(final), _ptr(wsum_out) if wsum_out is not None else None,
                                stream_ptr()), "rx_sw_finalize")


def sw_occupancy(slab, origins, patch, value, counts):
    """per origin, the raw voxels of its patch (all channels) with float32(v) > `value`, counted into the device int64 tensor
    `counts` (at least one element per origin); returns them as np.uint64 [N] -- the one read-back of this family."""
    cin, ring, y, x = _sw_slab("rx_sw_occupancy", slab)
    n = len(origins)
    if counts.dtype != torch.int64 or counts.numel() < n or not counts.is_cuda:
        raise _l.RxError(f"rx_sw_occupancy: `counts` must be a device int64 tensor of at least {n} elements")
    pz, py, px = (int(p) for p in patch)
    check(load().rx_sw_occupancy(_SW_IN[slab.dtype], _ptr(slab), cin, ring, y, x, n, _sw_table("rx_sw_occupancy", origins, n, 3),
                                 pz, py, px, float(value), _ptr(counts), stream_ptr()), "rx_sw_occupancy")
    return counts[:n].cpu().numpy().view(np.uint64)


# ---- validation metrics (training/metrics/metrics.py holds the numpy statements and `ValidationMetrics`) --------------------------
def _metric_pred(fn, pred, min_dim=3):
    if not isinstance(pred, torch.Tensor) or not pred.is_cuda:
        raise _l.RxError(f"{fn}: the prediction must be a device tensor (the host statement is training.metrics.{fn}_numpy)")
    if pred.dtype not in _l.DTYPE_CODE:
        raise _l.RxError(f"{fn}: prediction dtype {pred.dtype} (float32, bfloat16 or float16)")
    if pred.dim() < min_dim or pred.numel() == 0:
        raise _l.RxError(f"{fn}: expected a non-empty (N, C, *spatial) prediction, got {tuple(pred.shape)}")
    return pred.contiguous()


def _metric_f32_target(fn, pred, target):
    if not isinstance(target, torch.Tensor) or target.device != pred.device:
        raise _l.RxError(f"{fn}: the target must be a tensor on the prediction's device")
    if target.dtype != torch.float32:
        raise _l.RxError(f"{fn}: target dtype {target.dtype} (float32)")
    if target.shape != pred.shape:
        raise _l.RxError(f"{fn}: target shape {tuple(target.shape)} against prediction shape {tuple(pred.shape)}")
    return target.contiguous()


def _metric_out(fn, name, out, shape, dtype, device):
    if out is None:
        return torch.zeros(shape, dtype=dtype, device=device)
    if (not isinstance(out, torch.Tensor) or out.device != device or out.dtype != dtype or tuple(out.shape) != tuple(shape)
            or not out.is_contiguous()):
        raise _l.RxError(f"{fn}: `{name}` must be a contiguous {dtype} tensor of shape {tuple(shape)} on {device}")
    return out


def seg_counts(pred, target, thr_pred=0.5, thr_target=0.5, out=None):
    """binary confusion per (sample, channel) of a float32 / bfloat16 / float16 (N, C, *spatial) device prediction against a float32
    target of the same shape: int64 (N, C, 3) = (TP, FP, FN) of `pred > thr_pred` against `target > thr_target`, float32 compares,
    a NaN is negative (training.metrics.seg_counts_numpy is the statement).  ADDED into `out` when given (the caller zeroes it),
    else returned in a fresh zeroed tensor; on the current stream, no synchronisation."""
    p = _metric_pred("seg_counts", pred, 2)
    t = _metric_f32_target("seg_counts", p, target)
    n, c, v = _ncv(p)
    out = _metric_out("seg_counts", "out", out, (n, c, 3), torch.int64, p.device)
    timed_bytes("seg_counts", p.numel() * (p.element_size() + 4),
                lambda: check(load().rx_seg_counts(_ptr(p), _code(p.dtype), _ptr(t), n, c, v, float(thr_pred), float(thr_target), _ptr(out),
                                                   stream_ptr()), "rx_seg_counts"))
    return out


def class_counts(pred, target, ignore_index=-100, out=None):
    """multi-class confusion by arg-max over the 2..64 channels of an (N, C, *spatial) device prediction; `target` is float32 class
    probabilities of the same shape or int64 class indices (N, *spatial), where `ignore_index` voxels are skipped: int64 (N, C, 3)
    = per-class (TP, FP, FN) (training.metrics.class_counts_numpy is the statement).  ADDED into `out` when given."""
    p = _metric_pred("class_counts", pred)
    n, c, v = _ncv(p)
    if isinstance(target, torch.Tensor) and target.dtype == torch.int64:
        if target.device != p.device or tuple(target.shape) != (n,) + tuple(p.shape[2:]):
            raise _l.RxError(f"class_counts: index target {tuple(target.shape)} on {target.device} against prediction {tuple(p.shape)} "
                             f"on {p.device}")
        tp, ti, tbytes = None, target.contiguous(), n * v * 8
    else:
        tp, ti, tbytes = _metric_f32_target("class_counts", p, target), None, p.numel() * 4
    out = _metric_out("class_counts", "out", out, (n, c, 3), torch.int64, p.device)
    timed_bytes("class_counts", p.numel() * p.element_size() + tbytes,
                lambda: check(load().rx_class_counts(_ptr(p), _code(p.dtype), _ptr(tp), _ptr(ti), int(ignore_index), n, c, v, _ptr(out),
                                                     stream_ptr()), "rx_class_counts"))
    return out


def normal_stats(pred, target, out=None, ws=None):
    """angular agreement of a 3-channel (N, 3, *spatial) device prediction with a float32 target over the voxels where |target| >
    1e-6: (count int64 (N,), sums float64 (N, 2) = (sum of cos, sum of the angle in degrees)), float32 per voxel, float64 sums in a
    fixed order (training.metrics.normal_stats_numpy is the statement).  ADDED into `out=(count, sums)` when given.  `ws`: a float64
    device tensor of at least `rx_normal_stats_workspace(N, V) / 8` elements for the partials, else one is taken from the allocator."""
    p = _metric_pred("normal_stats", pred)
    t = _metric_f32_target("normal_stats", p, target)
    n, c, v = _ncv(p)
    if c != 3:
        raise _l.RxError(f"normal_stats: expected 3 channels, got {tuple(p.shape)}")
    if out is not None and (not isinstance(out, (tuple, list)) or len(out) != 2):
        raise _l.RxError("normal_stats: `out` must be the pair (count, sums)")
    count = _metric_out("normal_stats", "out[0]", None if out is None else out[0], (n,), torch.int64, p.device)
    sums = _metric_out("normal_stats", "out[1]", None if out is None else out[1], (n, 2), torch.float64, p.device)
    nbytes = load().rx_normal_stats_workspace(n, v)
    if ws is None:
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device=p.device)
    elif not isinstance(ws, torch.Tensor) or ws.device != p.device or ws.dtype != torch.float64 or not ws.is_contiguous():
        raise _l.RxError(f"normal_stats: `ws` must be a contiguous float64 tensor on {p.device}")
    timed_bytes("normal_stats", p.numel() * (p.element_size() + 4),
                lambda: check(load().rx_normal_stats(_ptr(p), _code(p.dtype), _ptr(t), n, v, _ptr(count), _ptr(sums), _ptr(ws), ws.numel() * 8,
                                                     stream_ptr()), "rx_normal_stats"))
    return count, sums


# ---- validation preview (training/visualization/preview.py holds the numpy statements, the config and the GIF writer) -------------
def _preview_vol(fn, vol):
    if not isinstance(vol, torch.Tensor) or not vol.is_cuda:
        raise _l.RxError(f"{fn}: the volume must be a device tensor (the host statement is training.visualization.panel_numpy)")
    if vol.dtype not in _l.DTYPE_CODE:
        raise _l.RxError(f"{fn}: volume dtype {vol.dtype} (float32, bfloat16 or float16)")
    if vol.dim() != 4 or vol.numel() == 0:
        raise _l.RxError(f"{fn}: expected one sample's non-empty (C, Z, H, W) volume, got {tuple(vol.shape)}")
    if not vol.is_contiguous():
        raise _l.RxError(f"{fn}: the sample must be contiguous (strides {vol.stride()} for shape {tuple(vol.shape)})")
    return vol


def _preview_launch(vol, frames, y0, x0, z_step, sigmoid, minmax):
    c, z, h, w = vol.shape
    check(load().rx_preview_panel(_ptr(vol), _code(vol.dtype), c, z, h, w, z_step, 1 if sigmoid else 0, _ptr(frames), frames.stride(0),
                                  frames.stride(1), y0, x0, _ptr(minmax), stream_ptr()), "rx_preview_panel")


def _preview_bytes(vol, z_step):
    c, z, h, w = vol.shape
    zk = -(-z // z_step)
    return zk * h * w * ((3 if c == 3 else 1) * vol.element_size() + 3)


def preview_panel(vol4, frames, y0, x0, z_step=1, sigmoid=False, minmax=None):
    """draws one sample's (C, Z, H, W) float32 / bfloat16 / float16 device volume into the uint8 device frames (Zf, Hf, Wf, 3) (rows and
    pixels packed: strides (*, *, 3, 1)): the panel of kept slice j = source slice j * z_step occupies rows y0 .. y0 + H and
    columns x0 .. x0 + W of frame j; nothing else is written.  Every slice of every drawn channel is scaled to its own range
    (training.visualization.panel_numpy is the statement; `sigmoid` draws 1 / (1 + exp(-v))).  `minmax`: an optional contiguous
    float32 (c_drawn, Zk, 2) device tensor that receives (lo, hi).  On the current stream, no synchronisation; returns `frames`."""
    vol = _preview_vol("preview_panel", vol4)
    c, z, h, w = vol.shape
    z_step, y0, x0 = int(z_step), int(y0), int(x0)
    if z_step < 1 or y0 < 0 or x0 < 0:
        raise _l.RxError(f"preview_panel: z_step must be >= 1 and y0, x0 >= 0 (got z_step={z_step} y0={y0} x0={x0})")
    zk = -(-z // z_step)
    if (not isinstance(frames, torch.Tensor) or frames.device != vol.device or frames.dtype != torch.uint8 or frames.dim() != 4
            or frames.shape[3] != 3 or frames.stride(3) != 1 or frames.stride(2) != 3):
        raise _l.RxError(f"preview_panel: `frames` must be a uint8 (Z, H, W, 3) tensor with packed pixels on {vol.device}")
    if frames.shape[0] < zk or frames.shape[1] < y0 + h or frames.shape[2] < x0 + w:
        raise _l.RxError(f"preview_panel: a {zk} x {h} x {w} panel at (y0={y0}, x0={x0}) does not fit frames of shape {tuple(frames.shape)}")
    if minmax is not None:
        shape = (3 if c == 3 else 1, zk, 2)
        if (not isinstance(minmax, torch.Tensor) or minmax.device != vol.device or minmax.dtype != torch.float32
                or tuple(minmax.shape) != shape or not minmax.is_contiguous()):
            raise _l.RxError(f"preview_panel: `minmax` must be a contiguous float32 tensor of shape {shape} on {vol.device}")
    timed_bytes("preview_panel", _preview_bytes(vol, z_step), lambda: _preview_launch(vol, frames, y0, x0, z_step, sigmoid, minmax))
    return frames


def preview_frames(image, targets, preds, sample=0, every=1, sigmoid_tasks=(), out=None):
    """the frames of the validation preview of one sample of a batch: image (B, C, Z, H, W), targets / preds {task: (B, C, Z, H, W)}
    device tensors -> uint8 (Zk, 2H, (1 + T)W, 3) on the device, Zk = ceil(Z / every): the input panel and one target panel per task
    (sorted by name) above a blank tile and the prediction panels (training.visualization.frames_numpy is the statement).  One
    rx_preview_panel launch per panel on the current stream, no synchronisation.  The tensor is zeroed when it is created and the
    blank tile is never written, so `out` -- a tensor an earlier call of the same shapes returned -- is reused as it is."""
    names = sorted(targets)
    vols = [("image", image, False)] + [(f"targets['{n}']", targets[n], False) for n in names]
    for n in names:
        if n not in preds:
            raise _l.RxError(f"preview_frames: no prediction for task '{n}'")
        vols.append((f"preds['{n}']", preds[n], None))
    sample, every = int(sample), int(every)
    if every < 1:
        raise _l.RxError(f"preview_frames: every must be >= 1 (got {every})")
    samples = []
    for label, t, _ in vols:
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise _l.RxError(f"preview_frames: {label} must be a device tensor")
        if t.dim() != 5:
            raise _l.RxError(f"preview_frames: {label}: expected (B, C, Z, H, W), got {tuple(t.shape)} (2-D patches have no slices to page through)")
        if not 0 <= sample < t.shape[0]:
            raise _l.RxError(f"preview_frames: sample {sample} of a batch of {t.shape[0]}")
        samples.append(_preview_vol("preview_frames", t[sample]))
    z, h, w = samples[0].shape[1:]
    for (label, _, _), s in zip(vols, samples):
        if tuple(s.shape[1:]) != (z, h, w) or s.device != samples[0].device:
            raise _l.RxError(f"preview_frames: {label} is {tuple(s.shape[1:])} on {s.device}, the image {(z, h, w)} on {samples[0].device}")
    t_n = len(names)
    shape = (-(-z // every), 2 * h, (1 + t_n) * w, 3)
    if out is None:
        out = torch.zeros(shape, dtype=torch.uint8, device=samples[0].device)
    elif (not isinstance(out, torch.Tensor) or out.device != samples[0].device or out.dtype != torch.uint8 or tuple(out.shape) != shape
          or not out.is_contiguous()):
        raise _l.RxError(f"preview_frames: `out` must be a contiguous uint8 tensor of shape {shape} on {samples[0].device}")

    def run():
        for i, s in enumerate(samples):
            row, col = divmod(i, 1 + t_n) if i <= t_n else (1, i - t_n)
            sig = i > t_n and names[i - t_n - 1] in sigmoid_tasks and s.shape[0] == 1
            _preview_launch(s, out, row * h, col * w, every, sig, None)
    timed_bytes("preview_frames", sum(_preview_bytes(s, every) for s in samples), run)
    return out


# ---- mesh targets (csrc/rx_meshslice.hip; the statements live in tasks/normals/mesh_targets.py) -------------------------------
_U16 = getattr(torch, "uint16", torch.int16)      # the uint16 codes; older torch carries the same bits as int16
_MESH_MAX_COORD = float(1 << 24)


def _mesh_check(who, vertices, triangles, normals, w, h, z0, nz, window):
    """the refusals the library cannot make (it never reads device data on the host) -> (y0, x0, wh, ww)"""
    _l.require_device()
    if not isinstance(vertices, torch.Tensor) or not isinstance(triangles, torch.Tensor):
        raise _l.RxError(f"{who}: `vertices` and `triangles` must be device tensors")
    dev = vertices.device
    for name, t, dt in (("vertices", vertices, torch.float32), ("triangles", triangles, torch.int32), ("normals", normals, torch.float32)):
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != dev or t.dtype != dt or t.dim() != 2 or t.shape[1] != 3 \
                or not t.is_contiguous():
            raise _l.RxError(f"{who}: `{name}` must be a contiguous {dt} (n, 3) device tensor")
    if vertices.shape[0] < 1:
        raise _l.RxError(f"{who}: no vertices")
    if normals is not None and normals.shape != vertices.shape:
        raise _l.RxError(f"{who}: `normals` must match `vertices` {tuple(vertices.shape)}")
    if not bool(torch.isfinite(vertices).all()) or (normals is not None and not bool(torch.isfinite(normals).all())):
        raise _l.RxError(f"{who}: vertices and normals must be finite")
    if float(vertices.abs().max()) >= _MESH_MAX_COORD:
        raise _l.RxError(f"{who}: coordinates at or beyond 2^24 are not supported on the device")
    if triangles.shape[0] and (int(triangles.min()) < 0 or int(triangles.max()) >= vertices.shape[0]):
        raise _l.RxError(f"{who}: triangle indices must lie in [0, {vertices.shape[0]})")
    y0, x0, wh, ww = (0, 0, h, w) if window is None else (int(a) for a in window)
    if w < 1 or h < 1 or nz < 1 or y0 < 0 or x0 < 0 or wh < 1 or ww < 1 or y0 + wh > h or x0 + ww > w:
        raise _l.RxError(f"{who}: window {(y0, x0, wh, ww)} / slab of {nz} slices does not fit the {w} x {h} image")
    return y0, x0, wh, ww


def _mesh_out(who, out, name, shape, dtype, device):
    t = None if out is None else out.get(name)
    if t is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if not isinstance(t, torch.Tensor) or t.device != device or t.element_size() != torch.empty((), dtype=dtype).element_size() \
            or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise _l.RxError(f"{who}: out[{name!r}] must be a contiguous {dtype} tensor of shape {tuple(shape)} on {device}")
    return t


def mesh_slice_normals(vertices, triangles, normals, w, h, z0, nz, window=None, exp_factor=1.5, want_viz=False, want_mask=False,
                       keys=None, out=None):
    """slices [z0, z0 + nz) of the meshes' interpolated vertex normals, window (y0, x0, wh, ww) of the w x h image ->
    {"normals": uint16 (nz, wh, ww, 3), "keys": int64 (nz, wh, ww) order keys[, "viz": uint8 (nz, wh, ww, 3)][, "mask": uint8
    (nz, wh, ww)]}, equal to tasks/normals/mesh_targets.py: slice_normals_numpy slice by slice.  `keys`: a reusable int64 buffer of
    that shape (cleared here); `out`: optional preallocated result tensors by name."""
    who = "mesh_slice_normals"
    y0, x0, wh, ww = _mesh_check(who, vertices, triangles, normals, w, h, z0, nz, window)
    if normals is None:
        raise _l.RxError(f"{who}: `normals` is required")
    dev = vertices.device
    keys = _mesh_out(who, {"keys": keys}, "keys", (nz, wh, ww), torch.int64, dev)
    keys.zero_()
    res = {"keys": keys, "normals": _mesh_out(who, out, "normals", (nz, wh, ww, 3), _U16, dev)}
    if want_viz:
        res["viz"] = _mesh_out(who, out, "viz", (nz, wh, ww, 3), torch.uint8, dev)
    if want_mask:
        res["mask"] = _mesh_out(who, out, "mask", (nz, wh, ww), torch.uint8, dev)
    lib, st = load(), stream_ptr()
    geom = (int(w), int(h), int(z0), int(nz), y0, x0, wh, ww)
    check(lib.rx_mesh_slice_keys(0, _ptr(vertices), vertices.shape[0], _ptr(triangles), triangles.shape[0], _ptr(normals), *geom,
                                 float(exp_factor), _ptr(keys), st), "rx_mesh_slice_keys")
    check(lib.rx_mesh_resolve_normals(_ptr(keys), _ptr(vertices), vertices.shape[0], _ptr(triangles), triangles.shape[0], _ptr(normals), *geom,
                                      _ptr(res["normals"]), _ptr(res.get("viz")), _ptr(res.get("mask")), st), "rx_mesh_resolve_normals")
    return res


def mesh_slice_labels(vertices, triangles, tri_labels, w, h, z0, nz, window=None, want_mask=False, keys=None, out=None):
    """slices [z0, z0 + nz) of per-triangle labels (`tri_labels`: int32 device tensor, values in [0, 65535]) ->
    {"labels": uint16 (nz, wh, ww), "keys": int32 (nz, wh, ww)[, "mask": uint8 (nz, wh, ww)]}, equal to
    tasks/normals/mesh_targets.py: slice_labels_numpy slice by slice"""
    who = "mesh_slice_labels"
    y0, x0, wh, ww = _mesh_check(who, vertices, triangles, None, w, h, z0, nz, window)
    dev = vertices.device
    if not isinstance(tri_labels, torch.Tensor) or tri_labels.device != dev or tri_labels.dtype != torch.int32 \
            or tuple(tri_labels.shape) != (triangles.shape[0],) or not tri_labels.is_contiguous():
        raise _l.RxError(f"{who}: `tri_labels` must be a contiguous int32 ({triangles.shape[0]},) device tensor")
    if tri_labels.numel() and (int(tri_labels.min()) < 0 or int(tri_labels.max()) > 65535):
        raise _l.RxError(f"{who}: labels must lie in [0, 65535]")
    keys = _mesh_out(who, {"keys": keys}, "keys", (nz, wh, ww), torch.int32, dev)
    keys.zero_()
    res = {"keys": keys, "labels": _mesh_out(who, out, "labels", (nz, wh, ww), _U16, dev)}
    if want_mask:
        res["mask"] = _mesh_out(who, out, "mask", (nz, wh, ww), torch.uint8, dev)
    lib, st = load(), stream_ptr()
    check(lib.rx_mesh_slice_keys(1, _ptr(vertices), vertices.shape[0], _ptr(triangles), triangles.shape[0], None, int(w), int(h), int(z0),
                                 int(nz), y0, x0, wh, ww, 0.0, _ptr(keys), st), "rx_mesh_slice_keys")
    check(lib.rx_mesh_resolve_labels(_ptr(keys), _ptr(tri_labels), triangles.shape[0], nz * wh * ww, _ptr(res["labels"]),
                                     _ptr(res.get("mask")), st), "rx_mesh_resolve_labels")
    return res


def aug_philox_u32(key, n, device):
    """test hook: the raw Philox4x32-10 outputs behind the noise of voxels 0..n-1 -> int64 tensor of the uint32 values"""
    out = torch.empty(n, dtype=torch.int32, device=device)
    check(load().rx_aug_philox_u32(int(key), n, _ptr(out), stream_ptr()), "rx_aug_philox_u32")
    return out.to(torch.int64) & 0xFFFFFFFF


# ---- bench.py's `hbm` block: the HBM-bound launches timed against their ALGORITHMIC bytes ---------------------------
# (every operand tensor touched once at its storage type, SURVEY 8(d): a standalone statistics pass or the first pass of a
# two-pass backward is extra TIME, not extra algorithmic bytes).  Wrappers cost one Python call when no profiler is set.
def timed_bytes(name, nbytes, fn):
    if _PROF is None:
        return fn()
    return _PROF.run_bytes(name, nbytes, fn)


def _tb(a):
    """bytes of one pass over the channels an activation view addresses (0 for None)"""
    return 0 if a is None else a.dims[0] * a.voxels * a.c * a.t.element_size()


def _hbm(label, nbytes):
    def deco(f):
        def wrapped(*a, **k):
            if _PROF is None:
                return f(*a, **k)
            return _PROF.run_bytes(label, nbytes(*a, **k), lambda: f(*a, **k))
        wrapped.__name__, wrapped.__doc__ = f.__name__, f.__doc__
        return wrapped
    return deco


def _bwd_bytes(g, y, out, dy, d_residual, acc):
    return _tb(g) + _tb(y) + _tb(dy) + _tb(out) + _tb(d_residual) * (2 if acc else 1)


def _pack_bytes(w, dtype, w_fwd=None, w_bwd=None, want_fwd=True, want_bwd=True):
    e = torch.empty((), dtype=dtype).element_size()
    return w.numel() * (4 + (e if want_fwd else 0) + (e if want_bwd else 0))


instnorm_stats = _hbm("in_stats(colreduce)", lambda y, stats, eps=1e-5, ws=None: _tb(y))(instnorm_stats)
instnorm_act_fwd = _hbm("in_act_fwd", lambda y, stats, out, slope=0.01, residual=None: _tb(y) + _tb(out) + _tb(residual))(instnorm_act_fwd)
instnorm_fwd = _hbm("in_fwd(stats+apply)", lambda y, stats, out, slope=0.01, residual=None, eps=1e-5, ws=None:
                    _tb(y) + _tb(out) + _tb(residual))(instnorm_fwd)
instnorm_act_bwd = _hbm("in_act_bwd(colreduce+apply)",
                        lambda g, y, stats, out, dy, slope=0.01, d_residual=None, accumulate_residual=False, ws=None:
                        _bwd_bytes(g, y, out, dy, d_residual, accumulate_residual))(instnorm_act_bwd)
instnorm_act_bwd_res = _hbm("in_act_bwd_res(colreduce+apply)",
                            lambda g, y, stats, out, dy, d_residual, slope=0.01, pool_dy=None, pool_stride=(1, 1, 1), ws=None:
                            _tb(g) + _tb(y) + _tb(out) + _tb(dy) + _tb(d_residual) + _tb(pool_dy))(instnorm_act_bwd_res)
instnorm_act_bwd_apply = _hbm("in_act_bwd_apply",
                              lambda g, y, stats, out, dy, m12, slope=0.01, d_residual=None, accumulate_residual=False:
                              _bwd_bytes(g, y, out, dy, d_residual, accumulate_residual))(instnorm_act_bwd_apply)
se_gate_fwd = _hbm("se_gate_fwd(linesum+gate)", lambda y, *a, **k: _tb(y))(se_gate_fwd)
instnorm_gate_act_fwd = _hbm("in_gate_act_fwd", lambda y, stats, mult, keep_x, out, slope=0.01, residual=None:
                             _tb(y) + _tb(out) + _tb(residual))(instnorm_gate_act_fwd)
se_gate_bwd = _hbm("se_gate_bwd(linesums+gate)", lambda g, y, stats, out, *a, **k: _tb(g) + _tb(y) + _tb(out))(se_gate_bwd)
instnorm_gate_act_bwd = _hbm("in_gate_act_bwd",
                             lambda g, y, stats, out, slope, mult, dadd, m12, keep_x, dy, d_residual=None, accumulate_residual=False:
                             _bwd_bytes(g, y, out, dy, d_residual, accumulate_residual))(instnorm_gate_act_bwd)
avgpool_fwd = _hbm("avgpool_fwd", lambda x, y, stride: _tb(x) + _tb(y))(avgpool_fwd)
instnorm_act_pool_fwd = _hbm("in_act_pool_fwd", lambda y, stats, out, pooled, stride, slope=0.01, residual=None:
                             _tb(y) + _tb(out) + _tb(pooled) + _tb(residual))(instnorm_act_pool_fwd)
avgpool_bwd = _hbm("avgpool_bwd", lambda dy, dx, stride, accumulate=False: _tb(dy) + _tb(dx) * (2 if accumulate else 1))(avgpool_bwd)
head_fwd = _hbm("head_fwd", lambda x, w, b, out_ncdhw, act=0: _tb(x) + out_ncdhw.numel() * 4)(head_fwd)
head_bwd = _hbm("head_bwd", lambda dout_ncdhw, x, w, dx, dw, db, ws=None: dout_ncdhw.numel() * 4 + _tb(x) + _tb(dx))(head_bwd)
instnorm_act_head_fwd = _hbm("in_act_head_fwd", lambda y, stats, out, w, b, out_ncdhw, act, slope=0.01:
                             _tb(y) + _tb(out) + out_ncdhw.numel() * 4)(instnorm_act_head_fwd)
instnorm_act_bwd_head = _hbm("in_act_bwd_head(colreduce+apply)", lambda dout_ncdhw, w, y, stats, dy, slope=0.01, ws=None, dw=None, db=None:
                             dout_ncdhw.numel() * 4 + _tb(y) + _tb(dy))(instnorm_act_bwd_head)
channel_sum = _hbm("channel_sum", lambda x, out, ws=None: _tb(x))(channel_sum)
pack_conv_weight = _hbm("pack", _pack_bytes)(pack_conv_weight)
pack_convT_weight = _hbm("pack", _pack_bytes)(pack_convT_weight)
stem_conv_fwd = _hbm("stem_conv_fwd", lambda x_ncdhw, w, bias, out, kernel: x_ncdhw.numel() * 4 + _tb(out))(stem_conv_fwd)
stem_conv_fwd_stats = _hbm("stem_conv_fwd", lambda x_ncdhw, w, bias, out, kernel, stats, eps=1e-5, ws=None: x_ncdhw.numel() * 4 + _tb(out))(stem_conv_fwd_stats)
stem_conv_bwd_weight = _hbm("stem_conv_bwd_weight", lambda x_ncdhw, dy, dw, kernel, ws=None: x_ncdhw.numel() * 4 + _tb(dy))(stem_conv_bwd_weight)
convT3d_fwd = _hbm("convT_fwd", lambda x, w_fwd, bias, y, stride, ws=None: _tb(x) + _tb(y))(convT3d_fwd)
convT3d_bwd_data = _hbm("convT_bwd_data", lambda dy, w_bwd, dx, stride, accumulate=False, ws=None:
                        _tb(dy) + _tb(dx) * (2 if accumulate else 1))(convT3d_bwd_data)
convT3d_bwd_weight = _hbm("convT_bwd_weight", lambda x, dy, dw, stride, ws=None: _tb(x) + _tb(dy))(convT3d_bwd_weight)
