"""What every subject module of `engine.ops` stands on: `Act`, the scratch workspace, the pointer helpers, numbered events and
launch programs, the profiler with its two accounting decorators, the argument checks, and the integer codes the library takes.
The profiler state lives here and nowhere else: read it with `profiling()`."""
import ctypes
import inspect
from ctypes import byref, c_void_p

import numpy as np
import torch

from .. import lib as _l
from ..lib import RxAct, check, load, stream_ptr

_WS = {}
_PROF = None      # optional launch profiler (bench.py): times the conv launches with HIP events on the stream they are enqueued
                  # on and attributes algorithmic FLOPs to kernel instantiations.  A copy of this name goes stale: `profiling()`


def set_profiler(p):
    global _PROF
    _PROF = p


def profiling():
    """the profiler set by `set_profiler`, or None"""
    return _PROF


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

    @staticmethod
    def _timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        return r, e0, e1

    def run(self, name, flops, launches, fn):
        r, e0, e1 = self._timed(fn)
        kind = name.split(":")[0]
        if launches == 1:      # the library tells which instantiation it actually dispatched
            name = kind + ":" + load().rx_last_conv_kernel().decode()
        self.pending.append((name, flops, launches, e0, e1))
        return r

    def run_bytes(self, name, nbytes, fn):
        """an HBM-bound launch (or launch pair): `nbytes` = ALGORITHMIC bytes (every operand tensor touched once at its storage
        type); timed like the convs, on the stream it is enqueued on"""
        r, e0, e1 = self._timed(fn)
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


# ---- accounting: bench.py's `hbm` block (HBM-bound launches against their ALGORITHMIC bytes: every operand tensor touched once at
# its storage type, SURVEY 8(d) -- a statistics pass of its own or the first pass of a two-pass backward is extra TIME, not extra
# bytes) and its `kernels` block (conv FLOPs).  With no profiler set a decorated call costs one wrapper frame and one `is None`.
def timed_bytes(name, nbytes, fn):
    if _PROF is None:
        return fn()
    return _PROF.run_bytes(name, nbytes, fn)


def _tb(a):
    """bytes of one pass over the channels an activation view addresses (0 for None)"""
    return 0 if a is None else a.dims[0] * a.voxels * a.c * a.t.element_size()


def _accounted(formula, report):
    """decorator: under a set profiler a call goes through `report(formula(...), launch)`.  `formula` takes the parameters of the
    decorated function that it NAMES (bound as a call binds them, defaults included -- under a set profiler only); a name the
    function does not have is refused when the module is imported."""
    names = formula.__code__.co_varnames[:formula.__code__.co_argcount]

    def deco(f):
        sig = inspect.signature(f)
        unknown = [n for n in names if n not in sig.parameters]
        if unknown:
            raise TypeError(f"{f.__name__}: the accounting formula reads {unknown}, which are not parameters of the function")

        def wrapped(*a, **k):
            if _PROF is None:
                return f(*a, **k)
            bound = sig.bind(*a, **k)
            bound.apply_defaults()
            return report(formula(*[bound.arguments[n] for n in names]), lambda: f(*a, **k))
        wrapped.__name__, wrapped.__doc__ = f.__name__, f.__doc__
        return wrapped
    return deco


def hbm(label, nbytes):
    """accounts the decorated launch under `label` with `nbytes(<parameters>)` algorithmic bytes"""
    return _accounted(nbytes, lambda n, launch: _PROF.run_bytes(label, n, launch))


def flops(name_and_flops):
    """accounts the decorated single conv launch: `name_and_flops(<parameters>)` -> ("kind:kernel", FLOPs)"""
    return _accounted(name_and_flops, lambda nf, launch: _PROF.run(nf[0], nf[1], 1, launch))


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
        return (c_void_p * len(streams))(*[s.cuda_stream for s in streams])

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
    """host-side handle of a channels-last activation (n, z, y, x, c) living in a torch tensor (n, z, y, x, ld); `slice(c0, c)`
    addresses a channel range of the same buffer (how the decoder's `torch.cat((up, skip), 1)` -- decoder.py:147 -- is eliminated)"""
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


def _desc(a):
    """pointer to the descriptor of an optional `Act` (NULL for None)"""
    return byref(a.desc()) if a is not None else None


def _ws_args(ws):
    """(pointer, bytes) of a scratch tensor; None: the device's shared `workspace()`"""
    ws = workspace() if ws is None else ws
    return c_void_p(ws.data_ptr()), ws.numel()


def _ncv(t):
    n, c = t.shape[0], t.shape[1]
    return n, c, t.numel() // (n * c)


# ---- the integer codes the library takes (include/rxunet.h); the dataloading modules re-export them under these names --------------
INTERP = {"linear": _l.RX_AFFINE_LINEAR, "nearest": _l.RX_AFFINE_NEAREST}
BORDER = {"constant": _l.RX_AFFINE_CONSTANT, "clamp": _l.RX_AFFINE_CLAMP}
RULES = ("copy", "div255", "div65535", "normal_u16", "normal_mul2")      # index == rx_ingest_rule
_U16 = getattr(torch, "uint16", torch.int16)      # the uint16 codes; older torch carries the same bits as int16
# raw voxel types (rx_sw_dtype); int16 is read as the uint16 bits it holds.  Every caller names the subset it accepts.
SW_DTYPE = {torch.uint8: _l.RX_SW_U8, torch.int16: _l.RX_SW_U16, _U16: _l.RX_SW_U16, torch.float32: _l.RX_SW_F32}


def rule_code(rule):
    """a rule's name (or its code) -> the code rx_ingest takes; anything else raises ValueError"""
    if isinstance(rule, str) and rule.lower() in RULES:
        return RULES.index(rule.lower())
    if not isinstance(rule, (bool, str)) and isinstance(rule, (int, np.integer)) and 0 <= int(rule) < len(RULES):
        return int(rule)
    raise ValueError(f"ingest: unknown rule {rule!r} (one of {', '.join(RULES)})")


# ---- argument checks: each takes the calling function's name, so every refusal starts with it ------------------------------------------
FLOATS = tuple(_l.DTYPE_CODE)      # float32, bfloat16, float16


def _names(dtypes):
    return " / ".join(str(d).replace("torch.", "") for d in dtypes)


def device_batch(fn, t, hint, what="batch", dtypes=(torch.float32,), rank=5, or_more=False, layout="(B, C, Z, Y, X)"):
    """refuses, in this order, what is not a device tensor (`hint` tells where the host path is), not of one of `dtypes`, not of
    `rank` dimensions (`or_more`: at least `rank`) or empty -> the tensor made contiguous"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _l.RxError(f"{fn}: the {what} must be a device tensor ({hint})")
    if t.dtype not in dtypes:
        raise _l.RxError(f"{fn}: {what} dtype {t.dtype}: expected a {_names(dtypes)} {layout} {what}")
    if (t.dim() < rank if or_more else t.dim() != rank) or t.numel() == 0:
        raise _l.RxError(f"{fn}: expected a non-empty {_names(dtypes)} {layout} {what}, got {t.dtype} {tuple(t.shape)}")
    return t.contiguous()


def result_tensor(fn, name, t, shape, dtype, device, alloc=torch.empty, same_width=False):
    """`t` None: a new `alloc` (torch.empty / torch.zeros) tensor; else `t` itself, refused unless it is a contiguous `dtype` tensor
    of `shape` on `device`.  `same_width`: any dtype of the same storage width passes -- uint16 results held in int16 storage
    where torch has no uint16."""
    shape = tuple(shape)
    if t is None:
        return alloc(shape, dtype=dtype, device=device)
    if not isinstance(t, torch.Tensor) or t.device != device or tuple(t.shape) != shape or not t.is_contiguous() or (
            t.element_size() != torch.empty((), dtype=dtype).element_size() if same_width else t.dtype != dtype):
        raise _l.RxError(f"{fn}: `{name}` must be a contiguous {_names((dtype,))} tensor of shape {shape} on {device}")
    return t
