"""A recording proxy for the `ops` module that engine/plan.py sees (a plain module, used by tests/test_plan_audit_gpu.py).

`install(monkeypatch, net)` replaces the name `ops` in the plan module.  Every launch a plan then issues goes through
`OpsAudit._call`: synchronise, snapshot what the launch reads (fp64 on the CPU, an `Act` through its own `to_ncdhw()` view, the old
contents of every destination included), make the real call, synchronise, and hand both snapshots to the auditor registered for
that op name.  An auditor computes the fp64 reference FROM THE BYTES THE LAUNCH READ and applies the bound the op tests use
(tests/op_bounds.py, tests/norm_bounds.py): LeakyReLU mask flips upstream, which make an end-to-end 16-bit comparison loose, do not
enter.  A launch without an auditor is a failure that names the op, so a new fused entry point cannot enter a plan unaudited.

Stale state: the proxy records what the forward and the backward launches write.  `begin(phase, strict=True)` fills those buffers
with NaN before the pass (backward-written buffers that share storage with a forward-written one are live activations and stay;
packed weights, parameters and the input are never touched), and every strict launch must then read only finite values and leave
only finite values behind -- whatever was not produced in this pass is NaN and names the launch that read it.

Failures are collected per launch, in launch order, and raised by `check()` at the end of the pass."""
import sys

import torch
import torch.nn.functional as F

from exact_ops import U32, assert_within, gamma, half_ulp
from norm_bounds import (_mr, check_dres, check_norm_bwd, check_norm_bwd_res, check_norm_fwd, check_stats, lrelu_mask)
from op_bounds import (check, check_m12, head_dx_ref, head_grads_ref, head_logits_ref, pool_bwd_bound, pool_fwd_bound)

# attributes of `ops` that launch nothing: the handle class, the scratch buffer, numbered events, the profiler hook
PASS_THROUGH = {"Act", "workspace", "event_new", "event_free", "event_record", "stream_wait", "profiling", "set_profiler",
                "Program", "LaunchProfiler", "se_workspace_bytes"}
DW5 = ("co", "ci", "kz", "ky", "kx")


def _snap(v):
    if hasattr(v, "to_ncdhw"):
        return v.to_ncdhw().detach().double().cpu()
    if torch.is_tensor(v):
        return v.detach().double().cpu().clone()
    if isinstance(v, (list, tuple)) and any(torch.is_tensor(i) or isinstance(i, (list, tuple)) for i in v):
        return [_snap(i) for i in v]
    return v


def _finite(v):
    if torch.is_tensor(v):
        return bool(torch.isfinite(v).all())
    if isinstance(v, list):
        return all(_finite(i) for i in v)
    return True


def _pad(k):
    return [(kk - 1) // 2 for kk in k]


def _lrelu64(y, stats, slope, dtype):
    """the activated output of a plain layer that the launch did not store, in fp64, with a bound of what the kernel holds in its
    place: check_norm_fwd's fp32 bound e32 (5 roundings), once more for an element within e32 of 0 that took the other LeakyReLU
    branch (the two branches differ by (1 - slope) |pre| < e32 there), and the rounding into the storage type"""
    mean, rstd = _mr(stats, *y.shape[:2])
    t = (y - mean) * rstd
    a = t if slope == 1.0 else torch.where(t > 0, t, t * slope)
    e32 = 5 * U32 * t.abs()
    return a, 2 * e32 + half_ulp(a.abs() + e32, dtype)


# ---- auditors: (signature, reads, writes, {destination: accumulate flag}, check) ---------------------------------------------------
def a_conv_fwd(A, tag, args, pre, post, ret):
    x, w, b = pre["x"], pre["w_fwd"], pre["bias"]
    k, s = list(args["kernel"]), list(args["stride"])
    T, co, ci = w.shape
    W = w.view(*k, co, ci).permute(3, 4, 0, 1, 2)
    ref = F.conv3d(x, W, b, stride=s, padding=_pad(k))
    a = F.conv3d(x.abs(), W.abs(), None if b is None else b.abs(), stride=s, padding=_pad(k))
    check(post["y"], ref, a, ci * T + (b is not None), args["x"].dtype, f"{tag} y")
    if "stats" in post:
        check_stats(post["stats"], post["y"], args["eps"], what=f"{tag} stats")
        A.last_stats = args["stats"].data_ptr()


def a_conv_bwd_data(A, tag, args, pre, post, ret):
    dy, w, old = pre["dy"], pre["w_bwd"], pre["dx"]
    k, s = list(args["kernel"]), list(args["stride"])
    T, ci, co = w.shape
    W = w.view(*k, ci, co).permute(4, 3, 0, 1, 2)
    ref = torch.nn.grad.conv3d_input(old.shape, W, dy, stride=s, padding=_pad(k))
    a = torch.nn.grad.conv3d_input(old.shape, W.abs(), dy.abs(), stride=s, padding=_pad(k))
    terms, dtype = co * T, args["dy"].dtype
    if args["accumulate"]:
        ref, a, terms = ref + old, a + old.abs(), terms + 1
    check(post["dx"], ref, a, terms, dtype, f"{tag} dx{' +=' if args['accumulate'] else ''}")
    if "m12" in args:
        A.instats[args["m12"].data_ptr()] = bool(ret)
        if ret:
            mean, rstd = _mr(pre["in_stats"], *pre["in_y"].shape[:2])
            check_m12(post["m12"], post["dx"], (pre["in_y"] - mean) * rstd, args["slope"], dtype, f"{tag} m12")
        else:
            assert torch.equal(post["m12"].nan_to_num(7.0), pre["m12"].nan_to_num(7.0)), f"{tag}: m12 written by a call that returned fused = 0"


def a_conv_bwd_weight(A, tag, args, pre, post, ret):
    x, dy = pre["x"], pre["dy"]
    k, s = list(args["kernel"]), list(args["stride"])
    shape = tuple(post["dw"].shape)
    ref = torch.nn.grad.conv3d_weight(x, shape, dy, stride=s, padding=_pad(k))
    a = torch.nn.grad.conv3d_weight(x.abs(), shape, dy.abs(), stride=s, padding=_pad(k))
    check(post["dw"].float(), ref, a, dy.shape[0] * dy[0, 0].numel(), args["dy"].dtype, f"{tag} dw", names=DW5)


def a_convT_fwd(A, tag, args, pre, post, ret):
    x, w, b = pre["x"], pre["w_fwd"], pre["bias"]
    s = list(args["stride"])
    T, co, ci = w.shape
    W = w.view(*s, co, ci).permute(4, 3, 0, 1, 2)
    ref = F.conv_transpose3d(x, W, b, stride=s)
    a = F.conv_transpose3d(x.abs(), W.abs(), None if b is None else b.abs(), stride=s)
    check(post["y"], ref, a, ci + (b is not None), args["x"].dtype, f"{tag} up")


def a_convT_bwd_data(A, tag, args, pre, post, ret):
    dy, w, old = pre["dy"], pre["w_bwd"], pre["dx"]
    s = list(args["stride"])
    T, ci, co = w.shape
    W = w.view(*s, ci, co).permute(3, 4, 0, 1, 2)
    ref, a, terms = F.conv3d(dy, W, stride=s), F.conv3d(dy.abs(), W.abs(), stride=s), co * T
    if args["accumulate"]:
        ref, a, terms = ref + old, a + old.abs(), terms + 1
    check(post["dx"], ref, a, terms, args["dy"].dtype, f"{tag} dx{' +=' if args['accumulate'] else ''}")


def a_convT_bwd_weight(A, tag, args, pre, post, ret):
    x, dy, s = pre["x"], pre["dy"], list(args["stride"])

    def wgrad(x_, g_):       # the weight gradient of the stride-s conv that maps dy back to x (the transposed conv's adjoint)
        return torch.nn.grad.conv3d_weight(g_, tuple(post["dw"].shape), x_, stride=s)
    check(post["dw"].float(), wgrad(x, dy), wgrad(x.abs(), dy.abs()), x.shape[0] * x[0, 0].numel(), args["x"].dtype, f"{tag} dw",
          names=("ci", "co", "kz", "ky", "kx"))


def a_stem_fwd(A, tag, args, pre, post, ret):
    """the bound of test_stem_head_gpu.stem_ref: gamma(cin * taps + 1) of the magnitudes, then one rounding.  (The 16-bit MFMA
    kernels convert image and weights to the storage type: the audited runs feed values representable in it, as stem_ref does.)"""
    x, W, b = pre["x_ncdhw"], pre["w"], pre["bias"]
    k = list(args["kernel"])
    dtype = args["out"].dtype
    ref = F.conv3d(x, W, b, padding=_pad(k))
    e = gamma(W[0].numel() + 1) * F.conv3d(x.abs(), W.abs(), None if b is None else b.abs(), padding=_pad(k))
    assert_within(post["out"], ref, e + half_ulp(ref.abs() + e, dtype), f"{tag} y")
    if "stats" in post:
        check_stats(post["stats"], post["out"], args["eps"], what=f"{tag} stats")
        A.last_stats = args["stats"].data_ptr()


def a_stem_bwd_weight(A, tag, args, pre, post, ret):
    x, dy, k = pre["x_ncdhw"], pre["dy"], list(args["kernel"])
    shape = tuple(post["dw"].shape)
    ref = torch.nn.grad.conv3d_weight(x, shape, dy, padding=_pad(k))
    e = gamma(x.shape[0] * x[0, 0].numel()) * torch.nn.grad.conv3d_weight(x.abs(), shape, dy.abs(), padding=_pad(k))
    assert_within(post["dw"], ref, e, f"{tag} dw", names=DW5)


def a_channel_sum(A, tag, args, pre, post, ret):
    x = pre["x"]
    check(post["out"].float(), x.sum((0, 2, 3, 4)), x.abs().sum((0, 2, 3, 4)), x.shape[0] * x[0, 0].numel(), args["x"].dtype,
          f"{tag} db", names=("c",))


def a_pack(A, tag, args, pre, post, ret):
    dtype = args["dtype"]
    for i, ((w, kind, _, _), (_, _, f, b)) in enumerate(zip(pre["items"], post["items"])):
        flat = w.reshape(w.shape[0], w.shape[1], -1).float()
        same, swp = flat.permute(2, 0, 1).to(dtype).double(), flat.permute(2, 1, 0).to(dtype).double()
        wf, wb = (same, swp) if kind == 0 else (swp, same)
        assert f is None or torch.equal(f, wf), f"{tag}: w_fwd of item {i} is not the rounded permutation of its parameter"
        assert b is None or torch.equal(b, wb), f"{tag}: w_bwd of item {i} is not the rounded permutation of its parameter"


def a_stats(A, tag, args, pre, post, ret):
    check_stats(post["stats"], pre["y"], args["eps"], what=f"{tag} stats")


def a_stats_mask(A, tag, args, pre, post, ret):
    keep = pre["keep"].view(-1)
    old, new = pre["stats"].view(-1, 2), post["stats"].view(-1, 2)
    assert torch.equal(new[:, 0], old[:, 0]) and torch.equal(new[:, 1], old[:, 1] * keep), f"{tag}: not (mean, rstd * keep)"
    if A.last_stats == args["stats"].data_ptr():
        A.ledger.add("fused_stats->mask")


def a_act_fwd(A, tag, args, pre, post, ret):
    A.layer_stats(tag, args, pre)
    check_norm_fwd(post["out"], pre["y"], pre["stats"], pre["residual"], args["slope"], args["y"].dtype, f"{tag} out")


def a_norm_fwd(A, tag, args, pre, post, ret):
    check_stats(post["stats"], pre["y"], args["eps"], what=f"{tag} stats")
    A.layer_stats(tag, args, dict(pre, stats=post["stats"]))
    check_norm_fwd(post["out"], pre["y"], post["stats"], pre["residual"], args["slope"], args["y"].dtype, f"{tag} out")


def a_act_pool_fwd(A, tag, args, pre, post, ret):
    a_act_fwd(A, tag, args, pre, post, ret)
    s, out = tuple(args["stride"]), post["out"]       # the pool of the output as stored (the fused call equals the two calls)
    ref, e = F.avg_pool3d(out, s, s), pool_fwd_bound(out, s)
    assert_within(post["pooled"], ref, e + half_ulp(ref.abs() + e, args["y"].dtype), f"{tag} pooled")


def a_act_head_fwd(A, tag, args, pre, post, ret):
    assert args["act"] == 0, f"{tag}: no auditor for an eval activation fused into the head"
    A.layer_stats(tag, args, pre)
    dtype, w, b = args["y"].dtype, pre["w"], pre["b"]
    if args["out"] is not None:
        A.ledger.add("instnorm_act_head_fwd:out=stored")
        check_norm_fwd(post["out"], pre["y"], pre["stats"], None, args["slope"], dtype, f"{tag} out")
        want, e = head_logits_ref(post["out"], w, b)
    else:
        A.ledger.add("instnorm_act_head_fwd:out=None")
        a, e_a = _lrelu64(pre["y"], pre["stats"], args["slope"], dtype)
        want, e = head_logits_ref(a, w, b)
        e = e + (1 + gamma(w.shape[1] + 1)) * torch.einsum("nczyx,kc->nkzyx", e_a, w.abs())
    assert_within(post["out_ncdhw"], want, e, f"{tag} logits")


def a_head_fwd(A, tag, args, pre, post, ret):
    assert args["act"] == 0, f"{tag}: no auditor for an eval activation fused into the head"
    want, e = head_logits_ref(pre["x"], pre["w"], pre["b"])
    assert_within(post["out_ncdhw"], want, e, f"{tag} logits")


def a_head_bwd(A, tag, args, pre, post, ret):
    d, a, w = pre["dout_ncdhw"], pre["x"], pre["w"]
    k = w.shape[0]
    if args["dx"] is not None:
        g_un, d_g = head_dx_ref(d, w, args["x"].dtype)
        assert_within(post["dx"], g_un, d_g, f"{tag} dx")
    else:
        A.ledger.add("head_bwd:dx=None")
    dw_ref, db_ref, e_dw, e_db = head_grads_ref(d, a)
    assert_within(post["dw"].view(k, -1), dw_ref, e_dw, f"{tag} dw", names=("k", "c"))
    assert_within(post["db"], db_ref, e_db, f"{tag} db", names=("k",))


def a_bwd_head(A, tag, args, pre, post, ret):
    d, w, y, stats, slope, dtype = pre["dout_ncdhw"], pre["w"], pre["y"], pre["stats"], args["slope"], args["y"].dtype
    g_un, d_g = head_dx_ref(d, w, dtype)
    check_norm_bwd(post["dy"], g_un, y, stats, lrelu_mask(None, y, stats, slope), slope, dtype, f"{tag} dy", d_g=d_g)
    A.ledger.add("instnorm_act_bwd_head:" + ("dw" if args["dw"] is not None else "nodw"))
    if args["dw"] is not None:
        # the head bound of test_stem_head_gpu on the activation recomputed from y: its error e_a enters each of the n * V terms
        a, e_a = _lrelu64(y, stats, slope, dtype)
        dw_ref, db_ref, e_dw, e_db = head_grads_ref(d, a)
        e_dw = e_dw + (1 + gamma(d.shape[0] * d[0, 0].numel())) * torch.einsum("nkzyx,nczyx->kc", d.abs(), e_a)
        assert_within(post["dw"], dw_ref, e_dw, f"{tag} dw", names=("k", "c"))
        assert_within(post["db"], db_ref, e_db, f"{tag} db", names=("k",))


def _dres(tag, args, pre, post, mask):
    if args["d_residual"] is not None:
        acc = args["accumulate_residual"]
        check_dres(post["d_residual"], pre["g"], mask, args["slope"], args["y"].dtype, f"{tag} d_residual{' +=' if acc else ''}",
                   old=pre["d_residual"] if acc else None)


def a_act_bwd(A, tag, args, pre, post, ret):
    y, stats, slope = pre["y"], pre["stats"], args["slope"]
    mask = lrelu_mask(pre["out"], y, stats, slope)
    rec = A.rec_for(args["stats"])
    if rec is not None and rec.head_src is not None:
        A.ledger.add("head_src:dlogits=None")
    if "m12" in args:
        assert A.instats.pop(args["m12"].data_ptr(), False), f"{tag}: m12 was not left by a conv3d_bwd_data_instats of this pass"
        A.ledger.add("instats->apply")
    check_norm_bwd(post["dy"], pre["g"], y, stats, mask, slope, args["y"].dtype, f"{tag} dy")
    _dres(tag, args, pre, post, mask)


def a_bwd_res(A, tag, args, pre, post, ret):
    pool = tuple(args["pool_stride"]) if args["pool_dy"] is not None else None
    A.ledger.add("instnorm_act_bwd_res:" + ("pool" if pool else "nopool"))
    check_norm_bwd_res(post["d_residual"], post["dy"], pre["g"], pre["pool_dy"], pool, pre["out"], pre["y"], pre["stats"],
                       args["slope"], args["y"].dtype, tag)


def a_pool_fwd(A, tag, args, pre, post, ret):
    s, x = tuple(args["stride"]), pre["x"]
    ref, e = F.avg_pool3d(x, s, s), pool_fwd_bound(x, s)
    assert_within(post["y"], ref, e + half_ulp(ref.abs() + e, args["x"].dtype), f"{tag} pool")


def a_pool_bwd(A, tag, args, pre, post, ret):
    s, de = tuple(args["stride"]), pre["dy"]
    for ax, ss in enumerate(s):
        de = de.repeat_interleave(ss, dim=2 + ax)
    de = de / (s[0] * s[1] * s[2])
    old = pre["dx"] if args["accumulate"] else None
    want = de if old is None else old + de
    e = pool_bwd_bound(de, old)
    assert_within(post["dx"], want, e + half_ulp(want.abs() + e, args["dy"].dtype), f"{tag} pool dx{' +=' if old is not None else ''}")


AUDITORS = {
    "pack_weights_multi": (lambda items, dtype: locals(), [], ["items"], {}, a_pack),
    "conv3d_fwd": (lambda x, w_fwd, bias, y, kernel, stride, ws=None: locals(), ["x", "w_fwd", "bias"], ["y"], {}, a_conv_fwd),
    "conv3d_fwd_stats": (lambda x, w_fwd, bias, y, kernel, stride, stats, eps=1e-5, ws=None: locals(),
                         ["x", "w_fwd", "bias"], ["y", "stats"], {}, a_conv_fwd),
    "conv3d_bwd_data": (lambda dy, w_bwd, dx, kernel, stride, accumulate=False, ws=None: locals(),
                        ["dy", "w_bwd"], ["dx"], {"dx": "accumulate"}, a_conv_bwd_data),
    "conv3d_bwd_data_instats": (lambda dy, w_bwd, dx, kernel, stride, accumulate, in_y, in_stats, slope, m12, ws=None: locals(),
                                ["dy", "w_bwd", "in_y", "in_stats"], ["dx", "m12"], {"dx": "accumulate"}, a_conv_bwd_data),
    "conv3d_bwd_weight": (lambda x, dy, dw, kernel, stride, ws=None: locals(), ["x", "dy"], ["dw"], {}, a_conv_bwd_weight),
    "convT3d_fwd": (lambda x, w_fwd, bias, y, stride, ws=None: locals(), ["x", "w_fwd", "bias"], ["y"], {}, a_convT_fwd),
    "convT3d_bwd_data": (lambda dy, w_bwd, dx, stride, accumulate=False, ws=None: locals(),
                         ["dy", "w_bwd"], ["dx"], {"dx": "accumulate"}, a_convT_bwd_data),
    "convT3d_bwd_weight": (lambda x, dy, dw, stride, ws=None: locals(), ["x", "dy"], ["dw"], {}, a_convT_bwd_weight),
    "stem_conv_fwd": (lambda x_ncdhw, w, bias, out, kernel: locals(), ["x_ncdhw", "w", "bias"], ["out"], {}, a_stem_fwd),
    "stem_conv_fwd_stats": (lambda x_ncdhw, w, bias, out, kernel, stats, eps=1e-5, ws=None: locals(),
                            ["x_ncdhw", "w", "bias"], ["out", "stats"], {}, a_stem_fwd),
    "stem_conv_bwd_weight": (lambda x_ncdhw, dy, dw, kernel, ws=None: locals(), ["x_ncdhw", "dy"], ["dw"], {}, a_stem_bwd_weight),
    "channel_sum": (lambda x, out, ws=None: locals(), ["x"], ["out"], {}, a_channel_sum),
    "instnorm_stats": (lambda y, stats, eps=1e-5, ws=None: locals(), ["y"], ["stats"], {}, a_stats),
    "instnorm_stats_mask": (lambda stats, keep: locals(), ["stats", "keep"], ["stats"], {}, a_stats_mask),
    "instnorm_act_fwd": (lambda y, stats, out, slope=0.01, residual=None: locals(), ["y", "stats", "residual"], ["out"], {}, a_act_fwd),
    "instnorm_fwd": (lambda y, stats, out, slope=0.01, residual=None, eps=1e-5, ws=None: locals(),
                     ["y", "residual"], ["stats", "out"], {}, a_norm_fwd),
    "instnorm_act_pool_fwd": (lambda y, stats, out, pooled, stride, slope=0.01, residual=None: locals(),
                              ["y", "stats", "residual"], ["out", "pooled"], {}, a_act_pool_fwd),
    "instnorm_act_head_fwd": (lambda y, stats, out, w, b, out_ncdhw, act, slope=0.01: locals(),
                              ["y", "stats", "w", "b"], ["out", "out_ncdhw"], {}, a_act_head_fwd),
    "head_fwd": (lambda x, w, b, out_ncdhw, act=0: locals(), ["x", "w", "b"], ["out_ncdhw"], {}, a_head_fwd),
    "head_bwd": (lambda dout_ncdhw, x, w, dx, dw, db, ws=None: locals(), ["dout_ncdhw", "x", "w"], ["dx", "dw", "db"], {}, a_head_bwd),
    "instnorm_act_bwd_head": (lambda dout_ncdhw, w, y, stats, dy, slope=0.01, ws=None, dw=None, db=None: locals(),
                              ["dout_ncdhw", "w", "y", "stats"], ["dy", "dw", "db"], {}, a_bwd_head),
    "instnorm_act_bwd": (lambda g, y, stats, out, dy, slope=0.01, d_residual=None, accumulate_residual=False, ws=None: locals(),
                         ["g", "y", "stats", "out"], ["dy", "d_residual"], {"d_residual": "accumulate_residual"}, a_act_bwd),
    "instnorm_act_bwd_apply": (lambda g, y, stats, out, dy, m12, slope=0.01, d_residual=None, accumulate_residual=False: locals(),
                               ["g", "y", "stats", "out", "m12"], ["dy", "d_residual"], {"d_residual": "accumulate_residual"},
                               a_act_bwd),
    "instnorm_act_bwd_res": (lambda g, y, stats, out, dy, d_residual, slope=0.01, pool_dy=None, pool_stride=(1, 1, 1), ws=None: locals(),
                             ["g", "y", "stats", "out", "pool_dy"], ["dy", "d_residual"], {}, a_bwd_res),
    "avgpool_fwd": (lambda x, y, stride: locals(), ["x"], ["y"], {}, a_pool_fwd),
    "avgpool_bwd": (lambda dy, dx, stride, accumulate=False: locals(), ["dy"], ["dx"], {"dx": "accumulate"}, a_pool_bwd),
}
NEVER_POISONED = {"pack_weights_multi"}      # packed weights are refreshed only when a parameter moved


def _extent(v):
    """(first byte, past the last byte) of the buffer a written object lives in"""
    t = v if not hasattr(v, "to_ncdhw") else v.root if v.is_planar_cat else v.t
    return t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()


def _storage_view(v):
    """what a written object addresses, as a view that can be filled in place (a planar concat: its root, every plane of it)"""
    if not hasattr(v, "to_ncdhw"):
        return v
    return v.root if v.is_planar_cat else v.tensor()


def _dev_finite(v):
    """the finite check of a launch that is not held to its fp64 reference: on the device, no copy"""
    if hasattr(v, "to_ncdhw") or (torch.is_tensor(v) and v.is_floating_point()):
        return bool(torch.isfinite(_storage_view(v)).all())
    return True


class OpsAudit:
    """only: op names held to their fp64 reference (None: all).  The launches of every other op keep the stale-state check (finite
    reads and writes under the poison, on the device) but no reference: a configuration whose fp64 convolutions would take
    minutes audits the launches it is there for, and leaves the rest to the configurations that are small enough."""

    def __init__(self, real, net, only=None):
        self.real, self.net, self.only = real, net, only
        self.phase, self.strict = "fwd", False
        self.calls, self.failures, self.ledger = [], [], set()
        self.written = {"fwd": {}, "bwd": {}}
        self.instats, self.last_stats = {}, None
        self.poisoned = {"fwd": 0, "bwd": 0}       # ranges the last strict begin() of each phase filled / left alone as live
        self.kept_live = {"fwd": 0, "bwd": 0}

    def __getattr__(self, name):
        v = getattr(self.real, name)
        if name in PASS_THROUGH or not callable(v):
            return v
        return lambda *a, **k: self._call(name, v, *a, **k)

    # ---- the plan's records, for what a launch cannot know: which layer a statistics buffer belongs to --------------------------
    def rec_for(self, stats):
        for plan in self.net._plans.values():
            for tape in [plan.enc_tape] + plan.dec_tapes:
                for r in tape:
                    if r.kind == "inact" and r.stats.data_ptr() == stats.data_ptr():
                        return r
        return None

    def layer_stats(self, tag, args, pre):
        """the statistics an apply launch reads are those of ITS layer's y under ITS layer's eps (a dropped plane: rstd exactly 0),
        whoever produced them"""
        rec = self.rec_for(args["stats"])
        assert rec is not None and rec.y.act.t.data_ptr() == args["y"].t.data_ptr(), f"{tag}: statistics buffer of another layer"
        eps, keep = rec.eps, None
        if rec.drop is not None and self.net.training:
            eps, keep = rec.drop.eps * (1.0 - rec.drop.p) ** 2, rec.drop.keep
        check_stats(pre["stats"], pre["y"], eps, what=f"{tag}: the statistics it reads", keep=keep)

    # ---- one launch -------------------------------------------------------------------------------------------------------------------
    def _call(self, name, fn, *a, **k):
        tag = f"{self.phase}#{len(self.calls)} {name}"
        self.calls.append((self.phase, name))
        self.ledger.add(name)
        spec = AUDITORS.get(name)
        if spec is None:
            self.failures.append(f"{tag}: a launch with no auditor (tests/plan_audit.py::AUDITORS)")
            return fn(*a, **k)
        sig, reads, writes, acc, audit = spec
        args = sig(*a, **k)
        full = self.only is None or name in self.only
        read_now = reads + [d for d, flag in acc.items() if args[flag]]
        torch.cuda.synchronize()
        if full:
            pre = {n: _snap(v) for n, v in args.items() if n != "ws"}
            stale = [n for n in read_now if not _finite(pre[n])]
        else:
            stale = [n for n in read_now if not _dev_finite(args[n])] if self.strict else []
        ret = fn(*a, **k)
        torch.cuda.synchronize()
        wrote = [n for n in writes if args[n] is not None]
        if name not in NEVER_POISONED:
            for n in wrote:
                v = args[n]
                self.written[self.phase][(_extent(v), getattr(v, "c0", 0), getattr(v, "c", 0))] = v
        try:
            if self.strict:
                assert not stale, f"{tag}: reads `{stale[0]}`, which nothing has written in this pass (NaN-poisoned)"
            post = {n: _snap(args[n]) for n in wrote} if full else {}
            if full:
                audit(self, tag, args, pre, post, ret)
            if self.strict:
                for n in wrote:
                    if not (n == "m12" and name == "conv3d_bwd_data_instats" and not ret):
                        assert _finite(post[n]) if full else _dev_finite(args[n]), f"{tag}: leaves non-finite values in `{n}`"
        except AssertionError as e:
            msg = str(e)
            self.failures.append(msg if msg.startswith(tag) else f"{tag}: {msg}")
        return ret

    # ---- passes ---------------------------------------------------------------------------------------------------------------------
    def begin(self, phase, strict=False):
        """start a pass; strict: poison what the launches of this phase wrote so far, and hold every launch to finite reads"""
        torch.cuda.synchronize()
        self.phase, self.strict = phase, strict
        self.instats, self.last_stats = {}, None
        if not strict:
            return
        live = [e for (e, _, _) in self.written["fwd"]] if phase == "bwd" else []
        self.poisoned[phase] = self.kept_live[phase] = 0
        for (e, _, _), v in self.written[phase].items():
            if any(e[0] < hi and lo < e[1] for lo, hi in live):
                self.kept_live[phase] += 1      # a live activation the backward still reads
                continue
            t = _storage_view(v)
            t.fill_(float("nan") if t.is_floating_point() else -(1 << 30))
            self.poisoned[phase] += 1
        torch.cuda.synchronize()

    def check(self):
        torch.cuda.synchronize()
        f, self.failures = self.failures, []
        assert not f, f"{len(f)} launches failed their audit; first:\n" + "\n".join(f[:4])

    def names(self, phase=None):
        return [n for p, n in self.calls if phase in (None, p)]


def install(monkeypatch, net, only=None):
    """replace the name `ops` in the plan module that `net` builds its plans from; returns the proxy"""
    planmod = sys.modules[sys.modules[type(net).__module__].Plan.__module__]
    audit = OpsAudit(planmod.ops, net, only)
    monkeypatch.setattr(planmod, "ops", audit)
    return audit
