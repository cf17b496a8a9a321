"""CPU: the argument checks every wrapper of engine.ops shares (engine/ops/core.py) -- directly, on host tensors with the expected
device passed in, and through the public functions: each one that takes a device batch refuses a host tensor by its own name."""
import numpy as np
import pytest
import torch

import mt3d_amd  # noqa: F401
from mt3d_amd.engine import ops
from mt3d_amd.engine.lib import RxError
from mt3d_amd.engine.ops import core

CPU = torch.device("cpu")


class OnDevice(torch.Tensor):
    """a host tensor that answers `is_cuda` like a device tensor, so that the checks behind the first one are reached"""
    is_cuda = property(lambda self: True)


def dev(t):
    return t.as_subclass(OnDevice)


# ---- device_batch ------------------------------------------------------------------------------------------------------------------
def test_device_batch_refuses_in_order_and_returns_a_contiguous_tensor():
    good = dev(torch.arange(2 * 1 * 2 * 3 * 4, dtype=torch.float32).reshape(2, 1, 2, 3, 4))
    assert core.device_batch("f", good, "hint") is good
    strided = good.transpose(3, 4)
    made = core.device_batch("f", strided, "hint")
    assert made.is_contiguous() and not strided.is_contiguous() and torch.equal(made, strided)
    for bad in (good.as_subclass(torch.Tensor), np.zeros((1, 1, 2, 2, 2), np.float32), None):      # a host tensor, not a tensor
        with pytest.raises(RxError, match=r"^f: the batch must be a device tensor \(the host path is elsewhere\)$"):
            core.device_batch("f", bad, "the host path is elsewhere")
    with pytest.raises(RxError, match=r"^f: batch dtype torch.float16: expected a float32 \(B, C, Z, Y, X\) batch"):
        core.device_batch("f", good.half(), "hint")
    with pytest.raises(RxError, match="dtype"):      # the dtype is judged before the rank
        core.device_batch("f", good[0].half(), "hint")
    with pytest.raises(RxError, match=r"^f: expected a non-empty float32 \(B, C, Z, Y, X\) batch, got torch.float32 \(1, 2, 3, 4\)$"):
        core.device_batch("f", good[0], "hint")
    with pytest.raises(RxError, match="non-empty"):
        core.device_batch("f", good[:0], "hint")


def test_device_batch_takes_other_dtypes_ranks_and_words():
    kw = dict(what="prediction", dtypes=core.FLOATS, rank=3, or_more=True, layout="(N, C, *spatial)")
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        for shape in ((2, 3, 4), (2, 3, 4, 5, 6)):
            t = dev(torch.zeros(shape, dtype=dt))
            assert core.device_batch("m", t, "hint", **kw) is t
    with pytest.raises(RxError, match=r"^m: prediction dtype torch.int32: expected a float32 / bfloat16 / float16 \(N, C, \*spatial\)"):
        core.device_batch("m", dev(torch.zeros(2, 3, 4, dtype=torch.int32)), "hint", **kw)
    with pytest.raises(RxError, match=r"^m: expected a non-empty .* prediction, got torch.float32 \(2, 3\)$"):
        core.device_batch("m", dev(torch.zeros(2, 3)), "hint", **kw)
    with pytest.raises(RxError, match=r"^m: the prediction must be a device tensor"):
        core.device_batch("m", torch.zeros(2, 3, 4), "hint", **kw)


# ---- result_tensor -----------------------------------------------------------------------------------------------------------------
def test_result_tensor_allocates_with_the_requested_allocator():
    got = core.result_tensor("f", "out", None, [2, 3], torch.int64, CPU, torch.zeros)
    assert got.shape == (2, 3) and got.dtype == torch.int64 and got.device == CPU and int(got.abs().sum()) == 0
    filled = []

    def ones(shape, dtype, device):
        filled.append((shape, dtype, device))
        return torch.ones(shape, dtype=dtype, device=device)
    got = core.result_tensor("f", "out", None, (4,), torch.float32, CPU, ones)
    assert filled == [((4,), torch.float32, CPU)] and float(got.sum()) == 4.0
    assert core.result_tensor("f", "out", None, (4,), torch.uint8, CPU).shape == (4,)      # torch.empty by default


def test_result_tensor_hands_back_a_fitting_tensor_and_refuses_the_rest():
    fit = torch.full((2, 3), 7.0)
    assert core.result_tensor("f", "out", fit, (2, 3), torch.float32, CPU, torch.zeros) is fit and float(fit.sum()) == 42.0
    bad = {"shape": torch.zeros(3, 2), "dtype": torch.zeros(2, 3, dtype=torch.float64), "contiguity": torch.zeros(3, 2).t(),
           "device": torch.zeros(2, 3, device="meta"), "type": np.zeros((2, 3), np.float32)}
    for what, t in bad.items():
        with pytest.raises(RxError, match=r"^f: `out` must be a contiguous float32 tensor of shape \(2, 3\) on cpu$"):
            core.result_tensor("f", "out", t, (2, 3), torch.float32, CPU)
            pytest.fail(f"a wrong {what} was accepted")


def test_result_tensor_storage_width_switch():
    u16 = core._U16
    i16, i32 = torch.zeros(5, dtype=torch.int16), torch.zeros(5, dtype=torch.int32)
    assert core.result_tensor("f", "out['labels']", i16, (5,), u16, CPU, same_width=True) is i16
    with pytest.raises(RxError, match=r"out\['labels'\]"):
        core.result_tensor("f", "out['labels']", i32, (5,), u16, CPU, same_width=True)
    if u16 is not torch.int16:      # without the switch the dtype itself is compared
        with pytest.raises(RxError, match="uint16"):
            core.result_tensor("f", "out", i16, (5,), u16, CPU)
    with pytest.raises(RxError):      # the switch waives the dtype, nothing else
        core.result_tensor("f", "out", i16, (6,), u16, CPU, same_width=True)


# ---- the code tables and the small helpers ---------------------------------------------------------------------------------------------
def test_one_table_of_raw_voxel_types():
    from mt3d_amd.engine import lib
    assert core.SW_DTYPE[torch.uint8] == lib.RX_SW_U8 and core.SW_DTYPE[torch.float32] == lib.RX_SW_F32
    assert core.SW_DTYPE[torch.int16] == lib.RX_SW_U16 and core.SW_DTYPE[core._U16] == lib.RX_SW_U16
    if hasattr(torch, "uint16"):
        assert torch.uint16 in core.SW_DTYPE and core._U16 is torch.uint16
    assert set(ops.infer._SW_IN) < set(core.SW_DTYPE) and torch.int16 in ops.infer._SW_IN


def test_codes_are_shared_with_the_dataloading_modules():
    from mt3d_amd.dataloading import elastic_device, ingest_device, spatial_device
    from mt3d_amd.engine import lib
    assert spatial_device.INTERP is core.INTERP and spatial_device.BORDER is core.BORDER and elastic_device.INTERP is core.INTERP
    assert ingest_device.RULES is core.RULES and ingest_device.rule_code is core.rule_code
    assert core.INTERP == {"linear": lib.RX_AFFINE_LINEAR, "nearest": lib.RX_AFFINE_NEAREST} == {"linear": 0, "nearest": 1}
    assert core.BORDER == {"constant": lib.RX_AFFINE_CONSTANT, "clamp": lib.RX_AFFINE_CLAMP} == {"constant": 0, "clamp": 1}
    assert [core.rule_code(r) for r in core.RULES] == [lib.RX_INGEST_COPY, lib.RX_INGEST_DIV255, lib.RX_INGEST_DIV65535,
                                                       lib.RX_INGEST_NORMAL_U16, lib.RX_INGEST_NORMAL_MUL2]
    assert core.rule_code("DIV255") == 1 and core.rule_code(np.int64(4)) == 4
    for bad in ("div256", 5, -1, True, 1.0, None):
        with pytest.raises(ValueError, match="rule"):
            core.rule_code(bad)


def test_optional_descriptor():
    a = ops.Act(torch.zeros(1, 2, 2, 2, 8), 2, 4)
    assert core._desc(None) is None
    assert core._desc(a)._obj is a.desc()


def test_a_formula_that_names_a_missing_parameter_is_refused_at_definition():
    with pytest.raises(TypeError, match="resid"):
        @core.hbm("label", lambda y, resid: 0)
        def f(y, stats, residual=None):
            pass
    with pytest.raises(TypeError, match="kernel"):
        @core.flops(lambda x, kernel: ("k", 0.0))
        def g(x, y):
            pass


# ---- through the public functions ------------------------------------------------------------------------------------------------------
B5 = torch.zeros(1, 1, 4, 4, 4)
HOST_CALLS = {
    "geom_apply": lambda: ops.geom_apply(B5, [(0, 1, 2, 0, 0, 0, 0, 1, 2, 0, 0, 0)], False),
    "affine_apply": lambda: ops.affine_apply(B5, np.zeros((1, 18), np.float32), "linear", "constant"),
    "elastic_apply": lambda: ops.elastic_apply(B5, None, None, (8, 8, 8), "linear", "constant"),
    "label_dilate": lambda: ops.label_dilate(B5, 2),
    "box_stats": lambda: ops.box_stats(torch.zeros(4, 4, 4, dtype=torch.uint8), np.array([[0, 0, 0, 2, 2, 2]])),
    "ingest": lambda: ops.ingest(torch.zeros(1, 4, 4, 4, dtype=torch.uint8), "div255"),
    "augment_batch": lambda: ops.augment_batch(B5, None, None, 0, False),
    "seg_counts": lambda: ops.seg_counts(B5, B5),
    "class_counts": lambda: ops.class_counts(torch.zeros(1, 2, 4, 4, 4), torch.zeros(1, 2, 4, 4, 4)),
    "normal_stats": lambda: ops.normal_stats(torch.zeros(1, 3, 4, 4, 4), torch.zeros(1, 3, 4, 4, 4)),
    "preview_panel": lambda: ops.preview_panel(B5[0], torch.zeros(4, 4, 4, 3, dtype=torch.uint8), 0, 0),
    "preview_frames": lambda: ops.preview_frames(B5, {"a": B5}, {"a": B5}),
}


@pytest.mark.parametrize("name", sorted(HOST_CALLS))
def test_public_functions_refuse_a_host_batch_by_name(name):
    with pytest.raises(RxError, match=rf"^{name}: .*device tensor"):
        HOST_CALLS[name]()


def test_post_device_refusals_keep_their_order():
    """what comes behind `is_cuda`, on host tensors that pass for device tensors: the same refusal for the same bad input as before"""
    b5 = dev(B5.clone())
    for call in (lambda t: ops.geom_apply(t, [], False), lambda t: ops.affine_apply(t, [], "linear", "constant"),
                 lambda t: ops.elastic_apply(t, None, None, (8, 8, 8), "linear", "constant"), lambda t: ops.label_dilate(t)):
        for bad in (b5[0], b5.double()):
            with pytest.raises(RxError, match="expected"):
                call(bad)
    with pytest.raises(RxError, match="interp 'cubic'"):      # the modes before the table, the records and `out`
        ops.affine_apply(b5, [], "cubic", "constant", out=B5)
    with pytest.raises(RxError, match="0 records for a batch of 1"):      # the records before `out`
        ops.affine_apply(b5, np.zeros((0, 18), np.float32), "linear", "clamp", out=B5.double())
    with pytest.raises(RxError, match=r"^affine_apply: `out` must be a contiguous float32 tensor of shape \(1, 1, 4, 4, 4\) on cpu$"):
        ops.affine_apply(b5, np.zeros((1, 18), np.float32), "linear", "clamp", out=B5.double())
    with pytest.raises(RxError, match="label_dilate: `out`"):
        ops.label_dilate(b5, 2, out=B5[..., :2])
    with pytest.raises(RxError, match="ingest: dtype torch.int16"):      # ingest takes a store's own types only
        ops.ingest(dev(torch.zeros(1, 4, 4, 4, dtype=torch.int16)), "copy")
    with pytest.raises(RxError, match="ingest: expected"):
        ops.ingest(dev(torch.zeros(4, 4, 4, dtype=torch.uint8)), "copy")
    with pytest.raises(RxError, match="unknown rule"):
        ops.ingest(dev(torch.zeros(1, 4, 4, 4, dtype=torch.uint8)), "div256", out=B5.double())
    with pytest.raises(RxError, match="ingest: `out`"):
        ops.ingest(dev(torch.zeros(1, 4, 4, 4, dtype=torch.uint8)), "div255", out=B5.double())
    with pytest.raises(RxError, match="seg_counts: prediction dtype torch.int32"):
        ops.seg_counts(dev(B5.int()), B5)
    with pytest.raises(RxError, match="class_counts: expected a non-empty"):      # class_counts wants (N, C, spatial...), seg_counts (N, C)
        ops.class_counts(dev(torch.zeros(2, 3)), torch.zeros(2, 3))
    with pytest.raises(RxError, match="seg_counts: `out`"):
        ops.seg_counts(dev(torch.zeros(2, 3)), torch.zeros(2, 3), out=torch.zeros(2, 3, 3))
    with pytest.raises(RxError, match=r"normal_stats: `out\[1\]`"):
        ops.normal_stats(dev(torch.zeros(1, 3, 8)), torch.zeros(1, 3, 8), out=(torch.zeros(1, dtype=torch.int64), torch.zeros(1, 2)))
    with pytest.raises(RxError, match="preview_panel: the sample must be contiguous"):
        ops.preview_panel(dev(torch.zeros(1, 2, 4, 3)).transpose(2, 3), torch.zeros(2, 3, 4, 3, dtype=torch.uint8), 0, 0)
    with pytest.raises(RxError, match="preview_panel: `minmax`"):
        ops.preview_panel(dev(torch.zeros(1, 2, 3, 4)), torch.zeros(2, 3, 4, 3, dtype=torch.uint8), 0, 0, minmax=torch.zeros(1, 2, 3))
    with pytest.raises(RxError, match="preview_frames: `out`"):
        ops.preview_frames(b5, {}, {}, out=torch.zeros(4, 8, 4, 3))
