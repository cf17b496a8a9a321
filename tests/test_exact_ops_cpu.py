"""CPU: the exact-data helpers of tests/exact_ops.py have teeth.  Faults of the kind a kernel can have (a dropped product, a
dropped tap row at a tile edge, swapped weight indices, truncation instead of rounding, an unwritten element, a write into a
neighbouring channel) are planted into fp64 CPU results; every one fails the new checks, and the single-element ones pass the old
per-tensor `rel < TOL[bf16]` assertion of the op tests."""
import pytest
import torch
import torch.nn.functional as F

from exact_ops import Guarded, assert_bits, assert_exact_precondition, assert_within, exact_tensor

TOL_BF16 = 1.2e-2          # the per-tensor rel-L2 bar of tests/test_ops_gpu.py in bf16


def rel(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return ((a - b).norm() / b.norm().clamp(min=1e-30)).item()


def old_check_passes(got, want):
    return rel(got, want) < TOL_BF16


@pytest.fixture(scope="module")
def conv():
    """one 3x3x3 layer (2 x 32 -> 32 channels at 8^3) with exact data, its fp64 output, and the rounded bf16 output"""
    x = exact_tensor((2, 32, 8, 8, 8), 1, -4, 4, 0.5, 2.0 ** -2)
    w = exact_tensor((32, 32, 3, 3, 3), 2, -4, 4, 0.5, 2.0 ** -3)
    assert_exact_precondition(lambda a, b: F.conv3d(a, b, padding=1), (x, w), 2.0 ** -5, terms=32 * 27, what="conv")
    y = F.conv3d(x, w, padding=1)
    return x, w, y, y.float().to(torch.bfloat16)


def test_exact_tensor_is_representable_and_sparse():
    t = exact_tensor((4, 64, 9, 9), 7, -5, 5, 0.25, 2.0 ** -6)
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        assert torch.equal(t.to(dt).double(), t)
    ints = t * 2 ** 6
    assert torch.equal(ints, ints.round()) and ints.abs().max() <= 5
    assert 0.7 < (t == 0).double().mean().item() < 0.85          # 1 - 0.25 forced zeros, plus the drawn zeros
    assert torch.equal(t, exact_tensor((4, 64, 9, 9), 7, -5, 5, 0.25, 2.0 ** -6))


def test_precondition_fails_loudly():
    a = exact_tensor((1, 64, 4, 4, 4), 3, -200, 200, 1.0, 1.0)
    b = exact_tensor((64, 64, 3, 3, 3), 4, -200, 200, 1.0, 1.0)
    op = lambda u, v: F.conv3d(u, v, padding=1)                    # noqa: E731
    with pytest.raises(AssertionError, match="2\\^24"):
        assert_exact_precondition(op, (a, b), 1.0, terms=64 * 27, out16=False)
    with pytest.raises(AssertionError, match="fp16 range"):
        assert_exact_precondition(op, (a.clamp(-20, 20), b.clamp(-20, 20)), 1.0, terms=64 * 27)
    assert_exact_precondition(op, (a.clamp(-3, 3), b.clamp(-3, 3)), 1.0, terms=64 * 27)


def test_correct_result_passes(conv):
    x, w, y, y16 = conv
    assert_bits(y16, y, torch.bfloat16, "y")
    assert_bits(y.float(), y, torch.float32, "y32")


def test_dropped_product_at_corner_voxel(conv):
    x, w, y, _ = conv
    bad = y.clone()
    ci = int((x[1, :, 0, 0, 0] != 0).nonzero()[0])
    t = (w[5, ci, 1:, 1:, 1:] * x[1, ci, 0:2, 0:2, 0:2]).nonzero()[0]          # a non-zero term of the (0, 0, 0) voxel
    bad[1, 5, 0, 0, 0] -= w[5, ci, 1 + t[0], 1 + t[1], 1 + t[2]] * x[1, ci, t[0], t[1], t[2]]
    with pytest.raises(AssertionError, match=r"(?s)1 of .* wrong.*'n': 1, 'c': 5, 'z': 0, 'y': 0, 'x': 0"):
        assert_bits(bad.float().to(torch.bfloat16), y, torch.bfloat16, "y")
    assert old_check_passes(bad.float().to(torch.bfloat16), y)


def test_dropped_tap_row_at_tile_edge(conv):
    x, w, y, _ = conv
    w_row = w.clone()
    w_row[:, :, :, 2, :] = 0                                                   # the halo row below the tile is never read
    bad = y.clone()
    bad[:, :, :, 3, :] = F.conv3d(x, w_row, padding=1)[:, :, :, 3, :]         # last row of a 4-row tile
    with pytest.raises(AssertionError, match="'y': 3"):
        assert_bits(bad.float().to(torch.bfloat16), y, torch.bfloat16, "y")


def test_swapped_row_col_of_asymmetric_weight(conv):
    x, w, y, _ = conv
    assert not torch.equal(w, w.transpose(3, 4))
    bad = F.conv3d(x, w.transpose(3, 4), padding=1)
    with pytest.raises(AssertionError, match="wrong"):
        assert_bits(bad.float().to(torch.bfloat16), y, torch.bfloat16, "y")
    g = exact_tensor((3, 32), 5, -4, 4, 1.0, 2.0 ** -2)                       # head weights (k, c) indexed as (c, k)
    xs = exact_tensor((32, 3), 6, -4, 4, 1.0, 1.0)
    with pytest.raises(AssertionError, match="wrong"):
        assert_bits((g.t().reshape(3, 32) @ xs).float(), g @ xs, torch.float32, "head", names=None)


def test_truncation_instead_of_round_to_nearest_even(conv):
    _, _, y, y16 = conv
    bits = y.float().view(torch.int32) & ~0xFFFF                            # drop the low 16 bits: round toward zero
    trunc = bits.view(torch.float32).to(torch.bfloat16)
    assert not torch.equal(trunc, y16)
    with pytest.raises(AssertionError, match="wrong"):
        assert_bits(trunc, y, torch.bfloat16, "y")
    assert old_check_passes(trunc, y)


def test_unwritten_zero_element():
    """a kernel that skips one element whose true value is 0 (a structurally-zero dx class): invisible on a zero-filled buffer,
    caught on a NaN-poisoned one"""
    want = exact_tensor((2, 32, 4, 4, 4), 8, -4, 4, 0.5, 1.0)
    want[0, 3, 1, 2, 3] = 0.0
    out = Guarded(2, (4, 4, 4), 32, torch.bfloat16, device="cpu")
    v = out.ncdhw()
    v.copy_(want.to(torch.bfloat16))
    v[0, 3, 1, 2, 3] = float("nan")                                           # never written: the poison stays
    with pytest.raises(AssertionError, match="unwritten"):
        out.check("dx")
    with pytest.raises(AssertionError, match="'c': 3, 'z': 1, 'y': 2, 'x': 3"):
        assert_bits(v, want, torch.bfloat16, "dx")
    zeroed = want.to(torch.bfloat16).clone()                                 # the same kernel on a zero-initialised buffer
    assert old_check_passes(zeroed, want)


def test_write_into_guard_channel():
    want = exact_tensor((1, 32, 4, 4, 4), 9, -4, 4, 0.5, 1.0)
    out = Guarded(1, (4, 4, 4), 32, torch.float16, device="cpu")
    out.ncdhw().copy_(want.to(torch.float16))
    out.check("y")
    out.buf[0, 2, 1, 0, out.c0 + out.c] = 0.0                               # one element of the channel after the slice
    with pytest.raises(AssertionError, match="guard channels written"):
        out.check("y")
    assert_bits(out.ncdhw(), want, torch.float16, "y")                       # the addressed channels alone look right


def test_accumulate_rounds_once():
    """dx += t with t an exact fp32 sum of 12 significant bits: one rounding of old + t; rounding t to bf16 first is caught"""
    old = exact_tensor((256,), 10, -100, 100, 1.0, 2.0 ** -4)
    t = torch.randint(-4000, 4001, (256,), generator=torch.Generator().manual_seed(11)).double() * 2.0 ** -7
    once = (old.float() + t.float()).to(torch.bfloat16)
    assert_bits(once, old + t, torch.bfloat16, "dx+", names=None)
    twice = (old.float() + t.float().to(torch.bfloat16).float()).to(torch.bfloat16)   # the new term rounded before the add
    assert not torch.equal(twice, once)
    with pytest.raises(AssertionError, match="wrong"):
        assert_bits(twice, old + t, torch.bfloat16, "dx+", names=None)


def test_within_reports_and_exempts():
    ref = torch.linspace(-1, 1, 101, dtype=torch.float64)
    got = ref + 1e-4
    assert_within(got, ref, 2e-4, names=None)
    got[50] += 1.0
    with pytest.raises(AssertionError, match="1 of 101"):
        assert_within(got, ref, 2e-4, names=None)
    ex = torch.zeros(101, dtype=torch.bool)
    ex[50] = True
    with pytest.raises(AssertionError, match="branch point"):
        assert_within(got, ref, 2e-4, names=None, exempt=ex, max_exempt=1e-3)
    assert_within(got, ref, 2e-4, names=None, exempt=ex, max_exempt=0.01)
