"""The case matrix of the SqueezeExcite / DropPath tests and its inputs (a plain module, shared by tests/test_se_ref_cpu.py, which
entitles the bounds of tests/se_ref.py on an fp32 emulation, and tests/test_se_gpu.py, which holds the kernels to them)."""
import zlib
from collections import namedtuple

import torch

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
SMALL, GENERAL = "se_gate_bwd_small_kernel", "se_gate_bwd_kernel"

# bwd: the gate-backward kernel rx_se_gate_bwd must choose; n = 2 unless given; flag "misaligned": w1 / w2 are views 4 bytes into
# larger buffers; flag "offset": y carries a per-channel offset of about 30 standard deviations
Case = namedtuple("Case", "c rd dims keep_x bwd n flag", defaults=(2, None))
MATRIX = [
    Case(32, 8, (6, 5, 16), 1, SMALL),                    # baseline small kernel, KL = 8
    Case(32, 8, (6, 5, 16), 1, SMALL, flag="offset"),     # |mean| / std ~ 30: the pooled subtraction cancels
    Case(96, 8, (3, 4, 6), 1, SMALL),                     # 256 % C != 0, KL = 2, 64 idle gather threads
    Case(160, 12, (3, 4, 7), 1, SMALL),                   # KL = 1 with threads kl >= KL; rd % 8 != 0; L = 7 (m12 tail only)
    Case(256, 16, (3, 3, 9), 1, SMALL),                   # first C >= 256 gather; L = 9 (unrolled 8 + tail 1)
    Case(264, 16, (2, 3, 4), 1, SMALL),                   # second pass of the c += 256 loops; odd channel-vector count in 16-bit
    Case(512, 32, (2, 2, 2), 1, SMALL),                   # the small kernel's upper limit
    Case(520, 32, (2, 2, 2), 1, GENERAL),                 # first shape above it: general kernel, 16-byte branch
    Case(512, 40, (2, 2, 3), 1, GENERAL),                 # rd > 32: se_mv_rows<64>, se_dot_row with 3 groups
    Case(512, 64, (2, 2, 3), 1, GENERAL),                 # ... and 4 groups
    Case(64, 6, (3, 4, 5), 1, GENERAL),                   # rd % 4 != 0: scalar forward and scalar backward
    Case(64, 1, (3, 4, 5), 1, GENERAL),
    Case(320, 33, (2, 3, 5), 1, GENERAL),
    Case(64, 8, (3, 4, 5), 1, GENERAL, flag="misaligned"),    # the misaligned-weights fallbacks
    Case(2048, 64, (2, 2, 3), 1, GENERAL, n=1),           # RX_SE_MAX_C
    Case(32, 8, (5, 7, 6), 0, SMALL),                     # keep_x = 0, 4 chunks, ragged last (9, 9, 9, 8), X > 1
    Case(32, 8, (1, 37, 6), 0, SMALL),                    # the 2-D net's form, 4 chunks
    Case(32, 8, (32, 33, 4), 1, SMALL),                   # 1056 rows: the `want` clamp of 128, 118 chunks of 9 with a ragged last
    Case(64, 8, (3, 3, 40), 1, SMALL),                    # > 256 (x, vector) pairs: several x segments with a ragged last; L = 40
    Case(32, 0, (4, 4, 8), 1, GENERAL, n=3),              # DropPath only: se_fill_mult_kernel, w1 == nullptr backward
]
# the option cross runs on one small-kernel, one general-kernel and one DropPath-only case
CROSS = [MATRIX[0], MATRIX[10], MATRIX[-1]]
Opts = namedtuple("Opts", "slope residual dres scale", defaults=(0.01, True, "accumulate", True))
OPTIONS = [Opts(s, r, d, p) for s in (0.01, 1.0) for r in (True, False) for d in (None, "overwrite", "accumulate") for p in (False, True)]
DETERMINISM = [MATRIX[17], MATRIX[6]]                     # chunks > 64; C = 512


def case_id(c):
    return f"c{c.c}-rd{c.rd}-{'x'.join(map(str, c.dims))}-k{c.keep_x}" + (f"-{c.flag}" if c.flag else "")


def path_scale(case, on):
    """DropPath factors with one dropped sample (none to drop in a batch of one)"""
    if not on:
        return None
    return torch.tensor({1: [1.25], 2: [1.25, 0.0], 3: [0.0, 1.25, 1.25]}[case.n], dtype=torch.float64)


def make_inputs(case, dtype, opts=Opts()):
    """fp64 inputs whose activations are representable in `dtype` (weights and scale in fp32): the dict tests/se_ref.stage_checks takes"""
    gen = torch.Generator().manual_seed(zlib.crc32(repr(tuple(case)).encode()) % 100000)
    shape = (case.n, case.c, *case.dims)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)                                     # noqa: E731
    y = rnd(*shape)
    if case.flag == "offset":
        y = y + 30.0 * torch.where(rnd(1, case.c, 1, 1, 1) > 0, 1.0, -1.0)
    st = lambda t: t.to(dtype).double()                                                                    # noqa: E731
    y, res, g = st(y), st(rnd(*shape)), st(rnd(*shape) * 0.1)
    se = None
    if case.rd:
        f32 = lambda t: t.float().double()                                                                 # noqa: E731
        se = (f32(rnd(case.rd, case.c) * 2 * case.c ** -0.5), f32(rnd(case.rd) * 0.1),
              f32(rnd(case.c, case.rd) * case.rd ** -0.5), f32(rnd(case.c) * 0.1))
    old = st(rnd(*shape) * 0.5) if opts.dres == "accumulate" else None
    return dict(y=y, res=res if opts.residual else None, g=g, se=se, scale=path_scale(case, opts.scale), keep_x=case.keep_x,
                slope=opts.slope, dtype=dtype, old_dres=old, has_dres=opts.dres is not None)
