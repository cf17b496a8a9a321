"""Exact-data helpers for the op tests (a plain module, imported by the test files).

Most kernels multiply values that are representable in the storage type and accumulate in fp32.  With small integers times a
power of two as data, and every partial sum below 2^24 units of the product scale, every fp32 sum is exact in ANY order (any
split-K partition, slab reduce, MFMA k-permutation or tile order), so the kernel either returns round-to-nearest-even of the fp64
reference or it is wrong.  `assert_bits` checks exactly that, element by element; `assert_within` is the per-element check for the
ops whose result is not exact; `Guarded` poisons an output and fences it with guard channels."""
import math

import torch

F32_EXACT = 2.0 ** 24        # integers up to here are exact in fp32
FP16_MAX = 65504.0
NAMES5 = ("n", "c", "z", "y", "x")
STORAGE = (torch.float32, torch.bfloat16, torch.float16)


def _is_pow2(s):
    m, _ = math.frexp(s)
    return s > 0 and m == 0.5


def exact_tensor(shape, seed, lo=-4, hi=4, density=0.5, scale=1.0):
    """fp64 tensor of integers in [lo, hi] times the power of two `scale`; a share 1 - density of the entries is forced to zero.
    Every value is exact in bf16, fp16 and fp32, so one fp64 reference serves all three storage types."""
    assert _is_pow2(scale), scale
    assert -256 <= lo <= hi <= 256, (lo, hi)                  # 8 significant bits: exact in bf16
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(lo, hi + 1, tuple(shape), generator=g, dtype=torch.int64).double()
    keep = torch.rand(tuple(shape), generator=g, dtype=torch.float64) < density
    t = torch.where(keep, v, torch.zeros_like(v)) * scale
    for dt in STORAGE:
        assert torch.equal(t.to(dt).double(), t), ("exact_tensor: not representable", dt, lo, hi, scale)
    return t


def assert_exact_precondition(op, operands, scale, terms=None, extra=None, out16=True, what=""):
    """Fail (never skip) unless every output of the reduction `op(*operands)` is exact in fp32 whatever the summation order:
    sum |a*b| / scale < 2^24 for every output, `scale` being the product scale (the power of two every product is a multiple of).
    out16: the result is stored in a 16-bit type, so it must also stay below the fp16 maximum 65504.
    terms: the number of products per output.  When terms * max|a| * max|b| already meets both bounds, that upper bound stands in
    for the op on absolute values (which is then not evaluated); otherwise the bound is op(|a|, |b|, ...), evaluated in fp64.
    op may be None when the cheap bound must suffice.
    extra: further absolute terms added into every output (bias, the old value of an accumulate), a scalar or a tensor
    broadcastable to the output."""
    assert _is_pow2(scale), scale
    ex = 0.0 if extra is None else (extra.abs().max().item() if torch.is_tensor(extra) else abs(float(extra)))
    if terms is not None:
        bound = terms * math.prod(o.abs().max().item() for o in operands) + ex
    if terms is None or bound / scale >= F32_EXACT or (out16 and bound >= FP16_MAX):
        assert op is not None, f"{what}: the cheap bound {bound:.4g} fails and no op was given to tighten it"
        b = op(*[o.abs() for o in operands])
        bound = b.max().item() + ex
    assert bound / scale < F32_EXACT, f"{what}: sum |a*b| = {bound / scale:.4g} product units >= 2^24: fp32 sums are not exact " \
                                      f"-- the test must use a smaller range or density"
    assert not out16 or bound < FP16_MAX, f"{what}: outputs up to {bound:.4g} leave the fp16 range -- the test must use a smaller scale"


def _coords(idx, shape, names):
    out = []
    for flat in idx:
        c = []
        for d in reversed(shape):
            c.append(flat % d)
            flat //= d
        c = tuple(reversed(c))
        out.append(dict(zip(names, c)) if names and len(names) == len(shape) else c)
    return out


def _report(what, bad, got, want, names, extra=None, first=6):
    idx = bad.flatten().nonzero().flatten()[:first].tolist()
    gf, wf = got.flatten(), want.flatten()
    lines = [f"{what}: {int(bad.sum())} of {bad.numel()} elements wrong; first:"]
    for i, c in zip(idx, _coords(idx, tuple(bad.shape), names)):
        line = f"  {c}: got {gf[i].item()!r} want {wf[i].item()!r}"
        if extra is not None:
            line += f" bound {extra.flatten()[i].item():.3g}"
        lines.append(line)
    return "\n".join(lines)


def assert_bits(got, want, dtype, what="", names=NAMES5):
    """got (stored in `dtype`, any device) == want.to(fp32).to(dtype), i.e. round to nearest even of the exact fp32 value of the
    fp64 reference `want` (the sign of a zero is not compared).  `names` labels the coordinates of a failure ((n, c, z, y, x) for an
    activation in NCDHW order) so that it points at a tile edge."""
    want = want.detach().double().cpu()
    w32 = want.to(torch.float32)
    assert torch.equal(w32.double(), want), f"{what}: the reference is not exact in fp32 (a fault in the test)"
    assert got.dtype == dtype, (what, got.dtype, dtype)
    g = got.detach().double().cpu()
    w = w32.to(dtype).double()
    assert g.shape == w.shape, (what, tuple(g.shape), tuple(w.shape))
    bad = ~(g == w)                                   # NaN (an unwritten poisoned element) is never equal
    assert not bad.any(), _report(what, bad, g, w, names)


def assert_within(got, ref, bound, what="", names=NAMES5, exempt=None, max_exempt=1e-3):
    """|got - ref| <= bound per element (bound: a tensor broadcastable to ref, or a scalar).  Elements flagged by `exempt` (e.g. a
    pre-activation within its bound of 0, which may take either LeakyReLU branch) are not compared, but there may be at most a
    share `max_exempt` of them."""
    g = got.detach().double().cpu()
    r = ref.detach().double().cpu()
    b = torch.as_tensor(bound, dtype=torch.float64).cpu().expand_as(r)
    ok = (g - r).abs() <= b                                # NaN fails
    if exempt is not None:
        exempt = exempt.cpu().expand_as(r)
        n_ex = int(exempt.sum())
        assert n_ex <= max_exempt * r.numel(), f"{what}: {n_ex} of {r.numel()} elements within the bound of a branch point"
        ok = ok | exempt
    assert ok.all(), _report(what, ~ok, g, r, names, extra=b)


class Guarded:
    """An output written into the channel slice [guard, guard + c) of a (n, z, y, x, c + 2 * guard) buffer, as the plan writes through
    concat views.  The guard channels hold a sentinel; the addressed channels hold NaN (a call that must write every element) or
    `init_ncdhw` (the old values of an accumulating call, in NCDHW order)."""

    def __init__(self, n, dims, c, dtype, device="cuda", init_ncdhw=None, guard=32):
        ld = c + 2 * guard
        buf = torch.empty((n, *dims, ld), dtype=dtype, device=device)
        sent = -(97.0 + torch.arange(2 * guard, dtype=torch.float64))      # a different value per guard channel
        buf[..., :guard] = sent[:guard].to(dtype).to(device)
        buf[..., guard + c:] = sent[guard:].to(dtype).to(device)
        if init_ncdhw is None:
            buf[..., guard:guard + c] = float("nan")
        else:
            buf[..., guard:guard + c] = init_ncdhw.permute(0, 2, 3, 4, 1).to(dtype).to(device)
        self.buf, self.c0, self.c = buf, guard, c
        self.snap = torch.cat([buf[..., :guard], buf[..., guard + c:]], -1).clone()

    def act(self, ops):
        return ops.Act(self.buf, self.c0, self.c)

    def ncdhw(self):
        return self.buf[..., self.c0:self.c0 + self.c].permute(0, 4, 1, 2, 3)

    def check(self, what=""):
        """the guard channels are bit-identical to what they were, and no addressed element is NaN (was left unwritten)"""
        now = torch.cat([self.buf[..., :self.c0], self.buf[..., self.c0 + self.c:]], -1)
        bits = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}[self.buf.dtype]
        bad = now.view(bits) != self.snap.view(bits)
        assert not bad.any(), _report(f"{what}: guard channels written", bad.cpu(), now.double().cpu(), self.snap.double().cpu(),
                                      ("n", "z", "y", "x", "guard channel"))
        nan = torch.isnan(self.ncdhw())
        assert not nan.any(), _report(f"{what}: elements left unwritten (NaN)", nan.cpu(), self.ncdhw().double().cpu(),
                                      torch.zeros(nan.shape, dtype=torch.float64), NAMES5)


def poisoned(shape, dtype=torch.float32, device="cuda"):
    """a NaN-filled output for a call that must write every element (the exact / per-element checks then catch a missed one)"""
    return torch.full(tuple(shape), float("nan"), dtype=dtype, device=device)


U32 = 2.0 ** -24             # unit roundoff of fp32


def gamma(n):
    """Higham's gamma_n = n u / (1 - n u): the relative error bound of an fp32 sum of n terms in ANY order, against the sum of
    their magnitudes"""
    return n * U32 / (1 - n * U32)


def half_ulp(v, dtype):
    """half an ulp of `dtype` at |v| (fp64 tensor): the error of one round-to-nearest into dtype; 0 for fp32 (no output rounding)"""
    if dtype == torch.float32:
        return torch.zeros_like(v)
    mant, emin = {torch.bfloat16: (8, -126), torch.float16: (11, -14)}[dtype]
    e = torch.floor(torch.log2(v.abs().clamp(min=2.0 ** emin)))
    return torch.exp2(e - mant)        # 2^(e - (p - 1)) / 2
