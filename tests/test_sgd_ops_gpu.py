"""GPU (-m gpu): the SGD entries of rx_pack_optim.hip called through the C ABI -- rx_sgd_flat_multi and rx_sgd_pack -- each output
held per element to the fp32 error bound of tests/sgd_ref.py around an fp64 SGD evaluated from the device's own previous (p, buf).
Every tensor sits between sentinel fences inside a larger buffer; a momentum buffer that a first step must only write, and the packed
copies, are NaN before the call."""
import ctypes

import pytest
import torch

from sgd_ref import CLIP, HYPERS, RATIOS, check_step, make_inputs, next_grad, sgd_args
from test_optim_ops_gpu import BITS, Arena, L, _ptr, _sync  # noqa: F401  (L: the module fixture)

pytestmark = pytest.mark.gpu

IDS = ["lr%g_mu%g_damp%g_wd%g_%s" % (h[0], h[1], h[2], h[3], "nesterov" if h[4] else "plain") for h in HYPERS]


def _dev_clip(with_clip):
    """(device scalar or None, the fp32 value it holds or None)"""
    if not with_clip:
        return None, None
    t = torch.tensor([CLIP], dtype=torch.float32, device="cuda")
    return t, t.item()


def _print_ratios(key):
    r = RATIOS.get(key)
    if r:
        print(f"{key}: largest error / bound p' {r[0]:.3f} buf' {r[1]:.3f}")


def _flat_multi(L, P, G, Bf, hyper, first, clip_t):
    k = len(P)
    VP, LP = ctypes.c_void_p * k, ctypes.c_long * k
    bufs = VP(*[t.data_ptr() for t in Bf]) if Bf is not None else None
    lr, mu, damp, wd, nesterov = hyper
    rc = L.load().rx_sgd_flat_multi(k, VP(*[t.data_ptr() for t in P]), VP(*[t.data_ptr() for t in G]), bufs,
                                    LP(*[t.numel() for t in P]), _ptr(clip_t), lr, mu, damp, wd, int(nesterov), int(first), L.stream_ptr())
    _sync()
    return rc


def _run_flat_multi(L, sizes, p_shifts, hyper, first, with_clip, seed, what):
    """two consecutive calls (the second never `first`).  All tensors of one array share one fenced arena; without momentum there
    is no buffer arena and the call gets a NULL `buf`."""
    clip_t, clip = _dev_clip(with_clip)
    mom = hyper[1] != 0
    ap, ag = Arena(sizes, shifts=p_shifts), Arena(sizes)
    ab = Arena(sizes) if mom else None
    ins = [make_inputs(n, seed + j, first, hyper) for j, n in enumerate(sizes)]
    for j in range(len(sizes)):
        ap.views[j].copy_(ins[j][0]), ag.views[j].copy_(ins[j][1])
        if mom and not first:
            ab.views[j].copy_(ins[j][2])                   # (first: the buffers stay NaN -- they must be written, never read)
    P, G, Bf = ap.views, ag.views, (ab.views if mom else None)
    for k in range(2):
        fk = first and k == 0
        if k:
            for j, gv in enumerate(G):
                gv.copy_(next_grad(gv.numel(), seed + j, k))
        before = [(P[j].cpu(), Bf[j].cpu() if mom and not fk else None) for j in range(len(sizes))]
        gbits = ag.bits()
        L.check(_flat_multi(L, P, G, Bf, hyper, fk, clip_t), "rx_sgd_flat_multi")
        args = sgd_args(*hyper, fk)
        for j in range(len(sizes)):
            check_step((P[j], Bf[j] if mom else None), before[j], G[j].cpu(), clip, args, f"{what}: tensor {j} of {sizes[j]} call {k}")
        assert torch.equal(ag.bits(), gbits), "grad written"
        for a in (ap, ag, ab):
            if a is not None:
                a.check(what)
    _print_ratios(what)


# one tensor of every size around the 4096-element chunk, and an 8192-element one whose p starts 4 bytes off a 16-byte boundary
# (the whole tensor on the scalar path between neighbours on the 16-byte path)
SIZES = [1, 3, 4095, 4096, 4097, 2 * 4096 + 5, 8192]
SHIFTS = [0, 0, 0, 0, 0, 0, 1]


@pytest.mark.parametrize("with_clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("first", [True, False], ids=["first", "later"])
@pytest.mark.parametrize("hi", range(len(HYPERS)), ids=IDS)
def test_sgd_flat_multi_per_element(L, hi, first, with_clip):
    _run_flat_multi(L, SIZES, SHIFTS, HYPERS[hi], first, with_clip, 300 + 10 * hi, "sgd_flat_multi")


@pytest.mark.parametrize("first", [True, False], ids=["first", "later"])
def test_sgd_flat_multi_49_tensors_take_two_launches(L, first):
    """one more tensor than the table holds; sizes around the chunk mixed with small ragged ones"""
    base = [1, 3, 255, 4095, 4096, 4097, 8192, 12289]
    sizes = [base[j % 8] if j % 3 == 0 else 17 + 131 * j for j in range(49)]
    _run_flat_multi(L, sizes, None, HYPERS[0 if first else 2], first, True, 700, "sgd_flat_multi")


@pytest.mark.parametrize("which", ["g", "buf"])
def test_sgd_flat_multi_other_misaligned_arrays(L, which):
    """`vec` ORs the three pointers: a misaligned grad or buf alone must also send the tensor down the scalar path"""
    hyper = HYPERS[0]
    sizes = [4096, 8192, 4097]
    clip_t, clip = _dev_clip(True)
    ap = Arena(sizes)
    ag = Arena(sizes, shifts=[0, 1, 0] if which == "g" else None)
    ab = Arena(sizes, shifts=[0, 1, 0] if which == "buf" else None)
    for j, n in enumerate(sizes):
        for a, t in zip((ap, ag, ab), make_inputs(n, 800 + j, False, hyper)):
            a.views[j].copy_(t)
    before = [(p.cpu(), b.cpu()) for p, b in zip(ap.views, ab.views)]
    L.check(_flat_multi(L, ap.views, ag.views, ab.views, hyper, False, clip_t), "rx_sgd_flat_multi")
    for j in range(3):
        check_step((ap.views[j], ab.views[j]), before[j], ag.views[j].cpu(), clip, sgd_args(*hyper, False), f"sgd_flat_multi: misaligned {which} {j}")
    for a in (ap, ag, ab):
        a.check("sgd_flat_multi")


def test_sgd_flat_multi_refuses_bad_arguments(L):
    """each RX_EINVAL condition returns its code and writes nothing"""
    sizes = [4096, 100]
    ap, ag, ab = Arena(sizes), Arena(sizes), Arena(sizes)
    for a in (ap, ag, ab):
        for v in a.views:
            v.fill_(1.0)
    snaps = [a.bits() for a in (ap, ag, ab)]
    so = L.load()
    VP, LP = ctypes.c_void_p * 2, ctypes.c_long * 2
    P, G, Bf = (VP(*[t.data_ptr() for t in a.views]) for a in (ap, ag, ab))
    N = LP(*sizes)
    ok = dict(count=2, p=P, g=G, buf=Bf, n=N, mu=0.9, damp=0.0, nesterov=1)
    bad = [dict(count=-1), dict(p=None), dict(g=None), dict(n=None), dict(buf=None), dict(n=LP(4096, 0)), dict(p=VP(ap.views[0].data_ptr(), 0)),
           dict(g=VP(0, ag.views[1].data_ptr())), dict(buf=VP(ab.views[0].data_ptr(), 0)), dict(mu=0.0, buf=None), dict(mu=-0.5),
           dict(damp=0.1)]
    einval = None
    for change in bad:
        a = dict(ok, **change)
        rc = so.rx_sgd_flat_multi(a["count"], a["p"], a["g"], a["buf"], a["n"], None, 1e-2, a["mu"], a["damp"], 0.0, a["nesterov"], 0,
                                  L.stream_ptr())
        _sync()
        assert rc != 0 and b"rx_sgd_flat_multi" in so.rx_last_error(), change
        einval = rc if einval is None else einval
        assert rc == einval, (change, rc)                       # one code for all of them: RX_EINVAL
        for arena, snap in zip((ap, ag, ab), snaps):
            assert torch.equal(arena.bits(), snap), change
    assert so.rx_adamw_flat_multi(-1, None, None, None, None, None, None, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, L.stream_ptr()) == einval
    assert so.rx_sgd_flat_multi(0, None, None, None, None, None, 1e-2, 0.9, 0.0, 0.0, 1, 0, L.stream_ptr()) == 0      # nothing to do


# ---- rx_sgd_pack -----------------------------------------------------------------------------------------------------------------
# (kind, A, B, taps): the 16-byte path; ragged tiles of multiples of 8 (the f16 tie case named above `stored_f32`); TT == 1; convT
PACK_CASES = [(0, 32, 32, 27), (0, 40, 24, 27), (0, 64, 32, 1), (1, 8, 40, 8)]


def _repack(L, code, p, kind, A, B, taps, dtype):
    """both packed copies of the fp32 weight `p` as the engine's own packers write them (rx_pack_conv_weight / rx_pack_convT_weight)"""
    n = A * B * taps
    wf, wb = (torch.full((n,), float("nan"), dtype=dtype, device="cuda") for _ in range(2))
    fn = L.load().rx_pack_conv_weight if kind == 0 else L.load().rx_pack_convT_weight
    L.check(fn(code, _ptr(p), A, B, taps, _ptr(wf), _ptr(wb), L.stream_ptr()), "rx_pack")
    _sync()
    return wf, wb


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bfloat16", "float16"])
@pytest.mark.parametrize("ci", range(len(PACK_CASES)), ids=lambda i: "k%d_%dx%dx%d" % PACK_CASES[i])
def test_sgd_pack_per_element(L, dtype, ci):
    """three consecutive rx_sgd_pack calls starting with a first step (NaN momentum buffer): p' and buf' per element inside the bound,
    grad untouched, both packed copies bit-equal to what rx_pack_conv(T)_weight writes from the device's own p', fences intact"""
    kind, A, B, taps = PACK_CASES[ci]
    hyper = HYPERS[ci]                              # nesterov + wd, nesterov, dampening + wd, plain momentum
    lr, mu, damp, wd, nesterov = hyper
    clip_t, clip = _dev_clip(ci != 2)
    n = A * B * taps
    p0, g0, _ = make_inputs(n, 40 + ci, True, hyper)
    f = Arena([n, n, n])
    p, g, buf = f.views
    p.copy_(p0), g.copy_(g0)
    packs = Arena([n, n], dtype)
    wf, wb = packs.views
    code = L.DTYPE_CODE[dtype]
    what = "sgd_pack"
    for k in range(3):
        first = k == 0
        if k:
            g.copy_(next_grad(n, 40 + ci, k))
        for w in packs.views:
            w.fill_(float("nan"))
        before, gbits = (p.cpu(), None if first else buf.cpu()), g.view(torch.int32).clone()
        L.check(L.load().rx_sgd_pack(code, _ptr(p), _ptr(g), _ptr(buf), _ptr(clip_t), lr, mu, damp, wd, int(nesterov), int(first), kind, A, B,
                                     taps, _ptr(wf), _ptr(wb), L.stream_ptr()), "rx_sgd_pack")
        _sync()
        check_step((p, buf), before, g.cpu(), clip, sgd_args(*hyper, first), f"{what}: case {ci} {dtype} call {k}")
        assert torch.equal(g.view(torch.int32), gbits), "grad written"
        ef, eb = _repack(L, code, p, kind, A, B, taps, dtype)
        for name, got, want in (("w_fwd", wf, ef), ("w_bwd", wb, eb)):
            assert not torch.isnan(got).any(), f"{what}: case {ci} call {k} {name} left unwritten (NaN)"
            bad = got.view(BITS[dtype]) != want.view(BITS[dtype])
            assert not bad.any(), f"{what}: case {ci} call {k} {name}: {int(bad.sum())} of {n} elements are not the pack of the stored p'"
        f.check(what), packs.check(what)
    _print_ratios(what)


def test_sgd_pack_without_momentum(L):
    """momentum == 0: NULL buf, u = d"""
    kind, A, B, taps = PACK_CASES[1]
    hyper = HYPERS[6]
    lr, mu, damp, wd, nesterov = hyper
    n = A * B * taps
    f = Arena([n, n])
    p, g = f.views
    p0, g0, _ = make_inputs(n, 60, True, hyper)
    p.copy_(p0), g.copy_(g0)
    packs = Arena([n, n], torch.bfloat16)
    before = (p.cpu(), None)
    code = L.DTYPE_CODE[torch.bfloat16]
    L.check(L.load().rx_sgd_pack(code, _ptr(p), _ptr(g), None, None, lr, mu, damp, wd, 0, 0, kind, A, B, taps, _ptr(packs.views[0]),
                                 _ptr(packs.views[1]), L.stream_ptr()), "rx_sgd_pack")
    _sync()
    check_step((p, None), before, g.cpu(), None, sgd_args(*hyper, False), "sgd_pack: no momentum")
    ef, eb = _repack(L, code, p, kind, A, B, taps, torch.bfloat16)
    assert torch.equal(packs.views[0].view(torch.int16), ef.view(torch.int16)) and torch.equal(packs.views[1].view(torch.int16), eb.view(torch.int16))
    f.check("sgd_pack"), packs.check("sgd_pack")


def test_sgd_pack_refuses_bad_arguments(L):
    A, B, taps = 32, 32, 3
    n = A * B * taps
    f = Arena([n, n, n])
    for v in f.views:
        v.fill_(1.0)
    packs = Arena([n, n], torch.bfloat16)
    snap, psnap = f.bits(), packs.bits()
    p, g, buf = f.views
    so = L.load()
    ok = dict(p=p, g=g, buf=buf, mu=0.9, damp=0.0, nesterov=1, A=A, B=B, taps=taps)
    bad = [dict(p=None), dict(g=None), dict(buf=None), dict(taps=0), dict(taps=28), dict(A=0), dict(B=0), dict(mu=0.0, buf=None), dict(mu=-0.5),
           dict(damp=0.1)]
    for change in bad:
        a = dict(ok, **change)
        rc = so.rx_sgd_pack(L.DTYPE_CODE[torch.bfloat16], _ptr(a["p"]), _ptr(a["g"]), _ptr(a["buf"]), None, 1e-2, a["mu"], a["damp"], 0.0,
                            a["nesterov"], 0, 0, a["A"], a["B"], a["taps"], _ptr(packs.views[0]), _ptr(packs.views[1]), L.stream_ptr())
        _sync()
        assert rc != 0 and b"rx_sgd_pack" in so.rx_last_error(), change
        assert rc == so.rx_adamw_pack(L.DTYPE_CODE[torch.bfloat16], None, None, None, None, None, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 0, A, B, taps,
                                      None, None, L.stream_ptr()), change                # RX_EINVAL, as its neighbour
        assert torch.equal(f.bits(), snap) and torch.equal(packs.bits(), psnap), change
