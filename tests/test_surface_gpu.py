"""GPU: rx_mask_edges, rx_edt_sq and rx_surface_hist (csrc/rx_surface.hip) through engine.ops against the numpy statements of
training/metrics/surface.py, and `ValidationMetrics` with a `surface` block.  Every device result is an integer and every score is
host float64 of the same integers, so everything is compared with `np.array_equal` / `==`: there is no tolerance in this file."""
import numpy as np
import pytest
import torch

import mt3d_amd  # noqa: F401
from mt3d_amd.training import metrics as M
from mt3d_amd.training.metrics import surface as S

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
# one voxel; one line longer than a wave along x and along y; a unit axis in the middle; small odd extents; several workgroups per
# pass; y and z lines longer than 128; y and x lines longer than 256 (narrower line tiles, fewer rows per workgroup); the largest
# extent (the largest LDS tile: 16 lines of 1024)
SHAPES = [(1, 1, 1), (1, 1, 70), (1, 70, 1), (5, 1, 3), (9, 10, 12), (33, 17, 70), (3, 130, 5), (130, 3, 5), (2, 257, 20), (2, 3, 257),
          (1024, 3, 3)]
THR = 0.25      # exact in every dtype
_CASES = {}


def ops():
    from mt3d_amd.engine import ops as E
    return E


def rng_of(shape, salt=0):
    return np.random.default_rng(1000 * salt + shape[0] * 7 + shape[1] * 3 + shape[2])


# ---- edt_sq -------------------------------------------------------------------------------------------------------------------------
def feature_sets(shape):
    """the seven feature volumes of a shape: empty, full, one voxel at each of two opposite corners, a plane, random 0.02 and 0.9"""
    r = rng_of(shape)
    first, last, plane = (np.zeros(shape, dtype=bool) for _ in range(3))
    first[0, 0, 0], last[-1, -1, -1] = True, True
    plane[shape[0] // 2] = True
    return {"empty": np.zeros(shape, dtype=bool), "full": np.ones(shape, dtype=bool), "first": first, "last": last, "plane": plane,
            "sparse": r.random(shape) < 0.02, "dense": r.random(shape) < 0.9}


def edt_case(shape):
    """two (2, 2, Z, Y, X) batches of four DIFFERENT volumes each, and their oracles; made once, never written to"""
    if ("edt", shape) not in _CASES:
        f = feature_sets(shape)
        want = {k: S.edt_sq_numpy(v) for k, v in f.items()}
        batches = []
        for names in (("empty", "full", "first", "sparse"), ("last", "plane", "dense", "empty")):
            batches.append((np.stack([f[k] for k in names]).reshape((2, 2) + shape), np.stack([want[k] for k in names]).reshape((2, 2) + shape)))
        _CASES[("edt", shape)] = batches
    return _CASES[("edt", shape)]


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_edt_sq_equals_the_statement(shape):
    for i, (feature, want) in enumerate(edt_case(shape)):
        f = torch.from_numpy(feature).cuda()
        got = ops().edt_sq(f if i else f.to(torch.uint8))      # bool and uint8 storage alike
        assert got.dtype == torch.int32 and tuple(got.shape) == (2, 2) + shape
        assert np.array_equal(got.cpu().numpy(), want)
    assert (want[1, 1] == S.EDT_NONE).all() and want[0, 0].max() < S.EDT_NONE      # the empty volume next to finite ones
    out = torch.full((2, 2) + shape, -7, dtype=torch.int32, device="cuda")
    assert ops().edt_sq(f, out=out) is out and np.array_equal(out.cpu().numpy(), want)
    # values other than 0 / 1 are features too
    g = f.to(torch.uint8) * 200
    assert np.array_equal(ops().edt_sq(g).cpu().numpy(), want)


# ---- mask_edges -----------------------------------------------------------------------------------------------------------------------
def edges_case(shape, dtype):
    """(2, 2, Z, Y, X) values in `dtype`: volume (0, 0) random with values exactly at the threshold and a NaN; (0, 1) a full mask,
    and behind it (1, 0) with an EMPTY first slice; (1, 0) ends in a full slice and (1, 1) starts with one (and is dense)"""
    key = ("edges", shape, dtype)
    if key not in _CASES:
        g = torch.Generator().manual_seed(sum(shape) + 17 * DTYPES.index(dtype))
        v = torch.randn((2, 2) + shape, generator=g).to(dtype)
        flat = v[0, 0].reshape(-1)
        flat[::3] = THR      # at the threshold: not above it, so not in the mask
        flat[flat.numel() // 2] = float("nan")
        v[0, 1] = 1.0
        v[1, 0, 0], v[1, 0, -1] = -1.0, 1.0
        v[1, 1] = (torch.rand(shape, generator=g) < 0.9).to(dtype) * 2.0 - 1.0
        v[1, 1, 0] = 1.0
        if shape[0] == 1:      # one slice: keep sample 1's first volume empty behind the full one
            v[1, 0] = -1.0
        h = v.float().numpy()
        want = np.stack([S.edges_numpy(h[n, c] > np.float32(THR)) for n in range(2) for c in range(2)]).reshape(h.shape).astype(np.uint8)
        _CASES[key] = (v, want)
    return _CASES[key]


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).replace("torch.", ""))
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_mask_edges_equals_the_statement(shape, dtype):
    v, want = edges_case(shape, dtype)
    got = ops().mask_edges(v.cuda(), THR)
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
    # the full mask: only the volume's shell
    shell = np.ones(shape, dtype=bool)
    shell[1:-1, 1:-1, 1:-1] = False
    assert np.array_equal(want[0, 1].astype(bool), shell)
    out = torch.full(v.shape, 9, dtype=torch.uint8, device="cuda")
    assert ops().mask_edges(v.cuda(), THR, out=out) is out and np.array_equal(out.cpu().numpy(), want)


# ---- surface_hist ---------------------------------------------------------------------------------------------------------------------
HSHAPE = (9, 20, 24)


def hist_pairs():
    """four (prediction, target) volumes: a plane against itself shifted by 3, a random pair, target empty, both empty"""
    if "pairs" not in _CASES:
        r = rng_of(HSHAPE, salt=2)
        zero = np.zeros(HSHAPE, dtype=np.float32)
        a, b = zero.copy(), zero.copy()
        a[2], b[5] = 1.0, 1.0
        ra = (r.random(HSHAPE) < 0.3).astype(np.float32) * r.random(HSHAPE).astype(np.float32)
        rb = (r.random(HSHAPE) < 0.2).astype(np.float32)
        pairs = [(a, b), (ra, rb), (a, zero), (zero, zero)]
        _CASES["pairs"] = (pairs, [S.surface_hist_numpy(p, t, THR, 0.5) for p, t in pairs])
    return _CASES["pairs"]


def as_batch(vols, n, c, dtype=torch.float32):
    return torch.from_numpy(np.stack(vols).reshape((n, c) + HSHAPE)).to(dtype).cuda()


@pytest.mark.parametrize("i", range(4), ids=["shifted-plane", "random", "one-side-empty", "both-empty"])
def test_surface_hist_of_one_pair(i):
    pairs, wants = hist_pairs()
    hist, counts = ops().surface_hist(as_batch([pairs[i][0]], 1, 1), as_batch([pairs[i][1]], 1, 1), THR, 0.5)
    assert hist.dtype == counts.dtype == torch.int64 and tuple(hist.shape) == (2, S.default_bins(HSHAPE))
    assert np.array_equal(hist.cpu().numpy(), wants[i][0]) and np.array_equal(counts.cpu().numpy(), wants[i][1])
    if i == 0:
        assert wants[0][0][0, 9] == wants[0][0][1, 9] == 20 * 24 and wants[0][0].sum() == 2 * 20 * 24
    if i == 2:      # nothing to match: the `unmatched` path, `hist` untouched
        assert wants[2][0].sum() == 0 and wants[2][1].tolist() == [480, 0, 480, 0]
    if i == 3:
        assert wants[3][0].sum() == 0 and wants[3][1].tolist() == [0, 0, 0, 0]


def test_surface_hist_pools_a_batch_and_accumulates_over_calls():
    pairs, wants = hist_pairs()
    E = ops()
    pred, target = as_batch([p for p, _ in pairs], 2, 2), as_batch([t for _, t in pairs], 2, 2)
    bins = S.default_bins(HSHAPE)
    hist = torch.zeros((2, bins), dtype=torch.int64, device="cuda")
    counts = torch.zeros(4, dtype=torch.int64, device="cuda")
    scratch = E.surface_scratch(pred.shape, pred.device)
    E.surface_hist(pred, target, THR, 0.5, hist=hist, counts=counts, scratch=scratch)      # warm: code objects loaded
    hist.zero_(), counts.zero_()
    # the second call: the random pair alone, as a bfloat16 prediction (the oracle sees the rounded values)
    p16, t1 = as_batch([pairs[1][0]], 1, 1, torch.bfloat16), as_batch([pairs[1][1]], 1, 1)
    s1 = E.surface_scratch(p16.shape, p16.device)
    torch.cuda.set_sync_debug_mode("error")      # no host synchronisation in either call
    try:
        got = E.surface_hist(pred, target, THR, 0.5, hist=hist, counts=counts, scratch=scratch)
        E.surface_hist(p16, t1, THR, 0.5, hist=hist, counts=counts, scratch=s1)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert got[0] is hist and got[1] is counts
    want16 = S.surface_hist_numpy(p16[0, 0].float().cpu().numpy(), pairs[1][1], THR, 0.5)
    want_h = sum(w[0] for w in wants) + want16[0]
    want_c = sum(w[1] for w in wants) + want16[1]
    assert np.array_equal(hist.cpu().numpy(), want_h) and np.array_equal(counts.cpu().numpy(), want_c)


def test_surface_hist_allocates_nothing_with_scratch():
    pairs, _ = hist_pairs()
    E = ops()
    pred, target = as_batch([pairs[1][0]], 1, 1), as_batch([pairs[1][1]], 1, 1)
    hist = torch.zeros((2, S.default_bins(HSHAPE)), dtype=torch.int64, device="cuda")
    counts = torch.zeros(4, dtype=torch.int64, device="cuda")
    scratch = E.surface_scratch(pred.shape, pred.device)
    E.surface_hist(pred, target, THR, 0.5, hist=hist, counts=counts, scratch=scratch)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    E.surface_hist(pred, target, THR, 0.5, hist=hist, counts=counts, scratch=scratch)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() == before == torch.cuda.memory_allocated()


def test_surface_hist_with_few_bins_fills_the_last_bin():
    pairs, _ = hist_pairs()
    for i in (0, 1):
        want = S.surface_hist_numpy(pairs[i][0], pairs[i][1], THR, 0.5, bins=5)
        hist = torch.zeros((2, 5), dtype=torch.int64, device="cuda")
        _, counts = ops().surface_hist(as_batch([pairs[i][0]], 1, 1), as_batch([pairs[i][1]], 1, 1), THR, 0.5, hist=hist)
        assert np.array_equal(hist.cpu().numpy(), want[0]) and np.array_equal(counts.cpu().numpy(), want[1])
    assert S.surface_hist_numpy(pairs[0][0], pairs[0][1], THR, 0.5, bins=5)[0].tolist() == [[0, 0, 0, 0, 480], [0, 0, 0, 0, 480]]
    # distances past the bins kept in LDS: a plane against one 20 voxels away, d^2 = 400
    shape = (24, 6, 7)
    a, b = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
    a[1], b[21] = 1.0, 1.0
    want = S.surface_hist_numpy(a, b, THR, 0.5)
    hist, counts = ops().surface_hist(torch.from_numpy(a).cuda()[None, None], torch.from_numpy(b).cuda()[None, None], THR, 0.5)
    assert want[0][0, 400] == 42 and np.array_equal(hist.cpu().numpy(), want[0]) and np.array_equal(counts.cpu().numpy(), want[1])


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_the_wrappers_refuse_what_they_do_not_take():
    from mt3d_amd.engine.lib import RxError
    E = ops()
    v = torch.zeros((1, 1, 4, 5, 6), device="cuda")
    f = torch.zeros((1, 1, 4, 5, 6), dtype=torch.uint8, device="cuda")
    for call in (lambda: E.mask_edges(v.cpu(), 0.5), lambda: E.edt_sq(f.cpu()), lambda: E.surface_hist(v.cpu(), v.cpu(), 0.5, 0.5),
                 lambda: E.surface_hist(v, v.cpu(), 0.5, 0.5)):      # CPU tensors
        with pytest.raises(RxError):
            call()
    for call in (lambda: E.mask_edges(v.double(), 0.5), lambda: E.mask_edges(f, 0.5), lambda: E.edt_sq(v), lambda: E.edt_sq(f.to(torch.int32)),
                 lambda: E.surface_hist(f, v, 0.5, 0.5)):      # other dtypes
        with pytest.raises(RxError, match="dtype"):
            call()
    with pytest.raises(RxError, match="float32"):      # the target is float32
        E.surface_hist(v, v.to(torch.bfloat16), 0.5, 0.5)
    with pytest.raises(RxError, match="shape"):
        E.surface_hist(v, v[:, :, :3], 0.5, 0.5)
    for call in (lambda: E.mask_edges(v[0], 0.5), lambda: E.edt_sq(f[0]), lambda: E.surface_hist(v[0], v[0], 0.5, 0.5)):      # a 2-D patch
        with pytest.raises(RxError, match=r"\(N, C, Z, Y, X\)"):
            call()
    big = torch.zeros((1, 1, 1, 1025, 1), device="cuda")
    for call in (lambda: E.mask_edges(big, 0.5), lambda: E.edt_sq(big.to(torch.uint8)), lambda: E.surface_hist(big, big, 0.5, 0.5)):
        with pytest.raises(RxError, match="1024"):
            call()
    for bad in (torch.zeros((3, 8), dtype=torch.int64, device="cuda"), torch.zeros((2, 8), dtype=torch.int32, device="cuda"),
                torch.zeros(16, dtype=torch.int64, device="cuda"), torch.zeros((2, 8), dtype=torch.int64)):
        with pytest.raises(RxError, match="hist"):
            E.surface_hist(v, v, 0.5, 0.5, hist=bad)
    with pytest.raises(RxError, match="counts"):
        E.surface_hist(v, v, 0.5, 0.5, counts=torch.zeros(3, dtype=torch.int64, device="cuda"))
    with pytest.raises(RxError, match="scratch"):
        E.surface_hist(v, v, 0.5, 0.5, scratch=(f, f))
    with pytest.raises(RxError, match="scratch"):
        E.surface_hist(v, v, 0.5, 0.5, scratch=(f, f, f))
    with pytest.raises(RxError, match="out"):
        E.edt_sq(f, out=torch.zeros((1, 1, 4, 5, 6), dtype=torch.int64, device="cuda"))


# ---- ValidationMetrics ------------------------------------------------------------------------------------------------------------------
TASKS = {"sheet": {"channels": 1, "activation": "none"}, "normals": {"channels": 3, "activation": "none"}}
VSHAPE = (12, 20, 24)


def val_batches():
    """two batches of (2, 1, 12, 20, 24) logits against a bent two-voxel sheet, and (2, 3, ...) normals"""
    r = np.random.default_rng(5)
    out = []
    for b in range(2):
        zz, yy, xx = np.meshgrid(np.arange(VSHAPE[0]), np.arange(VSHAPE[1]), np.arange(VSHAPE[2]), indexing="ij")
        tgt, prd = [], []
        for n in range(2):
            mid = 4 + b + n + 2.0 * np.sin(xx / 9.0 + n) * np.cos(yy / 11.0)
            t = ((zz >= mid) & (zz < mid + 2)).astype(np.float32)
            p = (((zz >= mid + 1.2 * n) & (zz < mid + 2.4)) ^ (r.random(VSHAPE) < 0.01)).astype(np.float32) * 4.0 - 2.0      # logits
            tgt.append(t), prd.append(p)
        sheet_t, sheet_p = np.stack(tgt)[:, None], np.stack(prd)[:, None]
        nt = r.standard_normal((2, 3) + VSHAPE).astype(np.float32) * sheet_t
        npred = r.standard_normal((2, 3) + VSHAPE).astype(np.float32)
        out.append(({"sheet": sheet_p, "normals": npred}, {"sheet": sheet_t, "normals": nt}))
    return out


def test_validation_metrics_with_a_surface_block():
    batches = val_batches()
    vm = M.ValidationMetrics(TASKS, {"surface": {"tolerances": [0, 1, 1.5]}})
    plain = M.ValidationMetrics(TASKS, True)
    assert vm.surface == {"tolerances": (0.0, 1.0, 1.5), "tasks": ("sheet",)} and plain.surface is None
    dev = [({k: torch.from_numpy(v).cuda() for k, v in o.items()}, {k: torch.from_numpy(v).cuda() for k, v in t.items()}) for o, t in batches]
    vm.update(*dev[0]), plain.update(*dev[0])      # the first call creates the buffers
    torch.cuda.set_sync_debug_mode("error")
    try:
        vm.update(*dev[1]), plain.update(*dev[1])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    got, base = vm.compute(), plain.compute()
    hist, counts = 0, 0
    for o, t in batches:
        for n in range(2):
            h, c = S.surface_hist_numpy(o["sheet"][n, 0], t["sheet"][n, 0], 0.0, 0.5)      # `activation: none` at 0.5: logit 0
            hist, counts = hist + h, counts + c
    want = S.surface_scores(hist, counts, (0.0, 1.0, 1.5))
    assert counts[0] > 0 and counts[1] > 0 and 0.0 < want["surface_dice_1"] < 1.0 and want["hd95"] > 0.0
    names = M.metric_names("binary", vm.surface)
    assert list(got["sheet"]) == list(names) and set(want) == set(names) - set(M.metric_names("binary"))
    for k, v in want.items():
        assert got["sheet"][k] == v, (k, got["sheet"][k], v)
    # the pre-existing metrics are those of an accumulator built without `surface`
    assert {k: got["sheet"][k] for k in M.metric_names("binary")} == base["sheet"] and got["normals"] == base["normals"]
    assert list(base["sheet"]) == list(M.metric_names("binary"))
    # a second patch shape is refused: the histogram length is fixed by the first
    small = ({k: v[:, :, :8].contiguous() for k, v in dev[0][0].items()}, {k: v[:, :, :8].contiguous() for k, v in dev[0][1].items()})
    with pytest.raises(ValueError, match="shape"):
        vm.update(*small)
    plain.update(*small)      # ... by the surface block only
    vm.reset()
    cleared = vm.compute()["sheet"]
    assert cleared["surface_voxels"] == 0.0 and all(v != v for k, v in cleared.items() if k != "surface_voxels")
    vm.update(*dev[0])
    h0, c0 = 0, 0
    for n in range(2):
        h, c = S.surface_hist_numpy(batches[0][0]["sheet"][n, 0], batches[0][1]["sheet"][n, 0], 0.0, 0.5)
        h0, c0 = h0 + h, c0 + c
    again = vm.compute()["sheet"]
    for k, v in S.surface_scores(h0, c0, (0.0, 1.0, 1.5)).items():
        assert again[k] == v
