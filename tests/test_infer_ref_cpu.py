"""The checkers of tests/infer_ref.py against numpy, without a device: an fp32 twin of every statement (float32 arithmetic in slot
order; the softmax takes expf as a correctly rounded fp32 function) passes every checker over the whole case table, so no bound is too tight; and every deliberately wrong variant of the twin
is rejected by a case named here, so no bound is vacuous and no case is idle.  A mutant the table cannot reject means the table
lacks a case."""
import numpy as np
import pytest

import infer_ref as R

F = np.float32


# ---- the fp32 twins (mut: the name of one deliberate fault) ---------------------------------------------------------------------
def gather_twin(vol, origins, patch, zscore, mut=None):
    pz, py, px = patch
    out = []
    for z, y, x in origins:
        p = vol[:, z:z + pz, y:y + py, x:x + px]
        if p.dtype != np.float32:
            p = p.astype(F) / F(np.iinfo(p.dtype).max)
        if zscore:
            groups = [p[c:c + 1] for c in range(p.shape[0])] if mut == "per-channel" else [p]
            done = []
            for g in groups:
                v = g.astype(np.float64)
                mean = v.sum() / v.size
                var = max((v * v).sum() / v.size - mean * mean, 0.0)
                if mut == "sample-std":
                    var = var * v.size / (v.size - 1)
                sd = F(np.sqrt(var))
                if mut != "no-clamp":
                    sd = max(sd, F(1e-10))
                with np.errstate(invalid="ignore", divide="ignore"):
                    done.append(((g - F(mean)) / sd).astype(F))
            p = np.concatenate(done)
        out.append(p)
    return np.stack(out)


def _act32(lg, act, mut):
    with np.errstate(over="ignore", invalid="ignore"):
        if act == 1:
            return (F(1) / (F(1) + np.exp(-lg))).astype(F)
        if act == 2:
            axis = 1 if mut == "softmax-axis" else 0
            # expf as a correctly rounded fp32 function: numpy's own float32 exp is a SIMD approximation of a few ulps on some
            # hosts and no model of any device's; every other operation is float32
            e = np.exp((lg if mut == "softmax-no-max" else lg - lg.max(axis, keepdims=True)).astype(np.float64)).astype(F)
            den = np.zeros_like(e.sum(axis, keepdims=True))
            for k in range(e.shape[axis]):
                den = den + np.take(e, [k], axis)
            return (e / den).astype(F)
    return lg


def accumulate_twin(sum0, wsum0, logits, case, w, mut=None):
    s, ws = sum0.copy(), wsum0.copy()
    Rr, (pz, py, px) = case["R"], case["patch"]
    rows, vector, valid = case["rows"], case["vector"], case["valid"]
    if mut == "beyond-valid":
        valid += 1
    if mut == "vector-dropped":
        vector = 0
    if mut == "perm-to-nonvector":
        vector = 1
    seen = set()
    for b in range(valid):
        z, y, x = case["origins"][b]
        if mut == "repeat-once" and (z, y, x) in seen:
            continue
        seen.add((z, y, x))
        p = _act32(logits[b], case["act"], mut)
        wb = w
        if rows is not None:
            row = rows[b]
            if mut == "sign-dropped":
                row = row[:9] + (0, 0, 0)
            p = R.apply_record(row, p, bool(vector))
            if mut == "weight-view-frame":
                wb = R.apply_record(row, w[None])[0]
        for i in range(pz):
            r = (z % Rr + i) if mut == "ring-row" else (z + i) % Rr
            if r >= Rr:
                continue
            s[:, r, y:y + py, x:x + px] += wb[i] * p[:, i]
            ws[r, y:y + py, x:x + px] += wb[i]
    return s, ws


def finalize_twin(s, ws, case, blend, cast, mut=None):
    Rr, z0, rows, reset = case["R"], case["z0"], case["rows"], case["reset"]
    rr = [(z0 + i) % Rr for i in range(rows)]
    v, wr = s[:, rr], ws[rr]
    pos = np.ones_like(wr, bool) if mut == "divide-at-zero-weight" else wr > 0
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if blend == 0:
            v = np.where(pos, v / np.where(wr != 0, wr, F(0) if mut == "divide-at-zero-weight" else F(1)), v)
        elif blend == 1:
            mag = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
            if mut != "no-eps":
                mag = mag + F(1e-8)
            v = np.where(pos, v / mag, v)
        v = v.astype(F)
        t = (v + F(1)) / F(2) * F(65535) if cast == 1 else v * F(255)
        t = np.minimum(np.maximum(t, F(0)), F(65535 if cast == 1 else 255))
        t = np.rint(t) if mut == "round" else np.trunc(t)
        fin = t.astype(np.uint16 if cast == 1 else np.uint8)
    s_after, w_after = s.copy(), ws.copy()
    if reset >= 1 or mut == "reset0-clears":
        s_after[:, rr] = 0
    if reset == 2 or mut == "reset1-clears-wsum":
        w_after[rr] = 0
    return v, fin, wr.copy(), s_after, w_after


# ---- running one case through its checker -----------------------------------------------------------------------------------------
GATHER = {c["name"]: c for c in R.gather_cases()}
ACC = {c["name"]: c for c in R.accumulate_cases()}
FIN = {c["name"]: c for c in R.finalize_cases()}


def run_gather(case, mut=None):
    vol = R.gather_volume(case)
    scaled = R.gather_scale_ref(vol, case["origins"], case["patch"])
    got = gather_twin(vol, case["origins"], case["patch"], False, mut)
    assert np.array_equal(R.bits(got), R.bits(scaled)), case["name"]
    if case["kind"] == "random" and case["dt"] != "f32":
        assert got[0, 0, 0, 0, 0] == 1.0
    if not case["zscore"]:
        return 0.0
    return R.check_zscore(gather_twin(vol, case["origins"], case["patch"], True, mut), scaled, case["name"])


def run_accumulate(case, mut=None):
    sum0, wsum0, logits, w = R.accumulate_data(case)
    ref = R.accumulate_ref(sum0, wsum0, logits, case["origins"], case["valid"], w, case["act"], case["R"], case["rows"], case["vector"])
    s, ws = accumulate_twin(sum0, wsum0, logits, case, w, mut)
    return R.check_accumulate(s, ws, ref, sum0, wsum0, case["name"], exact=case["act"] == 0)


def run_finalize(case, mode, mut=None):
    blend, cast, c = mode
    s, ws = R.finalize_data(case, blend, cast, c)
    want = R.finalize_ref(s, ws, case["R"], case["z0"], case["rows"], blend, cast, case["reset"])
    R.check_finalize(finalize_twin(s, ws, case, blend, cast, mut), want, f"{case['name']} {mode}")


# ---- the twin passes everywhere ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GATHER))
def test_fp32_twin_passes_gather(name):
    assert run_gather(GATHER[name]) <= 1.0


def test_fp32_twin_passes_accumulate():
    worst = (0.0, 0.0)
    for case in ACC.values():
        r = run_accumulate(case)
        worst = (max(worst[0], r[0]), max(worst[1], r[1]))
    print("fp32 twin, accumulate: largest err / bound (sum, wsum)", worst)
    assert worst[0] <= 1.0 and worst[1] <= 1.0


def test_fp32_twin_passes_finalize():
    for case in FIN.values():
        for mode in R.FIN_MODES:
            run_finalize(case, mode)


def test_special_values_of_the_tables():
    """what the tables demand exactly: saturated sigmoids are 0 and 1, equal logits at 1000 give 1 / c, a channel at -inf gives 0,
    a softmax over one channel is 1"""
    p = R.act_ref(R.SIGMOID_TABLE[None], 1)[0]
    want = {88.0: 1.0, 100.0: 1.0, -100.0: 0.0, np.inf: 1.0, -np.inf: 0.0}
    for x, v in zip(R.SIGMOID_TABLE, p):
        if float(x) in want:
            assert v == want[float(x)], (x, v)
    assert 0 < p[list(R.SIGMOID_TABLE).index(-88)] < 2.0 ** -126 and 0 < p[1] < 1e-12
    q = R.act_ref(R.SOFTMAX_TABLE.T, 2).T
    assert not np.isnan(q).any() and np.allclose(q.sum(1), 1.0, rtol=1e-15)
    assert (q[5] == 1.0 / 3).all() and q[6, 0] == 0 and q[7, 1] == 0 and q[8, 2] == 0
    assert (R.act_ref(np.array([[3.5, -200.0, 1000.0]]), 2) == 1.0).all()


# ---- every mutant is rejected by a named case --------------------------------------------------------------------------------------
MUTANTS = [
    ("gather", "sample-std", "odd-n-u8"),
    ("gather", "sample-std", "grid-cap-104-u8"),
    ("gather", "no-clamp", "constant-u8"),
    ("gather", "per-channel", "c3-p2x4x3-u16"),
    ("accumulate", "softmax-no-max", "softmax-table-X24"),
    ("accumulate", "softmax-axis", "span-c3-softmax-uniform-X24"),
    ("accumulate", "beyond-valid", "span-c1-none-uniform-X22"),
    ("accumulate", "repeat-once", "span-c2-sigmoid-gauss-X24"),
    ("accumulate", "ring-row", "span-c1-none-gauss-X24"),
    ("accumulate", "weight-view-frame", "geom566-v0-none-X24"),
    ("accumulate", "weight-view-frame", "geom567-v1-none-X22"),
    ("accumulate", "vector-dropped", "geom656-v1-none-X24"),
    ("accumulate", "sign-dropped", "geom665-v1-none-X22"),
    ("accumulate", "perm-to-nonvector", "geom566-v0-sigmoid-X24"),
    ("finalize", "divide-at-zero-weight", ("plane9x7-reset2", (0, 0, 1))),
    ("finalize", "round", ("plane5x6-reset2", (2, 1, 2))),
    ("finalize", "round", ("plane9x7-reset2", (0, 0, 3))),
    ("finalize", "no-eps", ("plane12x20-reset1", (1, 1, 3))),
    ("finalize", "reset1-clears-wsum", ("plane9x7-reset1", (0, 0, 1))),
    ("finalize", "reset0-clears", ("plane5x6-reset0", (2, 0, 4))),
]


@pytest.mark.parametrize("op,mut,where", MUTANTS, ids=[f"{m[1]}@{m[2]}" for m in MUTANTS])
def test_mutant_is_rejected(op, mut, where):
    with pytest.raises(AssertionError):
        if op == "gather":
            run_gather(GATHER[where], mut)
        elif op == "accumulate":
            run_accumulate(ACC[where], mut)
        else:
            run_finalize(FIN[where[0]], where[1], mut)
    # the same case passes without the fault: the rejection is the mutant's
    if op == "gather":
        run_gather(GATHER[where])
    elif op == "accumulate":
        run_accumulate(ACC[where])
    else:
        run_finalize(FIN[where[0]], where[1])


def test_the_tables_reach_the_paths_they_are_named_for():
    """the shape arithmetic of csrc/rx_infer.hip restated: which cases reach the scalar and the capped forms"""
    n41, n104 = 41 ** 3, 104 * 101 * 100
    assert n41 % 4 and (n41 + 1023) // 1024 > 64 and (n41 + 63) // 64 * 64 != n41              # scalar, chunks capped, ragged per
    assert n104 % 4 == 0 and n104 > 2 ** 20 and (n104 // 4 + 255) // 256 > 1024                 # vector, grid capped
    assert (3 * 3 * 5) % 4 and any(c["patch"] == (3, 3, 5) and c["cin"] == 1 for c in GATHER.values())
    assert {c["patch"][2] for c in GATHER.values()} >= {1, 3, 4, 5, 10}
    for c in FIN.values():
        assert (c["Y"] * c["X"]) % 4 in ((3, 2, 0)[(63, 30, 240).index(c["Y"] * c["X"])],)
    for c in ACC.values():
        k = [c["origins"][b] for b in range(c["valid"])]
        if c["name"].startswith("span"):
            assert {z for z, _, _ in k} == {10, 12, 15} and min(x for _, _, x in k) in (5, 6)
            assert max(x for _, _, x in k) + c["patch"][2] & 3 and max(z for z, _, _ in k) + c["patch"][0] > c["R"]
