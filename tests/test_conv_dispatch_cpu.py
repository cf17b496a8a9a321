"""tests/conv_dispatch_cases.py held against the code, without a GPU.

  * the halo selector rx_ch_choose is swept (through the host program of test_conv_halo_plan_cpu.py) over the queries the entry points
    can make on small layers; every (kernel, FLIP, STATS, ACC, BS) it launches needs a ledger row, and every halo row's own query
    must return what the row claims;
  * every kernel name the conv sources can hand to rx_note_kernel needs a row, in every dtype in which it is reachable;
  * no row is spare: each one is the only cover of something, and a test deletes every row in turn and requires a failure that
    names its kernel;
  * the split counts rows claim are recomputed by a pure-Python restatement of igemm_launch, plan_split and wgh_plan (source lines
    cited).  That restatement DOCUMENTS the rows; it does not follow later changes to the C++ -- the kernel names asserted on the
    GPU, and the exact values, are what follows those."""
import collections
import itertools
import math
import os
import re

import pytest

import conv_dispatch_cases as L
import conv_halo_cases as C
from test_conv_halo_plan_cpu import choose  # noqa: F401  (the fixture: csrc/tools/conv_halo_plan_check.cpp under ASan / UBSan)

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "multi-task-3d-resencoder-unet_amd", "csrc")
WS = C.WS_BYTES
HALO = ("conv_halo32p_kernel", "conv_halo32ws_kernel", "conv_halo32_kernel", "conv_halo64ws_kernel", "conv_halo_kernel<32>",
        "conv_halo_kernel<64>")


def cls(dtype_name):
    return "float32" if dtype_name == "float32" else "half"


def tag(row):
    """the sub-branch of a row as a string: split counts only as '= 1' / '> 1' (the value itself is checked below)"""
    s = row.sub
    if s is None or isinstance(s, str):
        return s or ""
    parts = []
    for c, v in sorted(s.get("ks", {}).items()):
        parts.append(f"ks[{c}]{'=1' if v == 1 else '>1'}")
    if "S" in s:
        parts.append("S=1" if s["S"] == 1 else "S>1")
    parts += [f"{k}={s[k]}" for k in ("reduce", "stride") if k in s]
    return " ".join(parts)


# ---- the queries behind the entry points (rx_igemm.hip: rx_conv3d_fwd passes flip 0 / accumulate 0 and no buffer, rx_conv3d_fwd_stats
# offers the workspace, rx_conv3d_bwd_data passes flip 1 and no buffer, rx_conv3d_bwd_data_instats offers the workspace and the sums)
def entry_queries(dt, n, dims, ci, co):
    st = dict(stat_offered=1, stat_bytes=WS)
    return {L.FWD: C.query(dt, n, dims, ci, co), L.STATS: C.query(dt, n, dims, ci, co, **st),
            L.DX: C.query(dt, n, dims, co, ci, flip=1), L.DXA: C.query(dt, n, dims, co, ci, flip=1, accumulate=1),
            L.BS: C.query(dt, n, dims, co, ci, flip=1, want_bs=1, bs_ldy=ci, **st),
            L.BSA: C.query(dt, n, dims, co, ci, flip=1, accumulate=1, want_bs=1, bs_ldy=ci, **st)}


def flags(ch):
    return tuple(ch[k] for k in ("FLIP", "STATS", "ACC", "BS"))


def halo_key(entry, ch):
    """what a launched choice demands a row for: the statistics entry points only where they change the instantiation"""
    f = flags(ch)
    if entry == L.STATS and not f[1]:
        entry = L.FWD
    if entry in (L.BS, L.BSA) and not f[3]:
        entry = L.DX if entry == L.BS else L.DXA
    return entry, ch["name"], f


def row_query(row, dt):
    """the selector query of a halo row, from the shape it names"""
    if isinstance(row.shape, str):
        s = L.SHAPES[row.shape]
        n, ci, co, dims = s.n, s.ci, s.co, s.dims
    elif len(row.shape) == 5:                         # a CONV_CASES tuple: n = 2
        n, (ci, co, dims) = 2, row.shape[:3]
    elif len(row.shape) == 3:                         # test_conv3d_fwd_stats: (ci, co, dims), n = 3 for the 30-deep case
        ci, co, dims = row.shape
        n = 3 if dims[0] == 30 else 2
    else:                                             # test_conv3d_bwd_data_instats: (c, dims), n = 3
        n, ci, co, dims = 3, row.shape[0], row.shape[0], row.shape[1]
    return entry_queries(dt, n, dims, ci, co)[row.entry]


@pytest.fixture(scope="module")
def sweep(choose):  # noqa: F811
    """{(dtype, entry, kernel, flags)} over N in {1, 2}, Ci / Co in {32 .. 256}, extents up to 64: operands far below 2 GiB"""
    qs, meta = [], []
    for dt, n, z, y, x, ci, co in itertools.product(L.ALL, (1, 2), (4, 8, 14, 16, 30, 32, 48), (4, 8, 16, 32, 36), (4, 8, 16, 32, 48, 64),
                                                   (32, 64, 96, 128, 256), (32, 64, 96, 128, 256)):
        if n * z * y * x * max(ci, co) * 4 >= 1 << 31:
            continue
        for e, q in entry_queries(dt, n, (z, y, x), ci, co).items():
            qs.append(q)
            meta.append((dt, e))
    seen = set()
    for i in range(0, len(qs), 40000):
        for (dt, e), ch in zip(meta[i:i + 40000], choose(qs[i:i + 40000])):
            if ch["kind"] == "launch":
                assert ch["XDMA"] == (ch["name"] in ("conv_halo32ws_kernel", "conv_halo64ws_kernel")), ch      # nothing here is past 2 GiB
                seen.add((dt,) + halo_key(e, ch))
    return seen


def test_every_halo_row_reaches_what_it_claims(choose):  # noqa: F811
    rows = [(r, dt) for r in L.ROWS if r.kernel in HALO for dt in r.dtypes]
    got = choose([row_query(r, dt) for r, dt in rows])
    for (r, dt), ch in zip(rows, got):
        assert ch["kind"] == "launch" and ch["name"] == r.kernel and flags(ch) == r.flags, (r.entry, r.shape, dt, ch)
        if r.entry in (L.BS, L.BSA):
            assert bool(ch["take_bs"]) == (r.sub != "not fused"), (r.shape, dt, ch)
        if r.entry == L.STATS:
            assert ch["stat_chunks"] > 0, (r.shape, dt, ch)
        if r.kernel == "conv_halo64ws_kernel":
            assert r.sub == f"grid_y={ch['grid_y']}", (r.shape, dt, ch)
        if r.sub == "tile 4x4x16":
            assert ch["tile"] == "4x4x16", (r.shape, dt, ch)
        if r.kernel.startswith("conv_halo_kernel") and r.sub != "tile 4x4x16":
            assert ch["tile"] == "4x8x8", (r.shape, dt, ch)


# ---- kernel names, read from the sources -------------------------------------------------------------------------------------------
# the 16-bit-only kernels: (source, the guard that keeps fp32 off them, quoted).  Every other name is reachable in all three dtypes.
F32_GUARD = {
    "igemm_fat_kernel": ("rx_igemm.hip", "if (dt != RX_F32 && g.nph == 1 && g.Ci % KE == 0"),
    "dgrad_s2p_kernel": ("rx_dgrad_s2.hip", "if (dt == RX_F32 || dy->c != 64"),
    "pointwise_kernel": ("rx_pointwise.hip", "if (dt == RX_F32 || in->cs || out->cs) return 0;"),
    "wgrad_halo_kernel": ("rx_wgrad_halo.hip", "if (dt == RX_F32) return 0;"),
    "wgrad_halo16ws_kernel": ("rx_wgrad_halo.hip", "if (dt == RX_F32) return 0;"),
    "convT_wgrad_kernel": ("rx_wgrad.hip", "if (dt == RX_F32 || taps > 8"),
    "conv_halo32p_kernel": ("rx_conv_halo_plan.h", "if (BN == 32 && tile4416 && dt != RX_F32 && Ci == 32 && Co == 32 && c.NT >= 512) {"),
    "conv_halo32ws_kernel": ("rx_conv_halo_plan.h", "if (BN == 32 && tile4416 && dt != RX_F32 && !q.out_cs && Ci >= 64"),
    "conv_halo64ws_kernel": ("rx_conv_halo_plan.h", "if (Co % 64 == 0 && tile4416 && dt != RX_F32 && (long)c.NT * (Co / 64) >= 256) {"),
}


def reach(name):
    return L.HALF if name in F32_GUARD else L.ALL


def source(f):
    with open(os.path.join(CSRC, f)) as fh:
        return fh.read()


def source_names():
    names = set()
    for f in ("rx_igemm.hip", "rx_wgrad.hip", "rx_wgrad_halo.hip", "rx_dgrad_s2.hip", "rx_pointwise.hip"):
        for call in re.finditer(r"rx_note_kernel\(([^;]*)\);", source(f)):
            names.update(re.findall(r'"([^"]+)"', call.group(1)))
    names.update(re.findall(r'rx_ch_launch\(c, \w+, "([^"]+)"', source("rx_conv_halo_plan.h")))
    return names


def test_the_fp32_guards_are_where_they_are_quoted_from():
    """the dtype column of the ledger rests on these lines; a guard that moves or changes fails here, not silently"""
    for name, (f, guard) in F32_GUARD.items():
        assert guard in source(f), f"{name}: `{guard}` is no longer in {f}: is the kernel still 16-bit only?"
    # and no other conv dispatch is closed to fp32: every `RX_F32` test in the host code of these sources is one of the above, the
    # element sizes (per16 / KB / KE), the selector's planar-concat refusal or its statistics flag
    known = [g for _, g in F32_GUARD.values()] + ["dt == RX_F32 ? 4 : 8", "dt == RX_F32 ? ", "if (planar && dt == RX_F32) return c;",
                                                  "dt != RX_F32 && Ci / KB >= 4", "if (dt != RX_F32 && dt != RX_BF16 && dt != RX_F16) return c;"]
    for f in ("rx_igemm.hip", "rx_wgrad.hip", "rx_wgrad_halo.hip", "rx_dgrad_s2.hip", "rx_pointwise.hip", "rx_conv_halo_plan.h"):
        for line in source(f).splitlines():
            if "RX_F32" in line and "RX_DISPATCH" not in line and not line.lstrip().startswith("//"):
                assert any(k in line for k in known), f"{f}: an fp32 condition the ledger's dtype column does not know: {line.strip()}"


# ---- what the rows that point elsewhere point at -----------------------------------------------------------------------------------
# the pins test_conv3d_fwd_bwd carried before it read them from the ledger: (fwd, bwd-data, bwd-weight); they may grow, not shrink
PINS = {
    L.P_F1: ("igemm_fat_kernel", "igemm_fat_kernel", "wgrad_halo_kernel"),
    L.P_F512: ("igemm_fat_kernel", "igemm_fat_kernel", "wgrad_halo_kernel"),
    L.P_F388: ("igemm_fat_kernel", "igemm_fat_kernel", "wgrad_halo_kernel"),
    L.P_A: ("conv_halo32p_kernel", "conv_halo32p_kernel", "wgrad_halo16ws_kernel"),
    L.P_B1: ("conv_halo64ws_kernel", "conv_halo64ws_kernel", "wgrad_halo16ws_kernel"),
    L.P_C: ("conv_halo32ws_kernel", "conv_halo32ws_kernel", None),
    L.P_S2: (None, "dgrad_s2p_kernel", None),
    L.P_S2R: (None, "dgrad_s2p_kernel", None),
    L.P_PW: ("pointwise_kernel", "pointwise_kernel", None),
}


def pinned(r):
    """a row PINS above answers for"""
    return r.covered_by == L.PIN and r.entry in (L.FWD, L.DX, L.DW)


def test_rows_that_point_at_existing_tests_point_at_real_cases():
    import inspect

    import test_ops_gpu as G
    assert G.EXPECT_KERNELS == L.expect_kernels()
    assert set(PINS) <= set(G.CONV_CASES)
    src = {name: inspect.getsource(getattr(G, name)) for name in ("test_conv3d_fwd_bwd", "test_conv3d_fwd_stats", "test_conv3d_bwd_data_instats",
                                                                  "test_convT3d_fwd_bwd")}
    for r in L.ROWS:
        if r.covered_by is None:
            assert r.shape in L.SHAPES, r
            continue
        name = r.covered_by.split("::")[1]
        if name == "test_conv3d_fwd_bwd":
            assert r.shape in G.CONV_CASES and r.entry in (L.FWD, L.DX, L.DXA, L.DW), r
            assert "EXPECT_KERNELS[case]" in src[name] and 'covered_kernel("test_conv3d_fwd_bwd", case, conv_dispatch_cases.DXA)' in src[name]
        elif name == "test_convT3d_fwd_bwd":
            assert r.shape in G.CONVT_CASES and f'== "{r.kernel}"' in src[name], r
        else:                                              # the case is a literal of the test's parametrize list, the name is read from here
            assert re.sub(r"\s", "", repr(r.shape)) in re.sub(r"\s", "", src[name]), r
            assert f'covered_kernel("{name}"' in src[name], r
            assert L.covered_kernel(name, r.shape, r.entry) == r.kernel


# ---- no spare rows, none missing ----------------------------------------------------------------------------------------------------
# What the issue asks for, as (entry, kernel, tag): every row that PINS does not answer for.  A row is the only one of its identity.
NEEDED = {
    # the persistent halo kernels' remaining instantiations: checked by the tests the rows point at
    (L.DXA, "conv_halo32p_kernel", ""), (L.STATS, "conv_halo32p_kernel", ""), (L.BS, "conv_halo32p_kernel", ""), (L.BSA, "conv_halo32p_kernel", ""),
    (L.DXA, "conv_halo64ws_kernel", "grid_y=1"), (L.STATS, "conv_halo64ws_kernel", "grid_y=1"),
    (L.BS, "conv_halo64ws_kernel", "grid_y=1"), (L.BSA, "conv_halo64ws_kernel", "grid_y=1"),
    (L.DXA, "conv_halo32ws_kernel", ""), (L.STATS, "conv_halo32ws_kernel", ""),
    # B2, D1, D2, E1, E2 and their data gradients
    (L.FWD, "conv_halo64ws_kernel", "grid_y=2"), (L.STATS, "conv_halo64ws_kernel", "grid_y=2"),
    (L.DX, "conv_halo64ws_kernel", "grid_y=2"), (L.DXA, "conv_halo64ws_kernel", "grid_y=2"),
    (L.BS, "conv_halo64ws_kernel", "grid_y=2"), (L.BSA, "conv_halo64ws_kernel", "grid_y=2"),
    (L.FWD, "conv_halo32_kernel", ""), (L.DX, "conv_halo32_kernel", ""), (L.STATS, "conv_halo32_kernel", ""),
    (L.DXA, "conv_halo32_kernel", "g.accumulate=1"), (L.BS, "conv_halo32_kernel", "not fused"),
    (L.FWD, "conv_halo_kernel<32>", ""), (L.FWD, "conv_halo_kernel<64>", ""),
    (L.DX, "conv_halo_kernel<32>", "g.flip=1"), (L.DXA, "conv_halo_kernel<32>", "g.flip=1 g.accumulate=1"),
    (L.DX, "conv_halo_kernel<64>", "g.flip=1"), (L.DXA, "conv_halo_kernel<64>", "g.flip=1 g.accumulate=1"),
    (L.FWD, "conv_halo_kernel<64>", "tile 4x4x16"),
    # every igemm_kernel<BM,BN> forward and backward, ks == 1 and ks > 1, stride 2 and (1,2,2)
    (L.FWD, "igemm_kernel<128,32>", "ks[float32]>1 ks[half]>1"),
    (L.DX, "igemm_kernel<128,64>", "ks[float32]>1 ks[half]=1"), (L.DXA, "igemm_kernel<128,64>", "ks[float32]>1 ks[half]=1"),
    (L.FWD, "igemm_kernel<128,64>", "ks[float32]>1 ks[half]>1 stride=2"),
    (L.DX, "igemm_kernel<128,64>", "ks[float32]>1 ks[half]>1 stride=2"), (L.DXA, "igemm_kernel<128,64>", "ks[float32]>1 ks[half]>1 stride=2"),
    (L.FWD, "igemm_kernel<128,64>", "ks[float32]>1 ks[half]>1 stride=(1, 2, 2)"),
    (L.DX, "igemm_kernel<128,32>", "ks[float32]>1 ks[half]>1 stride=(1, 2, 2)"),
    (L.DXA, "igemm_kernel<128,32>", "ks[float32]>1 ks[half]>1 stride=(1, 2, 2)"),
    (L.FWD, "igemm_kernel<256,64>", "ks[float32]>1 ks[half]=1"),
    (L.DX, "igemm_kernel<256,32>", "ks[float32]>1 ks[half]>1"), (L.DXA, "igemm_kernel<256,32>", "ks[float32]>1 ks[half]>1"),
    (L.FWD, "igemm_kernel<256,32>", "ks[float32]>1 ks[half]=1"),
    (L.FWD, "igemm_kernel<256,64>", "ks[float32]>1 ks[half]>1"),
    (L.DX, "igemm_kernel<256,64>", "ks[float32]>1 ks[half]>1"), (L.DXA, "igemm_kernel<256,64>", "ks[float32]>1 ks[half]>1"),
    (L.FWD, "igemm_kernel<256,64>", "ks[float32]=1"),
    (L.FWD, "igemm_fat_kernel", "ks[half]=1"), (L.DX, "igemm_fat_kernel", "ks[half]>1"), (L.DXA, "igemm_fat_kernel", "ks[half]>1"),
    # every wgrad_kernel<BR,BC>, both reduce forms
    (L.DW, "wgrad_kernel<32,64>", "S=1"), (L.DW, "wgrad_kernel<64,32>", "S=1"), (L.DW, "wgrad_kernel<32,32>", "S=1"),
    (L.DW, "wgrad_kernel<64,64>", "S=1"), (L.TDW, "wgrad_kernel<64,64>", "S=1"),
    (L.DW, "wgrad_kernel<32,32>", "S>1 reduce=wgrad_reduce"), (L.DW, "wgrad_kernel<32,32>", "S>1 reduce=wgrad_reduce_manysplits"),
    # the halo weight-gradient kernels: S == 1 and S > 1, both reduce forms, the strided tiles
    (L.DW, "wgrad_halo_kernel", "S=1"), (L.DW, "wgrad_halo_kernel", "S>1 reduce=wgrad_reduce stride=2"),
    (L.DW, "wgrad_halo_kernel", "S>1 reduce=wgrad_reduce stride=(1, 2, 2)"), (L.DW, "wgrad_halo_kernel", "S>1 reduce=wgrad_reduce_manysplits"),
    (L.DW, "wgrad_halo16ws_kernel", "S=1"), (L.DW, "wgrad_halo16ws_kernel", "S>1 reduce=wgrad_reduce"),
    (L.DW, "wgrad_halo16ws_kernel", "S>1 reduce=wgrad_reduce_manysplits"),
    # the transposed conv
    (L.TFWD, "pointwise_kernel", ""), (L.TDW, "convT_wgrad_kernel", ""),
    (L.TFWD, "igemm_kernel<128,64>", "ks[float32]=1 ks[half]=1"),
    (L.TDX, "igemm_kernel<128,64>", "ks[float32]>1 ks[half]>1"), (L.TDXA, "igemm_kernel<128,64>", "ks[float32]>1 ks[half]>1"),
}


def ledger_problems(rows, swept):
    """everything the ledger `rows` leaves uncovered or claims twice, as text"""
    out = []
    have = {(dt, r.entry, r.kernel, r.flags) for r in rows if r.kernel in HALO for dt in r.dtypes}
    out += [f"launched by rx_ch_choose, no ledger row: {k}" for k in sorted(swept - have)]
    not_fused = {(dt, r.entry, r.kernel, r.flags) for r in rows if r.sub == "not fused" for dt in r.dtypes}      # the data gradient's launch
    out += [f"a ledger row the sweep never reaches: {k}" for k in sorted(have - swept - not_fused)]
    names = source_names()
    named = {(r.kernel, dt) for r in rows for dt in r.dtypes}
    out += [f"kernel name without a checked case: {nm} in {dt}" for nm in sorted(names) for dt in reach(nm) if (nm, dt) not in named]
    out += [f"a row names a kernel the sources do not: {r.kernel}" for r in rows if r.kernel not in names]
    out += [f"a row claims {r.kernel} in a dtype its guard excludes: {r.dtypes}" for r in rows if not set(r.dtypes) <= set(reach(r.kernel))]
    got = L.expect_kernels(rows)
    out += [f"pin of test_conv3d_fwd_bwd changed: {c}: {got.get(c)} for {PINS.get(c)}" for c in sorted(set(got) | set(PINS), key=repr)
            if got.get(c) != PINS.get(c)]
    ident = collections.Counter((r.entry, r.kernel, tag(r)) for r in rows if not pinned(r))
    out += [f"no row for {k}" for k in sorted(NEEDED - set(ident))]
    out += [f"a row nobody asked for: {k}" for k in sorted(set(ident) - NEEDED)]
    out += [f"two rows for one branch: {k}" for k, v in sorted(ident.items()) if v > 1]
    for key, s in L.SHAPES.items():
        mine = [r for r in rows if r.shape == key]
        out += [f"{r.entry} on {key}: dtypes the shape does not run" for r in mine if not set(r.dtypes) <= set(s.dtypes)]
        out += [f"shape {key} runs in {dt} for no row" for dt in s.dtypes if not any(dt in r.dtypes for r in mine)]
    return out


def test_the_ledger_is_complete_and_has_no_spare_row(sweep):
    assert {k[2] for k in sweep} == set(HALO)
    assert len(source_names()) == 20      # 4 igemm, fat, 4 wgrad, convT_wgrad, 2 wgrad_halo, s2p, pointwise, 6 halo
    problems = ledger_problems(L.ROWS, sweep)
    assert not problems, "\n".join(problems)


def test_deleting_any_one_row_is_noticed_and_names_it(sweep):
    """every row, one at a time: without it the checks above report a problem that names the row's kernel"""
    for i, r in enumerate(L.ROWS):
        problems = ledger_problems(L.ROWS[:i] + L.ROWS[i + 1:], sweep)
        assert any(r.kernel in p for p in problems), f"row {i} ({r.entry}, {r.kernel}, {r.shape}) can be deleted unnoticed: {problems}"


def test_unreachable_instantiations_are_past_the_buffer_range(choose):  # noqa: F811
    """each entry of UNREACHABLE, held against the code: the instantiation appears exactly where an operand passes 0x7fffff00 bytes
    (64 channels at 128^3 are 2^28 bytes a sample: 7 samples fit, 8 do not), and nothing the ledger runs comes near"""
    big = (128, 128, 128)
    ch = choose([C.query("bfloat16", n, big, 64, 64) for n in (7, 8)] + [C.query("float16", n, big, 64, 96) for n in (7, 8)])
    checks = {
        "conv_halo64ws_kernel<XDMA=false>": [c["name"] == "conv_halo64ws_kernel" for c in ch[:2]] + [ch[0]["XDMA"] == 1, ch[1]["XDMA"] == 0],
        "conv_halo32_kernel in place of conv_halo32ws_kernel": [ch[2]["name"] == "conv_halo32ws_kernel", ch[3]["name"] == "conv_halo32_kernel"],
        "wgrad_halo16ws_kernel<DMA=false>": ["const bool dma_ok = (long)g.N * g.g_ss * 2 < 0x7fffff00L &&" in source("rx_wgrad_halo.hip"),
                                             "if (dma_ok && dt == RX_BF16)" in source("rx_wgrad_halo.hip")],
    }
    assert set(checks) == set(L.UNREACHABLE)
    for what, oks in checks.items():
        assert all(oks), (what, oks)
        assert re.search(r"GiB|0x7fffff00", L.UNREACHABLE[what]), what
    for key, s in L.SHAPES.items():                    # (the sweep asserts XDMA for every query it makes)
        assert s.n * math.prod(s.dims) * (max(s.ci, s.co) + 32) * 4 < 0x7fffff00 // 8, key


# ---- split counts: a restatement of the host code, to document the rows --------------------------------------------------------------
def cdiv(a, b):
    return -(-a // b)


def p2ceil(v):
    p = 1
    while p < v:
        p <<= 1
    return p


def out_dim(i, k, s):
    return (i + 2 * ((k - 1) // 2) - k) // s + 1


def igemm_ks(dt, n, ci, co, phases, out_stride1=True):
    """rx_igemm.hip igemm_launch (lines 423-526): (kernel, ks).  phases = [(voxels, taps)]; ci / co as the launch sees them"""
    f32 = dt == "float32"
    KB = 16 if f32 else 32
    vmax = max(v for v, _ in phases)
    nkt_max = max(t for _, t in phases) * (ci // KB)
    NV = n * phases[0][0]
    if not f32 and len(phases) == 1 and ci % 128 == 0 and co % 64 == 0 and NV <= 2048 and phases[0][1] * (ci // 128) >= 8 and out_stride1:
        nsteps = phases[0][1] * (ci // 128)                                  # lines 442-450
        base = cdiv(NV, 128) * (co // 64)
        ks = max(1, min(cdiv(512, base), nsteps // 4))
        assert ks * NV * co * 4 <= WS
        return "igemm_fat_kernel", ks
    BN = 64 if co % 64 == 0 else 32                                          # lines 492-515
    BM = 128 if vmax <= 128 else 256
    wgs = sum(cdiv(v, BM) for v, _ in phases) * (co // BN) * n
    ks = 1
    if wgs < 192 and nkt_max >= 16:
        ks = max(1, min(cdiv(512, wgs), nkt_max // 4, 32))
        assert ks * n * sum(v for v, _ in phases) * co * 4 <= WS
    return f"igemm_kernel<{BM},{BN}>", ks


def dgrad_phases(dims, k, s):
    """rx_igemm.hip rx_conv3d_bwd_data (lines 695-735): one phase per parity class"""
    ph = []
    for r in itertools.product(*[range(ss) for ss in s]):
        q = [cdiv(dims[a] - r[a], s[a]) for a in range(3)]
        cnt = math.prod(sum(1 for t in range(k[a]) if (r[a] + (k[a] - 1) // 2 - t) % s[a] == 0) for a in range(3))
        if math.prod(q) > 0:
            ph.append((math.prod(q), cnt))
    assert len(ph) <= 8
    return ph


def wgrad_splits(R, Cc, taps, NQ):
    """rx_wgrad.hip plan_split (lines 229-243) and wgrad_launch (286)"""
    BR, BC = (64 if R % 64 == 0 else 32), (64 if Cc % 64 == 0 else 32)
    ktiles = cdiv(NQ, 64)
    S = max(1, min(cdiv(1024, (R // BR) * (Cc // BC) * taps), ktiles // 4))
    return f"wgrad_kernel<{BR},{BC}>", cdiv(ktiles, cdiv(ktiles, S))


def wgh_splits(n, ci, co, odims, s):
    """rx_wgrad_halo.hip wgh_plan (lines 502-546) and rx_wgrad_halo_try (567): (kernel, S), None when the plan refuses"""
    strided = max(s) > 1
    TX = min(16, max(4, p2ceil(odims[2])))
    if strided:
        TX = min(TX, 8)
    rem = (64 if strided else 256) // TX
    TY = min(p2ceil(odims[1]), 4 if (TX == 16 or strided) else 8, rem)
    TZ = min(p2ceil(odims[0]), rem // TY)
    HV = (s[0] * (TZ - 1) + 3) * (s[1] * (TY - 1) + 3) * (s[2] * (TX - 1) + 3)
    if not 16 <= TZ * TY * TX <= 256 or HV > 768:
        return None
    NT = n * cdiv(odims[0], TZ) * cdiv(odims[1], TY) * cdiv(odims[2], TX)
    PP = (co // 32) * (ci // 32)
    t16 = not strided and (TZ, TY, TX) == (4, 4, 16)
    target = 256 if (t16 and NT * PP >= 16 * 256) else 512
    S = 1 if PP >= 256 else cdiv(target, PP)
    S = max(1, min(S, NT))
    assert S * 27 * co * ci * 4 <= WS
    return ("wgrad_halo16ws_kernel" if t16 else "wgrad_halo_kernel"), cdiv(NT, cdiv(NT, S))


def reduce_form(S, taps):
    """rx_wgrad.hip rx_wgrad_reduce_launch (lines 301-307); the halo kernels skip it when S == 1"""
    return "wgrad_reduce_manysplits" if (S >= 8 or taps > 27) else "wgrad_reduce"


def shape_of(row):
    if isinstance(row.shape, str):
        s = L.SHAPES[row.shape]
        return s.kind, s.n, s.ci, s.co, s.dims, s.k, s.s
    ci, co, dims, k, s = row.shape
    return "conv", 2, ci, co, dims, k, s


def test_the_split_counts_rows_claim():
    checked = 0
    for r in L.ROWS:
        if not isinstance(r.sub, dict) or not (set(r.sub) & {"ks", "S"}):
            continue
        kind, n, ci, co, dims, k, s = shape_of(r)
        for dt in r.dtypes:
            if kind == "convT":
                v, taps = math.prod(dims), math.prod(s)
                got = {L.TFWD: lambda: igemm_ks(dt, n, ci, co, [(v, 1)] * taps, False), L.TDX: lambda: igemm_ks(dt, n, co, ci, [(v, taps)]),
                       L.TDXA: lambda: igemm_ks(dt, n, co, ci, [(v, taps)]), L.TDW: lambda: wgrad_splits(ci, co, taps, n * v)}[r.entry]()
            else:
                od = tuple(out_dim(d, kk, ss) for d, kk, ss in zip(dims, k, s))
                taps = math.prod(k)
                if r.entry == L.FWD:
                    got = igemm_ks(dt, n, ci, co, [(math.prod(od), taps)])
                elif r.entry in (L.DX, L.DXA):
                    got = igemm_ks(dt, n, co, ci, dgrad_phases(dims, k, s), s == (1, 1, 1))
                else:
                    halo = wgh_splits(n, ci, co, od, s) if (k == (3, 3, 3) and dt != "float32") else None
                    got = halo or wgrad_splits(co, ci, taps, n * math.prod(od))
            assert got[0] == r.kernel, (r.entry, r.shape, dt, got)
            want = r.sub["ks"][cls(dt)] if "ks" in r.sub else r.sub["S"]
            assert got[1] == want, (r.entry, r.shape, dt, got, want)
            if "S" in r.sub:
                assert r.sub.get("reduce") == (None if (got[1] == 1) else reduce_form(got[1], taps)), (r.entry, r.shape, dt, got)
            if "stride" in r.sub:
                assert s == (r.sub["stride"] if isinstance(r.sub["stride"], tuple) else (r.sub["stride"],) * 3), r
            checked += 1
    assert checked >= 100
