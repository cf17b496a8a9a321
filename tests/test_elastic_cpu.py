"""CPU: dataloading/elastic_device.py -- the B-spline tables, `displacement_numpy` and `elastic_numpy` (the statement of
rx_elastic_apply and the host path) against an independent float64 tensor-product B-spline written here (truncated powers, dense
basis matrices), the vector rule against `spatial_device.rotation_op`, the fold bound, the draw order, the config parser, the host
path of both datasets, and the kernel's own per-voxel functions run on the CPU under AddressSanitizer.  Every check is a function
over the module's attributes, so the last test can plant faults in them and count the checks each one trips."""
import os
import random
import struct
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mt3d_amd  # noqa: F401
from mt3d_amd.dataloading import elastic_device as M
from mt3d_amd.dataloading import spatial_device as S
from mt3d_amd.dataloading import zarr_lite

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24          # unit roundoff of float32
TASKS = {"sheet": {"channels": 1}, "normals": {"channels": 3, "loss_fn": "MaskedCosineLoss"}}
BLOCK = {"spacing": 8, "magnitude": [0, 1.25], "p": 0.3, "normal_keys": ["normals"], "image_border": "constant", "where": "device"}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and bool((a.view(np.int32) == b.view(np.int32)).all())


def positive_field(shape, seed):
    """no -0.0 and no exact 0.0: a lerp with weight 0 computes a + 0 * (b - a), which turns a = -0.0 into +0.0"""
    return (np.random.default_rng(seed).random(shape, dtype=np.float32) + np.float32(0.25)).astype(np.float32)


def random_field(shape, spacing, amplitude, seed):
    spacing = (spacing,) * 3 if isinstance(spacing, int) else tuple(spacing)
    g = M.grid_shape(shape, spacing)
    return M.ElasticField(np.random.default_rng(seed).uniform(-amplitude, amplitude, (3,) + g), spacing)


# ---- the independent formulation: float64, truncated powers, one dense basis matrix per axis --------------------------------------
def b3(t, order=0):
    """the uniform cubic B-spline on [0, 4] (order 0) or its derivative (order 1): sum_j (-1)^j C(4, j) (t - j)_+^3 / 6"""
    t = np.asarray(t, dtype=np.float64)
    out = np.zeros_like(t)
    for j, cj in enumerate((1.0, -4.0, 6.0, -4.0, 1.0)):
        r = np.maximum(t - j, 0.0)
        out += cj * (r ** 3 / 6.0 if order == 0 else r ** 2 / 2.0)
    return out


def basis(pos, s, G, order=0):
    """[len(pos), G]: the weight of node g at the (continuous) voxel coordinate pos.  Node g + a of a voxel with u = pos / s =
    i + f has the weight b3(f + 3 - a) = b3(u - g + 3); the derivative with respect to pos carries 1 / s."""
    m = b3(np.asarray(pos, dtype=np.float64)[:, None] / s - np.arange(G)[None, :] + 3.0, order)
    return m / s if order else m


def field64(nodes, spacing, pos, orders=(0, 0, 0)):
    """D (or a partial derivative of it) at the grid pos[0] x pos[1] x pos[2], float64: (3, len z, len y, len x)"""
    bz, by, bx = (basis(pos[d], spacing[d], nodes.shape[1 + d], orders[d]) for d in range(3))
    return np.einsum("cijk,zi,yj,xk->czyx", nodes.astype(np.float64), bz, by, bx, optimize=True)


def jacobian64(nodes, spacing, shape):
    pos = [np.arange(n, dtype=np.float64) for n in shape]
    return np.stack([field64(nodes, spacing, pos, tuple(int(e == d) for d in range(3))) for e in range(3)], axis=1)      # [d][e]


# ---- the checks -------------------------------------------------------------------------------------------------------------------
def check_tables():
    for n, s in [(9, 8), (17, 8), (33, 16), (70, 32), (128, 32), (56, 11)]:
        G = (n - 1) // s + 4
        idx, w, dw = M.bspline_tables(n, s)
        assert idx.dtype == np.int32 and w.dtype == np.float32 and dw.dtype == np.float32
        assert idx.shape == (n,) and w.shape == (n, 4) and dw.shape == (n, 4)
        assert idx.min() == 0 and idx.max() == G - 4 and (idx == np.arange(n) // s).all()
        # four roundings of the table and three of the sum, each at most U of a term <= 1 (dw: <= 1 / s)
        assert np.abs(((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3] - np.float32(1.0)).max() <= 7 * U
        assert np.abs(((dw[:, 0] + dw[:, 1]) + dw[:, 2]) + dw[:, 3]).max() <= 7 * U / s
        o = np.arange(n)
        for a in range(4):
            # the independent evaluation (truncated powers: terms up to 4^3 / 6, so 1e-13 of float64 slack), rounded once
            for got, want in ((w[:, a], b3(o / s - (idx + a) + 3.0)), (dw[:, a], b3(o / s - (idx + a) + 3.0, 1) / s)):
                assert (np.abs(got.astype(np.float64) - want) <= U * np.abs(want) + 1e-13).all(), (n, s, a)


def check_displacement():
    """|D32 - D64| <= 16 U max|nodes|: three nested 4-term sums, each term one product and at most three additions, on weights that
    carry one rounding (5 U per level on a convex combination, 15 U and the second order).  E: the same count on weights with
    sum_a |dw_a| <= 1.5 / s_e."""
    for shape, spacing, seed in [((9, 10, 11), (8, 8, 8), 0), ((17, 33, 70), (8, 16, 32), 1), ((24, 40, 56), (11, 9, 13), 2)]:
        f = random_field(shape, spacing, 3.0, seed)
        D, E = M.displacement_numpy(f, shape)
        assert D.dtype == np.float32 and D.shape == (3, *shape) and E.dtype == np.float32 and E.shape == (3, 3, *shape)
        top = float(np.abs(f.nodes).max())
        pos = [np.arange(n, dtype=np.float64) for n in shape]
        assert np.abs(D - field64(f.nodes, spacing, pos)).max() <= 16 * U * top
        J = jacobian64(f.nodes, spacing, shape)
        for e in range(3):
            assert np.abs(E[:, e] - J[:, e]).max() <= 16 * U * top * 1.5 / spacing[e], e
        # central differences of the float64 field, h = 1e-3: truncation h^2 / 6 * |D'''| <= 1e-6 / 6 * 8 top / s^3, cancellation 1e-13 / h
        h = 1e-3
        for e in range(3):
            hi = [p + h * (d == e) for d, p in enumerate(pos)]
            lo = [p - h * (d == e) for d, p in enumerate(pos)]
            fd = (field64(f.nodes, spacing, hi) - field64(f.nodes, spacing, lo)) / (2 * h)
            assert np.abs(E[:, e] - fd).max() <= 16 * U * top * 1.5 / spacing[e] + 1e-8 * top, e


def linear_field(shape, spacing, A, b):
    """nodes linear in node position reproduce D(o) = A o + b: node g of an axis sits at voxel (g - 1) * s -- the coefficients
    c_g = g give sum_g g b3(u - g + 3) = u + 1"""
    g = M.grid_shape(shape, spacing)
    pos = np.stack(np.meshgrid(*[(np.arange(g[d]) - 1.0) * spacing[d] for d in range(3)], indexing="ij"))      # (3, Gz, Gy, Gx)
    return M.ElasticField(np.einsum("ce,eijk->cijk", np.asarray(A, dtype=np.float64), pos) + np.asarray(b, dtype=np.float64)[:, None, None, None],
                          spacing)


def check_linear_nodes_give_a_linear_field():
    shape, spacing = (17, 20, 33), (8, 16, 9)
    A = np.array([[0.01, -0.02, 0.03], [0.015, 0.0, -0.01], [-0.02, 0.025, 0.005]])
    b = np.array([0.5, -0.25, 1.0])
    f = linear_field(shape, spacing, A, b)
    D, E = M.displacement_numpy(f, shape)
    o = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij"))
    top = float(np.abs(f.nodes).max())
    assert np.abs(D - (np.einsum("ce,ezyx->czyx", A, o) + b[:, None, None, None])).max() <= 17 * U * top      # (+ the nodes' own rounding)
    for d in range(3):
        for e in range(3):
            assert np.abs(E[d, e] - A[d, e]).max() <= 17 * U * top * 1.5 / spacing[e], (d, e)


def check_identity():
    """the zero field returns the input's bits.  Linear: a + 0 * (b - a) is a for finite data without -0.0 (that one becomes
    +0.0: `positive_field`).  Vector rule: t = n and k = sqrt(q / q) = 1 EXCEPT where q = |s|^2 leaves the float32 range: all
    components below about 1e-23 (q = 0: the output is 0) or one above about 1e19 (q = inf); elsewhere -- a -0.0 component aside,
    n + 0 is +0.0 -- the bits are the input's, and values compare == everywhere in range."""
    shape = (9, 12, 17)
    zero = M.ElasticField.zero(shape, 8)
    assert zero.is_identity() and zero.nodes.shape == (3, 5, 5, 6) and zero.fits(shape) and not zero.fits((9, 12, 18 + 8))
    x = positive_field((3, *shape), 0)
    for interp in ("linear", "nearest"):
        for border in ("constant", "clamp"):
            for fill in (0.0, 0.5):
                assert same_bits(M.elastic_numpy(zero, x, interp, border, fill), x), (interp, border, fill)
                assert same_bits(M.elastic_numpy(zero, x[0], interp, border, fill), x[0])
            assert same_bits(M.elastic_numpy(zero, x, interp, border, 0.0, True), x), (interp, border)
    signed = (x - np.float32(0.75)) * (np.random.default_rng(1).random(shape) < 0.6).astype(np.float32)      # zeros of both signs
    got = M.elastic_numpy(zero, signed, "nearest", "constant", 0.0, True)
    assert (got == signed).all() and same_bits(np.abs(got), np.abs(signed))
    tiny = np.full((3, *shape), 1e-30, dtype=np.float32)                                            # the stated exception
    assert (M.elastic_numpy(zero, tiny, "nearest", "constant", 0.0, True) == 0).all()


def check_uniform_shift():
    """every node 0.6 along x: D_x = 0.6 to rounding, nearest reads the next voxel (floor(o + 0.6 + 0.5) = o + 1), linear blends"""
    shape = (9, 10, 20)
    nodes = np.zeros((3,) + M.grid_shape(shape, (8, 8, 8)))
    nodes[2] = 0.6
    f = M.ElasticField(nodes, 8)
    x = positive_field(shape, 3)
    near = M.elastic_numpy(f, x, "nearest", "constant", 7.0)
    assert same_bits(near[..., :-1], x[..., 1:]) and (near[..., -1] == 7.0).all()
    near = M.elastic_numpy(f, x, "nearest", "clamp")
    assert same_bits(near[..., :-1], x[..., 1:]) and same_bits(near[..., -1], x[..., -1])
    lin = M.elastic_numpy(f, x, "linear", "clamp")
    assert np.abs(lin[..., :-1] - (0.4 * x[..., :-1].astype(np.float64) + 0.6 * x[..., 1:])).max() < 1e-5
    nodes[2], nodes[0] = 0.0, -1.0                                                          # along z: one plane back (the weights sum to 1 +- 7 U)
    assert np.abs(M.elastic_numpy(M.ElasticField(nodes, 8), x, "linear", "clamp")[1:] - x[:-1]).max() < 1e-5


def rotation_field(shape, spacing, axis, deg):
    """the displacement of `rotation_op(axis, deg)`: p = point (o - c) + c, so D(o) = (point - I)(o - c)"""
    op = S.rotation_op(axis, deg)
    A = op.point64 - np.eye(3)
    c = (np.array(shape, dtype=np.float64) - 1.0) / 2.0
    return op, linear_field(shape, spacing, A, -A @ c)


def check_vector_rule():
    shape, spacing = (16, 18, 20), (8, 8, 8)
    rng = np.random.default_rng(5)
    for axis, deg in (("z", 4.0), ("y", -3.0), ("x", 5.0)):
        op, f = rotation_field(shape, spacing, axis, deg)
        D, E = M.displacement_numpy(f, shape)
        # I + E is the pull-back (`point`) matrix; its transpose, read in (x, y, z) order, is the `vector` matrix
        JT = (np.eye(3)[:, :, None, None, None] + E.astype(np.float64)).transpose(1, 0, 2, 3, 4)[::-1, ::-1]
        assert np.abs(JT - op.vector64[:, :, None, None, None]).max() <= 1e-5, axis
        n = rng.standard_normal(3)
        n = (n / np.linalg.norm(n)).astype(np.float32)
        const = np.broadcast_to(n[:, None, None, None], (3, *shape)).copy()
        got = M.elastic_numpy(f, const, "nearest", "clamp", 0.0, True)
        assert np.abs(got - (op.vector64 @ n.astype(np.float64))[:, None, None, None]).max() <= 1e-5, axis
    # any field: the sampled length is kept (k carries / and sqrt: 1 U; t * k: 1 U per component; the length's own sums: 2 U; 8 U
    # covers them with the second order), zero normals stay zero, a binary label stays binary
    shape = (17, 33, 70)
    f = random_field(shape, (8, 16, 32), 8 / 6 * 0.999, 7)
    mask = rng.random(shape) < 0.4
    normals = rng.standard_normal((3, *shape)).astype(np.float32) * mask
    label = mask.astype(np.float32)
    out_n = M.elastic_numpy(f, normals, "nearest", "constant", 0.0, True)
    out_l = M.elastic_numpy(f, label, "nearest", "constant", 0.0)
    sampled = M.elastic_numpy(f, normals, "nearest", "constant", 0.0, False)
    assert set(np.unique(out_l)) <= {0.0, 1.0} and 0.2 < out_l.mean() < 0.6
    assert (out_n[:, out_l == 0] == 0).all() and (np.abs(out_n[:, out_l == 1]).sum(axis=0) > 0).all()
    len_s, len_o = np.linalg.norm(sampled.astype(np.float64), axis=0), np.linalg.norm(out_n.astype(np.float64), axis=0)
    assert np.abs(len_o - len_s).max() <= 8 * U * len_s.max()
    assert not same_bits(out_n, sampled)
    # the rule itself, against float64: (I + E)^T n at the sampled length
    D, E = M.displacement_numpy(f, shape)
    J = np.eye(3)[:, :, None, None, None] + E.astype(np.float64)
    nz = sampled[::-1].astype(np.float64)
    t = np.einsum("dezyx,dzyx->ezyx", J, nz)
    want = (t / np.maximum(np.linalg.norm(t, axis=0), 1e-300) * len_s)[::-1]
    assert np.abs(out_n - want).max() <= 1e-5


def check_no_folding():
    """hi just under min(spacing) / 6: rows of I + E are strictly diagonally dominant, so det > 0 at every voxel"""
    shape, spacing = (24, 40, 56), (8, 12, 16)
    hi = min(spacing) / 6.0 * (1.0 - 1e-9)
    rng = random.Random(2024)
    smallest = np.inf
    for _ in range(20):
        f = M.draw_elastic(rng, shape, spacing, (hi, hi), 1.0)
        assert not f.is_identity() and float(np.abs(f.nodes).max()) <= hi
        E = jacobian64(f.nodes, spacing, shape)
        for e in range(3):
            assert np.abs(E[:, e]).max() <= 2 * hi / spacing[e] * (1 + 1e-6)
        J = (np.eye(3)[:, :, None, None, None] + E).transpose(2, 3, 4, 0, 1)
        smallest = min(smallest, float(np.linalg.det(J).min()))
    assert smallest > 0.0
    with pytest.raises(ValueError, match=r"elastic\.magnitude.*fold"):
        M.parse_elastic({"elastic": dict(BLOCK, spacing=[8, 12, 16], magnitude=[0, 8 / 6])}, (24, 40, 56), TASKS)
    assert M.parse_elastic({"elastic": dict(BLOCK, spacing=[8, 12, 16], magnitude=[0, hi])}, (24, 40, 56), TASKS)["magnitude"] == (0.0, hi)


class RecordingRng:
    def __init__(self, first):
        self.calls, self.first, self.inner = [], first, random.Random(9)

    def random(self):
        self.calls.append(("random",))
        return self.first

    def uniform(self, lo, hi):
        self.calls.append(("uniform", lo, hi))
        return self.inner.uniform(lo, hi)


def check_draw_order():
    shape, spacing = (9, 17, 33), (8, 8, 16)
    g = M.grid_shape(shape, spacing)
    assert g == (5, 6, 6)
    miss = RecordingRng(0.3)
    f = M.draw_elastic(miss, shape, spacing, (1.0, 1.2), 0.3)          # 0.3 is not < 0.3
    assert miss.calls == [("random",)] and f.is_identity() and f.nodes.shape == (3, *g) and f.spacing == spacing
    hit = RecordingRng(0.29)
    f = M.draw_elastic(hit, shape, spacing, (1.0, 1.2), 0.3)
    assert hit.calls == [("random",), ("uniform", 1.0, 1.2)] + [("uniform", -1.0, 1.0)] * (3 * 5 * 6 * 6)
    replay = random.Random(9)
    a = replay.uniform(1.0, 1.2)
    want = np.array([replay.uniform(-1.0, 1.0) * a for _ in range(3 * 5 * 6 * 6)]).astype(np.float32).reshape(3, *g)      # C order of (c, z, y, x)
    assert same_bits(f.nodes, want) and f == M.ElasticField(want, spacing) and f != M.ElasticField(want, (8, 8, 17))


# ---- the kernel's own functions on the CPU, under AddressSanitizer ---------------------------------------------------------------------
_EXE = {}


def host_check_exe(tmp_dir):
    if "exe" not in _EXE:
        csrc = os.path.join(ROOT, "multi-task-3d-resencoder-unet_amd", "csrc")
        exe = os.path.join(str(tmp_dir), "elastic_host_check")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-Wno-unknown-pragmas", os.path.join(csrc, "tools", "elastic_host_check.cpp"), "-o", exe])
        _EXE["exe"] = exe
    return _EXE["exe"]


def check_host_program(tmp_dir, shapes=(((9, 10, 11), (8, 8, 8)), ((6, 12, 20), (8, 16, 9)), ((9, 5, 33), (11, 8, 32)))):
    """csrc/rx_elastic_core.h and rx_affine_core.h are what the kernel calls.  A stand-alone C++ program runs them over small cases
    against a dump of elastic_numpy, compiled with -fsanitize=address,undefined (and without fp contraction): every voxel must have
    elastic_numpy's bits and no load may leave the heap buffers of nodes, tables and sample, whatever the nodes hold."""
    exe = host_check_exe(tmp_dir)
    cases = []
    for si, (shape, spacing) in enumerate(shapes):
        fields = [M.ElasticField.zero(shape, spacing), random_field(shape, spacing, min(spacing) / 6 * 0.999, si),
                  random_field(shape, spacing, 3.0, 10 + si), random_field(shape, spacing, 1e6, 20 + si)]
        for ci, (channels, interp, border, fill, vector) in enumerate([(1, "linear", "constant", 0.0, False), (2, "linear", "constant", 0.5, False),
                                                                       (3, "linear", "clamp", 0.0, True), (3, "nearest", "constant", 0.0, True),
                                                                       (3, "nearest", "clamp", 0.5, False), (3, "linear", "constant", 0.5, True)]):
            x = positive_field((channels, *shape), ci) - np.float32(0.6 if vector else 0.0)
            for f in fields:
                cases.append((x, f, S.INTERP[interp], S.BORDER[border], fill, vector, M.elastic_numpy(f, x, interp, border, fill, vector)))
    dump = os.path.join(str(tmp_dir), "cases.bin")
    with open(dump, "wb") as fh:
        fh.write(struct.pack("<i", len(cases)))
        for x, f, interp, border, fill, vector, want in cases:
            fh.write(struct.pack("<10i", *x.shape, interp, border, int(vector), *f.spacing))
            fh.write(struct.pack("<f", fill))
            fh.write(f.nodes.astype("<f4").tobytes())
            for n, s in zip(x.shape[1:], f.spacing):
                idx, w, dw = M.bspline_tables(n, s)
                fh.write(idx.astype("<i4").tobytes() + w.astype("<f4").tobytes() + dw.astype("<f4").tobytes())
            fh.write(x.astype("<f4").tobytes())
            fh.write(want.astype("<f4").tobytes())
    r = subprocess.run([exe, dump], capture_output=True, text=True, timeout=300)
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and f"{len(cases)} cases, 0 voxels differ" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    assert len(cases) == 24 * len(shapes)


# ---- the tests ------------------------------------------------------------------------------------------------------------------
def test_tables():
    check_tables()


def test_displacement_and_jacobian_against_float64():
    check_displacement()


def test_linear_nodes_give_a_linear_field():
    check_linear_nodes_give_a_linear_field()


def test_zero_field_is_the_identity():
    check_identity()


def test_uniform_shift():
    check_uniform_shift()


def test_vector_rule():
    check_vector_rule()


def test_no_folding_below_the_parsers_limit():
    check_no_folding()


def test_draw_order():
    check_draw_order()


def test_kernel_arithmetic_on_the_cpu_matches_the_statement(tmp_path):
    check_host_program(tmp_path)


def test_fields_and_statement_arguments():
    with pytest.raises(ValueError, match=r"ElasticField\.spacing"):
        M.ElasticField(np.zeros((3, 5, 5, 5)), 7)
    with pytest.raises(ValueError, match=r"ElasticField\.spacing"):
        M.ElasticField(np.zeros((3, 5, 5, 5)), (8, 8))
    with pytest.raises(ValueError, match=r"ElasticField\.spacing"):
        M.ElasticField(np.zeros((3, 5, 5, 5)), 8.0)
    with pytest.raises(ValueError, match=r"ElasticField\.nodes"):
        M.ElasticField(np.zeros((2, 5, 5, 5)), 8)
    with pytest.raises(ValueError, match=r"ElasticField\.nodes"):
        M.ElasticField(np.zeros((3, 3, 5, 5)), 8)
    f = M.ElasticField.zero((9, 9, 9), 8)
    with pytest.raises(ValueError):
        f.nodes[0, 0, 0, 0] = 1.0
    x = positive_field((3, 9, 9, 9), 0)
    with pytest.raises(ValueError, match="do not fit"):
        M.elastic_numpy(f, positive_field((9, 9, 17), 0), "linear", "constant")
    with pytest.raises(ValueError, match="interp"):
        M.elastic_numpy(f, x, "cubic", "constant")
    with pytest.raises(ValueError, match="border"):
        M.elastic_numpy(f, x, "linear", "reflect")
    with pytest.raises(ValueError, match="3 components"):
        M.elastic_numpy(f, x[:2], "nearest", "constant", 0.0, True)
    with pytest.raises(ValueError, match="float32"):
        M.elastic_numpy(f, x.astype(np.float64), "linear", "constant")
    g = random_field((9, 9, 9), 8, 1.0, 0)
    y = M.elastic_numpy(g, x, "linear", "clamp")
    assert y.flags["C_CONTIGUOUS"] and not np.shares_memory(y, x) and same_bits(y[1], M.elastic_numpy(g, x[1], "linear", "clamp"))
    item = M.apply_item_numpy(g, {"image": torch.from_numpy(x[:1]), "sheet": x[1], "normals": x}, ("normals",), "clamp", 0.0)
    assert isinstance(item["image"], torch.Tensor) and same_bits(item["image"].numpy(), M.elastic_numpy(g, x[:1], "linear", "clamp"))
    assert same_bits(item["sheet"], M.elastic_numpy(g, x[1], "nearest", "constant")) and isinstance(item["sheet"], np.ndarray)
    assert same_bits(item["normals"], M.elastic_numpy(g, x, "nearest", "constant", 0.0, True))


def test_parse_elastic():
    assert M.parse_elastic({}, (16, 16, 16), TASKS) is None and M.parse_elastic(None, (16, 16, 16), TASKS) is None
    assert M.parse_elastic({"elastic": False}, (16, 16, 16), TASKS) is None
    assert M.parse_elastic({"elastic": BLOCK}, (16, 16, 16), TASKS) == {
        "spacing": (8, 8, 8), "magnitude": (0.0, 1.25), "p": 0.3, "normal_keys": ("normals",), "image_border": "constant", "where": "device"}
    assert M.parse_elastic({"elastic": True}, (128, 128, 128), TASKS) == {
        "spacing": (32, 32, 32), "magnitude": (0.0, 4.0), "p": 0.3, "normal_keys": ("normals",), "image_border": "constant", "where": "device"}
    got = M.parse_elastic({"elastic": {"spacing": [8, 16, 32], "where": "HOST", "image_border": "clamp", "magnitude": [1, 1], "p": 1}}, (16, 16, 16), TASKS)
    assert got["spacing"] == (8, 16, 32) and got["where"] == "host" and got["image_border"] == "clamp" and got["magnitude"] == (1.0, 1.0)
    refused = {
        "elastic: unknown": dict(BLOCK, rotation={}),
        "elastic.p": dict(BLOCK, p=1.5),
        "elastic.p:": dict(BLOCK, p=-0.1),
        "elastic.spacing": dict(BLOCK, spacing=7),
        "elastic.spacing:": dict(BLOCK, spacing=[8, 8]),
        "elastic.spacing: ": dict(BLOCK, spacing=8.5),
        "elastic.spacing:  ": dict(BLOCK, spacing=[8, 16, 4]),
        "elastic.magnitude": dict(BLOCK, magnitude=[-1, 1]),
        "elastic.magnitude:": dict(BLOCK, magnitude=[1, 0.5]),
        "elastic.magnitude: ": dict(BLOCK, magnitude=3),
        "elastic.magnitude:  ": dict(BLOCK, magnitude=[0, 8 / 6]),          # the fold condition: hi < min(spacing) / 6
        "elastic.where": dict(BLOCK, where="gpu"),
        "elastic.image_border": dict(BLOCK, image_border="reflect"),
    }
    for key, block in refused.items():
        with pytest.raises(ValueError, match=r"dataset_config\." + key.rstrip(": ").replace(".", r"\.")):
            M.parse_elastic({"elastic": block}, (16, 16, 16), TASKS)
    with pytest.raises(ValueError, match=r"dataset_config\.elastic.*3-D patch"):
        M.parse_elastic({"elastic": BLOCK}, (64, 64), TASKS)
    with pytest.raises(ValueError, match=r"dataset_config\.elastic\.normal_keys.*sheet"):
        M.parse_elastic({"elastic": dict(BLOCK, normal_keys=["sheet"])}, (16, 16, 16), TASKS)
    with pytest.raises(ValueError, match=r"dataset_config\.elastic: expected a mapping"):
        M.parse_elastic({"elastic": 3}, (16, 16, 16), TASKS)
    # the neighbours' blocks and parsers are untouched by the new one
    assert S.parse_spatial({"elastic": BLOCK}, (16, 16, 16), TASKS) is None
    with pytest.raises(ValueError, match=r"DeviceElastic\.magnitude"):
        M.DeviceElastic(spacing=8, magnitude=(0, 2))


def test_zarr_dataset_refuses_host_elastic_behind_device_stages(tmp_path):
    from mt3d_amd.dataloading.dataset import ZarrSegmentationDataset3D
    from mt3d_amd.dataloading.stages import check_stage_order

    def mgr(dilate_label=False, **dataset_config):
        return SimpleNamespace(model_name="m", tasks=TASKS, train_patch_size=(16, 16, 16), min_labeled_ratio=0.1, min_bbox_percent=0.9,
                               dilate_label=dilate_label, use_cache=False, cache_folder=str(tmp_path), volume_paths=[],
                               dataset_config=dict(augment=False, **dataset_config))
    host = dict(BLOCK, where="host")
    with pytest.raises(ValueError, match=r"dataset_config\.elastic\.where.*ingest"):
        ZarrSegmentationDataset3D(mgr(elastic=host, ingest={"where": "device"}))
    with pytest.raises(ValueError, match=r"dataset_config\.elastic\.where.*dilate"):
        ZarrSegmentationDataset3D(mgr(dilate_label=True, elastic=host, dilate={"where": "device"}))
    with pytest.raises(ValueError, match=r"dataset_config\.elastic\.where.*ingest"):
        check_stage_order(False, None, None, {"where": "device"}, None, {"where": "host"})
    check_stage_order(False, None, {"where": "device"}, {"where": "device"}, None, {"where": "device"})
    check_stage_order(False, None, {"where": "device"}, {"where": "device"}, None, None)
    assert ZarrSegmentationDataset3D(mgr(elastic=BLOCK, ingest={"where": "device"})).device_elastic["where"] == "device"
    ds = ZarrSegmentationDataset3D(mgr(dilate_label=True, elastic=host, dilate={"where": "host"}))
    assert ds.device_elastic is None and ds.elastic["where"] == "host"
    assert ZarrSegmentationDataset3D(mgr()).elastic is None and ZarrSegmentationDataset3D(mgr()).device_elastic is None


def _synthetic(**dataset_config):
    from mt3d_amd.dataloading.dataset import SyntheticPatchDataset
    return SyntheticPatchDataset(SimpleNamespace(train_patch_size=(12, 12, 12), in_channels=1, tasks=TASKS,
                                                 dataset_config=dict(synthetic_length=8, synthetic_pool=4, **dataset_config)))


def _check_host_items(host, plain, indices):
    host.elastic_rng = random.Random(7)
    want_rng = random.Random(7)
    cfg = host.elastic
    for idx in indices:
        item, raw = host[idx], plain[idx]
        f = M.draw_elastic(want_rng, (12, 12, 12), cfg["spacing"], cfg["magnitude"], cfg["p"])
        assert host.last_elastic_field == f and not f.is_identity()
        assert same_bits(item["image"].numpy(), M.elastic_numpy(f, raw["image"].numpy(), "linear", "constant", 0.0))
        assert same_bits(item["sheet"].numpy(), M.elastic_numpy(f, raw["sheet"].numpy(), "nearest", "constant", 0.0))
        assert same_bits(item["normals"].numpy(), M.elastic_numpy(f, raw["normals"].numpy(), "nearest", "constant", 0.0, True))
        assert not torch.equal(item["image"], raw["image"])
        assert item["image"].dtype == torch.float32 and item["normals"].shape == raw["normals"].shape


def test_host_path_of_the_synthetic_dataset():
    plain, dev = _synthetic(), _synthetic(elastic=BLOCK)
    assert plain.elastic is None and plain.device_elastic is None
    assert dev.device_elastic == dev.elastic and dev.elastic["where"] == "device"
    for k, v in dev[1].items():          # where: device leaves the items alone; the key absent: the items of before
        assert torch.equal(v, plain[1][k])
    host = _synthetic(elastic=dict(BLOCK, where="host", p=1.0, magnitude=[0.5, 1.25]))
    assert host.device_elastic is None
    _check_host_items(host, plain, (1, 2, 1))
    assert set(np.unique(host[3]["sheet"].numpy())) <= {0.0, 1.0}
    for k, v in plain[1].items():          # the pool's cached items were not written to
        assert torch.equal(v, _synthetic()[1][k])
    never = _synthetic(elastic=dict(BLOCK, where="host", p=0.0))
    for k, v in never[2].items():
        assert torch.equal(v, plain[2][k])
    assert never.last_elastic_field.is_identity()
    # after the host spatial stage: spatial, then elastic
    both = _synthetic(spatial={"rotation": {"p": 1.0}, "where": "host"}, elastic=dict(BLOCK, where="host", p=1.0, magnitude=[1, 1]))
    both.spatial_rng, both.elastic_rng = random.Random(1), random.Random(2)
    item, raw = both[0], plain[0]
    mid = S.affine_numpy(both.last_spatial_op, raw["image"].numpy(), "linear", "constant", 0.0)
    assert same_bits(item["image"].numpy(), M.elastic_numpy(both.last_elastic_field, mid, "linear", "constant", 0.0))


def test_host_path_of_the_zarr_dataset(tmp_path):
    from mt3d_amd.dataloading.dataset import ZarrSegmentationDataset3D
    D = 24
    idx = (np.arange(D ** 3, dtype=np.int64) % 60000 + 1).astype(np.uint16).reshape(D, D, D)
    nrm = np.stack([idx // 3, idx // 3 + 20000, idx // 3 + 40000], axis=-1).astype(np.uint16)
    paths = {}
    for name, arr, ch in [("img", idx, (16, 16, 16)), ("sheet", idx, (16, 16, 16)), ("normals", nrm, (16, 16, 16, 3))]:
        paths[name] = str(tmp_path / f"{name}.zarr")
        zarr_lite.write_array(paths[name], arr, ch, compressor="zlib")

    def mgr(**dataset_config):
        return SimpleNamespace(model_name="e", tasks=TASKS, train_patch_size=(12, 12, 12), min_labeled_ratio=0.1, min_bbox_percent=0.5,
                               dilate_label=False, use_cache=False, cache_folder=str(tmp_path / "cache"),
                               dataset_config=dict(augment=False, **dataset_config),
                               volume_paths=[{"input": paths["img"], "sheet": paths["sheet"], "normals": paths["normals"], "ref_label": "sheet"}])
    plain = ZarrSegmentationDataset3D(mgr())
    host = ZarrSegmentationDataset3D(mgr(elastic=dict(BLOCK, where="host", p=1.0, magnitude=[0.5, 1.25])))
    dev = ZarrSegmentationDataset3D(mgr(elastic=BLOCK))
    assert len(plain) > 0 and len(host) == len(plain) and dev.device_elastic is not None and host.device_elastic is None
    for k, v in plain[0].items():          # where: device -> the items of the run without the key, bit for bit
        assert torch.equal(v, dev[0][k]) and v.dtype == dev[0][k].dtype
    _check_host_items(host, plain, (0, len(plain) - 1, 0))


# ---- planted faults ---------------------------------------------------------------------------------------------------------------
def _displacement_xyz(field, shape):
    """`displacement_numpy` with the sums taken x first, then y, then z: the same value up to rounding"""
    (iz, wz, dwz), (iy, wy, dwy), (ix, wx, dwx) = (M.bspline_tables(n, s) for n, s in zip(shape, field.spacing))
    iz, iy, ix = iz.astype(np.int64), iy.astype(np.int64), ix.astype(np.int64)

    def total(az, ay, ax):
        return M._sum4(az, M._sum4(ay, M._sum4(ax, field.nodes, 3, ix), 2, iy), 1, iz)
    D = total(wz, wy, wx)
    E = np.stack([total(dwz, wy, wx), total(wz, dwy, wx), total(wz, wy, dwx)], axis=1)
    return np.ascontiguousarray(D, dtype=np.float32), np.ascontiguousarray(E, dtype=np.float32)


def test_planted_faults_are_caught(tmp_path, monkeypatch):
    """each fault, planted in the module, must make at least one of the checks above fail.  Counted here (checks that fail out of
    the nine): transposed Jacobian 4, component order (Nz, Ny, Nx) 2, sum order x, y, z 1 (the bit-for-bit host program: the
    value is the same to rounding), dw not divided by the spacing 4, nearest as floor(p) 2."""
    real_disp, real_rule, real_tables, real_sample = M.displacement_numpy, M.vector_rule_numpy, M.bspline_tables, M.sample_numpy

    def transposed(field, shape):
        D, E = real_disp(field, shape)
        return D, np.ascontiguousarray(E.transpose(1, 0, 2, 3, 4))

    def zyx_components(s, E):
        return real_rule(s[::-1], E)[::-1]

    def dw_not_divided(n, s):
        idx, w, dw = real_tables(n, s)
        return idx, w, (dw.astype(np.float64) * s).astype(np.float32)

    def nearest_is_floor(a, p, interp, border, fill=0.0):
        if interp == "nearest":
            p = [v - np.float32(0.5) for v in p]
        return real_sample(a, p, interp, border, fill)

    faults = {"transposed Jacobian": ("displacement_numpy", transposed), "component order (Nz, Ny, Nx)": ("vector_rule_numpy", zyx_components),
              "sum order x, y, z": ("displacement_numpy", _displacement_xyz), "dw not divided by s": ("bspline_tables", dw_not_divided),
              "nearest as floor(p)": ("sample_numpy", nearest_is_floor)}
    small = (((9, 10, 11), (8, 8, 8)),)
    checks = [check_tables, check_displacement, check_linear_nodes_give_a_linear_field, check_identity, check_uniform_shift,
              check_vector_rule, check_no_folding, check_draw_order, lambda: check_host_program(tmp_path, small)]
    for c in checks:          # (all green without a fault)
        c()
    tripped = {}
    for name, (attr, fn) in faults.items():
        with monkeypatch.context() as mp:
            mp.setattr(M, attr, fn)
            count = 0
            for c in checks:
                try:
                    c()
                except AssertionError:
                    count += 1
            tripped[name] = count
    print("planted faults -> failing checks:", tripped)
    assert all(v >= 1 for v in tripped.values()), tripped
