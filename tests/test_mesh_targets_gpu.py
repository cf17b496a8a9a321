"""GPU: csrc/rx_meshslice.hip through engine/ops/mesh.py against the numpy statement (tasks/normals/mesh_targets.py), bit for bit: every
golden case of tests/golden/mesh_slices.npz on every output (codes, viz bytes, mask, labels, keys), slabs that cut through a
triangle's z-range, windows with odd offsets and widths that are no multiple of 4 (the dword stores' edges), 24 seeded random
meshes with degenerate and duplicate triangles, and two runs of one input byte for byte.  Outputs live in 0xFF-poisoned buffers with
fences on both sides."""
import numpy as np
import pytest
import torch

import mt3d_amd  # noqa: F401
from mt3d_amd.engine import lib as L
from mt3d_amd.engine import ops
from mt3d_amd.tasks.normals import mesh_targets as M

from mesh_cases import golden, random_statement

pytestmark = pytest.mark.gpu
CASES, META = golden()
FENCE = 256      # bytes; a multiple of 16 keeps the payload's alignment


class Fenced:
    """a payload of `shape` x `dtype` inside a 0xFF-filled byte buffer"""

    def __init__(self, shape, dtype):
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        self.n = n
        self.buf = torch.full((FENCE + n + FENCE,), 0xFF, dtype=torch.uint8, device="cuda")
        self.t = self.buf[FENCE:FENCE + n].view(dtype).view(shape)

    def check(self):
        b = self.buf.cpu().numpy()
        assert (b[:FENCE] == 0xFF).all() and (b[FENCE + self.n:] == 0xFF).all(), "a store left the output"


def dev(m):
    return (torch.from_numpy(m["vertices"]).cuda(), torch.from_numpy(m["triangles"].astype(np.int32)).cuda(),
            torch.from_numpy(m["normals"]).cuda(), torch.from_numpy(m["tri_labels"].astype(np.int32)).cuda())


def u16(t):
    return t.cpu().view(torch.int16).numpy().view(np.uint16)


def run_normals(m, d, z0, nz, window, exp_factor=1.5):
    y0, x0, wh, ww = window if window is not None else (0, 0, m["h"], m["w"])
    out = {"normals": Fenced((nz, wh, ww, 3), ops._U16), "viz": Fenced((nz, wh, ww, 3), torch.uint8), "mask": Fenced((nz, wh, ww), torch.uint8)}
    keys = Fenced((nz, wh, ww), torch.int64)
    r = ops.mesh_slice_normals(d[0], d[1], d[2], m["w"], m["h"], z0, nz, window=window, exp_factor=exp_factor, want_viz=True, want_mask=True,
                               keys=keys.t, out={k: f.t for k, f in out.items()})
    torch.cuda.synchronize()
    for f in (*out.values(), keys):
        f.check()
    return u16(r["normals"]), r["viz"].cpu().numpy(), r["mask"].cpu().numpy(), r["keys"].cpu().numpy()


def run_labels(m, d, z0, nz, window):
    y0, x0, wh, ww = window if window is not None else (0, 0, m["h"], m["w"])
    out = {"labels": Fenced((nz, wh, ww), ops._U16), "mask": Fenced((nz, wh, ww), torch.uint8)}
    keys = Fenced((nz, wh, ww), torch.int32)
    r = ops.mesh_slice_labels(d[0], d[1], d[3], m["w"], m["h"], z0, nz, window=window, want_mask=True, keys=keys.t,
                              out={k: f.t for k, f in out.items()})
    torch.cuda.synchronize()
    for f in (*out.values(), keys):
        f.check()
    return u16(r["labels"]), r["mask"].cpu().numpy(), r["keys"].cpu().numpy()


def check_against(m, d, img, viz, lab, z0, nz, window):
    """device slab [z0, z0 + nz) x window == the statement's volume (slices from m['z0'] on) cropped"""
    y0, x0, wh, ww = window if window is not None else (0, 0, m["h"], m["w"])
    k0 = z0 - m["z0"]
    crop = np.s_[k0:k0 + nz, y0:y0 + wh, x0:x0 + ww]
    gi, gv, gm, gk = run_normals(m, d, z0, nz, window)
    assert np.array_equal(gi, img[crop]), f"{int((gi != img[crop]).sum())} codes differ"
    assert np.array_equal(gv, viz[crop])
    assert np.array_equal(gm, img[crop].any(axis=3).astype(np.uint8) * 255)
    assert np.array_equal(gk != 0, img[crop].any(axis=3))
    gl, glm, glk = run_labels(m, d, z0, nz, window)
    assert np.array_equal(gl, lab[crop]), f"{int((gl != lab[crop]).sum())} labels differ"
    assert np.array_equal(glm, (lab[crop] > 0).astype(np.uint8) * 255)
    return gk, glk


@pytest.mark.parametrize("ci", range(len(CASES)))
def test_golden_cases_full(ci):
    c = CASES[ci]
    gk, glk = check_against(c, dev(c), c["img"], c["viz"], c["lab"], c["z0"], c["nz"], None)
    # the keys themselves are the statement's: the same winner, not just the same value
    k = c["nz"] // 2
    want = M.keys_normals_numpy(c["vertices"], c["triangles"], c["normals"], c["z0"] + k, c["w"], c["h"], META["exp_factor"])
    assert np.array_equal(gk[k].view(np.uint64), want)
    assert np.array_equal(glk[k].view(np.uint32), M.keys_labels_numpy(c["vertices"], c["triangles"], c["z0"] + k, c["w"], c["h"]))


@pytest.mark.parametrize("ci", range(len(CASES)))
def test_slabs_and_windows_are_crops(ci):
    """slab starts and ends inside triangles' z-ranges (every interior slice of these cases is); window offsets odd, widths 1, 3, 5, 7
    and 9 (no multiple of 4), so rows start and end inside dwords of the uint16 x 3, uint8 x 3, uint16 and uint8 streams"""
    c = CASES[ci]
    d = dev(c)
    w, h = c["w"], c["h"]
    for (z0, nz), window in [((c["z0"] + 1, 1), (1, 3, h - 4, w - 7)), ((c["z0"] + 2, 3), (h // 2 - 1, w // 3 | 1, 5, 9)),
                             ((c["z0"] + 3, 2), (0, 1, 7, 3)), ((c["z0"] + 1, c["nz"] - 2), (3, 5, 3, 5)), ((c["z0"] + 2, 1), (h - 1, w - 1, 1, 1)),
                             ((c["z0"] + 1, 2), (5, 0, 1, w))]:
        check_against(c, d, c["img"], c["viz"], c["lab"], z0, nz, window)


def test_exp_factor_other_than_default():
    c = CASES[0]
    d = dev(c)
    for ef in (0.5, 3.2):      # 3 and 16 samples
        want = M.normals_volume_numpy(c["vertices"], c["triangles"], c["normals"], c["w"], c["h"], 2, 2, exp_factor=ef)
        got = run_normals(c, d, 2, 2, None, exp_factor=ef)[0]
        assert np.array_equal(got, want)


@pytest.mark.parametrize("seed", range(24))
def test_random_meshes(seed):
    m, img, viz, lab = random_statement(seed)
    d = dev(m)
    check_against(m, d, img, viz, lab, 0, m["nz"], None)
    if m["nz"] >= 3 and m["w"] >= 8 and m["h"] >= 8:
        check_against(m, d, img, viz, lab, 1, m["nz"] - 2, (1, 3, m["h"] - 3, m["w"] - 6))


def test_two_runs_are_byte_identical():
    c = CASES[2]
    d = dev(c)
    a = run_normals(c, d, c["z0"], c["nz"], None)
    b = run_normals(c, d, c["z0"], c["nz"], None)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    la, lb = run_labels(c, d, c["z0"], c["nz"], None), run_labels(c, d, c["z0"], c["nz"], None)
    for x, y in zip(la, lb):
        assert x.tobytes() == y.tobytes()


def test_device_refusals():
    c = CASES[1]
    v, t, n, lab = dev(c)
    w, h = c["w"], c["h"]
    bad = v.clone()
    bad[2, 0] = float("nan")
    with pytest.raises(L.RxError):
        ops.mesh_slice_normals(bad, t, n, w, h, 0, 2)
    bad[2, 0] = 2.0 ** 24
    with pytest.raises(L.RxError):
        ops.mesh_slice_labels(bad, t, lab, w, h, 0, 2)
    tt = t.clone()
    tt[1, 1] = v.shape[0]
    with pytest.raises(L.RxError):
        ops.mesh_slice_normals(v, tt, n, w, h, 0, 2)
    tt[1, 1] = -1
    with pytest.raises(L.RxError):
        ops.mesh_slice_labels(v, tt, lab, w, h, 0, 2)
    with pytest.raises(L.RxError):
        ops.mesh_slice_normals(v, t, n, w, h, 0, 2, exp_factor=3.4)          # 17 samples
    with pytest.raises(L.RxError):
        ops.mesh_slice_normals(v, t, n, w, h, 0, 2, exp_factor=0.01)         # 1 sample
    with pytest.raises(L.RxError):
        ops.mesh_slice_normals(v, t, n, w, h, 0, 2, window=(0, 0, h, w + 1))
    with pytest.raises(L.RxError):
        ops.mesh_slice_labels(v, t, lab + 65536, w, h, 0, 2)
    with pytest.raises(L.RxError):
        ops.mesh_slice_normals(v, t.to(torch.int64), n, w, h, 0, 2)
    # the key's 20 step bits: an image whose diagonal allows 2^20 steps is refused by the library before any launch
    keys = torch.zeros((1, 1, 1), dtype=torch.int64, device="cuda")
    rc = L.load().rx_mesh_slice_keys(0, v.data_ptr(), v.shape[0], t.data_ptr(), t.shape[0], n.data_ptr(), 1 << 19, 1 << 19, 0, 1, 0, 0, 1, 1, 1.5,
                                     keys.data_ptr(), None)
    assert rc != 0 and b"2^20" in L.load().rx_last_error()
    torch.cuda.synchronize()
