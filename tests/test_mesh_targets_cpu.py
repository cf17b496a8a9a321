"""CPU: tasks/normals/mesh_targets.py -- the two statements against the slices the reference's own functions painted
(tests/golden/mesh_slices.npz), the order-key argument (paint serially == take the largest key, then resolve), the key fields at
their limits, the refusals, slabs and windows as crops, the OBJ reader, the vertex normals where they are known, the fixture's hit
counts, the host path of the builder, and the kernels' own per-pixel functions run on the CPU under AddressSanitizer."""
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import mt3d_amd  # noqa: F401
from mt3d_amd.dataloading import zarr_lite
from mt3d_amd.tasks.normals import mesh_targets as M

from mesh_cases import golden, random_statement

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES, META = golden()
MINIMUM = {"on_plane_vertex": 1, "duplicate_point": 1, "in_plane_triangle": 1, "flat_edge_off_plane": 1, "margin_t_normals": 1,
           "margin_t_labels": 1, "segment_dropped_normals": 1, "label_pixel_clipped": 1, "half_coordinate": 1, "negative_half_coordinate": 1,
           "one_step_segment": 1, "zero_norm_pixel": 1, "pixels_two_triangles": 50, "pixels_one_triangle_twice": 20, "two_label_values": 1,
           "empty_slice": 1}


def mesh_args(c):
    return c["vertices"], c["triangles"], c["normals"]


@pytest.mark.parametrize("ci", range(len(CASES)))
def test_normals_statement_equals_reference(ci):
    c = CASES[ci]
    for k in range(c["nz"]):
        img, viz = M.slice_normals_numpy(*mesh_args(c), np.int64(c["z0"] + k), c["w"], c["h"], META["exp_factor"], return_viz=True)
        assert img.dtype == np.uint16 and viz.dtype == np.uint8
        assert np.array_equal(img, c["img"][k]), (ci, k)
        assert np.array_equal(viz, c["viz"][k]), (ci, k)


@pytest.mark.parametrize("ci", range(len(CASES)))
def test_labels_statement_equals_reference(ci):
    c = CASES[ci]
    for k in range(c["nz"]):
        lab = M.slice_labels_numpy(c["vertices"], c["triangles"], c["tri_labels"], np.int64(c["z0"] + k), c["w"], c["h"])
        assert lab.dtype == np.uint16 and np.array_equal(lab, c["lab"][k]), (ci, k)


def test_fixture_hits_every_condition():
    assert META["numpy_version"].split(".")[0] == "2"
    assert set(MINIMUM) <= set(META["hits"])
    for name, need in MINIMUM.items():
        assert META["hits"][name] >= need, (name, META["hits"][name])
        assert META["minimum"][name] >= need
    for c in CASES:
        assert c["w"] <= 96 and c["h"] <= 80 and len(c["triangles"]) <= 400 and c["nz"] <= 12
    assert sorted(np.unique(CASES[2]["tri_labels"])) == [1, 2]


@pytest.mark.parametrize("ci", range(len(CASES)))
def test_serial_paint_equals_max_key_then_resolve(ci):
    c = CASES[ci]
    for k in range(c["nz"]):
        z = c["z0"] + k
        keys = M.keys_normals_numpy(*mesh_args(c), z, c["w"], c["h"], META["exp_factor"])
        assert keys.dtype == np.uint64 and np.array_equal(keys != 0, c["img"][k].any(axis=2))
        img, viz = M.resolve_normals_numpy(keys, *mesh_args(c), z, c["w"], c["h"], return_viz=True)
        assert np.array_equal(img, c["img"][k]) and np.array_equal(viz, c["viz"][k])
        lk = M.keys_labels_numpy(c["vertices"], c["triangles"], z, c["w"], c["h"])
        assert lk.dtype == np.uint32 and np.array_equal(M.resolve_labels_numpy(lk, c["tri_labels"]), c["lab"][k])


def test_serial_paint_equals_max_key_on_random_meshes():
    for seed in (0, 1, 2):
        m, img, viz, lab = random_statement(seed)
        for k in range(m["nz"]):
            keys = M.keys_normals_numpy(m["vertices"], m["triangles"], m["normals"], k, m["w"], m["h"])
            assert np.array_equal(M.resolve_normals_numpy(keys, m["vertices"], m["triangles"], m["normals"], k, m["w"], m["h"]), img[k])
            lk = M.keys_labels_numpy(m["vertices"], m["triangles"], k, m["w"], m["h"])
            assert np.array_equal(M.resolve_labels_numpy(lk, m["tri_labels"]), lab[k])


def test_key_fields_round_trip_at_their_limits():
    top = M.KEY_MAX_TRIANGLES - 1
    for tri in (0, 1, 12345, top):
        for pair in (0, 1, 2):
            for step in (0, 1, M.KEY_MAX_STEPS - 1):
                for e in (0, 7, M.KEY_MAX_SAMPLES - 1):
                    k = M.key_pack_normals(tri, pair, step, e)
                    assert 0 < k < 1 << 64 and M.key_unpack_normals(k) == (tri, pair, step, e)
                    assert int(np.uint64(k)) == k
    assert M.key_pack_normals(top, 2, M.KEY_MAX_STEPS - 1, 15) == ((1 << 38) - 2) << 26 | 2 << 24 | ((1 << 20) - 1) << 4 | 15
    # the order of the keys is the order of the paints
    order = [(0, 0, 0, 0), (0, 0, 0, 1), (0, 0, 1, 0), (0, 0, M.KEY_MAX_STEPS - 1, 15), (0, 1, 0, 0), (0, 2, 5, 3), (1, 0, 0, 0), (top, 0, 0, 0)]
    packed = [M.key_pack_normals(*o) for o in order]
    assert packed == sorted(packed) and len(set(packed)) == len(packed)
    for tri in (0, 77, M.LABEL_KEY_MAX_TRIANGLES - 1):
        assert M.key_unpack_label(M.key_pack_label(tri)) == tri and 0 < M.key_pack_label(tri) < 1 << 32


def test_refusals():
    E = M.MeshTargetError
    with pytest.raises(E):
        M.key_pack_normals(0, 0, M.KEY_MAX_STEPS, 0)            # a segment of 2^20 steps or more
    with pytest.raises(E):
        M.key_pack_normals(0, 0, 0, M.KEY_MAX_SAMPLES)          # more than 16 samples
    with pytest.raises(E):
        M.key_pack_normals(M.KEY_MAX_TRIANGLES, 0, 0, 0)        # more than 2^38 - 2 triangles
    with pytest.raises(E):
        M.key_pack_normals(0, 3, 0, 0)
    with pytest.raises(E):
        M.key_pack_label(M.LABEL_KEY_MAX_TRIANGLES)
    with pytest.raises(E):
        M.key_unpack_normals(0)
    c = CASES[1]
    v, t, n = mesh_args(c)
    with pytest.raises(E):
        M.slice_normals_numpy(v, t, n, 1, c["w"], c["h"], exp_factor=3.4)
    with pytest.raises(E):
        M.slice_normals_numpy(v, t, n, 1, c["w"], c["h"], exp_factor=0.01)      # one sample: the reference divides by zero
    bad = v.copy()
    bad[3, 1] = np.nan
    with pytest.raises(E):
        M.slice_normals_numpy(bad, t, n, 1, c["w"], c["h"])
    bad[3, 1] = np.inf
    with pytest.raises(E):
        M.slice_labels_numpy(bad, t, c["tri_labels"], 1, c["w"], c["h"])
    for wrong in (len(v), -1):
        tt = t.copy()
        tt[2, 1] = wrong
        with pytest.raises(E):
            M.slice_normals_numpy(v, tt, n, 1, c["w"], c["h"])
        with pytest.raises(E):
            M.slice_labels_numpy(v, tt, c["tri_labels"], 1, c["w"], c["h"])
    with pytest.raises(E):
        M.slice_normals_numpy(v, t, n[:-1], 1, c["w"], c["h"])
    with pytest.raises(E):
        M.slice_labels_numpy(v, t, c["tri_labels"][:-1], 1, c["w"], c["h"])
    with pytest.raises(E):
        M.keys_normals_numpy(v, t, n, 1, c["w"], c["h"], window=(0, 0, c["h"] + 1, 4))
    with pytest.raises(E):
        M.MeshTargetBuilder([(v, t, n)], (4, c["h"], c["w"]), where="eager")


def test_expansion_sample_counts():
    assert M.expansion_samples(1.5) == (1.5 * 1.2, 8)
    assert M.expansion_samples(3.2)[1] == 16      # the most the key holds: 3.4 gives 17 and is refused (test_refusals)


@pytest.mark.parametrize("ci", (0, 1, 2))
def test_slab_and_window_are_crops(ci):
    c = CASES[ci]
    w, h = c["w"], c["h"]
    for window in ((1, 3, h - 4, w - 7), (h // 2, w // 3, 5, 9), (0, 0, 1, w), (h - 1, 0, 1, 1)):
        y0, x0, wh, ww = window
        for k in (1, c["nz"] // 2):
            z = c["z0"] + k
            keys = M.keys_normals_numpy(*mesh_args(c), z, w, h, META["exp_factor"], window=window)
            assert keys.shape == (wh, ww)
            got = M.resolve_normals_numpy(keys, *mesh_args(c), z, w, h)
            assert np.array_equal(got, c["img"][k][y0:y0 + wh, x0:x0 + ww])
            lk = M.keys_labels_numpy(c["vertices"], c["triangles"], z, w, h, window=window)
            assert np.array_equal(M.resolve_labels_numpy(lk, c["tri_labels"]), c["lab"][k][y0:y0 + wh, x0:x0 + ww])
    vol = M.normals_volume_numpy(*mesh_args(c), w, h, c["z0"] + 2, 3, window=(1, 3, h - 4, w - 7), exp_factor=META["exp_factor"])
    assert np.array_equal(vol, c["img"][2:5, 1:h - 3, 3:w - 4])
    lab = M.labels_volume_numpy(c["vertices"], c["triangles"], c["tri_labels"], w, h, c["z0"] + 2, 3, window=(1, 3, h - 4, w - 7))
    assert np.array_equal(lab, c["lab"][2:5, 1:h - 3, 3:w - 4])


def test_read_obj(tmp_path):
    p = tmp_path / "m.obj"
    p.write_text("# a comment\nmtllib x.mtl\nv 0 0 0\nv 1 0 0 0.5\nvn 0 0 1\nv 1 1 0\nvt 0 0\nv 0 1 0.5\n"
                 "f 1 2 3\nf 1/1 3/2 4/3\nf 1//1 2//1 3//1 4//1\nf -4 -3 -1\nf 1/1/1 2/1/1 3/1/1 4/1/1 1/1/1\n")
    v, t = M.read_obj(p)
    assert v.dtype == np.float32 and t.dtype == np.int64
    assert np.array_equal(v, np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0.5]], np.float32))
    assert t.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 2], [0, 2, 3], [0, 1, 3], [0, 1, 2], [0, 2, 3], [0, 3, 0]]
    for text in ("v 0 0 0\nf 1 2 3\n", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2\n", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 0 1 2\n", "v 0 0\n"):
        p.write_text(text)
        with pytest.raises(M.MeshTargetError):
            M.read_obj(p)
    p.write_text("")
    v, t = M.read_obj(p)
    assert v.shape == (0, 3) and t.shape == (0, 3)


def test_vertex_normals_known():
    # a cube of 12 outward triangles: every vertex normal is its own direction from the centre, (+-1, +-1, +-1) / sqrt(3) ... only when
    # the three faces at a vertex weigh the same, so split every face by BOTH diagonals (4 triangles around a centre vertex)
    corners = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float32)
    faces = [(0, 1, 3, 2, (-1, 0, 0)), (4, 6, 7, 5, (1, 0, 0)), (0, 4, 5, 1, (0, -1, 0)), (2, 3, 7, 6, (0, 1, 0)), (0, 2, 6, 4, (0, 0, -1)),
             (1, 5, 7, 3, (0, 0, 1))]
    verts, tris = list(corners), []
    for a, b, c, d, out in faces:
        m = len(verts)
        verts.append((corners[a] + corners[b] + corners[c] + corners[d]) / 4)
        for p, q in ((a, b), (b, c), (c, d), (d, a)):
            tri = [p, q, m]
            nrm = np.cross(verts[q] - verts[p], verts[m] - verts[p])
            tris.append(tri if np.dot(nrm, out) > 0 else [q, p, m])
    n = M.vertex_normals_numpy(np.asarray(verts, np.float32), np.asarray(tris))
    assert n.dtype == np.float32 and n.shape == (14, 3)
    want = (corners - 0.5) / np.linalg.norm(corners - 0.5, axis=1, keepdims=True)
    assert np.allclose(n[:8], want, atol=2e-7)
    assert np.allclose(n[8:], np.array([f[4] for f in faces], np.float32), atol=2e-7)
    # a flat sheet in the plane z = 2, counter-clockwise seen from +z: every normal is (0, 0, 1) exactly; an unused vertex gets zero
    g = np.array([[x, y, 2] for x in range(4) for y in range(3)] + [[9, 9, 9]], np.float32)
    t = []
    for x in range(3):
        for y in range(2):
            a, b, c, d = x * 3 + y, (x + 1) * 3 + y, (x + 1) * 3 + y + 1, x * 3 + y + 1
            t += [[a, b, c], [a, c, d]]
    n = M.vertex_normals_numpy(g, np.asarray(t))
    assert np.array_equal(n[:-1], np.tile(np.array([0, 0, 1], np.float32), (12, 1))) and np.array_equal(n[-1], np.zeros(3, np.float32))


def test_builder_host_store(tmp_path):
    """where="host": the stores, their attributes and chunking; a slab that does not divide the volume"""
    c = CASES[2]
    half = len(c["vertices"]) // 2
    ta = c["triangles"][c["tri_labels"] == 1]
    tb = c["triangles"][c["tri_labels"] == 2] - half
    meshes = [(c["vertices"][:half], ta, c["normals"][:half]), (c["vertices"][half:], tb, c["normals"][half:])]
    b = M.MeshTargetBuilder(meshes, (5, c["h"], c["w"]), slab=2, min_z=3, where="host", exp_factor=META["exp_factor"])
    assert np.array_equal(b.vertices, c["vertices"]) and np.array_equal(b.triangles, c["triangles"]) and np.array_equal(b.tri_labels, c["tri_labels"])
    arr = zarr_lite.open(b.normals_volume(tmp_path / "n.zarr"))
    assert arr.shape == (5, c["h"], c["w"], 3) and arr.chunks == (128, 128, 128, 3) and arr.dtype == np.uint16
    assert np.array_equal(arr[:], c["img"][3:8])
    attrs = json.load(open(tmp_path / "n.zarr" / ".zattrs"))
    assert attrs["n_channels"] == 3 and attrs["dimensions"] == ["z", "y", "x", "c"] and attrs["min_z"] == 3 and attrs["max_z"] == 7
    assert attrs["chunk_size"] == [128, 128, 128, 3] and json.load(open(tmp_path / "n.zarr" / ".zgroup")) == {"zarr_format": 2}
    lab = zarr_lite.open(b.labels_volume(tmp_path / "l.zarr"))
    assert lab.shape == (5, c["h"], c["w"]) and lab.dtype == np.uint16 and np.array_equal(lab[:], c["lab"][3:8])
    mask = zarr_lite.open(b.sheet_mask(tmp_path / "m.zarr"))
    assert mask.dtype == np.uint8 and np.array_equal(mask[:], c["img"][3:8].any(axis=3).astype(np.uint8) * 255)
    with pytest.raises(FileExistsError):
        b.labels_volume(tmp_path / "l.zarr")
    win = M.MeshTargetBuilder(meshes, (5, c["h"], c["w"]), slab=4, min_z=3, window=(7, 9, 33, 41), where="host", exp_factor=META["exp_factor"])
    assert np.array_equal(zarr_lite.open(win.labels_volume(tmp_path / "lw.zarr"))[:], c["lab"][3:8, 7:40, 9:50])


def test_cli_host(tmp_path):
    """scripts/mesh_to_targets.py end to end on the host path: two OBJ files -> a label store"""
    c = CASES[0]
    for name, shift in (("a.obj", 0.0), ("b.obj", 1.5)):
        with open(tmp_path / name, "w") as f:
            for x, y, z in c["vertices"]:
                f.write(f"v {float(x)!r} {float(y + np.float32(shift))!r} {float(z)!r}\n")
            for t in c["triangles"]:
                f.write("f " + " ".join(str(int(i) + 1) for i in t) + "\n")
    out = tmp_path / "labels.zarr"
    env = dict(os.environ, PYTHONPATH=ROOT)
    subprocess.check_call([sys.executable, os.path.join(ROOT, "scripts", "mesh_to_targets.py"), str(tmp_path / "*.obj"), "--out", str(out), "--shape",
                           "7", str(c["h"]), str(c["w"]), "--labels", "--where", "host"], env=env)
    got = zarr_lite.open(out / "volume")[:]
    va = c["vertices"]
    vb = (va + np.array([0, 1.5, 0], np.float32)).astype(np.float32)
    nt = len(c["triangles"])
    want = M.labels_volume_numpy(np.vstack([va, vb]), np.vstack([c["triangles"], c["triangles"] + len(va)]),
                                 np.concatenate([np.full(nt, 1), np.full(nt, 2)]), c["w"], c["h"], 0, 7)
    assert np.array_equal(got, want) and set(np.unique(got)) == {0, 1, 2}


# ---- the kernels' own functions on the CPU, under AddressSanitizer ---------------------------------------------------------------------
def dump_case(f, m, img, viz, lab, exp_factor):
    v, t, n = m["vertices"], m["triangles"], m["normals"]
    f.write(struct.pack("<6id", len(v), len(t), m["w"], m["h"], m["z0"], m["nz"], exp_factor))
    f.write(np.ascontiguousarray(v, np.float32).tobytes())
    f.write(np.ascontiguousarray(t, np.int32).tobytes())
    f.write(np.ascontiguousarray(n, np.float32).tobytes())
    f.write(np.ascontiguousarray(m["tri_labels"], np.int32).tobytes())
    f.write(np.ascontiguousarray(img, np.uint16).tobytes())
    f.write(np.ascontiguousarray(viz, np.uint8).tobytes())
    f.write(np.ascontiguousarray(lab, np.uint16).tobytes())


def test_host_program_under_sanitizers(tmp_path):
    """csrc/rx_meshslice_core.h is what the kernels call.  A stand-alone C++ program runs it over the golden cases and six random
    meshes, compiled with -fsanitize=address,undefined (and without fp contraction): every code, viz byte and label must equal the
    statement's, by key-then-resolve and by serial paint, and no access may leave the heap buffers."""
    csrc = os.path.join(ROOT, "multi-task-3d-resencoder-unet_amd", "csrc")
    exe = str(tmp_path / "meshslice_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wno-unknown-pragmas", os.path.join(csrc, "tools", "meshslice_host_check.cpp"), "-o", exe])
    dump = str(tmp_path / "cases.bin")
    seeds = range(6)
    with open(dump, "wb") as f:
        f.write(struct.pack("<i", len(CASES) + len(seeds)))
        for c in CASES:
            dump_case(f, c, c["img"], c["viz"], c["lab"], META["exp_factor"])
        for s in seeds:
            m, img, viz, lab = random_statement(s)
            dump_case(f, m, img, viz, lab, 1.5)
    r = subprocess.run([exe, dump], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{len(CASES) + len(seeds)} cases, 0 values differ" in r.stdout
    # the check has teeth: one flipped code in the dump is found
    raw = bytearray(open(dump, "rb").read())
    c = CASES[0]
    off = 4 + 32 + 4 * (3 * len(c["vertices"]) * 2 + 3 * len(c["triangles"]) + len(c["triangles"]))
    k = int(np.flatnonzero(c["img"].reshape(-1))[0])
    raw[off + 2 * k] ^= 1
    open(dump, "wb").write(bytes(raw))
    r = subprocess.run([exe, dump], capture_output=True, text=True)
    assert r.returncode == 1 and "2 values differ" in r.stdout, r.stdout + r.stderr
