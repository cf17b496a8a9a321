"""Regenerate tests/golden/geometry.npz: what the REFERENCE's own RandomFlipWithNormals / RandomRotate90WithNormals
(training/transforms/geometric/geometry.py) do to small patches, pinning dataloading/geometry_device.py, the host classes and,
through `apply_op_numpy`, the device kernel.

    RX_REFERENCE_ROOT=<reference checkout> python scripts/make_geometry_fixture.py

Every case is `random.seed(seed)` followed by a chain of the real classes on {"image": (Z, Y, X), "sheet": (1, Z, Y, X),
"normals": (3, Z, Y, X)}.  Recorded per case: the seed, the chain (class names and arguments, JSON), the three arrays that came
out, and the op (src_axis, flip, ch_src, ch_neg -- the record of `rx_geom_sample`) READ BACK from a second run of the same seed
on an index volume and a constant-component normals array, so the recorded op owes nothing to this project's code.  Inputs are
stored once per shape.  All values are multiples of 1/8 in [-1, 1] (about half of the normals voxels exactly zero), which float16
holds exactly, sign of zero included: the outputs are stored as float16 to keep the file small and compare bit for bit after
the cast back to float32.

Cases: (a) every flip mask x {no rotation, each (axis, k)} = 80 chains flip -> rot90 on 6^3, the seed of each found by search;
(b) 40 chains flip -> rot90 -> rot90 whose second rotation is about another axis (one rotation only swaps two axes; the cyclic
axis permutations need two), chosen so that (a) and (b) together reach all 48 signed axis permutations; (c) 6 chains on (4, 6, 6)
rotated about z only; (d) 12 seeded draws with every probability below 1.  Needs the reference tree at generation time only."""
import importlib.util
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "geometry.npz")
CUBE, FLAT = (6, 6, 6), (4, 6, 6)


def inputs(shape, seed):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 9, size=shape).astype(np.float32) / 8
    sheet = (rng.integers(0, 9, size=(1, *shape)).astype(np.float32) / 8)
    nrm = rng.integers(-8, 9, size=(3, *shape)).astype(np.float32) / 8
    nrm *= (rng.random(shape) < 0.5).astype(np.float32)[None]
    nrm[nrm == 0] = 0.0          # masked-out voxels: +0.0, as a real target's
    return {"image": img, "sheet": sheet, "normals": nrm}


def build(ref, chain):
    cls = {"flip": ref.RandomFlipWithNormals, "rot90": ref.RandomRotate90WithNormals}
    return [cls[name](**{k: (tuple(v) if k == "axes" else v) for k, v in kw.items()}) for name, kw in chain]


def run(ref, chain, seed, data):
    random.seed(seed)
    d = {k: v.copy() for k, v in data.items()}
    for t in build(ref, chain):
        d = t(d)
    return d


def read_back_op(ref, chain, seed, shape):
    """the op of (chain, seed), from what the real classes do to an index volume and to constant components (1, 2, 3)"""
    idx = np.arange(int(np.prod(shape)), dtype=np.float64).reshape(shape)
    comp = np.broadcast_to(np.array([1.0, 2.0, 3.0])[:, None, None, None], (3, *shape)).copy()
    out = run(ref, chain, seed, {"vol": idx, "normals": comp})
    vol = out["vol"]
    assert vol.shape == tuple(shape), "the chain changed the shape"
    src, flip = [], []
    at0 = np.array(np.unravel_index(int(vol[0, 0, 0]), shape))
    for d in range(3):
        o = [0, 0, 0]
        o[d] = shape[d] - 1
        end = np.array(np.unravel_index(int(vol[tuple(o)]), shape))
        moved = np.nonzero(end != at0)[0]
        assert len(moved) == 1
        a = int(moved[0])
        src.append(a)
        flip.append(int(at0[a] == shape[a] - 1))
    n = out["normals"][:, 0, 0, 0]
    ch_src = [int(abs(v)) - 1 for v in n]
    ch_neg = [int(v < 0) for v in n]
    return src + flip + ch_src + ch_neg


def main():
    ref_root = os.environ.get("RX_REFERENCE_ROOT")
    if not ref_root:
        sys.exit("set RX_REFERENCE_ROOT to the reference checkout")
    sys.dont_write_bytecode = True
    spec = importlib.util.spec_from_file_location(
        "ref_geometry", os.path.join(ref_root, "training", "transforms", "geometric", "geometry.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    def drawn(chain, seed):
        """what the real classes drew: (flip mask, [(axis, k) | None per rot90 of the chain]) -- by watching `random`"""
        random.seed(seed)
        mask, rots = 0, []
        for name, kw in chain:
            if name == "flip":
                if random.random() < kw.get("p_transform", 1.0):
                    for bit in range(3):
                        if random.random() < kw.get("p", 0.5):
                            mask |= 1 << bit
            else:
                if random.random() >= kw.get("p_transform", 1.0) or random.random() >= kw.get("p", 0.5):
                    rots.append(None)
                else:
                    axis = random.choice(tuple(kw.get("axes", ("x", "y", "z"))))
                    rots.append((axis, random.choice([1, 2, 3])))
        return mask, rots

    cases = []      # (shape, chain, seed)
    # (a) 8 flip masks x (no rotation + 9 rotations)
    chain_a = [("flip", {"p": 0.5, "p_transform": 1.0}), ("rot90", {"axes": ["x", "y", "z"], "p": 0.5, "p_transform": 1.0})]
    want = {(m, r) for m in range(8) for r in [None] + [(a, k) for a in "xyz" for k in (1, 2, 3)]}
    found = {}
    seed = 0
    while len(found) < len(want):
        mask, rots = drawn(chain_a, seed)
        found.setdefault((mask, rots[0]), seed)
        seed += 1
    for key in sorted(found, key=lambda t: (t[0], t[1] is not None, t[1] or ("", 0))):
        cases.append((CUBE, chain_a, found[key]))
    ops_a = {tuple(read_back_op(ref, ch, s, sh)[:6]) for sh, ch, s in cases}
    # (b) a second rotation about another axis: first whatever reaches a new axis op, then new (mask, rot, rot) draws up to 40
    chain_b = chain_a + [("rot90", {"axes": ["x", "y", "z"], "p": 1.0, "p_transform": 1.0})]
    reached, picked, used = set(ops_a), [], set()
    seed = 0
    while len(picked) < 40:
        mask, rots = drawn(chain_b, seed)
        if rots[0] is not None and rots[1][0] != rots[0][0] and (mask, rots[0]) not in used:
            axis_op = tuple(read_back_op(ref, chain_b, seed, CUBE)[:6])
            if axis_op not in reached or len(reached) == 48:
                reached.add(axis_op)
                used.add((mask, rots[0]))
                picked.append(seed)
        seed += 1
        assert seed < 200000
    cases += [(CUBE, chain_b, s) for s in picked]
    # (c) a non-cubic patch, rotated about z only
    chain_c = [("flip", {"p": 0.5, "p_transform": 1.0}), ("rot90", {"axes": ["z"], "p": 1.0, "p_transform": 1.0})]
    cases += [(FLAT, chain_c, s) for s in range(6)]
    # (d) every probability below 1
    chain_d = [("flip", {"p": 0.5, "p_transform": 0.7}), ("rot90", {"axes": ["x", "y", "z"], "p": 0.5, "p_transform": 0.8})]
    cases += [(CUBE, chain_d, 1000 + s) for s in range(12)]

    data = {CUBE: inputs(CUBE, 11), FLAT: inputs(FLAT, 12)}
    arrays = {}
    for shape, d in data.items():
        for k, v in d.items():
            arrays[f"in_{'x'.join(map(str, shape))}_{k}"] = v
    ops, seeds, shapes, chains = [], [], [], []
    for i, (shape, chain, s) in enumerate(cases):
        out = run(ref, chain, s, data[shape])
        for k, v in out.items():
            assert v.dtype == np.float32 and v.shape == data[shape][k].shape
            h = v.astype(np.float16)
            assert np.array_equal(h.astype(np.float32).view(np.int32), np.ascontiguousarray(v).view(np.int32))
            arrays[f"c{i:03d}_{k}"] = h
        ops.append(read_back_op(ref, chain, s, shape))
        seeds.append(s)
        shapes.append(shape)
        chains.append(json.dumps(chain))
    arrays["ops"] = np.array(ops, np.int32)
    arrays["seeds"] = np.array(seeds, np.int64)
    arrays["shapes"] = np.array(shapes, np.int32)
    arrays["chains"] = np.array(chains)
    n_a = len({tuple(o[:6]) for o in ops[:80]})
    n_all = len({tuple(o[:6]) for o in ops})
    print(f"{len(cases)} cases; distinct signed axis permutations: {n_a} from flip + one rotation, {n_all} with the two-rotation cases")
    assert n_a == 32 and n_all == 48
    assert any(np.signbit(arrays[k]).any() and (arrays[k][np.signbit(arrays[k])] == 0).any() for k in arrays if k.endswith("_normals") and k[0] == "c")
    np.savez_compressed(OUT, **arrays)
    size = os.path.getsize(OUT)
    print(OUT, size, "bytes")
    assert size < 256 * 1024


if __name__ == "__main__":
    main()
