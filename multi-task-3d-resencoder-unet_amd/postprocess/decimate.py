"""Decimation of a triangle mesh by vertex clustering on a uniform grid (Rossignac-Borrel): the numpy statement of
csrc/rx_meshdecimate.hip, the config block and the `MeshDecimator` driver.

Surface nets emit one vertex per crossing cell at voxel resolution, so the mesh of a real volume is far larger than any viewer or
flattening tool wants.  Clustering puts a grid of `cell`-sized cubes over the mesh, replaces all vertices of a cube by one
representative and drops the triangles that collapse.  It is linear in the mesh, parallel per vertex and per triangle, and its
result is a property of the mesh alone: every number below is derived from cell keys and smallest member ids, every float32
operation is one rounding in the order written here, and the kernels reproduce that -- results compare with array_equal, floats by
their bits.  The statement uses numpy only."""
import numpy as np

from .mesh_io import F32, _check_mesh, gather_sum
from .refine import vertex_normals_numpy
from .stage import MeshStage, parse_stage_block

KEY = "inference_config.postprocess.decimate"
REPRESENTATIVES = ("mean", "nearest")
KEY_RANGE = 2**20      # a cell index k has |k| < 2^20 per component: three of them plus the offset fill 63 bits
# device memory of a resident run, MeshDecimator.scratch_bytes.  Per vertex: its position (12), cell key (8), table slot (4), the
# flag "smallest of its cluster" (4), the scan of those flags (8), cluster_of (8), the hash table -- the smallest power of two that
# is at least 2 V + 2 slots, so fewer than 4 V + 4, of an 8-byte key and a 4-byte smallest id (48) --; per cluster, of which there
# are at most V: the member counts, their scan and the member list (4 + 8 + 4; `nearest` has its 8-byte packed minimum instead), the
# representative (12), the counts of attached triangles and their scan (4 + 8), the referenced flag and its scan (4 + 8), the output
# position (12).  Per triangle: its ids (24), its (middle, largest, index) entry (12), the keep flag and its scan (4 + 8), the
# output ids (24).
BYTES_PER_VERTEX = 156
BYTES_PER_TRIANGLE = 72
BYTES_FIXED = 96      # four more table slots (48), the last word of the five scans (40), the flag (4), padded


def scratch_bytes(n_vertices, n_triangles):
    """device bytes of a resident decimation of a mesh of `n_vertices` vertices and `n_triangles` triangles, inputs and outputs included"""
    return BYTES_PER_VERTEX * int(n_vertices) + BYTES_PER_TRIANGLE * int(n_triangles) + BYTES_FIXED


def _cell(name, cell):
    """`cell` as a float32: finite and greater than 0 after the rounding"""
    if isinstance(cell, bool) or not isinstance(cell, (int, float, np.integer, np.floating)):
        raise ValueError(f"{name} {cell!r} (a finite number > 0)")
    with np.errstate(over="ignore"):
        c = F32(cell)
    if not (np.isfinite(c) and c > 0):
        raise ValueError(f"{name} {cell!r} (a finite float32 > 0)")
    return c


def _representative(name, representative):
    if representative not in REPRESENTATIVES:
        raise ValueError(f"{name} {representative!r} (one of {', '.join(REPRESENTATIVES)})")
    return representative


# ---- the statement ----------------------------------------------------------------------------------------------------------------------------
def cell_keys_numpy(vertices, cell):
    """-> (k int64 (V, 3), key int64 (V,)): per component q = p / float32(cell) is one float32 division and k = floor(q); the key is
    ((k0 + 2^20) << 42) | ((k1 + 2^20) << 21) | (k2 + 2^20).  A mesh with some |k| >= 2^20 is refused."""
    p = np.ascontiguousarray(vertices, F32)
    c = _cell("cell_keys_numpy: cell", cell)
    with np.errstate(over="ignore"):
        f = np.floor(p / c)
    if len(f) and not (np.abs(f) < KEY_RANGE).all():      # an infinity included
        raise ValueError(f"decimate: cell {float(c)!r} puts a vertex in a grid cell with an index of 2^20 or more; choose a larger cell")
    k = f.astype(np.int64)
    return k, ((k[:, 0] + KEY_RANGE) << 42) | ((k[:, 1] + KEY_RANGE) << 21) | (k[:, 2] + KEY_RANGE)


def cluster_rows(cluster_of, triangles):
    """-> int64 (C,): the row of each cluster in the output vertices of `decimate_numpy`, -1 for a cluster that was not kept.  A
    cluster is kept exactly when some input triangle has it at a corner and three different clusters at its corners; the kept ones
    are in ascending cluster number."""
    cluster_of = np.asarray(cluster_of, np.int64)
    ct = cluster_of[np.asarray(triangles, np.int64).reshape(-1, 3)]
    live = ct[(ct[:, 0] != ct[:, 1]) & (ct[:, 1] != ct[:, 2]) & (ct[:, 0] != ct[:, 2])]
    rows = np.full(int(cluster_of.max()) + 1 if len(cluster_of) else 0, -1, np.int64)
    used = np.unique(live)
    rows[used] = np.arange(len(used))
    return rows


def decimate_numpy(vertices, triangles, cell, representative="mean"):
    """vertex clustering -> (vertices float32 (V', 3), triangles int64 (T', 3), cluster_of int64 (V,)).

    Cells: see `cell_keys_numpy`.  Clusters: the vertices with equal keys, referenced by a triangle or not, numbered 0 .. C - 1 by
    ascending smallest member id; cluster_of[v] is that number.  Representative of a cluster of n members, per component, one
    rounding per float32 operation: "mean": s = the sequential sum, from 0, of the members' positions in ascending vertex id, and the
    representative is s / float32(n); "nearest": the member with the smallest d = dx*dx + dy*dy + dz*dz (three products summed left to
    right, no fused multiply-add), where dx = p - centre and centre = (float32(k) + 0.5f) * cell as two operations; ties go to the
    lowest vertex id; the output is that member's bits.

    Triangles: each corner id is replaced by its cluster; a triangle with two equal cluster ids is dropped; among triangles with the
    same unordered cluster triple the one with the lowest input index is kept, with its own corner order and so its winding; kept
    triangles stay in ascending input index.  The output vertices are the representatives of the clusters some kept triangle names,
    in ascending cluster number, and the triangles are renumbered to match.  `cluster_of` keeps the numbers from before that
    compaction: `cluster_rows(cluster_of, triangles)[c]` is the output row of cluster c, or -1 if it was not kept.

    What the result does not promise: clustering can create non-manifold edges and vertices; it can merge the two faces of a sheet
    thinner than `cell`, after which the duplicate rule keeps one face (and one winding); it does not pin boundaries, which move
    with their clusters; it minimises no error measure."""
    p, t = _check_mesh("decimate_numpy", vertices, triangles)
    c = _cell("decimate_numpy: cell", cell)
    _representative("decimate_numpy: representative", representative)
    V = len(p)
    if V == 0:
        return np.zeros((0, 3), F32), np.zeros((0, 3), np.int64), np.zeros(0, np.int64)
    k, key = cell_keys_numpy(p, c)
    _, first, inverse = np.unique(key, return_index=True, return_inverse=True)      # first: the smallest member id of each key
    number = np.empty(len(first), np.int64)
    number[np.argsort(first)] = np.arange(len(first))
    cluster_of = number[inverse.reshape(-1)]
    C = len(first)
    members = np.argsort(cluster_of, kind="stable")      # by cluster, ascending id within one
    n = np.bincount(cluster_of, minlength=C)
    offsets = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    if representative == "mean":
        rep = (gather_sum(p, offsets, members, np.arange(C)) / n.astype(F32)[:, None]).astype(F32)
    else:
        with np.errstate(over="ignore"):
            centre = (k.astype(F32) + F32(0.5)) * c
            dx = p - centre
            d = dx[:, 0] * dx[:, 0] + dx[:, 1] * dx[:, 1] + dx[:, 2] * dx[:, 2]
        packed = (d.astype(F32).view(np.int32).astype(np.int64) << 32) | np.arange(V, dtype=np.int64)      # d >= 0: its bits order as integers
        rep = p[np.minimum.reduceat(packed[members], offsets[:-1]) & 0xFFFFFFFF]
    ct = cluster_of[t]
    live = np.nonzero((ct[:, 0] != ct[:, 1]) & (ct[:, 1] != ct[:, 2]) & (ct[:, 0] != ct[:, 2]))[0]
    if len(live):
        _, lowest = np.unique(np.sort(ct[live], axis=1), axis=0, return_index=True)      # the first, so the lowest, index of each triple
        kept = ct[live[np.sort(lowest)]]
    else:
        kept = np.zeros((0, 3), np.int64)
    used = np.unique(kept)
    rows = np.full(C, -1, np.int64)
    rows[used] = np.arange(len(used))
    return np.ascontiguousarray(rep[used], F32).reshape(-1, 3), rows[kept].reshape(-1, 3), cluster_of


# ---- the config block -------------------------------------------------------------------------------------------------------------------------
_DEFAULTS = {"representative": "mean", "normals": True}


def parse_decimate_config(m, mesh_tasks):
    """`inference_config.postprocess.decimate` -> {tasks, cell, representative, normals, max_device_gb}.  Unknown keys and bad values
    raise ValueError naming the key; `mesh_tasks`: the tasks the `mesh` block of the same config writes a mesh of (None: no such
    block) -- every task decimated must be one of them.  `cell` has no default: it is in the mesh's units (voxels)."""
    o = parse_stage_block(KEY, m, mesh_tasks, _DEFAULTS, required={"cell": "the edge of a grid cell, in voxels"})
    cell = float(_cell(f"{KEY}.cell:", o["cell"]))
    _representative(f"{KEY}.representative:", o["representative"])
    if not isinstance(o["normals"], bool):
        raise ValueError(f"{KEY}.normals: {o['normals']!r} (true or false)")
    return dict(o, cell=cell)


# ---- the driver -------------------------------------------------------------------------------------------------------------------------------
class MeshDecimator(MeshStage):
    """The stage (stage.py: MeshStage) that decimates a mesh (`decimate_numpy` is the statement), takes the normals of the decimated
    mesh (`vertex_normals_numpy`) and writes `<stem>_decimated.<ext>`.  `normals=False` writes positions only.

    The whole mesh is resident on the device: `scratch_bytes(V, T)` = 156 V + 72 T + 96 bytes (BYTES_PER_VERTEX, BYTES_PER_TRIANGLE,
    inputs and outputs included), and a mesh that needs more than `max_device_bytes` (default: half of the free device memory) raises
    MemoryError.  There is no out-of-core path.  `decimator`: None runs the HIP kernels; a callable
    (vertices, triangles, cell, representative) -> (vertices, triangles, cluster_of), such as `decimate_numpy`, replaces them and
    the normals are then taken on the host, which is how the driver runs there."""
    suffix = "decimated"

    def __init__(self, cell, representative="mean", normals=True, fmt=None, max_device_bytes=None, decimator=None):
        self.cell = float(_cell("MeshDecimator: cell", cell))
        self.representative = _representative("MeshDecimator: representative", representative)
        super().__init__(fmt, max_device_bytes)
        self.normals, self.decimator = bool(normals), decimator

    scratch_bytes = staticmethod(scratch_bytes)

    def decimate(self, vertices, triangles):
        """host arrays -> (vertices, triangles, cluster_of, normals or None)"""
        if self.decimator is not None:
            v, t, cluster_of = self.decimator(vertices, triangles, self.cell, self.representative)
            return v, t, cluster_of, vertex_normals_numpy(v, t) if self.normals else None
        import torch
        from ..engine import ops
        self._budget(scratch_bytes(len(vertices), len(triangles)), f"a mesh of {len(vertices)} vertices and {len(triangles)} triangles")
        v, t, cluster_of = ops.mesh_decimate(torch.from_numpy(vertices).cuda(), torch.from_numpy(triangles).cuda(), self.cell, self.representative)
        n = ops.mesh_vertex_normals(v, t) if self.normals else None
        return v.cpu().numpy(), t.cpu().numpy(), cluster_of.cpu().numpy(), None if n is None else n.cpu().numpy()

    def _work(self, vertices, triangles):
        v, t, cluster_of, n = self.decimate(vertices, triangles)
        # the largest float32 |representative - p| over the components of the input vertices whose cluster is in the output
        rows = cluster_rows(cluster_of, triangles)[cluster_of] if len(cluster_of) else np.zeros(0, np.int64)
        moved = float(np.abs(v[rows[rows >= 0]] - vertices[rows >= 0]).max()) if (rows >= 0).any() else 0.0
        return v, t, n, dict(vertices=len(v), triangles=len(t), input_vertices=len(vertices), input_triangles=len(triangles),
                             clusters=int(cluster_of.max()) + 1 if len(cluster_of) else 0, cell=self.cell, max_displacement=moved)
