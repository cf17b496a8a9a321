"""What the mesh stages after the mesher (refine.py, decimate.py, orient.py) have in common: the preamble of their config blocks and
the skeleton of their drivers.  A stage reads the mesh file the stage before it wrote and writes `<stem>_<suffix>.<ext>` next to it."""
import os

from .mesh_io import FORMATS, _check_mesh, read_mesh, write_refined


def parse_stage_block(key, m, mesh_tasks, defaults, required=()):
    """the block `key` of inference_config.postprocess -> {tasks, every key of `required` and of `defaults`, max_device_gb}, the
    stage's own values as given and still to be checked.  Checked here: `m` is a mapping of known keys; `tasks` is a name or a list
    of names, each one of `mesh_tasks`, the tasks the `mesh` block of the same config writes a mesh of (None: no such block);
    `required` ({key: what it is}) are present; `max_device_gb` is a positive number or None.  Refusals are ValueErrors naming the key."""
    required = dict(required)
    if not isinstance(m, dict):
        raise ValueError(f"{key}: expected a mapping, got {m!r}")
    known = ("tasks",) + tuple(required) + tuple(defaults) + ("max_device_gb",)
    for k in m:
        if k not in known:
            raise ValueError(f"{key}.{k}: unknown key ({', '.join(known)})")
    tasks = m.get("tasks")
    if isinstance(tasks, str):
        tasks = [tasks]
    if not isinstance(tasks, (list, tuple)) or not tasks:
        raise ValueError(f"{key}.tasks: {tasks!r} (a list of task names)")
    for t in tasks:
        if mesh_tasks is None or t not in mesh_tasks:
            raise ValueError(f"{key}.tasks: task {t!r} is not listed under inference_config.postprocess.mesh, so no mesh of it is written")
    for k, what in required.items():
        if k not in m:
            raise ValueError(f"{key}.{k}: missing ({what})")
    gb = m.get("max_device_gb")
    if gb is not None and (isinstance(gb, bool) or not isinstance(gb, (int, float)) or not gb > 0):
        raise ValueError(f"{key}.max_device_gb: {gb!r} (a positive number)")
    return dict({k: m.get(k, d) for k, d in defaults.items()}, **{k: m[k] for k in required}, tasks=tuple(tasks),
                max_device_gb=None if gb is None else float(gb))


class MeshStage:
    """The driver of one stage: `run(path, out=None)` reads an OBJ or a PLY mesh as mesh_io writes them (normals in the file are not
    used), hands the checked arrays to the subclass's `_work(vertices, triangles, **kwargs) -> (vertices, triangles, normals or
    None, summary)`, writes `<stem>_<suffix>.<ext>` next to the input (or `out`) under `<name>.partial`, renamed at the end, and
    returns the summary.  An existing output file is refused before any work.  `fmt`: "obj" or "ply"; None keeps the input's.
    `max_device_bytes`: the stage's device budget, None for half of the free device memory."""
    suffix = None

    def __init__(self, fmt, max_device_bytes):
        who = type(self).__name__
        if fmt is not None and fmt not in FORMATS:
            raise ValueError(f"{who}: fmt {fmt!r} (one of {', '.join(FORMATS)}, or None for the input's)")
        if max_device_bytes is not None and int(max_device_bytes) < 1:
            raise ValueError(f"{who}: max_device_bytes {max_device_bytes}")
        self.fmt, self.max_device_bytes = fmt, None if max_device_bytes is None else int(max_device_bytes)

    def _budget(self, need, what):
        """refuses a resident run of `what` that needs more than the budget"""
        budget = self.max_device_bytes
        if budget is None:
            import torch
            budget = torch.cuda.mem_get_info()[0] // 2
        if need > budget:
            raise MemoryError(f"{type(self).__name__}: {what} needs {need} bytes on the device, the budget is {budget} (the whole mesh is "
                              f"resident; there is no out-of-core path)")

    def run(self, path, out=None, **kwargs):
        path = str(path)
        vertices, triangles, _ = read_mesh(path)
        stem, ext = os.path.splitext(path)
        fmt = self.fmt or ext[1:].lower()
        out = f"{stem}_{self.suffix}.{fmt}" if out is None else str(out)
        if os.path.exists(out):
            raise FileExistsError(f"{out} already exists")
        vertices, triangles = _check_mesh(type(self).__name__, vertices, triangles)
        v, t, n, summary = self._work(vertices, triangles, **kwargs)
        write_refined(out, fmt, v, t, n)
        return summary
