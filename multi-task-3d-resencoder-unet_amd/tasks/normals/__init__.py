"""Mesh -> normals / label / sheet-mask volumes (mesh_targets.py)."""
from .mesh_targets import MeshTargetBuilder, read_obj, vertex_normals_numpy  # noqa: F401
