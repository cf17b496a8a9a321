"""Post-processing of a prediction store.  Connected-component filtering of `<task>_final` (components.py: the numpy statements, the
host half of the out-of-core run, the config block and the `ComponentFilter` driver; the kernels are csrc/rx_components.hip).  The
triangle mesh of `<task>_filtered` or `<task>_final` by surface nets (isosurface.py: the numpy statement, the config block and the
`SurfaceMesher` driver; csrc/rx_isosurface.hip).  Then the mesh stages, each a module with its numpy statements, its config block
and its driver, each reading the file the stage before it wrote: refinement by Taubin smoothing and vertex normals (refine.py,
`MeshRefiner`; csrc/rx_meshrefine.hip), decimation by vertex clustering (decimate.py, `MeshDecimator`; csrc/rx_meshdecimate.hip)
and orientation against the predicted normal field (orient.py, `MeshOrienter`; csrc/rx_meshsample.hip).  What the stages share:
mesh_io.py (the mesh as a file and as arrays: checks, OBJ / PLY writers and readers, with or without normals) and stage.py (the
preamble of a stage's config block, `parse_stage_block`, and the skeleton of its driver, `MeshStage`)."""
from .components import (ComponentFilter, component_sizes_numpy, filter_numpy, label_numpy, label_values_numpy,      # noqa: F401
                         merge_slabs, parse_config)
from .isosurface import SurfaceMesher, counts_numpy, surface_nets_numpy      # noqa: F401
from .mesh_io import read_mesh, read_ply, write_obj, write_ply, write_refined      # noqa: F401
from .refine import (MeshRefiner, adjacency_numpy, parse_refine_config, refine_numpy, smooth_numpy,      # noqa: F401
                     vertex_normals_numpy)
from .decimate import MeshDecimator, cluster_rows, decimate_numpy, parse_decimate_config      # noqa: F401
from .orient import (MeshOrienter, decode_numpy, face_cos_numpy, parse_orient_config, sample_points_numpy, select_numpy,      # noqa: F401
                     side_numpy, slab_ranges, unit_numpy)
