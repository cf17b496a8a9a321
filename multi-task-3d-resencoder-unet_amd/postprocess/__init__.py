"""Post-processing of a prediction store: connected-component filtering of `<task>_final` (components.py: the numpy statements, the
host half of the out-of-core run, the config block and the `ComponentFilter` driver; the kernels are csrc/rx_components.hip),
the triangle mesh of `<task>_filtered` or `<task>_final` by surface nets (isosurface.py: the numpy statement, the OBJ / PLY writers
and the `SurfaceMesher` driver; the kernels are csrc/rx_isosurface.hip) and the refinement of that mesh by Taubin smoothing and
vertex normals (refine.py: the numpy statements, the readers and writers with normals and the `MeshRefiner` driver; the kernels are
csrc/rx_meshrefine.hip) and its decimation by vertex clustering (decimate.py: the numpy statement, the config block and the
`MeshDecimator` driver; the kernels are csrc/rx_meshdecimate.hip) and its orientation against the predicted normal field (orient.py: the
numpy statements of sampling, the per-triangle cosine, the front / back / rim classification and the selection of one face, the
config block and the `MeshOrienter` driver; the kernels are csrc/rx_meshsample.hip)."""
from .components import (ComponentFilter, component_sizes_numpy, filter_numpy, label_numpy, label_values_numpy,      # noqa: F401
                         merge_slabs, parse_config)
from .isosurface import SurfaceMesher, counts_numpy, surface_nets_numpy, write_obj, write_ply      # noqa: F401
from .refine import (MeshRefiner, adjacency_numpy, parse_refine_config, read_mesh, read_ply, refine_numpy, smooth_numpy,      # noqa: F401
                     vertex_normals_numpy, write_refined)
from .decimate import MeshDecimator, cluster_rows, decimate_numpy, parse_decimate_config      # noqa: F401
from .orient import (MeshOrienter, decode_numpy, face_cos_numpy, parse_orient_config, sample_points_numpy, select_numpy,      # noqa: F401
                     side_numpy, slab_ranges, unit_numpy)
