"""Thin Python wrappers over the C ABI (one function per entry point of include/rxunet.h), split by subject: core (Act, workspace,
events and programs, the profiler and its accounting, the argument checks, codes), network, losses, pipeline, infer, validation,
mesh, postprocess.  Nothing here computes on the host or with torch ops: every function enqueues HIP kernels on torch's current stream.

Every wrapper is reached as `ops.NAME`, looked up at call time, so a replaced `ops.NAME` (a test's spy, a tracer) is what callers
get.  A subject module imports from core only.  The profiler is read with `ops.profiling()`, never as a variable."""
from ctypes import byref, c_int32, c_void_p      # noqa: F401 -- these and the lib names below: callers reach them as ops.NAME

import numpy as np      # noqa: F401
import torch      # noqa: F401

from .. import lib as _l      # noqa: F401
from ..lib import I3, RxAct, check, load, stream_ptr      # noqa: F401
from . import core, infer, losses, mesh, network, pipeline, postprocess, validation      # noqa: F401
from .core import (_U16, Act, LaunchProfiler, Program, event_free, event_new, event_record, profiling,      # noqa: F401
                   set_profiler, stream_wait, timed_bytes, workspace)
from .infer import (SW_ACT, SW_BLEND, SW_CAST, SW_NORM, sw_accumulate, sw_finalize, sw_gather,      # noqa: F401
                    sw_gather_workspace, sw_occupancy)
from .losses import (bce_dice_loss_bwd, bce_dice_loss_fwd, cross_entropy_loss_bwd, cross_entropy_loss_fwd,      # noqa: F401
                     elem_loss_bwd, elem_loss_fwd, masked_cosine_loss_bwd, masked_cosine_loss_fwd)
from .mesh import (MeshAdjacency, mesh_adjacency, mesh_decimate, mesh_face_cos, mesh_sample, mesh_select,      # noqa: F401
                   mesh_slice_labels, mesh_slice_normals, mesh_smooth, mesh_vertex_normals)
from .network import (avgpool_bwd, avgpool_fwd, channel_sum, conv3d_bwd_data, conv3d_bwd_data_instats,      # noqa: F401
                      conv3d_bwd_weight, conv3d_fwd, conv3d_fwd_stats, convT3d_bwd_data, convT3d_bwd_weight, convT3d_fwd,
                      head_bwd, head_fwd, instnorm_act_bwd, instnorm_act_bwd_apply, instnorm_act_bwd_head,
                      instnorm_act_bwd_res, instnorm_act_fwd, instnorm_act_head_fwd, instnorm_act_pool_fwd, instnorm_fwd,
                      instnorm_gate_act_bwd, instnorm_gate_act_fwd, instnorm_stats, instnorm_stats_mask, pack_conv_weight,
                      pack_convT_weight, pack_weights_multi, se_gate_bwd, se_gate_fwd, se_workspace_bytes,
                      stem_conv_bwd_weight, stem_conv_fwd, stem_conv_fwd_stats)
from .pipeline import (affine_apply, affine_table, aug_filter_zy, aug_philox_u32, aug_pointwise, augment_batch,      # noqa: F401
                       box_stats, elastic_apply, elastic_nodes, elastic_tables, geom_apply, geom_table, ingest, label_dilate)
from .postprocess import cc_filter, cc_label, cc_sizes, iso_counts, iso_mesh      # noqa: F401
from .validation import (class_counts, edt_sq, mask_edges, normal_stats, preview_frames, preview_panel, seg_counts,      # noqa: F401
                         surface_hist, surface_scratch)
