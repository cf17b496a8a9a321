from .metrics import (KINDS, MAX_CLASSES, RATES, ValidationMetrics, argmax_numpy, class_counts_numpy, infer_kind, metric_names,
                      normal_mask_numpy, normal_stats_numpy, parse_config, pred_threshold, scores_from_counts, seg_counts_numpy)
from .surface import EDT_NONE, default_bins, edges_numpy, edt_sq_numpy, parse_surface, surface_hist_numpy, surface_scores

__all__ = ["EDT_NONE", "KINDS", "MAX_CLASSES", "RATES", "ValidationMetrics", "argmax_numpy", "class_counts_numpy", "default_bins",
           "edges_numpy", "edt_sq_numpy", "infer_kind", "metric_names", "normal_mask_numpy", "normal_stats_numpy", "parse_config",
           "parse_surface", "pred_threshold", "scores_from_counts", "seg_counts_numpy", "surface_hist_numpy", "surface_scores"]
