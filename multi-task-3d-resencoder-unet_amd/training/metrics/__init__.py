from .metrics import (KINDS, MAX_CLASSES, RATES, ValidationMetrics, argmax_numpy, class_counts_numpy, infer_kind, metric_names,
                      normal_mask_numpy, normal_stats_numpy, parse_config, pred_threshold, scores_from_counts, seg_counts_numpy)

__all__ = ["KINDS", "MAX_CLASSES", "RATES", "ValidationMetrics", "argmax_numpy", "class_counts_numpy", "infer_kind", "metric_names",
           "normal_mask_numpy", "normal_stats_numpy", "parse_config", "pred_threshold", "scores_from_counts", "seg_counts_numpy"]
