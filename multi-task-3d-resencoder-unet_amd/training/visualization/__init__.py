from .preview import (DEFAULTS, frames_numpy, minmax_numpy, panel_numpy, parse_config, sigmoid_tasks_of, write_gif)

__all__ = ["DEFAULTS", "frames_numpy", "minmax_numpy", "panel_numpy", "parse_config", "sigmoid_tasks_of", "write_gif"]
