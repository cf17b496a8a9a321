"""Post-processing of a prediction store: connected-component filtering of `<task>_final` (components.py: the numpy statements, the
host half of the out-of-core run, the config block and the `ComponentFilter` driver; the kernels are csrc/rx_components.hip)."""
from .components import (ComponentFilter, component_sizes_numpy, filter_numpy, label_numpy, label_values_numpy,      # noqa: F401
                         merge_slabs, parse_config)
