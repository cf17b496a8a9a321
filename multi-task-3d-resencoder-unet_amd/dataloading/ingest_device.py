"""Ingest -- what the reference's `__getitem__` (dataloading/dataset.py) does to every array between the store and the first
transform: `astype(np.float32)`, the dtype scaling, and for a channels-last normals store `transpose(3, 0, 1, 2)` -- stated once
in numpy and run on the device (csrc/rx_ingest.hip: rx_ingest), so that the item, the pinned batch and the host-to-device copy
hold what the store holds: 1 or 2 bytes per voxel instead of 4.

One rule per array (float32 throughout, true division):

    copy          v.astype(float32)                      float32 arrays (bit for bit) and whatever else needs no scaling
    div255        v.astype(float32) / 255.0              uint8 image and labels
    div65535      v.astype(float32) / 65535.0            uint16 image and labels
    normal_u16    (v.astype(float32) / 32767.5) - 1.0    uint16 normals
    normal_mul2   (v.astype(float32) * 2.0) - 1.0        normals of any other dtype (the reference's `else`: uint8 too)

`ingest_numpy` is that statement plus the layout change ((Z, Y, X) -> (1, Z, Y, X), channels-last (Z, Y, X, C) -> (C, Z, Y, X))
and the oracle of the GPU tests; `ingest_rule` is the rule `__getitem__` applies today for a key and dtype.  `parse_ingest` reads
`dataset_config.ingest` ({where: host | device}; absent: {where: host}, every item as it is today); `DeviceIngest` is the stage
the trainer puts behind the feeder's copies for `where: device`, before dilation, geometry and the intensity stack."""
import numpy as np

from ..engine.ops.core import RULES, rule_code      # noqa: F401 -- the library's codes (index == rx_ingest_rule), beside its binding
from . import stages

DTYPES = (np.dtype(np.uint8), np.dtype(np.uint16), np.dtype(np.float32))
MAX_CHANNELS = 8


def ingest_rule(key, np_dtype):
    """the rule the host `__getitem__` applies to the array of `key` (\"image\" or a task name) stored as `np_dtype`"""
    dt = np.dtype(np_dtype)
    if str(key).lower() == "normals":
        return "normal_u16" if dt == np.uint16 else "normal_mul2"
    if dt == np.uint8:
        return "div255"
    if dt == np.uint16:
        return "div65535"
    return "copy"


def ingest_numpy(arr, rule):
    """what rx_ingest computes for ONE sample, in numpy: (Z, Y, X) or channels-last (Z, Y, X, C) in, float32 (C, Z, Y, X) out
    (C = 1 for a 3-D sample)"""
    code = rule_code(rule)
    arr = np.asarray(arr)
    if arr.ndim not in (3, 4):
        raise ValueError(f"ingest_numpy: expected (Z, Y, X) or (Z, Y, X, C), got {arr.shape}")
    t = arr.astype(np.float32)
    if code == 1:
        t /= 255.0
    elif code == 2:
        t /= 65535.0
    elif code == 3:
        t = (t / 32767.5) - 1.0
    elif code == 4:
        t = (t * 2.0) - 1.0
    t = t[None, ...] if t.ndim == 3 else t.transpose(3, 0, 1, 2)
    return np.ascontiguousarray(t, dtype=np.float32)


def parse_ingest(dataset_config):
    """`dataset_config.ingest` -> {"where": "host" | "device"}.  Absent: {where: host}.  Unknown keys and a `where` that is
    neither host nor device raise with the key named."""
    return {"where": stages.block(dataset_config, "ingest", ("where",), "host", {})["where"]}


class DeviceIngest:
    """`ingest(batch_dict) -> batch_dict` on the CURRENT stream: every key of `rules` -- a raw device batch, uint8, uint16 or
    float32, (B, Z, Y, X) or channels-last (B, Z, Y, X, C) -- becomes the float32 batch the host items collate to:
    (B, C, Z, Y, X), except that a 3-D `normals` array stays (B, Z, Y, X) as the host leaves it.  A key without a rule must
    already be float32 and stays the tensor object it was."""

    def __init__(self, rules):
        self.rules = {str(k): RULES[rule_code(v)] for k, v in dict(rules).items()}

    def __call__(self, batch):
        import torch
        from ..engine import ops as E
        from ..engine.lib import RxError
        out = {}
        for k, t in batch.items():
            rule = self.rules.get(k)
            if rule is None:
                if getattr(t, "dtype", None) != torch.float32:
                    raise RxError(f"DeviceIngest: {k!r} is {getattr(t, 'dtype', type(t))} and has no rule (rules: {sorted(self.rules)})")
                out[k] = t
                continue
            stages.check_tensor("DeviceIngest", k, t, "dataset_config.ingest.where: host scales in the dataset",
                                "(B, Z, Y, X) or (B, Z, Y, X, C)")
            r = E.ingest(t, rule)
            out[k] = r[:, 0] if t.dim() == 4 and k.lower() == "normals" else r
        for k in self.rules:
            if k not in batch:
                raise RxError(f"DeviceIngest: the batch has no {k!r} (it has {sorted(batch)})")
        return out
