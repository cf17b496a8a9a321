"""What the device stages of the training input side share, each piece written once: the generator (`stage_rng`), the batch
contract (`check_tensor`, `check_batch`, `batch_draws`, `per_tensor`, `resample_batch`), the host item path (`apply_item`,
`check_resample_args`, `finish_resample`), the `dataset_config` blocks (`block`, `probability`, `normal_keys`, `patch3d`,
`check_stage_order`, `parse_stages`) and the ORDER of the stages (`DevicePipeline`: its docstring is the one statement of it).
The stages themselves -- their records, draws, numpy oracles and kernels -- stay in their own `*_device.py`."""
import random as _random
from dataclasses import dataclass

import numpy as np

from ..engine.ops.core import BORDER, INTERP

MAX_EXTENT = 1 << 24      # float32 holds every voxel index below this exactly
WHERE = ("host", "device")


def stage_rng(seed=None, rank=0):
    """the generator of one stage: seeded from `torch.initial_seed()` (`seed` None) and the rank -- ranks differ, a seeded run
    repeats.  Every stage keeps an instance of its own, so a stage's draws do not depend on which other stages are on."""
    if seed is None:
        import torch
        seed = torch.initial_seed()
    return _random.Random((int(seed) % (1 << 63)) * 4096 + int(rank) % 4096)


# ---- the batch contract: a dict of device tensors, (B, C, Z, Y, X) or (B, Z, Y, X) -----------------------------------------------------
def check_tensor(owner, k, t, host_hint, layouts="(B, C, Z, Y, X) or (B, Z, Y, X)", B=None):
    from ..engine.lib import RxError
    if not hasattr(t, "is_cuda") or not t.is_cuda:
        raise RxError(f"{owner}: {k!r} must be a device tensor ({host_hint})")
    if t.dim() not in (4, 5) or (B is not None and int(t.shape[0]) != B):
        raise RxError(f"{owner}: {k!r} {tuple(t.shape)}: expected {layouts}" + (f" with B = {B}" if B is not None else ""))


def check_batch(owner, batch, normal_keys=(), host_hint=""):
    """every tensor on the device, 4-D or 5-D with one B, the `normal_keys` (B, 3, Z, Y, X) -> (B, (Z, Y, X) of the first tensor)"""
    from ..engine.lib import RxError
    first = next(iter(batch.values()))
    B = int(first.shape[0])
    for k, t in batch.items():
        check_tensor(owner, k, t, host_hint, B=B)
        if k in normal_keys and (t.dim() != 5 or int(t.shape[1]) != 3):
            raise RxError(f"{owner}: {k!r} {tuple(t.shape)} is in normal_keys and must be (B, 3, Z, Y, X)")
    return B, tuple(int(v) for v in first.shape[-3:])


def batch_draws(owner, noun, given, B, draw):
    """the per-sample draws of a call: `given`, or B calls of `draw`"""
    draws = [draw() for _ in range(B)] if given is None else list(given)
    if len(draws) != B:
        raise ValueError(f"{owner}: {len(draws)} {noun} for a batch of {B}")
    return draws


def per_tensor(batch, fn):
    """{k: fn(k, the 5-D view of batch[k])}, each result in the rank its tensor came in"""
    out = {}
    for k, t in batch.items():
        r = fn(k, t if t.dim() == 5 else t.unsqueeze(1))
        out[k] = r if t.dim() == 5 else r.squeeze(1)
    return out


def resample_batch(batch, normal_keys, image_border, image_fill, apply):
    """the sampling rules of a resampling stage: `image` linear with the image border rule, every other tensor nearest / constant /
    fill 0, the tensors named in `normal_keys` with the vector rule.  `apply(five, interp, border, fill, vector=False)` launches."""
    def one(k, five):
        if k == "image":
            return apply(five, "linear", image_border, image_fill)
        return apply(five, "nearest", "constant", 0.0, vector=k in normal_keys)
    return per_tensor(batch, one)


# ---- the host item path of a resampling stage ------------------------------------------------------------------------------------------
def apply_item(item, normal_keys, image_border, image_fill, fn):
    """`fn(array, interp, border, fill, is_normal)` on every array of a dataset item under the rules of `resample_batch`.  Torch
    tensors come back as torch tensors."""
    out = {}
    for k, v in item.items():
        is_t = hasattr(v, "numpy")
        x = np.ascontiguousarray(v.numpy() if is_t else v, dtype=np.float32)
        y = fn(x, "linear", image_border, image_fill, False) if k == "image" else fn(x, "nearest", "constant", 0.0, k in normal_keys)
        if is_t:
            import torch
            y = torch.from_numpy(y)
        out[k] = y
    return out


def check_resample_args(who, arr, interp, border, is_normal):
    """the argument checks of `affine_numpy` / `elastic_numpy` -> (`arr` as an array, its (C, Z, Y, X) view)"""
    if interp not in INTERP:
        raise ValueError(f"{who}: interp {interp!r} (linear or nearest)")
    if border not in BORDER:
        raise ValueError(f"{who}: border {border!r} (constant or clamp)")
    arr = np.asarray(arr)
    a = arr[None] if arr.ndim == 3 else arr
    if a.ndim != 4 or a.dtype != np.float32:
        raise ValueError(f"{who}: expected float32 (Z, Y, X) or (C, Z, Y, X), got {arr.dtype} {arr.shape}")
    if is_normal and a.shape[0] != 3:
        raise ValueError(f"{who}: a normals array has 3 components, got {a.shape[0]}")
    if max(a.shape[1:]) > MAX_EXTENT:
        raise ValueError(f"{who}: an extent of {a.shape[1:]} is beyond {MAX_EXTENT} (float32 coordinates)")
    return arr, a


def finish_resample(s, arr):
    """the sampled (C, Z, Y, X) values as a new contiguous float32 array in the rank of `arr`"""
    out = np.ascontiguousarray(s, dtype=np.float32)
    if np.shares_memory(out, arr):
        out = out.copy()
    return out[0] if arr.ndim == 3 else out


# ---- dataset_config blocks -------------------------------------------------------------------------------------------------------------
def block(dataset_config, name, known, default_where, absent):
    """`dataset_config.<name>` -> a copy of the mapping with `where` lower-cased and filled in.  An absent, null or false block is
    `absent`: None (the stage is off; None comes back) or {} (the stage always has a block; its defaults).  True is {}.  Anything
    but a mapping, a key outside `known` and a `where` that is neither host nor device raise with the key named."""
    g = (dataset_config or {}).get(name, None)
    if g is None or g is False:
        g = absent
    elif g is True:
        g = {}
    if g is None:
        return None
    if not isinstance(g, dict):
        raise ValueError(f"dataset_config.{name}: expected a mapping ({', '.join(known)}), got {g!r}")
    unknown = sorted(str(k) for k in set(g) - set(known))
    if unknown:
        raise ValueError(f"dataset_config.{name}: unknown key(s) {unknown} (known: {', '.join(known)})")
    where = g.get("where", default_where)
    if str(where).lower() not in WHERE:
        raise ValueError(f"dataset_config.{name}.where: {where!r} (\"host\" or \"device\")")
    return dict(g, where=str(where).lower())


def probability(owner, key, value):
    try:
        p = float(value)
    except (TypeError, ValueError):
        p = -1.0
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"{owner}.{key}: {value!r} is not a probability")
    return p


def normal_keys(owner, g, tasks):
    """`normal_keys` of a block (a name or a list; default ("normals",)) as a tuple; a task named there has 3 channels"""
    nk = g.get("normal_keys", ("normals",))
    nk = tuple(str(k) for k in ((nk,) if isinstance(nk, str) else nk))
    for k in nk:
        if k in (tasks or {}) and int(tasks[k].get("channels", 0)) != 3:
            raise ValueError(f"{owner}.normal_keys: task {k!r} has channels = {tasks[k].get('channels')}, a normals target has 3")
    return nk


def patch3d(owner, patch_size):
    patch = tuple(int(v) for v in patch_size)
    if len(patch) != 3:
        raise ValueError(f"{owner}: needs a 3-D patch, patch_size is {list(patch)}")
    return patch


def image_border(owner, g):
    border = str(g.get("image_border", "constant")).lower()
    if border not in BORDER:
        raise ValueError(f"{owner}.image_border: {g.get('image_border')!r} (\"constant\" or \"clamp\")")
    return border


_FLOAT_ITEMS = "(the items are the store's integers)"
# (stage, its place, a second stage, its place, what to say): a combination that cannot be served.  Device ingest hands out the
# store's integers, so no host stage that works on scaled floats can follow it; a host resampling stage cannot precede the device
# dilation, because the ball commutes with the signed permutations only.
_ORDER = (
    ("augment", "host", "ingest", "device",
     "dataset_config.augment: the restated stack runs on the host, on scaled floats; "
     "dataset_config.ingest.where: device needs augment: \"device\" or false"),
    ("geometric", "host", "ingest", "device",
     "dataset_config.geometric.where: the host transforms work on scaled floats; "
     "dataset_config.ingest.where: device needs geometric absent or where: device"),
    ("dilate", "host", "ingest", "device",
     "dataset_config.dilate.where: the host dilation (the default under tr_setup.dilate_label) works on scaled "
     "floats; dataset_config.ingest.where: device needs dilate.where: device or dilate_label off"),
    ("spatial", "host", "ingest", "device",
     f"dataset_config.spatial.where: \"host\" cannot follow dataset_config.ingest.where: \"device\" {_FLOAT_ITEMS}; "
     "take spatial.where: \"device\""),
    ("spatial", "host", "dilate", "device",
     "dataset_config.spatial.where: \"host\" cannot precede dataset_config.dilate.where: \"device\" (the ball is "
     "not scale-invariant: dilation comes first); take spatial.where: \"device\" or dilate.where: \"host\""),
    ("elastic", "host", "ingest", "device",
     f"dataset_config.elastic.where: \"host\" cannot follow dataset_config.ingest.where: \"device\" {_FLOAT_ITEMS}; "
     "take elastic.where: \"device\""),
    ("elastic", "host", "dilate", "device",
     "dataset_config.elastic.where: \"host\" cannot precede dataset_config.dilate.where: \"device\" (the ball is "
     "not deformation-invariant: dilation comes first); take elastic.where: \"device\" or dilate.where: \"host\""),
)


def check_stage_order(augment, geometric, dilate, ingest, spatial, elastic):
    """`augment`: True when the dataset applies the restated intensity stack; the others: parsed blocks or None.  Raises ValueError
    with the message of the first row of `_ORDER` that holds."""
    place = {"augment": "host" if augment else None}
    for name, cfg in (("geometric", geometric), ("dilate", dilate), ("ingest", ingest), ("spatial", spatial), ("elastic", elastic)):
        place[name] = None if cfg is None else cfg.get("where")
    for a, where_a, b, where_b, message in _ORDER:
        if place[a] == where_a and place[b] == where_b:
            raise ValueError(message)


@dataclass(frozen=True)
class Stages:
    """the parsed blocks of a dataset (`parse_stages`); `device_<name>`: the block if it says `where: device`, else None"""
    geometric: dict
    spatial: dict
    elastic: dict
    dilate: dict
    ingest: dict
    patch_search: dict

    def device(self, name):
        cfg = getattr(self, name)
        return cfg if cfg is not None and cfg["where"] == "device" else None

    device_geometric = property(lambda self: self.device("geometric"))
    device_spatial = property(lambda self: self.device("spatial"))
    device_elastic = property(lambda self: self.device("elastic"))
    device_dilate = property(lambda self: self.device("dilate"))

    def attributes(self):
        """what a dataset exposes under its own attribute names (`device_ingest` is the dataset's: the rules of its stores)"""
        names = ("geometric", "spatial", "elastic", "dilate", "ingest", "patch_search", "device_geometric", "device_spatial",
                 "device_elastic", "device_dilate")
        return {n: getattr(self, n) for n in names}


def parse_stages(dataset_config, patch, tasks, dilate_label=False, augment=False):
    """every stage block of `dataset_config`, parsed and checked against the others -> `Stages`"""
    from .dilate_device import parse_dilate
    from .elastic_device import parse_elastic
    from .geometry_device import parse_geometric
    from .ingest_device import parse_ingest
    from .patch_search_device import parse_patch_search
    from .spatial_device import parse_spatial
    st = Stages(geometric=parse_geometric(dataset_config, patch, tasks), spatial=parse_spatial(dataset_config, patch, tasks),
                elastic=parse_elastic(dataset_config, patch, tasks), dilate=parse_dilate(dataset_config, dilate_label, tasks),
                ingest=parse_ingest(dataset_config), patch_search=parse_patch_search(dataset_config))
    check_stage_order(augment, st.geometric, st.dilate, st.ingest, st.spatial, st.elastic)
    return st


# ---- the order -------------------------------------------------------------------------------------------------------------------------
class DevicePipeline:
    """The device stages of a training batch, in the ONE order they are applied in, behind `DeviceFeeder`'s copies and in
    `forward_loss` for every batch the feeder did not stage (RX_DEVICE_FEEDER=0, validation) alike:

        ingest     `DeviceIngest`     the store's integers -> the float32 (B, C, Z, Y, X) batch the host items collate to
        dilate     `DeviceDilate`     the label targets, in place, with the ball: before anything moves (the ball commutes with the
                                      signed permutations only)
        geometry   `DeviceGeometry`   flips and 90-degree rotations, image and targets together
        spatial    `DeviceSpatial`    small-angle rotation and scale, image and targets together
        elastic    `DeviceElastic`    the B-spline deformation, image and targets together
        augmenter  `DeviceAugmenter`  the intensity stack, on `image` only

    the order `__getitem__` applies the `where: host` counterparts in.  A stage that is None is skipped; a pipeline without a
    stage is falsy and hands a batch back as it came."""
    BATCH_STAGES = ("ingest", "dilate", "geometry", "spatial", "elastic")      # each takes and returns the whole dict; then `augmenter`

    def __init__(self, ingest=None, dilate=None, geometry=None, spatial=None, elastic=None, augmenter=None):
        self.ingest, self.dilate, self.geometry = ingest, dilate, geometry
        self.spatial, self.elastic, self.augmenter = spatial, elastic, augmenter

    def __bool__(self):
        return self.augmenter is not None or any(getattr(self, name) is not None for name in self.BATCH_STAGES)

    def to_device(self, batch, device):
        """the host-to-device copies, non-blocking, on the current stream: in the store's dtype when `ingest` scales on the device
        (integers over the link), as float32 otherwise"""
        import torch
        dtype = None if self.ingest is not None else torch.float32
        return {k: v.to(device, dtype=dtype, non_blocking=True) for k, v in batch.items()}

    def __call__(self, batch):
        """`batch`: a dict of device tensors -> the dict after every stage, on the current stream"""
        for name in self.BATCH_STAGES:
            stage = getattr(self, name)
            if stage is not None:
                batch = stage(batch)
        if self.augmenter is not None:
            batch["image"] = self.augmenter(batch["image"])
        return batch

    @classmethod
    def from_dataset(cls, dataset, rank=0):
        """the stages a dataset's parsed blocks ask for (`Stages.attributes`; `device_augment`, `device_ingest`: the dataset's own)"""
        from .augment_device import DeviceAugmenter
        from .dilate_device import DeviceDilate
        from .elastic_device import DeviceElastic
        from .geometry_device import DeviceGeometry
        from .ingest_device import DeviceIngest
        from .spatial_device import DeviceSpatial

        def build(attribute, make):
            cfg = getattr(dataset, attribute, None)
            return None if cfg is None or cfg is False else make(cfg)
        resample = ("normal_keys", "image_border")
        return cls(
            ingest=build("device_ingest", DeviceIngest),
            dilate=build("device_dilate", lambda c: DeviceDilate(c["keys"], c["radius"])),
            geometry=build("device_geometric", lambda c: DeviceGeometry(rank=rank, **{k: c[k] for k in ("flip", "rot90", "normal_keys")})),
            spatial=build("device_spatial", lambda c: DeviceSpatial(rank=rank, **{k: c[k] for k in ("rotation", "scale") + resample})),
            elastic=build("device_elastic", lambda c: DeviceElastic(rank=rank, **{k: c[k] for k in ("spacing", "magnitude", "p") + resample})),
            augmenter=build("device_augment", lambda c: DeviceAugmenter(rank=rank)))
