"""CPU: `dataloading/stages.py` -- the config helpers through every `parse_*`, the table of stage-order constraints row by row,
`DevicePipeline`'s order with recording fake stages, and `stage_rng` against the expression it replaced."""
import random

import pytest
import torch

import mt3d_amd  # noqa: F401
from mt3d_amd.dataloading import stages
from mt3d_amd.dataloading.dilate_device import parse_dilate
from mt3d_amd.dataloading.elastic_device import parse_elastic
from mt3d_amd.dataloading.geometry_device import parse_geometric
from mt3d_amd.dataloading.ingest_device import parse_ingest
from mt3d_amd.dataloading.patch_search_device import parse_patch_search
from mt3d_amd.dataloading.spatial_device import parse_spatial

TASKS = {"sheet": {"channels": 1}, "normals": {"channels": 3}}
PATCH = (16, 16, 16)
# name -> (parse(dataset_config, patch, tasks), what an absent block gives, has a patch, has normal_keys)
PARSERS = {
    "geometric": (parse_geometric, None, True, True),
    "spatial": (parse_spatial, None, True, True),
    "elastic": (parse_elastic, None, True, True),
    "dilate": (lambda cfg, patch, tasks: parse_dilate(cfg, True, tasks), {"radius": 5, "where": "host", "keys": ["sheet"]}, False, False),
    "ingest": (lambda cfg, patch, tasks: parse_ingest(cfg), {"where": "host"}, False, False),
    "patch_search": (lambda cfg, patch, tasks: parse_patch_search(cfg), {"where": "host", "max_device_bytes": None}, False, False),
}
# (case, block, patch, tasks, the key the ValueError names -- None: accepted, "absent": what an absent block gives)
CASES = [
    ("false", False, PATCH, TASKS, "absent"),
    ("null", None, PATCH, TASKS, "absent"),
    ("true", True, PATCH, TASKS, None),
    ("a non-mapping", "device", PATCH, TASKS, ": expected a mapping"),
    ("an unknown key", {"bogus": 1}, PATCH, TASKS, r": unknown key\(s\) \['bogus'\]"),
    ("a bad where", {"where": "gpu"}, PATCH, TASKS, r"\.where"),
    ("where: null", {"where": None}, PATCH, TASKS, r"\.where"),
    ("a 2-D patch", {}, (16, 16), TASKS, ".*3-D patch"),
    ("normal_keys as a string", {"normal_keys": "normals"}, PATCH, TASKS, None),
    ("a 1-channel task in normal_keys", {"normal_keys": ["sheet"]}, PATCH, TASKS, r"\.normal_keys.*'sheet'.*channels = 1"),
]


@pytest.mark.parametrize("name", list(PARSERS))
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_one_table_through_every_parser(name, case):
    parse, absent, has_patch, has_normal_keys = PARSERS[name]
    what, blk, patch, tasks, key = case
    if (what == "a 2-D patch" and not has_patch) or ("normal_keys" in what and not has_normal_keys):
        key = r": unknown key" if isinstance(blk, dict) and blk else None          # not this stage's key: refused as unknown, or moot
    if key is None:
        got = parse({name: blk}, patch, tasks)
        assert got["where"] == ("host" if absent is not None else "device")
        if has_normal_keys:
            assert got["normal_keys"] == ("normals",)
    elif key == "absent":
        assert parse({name: blk}, patch, tasks) == absent and parse({}, patch, tasks) == absent and parse(None, patch, tasks) == absent
    else:
        with pytest.raises(ValueError, match=rf"dataset_config\.{name}{key}"):
            parse({name: blk}, patch, tasks)


def test_probability():
    assert stages.probability("o", "p", 1) == 1.0 and stages.probability("o", "p", "0.25") == 0.25
    for bad in (1.5, -0.1, float("nan"), "often", None, [0.5]):
        with pytest.raises(ValueError, match=r"o\.k\.p: .* is not a probability"):
            stages.probability("o.k", "p", bad)
    for parse, blk, key in [(parse_geometric, {"flip": {"p": 1.5}}, r"geometric\.flip\.p"), (parse_geometric, {"rot90": {"p_transform": -1}}, r"geometric\.rot90\.p_transform"),
                            (parse_spatial, {"rotation": {"p": 2}}, r"spatial\.rotation\.p"), (parse_spatial, {"scale": {"p": "x"}}, r"spatial\.scale\.p"),
                            (parse_elastic, {"p": 1.01}, r"elastic\.p")]:
        name = key.split("\\")[0]
        with pytest.raises(ValueError, match=r"dataset_config\." + key + ": .* is not a probability"):
            parse({name: blk}, PATCH, TASKS)


# ---- the order constraints ---------------------------------------------------------------------------------------------------------
def _arguments(**where):
    """check_stage_order's arguments from {stage: place}"""
    return dict(augment=where.get("augment") == "host",
                **{n: ({"where": where[n]} if n in where else None) for n in ("geometric", "dilate", "ingest", "spatial", "elastic")})


# the texts of the three functions this table replaced, one per row, in the table's order
MESSAGES = [
    r"dataset_config\.augment: the restated stack runs on the host, on scaled floats; dataset_config\.ingest\.where: device needs "
    r"augment: \"device\" or false",
    r"dataset_config\.geometric\.where: the host transforms work on scaled floats; dataset_config\.ingest\.where: device needs "
    r"geometric absent or where: device",
    r"dataset_config\.dilate\.where: the host dilation \(the default under tr_setup\.dilate_label\) works on scaled floats; "
    r"dataset_config\.ingest\.where: device needs dilate\.where: device or dilate_label off",
    r"dataset_config\.spatial\.where: \"host\" cannot follow dataset_config\.ingest\.where: \"device\" \(the items are the store's "
    r"integers\); take spatial\.where: \"device\"",
    r"dataset_config\.spatial\.where: \"host\" cannot precede dataset_config\.dilate\.where: \"device\" \(the ball is not "
    r"scale-invariant: dilation comes first\); take spatial\.where: \"device\" or dilate\.where: \"host\"",
    r"dataset_config\.elastic\.where: \"host\" cannot follow dataset_config\.ingest\.where: \"device\" \(the items are the store's "
    r"integers\); take elastic\.where: \"device\"",
    r"dataset_config\.elastic\.where: \"host\" cannot precede dataset_config\.dilate\.where: \"device\" \(the ball is not "
    r"deformation-invariant: dilation comes first\); take elastic\.where: \"device\" or dilate\.where: \"host\"",
]


def test_every_order_constraint_violated_and_satisfied():
    assert len(stages._ORDER) == len(MESSAGES) == 7
    for (a, where_a, b, where_b, _), message in zip(stages._ORDER, MESSAGES):
        with pytest.raises(ValueError, match="^" + message + "$"):
            stages.check_stage_order(**_arguments(**{a: where_a, b: where_b}))
        other = {"host": "device", "device": "host"}
        if a != "augment":
            stages.check_stage_order(**_arguments(**{a: other[where_a], b: where_b}))          # the first stage elsewhere
        stages.check_stage_order(**_arguments(**{a: where_a, b: other[where_b]}))              # the second stage elsewhere
        stages.check_stage_order(**_arguments(**{a: where_a}))                                 # ... or off
        stages.check_stage_order(**_arguments(**{b: where_b}))
    stages.check_stage_order(False, None, None, None, None, None)
    everything = {n: "device" for n in ("geometric", "dilate", "ingest", "spatial", "elastic")}
    stages.check_stage_order(**_arguments(**everything))
    stages.check_stage_order(**_arguments(augment="host", **{n: "host" for n in everything}))
    with pytest.raises(ValueError, match="^" + MESSAGES[0]):          # several at once: the first row
        stages.check_stage_order(**_arguments(augment="host", ingest="device", spatial="host", geometric="host"))


def test_parse_stages_is_the_parsers_and_the_order_check():
    cfg = {"geometric": {"flip": {}}, "spatial": {"scale": {}, "where": "host"}, "elastic": True, "dilate": {"where": "device", "radius": 2},
           "patch_search": {"max_device_gb": 1}}
    with pytest.raises(ValueError, match=MESSAGES[4]):
        stages.parse_stages(cfg, PATCH, TASKS, dilate_label=True)
    st = stages.parse_stages(cfg, PATCH, TASKS, dilate_label=False)
    assert st.geometric == parse_geometric(cfg, PATCH, TASKS) and st.spatial == parse_spatial(cfg, PATCH, TASKS)
    assert st.elastic == parse_elastic(cfg, PATCH, TASKS) and st.dilate is None and st.ingest == {"where": "host"}
    assert st.patch_search == {"where": "host", "max_device_bytes": 1 << 30}
    assert st.device_geometric is st.geometric and st.device_spatial is None and st.device_elastic is st.elastic and st.device_dilate is None
    st = stages.parse_stages(dict(cfg, spatial=False), PATCH, TASKS, dilate_label=True)
    assert st.device_dilate == {"radius": 2, "where": "device", "keys": ["sheet"]} and st.spatial is None
    assert set(st.attributes()) == {"geometric", "spatial", "elastic", "dilate", "ingest", "patch_search", "device_geometric",
                                    "device_spatial", "device_elastic", "device_dilate"}
    with pytest.raises(ValueError, match=MESSAGES[0]):
        stages.parse_stages({"ingest": {"where": "device"}}, PATCH, TASKS, augment=True)


# ---- the pipeline ------------------------------------------------------------------------------------------------------------------
def _recording(name, calls):
    def stage(batch):
        calls.append((name, sorted(batch) if isinstance(batch, dict) else tuple(batch.shape)))
        if isinstance(batch, dict):
            return {k: v + 1 for k, v in batch.items()}
        return batch + 100
    return stage


def test_pipeline_order_with_recording_stages():
    names = ("ingest", "dilate", "geometry", "spatial", "elastic", "augmenter")
    calls = []
    pipe = stages.DevicePipeline(**{n: _recording(n, calls) for n in reversed(names)})          # keywords in any order
    assert pipe
    batch = {"image": torch.zeros(2, 1, 2, 2, 2), "sheet": torch.zeros(2, 2, 2, 2)}
    out = pipe(batch)
    assert [c[0] for c in calls] == list(names)
    assert all(c[1] == ["image", "sheet"] for c in calls[:5]) and calls[5][1] == (2, 1, 2, 2, 2)          # the augmenter: `image` only
    assert bool((out["image"] == 105).all()) and bool((out["sheet"] == 5).all())
    del calls[:]
    some = stages.DevicePipeline(elastic=_recording("elastic", calls), dilate=_recording("dilate", calls))
    assert some and [some(batch), [c[0] for c in calls]][1] == ["dilate", "elastic"]            # absent stages are skipped
    del calls[:]
    only = stages.DevicePipeline(augmenter=_recording("augmenter", calls))
    out = only(dict(batch))
    assert only and calls == [("augmenter", (2, 1, 2, 2, 2))] and out["sheet"] is batch["sheet"]
    empty = stages.DevicePipeline()
    assert not empty and empty(batch) is batch


def test_pipeline_copies_in_the_stores_dtype_only_behind_ingest():
    batch = {"image": torch.zeros(1, 2, 2, 2, dtype=torch.uint8), "normals": torch.zeros(1, 2, 2, 2, 3, dtype=torch.int16)}
    got = stages.DevicePipeline(ingest=lambda b: b).to_device(batch, "cpu")
    assert got["image"].dtype == torch.uint8 and got["normals"].dtype == torch.int16
    for pipe in (stages.DevicePipeline(), stages.DevicePipeline(dilate=lambda b: b)):
        assert all(v.dtype == torch.float32 for v in pipe.to_device(batch, "cpu").values())


def test_from_dataset_maps_the_blocks_to_the_stages():
    from types import SimpleNamespace
    cfg = {"geometric": {"flip": {"p": 1.0}}, "spatial": {"rotation": {"max_degrees": 10}, "image_border": "clamp"},
           "elastic": {"spacing": 8, "magnitude": [0, 1], "p": 1.0}, "dilate": {"where": "device", "radius": 2}}
    ds = SimpleNamespace(device_ingest={"image": "div255"}, device_augment=False,
                         **stages.parse_stages(cfg, PATCH, TASKS, dilate_label=True).attributes())
    pipe = stages.DevicePipeline.from_dataset(ds, rank=3)
    assert pipe.ingest.rules == {"image": "div255"} and pipe.dilate.radius == 2 and pipe.dilate.keys == ["sheet"]
    assert pipe.geometry.flip == {"p": 1.0} and pipe.geometry.rot90 is None and pipe.geometry.normal_keys == {"normals"}
    assert pipe.spatial.rotation["max_degrees"] == 10.0 and pipe.spatial.scale is None and pipe.spatial.image_border == "clamp"
    assert pipe.elastic.spacing == (8, 8, 8) and pipe.elastic.magnitude == (0.0, 1.0) and pipe.elastic.p == 1.0
    assert pipe.augmenter is None
    assert pipe.geometry.rng.random() == stages.stage_rng(rank=3).random()          # the rank reaches every stage's generator
    off = SimpleNamespace(device_ingest=None, device_augment=False, **stages.parse_stages({}, PATCH, TASKS).attributes())
    assert not stages.DevicePipeline.from_dataset(off) and not stages.DevicePipeline.from_dataset(object())


# ---- the generator -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,rank", [(1234, 0), (7, 4097), ((1 << 63) + 12345, 3), (-5, 1)])
def test_stage_rng_is_the_expression_it_replaces(seed, rank):
    old = random.Random((seed % (1 << 63)) * 4096 + int(rank) % 4096)
    new = stages.stage_rng(seed, rank)
    assert [old.random() for _ in range(8)] == [new.random() for _ in range(8)]
    before = torch.initial_seed()
    torch.manual_seed(seed % (1 << 62))          # seed None: torch's
    try:
        old = random.Random((torch.initial_seed() % (1 << 63)) * 4096 + int(rank) % 4096)
        new = stages.stage_rng(None, rank)
        assert [old.random() for _ in range(8)] == [new.random() for _ in range(8)]
    finally:
        torch.manual_seed(before)
