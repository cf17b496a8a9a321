"""CPU: the validation preview's numpy statement (training/visualization/preview.py) against the frames the reference's own
`save_debug_gif` produced (tests/golden/preview.npz, scripts/make_preview_fixture.py), its own rules where the reference has none,
the layout, the config parser, the GIF writer and the C ABI entry."""
import os
import re

import numpy as np
import pytest
import torch

import mt3d_amd  # noqa: F401
from mt3d_amd.training import visualization as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "preview.npz"))
TASKS = {"sheet": {"channels": 1, "activation": "sigmoid"}, "normals": {"channels": 3, "activation": "none"},
         "ink": {"channels": 1, "activation": "none"}}


def _case(i):
    pick = lambda prefix: {k[len(prefix):]: GOLDEN[k][0] for k in GOLDEN.files if k.startswith(prefix)}
    return GOLDEN[f"image_{i}"][0], pick(f"target_{i}_"), pick(f"pred_{i}_"), tuple(str(s) for s in GOLDEN[f"sigmoid_{i}"]), GOLDEN[f"frames_{i}"]


def _cases(with_sigmoid):
    return [i for i in range(int(GOLDEN["n_cases"])) if (len(GOLDEN[f"sigmoid_{i}"]) > 0) == with_sigmoid]


def test_fixture_has_the_cases_the_statement_is_pinned_on():
    assert len(_cases(False)) >= 2 and len(_cases(True)) >= 1
    _, targets, _, _, frames = _case(1)
    assert frames.shape == (4, 12, 21, 3)
    r = targets["sheet"][0].reshape(4, -1)
    r = r.max(1) - r.min(1)
    assert r[1] == np.float32(5e-7) and r[2] == np.float32(2e-6)      # one slice on either side of the 1e-6 test


@pytest.mark.parametrize("i", _cases(False))
def test_frames_equal_the_reference_byte_for_byte(i):
    image, targets, preds, _, want = _case(i)
    got = V.frames_numpy(image, targets, preds)
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert np.array_equal(got, want)


@pytest.mark.parametrize("i", _cases(True))
def test_reference_sigmoid_within_one_grey_level(i):
    image, targets, preds, sig, want = _case(i)
    for n in sig:      # what makes the cap a property of the inputs: every slice spans at least 0.1 after the sigmoid
        s = 1.0 / (1.0 + np.exp(-preds[n].astype(np.float64)))
        s = s.reshape(s.shape[0] * s.shape[1], -1)
        assert (s.max(1) - s.min(1)).min() >= 0.1
    got = V.frames_numpy(image, targets, preds, sigmoid_tasks=sig)
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    print(f"case {i}: max byte difference {d.max()}, share of differing bytes {(d > 0).mean():.5f}")
    assert d.max() <= 1 and (d > 0).mean() <= 0.01
    # ... and without the second sigmoid the panel is a different one (the option does something)
    assert not np.array_equal(V.frames_numpy(image, targets, preds), want)
    # a float64 evaluation of the same statement stays inside the same cap against the float32 one
    for n in sig:
        a, b = V.panel_numpy(preds[n], sigmoid=True), V.panel_numpy(preds[n], sigmoid=True, dtype=np.float64)
        d = np.abs(a.astype(np.int32) - b.astype(np.int32))
        print(f"case {i} {n}: float64 against float32: max {d.max()}, share {(d > 0).mean():.5f}")
        assert d.max() <= 1 and (d > 0).mean() <= 0.01


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_slice_with_a_non_finite_value_is_127(bad):
    rng = np.random.default_rng(5)
    vol = rng.standard_normal((3, 3, 4, 5)).astype(np.float32)
    clean = V.panel_numpy(vol)
    vol[1, 2, 3, 4] = bad
    got = V.panel_numpy(vol)
    assert (got[2, :, :, 1] == 127).all()
    keep = np.ones(got.shape, bool)
    keep[2, :, :, 1] = False
    assert np.array_equal(got[keep], clean[keep])      # the other slices and the other channels of that slice are untouched
    mm = V.minmax_numpy(vol)
    assert mm.shape == (3, 3, 2) and np.isnan(mm[1, 2]).all() and np.isfinite(np.delete(mm.reshape(9, 2), 5, axis=0)).all()


def test_a_range_that_overflows_is_127_and_flat_slices_are_127():
    vol = np.zeros((1, 3, 2, 2), np.float32)
    vol[0, 0] = [[3e38, -3e38], [0, 1]]
    vol[0, 1] = 4.5
    vol[0, 2] = [[0, 1], [0.5, 0.25]]
    got = V.panel_numpy(vol)
    assert (got[0] == 127).all() and (got[1] == 127).all()
    assert np.array_equal(got[2, :, :, 0], [[0, 255], [127, 63]])
    assert np.array_equal(got[..., 0], got[..., 1]) and np.array_equal(got[..., 0], got[..., 2])      # grey: three equal bytes


@pytest.mark.parametrize("c", [2, 4, 5])
def test_other_channel_counts_draw_channel_0(c):
    vol = np.random.default_rng(c).standard_normal((c, 2, 3, 4)).astype(np.float32)
    assert np.array_equal(V.panel_numpy(vol), V.panel_numpy(vol[:1]))


def test_three_channels_have_their_own_ranges_in_rgb_order():
    vol = np.random.default_rng(9).standard_normal((3, 2, 3, 4)).astype(np.float32) * np.array([1, 10, 100], np.float32)[:, None, None, None]
    got = V.panel_numpy(vol)
    for k in range(3):
        assert np.array_equal(got[..., k], V.panel_numpy(vol[k:k + 1])[..., 0])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_16_bit_inputs_are_the_statement_on_their_converted_values(dtype):
    t = torch.randn(3, 2, 5, 6, generator=torch.Generator().manual_seed(3)).to(dtype)
    want = V.panel_numpy(t.float().numpy())
    assert np.array_equal(V.panel_numpy(t), want)
    if dtype == torch.float16:
        assert np.array_equal(V.panel_numpy(t.numpy()), want)
    assert np.array_equal(V.panel_numpy(t, sigmoid=True), V.panel_numpy(t.float().numpy(), sigmoid=True))


@pytest.mark.parametrize("names", [("b",), ("zeta", "alpha")])
def test_layout(names):
    rng = np.random.default_rng(11)
    z, h, w = 5, 3, 4
    image = rng.standard_normal((1, z, h, w)).astype(np.float32)
    chans = {"b": 1, "zeta": 1, "alpha": 3}
    targets = {n: rng.standard_normal((chans[n], z, h, w)).astype(np.float32) for n in names}
    preds = {n: rng.standard_normal((chans[n], z, h, w)).astype(np.float32) for n in names}
    got = V.frames_numpy(image, targets, preds)
    t = len(names)
    assert got.shape == (z, 2 * h, (1 + t) * w, 3)
    assert np.array_equal(got[:, :h, :w], V.panel_numpy(image))
    assert not got[:, h:, :w].any()                                              # the blank tile
    for i, n in enumerate(sorted(names)):                                        # sorted task order, whatever the dict's order
        assert np.array_equal(got[:, :h, (1 + i) * w:(2 + i) * w], V.panel_numpy(targets[n]))
        assert np.array_equal(got[:, h:, (1 + i) * w:(2 + i) * w], V.panel_numpy(preds[n]))
    for every, kept in ((2, [0, 2, 4]), (3, [0, 3])):
        assert np.array_equal(V.frames_numpy(image, targets, preds, every=every), got[kept])
    sig = V.frames_numpy(image, targets, preds, sigmoid_tasks=names)              # only one-channel predictions take the sigmoid
    for i, n in enumerate(sorted(names)):
        assert np.array_equal(sig[:, h:, (1 + i) * w:(2 + i) * w], V.panel_numpy(preds[n], sigmoid=chans[n] == 1))
    assert np.array_equal(sig[:, :h], got[:, :h])


def test_parse_config_defaults_and_off():
    assert V.parse_config(None, TASKS) is None and V.parse_config(False, TASKS) is None
    cfg = V.parse_config(True, TASKS, model_name="M")
    assert cfg == {"sample": 0, "every": 1, "fps": 5, "tasks": ["ink", "normals", "sheet"], "reference_sigmoid": False, "path": "M_debug.gif"}
    assert V.parse_config({}, TASKS, model_name="M") == cfg
    cfg = V.parse_config({"sample": 1, "every": 2, "fps": 2.5, "tasks": ["sheet", "normals"], "reference_sigmoid": True, "path": "a/b.gif"}, TASKS)
    assert cfg == {"sample": 1, "every": 2, "fps": 2.5, "tasks": ["normals", "sheet"], "reference_sigmoid": True, "path": "a/b.gif"}
    assert V.sigmoid_tasks_of(TASKS, cfg) == ("sheet",)                           # one channel AND activation: sigmoid
    assert V.sigmoid_tasks_of(TASKS, V.parse_config(True, TASKS)) == ()


@pytest.mark.parametrize("value, key", [
    ({"slices": 2}, "slices"), ({"tasks": ["sheet", "nope"]}, "tasks"), ({"tasks": "sheet"}, "tasks"), ({"sample": -1}, "sample"),
    ({"sample": 0.5}, "sample"), ({"every": 0}, "every"), ({"every": -2}, "every"), ({"every": 1.5}, "every"), ({"fps": 0}, "fps"),
    ({"fps": -5}, "fps"), ({"fps": "fast"}, "fps"), ({"reference_sigmoid": "yes"}, "reference_sigmoid"), ({"path": ""}, "path"),
    ("on", "val_preview"), (3, "val_preview")])
def test_parse_config_rejections_name_the_key(value, key):
    with pytest.raises(ValueError, match=re.escape(key)) as e:
        V.parse_config(value, TASKS)
    assert "tr_config.val_preview" in str(e.value)
    if isinstance(value, dict) and key == "tasks" and isinstance(value["tasks"], list):
        assert "nope" in str(e.value)


@pytest.mark.parametrize("fps", [5, 10, 4])
def test_write_gif_round_trip(tmp_path, fps):
    from PIL import Image
    frames = np.random.default_rng(1).integers(0, 256, size=(4, 12, 21, 3), dtype=np.uint8)
    path = tmp_path / "sub" / "dir" / "x_debug.gif"      # the parent directory is created
    assert V.write_gif(frames, str(path), fps) == str(path)
    with Image.open(path) as im:
        assert im.n_frames == 4 and im.size == (21, 12)
        assert im.info["duration"] == 1000 // fps and im.info.get("loop") == 0
    with pytest.raises(ValueError):
        V.write_gif(frames.astype(np.float32), str(path), fps)


def test_write_gif_without_pil_logs_once_and_writes_nothing(tmp_path, monkeypatch, caplog):
    import builtins
    import logging
    real = builtins.__import__

    def no_pil(name, *a, **k):
        if name == "PIL" or name.startswith("PIL."):
            raise ImportError("No module named 'PIL'")
        return real(name, *a, **k)
    monkeypatch.setattr(builtins, "__import__", no_pil)
    monkeypatch.setattr(V.preview, "_warned_no_pil", False)
    frames = np.zeros((2, 4, 4, 3), np.uint8)
    with caplog.at_level(logging.WARNING):
        assert V.write_gif(frames, str(tmp_path / "a.gif")) is None and V.write_gif(frames, str(tmp_path / "a.gif")) is None
    assert sum("PIL" in r.getMessage() for r in caplog.records) == 1 and not os.listdir(tmp_path)


def test_entry_point_is_declared_built_and_bound():
    import ctypes
    import __graft_entry__
    __graft_entry__.build()
    from mt3d_amd.engine import lib
    hdr = open(os.path.join(ROOT, "include", "rxunet.h")).read()
    assert re.search(r"\bint\s+rx_preview_panel\s*\(", hdr)
    assert hasattr(ctypes.CDLL(lib.LIB_PATH), "rx_preview_panel")
    assert "rx_preview_panel" in lib.exported_symbols()
    assert lib.load().rx_abi_version() == 1
    from mt3d_amd.engine import ops
    with pytest.raises(lib.RxError):      # no host fallback: a CPU tensor is an error
        ops.preview_panel(torch.zeros(1, 2, 3, 4), torch.zeros(2, 3, 4, 3, dtype=torch.uint8), 0, 0)
    with pytest.raises(lib.RxError):
        ops.preview_frames(torch.zeros(1, 1, 2, 3, 4), {"a": torch.zeros(1, 1, 2, 3, 4)}, {"a": torch.zeros(1, 1, 2, 3, 4)})
