"""Regenerate tests/golden/preview.npz: the frames the REFERENCE's own `save_debug_gif` (training/visualization/plotting.py) hands
to its GIF writer on small seeded inputs, pinning training/visualization/preview.py: panel_numpy / frames_numpy and, through them,
the device preview.

    RX_REFERENCE_ROOT=<reference checkout> python scripts/make_preview_fixture.py

plotting.py imports `cv2`, `imageio`, `tifffile` and `torch.utils.tensorboard` at module level.  Whichever is not installed is
stubbed (`load_reference_plotting`): `cv2.cvtColor(img, COLOR_GRAY2BGR)` as a three-fold repeat of the grey byte, which is what
OpenCV does; `imageio.mimsave` as a function that keeps the frames it is given instead of encoding them; the other two are never
called.  `save_debug_gif` runs as it is.  Recorded per case i: `image_i` (1, 1, Z, H, W), `target_i_<task>` and `pred_i_<task>`
(1, C, Z, H, W), all float32, `sigmoid_i` (the names of the tasks with `activation: sigmoid`) and `frames_i` (Z, 2H, (1 + T)W, 3)
uint8.  Every case is Z = 4, H = 6, W = 7 with a 1-channel task and a 3-channel task, all values finite:
  0  seeded noise;
  1  the edges of the range test: a constant slice, a slice of range 5e-7 and one of range 2e-6 (either side of the 1e-6 test);
  2  a 1-channel `activation: sigmoid` task whose prediction the reference draws through a second sigmoid: logits whose sigmoid
     spans more than 0.1 in every slice.
Needs the reference tree at generation time only."""
import importlib
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "preview.npz")
Z, H, W = 4, 6, 7
CAPTURED = []


def _stubs():
    cv2 = types.ModuleType("cv2")
    cv2.COLOR_GRAY2BGR = 8

    def cvtColor(img, code):
        assert code == cv2.COLOR_GRAY2BGR and img.ndim == 2
        return np.repeat(img[:, :, None], 3, axis=2)
    cv2.cvtColor = cvtColor
    imageio = types.ModuleType("imageio")

    def mimsave(path, frames, fps=None, **kw):
        CAPTURED.append(np.stack([np.asarray(f) for f in frames]))
    imageio.mimsave = mimsave
    tb = types.ModuleType("torch.utils.tensorboard")
    tb.SummaryWriter = type("SummaryWriter", (), {})
    return {"cv2": cv2, "imageio": imageio, "tifffile": types.ModuleType("tifffile"), "torch.utils.tensorboard": tb}


def load_reference_plotting(ref_root):
    """the reference's plotting.py as a module, with its absent third-party imports stubbed; imageio is always the capturing stub"""
    sys.dont_write_bytecode = True
    for name, stub in _stubs().items():
        if name != "imageio":
            try:
                importlib.import_module(name)
                continue
            except Exception:
                pass
        sys.modules[name] = stub
    spec = importlib.util.spec_from_file_location("ref_plotting", os.path.join(ref_root, "training", "visualization", "plotting.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    return ref


def cases():
    """(image, targets, preds, tasks)"""
    out = []
    rng = np.random.default_rng(2024)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    plain = {"normals": {"activation": "none"}, "sheet": {"activation": "none"}}
    out.append((f(1, 1, Z, H, W), {"sheet": f(1, 1, Z, H, W), "normals": f(1, 3, Z, H, W)},
                {"sheet": f(1, 1, Z, H, W), "normals": f(1, 3, Z, H, W)}, plain))
    image, ts, tn, ps, pn = f(1, 1, Z, H, W), f(1, 1, Z, H, W), f(1, 3, Z, H, W), f(1, 1, Z, H, W), f(1, 3, Z, H, W)
    image[0, 0, 0] = np.float32(0.25)                                             # a constant slice
    ts[0, 0, 1] = (rng.random((H, W)) * 5e-7).astype(np.float32)
    ts[0, 0, 1, 0, 0], ts[0, 0, 1, 0, 1] = 0.0, np.float32(5e-7)                    # range 5e-7: below the test
    ts[0, 0, 2] = (rng.random((H, W)) * 2e-6).astype(np.float32)
    ts[0, 0, 2, 0, 0], ts[0, 0, 2, 0, 1] = 0.0, np.float32(2e-6)                    # range 2e-6: above it
    pn[0, 1, 3] = np.float32(-1.5)                                                # one constant channel slice of the 3-channel panel
    tn[0, 2, 0] = (rng.random((H, W)) * 5e-7).astype(np.float32) + np.float32(1.0)  # a tiny range away from zero
    ps[0, 0, 2] = 0.0
    out.append((image, {"sheet": ts, "normals": tn}, {"sheet": ps, "normals": pn}, plain))
    logits = (f(1, 1, Z, H, W) * np.float32(2.0)).astype(np.float32)
    logits[0, 0, :, 0, 0], logits[0, 0, :, 0, 1] = -2.0, 2.0                        # every slice spans at least 0.76 after the sigmoid
    out.append((f(1, 1, Z, H, W), {"sheet": (f(1, 1, Z, H, W) > 0).astype(np.float32), "normals": f(1, 3, Z, H, W)},
                {"sheet": logits, "normals": f(1, 3, Z, H, W)},
                {"normals": {"activation": "none"}, "sheet": {"activation": "sigmoid"}}))
    return out


def main():
    ref_root = os.environ.get("RX_REFERENCE_ROOT")
    if not ref_root:
        sys.exit("set RX_REFERENCE_ROOT to the reference checkout")
    import contextlib
    import io
    import tempfile
    import torch
    ref = load_reference_plotting(ref_root)
    arrays = {}
    all_cases = cases()
    for i, (image, targets, preds, tasks) in enumerate(all_cases):
        del CAPTURED[:]
        with contextlib.redirect_stdout(io.StringIO()), tempfile.TemporaryDirectory() as tmp:      # (it creates the GIF's directory)
            ref.save_debug_gif(torch.from_numpy(image), {k: torch.from_numpy(v) for k, v in targets.items()},
                               {k: torch.from_numpy(v) for k, v in preds.items()}, tasks, epoch=0,
                               save_path=os.path.join(tmp, "debug.gif"))
        assert len(CAPTURED) == 1
        frames = CAPTURED[0]
        assert frames.dtype == np.uint8 and frames.shape == (Z, 2 * H, 3 * W, 3), (frames.dtype, frames.shape)
        arrays[f"image_{i}"] = image
        for k in targets:
            assert np.isfinite(targets[k]).all() and np.isfinite(preds[k]).all()
            arrays[f"target_{i}_{k}"] = targets[k]
            arrays[f"pred_{i}_{k}"] = preds[k]
        arrays[f"sigmoid_{i}"] = np.array(sorted(k for k, v in tasks.items() if v["activation"] == "sigmoid"), dtype="U16")
        arrays[f"frames_{i}"] = frames
    arrays["n_cases"] = np.array(len(all_cases), np.int64)
    np.savez_compressed(OUT, **arrays)
    size = os.path.getsize(OUT)
    print(OUT, size, "bytes")
    assert size < 256 * 1024


if __name__ == "__main__":
    main()
