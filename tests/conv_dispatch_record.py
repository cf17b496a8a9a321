"""The recording behind tests/data/conv_dispatch.json: per ledger shape and dtype (test_conv_dispatch_gpu.py::test_ledger_row), and per
pinned case of test_ops_gpu.py (PINNED below), the kernel rx_last_conv_kernel() names at every entry point and a SHA-256 of the
output that call wrote -- y, dx, dx += and dw of the seeded random pass, whose operands are generated on the CPU.

scripts/record_conv_dispatch.py writes the file (at the commit whose behaviour is to be pinned, twice) and replays all of it with
--check; test_ledger_row replays its own part on every run, through note().  A changed split count changes the order in which
random fp data is summed, so an unchanged digest pins ks / S on hardware -- evidence, not proof.  A null digest was not reproducible
between the two recording runs and is pinned by name only."""
import hashlib
import json
import os

import torch

import conv_dispatch_cases as L

JSON_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "conv_dispatch.json")
RECORDING = None            # the recorder sets a dict: note() then fills it and compares nothing
_LOADED = {}

# the CONV_CASES whose kernels test_conv3d_fwd_bwd pins and the two CONVT_CASES test_convT3d_fwd_bwd asserts a name on (n = 2 there)
PINNED = {f"conv{i}": L.Shape("conv", 2, *c, L.ALL) for i, c in enumerate(
    (L.P_A, L.P_B1, L.P_C, L.P_F1, L.P_F512, L.P_F388, L.P_S2, L.P_S2R, L.P_PW))}
PINNED.update({f"convT{i}": L.Shape("convT", 2, ci, co, dims, None, s, L.ALL) for i, (ci, co, dims, s) in enumerate(
    ((64, 32, (12, 18, 20), L.S2), (64, 32, (16, 32, 40), L.S2)))})


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def recorded():
    if not _LOADED:
        with open(JSON_PATH) as f:
            _LOADED.update(json.load(f)["cases"])
    return _LOADED


def note(case, entry, kernel, out):
    """one call of `entry` in `case` ("<shape key>-<dtype>") named `kernel` and wrote the tensor `out`"""
    digest = sha(out)
    if RECORDING is not None:
        RECORDING.setdefault(case, {})[entry] = {"kernel": kernel, "sha": digest}
        return
    was = recorded()[case][entry]
    assert kernel == was["kernel"], f"{case} {entry}: {kernel}, recorded {was['kernel']}"
    assert was["sha"] in (None, digest), f"{case} {entry} ({kernel}): the output's bits differ from the recording"
