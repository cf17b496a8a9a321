"""GPU (-m gpu): the stride-1 3x3x3 conv entry points dispatch and compute what they did when tests/data/conv_halo_dispatch.json was
recorded (scripts/record_conv_halo_dispatch.py, at the commit before the selector of csrc/rx_conv_halo_plan.h existed): the same
kernel family, the same `fused` answer, the same refusal, and every output bit for bit (SHA-256).  The inputs are random floats, so a
persistent grid that split its tiles differently would change the fused sums' bits.  A digest recorded as null (not reproducible
between two runs of the recording) pins name and flag only."""
import pytest

import conv_halo_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    import mt3d_amd  # noqa: F401
    from mt3d_amd.engine import lib, ops as _ops
    lib.require_device()
    return _ops


@pytest.fixture(scope="module")
def recorded():
    return C.recorded()


@pytest.mark.parametrize("cid", C.case_ids())
def test_dispatch_and_bits_as_recorded(ops, recorded, cid):
    want = recorded[cid]
    got = C.run(ops, cid)
    assert got["kernel"] == want["kernel"]
    assert got.get("fused") == want.get("fused") and got.get("raises") == want.get("raises")
    assert sorted(got["sha"]) == sorted(want["sha"])
    for name, digest in want["sha"].items():
        if digest is not None:
            assert got["sha"][name] == digest, name
