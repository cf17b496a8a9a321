"""GPU: the mesh chain through the HIP kernels -- extract, refine, decimate, orient through the drivers on the device -- writes the
files and returns the summaries that the host statements recorded in tests/data/mesh_chain_digests.json."""
import pytest

import mesh_chain

pytestmark = pytest.mark.gpu


def test_device_chain_writes_the_recorded_bytes(tmp_path):
    got, want = mesh_chain.run(tmp_path, device=True), mesh_chain.recorded()
    assert sorted(got) == sorted(want) and len(got) == 4
    for name in want:
        assert len(want[name]["files"]) == 7 and got[name] == want[name], name
