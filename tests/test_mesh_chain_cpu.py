"""CPU: the mesh chain on the host -- extract, refine, decimate, orient through the drivers with the numpy statements -- writes the
files and returns the summaries that tests/data/mesh_chain_digests.json records, in both formats, with and without normals."""
import mesh_chain


def test_host_chain_writes_the_recorded_bytes(tmp_path):
    got, want = mesh_chain.run(tmp_path, device=False), mesh_chain.recorded()
    assert sorted(got) == sorted(want) and len(got) == 4
    for name in want:
        assert len(want[name]["files"]) == 7 and got[name] == want[name], name
