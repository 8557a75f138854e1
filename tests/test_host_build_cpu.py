"""Everything build_host_scene leaves behind, digest by digest, against a record (golden/host_build_digests.json).

The record pins a refactor of the host build: it was taken from the builder as it stood at the commit the file names
(`recorded_from`), before the build was cut into phases and the recursive BLAS layout removed, and the arrays have to come
out byte for byte as they did then.  It does NOT say what a correct tree is -- test_oracle_bvh.py, test_builder_edges_cpu.py
and the literal builder do that.  A change that alters a layout on purpose re-records the file (the digests of
`python tests/host_build_probe.py digests CASE`, at RAYCA_HOST_THREADS=1 and =16) and says so; nothing else is needed.

Cases (host_build_probe.py), each under both builders: the Cornell room (22 binary nodes under SAH) and the one with a quad
light, a scene of spheres, the quad-light Cornell and a soup of 200 triangles without a BVH (one leaf; the soup's is a chain
of 64-primitive links), and the atrium at detail 4 (9 997 binary nodes) and 14 (135 379, and 67 482 4-wide nodes: above the
threshold of the parallel 4-wide collapse).  Each case runs in a process of its own, on one host thread and -- the atrium --
on sixteen: the count is set, not left to the machine, because the numbering of the reference tree's leaves (`ref_leaf_boxes`,
`ref_leaf_of`) follows the arena, and the arena's order follows the number of threads the builder may split across.
`ref_leaf_box_of_slot` is the same information without the numbering and is the same at every count."""
import json
import os
import subprocess
import sys

import pytest

import host_build_probe as probe

with open(os.path.join(probe.GOLDEN, "host_build_digests.json")) as f:
    RECORD = json.load(f)["cases"]


@pytest.fixture(scope="module")
def probe_so(tmp_path_factory):
    return probe.compile_probe(str(tmp_path_factory.mktemp("host_build_probe") / "libhost_build_probe.so"))


def test_the_record_covers_every_case():
    assert sorted(RECORD) == sorted(probe.CASES)
    sah = RECORD["atrium14"]["16"]["sah"]
    assert (sah["dev_nodes.count"], sah["dev_nodes4.count"]) == ("135379", "67482")
    assert RECORD["cornell"]["1"]["sah"]["dev_nodes.count"] == "22" and RECORD["atrium4"]["1"]["sah"]["dev_nodes.count"] == "9997"


# (every case on one thread; on sixteen the large ones, where the threads have something to split: the file stays near 20 s)
RUNS = [(case, "1") for case in probe.CASES] + [(case, "16") for case in ("atrium4", "atrium14")]


@pytest.mark.parametrize("case,threads", RUNS)
def test_host_build_gives_the_recorded_digests(probe_so, case, threads):
    env = dict(os.environ, RAYCA_HOST_THREADS=threads)
    run = subprocess.run([sys.executable, os.path.join(probe.ROOT, "tests", "host_build_probe.py"), "digests", case, probe_so], env=env,
                         check=True, capture_output=True, text=True)
    got = json.loads(run.stdout)
    want = RECORD[case][threads]
    for builder in sorted(want):
        differ = {k: (got[builder].get(k), v) for k, v in want[builder].items() if got[builder].get(k) != v}
        assert not differ and sorted(got[builder]) == sorted(want[builder]), (case, builder, differ)
    for builder in sorted(want):   # (the leaves' numbering aside, the reference tables do not depend on the thread count)
        assert want[builder]["ref_leaf_box_of_slot"] == RECORD[case]["1"][builder]["ref_leaf_box_of_slot"]
