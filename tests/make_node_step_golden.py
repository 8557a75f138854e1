"""Writes tests/golden/node_step_counters.json: the counters of the frames and of the ray batch in test_gpu_node_step.py, as
the library in use reports them -- recorded from the build BEFORE a change of the node step, which the build after it must
reproduce (needs a GPU; RAYCA_HIP_LIB picks another build of the library than the tree's).
usage: python tests/make_node_step_golden.py [output path]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import node_step_cases as N   # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else N.GOLDEN
json.dump({"frames": {name: N.frame_counters(name) for name in N.SPILL_SCENES}, "table_rays": N.table_counters()},
          open(out, "w"), indent=1, sort_keys=True)
print("wrote", out)
