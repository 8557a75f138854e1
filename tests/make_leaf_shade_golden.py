"""Writes tests/golden/leaf_shade_counters.json: the counters of the fused engine's frames in test_gpu_leaf_shade.py, as the
library in use reports them (needs a GPU; RAYCA_HIP_LIB picks another build of the library than the tree's).
usage: python tests/make_leaf_shade_golden.py [output path]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import leaf_shade_cases as L   # noqa: E402
import test_gpu_leaf_shade as T   # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(L.G, "leaf_shade_counters.json")
json.dump({name: T.frame_counters(name)[0] for name in L.FRAME_SCENES}, open(out, "w"), indent=1, sort_keys=True)
print("wrote", out)
