"""Device functions left in a unit's gfx950 code object besides its kernels: every one of them is the target of a real call.
The functions of the RAYCA_NO_PK_F32 region (rayca_amd/csrc/no_pk.hpp) are compiled for other target features than the
runtime's and the device library's, and what does not share them does not inline -- silently.  There must be none.
usage: python tests/device_calls.py [extra hipcc flags ...]   (compiles kernels.hip and refill.hip device-only into /tmp;
exit status 1 if a function is left)"""
import os, re, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g
LLVM = "/opt/rocm/lib/llvm/bin/"
left = 0
for unit in ("kernels", "refill"):
    out = f"/tmp/rayca_{unit}_calls.o"
    subprocess.run([g.HIPCC, "--offload-arch=gfx950", "--cuda-device-only", *g.COMMON, *sys.argv[1:], "-c", os.path.join(g.CSRC, unit + ".hip"), "-o", out], check=True)
    subprocess.run([LLVM + "clang-offload-bundler", "--unbundle", "--type=o", "--input=" + out, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                    "--output=" + out + ".co"], check=True)
    syms = subprocess.run([LLVM + "llvm-readelf", "--symbols", "-W", out + ".co"], capture_output=True, text=True, check=True).stdout
    rows = [ln.split() for ln in syms.splitlines() if re.match(r"\s*\d+:", ln)]
    names = {r[7] for r in rows if len(r) > 7 and r[6] != "UND"}
    funcs = sorted(r[7] for r in rows if len(r) > 7 and r[3] == "FUNC" and r[6] != "UND" and r[7] + ".kd" not in names)
    kernels = sum(1 for n in names if n.endswith(".kd"))
    print(f"{unit}.hip: {kernels} kernels, {len(funcs)} other device functions")
    for f in funcs:
        print("   ", subprocess.run(["c++filt", f], capture_output=True, text=True).stdout.strip())
    left += len(funcs)
sys.exit(1 if left else 0)
