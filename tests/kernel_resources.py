"""Register / spill / scratch / LDS figures of every kernel, read from the gfx950 code object's metadata.
usage: python tests/kernel_resources.py [extra hipcc flags ...]   (compiles rayca_amd/csrc/kernels.hip device-only into /tmp;
RAYCA_KRES_UNIT=refill|bvh_build picks another translation unit)
compile_device() and unbundle() are also what tests/kernel_isa_diff.py compiles its two sides with."""
import os, re, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g
LLVM = "/opt/rocm/lib/llvm/bin/"


def compile_device(src, out, flags=()):
    """one translation unit, device pass only, with the flags of build()"""
    subprocess.run([g.HIPCC, "--offload-arch=gfx950", "--cuda-device-only", *g.COMMON, *flags, "-c", src, "-o", out], check=True)


def unbundle(obj):
    """the device-only object is still an offload bundle: take the gfx950 code object out of it"""
    co = obj + ".co"
    subprocess.run([LLVM + "clang-offload-bundler", "--unbundle", "--type=o", "--input=" + obj, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                    "--output=" + co], check=True)
    return co


def main():
    unit = os.environ.get("RAYCA_KRES_UNIT", "kernels")
    out = f"/tmp/rayca_{unit}_dev.o"
    if not os.environ.get("RAYCA_KRES_REUSE"):
        compile_device(os.path.join(g.CSRC, unit + ".hip"), out, sys.argv[1:])
    notes = subprocess.run([LLVM + "llvm-readelf", "--notes", unbundle(out)], capture_output=True, text=True, check=True).stdout
    rows = []
    for blk in notes.split("- .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        f = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
        dem = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
        dem = dem.replace("(anonymous namespace)::", "").replace("void rayca::", "").replace("rayca::", "")
        dem = re.sub(r"\(.*", "", dem)
        rows.append((dem, f("vgpr_count"), f("vgpr_spill_count"), f("sgpr_count"), f("sgpr_spill_count"), f("private_segment_fixed_size")))
    print(f"{'kernel':64s} vgpr vspill sgpr sspill scratch_B")
    for r in sorted(rows):
        print(f"{r[0]:64s} {r[1]:4d} {r[2]:6d} {r[3]:4d} {r[4]:6d} {r[5]:9d}")


if __name__ == "__main__":
    main()
