"""The host-side scene build on the CPU (no GPU needed: the BLAS is built by the host builder).
usage: RAYCA_BUILD_TIMING=1 python tests/host_build_probe.py [atrium|soup|cornell] [repeats]      phase times on stderr
       python tests/host_build_probe.py digests CASE [LIBRARY]       digests of one case of CASES, both builders, as JSON
(test_host_build_cpu.py compiles the probe once and runs the second form in a child process per case; compile_probe(so, source)
builds against another host_scene.cpp, for A/B timing of two versions of the builder.)"""
import ctypes as C, json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
HOST_SCENE = os.path.join(ROOT, "rayca_amd", "csrc", "host_scene.cpp")
DEFAULT_SO = os.path.join(ROOT, "tests", "cpp", "_build", "libhost_build_probe.so")


def compile_probe(so=DEFAULT_SO, source=HOST_SCENE):
    os.makedirs(os.path.dirname(so), exist_ok=True)
    subprocess.run(["g++", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-pthread", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "host_build_probe.cpp"), source, "-o", so], check=True)
    return so


def _sdtf_scene(name):
    from rayca_amd import model, sdtf
    scene = model.Scene()
    sdtf.push_sdtf_from_path(scene, os.path.join(GOLDEN, name))
    return scene


def _cases():
    from rayca_amd import scenes
    # name -> (scene, use_bvh)
    return {
        "cornell": (scenes.cornell_scene, True),                                # 22 binary nodes under the SAH builder
        "cornell_quad": (lambda: _sdtf_scene("cornell_quad.sdtf"), True),       # a quad light's two triangles; a tree of a few nodes
        "spheres": (lambda: _sdtf_scene("spheres.sdtf"), True),
        "cornell_quad_flat": (lambda: _sdtf_scene("cornell_quad.sdtf"), False),  # one leaf of all primitives
        "soup200_flat": (lambda: scenes.soup_scene(200), False),                # one leaf above 64 primitives: a chain of four links
        "atrium4": (lambda: scenes.atrium_scene(4), True),                      # ~10^4 binary nodes
        "atrium14": (lambda: scenes.atrium_scene(14), True),                    # 135 379 binary nodes: the parallel 4-wide collapse
    }


CASES = ["cornell", "cornell_quad", "spheres", "cornell_quad_flat", "soup200_flat", "atrium4", "atrium14"]
BUILDERS = {"reference": 0, "sah": 1}   # abi.BUILDER_REFERENCE, abi.BUILDER_SAH


def digests(lib, case):
    """{builder: {item: value}} of one case: what host_build_digests (cpp/host_build_probe.cpp) writes, one build per builder"""
    from rayca_amd import flatten
    make, use_bvh = _cases()[case]
    desc = flatten(make())
    lib.host_build_digests.argtypes = [C.c_void_p, C.c_uint, C.c_int, C.c_char_p, C.c_size_t]
    out = {}
    for name, builder in BUILDERS.items():
        buf = C.create_string_buffer(1 << 16)
        rc = lib.host_build_digests(C.cast(desc.ptr(), C.c_void_p), builder, int(use_bvh), buf, len(buf))
        if rc:
            raise RuntimeError(f"host_build_digests({case}, {name}) returned {rc}")
        out[name] = dict(line.split(" ") for line in buf.value.decode().splitlines())
    return out


def main(argv):
    if argv[:1] == ["digests"]:
        so = argv[2] if len(argv) > 2 else compile_probe()
        print(json.dumps(digests(C.CDLL(so), argv[1]), sort_keys=True))
        return 0
    from rayca_amd import abi, flatten, scenes
    lib = C.CDLL(compile_probe())
    which = argv[0] if argv else "atrium"
    desc = flatten({"atrium": scenes.atrium_scene, "cornell": scenes.cornell_scene}.get(which, lambda: scenes.soup_scene(1_000_000))())
    lib.host_build_probe.argtypes = [C.c_void_p, C.c_uint, C.c_int]
    return lib.host_build_probe(C.cast(desc.ptr(), C.c_void_p), abi.BUILDER_SAH, int(argv[1]) if len(argv) > 1 else 3)


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
