"""Did a change touch any kernel?  Compares the gfx950 instruction listings of one translation unit between two sides, symbol by symbol.
usage: python tests/kernel_isa_diff.py SIDE_A SIDE_B [--unit kernels|refill|bvh_build] [hipcc flags ...]
A side is a source tree (a directory with rayca_amd/csrc in it: its <unit>.hip is compiled device-only, with the flags of build(),
as tests/kernel_resources.py does -- the flags of THIS tree's build() for both sides, not each side's own: compare trees whose flags are
equal, or hand over code objects) or a gfx950 code object (a file).  Reports the symbols that only one side has and the symbols
whose listing differs, and exits 1 if there is any of either.  The order of the symbols in .text does not count -- the compiler emits
template instantiations in the order the host code first names them -- and neither do addresses: the comparison is of text, per symbol,
and knows nothing about particular instructions."""
import os, re, subprocess, sys, tempfile
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_resources import LLVM, compile_device, unbundle

HEADER = re.compile(r"^[0-9a-f]+ <(.+)>:\s*$")


def code_object(side, unit, flags, tmp, tag):
    if os.path.isfile(side):
        return side
    src = os.path.join(side, "rayca_amd", "csrc", unit + ".hip")
    if not os.path.isfile(src):
        sys.exit(f"{side}: neither a code object nor a tree with {os.path.relpath(src, side)}")
    out = os.path.join(tmp, f"{tag}_{unit}.o")
    compile_device(src, out, flags)
    return unbundle(out)


def listings(co):
    """symbol -> its instruction lines, without addresses and encodings"""
    text = subprocess.run([LLVM + "llvm-objdump", "-d", "--no-show-raw-insn", co], capture_output=True, text=True, check=True).stdout
    syms, cur = {}, None
    for line in text.splitlines():
        m = HEADER.match(line)
        if m:
            cur = syms.setdefault(m.group(1), [])
        elif cur is not None and line.strip() not in ("", "..."):   # ("...": objdump's mark for the zero padding up to the next symbol)
            cur.append(re.sub(r"\s*//.*$", "", line).strip())
    return syms


def main(argv):
    unit = "kernels"
    if "--unit" in argv:
        i = argv.index("--unit")
        unit = argv[i + 1]
        del argv[i:i + 2]
    if len(argv) < 2:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory(prefix="rayca_isa_") as tmp:
        a, b = (listings(code_object(side, unit, argv[2:], tmp, tag)) for side, tag in ((argv[0], "a"), (argv[1], "b")))
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    differ = sorted(s for s in set(a) & set(b) if a[s] != b[s])
    for title, names in (("only in " + argv[0], only_a), ("only in " + argv[1], only_b), ("listing differs", differ)):
        for s in names:
            extra = f"  ({len(a[s])} -> {len(b[s])} instructions)" if names is differ else ""
            print(f"{title}: {s}{extra}")
    print(f"{unit}.hip: {len(a)} and {len(b)} symbols, {sum(map(len, a.values()))} and {sum(map(len, b.values()))} instructions; "
          f"{len(only_a)} only in the first, {len(only_b)} only in the second, {len(differ)} with a different listing")
    return 1 if only_a or only_b or differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
