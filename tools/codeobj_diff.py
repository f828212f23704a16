"""Are two builds of a library the same device code?  (CPU only; LABBOOK 16's method.)

    python3 tools/codeobj_diff.py PARENT_LIB NEW_LIB

Unbundles the gfx950 code object of both libraries (shipped_isa.extract) and compares: the set of kernel symbols; each
kernel's metadata (VGPR, SGPR, LDS, scratch); each kernel's disassembly with the `// address: encoding` comments and the
branch-target offsets stripped; and the exported names (`nm -D --defined-only`, the `__hip_cuid_<hash>` word apart: it
carries the hash of its own build).  Prints the counts and, per differing kernel, the instruction index and the first
differing pair of lines.  Exit status 0: no difference; 1: any.
"""
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import shipped_isa  # noqa: E402

LLVM = shipped_isa.LLVM
META = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")


def run(*cmd):
    return subprocess.run(cmd, capture_output=True, text=True, check=True).stdout


def kernels(lib):
    """symbol -> (metadata tuple, [instruction lines]) of every kernel in the library's gfx950 code object."""
    co = shipped_isa.extract(lib)
    meta = {}
    for blk in re.split(r"\n\s*- \.agpr_count:", run(os.path.join(LLVM, "llvm-readelf"), "--notes", co))[1:]:
        name = re.search(r"\.symbol:\s+(\S+)\.kd", blk)
        if name:
            meta[name.group(1)] = tuple(int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1)) for k in META)
    text = {}
    for m in re.finditer(r"^[0-9a-f]+ <(\S+)>:\n(.*?)(?=^\n|\Z)", run(os.path.join(LLVM, "llvm-objdump"), "-d", co), re.S | re.M):
        lines = [l.split("//")[0].strip() for l in m.group(2).splitlines()]
        text[m.group(1)] = [re.sub(r"\s+<[^>]*>$", "", re.sub(r"(s_c?branch\S*)\s+\d+", r"\1", l)) for l in lines if l]
    return {s: (meta[s], text.get(s, [])) for s in meta}


def exported(lib):
    names = [l.split()[-1] for l in run("nm", "-D", "--defined-only", lib).splitlines() if l.strip()]
    return sorted(n for n in names if not n.startswith("__hip_cuid_"))


def first_difference(a, b):
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return i, x, y
    i = min(len(a), len(b))
    return i, a[i] if i < len(a) else "(end)", b[i] if i < len(b) else "(end)"


def main(parent, new):
    ka, kb = kernels(parent), kernels(new)
    ea, eb = exported(parent), exported(new)
    only_a, only_b = sorted(set(ka) - set(kb)), sorted(set(kb) - set(ka))
    common = sorted(set(ka) & set(kb))
    meta_differ = [s for s in common if ka[s][0] != kb[s][0]]
    text_differ = [s for s in common if ka[s][1] != kb[s][1]]
    pretty = shipped_isa.demangle(only_a + only_b + sorted(set(meta_differ + text_differ)))
    print("kernel symbols: %d | %d, %d only in the first, %d only in the second" % (len(ka), len(kb), len(only_a), len(only_b)))
    for s in only_a:
        print("  only in %s: %s" % (parent, pretty[s]))
    for s in only_b:
        print("  only in %s: %s" % (new, pretty[s]))
    print("kernels whose metadata differ: %d" % len(meta_differ))
    for s in meta_differ:
        print("  %s: %s" % (pretty[s], ", ".join("%s %d | %d" % (k, x, y) for k, x, y in zip(META, ka[s][0], kb[s][0]) if x != y)))
    print("kernels whose text differs: %d" % len(text_differ))
    for s in text_differ:
        i, x, y = first_difference(ka[s][1], kb[s][1])
        print("  %s: %d | %d instructions, first at %d: `%s` | `%s`" % (pretty[s], len(ka[s][1]), len(kb[s][1]), i, x, y))
    print("exported names: %d | %d, %d only in the first, %d only in the second" % (len(ea), len(eb), len(set(ea) - set(eb)), len(set(eb) - set(ea))))
    for n in sorted(set(ea) - set(eb)):
        print("  only in %s: %s" % (parent, n))
    for n in sorted(set(eb) - set(ea)):
        print("  only in %s: %s" % (new, n))
    return 1 if only_a or only_b or meta_differ or text_differ or ea != eb else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
