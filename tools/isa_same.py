"""Are two gfx950 assembly listings (hipcc -S --cuda-device-only) the same device code, function by function?

    python tools/isa_same.py parent.s this.s

Splits each listing into one block per @function symbol and one amdhsa.kernels metadata entry per kernel
(register counts, LDS and scratch sizes, the kernel-argument layout), replaces what depends on a function's
position in the file (the ordinal in local labels) and on the source text's hash (__hip_cuid_), and compares by
symbol name, so moved or reordered source compares equal. Prints the number of functions and the names that
differ; exits 1 on any difference.
"""
import re
import sys


def blocks(path):
    text = open(path).read()
    text = re.sub(r"\.(LBB|Lfunc_begin|Lfunc_end|LJTI|Ltmp)\d+", r".\1N", text)
    text = re.sub(r"__hip_cuid_\w+", "__hip_cuid_", text)
    # a function's block: its code, kernel descriptor, .set lines and "Kernel info" up to the next .text
    funcs = {m.group(1): m.group(2) for m in re.finditer(
        r"^\t\.type\t(\S+),@function\n(.*?^\.Lfunc_endN:\n.*?)(?=^\t\.text\n|^\t\.section\t(?!\.AMDGPU\.csdata))",
        text, re.M | re.S)}
    meta = {}
    md = text[text.find("amdhsa.kernels:"):text.find("amdhsa.target:")]
    for entry in re.split(r"^  - ", md, flags=re.M)[1:]:
        meta[re.search(r"^ {4}\.name: +(\S+)", entry, re.M).group(1)] = entry
    return funcs, meta


def main():
    (fa, ma), (fb, mb) = blocks(sys.argv[1]), blocks(sys.argv[2])
    print("functions: %d and %d, metadata entries: %d and %d" % (len(fa), len(fb), len(ma), len(mb)))
    bad = 0
    for what, a, b in (("function", fa, fb), ("metadata entry", ma, mb)):
        only = sorted(set(a) ^ set(b))
        differ = sorted(k for k in set(a) & set(b) if a[k] != b[k])
        print("%s names in one listing only: %s" % (what, only or "none"))
        print("%s differs: %s" % (what, differ or "none"))
        bad += len(only) + len(differ)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
