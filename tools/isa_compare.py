"""Function-by-function comparison of two device assembly listings of csrc/rollout.hip (a refactor's proof that no kernel changed).

Make the listings with the flags of d3il_amd/build.py without -shared, plus `--cuda-device-only -S -o <file>.s`, once per tree, then
    python tools/isa_compare.py parent.s tree.s
A function body is the text between `.type <name>,@function` and its `.Lfunc_end` label with comments and blank lines stripped.  Local labels carry the index of
their function in the translation unit (`.LBB<index>_<block>`); moving a function renumbers them, so that index is replaced by a fixed token - which is all the
normalisation there is, and the label's block number stays.  Prints the symbol sets' difference and every function whose body differs; exit status 1 if any does."""
import re
import sys


def functions(path):
    """name -> normalised body lines, in file order."""
    out, name, body = {}, None, None
    for line in open(path):
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if re.match(r"\s*\.Lfunc_end\d+:", line):
            out[name], name = body, None
            continue
        line = re.sub(r"\s*;.*", "", line).strip()      # comments (after the instruction or on a line of their own)
        if line:
            body.append(re.sub(r"\.LBB\d+_", ".LBB#_", line))
    return out


def main():
    a, b = functions(sys.argv[1]), functions(sys.argv[2])
    kernels = [set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", open(p).read(), re.M)) for p in sys.argv[1:3]]
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    differ = [n for n in a if n in b and a[n] != b[n]]
    print("functions: %d / %d (kernels: %d / %d), %d / %d body lines" % (len(a), len(b), len(kernels[0]), len(kernels[1]), sum(len(v) for v in a.values()),
                                                                        sum(len(v) for v in b.values())))
    if kernels[0] != kernels[1]:
        print("kernel sets differ: %s" % sorted(kernels[0] ^ kernels[1]))
    for n in only_a:
        print("only in %s: %s" % (sys.argv[1], n))
    for n in only_b:
        print("only in %s: %s" % (sys.argv[2], n))
    for n in differ:
        first = next((i for i, (x, y) in enumerate(zip(a[n], b[n])) if x != y), min(len(a[n]), len(b[n])))
        print("differs: %s (%d / %d lines, first difference at line %d)" % (n, len(a[n]), len(b[n]), first))
    same = not (only_a or only_b or differ) and kernels[0] == kernels[1]
    print("identical: same symbols, every body equal" if same else "NOT identical")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
