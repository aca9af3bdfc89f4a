#!/usr/bin/env python3
"""Compare two device assembly listings (hipcc --cuda-device-only -S) function by function.

    tools/isa_diff.py [--diff | --classify] old.s new.s

Prints one line per function -- same / changed / removed / added -- and exits
non-zero unless every function is the same.  A function's text is its code,
its kernel descriptor and its metadata entry.  Ignored, because they differ
between builds of identical code: assembler comments (they carry basic-block
numbers), the __hip_cuid_<hex> symbol, and the per-file function index inside
.LBB<n>_, .LJTI<n>_, .Lfunc_begin<n> and .Lfunc_end<n> labels (it shifts when
a function before it is added or removed).
--diff      also prints the differing lines of each changed function.
--classify  also counts them by kind: "immediate" lines are equal once
            numeric literals (not register numbers) are masked, counted per
            mnemonic or key; if the masked texts differ too, the function is
            marked STRUCTURE DIFFERS (other instructions, registers or order).
Text only: no GPU, no network.
"""
import collections
import difflib
import re
import sys

OWNER = re.compile(r"\s*(?:\.section\s+\.text\.|\.type\s+|\.amdhsa_kernel\s+)([\w$.]+?)(?:,.*)?$")
INDEX = re.compile(r"\.(LBB|LJTI|Lfunc_begin|Lfunc_end)\d+")
LITERAL = re.compile(r"(?<![\w\[])(?:0x[0-9a-fA-F]+|\d+)(?![\w\]:])")  # 0x2b0, offset:16, 704; not v12, s[4:5]


def functions(path):
    """{function name: its lines}; what belongs to no function is under "(file)"."""
    out, cur, entries, meta = collections.defaultdict(list), "(file)", [], False
    for line in open(path):
        line = INDEX.sub(r".\1", re.sub(r"__hip_cuid_\w+", "__hip_cuid", line.split(";")[0])).rstrip()
        if not line:
            continue
        if ".amdgpu_metadata" in line:
            meta, cur = not meta, "(file)"
        elif meta and line.startswith("  - "):  # an entry of amdhsa.kernels: named after the loop
            entries.append([])
            cur = None
        elif meta and line[0] != " ":           # a top-level key
            cur = "(file)"
        elif not meta and ".AMDGPU.gpr_maximums" in line:
            cur = "(file)"
        elif not meta and "@object" not in line and OWNER.match(line):
            cur = OWNER.match(line).group(1)
        (entries[-1] if cur is None else out[cur]).append(line)
    for e in entries:  # a kernel's own name is at depth 4 (its arguments' names are deeper); other lists have none
        out[next((l.split()[1] for l in e if l.startswith("    .name:")), "(file)")] += e
    return out


def classify(old, new):
    if [LITERAL.sub("N", l) for l in old] != [LITERAL.sub("N", l) for l in new]:
        return ["STRUCTURE DIFFERS"]
    kinds = collections.Counter(a.replace("- ", "").split()[0] for a, b in zip(old, new) if a != b)
    return [f"{n:4d} x immediate of {k}" for k, n in sorted(kinds.items())]


def main(argv):
    flags = [a for a in argv if a.startswith("--")]
    paths = [a for a in argv if not a.startswith("--")]
    if len(paths) != 2 or any(f not in ("--diff", "--classify") for f in flags):
        sys.exit(__doc__)
    old, new = (functions(p) for p in paths)
    n = {"same": 0, "changed": 0, "removed": 0, "added": 0}
    for f in list(old) + [f for f in new if f not in old]:
        s = "removed" if f not in new else "added" if f not in old else "same" if old[f] == new[f] else "changed"
        n[s] += 1
        print(f"{s:8} {f}")
        if s == "changed" and "--diff" in flags:
            for d in difflib.unified_diff(old[f], new[f], "old", "new", n=0, lineterm=""):
                print("    " + d)
        if s == "changed" and "--classify" in flags:
            for c in classify(old[f], new[f]):
                print("        " + c)
    print(", ".join(f"{v} {k}" for k, v in n.items()))
    return 0 if n["same"] == sum(n.values()) else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
