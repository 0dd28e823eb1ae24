#!/usr/bin/env python3
"""Compare two device-assembly files (hipcc --cuda-device-only -S) kernel by kernel.

    python tools/isa_diff.py parent.s new.s [-v]

Per kernel symbol: `identical` (the same instruction text once comment and directive lines are dropped),
`scalar-only` (the same sequence of non-scalar instructions -- s_waitcnt / s_barrier included, SGPR names masked)
or `different`; both instruction counts; whether the .amdhsa_ resource fields agree.  Exit status 1 when a kernel is
missing on either side or a resource field differs.  Text comparison only: for source-only refactors of a kernel file.
"""
import re
import sys

FIELDS = ("next_free_vgpr", "next_free_sgpr", "accum_offset", "group_segment_fixed_size", "private_segment_fixed_size")
SGPR = re.compile(r"\b(s\[\d+:\d+\]|s\d+|vcc(_lo|_hi)?|ttmp\d+|m0)\b")


def parse(path):
    """-> {kernel: (instruction lines, {resource field: value})}"""
    body, res, cur, desc = {}, {}, None, None
    for raw in open(path, errors="replace"):
        line = raw.split(";", 1)[0].strip()      # (a `;` starts a comment; no string operands in device code)
        if not line:
            continue
        if line.startswith(".amdhsa_kernel "):
            desc = line.split()[1]
            res[desc] = {}
        elif line == ".end_amdhsa_kernel":
            desc = None
        elif desc is not None:
            m = re.match(r"\.amdhsa_(\w+)\s+(\S+)", line)
            if m and m.group(1) in FIELDS:
                res[desc][m.group(1)] = m.group(2)
        elif re.match(r"\.type\s+\S+,@function", line):
            cur = line.split()[1].split(",")[0]
            body[cur] = []
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None and not (line.startswith(".") and not line.endswith(":")) and line != cur + ":":
            body[cur].append(line)               # instructions and block labels
    return {k: (body.get(k, []), res[k]) for k in res}


def vector_view(lines):
    keep = []
    for l in lines:
        op = l.split()[0]
        if l.endswith(":") or (op.startswith("s_") and op not in ("s_waitcnt", "s_barrier")):
            continue
        keep.append(SGPR.sub("S", l))
    return keep


def count(lines):
    return sum(not l.endswith(":") for l in lines)


def main(argv):
    verbose = "-v" in argv
    paths = [a for a in argv if a != "-v"]
    if len(paths) != 2:
        sys.exit(__doc__)
    old, new = parse(paths[0]), parse(paths[1])
    tally, bad = {"identical": 0, "scalar-only": 0, "different": 0}, 0
    for k in sorted(set(old) | set(new)):
        if k not in old or k not in new:
            print(f"MISSING in {'parent' if k not in old else 'new'}: {k}")
            bad += 1
            continue
        (lo, ro), (ln, rn) = old[k], new[k]
        kind = "identical" if lo == ln else "scalar-only" if vector_view(lo) == vector_view(ln) else "different"
        tally[kind] += 1
        res_ok = ro == rn
        bad += not res_ok
        if verbose or kind != "identical" or not res_ok:
            print(f"{kind:11s} {count(lo):6d} {count(ln):6d}  resources {'equal' if res_ok else f'DIFFER {ro} -> {rn}'}  {k}")
    print(f"{len(old)} / {len(new)} kernels: " + ", ".join(f"{v} {k}" for k, v in tally.items())
          + f"; {bad} missing or with other resource fields")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
