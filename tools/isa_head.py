#!/usr/bin/env python3
"""What a kernel does between its entry and its first vector-memory request.  usage: tools/isa_head.py file.s [name-filter ...] [-v]
For every kernel of a `hipcc -S --cuda-device-only` listing whose demangled name holds one of the filters: the scalar loads issued and the `s_waitcnt lgkmcnt`
waits met on the straight path from the entry to the first global / buffer / flat load (every such wait is a memory round trip with nothing else in flight), the
scalar loads issued only AFTER that first request, and the descriptor's kernarg preload length.  In a preload build the entry is the label behind the 256-byte
compatibility block that loads the head for firmware which does not preload.  -v prints the head's scalar-memory and wait instructions."""
import re
import subprocess
import sys


def kernels(path):
    cur, buf = None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur, buf = m.group(1), []
            continue
        if cur is not None:
            buf.append(line.rstrip("\n"))
            m = re.search(r"\.amdhsa_user_sgpr_kernarg_preload_length\s+(\d+)", line)
            if m:
                yield cur, buf, int(m.group(1))
                cur = None


def head(body, preload):
    """(scalar loads, lgkmcnt waits, instructions) from the entry up to the first vector load; scalar loads behind it up to the next wait on them"""
    start = 0
    if preload:                                   # skip the compatibility block: it ends at the first .p2align 8 / s_branch target
        for i, l in enumerate(body):
            if re.search(r"\.p2align\s+8", l):
                start = i + 1
                break
    loads = waits = 0
    lines = []
    first = None
    for i in range(start, len(body)):
        l = body[i].strip()
        if re.match(r"(global_load|buffer_load|flat_load|scratch_load)", l):
            first = i
            break
        if re.match(r"s_(buffer_)?load_", l):
            loads += 1; lines.append(l)
        elif re.match(r"s_waitcnt", l) and "lgkmcnt" in l:
            waits += 1; lines.append(l)
        elif re.match(r"s_(c)?branch|s_endpgm|s_barrier", l):
            lines.append(l)
    late = 0
    if first is not None:
        for l in body[first:]:
            l = l.strip()
            if re.match(r"s_(buffer_)?load_", l):
                late += 1
            elif re.match(r"s_waitcnt", l) and "lgkmcnt" in l and late:
                break
            elif re.match(r"s_endpgm", l):
                break
    return loads, waits, late, lines, first is not None


def main():
    args = [a for a in sys.argv[1:] if a != "-v"]
    verbose = "-v" in sys.argv
    path, filters = args[0], args[1:]
    rows = [(n, b, p) for n, b, p in kernels(path)]
    names = subprocess.run(["c++filt"] + [r[0] for r in rows], capture_output=True, text=True).stdout.splitlines() if rows else []
    for (sym, body, pre), n in zip(rows, names):
        n = re.sub(r"\(.*", "", n).replace("void mg4::", "")
        if filters and not any(f in n for f in filters):
            continue
        loads, waits, late, lines, has = head(body, pre)
        print(f"{n:52s} preload {pre:2d}  before the first vector load: {loads:2d} scalar loads, {waits} lgkmcnt waits{'' if has else ' (no vector load)'};  scalar loads first issued behind it: {late}")
        if verbose:
            for l in lines:
                print("        " + l)


if __name__ == "__main__":
    main()
