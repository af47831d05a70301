"""Instruction counts of one kernel by source region, from an ISA listing with line tables.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -gline-tables-only -S --cuda-device-only -Iinclude \
        vtgaussian-slam_amd/csrc/vtgs_composite_q.hip -o q.s
    python tools/isa_account.py q.s composite_forward_qILi0E            # the regions of REGIONS below
    python tools/isa_account.py q.s composite_forward_qILi0E --lines    # every source line on its own

Every instruction is attributed to the innermost `.loc` in front of it (file, line) and sorted into vector (v_*, without
MFMA), MFMA, scalar (s_*), LDS (ds_*) and memory (global_* / buffer_* / flat_* / scratch_*); s_nop, s_waitcnt and s_endpgm are
not counted.  STATIC counts: a line of source that the compiler emitted several times (an inlined function, a template
instantiated four times) is summed over its copies.  A macro's body is attributed to the line of its CALL, so the four
call sites of VTGS_Q_APPEND come out separately; what the macro inlines (tile_coefficients, quadrant_mask, q_ring_wrap)
is attributed to those functions' own lines, summed over the call sites.

REGIONS are found in the source files the listing names (`.file`), between a first and a last line given as regular
expressions, so the table of profiles/r7_forward_bookkeeping.md can be regenerated after the code has moved.
"""
import collections
import os
import re
import sys

Q, C, S = "vtgs_composite_q.hip", "vtgs_composite_common.h", "vtgs_sort_common.h"
# (file, regex of the first line, regex of the line AFTER the last one (None: the first line alone), name); first match wins
REGIONS = [
    (Q, r"VTGS_Q_APPEND\(g0_a", None, "append, prologue call site 1 (macro body; ring state constant)"),
    (Q, r"VTGS_Q_APPEND\(g0_b", None, "append, prologue call site 2 (macro body)"),
    (Q, r"VTGS_Q_APPEND\(g0_c", None, "append, prologue call site 3 (macro body)"),
    (Q, r"VTGS_Q_APPEND\(g0n", None, "append, in-loop call site (macro body)"),
    (Q, r"uint32_t q_ring_wrap\(", None, "q_ring_wrap, all uses (2 per use: appends and pop)"),
    (Q, r"uint32_t quadrant_mask\(", r"^}", "quadrant_mask, four call sites together"),
    (C, r"void tile_coefficients\(", r"^}", "tile_coefficients, four call sites together"),
    (Q, r"^template <bool DUAL, bool CLAMP, bool EXACT_FIRST>", r"^#ifndef VTGS_Q_WAVES", "q_forward_step (+ q_alpha, q_colour), three variants together"),
    (Q, r"T q_alpha\(|float q_alpha\(", r"^}", "q_forward_step (+ q_alpha, q_colour), three variants together"),
    (Q, r"f32x4 q_colour\(", r"^}", "q_forward_step (+ q_alpha, q_colour), three variants together"),
    (Q, r"const int avail = min\(16", r"\+\+nsteps;", "one step outside q_forward_step (pops, payload addresses, head, c0..c2)"),
    (Q, r"ka\[kQDummy\] = ", r"#define VTGS_Q_APPEND", "sort end -> first append (dummy slot, queue clear, ring state, entry / fetch)"),
    (Q, r"static_assert\(kQChunks == 3", r"VTGS_Q_APPEND\(g0_a", "sort end -> first append (dummy slot, queue clear, ring state, entry / fetch)"),
    (S, r"bool wave_count_sort\(", r"^// The same counting sort by a whole", "wave_count_sort, four instantiations together"),
]


def classify(op):
    if op.startswith("v_mfma"):
        return "mfma"
    if op.startswith("v_"):
        return "vector"
    if op.startswith("s_"):
        return "scalar"
    if op.startswith("ds_"):
        return "lds"
    if op.split("_")[0] in ("global", "buffer", "flat", "scratch"):
        return "mem"
    return "other"


def region_ranges(paths):
    """{file suffix: [(first, last, name)]} from the sources on disk."""
    out = collections.defaultdict(list)
    for suf, first, after, name in REGIONS:
        path = next((p for p in paths if p.endswith(suf) and os.path.exists(p)), None)
        if path is None:
            continue
        lines = open(path).read().splitlines()
        a = next((i for i, l in enumerate(lines) if re.search(first, l)), None)
        if a is None:
            continue
        b = a if after is None else next((i - 1 for i in range(a + 1, len(lines)) if re.search(after, lines[i])), len(lines) - 1)
        out[suf].append((a + 1, b + 1, name))
    return out


def main():
    path, kernel = sys.argv[1], sys.argv[2]
    by_line = len(sys.argv) > 3 and sys.argv[3] == "--lines"
    files, cur, inside = {}, ("?", 0), False
    counts = collections.defaultdict(collections.Counter)
    for raw in open(path):
        line = raw.strip()
        m = re.match(r'\.file\s+(\d+)\s+"([^"]*)"(?:\s+"([^"]*)")?', line)
        if m:
            files[int(m.group(1))] = os.path.join(m.group(2), m.group(3)) if m.group(3) else m.group(2)
            continue
        if re.match(r"^_Z\w+:", line):
            inside = kernel in line
            continue
        if not inside:
            continue
        if line.startswith(".Lfunc_end"):
            inside = False
            continue
        m = re.match(r"\.loc\s+(\d+)\s+(\d+)", line)
        if m:
            cur = (files.get(int(m.group(1)), "?"), int(m.group(2)))
            continue
        if not line or line[0] in ".;" or line.endswith(":"):
            continue
        op = line.split()[0]
        if op in ("s_nop", "s_waitcnt", "s_endpgm", "s_code_end"):
            continue
        counts[cur][classify(op)] += 1
    ranges = {} if by_line else region_ranges(set(files.values()))
    out, order = collections.defaultdict(collections.Counter), []
    for (f, ln), c in sorted(counts.items(), key=lambda kv: (os.path.basename(kv[0][0] or ""), kv[0][1])) if counts else []:
        key = None
        for suf, rs in ranges.items():
            if f.endswith(suf):
                key = next((name for a, b, name in rs if a <= ln <= b), None)
        if key is None:
            key = "%s:%d" % (os.path.basename(f), ln) if by_line else "everything else"
        if key not in out:
            order.append(key)
        out[key].update(c)
    cols = ("vector", "mfma", "scalar", "lds", "mem", "other")
    print("%-86s" % "region", " ".join("%7s" % c for c in cols))
    tot = collections.Counter()
    for key in order:
        print("%-86s" % key, " ".join("%7d" % out[key][c] for c in cols))
        tot.update(out[key])
    print("%-86s" % "total", " ".join("%7d" % tot[c] for c in cols))


if __name__ == "__main__":
    main()
