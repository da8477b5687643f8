#!/usr/bin/env python3
"""Issue-to-wait distance of every vector memory load in a kernel's inner loop, counted in MFMAs of the same wave.

    hipcc <the build's flags> --cuda-device-only -S csrc/kernels_wino.hip -o wino.s
    python tools/kloop_schedule.py wino.s wino_fused_kernel

Reads the first loop marked "Inner Loop Header" of the named kernel, walks it three times as wave 0 of a middle iteration
would (every LDS-DMA block entered, no skip or exit branch taken) and replays the in-order vmcnt counter: a load is
covered by the first s_waitcnt vmcnt(N) that leaves at most N younger loads outstanding. Prints, for the middle
walk, each load with the number of MFMAs between its issue and that wait, and where the s_barrier falls.
Then a histogram of the middle walk's instructions by class: MFMA, fragment load, LDS-DMA, ds_read, s_nop, integer and
float vector ALU (a v_ instruction whose name carries _f16 / _f32 / _f64 is float; moves, lane reads and everything else
are integer), with the integer multiplies, lane reads and wait states of the s_nop (N + 1 each) spelled out, and the
other scalar instructions in one figure.
Needs no GPU; the listing is evidence for a reader, not a test.
"""
import re
import sys


def main():
    path, kernel = sys.argv[1], sys.argv[2]
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\w*%s\w*:" % kernel, l))
    head = next(i for i in range(start, len(lines)) if "Inner Loop Header" in lines[i])
    if not lines[head].startswith("."):          # a loop inside another: the label is on the line before
        head -= 1
    label = lines[head].split(":")[0]
    end = next(i for i in range(head, len(lines)) if ".end_amdhsa_kernel" in lines[i] or "s_endpgm" in lines[i])
    back = max(i for i in range(head, end) if re.search(r"s_c?branch\w*\s+%s\b" % re.escape(label), lines[i]))
    labels = {l.split(":")[0]: i for i, l in enumerate(lines[start:end], start) if re.match(r"^\.LBB\w+:", l)}

    events = []          # (walk, text) in execution order, three walks: the middle one is reported
    for walk in range(3):
        pc = head + 1
        steps = 0
        while steps < 20000:
            steps += 1
            t = lines[pc].strip()
            m = re.match(r"(s_c?branch\w*)\s+(\.LBB\w+)", t)
            if m:
                op, tgt = m.groups()
                ti = labels.get(tgt, -1)
                if pc == back:
                    break
                if pc > back:            # out-of-line block: back to the body by its unconditional branch only
                    pc = ti if op == "s_branch" else pc + 1
                    # a conditional branch back to the body skips the remaining DMA blocks: fall through instead,
                    # unless the next line is no DMA block of this loop
                    if op != "s_branch" and not re.match(r"^\.LBB", lines[pc]):
                        pc = ti
                    continue
                if ti > back and ti < end and "in Loop" in lines[ti]:
                    pc = ti              # into an out-of-line block of the loop (the LDS-DMA instructions)
                    continue
                pc += 1                  # skip and exit branches: not taken
                continue
            if t and not t.startswith(";") and not t.endswith(":") and not t.startswith("."):
                events.append((walk, t))
            pc += 1

    mfma = 0
    pending = []         # [walk, index in walk, text, mfma at issue]
    rows = {}
    order = []
    idx = 0
    for walk, t in events:
        op = t.split()[0]
        if op.startswith("v_mfma"):
            mfma += 1
        elif op.startswith(("buffer_load", "global_load", "flat_load")):
            idx += 1
            kind = "DMA" if t.endswith(" lds") else "B"
            key = (walk, idx)
            pending.append((key, mfma))
            rows[key] = [kind, mfma, None, t]
            order.append(key)
        elif op == "s_waitcnt":
            m = re.search(r"vmcnt\((\d+)\)", t)
            if m:
                n = int(m.group(1))
                while len(pending) > n:
                    key, at = pending.pop(0)
                    rows[key][2] = mfma
        elif op == "s_barrier":
            order.append(("barrier", walk, mfma))
    per_walk = sum(1 for w, t in events if w == 0 and t.startswith("v_mfma"))
    print("# %s: %d MFMAs per K-step; position = MFMAs issued since the top of the step" % (kernel, per_walk))
    print("# kind  issued-at  waited-at  MFMAs-between")
    for key in order:
        if key[0] == "barrier":
            if key[1] == 1:
                print("s_barrier at %d" % (key[2] - per_walk))
            continue
        if key[0] != 1:
            continue
        kind, at, w, t = rows[key]
        print("%-4s %9d %10s %8s" % (kind, at - per_walk, "-" if w is None else w - per_walk, "-" if w is None else w - at))
    histogram(kernel, [t for w, t in events if w == 1])


def classify(t):
    op = t.split()[0]
    if op.startswith("v_mfma"):
        return "MFMA"
    if op.startswith(("buffer_load", "global_load", "flat_load")):
        return "LDS-DMA" if t.endswith(" lds") else "fragment load"
    if op.startswith("ds_read") or op.startswith("ds_load"):
        return "ds_read"
    if op == "s_nop":
        return "s_nop"
    if op.startswith("v_"):
        return "float VALU" if re.search(r"_f(16|32|64)\b|_f(16|32|64)_", op) else "integer VALU"
    if op.startswith("s_"):
        return "other scalar"
    return "other"


def histogram(kernel, walk):
    classes = ["MFMA", "fragment load", "LDS-DMA", "ds_read", "s_nop", "integer VALU", "float VALU", "other scalar", "other"]
    n = dict.fromkeys(classes, 0)
    ops = {}
    nop_states = 0
    for t in walk:
        c = classify(t)
        n[c] += 1
        op = t.split()[0]
        if c in ("integer VALU", "float VALU"):
            ops[op] = ops.get(op, 0) + 1
        if c == "s_nop":
            nop_states += int(t.split()[1], 0) + 1
    print("# %s: instructions of one K-step (wave 0, a middle step), by class" % kernel)
    for c in classes:
        if n[c] or c != "other":
            print("%-14s %5d" % (c, n[c]))
    print("%-14s %5d" % ("vector ALU", n["integer VALU"] + n["float VALU"]))
    print("%-14s %5d" % ("s_nop states", nop_states))
    print("# vector ALU by instruction")
    for op in sorted(ops, key=lambda o: (-ops[o], o)):
        print("  %-22s %4d" % (op, ops[op]))


if __name__ == "__main__":
    main()
