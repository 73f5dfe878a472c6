#!/usr/bin/env python3
"""The traversal main loop of a kernel in the device asm (make asm -> build/rt_render.s): its text
and an instruction census by class and by basic block, with the s_waitcnt points (VERDICT r05
item 1: what a trip issues between one record's arrival and the next record's load).

The loop is the one whose header precedes the kernel's first `buffer_load_dwordx4` with an
`offset:32` operand (the third 16-B load of a record: the main loop; the wave-uniform prologue
reads through the scalar cache).  Blocks are listed in program order with their instruction
counts; a trip runs the head, then the inner-step and/or the triangle-step blocks (exec-masked:
a mixed trip runs both), then the tail.
A kernel with the octant loops (rt_kernel_body.inc traverse_fast) has several main loops per
traversal: WHICH (default 0) picks the WHICH-th of them in program order, and the census says how
many two-input v_min / v_max the loop holds (12 of them: a generic loop; none: an octant loop, or
the division form, which uses the compiler's own min / max).
The wave-uniform prologue loop that hands over to the chosen main loop (the loop that reads its record
with s_load_dwordx8 and whose exit leads to the main loop's preheader) gets the same census, in
OUT_PREFIX_prologue.{s,txt}.  Both censuses count the SGPR -> VGPR copies, v_readlane / v_writelane and
v_mad_u64_u32 the loop holds.
The main loop's census also says whether the child-ref load precedes the trip's first wait on its
record loads (ref_load_rule below); the exit status is 1 when it does not.
Usage: python3 scripts/isa_loop.py ASM KERNEL_SYMBOL_PREFIX OUT_PREFIX [WHICH]"""
import re
import sys


def classify(op):
    if op.startswith("s_waitcnt"):
        return "waitcnt"
    if op.startswith(("s_cbranch", "s_branch")):
        return "branch"
    if op.startswith(("buffer_", "global_", "flat_")):
        return "vmem"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("s_load", "s_buffer_load", "s_memrealtime")):
        return "smem"
    if op.startswith("s_nop"):
        return "nop"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("v_"):
        return "valu_trans" if re.match(r"v_(rcp|rsq|sqrt|exp|log|sin|cos)_", op) else "valu"
    return "other"


BLOCK = re.compile(r"^(\.LBB\w+|; %bb\.\d+):")


def loop_lines(body, hdr):
    """The lines of the loop whose header block starts at body[hdr]: the header and every block the
    assembler marks "in Loop: Header=<it>" (Depth=1)."""
    label = body[hdr].split(":")[0]
    tag = "Header=" + label[2:]   # ".LBB51_7" -> "Header=BB51_7"
    loop, inside = [], False
    for i, l in enumerate(body):
        if BLOCK.match(l.strip()):
            inside = i == hdr or (re.search(tag + r"\b", l) is not None and "Depth=1" in l)
        if inside:
            loop.append(l)
    return label, loop


def prologue_header(body, hdr):
    """The header of the wave-uniform prologue loop that hands over to the main loop at body[hdr]: walk
    back from the main loop's header through the blocks outside it (its preheaders: reached by a branch
    to their label, or by falling through) until a block of another loop, one that reads a record
    through the scalar cache (s_load_dwordx8), branches there.  None when there is none."""
    starts = [i for i, l in enumerate(body) if BLOCK.match(l.strip())]
    blocks = []   # (first line, last line + 1, label or None, loop tag or None)
    for k, s in enumerate(starts):
        e = starts[k + 1] if k + 1 < len(starts) else len(body)
        head = body[s].strip()
        m = re.search(r"Header=(BB\w+)", head)
        own = head.split(":")[0]
        tag = m.group(1) if m else (own[2:] if "Loop Header" in head and own.startswith(".L") else None)
        blocks.append((s, e, own if own.startswith(".L") else None, tag))
    main_tag = body[hdr].split(":")[0][2:]

    def ops(b):
        return [l.strip() for l in body[b[0] + 1:b[1]] if l.strip() and not l.strip().startswith((";", "."))]

    def falls_through(b):
        o = ops(b)
        return not o or not o[-1].startswith(("s_branch", "s_endpgm", "s_setpc"))

    want = {body[hdr].split(":")[0]}   # labels that lead to the main loop
    seen = set()
    for _ in range(6):
        grown = False
        for k, b in enumerate(blocks):
            if k in seen or b[3] == main_tag:
                continue
            targets = {o.split()[-1] for o in ops(b) if o.startswith(("s_cbranch", "s_branch"))}
            nxt = blocks[k + 1] if k + 1 < len(blocks) else None
            leads = bool(targets & want) or (nxt is not None and falls_through(b) and
                                             (nxt[2] in want or ("@%d" % (k + 1)) in want))
            if not leads:
                continue
            if b[3] is not None:   # a block of another loop
                h = next(i for i, l in enumerate(body) if l.startswith(".L" + b[3] + ":"))
                if any("s_load_dwordx8" in l for l in loop_lines(body, h)[1]):
                    return h
                continue
            seen.add(k)
            want.add(b[2] if b[2] else "@%d" % k)
            grown = True
        if not grown:
            break
    return None


def main():
    asm, sym, out = sys.argv[1], sys.argv[2], sys.argv[3]
    which = int(sys.argv[4]) if len(sys.argv) > 4 else 0
    lines = open(asm).read().splitlines()
    start = next(i for i, l in enumerate(lines) if l.startswith(sym) and l.rstrip().endswith(":") or
                 (l.startswith(sym) and ": ;" in l))
    end = next(i for i in range(start + 1, len(lines)) if lines[i].startswith(".Lfunc_end"))
    body = lines[start:end]
    hdrs = []   # the main loops' headers, in program order
    for ld in (i for i, l in enumerate(body) if "buffer_load_dwordx4" in l and "offset:32" in l):
        h = max(i for i in range(ld) if "Loop Header" in body[i])
        if h not in hdrs:
            hdrs.append(h)
    hdr = hdrs[which]
    label, loop = loop_lines(body, hdr)
    census(sym, f"main loop {which} of {len(hdrs)}", label, loop, out, ref_load_rule(loop))
    pro = prologue_header(body, hdr)
    if pro is None:
        print("no wave-uniform prologue loop found in front of this main loop")
    else:
        plabel, ploop = loop_lines(body, pro)
        census(sym, f"prologue of main loop {which}", plabel, ploop, out + "_prologue")
    if not ref_load_rule(loop)[0]:
        sys.exit(1)


def ref_load_rule(loop):
    """DESIGN.md 7.2, one round trip per trip: from the trip's first record load on, in program order
    (the inner step precedes the triangle step), the child-ref load (buffer_load_dwordx2 ... offset:48, or
    the cursor loop's load from the walk array, below) is issued before any s_waitcnt whose vmcnt is
    below the number of record loads issued so far, the first wait that can hold the wave for this
    trip's records.  -> (holds, one line of text)."""
    issued, started = 0, False
    # The cursor loop (traverse_ifif's CUR) reads its child refs from the walk array, not from the
    # record: its ref load is a buffer_load_dwordx2 with no offset whose address register was made by
    # v_lshl_add_u32 ADDR, CUR, 1, WALK_OFF (walk_off + (cur << 1)) inside the trip; nothing else counts.
    # (The waits the compiler leaves at that loop's head stand before the trip's first load and
    # retire nothing of this trip: no wait before the first record load was ever counted.)
    walk_addr = set()
    for l in loop:
        s = l.strip()
        m = re.match(r"v_lshl_add_u32 (v\d+), (v\d+), 1, (v\d+)$", s)
        # (after the trip's first record load, and of two different registers: the old decode's
        # 3 x = (x << 1) + x names one register twice and stands before the loads)
        if m and started and m.group(2) != m.group(3):
            walk_addr.add(m.group(1))
        if s.startswith("buffer_load_dwordx4") and "offset:" not in s:
            started = True
        if not started:
            continue
        m = re.match(r"buffer_load_dwordx2 v\[\d+:\d+\], (v\d+), ", s)
        if (s.startswith("buffer_load_dwordx2") and "offset:48" in s) or (m and "offset:" not in s and m.group(1) in walk_addr):
            return True, f"ref load rule: holds (the ref load is record load {issued + 1} of the trip, no wait on them before it)"
        if s.startswith("buffer_load_"):
            issued += 1
        m = re.match(r"s_waitcnt .*vmcnt\((\d+)\)", s)
        if m and int(m.group(1)) < issued:
            return False, f"ref load rule: BROKEN ({s} after {issued} record loads, before the ref load)"
    return False, "ref load rule: BROKEN (no ref load after the record loads)"


def census(sym, what, label, loop, out, rule=None):
    blocks, cur = [], {"name": "(entry)", "n": 0, "cls": {}}
    waits = []
    minmax = {}
    moves = {"v_mov_b32 from SGPR": 0, "v_readlane_b32": 0, "v_writelane_b32": 0, "v_mad_u64_u32": 0}
    for l in loop:
        s = l.strip()
        if re.match(r"^(\.LBB\w+|; %bb\.\d+):", s):
            blocks.append(cur)
            cur = {"name": s.split(":")[0], "n": 0, "cls": {}}
            continue
        if not s or s.startswith((";", ".")):
            continue
        op = s.split()[0]
        c = classify(op)
        if re.match(r"v_(min|max)3?_f32", op):
            minmax[op] = minmax.get(op, 0) + 1
        if re.match(r"v_mov_b32(_e32|_e64)?$", op) and re.search(r",\s*s\d+$", s):
            moves["v_mov_b32 from SGPR"] += 1
        for k in ("v_readlane_b32", "v_writelane_b32", "v_mad_u64_u32"):
            if op == k:
                moves[k] += 1
        cur["n"] += 1
        cur["cls"][c] = cur["cls"].get(c, 0) + 1
        if c == "waitcnt":
            waits.append(f"{cur['name']}: {s}")
    blocks.append(cur)
    tot = {}
    for b in blocks:
        for k, v in b["cls"].items():
            tot[k] = tot.get(k, 0) + v
    with open(out + ".s", "w") as f:
        f.write("\n".join(loop) + "\n")
    with open(out + ".txt", "w") as f:
        f.write(f"kernel {sym}, {what}, {label}: {sum(b['n'] for b in blocks)} instructions "
                f"in {len(blocks)} blocks\n")
        f.write("min/max: " + (", ".join(f"{k} {v}" for k, v in sorted(minmax.items())) or "none") + "\n")
        f.write("copies and wide multiplies: " + ", ".join(f"{k} {v}" for k, v in moves.items()) + "\n")
        if rule is not None:
            f.write(rule[1] + "\n")
        f.write("by class: " + ", ".join(f"{k} {v}" for k, v in sorted(tot.items())) + "\n\nblocks in program order:\n")
        for b in blocks:
            f.write(f"  {b['name']:12s} {b['n']:4d}  " + ", ".join(f"{k} {v}" for k, v in sorted(b["cls"].items())) + "\n")
        f.write("\ns_waitcnt points:\n" + "\n".join("  " + w for w in waits) + "\n")
    print(open(out + ".txt").read())


if __name__ == "__main__":
    main()
