#!/usr/bin/env python3
"""Scratch (spill) traffic of the 2-D GP evaluation, per loop depth of the blocked sweep.

Reads the device assembly of csrc/lcfe.hip and the compiler's resource remarks:

    cd mallorn-astrophysics_amd/csrc
    hipcc $(HIPFLAGS) --cuda-device-only -S -Rpass-analysis=kernel-resource-usage -o lcfe.s lcfe.hip 2> remarks.txt
    python tools/gp_sweep_scratch.py lcfe.s remarks.txt > profiles/gp_sweep_scratch_<tag>.txt

For every gp_eval<NP> instantiation (the evaluation is a function of its own; the sweep is inlined into it) the loops are
rebuilt from the listing's control flow (basic blocks, dominators, natural loops: the block layout is not contiguous, so
label order alone does not give the nesting).  The pivot-step loop is the outermost loop that holds MFMAs (only the
sweep uses them); "body" counts what sits directly in it, "tile-row loop" one loop further in (the row loops of the
update phase and of the gather), "tile loop" two and more further in (the trips over the tiles of a row).  Spill slots
are named by their scratch offset, so that a value stored at one depth and reloaded at another can be followed.
"""
import re
import sys
from collections import Counter

SCR = re.compile(r"^\s+scratch_(load|store)_dword(x\d)?\s+(.*?)(;.*)?$")
LABEL = re.compile(r"^(\.LBB\d+_\d+):")
BRANCH = re.compile(r"^\s+s_c?branch\w*\s+(\.LBB\d+_\d+)")
FUNC = re.compile(r"^\s+\.type\s+(\S+),@function")
EVAL = re.compile(r"gp_evalINS_8BlockDevILi(\d+)EEELi(\d+)EPU3AS(\d)d")


def functions(lines):
    name, start = None, 0
    for k, ln in enumerate(lines):
        m = FUNC.match(ln)
        if m:
            name, start = m.group(1), k
        elif name and ln.startswith(".Lfunc_end"):
            yield name, lines[start:k]
            name = None


def blocks_of(body):
    """Basic blocks of a function listing: [(first line, last line)], successor lists, line -> block."""
    at = {}
    starts = {0}
    for k, ln in enumerate(body):
        m = LABEL.match(ln)
        if m:
            at[m.group(1)] = k
            starts.add(k)
        elif BRANCH.match(ln) or re.match(r"^\s+s_(setpc_b64|endpgm)", ln):
            starts.add(k + 1)
    order = sorted(x for x in starts if x < len(body))
    blocks = [(a, (order[i + 1] if i + 1 < len(order) else len(body)) - 1) for i, a in enumerate(order)]
    first = {a: i for i, (a, _) in enumerate(blocks)}
    succ = []
    for i, (a, b) in enumerate(blocks):
        out = []
        last = next((body[k] for k in range(b, a - 1, -1) if body[k].startswith("\t") and not body[k].startswith("\t.")), "")
        m = BRANCH.match(last)
        if m and m.group(1) in at:
            out.append(first[at[m.group(1)]])
        ends = re.match(r"^\s+s_(setpc_b64|endpgm|branch)\b", last)
        if not ends and i + 1 < len(blocks):
            out.append(i + 1)
        succ.append(out)
    return blocks, succ


def loops_of(body):
    """Natural loops (header block -> set of blocks) from the dominator tree of the listing's control flow."""
    blocks, succ = blocks_of(body)
    n = len(blocks)
    pred = [[] for _ in range(n)]
    for u in range(n):
        for v in succ[u]:
            pred[v].append(u)
    full = (1 << n) - 1
    dom = [full] * n
    dom[0] = 1
    changed = True
    while changed:
        changed = False
        for v in range(1, n):
            d = full
            for u in pred[v]:
                d &= dom[u]
            d = (d | (1 << v)) if pred[v] else (1 << v)
            if d != dom[v]:
                dom[v], changed = d, True
    loops = {}
    for u in range(n):
        for h in succ[u]:
            if dom[u] >> h & 1:
                mem = loops.setdefault(h, {h})
                work = [u]
                while work:
                    x = work.pop()
                    if x not in mem:
                        mem.add(x)
                        work.extend(pred[x])
    return blocks, loops


def slot_of(operands):
    m = re.search(r"offset:(\d+)", operands)
    return int(m.group(1)) if m else 0


def analyse(body):
    blocks, loops = loops_of(body)
    mfma_blocks = {i for i, (a, b) in enumerate(blocks) if any("v_mfma_f64" in body[k] for k in range(a, b + 1))}
    with_mfma = {h: mem for h, mem in loops.items() if mem & mfma_blocks}
    outer = {h: mem for h, mem in with_mfma.items() if not any(h2 != h and mem < mem2 for h2, mem2 in with_mfma.items())}
    res = {"mfma": sum("v_mfma_f64" in ln for ln in body), "steps": len(outer), "depth": Counter(), "slots": {}, "outside": Counter()}
    block_at = {}
    for i, (a, b) in enumerate(blocks):
        for k in range(a, b + 1):
            block_at[k] = i
    for k, ln in enumerate(body):
        m = SCR.match(ln)
        if not m:
            continue
        kind, blk = m.group(1), block_at[k]
        home = [h for h, mem in outer.items() if blk in mem]
        if not home:
            res["outside"][kind] += 1
            continue
        d = sum(1 for h, mem in loops.items() if h != home[0] and blk in mem and mem < outer[home[0]])
        d = min(d, 2)
        res["depth"][(d, kind)] += 1
        res["slots"].setdefault(d, Counter())[(kind, slot_of(m.group(3)))] += 1
    return res


def remarks_of(path):
    out, cur = {}, None
    for ln in open(path):
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = m.group(1)
            out[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+)", ln)
        if m and cur:
            out[cur][m.group(1).strip()] = m.group(2)
    return out


def main():
    lines = open(sys.argv[1]).read().split("\n")
    rem = remarks_of(sys.argv[2]) if len(sys.argv) > 2 else {}
    names = ("body", "tile-row loop", "tile loop")
    for name, body in functions(lines):
        m = EVAL.search(name)
        if not m:
            continue
        threads, np_, space = int(m.group(1)), int(m.group(2)), m.group(3)
        r = analyse(body)
        print(f"gp_eval<NP = {np_}>  {threads} threads, matrix in {'LDS' if space == '3' else 'global scratch'}")
        for kname, kv in rem.items():
            if re.search(rf"gp_kernelILi{np_}E", kname):
                print("  kernel: VGPRs {VGPRs}, AGPRs {AGPRs}, scratch {ScratchSize} B/lane, {Occupancy} waves/SIMD, "
                      "VGPR spill {VGPRs Spill}, LDS {LDS Size} B".format(**kv))
        print(f"  MFMAs {r['mfma']}, pivot-step loops {r['steps']}; outside the step loop: "
              f"{r['outside']['load']} scratch loads, {r['outside']['store']} stores")
        for d in range(3):
            print(f"  {names[d]:14s}: {r['depth'][(d, 'load')]:4d} loads {r['depth'][(d, 'store')]:4d} stores")
        for d in sorted(r["slots"]):
            s = r["slots"][d]
            txt = ", ".join(f"{k[0][0].upper()}@{k[1]}" + (f"x{v}" if v > 1 else "") for k, v in sorted(s.items(), key=lambda kv: (kv[0][1], kv[0][0])))
            print(f"    {names[d]} slots (L = load, S = store, @byte offset): {txt}")
        print()


if __name__ == "__main__":
    main()
