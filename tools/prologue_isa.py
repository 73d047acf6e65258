#!/usr/bin/env python3
"""Static checks and counts on the gfx950 ISA of one scoring-kernel instance
(no GPU needed): cross-compiles sw_kernel<KR, AFFINE, COORDS, SPLIT> alone and
reports

  * the order of the prologue's memory operations: scalar (kernel-argument)
    loads after the first vector load, and vmcnt waits between the first
    vector load and the last 16-byte window load of the first round;
  * VALU / SALU / branch counts along one path from the kernel's entry to the
    header of the f16 loop (the last loop that holds v_perm_b32 table
    lookups): conditional branches on EXEC are taken as "some lane active"
    and loop bodies are counted once; wave-uniform branches (and EXEC
    branches round a region no lane of a fast-path wave runs) are not taken
    unless their target is listed in --taken, as LABEL or, for the branch
    at one line alone, LABEL@LINE (-v prints each one the walk
    meets, so the list is found by reading the ISA beside it).  Without
    --taken the walk is the one with the fewest instructions, among all
    choices at the wave-uniform forward branches, that issues in this order
    a length load, a read load, a 16-byte window load, a v_perm_b32 (the
    window bytes' canonical form) and a 16-byte LDS write -- the fast path's
    arms are the short ones: identity order, dword reads, selectors straight
    from the window bytes, no later round, no trace stamp -- and "taken" in
    the result lists the branches it took, to check against the ISA and to
    pin with --taken;
  * the same counts on the shortest way from that loop's exit to s_endpgm
    (the epilogue: the group maximum, the convert, the store);
  * VALU per iteration of that loop, NumVgprs, ScratchSize, code bytes.

Usage: python tools/prologue_isa.py [--kr 13] [--taken LBB0_2,LBB0_73,...] [--asm out.s]
       python tools/prologue_isa.py --from-asm file.s --taken ...
"""
from __future__ import annotations

import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mini_parallel_amd", "csrc")


def compile_instance(kr, affine, coords, split, out, csrc=CSRC):
    b = lambda v: "true" if v else "false"  # noqa: E731
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "one.hip")
        with open(src, "w") as f:
            f.write('#include "msw_device.h"\n'
                    f"template __global__ void msw::sw_kernel<{kr},{b(affine)},{b(coords)},{b(split)}>(msw::SwParams);\n")
        hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
        subprocess.run([hipcc, "-O3", "-std=c++17", "-falign-loops=32", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-I", csrc,
                        "-I", os.path.join(ROOT, "include"), src, "-o", out], check=True, stderr=subprocess.DEVNULL)


def kind(op):
    if op.startswith(("s_cbranch", "s_branch", "s_setpc")):
        return "branch"
    if op.startswith(("s_waitcnt", "s_nop", "s_load", "s_endpgm", "s_barrier", "s_sleep")):
        return "other"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("v_"):
        return "valu"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "vmem"
    if op.startswith("ds_"):
        return "lds"
    return "other"


def parse(path):
    """[(line number, label or None, opcode or None, operands)] of the kernel's text."""
    rows, inside = [], False
    for n, ln in enumerate(open(path), 1):
        s = ln.split(";")[0].strip()
        if not inside:
            inside = s.endswith(":") and s.startswith("_ZN3msw")
            continue
        if s.startswith(".Lfunc_end"):
            break
        if not s or s.startswith((".p2align", ".section", ".type", ".globl")):
            continue
        if s.endswith(":"):
            rows.append((n, s[:-1], None, ""))
        else:
            op, _, rest = s.partition(" ")
            op, _, rest2 = op.partition("\t")
            rows.append((n, None, op, (rest2 + " " + rest).strip()))
    return rows


def find_f16_loop(rows):
    """(header index, back-edge index) of the loop holding v_perm_b32 table
    lookups beside its three-way maxima: the shortest such span (a cold
    block laid out behind the loops and branching back in front of them
    spans them all)."""
    labels = {lab: i for i, (_, lab, _, _) in enumerate(rows) if lab}
    best = None
    for i, (_, _, op, args) in enumerate(rows):
        if op and op.startswith("s_cbranch") and args in labels and labels[args] < i:
            body = rows[labels[args]:i]
            if sum(1 for r in body if r[2] == "v_pk_maximum3_f16") > 8 and any(r[2] == "v_perm_b32" for r in body):
                if best is None or i - labels[args] < best[1] - best[0]:
                    best = (labels[args], i)
    return best


def successors(rows, labels, i, taken, staged=False):
    """Rows that may follow row i: [(row, branch was taken)].  taken None:
    wave-uniform forward branches go either way, and so does, once the walk
    has written selectors (staged), an EXEC branch round a region with vector
    loads: a fast-path wave issues every load before it stages, only the
    integer fallback loads again."""
    _, _, op, args = rows[i]
    if op is None or kind(op) != "branch":
        return [(i + 1, False)]
    tgt = labels.get(args)
    back = tgt is not None and tgt <= i
    if op == "s_branch":
        return [(tgt, True)]
    if tgt is None or back:
        return [(i + 1, False)]
    if op == "s_cbranch_execnz":
        return [(tgt, True)]
    listed = taken is not None and (args.lstrip(".") in taken or f"{args.lstrip('.')}@{rows[i][0]}" in taken)
    if op == "s_cbranch_execz" and taken is None and staged and any(
            r[2] and r[2].startswith("global_load") for r in rows[i + 1:tgt]):
        return [(i + 1, False), (tgt, True)]
    if op == "s_cbranch_execz" or taken is not None:
        return [(tgt, True)] if listed else [(i + 1, False)]
    return [(i + 1, False), (tgt, True)]


# What the default walk issues before the loop, in this order.
MARKS = (("global_load_ushort",), ("global_load_dword", "global_load_ubyte"), ("global_load_dwordx4",),
         ("v_perm_b32",), ("ds_write_b128",))


def shortest_walk(rows, stop, marks=MARKS, start=0):
    """The wave-uniform branches taken (LABEL@LINE) on the walk from row
    `start` to row `stop` that runs the fewest instructions and issues one
    opcode of each entry of `marks` in order; or None."""
    import heapq
    labels = {lab: i for i, (_, lab, _, _) in enumerate(rows) if lab}
    start, goal = (start, 0), (stop, len(marks))
    dist, prev, heap = {start: 0}, {}, [(0, start)]
    while heap:
        d, node = heapq.heappop(heap)
        i, seen = node
        if node == goal:
            break
        if d > dist.get(node, 1 << 60) or i >= len(rows) or i == stop:
            continue
        op = rows[i][2]
        cost = 1 if op and kind(op) != "other" else 0
        if seen < len(marks) and rows[i][2] in marks[seen]:
            seen += 1
        for j, took in successors(rows, labels, i, None, seen == len(marks)):
            nxt = (j, seen)
            if d + cost < dist.get(nxt, 1 << 60):
                dist[nxt] = d + cost
                prev[nxt] = (node, took)
                heapq.heappush(heap, (d + cost, nxt))
    if goal not in dist:
        return None
    out, node = [], goal
    while node in prev:
        node, took = prev[node]
        n, _, op, args = rows[node[0]]
        if took and op not in ("s_branch", "s_cbranch_execnz"):
            out.append(f"{args.lstrip('.')}@{n}")  # the branch at that line alone: a label may have several
    return out[::-1]


def walk(rows, stop, taken, verbose, start=0):
    """The rows run from row `start` to row `stop` with the listed branches
    taken, or a message where that walk leaves the path."""
    labels = {lab: i for i, (_, lab, _, _) in enumerate(rows) if lab}
    i, seen, path = start, set(), []
    while i != stop:
        if i in seen or i >= len(rows):
            return (f"left the path at line {rows[min(i, len(rows) - 1)][0]}: adjust --taken "
                    "(-v lists the branches met)"), path
        seen.add(i)
        path.append(i)
        n, _, op, args = rows[i]
        (j, took), = successors(rows, labels, i, taken)
        if verbose and op and op.startswith("s_cbranch") and not op.startswith("s_cbranch_exec"):
            print(f"  line {n}: {op} {args} -> {'taken' if took else 'falls through'}", file=sys.stderr)
        i = j
    return None, path


def count(rows, path):
    counts = {"valu": 0, "salu": 0, "branch": 0, "vmem": 0, "lds": 0}
    for i in path:
        k = kind(rows[i][2]) if rows[i][2] else "other"
        if k in counts:
            counts[k] += 1
    return counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kr", type=int, default=13)
    ap.add_argument("--affine", action="store_true")
    ap.add_argument("--coords", action="store_true")
    ap.add_argument("--split", action="store_true")
    ap.add_argument("--taken", default="", help="labels of the wave-uniform branches the fast path takes")
    ap.add_argument("--from-asm", default="", help="read this ISA file instead of compiling")
    ap.add_argument("--asm", default="", help="keep the ISA here")
    ap.add_argument("--csrc", default=CSRC, help="directory of msw_device.h (another checkout, for before/after)")
    ap.add_argument("-v", "--verbose", action="store_true")
    args = ap.parse_args()

    path = args.from_asm
    tmp = None
    if not path:
        path = args.asm
        if not path:
            tmp = tempfile.NamedTemporaryFile(suffix=".s", delete=False)
            path = tmp.name
        compile_instance(args.kr, args.affine, args.coords, args.split, path, args.csrc)
    rows = parse(path)
    text = open(path).read()
    ops = [(i, r) for i, r in enumerate(rows) if r[2]]
    first_vload = next(i for i, r in ops if r[2].startswith("global_load"))
    x4 = [i for i, r in ops if r[2] == "global_load_dwordx4"]
    # the first round's window loads: the 16-byte loads before the first LDS write
    first_lds = next(i for i, r in ops if r[2].startswith("ds_write"))
    round0 = [i for i in x4 if i < first_lds]
    last_round0 = max(round0) if round0 else first_vload
    res = {
        "instance": f"sw_kernel<{args.kr},{args.affine},{args.coords},{args.split}>".lower(),
        "s_load_after_first_vector_load": [rows[i][0] for i, r in ops if i > first_vload and r[2].startswith("s_load")],
        "vmcnt_waits_between_first_vector_load_and_last_first_round_window_load":
            [rows[i][0] for i, r in ops if first_vload < i < last_round0 and r[2] == "s_waitcnt" and "vmcnt" in r[3]],
        "vector_loads_before_first_vmcnt_wait": 0,
    }
    for i, r in ops:
        if i > first_vload and r[2] == "s_waitcnt" and "vmcnt" in r[3]:
            break
        if i >= first_vload and r[2].startswith("global_load"):
            res["vector_loads_before_first_vmcnt_wait"] += 1
    loop = find_f16_loop(rows)
    if loop:
        res["f16_loop_valu_per_iteration"] = sum(1 for r in rows[loop[0]:loop[1]] if r[2] and kind(r[2]) == "valu")
        taken = list(filter(None, args.taken.split(",")))
        if not taken:
            taken = shortest_walk(rows, loop[0]) or []
        res["taken"] = taken
        left, steps = walk(rows, loop[0], set(taken), args.verbose)
        res["prologue_path"] = left or count(rows, steps)
        on = [rows[i] for i in steps if rows[i][2]]
        loads = [k for k, r in enumerate(on) if r[2].startswith("global_load")]
        waits = [k for k, r in enumerate(on) if r[2] == "s_waitcnt" and "vmcnt" in r[3]]
        lds = [k for k, r in enumerate(on) if r[2].startswith("ds_write")]
        if loads:
            first_wait = next((k for k in waits if k > loads[0]), len(on))
            x4 = [k for k in loads if on[k][2] == "global_load_dwordx4" and (not lds or k < lds[0])]
            # along the walk, not in the text's order: the arms of the early
            # loads are laid out one behind the other
            res["vector_loads"] = len(loads)
            res["vector_loads_before_first_vmcnt_wait"] = sum(1 for k in loads if k < first_wait)
            res["vmcnt_waits_between_first_vector_load_and_last_first_round_window_load"] = \
                [on[k][0] for k in waits if x4 and loads[0] < k < x4[-1]]
        # behind the loop: the fewest instructions from its exit to s_endpgm
        # (every lane-masked region run, no trace record)
        ends = [i for i, r in enumerate(rows) if r[2] == "s_endpgm" and i > loop[1]]
        best = None
        for e in ends:
            t = shortest_walk(rows, e, (), loop[1] + 1)
            if t is not None:
                left, tail = walk(rows, e, set(t), False, loop[1] + 1)
                if not left and (best is None or len(tail) < best[0]):
                    best = (len(tail), count(rows, tail))
        if best:
            res["epilogue_path"] = best[1]
    for key in ("NumVgprs", "ScratchSize", "TotalNumSgprs", "codeLenInByte"):
        m = re.search(rf"; {key}[:=]? *=? *(\d+)", text)
        if m:
            res[key] = int(m.group(1))
    print(json.dumps(res))
    if tmp:
        os.unlink(path)


if __name__ == "__main__":
    main()
