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
    unless their target is listed in --taken (the walk prints each one it
    meets, so the list is found by reading the ISA beside it);
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
    """(header index, back-edge index) of the last loop holding v_perm_b32."""
    labels = {lab: i for i, (_, lab, _, _) in enumerate(rows) if lab}
    best = None
    for i, (_, _, op, args) in enumerate(rows):
        if op and op.startswith("s_cbranch") and args in labels and labels[args] < i:
            body = rows[labels[args]:i]
            if sum(1 for r in body if r[2] == "v_pk_maximum3_f16") > 8 and any(r[2] == "v_perm_b32" for r in body):
                best = (labels[args], i)
    return best


def walk(rows, stop, taken, verbose):
    labels = {lab: i for i, (_, lab, _, _) in enumerate(rows) if lab}
    counts = {"valu": 0, "salu": 0, "branch": 0, "vmem": 0, "lds": 0}
    i, seen = 0, set()
    while i != stop:
        if i in seen or i >= len(rows):
            return f"left the path at line {rows[min(i, len(rows) - 1)][0]}: adjust --taken (-v lists the branches met)"
        seen.add(i)
        n, lab, op, args = rows[i]
        if op is None:
            i += 1
            continue
        k = kind(op)
        if k in counts:
            counts[k] += 1
        if k == "branch":
            tgt = labels.get(args)
            back = tgt is not None and tgt <= i
            if op == "s_branch":
                go = True
            elif op == "s_cbranch_execz":  # skipped region (no lane active): only where listed
                go = args.lstrip(".") in taken and not back
            elif op == "s_cbranch_execnz":
                go = not back
            else:
                go = args.lstrip(".") in taken and not back
                if verbose:
                    print(f"  line {n}: {op} {args} -> {'taken' if go else 'falls through'}", file=sys.stderr)
            if go:
                i = tgt
                continue
        i += 1
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
        res["prologue_path"] = walk(rows, loop[0], set(filter(None, args.taken.split(","))), args.verbose)
    for key in ("NumVgprs", "ScratchSize", "TotalNumSgprs", "codeLenInByte"):
        m = re.search(rf"; {key}[:=]? *=? *(\d+)", text)
        if m:
            res[key] = int(m.group(1))
    print(json.dumps(res))
    if tmp:
        os.unlink(path)


if __name__ == "__main__":
    main()
