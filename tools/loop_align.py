#!/usr/bin/env python3
"""Where the 8-byte instructions of the scoring kernels' loops sit (no GPU
needed).  A lone wave runs a loop of 8-byte encodings slower when they
straddle 8-byte boundaries ("Loop alignment"); -falign-loops
fixes the header only, and every 4-byte instruction that stands alone in the
body flips the parity of what follows it.

Takes the built library (or any object / code object with gfx950 code), or
compiles one sw_kernel instance itself with the Makefile's flags, disassembles
the gfx950 code objects with ROCm's llvm-objdump and prints one JSON line per
loop (a backward s_cbranch_* whose body holds more than --min-body
instructions) of every kernel symbol:

  kernel, loop (ordinal within the kernel), header address, header_mod64,
  header_mod8, instructions, n4 (4-byte), n8_at0 / n8_at4 (8-byte encodings
  at 0 / 4 mod 8), four_byte ([index, mnemonic] of every 4-byte one; null if
  there are more than --max-four of them), kind (f16: holds v_perm_b32 table
  lookups, else integer), valu, perm (v_perm_b32),
  max3 (v_pk_maximum3_f16: zero in the staging loops, one or more per row and
  step in the DP loops) and other_size (encodings of neither 4 nor 8 bytes).

With --per-kernel: one line per kernel instead, holding its DP loops only
(max3 > 0), each as [kind, header_mod8, instructions, n4, n8_at0, n8_at4,
valu]; --changed-against FILE keeps the kernels whose line differs from FILE's.

Usage: python tools/loop_align.py [mini_parallel_amd/libmsw.so] [--kernels REGEX] [--min-body 100] [--per-kernel]
       python tools/loop_align.py --instance 13,false,false,false [--csrc DIR]
"""
from __future__ import annotations

import argparse
import json
import os
import re
import shutil
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mini_parallel_amd", "csrc")
LIB = os.path.join(ROOT, "mini_parallel_amd", "libmsw.so")
# the Makefile's device-side flags
FLAGS = ["-O3", "-std=c++17", "-fPIC", "-falign-loops=32", "--offload-arch=gfx950"]
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
MAX_FOUR = 16  # loops with more 4-byte instructions (staging, integer DP) are reported by count only


def rocm_tool(name):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for p in (os.path.join(rocm, "lib", "llvm", "bin", name), os.path.join(rocm, "llvm", "bin", name),
              os.path.join(rocm, "bin", name)):
        if os.path.exists(p):
            return p
    return shutil.which(name)


def have_tools():
    return all(rocm_tool(t) for t in ("llvm-objdump", "llvm-objcopy"))


def compile_instance(spec, out, csrc=CSRC):
    """One sw_kernel<KR, AFFINE, COORDS, SPLIT> as a gfx950 code object."""
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "one.hip")
        with open(src, "w") as f:
            f.write('#include "msw_device.h"\n'
                    f"template __global__ void msw::sw_kernel<{spec}>(msw::SwParams);\n")
        subprocess.run([rocm_tool("hipcc") or "hipcc", *FLAGS, "--cuda-device-only", "-c", "-I", csrc, "-I",
                        os.path.join(ROOT, "include"), src, "-o", out], check=True, stderr=subprocess.DEVNULL)


def code_objects(path, tmpdir):
    """Paths of the gfx950 code objects in `path`: the file itself if it is an
    AMDGPU ELF, else the gfx950 entries of every offload bundle in its
    .hip_fatbin section (one bundle per translation unit)."""
    with open(path, "rb") as f:
        head = f.read(20)
    if head[:4] == b"\x7fELF" and struct.unpack_from("<H", head, 18)[0] == 224:  # EM_AMDGPU
        return [path]
    if head.startswith(MAGIC[:20]):  # a bare bundle (hipcc --cuda-device-only -c)
        blob = open(path, "rb").read()
    else:
        blob_path = os.path.join(tmpdir, "fatbin")
        subprocess.run([rocm_tool("llvm-objcopy"), "--dump-section", f".hip_fatbin={blob_path}", path,
                        os.path.join(tmpdir, "copy")], check=True, stderr=subprocess.DEVNULL)
        blob = open(blob_path, "rb").read()
    out, pos = [], blob.find(MAGIC)
    if pos < 0 and b"CCOB" in blob:
        raise RuntimeError("compressed offload bundles: build without --offload-compress")
    while pos >= 0:
        (n,) = struct.unpack_from("<Q", blob, pos + len(MAGIC))
        q = pos + len(MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", blob, q)
            triple = blob[q + 24:q + 24 + tlen].decode()
            q += 24 + tlen
            if "gfx950" in triple and size:
                p = os.path.join(tmpdir, f"co{len(out)}.elf")
                with open(p, "wb") as f:
                    f.write(blob[pos + off:pos + off + size])
                out.append(p)
        pos = blob.find(MAGIC, pos + len(MAGIC))
    return out


LINE = re.compile(r"^\s+(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):\s*((?:[0-9A-Fa-f]{8}\s*)+)")
SYM = re.compile(r"^[0-9A-Fa-f]+ <(.*)>:\s*$")


def disassemble(co):
    """{symbol: [(address, size, mnemonic, first encoding word)]}."""
    txt = subprocess.run([rocm_tool("llvm-objdump"), "-d", "-C", co], check=True, capture_output=True,
                         text=True).stdout
    syms, cur = {}, None
    for ln in txt.splitlines():
        m = SYM.match(ln)
        if m:
            cur = syms.setdefault(m.group(1), [])
            continue
        m = LINE.match(ln)
        if m and cur is not None:
            words = m.group(4).split()
            cur.append((int(m.group(3), 16), 4 * len(words), m.group(1), int(words[0], 16)))
    return syms


def loops(insts, min_body):
    """(header index, back-edge index) of every loop: a backward s_cbranch_*
    (SOPP: target = address + 4 + 4 * simm16) with more than min_body instructions."""
    at = {a: i for i, (a, _, _, _) in enumerate(insts)}
    for i, (addr, _, op, word) in enumerate(insts):
        if not op.startswith("s_cbranch_"):
            continue
        simm = word & 0xFFFF
        simm -= 0x10000 if simm & 0x8000 else 0
        tgt = addr + 4 + 4 * simm
        if simm < 0 and tgt in at and i - at[tgt] + 1 > min_body:
            yield at[tgt], i


def report(kernel, insts, min_body, max_four=MAX_FOUR):
    # the name without its fixed parts: "sw_kernel<13, false, false, false, false>"
    kernel = re.sub(r"^void |msw::|\(.*\)$", "", kernel)
    for n, (h, b) in enumerate(loops(insts, min_body)):
        body = insts[h:b + 1]
        ops = [op for _, _, op, _ in body]
        four = [[i, op] for i, (_, s, op, _) in enumerate(body) if s == 4]
        yield {
            "kernel": kernel, "loop": n, "header": f"{body[0][0]:#x}", "header_mod64": body[0][0] % 64,
            "header_mod8": body[0][0] % 8, "instructions": len(body),
            "n4": sum(1 for _, s, _, _ in body if s == 4),
            "n8_at0": sum(1 for a, s, _, _ in body if s == 8 and a % 8 == 0),
            "n8_at4": sum(1 for a, s, _, _ in body if s == 8 and a % 8 == 4),
            "other_size": sum(1 for _, s, _, _ in body if s not in (4, 8)),
            "four_byte": four if len(four) <= max_four else None,
            "kind": "f16" if "v_perm_b32" in ops else "integer",
            "valu": sum(1 for op in ops if op.startswith("v_")),
            "perm": ops.count("v_perm_b32"),
            "max3": ops.count("v_pk_maximum3_f16"),  # the DP loops hold one or more per row and step
        }


def scan(path, kernels=".", min_body=100, max_four=MAX_FOUR):
    """The report rows of every kernel in `path` whose demangled name matches."""
    pat, rows = re.compile(kernels), []
    with tempfile.TemporaryDirectory() as d:
        for co in code_objects(path, d):
            for name, insts in disassemble(co).items():
                if pat.search(name):
                    rows += report(name, insts, min_body, max_four)
    rows.sort(key=lambda r: (r["kernel"], r["loop"]))
    return rows


PER_KERNEL = ["kind", "header_mod8", "instructions", "n4", "n8_at0", "n8_at4", "valu"]


def per_kernel(rows):
    """One row per kernel, its DP loops only (max3 > 0), each as the list of
    PER_KERNEL values: the compact form of the committed before / after records."""
    out = {}
    for r in rows:
        if r["max3"]:
            out.setdefault(r["kernel"], []).append([r[k] for k in PER_KERNEL])
    return [{"kernel": k, "dp_loops": v} for k, v in out.items()]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("path", nargs="?", default=LIB, help="library, object or code object (default: the built libmsw.so)")
    ap.add_argument("--instance", default="", help="KR,AFFINE,COORDS,SPLIT: compile this sw_kernel instance instead")
    ap.add_argument("--csrc", default=CSRC, help="directory of msw_device.h (another checkout, for before/after)")
    ap.add_argument("--kernels", default=r"msw::sw_", help="regex on the demangled kernel name")
    ap.add_argument("--min-body", type=int, default=100)
    ap.add_argument("--per-kernel", action="store_true",
                    help="one line per kernel: its DP loops as [" + ", ".join(PER_KERNEL) + "]")
    ap.add_argument("--changed-against", default="", metavar="JSONL",
                    help="with --per-kernel: only the kernels whose line differs from that of this earlier output")
    ap.add_argument("--max-four", type=int, default=MAX_FOUR, help="list the 4-byte instructions up to this many")
    args = ap.parse_args()
    if not have_tools():
        sys.exit("llvm-objdump / llvm-objcopy of ROCm not found")
    if args.instance:
        with tempfile.TemporaryDirectory() as d:
            co = os.path.join(d, "one.co")
            compile_instance(args.instance, co, args.csrc)
            rows = scan(co, args.kernels, args.min_body, args.max_four)
    else:
        rows = scan(args.path, args.kernels, args.min_body, args.max_four)
    if args.per_kernel:
        rows = per_kernel(rows)
        if args.changed_against:
            other = {ln.strip() for ln in open(args.changed_against)}
            rows = [r for r in rows if json.dumps(r) not in other]
    for r in rows:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
