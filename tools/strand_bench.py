"""Both strands on a device-resident batch: 40k reads of config 3's shape
(150-base reads, 300-base windows, affine) resident in HBM beside the genome
they come from, half of them reverse-complemented.  Each launch is timed with
HIP events on its stream, 5 warm-up + 20 timed launches:

  score          msw_align_reads_device
  strands        msw_align_reads_strands_device (cut, reverse complement, two
                 scoring passes, select)
  revcomp        the reverse-complement launch alone (msw_revcomp_device)
  select         the select launch alone (the library's internal launcher,
                 called by its C++ symbol: the C ABI has no entry for it)
  copy           hipMemcpyAsync device to device of the read slab: the yardstick
                 of the two byte movers, which move the same order of bytes

One JSON line.
  python3 tools/strand_bench.py [--reads 40000] [--coords] [--window 300]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SELECT_SYMBOL = "_ZN3msw20launch_strand_selectEPKhPKtjmPhjPiPsS6_PKiPKsSA_S4_P12ihipStream_t"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=40_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--window", type=int, default=300)
    ap.add_argument("--coords", action="store_true", help="score with best cells")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from mini_parallel_amd import Context, Scoring, reverse_complement
    from mini_parallel_amd._lib import OutT, check, lib
    from mini_parallel_amd.synthetic import lane_file_batch, wgs_genome
    sc = Scoring(match=2, mismatch=-1, gap_open=3, gap_extend=1, affine=True, want_coords=args.coords)
    g = wgs_genome()
    b = lane_file_batch(0, args.reads, genome_arr=g)
    n = b.n_pairs
    R = b.reads.copy()
    for p in range(0, n, 2):                       # every other read comes from the reverse strand
        m = int(b.read_len[p])
        R[p, :m] = reverse_complement(R[p, :m])
    ctx = Context(0)
    ctx.prepare(sc)
    genome = ctx.load_genome(g)
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream()
    s = st.cuda_stream
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_R, d_rl, d_pos = up(R), up(b.read_len.view(np.int16)), up(b.pos.astype(np.int64))
    rs, mr, W = R.shape[1], int(b.read_len.max()), args.window
    ors = (rs + 15) // 16 * 16
    z = lambda k, t: torch.zeros(k, dtype=t, device=dev)
    score, score_r = z(n, torch.int32), z(n, torch.int32)
    ei, ej, ei_r, ej_r = (z(n, torch.int16) for _ in range(4))
    strand, oriented, copy_dst = z(n, torch.uint8), z(n * ors, torch.uint8), z(n * rs, torch.uint8)
    out = OutT(score.data_ptr(), ei.data_ptr() if args.coords else None, ej.data_ptr() if args.coords else None)
    sc_c = sc.to_c()
    torch.cuda.synchronize()      # the uploads and fills above ran on torch's stream, the launches below do not
    P = ctypes.c_void_p
    select = getattr(lib(), SELECT_SYMBOL)
    select.restype = ctypes.c_int
    select.argtypes = [P, P, ctypes.c_uint32, ctypes.c_uint64, P, ctypes.c_uint32, P, P, P, P, P, P, P, P]

    def score_launch():
        check(lib().msw_align_reads_device(ctx.handle, ctypes.byref(sc_c), genome.handle, d_R.data_ptr(),
                                           d_rl.data_ptr(), rs, d_pos.data_ptr(), n, W, mr, ctypes.byref(out), None,
                                           ctypes.c_void_p(s)))

    def strands_launch():
        ctx.align_reads_strands_device(genome, d_R.data_ptr(), d_rl.data_ptr(), rs, d_pos.data_ptr(), n, W, mr,
                                       score.data_ptr(), strand.data_ptr(), oriented.data_ptr(), ors, sc,
                                       ei.data_ptr() if args.coords else 0, ej.data_ptr() if args.coords else 0, 0, s)

    def revcomp_launch():
        ctx.revcomp_device(d_R.data_ptr(), d_rl.data_ptr(), rs, n, oriented.data_ptr(), ors, s)

    def select_launch():
        # score_r holds zeros: every read takes the forward arm, the one that moves a row
        e = select(d_R.data_ptr(), d_rl.data_ptr(), rs, n, oriented.data_ptr(), ors, score.data_ptr(),
                   ei.data_ptr() if args.coords else None, ej.data_ptr() if args.coords else None, score_r.data_ptr(),
                   ei_r.data_ptr(), ej_r.data_ptr(), strand.data_ptr(), s)
        if e != 0:
            raise RuntimeError(f"launch_strand_select: hipError {e}")

    def copy_launch():
        with torch.cuda.stream(st):
            copy_dst.copy_(d_R.view(-1), non_blocking=True)         # hipMemcpyAsync, device to device

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(args.steps):
            fn()
        e1.record(st)
        torch.cuda.synchronize()
        return round(e0.elapsed_time(e1) / args.steps, 4)

    rec = {"shape": "config 3 (150 x 300, affine)", "reads": n, "steps": args.steps, "warmup": args.warmup,
           "coords": bool(args.coords), "read_stride": rs, "oriented_stride": ors}
    rec["score_ms"] = timed(score_launch)
    rec["strands_ms"] = timed(strands_launch)
    rec["reverse_reads"] = int(strand.cpu().sum())
    rec["revcomp_ms"] = timed(revcomp_launch)
    rec["select_ms"] = timed(select_launch)
    rec["copy_ms"] = timed(copy_launch)
    rec["slab_bytes"] = n * rs
    rec["strands_over_two_scores"] = round(rec["strands_ms"] / (2 * rec["score_ms"]), 3)
    rec["revcomp_over_copy"] = round(rec["revcomp_ms"] / rec["copy_ms"], 2)
    rec["select_over_copy"] = round(rec["select_ms"] / rec["copy_ms"], 2)
    print(json.dumps(rec), flush=True)
    genome.close()
    ctx.close()


if __name__ == "__main__":
    main()
