"""Alignment records on a device-resident batch: 40k reads of config 3's shape
(150-base reads, 300-base windows, affine) resident in HBM beside the genome
they come from.  Each launch is timed with HIP events on its stream, 5 warm-up
+ 20 timed launches:

  score          msw_align_reads_device with coordinates
  cut_trace      msw_genome_cut_device + msw_trace_batch_device (windows cut
                 into a slab first: the only way to trace genome windows
                 before msw_trace_reads_device)
  trace_reads    msw_trace_reads_device (windows read from the genome)
  pack           msw_aln_pack_device

cut_trace and trace_reads alternate over --rounds rounds in one process, so
their ranges can be compared.  --mode parent times cut_trace only and needs
nothing newer than the traceback itself: with --root it runs against another
checkout's package and library (an A/B against the commit before the feature,
alternating processes).  One JSON line.
  python3 tools/aln_bench.py [--reads 40000] [--rounds 5] [--stride 16] [--mode all|parent] [--root DIR]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=40_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--stride", type=int, default=16, help="CIGAR ops per read the trace rows hold")
    ap.add_argument("--window", type=int, default=300)
    ap.add_argument("--mode", choices=("all", "parent"), default="all")
    ap.add_argument("--root", default=ROOT, help="checkout whose mini_parallel_amd is imported")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    from mini_parallel_amd import AFFINE, Context
    from mini_parallel_amd._lib import OutT, check, lib
    from mini_parallel_amd.synthetic import lane_file_batch, wgs_genome
    sc = AFFINE
    g = wgs_genome()
    b = lane_file_batch(0, args.reads, genome_arr=g)
    n = b.n_pairs
    ctx = Context(0)
    ctx.prepare(sc)
    genome = ctx.load_genome(g)
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream()
    s = st.cuda_stream
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_R, d_rl, d_pos = up(b.reads), up(b.read_len.view(np.int16)), up(b.pos.astype(np.int64))
    rs, mr, W = b.reads.shape[1], int(b.read_len.max()), args.window
    ws = (W + 15) // 16 * 16
    d_want = up(np.full(n, W, np.uint16).view(np.int16))
    d_wins = torch.zeros(n * ws, dtype=torch.uint8, device=dev)
    d_wl = torch.zeros(n, dtype=torch.int16, device=dev)
    score = torch.zeros(n, dtype=torch.int32, device=dev)
    ei, ej, si, sj = (torch.zeros(n, dtype=torch.int16, device=dev) for _ in range(4))
    nc = torch.zeros(n, dtype=torch.int32, device=dev)
    rows = torch.zeros(n * args.stride, dtype=torch.int32, device=dev)
    out = OutT(score.data_ptr(), ei.data_ptr(), ej.data_ptr())
    sc_c = sc.to_c()

    def score_launch():
        check(lib().msw_align_reads_device(ctx.handle, ctypes.byref(sc_c), genome.handle, d_R.data_ptr(),
                                           d_rl.data_ptr(), rs, d_pos.data_ptr(), n, W, mr, ctypes.byref(out), None,
                                           ctypes.c_void_p(s)))

    def cut_trace():
        genome.cut_device(d_pos.data_ptr(), d_want.data_ptr(), n, d_wins.data_ptr(), ws, d_wl.data_ptr(), s)
        ctx.trace_batch_device(d_R.data_ptr(), d_rl.data_ptr(), d_wins.data_ptr(), d_wl.data_ptr(), rs, ws, n,
                               score.data_ptr(), ei.data_ptr(), ej.data_ptr(), si.data_ptr(), sj.data_ptr(),
                               nc.data_ptr(), rows.data_ptr(), args.stride, mr, W, sc, s)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(args.steps):
            fn()
        e1.record(st)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.steps

    rec = {"shape": "config 3 (150 x 300, affine)", "reads": n, "steps": args.steps, "warmup": args.warmup,
           "rounds": args.rounds, "stride": args.stride, "mode": args.mode}
    rec["score_ms"] = round(timed(score_launch), 4)          # also leaves the ends in place for the traces
    if args.mode == "parent":
        rec["cut_trace_ms"] = [round(timed(cut_trace), 4) for _ in range(args.rounds)]
        print(json.dumps(rec), flush=True)
        return

    def trace_reads():
        ctx.trace_reads_device(genome, d_R.data_ptr(), d_rl.data_ptr(), rs, d_pos.data_ptr(), n, W, mr,
                               score.data_ptr(), ei.data_ptr(), ej.data_ptr(), si.data_ptr(), sj.data_ptr(),
                               nc.data_ptr(), rows.data_ptr(), args.stride, sc, s)

    cap = n * (args.stride + 2)
    ref = torch.zeros(n, dtype=torch.int64, device=dev)
    nm = torch.zeros(n, dtype=torch.int32, device=dev)
    off = torch.zeros(n + 1, dtype=torch.int32, device=dev)
    ops = torch.zeros(cap, dtype=torch.int32, device=dev)
    ovf = torch.zeros(1, dtype=torch.int32, device=dev)

    def pack():
        ctx.aln_pack_device(genome, d_R.data_ptr(), d_rl.data_ptr(), rs, d_pos.data_ptr(), n, score.data_ptr(),
                            ei.data_ptr(), ej.data_ptr(), si.data_ptr(), sj.data_ptr(), nc.data_ptr(), rows.data_ptr(),
                            args.stride, ref.data_ptr(), nm.data_ptr(), off.data_ptr(), ops.data_ptr(), cap,
                            ovf.data_ptr(), s)

    old, new = [], []
    for _ in range(args.rounds):
        old.append(round(timed(cut_trace), 4))
        new.append(round(timed(trace_reads), 4))
    rec["cut_trace_ms"], rec["trace_reads_ms"] = old, new
    rec["pack_ms"] = round(timed(pack), 4)
    total = int(off.cpu().numpy().view(np.uint32)[n])
    packed_bytes = 8 + 4 + 4 + 4.0 * total / n               # ref_pos, nm, offset, ops
    rec.update({
        "trace_reads_over_score": round(min(new) / rec["score_ms"], 2),
        "ops_per_read": round(total / n, 3), "overflowed_reads": int(ovf.cpu()[0]),
        "mean_nm": round(float(nm.cpu().numpy().clip(0).mean()), 3),
        "copy_back_bytes_per_read_packed": round(packed_bytes, 2),
        "copy_back_bytes_per_read_padded": 2 + 2 + 4 + 4 * args.stride,   # start_i, start_j, n_cigar, the row
        "records_per_s": round(n / ((min(new) + rec["pack_ms"]) * 1e-3)),
    })
    print(json.dumps(rec), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
