"""Banded scoring against the full window on one device-resident batch: reads
of a seeded lane file resident in HBM beside their genome, every launch timed
with HIP events on one stream (--warmup launches, then enough launches to fill
--min-ms), the full-window call and the banded calls alternated over --rounds
rounds in one process so their ranges can be compared.

  full       msw_align_reads_device, window 2 x read length (the long-pair
             kernel at 1000 bases)
  band w     msw_align_reads_banded_device at half-width w, centred 3 off the
             diagonal of the full call's best cell
  trace      score + msw_trace_reads_device against the banded call with `tr`
             (score, best cell and traceback in one launch), 150 bases, w = 16

Each case runs linear score-only and affine with the best cell.  `same` is the
share of reads whose banded score equals the full one.  One JSON line per case.
  python3 tools/band_bench.py [--cases 10000x150,1000000x150,4000x1000] [--rounds 5]

--end-to-end times msw_align_reads_banded_e2e_device against the local banded
call instead, the two alternated at every width on the same diagonals: linear
score-only, affine with the end cell, and (reads up to 1008 bases) affine score
+ trace at w = 16.  `aligned` is the share of reads the end-to-end call aligns."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNPLACED = -(1 << 63)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="10000x150,1000000x150,4000x1000")
    ap.add_argument("--widths", default="8,16,32")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--min-ms", type=float, default=300.0, help="GPU time a timed window should fill")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--stride", type=int, default=16, help="CIGAR ops per read the trace rows hold")
    ap.add_argument("--end-to-end", action="store_true", help="the end-to-end launch against the local banded one")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from mini_parallel_amd import AFFINE, LINEAR, Context
    from mini_parallel_amd._lib import OutT, TraceT, check, lib
    from mini_parallel_amd.synthetic import lane_file_batch, wgs_genome
    g = wgs_genome()
    ctx = Context(0)
    genome = ctx.load_genome(g)
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream()
    s = ctypes.c_void_p(st.cuda_stream)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        steps, ms = 2, 0.0
        while True:  # grow the window until it fills min-ms
            e0.record(st)
            for _ in range(steps):
                fn()
            e1.record(st)
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1)
            if ms >= args.min_ms or steps >= 4096:
                return ms / steps
            steps = min(4096, max(steps * 2, int(steps * args.min_ms / max(ms, 1e-3)) + 1))

    for case in args.cases.split(","):
        n, L = (int(x) for x in case.split("x"))
        b = lane_file_batch(0, n, read_len=L, genome_arr=g)
        n, rs, mr, W = b.n_pairs, b.reads.shape[1], int(b.read_len.max()), 2 * L
        d_R, d_rl, d_pos = up(b.reads), up(b.read_len.view(np.int16)), up(b.pos.astype(np.int64))
        score, score_b = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(2))
        ei, ej, bi, bj, si, sj = (torch.zeros(n, dtype=torch.int16, device=dev) for _ in range(6))
        nc = torch.zeros(n, dtype=torch.int32, device=dev)
        out, out_b = OutT(score.data_ptr(), ei.data_ptr(), ej.data_ptr()), OutT(score_b.data_ptr(), bi.data_ptr(), bj.data_ptr())
        d_diag = torch.zeros(n, dtype=torch.int64, device=dev)

        def full(sc_c):
            check(lib().msw_align_reads_device(ctx.handle, ctypes.byref(sc_c), genome.handle, d_R.data_ptr(),
                                               d_rl.data_ptr(), rs, d_pos.data_ptr(), n, W, mr, ctypes.byref(out),
                                               None, s))

        def band(sc_c, w, tr=None, e2e=False):
            fn = lib().msw_align_reads_banded_e2e_device if e2e else lib().msw_align_reads_banded_device
            check(fn(ctx.handle, ctypes.byref(sc_c), genome.handle, d_R.data_ptr(), d_rl.data_ptr(), rs,
                     d_diag.data_ptr(), n, w, mr, ctypes.byref(out_b), None, None, tr, s))

        def against_local(rec, sc_c, w, tr=None):
            """local and end-to-end launches alternated; ms per launch and pairs/s, min-max over the rounds"""
            ms = {False: [], True: []}
            for _ in range(args.rounds):
                for e2e in (False, True):
                    ms[e2e].append(round(timed(lambda: band(sc_c, w, tr, e2e)), 4))
            rec[f"w{w}_local_ms"], rec[f"w{w}_e2e_ms"] = ms[False], ms[True]
            for e2e, key in ((False, "local"), (True, "e2e")):
                rec[f"w{w}_{key}_pairs_per_s"] = [round(n / (max(ms[e2e]) * 1e-3)), round(n / (min(ms[e2e]) * 1e-3))]
            rec[f"w{w}_e2e_over_local"] = round(min(ms[True]) / min(ms[False]), 3)
            torch.cuda.synchronize()   # the last timed launch was end to end
            rec[f"w{w}_aligned"] = round(float((score_b.cpu().numpy() > -(1 << 31)).mean()), 4)

        if args.end_to_end:
            aff_c = AFFINE.to_c()
            full(aff_c)  # the diagonals: the affine best cell's, 3 off centre
            torch.cuda.synchronize()
            c = (b.pos.astype(np.int64) + ej.cpu().numpy() - ei.cpu().numpy() + 3)
            c[score.cpu().numpy() <= 0] = UNPLACED
            d_diag.copy_(up(c))
            widths = [int(x) for x in args.widths.split(",")] if L <= 384 else [32]
            for name, sc in (("linear score", LINEAR), ("affine + end cell", AFFINE)):
                rec = {"case": case, "scheme": name, "reads": n, "rounds": args.rounds}
                for w in widths:
                    against_local(rec, sc.to_c(), w)
                print(json.dumps(rec), flush=True)
            if mr <= 1008:
                rows = torch.zeros(n * args.stride, dtype=torch.int32, device=dev)
                tr = TraceT(si.data_ptr(), sj.data_ptr(), nc.data_ptr(), rows.data_ptr(), args.stride)
                rec = {"case": case, "scheme": "affine score + trace", "reads": n, "rounds": args.rounds}
                against_local(rec, aff_c, 16, ctypes.byref(tr))
                print(json.dumps(rec), flush=True)
            continue

        for name, sc in (("linear score", LINEAR), ("affine + best cell", AFFINE)):
            sc_c, aff_c = sc.to_c(), AFFINE.to_c()
            full(aff_c)  # the diagonals: the affine best cell's, 3 off centre
            torch.cuda.synchronize()
            c = (b.pos.astype(np.int64) + ej.cpu().numpy() - ei.cpu().numpy() + 3)
            c[score.cpu().numpy() <= 0] = UNPLACED
            d_diag.copy_(up(c))
            full(sc_c)
            torch.cuda.synchronize()
            want = score.cpu().numpy().copy()
            rec = {"case": case, "scheme": name, "reads": n, "rounds": args.rounds, "full_ms": []}
            widths = [int(x) for x in args.widths.split(",")] if L <= 384 else [32]
            for w in widths:
                rec[f"band{w}_ms"] = []
            for _ in range(args.rounds):
                rec["full_ms"].append(round(timed(lambda: full(sc_c)), 4))
                for w in widths:
                    rec[f"band{w}_ms"].append(round(timed(lambda: band(sc_c, w)), 4))
            for w in widths:
                band(sc_c, w)
                torch.cuda.synchronize()
                rec[f"band{w}_same"] = round(float((score_b.cpu().numpy() == want).mean()), 4)
                rec[f"band{w}_speedup"] = round(min(rec["full_ms"]) / min(rec[f"band{w}_ms"]), 3)
                rec[f"band{w}_pairs_per_s"] = round(n / (min(rec[f"band{w}_ms"]) * 1e-3))
            rec["full_pairs_per_s"] = round(n / (min(rec["full_ms"]) * 1e-3))
            rec["full_spread_ms"] = round(max(rec["full_ms"]) - min(rec["full_ms"]), 4)
            print(json.dumps(rec), flush=True)

        if L == 150:  # score + trace: two launches on the parent's path, one banded launch
            rows = torch.zeros(n * args.stride, dtype=torch.int32, device=dev)
            tr = TraceT(si.data_ptr(), sj.data_ptr(), nc.data_ptr(), rows.data_ptr(), args.stride)
            aff_c = AFFINE.to_c()

            def score_trace():
                full(aff_c)
                check(lib().msw_trace_reads_device(ctx.handle, ctypes.byref(aff_c), genome.handle, d_R.data_ptr(),
                                                   d_rl.data_ptr(), rs, d_pos.data_ptr(), n, W, mr, ctypes.byref(out),
                                                   ctypes.byref(tr), s))

            old, new = [], []
            for _ in range(args.rounds):
                old.append(round(timed(score_trace), 4))
                new.append(round(timed(lambda: band(aff_c, 16, ctypes.byref(tr))), 4))
            print(json.dumps({"case": case, "scheme": "affine score + trace", "reads": n, "score_trace_ms": old,
                              "band16_trace_ms": new, "speedup": round(min(old) / min(new), 3),
                              "spread_ms": round(max(old) - min(old), 4)}), flush=True)
    genome.close()
    ctx.close()


if __name__ == "__main__":
    main()
