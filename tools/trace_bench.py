"""Traceback throughput on a device-resident batch (sw_trace_kernel,
msw_trace.hip): config 3's shape by default (150 x 300, affine), 40k pairs in
HBM.  Times the scoring launch with coordinates (msw_align_batch_device) and
the trace launch after it (msw_trace_batch_device) on the same batch in the
same process, each with HIP events on the launch stream after a warm-up, and
the two back to back.  One JSON line: alignments/s and the trace launch's time
as a multiple of the score + coords launch (the yardstick).
  python3 tools/trace_bench.py [--pairs 40000] [--config 3] [--steps 20] [--warmup 5] [--linear]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=40_000)
    ap.add_argument("--config", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--stride", type=int, default=32, help="CIGAR ops per pair the rows hold")
    ap.add_argument("--linear", action="store_true", help="the reference's linear scheme instead of config 3's affine")
    args = ap.parse_args()
    import torch
    from mini_parallel_amd import AFFINE, LINEAR_COORDS, Context
    from mini_parallel_amd.synthetic import config_batch
    sc = LINEAR_COORDS if args.linear else AFFINE
    b = config_batch(args.config, n_pairs=args.pairs)
    n = b.n_pairs
    ctx = Context(0)
    ctx.prepare(sc)
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream()
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in
         (b.reads, b.wins, b.read_len.view(np.int16), b.win_len.view(np.int16))]
    score = torch.zeros(n, dtype=torch.int32, device=dev)
    ei, ej, si, sj = (torch.zeros(n, dtype=torch.int16, device=dev) for _ in range(4))
    nc = torch.zeros(n, dtype=torch.int32, device=dev)
    cig = torch.zeros(n * args.stride, dtype=torch.int32, device=dev)
    mr, mw = int(b.read_len.max()), int(b.win_len.max())
    geom = (t[0].data_ptr(), t[2].data_ptr(), t[1].data_ptr(), t[3].data_ptr(), b.reads.shape[1], b.wins.shape[1], n)

    def score_launch():
        ctx.align_batch_device(*geom, score.data_ptr(), mr, mw, sc, ei.data_ptr(), ej.data_ptr(), st.cuda_stream)

    def trace_launch():
        ctx.trace_batch_device(*geom, score.data_ptr(), ei.data_ptr(), ej.data_ptr(), si.data_ptr(), sj.data_ptr(),
                               nc.data_ptr(), cig.data_ptr(), args.stride, mr, mw, sc, st.cuda_stream)

    def both():
        score_launch()
        trace_launch()

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

    score_ms = timed(score_launch)   # also leaves the ends in place for the trace
    trace_ms = timed(trace_launch)
    both_ms = timed(both)
    h_nc, h_ei, h_ej = nc.cpu().numpy(), ei.cpu().numpy().astype(np.int64), ej.cpu().numpy().astype(np.int64)
    cells = float((b.read_len.astype(np.int64) * b.win_len).sum())
    print(json.dumps({
        "shape": f"config {args.config}", "scheme": "linear" if args.linear else "affine", "pairs": n,
        "steps": args.steps, "warmup": args.warmup,
        "score_coords_ms": round(score_ms, 4), "trace_ms": round(trace_ms, 4), "score_then_trace_ms": round(both_ms, 4),
        "trace_over_score": round(trace_ms / score_ms, 2),
        "alignments_per_s": round(n / (both_ms * 1e-3)), "trace_only_alignments_per_s": round(n / (trace_ms * 1e-3)),
        "score_tcups": round(cells / (score_ms * 1e9), 2),
        "traced_cells_share": round(float(((h_ei + 1) * (h_ej + 1)).sum()) / cells, 3),
        "mean_ops": round(float(h_nc.mean()), 2), "max_ops": int(h_nc.max()),
        "overflowed_pairs": int((h_nc > args.stride).sum()),
    }), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
