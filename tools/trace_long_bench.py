"""Long-pair traceback throughput on device-resident batches (sw_trace_long_kernel,
msw_trace_long.hip): 4k pairs of 1000 x 2000 and the mixed-long batch (8k reads
of 257..2000 bases x 2m), linear and affine.  Times the scoring launch with
coordinates (msw_align_batch_device: the long-pair kernel for these bounds),
the trace launch after it (msw_trace_long_batch_device) and the two back to
back, each with HIP events on the launch stream after a warm-up.  One JSON
line per shape and scheme.  MSW_LIB_PATH selects another build of the library
(one compiled with -DMSW_TRACE_LONG_NO_WALK times the fills alone).
  python3 tools/trace_long_bench.py [--steps 20] [--warmup 5] [--only mixed] [--stride 64]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--stride", type=int, default=64, help="CIGAR ops per pair the rows hold")
    ap.add_argument("--only", default="", help="run the shapes whose name contains this")
    args = ap.parse_args()
    import torch
    from mini_parallel_amd import Context, Scoring
    from mini_parallel_amd.synthetic import make_pairs
    ctx = Context(0)
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream()
    schemes = {"linear": Scoring(want_coords=True),
               "affine": Scoring(affine=True, gap_open=3, gap_extend=1, want_coords=True)}
    for name, n, m in (("1000x2000", 4096, 1000), ("mixed_257-2000x2", 8192, (257, 2000))):
        if args.only not in name:
            continue
        b = make_pairs(n, m, win_factor=2.0, seed=4242)
        t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in
             (b.reads, b.wins, b.read_len.view(np.int16), b.win_len.view(np.int16))]
        score = torch.zeros(n, dtype=torch.int32, device=dev)
        ei, ej, si, sj = (torch.zeros(n, dtype=torch.int16, device=dev) for _ in range(4))
        nc = torch.zeros(n, dtype=torch.int32, device=dev)
        cig = torch.zeros(n * args.stride, dtype=torch.int32, device=dev)
        mr, mw = int(b.read_len.max()), int(b.win_len.max())
        geom = (t[0].data_ptr(), t[2].data_ptr(), t[1].data_ptr(), t[3].data_ptr(), b.reads.shape[1], b.wins.shape[1], n)
        cells = float((b.read_len.astype(np.int64) * b.win_len).sum())
        for sname, sc in schemes.items():
            ctx.prepare(sc)

            def score_launch():
                ctx.align_batch_device(*geom, score.data_ptr(), mr, mw, sc, ei.data_ptr(), ej.data_ptr(), st.cuda_stream)

            def trace_launch():
                ctx.trace_batch_device(*geom, score.data_ptr(), ei.data_ptr(), ej.data_ptr(), si.data_ptr(),
                                       sj.data_ptr(), nc.data_ptr(), cig.data_ptr(), args.stride, mr, mw, sc,
                                       st.cuda_stream, long_pairs=True)

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
            h_nc = nc.cpu().numpy()
            h_ei, h_ej = ei.cpu().numpy().astype(np.int64), ej.cpu().numpy().astype(np.int64)
            print(json.dumps({
                "shape": name, "scheme": sname, "pairs": n, "steps": args.steps, "warmup": args.warmup,
                "lib": os.path.basename(os.path.dirname(os.environ.get("MSW_LIB_PATH", ""))) or "in-tree",
                "score_coords_ms": round(score_ms, 4), "trace_ms": round(trace_ms, 4),
                "score_then_trace_ms": round(both_ms, 4), "trace_over_score": round(trace_ms / score_ms, 2),
                "alignments_per_s": round(n / (both_ms * 1e-3)), "score_tcups": round(cells / (score_ms * 1e9), 2),
                "traced_cells_share": round(float(((h_ei + 1) * (h_ej + 1)).sum()) / cells, 3),
                "mean_ops": round(float(h_nc.mean()), 2), "max_ops": int(h_nc.max()),
                "overflowed_pairs": int((h_nc > args.stride).sum()),
            }), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
