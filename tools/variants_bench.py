"""The variant call on a device-resident pileup (include/msw.h, "Variants").
One process, one JSON line; the sibling of tools/pileup_bench.py and the same
pileup: 40k reads of config 3's shape (150-base reads, affine, 300-base
windows) from lane file 0 of the synthetic dataset, every other read
reverse-complemented, seeded, scored on both strands, traced, packed and added
on the device over their 4 Mbase genome.

HIP events on the stream, 5 warm-up + 20 timed launches of

  count       msw_pileup_call_device with no output: the count pass, the scan of
              its 16,385 tile counts and the total
  call        the same with room for every record: count, scan and emit pass
  emit        call - count (the emit pass reads the rows a second time)
  call_dense  the whole call under thresholds that call every covered position
              with a non-reference observation (the emit pass writes)
  finish      msw_pileup_finish of a pileup holding one add (a fresh pileup per
              launch), and `summary`, the wall time of msw_pileup_summary: the
              two launches of the same build the call stands beside

and the wall time of msw_call_counts over the same counts on the host (two
calls: the count, then the fill), which uploads 128 MB per call.

The kernels' own times come from a profiler run of this script
(--kernel-trace --stats); `--steps` and `--warmup` size it.

  python3 tools/variants_bench.py [--reads 40000]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=40_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--window", type=int, default=300)
    ap.add_argument("--k", type=int, default=12)
    ap.add_argument("--cigar-stride", type=int, default=32)
    ap.add_argument("--genome-mbases", type=int, default=4)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from mini_parallel_amd import CallParams, Context, Scoring, reverse_complement
    from mini_parallel_amd.synthetic import lane_file_batch, wgs_genome
    ctx = Context(0)
    sc = Scoring(match=2, mismatch=-1, gap_open=3, gap_extend=1, affine=True, want_coords=True)
    g = wgs_genome(genome_bases=args.genome_mbases << 20)
    b = lane_file_batch(0, args.reads, genome_arr=g)
    n = b.n_pairs
    R = b.reads.copy()
    for p in range(0, n, 2):
        m = int(b.read_len[p])
        R[p, :m] = reverse_complement(R[p, :m])
    ctx.prepare(sc)
    genome = ctx.load_genome(g)
    index = ctx.build_index(genome, args.k, 64)
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream()
    s = st.cuda_stream
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    z = lambda k, t: torch.zeros(k, dtype=t, device=dev)  # noqa: E731
    d_R, d_rl = up(R), up(b.read_len.view(np.int16))
    rs, mr, W, cs = R.shape[1], int(b.read_len.max()), args.window, args.cigar_stride
    ors = (rs + 15) // 16 * 16
    wpos, votes, hits, flags = z(n, torch.int64), z(n, torch.int32), z(n, torch.int32), z(n, torch.uint8)
    score, ei, ej = z(n, torch.int32), z(n, torch.int16), z(n, torch.int16)
    strand, rc, oriented = z(n, torch.uint8), z(n * ors, torch.uint8), z(n * ors, torch.uint8)
    si, sj, nc, rows = z(n, torch.int16), z(n, torch.int16), z(n, torch.int32), z(n * cs, torch.int32)
    cap = n * (cs + 2)
    ref, nm, off, ops, ovf = z(n, torch.int64), z(n, torch.int32), z(n + 1, torch.int32), z(cap, torch.int32), z(1, torch.int32)
    # the batch's records, once: reverse complements, seeds, both-strand scores with end cells, trace, pack
    ctx.revcomp_device(d_R.data_ptr(), d_rl.data_ptr(), rs, n, rc.data_ptr(), ors, s)
    ctx.seed_reads_device(index, d_R.data_ptr(), d_rl.data_ptr(), rs, n, mr, wpos.data_ptr(), votes.data_ptr(),
                          hits.data_ptr(), flags.data_ptr(), rc_reads_ptr=rc.data_ptr(), rc_stride=ors, window=W, stream=s)
    ctx.align_reads_strands_device(genome, d_R.data_ptr(), d_rl.data_ptr(), rs, wpos.data_ptr(), n, W, mr,
                                   score.data_ptr(), strand.data_ptr(), oriented.data_ptr(), ors, sc, ei.data_ptr(),
                                   ej.data_ptr(), 0, s)
    ctx.trace_reads_device(genome, oriented.data_ptr(), d_rl.data_ptr(), ors, wpos.data_ptr(), n, W, mr, score.data_ptr(),
                           ei.data_ptr(), ej.data_ptr(), si.data_ptr(), sj.data_ptr(), nc.data_ptr(), rows.data_ptr(), cs,
                           sc, s)
    ctx.aln_pack_device(genome, oriented.data_ptr(), d_rl.data_ptr(), ors, wpos.data_ptr(), n, score.data_ptr(),
                        ei.data_ptr(), ej.data_ptr(), si.data_ptr(), sj.data_ptr(), nc.data_ptr(), rows.data_ptr(), cs,
                        ref.data_ptr(), nm.data_ptr(), off.data_ptr(), ops.data_ptr(), cap, ovf.data_ptr(), s)
    torch.cuda.synchronize()

    def add_to(pile):
        pile.add_device(oriented.data_ptr(), d_rl.data_ptr(), ors, n, ref.data_ptr(), nm.data_ptr(), off.data_ptr(),
                        ops.data_ptr(), cap, strand.data_ptr(), 0, 0, s)

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

    glen = int(g.shape[0])
    rec = {"row": "variants", "shape": "config 3 (150 x 300, affine)", "reads": n, "genome_bases": glen,
           "steps": args.steps, "warmup": args.warmup}
    # the fold and the summary of this build, as tools/pileup_bench.py times them
    ms = []
    for k in range(args.warmup + args.steps):
        pile = ctx.pileup(genome)
        add_to(pile)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        pile.finish(s)
        e1.record(st)
        torch.cuda.synchronize()
        if k >= args.warmup:
            ms.append(e0.elapsed_time(e1))
        if k + 1 < args.warmup + args.steps:
            pile.close()
    rec["finish_ms"] = round(sum(ms) / len(ms), 4)
    walls = []
    for k in range(args.warmup + args.steps):
        t0 = time.perf_counter()
        pile.summary(4)
        if k >= args.warmup:
            walls.append((time.perf_counter() - t0) * 1e3)
    rec["summary_wall_ms"] = round(sum(walls) / len(walls), 4)
    # the call: defaults, then thresholds under which the emit pass has records to write
    dense = CallParams(min_depth=1, min_alt=1, min_alt_permille=0, min_qual=0, prior_het=0, prior_hom=0)
    total_d = torch.zeros(1, dtype=torch.int64, device=dev)
    for name, q in (("", None), ("_dense", dense)):
        records = len(pile.call(q).pos)
        out = torch.zeros(max(records, 1) * 48, dtype=torch.uint8, device=dev)
        rec["records" + name] = records
        if not name:
            rec["count_ms"] = timed(lambda: pile.call_device(0, 0, total_d.data_ptr(), q, s))
        rec["call%s_ms" % name] = timed(lambda: pile.call_device(out.data_ptr(), records, total_d.data_ptr(), q, s))
        assert int(total_d.item()) == records
    rec["emit_ms"] = round(rec["call_ms"] - rec["count_ms"], 4)
    # what a pass reads: the 32-byte rows and the genome bytes
    pass_bytes = glen * 33
    rec["pass_bytes"] = pass_bytes
    rec["count_gb_s"] = round(pass_bytes / rec["count_ms"] / 1e6, 1)
    rec["call_gb_s"] = round(2 * pass_bytes / rec["call_ms"] / 1e6, 1)
    # the host form over the same counts: two calls, each uploading every row
    counts = pile.counts()
    walls = []
    for k in range(3):
        t0 = time.perf_counter()
        v = ctx.call_variants(g, counts)
        walls.append(round((time.perf_counter() - t0) * 1e3, 2))
    assert len(v.pos) == rec["records"]
    rec["call_counts_wall_ms"] = walls
    rec["counts_checksum"] = int(counts.astype(np.uint64).sum())
    print(json.dumps(rec), flush=True)
    pile.close()
    index.close()
    genome.close()
    ctx.close()


if __name__ == "__main__":
    main()
