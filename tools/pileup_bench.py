"""The pileup on a device-resident batch (include/msw.h, "Pileup").  One
process, one JSON line; ``--planes`` runs the same with the device counts as
eight planes instead of rows of eight (MSW_PILEUP_PLANES=1), so two runs give
the layout comparison of DESIGN.md 4.14.

40k reads of config 3's shape (150-base reads, affine, 300-base windows) from
lane file 0 of the synthetic dataset, every other read reverse-complemented,
resident in HBM beside their 4 Mbase genome and its index; seeded, scored on
both strands, traced and packed on the device.  HIP events on the stream,
5 warm-up + 20 timed launches of

  strands     msw_align_reads_strands_device of the batch (its scoring time)
  pack        msw_aln_pack_device of the batch (the yardstick: the launch the
              add stands beside in `rustseq_mini --pileup-out`)
  add         msw_pileup_add_device of the batch's records, strand and all
  contention  the same launch with every read a copy of read 0: one locus
  finish      msw_pileup_finish of a pileup holding one add (a fresh pileup per
              launch: the fold runs once per pileup)
  summary     msw_pileup_summary, wall time of the synchronous call
  add_qual    msw_pileup_add_qual_device (threshold 20) of the same records with
              quality rows, "binned" (NovaSeq-style, 84 % one value) and
              "illumina" (drifting, noisy) as synthetic.py writes them
  add_qsum    the same on a MSW_PILEUP_QSUM pileup, at
              thresholds 0 and 20, alternated with add_qual; qsum_atomics_per_read
              is the number of d_q adds the quality rows ask for (changes between
              neighbouring bases, the first and the last column), an upper bound
              that takes every read for one M run
  finish_qsum msw_pileup_finish of such a pileup (one more scan and fold)

  python3 tools/pileup_bench.py [--planes] [--reads 40000]"""
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
    ap.add_argument("--planes", action="store_true")
    args = ap.parse_args()
    if args.planes:
        os.environ["MSW_PILEUP_PLANES"] = "1"       # read once, when the context is created
    else:
        os.environ.pop("MSW_PILEUP_PLANES", None)
    sys.path.insert(0, ROOT)
    import torch
    from mini_parallel_amd import Context, Scoring, reverse_complement
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

    def strands():
        ctx.align_reads_strands_device(genome, d_R.data_ptr(), d_rl.data_ptr(), rs, wpos.data_ptr(), n, W, mr,
                                       score.data_ptr(), strand.data_ptr(), oriented.data_ptr(), ors, sc, ei.data_ptr(),
                                       ej.data_ptr(), 0, s)

    strands()
    ctx.trace_reads_device(genome, oriented.data_ptr(), d_rl.data_ptr(), ors, wpos.data_ptr(), n, W, mr, score.data_ptr(),
                           ei.data_ptr(), ej.data_ptr(), si.data_ptr(), sj.data_ptr(), nc.data_ptr(), rows.data_ptr(), cs,
                           sc, s)

    def pack():
        ctx.aln_pack_device(genome, oriented.data_ptr(), d_rl.data_ptr(), ors, wpos.data_ptr(), n, score.data_ptr(),
                            ei.data_ptr(), ej.data_ptr(), si.data_ptr(), sj.data_ptr(), nc.data_ptr(), rows.data_ptr(), cs,
                            ref.data_ptr(), nm.data_ptr(), off.data_ptr(), ops.data_ptr(), cap, ovf.data_ptr(), s)

    pack()
    torch.cuda.synchronize()
    h_nm, h_off = nm.cpu().numpy(), off.cpu().numpy().view(np.uint32)
    total_ops = int(h_off[n])
    # every read a copy of read `one` (the first with a record): the same words for every wave
    one = int(np.flatnonzero((ref.cpu().numpy() >= 0) & (h_nm >= 0))[0])
    k1 = int(h_off[one + 1] - h_off[one])
    c_rows = oriented.view(n, ors)[one].repeat(n)
    c_rl, c_ref, c_nm = d_rl[one].repeat(n), ref[one].repeat(n), nm[one].repeat(n)
    c_strand = strand[one].repeat(n)
    c_off = up((np.arange(n + 1, dtype=np.int64) * k1).astype(np.uint32).view(np.int32))
    c_ops = ops[int(h_off[one]):int(h_off[one + 1])].repeat(n)
    torch.cuda.synchronize()

    def add_to(pile):
        pile.add_device(oriented.data_ptr(), d_rl.data_ptr(), ors, n, ref.data_ptr(), nm.data_ptr(), off.data_ptr(),
                        ops.data_ptr(), cap, strand.data_ptr(), 0, 0, s)

    def contend_to(pile):
        pile.add_device(c_rows.data_ptr(), c_rl.data_ptr(), ors, n, c_ref.data_ptr(), c_nm.data_ptr(), c_off.data_ptr(),
                        c_ops.data_ptr(), n * k1, c_strand.data_ptr(), 0, 0, s)

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

    rec = {"row": "pileup", "layout": "planes" if args.planes else "rows8", "shape": "config 3 (150 x 300, affine)",
           "reads": n, "genome_bases": int(g.shape[0]), "steps": args.steps, "warmup": args.warmup,
           "ops": total_ops, "nm_sum": int(h_nm[h_nm > 0].sum()), "reads_with_record": int((h_nm >= 0).sum())}
    rec["strands_ms"] = timed(strands)      # the batch's scoring on both strands, with end cells
    rec["pack_ms"] = timed(pack)
    pile = ctx.pileup(genome)
    rec["counts_device"] = list(pile.counts_device()[1:])
    rec["add_ms"] = timed(lambda: add_to(pile))
    rec["add_over_pack"] = round(rec["add_ms"] / rec["pack_ms"], 3)
    rec["add_over_strands"] = round(rec["add_ms"] / rec["strands_ms"], 4)
    rec["contention_ms"] = timed(lambda: contend_to(pile))
    pile.close()
    # the fold: one per pileup, so each launch gets a pileup of its own with one add in it
    ms = []
    for k in range(args.warmup + args.steps):
        pk = ctx.pileup(genome)
        add_to(pk)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        pk.finish(s)
        e1.record(st)
        torch.cuda.synchronize()
        if k >= args.warmup:
            ms.append(e0.elapsed_time(e1))
        if k + 1 < args.warmup + args.steps:
            pk.close()
    rec["finish_ms"] = round(sum(ms) / len(ms), 4)

    # quality rows in the order of the reads as given, one per read, stride rs
    def quality_rows(kind):
        rng = np.random.default_rng(5)
        rl = b.read_len.astype(np.int64)
        if kind == "binned":
            q = rng.choice(np.frombuffer(b"F:,#", np.uint8), (n, rs), p=[0.84, 0.11, 0.04, 0.01])
        else:
            q = (np.clip(40 - np.arange(rs)[None, :] // 12 + rng.integers(-6, 3, (n, rs)), 2, 41) + 33).astype(np.uint8)
        inside = np.arange(rs)[None, :] < rl[:, None]
        changes = ((q[:, 1:] != q[:, :-1]) & inside[:, 1:]).sum() + 2 * n
        return up(q), round(float(changes) / n, 2)

    def add_qual_to(pile, d_q, min_baseq):
        pile.add_device(oriented.data_ptr(), d_rl.data_ptr(), ors, n, ref.data_ptr(), nm.data_ptr(), off.data_ptr(),
                        ops.data_ptr(), cap, strand.data_ptr(), 0, 0, s, d_q.data_ptr(), rs, min_baseq)

    for kind in ("binned", "illumina"):
        d_q, per_read = quality_rows(kind)
        rec["qsum_atomics_per_read_" + kind] = per_read
        plain, flagged = ctx.pileup(genome), ctx.pileup(genome, qsum=True)
        runs = {"add_qual_ms": [], "add_qsum_ms": [], "add_qsum_q0_ms": []}
        for _ in range(3):                      # alternated: one process, the same clocks
            runs["add_qual_ms"].append(timed(lambda: add_qual_to(plain, d_q, 20)))
            runs["add_qsum_ms"].append(timed(lambda: add_qual_to(flagged, d_q, 20)))
            runs["add_qsum_q0_ms"].append(timed(lambda: add_qual_to(flagged, d_q, 0)))
        for k, v in runs.items():
            rec[k + "_" + kind] = sorted(v)[1]
            rec[k + "_" + kind + "_runs"] = v
        plain.close()
        flagged.close()
    ms = []
    for k in range(args.warmup + args.steps):
        pq = ctx.pileup(genome, qsum=True)
        add_qual_to(pq, d_q, 0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        pq.finish(s)
        e1.record(st)
        torch.cuda.synchronize()
        if k >= args.warmup:
            ms.append(e0.elapsed_time(e1))
        if k + 1 < args.warmup + args.steps:
            pq.close()
    rec["finish_qsum_ms"] = round(sum(ms) / len(ms), 4)
    rec["qsum_checksum"] = int(pq.qsums().astype(np.uint64).sum())
    pq.close()
    walls = []
    for k in range(args.warmup + args.steps):
        t0 = time.perf_counter()
        summ = pk.summary(4)
        if k >= args.warmup:
            walls.append((time.perf_counter() - t0) * 1e3)
    rec["summary_wall_ms"] = round(sum(walls) / len(walls), 4)
    rec["summary"] = summ
    t0 = time.perf_counter()
    counts = pk.counts()
    rec["counts_copy_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    rec["counts_checksum"] = int(counts.astype(np.uint64).sum())
    print(json.dumps(rec), flush=True)
    pk.close()
    index.close()
    genome.close()
    ctx.close()


if __name__ == "__main__":
    main()
