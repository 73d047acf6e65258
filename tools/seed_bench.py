"""Placing reads on a device-resident batch (include/msw.h, "Placing reads").
One row per process, one JSON line each:

  --row index   the k-mer index build of a random genome of --genome-mbases
                (4 = the config genome's size, 256 = a large one): GPU time per
                pass from msw_index_info, and the wall time of msw_index_create
  --row seed    40k reads of config 3's shape (150-base reads, affine, 300-base
                windows) from lane file 0 of the synthetic dataset, every other
                read reverse-complemented, resident in HBM beside their genome
                and its index.  HIP events on the stream, 5 warm-up + 20 timed
                launches of
                  seed1     msw_seed_reads_device, forward only
                  seed2     msw_seed_reads_device with the reverse-complement slab
                  revcomp   msw_revcomp_device (what seed2's slab costs to make)
                  score     msw_align_reads_device        } the yardsticks, fed
                  strands   msw_align_reads_strands_device } with the seeded win_pos
                  cand1     msw_seed_candidates_device, forward only   } sep 0 (= W)
                  cand2     msw_seed_candidates_device with the slab   }
                  select    msw_mapq_select_device on the two strand results
                and the seed kernels' occupancy.

  python3 tools/seed_bench.py --row seed [--reads 40000] [--k 12] [--max-occ 64]
  python3 tools/seed_bench.py --row index --genome-mbases 256 [--k 12]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--row", choices=("index", "seed"), default="seed")
    ap.add_argument("--reads", type=int, default=40_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--window", type=int, default=300)
    ap.add_argument("--k", type=int, default=12)
    ap.add_argument("--max-occ", type=int, default=64)
    ap.add_argument("--band", type=int, default=16)
    ap.add_argument("--cap", type=int, default=4096)
    ap.add_argument("--genome-mbases", type=int, default=4)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from mini_parallel_amd import Context, Scoring, reverse_complement
    from mini_parallel_amd._lib import OutT, check, lib
    from mini_parallel_amd.synthetic import genome as random_genome, lane_file_batch, wgs_genome
    ctx = Context(0)
    if args.row == "index":
        g = random_genome(args.genome_mbases << 20, np.random.default_rng(1003))
        genome = ctx.load_genome(g)
        ctx.build_index(genome, args.k, args.max_occ).close()        # modules loaded, allocator warm
        t0 = time.perf_counter()
        index = ctx.build_index(genome, args.k, args.max_occ)
        wall = (time.perf_counter() - t0) * 1e3
        info = index.info()
        print(json.dumps({"row": "index", "genome_bases": int(g.shape[0]), "k": args.k, "max_occ": args.max_occ,
                          "n_pos": info["n_pos"], "n_masked": info["n_masked"],
                          "build_ms": {k: round(v, 3) for k, v in info["build_ms"].items()},
                          "build_gpu_ms": round(sum(info["build_ms"].values()), 3), "create_wall_ms": round(wall, 2)}),
              flush=True)
        index.close()
        genome.close()
        ctx.close()
        return
    sc = Scoring(match=2, mismatch=-1, gap_open=3, gap_extend=1, affine=True, want_coords=False)
    g = wgs_genome()
    b = lane_file_batch(0, args.reads, genome_arr=g)
    n = b.n_pairs
    R = b.reads.copy()
    for p in range(0, n, 2):
        m = int(b.read_len[p])
        R[p, :m] = reverse_complement(R[p, :m])
    ctx.prepare(sc)
    genome = ctx.load_genome(g)
    index = ctx.build_index(genome, args.k, args.max_occ)
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream()
    s = st.cuda_stream
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_R, d_rl = up(R), up(b.read_len.view(np.int16))
    rs, mr, W = R.shape[1], int(b.read_len.max()), args.window
    ors = (rs + 15) // 16 * 16
    z = lambda k, t: torch.zeros(k, dtype=t, device=dev)
    wpos, votes, hits, flags = z(n, torch.int64), z(n, torch.int32), z(n, torch.int32), z(n, torch.uint8)
    score, strand, rc, oriented = z(n, torch.int32), z(n, torch.uint8), z(n * ors, torch.uint8), z(n * ors, torch.uint8)
    out = OutT(score.data_ptr(), None, None)
    sc_c = sc.to_c()
    torch.cuda.synchronize()
    seed_kw = dict(band=args.band, cap=args.cap, window=W, stream=s)

    def seed1():
        ctx.seed_reads_device(index, d_R.data_ptr(), d_rl.data_ptr(), rs, n, mr, wpos.data_ptr(), votes.data_ptr(),
                              hits.data_ptr(), flags.data_ptr(), **seed_kw)

    def seed2():
        ctx.seed_reads_device(index, d_R.data_ptr(), d_rl.data_ptr(), rs, n, mr, wpos.data_ptr(), votes.data_ptr(),
                              hits.data_ptr(), flags.data_ptr(), rc_reads_ptr=rc.data_ptr(), rc_stride=ors, **seed_kw)

    def revcomp():
        ctx.revcomp_device(d_R.data_ptr(), d_rl.data_ptr(), rs, n, rc.data_ptr(), ors, s)

    def score_launch():
        check(lib().msw_align_reads_device(ctx.handle, ctypes.byref(sc_c), genome.handle, d_R.data_ptr(),
                                           d_rl.data_ptr(), rs, wpos.data_ptr(), n, W, mr, ctypes.byref(out), None,
                                           ctypes.c_void_p(s)))

    def strands_launch():
        ctx.align_reads_strands_device(genome, d_R.data_ptr(), d_rl.data_ptr(), rs, wpos.data_ptr(), n, W, mr,
                                       score.data_ptr(), strand.data_ptr(), oriented.data_ptr(), ors, sc, 0, 0, 0, s)

    wpos1, votes1, flags1 = z(n, torch.int64), z(n, torch.int32), z(n, torch.uint8)
    score1, strand1, oriented1 = z(n, torch.int32), z(n, torch.uint8), z(n * ors, torch.uint8)
    wlen, wlen1 = z(n, torch.int16), z(n, torch.int16)
    sub, mapq, cand = z(n, torch.int32), z(n, torch.uint8), z(n, torch.uint8)

    def cand_launch(both):
        ctx.seed_candidates_device(index, d_R.data_ptr(), d_rl.data_ptr(), rs, n, mr, wpos.data_ptr(), votes.data_ptr(),
                                   hits.data_ptr(), flags.data_ptr(), wpos1.data_ptr(), votes1.data_ptr(),
                                   flags1.data_ptr(), rc_reads_ptr=rc.data_ptr() if both else 0,
                                   rc_stride=ors if both else 0, sep=0, **seed_kw)

    def alt_strands_launch():
        ctx.align_reads_strands_device(genome, d_R.data_ptr(), d_rl.data_ptr(), rs, wpos1.data_ptr(), n, W, mr,
                                       score1.data_ptr(), strand1.data_ptr(), oriented1.data_ptr(), ors, sc, 0, 0,
                                       wlen1.data_ptr(), s)

    def select_launch():
        # in place: after a launch no alternate wins any more, so a repeated launch moves no rows
        ctx.mapq_select_device(dict(score=score.data_ptr(), win_len=wlen.data_ptr(), strand=strand.data_ptr(),
                                    oriented=oriented.data_ptr(), win_pos=wpos.data_ptr()),
                               dict(score=score1.data_ptr(), win_len=wlen1.data_ptr(), strand=strand1.data_ptr(),
                                    oriented=oriented1.data_ptr(), win_pos=wpos1.data_ptr()),
                               d_rl.data_ptr(), n, sc.match, sub.data_ptr(), mapq.data_ptr(), cand.data_ptr(),
                               oriented_stride=ors, stream=s)

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

    rec = {"row": "seed", "shape": "config 3 (150 x 300, affine)", "reads": n, "steps": args.steps,
           "warmup": args.warmup, "k": args.k, "max_occ": args.max_occ, "band": args.band, "cap": args.cap}
    rec["revcomp_ms"] = timed(revcomp)
    rec["seed1_ms"] = timed(seed1)
    rec["placed_forward_only"] = int((wpos.cpu() >= 0).sum())
    rec["seed2_ms"] = timed(seed2)
    rec["placed"] = int((wpos.cpu() >= 0).sum())
    rec["mean_hits"] = round(float(hits.cpu().double().mean()), 1)
    rec["reverse_hints"] = int((flags.cpu() & 1).sum())
    rec["truncated"] = int(((flags.cpu() >> 1) & 1).sum())
    rec["score_ms"] = timed(score_launch)          # against the windows seed2 chose
    rec["strands_ms"] = timed(strands_launch)
    rec["seed1_over_score"] = round(rec["seed1_ms"] / rec["score_ms"], 2)
    rec["seed2_over_strands"] = round(rec["seed2_ms"] / rec["strands_ms"], 2)
    rec["cand1_ms"] = timed(lambda: cand_launch(False))
    rec["cand2_ms"] = timed(lambda: cand_launch(True))
    rec["with_candidate_1"] = int((wpos1.cpu() >= 0).sum())
    rec["cand1_over_seed1"] = round(rec["cand1_ms"] / rec["seed1_ms"], 2)
    rec["cand2_over_seed2"] = round(rec["cand2_ms"] / rec["seed2_ms"], 2)
    strands_launch()
    alt_strands_launch()
    torch.cuda.synchronize()
    score0 = score.clone()                          # candidate 0's scores, before the select replaces the losers'
    select_launch()                                 # winners to move
    torch.cuda.synchronize()
    rec["alternate_wins"] = int(cand.cpu().sum())
    h = mapq.cpu().numpy()
    rec["mapq_hist"] = [int((h == 0).sum()), int(((h >= 1) & (h < 30)).sum()), int(((h >= 30) & (h < 60)).sum()),
                        int((h == 60).sum())]
    rec["select_ms"] = timed(select_launch)

    def restore():
        with torch.cuda.stream(st):
            score.copy_(score0)

    def restore_select():
        # candidate 0's scores put back: the same alternates win again and their rows are moved again
        restore()
        select_launch()

    rec["restore_ms"] = timed(restore)
    rec["restore_select_ms"] = timed(restore_select)
    rec["select_moving_ms"] = round(rec["restore_select_ms"] - rec["restore_ms"], 4)
    torch.cuda.synchronize()
    rec["alternate_wins_moving"] = int(cand.cpu().sum())
    for name, sym in (("cand_waves_per_cu", "_ZN3msw29seed_candidates_blocks_per_cuEj"),):
        fn = getattr(lib(), sym, None)
        if fn is not None:
            fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_uint32]
            rec[name] = int(fn(args.cap))
    get = getattr(lib(), "_ZN3msw18seed_blocks_per_cuEj", None)      # the library's occupancy query (C++ symbol)
    if get is not None:
        get.restype, get.argtypes = ctypes.c_int, [ctypes.c_uint32]
        rec["seed_waves_per_cu"] = int(get(args.cap))
    rec["seed_lds_bytes"] = 4 * (1 << (args.cap - 1).bit_length())
    print(json.dumps(rec), flush=True)
    index.close()
    genome.close()
    ctx.close()


if __name__ == "__main__":
    main()
