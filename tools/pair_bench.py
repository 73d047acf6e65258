#!/usr/bin/env python3
"""Paired-end mapping against the single-end call on the same rows.

64k pairs of 150 bp (insert sizes about 400 +- 40, 1 % substitutions, mate 2
reverse-complemented) on a synthetic 4 Mbase genome; three calls alternated in
one process: Context.map_pairs with rescue off, with rescue on, and
Context.map_reads(mapq=True) over the same 2n rows.  One warm-up round, then
--repeats rounds; prints one JSON line per call with every round's seconds and
the range in pairs per second.  --only runs one of the calls once (for a
kernel trace of its own).

    python tools/pair_bench.py [--pairs 65536] [--repeats 5] [--only pairs_rescue]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mini_parallel_amd as mpa  # noqa: E402

ACGT = np.frombuffer(b"ACGT", np.uint8)
COMP = np.arange(256, dtype=np.uint8)
COMP[ACGT] = ACGT[::-1]


def make_pairs(genome, n, read_len, rng):
    ins = np.clip(rng.normal(400, 40, n).astype(np.int64), read_len, 1000)
    left = rng.integers(0, genome.shape[0] - 1000, n)
    cols = np.arange(read_len)
    rows = np.empty((2 * n, read_len + 10), np.uint8)
    rows[:, read_len:] = 0
    rows[0::2, :read_len] = genome[left[:, None] + cols]
    rows[1::2, :read_len] = COMP[genome[(left + ins)[:, None] - 1 - cols]]
    hit = rng.random((2 * n, read_len)) < 0.01
    rows[:, :read_len][hit] = ACGT[rng.integers(0, 4, int(hit.sum()))]
    return rows, np.full(2 * n, read_len, np.uint16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=65536)
    ap.add_argument("--genome", type=int, default=4 << 20)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", choices=("reads", "pairs", "pairs_rescue"))
    a = ap.parse_args()
    rng = np.random.default_rng(2)
    g = ACGT[rng.integers(0, 4, a.genome)]
    rows, rl = make_pairs(g, a.pairs, a.read_len, rng)
    ctx = mpa.Context(0)
    genome = ctx.load_genome(g)
    index = ctx.build_index(genome, 12, 64)
    sc = mpa.Scoring(2, -1, 3, 1, True, True)
    on, off = mpa.PairParams(200, 600, 17, 60, 16), mpa.PairParams(200, 600, 17, 0, 0)
    calls = {"reads": lambda: ctx.map_reads(genome, index, rows, rl, sc, mapq=True),
             "pairs": lambda: ctx.map_pairs(genome, index, rows, rl, sc, off),
             "pairs_rescue": lambda: ctx.map_pairs(genome, index, rows, rl, sc, on)}
    if a.only:
        calls = {a.only: calls[a.only]}
    secs, last = {k: [] for k in calls}, {}
    for rnd in range((0 if a.only else 1) + (1 if a.only else a.repeats)):
        for name, fn in calls.items():
            t0 = time.perf_counter()
            last[name] = fn()
            if rnd or a.only:
                secs[name].append(time.perf_counter() - t0)
    for name, s in secs.items():
        out = dict(call=name, pairs=a.pairs, read_len=a.read_len, genome=a.genome, seconds=[round(x, 4) for x in s],
                   pairs_per_s=[round(a.pairs / max(s)), round(a.pairs / min(s))],
                   mapq_ge_20=int((last[name][7] >= 20).sum()))
        if name != "reads":
            out.update(proper=int((last[name][10] & 1).sum()), rescued=int((last[name][10] & 6 != 0).sum()))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
