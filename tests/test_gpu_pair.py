"""Pairs on the GPU (include/msw.h, "Pairs"): the three kernels and msw_map_pairs against tests/pair_oracle.py."""
import numpy as np
import pytest

import mapq_oracle as mo
import pair_oracle as po
import strand_oracle as so
from test_gpu_mapq import K as KMER, LIN, Dev, planted_genome
from test_gpu_seed import GUARD, Case, Guarded, pack, rand_seq

pytestmark = pytest.mark.gpu

KEYS = ("score", "end_i", "end_j", "win_len", "strand", "oriented", "win_pos")
Q = po.Params(100, 500, 17, 60, 8)


def candidates(n, K, stride, seed):
    """K candidates for 2n rows as the scoring calls leave them: few scores (ties), a quarter missing (win_pos
    -1, score 0), loci a few insert sizes apart (proper combinations) and some 2^33 away."""
    rng = np.random.default_rng(seed)
    rows = 2 * n
    lens = np.minimum(np.array([100, 150, 1, 17, 16, 0, 15], np.uint16)[np.arange(rows) % 7], stride).astype(np.uint16)
    home = np.repeat(rng.integers(0, 5000, n), 2)
    out = []
    for k in range(K):
        score = np.array([0, 50, 100, 100, 120, 300], np.int32)[rng.integers(0, 6, rows)]
        wp = home + np.array([0, 150, 300, 2900, 1 << 33])[rng.integers(0, 5, rows)]
        gone = (rng.random(rows) < 0.25) | (lens == 0)
        score[gone], wp[gone] = 0, -1
        ei = (rng.integers(0, 1 << 30, rows) % np.maximum(lens, 1)).astype(np.int16)
        ej = (ei + rng.integers(0, 60, rows)).astype(np.int16)
        ei[score == 0] = ej[score == 0] = -1
        o = rng.integers(1, 256, (rows, stride)).astype(np.uint8)
        o[np.arange(stride)[None, :] >= lens[:, None]] = 0
        out.append(dict(score=score, end_i=ei, end_j=ej, win_len=rng.integers(0, 769, rows).astype(np.uint16),
                        strand=rng.integers(0, 2, rows).astype(np.uint8), oriented=o, win_pos=wp.astype(np.int64)))
    return lens, out


as_cands = lambda C, r: [po.Cand(*(int(c[k][r]) for k in po.Cand._fields)) for c in C]
ptrs = lambda d: {k: v.ptr for k, v in d.items()}


@pytest.mark.parametrize("n", [1, 3, 64, 257])
@pytest.mark.parametrize("stride", [16, 400])
@pytest.mark.parametrize("K", [2, 3])
def test_select_and_plan(gpu_ctx, K, stride, n):
    import mini_parallel_amd as mpa
    import torch
    lens, C = candidates(n, K, stride, 1000 * K + stride + n)
    for bonus in (Q.pair_bonus, 0):
        q = Q._replace(pair_bonus=bonus)
        D = [{k: Dev(v) for k, v in c.items()} for c in C]
        d_rl, plan = Dev(lens), Guarded(2 * n, np.int64)
        sub, mq, cd = Guarded(2 * n, np.int32), Guarded(2 * n, np.uint8), Guarded(2 * n, np.uint8)
        fl, tl = Guarded(n, np.uint8), Guarded(n, np.int32)
        torch.cuda.synchronize()
        gpu_ctx.pair_plan_device([ptrs(d) for d in D], d_rl.ptr, n, mpa.PairParams(*q), plan.ptr)
        gpu_ctx.synchronize()
        want = [po.rescue_pos(as_cands(C, 2 * p), int(lens[2 * p]), as_cands(C, 2 * p + 1), int(lens[2 * p + 1]), q)
                for p in range(n)]
        assert plan.get().tolist() == [v for w in want for v in w]
        assert all(np.array_equal(D[k][key].get(), C[k][key]) for k in range(K) for key in KEYS)    # the plan only reads
        gpu_ctx.pair_select_device([ptrs(d) for d in D], d_rl.ptr, n, 2, mpa.PairParams(*q), sub.ptr, mq.ptr, cd.ptr,
                                   fl.ptr, tl.ptr, oriented_stride=stride)
        gpu_ctx.synchronize()
        ch = [po.choose(as_cands(C, 2 * p), int(lens[2 * p]), as_cands(C, 2 * p + 1), int(lens[2 * p + 1]), 2, q)
              for p in range(n)]
        per_row = lambda f: [v for c in ch for v in f(c)]
        cand = np.array(per_row(lambda c: c.cand), np.uint8)
        assert cd.get().tolist() == cand.tolist() and sub.get().tolist() == per_row(lambda c: c.sub_score)
        assert mq.get().tolist() == per_row(lambda c: c.mapq)
        assert fl.get().tolist() == [c.flags for c in ch] and tl.get().tolist() == [c.tlen for c in ch]
        for key in KEYS:          # the winner in candidate 0's arrays, padding included; everything else as it was
            w = C[0][key]
            for k in range(1, K):
                pick = cand == k
                w = np.where(pick[:, None] if key == "oriented" else pick, C[k][key], w)
            assert np.array_equal(D[0][key].get(), w), key
            assert all(np.array_equal(D[k][key].get(), C[k][key]) for k in range(1, K)), key
        if n >= 64:
            assert {0, 1, K - 1} <= set(cand.tolist()) and any(c.flags & 1 for c in ch) and any(po.NONE in c.c for c in ch)
        if bonus == 0 and K == 2:     # each mate's result is the single-end selection's, bit for bit
            S = [{k: Dev(v) for k, v in c.items()} for c in C]
            s1, m1, c1 = Guarded(2 * n, np.int32), Guarded(2 * n, np.uint8), Guarded(2 * n, np.uint8)
            gpu_ctx.mapq_select_device(ptrs(S[0]), ptrs(S[1]), d_rl.ptr, 2 * n, 2, s1.ptr, m1.ptr, c1.ptr,
                                       oriented_stride=stride)
            gpu_ctx.synchronize()
            assert all(np.array_equal(S[0][key].get(), D[0][key].get()) for key in KEYS)
            assert np.array_equal(s1.get(), sub.get()) and np.array_equal(m1.get(), mq.get())
            assert np.array_equal(c1.get(), cd.get())


@pytest.mark.parametrize("n,one_bin", [(0, False), (1, False), (5000, False), (5000, True)])
def test_insert_histogram(gpu_ctx, n, one_bin):
    import torch
    rng = np.random.default_rng(n + one_bin)
    tlen = np.array([0, 1, 4095, 4096, -7, 300, 301, 302, 1 << 20], np.int32)[rng.integers(0, 9, n)]
    if one_bin:
        tlen[:] = 333
    mapq = np.array([0, 19, 20, 60], np.uint8)[rng.integers(0, 4, 2 * n)]
    d_t, d_m, hist = Dev(tlen), Dev(mapq), Guarded(4096, np.int32)
    hist.t[GUARD:GUARD + 4096] = 0
    torch.cuda.synchronize()
    keep = [po.hist_adds(int(t), int(a), int(b), 20) for t, a, b in zip(tlen, mapq[0::2], mapq[1::2])]
    want = np.bincount(tlen[np.array(keep, bool)], minlength=4096) if n else np.zeros(4096, np.int64)
    for times in (1, 2):              # the call adds to what is there
        gpu_ctx.insert_hist_device(d_t.ptr if n else 0, d_m.ptr if n else 0, n, 20, hist.ptr)
        gpu_ctx.synchronize()
        assert np.array_equal(hist.get(), times * want)
    assert n < 5000 or want.sum() > 100 and (one_bin or np.count_nonzero(want) == 5)


def planted_pairs():
    """The planted genome of test_gpu_mapq.py; pairs named for the branch test_map_pairs asserts they take."""
    g, rng = planted_genome()
    sixth = lambda s: bytes(b if i % 6 else b ^ 6 for i, b in enumerate(s))     # A<->G, C<->E: no 8-mer survives
    pairs = {
        "repeat": (g[1210:1290], so.revcomp(g[1520:1600])),          # (a) E1 has copies at 500 and 1200
        "rescue": (g[2100:2180], so.revcomp(sixth(g[2350:2430]))),   # (b)
        "rescue_rev": (sixth(g[3210:3290]), so.revcomp(g[3400:3480])),      # the anchor on strand 1
        "same_strand": (g[2700:2780], g[2900:2980]),                 # (c)
        "over_start": (rand_seq(rng, 30) + g[:70], so.revcomp(g[200:280])),        # (d) left_u = -30
        "mate2_first": (so.revcomp(g[3700:3780]), g[3600:3680]),
        "unrelated": (rand_seq(rng, 80), rand_seq(rng, 80)),         # (e)
    }
    return g, [r for p in pairs.values() for r in p], list(pairs)


def test_map_pairs(gpu_ctx):
    import mini_parallel_amd as mpa
    g, reads, tags = planted_pairs()
    C = Case(gpu_ctx, g, KMER)
    q = po.Params(150, 600, 17, 60, 16)
    kw = dict(band=16, cap=4096, step=1, min_votes=4, window=0, sep=0)
    recs, flags, tlen = po.map_pairs(g, C.oix, reads, LIN, q, **kw)
    at = {t: p for p, t in enumerate(tags)}
    rec = lambda t, m: recs[2 * at[t] + m]
    # the cases take the branch they are named for
    single, _, _ = mo.map_records(g, C.oix, reads, LIN, True, **kw)
    assert (single[2 * at["repeat"]].cand, single[2 * at["repeat"]].ref_pos, single[2 * at["repeat"]].mapq) == (0, 510, 0)
    assert (rec("repeat", 0).cand, rec("repeat", 0).ref_pos, flags[at["repeat"]], tlen[at["repeat"]]) == (1, 1210, 1, 390)
    assert rec("repeat", 0).mapq > 0
    assert (rec("rescue", 1).cand, rec("rescue", 1).ref_pos, flags[at["rescue"]], tlen[at["rescue"]]) == (2, 2351, 5, 330)
    assert single[2 * at["rescue"] + 1].score == 0                   # no seed candidate
    assert (rec("rescue_rev", 0).cand, flags[at["rescue_rev"]], tlen[at["rescue_rev"]]) == (2, 3, 270)
    assert (flags[at["same_strand"]], tlen[at["same_strand"]], rec("same_strand", 1).score) == (0, 0, 160)
    assert (rec("over_start", 0).ref_pos, flags[at["over_start"]], tlen[at["over_start"]]) == (0, 1, 310)
    assert (flags[at["mate2_first"]], tlen[at["mate2_first"]]) == (1, 180)
    assert [rec("unrelated", m) for m in (0, 1)] == [mo.Mapped(0, -1, -1, 0, -1, 0, [], 0, 0, 0)] * 2
    R, rl = pack(reads, 112)
    R[np.arange(112)[None, :] >= rl[:, None]] = 0
    sc = mpa.Scoring(2, -1, 0, 2, False, True)
    for chunk in (3, 0):
        hist = np.zeros(4096, np.uint32)
        hist[7] = 5
        got = gpu_ctx.map_pairs(C.genome, C.index, R, rl, sc, mpa.PairParams(*q), chunk_pairs=chunk, hist=hist, **kw)
        s, ei, ej, strand, ref, nm, cigars, mq, sub, cand, fl, tl = got
        for p, r in enumerate(recs):
            have = (int(s[p]), int(ei[p]), int(ej[p]), int(strand[p]), int(ref[p]), int(nm[p]),
                    [int(o) for o in cigars[p]], int(mq[p]), int(sub[p]), int(cand[p]))
            assert have == tuple(r), (p, tags[p // 2])
        assert fl.tolist() == flags and tl.tolist() == tlen
        want = np.bincount([t for t in tlen if 0 < t < 4096], minlength=4096)
        want[7] += 5
        assert np.array_equal(hist, want)
    # the single-end call on the same rows leaves the repeat read at the lower copy with mapq 0
    one = gpu_ctx.map_reads(C.genome, C.index, R, rl, sc, mapq=True, **{k: v for k, v in kw.items()})
    p = 2 * at["repeat"]
    assert (int(one[4][p]), int(one[7][p]), int(one[9][p])) == (510, 0, 0) and int(ref[p]) == 1210 and int(mq[p]) > 0
    # rescue off and no bonus: every row is the single-end record
    off = gpu_ctx.map_pairs(C.genome, C.index, R, rl, sc, mpa.PairParams(1, 4095, 0, 0, 0), **kw)
    for a, b in zip(off[:10], one):
        assert all(np.array_equal(u, v) for u, v in zip(a, b)) if isinstance(a, list) else np.array_equal(a, b)
    # (f)
    for bad, code in ((dict(reads=R[:3], read_len=rl[:3]), -1), (dict(pair_params=mpa.PairParams(1, 4095, 0, 60, 0)), -2),
                      (dict(pair_params=mpa.PairParams(0, 500)), -2), (dict(pair_params=mpa.PairParams(9, 8)), -2)):
        with pytest.raises(mpa.MswError) as e:
            gpu_ctx.map_pairs(C.genome, C.index, **dict(dict(reads=R, read_len=rl, scoring=sc), **bad), **kw)
        assert e.value.code == code, bad
    C.close()
