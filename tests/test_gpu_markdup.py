"""Sorting and duplicates on the GPU (include/msw.h, "Sorting and duplicates"):
the radix sort against numpy's stable argsort, duplicate flags against a
dict-grouping restatement, coordinate order against np.lexsort, and mapped
copies of reads end to end.  Device arrays carry sentinels around them.
"""
import numpy as np
import pytest

import mini_parallel_amd as mpa
import strand_oracle as so
from mini_parallel_amd import SORT_TILE
from test_gpu_mapq import Dev, planted_genome
from test_gpu_seed import Case, Guarded, pack

pytestmark = pytest.mark.gpu

SCAN_TILE = 1024  # kAlnScanTile: 256 counters a tile cross it from the fifth tile on
N_BIG = min(300 * SORT_TILE + 5, (SCAN_TILE // 256) * SORT_TILE + 1)
M, I, D, S = 0, 1, 2, 4


def dev(*arrays):
    """The arrays on the device between sentinels, there before any library call (its streams do not wait for torch's)."""
    import torch
    out = [Dev(a) for a in arrays]
    torch.cuda.synchronize()
    return out


# ---------------------------------------------------------------------------
# 1. the sort
# ---------------------------------------------------------------------------
def sort_keys(kind, n, key_bits, rng):
    low = {"equal": np.full(n, 0x0123456789ABCDEF, np.uint64),
           "eight": rng.integers(0, 8, n).astype(np.uint64) * np.uint64(0x0101010101010101),
           "uniform": rng.integers(0, 1 << 64, n, dtype=np.uint64),
           "descending": np.arange(n, 0, -1).astype(np.uint64) * np.uint64(0x0000000100000081)}[kind]
    mask = np.uint64((1 << key_bits) - 1)
    return (low & mask) | (rng.integers(0, 1 << 64, n, dtype=np.uint64) & ~mask), mask


@pytest.mark.parametrize("kind", ["equal", "eight", "uniform", "descending"])
@pytest.mark.parametrize("key_bits", [1, 8, 9, 33, 64])
@pytest.mark.parametrize("n", [1, 63, 64, 65, SORT_TILE - 1, SORT_TILE, SORT_TILE + 1, 3 * SORT_TILE + 17, N_BIG])
def test_sort_pairs(gpu_ctx, n, key_bits, kind):
    rng = np.random.default_rng(n * 131 + key_bits)
    keys, mask = sort_keys(kind, n, key_bits, rng)
    vals = rng.integers(0, 1 << 32, n, dtype=np.uint32)
    dk, dv = dev(keys, vals)
    gpu_ctx.sort_pairs_device(dk.ptr, dv.ptr, n, key_bits)
    gpu_ctx.synchronize()
    idx = np.argsort(keys & mask, kind="stable")
    assert np.array_equal(dk.get(), keys[idx])      # the bits above key_bits travel with their key
    assert np.array_equal(dv.get(), vals[idx])


def test_sort_edges(gpu_ctx):
    rng = np.random.default_rng(7)
    keys = rng.integers(0, 1 << 64, 2 * SORT_TILE + 5, dtype=np.uint64)
    dk, = dev(keys)
    gpu_ctx.sort_pairs_device(dk.ptr, 0, keys.shape[0], 24)                       # keys only
    gpu_ctx.synchronize()
    assert np.array_equal(dk.get(), keys[np.argsort(keys & np.uint64(0xFFFFFF), kind="stable")])
    hk, hv = gpu_ctx.sort_pairs(keys, np.arange(keys.shape[0]), 64)               # the host form
    assert np.array_equal(hv, np.argsort(keys, kind="stable")) and np.array_equal(hk, np.sort(keys))
    gk, gv = Guarded(4, np.int64), Guarded(4, np.int32)
    gpu_ctx.sort_pairs_device(gk.ptr, gv.ptr, 0, 64)                              # n == 0 touches nothing
    gpu_ctx.synchronize()
    assert gk.untouched() and gv.untouched()
    for bits in (0, 65):
        with pytest.raises(mpa.MswError) as e:
            gpu_ctx.sort_pairs_device(gk.ptr, gv.ptr, 4, bits)
        assert e.value.code == -2                                                 # MSW_E_RANGE
    assert gk.untouched() and gv.untouched()


# ---------------------------------------------------------------------------
# 2. duplicates: the rule restated
# ---------------------------------------------------------------------------
def op(length, code):
    return length << 4 | code


FORMS = [[op(100, M)], [op(5, S), op(95, M)], [op(50, M), op(3, I), op(47, M)], [op(40, M), op(7, D), op(60, M)],
         [op(3, S), op(90, M), op(7, S)]]


def read_keys(ref_pos, nm, cigars, strand, score, ref_len):
    none = (ref_len + 65536) << 1
    keys = []
    for r in range(len(ref_pos)):
        if ref_pos[r] < 0 or score[r] <= 0 or nm[r] < 0:
            keys.append(none)
            continue
        ops = [(int(o) >> 4, int(o) & 15) for o in cigars[r]]
        lead = ops[0][0] if ops and ops[0][1] == S else 0
        trail = ops[-1][0] if len(ops) > 1 and ops[-1][1] == S else 0
        span = sum(length for length, code in ops if code in (M, D))
        u5 = int(ref_pos[r]) + span - 1 + trail if strand[r] else int(ref_pos[r]) - lead
        keys.append((u5 + 32768) << 1 | int(strand[r]))
    return keys, none


def mark(keys, none, score, pairs):
    """(order, dup per row, n_dup) of the header's rule, by grouping in a dict."""
    rows = [(2 * f, 2 * f + 1) for f in range(len(keys) // 2)] if pairs else [(f,) for f in range(len(keys))]
    frags = []
    for rs in rows:
        ks = sorted(keys[r] for r in rs) + [0]
        frags.append((ks[0], ks[1], sum(int(score[r]) for r in rs if keys[r] != none)))
    order = sorted(range(len(frags)), key=lambda f: frags[f][:2])
    groups = {}
    for f, (k1, k2, _) in enumerate(frags):
        if k1 != none:
            groups.setdefault((k1, k2), []).append(f)
    dup, n_dup = np.zeros(len(keys), np.uint8), 0
    for g in groups.values():
        best = max(g, key=lambda f: (frags[f][2], -f))
        for f in g:
            if f != best:
                n_dup += 1
                for r in rows[f]:
                    dup[r] = keys[r] != none
    return np.array(order, np.uint32), dup, n_dup, frags


def records(n, seed):
    """n reads over about n / 6 unclipped 5' sites (one of them negative), every CIGAR form on both strands."""
    rng = np.random.default_rng(seed)
    sites = np.concatenate([[-3], rng.integers(500, 4000, max(1, n // 6))])
    ref_pos, cigars = np.zeros(n, np.int64), []
    strand = rng.integers(0, 2, n).astype(np.uint8)
    score = rng.choice([90, 100], n).astype(np.int32)
    nm = rng.integers(0, 4, n).astype(np.int32)
    for r in range(n):
        u5, form = int(sites[rng.integers(0, len(sites))]), FORMS[rng.integers(0, len(FORMS))]
        if u5 < 0:
            strand[r], form = 0, FORMS[4]                       # ref_pos 0 behind a leading clip of 3
        lead = form[0] >> 4 if form[0] & 15 == S else 0
        trail = form[-1] >> 4 if len(form) > 1 and form[-1] & 15 == S else 0
        span = sum(o >> 4 for o in form if o & 15 in (M, D))
        ref_pos[r] = u5 - trail - span + 1 if strand[r] else u5 + lead
        cigars.append(np.array(form, np.uint32))
    for r in range(5, n, 11):                                   # the three unkeyed kinds in turn
        kind = (r // 11) % 3
        if kind == 0:
            ref_pos[r] = -1
        elif kind == 1:
            score[r] = 0
        else:
            nm[r], cigars[r] = -1, np.zeros(0, np.uint32)
    return ref_pos, nm, cigars, strand, score


REF_LEN = 4096


@pytest.mark.parametrize("n", [1, 65, 2 * SORT_TILE + 3])
def test_flags_single_end(gpu_ctx, n):
    ref_pos, nm, cigars, strand, score = records(n, n)
    keys, none = read_keys(ref_pos, nm, cigars, strand, score, REF_LEN)
    want_order, want_dup, want_n, frags = mark(keys, none, score, False)
    if n >= 65:
        clipped = np.array([len(c) > 0 and c[0] & 15 == S for c in cigars])
        by_key = {}
        for r, k in enumerate(keys):
            by_key.setdefault(k, []).append(r)
        mixed = {k & 1 for k, rs in by_key.items() if k != none and 0 < clipped[rs].sum() < len(rs)}
        assert mixed == {0, 1}                                  # clipped and unclipped reads share a u5, per strand
        assert any(k ^ 1 in by_key for k in by_key if k != none)     # both strands at one u5: two groups
        assert min(keys) < 32768 << 1                           # a negative u5
        assert any(k != none and any(o & 15 == I for o in cigars[r]) for r, k in enumerate(keys))
        assert any(k != none and any(o & 15 == D for o in cigars[r]) for r, k in enumerate(keys))
        assert (ref_pos < 0).any() and (score <= 0).any() and (nm < 0).any() and keys.count(none) >= 3
        assert any(sorted(score[rs])[-1] == sorted(score[rs])[-2] for k, rs in by_key.items() if k != none and len(rs) > 1)
        assert 1 < max(len(rs) for k, rs in by_key.items() if k != none) and 0 < want_n < n
    off = np.zeros(n + 1, np.uint32)
    off[1:] = np.cumsum([len(c) for c in cigars])
    cig = np.concatenate(cigars + [np.zeros(1, np.uint32)])
    d = dev(ref_pos, nm, off, cig, strand, score)
    order, dup, cnt = Guarded(n, np.int32), Guarded(n, np.uint8), Guarded(1, np.int64)
    gpu_ctx.mark_duplicates_device(d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, int(off[n]), d[4].ptr, d[5].ptr, n, REF_LEN,
                                   order.ptr, dup.ptr, cnt.ptr)
    gpu_ctx.synchronize()
    assert np.array_equal(order.get(np.uint32), want_order)
    assert np.array_equal(dup.get(), want_dup) and int(cnt.get()[0]) == want_n
    h_dup, h_order, h_n = gpu_ctx.mark_duplicates(ref_pos, nm, cigars, strand, score, REF_LEN)   # the host form
    assert np.array_equal(h_order, want_order) and np.array_equal(h_dup, want_dup) and h_n == want_n


@pytest.mark.parametrize("pairs", [6, 65, SORT_TILE + 3])
def test_flags_pairs(gpu_ctx, pairs):
    ref_pos, nm, cigars, strand, score = records(2 * pairs, pairs)

    def put(row, pos, s, sc=100):
        ref_pos[row], strand[row], score[row], nm[row], cigars[row] = pos, s, sc, 0, np.array(FORMS[0], np.uint32)

    # pairs 0 and 1: the same mates swapped; 2: mate a of pair 0 and an unkeyed mate; 3: none keyed;
    # 4: as pair 0 with a lower score; 5: as pair 2 (a one-keyed pair meets only its like)
    for p, (a, b) in enumerate([((700, 0), (901, 1)), ((901, 1), (700, 0)), ((700, 0), None), (None, None),
                                ((700, 0), (901, 1)), (None, (700, 0))]):
        for row, mate in ((2 * p, a), (2 * p + 1, b)):
            put(row, *(mate if mate else (-1, 0)), sc=90 if p == 4 else 100)
    keys, none = read_keys(ref_pos, nm, cigars, strand, score, REF_LEN)
    want_order, want_dup, want_n, frags = mark(keys, none, score, True)
    assert want_dup[:12].tolist() == [0, 0, 1, 1, 0, 0, 0, 0, 1, 1, 0, 1]
    assert frags[2][1] == none and frags[3][0] == none and frags[2][0] == frags[0][0]
    dup, order, n_dup = gpu_ctx.mark_duplicates(ref_pos, nm, cigars, strand, score, REF_LEN, pairs=True)
    assert np.array_equal(order, want_order) and np.array_equal(dup, want_dup) and n_dup == want_n
    with pytest.raises(mpa.MswError) as e:
        gpu_ctx.mark_duplicates(ref_pos[:-1], nm[:-1], cigars[:-1], strand[:-1], score[:-1], REF_LEN, pairs=True)
    assert e.value.code == -1                                   # MSW_E_INVALID


# ---------------------------------------------------------------------------
# 3. coordinate order
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 2 * SORT_TILE + 3])
def test_coordinate_order(gpu_ctx, n):
    rng = np.random.default_rng(n)
    ref_pos = rng.integers(-1, n // 4, n).astype(np.int64)
    strand = rng.integers(0, 2, n).astype(np.uint8)
    # stable; the last key is the primary one; the unplaced reads share one key, whatever their strand byte
    want = np.lexsort((np.where(ref_pos < 0, 0, strand), ref_pos, ref_pos < 0))
    assert (ref_pos < 0).any() and np.unique(ref_pos).shape[0] < n
    assert np.array_equal(gpu_ctx.coordinate_order(ref_pos, strand), want)
    assert np.array_equal(gpu_ctx.coordinate_order(ref_pos, strand, ref_len=n // 4), want)
    assert np.array_equal(gpu_ctx.coordinate_order(ref_pos), np.lexsort((ref_pos, ref_pos < 0)))
    (d_pos, d_strand), order = dev(ref_pos, strand), Guarded(n, np.int32)
    gpu_ctx.coordinate_order_device(d_pos.ptr, d_strand.ptr, n, order.ptr, ref_len=n // 4)
    gpu_ctx.synchronize()
    assert np.array_equal(order.get(np.uint32), want)


# ---------------------------------------------------------------------------
# 4. end to end: mapped copies
# ---------------------------------------------------------------------------
def test_mapped_copies(gpu_ctx):
    """48 reads of 80 bases at distinct places of the planted genome's unique stretch, every third one reverse
    complemented; the first four get two copies each and the next eight one, and one copy per group carries a
    mismatch in the middle (a lower score, the same coordinates).  The worse copy comes FIRST in its group."""
    g, rng = planted_genome()
    base = [g[2100 + 6 * i:2180 + 6 * i] for i in range(48)]
    reads, dups = [], []
    for i, r in enumerate(base):
        group = [r] * (3 if i < 4 else 2 if i < 12 else 1)
        if len(group) > 1:
            bad = bytearray(r)
            bad[40] = ord("A") if bad[40] != ord("A") else ord("C")
            group[0] = bytes(bad)
            dups += [len(reads)] + list(range(len(reads) + 2, len(reads) + len(group)))   # all but the first exact copy
        reads += [so.revcomp(x) if i % 3 == 0 else x for x in group]
    assert len(reads) == 64 and len(dups) == 16
    C = Case(gpu_ctx, g, 8)
    R, rl = pack(reads, 80)
    score, _, _, strand, ref_pos, nm, cigars = gpu_ctx.map_reads(C.genome, C.index, R, rl)
    dup, order, n_dup = gpu_ctx.mark_duplicates(ref_pos, nm, cigars, strand, score, len(g))
    assert np.flatnonzero(dup).tolist() == dups and n_dup == 16 and strand.any() and not strand.all()
    keep = dup == 0
    masked, kept = gpu_ctx.pileup(C.genome), gpu_ctx.pileup(C.genome)
    masked.add(R, rl, ref_pos, nm, cigars, strand=strand, mapq=255 * (1 - dup), min_mapq=1)
    kept.add(R[keep], rl[keep], ref_pos[keep], nm[keep], [c for c, k in zip(cigars, keep) if k], strand=strand[keep])
    masked.finish()
    kept.finish()
    assert np.array_equal(masked.counts(), kept.counts()) and masked.counts()[:, :4].sum() == 48 * 80
    C.close()
