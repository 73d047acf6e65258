"""The case generators of tests/range_cases.py against the oracle alone (CPU),
so the GPU tests built on them cannot pass on inputs that miss their target:
planted copies reach match x L, the f16-edge batches top out in the last f16
binade on the bound's two sides, the ceiling batches reach 64 m, and the three
restatements of the recurrence (scalar C, SIMD C, numpy) agree on them."""
import numpy as np
import pytest

import range_cases as rc
from oracle.sw_oracle_np import sw_batch_np


def kw(sc):
    return dict(match=sc.match, mismatch=sc.mismatch, gap_open=sc.gap_open, gap_extend=sc.gap_extend, affine=sc.affine)


def wide_batches():
    out = [rc.kr_batch(kr) for kr in rc.WIDE_KRS]
    out += list(rc.fallback_batches()) + list(rc.round_batches()) + [rc.bucket_edge_batch()]
    out += [rc.narrow_batch(m) for m in (221, 260, 312)]
    return out


def f16_cases():
    """(batch, match, mismatch, fits) of every B1 batch."""
    out = []
    for match, mis, length in rc.F16_EDGES:
        out.append((rc.f16_edge_batch(match, length), match, mis, True))
        out.append((rc.f16_edge_batch(match, length + 1), match, mis, False))
    match, mis, length = rc.F16_ALWAYS
    out.append((rc.f16_edge_batch(match, length), match, mis, True))
    out.append((rc.mirrored_batch(253), 8, -4, True))
    out.append((rc.mirrored_batch(254), 8, -4, False))
    return out


def test_f16_edge_table():
    """Each (match, L) sits on the bound: match (L + 2) < 2048 <= match (L + 3),
    the top score match L lies in the binade [1024, 2048), and match and
    mismatch are f16 values with a zero low byte (at most three significant
    bits) within match - mismatch <= 64."""
    for match, mis, length in rc.F16_EDGES:
        assert match * (length + 2) < 2048 <= match * (length + 3), (match, length)
        assert 1024 <= match * length < 2048
    match, mis, length = rc.F16_ALWAYS
    assert length == 384 and match * (length + 2) < 2048 and 1024 <= match * length < 2048
    for match, mis, _ in rc.F16_EDGES + [rc.F16_ALWAYS]:
        for v in (match, -mis):
            assert v == 0 or v >> max(v.bit_length() - 3, 0) << max(v.bit_length() - 3, 0) == v, v
        assert mis <= 0 and match - mis <= 64


@pytest.mark.parametrize("gaps", [(0, 2, False), (3, 1, True), (30000, 1024, True)],
                         ids=["lin2", "aff3+1", "aff30000+1024"])
def test_f16_batches_reach_their_top(oracle, gaps):
    """Exact copies score match x min(m, n) under linear 2, affine 3/1 and
    affine 30000/1024; the copies with one substitution or one deletion score
    less, so no two neighbouring pairs of a batch hold the same values."""
    go, ge, affine = gaps
    for b, match, mis, fits in f16_cases():
        s, i, j = oracle.sw_batch(b.reads, b.read_len, b.wins, b.win_len, match=match, mismatch=mis, gap_open=go,
                                  gap_extend=ge, affine=affine, threads=4)
        top = match * np.minimum(b.read_len, b.win_len).astype(np.int32)
        assert b.exact.any() and (~b.exact).any(), b.key
        assert np.array_equal(s[b.exact], top[b.exact]), (b.key, match)
        assert (s[~b.exact] < top[~b.exact]).all() and (s[~b.exact] > 0).all(), (b.key, s)
        length = int(min(b.read_len.max(), b.win_len.max()))
        assert (match * (length + 2) < 2048) == fits
        if fits:
            assert 1024 <= int(s.max()) < 2048, (b.key, match, int(s.max()))
        else:
            assert match * (length + 2) >= 2048 and int(s.max()) >= 1024


def test_top_gap_schemes_keep_the_gap_positive():
    for match, mis, length in rc.F16_EDGES + [rc.F16_ALWAYS]:
        for sc in rc.top_gap_schemes(match, mis, length).values():
            assert sc.affine and sc.gap_open <= 30000 and sc.gap_extend <= 1024
        s = list(rc.top_gap_schemes(match, mis, length).values())
        assert match * length - (s[0].gap_open + s[0].gap_extend) == 10
        assert s[1].gap_open + s[1].gap_extend == 2047 and s[2].gap_open + s[2].gap_extend == 2048


def test_ceiling_batches_reach_64m(oracle):
    """Identical 256 and 384 bp pairs score 64 m (24576 at 384) under every
    64/0 scheme; the largest value a register then holds is
    64 (384 + 1) + 1280 = 25920 < 0x7C00; neighbouring pairs differ."""
    assert 64 * (384 + 1) + 256 + 1024 == 25920 < 0x7C00
    for m in (256, 384):
        b = rc.ceiling_batch(m)
        assert all(b.kinds[i] != b.kinds[i + 1] for i in range(8)) and all(b.kinds[i] != b.kinds[i + 4] for i in range(5))
        for name, sc in rc.ceiling_schemes().items():
            s = rc.want(oracle, b, sc)[0]
            if sc.match == 64:
                assert (s[b.exact] == 64 * m).all() and s.max() == 64 * m, (name, s)
                # mismatch 0: one substitution costs exactly one match; a free gap
                # (gap_extend 0) hides the deletion, any other gap shows it
                sub = np.array([k == "sub" for k in b.kinds])
                assert (s[sub] == 64 * (m - 1)).all() and (s <= 64 * m).all(), (name, s)
            else:
                assert (s[b.exact] == sc.match * m).all() and len(set(s.tolist())) > 1, (name, s)


def test_wide_batches_hold_what_they_claim(oracle):
    """The wide generators: read lengths on the edges of every KR 17..24,
    windows on the staging rounds' edges, pure A/C/G/T except the bytes put
    there on purpose, and long alignments in every pair that has room."""
    for kr in rc.WIDE_KRS:
        b = rc.kr_batch(kr)
        assert sorted(set(b.read_len.tolist())) == [16 * (kr - 1) + 1, 16 * kr - 1, 16 * kr]
        assert np.array_equal(b.win_len, 2 * b.read_len) and np.isin(b.wins, rc.ACGT).all()
        s = rc.want(oracle, b, rc.FOUR["linear"])[0]
        assert (s >= 2 * b.read_len.astype(np.int32) - 40).all() and (s[b.exact] == 2 * b.read_len[b.exact]).all()
    clean, inside, padded = rc.fallback_batches()
    bad = ~np.isin(inside.wins, rc.ACGT)
    assert sorted(zip(*np.nonzero(bad))) == [(11, 599), (16, 0)]
    assert np.isin(padded.wins[:, :600], rc.ACGT).all() and not np.isin(padded.wins[:, 600:], rc.ACGT).any()
    assert np.array_equal(padded.wins[:, :600], clean.wins[:, :600])
    mixed, full768, full4096 = rc.round_batches()
    assert set(mixed.win_len.tolist()) == set(rc.ROUND_WIN_LENS)
    for w in rc.ROUND_WIN_LENS:  # every window length under both read lengths
        assert set(mixed.read_len[mixed.win_len == w].tolist()) == {300, 384}
    assert (full768.win_len == full768.wins.shape[1]).all() and (full4096.win_len == full4096.wins.shape[1]).all()
    assert mixed.reads.shape[1] == 384 and mixed.wins.shape[1] == 4096
    for b in (full768, full4096):  # every best cell lies in the row's last 16-byte chunk
        s, _, j = rc.want(oracle, b, rc.FOUR["linear"])
        assert (j >= b.wins.shape[1] - 16).all() and (s >= 2 * b.read_len.astype(np.int32) - 40).all(), (b.key, j)
    e = rc.bucket_edge_batch()
    assert e.read_len.min() == 241 and e.read_len.max() == 384
    counts = np.bincount(-(-e.read_len.astype(int) // 16), minlength=25)
    assert (counts[16:25] == 9).all()
    # every wide bucket's longest read is 16 KR, so under match 6 (7) the f16
    # bound match (16 KR + 2) < 2048 holds up to KR 21 (18) and fails above:
    # the wide buckets of one launch differ in f16_ok
    for match, last in ((6, 21), (7, 18)):
        fits = [match * (int(e.read_len[-(-e.read_len.astype(int) // 16) == kr].max()) + 2) < 2048 for kr in rc.WIDE_KRS]
        assert fits == [kr <= last for kr in rc.WIDE_KRS]
    assert e.read_len[-1] > 256  # a chunked call's last launch is a wide one
    for m, kr in ((221, 17), (260, 20), (312, 24)):
        b = rc.narrow_batch(m)
        assert b.read_len.max() == m and {-(-int(x) // 13) for x in b.read_len} == {kr}


def test_restatements_agree(oracle):
    """oracle.sw_batch and sw_batch_simd on every batch of A and B under the
    schemes the GPU tests use; the numpy restatement on a subsample of the
    longest ones (it is scalar over the cells)."""
    cases = [(b, sc) for b in wide_batches() for sc in (rc.FOUR["linear"], rc.FOUR["affine"])]
    cases += [(b, sc) for b in wide_batches()[:8] for sc in rc.with_scheme(rc.THREE, match=9, mismatch=-9).values()]
    for b, match, mis, _ in f16_cases():
        cases += [(b, sc) for sc in rc.with_scheme(rc.FOUR, match=match, mismatch=mis).values()]
        cases += [(b, sc) for sc in rc.top_gap_schemes(match, mis, int(b.read_len.max())).values()]
    for m in (256, 384):
        cases += [(rc.ceiling_batch(m), sc) for sc in rc.ceiling_schemes().values()]
    for b, sc in cases:
        a = rc.want(oracle, b, sc)
        s, i, j, _ = oracle.sw_batch_simd(b.reads, b.read_len, b.wins, b.win_len, threads=4, **kw(sc))
        assert np.array_equal(a[0], s) and np.array_equal(a[1], i) and np.array_equal(a[2], j), (b.key, sc)
    # numpy (vectorised over the pairs, scalar over the cells: seconds per
    # 100k cells): the 256-base ceiling batch under the largest penalties and
    # two f16-edge batches
    sub = [(rc.ceiling_batch(256), rc.ceiling_schemes()["64/0 affine 30000+1024"]),
           (rc.f16_edge_batch(32, 61), rc.with_scheme(rc.FOUR, match=32, mismatch=-4)["linear"]),
           (rc.f16_edge_batch(64, 29), rc.top_gap_schemes(64, 0, 29)["affine top-40+30"])]
    for b, sc in sub:
        a = rc.want(oracle, b, sc)
        n = sw_batch_np(b.reads, b.read_len, b.wins, b.win_len, **kw(sc))
        for x, y in zip(a, n):
            assert np.array_equal(x.astype(np.int32), y), (b.key, sc)
