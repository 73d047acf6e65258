"""The inputs of tests/test_gpu_trace_long_paths.py (tests/trace_long_inputs.py) do what that module needs
them to do, shown without a GPU from the full-matrix restatement (tests/traceback_oracle.py) alone: op counts
on either side of 4,096, end columns, gaps over rows 383 / 384, walks through every strip.
"""
import pytest

import traceback_oracle as tbo
import trace_long_inputs as ti
from test_gpu_trace_long import expected

S = ti.SCHEMES


def ops_of(x):
    return [(o >> 4, o & 15) for o in x[3]]


def gap_rows(x, op):
    """[(first read row, length)] of the I ops; for D ops the row they are walked in."""
    out, i = [], x[2][0]
    for n, c in ops_of(x):
        if c == op:
            out.append((i if c == tbo.I else i - 1, n))
        if c != tbo.D:
            i += n
    return out


@pytest.mark.parametrize("scheme", ti.OPS_SCHEMES)
def test_op_counts_around_lds_bound(scheme):
    """2 m - 1 ops of 1M 1D from (0, 0); 4,199 need the scratch layout, 4,095 fit either."""
    for m in (2100, 2048):
        r, w = ti.interleaved(m)
        x = expected(r, w, S[scheme])
        assert x[1:3] == ((m - 1, 2 * m - 2), (0, 0))
        assert ops_of(x) == [(1, tbo.M), (1, tbo.D)] * (m - 1) + [(1, tbo.M)]
        assert len(r) + len(w) > ti.LDS_OPS                       # max_rows + max_cols caps the op bound
    assert 2 * 2100 - 1 > 4100 > ti.LDS_OPS > 2 * 2048 - 1        # strides 4,224 / 4,100 / 4,097 are scratch layouts
    batch = ti.reuse_batch()
    assert [len(r) for r, _ in batch][2] == 0 and expected(*batch[4], S[scheme])[0] == 0
    assert 2 < len(expected(*batch[1], S[scheme])[3]) < ti.LDS_OPS and batch[1][0].shape[0] > ti.STRIP


@pytest.mark.parametrize("scheme", ["lin", "aff"])
@pytest.mark.parametrize("m,n,rpl", ti.ROWS_PER_LANE)
def test_rows_per_lane_inputs(m, n, rpl, scheme):
    pairs = ti.rows_per_lane_pairs(m, n)
    assert ti.rows_per_lane(pairs) == rpl and n > 4096 and m <= ti.STRIP
    assert [len(r) for r, _ in pairs] == [m, m, m, 0] and all(len(w) == n for _, w in pairs)
    last, first = expected(*pairs[0], S[scheme]), expected(*pairs[1], S[scheme])
    assert last[1][1] >= n - 3 and last[1][0] == m - 1
    assert 0 <= first[1][1] < 64 and first[0] > 0


def test_genome_reads_rows_per_lane():
    for m, rpl in ((100, 2), (150, 3)):
        g, reads = ti.genome_reads(m)
        assert ti.rows_per_lane([(r, g) for r in reads]) == rpl and max(ti.GENOME_WANT) > 4096


@pytest.mark.parametrize("scheme", ["lin", "aff"])
def test_narrow_end_columns(scheme):
    """end_j + 1 is the listed width, the best cell lies in the last row, and that row is past the first strip."""
    cases = ti.narrow_pairs() + [c for n in (1, 40, 64) for c in ti.narrow_pairs((769,), n)]
    assert sorted({e for e, _ in ti.narrow_pairs()}) == list(ti.NARROW_COLS)
    assert [len(ti.narrow_pairs((769,), n)) for n in (1, 40, 64)] == [1, 5, 7]
    for e, (r, w) in cases:
        x = expected(r, w, S[scheme])
        assert x[1] == (len(r) - 1, e - 1) and x[2] == (len(r) - e, 0) and len(r) > ti.STRIP, (len(r), e)


def test_narrow_crossing_walks_every_strip():
    for e, (r, w) in ti.narrow_crossing_pairs():
        x = expected(r, w, S["lin_gap0"])
        assert x[1] == (len(r) - 1, e - 1) and x[2] == (0, 0), (len(r), e)
        assert x[2][0] < ti.STRIP <= x[1][0] and len(x[3]) == 2 * e - 1


@pytest.mark.parametrize("scheme", ti.TIE_SCHEMES)
def test_gap_run_rows(scheme):
    """The 8-base gap of the A run lies at the run's left end: an insertion over rows 380..387 (across the
    boundary) and 384..391 (it opens in the strip's first row); a deletion walked in row 383 and in row 384."""
    for op, row, (r, w) in ti.gap_run_pairs():
        x = expected(r, w, S[scheme])
        if op == "I":
            assert gap_rows(x, tbo.I) == [(row, 8)] and not gap_rows(x, tbo.D), (row, tbo.cigar_text(x[3]))
            assert row <= ti.STRIP <= row + 7
        else:
            assert gap_rows(x, tbo.D) == [(row - 1, 8)] and not gap_rows(x, tbo.I), (row, tbo.cigar_text(x[3]))
            assert row - 1 in (ti.STRIP - 1, ti.STRIP)
        assert x[2][0] == 0 and x[1][0] == len(r) - 1


@pytest.mark.parametrize("scheme", ti.TIE_SCHEMES)
def test_tie_inputs_cross_the_boundary(scheme):
    for r, w in ti.homopolymers() + ti.dinucleotide_slips() + ti.read_twice() + ti.low_entropy_pairs():
        x = expected(r, w, S[scheme])
        assert x[2][0] < ti.STRIP <= x[1][0]
    for k, c in ((0, "D"), (1, "I")):
        x = expected(*ti.dinucleotide_slips()[k], S[scheme])
        assert tbo.cigar_text(x[3]) == f"382M1{c}599M1{c}219M"
    x = expected(*ti.read_twice()[0], S[scheme])
    assert x[1] == (799, 799) and x[2] == (0, 0)            # the first of the two equal copies


def test_bounds_inputs():
    r, w = ti.wide_pair(385)
    x = expected(r, w, S["lin"])
    assert len(w) == ti.LIMIT and x[1] == (384, ti.LIMIT - 1) and x[2][0] == 0       # two strips, the last column
    r, w = ti.wide_pair(40)
    x = expected(r, w, S["lin"])
    assert ti.rows_per_lane([(r, w)]) == 1 and x[1] == (39, ti.LIMIT - 1)
    r, w = ti.tall_pair()
    x = expected(r, w, S["lin_gap0"])
    assert len(r) == ti.LIMIT and (ti.LIMIT + ti.STRIP - 1) // ti.STRIP == 86
    assert x[2][0] == 0 and x[1] == (ti.LIMIT - 1, 299) and len(x[3]) == 599 < ti.LDS_OPS  # all 86 strips walked
