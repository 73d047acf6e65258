"""Hand-worked cases for tests/aln_oracle.py (the restatement the GPU
alignment records are compared with)."""
import aln_oracle as ao

LIN = (2, -1, 0, 2, False)
AFF = (2, -1, 3, 1, True)


def test_insertion_known_answer():
    # the 4M2I10M of test_traceback_oracle: the two inserted bases are the whole edit distance
    for scheme, score in ((LIN, 24), (AFF, 23)):
        r = ao.record(b"GGTTCACACACAGGTT", b"GGTTCACACAGGTT", 1000, *scheme)
        assert r == ao.Record(score, 15, 13, 1000, 2, [4 << 4, 2 << 4 | 1, 10 << 4])
        assert ao.cigar_text(r.ops) == "4M2I10M" and ao.read_bases(r.ops) == 16


def test_deletion_known_answer():
    for scheme, score in ((LIN, 20), (AFF, 19)):
        r = ao.record(b"GGTTCACAGGTT", b"GGTTCACACAGGTT", 7, *scheme)
        assert r == ao.Record(score, 11, 13, 7, 2, [4 << 4, 2 << 4 | 2, 8 << 4])
        assert ao.cigar_text(r.ops) == "4M2D8M" and ao.read_bases(r.ops) == 12


def test_leading_and_trailing_clip_with_a_mismatch():
    # read   GG ACGTAGGTACGT CC
    # window TT ACGTACGTACGT TT   12 columns, one mismatch: 11 * 2 - 1 = 21
    read, win = b"GGACGTAGGTACGTCC", b"TTACGTACGTACGTTT"
    for scheme in (LIN, AFF):
        r = ao.record(read, win, 500, *scheme)
        assert r == ao.Record(21, 13, 13, 502, 1, [2 << 4 | 4, 12 << 4, 2 << 4 | 4])
        assert ao.cigar_text(r.ops) == "2S12M2S" and ao.read_bases(r.ops) == len(read)


def test_one_sided_clips():
    # leading only: the alignment runs to the read's last base
    r = ao.record(b"GGGACGTACGT", b"ACGTACGT", 0, *LIN)
    assert (r.ref_pos, r.nm, ao.cigar_text(r.ops)) == (0, 0, "3S8M")
    # trailing only
    r = ao.record(b"ACGTACGTGGG", b"TACGTACGT", 10, *LIN)
    assert (r.ref_pos, r.nm, ao.cigar_text(r.ops)) == (11, 0, "8M3S")


def test_score_zero_and_empty():
    assert ao.record(b"AAAA", b"CCCCCC", 33, *LIN) == ao.Record(0, -1, -1, -1, 0, [])
    assert ao.record(b"", b"ACGT", 33, *AFF) == ao.Record(0, -1, -1, -1, 0, [])
    assert ao.record(b"ACGT", b"", 33, *LIN) == ao.Record(0, -1, -1, -1, 0, [])
    assert ao.cigar_text([]) == "*"


def test_window_rule():
    g = b"ACGTACGTAC"
    assert bytes(ao.window_of(g, 2, 4)) == b"GTAC"
    assert bytes(ao.window_of(g, 8, 4)) == b"AC"       # clipped at the genome end
    assert bytes(ao.window_of(g, 9, 4)) == b"C"
    assert len(ao.window_of(g, 10, 4)) == 0 and len(ao.window_of(g, -1, 4)) == 0
