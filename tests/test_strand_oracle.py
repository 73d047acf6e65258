"""tests/strand_oracle.py and mini_parallel_amd.reverse_complement on hand-worked
cases (CPU only): the complement table, short lengths, ties, a reverse read
and a reverse read with an insertion."""
import numpy as np
import pytest

import aln_oracle as ao
import strand_oracle as so

LIN = (2, -1, 0, 2, False)
AFF = (2, -1, 3, 1, True)
X = b"GATTACAGGCTTACCGATAGCATCCGTA"      # no reverse-complement self-similarity worth a score near its own


def test_only_eight_byte_values_change():
    every = bytes(range(256))
    rc = so.revcomp(every)
    comp = rc[::-1]
    changed = {b for b in range(256) if comp[b] != b}
    assert changed == set(b"ACGTacgt")
    assert [chr(comp[b]) for b in b"ACGTacgtNn"] == list("TGCAtgcaNn")
    assert so.revcomp(rc) == every


def test_package_function_agrees_with_the_table():
    from mini_parallel_amd import reverse_complement
    every = bytes(range(256))
    assert reverse_complement(every) == so.revcomp(every)
    assert reverse_complement("AACGtn") == "naCGTT"
    a = np.frombuffer(b"ACCGT", np.uint8)
    out = reverse_complement(a)
    assert out.dtype == np.uint8 and out.tobytes() == b"ACGGT"
    assert reverse_complement(b"") == b"" and reverse_complement("") == ""
    with pytest.raises(TypeError):
        reverse_complement(np.zeros(3, np.int32))


def test_lengths_0_1_2():
    assert so.revcomp(b"") == b""
    assert so.revcomp(b"A") == b"T" and so.revcomp(b"N") == b"N"
    assert so.revcomp(b"AC") == b"GT" and so.revcomp(b"aN") == b"Nt"


@pytest.mark.parametrize("scheme", [LIN, AFF])
def test_palindrome_is_a_tie_for_the_forward_strand(scheme):
    assert so.revcomp(b"ACGT") == b"ACGT"
    r = so.record(b"ACGT", b"TTACGTTT", 100, scheme)
    assert (r.score, r.strand, r.ref_pos, ao.cigar_text(r.ops)) == (8, 0, 102, "4M")


@pytest.mark.parametrize("scheme", [LIN, AFF])
def test_both_orientations_in_the_window_tie_forward_first_half(scheme):
    win = X + so.revcomp(X)
    r = so.record(X, win, 0, scheme)
    assert (r.score, r.strand, r.end_i, r.end_j) == (2 * len(X), 0, len(X) - 1, len(X) - 1)
    # the reverse complement scores the same, in the second half: a tie
    assert ao.record(so.revcomp(X), win, 0, *scheme)[:3] == (2 * len(X), len(X) - 1, 2 * len(X) - 1)


@pytest.mark.parametrize("scheme", [LIN, AFF])
def test_zero_and_empty_are_forward(scheme):
    for read, win in ((b"NNNN", b"ACGTACGT"), (b"", b"ACGT"), (b"ACGT", b"")):
        r = so.record(read, win, 7, scheme)
        assert r == so.Record(0, -1, -1, 0, -1, 0, [])


@pytest.mark.parametrize("scheme", [LIN, AFF])
def test_reverse_read(scheme):
    r = so.record(so.revcomp(X), X, 500, scheme)
    assert r == so.Record(2 * len(X), len(X) - 1, len(X) - 1, 1, 500, 0, [len(X) << 4])
    f = ao.record(so.revcomp(X), X, 500, *scheme)
    assert f.score < r.score          # what the one-strand call reports for it


@pytest.mark.parametrize("scheme", [LIN, AFF])
def test_reverse_read_with_an_insertion(scheme):
    """The oriented read is X with N inserted after 14 bases; the read in the
    file is its reverse complement.  The CIGAR is in oriented coordinates:
    14M 1I 14M, not 14M 1I 14M counted from the file read's first base -- the
    two differ here in nothing but the NM walk, so the soft-clipped variant
    below pins the direction."""
    orient = X[:14] + b"N" + X[14:]
    r = so.record(so.revcomp(orient), b"TT" + X + b"TT", 1000, scheme)
    assert r.strand == 1 and r.ref_pos == 1002 and r.nm == 1
    assert ao.cigar_text(r.ops) == "14M1I14M" and ao.read_bases(r.ops) == len(orient)
    # a leading clip in oriented coordinates: junk in front of the oriented read is at the END of the file read
    orient = b"NNN" + X[:14] + b"N" + X[14:]
    r = so.record(so.revcomp(orient), b"TT" + X + b"TT", 1000, scheme)
    assert r.strand == 1 and ao.cigar_text(r.ops) == "3S14M1I14M" and ao.read_bases(r.ops) == len(orient)
    assert r.end_i == len(orient) - 1


def test_batch_form_agrees_with_the_single_one():
    reads = [X, so.revcomp(X), b"ACGT", b"NNNN", b"", so.revcomp(X[:14] + b"N" + X[14:])]
    wins = [b"AA" + X + b"CC"] * 5 + [b"TT" + X + b"TT"]
    pos = [10, 20, 30, 40, 50, 60]
    for scheme in (LIN, AFF):
        assert so.records(reads, wins, pos, scheme) == [so.record(r, w, p, scheme) for r, w, p in zip(reads, wins, pos)]
