"""The GPU lane reader with quality rows (msw_gfastq_open_ex with
MSW_GFASTQ_QUAL, msw_gfastq_quals; GpuFastqReader(with_qual=True)).

Over the corpus of tests/fastq_cases.py and over cases of its own that put a
span cut inside a record, the reader's output concatenated over the batches
is that of the reader without the flag (fastq_cases.reference), and the
quality rows are those of the quality-row rule of include/msw_fastq.h,
restated here over the file's bytes.  In quality mode a span ends at a whole
record, so where one batch ends and the next begins is not compared; a file
that fails delivers a prefix of the reference's reads before it does."""
import re

import numpy as np
import pytest

import fastq_cases as fc
from mini_parallel_amd import MswError
from mini_parallel_amd.fastq import GpuFastqReader

pytestmark = pytest.mark.gpu

MAX_READS = 1 << 14


def quality_rows(data: bytes, stride: int) -> np.ndarray:
    """Row r: the first min(len, stride) bytes of valid line 4r + 4 (1-based),
    zero-padded; all zeros when the file ends before that line.  One row per
    valid line 4r + 2, whatever its length (a file that fails is compared up
    to the reads it delivered)."""
    valid = []
    pieces = data.split(b"\n")
    last = pieces.pop()                      # what follows the final \n: a line if non-empty, \r and all
    lines = [p[:-1] if p.endswith(b"\r") else p for p in pieces] + ([last] if last else [])
    for ln in lines:
        try:
            ln.decode("utf-8")
        except UnicodeDecodeError:
            continue
        valid.append(ln)
    n = (len(valid) + 2) // 4                # valid lines with number % 4 == 2
    rows = np.zeros((n, stride), np.uint8)
    for r in range(n):
        if 4 * r + 3 < len(valid):
            q = valid[4 * r + 3][:stride]
            rows[r, :len(q)] = np.frombuffer(q, np.uint8)
    return rows


def read_all(ctx, path, stride, max_reads=MAX_READS, with_pos=True, reader=None):
    """-> (rows, lens, pos, quals, batch sizes, stats, error or None) of one file."""
    g = reader or GpuFastqReader(ctx, path, stride, max_reads, with_pos=with_pos, span_bytes=fc.SPAN, with_qual=True)
    if reader is not None:
        g.reset(path)
    rows, lens, pos, quals, sizes, err = [], [], [], [], [], None
    try:
        while True:
            try:
                got = g.next_batch()
            except MswError as e:
                err = e
                break
            assert len(got) == 4
            if len(got[1]) == 0:
                assert g.quals_ptr() == 0            # the end-of-file call has no batch
                break
            assert g.quals_ptr() != 0 and len(got[1]) <= max_reads
            d = g.last
            assert d.max_len >= int(got[1].max()) and d.min_len <= int(got[1].min())
            sizes.append(len(got[1]))
            rows.append(got[0])
            lens.append(got[1])
            pos.append(got[2])
            quals.append(got[3])
        st = g.stats()
    finally:
        if reader is None or err is not None:
            g.close()
    cat = lambda xs, empty: np.concatenate(xs) if xs else empty  # noqa: E731
    return (cat(rows, np.zeros((0, stride), np.uint8)), cat(lens, np.zeros(0, np.uint16)),
            cat(pos, np.zeros(0, np.int64)) if with_pos else None, cat(quals, np.zeros((0, stride), np.uint8)), sizes, st,
            err)


def check(ctx, data, path, stride, ref, max_reads=MAX_READS, name=""):
    rows, lens, pos, quals, sizes, st, err = read_all(ctx, path, stride, max_reads)
    want_q = quality_rows(data, stride)
    n = len(lens)
    if ref.code == 0:
        assert err is None, (name, err)
        assert n == ref.reads == len(want_q), (name, n, ref.reads)
        assert (st["lines"], st["reads"], st["errors"], st["bases"]) == (ref.lines, ref.reads, ref.errors, ref.bases), \
            (name, st)
    else:
        assert err is not None, name
        assert (err.code, int(re.search(r"line (\d+)", str(err)).group(1))) == (ref.code, ref.err_line), (name, err)
        if ref.code == fc.E_INVALID:
            assert str(err) == ref.message
        assert n <= ref.reads, (name, n, ref.reads)
    assert np.array_equal(lens, ref.lens[:n]), name
    assert np.array_equal(pos, ref.pos[:n]), name
    assert np.array_equal(rows, ref.rows[:n]), name
    bad = np.flatnonzero((quals != want_q[:n]).any(axis=1))
    assert len(bad) == 0, (name, bad[:5], quals[bad[:2]].tobytes(), want_q[bad[:2]].tobytes())
    return sizes


@pytest.fixture(scope="module")
def lane_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("parse_qual")
    out = {}
    for i, c in enumerate(fc.cases()):
        p = d / ("%s%d.fastq.gz" % (c.family, i))
        p.write_bytes(c.blob)
        out[c.name] = str(p)
    return out


@pytest.mark.parametrize("family", ["P", "U", "E", "C"])
def test_corpus_with_quality_rows(gpu_ctx, lane_files, family):
    for c in fc.family(family):
        check(gpu_ctx, c.data, lane_files[c.name], c.stride, fc.reference(c), name=c.name)


def test_batches_of_7(gpu_ctx, lane_files):
    """The quality emit starts at a non-zero read of its span; the batch
    boundaries are the same on a second pass."""
    for c in fc.family("P"):
        a = check(gpu_ctx, c.data, lane_files[c.name], c.stride, fc.reference(c), max_reads=7, name=c.name)
        b = read_all(gpu_ctx, lane_files[c.name], c.stride, 7)[4]
        assert a == b and max(a) == 7 and len(a) > 50


def test_without_the_flag_there_is_no_fourth_item(gpu_ctx, lane_files):
    c = fc.family("P")[0]
    with GpuFastqReader(gpu_ctx, lane_files[c.name], c.stride, MAX_READS, with_pos=True, span_bytes=fc.SPAN) as g:
        got = g.next_batch()
        assert len(got) == 3 and len(got[1]) > 0 and g.quals_ptr() == 0
    with GpuFastqReader(gpu_ctx, lane_files[c.name], c.stride, MAX_READS, span_bytes=fc.SPAN, with_qual=True) as g:
        got = g.next_batch()
        assert len(got) == 4 and got[2] is None and np.array_equal(got[3], quality_rows(c.data, c.stride)[:len(got[1])])


def test_unknown_flag_bits(gpu_ctx, lane_files):
    import ctypes
    from mini_parallel_amd._lib import MSW_E_INVALID, lib
    h = ctypes.c_void_p()
    path = lane_files[fc.family("P")[0].name].encode()
    assert lib().msw_gfastq_open_ex(gpu_ctx.handle, path, 256, 16, 4, 0, ctypes.byref(h)) == MSW_E_INVALID
    assert lib().msw_gfastq_open_ex(gpu_ctx.handle, path, 256, 16, 0x80000002, 0, ctypes.byref(h)) == MSW_E_INVALID
    assert not h.value


# ---------------------------------------------------------------------------
# Cases of this test's own: a span cut at a chosen place in a record
# ---------------------------------------------------------------------------
S = fc._seq(48)
Q = bytes(33 + (7 * k) % 60 for k in range(48))        # a quality line that is not one repeated byte
BAD = b"junk \xff\xfe line\n"


def cut_case(name, situations, seed, stride=256, tail=b""):
    """Text with the k-th (pre, post) pair on the two sides of the k-th span
    cut (members of CUT_BLOCK bytes, spans of fc.SPAN), filler records
    between, `tail` at the end; check_cuts asserts from the members' ISIZEs
    that the cuts fell there."""
    t, marks = fc._Text(seed), []
    for i, (pre, post) in enumerate(situations):
        cut = (i + 1) * fc.SPAN
        t.fill_to(cut - len(pre))
        t.add(pre)
        t.add(post)
        marks.append((cut, pre, post))
    for _ in range(3):
        t.add(t.f.record())
    t.add(tail)
    c = fc.Case(name, "Q", t.bytes(), stride=stride, block=fc.CUT_BLOCK, marks=marks)
    fc.check_cuts(c)
    return c


def own_cases():
    rec = fc._rec(b"@whole pos=77", S, q=Q)
    out = [
        cut_case("after_sequence_and_after_plus",
                 [(b"@s pos=5\n" + S + b"\n", b"+\n" + Q + b"\n"), (b"@p pos=6\n" + S + b"\n+\n", Q + b"\n")], 301),
        cut_case("inside_quality_and_inside_sequence",
                 [(b"@q pos=7\n" + S + b"\n+\n" + Q[:19], Q[19:] + b"\n"),
                  (b"@m pos=8\n" + S[:31], S[31:] + b"\n+\n" + Q + b"\n")], 302),
        cut_case("after_header_and_after_record", [(b"@h pos=9\n", S + b"\n+\n" + Q + b"\n"), (rec, rec)], 303),
        cut_case("crlf_records",
                 [(b"@c pos=10\r\n" + S + b"\r", b"\n+\r\n" + Q + b"\r\n"),
                  (b"@d pos=11\r\n" + S + b"\r\n+\r\n" + Q + b"\r", b"\n" + rec.replace(b"\n", b"\r\n"))], 304),
        # quality lines longer than the stride (truncated) and shorter than the sequence (zeros), at a cut and not
        cut_case("quality_longer_and_shorter",
                 [(b"@l pos=12\n" + S + b"\n+\n" + Q * 3, Q * 4 + b"\n"), (b"@k pos=13\n" + S + b"\n+\n" + Q[:5], Q[5:9] + b"\n")],
                 305, tail=fc._rec(b"@t pos=1", S, q=Q * 6) + fc._rec(b"@t pos=2", S, q=b"") +
                 fc._rec(b"@t pos=3", S, q=Q[:1])),
        # the file ends after a sequence line: a read without a quality line, a zero row
        cut_case("ends_after_sequence", [(b"@e pos=14\n" + S + b"\n+", b"\n" + Q + b"\n")], 306,
                 tail=b"@last pos=15\n" + S + b"\n"),
        cut_case("ends_inside_plus", [(b"@e pos=14\n" + S[:1], S[1:] + b"\n+\n" + Q + b"\n")], 307,
                 tail=b"@last pos=15\n" + S + b"\n+"),
    ]
    # An invalid line just behind the last whole record of a span, the cut inside the next record: the next span
    # sees that line again.  Ten invalid lines in all: counted once each the file reads to its end with 10 errors.
    def bads(n):
        return b"".join(fc._bad(k) + fc._rec(b"@b%d pos=%d" % (k, k), S[:20 + k], q=Q[:20 + k]) for k in range(n))

    nine = bads(9)
    behind = [(nine + rec + BAD + b"@n pos=16\n" + S[:7], S[7:] + b"\n+\n" + Q + b"\n")]
    out.append(cut_case("invalid_behind_the_tail_10", behind, 308))
    # ... and an 11th further on ends the file at the line the host reader reports
    out.append(cut_case("invalid_behind_the_tail_11", behind + [(rec + BAD + rec + b"@o pos=17\n", S + b"\n+\n" + Q + b"\n")], 309))
    # two invalid lines behind the tail, the cut right behind them
    out.append(cut_case("invalid_lines_end_the_span", [(bads(8) + rec + BAD, BAD + rec)], 310))
    return out


@pytest.fixture(scope="module")
def own(tmp_path_factory):
    d = tmp_path_factory.mktemp("parse_qual_own")
    out = []
    for c in own_cases():
        p = d / (c.name + ".fastq.gz")
        p.write_bytes(c.blob)
        out.append((c, str(p)))
    return out


def test_cuts_inside_a_record(gpu_ctx, own):
    seen = {}
    for c, path in own:
        ref = fc.reference_parse(c.data, c.stride)
        seen[c.name] = ref
        check(gpu_ctx, c.data, path, c.stride, ref, name=c.name)
    assert seen["invalid_behind_the_tail_10"].errors == 10 and seen["invalid_behind_the_tail_10"].code == 0
    assert seen["invalid_behind_the_tail_11"].code == fc.E_INVALID
    assert seen["invalid_lines_end_the_span"].errors == 10 and seen["invalid_lines_end_the_span"].code == 0
    assert seen["ends_after_sequence"].reads == len(quality_rows(own[5][0].data, 256))
    assert not quality_rows(own[5][0].data, 256)[-1].any() and not quality_rows(own[6][0].data, 256)[-1].any()
    q = quality_rows(own[4][0].data, 256)
    assert (q[:, -1] != 0).sum() >= 2 and (q[-2:, 1] == 0).all()      # truncated rows, short rows


def test_cuts_inside_a_record_through_copies_and_small_batches(gpu_ctx, own, monkeypatch):
    monkeypatch.setenv("MSW_GZ_NO_MAP", "1")
    for c, path in own[:2]:
        check(gpu_ctx, c.data, path, c.stride, fc.reference_parse(c.data, c.stride), max_reads=7, name=c.name)
