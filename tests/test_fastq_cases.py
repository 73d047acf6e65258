"""The FASTQ parse corpus (tests/fastq_cases.py) on the CPU: the builders keep
their promises, and the host reader (msw_fastq.cpp) reads every case exactly
as reference_parse does -- rows, lengths, pos=, statistics, and for a file
that fails the error code, the line number and the error limit's message --
as gzip, as BGZF and as plain text.  The GPU parse meets the same corpus in
tests/test_gpu_parse_cases.py."""
import gzip
import re

import numpy as np
import pytest

import fastq_cases as fc
from mini_parallel_amd import MswError
from mini_parallel_amd.fastq import FastqReader
from test_fastq import reference_chunks

CHUNK = 1000  # reads per next_chunk call


def err_line_of(e: MswError) -> int:
    return int(re.search(r"line (\d+)", str(e)).group(1))


def host_parse(path, stride, with_pos=True):
    """-> rows, lens, pos (of the calls that succeeded), stats, the MswError or None."""
    rows, lens, pos, err = [], [], [], None
    with FastqReader(path) as fq:
        while True:
            try:
                got = fq.next_chunk(CHUNK, stride, with_pos=with_pos)
            except MswError as e:
                err = e
                break
            if len(got[1]) == 0:
                break
            rows.append(got[0])
            lens.append(got[1])
            pos.append(got[2] if with_pos else None)
        st = fq.stats()
    cat = (lambda a, e: np.concatenate(a) if a else e)
    return (cat(rows, np.zeros((0, stride), np.uint8)), cat(lens, np.zeros(0, np.uint16)),
            cat(pos, np.zeros(0, np.int64)) if with_pos else None, st, err)


def assert_host_matches(c, path, with_pos=True):
    ref = fc.reference(c, with_pos)
    rows, lens, pos, st, err = host_parse(path, c.stride, with_pos)
    # a failing call delivers nothing: whole chunks of the reads before the failure
    n = ref.reads if ref.code == 0 else ref.reads // CHUNK * CHUNK
    assert len(lens) == n, c.name
    assert np.array_equal(lens, ref.lens[:n]), c.name
    assert np.array_equal(rows, ref.rows[:n]), c.name
    if with_pos:
        assert np.array_equal(pos, ref.pos[:n]), (c.name, np.flatnonzero(pos != ref.pos[:n])[:5])
    if ref.code == 0:
        assert err is None, (c.name, err)
        assert (st["lines"], st["reads"], st["errors"]) == (ref.lines, ref.reads, ref.errors), c.name
    else:
        assert err is not None and err.code == ref.code, (c.name, err)
        assert err_line_of(err) == ref.err_line, (c.name, err)
        if ref.code == fc.E_INVALID:
            assert str(err) == ref.message


def test_builders_keep_their_promises():
    names = [c.name for c in fc.cases()]
    assert len(set(names)) == len(names)
    for c in fc.family("P"):
        ref = fc.reference(c)
        assert ref.code == 0 and ref.errors == 0 and ref.reads > 2500
        # tagged headers start on all four alignments, on both sides of the 60-byte limit
        assert all(c.info["align"][(a, big)] > 0 for a in range(4) for big in (False, True))
        assert ref.pos.min() < -10 ** 17 and ref.pos.max() >= 10 ** 17  # 18 digits, both signs
        assert len(c.cuts) == 0
    assert any(b"\xc3\xa9" in c.data for c in fc.family("P")) and any(max(c.data) < 0x80 for c in fc.family("P"))
    for c in fc.family("U"):
        ref = fc.reference(c)
        assert ref.code == c.info.get("code", 0), c.name
        if "errors" in c.info:  # within the budget: read to the end
            assert ref.code == 0 and ref.errors == c.info["errors"] <= 10, c.name
        if "err_line" in c.info:
            assert ref.err_line == c.info["err_line"], c.name
    u = {c.name: c for c in fc.family("U")}
    assert sum(fc.reference(c).errors == 10 and fc.reference(c).code == 0 for c in u.values()) >= 4
    assert fc.reference(u["U_err_first"]).message == fc.ERR_LIMIT_MSG % 0
    two = u["U_err_next_span"]
    assert two.cuts == [fc.SPAN] and list(fc.span_of(two.cuts, two.info["bad_at"])) == [0] * 10 + [1]
    for f in fc.U_VALID:
        f.decode("utf-8")
    for f in fc.U_INVALID + [t[0] for t in fc.U_TRUNC]:
        with pytest.raises(UnicodeDecodeError):
            f.decode("utf-8")
    for c in fc.family("E"):
        assert fc.reference(c).code == c.info["code"], c.name
    labels = []
    for c in fc.family("C"):
        fc.check_cuts(c)
        assert len(c.marks) == (2 if c.info["end"] is None else 1)
        if c.info["end"]:
            assert len(c.data) == 2 * fc.SPAN and (c.data[-1:] == b"\n") == (c.info["end"] == "nl")
        ref = fc.reference(c)
        per = np.bincount(fc.span_of(c.cuts, ref.ends), minlength=len(c.cuts) + 1)
        assert ref.code == 0 and len(per) == len(c.cuts) + 1 and per.min() > 0  # reads in every span
        labels += c.info["labels"]
    assert len(labels) == len(set(labels)) == 28
    # the carried part of the mid-sequence cuts: 1..17 bytes, every (16 - n) & 15
    carried = sorted(len(pre) - pre.index(b"\n") - 1 for c in fc.family("C") for _, pre, _ in c.marks
                     if pre.startswith(b"@m"))
    assert carried == list(range(1, 18))
    assert sum(len(c.data) for c in fc.cases()) < 34 << 20


@pytest.mark.parametrize("form", ["gzip", "bgzf", "plain"])
@pytest.mark.parametrize("family", list("PUEC"))
def test_host_reader_matches_reference(tmp_path, family, form):
    for i, c in enumerate(fc.family(family)):
        p = tmp_path / ("%d.fastq" % i if form == "plain" else "%d.fastq.gz" % i)
        p.write_bytes({"gzip": lambda: gzip.compress(c.data, 1), "bgzf": lambda: c.blob, "plain": lambda: c.data}[form]())
        assert_host_matches(c, str(p))
        if family in "PE" and form == "plain":
            assert_host_matches(c, str(p), with_pos=False)


def old_rule_sequences(data: bytes):
    """The sequences under the rule both readers used to follow: a trailing
    \\r stripped from every line, with or without a \\n after it."""
    lines = data.split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    out, count = [], 0
    for raw in lines:
        raw = raw[:-1] if raw.endswith(b"\r") else raw
        try:
            raw.decode("utf-8")
        except UnicodeDecodeError:
            continue
        count += 1
        if count % 4 == 2:
            out.append(raw)
    return out


def test_reference_agrees_with_reference_chunks():
    """Two independent restatements give the same sequences on every case
    that reads to the end (reference_chunks knows no stride and no pos=).
    The files ending in a sequence line's \\r without \\n are where the old
    rule and BufRead::lines differ: they do differ there."""
    differ = []
    for c in fc.cases():
        ref = fc.reference(c)
        if ref.code:
            continue
        want = [bytes(r[:n]) for r, n in zip(ref.rows, ref.lens)]
        got = [s.encode() for ch in reference_chunks(c.data, 777) for s in ch]
        assert got == want, c.name
        if old_rule_sequences(c.data) != want:
            differ.append(c.name)
    assert differ == ["E_cr_eof_seq", "E_cr_eof_crlf_file", "E_cr_only_seq_eof", "E_stride_crlf_eof"]
    c = {c.name: c for c in fc.family("E")}["E_cr_eof_seq"]
    assert bytes(fc.reference(c).rows[-1][:5]) == b"ACGT\r" and old_rule_sequences(c.data)[-1] == b"ACGT"
