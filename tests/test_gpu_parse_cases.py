"""The GPU record parse (msw_parse.hip through GpuFastqReader) against
reference_parse, a plain-Python restatement of aligner.rs:128-170, on the
corpus of tests/fastq_cases.py (checked against the host reader on the CPU by
tests/test_fastq_cases.py): pos= forms at the limits of the 16-lane parse,
every UTF-8 boundary form in each line of a record, line ends, and chosen
bytes on the two sides of a span cut.  Arrays and statistics bit-exact.

A reader's max_reads is at or above the reads of a span and batches never
cross spans, so the batch sizes are the reads per span predicted from the
members' ISIZEs: a cut case that did not meet its cut fails there."""
import re

import numpy as np
import pytest

import fastq_cases as fc
from mini_parallel_amd import MswError
from mini_parallel_amd.fastq import GpuFastqReader

pytestmark = pytest.mark.gpu

MAX_READS = 1 << 14


@pytest.fixture(scope="module")
def lane_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("parse_cases")
    out = {}
    for i, c in enumerate(fc.cases()):
        p = d / ("%s%d.fastq.gz" % (c.family, i))
        p.write_bytes(c.blob)
        out[c.name] = str(p)
    return out


class Readers:
    """One reader per stride, pointed at file after file (reset); a reader
    that failed a file is closed, the next file of that stride gets a new one."""

    def __init__(self, ctx, max_reads, with_pos):
        self.ctx, self.max_reads, self.with_pos, self.open = ctx, max_reads, with_pos, {}

    def reader(self, path, stride):
        g = self.open.get(stride)
        if g is None:
            g = self.open[stride] = GpuFastqReader(self.ctx, path, stride, self.max_reads, with_pos=self.with_pos,
                                                   span_bytes=fc.SPAN)
        else:
            g.reset(path)
        return g

    def drop(self, stride):
        self.open.pop(stride).close()

    def close(self):
        for g in self.open.values():
            g.close()
        self.open = {}


def check_case(rd: Readers, c, path):
    ref = fc.reference(c, rd.with_pos)
    want = fc.expected_batches(ref, c.cuts, rd.max_reads)
    per_span = np.bincount(fc.span_of(c.cuts, ref.ends), minlength=1)
    assert rd.max_reads >= per_span.max() or rd.max_reads == 7
    g = rd.reader(path, c.stride)
    rows, lens, pos, sizes, err = [], [], [], [], None
    while True:
        try:
            got = g.next_batch()
        except MswError as e:
            err = e
            break
        if len(got[1]) == 0:
            break
        d = g.last
        # the bounds the scorer picks its kernel by
        assert d.max_len >= int(got[1].max()) and d.min_len <= int(got[1].min()), (c.name, len(sizes))
        sizes.append(len(got[1]))
        rows.append(got[0])
        lens.append(got[1])
        pos.append(got[2] if rd.with_pos else None)
    st = g.stats()
    if err is not None:
        rd.drop(c.stride)
    assert sizes == want, (c.name, sizes, want)
    n = sum(want)
    if n:
        assert np.array_equal(np.concatenate(lens), ref.lens[:n]), c.name
        if rd.with_pos:
            p = np.concatenate(pos)
            bad = np.flatnonzero(p != ref.pos[:n])
            assert len(bad) == 0, (c.name, bad[:5], p[bad[:5]], ref.pos[bad[:5]])
        assert np.array_equal(np.concatenate(rows), ref.rows[:n]), c.name
    if ref.code == 0:
        assert err is None, (c.name, err)
        assert n == ref.reads
        assert (st["lines"], st["reads"], st["errors"], st["bases"]) == (ref.lines, ref.reads, ref.errors, ref.bases), \
            (c.name, st)
    else:
        assert err is not None, c.name
        assert (err.code, int(re.search(r"line (\d+)", str(err)).group(1))) == (ref.code, ref.err_line), (c.name, err)
        if ref.code == fc.E_INVALID:
            assert str(err) == ref.message


def run_family(ctx, lane_files, family, max_reads=MAX_READS, with_pos=True):
    rd = Readers(ctx, max_reads, with_pos)
    try:
        for c in fc.family(family):
            check_case(rd, c, lane_files[c.name])
    finally:
        rd.close()


@pytest.mark.parametrize("family", ["P", "U", "E"])
def test_parse_matches_reference(gpu_ctx, lane_files, family):
    run_family(gpu_ctx, lane_files, family)


@pytest.mark.parametrize("mode", ["map", "copy"])
def test_parse_at_span_cuts(gpu_ctx, lane_files, monkeypatch, mode):
    """Family C: every case's chosen bytes on the two sides of a 1 MiB span
    cut, compressed bytes from the file's mapping and through pinned copies."""
    monkeypatch.setenv("MSW_GZ_NO_MAP", "1" if mode == "copy" else "0")
    run_family(gpu_ctx, lane_files, "C")


@pytest.mark.parametrize("family", ["P", "U"])
def test_parse_without_pos(gpu_ctx, lane_files, family):
    run_family(gpu_ctx, lane_files, family, with_pos=False)


def test_parse_pos_small_batches(gpu_ctx, lane_files):
    """Batches of 7 reads: the emit starts at a non-zero read of its span."""
    run_family(gpu_ctx, lane_files, "P", max_reads=7)
