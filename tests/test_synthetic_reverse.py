"""synthetic.write_wgs_dataset(reverse_fraction=...) (CPU only): at 0.0 the
lane files and batches are those of a call without the argument; above it a
seeded share of the reads is written reverse-complemented and recorded."""
import dataclasses
import gzip
import os

import numpy as np

import strand_oracle as so
from mini_parallel_amd.synthetic import write_wgs_dataset

KW = dict(lanes=1, reads_per_lane=2, reads_per_file=120, bgzf=True)


def file_bytes(ds):
    return [open(f, "rb").read() for f in ds["files"]] + [open(ds["reference"], "rb").read()]


def test_zero_fraction_changes_nothing(tmp_path):
    a = write_wgs_dataset(str(tmp_path / "a"), **KW)
    b = write_wgs_dataset(str(tmp_path / "b"), reverse_fraction=0.0, **KW)
    assert file_bytes(a) == file_bytes(b)
    for x, y in zip(a["batches"], b["batches"]):
        assert x.reverse is None and y.reverse is None
        for f in dataclasses.fields(x):
            if f.name != "reverse":
                assert np.array_equal(getattr(x, f.name), getattr(y, f.name)), f.name
        assert y.slice(3, 9).reverse is None


def test_reverse_reads_are_written_and_recorded(tmp_path):
    a = write_wgs_dataset(str(tmp_path / "a"), **KW)
    b = write_wgs_dataset(str(tmp_path / "b"), reverse_fraction=0.5, **KW)
    c = write_wgs_dataset(str(tmp_path / "c"), reverse_fraction=0.5, **KW)
    assert file_bytes(b) == file_bytes(c) and file_bytes(b)[:2] != file_bytes(a)[:2]      # seeded
    for f, x, y in zip(b["files"], a["batches"], b["batches"]):
        assert y.reverse.dtype == bool and 30 < int(y.reverse.sum()) < 90
        assert np.array_equal(x.pos, y.pos) and np.array_equal(x.wins, y.wins) and np.array_equal(x.read_len, y.read_len)
        lines = gzip.open(f, "rb").read().split(b"\n")
        for p in range(y.n_pairs):
            m = int(y.read_len[p])
            fwd = x.reads[p, :m].tobytes()
            want = so.revcomp(fwd) if y.reverse[p] else fwd
            assert y.reads[p, :m].tobytes() == want and lines[4 * p + 1] == want, p
        assert np.array_equal(y.slice(5, 50).reverse, y.reverse[5:50])
    assert os.path.basename(b["files"][0]) == os.path.basename(a["files"][0])
