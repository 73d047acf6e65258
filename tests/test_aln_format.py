"""The .aln file format (mini_parallel_amd/alnfile.py): round trip with blocks
out of order, rejection of damaged files, and cigar_string with soft clips."""
import os
import struct
import subprocess

import numpy as np
import pytest

from mini_parallel_amd import AlnBlock, cigar_string, read_alignments, write_alignments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 4


def block(first, n, seed):
    rng = np.random.default_rng(seed)
    cigars = []
    for k in range(n):
        kind = (first + k) % 4
        if kind == 0:
            cigars.append(np.zeros(0, np.uint32))                               # score 0
        elif kind == 1:
            cigars.append(np.array([150 << 4], np.uint32))
        elif kind == 2:
            cigars.append(np.array([3 << 4 | S, 100 << 4, 2 << 4 | 1, 45 << 4], np.uint32))
        else:
            cigars.append(np.array([70 << 4, 1 << 4 | 2, 75 << 4, 5 << 4 | S], np.uint32))
    score = np.array([0 if len(c) == 0 else int(rng.integers(1, 300)) for c in cigars], np.int32)
    ref = np.where(score > 0, rng.integers(0, 3 << 32, n), -1).astype(np.int64)     # past 2^32: the field is 64-bit
    nm = np.where(score > 0, rng.integers(0, 9, n), 0).astype(np.int32)
    ei = np.where(score > 0, rng.integers(0, 150, n), -1).astype(np.int16)
    ej = np.where(score > 0, rng.integers(0, 300, n), -1).astype(np.int16)
    return AlnBlock(first, ref, score, nm, ei, ej, cigars)


def joined(blocks):
    blocks = sorted(blocks, key=lambda b: b.first_read)
    cat = lambda k: np.concatenate([getattr(b, k) for b in blocks])
    return cat("ref_pos"), cat("score"), cat("nm"), cat("end_i"), cat("end_j"), [c for b in blocks for c in b.cigars]


def test_round_trip_blocks_out_of_order(tmp_path):
    blocks = [block(0, 100, 1), block(100, 100, 2), block(200, 57, 3), block(257, 0, 4), block(257, 1, 5)]
    path = tmp_path / "lane.aln"
    write_alignments(path, [blocks[2], blocks[0], blocks[4], blocks[3], blocks[1]])
    got = read_alignments(path)
    ref, score, nm, ei, ej, cigars = joined([b for b in blocks if len(b.score)])
    assert got.ref_pos.dtype == np.int64 and got.score.dtype == np.int32 and got.end_i.dtype == np.int16
    for a, b in ((got.ref_pos, ref), (got.score, score), (got.nm, nm), (got.end_i, ei), (got.end_j, ej)):
        assert np.array_equal(a, b)
    assert len(got.cigars) == 258 and all(np.array_equal(a, b) for a, b in zip(got.cigars, cigars))
    assert np.array_equal(got.cigars.n_cigar, [len(c) for c in cigars])


def test_layout_is_the_documented_one(tmp_path):
    path = tmp_path / "one.aln"
    write_alignments(path, [AlnBlock(0, [12345678901], [40], [1], [19], [25], [[2 << 4 | S, 18 << 4]])])
    raw = path.read_bytes()
    assert raw[:32] == b"MSWA" + struct.pack("<IQII8x", 1, 0, 1, 2)
    assert raw[32:56] == struct.pack("<qiiIhh", 12345678901, 40, 1, 2, 19, 25)
    assert raw[56:] == struct.pack("<II", 2 << 4 | S, 18 << 4)


def test_empty_file_is_no_reads(tmp_path):
    path = tmp_path / "empty.aln"
    path.write_bytes(b"")
    got = read_alignments(path)
    assert len(got.score) == 0 and len(got.cigars) == 0


def test_rejects_gap_overlap_magic_truncation(tmp_path):
    a, b, c = block(0, 10, 1), block(10, 10, 2), block(20, 10, 3)
    path = tmp_path / "bad.aln"
    write_alignments(path, [a, c])
    with pytest.raises(ValueError, match="gap"):
        read_alignments(path)
    write_alignments(path, [block(1, 10, 1)])                   # does not start at read 0
    with pytest.raises(ValueError, match="gap"):
        read_alignments(path)
    write_alignments(path, [a, block(9, 10, 2)])
    with pytest.raises(ValueError, match="overlap"):
        read_alignments(path)
    write_alignments(path, [a, b, b])
    with pytest.raises(ValueError, match="overlap"):
        read_alignments(path)
    write_alignments(path, [a, b])
    good = path.read_bytes()
    path.write_bytes(b"MSWB" + good[4:])
    with pytest.raises(ValueError, match="magic"):
        read_alignments(path)
    path.write_bytes(good[:4] + struct.pack("<I", 2) + good[8:])
    with pytest.raises(ValueError, match="version"):
        read_alignments(path)
    for cut in (len(good) - 1, len(good) - 4, 40, 31, 3):       # inside the ops, the records, a header
        path.write_bytes(good[:cut])
        with pytest.raises(ValueError, match="truncated"):
            read_alignments(path)
    # a header whose op count disagrees with its records
    n_ops = struct.unpack_from("<I", good, 20)[0]
    path.write_bytes(good[:20] + struct.pack("<I", n_ops - 1) + good[24:])
    with pytest.raises(ValueError):
        read_alignments(path)


def test_cli_encoder_writes_the_format(tmp_path):
    """The CLI's C++ encoder (csrc/cli_aln_block.h, driven by tests/c/aln_block_dump.cpp
    with the arrays repeated here) against write_alignments / read_alignments:
    a block out of order, a read without ops, an empty block, values at the
    fields' limits."""
    M, I, D = 0, 1, 2
    a = AlnBlock(0, [1000, 2001, 3002], [300, 251, 12], [0, 3, 1], [149, 148, 9], [149, 299, 30],
                 [[150 << 4 | M], [100 << 4 | M, 2 << 4 | I, 47 << 4 | M], [6 << 4 | M, 144 << 4 | S]])
    b = AlnBlock(3, [70000, -1], [77, 0], [2, 0], [149, -1], [290, -1], [[5 << 4 | S, 140 << 4 | M, 5 << 4 | S], []])
    c = AlnBlock(5, [], [], [], [], [], [])
    d = AlnBlock(5, [(1 << 40) + 12345, (1 << 40) - 1], [2**31 - 1, -2**31], [-1, 2**31 - 1], [-1, 32767],
                 [-1, -32768], [[4095 << 4 | D, 1 << 4 | M], [0xFFFFFFFF]])
    exe = str(tmp_path / "aln_block_dump")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I",
                    os.path.join(ROOT, "mini_parallel_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c", "aln_block_dump.cpp"), "-o", exe], check=True)
    subprocess.run([exe, str(tmp_path / "cli.aln")], check=True)
    write_alignments(tmp_path / "py.aln", [b, a, c, d])
    assert (tmp_path / "cli.aln").read_bytes() == (tmp_path / "py.aln").read_bytes()
    got = read_alignments(tmp_path / "cli.aln")
    ref, score, nm, ei, ej, cigars = joined([a, b, d])
    for x, y in ((got.ref_pos, ref), (got.score, score), (got.nm, nm), (got.end_i, ei), (got.end_j, ej)):
        assert np.array_equal(x, y)
    assert len(got.cigars) == 7 and all(np.array_equal(x, np.asarray(y, np.uint32)) for x, y in zip(got.cigars, cigars))
    assert int(got.ref_pos[5]) == (1 << 40) + 12345 and int(got.cigars[5][0]) >> 4 == 4095


def test_cigar_string_soft_clips():
    assert cigar_string([3 << 4 | S, 12 << 4, 1 << 4 | 1, 30 << 4, 4 << 4 | S]) == "3S12M1I30M4S"
    assert cigar_string(np.array([4 << 4, 2 << 4 | 2, 8 << 4, 1 << 4 | S], np.uint32)) == "4M2D8M1S"
    assert cigar_string([]) == "*" and cigar_string(None) == "*"
    assert cigar_string([12 << 4, 1 << 4 | 1, 30 << 4]) == "12M1I30M"      # as before
