"""Strand bytes in ``.aln`` blocks (flag bit 0 of the version-1 header; CPU
only): round trips, the documented bytes, the padding, every refusal, and the
CLI's C++ encoder against write_alignments."""
import os
import struct
import subprocess

import numpy as np
import pytest

from mini_parallel_amd import AlnBlock, read_alignments, write_alignments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, I, S = 0, 1, 4


def block(first, n, seed, strand):
    rng = np.random.default_rng(seed)
    score = rng.integers(0, 300, n).astype(np.int32)
    cigars = [rng.integers(1, 1 << 12, int(k)).astype(np.uint32) << 4 for k in rng.integers(0, 4, n)]
    return AlnBlock(first, rng.integers(-1, 1 << 40, n), score, rng.integers(0, 9, n).astype(np.int32),
                    rng.integers(-1, 384, n).astype(np.int16), rng.integers(-1, 4096, n).astype(np.int16), cigars,
                    rng.integers(0, 2, n).astype(np.uint8) if strand else None)


def test_flagged_and_unflagged_blocks_in_one_file(tmp_path):
    blocks = [block(0, 100, 1, True), block(100, 57, 2, False), block(157, 0, 3, True), block(157, 3, 4, True)]
    path = tmp_path / "lane.aln"
    write_alignments(path, [blocks[3], blocks[1], blocks[0], blocks[2]])
    got = read_alignments(path)
    assert got.strand.dtype == np.uint8 and len(got.strand) == 160
    want = np.concatenate([blocks[0].strand, np.zeros(57, np.uint8), blocks[3].strand])
    assert np.array_equal(got.strand, want) and want[:100].any() and want[157:].size == 3
    for k in ("ref_pos", "score", "nm", "end_i", "end_j"):
        assert np.array_equal(getattr(got, k), np.concatenate([getattr(b, k) for b in blocks])), k
    assert all(np.array_equal(a, b) for a, b in zip(got.cigars, [c for b in blocks for c in b.cigars]))
    assert got[-1] is got.strand                    # the last field


def test_flagged_block_bytes_are_the_documented_ones(tmp_path):
    path = tmp_path / "one.aln"
    write_alignments(path, [AlnBlock(0, [12345678901], [40], [1], [19], [25], [[2 << 4 | S, 18 << 4]], [1])])
    raw = path.read_bytes()
    assert raw[:32] == b"MSWA" + struct.pack("<IQIII4x", 1, 0, 1, 2, 1)
    assert raw[32:56] == struct.pack("<qiiIhh", 12345678901, 40, 1, 2, 19, 25)
    assert raw[56:64] == struct.pack("<II", 2 << 4 | S, 18 << 4)
    assert raw[64:] == b"\x01\x00\x00\x00"


def test_unflagged_file_is_what_it_was(tmp_path):
    """The bytes tests/test_aln_format.py documents, from a block without strand."""
    path = tmp_path / "one.aln"
    write_alignments(path, [AlnBlock(0, [12345678901], [40], [1], [19], [25], [[2 << 4 | S, 18 << 4]])])
    raw = path.read_bytes()
    assert raw == (b"MSWA" + struct.pack("<IQII8x", 1, 0, 1, 2) + struct.pack("<qiiIhh", 12345678901, 40, 1, 2, 19, 25) +
                   struct.pack("<II", 2 << 4 | S, 18 << 4))
    got = read_alignments(path)
    assert got.strand.tolist() == [0]
    write_alignments(path, [(0, [12345678901], [40], [1], [19], [25], [[2 << 4 | S, 18 << 4]])])      # a plain 7-tuple
    assert path.read_bytes() == raw


@pytest.mark.parametrize("n,pad", [(1, 3), (3, 1), (4, 0), (5, 3), (0, 0)])
def test_padding(tmp_path, n, pad):
    path = tmp_path / "pad.aln"
    strand = [1] * n
    write_alignments(path, [AlnBlock(0, [7] * n, [2] * n, [0] * n, [0] * n, [0] * n, [[1 << 4]] * n, strand)])
    raw = path.read_bytes()
    assert len(raw) == 32 + 24 * n + 4 * n + n + pad and len(raw) % 4 == 0
    assert raw[len(raw) - n - pad:] == b"\x01" * n + b"\x00" * pad
    assert struct.unpack_from("<I", raw, 24)[0] == 1          # an empty flagged block still says so
    got = read_alignments(path)
    assert got.strand.tolist() == strand and len(got.score) == n


def test_refusals(tmp_path):
    path = tmp_path / "bad.aln"
    write_alignments(path, [block(0, 5, 9, True)])
    good = path.read_bytes()
    assert read_alignments(path).strand.size == 5
    put = lambda at, b: path.write_bytes(good[:at] + b + good[at + len(b):])
    put(24, struct.pack("<I", 3))                                   # bit 1 is not defined
    with pytest.raises(ValueError, match="flag"):
        read_alignments(path)
    put(24, struct.pack("<I", 0x80000001))
    with pytest.raises(ValueError, match="flag"):
        read_alignments(path)
    for at in (28, 31):                                             # bytes 28..31 stay zero
        put(at, b"\x01")
        with pytest.raises(ValueError, match="reserved"):
            read_alignments(path)
    put(len(good) - 8, b"\x02")                                     # the first of 5 strand bytes (+ 3 pad)
    with pytest.raises(ValueError, match="strand"):
        read_alignments(path)
    for cut in (1, 3, 4, 7):                                        # inside the padding and the strand bytes
        path.write_bytes(good[:len(good) - cut])
        with pytest.raises(ValueError, match="truncated"):
            read_alignments(path)
    # the flag set on a block that has no strand bytes behind it: the next header is not there
    write_alignments(path, [block(0, 5, 9, False)])
    plain = path.read_bytes()
    path.write_bytes(plain[:24] + struct.pack("<I", 1) + plain[28:])
    with pytest.raises(ValueError, match="truncated"):
        read_alignments(path)
    with pytest.raises(ValueError):
        write_alignments(path, [AlnBlock(0, [1], [1], [0], [0], [0], [[1 << 4]], [2])])
    with pytest.raises(ValueError):
        write_alignments(path, [AlnBlock(0, [1], [1], [0], [0], [0], [[1 << 4]], [0, 1])])


def test_cli_encoder_writes_strand_blocks(tmp_path):
    """csrc/cli_aln_block.h driven by tests/c/aln_strand_dump.cpp (the arrays
    repeated here) against write_alignments, byte for byte."""
    a = AlnBlock(0, [1000, 2001, -1], [300, 251, 0], [0, 3, 0], [149, 148, -1], [149, 299, -1],
                 [[150 << 4 | M], [100 << 4 | M, 2 << 4 | I, 47 << 4 | M], []], [1, 0, 0])
    b = AlnBlock(3, [70000], [77], [2], [149], [290], [[5 << 4 | S, 140 << 4 | M, 5 << 4 | S]])
    e = AlnBlock(4, [], [], [], [], [], [], [])
    c = AlnBlock(4, [-1, -1, -1, -1, 5], [0, 0, 0, 0, 16], [0] * 5, [-1, -1, -1, -1, 7], [-1, -1, -1, -1, 9],
                 [[], [], [], [], [8 << 4 | M]], [0, 0, 0, 0, 1])
    exe = str(tmp_path / "aln_strand_dump")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I",
                    os.path.join(ROOT, "mini_parallel_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c", "aln_strand_dump.cpp"), "-o", exe], check=True)
    subprocess.run([exe, str(tmp_path / "cli.aln")], check=True)
    write_alignments(tmp_path / "py.aln", [a, b, e, c])
    assert (tmp_path / "cli.aln").read_bytes() == (tmp_path / "py.aln").read_bytes()
    got = read_alignments(tmp_path / "cli.aln")
    assert got.strand.tolist() == [1, 0, 0, 0, 0, 0, 0, 0, 1] and got.score.tolist() == [300, 251, 0, 77, 0, 0, 0, 0, 16]
