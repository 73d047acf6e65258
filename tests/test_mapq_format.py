"""Flag bit 1 of the ``.aln`` format (mini_parallel_amd/alnfile.py): a mapq
byte and a sub-optimal score per read, after the strand bytes.  CPU only."""
import os
import struct
import subprocess

import numpy as np
import pytest

from mini_parallel_amd.alnfile import AlnBlock, read_alignments, write_alignments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, I, S = 0, 1, 4


def block(first, n, seed, strand, mapq):
    rng = np.random.default_rng(seed)
    score = rng.integers(0, 300, n).astype(np.int32)
    cigars = [rng.integers(1, 1 << 12, int(k)).astype(np.uint32) << 4 for k in rng.integers(0, 4, n)]
    return AlnBlock(first, rng.integers(-1, 1 << 40, n), score, rng.integers(0, 9, n).astype(np.int32),
                    rng.integers(-1, 384, n).astype(np.int16), rng.integers(-1, 4096, n).astype(np.int16), cigars,
                    rng.integers(0, 2, n).astype(np.uint8) if strand else None,
                    rng.integers(0, 61, n).astype(np.uint8) if mapq else None,
                    rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32) if mapq else None)


@pytest.mark.parametrize("strand", [True, False])
def test_round_trip(tmp_path, strand):
    blocks = [block(0, 100, 1, strand, True), block(100, 57, 2, strand, True), block(157, 0, 3, strand, True),
              block(157, 3, 4, strand, True)]
    path = tmp_path / "lane.aln"
    write_alignments(path, [blocks[3], blocks[1], blocks[0], blocks[2]])
    got = read_alignments(path)
    assert got.mapq.dtype == np.uint8 and got.sub_score.dtype == np.int32 and len(got.mapq) == 160
    for k in ("ref_pos", "score", "nm", "end_i", "end_j", "mapq", "sub_score") + (("strand",) if strand else ()):
        assert np.array_equal(getattr(got, k), np.concatenate([getattr(b, k) for b in blocks])), k
    if not strand:
        assert not got.strand.any()
    assert all(np.array_equal(a, b) for a, b in zip(got.cigars, [c for b in blocks for c in b.cigars]))
    assert got.mapq.max() == 60 and got.sub_score.min() < 0


def test_mixed_file(tmp_path):
    """Every combination of the two flags in one file; reads from blocks
    without bit 1 have mapq 255 and sub_score 0."""
    blocks = [block(0, 5, 1, False, False), block(5, 6, 2, True, False), block(11, 7, 3, False, True),
              block(18, 9, 4, True, True)]
    path = tmp_path / "mixed.aln"
    write_alignments(path, blocks)
    raw = path.read_bytes()
    got = read_alignments(path)
    assert got.mapq.tolist() == [255] * 11 + blocks[2].mapq.tolist() + blocks[3].mapq.tolist()
    assert got.sub_score.tolist() == [0] * 11 + blocks[2].sub_score.tolist() + blocks[3].sub_score.tolist()
    assert got.strand.tolist() == [0] * 5 + blocks[1].strand.tolist() + [0] * 7 + blocks[3].strand.tolist()
    flags, at = [], 0
    for b in blocks:
        n, n_ops, fl = struct.unpack_from("<III", raw, at + 16)
        flags.append(fl)
        at += 32 + 24 * n + 4 * n_ops + ((n + 3) // 4 * 4 if fl & 1 else 0) + ((n + 3) // 4 * 4 + 4 * n if fl & 2 else 0)
    assert flags == [0, 1, 2, 3] and at == len(raw)


def test_flagged_block_bytes_are_the_documented_ones(tmp_path):
    path = tmp_path / "one.aln"
    one = (0, [12345678901], [40], [1], [19], [25], [[2 << 4 | S, 18 << 4]])
    write_alignments(path, [AlnBlock(*one, [1], [37], [-2])])
    raw = path.read_bytes()
    assert raw == (struct.pack("<4sIQIIII", b"MSWA", 1, 0, 1, 2, 3, 0) + struct.pack("<qiiIhh", 12345678901, 40, 1, 2, 19, 25)
                   + struct.pack("<II", 2 << 4 | S, 18 << 4) + b"\x01\x00\x00\x00" + b"\x25\x00\x00\x00"
                   + struct.pack("<i", -2))
    write_alignments(path, [AlnBlock(*one, None, [37], [-2])])
    assert path.read_bytes() == raw[:24] + struct.pack("<I", 2) + raw[28:64] + raw[68:]


@pytest.mark.parametrize("strand", [True, False])
def test_a_block_without_bit_1_is_what_it_was(tmp_path, strand):
    """The writer's bytes for a block without mapq, against the layout built
    here field by field (the format before the bit existed)."""
    b = block(0, 7, 5, strand, False)
    path = tmp_path / "plain.aln"
    write_alignments(path, [b])
    n_ops = sum(len(c) for c in b.cigars)
    want = struct.pack("<4sIQIIII", b"MSWA", 1, 0, 7, n_ops, 1 if strand else 0, 0)
    for p in range(7):
        want += struct.pack("<qiiIhh", int(b.ref_pos[p]), int(b.score[p]), int(b.nm[p]), len(b.cigars[p]), int(b.end_i[p]),
                            int(b.end_j[p]))
    want += b"".join(np.asarray(c, "<u4").tobytes() for c in b.cigars)
    if strand:
        want += bytes(b.strand.tolist()) + b"\x00"
    assert path.read_bytes() == want
    # and the same block written through the three new fields left at None
    write_alignments(path, [AlnBlock(*b[:8], None, None)])
    assert path.read_bytes() == want


@pytest.mark.parametrize("n,pad", [(1, 3), (3, 1), (4, 0), (5, 3), (0, 0)])
def test_padding(tmp_path, n, pad):
    path = tmp_path / "pad.aln"
    write_alignments(path, [AlnBlock(0, [7] * n, [2] * n, [0] * n, [0] * n, [0] * n, [[1 << 4]] * n, None, [9] * n,
                                     [3] * n)])
    raw = path.read_bytes()
    assert len(raw) == 32 + 24 * n + 4 * n + n + pad + 4 * n
    assert raw[len(raw) - 4 * n - n - pad:len(raw) - 4 * n] == b"\x09" * n + b"\x00" * pad
    assert struct.unpack_from("<I", raw, 24)[0] == 2          # an empty flagged block still says so
    got = read_alignments(path)
    assert got.mapq.tolist() == [9] * n and got.sub_score.tolist() == [3] * n


def test_refusals(tmp_path):
    path = tmp_path / "bad.aln"
    write_alignments(path, [block(0, 5, 9, True, True)])
    good = path.read_bytes()
    assert read_alignments(path).mapq.size == 5
    put = lambda at, b: path.write_bytes(good[:at] + b + good[at + len(b):])
    for bits in (4, 7, 0x80000003):                                 # bits above 1 are not defined
        put(24, struct.pack("<I", bits))
        with pytest.raises(ValueError, match="flag"):
            read_alignments(path)
    mq = len(good) - 20 - 8                                          # 5 mapq bytes + 3 pad, then 5 x i32
    put(mq, b"\x3d")                                                # 61
    with pytest.raises(ValueError, match="mapq"):
        read_alignments(path)
    put(mq + 4, b"\xff")
    with pytest.raises(ValueError, match="mapq"):
        read_alignments(path)
    put(mq, b"\x3c")                                                # 60 is fine
    assert read_alignments(path).mapq[0] == 60
    for at in (mq + 5, mq + 7):                                     # the mapq padding
        put(at, b"\x01")
        with pytest.raises(ValueError, match="padding"):
            read_alignments(path)
    put(mq - 1, b"\x01")                                            # the strand padding in front of it
    with pytest.raises(ValueError, match="padding"):
        read_alignments(path)
    put(mq - 8, b"\x02")                                            # the first strand byte
    with pytest.raises(ValueError, match="strand"):
        read_alignments(path)
    for cut in (1, 4, 19, 20, 21, 27):                              # inside sub_score, the padding, the mapq bytes
        path.write_bytes(good[:len(good) - cut])
        with pytest.raises(ValueError, match="truncated"):
            read_alignments(path)
    # bit 1 set on a block that has no mapq bytes behind it
    write_alignments(path, [block(0, 5, 9, True, False)])
    plain = path.read_bytes()
    path.write_bytes(plain[:24] + struct.pack("<I", 3) + plain[28:])
    with pytest.raises(ValueError, match="truncated"):
        read_alignments(path)
    one = (0, [1], [1], [0], [0], [0], [[1 << 4]], None)
    for mapq, sub in (([61], [0]), ([-1], [0]), ([0, 1], [0, 0]), ([0], [0, 0]), ([0], None), (None, [0])):
        with pytest.raises(ValueError):
            write_alignments(path, [AlnBlock(*one, mapq, sub)])


def test_cli_encoder_writes_mapq_blocks(tmp_path):
    """csrc/cli_aln_block.h driven by tests/c/aln_mapq_dump.cpp (the arrays
    repeated here) against write_alignments, byte for byte."""
    a = AlnBlock(0, [1000, 2001, -1], [300, 251, 0], [0, 3, 0], [149, 148, -1], [149, 299, -1],
                 [[150 << 4 | M], [100 << 4 | M, 2 << 4 | I, 47 << 4 | M], []], [1, 0, 0], [60, 17, 0], [0, 208, -5])
    b = AlnBlock(3, [70000], [77], [2], [149], [290], [[5 << 4 | S, 140 << 4 | M, 5 << 4 | S]])
    e = AlnBlock(4, [], [], [], [], [], [], [], [], [])
    c = AlnBlock(4, [-1, -1, -1, -1, 5], [0, 0, 0, 0, 16], [0] * 5, [-1, -1, -1, -1, 7], [-1, -1, -1, -1, 9],
                 [[], [], [], [], [8 << 4 | M]], None, [0, 0, 0, 0, 59], [0, 0, 0, 0, 2 ** 31 - 1])
    exe = str(tmp_path / "aln_mapq_dump")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I",
                    os.path.join(ROOT, "mini_parallel_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c", "aln_mapq_dump.cpp"), "-o", exe], check=True)
    subprocess.run([exe, str(tmp_path / "cli.aln")], check=True)
    write_alignments(tmp_path / "py.aln", [a, b, e, c])
    assert (tmp_path / "cli.aln").read_bytes() == (tmp_path / "py.aln").read_bytes()
    got = read_alignments(tmp_path / "cli.aln")
    assert got.mapq.tolist() == [60, 17, 0, 255, 0, 0, 0, 0, 59]
    assert got.sub_score.tolist() == [0, 208, -5, 0, 0, 0, 0, 0, 2 ** 31 - 1]
    assert got.strand.tolist() == [1, 0, 0, 0, 0, 0, 0, 0, 0]


# ---------------------------------------------------------------------------
# rustseq_mini --mapq / --seed-sep: what the argument parser refuses before
# any device use
# ---------------------------------------------------------------------------
CLI = os.path.join(ROOT, "mini_parallel_amd", "rustseq_mini")
SW = ["--full-wgs", "--gpu", "--score-mode", "sw"]


def run_cli(args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([CLI] + args, capture_output=True, text=True, env=e, timeout=60)


def test_help_lists_the_mapq_flags():
    out = run_cli(["--help"]).stdout
    for flag in ("--mapq", "--seed-sep"):
        assert flag in out


@pytest.mark.parametrize("args,env,word", [
    (SW + ["--mapq"], {}, "--mapq needs --map"),
    (["--mapq", "-1", "ACGT", "-2", "ACGT", "--gpu"], {}, "--mapq needs --map"),
    (["--full-wgs", "--gpu", "--map", "--mapq"], {}, "--full-wgs --score-mode sw"),          # --map's own refusal
    (SW + ["--map", "--mapq"], {"MSW_GPU_INFLATE": "0"}, "host reader"),
    (SW + ["--map", "--seed-sep", "300"], {}, "--seed-sep needs --mapq"),
    (SW + ["--seed-sep", "300"], {}, "--seed-sep needs --mapq"),
    (SW + ["--map", "--mapq", "--seed-sep", "15"], {}, "--seed-sep must be"),                 # below the default band
    (SW + ["--map", "--mapq", "--seed-band", "64", "--seed-sep=63"], {}, "--seed-sep must be"),
    (SW + ["--map", "--mapq", "--seed-sep", "-1"], {}, "--seed-sep must be"),
    (SW + ["--map", "--mapq", "--seed-sep"], {}, "a value is required"),
])
def test_cli_refusals(args, env, word):
    r = run_cli(args, env)
    assert r.returncode == 1 and word in r.stderr and len(r.stderr.strip().splitlines()) == 1, r.stderr
    assert r.stdout == ""
