"""The ``.mpu`` pileup file (mini_parallel_amd.read_pileup / write_pileup,
DESIGN.md 4.14) and what ``rustseq_mini`` refuses of the pileup flags before
any device use."""
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mini_parallel_amd", "rustseq_mini")
SW = ["--full-wgs", "--gpu", "--score-mode", "sw"]
ALN = SW + ["--alignments-out", "out"]


@pytest.mark.parametrize("glen", [0, 1, 300])
def test_round_trip(tmp_path, glen):
    from mini_parallel_amd import read_pileup, write_pileup
    rng = np.random.default_rng(glen)
    counts = rng.integers(0, 2 ** 32, (glen, 8), dtype=np.uint64).astype(np.uint32)
    if glen:
        counts[0] = [0, 1, 2, 3, 4, 5, 6, 0xFFFFFFFF]
    path = tmp_path / "p.mpu"
    write_pileup(path, counts, 2 ** 40 + 7)
    data = open(path, "rb").read()
    assert len(data) == 32 + glen * 32
    # the documented bytes: "MSWPILE1", u32 version 1, u32 channels 8, u64 genome length, u64 reads_used
    assert data[:32] == b"MSWPILE1" + struct.pack("<IIQQ", 1, 8, glen, 2 ** 40 + 7)
    assert data[32:] == counts.astype("<u4").tobytes()
    got, used = read_pileup(path)
    assert got.dtype == np.uint32 and got.shape == (glen, 8) and np.array_equal(got, counts) and used == 2 ** 40 + 7


def test_refused_files(tmp_path):
    from mini_parallel_amd import read_pileup, write_pileup
    good = b"MSWPILE1" + struct.pack("<IIQQ", 1, 8, 2, 5) + bytes(64)
    path = tmp_path / "p.mpu"

    def refused(data, word):
        open(path, "wb").write(data)
        with pytest.raises(ValueError, match=word):
            read_pileup(path)

    open(path, "wb").write(good)
    assert read_pileup(path)[1] == 5
    refused(b"MSWPILE2" + good[8:], "magic")
    refused(b"MSWA" + good[4:], "magic")
    refused(good[:8] + struct.pack("<I", 2) + good[12:], "version")
    refused(good[:12] + struct.pack("<I", 4) + good[16:], "channels")
    refused(good[:-1], "bytes")                 # truncated counts
    refused(good + b"\0", "bytes")              # bytes after the counts
    refused(good[:31], "truncated header")
    refused(b"", "truncated header")
    with pytest.raises(ValueError, match="glen"):
        write_pileup(path, np.zeros((3, 7), np.uint32), 0)
    with pytest.raises(ValueError, match="32 bits"):
        write_pileup(path, np.full((1, 8), 2 ** 32, np.int64), 0)
    with pytest.raises(ValueError, match="32 bits"):
        write_pileup(path, np.full((1, 8), -1, np.int64), 0)


def run_cli(args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([CLI] + args, capture_output=True, text=True, env=e, timeout=60)


def test_help_lists_the_pileup_flags():
    out = run_cli(["--help"]).stdout
    for flag in ("--pileup-out", "--pileup-min-mapq", "--pileup-min-depth"):
        assert flag in out


@pytest.mark.parametrize("args,env,word", [
    (SW + ["--pileup-out", "p.mpu"], {}, "--pileup-out needs --alignments-out"),
    (SW + ["--map", "--mapq", "--pileup-out", "p.mpu"], {}, "--pileup-out needs --alignments-out"),
    (["--pileup-out", "p.mpu", "-1", "ACGT", "-2", "ACGT", "--gpu"], {}, "--pileup-out needs --alignments-out"),
    # --alignments-out's own refusals come first
    (["--full-wgs", "--gpu", "--alignments-out", "out", "--pileup-out", "p.mpu"], {}, "--full-wgs --score-mode sw"),
    (ALN + ["--pileup-out", "p.mpu"], {"MSW_GPU_INFLATE": "0"}, "host reader"),
    (ALN + ["--map", "--mapq", "--pileup-min-mapq", "30"], {}, "--pileup-min-mapq needs --pileup-out and --mapq"),
    (ALN + ["--pileup-out", "p.mpu", "--pileup-min-mapq", "30"], {}, "--pileup-min-mapq needs --pileup-out and --mapq"),
    (ALN + ["--map", "--pileup-out", "p.mpu", "--pileup-min-mapq=0"], {},
     "--pileup-min-mapq needs --pileup-out and --mapq"),
    (ALN + ["--map", "--mapq", "--pileup-out", "p.mpu", "--pileup-min-mapq", "61"], {}, "--pileup-min-mapq must be 0..60"),
    (ALN + ["--map", "--mapq", "--pileup-out", "p.mpu", "--pileup-min-mapq", "-1"], {}, "--pileup-min-mapq must be 0..60"),
    (ALN + ["--pileup-min-depth", "4"], {}, "--pileup-min-depth needs --pileup-out"),
    (ALN + ["--pileup-out", "p.mpu", "--pileup-min-depth", "0"], {}, "--pileup-min-depth must be at least 1"),
    (ALN + ["--pileup-out", "p.mpu", "--pileup-min-depth=-3"], {}, "--pileup-min-depth must be at least 1"),
    (ALN + ["--pileup-out"], {}, "a value is required"),
])
def test_cli_refusals(tmp_path, args, env, word):
    """Refused by the argument parser: one line on stderr, nothing on stdout,
    and no file is opened (neither the pileup nor the output directory)."""
    r = subprocess.run([CLI] + args, capture_output=True, text=True, env=dict(os.environ, **env), timeout=60,
                       cwd=tmp_path)
    assert r.returncode == 1 and word in r.stderr and len(r.stderr.strip().splitlines()) == 1, r.stderr
    assert r.stdout == ""
    assert os.listdir(tmp_path) == []
