"""The ``.mqs`` file of quality sums and the quality-weighted ``.var``
(``MSWVARQ1``) of mini_parallel_amd.alnfile: the documented bytes, round trips,
every refused file, and the CLI refusals of ``--call-baseq`` / ``--qsum-out``
that need no GPU."""
import os
import struct
import subprocess

import numpy as np
import pytest

from test_variant_format import ALN, CLI, DEFAULTS, ROWS, SW, variants


@pytest.mark.parametrize("glen", [0, 1, 300])
def test_qsums_round_trip(tmp_path, glen):
    from mini_parallel_amd import read_qsums, write_qsums
    rng = np.random.default_rng(glen)
    q = rng.integers(0, 2 ** 32, (glen, 4), dtype=np.uint64).astype(np.uint32)
    path = tmp_path / "q.mqs"
    write_qsums(path, q, 2 ** 40 + 5)
    data = open(path, "rb").read()
    assert len(data) == 32 + 16 * glen
    assert data[:32] == b"MSWQSUM1" + struct.pack("<IIQQ", 1, 4, glen, 2 ** 40 + 5)
    assert data[32:] == q.astype("<u4").tobytes()
    got, used = read_qsums(path)
    assert used == 2 ** 40 + 5 and got.dtype == np.uint32 and got.shape == (glen, 4) and np.array_equal(got, q)


def test_qsums_refused(tmp_path):
    from mini_parallel_amd import read_pileup, read_qsums, write_pileup, write_qsums
    path = tmp_path / "q.mqs"
    for bad in (np.zeros((3, 8), np.uint32), np.zeros(4, np.uint32), np.full((2, 4), -1), np.full((2, 4), 2 ** 32)):
        with pytest.raises(ValueError):
            write_qsums(path, bad, 0)
    write_qsums(path, np.arange(40, dtype=np.uint32).reshape(10, 4), 7)
    good = open(path, "rb").read()

    def refused(data, word):
        open(path, "wb").write(data)
        with pytest.raises(ValueError) as e:
            read_qsums(path)
        assert word in str(e.value), str(e.value)

    refused(b"MSWPILE1" + good[8:], "magic")
    refused(good[:8] + struct.pack("<I", 2) + good[12:], "version")
    refused(good[:12] + struct.pack("<I", 8) + good[16:], "channels")
    refused(good[:-1], "bytes")
    refused(good + b"\0", "bytes")
    refused(good[:16] + struct.pack("<Q", 11) + good[24:], "bytes")
    refused(good[:31], "truncated")
    refused(b"", "truncated")
    # the two dense files do not read each other
    open(path, "wb").write(good)
    with pytest.raises(ValueError):
        read_pileup(path)
    write_pileup(path, np.zeros((10, 8), np.uint32), 7)
    with pytest.raises(ValueError):
        read_qsums(path)


@pytest.mark.parametrize("n", [0, 1, 7])
def test_weighted_var_round_trip(tmp_path, n):
    from mini_parallel_amd import CallParams, QualParams, read_variants_qual, write_variants
    v = variants(ROWS[:n])
    params = CallParams(min_depth=3, min_alt=1, min_alt_permille=1000, min_qual=2 ** 32 - 1, q_hit=1, q_miss=65535,
                        q_het=7, prior_het=0, prior_hom=2 ** 32 - 1)
    path = tmp_path / "v.var"
    write_variants(path, v, 2 ** 40, params, QualParams(65535, 1))
    data = open(path, "rb").read()
    assert len(data) == 88 + 48 * n
    # the 72 bytes of MSWVARS1 under another magic, then q_scale, q_third and two zero words
    assert data[:88] == b"MSWVARQ1" + struct.pack("<IIQQ9II4I", 1, 48, 2 ** 40, n, 3, 1, 1000, 2 ** 32 - 1, 1, 65535, 7, 0,
                                                  2 ** 32 - 1, 0, 65535, 1, 0, 0)
    plain = tmp_path / "p.var"
    write_variants(plain, v, 2 ** 40, params)
    assert data[88:] == open(plain, "rb").read()[72:]
    got, glen, p, q = read_variants_qual(path)
    assert glen == 2 ** 40 and p == params and q == QualParams(65535, 1)
    for a, b in zip(got, v):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    # the defaults
    write_variants(path, v, 10, qual_params=QualParams())
    assert read_variants_qual(path)[2:] == (CallParams(), QualParams())
    assert open(path, "rb").read()[32:88] == struct.pack("<9II4I", *DEFAULTS, 0, 100, 477, 0, 0)


def test_weighted_var_refused(tmp_path):
    from mini_parallel_amd import QualParams, read_variants, read_variants_qual, write_variants
    path = tmp_path / "v.var"
    write_variants(path, variants(ROWS), 10, qual_params=QualParams())
    good = open(path, "rb").read()
    assert len(good) == 88 + 48 * len(ROWS)
    # read_variants goes on refusing anything but MSWVARS1
    with pytest.raises(ValueError) as e:
        read_variants(path)
    assert "magic" in str(e.value)

    def refused(data, word):
        open(path, "wb").write(data)
        with pytest.raises(ValueError) as e:
            read_variants_qual(path)
        assert word in str(e.value), str(e.value)

    refused(b"MSWVARS1" + good[8:], "magic")
    refused(good[:8] + struct.pack("<I", 2) + good[12:], "version")
    refused(good[:12] + struct.pack("<I", 40) + good[16:], "record size")
    refused(good[:68] + struct.pack("<I", 1) + good[72:], "reserved")
    refused(good[:80] + struct.pack("<I", 1) + good[84:], "reserved")
    refused(good[:84] + struct.pack("<I", 1) + good[88:], "reserved")
    refused(good[:-1], "bytes")
    refused(good + b"\0", "bytes")
    refused(good[:24] + struct.pack("<Q", len(ROWS) + 1) + good[32:], "bytes")
    refused(good[:87], "truncated")
    # the records' own checks: order, genome length, padding
    refused(good[:88] + good[88 + 48:88 + 96] + good[88:88 + 48] + good[88 + 96:], "ordered")
    refused(good[:16] + struct.pack("<Q", 8) + good[24:], "past the genome")
    refused(good[:88 + 47] + b"\1" + good[88 + 48:], "padding")
    # an MSWVARS1 file is not a weighted one
    write_variants(path, variants(ROWS), 10)
    with pytest.raises(ValueError):
        read_variants_qual(path)


def test_qual_params():
    from mini_parallel_amd import MswError, QualParams
    q = QualParams()
    assert (q.q_scale, q.q_third) == (100, 477) and QualParams.FIELDS == ("q_scale", "q_third")
    c = QualParams(7, 9).to_c()
    assert (c.q_scale, c.q_third) == (7, 9)
    for bad in (QualParams(-1, 0), QualParams(0, 2 ** 32)):
        with pytest.raises(MswError):
            bad.to_c()


def test_help_lists_the_flags():
    out = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "--call-baseq" in out and "--qsum-out" in out


@pytest.mark.parametrize("args,env,word", [
    (ALN + ["--call-baseq"], {}, "--call-baseq needs --variants-out"),
    (ALN + ["--pileup-out", "p.mpu", "--call-baseq"], {}, "--call-baseq needs --variants-out"),
    (ALN + ["--variants-out", "v.var", "--qsum-out", "q.mqs"], {}, "--qsum-out needs --call-baseq"),
    (ALN + ["--qsum-out", "q.mqs"], {}, "--qsum-out needs --call-baseq"),
    (ALN + ["--call-baseq", "--qsum-out", "q.mqs"], {}, "--call-baseq needs --variants-out"),
    (ALN + ["--variants-out", "v.var", "--call-baseq", "--qsum-out"], {}, "a value is required"),
    # the refusals in front of it come first, as for --pileup-min-baseq
    (SW + ["--variants-out", "v.var", "--call-baseq"], {}, "--variants-out needs --alignments-out"),
    (ALN + ["--variants-out", "v.var", "--call-baseq"], {"MSW_GPU_INFLATE": "0"}, "host reader"),
    (ALN + ["--variants-out", "v.var", "--call-baseq", "--pileup-min-baseq", "94"], {}, "--pileup-min-baseq must be 0..93"),
    (["--call-baseq", "-1", "ACGT", "-2", "ACGT", "--gpu"], {}, "--call-baseq needs --variants-out"),
])
def test_cli_refusals(tmp_path, args, env, word):
    """Refused by the argument parser: one line on stderr, nothing on stdout,
    and no file is opened."""
    r = subprocess.run([CLI] + args, capture_output=True, text=True, env=dict(os.environ, **env), timeout=60,
                       cwd=tmp_path)
    assert r.returncode == 1 and word in r.stderr and len(r.stderr.strip().splitlines()) == 1, r.stderr
    assert r.stdout == ""
    assert os.listdir(tmp_path) == []
