"""The ``.var`` file (mini_parallel_amd.read_variants / write_variants, DESIGN.md
4.15), the VCF text of ``write_vcf``, and what ``rustseq_mini`` refuses of the
variant flags before any device use."""
import os
import struct
import subprocess

import numpy as np
import pytest

import variant_oracle as vo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mini_parallel_amd", "rustseq_mini")
SW = ["--full-wgs", "--gpu", "--score-mode", "sw"]
ALN = SW + ["--alignments-out", "out"]
DEFAULTS = (4, 2, 200, 20, 4, 2477, 304, 3000, 3301)


def variants(rows):
    """rows: (pos, kind, ref, alt, gt, gq, qual, depth, ref_count, alt_count, pl)"""
    from mini_parallel_amd import Variants
    cols = list(zip(*rows)) if rows else [[]] * 11
    dt = (np.uint64, np.uint8, np.uint8, np.uint8, np.uint8, np.uint8, np.uint32, np.uint32, np.uint32, np.uint32)
    return Variants(*[np.array(c, d) for c, d in zip(cols[:10], dt)], np.array(cols[10], np.uint32).reshape(-1, 3))


HET = (1, 99, 157, 20, 10, 10, (187, 0, 187))
HOM = (2, 57, 462, 20, 0, 20, (495, 60, 0))
#          ACGTACGTAC
GENOME = b"ACGTACGTAC"
ROWS = [(0, vo.DEL, ord("A"), 0) + HOM, (1, vo.DEL, ord("C"), 0) + HOM,          # a deletion at position 0
        (3, vo.SNV, ord("T"), ord("C")) + HET,
        (4, vo.INS, ord("A"), 0) + HOM,
        (6, vo.DEL, ord("G"), 0) + HET, (7, vo.DEL, ord("T"), 0) + (1, 40, 90, 18, 9, 9, (100, 0, 100)),
        (8, vo.DEL, ord("A"), 0) + HET]                                           # a run of three


def test_record_layout_matches_the_oracle_and_the_header():
    from mini_parallel_amd.aligner import VARIANT_DTYPE
    assert VARIANT_DTYPE == vo.RECORD and VARIANT_DTYPE.itemsize == 48
    assert [VARIANT_DTYPE.fields[k][1] for k in ("pos", "depth", "ref_count", "alt_count", "qual", "pl", "kind", "ref",
                                                 "alt", "gt", "gq", "pad")] == [0, 8, 12, 16, 20, 24, 36, 37, 38, 39, 40, 41]


@pytest.mark.parametrize("n", [0, 1, 7])
def test_round_trip(tmp_path, n):
    from mini_parallel_amd import CallParams, read_variants, write_variants
    v = variants(ROWS[:n])
    params = CallParams(min_depth=3, min_alt=1, min_alt_permille=1000, min_qual=2 ** 32 - 1, q_hit=1, q_miss=65535,
                        q_het=7, prior_het=0, prior_hom=2 ** 32 - 1)
    path = tmp_path / "v.var"
    write_variants(path, v, 2 ** 40, params)
    data = open(path, "rb").read()
    assert len(data) == 72 + 48 * n
    # the documented bytes: "MSWVARS1", version 1, record size 48, genome length, record count, nine parameters, zero
    assert data[:72] == b"MSWVARS1" + struct.pack("<IIQQ9II", 1, 48, 2 ** 40, n, 3, 1, 1000, 2 ** 32 - 1, 1, 65535, 7, 0,
                                                  2 ** 32 - 1, 0)
    if n:
        assert data[72:120] == struct.pack("<QIIII3I5B7x", 0, 20, 0, 20, 462, 495, 60, 0, vo.DEL, ord("A"), 0, 2, 57)
    got, glen, p = read_variants(path)
    assert glen == 2 ** 40 and p == params
    for a, b in zip(got, v):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    # the defaults
    write_variants(path, v, 10)
    assert read_variants(path)[2] == CallParams() and open(path, "rb").read()[32:72] == struct.pack("<9II", *DEFAULTS, 0)


def test_refused_files(tmp_path):
    from mini_parallel_amd import read_variants, write_variants
    path = tmp_path / "v.var"
    write_variants(path, variants(ROWS), 10)
    good = open(path, "rb").read()
    assert len(read_variants(path)[0].pos) == 7

    def refused(data, word):
        open(path, "wb").write(data)
        with pytest.raises(ValueError, match=word):
            read_variants(path)

    def rec(k, field_off, byte):
        at = 72 + 48 * k + field_off
        return good[:at] + bytes([byte]) + good[at + 1:]

    refused(b"MSWVARS2" + good[8:], "magic")
    refused(b"MSWPILE1" + good[8:], "magic")
    refused(good[:8] + struct.pack("<I", 2) + good[12:], "version")
    refused(good[:12] + struct.pack("<I", 40) + good[16:], "record size")
    refused(good[:68] + struct.pack("<I", 1) + good[72:], "reserved")
    refused(good[:-1], "bytes")                              # truncated records
    refused(good + b"\0", "bytes")                           # bytes after the records
    refused(good[:24] + struct.pack("<Q", 8) + good[32:], "bytes")     # a record count that is not the file's
    refused(good[:71], "truncated header")
    refused(b"", "truncated header")
    refused(good[:16] + struct.pack("<Q", 8) + good[24:], "past the genome")
    refused(rec(2, 36, 3), "kind")
    refused(rec(2, 39, 0), "genotype")
    refused(rec(2, 39, 3), "genotype")
    refused(rec(2, 47, 1), "padding")
    refused(rec(1, 0, 0), "ordered")                         # two column records at position 0
    refused(rec(3, 0, 2), "ordered")                         # pos 3, then pos 2
    assert good != rec(3, 0, 3)
    open(path, "wb").write(rec(3, 0, 3))                     # the insertion of position 3 behind its SNV: in order
    assert [int(k) for k in read_variants(path)[0].pos[2:4]] == [3, 3]
    # the writer refuses the same records
    bad = variants([ROWS[2], ROWS[0]])
    with pytest.raises(ValueError, match="ordered"):
        write_variants(path, bad, 10)
    with pytest.raises(ValueError, match="past the genome"):
        write_variants(path, variants(ROWS), 8)


VCF = """##fileformat=VCFv4.2
##contig=<ID=chr9,length=10>
##ALT=<ID=INS,Description="Insertion after this base; the sequence is not known">
##ALT=<ID=DEL,Description="Deletion">
##INFO=<ID=DP,Number=1,Type=Integer,Description="Observations at the site">
##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">
##FORMAT=<ID=AD,Number=R,Type=Integer,Description="Observations of the reference and the alternative">
##FORMAT=<ID=GQ,Number=1,Type=Integer,Description="Genotype quality">
##FORMAT=<ID=PL,Number=G,Type=Integer,Description="Genotype costs, -10 log10 of the likelihood">
#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tNA1
chr9\t1\t.\tACG\tG\t462\t.\tDP=20\tGT:AD:GQ:PL\t1/1:0,20:57:495,60,0
chr9\t4\t.\tT\tC\t157\t.\tDP=20\tGT:AD:GQ:PL\t0/1:10,10:99:187,0,187
chr9\t5\t.\tA\t<INS>\t462\t.\tDP=20\tGT:AD:GQ:PL\t1/1:0,20:57:495,60,0
chr9\t6\t.\tCGTA\tC\t157\t.\tDP=20\tGT:AD:GQ:PL\t0/1:10,10:99:187,0,187
"""


def test_write_vcf(tmp_path):
    """An SNV, a deletion at position 0 (anchored at the base after it), an
    insertion, a run of three deleted bases (anchored at the base before, the
    first record's numbers); a het and a hom genotype."""
    from mini_parallel_amd import write_vcf
    path = tmp_path / "v.vcf"
    write_vcf(path, variants(ROWS), GENOME, contig="chr9", sample="NA1")
    assert open(path).read() == VCF
    # the defaults of contig and sample, a genome given as an array, no records
    write_vcf(path, variants([]), np.frombuffer(GENOME, np.uint8))
    text = open(path).read().splitlines()
    assert text[1] == "##contig=<ID=ref,length=10>" and text[-1].endswith("FORMAT\tsample") and len(text) == 10


def test_write_vcf_runs_end_at_a_gap_and_at_another_genotype(tmp_path):
    from mini_parallel_amd import write_vcf
    rows = [(2, vo.DEL, ord("G"), 0) + HET, (3, vo.DEL, ord("T"), 0) + HOM,      # another genotype: two deletions
            (5, vo.DEL, ord("C"), 0) + HET, (5, vo.INS, ord("C"), 0) + HET,      # an insertion inside a run
            (6, vo.DEL, ord("G"), 0) + HET,
            (8, vo.DEL, ord("A"), 0) + HET]                                      # a gap: a run of its own
    path = tmp_path / "v.vcf"
    write_vcf(path, variants(rows), GENOME)
    body = [ln.split("\t") for ln in open(path).read().splitlines() if not ln.startswith("#")]
    assert [(b[1], b[3], b[4], b[9].split(":")[0]) for b in body] == [
        ("2", "CG", "C", "0/1"), ("3", "GT", "G", "1/1"), ("5", "ACG", "A", "0/1"), ("6", "C", "<INS>", "0/1"),
        ("8", "TA", "T", "0/1")]


def test_help_lists_the_variant_flags():
    out = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60).stdout
    for flag in ("--variants-out", "--call-min-depth", "--call-min-alt", "--call-min-alt-permille", "--call-min-qual"):
        assert flag in out


@pytest.mark.parametrize("args,env,word", [
    (SW + ["--variants-out", "v.var"], {}, "--variants-out needs --alignments-out"),
    (SW + ["--map", "--mapq", "--variants-out", "v.var"], {}, "--variants-out needs --alignments-out"),
    (["--variants-out", "v.var", "-1", "ACGT", "-2", "ACGT", "--gpu"], {}, "--variants-out needs --alignments-out"),
    # --alignments-out's own refusals come first, as for --pileup-out
    (["--full-wgs", "--gpu", "--alignments-out", "out", "--variants-out", "v.var"], {}, "--full-wgs --score-mode sw"),
    (ALN + ["--variants-out", "v.var"], {"MSW_GPU_INFLATE": "0"}, "host reader"),
    (ALN + ["--variants-out", "v.var", "--pileup-min-mapq", "30"], {}, "--pileup-min-mapq needs --pileup-out and --mapq"),
    (ALN + ["--map", "--mapq", "--variants-out", "v.var", "--pileup-min-mapq", "61"], {}, "--pileup-min-mapq must be 0..60"),
    (ALN + ["--call-min-depth", "4"], {}, "thresholds need --variants-out"),
    (ALN + ["--pileup-out", "p.mpu", "--call-min-qual", "4"], {}, "thresholds need --variants-out"),
    (ALN + ["--call-min-alt=1"], {}, "thresholds need --variants-out"),
    (ALN + ["--call-min-alt-permille", "1"], {}, "thresholds need --variants-out"),
    (ALN + ["--variants-out", "v.var", "--call-min-depth", "0"], {}, "--call-min-depth must be 1..4294967295"),
    (ALN + ["--variants-out", "v.var", "--call-min-alt", "-1"], {}, "--call-min-alt must be 0..4294967295"),
    (ALN + ["--variants-out", "v.var", "--call-min-alt-permille", "1001"], {}, "--call-min-alt-permille must be 0..1000"),
    (ALN + ["--variants-out", "v.var", "--call-min-alt-permille=-1"], {}, "--call-min-alt-permille must be 0..1000"),
    (ALN + ["--variants-out", "v.var", "--call-min-qual", "-2"], {}, "--call-min-qual must be 0..4294967295"),
    (ALN + ["--variants-out", "v.var", "--call-min-qual", "4294967296"], {}, "--call-min-qual must be 0..4294967295"),
    (ALN + ["--variants-out"], {}, "a value is required"),
])
def test_cli_refusals(tmp_path, args, env, word):
    """Refused by the argument parser: one line on stderr, nothing on stdout,
    and no file is opened."""
    r = subprocess.run([CLI] + args, capture_output=True, text=True, env=dict(os.environ, **env), timeout=60,
                       cwd=tmp_path)
    assert r.returncode == 1 and word in r.stderr and len(r.stderr.strip().splitlines()) == 1, r.stderr
    assert r.stdout == ""
    assert os.listdir(tmp_path) == []
