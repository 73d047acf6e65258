"""``rustseq_mini --full-wgs ... --variants-out PATH --call-baseq [--qsum-out
PATH]``: the MSWVARQ1 file, the .mqs file and the run record equal
tests/variant_qual_oracle.py and tests/pileup_qsum_oracle.py over the run's own
.aln records and the lane files' quality lines; without the flag the run
writes what it wrote before.

The dataset is test_gpu_variants_cli.py's (its make_reads), with quality
strings of its own: at NOISE positions about a third of the covering reads
carry one wrong base at '#' (Q2), everything else is 'F' (Q37).  The
unweighted caller takes those positions for heterozygous sites; the weighted
one does not, and keeps every planted genotype."""
import json
import os

import numpy as np
import pytest

import pileup_oracle as po
import pileup_qsum_oracle as pqs
import strand_oracle as so
import variant_oracle as vo
import variant_qual_oracle as vq
from test_gpu_mapq_cli import run_cli, wgs_args, wgs_env
from test_gpu_variants_cli import (DEL_AT, FLAGS, GLEN, HET_SNVS, HOM_SNVS, INS_AFTER, PER_FILE, aln_bytes, check_planted,
                                   make_reads, run_id)

gpu = pytest.mark.gpu

NOISE = (500, 1500, 2500, 3700, 4900)              # away from the planted variants
NOISE_SEED = 2                                     # test_noise_is_called_unweighted_and_not_weighted holds for it
ACGT = b"ACGT"


def noisy_reads(seed=NOISE_SEED):
    """make_reads() with the noise put in: -> genome, alt, [(read as given, strand, ref_pos, ops, oriented,
    quality line as given)]"""
    g, alt, reads = make_reads()
    rng = np.random.default_rng(seed)
    wrong = {p: ACGT[(ACGT.index(g[p]) + 2) % 4] for p in NOISE}
    out = []
    for given, strand, at, ops, oriented in reads:
        seq, qual = bytearray(oriented), bytearray(b"F" * len(oriented))
        i, pos = 0, at
        for word in ops:
            ln, kind = int(word) >> 4, int(word) & 15
            if kind == po.OP_M:
                for p in NOISE:
                    if pos <= p < pos + ln and rng.random() < 1 / 3:
                        seq[i + p - pos], qual[i + p - pos] = wrong[p], ord("#")
                i, pos = i + ln, pos + ln
            elif kind == po.OP_I:
                i += ln
            elif kind == po.OP_D:
                pos += ln
        oriented = bytes(seq)
        out.append((so.revcomp(oriented) if strand else oriented, strand, at, ops, oriented,
                    bytes(qual[::-1]) if strand else bytes(qual)))
    return g, alt, out


def exact(g, reads, min_baseq=0):
    return pqs.pileup(g, [r[4] for r in reads], [len(r[4]) for r in reads], [r[2] for r in reads], [0] * len(reads),
                      [r[3] for r in reads], [r[5] for r in reads], [r[1] for r in reads], min_baseq=min_baseq)


def test_noise_is_called_unweighted_and_not_weighted():
    """On the CPU, every read lying exactly where it was drawn: the unweighted
    caller emits a record at each noise position, the weighted one none, and
    the planted calls are the same 14 records either way."""
    g, alt, reads = noisy_reads()
    counts, qsums, used, skipped, lowq = exact(g, reads)
    assert (used, skipped, lowq) == (2 * PER_FILE, 0, 0)
    plain = vo.call(g, counts)
    weighted = vq.call(g, counts, qsums)
    assert sorted(int(p) for p in plain["pos"] if int(p) in NOISE) == list(NOISE)
    assert all(int(r["gt"]) == 1 and int(r["kind"]) == vo.SNV for r in plain if int(r["pos"]) in NOISE)
    assert not [int(p) for p in weighted["pos"] if int(p) in NOISE]
    check_planted(weighted, alt, exact=True)
    check_planted(plain[[int(p) not in NOISE for p in plain["pos"]]], alt, exact=True)
    # with the Q2 bases dropped by a threshold both callers leave the noise out
    counts30, qsums30, _, _, lowq = exact(g, reads, 30)
    assert lowq == int(counts[:, :4].sum() - counts30[:, :4].sum()) > 20
    check_planted(vo.call(g, counts30), alt, exact=True)
    check_planted(vq.call(g, counts30, qsums30), alt, exact=True)


def write_dataset(root):
    from mini_parallel_amd.synthetic import bgzf_compress
    g, alt, reads = noisy_reads()
    os.makedirs(root / "wgs")
    with open(root / "wgs" / "reference.fa", "w") as out:
        s = g.decode()
        out.write(">planted\n" + "\n".join(s[k:k + 80] for k in range(0, len(s), 80)) + "\n")
    names, per_file = [], [reads[:PER_FILE], reads[PER_FILE:]]
    for k, f in enumerate(per_file):
        text = b"".join(b"@SYN:1:%d\n%s\n+\n%s\n" % (i, r[0], r[5]) for i, r in enumerate(f))
        names.append(str(root / "wgs" / ("SYN_L001_R%d_001.fastq.gz" % (k + 1))))
        with open(names[-1], "wb") as out:
            out.write(bgzf_compress(text, 1))
    return {"genome": g, "alt": alt, "reference": str(root / "wgs" / "reference.fa"), "files": names,
            "reads": [[r[0] for r in f] for f in per_file], "quals": [[r[5] for r in f] for f in per_file]}


def cli_run(root, ds, tag, extra=(), ck=None):
    """One run into root/<tag>/ (alignments), root/<tag>.mpu and root/<tag>.var; the stable run id."""
    (root / tag).mkdir(exist_ok=True)
    args = FLAGS + ["--alignments-out", root / tag, "--json", root / (tag + ".json"), "--pileup-out", root / (tag + ".mpu"),
                    "--variants-out", root / (tag + ".var")] + list(extra)
    env = wgs_env(root / "wgs")
    env.update(GPU_CHUNK_SIZE_READS="256", MSW_GFASTQ_BATCH="256")
    return run_cli(wgs_args(root, ds, ck or "ck_" + tag, args), env, root)


@pytest.fixture(scope="module")
def base(tmp_path_factory):
    root = tmp_path_factory.mktemp("call_qual_cli")
    ds = write_dataset(root)
    r = cli_run(root, ds, "w", ["--call-baseq", "--qsum-out", root / "w.mqs"])
    assert r.returncode == 0, r.stdout + r.stderr
    return root, ds, r


def chain(root, ds, tag, min_baseq):
    """The pileup oracle over the run's own records and the lane files' quality lines."""
    from mini_parallel_amd import read_alignments
    counts, qsums = po.new_counts(GLEN), pqs.new_qsums(GLEN)
    used = lowq = 0
    for path, reads, quals in zip(ds["files"], ds["reads"], ds["quals"]):
        x = read_alignments(root / tag / (os.path.basename(path) + ".aln"))
        rows = [so.revcomp(rd) if st else rd for rd, st in zip(reads, x.strand)]
        u, s, low = pqs.add(counts, qsums, rows, [len(rd) for rd in reads], x.ref_pos, x.nm, x.cigars, quals, x.strand,
                            x.mapq, 0, None, min_baseq)
        used, lowq = used + u, lowq + low
    return counts, qsums, used, lowq


def check_weighted(root, ds, tag, min_baseq, stdout):
    from mini_parallel_amd import CallParams, QualParams, read_pileup, read_qsums, read_variants, read_variants_qual
    counts, qsums, used, lowq = chain(root, ds, tag, min_baseq)
    got_counts, file_used = read_pileup(root / (tag + ".mpu"))
    got_qsums, qsum_used = read_qsums(root / (tag + ".mqs"))
    assert np.array_equal(got_counts, counts) and np.array_equal(got_qsums, qsums)
    assert file_used == qsum_used == used > 1100 and qsums.any()
    want = vq.call(ds["genome"], counts, qsums)
    data = open(root / (tag + ".var"), "rb").read()
    assert data[:8] == b"MSWVARQ1" and len(data) == 88 + 48 * len(want)
    got, glen, params, qparams = read_variants_qual(root / (tag + ".var"))
    assert glen == GLEN and params == CallParams() and qparams == QualParams()
    assert got.to_records().tobytes() == want.tobytes(), (len(got.pos), len(want))
    with pytest.raises(ValueError):
        read_variants(root / (tag + ".var"))
    rec = json.load(open(root / (tag + ".json")))["variants"]
    assert rec.pop("variants_ms") > 0
    kinds, gts = [int(k) for k in want["kind"]], [int(k) for k in want["gt"]]
    expect = dict(path=str(root / (tag + ".var")), min_mapq=0, params=vo.params(), records=len(want),
                  snv=kinds.count(vo.SNV), **{"del": kinds.count(vo.DEL)}, ins=kinds.count(vo.INS), het=gts.count(1),
                  hom=gts.count(2), baseq_weighted=True, q_scale=100, q_third=477)
    if min_baseq:
        expect.update(min_baseq=min_baseq, lowq_columns=lowq)
    assert rec == expect
    assert ("Variants: %d records" % len(want)) in stdout
    return want, counts


@gpu
def test_weighted_var_mqs_and_record_equal_the_oracles(base):
    root, ds, r = base
    want, counts = check_weighted(root, ds, "w", 0, r.stdout)
    check_planted(want, ds["alt"])
    # the noise: taken for variants by the unweighted caller over the same counts, left out by the weighted run
    # (most of them: a mapped read may clip a wrong base near its end, which exact alignments keep)
    plain = vo.call(ds["genome"], counts)
    assert len(set(NOISE) & set(int(p) for p in plain["pos"][plain["kind"] == vo.SNV])) >= 3
    assert not set(NOISE) & set(int(p) for p in want["pos"])


@gpu
def test_with_a_threshold_of_30(base):
    root, ds, _ = base
    r = cli_run(root, ds, "w30", ["--call-baseq", "--qsum-out", root / "w30.mqs", "--pileup-min-baseq", 30])
    assert r.returncode == 0, r.stdout + r.stderr
    want, counts = check_weighted(root, ds, "w30", 30, r.stdout)
    check_planted(want, ds["alt"])
    assert json.load(open(root / "w30.json"))["variants"]["lowq_columns"] > 20
    assert aln_bytes(root, ds, "w30") == aln_bytes(root, ds, "w")
    assert run_id(root, "w30") != run_id(root, "w")


@gpu
def test_without_the_flag_the_run_is_the_unweighted_one(base):
    from mini_parallel_amd import read_pileup, read_variants
    root, ds, _ = base
    outs = []
    for tag in ("p1", "p2"):
        r = cli_run(root, ds, tag)
        assert r.returncode == 0, r.stdout + r.stderr
        rec = json.load(open(root / (tag + ".json")))
        assert not {"baseq_weighted", "q_scale", "q_third", "min_baseq"} & set(rec["variants"])
        outs.append(aln_bytes(root, ds, tag) + [open(root / (tag + ext), "rb").read() for ext in (".mpu", ".var")])
        assert not (root / (tag + ".mqs")).exists()
    assert outs[0] == outs[1]
    # the records and the counts do not depend on the flag; the calls are MSWVARS1 ones over the same counts
    assert aln_bytes(root, ds, "p1") == aln_bytes(root, ds, "w")
    assert open(root / "p1.mpu", "rb").read() == open(root / "w.mpu", "rb").read()
    got, glen, params = read_variants(root / "p1.var")
    assert got.to_records().tobytes() == vo.call(ds["genome"], read_pileup(root / "p1.mpu")[0]).tobytes()
    assert open(root / "p1.var", "rb").read()[:8] == b"MSWVARS1"
    assert run_id(root, "p1") == run_id(root, "p2") != run_id(root, "w")


@gpu
def test_resume_across_the_flag(base):
    root, ds, _ = base
    # a checkpoint directory of this test's own
    r = cli_run(root, ds, "r", ["--call-baseq"])
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(root / "r.var", "rb").read() == open(root / "w.var", "rb").read() and not (root / "r.mqs").exists()
    # over its own checkpoint, which lists completed files, the weighted run is refused like any run with a pileup
    before = open(root / "r.var", "rb").read()
    r = cli_run(root, ds, "r", ["--call-baseq"])
    assert r.returncode == 1 and "remove the checkpoint" in r.stderr, r.stderr
    assert open(root / "r.var", "rb").read() == before
    # an unweighted run beside that checkpoint is another run: it resumes nothing and lists its own files
    r = cli_run(root, ds, "x", ck="ck_r")
    assert r.returncode == 0 and "Resuming" not in r.stdout, r.stdout + r.stderr
    cks = sorted(f for f in os.listdir(root / "ck_r") if f.startswith("checkpoint_wgs_"))
    assert len(cks) == 2
    assert open(root / "x.var", "rb").read()[:8] == b"MSWVARS1"
    # and the weighted run is refused over its own still
    r = cli_run(root, ds, "r", ["--call-baseq"])
    assert r.returncode == 1 and "remove the checkpoint" in r.stderr, r.stderr
