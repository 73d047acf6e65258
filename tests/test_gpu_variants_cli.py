"""``rustseq_mini --full-wgs ... --alignments-out DIR --variants-out PATH``: the
.var file and the run record equal tests/variant_oracle.py's calls over the
run's own pileup, the planted variants of a dataset made here are found, and
without the flag the run writes what it wrote before."""
import json
import os

import numpy as np
import pytest

import pileup_oracle as po
import strand_oracle as so
import variant_oracle as vo
from test_gpu_mapq_cli import run_cli, wgs_args, wgs_env

gpu = pytest.mark.gpu

FLAGS = ["--mapq", "--both-strands"]
GLEN, READ_LEN, PER_FILE = 6000, 100, 600          # 2 x 600 reads of 100 bases: 20 x depth
HOM_SNVS = (700, 1900, 3100, 4300, 5500)           # on both haplotypes
HET_SNVS = (1000, 2200, 3400, 4600, 5200)          # on one of the two
DEL_AT, DEL_LEN = 2800, 3                          # both haplotypes
INS_AFTER, INS_SEQ = 4000, b"GT"                   # both haplotypes, behind this base
SEED = 2039                                        # test_exact_alignments_give_the_planted_calls holds for it
ACGT = b"ACGT"


def make_reads(seed=SEED):
    """A random genome and reads drawn from a mutated copy of it, each with its
    exact alignment: -> genome, [(read bytes as given, strand, ref_pos, ops, oriented bytes)]."""
    rng = np.random.default_rng(seed)
    g = bytes(ACGT[k] for k in rng.integers(0, 4, GLEN))
    alt = {p: ACGT[(ACGT.index(g[p]) + 1 + int(rng.integers(0, 3))) % 4] for p in HOM_SNVS + HET_SNVS}
    reads = []
    for k in range(2 * PER_FILE):
        hap = int(rng.integers(0, 2))
        at = int(rng.integers(0, GLEN - READ_LEN - 8))
        while DEL_AT <= at < DEL_AT + DEL_LEN:       # a read does not start on a deleted base
            at += 1
        seq, ops, pos = bytearray(), [], at
        while len(seq) < READ_LEN:
            if DEL_AT <= pos < DEL_AT + DEL_LEN:
                ops.append(po.OP_D)
                pos += 1
                continue
            seq.append(alt[pos] if pos in alt and (pos in HOM_SNVS or hap) else g[pos])
            ops.append(po.OP_M)
            if pos == INS_AFTER:
                if len(seq) + len(INS_SEQ) >= READ_LEN:
                    break                            # no room for the insertion: the read ends in front of it
                seq += INS_SEQ
                ops += [po.OP_I] * len(INS_SEQ)
            pos += 1
        runs = []
        for o in ops:
            if runs and runs[-1][1] == o:
                runs[-1][0] += 1
            else:
                runs.append([1, o])
        strand = k % 2
        oriented = bytes(seq)
        reads.append((so.revcomp(oriented) if strand else oriented, strand, at,
                      np.array([po.op(n, o) for n, o in runs], np.uint32), oriented))
    return g, alt, reads


def exact_counts(g, reads):
    counts = po.new_counts(len(g))
    po.add(counts, [r[4] for r in reads], [len(r[4]) for r in reads], [r[2] for r in reads], [0] * len(reads),
           [r[3] for r in reads], [r[1] for r in reads])
    return counts


def check_planted(rec, alt, exact=False):
    """The planted SNVs are in `rec` at their coordinates with their genotypes,
    and the indels are found within the few bases an aligner may shift a gap.
    exact: nothing else is called."""
    by_pos = {}
    for r in rec:
        by_pos.setdefault(int(r["pos"]), []).append(r)
    for p in HOM_SNVS + HET_SNVS:
        col = [r for r in by_pos.get(p, []) if int(r["kind"]) != vo.INS]
        assert len(col) == 1, p
        assert (int(col[0]["kind"]), int(col[0]["alt"]), int(col[0]["gt"])) == (vo.SNV, alt[p], 2 if p in HOM_SNVS else 1), p
    dels = [int(r["pos"]) for r in rec if int(r["kind"]) == vo.DEL and int(r["gt"]) == 2]
    ins = [int(r["pos"]) for r in rec if int(r["kind"]) == vo.INS and int(r["gt"]) == 2]
    assert any(abs(p - DEL_AT) <= 3 for p in dels) and any(abs(p - INS_AFTER) <= 3 for p in ins)
    if exact:
        assert sorted(int(r["pos"]) for r in rec if int(r["kind"]) == vo.SNV) == sorted(HOM_SNVS + HET_SNVS)
        assert dels == [DEL_AT, DEL_AT + 1, DEL_AT + 2] and ins == [INS_AFTER] and len(rec) == 14


def test_exact_alignments_give_the_planted_calls():
    """On the CPU: the chosen seed and depth give the planted genotypes when
    every read lies exactly where it was drawn."""
    g, alt, reads = make_reads()
    rec = vo.call(g, exact_counts(g, reads))
    check_planted(rec, alt, exact=True)


def write_dataset(root):
    from mini_parallel_amd.synthetic import bgzf_compress
    g, alt, reads = make_reads()
    os.makedirs(root / "wgs")
    with open(root / "wgs" / "reference.fa", "w") as out:
        s = g.decode()
        out.write(">planted\n" + "\n".join(s[k:k + 80] for k in range(0, len(s), 80)) + "\n")
    names, per_file = [], [reads[:PER_FILE], reads[PER_FILE:]]
    for k, f in enumerate(per_file):
        text = b"".join(b"@SYN:1:%d\n%s\n+\n%s\n" % (i, r[0], b"I" * len(r[0])) for i, r in enumerate(f))
        names.append(str(root / "wgs" / ("SYN_L001_R%d_001.fastq.gz" % (k + 1))))
        with open(names[-1], "wb") as out:
            out.write(bgzf_compress(text, 1))
    return {"genome": g, "alt": alt, "reference": str(root / "wgs" / "reference.fa"), "files": names,
            "reads": [[r[0] for r in f] for f in per_file]}


def variants_run(root, ds, tag, extra=(), variants=True, pileup=True):
    """One run into root/<tag>/ (alignments), root/<tag>.mpu and root/<tag>.var;
    its own checkpoint directory, the stable run id."""
    (root / tag).mkdir()
    args = FLAGS + ["--alignments-out", root / tag, "--json", root / (tag + ".json")] + list(extra)
    if pileup:
        args += ["--pileup-out", root / (tag + ".mpu")]
    if variants:
        args += ["--variants-out", root / (tag + ".var")]
    env = wgs_env(root / "wgs")
    env.update(GPU_CHUNK_SIZE_READS="256", MSW_GFASTQ_BATCH="256")
    return run_cli(wgs_args(root, ds, "ck_" + tag, args), env, root)


def aln_bytes(root, ds, tag):
    return [open(root / tag / (os.path.basename(p) + ".aln"), "rb").read() for p in ds["files"]]


def run_id(root, tag):
    cks = [f for f in os.listdir(root / ("ck_" + tag)) if f.startswith("checkpoint_wgs_")]
    assert len(cks) == 1
    return json.load(open(root / ("ck_" + tag) / cks[0]))["run_id"]


@pytest.fixture(scope="module")
def base(tmp_path_factory):
    root = tmp_path_factory.mktemp("variants_cli")
    ds = write_dataset(root)
    r = variants_run(root, ds, "a")
    assert r.returncode == 0, r.stdout + r.stderr
    return root, ds, r


def check_var(root, ds, tag, counts, stdout, over=None, min_mapq=0):
    """The .var file and the run record against the oracle over `counts`."""
    from mini_parallel_amd import CallParams, read_variants
    p = vo.params(**(over or {}))
    want = vo.call(ds["genome"], counts, p)
    got, glen, params = read_variants(root / (tag + ".var"))
    assert glen == GLEN and params == CallParams(**p)
    assert got.to_records().tobytes() == want.tobytes(), (len(got.pos), len(want))
    rec = json.load(open(root / (tag + ".json")))["variants"]
    assert rec.pop("variants_ms") > 0
    kinds, gts = [int(k) for k in want["kind"]], [int(k) for k in want["gt"]]
    assert rec == dict(path=str(root / (tag + ".var")), min_mapq=min_mapq, params=p, records=len(want),
                       snv=kinds.count(vo.SNV), **{"del": kinds.count(vo.DEL)}, ins=kinds.count(vo.INS),
                       het=gts.count(1), hom=gts.count(2))
    assert ("Variants: %d records (%d SNV, %d DEL, %d INS; %d 0/1, %d 1/1)" % (
        len(want), rec["snv"], rec["del"], rec["ins"], rec["het"], rec["hom"])) in stdout
    return want


@gpu
def test_var_file_and_record_equal_the_oracle_over_the_runs_pileup(base):
    from mini_parallel_amd import read_alignments, read_pileup
    root, ds, r = base
    counts, used = read_pileup(root / "a.mpu")
    assert used > 1100
    want = check_var(root, ds, "a", counts, r.stdout)
    # every planted SNV at its coordinate with its genotype, and no other
    check_planted(want, ds["alt"])
    # the indels where the chain of oracles puts them: the pileup oracle over the run's own records, then the caller
    chain = po.new_counts(GLEN)
    for path, reads in zip(ds["files"], ds["reads"]):
        x = read_alignments(root / "a" / (os.path.basename(path) + ".aln"))
        rows = [so.revcomp(rd) if st else rd for rd, st in zip(reads, x.strand)]
        po.add(chain, rows, [len(rd) for rd in reads], x.ref_pos, x.nm, x.cigars, x.strand, x.mapq, 0)
    expect = vo.call(ds["genome"], chain)
    assert want.tobytes() == expect.tobytes()
    for kind in (vo.DEL, vo.INS):
        assert [int(p) for p in want["pos"][want["kind"] == kind]] == [int(p) for p in expect["pos"][expect["kind"] == kind]]
    # teardown, the pileup's phase and the calls' phase are told apart
    rec = json.load(open(root / "a.json"))
    assert rec["pileup"]["pileup_ms"] > 0 and rec["teardown_ms"] >= 0


@gpu
def test_thresholds_and_min_mapq(base):
    from mini_parallel_amd import read_pileup
    root, ds, _ = base
    extra = ["--call-min-depth", 2, "--call-min-alt", 1, "--call-min-alt-permille", 100, "--call-min-qual", 30,
             "--pileup-min-mapq", 30]
    r = variants_run(root, ds, "t", extra)
    assert r.returncode == 0, r.stdout + r.stderr
    counts, _ = read_pileup(root / "t.mpu")
    check_var(root, ds, "t", counts, r.stdout, dict(min_depth=2, min_alt=1, min_alt_permille=100, min_qual=30), 30)
    assert aln_bytes(root, ds, "t") == aln_bytes(root, ds, "a")
    assert run_id(root, "t") != run_id(root, "a")


@gpu
def test_without_the_flag_the_run_is_what_it_was(base):
    root, ds, _ = base
    r = variants_run(root, ds, "plain", variants=False)
    assert r.returncode == 0, r.stdout + r.stderr
    assert aln_bytes(root, ds, "plain") == aln_bytes(root, ds, "a")
    assert open(root / "plain.mpu", "rb").read() == open(root / "a.mpu", "rb").read()
    a, p = json.load(open(root / "a.json")), json.load(open(root / "plain.json"))
    assert "variants" not in p and "Variants" not in r.stdout and not (root / "plain.var").exists()
    for k in ("pileup_ms", "path"):
        a["pileup"].pop(k), p["pileup"].pop(k)
    assert a["pileup"] == p["pileup"] and a["total_score"] == p["total_score"]
    assert run_id(root, "plain") != run_id(root, "a")


@gpu
def test_variants_out_without_pileup_out(base):
    from mini_parallel_amd import read_pileup
    root, ds, _ = base
    r = variants_run(root, ds, "v", pileup=False)
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(root / "v.var", "rb").read() == open(root / "a.var", "rb").read()
    assert not (root / "v.mpu").exists() and "Pileup:" not in r.stdout
    rec = json.load(open(root / "v.json"))
    assert "pileup" not in rec
    check_var(root, ds, "v", read_pileup(root / "a.mpu")[0], r.stdout)
    assert aln_bytes(root, ds, "v") == aln_bytes(root, ds, "a")
    assert len({run_id(root, "v"), run_id(root, "a")}) == 2


@gpu
def test_resume_is_refused(base):
    root, ds, _ = base
    env = wgs_env(root / "wgs")
    env.update(GPU_CHUNK_SIZE_READS="256", MSW_GFASTQ_BATCH="256")
    # the same run again over its own checkpoint, which lists completed files: the pileup's refusal
    before = open(root / "a.var", "rb").read()
    args = FLAGS + ["--alignments-out", root / "a", "--pileup-out", root / "a.mpu", "--variants-out", root / "a.var"]
    r = run_cli(wgs_args(root, ds, "ck_a", args), env, root)
    assert r.returncode == 1 and "remove the checkpoint" in r.stderr and "--pileup-out" in r.stderr, r.stderr
    assert open(root / "a.var", "rb").read() == before
    # and with --variants-out alone
    r = variants_run(root, ds, "rv", pileup=False)
    assert r.returncode == 0, r.stdout + r.stderr
    before = open(root / "rv.var", "rb").read()
    args = FLAGS + ["--alignments-out", root / "rv", "--variants-out", root / "rv.var"]
    r = run_cli(wgs_args(root, ds, "ck_rv", args), env, root)
    assert r.returncode == 1 and "remove the checkpoint" in r.stderr and "--variants-out" in r.stderr, r.stderr
    assert open(root / "rv.var", "rb").read() == before
