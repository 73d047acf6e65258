"""``rustseq_mini --full-wgs ... --alignments-out DIR --pileup-out PATH``: the
.mpu file equals tests/pileup_oracle.py's pileup of the run's own .aln records
over the known reads, the run record carries the oracle's summary, and without
the flag the run writes what it wrote before."""
import json
import os

import numpy as np
import pytest

import pileup_oracle as po
import strand_oracle as so
from test_gpu_mapq_cli import planted_dataset, run_cli, wgs_args, wgs_env

pytestmark = pytest.mark.gpu

FLAGS = ["--mapq", "--both-strands"]


def pileup_run(root, ds, tag, extra=(), env=None, pileup=True):
    """One run into root/<tag>/ (alignments) and root/<tag>.mpu; its own
    checkpoint directory and run id."""
    (root / tag).mkdir()
    args = FLAGS + ["--alignments-out", root / tag, "--json", root / (tag + ".json")] + list(extra)
    if pileup:
        args += ["--pileup-out", root / (tag + ".mpu")]
    e = wgs_env(root / "wgs", tag)
    e.update(env or {})
    return run_cli(wgs_args(root, ds, "ck_" + tag, args), e, root)


def oracle_pileup(root, ds, tag, min_mapq):
    """The pileup of the run's .aln records: rows are the known reads,
    reverse-complemented where the record says strand 1."""
    from mini_parallel_amd import read_alignments
    counts = po.new_counts(len(ds["genome"]))
    used = skipped = 0
    for path, reads in zip(ds["files"], ds["reads"]):
        x = read_alignments(root / tag / (os.path.basename(path) + ".aln"))
        assert len(x.score) == len(reads)
        rows = [so.revcomp(r) if st else r for r, st in zip(reads, x.strand)]
        u, s = po.add(counts, rows, [len(r) for r in reads], x.ref_pos, x.nm, x.cigars, x.strand, x.mapq, min_mapq)
        used, skipped = used + u, skipped + s
    return counts, used, skipped


def aln_bytes(root, ds, tag):
    return [open(root / tag / (os.path.basename(p) + ".aln"), "rb").read() for p in ds["files"]]


@pytest.fixture(scope="module")
def base(tmp_path_factory):
    root = tmp_path_factory.mktemp("pileup_cli")
    ds = planted_dataset(root, per_file=70)
    r = pileup_run(root, ds, "a")
    assert r.returncode == 0, r.stdout + r.stderr
    return root, ds, r


def check_run(root, ds, tag, min_mapq, min_depth, stdout):
    from mini_parallel_amd import read_pileup
    want, used, skipped = oracle_pileup(root, ds, tag, min_mapq)
    got, file_used = read_pileup(root / (tag + ".mpu"))
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, (bad[:8].tolist(), got[bad[:8, 0]].tolist(), want[bad[:8, 0]].tolist())
    assert file_used == used and used + skipped == 140
    rec = json.load(open(root / (tag + ".json")))["pileup"]
    ms = rec.pop("pileup_ms")
    assert ms > 0
    assert rec == dict(po.summary(want, ds["genome"], min_depth), path=str(root / (tag + ".mpu")), min_mapq=min_mapq,
                       min_depth=min_depth, reads_used=used, reads_skipped=skipped)
    assert ("Pileup: %d reads used, %d skipped, %d bases covered" % (used, skipped, rec["covered"])) in stdout
    return got, used


def test_pileup_file_and_record_equal_the_oracle(base):
    root, ds, r = base
    got, used = check_run(root, ds, "a", 0, 4, r.stdout)
    # the planted reads cover both strands, gaps and soft clips; unplaced reads are skipped
    assert used > 100 and got[:, 7].any() and got[:, 5].any() and got[:, 6].any() and got[:, :4].any()


def test_min_mapq_30_and_min_depth(base):
    root, ds, _ = base
    r = pileup_run(root, ds, "q30", ["--pileup-min-mapq", 30, "--pileup-min-depth", 2])
    assert r.returncode == 0, r.stdout + r.stderr
    _, used30 = check_run(root, ds, "q30", 30, 2, r.stdout)
    assert 0 < used30 < oracle_pileup(root, ds, "a", 0)[1]
    assert aln_bytes(root, ds, "q30") == aln_bytes(root, ds, "a")


def test_first_trace_stride_1_gives_the_same_counts(base):
    """Every read overflows the first trace: the records are traced again at
    the exact stride, and each read is still added exactly once."""
    root, ds, _ = base
    r = pileup_run(root, ds, "s1", env={"MSW_CLI_CIGAR_STRIDE": "1"})
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(root / "s1.mpu", "rb").read() == open(root / "a.mpu", "rb").read()
    assert aln_bytes(root, ds, "s1") == aln_bytes(root, ds, "a")


def test_without_the_flag_the_run_is_what_it_was(base):
    root, ds, _ = base
    r = pileup_run(root, ds, "plain", pileup=False)
    assert r.returncode == 0, r.stdout + r.stderr
    assert aln_bytes(root, ds, "plain") == aln_bytes(root, ds, "a")
    assert "pileup" not in json.load(open(root / "plain.json")) and "Pileup" not in r.stdout
    assert not (root / "plain.mpu").exists()
    a, p = json.load(open(root / "a.json")), json.load(open(root / "plain.json"))
    assert a["total_score"] == p["total_score"] and a["mapq_histogram"] == p["mapq_histogram"]


def test_resume_is_refused_and_run_ids_differ(base):
    root, ds, _ = base
    # the same run again over its own checkpoint, which lists completed files
    before = open(root / "a.mpu", "rb").read()
    args = FLAGS + ["--alignments-out", root / "a", "--pileup-out", root / "a.mpu"]
    r = run_cli(wgs_args(root, ds, "ck_a", args), wgs_env(root / "wgs", "a"), root)
    assert r.returncode == 1 and "remove the checkpoint" in r.stderr and "--pileup-out" in r.stderr, r.stderr
    assert open(root / "a.mpu", "rb").read() == before
    # the stable run id depends on the flag and on the threshold
    ids = {}
    for tag, extra in (("i0", []), ("i1", ["--pileup-out", root / "i1.mpu"]),
                       ("i2", ["--pileup-out", root / "i2.mpu", "--pileup-min-mapq", 30])):
        (root / tag).mkdir()
        r = run_cli(wgs_args(root, ds, "ck_" + tag, FLAGS + ["--alignments-out", root / tag] + extra),
                    wgs_env(root / "wgs"), root)
        assert r.returncode == 0, r.stdout + r.stderr
        cks = [f for f in os.listdir(root / ("ck_" + tag)) if f.startswith("checkpoint_wgs_")]
        assert len(cks) == 1
        ids[tag] = json.load(open(root / ("ck_" + tag) / cks[0]))["run_id"]
    assert len(set(ids.values())) == 3
