"""``rustseq_mini --full-wgs --score-mode sw --both-strands`` on lane files with
reverse-complemented reads: .aln records and strand bytes, .scores, file sums
and the run record against tests/strand_oracle.py; the one-strand run on the
same files beside it."""
import json
import os
import subprocess

import numpy as np
import pytest

import aln_oracle as ao
import strand_oracle as so

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mini_parallel_amd", "rustseq_mini")
LIN = (2, -1, 0, 2, False)
AFF = (2, -1, 3, 1, True)
SCHEMES = {"lin": LIN, "aff": AFF}
REC_T = np.dtype([("score", "<i4"), ("end_i", "<i2"), ("end_j", "<i2")])


def run_cli(args, env, cwd):
    e = dict(os.environ)
    e.pop("WGS_RUN_ID", None)
    e.update(env)
    return subprocess.run([CLI] + [str(a) for a in args], capture_output=True, text=True, env=e, cwd=cwd, timeout=300)


def wgs_env(root, run_id=None, **extra):
    env = {"WGS_DATA_DIR": str(root / "wgs"), "WGS_SAMPLE_ID": "SYN", "WGS_LANES": "1", "WGS_READS_PER_LANE": "2",
           "GPU_CHUNK_SIZE_READS": "100", "MSW_GFASTQ_BATCH": "100", "MSW_GFASTQ_SPAN_MB": "1"}
    if run_id:
        env["WGS_RUN_ID"] = run_id
    env.update(extra)
    return env


def wgs_args(root, ds, scheme, ckdir):
    gap = ["--gap-model", "affine", "--gap-open", "3", "--gap-extend", "1"] if SCHEMES[scheme][4] else []
    (root / ckdir).mkdir(exist_ok=True)
    return ["--full-wgs", "--gpu", "--score-mode", "sw", "--reference", ds["reference"], "--window", "300",
            "--checkpoint-dir", root / ckdir] + gap


def batch_pairs(b):
    reads = [b.reads[p, :b.read_len[p]].tobytes() for p in range(b.n_pairs)]
    wins = [b.wins[p, :b.win_len[p]].tobytes() for p in range(b.n_pairs)]
    return reads, wins


def have_record(x, p):
    return (int(x.score[p]), int(x.end_i[p]), int(x.end_j[p]), int(x.strand[p]), int(x.ref_pos[p]), int(x.nm[p]),
            [int(o) for o in x.cigars[p]])


def file_sums(stdout):
    """{file number: score} from the 'File k: Score=...' lines."""
    return {int(l.split(":")[0].split()[1]): int(l.split("Score=")[1].split(",")[0])
            for l in stdout.splitlines() if l.startswith("File ") and "Score=" in l}


@pytest.mark.parametrize("scheme", ["lin", "aff"])
def test_cli_both_strands(tmp_path, scheme):
    """Two BGZF lane files of 300 reads, half of them reverse-complemented, in
    batches of 100.  With --both-strands every record and strand byte equals
    the oracle, .scores agrees with .aln, reverse_reads is the oracle's count
    and MSW_CLI_CIGAR_STRIDE=1 writes the same alignments; without the flag
    the same files still give the one-strand oracle, with lower file sums."""
    from mini_parallel_amd import read_alignments
    from mini_parallel_amd.synthetic import write_wgs_dataset
    from oracle import oracle_lib
    sch = SCHEMES[scheme]
    ds = write_wgs_dataset(str(tmp_path / "wgs"), lanes=1, reads_per_lane=2, reads_per_file=300, bgzf=True,
                           reverse_fraction=0.5)
    names = [os.path.basename(f) for f in ds["files"]]
    for d in ("aln", "aln1", "scores", "scores_one"):
        (tmp_path / d).mkdir()
    both = run_cli(wgs_args(tmp_path, ds, scheme, "both") + ["--both-strands", "--alignments-out", tmp_path / "aln",
                                                             "--scores-out", tmp_path / "scores", "--json",
                                                             tmp_path / "both.json"], wgs_env(tmp_path, "both"), tmp_path)
    assert both.returncode == 0, both.stdout + both.stderr
    s1 = run_cli(wgs_args(tmp_path, ds, scheme, "s1") + ["--both-strands", "--alignments-out", tmp_path / "aln1"],
                 wgs_env(tmp_path, "s1", MSW_CLI_CIGAR_STRIDE="1"), tmp_path)
    assert s1.returncode == 0, s1.stdout + s1.stderr
    one = run_cli(wgs_args(tmp_path, ds, scheme, "one") + ["--scores-out", tmp_path / "scores_one", "--json",
                                                           tmp_path / "one.json"], wgs_env(tmp_path, "one"), tmp_path)
    assert one.returncode == 0, one.stdout + one.stderr
    reverse = 0
    sums_both, sums_one = file_sums(both.stdout), file_sums(one.stdout)
    for k, (name, b) in enumerate(zip(names, ds["batches"])):
        reads, wins = batch_pairs(b)
        recs = so.records(reads, wins, b.pos, sch)
        got, got1 = read_alignments(tmp_path / "aln" / (name + ".aln")), read_alignments(tmp_path / "aln1" / (name + ".aln"))
        assert len(got.score) == b.n_pairs == 300
        for p, r in enumerate(recs):
            for x in (got, got1):
                assert have_record(x, p) == tuple(r), (name, p, ao.cigar_text(have_record(x, p)[6]), ao.cigar_text(r.ops))
        strand = np.array([r.strand for r in recs])
        reverse += int(strand.sum())
        # the dataset's reverse reads are found as such (unrelated reads aside, whichever way they fall)
        related = np.array([r.score for r in recs]) > 150
        assert np.array_equal(strand[related], b.reverse[related].astype(int)) and related.sum() > 200
        scores = np.fromfile(tmp_path / "scores" / (name + ".scores"), dtype=REC_T)
        assert np.array_equal(scores["score"], got.score) and np.array_equal(scores["end_i"], got.end_i)
        assert np.array_equal(scores["end_j"], got.end_j)
        assert sums_both[k + 1] == sum(r.score for r in recs)
        # the run without the flag: the one-strand oracle, as before the flag existed
        one_scores = np.fromfile(tmp_path / "scores_one" / (name + ".scores"), dtype=REC_T)
        m, x, go, ge, aff = sch
        ws, wi, wj = oracle_lib.sw_batch(b.reads, b.read_len, b.wins, b.win_len, match=m, mismatch=x, gap_open=go,
                                         gap_extend=ge, affine=aff, threads=4)
        assert np.array_equal(one_scores["score"], ws) and np.array_equal(one_scores["end_i"], wi)
        assert np.array_equal(one_scores["end_j"], wj)
        assert sums_one[k + 1] == int(ws.sum()) < sums_both[k + 1]          # the feature's point
    rec_both, rec_one = json.load(open(tmp_path / "both.json")), json.load(open(tmp_path / "one.json"))
    assert rec_both["both_strands"] is True and rec_both["reverse_reads"] == reverse > 200
    assert rec_one["both_strands"] is False and rec_one["reverse_reads"] == 0
    assert f"Both strands: {reverse} reverse reads" in both.stdout and "Both strands" not in one.stdout
    assert rec_both["total_score"] > rec_one["total_score"]


def test_cli_forward_dataset_and_sums_only(tmp_path):
    """On a dataset without reverse reads --both-strands writes the plain
    run's score for every read whose oracle strand is 0; the flag alone (sums
    only) prints the both-strand sums."""
    from mini_parallel_amd.synthetic import write_wgs_dataset
    ds = write_wgs_dataset(str(tmp_path / "wgs"), lanes=1, reads_per_lane=2, reads_per_file=300, bgzf=True)
    for d in ("scores", "scores_one"):
        (tmp_path / d).mkdir()
    both = run_cli(wgs_args(tmp_path, ds, "lin", "both") + ["--both-strands", "--scores-out", tmp_path / "scores"],
                   wgs_env(tmp_path, "both"), tmp_path)
    one = run_cli(wgs_args(tmp_path, ds, "lin", "one") + ["--scores-out", tmp_path / "scores_one"],
                  wgs_env(tmp_path, "one"), tmp_path)
    alone = run_cli(wgs_args(tmp_path, ds, "lin", "alone") + ["--both-strands", "--json", tmp_path / "alone.json"],
                    wgs_env(tmp_path, "alone"), tmp_path)
    for r in (both, one, alone):
        assert r.returncode == 0, r.stdout + r.stderr
    total, reverse = 0, 0
    for f, b in zip(ds["files"], ds["batches"]):
        name = os.path.basename(f)
        reads, wins = batch_pairs(b)
        s, ei, ej, strand = so.score_batch(reads, wins, LIN)
        a = np.fromfile(tmp_path / "scores" / (name + ".scores"), dtype=REC_T)
        o = np.fromfile(tmp_path / "scores_one" / (name + ".scores"), dtype=REC_T)
        fwd = strand == 0
        assert fwd.sum() > 250 and np.array_equal(a[fwd], o[fwd])
        assert np.array_equal(a["score"], s) and np.array_equal(a["end_i"], ei) and np.array_equal(a["end_j"], ej)
        total += int(s.sum())
        reverse += int(strand.sum())
    rec = json.load(open(tmp_path / "alone.json"))
    assert rec["total_score"] == total == sum(file_sums(alone.stdout).values())
    assert rec["reverse_reads"] == reverse and rec["both_strands"] is True


def test_cli_both_strands_file_switch(tmp_path):
    """Four BGZF lane files of 250 reads over the two workers of one GPU, in
    batches of 100, at MSW_CLI_CIGAR_STRIDE=1: a set's second trace reads its
    own oriented rows after the worker has gone on to the next file."""
    from mini_parallel_amd import read_alignments
    from mini_parallel_amd.synthetic import write_wgs_dataset
    ds = write_wgs_dataset(str(tmp_path / "wgs"), lanes=2, reads_per_lane=2, reads_per_file=250, bgzf=True,
                           reverse_fraction=0.5)
    assert len(ds["files"]) == 4
    for d in ("aln", "scores"):
        (tmp_path / d).mkdir()
    r = run_cli(wgs_args(tmp_path, ds, "lin", "sw4") + ["--both-strands", "--alignments-out", tmp_path / "aln",
                                                        "--scores-out", tmp_path / "scores"],
                wgs_env(tmp_path, "sw4", WGS_LANES="2", MSW_CLI_CIGAR_STRIDE="1"), tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    for f, b in zip(ds["files"], ds["batches"]):
        name = os.path.basename(f)
        got = read_alignments(tmp_path / "aln" / (name + ".aln"))
        assert len(got.score) == b.n_pairs == 250
        reads, wins = batch_pairs(b)
        for p, want in enumerate(so.records(reads, wins, b.pos, LIN)):
            assert have_record(got, p) == tuple(want), (name, p)
        scores = np.fromfile(tmp_path / "scores" / (name + ".scores"), dtype=REC_T)
        assert np.array_equal(scores["score"], got.score) and np.array_equal(scores["end_i"], got.end_i)
    ck = json.load(open(tmp_path / "sw4" / "checkpoint_sw4.json"))
    assert ck["completed_files"] == ck["total_files"] == 4


def test_cli_both_strands_refused(tmp_path):
    """Outside --full-wgs sw, with the host reader and on plain gzip lane
    files: status 1 and one line, nothing written."""
    from mini_parallel_amd.synthetic import write_wgs_dataset
    ds = write_wgs_dataset(str(tmp_path / "wgs"), lanes=1, reads_per_lane=2, reads_per_file=20, bgzf=True)
    (tmp_path / "scores").mkdir()
    base = wgs_args(tmp_path, ds, "lin", "r") + ["--both-strands", "--scores-out", tmp_path / "scores"]
    compat = [a for a in base]
    compat[compat.index("sw")] = "compat"
    for args, extra, word in ((base, {"MSW_GPU_INFLATE": "0"}, "host reader"), (compat, {}, "--score-mode sw")):
        r = run_cli(args, wgs_env(tmp_path, "r", **extra), tmp_path)
        assert r.returncode == 1 and word in r.stderr and len(r.stderr.strip().splitlines()) == 1, r.stderr
        assert os.listdir(tmp_path / "scores") == []
    ds = write_wgs_dataset(str(tmp_path / "wgs"), lanes=1, reads_per_lane=2, reads_per_file=20, bgzf=False)
    r = run_cli(base, wgs_env(tmp_path, "r"), tmp_path)
    assert r.returncode == 1 and "host reader" in r.stderr and len(r.stderr.strip().splitlines()) == 1, r.stderr
    assert os.listdir(tmp_path / "scores") == []


def test_checkpoints_of_the_two_modes_have_different_run_ids(tmp_path):
    from mini_parallel_amd.synthetic import write_wgs_dataset
    ds = write_wgs_dataset(str(tmp_path / "wgs"), lanes=1, reads_per_lane=2, reads_per_file=20, bgzf=True)
    ids = {}
    for tag, flag in (("one", []), ("both", ["--both-strands"])):
        r = run_cli(wgs_args(tmp_path, ds, "lin", tag) + flag, wgs_env(tmp_path), tmp_path)     # no WGS_RUN_ID: the stable id
        assert r.returncode == 0, r.stdout + r.stderr
        cks = [f for f in os.listdir(tmp_path / tag) if f.startswith("checkpoint_wgs_")]
        assert len(cks) == 1
        ids[tag] = json.load(open(tmp_path / tag / cks[0]))["run_id"]
    assert ids["one"] != ids["both"]
