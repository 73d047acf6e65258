"""``rustseq_mini --full-wgs --score-mode sw --map --mapq``: every read's two
candidate loci are scored on the GPU and the better one becomes its .aln
record, with a mapping quality and the other candidate's score (flag bit 1);
records, mapq and sub_score equal tests/mapq_oracle.py's composition.  Without
--mapq the run and its files are those of --map alone."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import mapq_oracle as mo
import seed_oracle as sd
import strand_oracle as so
from test_gpu_mapq import planted_reads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mini_parallel_amd", "rustseq_mini")
LIN = (2, -1, 0, 2, False)
AFF = (2, -1, 3, 1, True)
WINDOW = 300
K = 8
PER_FILE = 70
ACGT = np.frombuffer(b"ACGT", np.uint8)


def run_cli(args, env, cwd):
    e = dict(os.environ)
    e.pop("WGS_RUN_ID", None)
    e.update(env)
    return subprocess.run([CLI] + [str(a) for a in args], capture_output=True, text=True, env=e, cwd=cwd, timeout=300)


def wgs_env(data, run_id=None):
    env = {"WGS_DATA_DIR": str(data), "WGS_SAMPLE_ID": "SYN", "WGS_LANES": "1", "WGS_READS_PER_LANE": "2",
           "GPU_CHUNK_SIZE_READS": "50", "MSW_GFASTQ_BATCH": "50", "MSW_GFASTQ_SPAN_MB": "1"}
    if run_id:
        env["WGS_RUN_ID"] = run_id
    return env


def wgs_args(root, ds, ckdir, extra=()):
    (root / ckdir).mkdir(exist_ok=True)
    return ["--full-wgs", "--gpu", "--score-mode", "sw", "--reference", ds["reference"], "--window", WINDOW,
            "--checkpoint-dir", root / ckdir, "--map", "--seed-k", K] + list(extra)


def planted_dataset(root, per_file=PER_FILE):
    """The planted-repeat genome of test_gpu_mapq.py as reference.fa and two
    BGZF lane files without pos= tags: its hand-made reads of 1 .. 256 bases
    (exact and diverged copies, the read whose alternate wins, unique and
    unrelated ones), then reads drawn from anywhere with 3 % substitutions,
    every other one reverse-complemented."""
    from mini_parallel_amd.synthetic import bgzf_compress
    g, reads, tags = planted_reads()
    rng = np.random.default_rng(77)
    special = [(t, r) for t, r in zip(tags, reads) if 1 <= len(r) <= 256]
    files = [[], []]
    for k, tr in enumerate(special):
        files[k % 2].append(tr)
    for f in files:
        while len(f) < per_file:
            L = int(rng.integers(40, 200))
            at = int(rng.integers(0, len(g) - L))
            a = np.frombuffer(g[at:at + L], np.uint8).copy()
            hit = rng.random(L) < 0.03
            a[hit] = ACGT[rng.integers(0, 4, int(hit.sum()))]
            r = a.tobytes()
            f.append(("draw%d" % at, so.revcomp(r) if len(f) % 2 else r))
    os.makedirs(root / "wgs")
    with open(root / "wgs" / "reference.fa", "w") as out:
        s = g.decode()
        out.write(">planted\n" + "\n".join(s[k:k + 80] for k in range(0, len(s), 80)) + "\n")
    names = []
    for k, f in enumerate(files):
        text = b"".join(b"@SYN:1:%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, (_, r) in enumerate(f))
        names.append(str(root / "wgs" / ("SYN_L001_R%d_001.fastq.gz" % (k + 1))))
        with open(names[-1], "wb") as out:
            out.write(bgzf_compress(text, 1))
    return {"genome": g, "reference": str(root / "wgs" / "reference.fa"), "files": names,
            "reads": [[r for _, r in f] for f in files], "tags": [[t for t, _ in f] for f in files]}


def block_flags(path):
    """The flags word of every block of an .aln file."""
    data, at, flags = open(path, "rb").read(), 0, []
    while at < len(data):
        magic, version, first, n, n_ops, fl, zero = struct.unpack_from("<IIQIIII", data, at)
        assert magic == 0x4157534D and version == 1 and zero == 0
        pad = (n + 3) // 4 * 4
        at += 32 + n * 24 + n_ops * 4 + (pad if fl & 1 else 0) + (pad + 4 * n if fl & 2 else 0)
        flags.append(fl)
    assert at == len(data)
    return flags


def have_record(x, p):
    return (int(x.score[p]), int(x.end_i[p]), int(x.end_j[p]), int(x.strand[p]), int(x.ref_pos[p]), int(x.nm[p]),
            [int(o) for o in x.cigars[p]])


def histogram(mapqs):
    q = np.asarray(mapqs)
    return {"0": int((q == 0).sum()), "1-29": int(((q >= 1) & (q < 30)).sum()),
            "30-59": int(((q >= 30) & (q < 60)).sum()), "60": int((q == 60).sum())}


def test_cli_mapq_both_strands(tmp_path):
    """Two lane files of 70 reads in batches of 50 over two streams."""
    from mini_parallel_amd import read_alignments
    ds = planted_dataset(tmp_path)
    for d in ("aln", "aln_a", "aln_b"):
        (tmp_path / d).mkdir()
    flags = ["--both-strands", "--alignments-out"]
    env = wgs_env(tmp_path / "wgs", "q")
    mq = run_cli(wgs_args(tmp_path, ds, "q", ["--mapq"] + flags + [tmp_path / "aln", "--json", tmp_path / "q.json"]),
                 env, tmp_path)
    assert mq.returncode == 0, mq.stdout + mq.stderr
    plain = [run_cli(wgs_args(tmp_path, ds, d, flags + [tmp_path / d, "--json", tmp_path / (d + ".json")]), env, tmp_path)
             for d in ("aln_a", "aln_b")]
    assert all(r.returncode == 0 for r in plain), plain[0].stdout + plain[0].stderr
    ix = sd.Index(np.frombuffer(ds["genome"], np.uint8), K, 64)
    mapqs, alt_wins, total, total_plain = [], 0, 0, 0
    for path, reads, tags in zip(ds["files"], ds["reads"], ds["tags"]):
        name = os.path.basename(path) + ".aln"
        recs, c0, c1 = mo.map_records(ds["genome"], ix, reads, LIN, True, window=WINDOW)
        got = read_alignments(tmp_path / "aln" / name)
        assert len(got.score) == len(reads) == PER_FILE
        assert block_flags(tmp_path / "aln" / name) == [3, 3]
        for p, r in enumerate(recs):
            assert have_record(got, p) + (int(got.mapq[p]), int(got.sub_score[p])) == tuple(r)[:9], \
                (name, p, tags[p], r.cand)
        mapqs += [r.mapq for r in recs]
        alt_wins += sum(r.cand for r in recs)
        total += sum(r.score for r in recs)
        # without --mapq: the records of --map alone (candidate 0's, which tests/test_gpu_seed_cli.py holds
        # to its oracle), in blocks without bit 1, the same bytes run after run
        none = read_alignments(tmp_path / "aln_a" / name)
        for p, r in enumerate(recs):
            if r.cand == 0:
                assert have_record(none, p) == have_record(got, p), (name, p, tags[p])
            else:
                assert int(none.score[p]) == r.sub_score < r.score and int(none.ref_pos[p]) != r.ref_pos, (name, p)
        total_plain += int(none.score.sum())
        assert (none.mapq == 255).all() and not none.sub_score.any()
        assert block_flags(tmp_path / "aln_a" / name) == [1, 1]
        assert open(tmp_path / "aln_a" / name, "rb").read() == open(tmp_path / "aln_b" / name, "rb").read()
    # the planted cases are there: a read whose alternate wins, repeats at 0, unique reads at 60
    assert alt_wins >= 2 and total > total_plain
    want = histogram(mapqs)
    assert want["0"] > 5 and want["60"] > 50 and want["1-29"] + want["30-59"] > 0
    rec = json.load(open(tmp_path / "q.json"))
    assert rec["mapq"] is True and rec["seed_sep"] == 0 and rec["mapq_histogram"] == want
    assert rec["map"] is True and rec["total_score"] == total
    assert "MAPQ: %d reads at 0, %d at 1-29, %d at 30-59, %d at 60" % tuple(want.values()) in mq.stdout
    for d in ("aln_a", "aln_b"):
        rec_n = json.load(open(tmp_path / (d + ".json")))
        assert "mapq" not in rec_n and "mapq_histogram" not in rec_n and rec_n["total_score"] == total_plain
    assert "MAPQ" not in plain[0].stdout


def test_cli_mapq_one_strand_affine_sep(tmp_path):
    """One strand (no oriented rows to move), affine gaps, --seed-sep 40, with
    records and as sums only."""
    from mini_parallel_amd import read_alignments
    ds = planted_dataset(tmp_path, per_file=70)
    (tmp_path / "aln").mkdir()
    aff = ["--gap-model", "affine", "--gap-open", 3, "--gap-extend", 1, "--mapq", "--seed-sep", 40]
    env = wgs_env(tmp_path / "wgs", "o")
    r = run_cli(wgs_args(tmp_path, ds, "o", aff + ["--alignments-out", tmp_path / "aln"]), env, tmp_path)
    sums = run_cli(wgs_args(tmp_path, ds, "s", aff + ["--json", tmp_path / "s.json"]), env, tmp_path)
    assert r.returncode == 0 and sums.returncode == 0, r.stdout + r.stderr + sums.stdout + sums.stderr
    ix = sd.Index(np.frombuffer(ds["genome"], np.uint8), K, 64)
    mapqs, total = [], 0
    for path, reads, tags in zip(ds["files"], ds["reads"], ds["tags"]):
        recs = mo.map_records(ds["genome"], ix, reads, AFF, False, window=WINDOW, sep=40)[0]
        got = read_alignments(tmp_path / "aln" / (os.path.basename(path) + ".aln"))
        assert block_flags(tmp_path / "aln" / (os.path.basename(path) + ".aln")) == [2, 2]
        for p, w in enumerate(recs):
            assert have_record(got, p) + (int(got.mapq[p]), int(got.sub_score[p])) == tuple(w)[:9], (p, tags[p], w.cand)
        mapqs += [w.mapq for w in recs]
        total += sum(w.score for w in recs)
    rec = json.load(open(tmp_path / "s.json"))
    assert rec["mapq"] is True and rec["seed_sep"] == 40 and rec["mapq_histogram"] == histogram(mapqs)
    assert rec["total_score"] == total


def test_mapq_run_id_differs(tmp_path):
    """A checkpoint is not resumed across --mapq or another --seed-sep."""
    ds = planted_dataset(tmp_path, per_file=20)
    ids = {}
    for tag, flag in (("map", []), ("mapq", ["--mapq"]), ("sep", ["--mapq", "--seed-sep", 40])):
        r = run_cli(wgs_args(tmp_path, ds, tag, flag), wgs_env(tmp_path / "wgs"), tmp_path)   # the stable id
        assert r.returncode == 0, r.stdout + r.stderr
        cks = [f for f in os.listdir(tmp_path / tag) if f.startswith("checkpoint_wgs_")]
        assert len(cks) == 1
        ids[tag] = json.load(open(tmp_path / tag / cks[0]))["run_id"]
    assert len(set(ids.values())) == 3
