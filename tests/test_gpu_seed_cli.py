"""``rustseq_mini --full-wgs --score-mode sw --map``: lane files whose headers
carry no pos= tag are placed by the k-mer index and seed voting on the GPU;
every .aln record and strand byte equals the record oracles fed with the
window positions of tests/seed_oracle.py."""
import gzip
import json
import os
import re
import subprocess

import numpy as np
import pytest

import aln_oracle as ao
import seed_oracle as sd
import strand_oracle as so

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mini_parallel_amd", "rustseq_mini")
LIN = (2, -1, 0, 2, False)
WINDOW = 300


def run_cli(args, env, cwd):
    e = dict(os.environ)
    e.pop("WGS_RUN_ID", None)
    e.update(env)
    return subprocess.run([CLI] + [str(a) for a in args], capture_output=True, text=True, env=e, cwd=cwd, timeout=300)


def wgs_env(data, run_id, **extra):
    env = {"WGS_DATA_DIR": str(data), "WGS_SAMPLE_ID": "SYN", "WGS_LANES": "1", "WGS_READS_PER_LANE": "2",
           "GPU_CHUNK_SIZE_READS": "100", "MSW_GFASTQ_BATCH": "100", "MSW_GFASTQ_SPAN_MB": "1", "WGS_RUN_ID": run_id}
    env.update(extra)
    return env


def wgs_args(root, ds, ckdir):
    (root / ckdir).mkdir(exist_ok=True)
    return ["--full-wgs", "--gpu", "--score-mode", "sw", "--reference", ds["reference"], "--window", WINDOW,
            "--checkpoint-dir", root / ckdir]


def strip_tags(src_dir, dst_dir, files):
    """The same lane files without the pos= tags of their headers."""
    from mini_parallel_amd.synthetic import bgzf_compress
    os.makedirs(dst_dir)
    for f in files:
        text = gzip.open(f, "rb").read()
        bare, n = re.subn(rb" pos=-?\d+\n", b"\n", text)
        assert n == text.count(b"\n") // 4 and b"pos=" not in bare
        with open(os.path.join(dst_dir, os.path.basename(f)), "wb") as out:
            out.write(bgzf_compress(bare, 1))


def have_record(x, p):
    return (int(x.score[p]), int(x.end_i[p]), int(x.end_j[p]), int(x.strand[p]), int(x.ref_pos[p]), int(x.nm[p]),
            [int(o) for o in x.cigars[p]])


def test_cli_map(tmp_path):
    """Two BGZF lane files of 300 reads, half of them reverse-complemented,
    without pos= tags, in batches of 100 over two streams."""
    from mini_parallel_amd import read_alignments
    from mini_parallel_amd.synthetic import wgs_genome, write_wgs_dataset
    ds = write_wgs_dataset(str(tmp_path / "wgs"), lanes=1, reads_per_lane=2, reads_per_file=300, bgzf=True,
                           reverse_fraction=0.5)
    strip_tags(tmp_path / "wgs", tmp_path / "bare", ds["files"])
    names = [os.path.basename(f) for f in ds["files"]]
    for d in ("aln", "aln_tagged", "aln_nomap"):
        (tmp_path / d).mkdir()
    flags = ["--both-strands", "--alignments-out"]
    mapped = run_cli(wgs_args(tmp_path, ds, "m") + ["--map"] + flags + [tmp_path / "aln", "--json", tmp_path / "m.json"],
                     wgs_env(tmp_path / "bare", "m"), tmp_path)
    assert mapped.returncode == 0, mapped.stdout + mapped.stderr
    tagged = run_cli(wgs_args(tmp_path, ds, "t") + ["--map"] + flags + [tmp_path / "aln_tagged"],
                     wgs_env(tmp_path / "wgs", "t"), tmp_path)
    assert tagged.returncode == 0, tagged.stdout + tagged.stderr
    nomap = run_cli(wgs_args(tmp_path, ds, "n") + flags + [tmp_path / "aln_nomap", "--json", tmp_path / "n.json"],
                    wgs_env(tmp_path / "bare", "n"), tmp_path)
    assert nomap.returncode == 0, nomap.stdout + nomap.stderr
    g = wgs_genome()
    ix = sd.Index(g, 12, 64)
    placed, total = 0, 0
    for name, b in zip(names, ds["batches"]):
        reads = [b.reads[p, :b.read_len[p]].tobytes() for p in range(b.n_pairs)]
        wp, votes, hits, flags_ = sd.place(ix, reads, b.read_len, both=True, band=16, cap=4096, step=1, min_votes=1,
                                           window=WINDOW)
        wins = [ao.window_of(g, int(p), WINDOW).tobytes() for p in wp]
        recs = so.records(reads, wins, wp, LIN)
        got = read_alignments(tmp_path / "aln" / (name + ".aln"))
        assert len(got.score) == b.n_pairs == 300
        for p, r in enumerate(recs):
            assert have_record(got, p) == tuple(r), (name, p, int(wp[p]), ao.cigar_text(r.ops))
        placed += int((wp >= 0).sum())
        total += sum(r.score for r in recs)
        # the related reads land where they were drawn from, on the strand they were written on
        related = np.array([r.score for r in recs]) > 150
        strand = np.array([r.strand for r in recs])
        assert related.sum() > 200 and np.array_equal(strand[related], b.reverse[related].astype(int))
        # the tags change nothing under --map
        assert open(tmp_path / "aln" / (name + ".aln"), "rb").read() == \
            open(tmp_path / "aln_tagged" / (name + ".aln"), "rb").read()
        # without --map these files give nothing: the gap the flag closes
        none = read_alignments(tmp_path / "aln_nomap" / (name + ".aln"))
        assert len(none.score) == 300 and not none.score.any() and (none.ref_pos == -1).all()
    rec, rec_n = json.load(open(tmp_path / "m.json")), json.load(open(tmp_path / "n.json"))
    assert rec["map"] is True and rec["seed_k"] == 12 and rec["placed_reads"] == placed > 500
    assert rec["total_score"] == total > 0 and rec["setup_phases"]["index_ms"] > 0
    assert rec_n["map"] is False and rec_n["placed_reads"] == 0 and rec_n["total_score"] == 0
    assert f"{placed} of 600 reads placed" in mapped.stdout and "placed" not in nomap.stdout


def test_cli_map_one_strand_k10(tmp_path):
    """--map without --both-strands (no reverse-complement slab) at
    --seed-k 10 --seed-max-occ 8 --seed-band 4, sums only and with records."""
    from mini_parallel_amd import read_alignments
    from mini_parallel_amd.synthetic import wgs_genome, write_wgs_dataset
    ds = write_wgs_dataset(str(tmp_path / "wgs"), lanes=1, reads_per_lane=2, reads_per_file=150, bgzf=True)
    strip_tags(tmp_path / "wgs", tmp_path / "bare", ds["files"])
    (tmp_path / "aln").mkdir()
    seed = ["--map", "--seed-k", 10, "--seed-max-occ", 8, "--seed-band", 4]
    r = run_cli(wgs_args(tmp_path, ds, "a") + seed + ["--alignments-out", tmp_path / "aln"],
                wgs_env(tmp_path / "bare", "a"), tmp_path)
    sums = run_cli(wgs_args(tmp_path, ds, "s") + seed + ["--json", tmp_path / "s.json"],
                   wgs_env(tmp_path / "bare", "s"), tmp_path)
    assert r.returncode == 0 and sums.returncode == 0, r.stdout + r.stderr + sums.stdout + sums.stderr
    g = wgs_genome()
    ix = sd.Index(g, 10, 8)
    total, placed = 0, 0
    for f, b in zip(ds["files"], ds["batches"]):
        reads = [b.reads[p, :b.read_len[p]].tobytes() for p in range(b.n_pairs)]
        wp = sd.place(ix, reads, b.read_len, both=False, band=4, cap=4096, step=1, min_votes=1, window=WINDOW)[0]
        got = read_alignments(tmp_path / "aln" / (os.path.basename(f) + ".aln"))
        for p, read in enumerate(reads):
            w = ao.record(read, ao.window_of(g, int(wp[p]), WINDOW).tobytes(), int(wp[p]), *LIN)
            have = (int(got.score[p]), int(got.end_i[p]), int(got.end_j[p]), int(got.ref_pos[p]), int(got.nm[p]),
                    [int(o) for o in got.cigars[p]])
            assert have == tuple(w), (p, int(wp[p]))
            total += w.score
        placed += int((wp >= 0).sum())
    rec = json.load(open(tmp_path / "s.json"))
    assert rec["total_score"] == total and rec["placed_reads"] == placed and rec["seed_k"] == 10


def test_cli_map_refused_on_gzip_lane_files(tmp_path):
    """Plain gzip lane files go to the host reader, which has no --map."""
    from mini_parallel_amd.synthetic import write_wgs_dataset
    ds = write_wgs_dataset(str(tmp_path / "wgs"), lanes=1, reads_per_lane=2, reads_per_file=20, bgzf=False)
    r = run_cli(wgs_args(tmp_path, ds, "r") + ["--map"], wgs_env(tmp_path / "wgs", "r"), tmp_path)
    assert r.returncode == 1 and "host reader" in r.stderr and len(r.stderr.strip().splitlines()) == 1, r.stderr


def test_map_run_id_differs(tmp_path):
    from mini_parallel_amd.synthetic import write_wgs_dataset
    ds = write_wgs_dataset(str(tmp_path / "wgs"), lanes=1, reads_per_lane=2, reads_per_file=20, bgzf=True)
    ids = {}
    for tag, flag in (("one", []), ("map", ["--map"]), ("map10", ["--map", "--seed-k", 10])):
        env = wgs_env(tmp_path / "wgs", "x")
        env.pop("WGS_RUN_ID")                    # the stable id
        r = run_cli(wgs_args(tmp_path, ds, tag) + flag, env, tmp_path)
        assert r.returncode == 0, r.stdout + r.stderr
        cks = [f for f in os.listdir(tmp_path / tag) if f.startswith("checkpoint_wgs_")]
        assert len(cks) == 1
        ids[tag] = json.load(open(tmp_path / tag / cks[0]))["run_id"]
    assert len(set(ids.values())) == 3
