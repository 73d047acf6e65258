"""``rustseq_mini --full-wgs ... --pileup-out PATH --pileup-min-baseq N``: the
workers' readers keep the lane files' quality lines, and the .mpu file and
the run record's lowq_columns equal tests/pileup_qual_oracle.py fed with the
run's own .aln records, the reads and the quality lines parsed from the FASTQ
text.  With N == 0 every output file is what the run without the flag writes.

The threshold is 30: the "illumina" quality strings of synthetic.py run from
Q22 to Q41, so the issue's 20 drops nothing; at 30 the oracle drops 28 % of
the columns (asserted below to lie between 1 % and 50 %)."""
import gzip
import json
import os

import numpy as np
import pytest

import pileup_oracle as po
import pileup_qual_oracle as pq
import strand_oracle as so
from test_gpu_mapq_cli import run_cli

pytestmark = pytest.mark.gpu

WINDOW = 300
MIN_BASEQ = 30
FLAGS = ["--map", "--mapq", "--both-strands"]


def env_of(data, run_id):
    return {"WGS_DATA_DIR": str(data), "WGS_SAMPLE_ID": "SYN", "WGS_LANES": "1", "WGS_READS_PER_LANE": "2",
            "GPU_CHUNK_SIZE_READS": "500", "MSW_GFASTQ_BATCH": "500", "MSW_GFASTQ_SPAN_MB": "1", "WGS_RUN_ID": run_id}


def run(root, ds, tag, extra):
    (root / tag).mkdir()
    (root / ("ck_" + tag)).mkdir()
    args = ["--full-wgs", "--gpu", "--score-mode", "sw", "--reference", ds["reference"], "--window", WINDOW,
            "--checkpoint-dir", root / ("ck_" + tag)] + FLAGS + ["--alignments-out", root / tag,
                                                                  "--json", root / (tag + ".json")] + list(extra)
    return run_cli(args, env_of(root / "wgs", tag), root)


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from mini_parallel_amd.synthetic import write_wgs_dataset
    root = tmp_path_factory.mktemp("pileup_qual_cli")
    ds = write_wgs_dataset(str(root / "wgs"), bgzf=True, qual="illumina", lanes=1, reads_per_lane=2, reads_per_file=2000,
                           genome_bases=1 << 16, reverse_fraction=0.5, keep_batches=False)
    fa = open(ds["reference"]).read().split("\n", 1)[1]
    ds["genome"] = fa.replace("\n", "").encode()
    assert len(ds["genome"]) == 1 << 16
    ds["reads"], ds["quals"] = [], []
    for f in ds["files"]:
        lines = gzip.open(f, "rb").read().split(b"\n")
        ds["reads"].append(lines[1::4])
        ds["quals"].append(lines[3::4])
        assert len(lines[1::4]) == len(lines[3::4]) == 2000
    return root, ds


def files_of(root, ds, tag):
    out = {os.path.basename(p) + ".aln": open(root / tag / (os.path.basename(p) + ".aln"), "rb").read()
           for p in ds["files"]}
    for ext in (".mpu", ".var"):
        out[ext] = open(root / (tag + ext), "rb").read()
    return out


def test_counts_and_record_equal_the_oracle(dataset):
    from mini_parallel_amd import read_alignments, read_pileup
    root, ds = dataset
    r = run(root, ds, "q", ["--pileup-out", root / "q.mpu", "--pileup-min-baseq", MIN_BASEQ])
    assert r.returncode == 0, r.stdout + r.stderr
    want = po.new_counts(len(ds["genome"]))
    plain = po.new_counts(len(ds["genome"]))
    used = skipped = lowq = 0
    for path, reads, quals in zip(ds["files"], ds["reads"], ds["quals"]):
        x = read_alignments(root / "q" / (os.path.basename(path) + ".aln"))
        assert len(x.score) == len(reads)
        rows = [so.revcomp(rd) if st else rd for rd, st in zip(reads, x.strand)]
        rl = [len(rd) for rd in reads]
        u, s, low = pq.add(want, rows, rl, x.ref_pos, x.nm, x.cigars, x.strand, x.mapq, 0, quals, None, MIN_BASEQ)
        po.add(plain, rows, rl, x.ref_pos, x.nm, x.cigars, x.strand, x.mapq, 0)
        used, skipped, lowq = used + u, skipped + s, lowq + low
        assert x.strand.any() and not x.strand.all()
    # a threshold that matters for this dataset
    columns = int(plain[:, :5].sum())
    assert columns == int(want[:, :5].sum()) + lowq and 0.01 * columns < lowq < 0.5 * columns, (lowq, columns)
    got, file_used = read_pileup(root / "q.mpu")
    bad = np.argwhere(got != want)
    assert bad.size == 0, (bad[:8].tolist(), got[bad[:8, 0]].tolist(), want[bad[:8, 0]].tolist())
    assert file_used == used and used + skipped == 4000 and used > 3000
    rec = json.load(open(root / "q.json"))["pileup"]
    assert rec["min_baseq"] == MIN_BASEQ and rec["lowq_columns"] == lowq
    assert (rec["reads_used"], rec["reads_skipped"]) == (used, skipped)
    assert {k: rec[k] for k in ("covered", "depth_sum", "max_depth", "minority_ref")} == \
        po.summary(want, ds["genome"], rec["min_depth"])


def test_threshold_0_is_the_run_without_the_flag(dataset):
    root, ds = dataset
    outs = {}
    for tag, extra in (("none", []), ("zero", ["--pileup-min-baseq", 0])):
        r = run(root, ds, tag, ["--pileup-out", root / (tag + ".mpu"), "--variants-out", root / (tag + ".var")] + extra)
        assert r.returncode == 0, r.stdout + r.stderr
        outs[tag] = files_of(root, ds, tag)
        rec = json.load(open(root / (tag + ".json")))
        assert "min_baseq" not in rec["pileup"] and "lowq_columns" not in rec["pileup"]
    assert outs["none"] == outs["zero"] and len(outs["none"][".mpu"]) == 32 + (1 << 16) * 32
    # --variants-out alone takes the threshold too, and reports it with its calls
    r = run(root, ds, "vq", ["--variants-out", root / "vq.var", "--pileup-min-baseq", MIN_BASEQ])
    assert r.returncode == 0, r.stdout + r.stderr
    rec = json.load(open(root / "vq.json"))
    assert "pileup" not in rec and rec["variants"]["min_baseq"] == MIN_BASEQ and rec["variants"]["lowq_columns"] > 0


def test_run_id_depends_on_the_threshold(dataset):
    root, ds = dataset
    ids = {}
    for tag, extra in (("i0", ["--pileup-min-baseq", 0]), ("i30", ["--pileup-min-baseq", 30]), ("ip", [])):
        (root / tag).mkdir()
        (root / ("ck_" + tag)).mkdir()
        args = ["--full-wgs", "--gpu", "--score-mode", "sw", "--reference", ds["reference"], "--window", WINDOW,
                "--checkpoint-dir", root / ("ck_" + tag)] + FLAGS + ["--alignments-out", root / tag, "--pileup-out",
                                                                      root / (tag + ".mpu")] + extra
        e = env_of(root / "wgs", "")
        e.pop("WGS_RUN_ID")
        r = run_cli(args, e, root)
        assert r.returncode == 0, r.stdout + r.stderr
        cks = [f for f in os.listdir(root / ("ck_" + tag)) if f.startswith("checkpoint_wgs_")]
        assert len(cks) == 1
        ids[tag] = json.load(open(root / ("ck_" + tag) / cks[0]))["run_id"]
    assert ids["i0"] == ids["ip"] != ids["i30"]


def test_flag_needs_a_pileup_and_a_value_in_range(dataset):
    root, ds = dataset
    r = run(root, ds, "e1", ["--pileup-min-baseq", 20])
    assert r.returncode == 1 and "--pileup-min-baseq needs --pileup-out or --variants-out" in r.stderr, r.stderr
    r = run(root, ds, "e2", ["--pileup-out", root / "e2.mpu", "--pileup-min-baseq", 94])
    assert r.returncode == 1 and "--pileup-min-baseq must be 0..93" in r.stderr, r.stderr
    assert not (root / "e2.mpu").exists()
