#!/usr/bin/env python3
"""End-to-end A/B of `--variants-out`: the run of
tools/wgs_pileup_ab.py with its pileup -- 2 BGZF lane files x 250,000 reads,
half of them reverse-complemented, 4 Mbase genome, `--full-wgs --both-strands
--map --mapq --alignments-out --pileup-out`, affine, `--window 300`.  Runs,
alternated `--reps` times:

    old           another build's rustseq_mini (--old-cli), without the flag
    new           this build without the flag
    new_variants  this build with --variants-out

and prints / writes one JSON line per run, then one line saying whether the
.aln and .mpu files of the three are the same bytes.
"""
import argparse
import filecmp
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old-cli", default="", help="rustseq_mini of the build to compare with (skipped when empty)")
    ap.add_argument("--reads-per-file", type=int, default=250000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--reverse", action="store_true", help="run the three in the opposite order within a repetition")
    ap.add_argument("--out", default="wgs_variants_ab.jsonl")
    a = ap.parse_args()
    from mini_parallel_amd.synthetic import write_wgs_dataset
    new_cli = os.path.join(ROOT, "mini_parallel_amd", "rustseq_mini")
    top = tempfile.mkdtemp(prefix="variants_ab_")
    data = os.path.join(top, "wgs")
    ds = write_wgs_dataset(data, lanes=1, reads_per_lane=2, reads_per_file=a.reads_per_file, genome_bases=1 << 22,
                           keep_batches=False, bgzf=True, reverse_fraction=0.5, workers=2)
    runs = [("new", new_cli, False), ("new_variants", new_cli, True)]
    if a.old_cli:
        runs.insert(0, ("old", os.path.abspath(a.old_cli), False))
    if a.reverse:
        runs.reverse()
    kept = {}
    with open(a.out, "w") as out:
        for rep in range(a.reps):
            for name, cli, variants in runs:
                wd = os.path.join(top, "%s_%d" % (name, rep))
                os.makedirs(wd)
                env = dict(os.environ, WGS_DATA_DIR=data, WGS_SAMPLE_ID="SYN", WGS_LANES="1", WGS_READS_PER_LANE="2",
                           GPU_CHUNK_SIZE_READS="65536", WGS_RUN_ID="%s%d" % (name, rep))
                cmd = [cli, "--full-wgs", "--gpu", "--score-mode", "sw", "--reference", ds["reference"], "--window", "300",
                       "--checkpoint-dir", wd, "--json", os.path.join(wd, "rec.json"), "--num-gpus", "1",
                       "--gap-model", "affine", "--both-strands", "--alignments-out", wd, "--map", "--mapq",
                       "--pileup-out", os.path.join(wd, "run.mpu")]
                if variants:
                    cmd += ["--variants-out", os.path.join(wd, "run.var")]
                r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=wd, timeout=300)
                if r.returncode != 0:
                    raise SystemExit("%s rep %d: rc %d\n%s" % (name, rep, r.returncode, r.stderr[-3000:]))
                rec = json.load(open(os.path.join(wd, "rec.json")))
                row = {"run": name, "rep": rep, "wall_ms": round(rec["wall_ms"], 2),
                       "reads_per_s": int(rec["reads_per_second"]), "setup_ms": round(rec["setup_ms"], 1),
                       "teardown_ms": round(rec["teardown_ms"], 1), "total_score": rec["total_score"],
                       "pileup_ms": round(rec["pileup"]["pileup_ms"], 1), "variants": rec.get("variants")}
                if row["variants"]:
                    row["variants"]["path"] = os.path.basename(row["variants"]["path"])  # not the temporary directory
                line = json.dumps(row)
                print(line, flush=True)
                out.write(line + "\n")
                out.flush()
                if rep == 0:
                    kept[name] = wd
                else:
                    shutil.rmtree(wd)
        files = sorted(f for f in os.listdir(kept["new"]) if f.endswith(".aln") or f.endswith(".mpu"))
        same = {other: bool(files) and all(filecmp.cmp(os.path.join(kept["new"], f), os.path.join(kept[other], f),
                                                       shallow=False) for f in files)
                for other in kept if other != "new"}
        line = json.dumps({"files": files, "equal_to_new": same,
                           "bytes": [os.path.getsize(os.path.join(kept["new"], f)) for f in files]})
        print(line, flush=True)
        out.write(line + "\n")
    shutil.rmtree(top)


if __name__ == "__main__":
    main()
