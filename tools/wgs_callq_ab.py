#!/usr/bin/env python3
"""End-to-end A/B of `--call-baseq`: the run of
tools/wgs_variants_ab.py -- 2 BGZF lane files x 250,000 reads, half of them
reverse-complemented, 4 Mbase genome, `--full-wgs --both-strands --map --mapq
--alignments-out --pileup-out --variants-out`, affine, `--window 300` -- with
quality strings of `--qual` kind ("illumina" by default).  Runs, alternated
`--reps` times:

    old         another build's rustseq_mini (--old-cli), without the flag
    new         this build without the flag
    new_callq   this build with --call-baseq --qsum-out

and prints / writes one JSON line per run (wall time, and the phases after the
clock: pileup_ms, variants_ms), then one line saying whether the .aln, .mpu
and -- between the runs without the flag -- .var files are the same bytes.
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
    ap.add_argument("--qual", default="illumina", choices=["I", "binned", "illumina"])
    ap.add_argument("--out", default="wgs_callq_ab.jsonl")
    a = ap.parse_args()
    from mini_parallel_amd.synthetic import write_wgs_dataset
    new_cli = os.path.join(ROOT, "mini_parallel_amd", "rustseq_mini")
    top = tempfile.mkdtemp(prefix="callq_ab_")
    data = os.path.join(top, "wgs")
    ds = write_wgs_dataset(data, lanes=1, reads_per_lane=2, reads_per_file=a.reads_per_file, genome_bases=1 << 22,
                           keep_batches=False, bgzf=True, reverse_fraction=0.5, workers=2, qual=a.qual)
    runs = [("new", new_cli, False), ("new_callq", new_cli, True)]
    if a.old_cli:
        runs.insert(0, ("old", os.path.abspath(a.old_cli), False))
    kept = {}
    with open(a.out, "w") as out:
        for rep in range(a.reps):
            for name, cli, callq in runs:
                wd = os.path.join(top, "%s_%d" % (name, rep))
                os.makedirs(wd)
                env = dict(os.environ, WGS_DATA_DIR=data, WGS_SAMPLE_ID="SYN", WGS_LANES="1", WGS_READS_PER_LANE="2",
                           GPU_CHUNK_SIZE_READS="65536", WGS_RUN_ID="%s%d" % (name, rep))
                cmd = [cli, "--full-wgs", "--gpu", "--score-mode", "sw", "--reference", ds["reference"], "--window", "300",
                       "--checkpoint-dir", wd, "--json", os.path.join(wd, "rec.json"), "--num-gpus", "1",
                       "--gap-model", "affine", "--both-strands", "--alignments-out", wd, "--map", "--mapq",
                       "--pileup-out", os.path.join(wd, "run.mpu"), "--variants-out", os.path.join(wd, "run.var")]
                if callq:
                    cmd += ["--call-baseq", "--qsum-out", os.path.join(wd, "run.mqs")]
                r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=wd, timeout=300)
                if r.returncode != 0:
                    raise SystemExit("%s rep %d: rc %d\n%s" % (name, rep, r.returncode, r.stderr[-3000:]))
                rec = json.load(open(os.path.join(wd, "rec.json")))
                v = rec["variants"]
                row = {"run": name, "rep": rep, "qual": a.qual, "wall_ms": round(rec["wall_ms"], 2),
                       "reads_per_s": int(rec["reads_per_second"]), "setup_ms": round(rec["setup_ms"], 1),
                       "teardown_ms": round(rec["teardown_ms"], 1), "total_score": rec["total_score"],
                       "pileup_ms": round(rec["pileup"]["pileup_ms"], 1), "variants_ms": round(v["variants_ms"], 1),
                       "records": v["records"], "het": v["het"], "hom": v["hom"],
                       "baseq_weighted": bool(v.get("baseq_weighted", False))}
                line = json.dumps(row)
                print(line, flush=True)
                out.write(line + "\n")
                out.flush()
                if rep == 0:
                    kept[name] = wd
                else:
                    shutil.rmtree(wd)

        def same(other, exts):
            files = sorted(f for f in os.listdir(kept["new"]) if f.endswith(exts))
            return bool(files) and all(filecmp.cmp(os.path.join(kept["new"], f), os.path.join(kept[other], f),
                                                   shallow=False) for f in files)

        line = json.dumps({"aln_mpu_equal_to_new": {o: same(o, (".aln", ".mpu")) for o in kept if o != "new"},
                           "var_equal_to_new": {o: same(o, (".var",)) for o in kept if o not in ("new", "new_callq")}})
        print(line, flush=True)
        out.write(line + "\n")
    shutil.rmtree(top)


if __name__ == "__main__":
    main()
