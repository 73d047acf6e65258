"""``rustseq_mini --map``: what the argument parser refuses before any device
use, and the flags' place in --help.  CPU only."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mini_parallel_amd", "rustseq_mini")
SW = ["--full-wgs", "--gpu", "--score-mode", "sw", "--map"]


def run(args, env=None, cwd=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([CLI] + args, capture_output=True, text=True, env=e, cwd=cwd, timeout=60)


def test_help_lists_the_map_flags():
    out = run(["--help"]).stdout
    for flag in ("--map", "--seed-k", "--seed-max-occ", "--seed-band"):
        assert flag in out


@pytest.mark.parametrize("args,env,word", [
    (["--map", "-1", "ACGT", "-2", "ACGT", "--gpu"], {}, "--full-wgs --score-mode sw"),
    (["--full-wgs", "--gpu", "--map"], {}, "--full-wgs --score-mode sw"),                    # compat scoring
    (SW, {"MSW_GPU_INFLATE": "0"}, "host reader"),
    (SW + ["--scores-out", "scores"], {}, "--alignments-out"),
    (SW + ["--seed-k", "3"], {}, "--seed-k"),
    (SW + ["--seed-k=15"], {}, "--seed-k"),
    (SW + ["--seed-max-occ", "65"], {}, "--seed-max-occ"),
    (SW + ["--seed-max-occ", "0"], {}, "--seed-max-occ"),
    (SW + ["--seed-band", "0"], {}, "--seed-band"),
    (SW + ["--seed-k"], {}, "a value is required"),
])
def test_map_refusals(tmp_path, args, env, word):
    """Status 1 and one line, before a file is opened or a device touched."""
    r = run(args, env, tmp_path)
    assert r.returncode == 1 and word in r.stderr and len(r.stderr.strip().splitlines()) == 1, r.stderr
    assert os.listdir(tmp_path) == []
