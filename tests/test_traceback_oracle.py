"""CPU checks of the traceback contract (include/msw.h, "Traceback"):

 * tests/traceback_oracle.py, the full-matrix restatement the GPU tests compare
   against, agrees with the C oracle on score and best cell, gives the
   hand-worked answers, and its alignments have the properties the rule implies;
 * the feature's surface exists: header, library exports, binding struct, CLI flag.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import traceback_oracle as tbo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "msw.h")
CLI = os.path.join(ROOT, "mini_parallel_amd", "rustseq_mini")

# (match, mismatch, gap_open, gap_extend, affine)
SCHEMES = [
    (2, -1, 0, 2, False),    # the reference's constants
    (2, -1, 3, 1, True),     # config 3
    (2, -1, 0, 0, False),    # gap = 0
    (3, 0, 0, 2, False),     # mismatch = 0
    (2, -1, 4, 0, True),     # gap_extend = 0
    (2, 0, 0, 0, True),      # free gaps, free mismatches
    (64, 0, 10, 1, True),    # match 64 / mismatch 0
    (1, -3, 10, 1, True),
]


def random_pair(rng, max_m=24, max_n=40, alphabet=b"ACGT"):
    n = int(rng.integers(1, max_n + 1))
    w = rng.choice(np.frombuffer(alphabet, np.uint8), n)
    if rng.random() < 0.5:  # a mutated slice of the window
        a = int(rng.integers(0, n))
        r = list(w[a:a + int(rng.integers(1, max_m + 1))])
        for _ in range(int(rng.integers(0, 4))):
            k = int(rng.integers(0, len(r) + 1))
            what = rng.integers(0, 3)
            if what == 0 and r:
                r[min(k, len(r) - 1)] = int(rng.choice(np.frombuffer(alphabet, np.uint8)))
            elif what == 1:
                r[k:k] = [int(x) for x in rng.choice(np.frombuffer(alphabet, np.uint8), int(rng.integers(1, 4)))]
            elif len(r) > 3:
                del r[k:k + int(rng.integers(1, 3))]
        r = np.array(r[:max_m] or [w[0]], np.uint8)
    else:
        r = rng.choice(np.frombuffer(alphabet, np.uint8), int(rng.integers(1, max_m + 1)))
    return np.ascontiguousarray(r, np.uint8), np.ascontiguousarray(w, np.uint8)


def check_properties(res, r, w, scheme):
    """What the rule implies for every scheme the header allows."""
    match, mismatch, go, ge, affine = scheme
    score, (ei, ej), (si, sj), ops = res
    if score == 0:
        assert (ei, ej) == (-1, -1) and (si, sj) == (-1, -1) and len(ops) == 0
        return
    assert len(ops) >= 1
    assert (ops[0] & 15) == tbo.M and (ops[-1] & 15) == tbo.M, tbo.cigar_text(ops)
    assert all((o >> 4) >= 1 and (o & 15) in (0, 1, 2) for o in ops)
    assert all((a & 15) != (b & 15) for a, b in zip(ops, ops[1:])), tbo.cigar_text(ops)
    assert 0 <= si <= ei < len(r) and 0 <= sj <= ej < len(w)
    assert tbo.consumed(ops) == (ei - si + 1, ej - sj + 1)
    total, last = tbo.rescore(ops, r, w, (si, sj), match, mismatch, go, ge, affine)
    assert total == score and last == (ei, ej)


@pytest.mark.parametrize("scheme", SCHEMES[:4], ids=lambda s: "m%d_x%d_o%d_e%d_%s" % (s[:4] + ("aff" if s[4] else "lin",)))
def test_restatement_matches_c_oracle(oracle, scheme):
    match, mismatch, go, ge, affine = scheme
    from mini_parallel_amd import pack_batch
    rng = np.random.default_rng(11)
    pairs = [random_pair(rng) for _ in range(150)]
    R, rl, W, wl = pack_batch([r.tobytes() for r, _ in pairs], [w.tobytes() for _, w in pairs])
    s, ei, ej = oracle.sw_batch(R, rl, W, wl, match=match, mismatch=mismatch, gap_open=go, gap_extend=ge,
                                affine=affine)
    for p, (r, w) in enumerate(pairs):
        res = tbo.align(r, w, match, mismatch, go, ge, affine)
        assert (res[0], res[1][0], res[1][1]) == (int(s[p]), int(ei[p]), int(ej[p])), p


@pytest.mark.parametrize("scheme", SCHEMES, ids=lambda s: "m%d_x%d_o%d_e%d_%s" % (s[:4] + ("aff" if s[4] else "lin",)))
def test_properties(scheme):
    rng = np.random.default_rng(5)
    for k in range(120):
        r, w = random_pair(rng, alphabet=b"ACGT" if k % 3 else b"AC")
        check_properties(tbo.align(r, w, *scheme), r, w, scheme)


LIN, AFF = (2, -1, 0, 2, False), (2, -1, 3, 1, True)
KATS = [
    # homopolymer: every diagonal of length 4 scores 8; the best cell is the
    # first in row-major order, (3, 3), and the walk is diagonal all the way
    ("AAAA", "AAAAAA", LIN, 8, (3, 3), (0, 0), "4M"),
    ("AAAA", "AAAAAA", AFF, 8, (3, 3), (0, 0), "4M"),
    # CA x 4 in the read against CA x 3: the walk keeps to the diagonal from the
    # right for as long as it is optimal, so the 2-base insertion lands at the
    # left edge of the repeat.  14 matches - 2 * 2 = 24; affine 28 - (3 + 2) = 23
    ("GGTTCACACACAGGTT", "GGTTCACACAGGTT", LIN, 24, (15, 13), (0, 0), "4M2I10M"),
    ("GGTTCACACACAGGTT", "GGTTCACACAGGTT", AFF, 23, (15, 13), (0, 0), "4M2I10M"),
    # the mirror image: a 2-base deletion.  12 matches - 4 = 20; affine 24 - 5 = 19
    ("GGTTCACAGGTT", "GGTTCACACAGGTT", LIN, 20, (11, 13), (0, 0), "4M2D8M"),
    ("GGTTCACAGGTT", "GGTTCACACAGGTT", AFF, 19, (11, 13), (0, 0), "4M2D8M"),
    # a mismatch inside: 7 matches - 1 = 13 beats either flank alone (6 and 8)
    ("ACGTTGCA", "TTACGATGCATT", LIN, 13, (7, 9), (0, 2), "8M"),
    # nothing in common: score 0, no alignment
    ("AAAA", "CCCC", LIN, 0, (-1, -1), (-1, -1), "*"),
    # case-sensitive byte equality, N == N
    ("acgtN", "ACGTacgtN", LIN, 10, (4, 8), (0, 4), "5M"),
]


@pytest.mark.parametrize("read,win,scheme,score,end,start,cigar", KATS)
def test_known_answers(read, win, scheme, score, end, start, cigar):
    res = tbo.align(read, win, *scheme)
    assert (res[0], res[1], res[2], tbo.cigar_text(res[3])) == (score, end, start, cigar)
    check_properties(res, tbo._bytes(read), tbo._bytes(win), scheme)


def test_restatement_is_fast_enough():
    """The largest traced shape, 384 x 4096, within seconds."""
    import time
    rng = np.random.default_rng(3)
    w = rng.choice(np.frombuffer(b"ACGT", np.uint8), 4096)
    r = w[3712:].copy()
    t0 = time.time()
    res = tbo.align(r, w, *AFF)
    assert time.time() - t0 < 10.0
    assert res[:3] == (768, (383, 4095), (0, 3712)) and tbo.cigar_text(res[3]) == "384M"


# ---- the feature's surface (fails before the feature exists) ----
def test_header_declares_trace_calls():
    text = open(HEADER).read()
    for name in ("msw_trace_batch_device", "msw_align_batch_trace"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
    assert re.search(r"\}\s*msw_trace_t\s*;", text)


def test_library_exports_trace_calls():
    from mini_parallel_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "libmsw.so not built (run __graft_entry__.build())"
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r" T (msw_[a-z0-9_]+)$", out, re.M))
    assert {"msw_trace_batch_device", "msw_align_batch_trace"} <= exported
    assert {"msw_trace_batch_device", "msw_align_batch_trace"} <= set(_lib.EXPORTED)


def test_trace_struct_layout():
    from mini_parallel_amd import _lib
    assert ctypes.sizeof(_lib.TraceT) == 40
    assert _lib.TraceT.cigar_stride.offset == 32
    assert ctypes.sizeof(_lib.ScoringT) == 24 and ctypes.sizeof(_lib.OutT) == 24  # unchanged


def test_cigar_string():
    from mini_parallel_amd import cigar_string
    assert cigar_string(np.array([12 << 4, 1 << 4 | 1, 30 << 4], np.uint32)) == "12M1I30M"
    assert cigar_string([4 << 4, 2 << 4 | 2, 8 << 4]) == "4M2D8M"
    assert cigar_string([]) == "*"


def test_cli_help_lists_cigar():
    assert os.access(CLI, os.X_OK), "rustseq_mini not built (__graft_entry__.build())"
    out = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "--cigar" in out.stdout


def test_cli_cigar_needs_sw_mode():
    out = subprocess.run([CLI, "-1", "ACGT", "-2", "ACGT", "-g", "--cigar"], capture_output=True, text=True,
                         timeout=60)
    assert out.returncode != 0 and "--cigar" in out.stderr
