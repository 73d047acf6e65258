"""Inputs of tests/test_gpu_trace_long_paths.py, as plain functions.

TEST INFRASTRUCTURE ONLY.  tests/test_trace_long_inputs.py builds the same
inputs without a GPU and asserts, from tests/traceback_oracle.py alone, the
property each GPU test relies on (an op count past 4,096, an end column, a gap
over rows 383 / 384, a walk through every strip), so a GPU test that passes
has run the branch it names.

A strip of sw_trace_long_kernel is 64 R rows, R = min(6, ceil(max_rows / 64));
strips of 384 rows whenever the call's longest read has more than 320 bases.
"""
import numpy as np

from test_gpu_trace_long import SCHEMES as BASE_SCHEMES, junk, planted, window

SCHEMES = dict(BASE_SCHEMES,                       # the values of tests/test_gpu_traceback.py
               lin_gap0=(2, -1, 0, 0, False), lin_mismatch0=(3, 0, 0, 2, False),
               aff_open10=(2, -1, 10, 1, True), aff_m64_x0=(64, 0, 10, 1, True),
               aff_open0=(2, -1, 0, 1, True))
TIE_SCHEMES = ("lin", "aff", "aff_ext0", "lin_gap0", "lin_mismatch0", "aff_open10", "aff_m64_x0")
STRIP = 384
LDS_OPS = 4096      # kTraceLongLdsOps: a larger op bound puts the reverse ops in the block's scratch

EMPTY = np.zeros(0, np.uint8)
AC = np.frombuffer(b"AC", np.uint8)
CGT = np.frombuffer(b"CGT", np.uint8)
cat = np.concatenate


def text(t):
    return np.frombuffer(t, np.uint8).copy()


def rows_per_lane(pairs):
    m = max(len(r) for r, _ in pairs)
    return min(6, max(1, (m + 63) // 64))


def spread(w, m):
    """m rows of junk with the bytes of w at evenly spaced rows, the first in row 0 and the last in row m - 1."""
    r = junk(m)
    r[np.linspace(0, m - 1, len(w)).round().astype(np.int64)] = w
    return r


# --- A: more ops than LDS holds ----------------------------------------------------------------
OPS_SCHEMES = ("lin_gap0", "aff_open0")


def interleaved(m):
    """A random read of m bases against itself with a junk byte after every base: 1M1D1M ... 1M,
    2 m - 1 ops from (0, 0) to (m - 1, 2 m - 2) wherever a deletion costs less than a match gains."""
    r = window(m, m)
    w = junk(2 * m)
    w[0::2] = r
    return r, w


def reuse_batch():
    """4,199 ops, a few dozen, none (empty read), 4,095, none (score 0): one block's op buffer in turn."""
    w = window(31, 900)
    return [interleaved(2100), (planted(5, w, 150, 700), w), (EMPTY, w), interleaved(2048), (junk(8), w)]


# --- B: every rows-per-lane instance ------------------------------------------------------------
ROWS_PER_LANE = [(1, 4097, 1), (64, 4100, 1), (65, 4097, 2), (128, 4130, 2), (193, 4161, 4), (256, 4200, 4),
                 (257, 4104, 5), (320, 4112, 5), (321, 4097, 6), (384, 4105, 6)]


def rows_per_lane_pairs(m, n):
    """A read that ends in the window's last columns, one that ends before column 64, a random one, an empty one."""
    if m == 1:
        w = np.random.default_rng(n).choice(CGT, n).astype(np.uint8)
        w[n - 1] = ord("A")             # the only A
        return [(text(b"A"), w), (w[5:6].copy(), w), (text(b"G"), w), (EMPTY, w)]
    w = window(m * 7 + n, n)
    k = min(40, m)
    return [(planted(m, w, n - m - 1, m), w), (cat([junk(m - k), w[10:10 + k]]), w), (window(m + n, m), w), (EMPTY, w)]


GENOME_POS, GENOME_WANT = [400, 1000, 8000], [4500, 4500, 4500]   # the last window is clipped at the genome end


def genome_reads(m):
    g = window(123, 9000)
    return g, [planted(1, g, 700, m), planted(2, g, 3100, m), planted(3, g, 8300, m)]


# --- C: narrow rectangles under several strips --------------------------------------------------
NARROW_COLS = (1, 8, 16, 17, 40, 63, 64, 65, 127, 128)
NARROW_ROWS = (500, 769, 1200)


def narrow_pairs(rows=NARROW_ROWS, win_len=300):
    """[(cols, (read, window))]: junk, then the window's first `cols` bytes in the read's last rows: the best
    cell is (m - 1, cols - 1), in the last strip, and every strip above is filled `cols` columns wide."""
    w = window(77, 300)[:win_len]
    return [(e, (cat([junk(m - e), w[:e]]), w)) for m in rows for e in NARROW_COLS if e <= win_len]


def narrow_crossing_pairs():
    """Under free gaps: the window's first `cols` bytes spread over all rows, junk between them.  The walk
    goes from the last row to row 0 through every strip, inside a rectangle that narrows from `cols`."""
    w = window(77, 300)
    return [(e, (spread(w[:e], m), w)) for m in NARROW_ROWS for e in NARROW_COLS if e > 1]


# --- D: ties at the strip boundary --------------------------------------------------------------
def homopolymers():
    a = lambda n: np.full(n, ord("A"), np.uint8)
    return [(a(800), a(900)), (a(800), a(500))]


def dinucleotide_slips():
    """AC x 600 against a window with an extra A after 382 and an extra C after 983 bases, and the mirror."""
    r = text(b"AC" * 600)
    w = text(b"AC" * 191 + b"A" + b"AC" * 300 + b"C" + b"AC" * 200)
    return [(r, w), (w.copy(), r.copy())]


GAP_RUN = 20


def gap_run_pairs():
    """[(op, first read row of the window's A run, (read, window))]: a CGT window with one run of 20 A; the
    read carries the run 8 bases longer (I) or shorter (D).  Any placement of the gap inside the run ties;
    the canonical one is the run's left end: I over rows [row, row + 8), D walked in row - 1."""
    w = np.random.default_rng(17).choice(CGT, 1000).astype(np.uint8)
    c0 = 500
    w[c0:c0 + GAP_RUN] = ord("A")
    out = []
    for op, run, starts in (("I", GAP_RUN + 8, (380, 384)), ("D", GAP_RUN - 8, (384, 385))):
        for row in starts:
            r = cat([w[c0 - row:c0], np.full(run, ord("A"), np.uint8), w[c0 + GAP_RUN:c0 + GAP_RUN + 400]])
            out.append((op, row, (r, w)))
    return out


def read_twice():
    u = window(41, 800)
    return [(u, cat([u, window(42, 100), u]))]


def low_entropy_pairs():
    out = []
    for m, n in ((769, 1000), (1153, 1300)):
        w = np.random.default_rng(m).choice(AC, n).astype(np.uint8)
        out.append((planted(m, w, (n - m) // 2, m), w))
    return out


# --- E: the bounds ------------------------------------------------------------------------------
LIMIT = 32767


def wide_pair(m):
    """The last bytes of a 32,767-byte window, one junk base in the middle of the read."""
    w = window(5, LIMIT)
    r = w[LIMIT - m:].copy()
    r[m // 2] = ord("n")
    return r, w


def tall_pair(m=LIMIT):
    """Under free gaps: 300 window bytes spread over m rows; the walk visits every strip."""
    w = window(6, 300)
    return spread(w, m), w
