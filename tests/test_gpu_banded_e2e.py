"""Banded end-to-end alignment (msw_e2e.hip) against a plain exact DP in Python
ints that restates include/msw.h, "Banded end-to-end alignment": the seeded
start row, -inf for every cell that does not exist, no floor, the best cell of
the last row and the canonical walk up to the start row.  Every comparison is
for equality: score, end cell, start cell and the ops one by one.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SCHEMES = {"lin": (2, -1, 0, 2, False), "aff": (2, -1, 3, 1, True),
           "allgap": (1, -9, 0, 1, False),   # a gap is cheaper than a mismatch: all-gap starts win
           "ext0": (2, -3, 4, 0, True),      # gap_extend = 0: open / extend ties
           "open30000": (1, -63, 30000, 1000, True)}   # the largest penalties: true values and sentinels far out
ACGT = np.frombuffer(b"ACGT", np.uint8)
LENS = (1, 2, 63, 64, 65, 128, 129, 200)
INF = float("-inf")
NONE = -(1 << 31)
UNPLACED = -(1 << 63)
MODES = {"score": 1, "coords": 3, "trace": 6}   # how many of the reference's six values the call returns


def ref_e2e(read, win, c, w, scheme):
    """(score, end_i, end_j, start_i, start_j, ops) of the section's recurrence and walk."""
    m, x, go, ge, aff = scheme
    goe = go + ge if aff else ge
    L, W = len(read), len(win)
    H = {(-1, j): 0 for j in range(-1, W) if abs(j + 1 - c) <= w} if c != UNPLACED else {}
    E, F = {}, {}
    for i in range(L if H else 0):
        for j in range(max(0, i + c - w), min(W, i + c + w + 1)):
            E[i, j] = max(H.get((i, j - 1), INF) - goe, E.get((i, j - 1), INF) - ge if aff else INF)
            F[i, j] = max(H.get((i - 1, j), INF) - goe, F.get((i - 1, j), INF) - ge if aff else INF)
            H[i, j] = max(H.get((i - 1, j - 1), INF) + (m if read[i] == win[j] else x), E[i, j], F[i, j])
    ends = [(H[L - 1, j], -j) for j in range(W) if H.get((L - 1, j), INF) > INF] if L else []
    if not ends:
        return NONE, -1, -1, -1, -1, []
    score, i, j, state, rev = max(ends)[0], L - 1, -max(ends)[1], "H", []
    while i >= 0:
        if state == "H":
            if H[i, j] == H.get((i - 1, j - 1), INF) + (m if read[i] == win[j] else x):
                rev.append(0)
                i, j = i - 1, j - 1
            else:
                state = "F" if H[i, j] == F[i, j] else "E"
        elif state == "F":
            rev.append(1)
            state = "H" if not aff or F[i, j] == H.get((i - 1, j), INF) - goe else "F"
            i -= 1
        else:
            rev.append(2)
            state = "H" if not aff or E[i, j] == H.get((i, j - 1), INF) - goe else "E"
            j -= 1
    assert sum(op != 2 for op in rev) == L and rev[-1] != 2     # M + I = L, never a leading D
    ops = []
    for op in reversed(rev):
        if ops and ops[-1] & 15 == op:
            ops[-1] += 16
        else:
            ops.append(16 | op)
    return score, L - 1, -max(ends)[1], 0, j + 1, ops


def scoring(name, coords=True):
    from mini_parallel_amd import Scoring
    m, x, go, ge, aff = SCHEMES[name]
    return Scoring(match=m, mismatch=x, gap_open=go, gap_extend=ge, affine=aff, want_coords=coords)


def derived(rng, G, a, L):
    """A read of length L sampled at G[a:] whose edits lie where local alignment clips: a
    substitution at an end base and, for longer reads, one base inserted or deleted 1-4 bases from an end."""
    d = 0 if L <= 12 else (1 if rng.integers(2) else -1)
    r = G[a:a + L - d].copy()
    if L > 12:
        k = int(rng.integers(1, 5)) if rng.integers(2) else len(r) - int(rng.integers(1, 5))
        r = np.insert(r, k, rng.choice(ACGT)) if d == 1 else np.delete(r, k)
    if L > 1:
        r[-int(rng.integers(2))] = ord("n")   # the first or the last base
    assert len(r) == L
    return r


@functools.lru_cache(maxsize=None)
def padded_batch(w, scheme):
    """37 (read, window, c) and their reference results: the lengths mixed, the centres at, around and
    beyond the sampled diagonal c0, off the window's left edge, and windows cut short."""
    rng = np.random.default_rng(1000 + w)
    G = rng.choice(ACGT, 700).astype(np.uint8)
    pairs = []
    for n, L in enumerate((LENS * 5)[:37]):
        c0 = int(rng.integers(0, 40))
        read = derived(rng, G, 100 + c0, L)
        if n % 6 == 5:                     # random reads: bases of the window's alphabet, and bases that never match
            read = rng.choice(ACGT if n % 12 == 11 else ACGT + 32, L).astype(np.uint8)
        c = (c0, c0 + w, c0 - w, c0 + w + 3, c0 - w - 2, -w - 3, -3, c0, c0)[n % 9]
        W = c0 + L + w + int(rng.integers(0, 6))
        if n % 9 == 6:                     # sampled three bases before the window's first: I in column 0
            read = derived(rng, G, 97, L)
        if n % 9 == 7:
            W = max(0, L - 1 + c - w)      # row L - 1 starts at column L - 1 + c - w: no cell (W = 0 for short reads)
        if n % 9 == 8:
            W = c0 + L - 1                 # the last base's own column is cut off
        pairs.append((read, G[100:100 + W], c))
    return pairs, [ref_e2e(r, x, c, w, SCHEMES[scheme]) for r, x, c in pairs]


def run_padded(ctx, pairs, w, scheme, mode, **kw):
    from mini_parallel_amd import pack_batch
    R, rl, Wn, wl = pack_batch([bytes(r) for r, _, _ in pairs], [bytes(x) for _, x, _ in pairs])
    diag = np.array([c for _, _, c in pairs], np.int32)
    return ctx.align_batch_banded(R, rl, Wn, wl, diag, w, scoring(scheme, mode != "score"), trace=mode == "trace", **kw)


def check(got, want, mode, origin=None):
    for p, t in enumerate(want):
        o = int(origin[p]) if origin is not None and t[0] != NONE else 0
        exp = [t[0], t[1], t[2] - o, t[3], t[4] - o, t[5]][:MODES[mode]]
        have = [int(a[p]) for a in got[:min(MODES[mode], 5)]] + ([list(got[5][p])] if mode == "trace" else [])
        assert have == exp, (p, have, exp)
        if mode == "trace":
            assert int(got[5].n_cigar[p]) == len(t[5])


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("scheme", ["lin", "aff"])
@pytest.mark.parametrize("w", [0, 1, 15, 16, 31, 32, 63])
def test_matches_reference(gpu_ctx, w, scheme, mode):
    pairs, want = padded_batch(w, scheme)
    assert any(t[0] == NONE for t in want) and any(NONE < t[0] < 0 for t in want)
    assert any(1 in [op & 15 for op in t[5][:2]] for t in want) or w < 3   # I at the window's first column
    check(run_padded(gpu_ctx, pairs, w, scheme, mode, end_to_end=True), want, mode)


@pytest.mark.parametrize("scheme,w", [("allgap", 15), ("allgap", 32), ("ext0", 16), ("ext0", 63)])
def test_gap_heavy_schemes(gpu_ctx, scheme, w):
    pairs, want = padded_batch(w, scheme)
    check(run_padded(gpu_ctx, pairs, w, scheme, "trace", end_to_end=True), want, "trace")


@pytest.mark.parametrize("scheme", ["lin", "aff"])
@pytest.mark.parametrize("w", [7, 32])
def test_genome_form(gpu_ctx, w, scheme):
    """Diagonals at 0, negative, within w of the genome's end and past it, one unplaced read; the
    implied window is the local banded call's."""
    from mini_parallel_amd import pack_batch
    rng = np.random.default_rng(50 + w)
    G = rng.choice(ACGT, 900).astype(np.uint8)
    n = len(G)
    reads, diag = [], []
    for k in range(12):
        L = LENS[2 + k % 6]
        c = (0, 2, -3, -w - 5, n - L, n - L + 3, n - L - w + 1, n - 1, n + w + 2, UNPLACED, 300, 400 + w)[k]
        reads.append(derived(rng, G, max(0, min(c, n - L - 1)), L))
        diag.append(c)
    R, rl, _, _ = pack_batch([bytes(r) for r in reads], [b"A"] * len(reads))
    g = gpu_ctx.load_genome(bytes(G))
    try:
        got = gpu_ctx.align_reads_banded(g, R, rl, np.array(diag, np.int64), w, scoring(scheme), trace=True,
                                         end_to_end=True)
        local = gpu_ctx.align_reads_banded(g, R, rl, np.array(diag, np.int64), w, scoring(scheme), trace=True)
    finally:
        g.close()
    want = [ref_e2e(r, G, c, w, SCHEMES[scheme]) for r, c in zip(reads, diag)]
    assert sum(t[0] == NONE for t in want) >= 2 and sum(t[0] > 0 for t in want) >= 6
    check(got, want, "trace", origin=[max(0, c - w) for c in diag])
    assert np.array_equal(got[-2], local[-2]) and np.array_equal(got[-1], local[-1])
    assert int(got[-2][9]) == -1 and int(got[-1][9]) == 0


def test_trace_limit_and_sentinel_headroom(gpu_ctx):
    """A traced read at the LDS bound of 1008 rows and MSW_E_RANGE one past it; score-only at 3000 rows,
    w = 63 and the largest penalties: a deletion the score has to pay for, a band off the read's diagonal
    (a true score below -100,000) and one no path reaches, its cells made of sentinels for 3000 rows."""
    from mini_parallel_amd import MswError
    from mini_parallel_amd._lib import MSW_E_RANGE
    rng = np.random.default_rng(9)
    G = rng.choice(ACGT, 3300).astype(np.uint8)
    pairs = [(derived(rng, G, 40, 1008), G[:1100], 38), (derived(rng, G, 5, 100), G[:200], 5)]
    check(run_padded(gpu_ctx, pairs, 16, "aff", "trace", end_to_end=True),
          [ref_e2e(r, x, c, 16, SCHEMES["aff"]) for r, x, c in pairs], "trace")
    with pytest.raises(MswError) as e:
        run_padded(gpu_ctx, [(G[:1009], G[:1100], 0)], 16, "aff", "trace", end_to_end=True)
    assert e.value.code == MSW_E_RANGE
    long_read = np.concatenate([G[10:1500], G[1504:3014]])   # a 4-base deletion: 30000 + 4 x 1000
    pairs = [(long_read, G[:3200], c) for c in (10, -49, 80)] + [(G[:3000], G[70:3200], -70)]
    want = [ref_e2e(r, x, c, 63, SCHEMES["open30000"]) for r, x, c in pairs]
    assert want[0][0] == 3000 - 34000 and want[2][0] < -100000 and want[3][0] == NONE
    check(run_padded(gpu_ctx, pairs, 63, "open30000", "score", end_to_end=True), want, "score")


def test_keyword_off_is_the_local_call(gpu_ctx):
    pairs, _ = padded_batch(16, "aff")
    for a, b in zip(run_padded(gpu_ctx, pairs, 16, "aff", "trace", end_to_end=False),
                    run_padded(gpu_ctx, pairs, 16, "aff", "trace")):
        assert [list(x) for x in a] == [list(x) for x in b] if isinstance(a, list) else np.array_equal(a, b)
