"""Banded Smith-Waterman (msw_band.hip) against a plain masked DP: cells exist
exactly as include/msw.h, "Banded alignment", defines them, integers
throughout, and the canonical walk on the banded H, E and F.  Every comparison
is exact: score, end cell, start cell, n_cigar and the ops one by one.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SCHEMES = {"lin": (2, -1, 0, 2, False), "aff": (2, -1, 3, 1, True)}
ACGT = np.frombuffer(b"ACGT", np.uint8)
NEG = -(1 << 40)
UNPLACED = -(1 << 63)


def ref_band(read, win, c, w, scheme):
    """(score, end_i, end_j, start_i, start_j, ops) of the banded recurrence."""
    m, x, go, ge, aff = scheme
    goe = go + ge if aff else ge
    L, W = len(read), len(win)
    H, E, F = {}, {}, {}
    best = (0, -1, -1)
    for i in range(L):
        for j in range(max(0, i + c - w), min(W, i + c + w + 1)):
            d = H.get((i - 1, j - 1), 0) + (m if read[i] == win[j] else x)
            e = max(H[i, j - 1] - goe, E[i, j - 1] - ge if aff else NEG) if (i, j - 1) in H else NEG
            f = max(H[i - 1, j] - goe, F[i - 1, j] - ge if aff else NEG) if (i - 1, j) in H else NEG
            H[i, j], E[i, j], F[i, j] = max(0, d, e, f), e, f
            if H[i, j] > best[0]:
                best = (H[i, j], i, j)
    score, i, j = best
    rev, state, si, sj = [], "H", -1, -1
    while score and (i, j) in H:
        if state == "H":
            if H[i, j] == 0:
                break
            if H[i, j] == H.get((i - 1, j - 1), 0) + (m if read[i] == win[j] else x):
                rev.append(0)
                si, sj, i, j = i, j, i - 1, j - 1
            else:
                state = "F" if H[i, j] == F[i, j] else "E"
        elif state == "F":
            rev.append(1)
            state = "H" if not aff or F[i, j] == H[i - 1, j] - goe else "F"
            i -= 1
        else:
            rev.append(2)
            state = "H" if not aff or E[i, j] == H[i, j - 1] - goe else "E"
            j -= 1
    ops = []
    for op in reversed(rev):
        if ops and ops[-1] & 15 == op:
            ops[-1] += 16
        else:
            ops.append(16 | op)
    return score, best[1], best[2], si, sj, ops


def scoring(name, coords=True):
    from mini_parallel_amd import Scoring
    m, x, go, ge, aff = SCHEMES[name]
    return Scoring(match=m, mismatch=x, gap_open=go, gap_extend=ge, affine=aff, want_coords=coords)


def mutate(rng, seg):
    """seg with a few substitutions, and for longer reads one short insertion or deletion."""
    r = seg.copy()
    if len(r) > 4:
        r[rng.integers(0, len(r), max(1, len(r) // 20))] = ord("n")
    if len(r) > 12:
        k, n = int(rng.integers(3, len(r) - 3)), int(rng.integers(1, 4))
        r = np.concatenate([r[:k], rng.choice(ACGT, n).astype(np.uint8), r[k:]] if rng.integers(2)
                           else [r[:k], r[k + n:]])
    return r


def run(ctx, form, pairs, w, scheme, trace=True, **kw):
    """pairs: (read, window, c); in the genome form every window is the one genome and c its coordinate."""
    from mini_parallel_amd import pack_batch
    reads = [bytes(r) for r, _, _ in pairs]
    diag = np.array([c for _, _, c in pairs], np.int64)
    if form == "genome":
        R, rl, _, _ = pack_batch(reads, [b"A"] * len(pairs))
        g = ctx.load_genome(bytes(pairs[0][1]))
        try:
            return ctx.align_reads_banded(g, R, rl, diag, w, scoring(scheme), trace=trace, **kw)
        finally:
            g.close()
    R, rl, Wn, wl = pack_batch(reads, [bytes(x) for _, x, _ in pairs])
    return ctx.align_batch_banded(R, rl, Wn, wl, diag, w, scoring(scheme), trace=trace, **kw)


def check(got, form, pairs, w, scheme, trace=True):
    for p, (r, win, c) in enumerate(pairs):
        unplaced = c == UNPLACED
        want = ref_band(r, win, 0 if unplaced else c, -1 if unplaced else w, SCHEMES[scheme])
        o = max(0, c - w) if form == "genome" and not unplaced else 0
        exp = [want[0], want[1], want[2] - o if want[0] else -1]
        if trace:
            exp += [want[3], want[4] - o if want[0] else -1, want[5]]
            assert int(got[5].n_cigar[p]) == len(want[5]), (p, "n_cigar")
        have = [int(a[p]) for a in got[:3]] + ([int(got[3][p]), int(got[4][p]), list(got[5][p])] if trace else [])
        assert have == exp, (p, len(r), c, have, exp)
        if form == "genome":
            wlen = 0 if unplaced else max(0, min(len(win), c + len(r) + w) - o)
            assert (int(got[-2][p]), int(got[-1][p])) == (-1 if unplaced else o, wlen), (p, "window")


def batch(form, w, seed):
    """Mixed lengths in one batch (pairs of a wave end at different steps), bands at
    every edge, a band without a cell, an unplaced read, homopolymer and repeat ties."""
    rng = np.random.default_rng(seed)
    G = rng.choice(ACGT, 900).astype(np.uint8)
    G[300:360] = ord("A")
    G[400:460] = np.resize(np.frombuffer(b"AC", np.uint8), 60)
    pairs = []
    for L in (1, 2, 15, 16, 17, 33, 150, 384) * 3 + (1, 2, 15, 16, 17, 33) * 26:
        a = int(rng.integers(0, len(G) - L - 4))
        pairs.append((mutate(rng, G[a:a + L + 3])[:L], a + int(rng.integers(-2, 3))))
    for a, L in ((300, 20), (310, 33), (400, 17), (405, 40), (295, 30)):          # ties
        pairs += [(G[a:a + L].copy(), a), (G[a:a + L].copy(), a + w)]
    for c in (-5, -40 - w, -w, w, len(G) - 40, len(G) - 40 + w, len(G) - 1, len(G) + w, len(G) + w + 1):
        pairs.append((G[max(0, min(c, len(G) - 40)):][:40].copy(), c))           # edges, no cell
    if form == "genome":
        return [(r, G, c) for r, c in pairs] + [(G[5:30].copy(), G, UNPLACED)]
    out = []
    for r, c in pairs:  # a window of its own around the band, the centre relative to it
        lo = max(0, min(c - w - int(rng.integers(0, 9)), len(G) - 1))
        out.append((r, G[lo:lo + len(r) + 2 * w + int(rng.integers(0, 12))], c - lo))
    return out


@pytest.mark.parametrize("form", ["padded", "genome"])
@pytest.mark.parametrize("scheme", ["lin", "aff"])
@pytest.mark.parametrize("w", [0, 1, 7, 15, 16, 31, 32, 63])
def test_band_matches_reference(gpu_ctx, w, scheme, form):
    pairs = batch(form, w, 100 + w)
    check(run(gpu_ctx, form, pairs, w, scheme), form, pairs, w, scheme)
    untraced = run(gpu_ctx, form, pairs, w, scheme, trace=False)
    check(untraced, form, pairs, w, scheme, trace=False)


@pytest.mark.parametrize("scheme", ["lin", "aff"])
@pytest.mark.parametrize("w,k", [(3, 1), (3, 3), (16, 2), (16, 9)])
@pytest.mark.parametrize("kind", ["ins", "del"])
def test_gap_at_the_band_limit(gpu_ctx, kind, w, k, scheme):
    """One gap of k bases: its far side exactly w off centre fits, w + 1 off does not,
    and then the score is the banded one, below the full rectangle's."""
    rng = np.random.default_rng(7 * w + k)
    win = rng.choice(ACGT, 240).astype(np.uint8)
    if kind == "del":   # the read skips k window bases: diagonal 20, then 20 + k
        read, far = np.concatenate([win[20:80], win[80 + k:140 + k]]), 20 + k
    else:               # k extra read bases: diagonal 20, then 20 - k
        read, far = np.concatenate([win[20:80], np.full(k, ord("n"), np.uint8), win[80:140]]), 20 - k
    step = 1 if kind == "del" else -1
    fits, misses = far - step * w, far - step * (w + 1)
    pairs = [(read, win, fits), (read, win, misses)]
    got = run(gpu_ctx, "padded", pairs, w, scheme)
    check(got, "padded", pairs, w, scheme)
    full = ref_band(read, win, 0, 1000, SCHEMES[scheme])[0]
    assert int(got[0][0]) == full and int(got[0][1]) < full


@pytest.mark.parametrize("scheme", ["lin", "aff"])
def test_wide_band_is_the_full_rectangle(gpu_ctx, scheme):
    """w >= max(L, W) with every cell inside the band: the existing calls, bit for bit."""
    from mini_parallel_amd import pack_batch
    rng = np.random.default_rng(5)
    reads, wins = [], []
    for L, W in [(1, 1), (1, 40), (20, 1), (20, 40), (7, 13), (20, 20), (3, 40), (19, 33)] * 6:
        wn = rng.choice(ACGT[:2 + L % 3], W).astype(np.uint8)
        a = int(rng.integers(0, max(1, W - L)))
        reads.append(bytes(mutate(rng, np.resize(wn[a:], L))[:L]))
        wins.append(bytes(wn))
    R, rl, Wn, wl = pack_batch(reads, wins)
    sc = scoring(scheme)
    diag = np.full(len(reads), 10, np.int32)   # j - i in [-19, 39]: |j - i - 10| <= 29 <= 63
    full = gpu_ctx.align_batch_trace(R, rl, Wn, wl, sc)
    band = gpu_ctx.align_batch_banded(R, rl, Wn, wl, diag, 63, sc, trace=True)
    for a, b in zip(full[:5], band[:5]):
        assert np.array_equal(a, b)
    assert [list(o) for o in full[5]] == [list(o) for o in band[5]]
    for a, b in zip(gpu_ctx.align_batch(R, rl, Wn, wl, sc), gpu_ctx.align_batch_banded(R, rl, Wn, wl, diag, 63, sc)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("scheme", ["lin", "aff"])
def test_long_reads(gpu_ctx, scheme):
    """1,500 bases at w = 16 (no row registers, so no 384 limit), score and best cell;
    and a traced read at the LDS bound of 1008 rows."""
    rng = np.random.default_rng(11)
    G = rng.choice(ACGT, 4000).astype(np.uint8)
    pairs = [(mutate(rng, G[a:a + L + 3])[:L], G, a + 1) for a, L in ((100, 1500), (2400, 1200), (1800, 700))]
    check(run(gpu_ctx, "genome", pairs, 16, scheme, trace=False), "genome", pairs, 16, scheme, trace=False)
    pairs = [(mutate(rng, G[a:a + L + 3])[:L], G, a) for a, L in ((50, 1008), (2000, 100))]
    check(run(gpu_ctx, "genome", pairs, 16, scheme), "genome", pairs, 16, scheme)


def test_affine_gap_closing_outside_the_band(gpu_ctx):
    """A 5-base deletion under w = 2, centred on the first diagonal: the gap opens inside the
    band and would pass through and close outside it, so no band holds the whole alignment."""
    win = np.random.default_rng(21).choice(ACGT, 200).astype(np.uint8)
    read = np.concatenate([win[20:80], win[85:145]])
    pairs = [(read, win, 20), (read, win, 25), (read, win, 22)]   # first segment, second, the gap cut
    got = run(gpu_ctx, "padded", pairs, 2, "aff")
    check(got, "padded", pairs, 2, "aff")
    full = ref_band(read, win, 0, 1000, SCHEMES["aff"])[0]
    assert full == 240 - 3 - 5 and all(int(v) < full for v in got[0])


def test_cigar_overflow(gpu_ctx):
    """cigar_stride 2, the rows and 8 words behind them full of a sentinel.  The device call
    writes a fitting row up to its count and nothing else: not the overflowing rows, not the
    tail.  The host call copies whole rows back, so there a row's ops and the tail are checked."""
    import ctypes
    import torch
    from mini_parallel_amd import _lib, pack_batch
    rng = np.random.default_rng(3)
    win = rng.choice(ACGT, 200).astype(np.uint8)
    gapped = np.concatenate([win[10:50], win[52:90], win[93:130]])   # M D M D M: five ops
    pairs = [(win[10:60].copy(), win, 10), (gapped, win, 12)] * 4
    want = [ref_band(r, x, c, 8, SCHEMES["aff"]) for r, x, c in pairs]
    R, rl, Wn, wl = pack_batch([bytes(r) for r, _, _ in pairs], [bytes(x) for _, x, _ in pairs])
    B, S, GUARD = len(pairs), 2, 0x5EADBEEF
    diag = np.array([c for _, _, c in pairs], np.int32)
    dev = torch.device("cuda", 0)
    up = lambda a, dt=None: torch.from_numpy(a if dt is None else a.view(dt)).to(dev)
    dR, dW, drl, dwl, dd = up(R), up(Wn), up(rl, np.int16), up(wl, np.int16), up(diag)
    score, nc = (torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(2))
    ei, ej, si, sj = (torch.zeros(B, dtype=torch.int16, device=dev) for _ in range(4))
    cig = torch.full((B * S + 8,), GUARD, dtype=torch.int32, device=dev)
    batch = _lib.BatchT(dR.data_ptr(), dW.data_ptr(), drl.data_ptr(), dwl.data_ptr(), R.shape[1], Wn.shape[1], B)
    out = _lib.OutT(score.data_ptr(), ei.data_ptr(), ej.data_ptr())
    tr = _lib.TraceT(si.data_ptr(), sj.data_ptr(), nc.data_ptr(), cig.data_ptr(), S)
    sc = scoring("aff").to_c()
    _lib.check(_lib.lib().msw_align_batch_banded_device(
        gpu_ctx.handle, ctypes.byref(sc), ctypes.byref(batch), dd.data_ptr(), 8, ctypes.byref(out), ctypes.byref(tr),
        int(rl.max()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    assert nc.cpu().tolist() == [len(t[5]) for t in want] == [1, 5] * 4
    assert cig.cpu().tolist() == [want[0][5][0], GUARD, GUARD, GUARD] * 4 + [GUARD] * 8
    assert si.cpu().tolist() == [t[3] for t in want] and sj.cpu().tolist() == [t[4] for t in want]
    assert score.cpu().tolist() == [t[0] for t in want]
    # the host call
    h_nc, h_cig = np.zeros(B, np.int32), np.full(B * S + 8, GUARD, np.uint32)
    h = [np.zeros(B, np.int32)] + [np.zeros(B, np.int16) for _ in range(4)]
    batch = _lib.BatchT(R.ctypes.data, Wn.ctypes.data, rl.ctypes.data, wl.ctypes.data, R.shape[1], Wn.shape[1], B)
    out = _lib.OutT(*(a.ctypes.data for a in h[:3]))
    tr = _lib.TraceT(h[3].ctypes.data, h[4].ctypes.data, h_nc.ctypes.data, h_cig.ctypes.data, S)
    _lib.check(_lib.lib().msw_align_batch_banded(gpu_ctx.handle, ctypes.byref(sc), ctypes.byref(batch),
                                                 diag.ctypes.data, 8, ctypes.byref(out), ctypes.byref(tr), 3))
    assert h_nc.tolist() == [1, 5] * 4 and h_cig[0:B * S:2 * S].tolist() == [want[0][5][0]] * 4
    assert (h_cig[B * S:] == GUARD).all() and h[3].tolist() == [t[3] for t in want]


@pytest.mark.parametrize("L,w,trace", [(40, 64, False), (32767 - 31, 16, False), (1009, 16, True)])
def test_out_of_range_arguments(gpu_ctx, L, w, trace):
    from mini_parallel_amd import MswError
    from mini_parallel_amd._lib import MSW_E_RANGE
    R, Wn = np.full((1, L), 65, np.uint8), np.full((1, 64), 65, np.uint8)
    with pytest.raises(MswError) as e:
        gpu_ctx.align_batch_banded(R, np.array([L], np.uint16), Wn, np.array([64], np.uint16), np.zeros(1, np.int32),
                                   w, scoring("lin"), trace=trace)
    assert e.value.code == MSW_E_RANGE
