"""GPU traceback (msw_trace.hip) against the full-matrix restatement
(tests/traceback_oracle.py), op for op, plus checks that do not depend on it:
the CIGAR consumes exactly end - start + 1 bases of the read and of the window,
and re-scoring it under the scheme gives the score.

Nothing is left out: every listed shape runs under every scheme named for it.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import traceback_oracle as tbo

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mini_parallel_amd", "rustseq_mini")

LIN = (2, -1, 0, 2, False)     # the reference's constants
AFF = (2, -1, 3, 1, True)      # config 3
SCHEMES = {
    "lin": LIN,
    "aff": AFF,
    "lin_gap0": (2, -1, 0, 0, False),
    "lin_mismatch0": (3, 0, 0, 2, False),
    "aff_ext0": (2, -1, 4, 0, True),
    "aff_m64_x0": (64, 0, 10, 1, True),
    "aff_open10": (2, -1, 10, 1, True),
}
ACGT = np.frombuffer(b"ACGT", np.uint8)


def scoring(scheme, coords=True):
    from mini_parallel_amd import Scoring
    m, x, go, ge, aff = scheme
    return Scoring(match=m, mismatch=x, gap_open=go, gap_extend=ge, affine=aff, want_coords=coords)


_ORACLE = {}


def expected(r, w, scheme):
    """The restatement's answer for one pair, computed once."""
    key = (bytes(r), bytes(w), scheme)
    if key not in _ORACLE:
        _ORACLE[key] = tbo.align(r, w, *scheme)
    return _ORACLE[key]


def mutated(rng, w, a, m, alphabet=ACGT):
    """~m bases of w from a, with a few substitutions and short indels."""
    r = [int(x) for x in w[a:a + m]] or [int(alphabet[0])]
    for _ in range(1 + m // 24):
        k = int(rng.integers(0, len(r)))
        what = int(rng.integers(0, 3))
        if what == 0:
            r[k] = int(rng.choice(alphabet))
        elif what == 1:
            r[k:k] = [int(x) for x in rng.choice(alphabet, int(rng.integers(1, 4)))]
        elif len(r) > 4:
            del r[k:k + int(rng.integers(1, 3))]
    while len(r) < m:
        r.append(int(rng.choice(alphabet)))
    return np.array(r[:m], np.uint8)


def make_pairs(rng, lens, alphabet=ACGT):
    """Half mutated copies of a window slice, half random."""
    out = []
    for k, (m, n) in enumerate(lens):
        w = rng.choice(alphabet, n).astype(np.uint8)
        if k % 2 == 0:
            r = mutated(rng, w, int(rng.integers(0, max(1, n - m + 1))), m, alphabet)
        else:
            r = rng.choice(alphabet, m).astype(np.uint8)
        out.append((r, w))
    return out


def pack(pairs):
    from mini_parallel_amd import pack_batch
    return pack_batch([bytes(r) for r, _ in pairs], [bytes(w) for _, w in pairs])


def check_result(got, r, w, scheme, tag):
    """got = (score, end_i, end_j, start_i, start_j, ops) of one pair."""
    score, ei, ej, si, sj, ops = got
    ops = [int(o) for o in ops]
    # independent of the restatement
    if score == 0:
        assert (ei, ej, si, sj) == (-1, -1, -1, -1) and ops == [], tag
    else:
        assert (ops[0] & 15) == 0 and (ops[-1] & 15) == 0, (tag, tbo.cigar_text(ops))
        assert all((o >> 4) >= 1 and (o & 15) <= 2 for o in ops), tag
        assert all((a & 15) != (b & 15) for a, b in zip(ops, ops[1:])), (tag, tbo.cigar_text(ops))
        assert tbo.consumed(ops) == (ei - si + 1, ej - sj + 1), (tag, tbo.cigar_text(ops))
        m, x, go, ge, aff = scheme
        assert tbo.rescore(ops, r, w, (si, sj), m, x, go, ge, aff) == (score, (ei, ej)), (tag, tbo.cigar_text(ops))
    # op for op
    want = expected(r, w, scheme)
    assert (score, (ei, ej), (si, sj)) == want[:3], (tag, want[:3])
    assert ops == want[3], (tag, tbo.cigar_text(ops), tbo.cigar_text(want[3]))


def run_and_check(ctx, pairs, scheme, tag="", **kw):
    R, rl, W, wl = pack(pairs)
    s, ei, ej, si, sj, ops = ctx.align_batch_trace(R, rl, W, wl, scoring(scheme), **kw)
    assert len(ops) == len(pairs)
    for p, (r, w) in enumerate(pairs):
        assert ops[p] is not None, (tag, p, int(ops.n_cigar[p]))
        check_result((int(s[p]), int(ei[p]), int(ej[p]), int(si[p]), int(sj[p]), ops[p]), r, w, scheme,
                     f"{tag} pair {p} ({len(r)} x {len(w)})")
    # the feature changes nothing: plain scoring of the same batch agrees
    ps, pi, pj = ctx.align_batch(R, rl, W, wl, scoring(scheme))
    assert np.array_equal(ps, s) and np.array_equal(pi, ei) and np.array_equal(pj, ej), tag
    return s, ei, ej, si, sj, ops


READ_LENS = [1, 2, 15, 16, 17, 63, 64, 65, 128, 129, 150, 256, 257, 384]
WIN_LENS = [1, 7, 8, 9, 15, 16, 17, 64, 65, 300, 600]


@pytest.mark.parametrize("scheme", ["lin", "aff"])
@pytest.mark.parametrize("m", READ_LENS)
def test_read_lengths(gpu_ctx, m, scheme):
    """8 pairs per read length (64 rows per lane-row: 63 / 64 / 65, 128 / 129,
    256 / 257, 384 cross the rows-per-lane instances), over the window lengths."""
    rng = np.random.default_rng(1000 + m)
    lens = [(m, WIN_LENS[(k + m) % len(WIN_LENS)]) for k in range(6)] + [(m, 300), (m, 600)]
    run_and_check(gpu_ctx, make_pairs(rng, lens), SCHEMES[scheme], f"m={m} {scheme}")


@pytest.mark.parametrize("scheme", ["lin", "aff"])
@pytest.mark.parametrize("n", WIN_LENS)
def test_window_lengths(gpu_ctx, n, scheme):
    """8 pairs per window length (direction words hold 16 / 8 columns: 7, 8,
    9, 15, 16, 17 cross a word), over the read lengths."""
    rng = np.random.default_rng(2000 + n)
    lens = [(READ_LENS[(k * 3 + n) % len(READ_LENS)], n) for k in range(8)]
    run_and_check(gpu_ctx, make_pairs(rng, lens), SCHEMES[scheme], f"n={n} {scheme}")


@pytest.mark.parametrize("scheme", ["lin", "aff"])
def test_global_scratch_path(gpu_ctx, scheme):
    """Rectangles past the LDS budget keep their direction words in the
    block's global slab: 384 x 4096 and 300 x 2000, one pair ending in the
    last row and column, beside small pairs of the same batch (LDS)."""
    rng = np.random.default_rng(31)
    w0 = rng.choice(ACGT, 4096).astype(np.uint8)
    w1 = rng.choice(ACGT, 4096).astype(np.uint8)
    w2 = rng.choice(ACGT, 2000).astype(np.uint8)
    w3 = rng.choice(ACGT, 2000).astype(np.uint8)
    pairs = [
        (w0[4096 - 384:].copy(), w0),                 # ends at the last cell (383, 4095)
        (mutated(rng, w1, 3000, 384), w1),
        (rng.choice(ACGT, 20).astype(np.uint8), rng.choice(ACGT, 40).astype(np.uint8)),
        (mutated(rng, w2, 1650, 300), w2),
        (mutated(rng, w3, 10, 300), w3),              # ends early: a small rectangle
    ]
    s, ei, ej, _, _, _ = run_and_check(gpu_ctx, pairs, SCHEMES[scheme], f"global {scheme}")
    assert (int(ei[0]), int(ej[0])) == (383, 4095)


def queue_pairs(rng, n_small):
    """Slab pairs (200 x 700 ending at the window's far end: 17,600 affine /
    8,800 linear words, past the 8,192 kept in LDS) between small LDS pairs,
    an empty and a score-0 pair."""
    out = []
    for k in range(n_small):
        if k % 6 == 3:
            w = rng.choice(ACGT, 700).astype(np.uint8)
            out.append((mutated(rng, w, 496, 200), w))
        else:
            out += make_pairs(rng, [(int(rng.integers(1, 25)), int(rng.integers(1, 50)))])
    out[5] = (np.zeros(0, np.uint8), out[5][1])
    out[7] = (np.frombuffer(b"AAAA", np.uint8), np.frombuffer(b"CCCCCC", np.uint8))
    return out


@pytest.mark.parametrize("scheme", ["lin", "aff"])
@pytest.mark.parametrize("blocks", ["1", "3"])
def test_work_queue_few_blocks(fresh_ctx, monkeypatch, blocks, scheme):
    """MSW_TRACE_BLOCKS: 1 / 3 blocks take 44 pairs from the work queue, so a
    block traces many pairs in turn: its window and op buffer are overwritten,
    its slab is reused (a 384 x 4096 pair first, then 200 x 700 ones whose
    words land on the same addresses) and LDS and slab pairs alternate."""
    monkeypatch.setenv("MSW_TRACE_BLOCKS", blocks)
    rng = np.random.default_rng(41)
    w = rng.choice(ACGT, 4096).astype(np.uint8)
    pairs = [(mutated(rng, w, 3700, 384), w)] + queue_pairs(rng, 42) + [(w[4000:4060].copy(), w)]
    run_and_check(fresh_ctx, pairs, SCHEMES[scheme], f"queue {blocks} blocks {scheme}")


@pytest.mark.parametrize("scheme,n", [("aff", 380), ("lin", 720)])
def test_work_queue_default_grid(gpu_ctx, scheme, n):
    """The default grid of a slab launch is capped at 256 MiB of slabs (341
    blocks at 384 x 4096 affine, 682 linear): more pairs than that go through
    the queue."""
    rng = np.random.default_rng(43)
    w = rng.choice(ACGT, 4096).astype(np.uint8)
    lens = [(int(rng.integers(1, 9)), int(rng.integers(1, 17))) for _ in range(n)]
    pairs = [(mutated(rng, w, 3600, 384), w)] + make_pairs(rng, lens) + [(w[4030:4090].copy(), w)]
    run_and_check(gpu_ctx, pairs, SCHEMES[scheme], f"default grid {scheme}")


def mixed_pool():
    rng = np.random.default_rng(77)
    lens = [(int(rng.integers(1, 151)), int(rng.integers(1, 301))) for _ in range(65)]
    pairs = make_pairs(rng, lens)
    empty = np.zeros(0, np.uint8)
    pairs[2] = (empty, pairs[2][1])                                  # empty read
    pairs[3] = (pairs[3][0], empty)                                  # empty window
    pairs[4] = (np.frombuffer(b"AAAAAAAA", np.uint8), np.frombuffer(b"CCCCCCCCCCCC", np.uint8))  # score 0
    pairs[5] = (empty, empty)
    return pairs


@pytest.mark.parametrize("scheme", ["lin", "aff"])
@pytest.mark.parametrize("batch", [1, 7, 9, 65])
def test_batch_sizes_mixed_lengths(gpu_ctx, batch, scheme):
    pairs = mixed_pool()
    pairs = pairs[:batch] if batch > 1 else pairs[6:7]
    s, *_ = run_and_check(gpu_ctx, pairs, SCHEMES[scheme], f"B={batch} {scheme}")
    if batch >= 7:
        assert list(s[2:6]) == [0, 0, 0, 0]


@pytest.mark.parametrize("scheme", ["lin", "aff"])
def test_alignment_placement(gpu_ctx, scheme):
    rng = np.random.default_rng(5)
    w = rng.choice(ACGT, 64).astype(np.uint8)
    b = lambda t: np.frombuffer(t, np.uint8)
    pairs = [
        (w[10:40].copy(), w),                          # touches row 0
        (np.concatenate([b(b"TTTT"), w[:30]]), np.concatenate([w[:30], b(b"GGGG")])),  # touches column 0
        (b(b"AG"), b(b"ACCC")),                        # ends at (0, 0)
        (w[34:].copy(), w),                            # ends at the last cell
        (w.copy(), w),                                 # the whole rectangle
    ]
    s, ei, ej, si, sj, _ = run_and_check(gpu_ctx, pairs, SCHEMES[scheme], f"placement {scheme}")
    assert int(si[0]) == 0 and int(sj[1]) == 0
    assert (int(ei[2]), int(ej[2]), int(si[2]), int(sj[2])) == (0, 0, 0, 0)
    assert (int(ei[3]), int(ej[3])) == (29, 63)
    assert (int(si[4]), int(sj[4]), int(ei[4]), int(ej[4])) == (0, 0, 63, 63)


def gap_pairs():
    rng = np.random.default_rng(9)
    w = rng.choice(ACGT, 300).astype(np.uint8)
    ins = np.concatenate([w[50:120], rng.choice(ACGT, 20).astype(np.uint8), w[120:200]])   # 20-base insertion
    dele = np.concatenate([w[30:100], w[125:200]])                                         # 25-base deletion
    short = np.concatenate([w[40:70], w[71:100], np.frombuffer(b"T", np.uint8), w[100:130], w[132:170]])
    return [(ins, w), (dele, w), (short, w)]


def test_long_gaps_affine(gpu_ctx):
    """gap_open = 10: each long indel is ONE gap."""
    pairs = gap_pairs()
    _, _, _, _, _, ops = run_and_check(gpu_ctx, pairs, SCHEMES["aff_open10"], "gaps aff_open10")
    gaps = lambda o: [(int(x) >> 4, int(x) & 15) for x in o if int(x) & 15]
    assert gaps(ops[0]) == [(20, 1)], tbo.cigar_text(ops[0])
    assert gaps(ops[1]) == [(25, 2)], tbo.cigar_text(ops[1])
    run_and_check(gpu_ctx, pairs, AFF, "gaps aff")


def test_short_gaps_linear(gpu_ctx):
    pairs = gap_pairs()
    _, _, _, _, _, ops = run_and_check(gpu_ctx, pairs, LIN, "gaps lin")
    kinds = [int(x) & 15 for x in ops[2] if int(x) & 15]
    assert len(kinds) >= 3 and set(kinds) == {1, 2}, tbo.cigar_text(ops[2])   # several short gaps, both kinds


@pytest.mark.parametrize("scheme", sorted(SCHEMES))
def test_ties(gpu_ctx, scheme):
    """Homopolymers, tandem repeats, a window that holds the read twice."""
    b = lambda t: np.frombuffer(t, np.uint8)
    rng = np.random.default_rng(13)
    u = rng.choice(ACGT, 40).astype(np.uint8)
    pairs = [
        (b(b"AAAA"), b(b"AAAAAA")),
        (b(b"A" * 33), b(b"A" * 70)),
        (b(b"A" * 70), b(b"A" * 33)),
        (b(b"GGTTCACACACAGGTT"), b(b"GGTTCACACAGGTT")),
        (b(b"GGTTCACAGGTT"), b(b"GGTTCACACAGGTT")),
        (b(b"ACG" * 20), b(b"ACG" * 45)),
        (b(b"TT" + b"CAG" * 15 + b"GG"), b(b"TT" + b"CAG" * 11 + b"GG")),
        (u.copy(), np.concatenate([u, b(b"TTTT"), u])),
        (np.concatenate([u[:20], u[:20]]), u[:20].copy()),
    ]
    run_and_check(gpu_ctx, pairs, SCHEMES[scheme], f"ties {scheme}")


@pytest.mark.parametrize("scheme", sorted(SCHEMES))
def test_schemes(gpu_ctx, scheme):
    """Every scheme on mutated and random pairs; non-ACGT bytes (N, lower
    case) compare by byte equality."""
    rng = np.random.default_rng(21)
    lens = [(150, 300), (150, 300), (33, 70), (70, 33), (100, 100), (17, 129)]
    pairs = make_pairs(rng, lens)
    pairs += make_pairs(rng, [(60, 120), (60, 120), (31, 65), (90, 40)], np.frombuffer(b"ACGTNacgt", np.uint8))
    pairs += make_pairs(rng, [(40, 90), (90, 90)], np.frombuffer(b"AC", np.uint8))
    run_and_check(gpu_ctx, pairs, SCHEMES[scheme], f"schemes {scheme}")


def test_known_answers(gpu_ctx):
    from mini_parallel_amd import cigar_string
    for scheme, want in ((LIN, [(8, 3, 3, 0, 0, "4M"), (24, 15, 13, 0, 0, "4M2I10M"), (20, 11, 13, 0, 0, "4M2D8M")]),
                         (AFF, [(8, 3, 3, 0, 0, "4M"), (23, 15, 13, 0, 0, "4M2I10M"), (19, 11, 13, 0, 0, "4M2D8M")])):
        pairs = [(b"AAAA", b"AAAAAA"), (b"GGTTCACACACAGGTT", b"GGTTCACACAGGTT"), (b"GGTTCACAGGTT", b"GGTTCACACAGGTT")]
        R, rl, W, wl = pack(pairs)
        s, ei, ej, si, sj, ops = gpu_ctx.align_batch_trace(R, rl, W, wl, scoring(scheme, coords=False))
        got = [(int(s[p]), int(ei[p]), int(ej[p]), int(si[p]), int(sj[p]), cigar_string(ops[p])) for p in range(3)]
        assert got == want


def _raw_trace(ctx, R, rl, W, wl, scheme, stride, chunk_pairs=0, guard=8):
    """msw_align_batch_trace through ctypes with a sentinel-filled CIGAR buffer."""
    from mini_parallel_amd import _lib
    B = R.shape[0]
    s, ei, ej = np.zeros(B, np.int32), np.zeros(B, np.int16), np.zeros(B, np.int16)
    si, sj, nc = np.zeros(B, np.int16), np.zeros(B, np.int16), np.zeros(B, np.int32)
    cig = np.full(B * stride + guard, 0xDEADBEEF, np.uint32)
    batch = _lib.BatchT(R.ctypes.data, W.ctypes.data, rl.ctypes.data, wl.ctypes.data, R.shape[1], W.shape[1], B)
    out = _lib.OutT(s.ctypes.data, ei.ctypes.data, ej.ctypes.data)
    tr = _lib.TraceT(si.ctypes.data, sj.ctypes.data, nc.ctypes.data, cig.ctypes.data, stride)
    sc = scoring(scheme, coords=False).to_c()   # want_coords is forced by the call
    _lib.check(_lib.lib().msw_align_batch_trace(ctx.handle, ctypes.byref(sc), ctypes.byref(batch), ctypes.byref(out),
                                                ctypes.byref(tr), chunk_pairs))
    return s, ei, ej, si, sj, nc, cig


def test_cigar_overflow(gpu_ctx):
    """cigar_stride = 1 and a 3-op pair: its count and starts are right, the
    one-op neighbours' rows are exact, nothing is written past the rows."""
    pairs = [(b"AAAA", b"AAAAAA"), (b"GGTTCACACACAGGTT", b"GGTTCACACAGGTT"), (b"ACGTACGT", b"TTACGTACGTTT")]
    R, rl, W, wl = pack(pairs)
    s, ei, ej, si, sj, nc, cig = _raw_trace(gpu_ctx, R, rl, W, wl, LIN, 1)
    assert list(nc) == [1, 3, 1]
    assert (int(s[1]), int(ei[1]), int(ej[1]), int(si[1]), int(sj[1])) == (24, 15, 13, 0, 0)
    assert int(cig[0]) == 4 << 4 and int(cig[2]) == 8 << 4
    assert (cig[3:] == 0xDEADBEEF).all()
    # the Python wrapper: a given stride reports the overflow, None retries once
    *_, ops = gpu_ctx.align_batch_trace(R, rl, W, wl, scoring(LIN), cigar_stride=1)
    assert ops[1] is None and list(ops.n_cigar) == [1, 3, 1] and list(ops[0]) == [4 << 4]
    *_, ops = gpu_ctx.align_batch_trace(R, rl, W, wl, scoring(LIN), cigar_stride=None)
    assert [tbo.cigar_text([int(o) for o in x]) for x in ops] == ["4M", "4M2I10M", "8M"]


def test_python_stride_retry(gpu_ctx):
    """More ops than the wrapper's first stride: it repeats the call once."""
    rng = np.random.default_rng(3)
    w = rng.choice(ACGT, 600).astype(np.uint8)
    r = np.delete(w[100:400], np.arange(5, 300, 6))   # a deleted base every 6: ~50 gaps
    s, ei, ej, si, sj, ops = run_and_check(gpu_ctx, [(r, w), (w[:50].copy(), w)], AFF, "retry")
    assert len(ops[0]) > 32


@pytest.mark.parametrize("scheme", ["lin", "aff"])
def test_entry_points_agree(gpu_ctx, scheme):
    """msw_trace_batch_device fed by msw_align_batch_device, msw_align_batch_trace
    in chunks smaller than the batch, and the Python wrapper."""
    import torch
    sch = SCHEMES[scheme]
    pairs = mixed_pool()[:40]
    R, rl, W, wl = pack(pairs)
    B = len(pairs)
    ref = run_and_check(gpu_ctx, pairs, sch, f"entry {scheme}")
    stride = max(1, int(ref[5].n_cigar.max()))
    # chunked host call
    s, ei, ej, si, sj, nc, cig = _raw_trace(gpu_ctx, R, rl, W, wl, sch, stride, chunk_pairs=7)
    for a, b in zip((s, ei, ej, si, sj, nc), ref[:5] + (ref[5].n_cigar,)):
        assert np.array_equal(a, b)
    rows = cig[:B * stride].reshape(B, stride)
    assert all(np.array_equal(rows[p, :nc[p]], ref[5][p]) for p in range(B))
    assert (cig[B * stride:] == 0xDEADBEEF).all()
    # device-resident calls on torch's stream
    dev = torch.device("cuda", 0)
    t = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a) if dt is None else np.ascontiguousarray(a).view(dt)).to(dev)
    dR, dW, drl, dwl = t(R), t(W), t(rl, np.int16), t(wl, np.int16)
    dscore = torch.full((B,), -7, dtype=torch.int32, device=dev)
    dei, dej, dsi, dsj = (torch.full((B,), -9, dtype=torch.int16, device=dev) for _ in range(4))
    dnc = torch.full((B,), -5, dtype=torch.int32, device=dev)
    dcig = torch.full((B * stride + 8,), 0x5EADBEEF, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    mr, mw = int(rl.max()), int(wl.max())
    gpu_ctx.align_batch_device(dR.data_ptr(), drl.data_ptr(), dW.data_ptr(), dwl.data_ptr(), R.shape[1], W.shape[1],
                               B, dscore.data_ptr(), mr, mw, scoring(sch), dei.data_ptr(), dej.data_ptr(), st)
    # want_coords is not read by the trace call
    gpu_ctx.trace_batch_device(dR.data_ptr(), drl.data_ptr(), dW.data_ptr(), dwl.data_ptr(), R.shape[1], W.shape[1],
                               B, dscore.data_ptr(), dei.data_ptr(), dej.data_ptr(), dsi.data_ptr(), dsj.data_ptr(),
                               dnc.data_ptr(), dcig.data_ptr(), stride, mr, mw, scoring(sch, coords=False), st)
    torch.cuda.synchronize()
    for a, b in zip((dscore, dei, dej, dsi, dsj, dnc), ref[:5] + (ref[5].n_cigar,)):
        assert np.array_equal(a.cpu().numpy(), b)
    hc = dcig.cpu().numpy().view(np.uint32)
    rows = hc[:B * stride].reshape(B, stride)
    assert all(np.array_equal(rows[p, :nc[p]], ref[5][p]) for p in range(B))
    assert (hc[B * stride:] == 0x5EADBEEF).all()


def test_range_and_scoring_unchanged(gpu_ctx, oracle):
    """A 385-base read in a trace call is MSW_E_RANGE; the same batch still
    scores through align_batch, as before."""
    import mini_parallel_amd as mpa
    rng = np.random.default_rng(8)
    pairs = make_pairs(rng, [(385, 600), (150, 300), (10, 4097)])
    for sub in (pairs[:2], pairs[1:]):
        R, rl, W, wl = pack(sub)
        with pytest.raises(mpa.MswError) as e:
            gpu_ctx.align_batch_trace(R, rl, W, wl, scoring(LIN))
        assert e.value.code == -2
        got = gpu_ctx.align_batch(R, rl, W, wl, scoring(LIN))
        want = oracle.sw_batch(R, rl, W, wl, match=2, mismatch=-1, gap_open=0, gap_extend=2, affine=False)
        assert all(np.array_equal(a, b) for a, b in zip(got, want))


def run_cli(args):
    return subprocess.run([CLI] + args, capture_output=True, text=True, timeout=300)


def test_cli_cigar():
    base = ["-1", "GGTTCACACACAGGTT", "-2", "GGTTCACACAGGTT", "-g", "--score-mode", "sw"]
    plain = run_cli(base)
    assert plain.returncode == 0, plain.stderr
    assert plain.stdout.endswith("GPU Alignment score: 24\nBest cell: read 15, window 13\n")
    with_cigar = run_cli(base + ["--cigar"])
    assert with_cigar.returncode == 0, with_cigar.stderr
    assert with_cigar.stdout == plain.stdout + "Alignment start: read 0, window 0\nCIGAR: 4M2I10M\n"
    zero = run_cli(["-1", "AAAA", "-2", "CCCC", "-g", "--score-mode", "sw", "--cigar"])
    assert zero.returncode == 0 and zero.stdout.endswith("Alignment start: read -1, window -1\nCIGAR: *\n")
    long_read = run_cli(["-1", "ACGT" * 97, "-2", "ACGT" * 100, "-g", "--score-mode", "sw", "--cigar"])
    assert long_read.returncode == 1 and "384" in long_read.stderr


def _fastq(path, seqs):
    with open(path, "w") as f:
        for i, q in enumerate(seqs):
            f.write(f"@r{i}\n{q}\n+\n{'I' * len(q)}\n")


def test_cli_cigar_files(tmp_path):
    """--cigar with -f: the pair is the two files' bases (reads concatenated
    in file order)."""
    _fastq(tmp_path / "a.fastq", ["GGTTCACA", "CACAGGTT"])
    _fastq(tmp_path / "b.fastq", ["GGTTCA", "CACAGGTT"])
    args = ["-f", "-1", str(tmp_path / "a.fastq"), "-2", str(tmp_path / "b.fastq"), "-g", "--score-mode", "sw"]
    r = run_cli(args + ["--cigar"])
    assert r.returncode == 0, r.stderr
    assert f"Loaded 16 bases from {tmp_path / 'a.fastq'}\nLoaded 14 bases from {tmp_path / 'b.fastq'}\n" in r.stdout
    assert r.stdout.endswith("GPU Alignment score: 24\nBest cell: read 15, window 13\n"
                             "Alignment start: read 0, window 0\nCIGAR: 4M2I10M\n")
    _fastq(tmp_path / "c.fastq", ["ACGT" * 50, "ACGT" * 50])     # 400 bases: past the traced range
    r = run_cli(["-f", "-1", str(tmp_path / "c.fastq"), "-2", str(tmp_path / "b.fastq"), "-g", "--score-mode", "sw",
                 "--cigar"])
    assert r.returncode == 1 and "384" in r.stderr and "CIGAR" not in r.stdout
    _fastq(tmp_path / "d.fastq", ["ACGT" * 64] * 200)             # 51,200 bases: past every limit
    r = run_cli(["-f", "-1", str(tmp_path / "d.fastq"), "-2", str(tmp_path / "b.fastq"), "-g", "--score-mode", "sw",
                 "--cigar"])
    assert r.returncode == 1 and "CIGAR" not in r.stdout
