"""sw_trace_long_kernel (msw_trace_long.hip) on the paths tests/test_gpu_trace_long.py does not reach, against
the same full-matrix restatement, exactly: score, end, start, n_cigar and every op word.

 A  reverse ops in the block's scratch (an op bound past 4,096), read back at 4,199 ops; the LDS / scratch
    switch at strides 4,096 / 4,097; the op buffer reused by one block's next pairs
 B  every rows-per-lane instance (R = 1 .. 6 in one strip, linear and affine), batch and genome entry points
 C  rectangles of 1 .. 128 columns under 2, 3 and 4 strips; windows of 1, 40 and 64 bytes
 D  ties on the boundary between rows 383 and 384, under the seven schemes of tests/test_gpu_traceback.py
 E  32,767 columns; 32,767 rows, all 86 strips walked

The inputs are built by tests/trace_long_inputs.py; tests/test_trace_long_inputs.py shows from the oracle
alone that each has the property its test needs.  Not here: a 32,767 x 32,767 pair (no full-matrix oracle of
that size fits a host) and timing.
"""
import numpy as np
import pytest

import aln_oracle as ao
import trace_long_inputs as ti
import test_gpu_trace_long as base
from test_gpu_trace_long import expected, raw_trace, run_and_check, scoring

pytestmark = pytest.mark.gpu

S = ti.SCHEMES
GUARD = 8
FILL = 0x5EADBEEF


def device_trace(ctx, pairs, scheme, stride):
    """msw_align_batch_device, then msw_trace_long_batch_device, on device arrays that start as FILL: what
    the kernel itself leaves in the rows (the host call copies whole rows back from its own buffer)."""
    import torch
    from mini_parallel_amd import pack_batch
    R, rl, W, wl = pack_batch([bytes(r) for r, _ in pairs], [bytes(w) for _, w in pairs])
    B = len(pairs)
    dev = torch.device("cuda", 0)
    t = lambda a, dt=None: torch.from_numpy(a if dt is None else a.view(dt)).to(dev)
    dR, dW, drl, dwl = t(R), t(W), t(rl, np.int16), t(wl, np.int16)
    full = lambda n, v, dt: torch.full((n + GUARD,), v, dtype=dt, device=dev)
    d = {k: full(B, -21846, dt) for k, dt in (("s", torch.int32), ("ei", torch.int16), ("ej", torch.int16),
                                              ("si", torch.int16), ("sj", torch.int16), ("nc", torch.int32))}
    dcig = full(B * stride, FILL, torch.int32)
    st = torch.cuda.current_stream().cuda_stream
    mr, mw = int(rl.max()), int(wl.max())
    sc = scoring(scheme)
    ctx.align_batch_device(dR.data_ptr(), drl.data_ptr(), dW.data_ptr(), dwl.data_ptr(), R.shape[1], W.shape[1], B,
                           d["s"].data_ptr(), mr, mw, sc, d["ei"].data_ptr(), d["ej"].data_ptr(), st)
    ctx.trace_batch_device(dR.data_ptr(), drl.data_ptr(), dW.data_ptr(), dwl.data_ptr(), R.shape[1], W.shape[1], B,
                           d["s"].data_ptr(), d["ei"].data_ptr(), d["ej"].data_ptr(), d["si"].data_ptr(),
                           d["sj"].data_ptr(), d["nc"].data_ptr(), dcig.data_ptr(), stride, mr, mw, sc, st,
                           long_pairs=True)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in d.items()}
    cig = dcig.cpu().numpy().view(np.uint32)
    assert all((a[B:] == -21846).all() for a in out.values()) and (cig[B * stride:] == FILL).all()
    return {k: a[:B] for k, a in out.items()}, cig[:B * stride].reshape(B, stride)


def trace_rows(ctx, pairs, scheme, stride):
    """raw_trace's arrays, after the device-resident calls gave the same and left every row word behind a
    pair's ops, and the whole row of a pair that overflowed, as it was."""
    out, rows = raw_trace(ctx, pairs, scheme, stride)
    dout, drows = device_trace(ctx, pairs, scheme, stride)
    for k in dout:
        assert np.array_equal(out[k][:len(pairs)], dout[k]), k
    for p in range(len(pairs)):
        n = int(dout["nc"][p])
        kept = n if n <= stride else 0
        assert np.array_equal(rows[p, :kept], drows[p, :kept]), p
        assert (drows[p, kept:] == FILL).all(), (p, n)
    return out, rows


def check_pair(out, rows, p, want, stride):
    got = (int(out["s"][p]), (int(out["ei"][p]), int(out["ej"][p])), (int(out["si"][p]), int(out["sj"][p])))
    assert got == want[:3], (p, got, want[:3])
    assert int(out["nc"][p]) == len(want[3]), (p, int(out["nc"][p]), len(want[3]))
    if len(want[3]) <= stride:
        bad = np.flatnonzero(rows[p, :len(want[3])] != np.array(want[3], np.uint32))
        assert bad.size == 0, (p, "first wrong op word", int(bad[0]), len(want[3]))


# --- A: ops in scratch ---------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ti.OPS_SCHEMES)
def test_ops_in_scratch(gpu_ctx, scheme):
    """4,199 ops at stride 4,224: lane 0 stores them in reverse at mine + ops_off, the wave reads them back."""
    pair = ti.interleaved(2100)
    out, rows = trace_rows(gpu_ctx, [pair], S[scheme], 4224)
    want = expected(*pair, S[scheme])
    assert len(want[3]) == 4199
    check_pair(out, rows, 0, want, 4224)


@pytest.mark.parametrize("scheme", ti.OPS_SCHEMES)
def test_ops_in_scratch_overflow(gpu_ctx, scheme):
    """Stride 4,100 is a scratch layout that the 4,199 ops overflow: count, start and end, an untouched row."""
    pair = ti.interleaved(2100)
    out, rows = trace_rows(gpu_ctx, [pair], S[scheme], 4100)
    want = expected(*pair, S[scheme])
    check_pair(out, rows, 0, want, 4100)
    assert int(out["nc"][0]) == 4199 and (int(out["si"][0]), int(out["sj"][0])) == (0, 0)
    assert (int(out["ei"][0]), int(out["ej"][0])) == (2099, 4198)


@pytest.mark.parametrize("scheme", ti.OPS_SCHEMES)
def test_lds_scratch_switch(gpu_ctx, scheme):
    """4,095 ops at stride 4,096 (the last LDS layout) and 4,097 (the first scratch layout): the same row."""
    pair = ti.interleaved(2048)
    want = expected(*pair, S[scheme])
    assert len(want[3]) == 4095
    got = []
    for stride in (4096, 4097):
        out, rows = trace_rows(gpu_ctx, [pair], S[scheme], stride)
        check_pair(out, rows, 0, want, stride)
        got.append(rows[0, :4095].copy())
    assert np.array_equal(got[0], got[1])


@pytest.mark.parametrize("scheme", ti.OPS_SCHEMES)
def test_ops_scratch_reuse(fresh_ctx, monkeypatch, scheme):
    """One block takes 4,199 ops, a few dozen, an empty read, 4,095 ops and a score-0 pair through one op buffer."""
    monkeypatch.setenv("MSW_TRACE_BLOCKS", "1")
    pairs = ti.reuse_batch()
    out, rows = trace_rows(fresh_ctx, pairs, S[scheme], 4224)
    for p, (r, w) in enumerate(pairs):
        check_pair(out, rows, p, expected(r, w, S[scheme]), 4224)
    assert [int(n) for n in out["nc"][[0, 2, 3, 4]]] == [4199, 0, 4095, 0]


# --- B: every rows-per-lane instance --------------------------------------------------------------
@pytest.mark.parametrize("scheme", ["lin", "aff"])
@pytest.mark.parametrize("m,n,rpl", ti.ROWS_PER_LANE)
def test_rows_per_lane(gpu_ctx, m, n, rpl, scheme):
    """One call per shape: R follows the call's longest read; the window is past 4,096, so the call is long."""
    pairs = ti.rows_per_lane_pairs(m, n)
    assert ti.rows_per_lane(pairs) == rpl
    s, ei, ej, *_ = run_and_check(gpu_ctx, pairs, S[scheme], f"R={rpl} {m}x{n} {scheme}")
    assert int(ej[0]) >= n - 3 and 0 <= int(ej[1]) < 64 and int(s[3]) == 0


@pytest.mark.parametrize("scheme", ["lin", "aff"])
@pytest.mark.parametrize("m,rpl", [(100, 2), (150, 3)])
def test_records_rows_per_lane(gpu_ctx, m, rpl, scheme):
    """align_reads_trace(long_pairs=True): short reads, explicit windows of 4,500."""
    from mini_parallel_amd import pack_batch
    sch = S[scheme]
    g, reads = ti.genome_reads(m)
    assert ti.rows_per_lane([(r, g) for r in reads]) == rpl
    genome = gpu_ctx.load_genome(g)
    R, rl, _, _ = pack_batch([bytes(r) for r in reads], [b""] * len(reads))
    s, ei, ej, ref_pos, nm, cigars = gpu_ctx.align_reads_trace(genome, R, rl, np.array(ti.GENOME_POS),
                                                                np.array(ti.GENOME_WANT), scoring(sch), long_pairs=True)
    for p, r in enumerate(reads):
        want = ao.record(r, ao.window_of(g, ti.GENOME_POS[p], ti.GENOME_WANT[p]), ti.GENOME_POS[p], *sch)
        got = ao.Record(int(s[p]), int(ei[p]), int(ej[p]), int(ref_pos[p]), int(nm[p]), [int(o) for o in cigars[p]])
        assert got == want, (p, ao.cigar_text(got.ops), ao.cigar_text(want.ops))
        assert want.nm > 5 and ao.read_bases(got.ops) == len(r)
    genome.close()


# --- C: narrow rectangles under several strips ------------------------------------------------------
@pytest.mark.parametrize("scheme", ["lin", "aff"])
def test_narrow_rectangles(gpu_ctx, scheme):
    """2, 3 and 4 strips, 1 .. 128 columns wide, against one 300-byte window: the score-only tail store with
    some lanes, with none (64, 128), one column, and top-row blocks past the rectangle."""
    cases = ti.narrow_pairs()
    _, ei, ej, *_ = run_and_check(gpu_ctx, [pw for _, pw in cases], S[scheme], f"narrow {scheme}")
    assert [int(j) + 1 for j in ej] == [e for e, _ in cases]
    assert [int(i) + 1 for i in ei] == [len(r) for _, (r, _) in cases]


@pytest.mark.parametrize("scheme", ["lin", "aff"])
@pytest.mark.parametrize("win_len", [1, 40, 64])
def test_narrow_windows(gpu_ctx, win_len, scheme):
    """769 rows against windows of 1, 40 and 64 bytes: the smallest checkpoint rows, slab rows and LDS window."""
    cases = ti.narrow_pairs((769,), win_len)
    _, _, ej, *_ = run_and_check(gpu_ctx, [pw for _, pw in cases], S[scheme], f"window {win_len} {scheme}")
    assert [int(j) + 1 for j in ej] == [e for e, _ in cases] and max(e for e, _ in cases) == win_len


def test_narrow_crossing(gpu_ctx):
    """Free gaps: the walk crosses every strip boundary inside rectangles that narrow from 8 .. 128 columns."""
    cases = ti.narrow_crossing_pairs()
    _, ei, ej, si, *_ = run_and_check(gpu_ctx, [pw for _, pw in cases], S["lin_gap0"], "narrow crossing")
    assert [int(j) + 1 for j in ej] == [e for e, _ in cases]
    assert all(int(a) == 0 and int(b) == len(r) - 1 for a, b, (_, (r, _)) in zip(si, ei, cases))


# --- D: ties at the strip boundary ------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ti.TIE_SCHEMES)
def test_ties_homopolymers(gpu_ctx, scheme):
    run_and_check(gpu_ctx, ti.homopolymers(), S[scheme], f"homopolymers {scheme}")


@pytest.mark.parametrize("scheme", ti.TIE_SCHEMES)
def test_ties_dinucleotide_slips(gpu_ctx, scheme):
    *_, ops = run_and_check(gpu_ctx, ti.dinucleotide_slips(), S[scheme], f"slips {scheme}")
    assert [ao.cigar_text([int(o) for o in x]) for x in ops] == ["382M1D599M1D219M", "382M1I599M1I219M"]


@pytest.mark.parametrize("scheme", ti.TIE_SCHEMES)
def test_ties_gap_run_over_boundary(gpu_ctx, scheme):
    """The gap may lie anywhere in the A run; the rule puts it at the left end, over rows 383 / 384."""
    cases = ti.gap_run_pairs()
    *_, ops = run_and_check(gpu_ctx, [pw for *_, pw in cases], S[scheme], f"gap run {scheme}")
    want = [f"{row}M8{op}{len(r) - row - (8 if op == 'I' else 0)}M" for op, row, (r, _) in cases]
    assert [ao.cigar_text([int(o) for o in x]) for x in ops] == want


@pytest.mark.parametrize("scheme", ti.TIE_SCHEMES)
def test_ties_read_twice(gpu_ctx, scheme):
    _, ei, ej, si, sj, _ = run_and_check(gpu_ctx, ti.read_twice(), S[scheme], f"twice {scheme}")
    assert (int(si[0]), int(sj[0]), int(ei[0]), int(ej[0])) == (0, 0, 799, 799)


@pytest.mark.parametrize("scheme", ti.TIE_SCHEMES)
def test_ties_low_entropy(gpu_ctx, scheme):
    run_and_check(gpu_ctx, ti.low_entropy_pairs(), S[scheme], f"low entropy {scheme}")


# --- E: the bounds ------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ["lin", "aff"])
@pytest.mark.parametrize("m", [385, 40])
def test_widest_window(gpu_ctx, m, scheme):
    """32,767 columns: checkpoint rows of 32,896 words, slab rows of 2,048 / 4,096 words, a 32,896-byte window
    in LDS; 385 rows are two strips of R = 6, 40 rows one strip of R = 1."""
    r, w = ti.wide_pair(m)
    try:
        _, ei, ej, *_ = run_and_check(gpu_ctx, [(r, w)], S[scheme], f"{m}x32767 {scheme}")
    finally:
        base._ORACLE.pop((bytes(r), bytes(w), S[scheme]), None)
    assert (int(ei[0]), int(ej[0])) == (m - 1, ti.LIMIT - 1)


def test_longest_read(gpu_ctx):
    """32,767 rows under free gaps: 85 checkpoint rows, and the walk goes through all 86 strips."""
    r, w = ti.tall_pair()
    _, ei, ej, si, sj, ops = run_and_check(gpu_ctx, [(r, w)], S["lin_gap0"], "32767x300 lin_gap0")
    assert (int(si[0]), int(sj[0]), int(ei[0]), int(ej[0])) == (0, 0, ti.LIMIT - 1, 299) and len(ops[0]) == 599
