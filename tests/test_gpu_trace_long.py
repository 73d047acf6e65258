"""Traceback past the packed range (sw_trace_long_kernel, msw_trace_long.hip:
strips of 384 rows, checkpointed) against the full-matrix restatement
(tests/traceback_oracle.py) and tests/aln_oracle.py: score, end, start and op
list, exactly.  Every output array of the raw calls has guard words behind it.
The op buffer in scratch, the instances with R = 1, 2, 4, 5 rows per lane,
rectangles under 129 columns, ties on the strip boundary and the 32,767 bounds
are in tests/test_gpu_trace_long_paths.py.
"""
import ctypes

import numpy as np
import pytest

import aln_oracle as ao
import traceback_oracle as tbo

pytestmark = pytest.mark.gpu

SCHEMES = {"lin": (2, -1, 0, 2, False), "aff": (2, -1, 3, 1, True), "aff_ext0": (2, -1, 4, 0, True)}
ACGT = np.frombuffer(b"ACGT", np.uint8)
GUARD = 8
_ORACLE = {}


def scoring(scheme):
    from mini_parallel_amd import Scoring
    m, x, go, ge, aff = scheme
    return Scoring(match=m, mismatch=x, gap_open=go, gap_extend=ge, affine=aff, want_coords=True)


def expected(r, w, scheme):
    key = (bytes(r), bytes(w), scheme)
    if key not in _ORACLE:
        _ORACLE[key] = tbo.align(r, w, *scheme)
    return _ORACLE[key]


def planted(seed, w, a, m):
    """w[a : a + m] with an SNV every 37 bases, a 3-base insertion and a 2-base deletion (length m)."""
    rng = np.random.default_rng(seed)
    r = w[a:a + m + 2].copy()
    r[5::37] = (r[5::37] + 1 - 65) % 4 + 65  # another byte: never equal to the window's
    k, d = int(rng.integers(10, m // 2)), int(rng.integers(m // 2, m - 10))
    r = np.concatenate([r[:k], rng.choice(ACGT, 3).astype(np.uint8), r[k:d], r[d + 2:]])
    return r[:m]


def junk(n):
    return np.full(n, ord("n"), np.uint8)   # equals no window byte


def window(seed, n):
    return np.random.default_rng(seed).choice(ACGT, n).astype(np.uint8)


def raw_trace(ctx, pairs, scheme, stride):
    """msw_align_batch_trace_long through ctypes, guard words behind every output array."""
    from mini_parallel_amd import _lib, pack_batch
    R, rl, W, wl = pack_batch([bytes(r) for r, _ in pairs], [bytes(w) for _, w in pairs])
    B = len(pairs)
    out = {k: np.full(B + GUARD, -21846, dt) for k, dt in
           (("s", np.int32), ("ei", np.int16), ("ej", np.int16), ("si", np.int16), ("sj", np.int16), ("nc", np.int32))}
    cig = np.full(B * stride + GUARD, 0xDEADBEEF, np.uint32)
    batch = _lib.BatchT(R.ctypes.data, W.ctypes.data, rl.ctypes.data, wl.ctypes.data, R.shape[1], W.shape[1], B)
    o = _lib.OutT(out["s"].ctypes.data, out["ei"].ctypes.data, out["ej"].ctypes.data)
    tr = _lib.TraceT(out["si"].ctypes.data, out["sj"].ctypes.data, out["nc"].ctypes.data, cig.ctypes.data, stride)
    sc = scoring(scheme).to_c()
    _lib.check(_lib.lib().msw_align_batch_trace_long(ctx.handle, ctypes.byref(sc), ctypes.byref(batch),
                                                     ctypes.byref(o), ctypes.byref(tr), 0))
    assert all((a[B:] == -21846).all() for a in out.values()) and (cig[B * stride:] == 0xDEADBEEF).all()
    return out, cig[:B * stride].reshape(B, stride)


def run_and_check(ctx, pairs, scheme, tag):
    s, ei, ej, si, sj, ops = ctx.align_batch_trace(*pack(pairs), scoring(scheme), long_pairs=True)
    for p, (r, w) in enumerate(pairs):
        want = expected(r, w, scheme)
        got = (int(s[p]), (int(ei[p]), int(ej[p])), (int(si[p]), int(sj[p])), [int(o) for o in ops[p]])
        assert got[:3] == want[:3], (tag, p, got[:3], want[:3])
        assert got[3] == want[3], (tag, p, tbo.cigar_text(got[3]), tbo.cigar_text(want[3]))
    return s, ei, ej, si, sj, ops


def pack(pairs):
    from mini_parallel_amd import pack_batch
    return pack_batch([bytes(r) for r, _ in pairs], [bytes(w) for _, w in pairs])


# read x window: 2 strips with a 1-row last strip, 2 full strips, 3, 4; columns past 4096 across a
# 64-column checkpoint block and a direction word; one strip on the new kernel
SHAPES = [(385, 600), (768, 900), (769, 1000), (1153, 1300), (400, 4097), (500, 4161), (150, 4200)]


@pytest.mark.parametrize("scheme", sorted(SCHEMES))
@pytest.mark.parametrize("m,n", SHAPES)
def test_strip_shapes(gpu_ctx, m, n, scheme):
    """A read with planted edits that ends in the window's last column (the whole rectangle) and a random read."""
    w = window(m * 7 + n, n)
    pairs = [(planted(m, w, n - m - 1, m), w), (window(m + n, m), w)]
    s, ei, ej, *_ = run_and_check(gpu_ctx, pairs, SCHEMES[scheme], f"{m}x{n} {scheme}")
    assert int(ei[0]) == m - 1 and int(ej[0]) >= n - 3


@pytest.mark.parametrize("scheme", sorted(SCHEMES))
def test_strip_boundaries(gpu_ctx, scheme):
    """Alignments planted on the boundary between rows 383 and 384, score-0 and empty pairs between them."""
    w = window(99, 1500)
    a = 200
    cat = np.concatenate
    pairs = [
        (w[a:a + 800].copy(), w),                                   # 0: one M run across rows 383 -> 384
        (junk(8), w),                                               # 1: score 0
        (cat([w[a:a + 380], junk(8), w[a + 380:a + 780]]), w),      # 2: insertion rows 380..387 (F extends over the edge)
        (cat([w[a:a + 384], junk(8), w[a + 384:a + 784]]), w),      # 3: insertion rows 384..391 (F opens at the edge)
        (np.zeros(0, np.uint8), w),                                 # 4: empty read
        (cat([w[a:a + 385], w[a + 391:a + 791]]), w),               # 5: 6-column deletion walked in row 384
        (cat([junk(384), w[a:a + 300]]), w),                        # 6: first aligned cell in row 384
        (cat([w[a:a + 384], junk(300)]), w),                        # 7: end_i = 383: one strip of a long read
        (cat([w[a:a + 385], junk(300)]), w),                        # 8: end_i = 384
        (w[:50].copy(), np.zeros(0, np.uint8)),                     # 9: empty window
        (cat([junk(1053), w[a:a + 100]]), w),                       # 10: only the last strip of four is walked
    ]
    s, ei, ej, si, sj, ops = run_and_check(gpu_ctx, pairs, SCHEMES[scheme], f"boundaries {scheme}")
    op = lambda n, c: n << 4 | c
    assert list(ops[0]) == [op(800, 0)]
    assert list(ops[2]) == [op(380, 0), op(8, 1), op(400, 0)]
    assert list(ops[3]) == [op(384, 0), op(8, 1), op(400, 0)]
    # a D op that follows exactly 385 read bases is walked in row 384 (linear gaps may split into several runs)
    before = np.cumsum([0] + [(int(o) >> 4) * ((int(o) & 15) != 2) for o in ops[5]])
    assert any((int(o) & 15) == 2 and before[k] == 385 for k, o in enumerate(ops[5]))
    assert sum(int(o) >> 4 for o in ops[5] if (int(o) & 15) == 2) == 6
    if SCHEMES[scheme][4]:
        assert list(ops[5]) == [op(385, 0), op(6, 2), op(400, 0)]
    assert (int(si[6]), int(sj[6]), list(ops[6])) == (384, a, [op(300, 0)])
    assert (int(si[7]), int(ei[7])) == (0, 383) and (int(si[8]), int(ei[8])) == (0, 384)
    assert (int(si[10]), int(ei[10]), list(ops[10])) == (1053, 1152, [op(100, 0)])
    assert [int(s[p]) for p in (1, 4, 9)] == [0, 0, 0] and [len(ops[p]) for p in (1, 4, 9)] == [0, 0, 0]


@pytest.mark.parametrize("scheme", ["lin", "aff"])
@pytest.mark.parametrize("blocks", ["1", "3"])
def test_work_queue_scratch_reuse(fresh_ctx, monkeypatch, blocks, scheme):
    """1 / 3 blocks take 9 pairs of alternating 2- and 4-strip shapes from the queue: a block's checkpoint rows,
    slab and op words are the previous pair's."""
    monkeypatch.setenv("MSW_TRACE_BLOCKS", blocks)
    pairs = []
    for k in range(9):
        m, n = ((700, 900), (1200, 1400))[k % 2]
        w = window(500 + k, n)
        pairs.append((planted(k, w, (n - m - 1) >> (k % 3), m), w))
    stride = 64
    out, rows = raw_trace(fresh_ctx, pairs, SCHEMES[scheme], stride)
    for p, (r, w) in enumerate(pairs):
        want = expected(r, w, SCHEMES[scheme])
        got = (int(out["s"][p]), (int(out["ei"][p]), int(out["ej"][p])), (int(out["si"][p]), int(out["sj"][p])))
        assert got == want[:3] and int(out["nc"][p]) == len(want[3]) <= stride, (p, got, want[:3])
        assert [int(o) for o in rows[p, :len(want[3])]] == want[3], p


def test_cigar_overflow(gpu_ctx):
    """A 3-strip pair needs more ops than the row holds: count and start are right, nothing past the row."""
    w = window(7, 1000)
    pairs = [(planted(3, w, 100, 769), w), (w[10:60].copy(), w)]
    out, rows = raw_trace(gpu_ctx, pairs, SCHEMES["aff"], 2)
    want = expected(*pairs[0], SCHEMES["aff"])
    assert len(want[3]) > 2 and int(out["nc"][0]) == len(want[3])
    assert (int(out["si"][0]), int(out["sj"][0])) == want[2]
    assert int(out["nc"][1]) == 1 and int(rows[1, 0]) == 50 << 4


def short_batch():
    return [(planted(k, window(40 + k, 300), 20 + k, 150), window(40 + k, 300)) for k in range(6)]


def test_routing_packed_range(gpu_ctx):
    """Inside the packed range long_pairs=True is today's call, array for array."""
    args = pack(short_batch())
    a = gpu_ctx.align_batch_trace(*args, scoring(SCHEMES["aff"]))
    b = gpu_ctx.align_batch_trace(*args, scoring(SCHEMES["aff"]), long_pairs=True)
    assert all(np.array_equal(x, y) for x, y in zip(a[:5], b[:5]))
    assert all(np.array_equal(x, y) for x, y in zip(a[5], b[5]))


@pytest.mark.parametrize("scheme", ["lin", "aff"])
def test_routing_force_long(fresh_ctx, monkeypatch, scheme):
    """MSW_FORCE_LONG=1: the same batch on the new kernel (R = 3, one strip)."""
    monkeypatch.setenv("MSW_FORCE_LONG", "1")
    run_and_check(fresh_ctx, short_batch(), SCHEMES[scheme], f"force long {scheme}")


@pytest.mark.parametrize("scheme", ["lin", "aff"])
def test_records(gpu_ctx, scheme):
    """align_reads_trace(long_pairs=True): reads of 500 and 900 bases, explicit windows of 1200 and 4500."""
    sch = SCHEMES[scheme]
    g = window(123, 9000)
    genome = gpu_ctx.load_genome(g)
    reads = [planted(1, g, 700, 500), planted(2, g, 3100, 900), planted(3, g, 8300, 500)]
    pos, want_len = [400, 1000, 8000], [1200, 4500, 4500]   # the last window is clipped at the genome end
    from mini_parallel_amd import pack_batch
    R, rl, _, _ = pack_batch([bytes(r) for r in reads], [b""] * 3)
    s, ei, ej, ref_pos, nm, cigars = gpu_ctx.align_reads_trace(genome, R, rl, np.array(pos), np.array(want_len),
                                                                scoring(sch), long_pairs=True)
    for p, r in enumerate(reads):
        want = ao.record(r, ao.window_of(g, pos[p], want_len[p]), pos[p], *sch)
        got = ao.Record(int(s[p]), int(ei[p]), int(ej[p]), int(ref_pos[p]), int(nm[p]), [int(o) for o in cigars[p]])
        assert got == want, (p, ao.cigar_text(got.ops), ao.cigar_text(want.ops))
        assert want.nm > 5 and ao.read_bases(got.ops) == len(r)
    genome.close()


def test_bounds_and_arguments(gpu_ctx):
    """32,768 in either bound is MSW_E_RANGE (-2); NULL arrays and short strides are MSW_E_INVALID (-1)."""
    import torch
    import mini_parallel_amd as mpa
    d = torch.zeros(4096, dtype=torch.int32, device="cuda").data_ptr()
    call = lambda **k: gpu_ctx.trace_batch_device(
        k.get("reads", d), d, d, d, k.get("rs", 1024), 1024, 1, d, d, d, k.get("si", d), d, d, d, 4,
        k.get("mr", 500), k.get("mw", 600), scoring(SCHEMES["lin"]), long_pairs=True)
    genome = gpu_ctx.load_genome(window(1, 2000))
    reads_call = lambda window_, mr: gpu_ctx.trace_reads_device(genome, d, d, 1024, d, 1, window_, mr, d, d, d, d, d, d,
                                                                d, 4, scoring(SCHEMES["lin"]), long_pairs=True)
    for fn, code in ((lambda: call(mr=32768), -2), (lambda: call(mw=32768), -2), (lambda: call(reads=0), -1),
                     (lambda: call(si=0), -1), (lambda: call(rs=496), -1), (lambda: reads_call(32768, 500), -2),
                     (lambda: reads_call(600, 32768), -2), (lambda: reads_call(600, 1025), -1)):
        with pytest.raises(mpa.MswError) as e:
            fn()
        assert e.value.code == code
    big = np.full((1, 32768), 65, np.uint8)
    with pytest.raises(mpa.MswError) as e:
        gpu_ctx.align_batch_trace(big, np.array([32768]), big[:, :16], np.array([16]), scoring(SCHEMES["lin"]),
                                  long_pairs=True)
    assert e.value.code == -2
    genome.close()
