"""Candidates and mapping quality on the GPU (include/msw.h, "Candidates and
mapping quality"): seed_candidates_kernel, mapq_select_kernel and
msw_map_reads, array for array against tests/mapq_oracle.py.  Device outputs
carry sentinels around them.
"""
import ctypes

import numpy as np
import pytest

import mapq_oracle as mo
import strand_oracle as so
from test_gpu_seed import DEFAULTS, Case, Guarded, SeedOut, cycle, marker_case, pack, rand_seq, same, to_dev

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", np.uint8)
K = 8


# ---------------------------------------------------------------------------
# the planted genome: 4,096 bases, k = 8
# ---------------------------------------------------------------------------
def other_base(rng, b):
    return int(ACGT[(int(np.searchsorted(ACGT, b)) + int(rng.integers(1, 4))) % 4])


def planted_genome():
    """E1 = g[1200:1300] with an exact copy 700 below (candidate 0 is the
    lower copy: the other one sits at d0 + 700); E2 = g[1400:1500] with a copy
    700 below that differs in one base (reads of E2 get the upper copy as
    candidate 0 and the other at d0 - 700); a copy of E1 at 2500 that differs
    in every 20th base; T = g[3000:3150] whose last 80 bases also stand at
    1870 (a read of T with 20 bases deleted gathers equal votes at both and
    scores more at T: the alternate wins); g[0:70] again at 3500 (negative
    diagonals with a second candidate); X = g[3600:3812], unique."""
    rng = np.random.default_rng(4096)
    g = bytearray(rand_seq(rng, 4096))
    g[500:600] = g[1200:1300]
    g[700:800] = g[1400:1500]
    g[750] = other_base(rng, g[750])
    g[2500:2600] = g[1200:1300]
    for p in range(2505, 2600, 20):
        g[p] = other_base(rng, g[p])
    g[1870:1950] = g[3070:3150]
    g[3500:3570] = g[0:70]
    return bytes(g), rng


def planted_reads():
    g, rng = planted_genome()

    def mutate(s, rate=0.03):
        a = np.frombuffer(s, np.uint8).copy()
        hit = rng.random(a.shape[0]) < rate
        a[hit] = ACGT[rng.integers(0, 4, int(hit.sum()))]
        return a.tobytes()

    reads, tags = [], []
    for L in (0, K - 1, K, 63 + K, 64 + K, 150, 384, 1000):
        for rev in (False, True):
            at = int(rng.integers(0, len(g) - L))
            r = mutate(g[at:at + L]) if L > 20 else g[at:at + L]
            reads.append(so.revcomp(r) if rev else r)
            tags.append("len%d%s" % (L, "r" if rev else ""))
    X = g[3600:3812]
    T = g[3000:3150]
    extra = {
        "e1": g[1210:1290], "e1_r": so.revcomp(g[1205:1295]), "e1_mut": mutate(g[1200:1300], 0.02),
        "e1_wide": g[1150:1300],                       # the lower copy holds 100 of its 150 bases
        "e2": g[1410:1490], "e2_r": so.revcomp(g[1400:1500]),
        "div": g[2500:2600], "div_r": so.revcomp(g[2510:2590]),
        "del": T[:50] + T[70:], "del_r": so.revcomp(T[:50] + T[70:]),
        "over_start": rand_seq(rng, 30) + g[:70], "over_start_r": so.revcomp(rand_seq(rng, 30) + g[:70]),
        "clip": X[0:40] + X[52:82] + X[112:212],      # diagonals p, p + 12, p + 42
        "both_orient": g[2100:2150] + so.revcomp(g[2700:2740]),   # unique pieces, one per orientation
        "unique": g[2100:2250], "unrelated": rand_seq(rng, 150), "empty": b"",
        "n_everywhere": bytes(ord("N") if i % 8 == 3 else b for i, b in enumerate(g[1200:1300])),
    }
    for t, r in extra.items():
        reads.append(r)
        tags.append(t)
    return g, reads, tags


_CASE = {}


def planted_case(ctx):
    if "c" not in _CASE:
        g, reads, tags = planted_reads()
        _CASE["c"] = (Case(ctx, g, K), reads, tags)
    return _CASE["c"]


_MEMO = {}


def expect(oix, reads, both, sep=0, **kw):
    """mapq_oracle.candidates, each distinct read computed once."""
    p = dict(DEFAULTS, **kw)
    rows = []
    for r in reads:
        key = (id(oix), r, both, sep, tuple(sorted(p.items())))
        if key not in _MEMO:
            a, b = mo.candidates_one(oix, r, both, sep=sep, **p)
            _MEMO[key] = a + b
        rows.append(_MEMO[key])
    cols = list(zip(*rows)) if rows else [[]] * 7
    dt = (np.int64, np.uint32, np.uint32, np.uint8, np.int64, np.uint32, np.uint8)
    out = [np.array(c, d) for c, d in zip(cols, dt)]
    return tuple(out[:4]), tuple(out[4:])


def same_alt(have, want, what=""):
    for name, h, w in zip(("win_pos1", "votes1", "flags1"), have, want):
        bad = np.flatnonzero(np.asarray(h).astype(np.int64) != np.asarray(w).astype(np.int64))
        assert bad.size == 0, (what, name, bad[:6].tolist(), np.asarray(h)[bad[:6]].tolist(),
                               np.asarray(w)[bad[:6]].tolist())


class AltOut:
    def __init__(self, n):
        self.wp, self.votes, self.flags = Guarded(n, np.int64), Guarded(n, np.int32), Guarded(n, np.uint8)

    def get(self):
        return self.wp.get(), self.votes.get(np.uint32), self.flags.get()

    def untouched(self):
        return all(x.untouched() for x in (self.wp, self.votes, self.flags))


def enqueue(ctx, index, reads, stride, both, stream=0, base_off=0, sep=0, plain=True, **kw):
    """The candidates call on a fresh upload of `reads`, and (plain) the
    plain seeding call on the same input; returns (out, alt, plain out, keep)."""
    import torch
    R, rl = pack(reads, stride)
    n = len(reads)
    d_R = torch.zeros(base_off + R.size + 64, dtype=torch.uint8, device="cuda:0")
    d_R[base_off:base_off + R.size] = to_dev(R.ravel())
    d_rl = to_dev(rl if n else np.zeros(1, np.uint16), np.int16)
    max_len = int(rl.max()) if n else 0
    rc_stride = max(16, (max_len + 15) // 16 * 16)
    d_rc = torch.full((max(n, 1) * rc_stride,), 0x77, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    out, alt, ref = SeedOut(n), AltOut(n), SeedOut(n)
    if both:
        ctx.revcomp_device(d_R.data_ptr() + base_off, d_rl.data_ptr(), stride, n, d_rc.data_ptr(), rc_stride,
                           stream=stream)
    p = dict(DEFAULTS, **kw)
    rc = dict(rc_reads_ptr=d_rc.data_ptr() if both else 0, rc_stride=rc_stride if both else 0, stream=stream)
    ctx.seed_candidates_device(index, d_R.data_ptr() + base_off, d_rl.data_ptr(), stride, n, max_len, out.wp.ptr,
                               out.votes.ptr, out.hits.ptr, out.flags.ptr, alt.wp.ptr, alt.votes.ptr, alt.flags.ptr,
                               sep=sep, **rc, **p)
    if plain:
        ctx.seed_reads_device(index, d_R.data_ptr() + base_off, d_rl.data_ptr(), stride, n, max_len, ref.wp.ptr,
                              ref.votes.ptr, ref.hits.ptr, ref.flags.ptr, **rc, **p)
    return out, alt, ref, (d_R, d_rl, d_rc)


def check(ctx, C, reads, stride, both, what=None, **kw):
    out, alt, ref, keep = enqueue(ctx, C.index, reads, stride, both, **kw)
    ctx.synchronize()
    okw = {k: v for k, v in kw.items() if k not in ("stream", "base_off", "plain")}
    want0, want1 = expect(C.oix, reads, both, **okw)
    have0 = out.get()
    same(have0, want0, (what, kw))
    same(have0, ref.get(), ("the plain seeding call", what, kw))
    same_alt(alt.get(), want1, (what, kw))
    return want0, want1


# ---------------------------------------------------------------------------
# 1. candidates
# ---------------------------------------------------------------------------
def test_the_planted_cases_occur(gpu_ctx):
    """What the planted reads must come to by the contract (the construction
    is checked on the restatement), and the device against it at the default
    separation, with and without the reverse-complement slab."""
    C, reads, tags = planted_case(gpu_ctx)
    at = {t: p for p, t in enumerate(tags)}
    (wp, votes, hits, flags), (wp1, v1, f1) = check(gpu_ctx, C, reads, 1008, True)
    pad = lambda L: max(0, 2 * L - (L + 15)) // 2
    assert (wp[at["e1"]], wp1[at["e1"]]) == (510 - pad(80), 1210 - pad(80)) and v1[at["e1"]] == votes[at["e1"]] == 73
    assert (wp[at["e1_r"]], wp1[at["e1_r"]], f1[at["e1_r"]]) == (505 - pad(90), 1205 - pad(90), 1)
    assert (wp[at["e2"]], wp1[at["e2"]]) == (1410 - pad(80), 710 - pad(80)) and v1[at["e2"]] < votes[at["e2"]]
    assert (wp[at["div"]], wp1[at["div"]]) == (2500 - pad(100), 500 - pad(100))      # of the two exact copies, the lower
    assert (wp[at["del"]], wp1[at["del"]]) == (1820 - pad(130), 3020 - pad(130)) and v1[at["del"]] == votes[at["del"]]
    assert wp[at["over_start"]] == 0 and wp1[at["over_start"]] == 3470 - pad(100)
    assert f1[at["both_orient"]] == 1 and flags[at["both_orient"]] & 1 == 0
    assert wp1[at["empty"]] == -1 and v1[at["n_everywhere"]] == 0 and v1[at["unique"]] < 8
    assert (wp1[[at["len0"], at["len7"], at["len7r"]]] == -1).all()
    check(gpu_ctx, C, reads, 1001, False)


@pytest.mark.parametrize("kw", [dict(sep=16), dict(sep=700), dict(sep=701), dict(sep=699), dict(sep=40), dict(sep=41),
                                dict(sep=43), dict(sep=4096), dict(sep=1 << 31), dict(sep=1, band=1),
                                dict(sep=300, window=300), dict(sep=0, window=4096, band=40), dict(sep=0, band=40),
                                dict(sep=64, step=3), dict(sep=0, min_votes=60), dict(sep=0, min_votes=74),
                                dict(sep=0, min_votes=1 << 31), dict(sep=100, cap=100, band=3, step=2),
                                dict(sep=1 << 20, band=1 << 20), dict(sep=0, cap=1)])
def test_candidate_parameters(gpu_ctx, kw):
    C, reads, tags = planted_case(gpu_ctx)
    at = {t: p for p, t in enumerate(tags)}
    want0, (wp1, v1, f1) = check(gpu_ctx, C, reads, 1001, True, **kw)
    pad = lambda L: max(0, 2 * L - (L + 15)) // 2
    if kw == dict(sep=700):       # exactly sep away, above and below: admissible
        assert wp1[at["e1"]] == 1210 - pad(80) and wp1[at["e2"]] == 710 - pad(80)
    if kw == dict(sep=701):       # sep - 1 away: not; the copy with a base in every 20th changed is what is left
        assert wp1[at["e1"]] == 2510 - pad(80) and wp1[at["e2"]] not in (710 - pad(80), -1)
    if kw == dict(sep=40):        # the band [p, p + 16) holds p + 12, which is 30 from d0 = p + 42: clipped
        assert (want0[0][at["clip"]], wp1[at["clip"]]) == (3642 - pad(170), 3600 - pad(170))
        assert 33 <= v1[at["clip"]] < 33 + 23      # the 33 k-mers of the piece at p, without the 23 of the piece at p + 12
    if kw == dict(sep=43):        # p is 42 from d0: nothing of that cluster is left
        assert v1[at["clip"]] < 5
    if kw in (dict(sep=4096), dict(sep=1 << 31)):
        assert (wp1 == -1).all() and (v1 == 0).all() and (f1 == 0).all()
    if kw == dict(sep=0, min_votes=74):
        assert wp1[at["e1"]] == -1 and v1[at["e1"]] == 0 and want0[0][at["e1"]] == -1 and want0[1][at["e1"]] == 73


def test_hit_counts_and_cap(gpu_ctx):
    """Hit totals 0, 1, 63, 64, 65, 320 and cap - 1, cap, cap + 1 at cap 64
    and 4096 (the marker genome of the seeding tests: 64 copies of a marker, 9
    bases apart, so every read has second bands at every separation)."""
    C, reads = marker_case(gpu_ctx)
    totals = sorted(reads)
    batch = [reads[t] for t in totals]
    for cap, band, sep in ((4096, 16, 16), (64, 16, 0), (4096, 1, 9), (63, 700, 700), (8192, 4, 300), (4096, 16, 100)):
        for both in (False, True):
            want0, want1 = check(gpu_ctx, C, batch, 608, both, cap=cap, band=band, sep=sep)
            if (cap, both) == (4096, False):
                assert want0[2].tolist()[:5] == [0, 1, 63, 64, 65] and (want1[1][3:] > 0).all()
    C.close()


@pytest.mark.parametrize("n,stride", [(1, 1008), (2, 1001), (65, 1008), (65, 1001), (600, 1008), (600, 1001)])
def test_candidate_batches(gpu_ctx, n, stride):
    C, reads, tags = planted_case(gpu_ctx)
    batch = cycle(reads[21:] + reads[:21], n)
    for both in (True, False):
        for base_off in (0, 1):
            want0, want1 = check(gpu_ctx, C, batch, stride, both, base_off=base_off, sep=0 if both else 64)
        if n >= 65:
            assert (want1[0] >= 0).sum() > n // 8 and (want1[0] == -1).sum() > n // 8
            assert (want1[2] == 1).any() == both


def test_two_streams_in_flight(gpu_ctx):
    from mini_parallel_amd._lib import check as ok, lib
    C, reads, tags = planted_case(gpu_ctx)
    streams = [ctypes.c_void_p() for _ in range(2)]
    for st in streams:
        ok(lib().msw_stream_create(gpu_ctx.handle, ctypes.byref(st)))
    batches = [cycle(reads, 600), cycle(reads[7:], 65)]
    kws = [dict(sep=0), dict(sep=700, band=4)]
    outs = [enqueue(gpu_ctx, C.index, bt, 1008, True, stream=st.value, plain=False, **kw)
            for bt, st, kw in zip(batches, streams, kws)]
    gpu_ctx.synchronize()
    for bt, (out, alt, ref, keep), kw in zip(batches, outs, kws):
        want0, want1 = expect(C.oix, bt, True, **kw)
        same(out.get(), want0, kw)
        same_alt(alt.get(), want1, kw)
    for st in streams:
        ok(lib().msw_stream_destroy(gpu_ctx.handle, st))


def test_host_form(gpu_ctx):
    C, reads, tags = planted_case(gpu_ctx)
    batch = cycle(reads, 130)
    R, rl = pack(batch, 1001)
    for both in (True, False):
        want0, want1 = expect(C.oix, batch, both, sep=700, band=8)
        for chunk in (0, 100, 7):
            have0, have1 = gpu_ctx.seed_candidates(C.index, R, rl, both_strands=both, band=8, sep=700,
                                                   chunk_reads=chunk)
            same(have0, want0, (both, chunk))
            same_alt(have1, want1, (both, chunk))
    a, b = gpu_ctx.seed_candidates(C.index, np.zeros((0, 16), np.uint8), np.zeros(0, np.uint16))
    assert all(x.shape == (0,) for x in a + b)


# ---------------------------------------------------------------------------
# 2. the selection
# ---------------------------------------------------------------------------
PAD = 256


class Dev:
    """A host array on the device between PAD sentinel bytes."""

    def __init__(self, a):
        import torch
        self.a = np.ascontiguousarray(a)
        raw = np.full(self.a.nbytes + 2 * PAD, 0xA5, np.uint8)
        raw[PAD:PAD + self.a.nbytes] = self.a.view(np.uint8).ravel()
        self.t = torch.from_numpy(raw).to("cuda:0")
        assert self.t.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return self.t.data_ptr() + PAD

    def get(self):
        raw = self.t.cpu().numpy()
        assert (raw[:PAD] == 0xA5).all() and (raw[PAD + self.a.nbytes:] == 0xA5).all(), "sentinels overwritten"
        return raw[PAD:PAD + self.a.nbytes].view(self.a.dtype).reshape(self.a.shape)


def select_inputs(n, stride, seed):
    """n reads whose lengths cycle through the row lengths of interest and
    whose score pairs cycle through: alternate wins, tie, loses, both 0,
    negative and large values."""
    rng = np.random.default_rng(seed)
    lens = np.array([0, 1, 15, 16, 17, 150, 384], np.uint16)[np.arange(n) % 7]
    pairs = [(100, 120), (120, 120), (120, 100), (0, 0), (0, 7), (7, 0), (300, 299), (299, 300), (-4, 0), (0, -4),
             (768, 0), (2 ** 31 - 1, 5), (150, 1), (260, 141)]
    sp = np.array([pairs[(p // 7 + p) % len(pairs)][0] for p in range(n)], np.int32)
    sa = np.array([pairs[(p // 7 + p) % len(pairs)][1] for p in range(n)], np.int32)

    def cand(score):
        rows = rng.integers(1, 256, (n, stride)).astype(np.uint8)
        rows[np.arange(stride)[None, :] >= lens[:, None]] = 0
        return dict(score=score, end_i=rng.integers(-1, 384, n).astype(np.int16),
                    end_j=rng.integers(-1, 768, n).astype(np.int16), win_len=rng.integers(0, 769, n).astype(np.uint16),
                    strand=rng.integers(0, 2, n).astype(np.uint8), oriented=rows,
                    win_pos=rng.integers(-1, 1 << 33, n).astype(np.int64))
    return lens, cand(sp), cand(sa)


@pytest.mark.parametrize("arm", ["strands", "one_strand", "score_only", "strands_no_win_len"])
@pytest.mark.parametrize("n", [1, 7, 16, 17, 1000])
def test_select(gpu_ctx, arm, n):
    stride, match = 384, 2
    lens, P, A = select_inputs(n, stride, n)
    drop = {"strands": (), "one_strand": ("strand", "oriented"), "score_only": ("end_i", "end_j", "strand", "oriented"),
            "strands_no_win_len": ("win_len",)}[arm]
    dP = {k: Dev(v) for k, v in P.items() if k not in drop}
    dA = {k: Dev(v) for k, v in A.items() if k not in drop}
    d_rl = Dev(lens)
    sub, mq, cd = Dev(np.full(n, 0x5EADBEEF, np.int32)), Dev(np.full(n, 0xEE, np.uint8)), Dev(np.full(n, 0xEE, np.uint8))
    import torch
    torch.cuda.synchronize()
    gpu_ctx.mapq_select_device({k: v.ptr for k, v in dP.items()}, {k: v.ptr for k, v in dA.items()}, d_rl.ptr, n, match,
                               sub.ptr, mq.ptr, cd.ptr, oriented_stride=stride if "oriented" not in drop else 0)
    gpu_ctx.synchronize()
    want = [mo.select(int(a), int(b)) for a, b in zip(P["score"], A["score"])]
    cand = np.array([w[0] for w in want], np.uint8)
    assert np.array_equal(cd.get(), cand)
    assert np.array_equal(sub.get(), np.array([w[2] for w in want], np.int32))
    assert np.array_equal(mq.get(), np.array([mo.mapq(w[1], w[2], match, int(L)) for w, L in zip(want, lens)], np.uint8))
    if n >= 16:
        assert 0 < cand.sum() < n and {0, 24, 47, 60} <= set(mq.get().tolist())      # 0, floors, the cap
    for k in dP:
        pick = cand.astype(bool)
        if k == "oriented":
            pick = pick[:, None]
        assert np.array_equal(dP[k].get(), np.where(pick, A[k], P[k])), k      # the winner, untouched rows bit-identical
        assert np.array_equal(dA[k].get(), A[k]), k                            # the alternate's arrays are inputs


def test_select_rows_of_another_stride(gpu_ctx):
    """Stride 16 and 400 (25 chunks: more than the sixteen lanes of a read)."""
    for stride in (16, 400):
        n = 33
        lens, P, A = select_inputs(n, stride, stride)
        lens = np.minimum(lens, stride).astype(np.uint16)
        dP, dA = {k: Dev(v) for k, v in P.items()}, {k: Dev(v) for k, v in A.items()}
        d_rl, sub, mq, cd = Dev(lens), Dev(np.zeros(n, np.int32)), Dev(np.zeros(n, np.uint8)), Dev(np.zeros(n, np.uint8))
        import torch
        torch.cuda.synchronize()
        gpu_ctx.mapq_select_device({k: v.ptr for k, v in dP.items()}, {k: v.ptr for k, v in dA.items()}, d_rl.ptr, n, 2,
                                   sub.ptr, mq.ptr, cd.ptr, oriented_stride=stride)
        gpu_ctx.synchronize()
        pick = cd.get().astype(bool)
        assert np.array_equal(pick, A["score"] > P["score"])
        assert np.array_equal(dP["oriented"].get(), np.where(pick[:, None], A["oriented"], P["oriented"]))
        assert np.array_equal(dA["oriented"].get(), A["oriented"])


# ---------------------------------------------------------------------------
# 3. msw_map_reads / Context.map_reads(mapq=True)
# ---------------------------------------------------------------------------
LIN = (2, -1, 0, 2, False)
AFF = (2, -1, 3, 1, True)


@pytest.mark.parametrize("scheme,both", [(LIN, True), (AFF, True), (LIN, False), (AFF, False)])
def test_map_reads(gpu_ctx, scheme, both):
    from mini_parallel_amd import Scoring
    C, reads, tags = planted_case(gpu_ctx)
    keep = [p for p, r in enumerate(reads) if len(r) <= 384]
    batch, tg = [reads[p] for p in keep], [tags[p] for p in keep]
    R, rl = pack(batch, 400)
    R[np.arange(400)[None, :] >= rl[:, None]] = 0
    m, x, go, ge, aff = scheme
    sc = Scoring(m, x, go, ge, aff, True)
    got = gpu_ctx.map_reads(C.genome, C.index, R, rl, sc, both_strands=both, chunk_pairs=16, mapq=True)
    recs, c0, c1 = mo.map_records(C.g, C.oix, batch, scheme, both)
    if both:
        s, ei, ej, strand, ref, nm, cigars, mq, sub, cand = got
    else:
        s, ei, ej, ref, nm, cigars, mq, sub, cand = got
        strand = np.zeros(len(batch), np.uint8)
    for p, r in enumerate(recs):
        have = (int(s[p]), int(ei[p]), int(ej[p]), int(strand[p]), int(ref[p]), int(nm[p]), [int(o) for o in cigars[p]],
                int(mq[p]), int(sub[p]), int(cand[p]))
        assert have == tuple(r), (p, tg[p])
    at = {t: p for p, t in enumerate(tg)}
    # the alternate wins where the seeding preferred the locus that scores less
    assert recs[at["del"]].cand == 1 and recs[at["del"]].ref_pos == 3000 and recs[at["del"]].mapq > 0
    if both:
        assert recs[at["del_r"]].cand == 1 and recs[at["del_r"]].strand == 1
    assert recs[at["e1"]].cand == 0 and recs[at["e1"]].mapq == 0 and recs[at["e1"]].sub_score == recs[at["e1"]].score
    assert recs[at["unique"]].mapq == 60 and recs[at["div"]].mapq in range(1, 60)
    assert recs[at["empty"]].mapq == 0 and recs[at["n_everywhere"]] == mo.Mapped(0, -1, -1, 0, -1, 0, [], 0, 0, 0)
    # one chunk gives the same
    again = gpu_ctx.map_reads(C.genome, C.index, R, rl, sc, both_strands=both, mapq=True, sep=0)
    for a, b in zip(got, again):
        assert all(np.array_equal(u, v) for u, v in zip(a, b)) if isinstance(a, list) else np.array_equal(a, b)


@pytest.mark.parametrize("both", [True, False])
def test_map_reads_without_mapq_is_the_seed_then_align_composition(gpu_ctx, both):
    from mini_parallel_amd import Scoring
    C, reads, tags = planted_case(gpu_ctx)
    batch = [r for r in reads if len(r) <= 384]
    R, rl = pack(batch, 400)
    R[np.arange(400)[None, :] >= rl[:, None]] = 0
    sc = Scoring(2, -1, 3, 1, True, True)
    got = gpu_ctx.map_reads(C.genome, C.index, R, rl, sc, both_strands=both, mapq=False)
    wp = gpu_ctx.seed_reads(C.index, R, rl, both)[0]
    wl = np.minimum(2 * rl.astype(np.int64), 4096).astype(np.uint16)
    want = (gpu_ctx.align_reads_strands(C.genome, R, rl, wp, wl, sc, trace=True) if both
            else gpu_ctx.align_reads_trace(C.genome, R, rl, wp, wl, sc))
    assert len(got) == len(want) == (7 if both else 6)
    for a, b in zip(got, want):
        assert all(np.array_equal(u, v) for u, v in zip(a, b)) if isinstance(a, list) else np.array_equal(a, b)


# ---------------------------------------------------------------------------
# 4. error paths
# ---------------------------------------------------------------------------
def test_argument_errors(gpu_ctx):
    import mini_parallel_amd as mpa
    C, reads, tags = planted_case(gpu_ctx)
    batch = reads[:9]
    R, rl = pack(batch, 1008)
    d_R, d_rl = to_dev(R), to_dev(rl, np.int16)
    out, alt = SeedOut(9), AltOut(9)
    okc = dict(DEFAULTS, reads_ptr=d_R.data_ptr(), read_len_ptr=d_rl.data_ptr(), read_stride=1008, n=9, max_read_len=1000,
               win_pos_ptr=out.wp.ptr, votes_ptr=out.votes.ptr, hits_ptr=out.hits.ptr, flags_ptr=out.flags.ptr,
               win_pos1_ptr=alt.wp.ptr, votes1_ptr=alt.votes.ptr, flags1_ptr=alt.flags.ptr, sep=0)
    bad = [(dict(band=0), -2), (dict(cap=0), -2), (dict(cap=8193), -2), (dict(step=0), -2), (dict(min_votes=0), -2),
           (dict(window=32768), -2), (dict(max_read_len=32768, read_stride=40000), -2), (dict(sep=15), -2),
           (dict(sep=1, band=2), -2), (dict(sep=15, n=0), -2),
           (dict(reads_ptr=0), -1), (dict(read_len_ptr=0), -1), (dict(win_pos_ptr=0), -1), (dict(votes_ptr=0), -1),
           (dict(hits_ptr=0), -1), (dict(flags_ptr=0), -1), (dict(win_pos1_ptr=0), -1), (dict(votes1_ptr=0), -1),
           (dict(flags1_ptr=0), -1), (dict(read_stride=999), -1), (dict(read_stride=0), -1),
           (dict(rc_reads_ptr=d_R.data_ptr(), rc_stride=992), -1)]
    for change, code in bad:
        with pytest.raises(mpa.MswError) as e:
            gpu_ctx.seed_candidates_device(C.index, **dict(okc, **change))
        assert e.value.code == code and str(e.value), change
    gpu_ctx.seed_candidates_device(C.index, **dict(okc, n=0, reads_ptr=0, read_len_ptr=0))
    gpu_ctx.synchronize()
    assert out.untouched() and alt.untouched()
    with pytest.raises(mpa.MswError) as e:
        gpu_ctx.seed_candidates(C.index, R, rl, sep=3)
    assert e.value.code == -2
    with pytest.raises(mpa.MswError) as e:
        gpu_ctx.seed_candidates(C.index, R[:, :16], rl)
    assert e.value.code == -1
    other = mpa.Context(0)
    try:
        with pytest.raises(mpa.MswError) as e:
            other.seed_candidates(C.index, R, rl)
        assert e.value.code == -1
        with pytest.raises(mpa.MswError) as e:
            other.map_reads(C.genome, C.index, R[:, :400], np.minimum(rl, 384), mapq=True)
        assert e.value.code == -1
    finally:
        other.close()

    # the selection
    n = 5
    lens, P, A = select_inputs(n, 32, 1)
    lens = np.minimum(lens, 32).astype(np.uint16)
    dP, dA = {k: Dev(v) for k, v in P.items()}, {k: Dev(v) for k, v in A.items()}
    d_len, sub, mq, cd = Dev(lens), Dev(np.zeros(n, np.int32)), Dev(np.zeros(n, np.uint8)), Dev(np.zeros(n, np.uint8))
    pp, pa = {k: v.ptr for k, v in dP.items()}, {k: v.ptr for k, v in dA.items()}
    oks = dict(primary=pp, alt=pa, read_len_ptr=d_len.ptr, n=n, match=2, sub_score_ptr=sub.ptr, mapq_ptr=mq.ptr,
               cand_ptr=cd.ptr, oriented_stride=32)
    without = lambda d, *ks: {k: v for k, v in d.items() if k not in ks}
    bad = [(dict(match=-1), -2), (dict(match=65), -2), (dict(read_len_ptr=0), -1), (dict(sub_score_ptr=0), -1),
           (dict(mapq_ptr=0), -1), (dict(cand_ptr=0), -1), (dict(primary=without(pp, "score")), -1),
           (dict(alt=without(pa, "score")), -1), (dict(alt=without(pa, "win_pos")), -1),
           (dict(alt=without(pa, "end_i")), -1), (dict(primary=without(pp, "end_j")), -1),
           (dict(alt=without(pa, "strand")), -1), (dict(primary=without(pp, "oriented")), -1),
           (dict(alt=without(pa, "win_len")), -1), (dict(oriented_stride=0), -1), (dict(oriented_stride=24), -1),
           (dict(primary=dict(pp, oriented=pp["oriented"] + 4)), -1), (dict(alt=dict(pa, oriented=pa["oriented"] + 8)), -1)]
    for change, code in bad:
        with pytest.raises(mpa.MswError) as e:
            gpu_ctx.mapq_select_device(**dict(oks, **change))
        assert e.value.code == code and str(e.value), change
    gpu_ctx.mapq_select_device(**dict(oks, n=0))
    gpu_ctx.synchronize()
    assert all(np.array_equal(dP[k].get(), P[k]) for k in P) and not cd.get().any()

    # msw_map_reads
    R4, rl4 = pack([r for r in reads if 20 < len(r) <= 384][:6], 400)
    R4[np.arange(400)[None, :] >= rl4[:, None]] = 0
    for change, code in [(dict(sep=5), -2), (dict(band=0), -2), (dict(min_votes=0), -2), (dict(cap=9000), -2),
                         (dict(window=4097), -2)]:
        with pytest.raises(mpa.MswError) as e:
            gpu_ctx.map_reads(C.genome, C.index, R4, rl4, mapq=True, **change)
        assert e.value.code == code, change
    with pytest.raises(mpa.MswError) as e:                 # a read over 384: the traceback range
        gpu_ctx.map_reads(C.genome, C.index, *pack(reads, 1008), mapq=True)
    assert e.value.code == -2
    with pytest.raises(mpa.MswError) as e:
        gpu_ctx.map_reads(C.genome, C.index, R4[:, :16], rl4, mapq=True)
    assert e.value.code == -1
    got = gpu_ctx.map_reads(C.genome, C.index, np.zeros((0, 16), np.uint8), np.zeros(0, np.uint16), mapq=True)
    assert len(got) == 10 and all(len(a) == 0 for a in got)
