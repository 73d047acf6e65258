"""Quality-weighted variant calls on the GPU (msw_pileup_call_qual[_device],
msw_call_counts_qual; include/msw.h, "Quality sums and weighted genotypes"):
bit-exact against tests/variant_qual_oracle.py.  Crafted counts and sums go
through msw_call_counts_qual, so any row can be tested; Pileup.call runs over
real MSW_PILEUP_QSUM pileups."""
import ctypes

import numpy as np
import pytest

import variant_oracle as vo
import variant_qual_oracle as vq
from test_gpu_call import LENIENT, craft
from test_gpu_pileup import planted, to_dev

pytestmark = pytest.mark.gpu

U32 = 2 ** 32 - 1


def craft_q(rng, glen, busy=0.6, q20=False):
    """craft() of test_gpu_call plus sums: per observation a Phred value of
    2 .. 41 (a few rows arbitrary, the sums need not fit the counts)."""
    g, c = craft(rng, glen, busy)
    if q20:
        return g, c, (c[:, :4] * 20).astype(np.uint32)
    w = (c[:, :4].astype(np.uint64) * rng.integers(2, 42, (glen, 4)).astype(np.uint64)).astype(np.uint32)
    odd = rng.random(glen) < 0.05
    w[odd] = rng.integers(0, 5000, (int(odd.sum()), 4))
    return g, c, w


def raw_call(ctx, genome, counts, qsums, q=None, qq=None, chunk_pos=0, cap=None, room=None):
    """msw_call_counts_qual itself: -> (return code, total, the output buffer, which starts out as 0xAB bytes)."""
    from mini_parallel_amd._lib import lib
    from mini_parallel_amd.aligner import VARIANT_DTYPE
    g = np.frombuffer(genome, np.uint8)
    c = np.ascontiguousarray(counts, np.uint32)
    w = None if qsums is None else np.ascontiguousarray(qsums, np.uint32)
    room = cap if room is None else room
    out = np.full(max(room or 0, 1) * VARIANT_DTYPE.itemsize, 0xAB, np.uint8)
    total = ctypes.c_uint64(12345)
    rc = lib().msw_call_counts_qual(ctx.handle, g.ctypes.data if len(g) else None, len(g),
                                    c.ctypes.data if c.size else None, w.ctypes.data if w is not None and w.size else None,
                                    ctypes.byref(q) if q is not None else None,
                                    ctypes.byref(qq) if qq is not None else None, chunk_pos,
                                    out.ctypes.data if cap is not None else None, cap or 0, ctypes.byref(total))
    return rc, int(total.value), out


def same(ctx, genome, counts, qsums, p=None, q=None, chunk_pos=0):
    """Context.call_variants(qsums=) against the oracle, byte for byte; -> the oracle's records."""
    from mini_parallel_amd import CallParams, QualParams
    want = vq.call(genome, counts, qsums, vo.params(**p) if p else None, vq.qparams(**q) if q else None)
    got = ctx.call_variants(genome, counts, CallParams(**p) if p else None, chunk_pos, qsums=qsums,
                            qual_params=QualParams(**q) if q else None).to_records()
    assert len(got) == len(want), (len(got), len(want))
    if got.tobytes() != want.tobytes():
        k = next(i for i in range(len(want)) if got[i].tobytes() != want[i].tobytes())
        raise AssertionError((k, got[k], want[k]))
    return want


@pytest.mark.parametrize("glen", [1, 63, 64, 65, 257, 3000])
def test_lengths_and_chunks_against_the_oracle(gpu_ctx, glen):
    rng = np.random.default_rng(glen)
    g, c, w = craft_q(rng, glen, busy=0.9)
    c[-1, 6] = 9
    c[glen // 2, 6] = 30                                  # an insertion whose look-ahead row is another chunk's first
    want = same(gpu_ctx, g, c, w)
    plain = vo.call(g, c)
    if glen >= 257:
        kinds = set(int(k) for k in want["kind"])
        assert kinds == {vo.SNV, vo.DEL, vo.INS} and want.tobytes() != plain.tobytes()
    # insertion records are the unweighted ones
    assert want[want["kind"] == vo.INS].tobytes() == plain[plain["kind"] == vo.INS].tobytes()
    for chunk in (1, 64, 257) if glen < 3000 else (257, 1000):
        same(gpu_ctx, g, c, w, chunk_pos=chunk)
    same(gpu_ctx, g, c, w, dict(LENIENT), dict(q_scale=65535, q_third=65535))
    same(gpu_ctx, g, c, w, dict(LENIENT), dict(q_scale=0, q_third=0), chunk_pos=64)
    same(gpu_ctx, g, np.full((glen, 8), U32, np.uint32), np.full((glen, 4), U32, np.uint32),
         dict(LENIENT), dict(q_scale=65535, q_third=65535))


def test_glen_zero(gpu_ctx):
    assert len(gpu_ctx.call_variants(b"", np.zeros((0, 8), np.uint32), qsums=np.zeros((0, 4), np.uint32)).pos) == 0


def test_q20_invariant(gpu_ctx):
    """Every base at Phred 20 and the default weights: the records of the unweighted caller."""
    rng = np.random.default_rng(20)
    for p in (None, dict(LENIENT)):
        g, c, w = craft_q(rng, 1500, busy=0.9, q20=True)
        want = same(gpu_ctx, g, c, w, p, chunk_pos=333)
        assert want.tobytes() == vo.call(g, c, vo.params(**p) if p else None).tobytes() and len(want) > 200
        from mini_parallel_amd import CallParams
        assert gpu_ctx.call_variants(g, c, CallParams(**p) if p else None).to_records().tobytes() == want.tobytes()


def test_cap_below_the_total_and_the_count_only_form(gpu_ctx):
    rng = np.random.default_rng(5)
    g, c, w = craft_q(rng, 700, busy=0.9)
    want = vq.call(g, c, w)
    total, size = len(want), want.dtype.itemsize
    assert total > 100
    assert raw_call(gpu_ctx, g, c, w)[:2] == (0, total)                   # the count pass alone
    for chunk in (0, 100):
        for cap in (0, 1, total // 2, total - 1, total, total + 3):
            rc, n, out = raw_call(gpu_ctx, g, c, w, chunk_pos=chunk, cap=cap, room=total + 4)
            assert (rc, n) == (0, total)
            k = min(cap, total)
            assert out[:k * size].tobytes() == want[:k].tobytes()
            assert (out[k * size:] == 0xAB).all()


class Piles:
    pass


@pytest.fixture(scope="module")
def piles(gpu_ctx):
    """The planted 20 kbase genome through map_reads(mapq=True), piled up once
    with real-looking qualities: a flagged pileup and an unflagged one."""
    from mini_parallel_amd import Scoring
    b = Piles()
    b.g, batch, R, rl = planted()
    b.genome = gpu_ctx.load_genome(b.g)
    index = gpu_ctx.build_index(b.genome, 8)
    s, ei, ej, strand, ref, nm, cigars, mq, sub, cand = gpu_ctx.map_reads(b.genome, index, R, rl,
                                                                          Scoring(2, -1, 0, 2, False, True), mapq=True)
    rng = np.random.default_rng(31)
    quals = (33 + rng.choice(np.array([2, 11, 25, 37]), R.shape, p=[0.05, 0.1, 0.15, 0.7])).astype(np.uint8)
    b.pile = gpu_ctx.pileup(b.genome, qsum=True)
    b.pile.add(R, rl, ref, nm, cigars, strand=strand, mapq=mq, quals=quals, min_baseq=0)
    b.pile.finish()
    b.plain = gpu_ctx.pileup(b.genome)
    b.plain.add(R, rl, ref, nm, cigars, strand=strand, mapq=mq)
    b.plain.finish()
    index.close()
    yield b
    b.pile.close()
    b.plain.close()
    b.genome.close()


def test_pileup_call_over_map_reads(gpu_ctx, piles):
    from mini_parallel_amd import CallParams, QualParams
    counts, qsums = piles.pile.counts(), piles.pile.qsums()
    assert np.array_equal(counts, piles.plain.counts()) and qsums.any()
    sizes = []
    for over, qover in (({}, {}), (LENIENT, {}), (dict(LENIENT, min_depth=2), dict(q_scale=50, q_third=1000))):
        want = vq.call(piles.g, counts, qsums, vo.params(**over), vq.qparams(**qover))
        first = piles.pile.call(CallParams(**over), QualParams(**qover)).to_records()
        assert first.tobytes() == want.tobytes(), (len(first), len(want))
        assert piles.pile.call(CallParams(**over), QualParams(**qover)).to_records().tobytes() == first.tobytes()
        # the host-array form over the same counts and sums
        host = gpu_ctx.call_variants(piles.g, counts, CallParams(**over), 4099, qsums=qsums, qual_params=QualParams(**qover))
        assert host.to_records().tobytes() == want.tobytes()
        sizes.append(len(want))
    assert sizes[1] > 100 and sizes[1] > sizes[2] > 0
    # without qual_params the flag changes nothing: the unweighted records of the same counts
    plain = piles.pile.call(CallParams(**LENIENT)).to_records()
    assert plain.tobytes() == vo.call(piles.g, counts, vo.params(**LENIENT)).tobytes()
    assert plain.tobytes() == piles.plain.call(CallParams(**LENIENT)).to_records().tobytes()
    assert plain.tobytes() != piles.pile.call(CallParams(**LENIENT), QualParams()).to_records().tobytes()


def test_device_form_cap_and_count_only(gpu_ctx, piles):
    import torch
    from mini_parallel_amd import CallParams, QualParams
    from mini_parallel_amd.aligner import VARIANT_DTYPE
    want = vq.call(piles.g, piles.pile.counts(), piles.pile.qsums(), vo.params(**LENIENT))
    total = len(want)
    assert total > 100
    for cap in (0, 7, total, total + 5):
        out = torch.full(((total + 8) * 48,), 0xAB, dtype=torch.uint8, device="cuda:0")
        n = torch.zeros(1, dtype=torch.int64, device="cuda:0")
        piles.pile.call_device(out.data_ptr() if cap else 0, cap, n.data_ptr(), CallParams(**LENIENT),
                               qual_params=QualParams())
        gpu_ctx.synchronize()
        assert int(n.item()) == total
        host = out.cpu().numpy()
        k = min(cap, total)
        assert host[:k * 48].tobytes() == want[:k].tobytes() and (host[k * 48:] == 0xAB).all()
    assert VARIANT_DTYPE.itemsize == 48


def test_error_paths(gpu_ctx, fresh_ctx, piles):
    import mini_parallel_amd as mpa
    from mini_parallel_amd._lib import MSW_E_INVALID, MSW_E_RANGE, CallParamsT, CallQParamsT, lib
    L = lib()
    qq = CallQParamsT()
    L.msw_call_qparams_default(ctypes.byref(qq))
    assert (qq.q_scale, qq.q_third) == (100, 477) and mpa.QualParams() == mpa.QualParams(**vq.QDEFAULTS)
    L.msw_call_qparams_default(None)
    g, c, w = craft_q(np.random.default_rng(1), 40, busy=0.9)
    for name in ("q_scale", "q_third"):
        bad = CallQParamsT(100, 477)
        setattr(bad, name, 65536)
        assert raw_call(gpu_ctx, g, c, w, qq=bad)[0] == MSW_E_INVALID and "65535" in L.msw_last_error().decode()
        with pytest.raises(mpa.MswError) as e:
            gpu_ctx.call_variants(g, c, qsums=w, qual_params=mpa.QualParams(**{name: 65536}))
        assert e.value.code == MSW_E_INVALID
        with pytest.raises(mpa.MswError) as e:
            piles.pile.call(qual_params=mpa.QualParams(**{name: 65536}))
        assert e.value.code == MSW_E_INVALID
    bad = CallParamsT()
    L.msw_call_params_default(ctypes.byref(bad))
    bad.q_miss = 65536
    assert raw_call(gpu_ctx, g, c, w, q=bad)[0] == MSW_E_INVALID
    assert raw_call(gpu_ctx, g, c, w, chunk_pos=(1 << 24) + 1)[0] == MSW_E_RANGE
    assert raw_call(gpu_ctx, g, c, None)[0] == MSW_E_INVALID                 # qsums NULL
    gp, cp, wp, n = np.frombuffer(g, np.uint8).ctypes.data, c.ctypes.data, w.ctypes.data, ctypes.c_uint64()
    assert L.msw_call_counts_qual(None, gp, 40, cp, wp, None, None, 0, None, 0, ctypes.byref(n)) == MSW_E_INVALID
    assert L.msw_call_counts_qual(gpu_ctx.handle, gp, 40, cp, wp, None, None, 0, None, 0, None) == MSW_E_INVALID
    assert L.msw_call_counts_qual(gpu_ctx.handle, gp, 40, cp, wp, None, None, 0, None, 5, ctypes.byref(n)) == MSW_E_INVALID
    assert L.msw_call_counts_qual(gpu_ctx.handle, None, 40, cp, wp, None, None, 0, None, 0, ctypes.byref(n)) == MSW_E_INVALID
    assert L.msw_call_counts_qual(gpu_ctx.handle, gp, 40, None, wp, None, None, 0, None, 0, ctypes.byref(n)) == MSW_E_INVALID
    n.value = 9
    assert L.msw_call_counts_qual(gpu_ctx.handle, None, 0, None, None, None, None, 0, None, 0, ctypes.byref(n)) == 0
    assert n.value == 0
    with pytest.raises(mpa.MswError):
        gpu_ctx.call_variants(g, c, qsums=w[:39])
    with pytest.raises(mpa.MswError):
        gpu_ctx.call_variants(g, c, qual_params=mpa.QualParams())            # weights without sums
    # the pileup forms: without the flag, before the finish, another context, out NULL with cap > 0
    for f in (lambda: piles.plain.call(qual_params=mpa.QualParams()),
              lambda: piles.plain.call_device(0, 0, 0, qual_params=mpa.QualParams())):
        with pytest.raises(mpa.MswError) as e:
            f()
        assert e.value.code == MSW_E_INVALID and "MSW_PILEUP_QSUM" in str(e.value)
    fresh = gpu_ctx.pileup(piles.genome, qsum=True)
    with pytest.raises(mpa.MswError) as e:
        fresh.call(qual_params=mpa.QualParams())
    assert e.value.code == MSW_E_INVALID and "finish" in str(e.value)
    fresh.close()
    h = piles.pile.handle
    assert L.msw_pileup_call_qual(fresh_ctx.handle, h, None, None, None, 0, ctypes.byref(n)) == MSW_E_INVALID
    assert L.msw_pileup_call_qual(gpu_ctx.handle, None, None, None, None, 0, ctypes.byref(n)) == MSW_E_INVALID
    assert L.msw_pileup_call_qual(gpu_ctx.handle, h, None, None, None, 0, None) == MSW_E_INVALID
    assert L.msw_pileup_call_qual(gpu_ctx.handle, h, None, None, None, 3, ctypes.byref(n)) == MSW_E_INVALID
    assert L.msw_pileup_call_qual_device(gpu_ctx.handle, h, None, None, None, 3, None, None) == MSW_E_INVALID
    # NULL params and qparams are the defaults
    assert L.msw_pileup_call_qual(gpu_ctx.handle, h, None, None, None, 0, ctypes.byref(n)) == 0
    assert n.value == len(piles.pile.call(qual_params=mpa.QualParams()).pos)
