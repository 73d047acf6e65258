"""Variant calls on the GPU (msw_pileup_call*, msw_call_counts; include/msw.h,
"Variants"): bit-exact against tests/variant_oracle.py, the position by
position restatement.  Crafted counts go through msw_call_counts, so any row
can be tested; Pileup.call runs over real pileups."""
import ctypes

import numpy as np
import pytest

import variant_oracle as vo
from test_gpu_pileup import add_device, build, planted, rand_genome

pytestmark = pytest.mark.gpu

U32 = 2 ** 32 - 1
ALPHABET = np.frombuffer(b"ACGTACGTACGTNacgt\x00", np.uint8)
SCAN_TILE_POSITIONS = 1023 * 256        # tiles + 1 offsets fill one scan tile of 1024 up to this many positions


def craft(rng, glen, busy=0.6):
    """A genome (mostly ACGT) and counts[glen][8] whose rows are a mixture:
    empty, reference only, two alleles, a lone alternative, deleted, with
    insertions, and arbitrary small numbers."""
    g = ALPHABET[rng.integers(0, len(ALPHABET), glen)].copy()
    c = np.zeros((glen, 8), np.uint32)
    kind = rng.integers(0, 8, glen)
    kind[rng.random(glen) >= busy] = 0
    for pos in np.flatnonzero(kind):
        k = int(kind[pos])
        depth = int(rng.integers(1, 40))
        r = vo.code(g[pos]) if vo.code(g[pos]) < 4 else int(rng.integers(0, 4))
        if k == 1:
            c[pos, r] = depth
        elif k == 2:
            c[pos, r], c[pos, (r + int(rng.integers(1, 4))) % 4] = depth, int(rng.integers(0, 40))
        elif k == 3:
            c[pos, int(rng.integers(0, 4))] = depth
        elif k == 4:
            c[pos, r], c[pos, 5] = int(rng.integers(0, 20)), depth
        elif k == 5:
            c[pos, r], c[pos, 6] = depth, int(rng.integers(0, 40))
        elif k == 6:
            c[pos] = rng.integers(0, 12, 8)
        else:
            c[pos, :4] = rng.integers(0, 6, 4)           # ties among the alternatives
            c[pos, 5] = int(c[pos, :4].max())
    return g.tobytes(), c


def raw_call(ctx, genome, counts, q=None, chunk_pos=0, cap=None, room=None):
    """msw_call_counts itself: -> (return code, total, the `room` records of the
    output buffer, which starts out as 0xAB bytes)."""
    from mini_parallel_amd._lib import lib
    from mini_parallel_amd.aligner import VARIANT_DTYPE
    g = np.frombuffer(genome, np.uint8)
    c = np.ascontiguousarray(counts, np.uint32)
    room = cap if room is None else room
    out = np.full(max(room or 0, 1) * VARIANT_DTYPE.itemsize, 0xAB, np.uint8)
    total = ctypes.c_uint64(12345)
    rc = lib().msw_call_counts(ctx.handle, g.ctypes.data if len(g) else None, len(g), c.ctypes.data if c.size else None,
                               ctypes.byref(q) if q is not None else None, chunk_pos,
                               out.ctypes.data if cap is not None else None, cap or 0, ctypes.byref(total))
    return rc, int(total.value), out


def same(ctx, genome, counts, p=None, chunk_pos=0):
    """Context.call_variants against the oracle, byte for byte; -> the oracle's records."""
    from mini_parallel_amd import CallParams
    want = vo.call(genome, counts, p)
    got = ctx.call_variants(genome, counts, CallParams(**p) if p else None, chunk_pos).to_records()
    assert len(got) == len(want), (len(got), len(want))
    if got.tobytes() != want.tobytes():
        k = next(i for i in range(len(want)) if got[i].tobytes() != want[i].tobytes())
        raise AssertionError((k, got[k], want[k]))
    return want


@pytest.mark.parametrize("glen", [1, 2, 63, 64, 65, 255, 256, 257])
def test_lengths_round_the_wave_and_the_tile(gpu_ctx, glen):
    rng = np.random.default_rng(glen)
    for rep in range(3):
        g, c = craft(rng, glen, busy=0.9)
        c[-1, 6] = 9 * (rep % 2)                         # the insertion behind the last position: depth(glen) is 0
        same(gpu_ctx, g, c)
        same(gpu_ctx, g, c, vo.params(min_depth=1, min_alt=1, min_qual=0, prior_het=0, prior_hom=0))


def test_one_past_the_scan_tile(gpu_ctx):
    """1025 tile offsets: the scan takes its two-level path.  Sparse rows, with
    records at the first and last position of the tiles round the level's edge."""
    glen = SCAN_TILE_POSITIONS + 1
    rng = np.random.default_rng(77)
    g, c = craft(rng, glen, busy=0.01)
    for pos in (0, 255, 256, 1024 * 256 - 257, SCAN_TILE_POSITIONS - 1, SCAN_TILE_POSITIONS):
        c[pos] = [0, 0, 0, 0, 0, 0, 8, 0]
    want = same(gpu_ctx, g, c)
    assert int(want["pos"][-1]) == glen - 1 and len(want) > 200


def test_every_position_two_records_and_none(gpu_ctx):
    glen = 600
    c = np.tile(np.array([10, 10, 0, 0, 0, 0, 10, 0], np.uint32), (glen, 1))
    want = same(gpu_ctx, b"A" * glen, c)
    assert len(want) == 2 * glen and [int(k) for k in want["kind"][:4]] == [vo.SNV, vo.INS, vo.SNV, vo.INS]
    assert int(want["gt"][-1]) == 2 and int(want["gt"][-3]) == 1     # behind the last position nothing spans
    # nothing to emit: empty rows, reference-only rows, a genome of N
    assert len(same(gpu_ctx, b"A" * glen, np.zeros((glen, 8), np.uint32))) == 0
    ref_only = np.zeros((glen, 8), np.uint32)
    ref_only[:, 2] = 30
    assert len(same(gpu_ctx, b"G" * glen, ref_only)) == 0
    assert len(same(gpu_ctx, b"N" * glen, ref_only)) == 0
    for rc, total, _ in (raw_call(gpu_ctx, b"G" * glen, ref_only), raw_call(gpu_ctx, b"G" * glen, ref_only, cap=4)):
        assert (rc, total) == (0, 0)


def test_records_only_at_wave_ends_and_block_ends(gpu_ctx):
    glen = 1000
    for spots in ([k for k in range(glen) if k % 64 == 63], [k for k in range(glen) if k % 256 in (255, 0)],
                  [63], [255], [256], [999]):
        c = np.zeros((glen, 8), np.uint32)
        c[:, 3] = 12
        for k in spots:
            c[k] = [0, 7, 0, 5, 0, 0, 6, 0]
        want = same(gpu_ctx, b"T" * glen, c)
        assert sorted(set(int(p) for p in want["pos"])) == spots and len(want) == 2 * len(spots)


def test_cap_zero_below_and_equal(gpu_ctx):
    rng = np.random.default_rng(5)
    g, c = craft(rng, 700, busy=0.9)
    want = vo.call(g, c)
    total = len(want)
    assert total > 100
    size = want.dtype.itemsize
    assert raw_call(gpu_ctx, g, c)[:2] == (0, total)                     # the count pass alone
    for chunk in (0, 100):
        for cap in (0, 1, total // 2, total - 1, total, total + 3):
            rc, n, out = raw_call(gpu_ctx, g, c, chunk_pos=chunk, cap=cap, room=total + 4)
            assert (rc, n) == (0, total)
            k = min(cap, total)
            assert out[:k * size].tobytes() == want[:k].tobytes()
            assert (out[k * size:] == 0xAB).all()                        # nothing past cap, or past the total


@pytest.mark.parametrize("glen", [700, 65])
def test_chunk_pos_does_not_change_the_bytes(gpu_ctx, glen):
    rng = np.random.default_rng(6)
    g, c = craft(rng, glen, busy=0.9)
    c[glen // 2, 6] = 30                              # an insertion whose look-ahead row is another chunk's first
    for chunk in (1, 64, 257, 0):
        same(gpu_ctx, g, c, chunk_pos=chunk)


def test_saturating_counts(gpu_ctx):
    full = np.full((5, 8), U32, np.uint32)
    want = same(gpu_ctx, b"ANCGT", full)
    assert (want["qual"] == U32).any() and (want["depth"] == U32).all()
    want = same(gpu_ctx, b"ANCGT", full, vo.params(min_alt_permille=100))
    assert int((want["kind"] == vo.INS).sum()) == 5 and (want["ref_count"][want["kind"] == vo.INS][:4] == U32).all()
    mixed = full.copy()
    mixed[1] = [U32, 0, 0, 0, U32, 0, U32, 0]
    mixed[3] = [0, 0, 0, 0, 0, U32, 3, U32]
    same(gpu_ctx, b"ANCGT", mixed, vo.params(min_alt_permille=1))
    same(gpu_ctx, b"ANCGT", mixed, chunk_pos=2)


@pytest.mark.parametrize("over", [
    dict(q_hit=65535, q_miss=65535, q_het=65535),
    dict(q_hit=0, q_miss=65535, q_het=0, prior_het=U32, prior_hom=U32),
    dict(q_hit=65535, q_miss=0, q_het=1, prior_het=0, prior_hom=0, min_qual=0),
    dict(min_alt_permille=1000, min_alt=0, min_depth=1, min_qual=0),
    dict(min_alt_permille=0, min_alt=0, min_depth=1, min_qual=0, prior_het=0, prior_hom=0),
    dict(min_depth=U32, min_alt=U32, min_qual=U32),
    dict(min_qual=U32, q_miss=65535, q_hit=0),
])
def test_parameters_at_their_limits(gpu_ctx, over):
    rng = np.random.default_rng(8)
    g, c = craft(rng, 300, busy=0.9)
    c[7] = U32
    c[8] = [0, U32, 0, 0, 0, 0, U32, 0]
    c[9] = [U32, 0, 0, 0, 0, 0, 0, 0]
    same(gpu_ctx, g, c, vo.params(**over))


def test_error_paths(gpu_ctx, fresh_ctx):
    import mini_parallel_amd as mpa
    from mini_parallel_amd._lib import MSW_E_INVALID, MSW_E_RANGE, CallParamsT, lib
    L = lib()
    q = CallParamsT()
    L.msw_call_params_default(ctypes.byref(q))
    assert [getattr(q, k) for k in mpa.CallParams.FIELDS] == [vo.DEFAULTS[k] for k in mpa.CallParams.FIELDS]
    assert mpa.CallParams() == mpa.CallParams(**vo.DEFAULTS)
    L.msw_call_params_default(None)
    g, c = craft(np.random.default_rng(1), 40, busy=0.9)
    for name, v in (("q_hit", 65536), ("q_miss", 65536), ("q_het", U32), ("min_depth", 0), ("min_alt_permille", 1001)):
        bad = CallParamsT()
        L.msw_call_params_default(ctypes.byref(bad))
        setattr(bad, name, v)
        rc, total, _ = raw_call(gpu_ctx, g, c, bad)
        assert rc == MSW_E_INVALID and name.split("_")[0] in L.msw_last_error().decode(), name
        with pytest.raises(mpa.MswError) as e:
            gpu_ctx.call_variants(g, c, mpa.CallParams(**{name: v}))
        assert e.value.code == MSW_E_INVALID
    assert raw_call(gpu_ctx, g, c, chunk_pos=(1 << 24) + 1)[0] == MSW_E_RANGE
    assert raw_call(gpu_ctx, g, c, chunk_pos=1 << 24)[:2] == (0, len(vo.call(g, c)))
    gp, cp, n = np.frombuffer(g, np.uint8).ctypes.data, c.ctypes.data, ctypes.c_uint64()
    assert L.msw_call_counts(None, gp, 40, cp, None, 0, None, 0, ctypes.byref(n)) == MSW_E_INVALID
    assert L.msw_call_counts(gpu_ctx.handle, gp, 40, cp, None, 0, None, 0, None) == MSW_E_INVALID
    assert L.msw_call_counts(gpu_ctx.handle, gp, 40, cp, None, 0, None, 5, ctypes.byref(n)) == MSW_E_INVALID   # out NULL
    assert L.msw_call_counts(gpu_ctx.handle, None, 40, cp, None, 0, None, 0, ctypes.byref(n)) == MSW_E_INVALID
    assert L.msw_call_counts(gpu_ctx.handle, gp, 40, None, None, 0, None, 0, ctypes.byref(n)) == MSW_E_INVALID
    n.value = 9
    assert L.msw_call_counts(gpu_ctx.handle, None, 0, None, None, 0, None, 0, ctypes.byref(n)) == 0 and n.value == 0
    with pytest.raises(mpa.MswError):
        gpu_ctx.call_variants(g, c[:39])
    assert len(gpu_ctx.call_variants(b"", np.zeros((0, 8), np.uint32)).pos) == 0
    # the pileup forms: before finish, another context, out NULL with cap > 0, NULL handles
    genome = gpu_ctx.load_genome(g)
    pile = gpu_ctx.pileup(genome)
    with pytest.raises(mpa.MswError) as e:
        pile.call()
    assert e.value.code == MSW_E_INVALID and "finish" in str(e.value)
    assert L.msw_pileup_call_device(gpu_ctx.handle, pile.handle, None, None, 0, None, None) == MSW_E_INVALID
    pile.finish()
    assert len(pile.call().pos) == 0
    assert L.msw_pileup_call(fresh_ctx.handle, pile.handle, None, None, 0, ctypes.byref(n)) == MSW_E_INVALID
    assert L.msw_pileup_call(gpu_ctx.handle, None, None, None, 0, ctypes.byref(n)) == MSW_E_INVALID
    assert L.msw_pileup_call(gpu_ctx.handle, pile.handle, None, None, 0, None) == MSW_E_INVALID
    assert L.msw_pileup_call(gpu_ctx.handle, pile.handle, None, None, 3, ctypes.byref(n)) == MSW_E_INVALID
    assert L.msw_pileup_call_device(gpu_ctx.handle, pile.handle, None, None, 3, None, None) == MSW_E_INVALID
    bad = CallParamsT()
    assert L.msw_pileup_call(gpu_ctx.handle, pile.handle, ctypes.byref(bad), None, 0, ctypes.byref(n)) == MSW_E_INVALID
    pile.close()
    genome.close()


LENIENT = dict(min_depth=1, min_alt=1, min_qual=0, prior_het=0, prior_hom=0)


def pileup_calls(pile, g, params_list):
    """Pileup.call against the oracle over Pileup.counts(), twice: equal bytes."""
    from mini_parallel_amd import CallParams
    counts = pile.counts()
    sizes = []
    for over in params_list:
        want = vo.call(g, counts, vo.params(**over))
        first = pile.call(CallParams(**over) if over else None).to_records()
        again = pile.call(CallParams(**over) if over else None).to_records()
        assert first.tobytes() == want.tobytes(), (len(first), len(want))
        assert again.tobytes() == first.tobytes()
        sizes.append(len(want))
    return counts, sizes


def test_pileup_call_over_map_reads(gpu_ctx):
    from mini_parallel_amd import Scoring
    g, batch, R, rl = planted()
    genome = gpu_ctx.load_genome(g)
    index = gpu_ctx.build_index(genome, 8)
    s, ei, ej, strand, ref, nm, cigars, mq, sub, cand = gpu_ctx.map_reads(genome, index, R, rl, Scoring(2, -1, 0, 2, False, True),
                                                                          mapq=True)
    pile = gpu_ctx.pileup(genome)
    pile.add(R, rl, ref, nm, cigars, strand=strand, mapq=mq)
    pile.finish()
    counts, sizes = pileup_calls(pile, g, [{}, LENIENT, dict(LENIENT, min_depth=2)])
    assert sizes[1] > 100 and sizes[1] > sizes[2] > 0
    # the host form over the same counts gives the same records
    from mini_parallel_amd import CallParams
    assert gpu_ctx.call_variants(g, counts, CallParams(**LENIENT), 4099).to_records().tobytes() == \
        pile.call(CallParams(**LENIENT)).to_records().tobytes()
    pile.close()
    index.close()
    genome.close()


def test_planes_layout(fresh_ctx, monkeypatch):
    """MSW_PILEUP_PLANES=1: the kernels read the eight planes through their strides."""
    monkeypatch.setenv("MSW_PILEUP_PLANES", "1")
    rng = np.random.default_rng(9)
    genome = rand_genome(rng, 301)
    rec = build(rng, genome, [(int(rng.integers(0, 290)), "1S40M3D20M2I30M", None, 5) for _ in range(90)], strand=True)
    g = fresh_ctx.load_genome(genome)
    pile = fresh_ctx.pileup(g)
    assert pile.counts_device()[1:] == (1, 301)
    keep = add_device(pile, rec)
    pile.finish()
    # costs under which every covered position is called 0/1, so the records show every row
    every = dict(min_depth=1, min_alt=0, min_alt_permille=0, min_qual=0, q_hit=100, q_miss=100, q_het=1, prior_het=0,
                 prior_hom=0)
    counts, sizes = pileup_calls(pile, genome, [{}, LENIENT, every])
    assert sizes[2] > 300
    del keep
    pile.close()
    g.close()
