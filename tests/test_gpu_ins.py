"""Inserted sequences of a MSW_PILEUP_INS pileup on the GPU (msw_pileup_ins_*;
include/msw.h, "Pileup", "Inserted sequences"): the table field for field
against tests/ins_oracle.py, and events == counts[:, 6] at every site."""
import numpy as np
import pytest

import ins_oracle as io
import pileup_oracle as po
import pileup_qsum_oracle as pqs
import strand_oracle as so
from test_gpu_pileup import ACGT, Records, add_device, build, rand_genome

pytestmark = pytest.mark.gpu
TILE = 1024  # MSW_INS_VOTE_TILE


def with_runs(rng, genome, specs, **kw):
    """build() of (ref, cigar, read_len, [bytes of I run 0, 1, ...]); a run without bytes is random ACGT"""
    rec = build(rng, genome, [s[:3] + (0,) for s in specs], **kw)
    for p, spec in enumerate(specs):
        i, runs = 0, list(spec[3]) if len(spec) > 3 else []
        for word in rec.cigars[p]:
            ln, kind = int(word) >> 4, int(word) & 15
            if kind == po.OP_I:
                fill = runs.pop(0) if runs else ACGT[rng.integers(0, 4, ln)].tobytes()
                rec.rows[p, i:i + ln] = np.frombuffer(fill, np.uint8)[:max(0, rec.rows.shape[1] - i)][:ln]
            if kind != po.OP_D:
                i += ln
    return rec


def events_of(glen, rec, min_mapq=0, **kw):
    return io.events(glen, rec.rows, rec.rl, rec.ref, rec.nm, rec.cigars, rec.strand, rec.mapq, min_mapq, **kw)


def compare(pile, ev):
    """finish(), then table == oracle and events == channel 6 everywhere; returns the counts."""
    pile.finish()
    got, want, counts = pile.insertions(), io.table(ev), pile.counts()
    assert io.as_tuples(got) == want
    assert np.array_equal(np.flatnonzero(counts[:, 6]), got["pos"]) and np.array_equal(counts[got["pos"], 6], got["events"])
    info = pile.ins_info()
    assert (info["events"], info["dropped"], info["sites"]) == (sum(len(v) for v in ev.values()), 0, len(want))
    return counts


def check(ctx, genome, batches, min_mapq=0, **kw):
    g = ctx.load_genome(genome)
    pile, plain, ev = ctx.pileup(g, ins=True), ctx.pileup(g), {}
    keep = [add_device(pl, rec, min_mapq, **kw) for rec in batches for pl in (pile, plain)]
    for rec in batches:
        events_of(len(genome), rec, min_mapq, into=ev)
    counts = compare(pile, ev)
    plain.finish()
    assert np.array_equal(plain.counts(), counts)        # the flag changes no count
    del keep
    return ev


def test_lengths_placements_and_bases(gpu_ctx):
    rng = np.random.default_rng(1)
    glen = 400
    genome = rand_genome(rng, glen)
    specs = [(10 * k, "6M%dI6M" % ln, None) for k, ln in enumerate((1, 2, 31, 32, 33, 100))]
    specs += [(100, "3S4I9M", None), (110, "9M4I", None),                      # directly after an S, as the last op
              (120, "8M6I8M", 11), (130, "8M6I8M", 8), (140, "8M40I", 20),      # i + len crosses read_len, starts at it
              (150, "8M5I8M", None, [b"ACgTA"]), (150, "8M5I8M", None, [b"ACNTA"]), (150, "8M5I8M", None, [b"AC\0TA"]),
              (160, "4M2I4M3I4M", None, [b"GT", b"CCA"]), (160, "4M2I4M3I4M", None, [b"GT", b"CCA"]),   # two runs a read
              (0, "2I5M", None), (glen - 3, "3M2I", None), (glen, "3I", None), (glen - 1, "1M1D2I", None)]
    ev = check(gpu_ctx, genome, [with_runs(rng, genome, specs, stride=128)])
    assert ev[163] == [(2, 0, 2 | 3 << 2)] * 2 and ev[167] == [(3, 0, 1 | 1 << 2)] * 2 and -1 not in ev
    assert ev[157] == [(5, io.OTHER, 0)] * 3 and glen - 1 in ev and ev[127][0][1] == io.OTHER


@pytest.mark.parametrize("depth", [1, 2, 63, 64, 65, 200, pytest.param(TILE + 1, id="MSW_INS_VOTE_TILE+1")])
def test_site_depth_with_mixed_alleles(gpu_ctx, depth):
    """One site `depth` events deep and a shallow neighbour; A and C tie where depth % 7 is not 1 or 4."""
    rng = np.random.default_rng(depth)
    genome = rand_genome(rng, 200)
    alleles = [b"A", b"C", b"AA", b"A", b"C", b"ACNGT", b"T" * 33]
    order = rng.permutation(depth)
    specs = [(50, "7M%dI7M" % len(alleles[k % 7]), None, [alleles[k % 7]]) for k in order]
    specs += [(52, "7M2I7M", None, [b"GG"]), (52, "7M2I7M", None, [b"GT"]), (52, "7M2I7M", None, [b"GG"])]
    ev = check(gpu_ctx, genome, [with_runs(rng, genome, specs, stride=48)])
    assert len(ev[56]) == depth and io.table(ev)[1][3:5] == (2, 1)


def test_strand_1_device_and_host_form_agree(gpu_ctx):
    rng = np.random.default_rng(3)
    genome = rand_genome(rng, 300)
    specs = [(int(rng.integers(0, 250)), c, None) for c in ("20M3I20M", "2S9M33I9M", "12M1I5M2D6M4I3M") for _ in range(15)]
    rec = with_runs(rng, genome, specs, stride=64, strand=True, mapq=True)
    ev = check(gpu_ctx, genome, [rec], min_mapq=20)
    given = rec.rows.copy()
    for p in np.flatnonzero(rec.strand):
        L = int(rec.rl[p])
        given[p, :L] = np.frombuffer(so.revcomp(rec.rows[p, :L].tobytes()), np.uint8)
    flipped = Records(given, rec.rl, rec.ref, rec.nm, rec.cigars, rec.strand, rec.mapq)
    assert events_of(300, flipped, 20, flip=True) == ev
    g = gpu_ctx.load_genome(genome)
    pile = gpu_ctx.pileup(g, ins=True)
    pile.add(given, rec.rl, rec.ref, rec.nm, rec.cigars, strand=rec.strand, mapq=rec.mapq, min_mapq=20, chunk_reads=7)
    compare(pile, ev)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_skipped_reads_and_the_lane_per_read_boundary(gpu_ctx, n):
    rng = np.random.default_rng(4)
    genome = rand_genome(rng, 300)
    rec = with_runs(rng, genome, [(int(rng.integers(0, 250)), "9M3I9M", None) for _ in range(65)], stride=32, mapq=True)
    rec.mapq[:] = 30
    rec.ref[2], rec.nm[3], rec.mapq[5] = -4, -1, 9
    part = Records(rec.rows[:n], rec.rl[:n], rec.ref[:n], rec.nm[:n], rec.cigars[:n], None, rec.mapq[:n])
    ev = check(gpu_ctx, genome, [part], min_mapq=10)
    assert sum(len(v) for v in ev.values()) == n - sum(k < n for k in (2, 3, 5))
    if n == 65:      # reads whose ops end past cigar_cap are skipped: the oracle sees them without ops
        cap = int(part.packed()[0][40])
        cut = Records(rec.rows, rec.rl, rec.ref, rec.nm, rec.cigars[:40] + [None] * 25, None, rec.mapq)
        g = gpu_ctx.load_genome(genome)
        pile = gpu_ctx.pileup(g, ins=True)
        keep = add_device(pile, part, 10, cap=cap)
        compare(pile, events_of(300, cut, 10))
        del keep


def test_two_streams_against_one_add_and_quality_sums(gpu_ctx):
    import torch
    rng = np.random.default_rng(5)
    genome = rand_genome(rng, 300)
    specs = [(int(rng.integers(0, 40)) * 6, c, None) for c in ("20M2I20M", "9M1I30M", "30M") for _ in range(40)]
    a, b = (with_runs(rng, genome, specs, stride=48, strand=True) for _ in range(2))
    ev = check(gpu_ctx, genome, [a + b])
    g = gpu_ctx.load_genome(genome)
    pile = gpu_ctx.pileup(g, ins=True)
    streams = [torch.cuda.Stream() for _ in range(2)]
    keep = [add_device(pile, r, stream=s.cuda_stream) for r, s in zip((a, b), streams)]
    torch.cuda.synchronize()
    compare(pile, ev)
    # MSW_PILEUP_QSUM | MSW_PILEUP_INS through the host add_qual: the oriented rows, no strand flip
    both = a + b
    quals = (33 + rng.integers(0, 42, both.rows.shape)).astype(np.uint8)
    pile = gpu_ctx.pileup(g, qsum=True, ins=True)
    pile.add(both.rows, both.rl, both.ref, both.nm, both.cigars, quals=quals, min_baseq=15, chunk_reads=50)
    counts = compare(pile, ev)
    want = pqs.pileup(genome, both.rows, both.rl, both.ref, both.nm, both.cigars, quals, None, None, 0, 48, 15)
    assert np.array_equal(counts, want[0]) and np.array_equal(pile.qsums(), want[1])
    del keep


def test_a_full_log_and_the_error_paths(gpu_ctx):
    import mini_parallel_amd as mpa
    from mini_parallel_amd._lib import MSW_E_INVALID, MSW_E_RANGE
    rng = np.random.default_rng(6)
    genome = rand_genome(rng, 100)
    rec = with_runs(rng, genome, [(10 * k, "9M3I9M", None) for k in range(5)], stride=32)
    g = gpu_ctx.load_genome(genome)
    pile = gpu_ctx.pileup(g, ins=True, ins_capacity=4)
    with pytest.raises(mpa.MswError) as e:                   # before the finish
        pile.insertions()
    assert e.value.code == MSW_E_INVALID and "finish" in str(e.value)
    pile.add(rec.rows, rec.rl, rec.ref, rec.nm, rec.cigars)
    info = pile.ins_info()
    assert (info["events"], info["dropped"], info["sites"], info["capacity"]) == (5, 1, 0, 4)
    assert mpa._lib.lib().msw_pileup_ins_capacity(gpu_ctx.handle, pile.handle, 8) == MSW_E_INVALID    # after an add
    pile.finish()
    with pytest.raises(mpa.MswError) as e:
        pile.insertions()
    assert e.value.code == MSW_E_RANGE and pile.ins_info()["sites"] == 0
    assert np.array_equal(pile.counts(), po.pileup(genome, rec.rows, rec.rl, rec.ref, rec.nm, rec.cigars)[0])
    fresh = gpu_ctx.pileup(g, qsum=True, ins=True)
    assert [mpa._lib.lib().msw_pileup_ins_capacity(gpu_ctx.handle, fresh.handle, n) for n in (0, 2 ** 31)] == [MSW_E_RANGE] * 2
    assert fresh.ins_info() == {"events": 0, "dropped": 0, "sites": 0, "capacity": 2 ** 20}
    plain = gpu_ctx.pileup(g)
    assert not plain.ins
    for f in (plain.ins_info, plain.insertions, lambda: mpa._lib.check(
            mpa._lib.lib().msw_pileup_ins_capacity(gpu_ctx.handle, plain.handle, 8))):
        with pytest.raises(mpa.MswError) as e:
            f()
        assert e.value.code == MSW_E_INVALID and "MSW_PILEUP_INS" in str(e.value)
    assert mpa._lib.lib().msw_pileup_ins_sites_device(gpu_ctx.handle, plain.handle, None, None) == MSW_E_INVALID


def test_map_reads_to_a_vcf_line_with_the_planted_bases(gpu_ctx, tmp_path):
    from mini_parallel_amd import AFFINE, ins_sequence, write_vcf
    rng = np.random.default_rng(7)
    g = bytearray(ACGT[rng.integers(0, 4, 4000)].tobytes())
    P, INS = 2000, b"CGTCG"
    g[P - 1:P + 1] = b"AA"            # the anchor and the base after: the run cannot slide either way
    g = bytes(g)
    reads = [g[s:P] + INS + g[P:s + 95] for s in range(P - 70, P - 22, 4)]       # a dozen with the insertion
    reads += [g[s:s + 100] for s in range(P - 90, P + 10, 5)]
    reads = [so.revcomp(r) if k % 2 else r for k, r in enumerate(reads)]
    R = np.frombuffer(b"".join(reads), np.uint8).reshape(len(reads), 100)
    rl = np.full(len(reads), 100, np.uint16)
    genome = gpu_ctx.load_genome(g)
    index = gpu_ctx.build_index(genome, 8)
    s, ei, ej, strand, ref, nm, cigars, mq, sub, cand = gpu_ctx.map_reads(genome, index, R, rl, AFFINE, mapq=True)
    pile = gpu_ctx.pileup(genome, ins=True)
    pile.add(R, rl, ref, nm, cigars, strand=strand, mapq=mq)
    ev = io.events(len(g), R, rl, ref, nm, cigars, strand, mq, 0, flip=True)
    compare(pile, ev)
    table = pile.insertions()
    top = table[np.argmax(table["events"])]
    assert int(top["pos"]) == P - 1 and int(top["events"]) == 12 == int(top["best_count"])
    assert ins_sequence(int(top["best_len"]), int(top["seq"])) == INS
    write_vcf(tmp_path / "v.vcf", pile.call(), g, insertions=table)
    body = [ln.split("\t") for ln in open(tmp_path / "v.vcf").read().splitlines() if not ln.startswith("#")]
    assert [(b[3], b[4]) for b in body if b[1] == str(P)] == [("A", "A" + INS.decode())]
