"""Hand-worked sites for tests/variant_oracle.py, the restatement of the caller
in include/msw.h ("Variants").  Every expected number below was worked out by
hand from the definition's integers (q_hit 4, q_miss 2477, q_het 304,
prior_het 3000, prior_hom 3301)."""
import numpy as np
import pytest

import variant_oracle as vo

U32 = 2 ** 32 - 1


def row(a=0, c=0, g=0, t=0, other=0, dele=0, ins=0, rev=0):
    return [a, c, g, t, other, dele, ins, rev]


def one(rec):
    assert len(rec) == 1
    r = rec[0]
    return {k: (r[k].tolist() if k == "pl" else int(r[k])) for k in ("pos", "depth", "ref_count", "alt_count", "qual",
                                                                     "pl", "kind", "ref", "alt", "gt", "gq")}


def test_sanity_rows_of_the_defaults():
    p = vo.params()
    # ref 10 / alt 10: raw 24810, 6080, 24810; post 24810, 9080, 28111
    assert vo.genotype(10, 10, p) == (1, 157, 99, [187, 0, 187])
    # 0 / 20: raw 49540, 6080, 80; post 49540, 9080, 3381
    assert vo.genotype(0, 20, p) == (2, 462, 57, [495, 60, 0])
    # 17 / 3: raw 7499, 6080, 42121; post 7499, 9080, 45422 -> 0/0 (and 3000 < 200 * 20: no candidate either)
    assert vo.genotype(17, 3, p)[0] == 0
    assert vo.site(20, 17, 3, p) is None
    # 2 / 2: raw 4962, 1216, 4962; post 4962, 4216, 8263 -> 0/1 with qual 7, below min_qual
    assert vo.genotype(2, 2, p)[:2] == (1, 7)
    assert vo.site(4, 2, 2, p) is None
    assert vo.site(4, 2, 2, vo.params(min_qual=7))["qual"] == 7
    assert vo.site(4, 2, 2, vo.params(min_qual=8)) is None


def test_snv_record_fields():
    # genome G; 10 G, 10 T and 3 "other" reads, which say nothing
    rec = one(vo.call(b"G", [row(g=10, t=10, other=3, rev=9)]))
    assert rec == dict(pos=0, depth=20, ref_count=10, alt_count=10, qual=157, pl=[187, 0, 187], kind=vo.SNV,
                       ref=ord("G"), alt=ord("T"), gt=1, gq=99)
    assert bytes(vo.call(b"G", [row(g=10, t=10)])[0]["pad"]) == bytes(7)


def test_alternative_tie_takes_the_lowest_channel():
    # C, G and the deletion channel tie at 8: C (channel 1) wins
    assert one(vo.call(b"A", [row(a=2, c=8, g=8, dele=8)]))["alt"] == ord("C")
    # G and the deletion channel tie: G (channel 2 < 5), an SNV
    r = one(vo.call(b"A", [row(a=2, g=8, dele=8)]))
    assert (r["kind"], r["alt"], r["depth"], r["alt_count"]) == (vo.SNV, ord("G"), 18, 8)
    # the deletion channel alone on top: a DEL, alt 0
    r = one(vo.call(b"A", [row(a=2, g=7, dele=8)]))
    assert (r["kind"], r["alt"], r["alt_count"], r["ref_count"]) == (vo.DEL, 0, 8, 2)
    # the reference channel is never the alternative, however high
    assert one(vo.call(b"T", [row(t=9, a=9)]))["alt"] == ord("A")


def test_post_tie_takes_the_lowest_genotype():
    # ref 2, a 6, q_hit 0, q_miss 40, q_het 10, no priors: raw = post = 240, 80, 80 -> 0/1
    p = vo.params(q_hit=0, q_miss=40, q_het=10, prior_het=0, prior_hom=0, min_qual=0)
    assert vo.genotype(2, 6, p) == (1, 2, 0, [2, 0, 0])
    # all three equal: 0/0, nothing is emitted
    z = vo.params(q_hit=0, q_miss=0, q_het=0, prior_het=0, prior_hom=0, min_qual=0)
    assert vo.genotype(5, 5, z)[0] == 0 and len(vo.call(b"A", [row(a=5, c=5)], z)) == 0
    # 0/0 and 0/1 tie: 0/0
    t = vo.params(q_hit=0, q_miss=10, q_het=5, prior_het=0, prior_hom=50, min_qual=0)
    assert vo.genotype(4, 4, t)[0] == 0          # raw 40, 40, 40; post 40, 40, 90


def test_insertion_at_the_last_position_and_inside():
    # depth(glen) is 0: span 0, ref 0, n = a = 5; raw 12385, 1520, 20; post 12385, 4520, 3321
    counts = [row(a=9), row(a=9, ins=5)]
    rec = one(vo.call(b"AA", counts))
    assert rec == dict(pos=1, depth=5, ref_count=0, alt_count=5, qual=91, pl=[124, 15, 0], kind=vo.INS, ref=ord("A"),
                       alt=0, gt=2, gq=12)
    # inside: span = min(12, 20) = 12, ref 6, a 6, n 12; raw 14886, 3648, 14886 -> 0/1, qual (14886 - 6648 + 50) / 100
    rec = one(vo.call(b"CCA", [row(c=12, ins=6), row(c=20), row(a=1)]))
    assert (rec["pos"], rec["kind"], rec["depth"], rec["ref_count"], rec["alt_count"], rec["gt"], rec["qual"]) == \
        (0, vo.INS, 12, 6, 6, 1, 82)
    # more insertions than spanning reads: ref 0
    rec = one(vo.call(b"CC", [row(c=3, ins=6), row(c=2)]))
    assert (rec["depth"], rec["ref_count"], rec["alt_count"], rec["gt"]) == (6, 0, 6, 2)


def test_non_acgt_genome_byte_has_no_column_record_but_an_insertion():
    counts = [row(a=10, c=10, ins=10), row(a=20)]
    for g in (b"NA", b"aA", b"\x00A"):
        rec = one(vo.call(g, counts))
        assert (rec["kind"], rec["ref"]) == (vo.INS, g[0])
    both = vo.call(b"AA", counts)
    assert [int(k) for k in both["kind"]] == [vo.SNV, vo.INS] and [int(k) for k in both["pos"]] == [0, 0]


def test_two_records_order_column_first_then_by_position():
    counts = [row(a=10, dele=10, ins=10), row(a=0, t=20, ins=20), row(a=20)]
    rec = vo.call(b"AAA", counts)
    assert [(int(r["pos"]), int(r["kind"])) for r in rec] == [(0, vo.DEL), (0, vo.INS), (1, vo.SNV), (1, vo.INS)]


@pytest.mark.parametrize("name,at,below", [
    ("min_depth", 20, 21), ("min_alt", 10, 11), ("min_qual", 157, 158),
])
def test_thresholds_at_equality_and_one_past(name, at, below):
    counts = [row(a=10, c=10)]
    assert len(vo.call(b"A", counts, vo.params(**{name: at}))) == 1
    assert len(vo.call(b"A", counts, vo.params(**{name: below}))) == 0


def test_permille_at_equality_and_one_below():
    p = vo.params(min_alt_permille=500)
    assert len(vo.call(b"A", [row(a=10, c=10)], p)) == 1     # 10000 >= 500 * 20
    assert len(vo.call(b"A", [row(a=11, c=10)], p)) == 0     # 10000 < 500 * 21
    assert len(vo.call(b"A", [row(a=11, c=10)])) == 1        # a het call under the default 200
    # the default at equality: a 2, n 10 is a candidate, but 0/0 wins (raw 4986, 3040; post 4986, 6040)
    assert vo.site(10, 8, 2, vo.params()) is None and vo.genotype(8, 2, vo.params())[0] == 0


def test_saturating_counts():
    # every channel 2^32 - 1 over genome A: n = 5 * U32 (1000 * U32 >= 200 * 5 * U32 holds at equality),
    # ref = a = U32 (C: the lowest channel of the tie); raw U32 * 2481, U32 * 608, U32 * 2481 -> 0/1
    full = [U32] * 8
    rec = vo.call(b"A", [full])
    assert len(rec) == 2
    col = {k: rec[0][k].tolist() for k in rec.dtype.names}
    assert (col["kind"], col["alt"], col["gt"], col["gq"]) == (vo.SNV, ord("C"), 1, 99)
    assert (col["depth"], col["ref_count"], col["alt_count"], col["qual"], col["pl"]) == (U32, U32, U32, U32, [U32, 0, U32])
    # the insertion behind the only position: span 0, n = a = U32 -> 1/1, everything saturates
    ins = {k: rec[1][k].tolist() for k in rec.dtype.names}
    assert (ins["kind"], ins["gt"], ins["depth"], ins["ref_count"], ins["alt_count"], ins["qual"]) == \
        (vo.INS, 2, U32, 0, U32, U32)
    assert ins["pl"] == [U32, U32, 0]       # (U32 * 608 - U32 * 4 + 50) / 100 = about 6 * U32: saturated too
    # two full rows: span 6 * U32, ref 5 * U32 saturates in the record; a candidate only under a lower permille
    assert [int(k) for k in vo.call(b"AA", [full, full])["kind"]] == [vo.SNV, vo.SNV, vo.INS]
    # (raw U32 * 2497, U32 * 1824, U32 * 12389 -> 0/1)
    rec = vo.call(b"NN", [full, full], vo.params(min_alt_permille=100))
    assert [(int(r["pos"]), int(r["kind"])) for r in rec] == [(0, vo.INS), (1, vo.INS)]
    first = {k: rec[0][k].tolist() for k in rec.dtype.names}
    assert (first["pos"], first["kind"], first["depth"], first["ref_count"], first["alt_count"], first["gt"]) == \
        (0, vo.INS, U32, U32, U32, 1)


def test_depth_is_the_sum_of_channels_0_to_5():
    counts = np.array([[1, 2, 3, 4, 5, 6, 70, 80]], np.uint32)
    assert vo.depth(counts, 0) == 21 and vo.depth(counts, 1) == 0
    assert vo.depth(np.full((1, 8), U32, np.uint32), 0) == 6 * U32
    assert [vo.code(b) for b in b"ACGTNacgt\x00"] == [0, 1, 2, 3, 4, 4, 4, 4, 4, 4]
