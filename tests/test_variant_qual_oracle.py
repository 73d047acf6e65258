"""tests/variant_qual_oracle.py against sites worked out by hand from
include/msw.h ("Quality sums and weighted genotypes"), and against
tests/variant_oracle.py where every base is Q20."""
import numpy as np

import variant_oracle as vo
import variant_qual_oracle as vq


def site(ref_q, alt_q, ref=8, alt=4, alt_ch=2):
    """One A position with `ref` reference observations at Phred ref_q and `alt` at alt_q on alt_ch."""
    counts = np.zeros((1, 8), np.uint32)
    qsums = np.zeros((1, 4), np.uint32)
    counts[0, 0], counts[0, alt_ch] = ref, alt
    qsums[0, 0] = ref * ref_q
    if alt_ch < 4:
        qsums[0, alt_ch] = alt * alt_q
    return counts, qsums


def test_the_worked_sites():
    """8 ref + 4 alt at min_qual 20.
    Unweighted: raw = [8*4 + 4*2477, 12*304, 8*2477 + 4*4] = [9940, 3648, 19832];
    post = [9940, 6648, 23133]: 0/1, qual = (9940 - 6648 + 50) // 100 = 33."""
    counts, qsums = site(20, 20)
    rec = vo.call(b"A", counts)
    assert len(rec) == 1 and (int(rec["gt"][0]), int(rec["qual"][0])) == (1, 33)
    # alts at Q5, refs at Q37: Walt = 100*20 + 477*4 = 3908, raw[0] = 32 + 3908 = 3940 < post[1] = 6648: 0/0
    counts, qsums = site(37, 5)
    assert len(vq.call(b"A", counts, qsums)) == 0 and len(vo.call(b"A", counts)) == 1
    # all at Q37: Walt = 100*148 + 1908 = 16708, raw[0] = 16740, qual = (16740 - 6648 + 50) // 100 = 101
    counts, qsums = site(37, 37)
    rec = vq.call(b"A", counts, qsums)
    assert len(rec) == 1 and (int(rec["gt"][0]), int(rec["qual"][0])) == (1, 101)
    # Wref = 100*296 + 477*8 = 33416, raw[2] = 33416 + 16 = 33432; pl from raw - 3648
    assert [int(v) for v in rec["pl"][0]] == [(16740 - 3648 + 50) // 100, 0, (33432 - 3648 + 50) // 100]
    assert (int(rec["depth"][0]), int(rec["ref_count"][0]), int(rec["alt_count"][0])) == (12, 8, 4)
    assert (int(rec["kind"][0]), bytes([rec["ref"][0], rec["alt"][0]])) == (vo.SNV, b"AG")
    # at Q20 the weighted record is the unweighted one
    counts, qsums = site(20, 20)
    assert vq.call(b"A", counts, qsums).tobytes() == vo.call(b"A", counts).tobytes()


def test_a_deletion_has_no_base_quality():
    counts, qsums = site(37, 0, alt_ch=5)
    rec = vq.call(b"A", counts, qsums)
    # raw[0] = 8*4 + 4*q_miss = 9940 as unweighted; raw[2] = Wref + 16 = 33432
    assert len(rec) == 1 and int(rec["kind"][0]) == vo.DEL and int(rec["qual"][0]) == 33
    assert int(rec["pl"][0][2]) == (33432 - 3648 + 50) // 100


def test_the_alternative_is_chosen_by_count_not_by_quality():
    counts = np.array([[8, 3, 4, 0, 0, 0, 0, 0]], np.uint32)
    qsums = np.array([[8 * 37, 3 * 41, 4 * 30, 0]], np.uint32)
    lenient = vo.params(min_qual=0, prior_het=0, prior_hom=0)
    rec = vq.call(b"A", counts, qsums, lenient)
    assert len(rec) == 1 and rec["alt"][0] == ord("G") and int(rec["alt_count"][0]) == 4


def test_weights_scale_the_costs():
    counts, qsums = site(37, 37)
    a = vq.call(b"A", counts, qsums, None, vq.qparams(q_scale=0, q_third=2477))
    assert a.tobytes() == vo.call(b"A", counts).tobytes()
    b = vq.call(b"A", counts, qsums, None, vq.qparams(q_scale=65535, q_third=65535))
    assert int(b["qual"][0]) == (32 + 65535 * 148 + 65535 * 4 - 6648 + 50) // 100


def random_q20(rng, glen):
    g = rng.choice(np.frombuffer(b"ACGTACGTNa", np.uint8), glen).tobytes()
    counts = rng.integers(0, 30, (glen, 8)).astype(np.uint32)
    counts[rng.random(glen) < 0.3, 5] = 40               # DEL alternatives
    counts[rng.random(glen) < 0.3, 6] = 25               # INS sites
    counts[rng.random(glen) < 0.2] = 0
    counts[rng.random((glen, 8)) < 0.4] = 0
    return g, counts, (counts[:, :4] * 20).astype(np.uint32)


def test_q20_invariant_on_random_counts():
    rng = np.random.default_rng(11)
    kinds = set()
    for glen in (1, 50, 400):
        for p in (None, vo.params(min_depth=1, min_alt=1, min_qual=0, prior_het=0, prior_hom=0)):
            g, counts, qsums = random_q20(rng, glen)
            want = vo.call(g, counts, p)
            got = vq.call(g, counts, qsums, p)
            assert got.tobytes() == want.tobytes()
            kinds |= set(int(k) for k in want["kind"])
    assert kinds == {vo.SNV, vo.DEL, vo.INS}


def test_insertions_are_unweighted_and_n_positions_have_no_column_record():
    counts = np.array([[10, 0, 0, 0, 0, 0, 6, 0], [10, 0, 6, 0, 0, 0, 0, 0]], np.uint32)
    qsums = np.array([[20, 0, 0, 0], [370, 0, 222, 0]], np.uint32)
    rec = vq.call(b"AN", counts, qsums)
    assert [int(k) for k in rec["kind"]] == [vo.INS]
    assert rec.tobytes() == vo.call(b"AN", counts).tobytes()
