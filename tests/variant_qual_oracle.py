"""The weighted caller of include/msw.h ("Quality sums and weighted
genotypes"), restated position by position beside tests/variant_oracle.py.

Plain Python integers over finished counts and quality sums; it shares nothing
with the kernels (msw_call.hip).  Only raw[] of a column site differs from
"Variants": everything behind it (posteriors, genotype, pl, qual, gq,
emission) is written out again here rather than borrowed, so that the two
oracles can be compared with each other as well (the Q20 invariant).
"""
import numpy as np

import variant_oracle as vo

QDEFAULTS = dict(q_scale=100, q_third=477)
U32 = vo.U32


def qparams(**over) -> dict:
    q = dict(QDEFAULTS)
    for k, v in over.items():
        assert k in q, k
        q[k] = int(v)
    return q


def numbers(n, ref, a, raw, p):
    """The record's numbers from raw[0..2] when the site is a candidate and is emitted, else None."""
    if not (n >= p["min_depth"] and a >= p["min_alt"] and 1000 * a >= p["min_alt_permille"] * n):
        return None
    post = [raw[0], raw[1] + p["prior_het"], raw[2] + p["prior_hom"]]
    gt = 0
    for g in (1, 2):
        if post[g] < post[gt]:
            gt = g
    qual = min((post[0] - post[gt] + 50) // 100, U32)
    if gt == 0 or qual < p["min_qual"]:
        return None
    lowest = min(raw)
    pl = [min((r - lowest + 50) // 100, U32) for r in raw]
    rest = [post[g] for g in range(3) if g != gt]
    gq = min(99, (min(rest) - post[gt] + 50) // 100)
    return dict(depth=min(n, U32), ref_count=min(ref, U32), alt_count=min(a, U32), qual=qual, pl=pl, gt=gt, gq=gq)


def column(row, qrow, gbyte, p, q):
    """The weighted column record (SNV or DEL) of one position, or None."""
    r = vo.code(gbyte)
    if r >= 4:
        return None
    c = [int(v) for v in row]
    w = [int(v) for v in qrow]
    n = c[0] + c[1] + c[2] + c[3] + c[5]
    alt_ch, a = None, -1
    for ch in (0, 1, 2, 3, 5):
        if ch != r and c[ch] > a:                    # the highest count, the lowest channel index on a tie
            alt_ch, a = ch, c[ch]
    ref = c[r]
    wref = q["q_scale"] * w[r] + q["q_third"] * ref
    walt = q["q_scale"] * w[alt_ch] + q["q_third"] * a if alt_ch < 4 else a * p["q_miss"]
    raw = [ref * p["q_hit"] + walt, (ref + a) * p["q_het"], wref + a * p["q_hit"]]
    rec = numbers(n, ref, a, raw, p)
    if rec is None:
        return None
    rec.update(kind=vo.DEL if alt_ch == 5 else vo.SNV, ref=int(gbyte), alt=0 if alt_ch == 5 else b"ACGT"[alt_ch])
    return rec


def call(genome, counts, qsums, p=None, q=None):
    """-> the records as a variant_oracle.RECORD array, ordered by pos, then kind."""
    p, q = p or vo.params(), q or qparams()
    g = bytes(genome) if isinstance(genome, (bytes, bytearray)) else bytes(np.asarray(genome, np.uint8).tobytes())
    assert len(g) == len(counts) == len(qsums)
    if isinstance(counts, np.ndarray):
        counts = counts.tolist()
    if isinstance(qsums, np.ndarray):
        qsums = qsums.tolist()
    out = []
    for pos in range(len(g)):
        # insertion sites keep the unweighted formula
        for rec in (column(counts[pos], qsums[pos], g[pos], p, q), vo.insertion(counts, pos, g[pos], p)):
            if rec is not None:
                rec["pos"] = pos
                out.append(rec)
    arr = np.zeros(len(out), vo.RECORD)
    if out:
        for name in out[0]:
            arr[name] = [rec[name] for rec in out]
    return arr
