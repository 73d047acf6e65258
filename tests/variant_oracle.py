"""The caller of include/msw.h ("Variants"), restated position by position.

Plain Python integers over finished pileup counts: no numpy arithmetic, no
sharing with the kernels (msw_call.hip), so the two can be compared value for
value.  The parameters are the integers of the definition, not the formulas
they came from.
"""
import numpy as np

SNV, DEL, INS = 0, 1, 2
U32 = 2 ** 32 - 1
DEFAULTS = dict(min_depth=4, min_alt=2, min_alt_permille=200, min_qual=20, q_hit=4, q_miss=2477, q_het=304,
                prior_het=3000, prior_hom=3301)
RECORD = np.dtype([("pos", "<u8"), ("depth", "<u4"), ("ref_count", "<u4"), ("alt_count", "<u4"), ("qual", "<u4"),
                   ("pl", "<u4", (3,)), ("kind", "u1"), ("ref", "u1"), ("alt", "u1"), ("gt", "u1"), ("gq", "u1"),
                   ("pad", "u1", (7,))])
assert RECORD.itemsize == 48


def params(**over) -> dict:
    p = dict(DEFAULTS)
    for k, v in over.items():
        assert k in p, k
        p[k] = int(v)
    return p


def code(byte) -> int:
    return {65: 0, 67: 1, 71: 2, 84: 3}.get(int(byte), 4)


def depth(counts, pos) -> int:
    """The sum of channels 0..5; depth(glen) is 0."""
    return sum(int(counts[pos][ch]) for ch in range(6)) if pos < len(counts) else 0


def genotype(ref, a, p):
    """-> (gt, qual, gq, pl) of a site with `ref` reference and `a` alternative observations."""
    raw = [ref * p["q_hit"] + a * p["q_miss"], (ref + a) * p["q_het"], ref * p["q_miss"] + a * p["q_hit"]]
    post = [raw[0], raw[1] + p["prior_het"], raw[2] + p["prior_hom"]]
    gt = post.index(min(post))                       # the lowest g on a tie
    pl = [min((r - min(raw) + 50) // 100, U32) for r in raw]
    qual = min((post[0] - min(post) + 50) // 100, U32)
    ordered = sorted(post)
    gq = min(99, (ordered[1] - ordered[0] + 50) // 100)
    return gt, qual, gq, pl


def site(n, ref, a, p):
    """The record's numbers when the site (n, ref, a) is a candidate and is emitted, else None."""
    if not (n >= p["min_depth"] and a >= p["min_alt"] and 1000 * a >= p["min_alt_permille"] * n):
        return None
    gt, qual, gq, pl = genotype(ref, a, p)
    if gt == 0 or qual < p["min_qual"]:
        return None
    return dict(depth=min(n, U32), ref_count=min(ref, U32), alt_count=min(a, U32), qual=qual, pl=pl, gt=gt, gq=gq)


def column(row, gbyte, p):
    """The column record (SNV or DEL) of one position, or None."""
    r = code(gbyte)
    if r >= 4:
        return None
    c = [int(v) for v in row]
    n = c[0] + c[1] + c[2] + c[3] + c[5]
    alt_ch, a = None, -1
    for ch in [k for k in (0, 1, 2, 3) if k != r] + [5]:
        if c[ch] > a:                                # the lowest channel index on a tie
            alt_ch, a = ch, c[ch]
    rec = site(n, c[r], a, p)
    if rec is None:
        return None
    rec.update(kind=DEL if alt_ch == 5 else SNV, ref=int(gbyte), alt=0 if alt_ch == 5 else b"ACGT"[alt_ch])
    return rec


def insertion(counts, pos, gbyte, p):
    """The insertion record after position pos, or None."""
    a = int(counts[pos][6])
    span = min(depth(counts, pos), depth(counts, pos + 1))
    ref = span - a if span > a else 0
    rec = site(ref + a, ref, a, p)
    if rec is None:
        return None
    rec.update(kind=INS, ref=int(gbyte), alt=0)
    return rec


def call(genome, counts, p=None):
    """-> the records as a RECORD array, ordered by pos, then kind."""
    p = p or params()
    g = bytes(genome) if isinstance(genome, (bytes, bytearray)) else bytes(np.asarray(genome, np.uint8).tobytes())
    assert len(g) == len(counts)
    if isinstance(counts, np.ndarray):
        counts = counts.tolist()                     # Python integers from here on
    out = []
    for pos in range(len(g)):
        for rec in (column(counts[pos], g[pos], p), insertion(counts, pos, g[pos], p)):
            if rec is not None:
                rec["pos"] = pos
                out.append(rec)
    arr = np.zeros(len(out), RECORD)
    if out:
        for name in out[0]:
            arr[name] = [rec[name] for rec in out]
    return arr
