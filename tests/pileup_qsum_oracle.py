"""The quality sums of include/msw.h ("Quality sums and weighted genotypes"),
restated column by column beside tests/pileup_qual_oracle.py.

Plain Python integers: every counted M column adds 1 to its channel and, where
the read byte's code is below 4, its Phred value to qsum[pos][code].  It shares
nothing with the kernel's difference form (msw_pileup.hip), so the two can be
compared value for value.  Unlike the threshold's oracle it takes min_baseq 0
as a threshold too: a column then counts when its quality byte exists
(t < qual_stride).
"""
import numpy as np

import pileup_oracle as po

QCHANNELS = 4
MOD = 1 << 32


def phred(byte) -> int:
    """The Phred value of a FASTQ quality byte: b - 33, and 0 below 33."""
    b = int(byte)
    return b - 33 if b >= 33 else 0


def new_qsums(glen) -> np.ndarray:
    return np.zeros((glen, QCHANNELS), np.uint32)


def add(counts, qsums, rows, read_len, ref_pos, nm, cigars, quals, strand=None, mapq=None, min_mapq=0,
        qual_stride=None, min_baseq=0):
    """Adds the batch's records to counts[glen][8] and qsums[glen][4] in place;
    returns (reads_used, reads_skipped, lowq_columns).

    rows[p] are the bytes the CIGAR of read p refers to (the oriented read);
    quals[p] the quality bytes of read p AS GIVEN, of which the first
    qual_stride (default: all of quals[p]) exist."""
    glen = counts.shape[0]
    used = skipped = lowq = 0
    for p in range(len(ref_pos)):
        ops = cigars[p]
        counted = (int(ref_pos[p]) >= 0 and int(nm[p]) >= 0 and ops is not None and len(ops) > 0
                   and (mapq is None or int(mapq[p]) >= min_mapq))
        if not counted:
            skipped += 1
            continue
        used += 1
        row, rl, q = rows[p], int(read_len[p]), quals[p]
        qs = len(q) if qual_stride is None else int(qual_stride)
        rev = strand is not None and int(strand[p]) != 0
        i, g = 0, int(ref_pos[p])
        for word in ops:
            ln, kind = int(word) >> 4, int(word) & 15
            if kind == po.OP_S:
                i += ln
            elif kind == po.OP_M:
                for k in range(ln):
                    if 0 <= g + k < glen and i + k < rl:
                        t = rl - 1 - (i + k) if rev else i + k
                        if t < qs and phred(q[t]) >= min_baseq:
                            c = po.code(row[i + k])
                            counts[g + k, c] = (int(counts[g + k, c]) + 1) % MOD
                            if rev:
                                counts[g + k, po.CH_REV] = (int(counts[g + k, po.CH_REV]) + 1) % MOD
                            if c < QCHANNELS:
                                qsums[g + k, c] = (int(qsums[g + k, c]) + phred(q[t])) % MOD
                        else:
                            lowq += 1
                i += ln
                g += ln
            elif kind == po.OP_I:
                if 0 <= g - 1 < glen:
                    counts[g - 1, po.CH_INS] = (int(counts[g - 1, po.CH_INS]) + 1) % MOD
                i += ln
            elif kind == po.OP_D:
                for k in range(ln):
                    if 0 <= g + k < glen:
                        counts[g + k, po.CH_DEL] = (int(counts[g + k, po.CH_DEL]) + 1) % MOD
                g += ln
    return used, skipped, lowq


def pileup(genome, rows, read_len, ref_pos, nm, cigars, quals, strand=None, mapq=None, min_mapq=0, qual_stride=None,
           min_baseq=0):
    """-> (counts, qsums, reads_used, reads_skipped, lowq_columns) of one batch over `genome`."""
    counts, qsums = po.new_counts(len(genome)), new_qsums(len(genome))
    used, skipped, lowq = add(counts, qsums, rows, read_len, ref_pos, nm, cigars, quals, strand, mapq, min_mapq,
                              qual_stride, min_baseq)
    return counts, qsums, used, skipped, lowq
