"""The base-quality rules of include/msw.h ("Pileup", "Base qualities"),
restated column by column beside tests/pileup_oracle.py.

Plain Python: one increment per counted column and one per dropped column.
It shares nothing with the kernel's corrections to the difference form
(msw_pileup.hip), so the two can be compared value for value.
"""
import pileup_oracle as po


def phred(byte) -> int:
    """The Phred value of a FASTQ quality byte: b - 33, and 0 below 33."""
    b = int(byte)
    return b - 33 if b >= 33 else 0


def add(counts, rows, read_len, ref_pos, nm, cigars, strand=None, mapq=None, min_mapq=0, quals=None, qual_stride=None,
        min_baseq=0):
    """Adds the batch's records to counts[glen][8] in place; returns
    (reads_used, reads_skipped, lowq_columns).

    rows[p] are the bytes the CIGAR of read p refers to (the oriented read).
    quals[p] are the quality bytes of read p AS GIVEN, of which the first
    qual_stride (default: all of quals[p]) exist: for a strand-1 read, column
    i + k of the row has quality index read_len[p] - 1 - (i + k)."""
    if quals is None or min_baseq == 0:
        used, skipped = po.add(counts, rows, read_len, ref_pos, nm, cigars, strand, mapq, min_mapq)
        return used, skipped, 0
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
                            counts[g + k, po.code(row[i + k])] += 1
                            if rev:
                                counts[g + k, po.CH_REV] += 1
                        else:
                            lowq += 1
                i += ln
                g += ln
            elif kind == po.OP_I:
                if 0 <= g - 1 < glen:
                    counts[g - 1, po.CH_INS] += 1
                i += ln
            elif kind == po.OP_D:
                for k in range(ln):
                    if 0 <= g + k < glen:
                        counts[g + k, po.CH_DEL] += 1
                g += ln
    return used, skipped, lowq


def pileup(genome, rows, read_len, ref_pos, nm, cigars, strand=None, mapq=None, min_mapq=0, quals=None,
           qual_stride=None, min_baseq=0):
    """-> (counts, reads_used, reads_skipped, lowq_columns) of one batch over `genome`."""
    counts = po.new_counts(len(genome))
    used, skipped, lowq = add(counts, rows, read_len, ref_pos, nm, cigars, strand, mapq, min_mapq, quals, qual_stride,
                              min_baseq)
    return counts, used, skipped, lowq
