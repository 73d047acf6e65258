"""Alignment records restated on the host (include/msw.h, "Alignment records").

TEST INFRASTRUCTURE ONLY.  From the canonical alignment of
tests/traceback_oracle.align plus the read, its window and the window's genome
position: the genome coordinate of the first aligned base, the CIGAR with soft
clips so that it consumes the whole read, and the edit distance (SAM's NM),
counted column by column.

    record(read, win, win_pos, match, mismatch, gap_open, gap_extend, affine)
        -> Record(score, end_i, end_j, ref_pos, nm, ops)
"""
from typing import NamedTuple

import traceback_oracle as tbo

S = 4  # BAM soft clip


class Record(NamedTuple):
    score: int
    end_i: int
    end_j: int
    ref_pos: int
    nm: int
    ops: list


def soft_clipped(ops, read_len, start_i, end_i):
    """S start_i, the traced ops, S (read_len - 1 - end_i); zero-length clips left out."""
    if not ops:
        return []
    out = [start_i << 4 | S] if start_i > 0 else []
    out += list(ops)
    if read_len - 1 - end_i > 0:
        out.append((read_len - 1 - end_i) << 4 | S)
    return out


def edit_distance(ops, read, win, start_i, start_j):
    """I lengths + D lengths + M columns whose bytes differ, walking from (start_i, start_j)."""
    r, w = tbo._bytes(read), tbo._bytes(win)
    i, j, nm = start_i, start_j, 0
    for o in ops:
        n, op = o >> 4, o & 15
        if op == tbo.M:
            for _ in range(n):
                nm += int(r[i] != w[j])
                i, j = i + 1, j + 1
        elif op == tbo.I:
            nm += n
            i += n
        else:
            nm += n
            j += n
    return nm


def from_alignment(read, win, win_pos, aligned):
    """aligned = traceback_oracle.align's tuple for (read, win)."""
    score, (ei, ej), (si, sj), ops = aligned
    if score == 0:
        return Record(0, -1, -1, -1, 0, [])
    return Record(score, ei, ej, win_pos + sj, edit_distance(ops, read, win, si, sj),
                  soft_clipped(ops, len(tbo._bytes(read)), si, ei))


def record(read, win, win_pos, match=2, mismatch=-1, gap_open=0, gap_extend=2, affine=False):
    return from_alignment(read, win, win_pos, tbo.align(read, win, match, mismatch, gap_open, gap_extend, affine))


def window_of(genome, pos, want):
    """The window rule: genome[pos, pos + want) clipped at the genome end; a
    position outside [0, len) is an empty window."""
    g = tbo._bytes(genome)
    if pos < 0 or pos >= len(g):
        return g[:0]
    return g[pos:pos + want]


def cigar_text(ops):
    return "".join(f"{o >> 4}{'MID?S'[o & 15]}" for o in ops) if len(ops) else "*"


def read_bases(ops):
    """Read bases an op list consumes (M, I and S)."""
    return sum(o >> 4 for o in ops if (o & 15) in (tbo.M, tbo.I, S))
