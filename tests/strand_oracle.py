"""Both strands restated on the host (include/msw.h, "Both strands").

TEST INFRASTRUCTURE ONLY.  The reverse complement by a 256-entry table, the
choice between the two orientations by the contract (strand 1 exactly when the
reverse complement scores strictly higher), and the record of the oriented
read.  Scores and end cells come from the C oracle (oracle/oracle_lib), as in
the other tests; the alignment of the winning orientation comes from
tests/aln_oracle.record and must agree with it.

    revcomp(seq) -> bytes
    score_batch(reads, wins, scheme) -> (score, end_i, end_j, strand) arrays
    record(read, win, win_pos, scheme) -> Record(score, end_i, end_j, strand, ref_pos, nm, ops)
    oriented(read, strand) -> bytes
"""
from typing import NamedTuple

import numpy as np

import aln_oracle as ao

PAIRS = ((ord("A"), ord("T")), (ord("C"), ord("G")), (ord("a"), ord("t")), (ord("c"), ord("g")))
TABLE = list(range(256))
for _a, _b in PAIRS:
    TABLE[_a], TABLE[_b] = _b, _a
TABLE = bytes(TABLE)


class Record(NamedTuple):
    score: int
    end_i: int
    end_j: int
    strand: int
    ref_pos: int
    nm: int
    ops: list


def _b(x):
    if isinstance(x, str):
        return x.encode("latin-1")
    return bytes(x) if isinstance(x, (bytes, bytearray)) else np.asarray(x, np.uint8).tobytes()


def revcomp(seq) -> bytes:
    return _b(seq)[::-1].translate(TABLE)


def oriented(read, strand) -> bytes:
    return revcomp(read) if strand else _b(read)


def _pack(seqs):
    ln = np.array([len(s) for s in seqs], np.uint16)
    a = np.zeros((len(seqs), max(1, int(ln.max()) if len(seqs) else 1)), np.uint8)
    for k, s in enumerate(seqs):
        a[k, :len(s)] = np.frombuffer(s, np.uint8)
    return a, ln


def score_batch(reads, wins, scheme, threads=4):
    """Both orientations of every read through the C oracle; the winner's
    score and end cell and the strand, by the contract."""
    from oracle import oracle_lib
    m, x, go, ge, aff = scheme
    fwd = [_b(r) for r in reads]
    W, wl = _pack([_b(w) for w in wins])
    res = []
    for rows in (fwd, [revcomp(r) for r in fwd]):
        R, rl = _pack(rows)
        res.append(oracle_lib.sw_batch(R, rl, W, wl, match=m, mismatch=x, gap_open=go, gap_extend=ge, affine=aff,
                                       threads=threads))
    (sf, if_, jf), (sr, ir, jr) = res
    strand = (sr > sf).astype(np.uint8)      # ties: forward
    pick = lambda f, r: np.where(strand == 1, r, f)
    return pick(sf, sr).astype(np.int32), pick(if_, ir).astype(np.int16), pick(jf, jr).astype(np.int16), strand


def record(read, win, win_pos, scheme):
    """aln_oracle.record on both orientations, chosen by the contract; the
    C oracle's winner must be the same cell with the same score."""
    read, win = _b(read), _b(win)
    f = ao.record(read, win, win_pos, *scheme)
    r = ao.record(revcomp(read), win, win_pos, *scheme)
    strand = 1 if r.score > f.score else 0
    w = r if strand else f
    s, ei, ej, st = score_batch([read], [win], scheme, threads=1)
    assert (int(s[0]), int(ei[0]), int(ej[0]), int(st[0])) == (w.score, w.end_i, w.end_j, strand), \
        "the two oracles disagree"
    return Record(w.score, w.end_i, w.end_j, strand, w.ref_pos, w.nm, w.ops)


def records(reads, wins, win_pos, scheme):
    """record() for a batch: the C oracle picks the strands in one call, and
    only the winning orientation is traced in Python."""
    s, ei, ej, st = score_batch(reads, wins, scheme)
    out = []
    for k, (read, win) in enumerate(zip(reads, wins)):
        w = ao.record(oriented(read, int(st[k])), _b(win), int(win_pos[k]), *scheme)
        assert (w.score, w.end_i, w.end_j) == (int(s[k]), int(ei[k]), int(ej[k])), "the two oracles disagree"
        out.append(Record(w.score, w.end_i, w.end_j, int(st[k]), w.ref_pos, w.nm, w.ops))
    return out
