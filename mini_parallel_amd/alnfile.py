"""The ``.aln`` files of ``rustseq_mini --full-wgs --alignments-out``.

Little-endian, a sequence of self-contained blocks in whatever order the
batches of a lane file settled:

  header, 32 B   u32 magic "MSWA", u32 version = 1, u64 first_read (index in
                 the lane file), u32 n_reads, u32 n_ops, 8 B zero
  n_reads x 24 B i64 ref_pos, i32 score, i32 nm, u32 n_ops, i16 end_i, i16 end_j
  n_ops x u32    packed ops in read order (len << 4 | op, M=0 I=1 D=2 S=4)
"""
from __future__ import annotations

from typing import NamedTuple, Sequence

import numpy as np

from .aligner import CigarList

MAGIC = b"MSWA"
VERSION = 1
HEADER = np.dtype([("magic", "S4"), ("version", "<u4"), ("first_read", "<u8"), ("n_reads", "<u4"),
                   ("n_ops", "<u4"), ("zero", "<u8")])
RECORD = np.dtype([("ref_pos", "<i8"), ("score", "<i4"), ("nm", "<i4"), ("n_ops", "<u4"), ("end_i", "<i2"),
                   ("end_j", "<i2")])
assert HEADER.itemsize == 32 and RECORD.itemsize == 24


class Alignments(NamedTuple):
    """Per-read arrays in read order; ``cigars[p]`` is a uint32 array."""
    ref_pos: np.ndarray
    score: np.ndarray
    nm: np.ndarray
    end_i: np.ndarray
    end_j: np.ndarray
    cigars: CigarList


class AlnBlock(NamedTuple):
    """One block to write: reads first_read .. first_read + len(score)."""
    first_read: int
    ref_pos: Sequence
    score: Sequence
    nm: Sequence
    end_i: Sequence
    end_j: Sequence
    cigars: Sequence


def write_alignments(path, blocks: Sequence[AlnBlock]) -> None:
    """Write `blocks` in the order given (the inverse of read_alignments)."""
    with open(path, "wb") as f:
        for b in blocks:
            b = AlnBlock(*b)
            n = len(b.score)
            if not (len(b.ref_pos) == len(b.nm) == len(b.end_i) == len(b.end_j) == len(b.cigars) == n):
                raise ValueError("block arrays disagree on the number of reads")
            rec = np.zeros(n, RECORD)
            rec["ref_pos"], rec["score"], rec["nm"] = b.ref_pos, b.score, b.nm
            rec["end_i"], rec["end_j"] = b.end_i, b.end_j
            rec["n_ops"] = [len(c) for c in b.cigars]
            ops = (np.concatenate([np.asarray(c, "<u4") for c in b.cigars]) if n else np.zeros(0, "<u4")).astype("<u4")
            head = np.zeros(1, HEADER)
            head["magic"], head["version"], head["first_read"] = MAGIC, VERSION, int(b.first_read)
            head["n_reads"], head["n_ops"] = n, ops.size
            f.write(head.tobytes() + rec.tobytes() + ops.tobytes())


def read_alignments(path) -> Alignments:
    """Read an ``.aln`` file back into read order.  Raises ValueError on a bad
    magic or version, a truncated block, op counts that do not add up, or
    blocks that do not tile [0, N) exactly (a gap or an overlap)."""
    with open(path, "rb") as f:
        data = f.read()
    blocks = []
    at = 0
    while at < len(data):
        if len(data) - at < HEADER.itemsize:
            raise ValueError(f"{path}: truncated block header at byte {at}")
        head = np.frombuffer(data, HEADER, 1, at)[0]
        if bytes(head["magic"]) != MAGIC:
            raise ValueError(f"{path}: bad magic at byte {at}")
        if int(head["version"]) != VERSION:
            raise ValueError(f"{path}: version {int(head['version'])}, expected {VERSION}")
        if int(head["zero"]) != 0:
            raise ValueError(f"{path}: reserved header bytes are not zero at byte {at}")
        n, n_ops = int(head["n_reads"]), int(head["n_ops"])
        size = HEADER.itemsize + n * RECORD.itemsize + n_ops * 4
        if len(data) - at < size:
            raise ValueError(f"{path}: truncated block at byte {at} ({len(data) - at} of {size} bytes)")
        rec = np.frombuffer(data, RECORD, n, at + HEADER.itemsize)
        ops = np.frombuffer(data, "<u4", n_ops, at + HEADER.itemsize + n * RECORD.itemsize)
        if int(rec["n_ops"].sum(dtype=np.uint64)) != n_ops:
            raise ValueError(f"{path}: the records of the block at byte {at} hold "
                             f"{int(rec['n_ops'].sum(dtype=np.uint64))} ops, its header says {n_ops}")
        blocks.append((int(head["first_read"]), rec, ops))
        at += size
    blocks.sort(key=lambda b: (b[0], len(b[1])))  # an empty block sits before the reads at its index
    nxt = 0
    for first, rec, _ in blocks:
        if first > nxt:
            raise ValueError(f"{path}: gap: reads {nxt}..{first - 1} are in no block")
        if first < nxt:
            raise ValueError(f"{path}: overlap: read {first} is in two blocks")
        nxt = first + len(rec)
    rec = np.concatenate([b[1] for b in blocks]) if blocks else np.zeros(0, RECORD)
    cigars = CigarList()
    for _, r, ops in blocks:
        off = np.concatenate([[0], np.cumsum(r["n_ops"], dtype=np.int64)])
        cigars.extend(ops[off[k]:off[k + 1]].astype(np.uint32) for k in range(len(r)))
    cigars.n_cigar = rec["n_ops"].astype(np.int32)
    return Alignments(rec["ref_pos"].astype(np.int64), rec["score"].astype(np.int32), rec["nm"].astype(np.int32),
                      rec["end_i"].astype(np.int16), rec["end_j"].astype(np.int16), cigars)
