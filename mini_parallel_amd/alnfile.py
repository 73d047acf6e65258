"""The ``.aln`` files of ``rustseq_mini --full-wgs --alignments-out``.

Little-endian, a sequence of self-contained blocks in whatever order the
batches of a lane file settled:

  header, 32 B   u32 magic "MSWA", u32 version = 1, u64 first_read (index in
                 the lane file), u32 n_reads, u32 n_ops, u32 flags, 4 B zero
  n_reads x 24 B i64 ref_pos, i32 score, i32 nm, u32 n_ops, i16 end_i, i16 end_j
  n_ops x u32    packed ops in read order (len << 4 | op, M=0 I=1 D=2 S=4)
  flags bit 0:   n_reads x u8 strand (0 / 1), zero-padded to a multiple of 4 B
  flags bit 1:   n_reads x u8 mapq (0 .. 60), zero-padded to a multiple of 4 B,
                 then n_reads x i32 sub_score (after the strand bytes, if any)

Flag bit 0 (``--both-strands``): the block carries one strand byte per read; a
strand-1 record's end_i and CIGAR are in the coordinates of the read's reverse
complement (include/msw.h, "Both strands").  A block without the flag is byte
for byte what it was before the flag existed (the field was 8 zero bytes), and
a file may hold both kinds.

Flag bit 1 (``--mapq``): the block carries a mapping quality and the score of
the read's other candidate locus per read (include/msw.h, "Candidates and
mapping quality").  Reads from blocks without it have mapq 255 (SAM's
"unavailable") and sub_score 0.  A block without bit 1 is byte for byte what
it was before the bit existed.  Every other flag bit is refused.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence

import numpy as np

from .aligner import VAR_DEL, VAR_INS, VAR_SNV, VARIANT_DTYPE, CallParams, CigarList, QualParams, Variants

MAGIC = b"MSWA"
VERSION = 1
FLAG_STRAND = 1
FLAG_MAPQ = 2
MAPQ_MAX = 60
MAPQ_UNAVAILABLE = 255
HEADER = np.dtype([("magic", "S4"), ("version", "<u4"), ("first_read", "<u8"), ("n_reads", "<u4"),
                   ("n_ops", "<u4"), ("flags", "<u4"), ("zero", "<u4")])
RECORD = np.dtype([("ref_pos", "<i8"), ("score", "<i4"), ("nm", "<i4"), ("n_ops", "<u4"), ("end_i", "<i2"),
                   ("end_j", "<i2")])
assert HEADER.itemsize == 32 and RECORD.itemsize == 24


class Alignments(NamedTuple):
    """Per-read arrays in read order; ``cigars[p]`` is a uint32 array;
    ``strand`` is 0 for reads from blocks without strand bytes; ``mapq`` is
    255 and ``sub_score`` 0 for reads from blocks without flag bit 1."""
    ref_pos: np.ndarray
    score: np.ndarray
    nm: np.ndarray
    end_i: np.ndarray
    end_j: np.ndarray
    cigars: CigarList
    mapq: np.ndarray
    sub_score: np.ndarray
    strand: np.ndarray          # stays the last field


class AlnBlock(NamedTuple):
    """One block to write: reads first_read .. first_read + len(score).  With
    ``strand`` (0 / 1 per read) the block is written with flag bit 0; with
    ``mapq`` (0 .. 60) and ``sub_score``, which go together, with flag bit 1."""
    first_read: int
    ref_pos: Sequence
    score: Sequence
    nm: Sequence
    end_i: Sequence
    end_j: Sequence
    cigars: Sequence
    strand: Optional[Sequence] = None
    mapq: Optional[Sequence] = None
    sub_score: Optional[Sequence] = None


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
            tail = b""
            if b.strand is not None:
                strand = np.asarray(b.strand, np.int64).reshape(-1)
                if strand.size != n:
                    raise ValueError("block arrays disagree on the number of reads")
                if ((strand != 0) & (strand != 1)).any():
                    raise ValueError("a strand byte is neither 0 nor 1")
                head["flags"] = FLAG_STRAND
                tail = strand.astype(np.uint8).tobytes() + bytes(-n % 4)
            if (b.mapq is None) != (b.sub_score is None):
                raise ValueError("mapq and sub_score go together")
            if b.mapq is not None:
                mapq = np.asarray(b.mapq, np.int64).reshape(-1)
                sub = np.asarray(b.sub_score, np.int64).reshape(-1)
                if mapq.size != n or sub.size != n:
                    raise ValueError("block arrays disagree on the number of reads")
                if ((mapq < 0) | (mapq > MAPQ_MAX)).any():
                    raise ValueError(f"a mapq is outside [0, {MAPQ_MAX}]")
                head["flags"] |= FLAG_MAPQ
                tail += mapq.astype(np.uint8).tobytes() + bytes(-n % 4) + sub.astype("<i4").tobytes()
            f.write(head.tobytes() + rec.tobytes() + ops.tobytes() + tail)


def read_alignments(path) -> Alignments:
    """Read an ``.aln`` file back into read order.  Raises ValueError on a bad
    magic or version, an undefined flag bit or non-zero reserved bytes, a
    truncated block (inside its strand or mapq bytes included), a strand byte
    other than 0 / 1, a mapq above 60, non-zero padding, op counts that do not
    add up, or blocks that do not tile [0, N) exactly (a gap or an overlap)."""
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
        flags = int(head["flags"])
        if flags & ~(FLAG_STRAND | FLAG_MAPQ):
            raise ValueError(f"{path}: undefined flag bits {flags & ~(FLAG_STRAND | FLAG_MAPQ):#x} at byte {at}")
        if int(head["zero"]) != 0:
            raise ValueError(f"{path}: reserved header bytes are not zero at byte {at}")
        n, n_ops = int(head["n_reads"]), int(head["n_ops"])
        strand_bytes = (n + 3) // 4 * 4 if flags & FLAG_STRAND else 0
        mapq_bytes = (n + 3) // 4 * 4 + 4 * n if flags & FLAG_MAPQ else 0
        size = HEADER.itemsize + n * RECORD.itemsize + n_ops * 4 + strand_bytes + mapq_bytes
        if len(data) - at < size:
            raise ValueError(f"{path}: truncated block at byte {at} ({len(data) - at} of the {size} bytes "
                             f"its counts and flags {flags:#x} ask for)")
        rec = np.frombuffer(data, RECORD, n, at + HEADER.itemsize)
        ops = np.frombuffer(data, "<u4", n_ops, at + HEADER.itemsize + n * RECORD.itemsize)
        if int(rec["n_ops"].sum(dtype=np.uint64)) != n_ops:
            raise ValueError(f"{path}: the records of the block at byte {at} hold "
                             f"{int(rec['n_ops'].sum(dtype=np.uint64))} ops, its header says {n_ops}")
        strand = np.zeros(n, np.uint8)
        if flags & FLAG_STRAND:
            raw = np.frombuffer(data, np.uint8, strand_bytes, at + size - mapq_bytes - strand_bytes)
            if (raw[:n] > 1).any():
                raise ValueError(f"{path}: a strand byte of the block at byte {at} is neither 0 nor 1")
            if raw[n:].any():
                raise ValueError(f"{path}: the strand padding of the block at byte {at} is not zero")
            strand = raw[:n].copy()
        mapq, sub = np.full(n, MAPQ_UNAVAILABLE, np.uint8), np.zeros(n, np.int32)
        if flags & FLAG_MAPQ:
            raw = np.frombuffer(data, np.uint8, mapq_bytes - 4 * n, at + size - mapq_bytes)
            if (raw[:n] > MAPQ_MAX).any():
                raise ValueError(f"{path}: a mapq of the block at byte {at} is above {MAPQ_MAX}")
            if raw[n:].any():
                raise ValueError(f"{path}: the mapq padding of the block at byte {at} is not zero")
            mapq = raw[:n].copy()
            sub = np.frombuffer(data, "<i4", n, at + size - 4 * n).astype(np.int32)
        blocks.append((int(head["first_read"]), rec, ops, strand, mapq, sub))
        at += size
    blocks.sort(key=lambda b: (b[0], len(b[1])))  # an empty block sits before the reads at its index
    nxt = 0
    for first, rec, *_ in blocks:
        if first > nxt:
            raise ValueError(f"{path}: gap: reads {nxt}..{first - 1} are in no block")
        if first < nxt:
            raise ValueError(f"{path}: overlap: read {first} is in two blocks")
        nxt = first + len(rec)
    rec = np.concatenate([b[1] for b in blocks]) if blocks else np.zeros(0, RECORD)
    strand = np.concatenate([b[3] for b in blocks]) if blocks else np.zeros(0, np.uint8)
    mapq = np.concatenate([b[4] for b in blocks]) if blocks else np.zeros(0, np.uint8)
    sub = np.concatenate([b[5] for b in blocks]) if blocks else np.zeros(0, np.int32)
    cigars = CigarList()
    for _, r, ops, *_ in blocks:
        off = np.concatenate([[0], np.cumsum(r["n_ops"], dtype=np.int64)])
        cigars.extend(ops[off[k]:off[k + 1]].astype(np.uint32) for k in range(len(r)))
    cigars.n_cigar = rec["n_ops"].astype(np.int32)
    return Alignments(rec["ref_pos"].astype(np.int64), rec["score"].astype(np.int32), rec["nm"].astype(np.int32),
                      rec["end_i"].astype(np.int16), rec["end_j"].astype(np.int16), cigars, mapq, sub, strand)


# The ``.mpu`` file of ``rustseq_mini --full-wgs --pileup-out``,
# little-endian: a 32-byte header -- "MSWPILE1", u32 version = 1, u32 channels =
# 8, u64 genome length, u64 reads_used -- then genome length x 8 u32 counts
# (include/msw.h, "Pileup").  Dense: 32 bytes per genome base.
PILEUP_MAGIC = b"MSWPILE1"
PILEUP_VERSION = 1
PILEUP_CHANNELS = 8
PILEUP_HEADER = np.dtype([("magic", "S8"), ("version", "<u4"), ("channels", "<u4"), ("glen", "<u8"),
                          ("reads_used", "<u8")])
assert PILEUP_HEADER.itemsize == 32


def write_pileup(path, counts, reads_used: int) -> None:
    """Write uint32 ``counts[glen][8]`` and the number of reads behind them."""
    counts = np.asarray(counts)
    if counts.ndim != 2 or counts.shape[1] != PILEUP_CHANNELS:
        raise ValueError(f"counts must be [glen][{PILEUP_CHANNELS}]")
    if counts.size and (counts.min() < 0 or counts.max() > 0xFFFFFFFF):
        raise ValueError("a count does not fit 32 bits")
    head = np.zeros(1, PILEUP_HEADER)
    head["magic"], head["version"], head["channels"] = PILEUP_MAGIC, PILEUP_VERSION, PILEUP_CHANNELS
    head["glen"], head["reads_used"] = counts.shape[0], int(reads_used)
    with open(path, "wb") as f:
        f.write(head.tobytes())
        f.write(np.ascontiguousarray(counts, dtype="<u4").tobytes())


def read_pileup(path):
    """-> (counts uint32[glen][8], reads_used).  Raises ValueError on a bad
    magic, version or channel count, and on a size that does not match the
    header's genome length (truncated, or bytes after the counts)."""
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < PILEUP_HEADER.itemsize:
        raise ValueError(f"{path}: truncated header")
    head = np.frombuffer(data, PILEUP_HEADER, 1)[0]
    if bytes(head["magic"]) != PILEUP_MAGIC:
        raise ValueError(f"{path}: bad magic")
    if int(head["version"]) != PILEUP_VERSION:
        raise ValueError(f"{path}: version {int(head['version'])}, expected {PILEUP_VERSION}")
    if int(head["channels"]) != PILEUP_CHANNELS:
        raise ValueError(f"{path}: {int(head['channels'])} channels, expected {PILEUP_CHANNELS}")
    glen = int(head["glen"])
    want = PILEUP_HEADER.itemsize + glen * PILEUP_CHANNELS * 4
    if len(data) != want:
        raise ValueError(f"{path}: {len(data)} bytes, the header's genome length {glen} asks for {want}")
    counts = np.frombuffer(data, "<u4", glen * PILEUP_CHANNELS, PILEUP_HEADER.itemsize)
    return counts.reshape(glen, PILEUP_CHANNELS).astype(np.uint32), int(head["reads_used"])


# The ``.mqs`` file of ``rustseq_mini --full-wgs --call-baseq --qsum-out``
# (DESIGN.md 4.17), little-endian: a 32-byte header -- "MSWQSUM1", u32 version =
# 1, u32 channels = 4, u64 genome length, u64 reads_used -- then genome length x
# 4 u32 quality sums (include/msw.h, "Quality sums and weighted genotypes").
QSUM_MAGIC = b"MSWQSUM1"
QSUM_VERSION = 1
QSUM_CHANNELS = 4


def write_qsums(path, qsums, reads_used: int) -> None:
    """Write uint32 ``qsums[glen][4]`` and the number of reads behind them."""
    qsums = np.asarray(qsums)
    if qsums.ndim != 2 or qsums.shape[1] != QSUM_CHANNELS:
        raise ValueError(f"qsums must be [glen][{QSUM_CHANNELS}]")
    if qsums.size and (qsums.min() < 0 or qsums.max() > 0xFFFFFFFF):
        raise ValueError("a sum does not fit 32 bits")
    head = np.zeros(1, PILEUP_HEADER)
    head["magic"], head["version"], head["channels"] = QSUM_MAGIC, QSUM_VERSION, QSUM_CHANNELS
    head["glen"], head["reads_used"] = qsums.shape[0], int(reads_used)
    with open(path, "wb") as f:
        f.write(head.tobytes())
        f.write(np.ascontiguousarray(qsums, dtype="<u4").tobytes())


def read_qsums(path):
    """-> (qsums uint32[glen][4], reads_used).  Raises ValueError on a bad
    magic, version or channel count, and on a size that does not match the
    header's genome length (truncated, or bytes after the sums)."""
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < PILEUP_HEADER.itemsize:
        raise ValueError(f"{path}: truncated header")
    head = np.frombuffer(data, PILEUP_HEADER, 1)[0]
    if bytes(head["magic"]) != QSUM_MAGIC:
        raise ValueError(f"{path}: bad magic")
    if int(head["version"]) != QSUM_VERSION:
        raise ValueError(f"{path}: version {int(head['version'])}, expected {QSUM_VERSION}")
    if int(head["channels"]) != QSUM_CHANNELS:
        raise ValueError(f"{path}: {int(head['channels'])} channels, expected {QSUM_CHANNELS}")
    glen = int(head["glen"])
    want = PILEUP_HEADER.itemsize + glen * QSUM_CHANNELS * 4
    if len(data) != want:
        raise ValueError(f"{path}: {len(data)} bytes, the header's genome length {glen} asks for {want}")
    qsums = np.frombuffer(data, "<u4", glen * QSUM_CHANNELS, PILEUP_HEADER.itemsize)
    return qsums.reshape(glen, QSUM_CHANNELS).astype(np.uint32), int(head["reads_used"])


# The ``.var`` file of ``rustseq_mini --full-wgs --variants-out``,
# little-endian: a 72-byte header -- "MSWVARS1", u32 version = 1, u32 record size
# = 48, u64 genome length, u64 record count, the nine u32 of msw_call_params_t in
# their order, u32 zero -- then the records (msw_variant_t of include/msw.h,
# "Variants"), ordered by pos, then kind.
VARIANTS_MAGIC = b"MSWVARS1"
VARIANTS_VERSION = 1
VARIANTS_HEADER = np.dtype([("magic", "S8"), ("version", "<u4"), ("record_size", "<u4"), ("glen", "<u8"),
                            ("count", "<u8"), ("params", "<u4", (9,)), ("reserved", "<u4")])
assert VARIANTS_HEADER.itemsize == 72
# The quality-weighted ``.var`` (``--call-baseq``): magic
# "MSWVARQ1" and an 88-byte header -- the 72 bytes above, then q_scale, q_third
# (msw_call_qparams_t) and two zero words; the records are the same.
VARIANTS_QUAL_MAGIC = b"MSWVARQ1"
VARIANTS_QUAL_HEADER = np.dtype(VARIANTS_HEADER.descr + [("qparams", "<u4", (2,)), ("reserved2", "<u4", (2,))])
assert VARIANTS_QUAL_HEADER.itemsize == 88


def _check_variant_records(path, rec, glen) -> None:
    if not len(rec):
        return
    if int(rec["kind"].max()) > VAR_INS:
        raise ValueError(f"{path}: a record of unknown kind")
    if not np.isin(rec["gt"], (1, 2)).all():
        raise ValueError(f"{path}: a record with a genotype other than 0/1 and 1/1")
    if rec["pad"].any():
        raise ValueError(f"{path}: a record's padding is not zero")
    if int(rec["pos"].max()) >= glen:
        raise ValueError(f"{path}: a record lies past the genome length {glen}")
    pos, col = rec["pos"], rec["kind"] != VAR_INS
    # at most one column record and one insertion per position, the column record first
    later = (pos[1:] > pos[:-1]) | ((pos[1:] == pos[:-1]) & col[:-1] & ~col[1:])
    if not later.all():
        raise ValueError(f"{path}: the records are not ordered by pos, then kind")


def write_variants(path, variants: Variants, glen: int, params: Optional[CallParams] = None,
                   qual_params: Optional[QualParams] = None) -> None:
    """Write the records of a genome of ``glen`` bases and the parameters they
    were called with (the defaults when None).  With ``qual_params`` (records
    of a quality-weighted call) the file is an ``MSWVARQ1`` one, which
    :func:`read_variants_qual` reads."""
    params = params or CallParams()
    rec = variants.to_records()
    _check_variant_records(str(path), rec, int(glen))
    head = np.zeros(1, VARIANTS_HEADER if qual_params is None else VARIANTS_QUAL_HEADER)
    head["magic"], head["version"], head["record_size"] = VARIANTS_MAGIC, VARIANTS_VERSION, VARIANT_DTYPE.itemsize
    head["glen"], head["count"] = int(glen), len(rec)
    head["params"] = [int(getattr(params, k)) for k in CallParams.FIELDS]
    if qual_params is not None:
        head["magic"] = VARIANTS_QUAL_MAGIC
        head["qparams"] = [int(getattr(qual_params, k)) for k in QualParams.FIELDS]
    with open(path, "wb") as f:
        f.write(head.tobytes())
        f.write(rec.tobytes())


def read_variants(path):
    """-> (Variants, genome length, CallParams).  Raises ValueError on a bad
    magic, version or record size, on a size that does not match the header's
    record count, and on records that are out of order, past the genome, of an
    unknown kind or genotype or with non-zero padding."""
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < VARIANTS_HEADER.itemsize:
        raise ValueError(f"{path}: truncated header")
    head = np.frombuffer(data, VARIANTS_HEADER, 1)[0]
    if bytes(head["magic"]) != VARIANTS_MAGIC:
        raise ValueError(f"{path}: bad magic")
    if int(head["version"]) != VARIANTS_VERSION:
        raise ValueError(f"{path}: version {int(head['version'])}, expected {VARIANTS_VERSION}")
    if int(head["record_size"]) != VARIANT_DTYPE.itemsize:
        raise ValueError(f"{path}: record size {int(head['record_size'])}, expected {VARIANT_DTYPE.itemsize}")
    if int(head["reserved"]) != 0:
        raise ValueError(f"{path}: the header's reserved word is not zero")
    glen, count = int(head["glen"]), int(head["count"])
    want = VARIANTS_HEADER.itemsize + count * VARIANT_DTYPE.itemsize
    if len(data) != want:
        raise ValueError(f"{path}: {len(data)} bytes, the header's record count {count} asks for {want}")
    rec = np.frombuffer(data, VARIANT_DTYPE, count, VARIANTS_HEADER.itemsize)
    _check_variant_records(str(path), rec, glen)
    return Variants.from_records(rec), glen, CallParams(*(int(v) for v in head["params"]))


def read_variants_qual(path):
    """-> (Variants, genome length, CallParams, QualParams) of an ``MSWVARQ1``
    file.  Raises ValueError as :func:`read_variants` does, and on a non-zero
    word behind the weights."""
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < VARIANTS_QUAL_HEADER.itemsize:
        raise ValueError(f"{path}: truncated header")
    head = np.frombuffer(data, VARIANTS_QUAL_HEADER, 1)[0]
    if bytes(head["magic"]) != VARIANTS_QUAL_MAGIC:
        raise ValueError(f"{path}: bad magic")
    if int(head["version"]) != VARIANTS_VERSION:
        raise ValueError(f"{path}: version {int(head['version'])}, expected {VARIANTS_VERSION}")
    if int(head["record_size"]) != VARIANT_DTYPE.itemsize:
        raise ValueError(f"{path}: record size {int(head['record_size'])}, expected {VARIANT_DTYPE.itemsize}")
    if int(head["reserved"]) != 0 or head["reserved2"].any():
        raise ValueError(f"{path}: a reserved word of the header is not zero")
    glen, count = int(head["glen"]), int(head["count"])
    want = VARIANTS_QUAL_HEADER.itemsize + count * VARIANT_DTYPE.itemsize
    if len(data) != want:
        raise ValueError(f"{path}: {len(data)} bytes, the header's record count {count} asks for {want}")
    rec = np.frombuffer(data, VARIANT_DTYPE, count, VARIANTS_QUAL_HEADER.itemsize)
    _check_variant_records(str(path), rec, glen)
    return (Variants.from_records(rec), glen, CallParams(*(int(v) for v in head["params"])),
            QualParams(*(int(v) for v in head["qparams"])))


def write_vcf(path, variants: Variants, genome, contig: str = "ref", sample: str = "sample") -> None:
    """VCF 4.2 text of the records over ``genome`` (bytes or a uint8 array).
    An SNV is written as it is.  Consecutive DEL records (pos, pos + 1, ...
    with equal genotype) become one deletion with the first record's numbers,
    anchored at the base before the run, or at the base after it when the run
    starts at position 0.  An insertion is the symbolic ``<INS>`` at its anchor
    base: the pileup does not hold the inserted sequence."""
    g = bytes(genome) if isinstance(genome, (bytes, bytearray)) else np.asarray(genome, np.uint8).tobytes()
    rec = variants.to_records()

    def seq(lo, hi):
        return "".join(chr(b) if chr(b).isalpha() else "N" for b in g[lo:hi])

    lines = []  # (POS, order, text)

    def line(vpos, ref, alt, r):
        gt = "0/1" if int(r["gt"]) == 1 else "1/1"
        lines.append((vpos, len(lines), "%s\t%d\t.\t%s\t%s\t%d\t.\tDP=%d\tGT:AD:GQ:PL\t%s:%d,%d:%d:%d,%d,%d" % (
            contig, vpos, ref, alt, int(r["qual"]), int(r["depth"]), gt, int(r["ref_count"]), int(r["alt_count"]),
            int(r["gq"]), int(r["pl"][0]), int(r["pl"][1]), int(r["pl"][2]))))

    def insertion(r):
        line(int(r["pos"]) + 1, seq(int(r["pos"]), int(r["pos"]) + 1), "<INS>", r)

    k = 0
    while k < len(rec):
        r = rec[k]
        pos, kind = int(r["pos"]), int(r["kind"])
        if kind == VAR_SNV:
            line(pos + 1, seq(pos, pos + 1), chr(int(r["alt"])), r)
        elif kind == VAR_INS:
            insertion(r)
        else:
            # the run's further DEL records; an insertion record between two of them does not end the run
            end, j = pos + 1, k + 1
            while j < len(rec):
                if int(rec[j]["kind"]) == VAR_DEL and int(rec[j]["pos"]) == end and rec[j]["gt"] == r["gt"]:
                    end += 1
                elif not (int(rec[j]["kind"]) == VAR_INS and int(rec[j]["pos"]) == end - 1):
                    break
                j += 1
            if pos > 0:
                line(pos, seq(pos - 1, end), seq(pos - 1, pos), r)
            elif end < len(g):
                line(1, seq(0, end + 1), seq(end, end + 1), r)
            else:
                line(1, seq(0, end), "<DEL>", r)  # the whole genome: no base to anchor at
            for m in range(k + 1, j):
                if int(rec[m]["kind"]) == VAR_INS:
                    insertion(rec[m])
            k = j - 1
        k += 1
    lines.sort(key=lambda t: (t[0], t[1]))
    with open(path, "w") as f:
        f.write("##fileformat=VCFv4.2\n")
        f.write("##contig=<ID=%s,length=%d>\n" % (contig, len(g)))
        f.write('##ALT=<ID=INS,Description="Insertion after this base; the sequence is not known">\n')
        f.write('##ALT=<ID=DEL,Description="Deletion">\n')
        f.write('##INFO=<ID=DP,Number=1,Type=Integer,Description="Observations at the site">\n')
        f.write('##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">\n')
        f.write('##FORMAT=<ID=AD,Number=R,Type=Integer,Description="Observations of the reference and the alternative">\n')
        f.write('##FORMAT=<ID=GQ,Number=1,Type=Integer,Description="Genotype quality">\n')
        f.write('##FORMAT=<ID=PL,Number=G,Type=Integer,Description="Genotype costs, -10 log10 of the likelihood">\n')
        f.write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t%s\n" % sample)
        for _, _, text in lines:
            f.write(text + "\n")
