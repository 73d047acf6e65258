"""FASTQ record-parse reference and corpus (no GPU).

`reference_parse` restates process_fastq_file_in_chunks (aligner.rs:128-170)
in plain Python, plus the two things this project adds to it: the `pos=` tag
of a record's header and the slab stride.  It shares no code with the C++
reader, the GPU parse or tests/test_fastq.py::reference_chunks:

  lines      BufRead::lines: split at \\n, one \\r stripped only from a line
             that had a \\n; a final piece without \\n is a line if non-empty
  validity   bytes.decode("utf-8"), strict; a failure is an error: the line
             is skipped and not counted, the 11th error ends the file
  position   valid line number % 4 == 1: leftmost match of pos=(-?[0-9]+)
  reads      valid line number % 4 == 2; longer than the stride ends the file

The corpus places the bytes the parse branches on where it branches:
  P  pos= forms: every header length 1..75 and tag offset, 1..18 digits,
     decoys, tags past the header's end, multi-byte headers
  U  UTF-8: every boundary form valid and invalid in each of a record's four
     lines, truncated sequences, the error budget and its order against a
     too-long read
  E  line ends: \\r without \\n at end of file, \\r\\r\\n, lone \\r, empty lines,
     the stride and stride + 1 before \\r\\n
  C  span cuts: text of just over 2 MiB in 32 KiB BGZF members read with
     1 MiB spans, so spans end at byte 1 MiB and 2 MiB exactly, with a chosen
     byte pair on the two sides of each cut
Everything is deterministic (seeded), like deflate_writer.corpus().
"""
import functools
import re
import struct
from collections import Counter
from dataclasses import dataclass, field

import numpy as np

from mini_parallel_amd.synthetic import bgzf_compress

SPAN = 1 << 20       # the reader's smallest span (msw_gfastq_open clamps to it)
CUT_BLOCK = 32768    # BGZF member size of the cut files: 32 members per span
E_INVALID, E_RANGE = -1, -2
ERR_LIMIT_MSG = "Too many read errors (>10), stopping at line %d"

_POS = re.compile(rb"pos=(-?[0-9]+)")


# ---------------------------------------------------------------------------
# The reference
# ---------------------------------------------------------------------------
@dataclass
class Parsed:
    rows: np.ndarray      # u8[n, stride], zero padded
    lens: np.ndarray      # u16[n]
    pos: np.ndarray       # i64[n], None without with_pos
    ends: np.ndarray      # i64[n]: offset of each read's \n (len(data) for an unterminated final line)
    lines: int            # valid lines
    reads: int
    errors: int
    bases: int
    code: int = 0         # 0, E_INVALID (the error limit) or E_RANGE (a read longer than the stride)
    err_line: int = None  # valid lines so far (error limit) / the read's valid line number (too long)
    err_end: int = None   # offset of the end of the line that ended the file
    message: str = None   # the error limit's message


def reference_parse(data: bytes, stride: int, with_pos=True) -> Parsed:
    seqs, poss, ends = [], [], []
    valid = errors = 0
    pending = -1
    code, err_line, err_end, message = 0, None, None, None
    i, n = 0, len(data)
    while i < n:
        j = data.find(b"\n", i)
        if j < 0:  # the final piece: a line as it stands, \r and all
            line, end, i = data[i:], n, n
        else:
            line, end, i = data[i:j], j, j + 1
            if line.endswith(b"\r"):
                line = line[:-1]
        try:
            line.decode("utf-8")
        except UnicodeDecodeError:
            errors += 1
            if errors > 10:
                code, err_line, err_end, message = E_INVALID, valid, end, ERR_LIMIT_MSG % valid
                break
            continue
        valid += 1
        if valid % 4 == 1:
            m = _POS.search(line) if with_pos else None
            pending = int(m.group(1)) if m else -1
        elif valid % 4 == 2:
            if len(line) > stride:
                code, err_line, err_end = E_RANGE, valid, end
                break
            seqs.append(line)
            poss.append(pending)
            ends.append(end)
            pending = -1
    rows = np.frombuffer(b"".join(s.ljust(stride, b"\0") for s in seqs), np.uint8).reshape(len(seqs), stride)
    lens = np.array([len(s) for s in seqs], np.uint16)
    return Parsed(rows, lens, np.array(poss, np.int64) if with_pos else None, np.array(ends, np.int64), valid,
                  len(seqs), errors, int(lens.astype(np.int64).sum()), code, err_line, err_end, message)


# ---------------------------------------------------------------------------
# Spans: the longest runs of whole BGZF members whose ISIZEs sum to <= span
# ---------------------------------------------------------------------------
def member_isizes(blob: bytes):
    out, p = [], 0
    while p < len(blob):
        bsize = struct.unpack_from("<H", blob, p + 16)[0] + 1
        out.append(struct.unpack_from("<I", blob, p + bsize - 4)[0])
        p += bsize
    assert p == len(blob)
    return out


def span_cuts(isizes, span=SPAN):
    """Text offsets at which a span ends and another begins."""
    cuts, ob, total = [], 0, 0
    for s in isizes:
        assert s <= span
        if ob + s > span:
            cuts.append(total)
            ob = 0
        ob += s
        total += s
    return cuts


def span_of(cuts, offsets):
    """Span in which a line ending at each offset is complete."""
    return np.searchsorted(np.asarray(cuts, np.int64), np.asarray(offsets, np.int64), side="right")


def expected_batches(ref: Parsed, cuts, max_reads):
    """Sizes of the batches a reader with this max_reads delivers: batches
    never cross spans, a span without reads gives none, and the span in which
    the file fails (and every later one) gives none."""
    per = np.bincount(span_of(cuts, ref.ends), minlength=len(cuts) + 1)
    if ref.code:
        per = per[:int(span_of(cuts, [ref.err_end])[0])]
    out = []
    for c in per:
        out += [max_reads] * (int(c) // max_reads) + ([int(c) % max_reads] if int(c) % max_reads else [])
    return out


# ---------------------------------------------------------------------------
# Cases
# ---------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    family: str
    data: bytes
    stride: int = 256
    block: int = 20000     # BGZF member size
    marks: list = field(default_factory=list)  # C: (cut, bytes before it, bytes after it)
    info: dict = field(default_factory=dict)   # what the builder promises (checked by the CPU tests)

    @functools.cached_property
    def blob(self) -> bytes:
        return bgzf_compress(self.data, 1, block=self.block)

    @functools.cached_property
    def cuts(self):
        return span_cuts(member_isizes(self.blob))


def _seq(m, k=0):
    return (b"ACGTTGCAAGCTGATC" * (m // 16 + 2))[k % 16:k % 16 + m]


def _rec(h, s, nl=b"\n", q=None):
    return h + nl + s + nl + b"+" + nl + (b"I" * len(s) if q is None else q) + nl


# --- P: pos= forms ----------------------------------------------------------
_FILL = b"abcdefghijklmn"  # no digit, none of "pos=-"


def _hdr(L, off, tag):
    """A header of L bytes with tag at offset off (letters around it)."""
    lead = (b"@" + _FILL * 6)[:off]
    return lead + tag + (_FILL * 6)[:L - off - len(tag)]


def _digits(d, salt):
    return bytes([49 + (salt * 7 + d) % 9] + [48 + (salt * 31 + 7 * k * k + d) % 10 for k in range(1, d)])


def _p_items(multibyte):
    """(header, sequence or None, newline) per record."""
    tags = [b"pos=7", b"pos=-31", b"pos=123456", b"pos=-9876543210"]
    it = []
    for L in range(1, 76):  # both sides of the 60-byte fast-path limit, the tag at every offset
        it.append((_hdr(L, L, b""), None, b"\n"))
        for off in range(0, L - 4):
            tag = tags[(L + off) % 4]
            if off + len(tag) > L:
                tag = b"pos=7"
            it.append((_hdr(L, off, tag), None, b"\n"))
    for d in range(1, 19):  # the serial fallback starts at 16 digits
        for sign in (b"", b"-"):
            for tail in (b"", b" t"):  # b"": the number ends the header
                for lead in (b"@d ", b"@d " + _FILL * 4 + b" "):  # short, and over 60 bytes
                    it.append((lead + b"pos=" + sign + _digits(d, len(it)) + tail, None, b"\n"))
    for d in (1, 5, 15, 16, 17, 18):  # the number ends the header, before a \r
        it.append((b"@e pos=" + _digits(d, d), None, b"\r\n"))
        it.append((b"@e pos=-" + _digits(d, d + 1), None, b"\r\n"))
    for d in (15, 16, 17, 18):
        it.append((b"@n pos=" + b"9" * d, None, b"\n"))
        it.append((b"@n pos=-" + b"9" * d + b" t", None, b"\n"))
        it.append((b"@z pos=" + b"0" * (d - 2) + b"42", None, b"\n"))
    decoys = [b"pos=", b"pos=-", b"pos=-x", b"pos=x", b"xpos=12", b"pos==3", b"pos=+3"]
    for dc in decoys:
        it.append((b"@q " + dc, None, b"\n"))           # alone; "pos=" as the header's last four bytes
        it.append((b"@q " + dc, None, b"\r\n"))
        it.append((b"@q " + dc + b" z", None, b"\n"))
        it.append((b"@q " + dc + b" pos=5", None, b"\n"))  # before the real tag
        it.append((b"@q " + dc + b"pos=-8", None, b"\n"))
    for cut in (b"@q pos", b"@q po", b"@q p", b"pos", b"@q pos=-", b"pos="):  # "pos" cut by the line end
        it.append((cut, None, b"\n"))
        it.append((cut, b"7777", b"\n"))
    it.append((b"@t pos=3 pos=4", None, b"\n"))  # the first wins
    it.append((b"@t pos=-3 pos=4", None, b"\n"))
    it.append((b"@t pos=12pos=4", None, b"\n"))
    # a candidate within the 64 bytes the lanes look at but past the header's end: -1
    for h in (b"@a", b"@", b"", b"@ab", b"@abc"):
        for s in (b"pos=7", b"ACpos=-12GT", b"pos=1234567890123456"):
            it.append((h, s, b"\n"))
            it.append((h, s, b"\r\n"))
    it.append((b"@a pos=12", b"3456", b"\n"))  # the digits go on in the next line
    it.append((b"@a pos=-", b"5", b"\n"))
    if multibyte:  # valid multi-byte characters: the span takes the vline path
        for k in range(0, 20):
            it.append(("@".encode() + "é".encode() * k + b" pos=%d" % (100 + k), None, b"\n"))
        it.append(("@中中 pos=-9".encode(), None, b"\n"))
        it.append(("@\U0001F600 pos=10 é".encode(), None, b"\r\n"))
        it.append(("@é中\U0001F600".encode(), b"pos=7", b"\n"))
    return it


def family_p():
    out = []
    for name, mb in (("P_ascii", False), ("P_utf8", True)):
        parts, at = [], 0
        align = Counter()   # (header start & 3, header over 60 bytes) of tagged headers
        for i, (h, s, nl) in enumerate(_p_items(mb)):
            s = _seq(1 + (i * 5) % 7, i) if s is None else s  # lengths that move the next header's alignment
            if _POS.search(h):
                align[(at & 3, len(h) > 60)] += 1
            r = _rec(h, s, nl)
            parts.append(r)
            at += len(r)
        out.append(Case(name, "P", b"".join(parts), info={"align": align, "errors": 0}))
        assert all(align[(a, big)] > 0 for a in range(4) for big in (False, True)), align
    return out


# --- U: UTF-8 ---------------------------------------------------------------
U_VALID = [b"\xc2\x80", b"\xdf\xbf", b"\xe0\xa0\x80", b"\xed\x9f\xbf", b"\xee\x80\x80", b"\xef\xbf\xbf",
           b"\xf0\x90\x80\x80", b"\xf4\x8f\xbf\xbf"]
U_INVALID = [b"\xc0\x80", b"\xc1\xbf", b"\xe0\x9f\xbf", b"\xed\xa0\x80", b"\xed\xbf\xbf", b"\xf0\x8f\xbf\xbf",
             b"\xf4\x90\x80\x80", b"\xf5\x80\x80\x80", b"\xf8\x88\x80\x80\x80", b"\x80", b"\xff"]
# a sequence cut short by the line end (the last three give their own line end)
U_TRUNC = [(b"\xc3", b"\n"), (b"\xc3", b"\r\n"), (b"\xe2\x82", b"\n"), (b"\xf0\x90\x80", b"\r\n"), (b"\xc3", b"\n")]


def _u_line(role, form, k, at_end):
    """Line `role` of record k (0 header, 1 sequence, 2 plus, 3 quality) holding form."""
    if role == 0:
        return (b"@u%d " % k + form + b" pos=%d" % (k + 1) + (b"" if at_end else b" z")) if k % 2 \
            else (b"@u%d pos=%d " % (k, k + 1) + form)
    if role == 1:
        return b"AC" + form + (b"" if at_end else b"GT")
    if role == 2:
        return b"+" + form
    return b"II" + form + (b"" if at_end else b"II")


def _u_files():
    ev = []  # (role, form, newline, at_end, invalid)
    for role in range(4):
        bad = [(role, f, b"\n", False, True) for f in U_INVALID] + [(role, f, nl, True, True) for f, nl in U_TRUNC]
        for i, e in enumerate(bad):  # a valid form after every other invalid one
            ev.append(e)
            if i % 2 == 0:
                ev.append((role, U_VALID[i // 2], b"\n", False, False))
    # interleave the roles so that each file shifts the phase every way
    ev = [ev[(i % 4) * (len(ev) // 4) + i // 4] for i in range(len(ev))]
    files, cur, bad, k = [], [], 0, 0
    for role, f, nl, at_end, inv in ev:
        if inv and bad == 10:  # exactly ten invalid lines per file: read to the end
            files.append((b"".join(cur), bad))
            cur, bad = [], 0
        lines = [b"@r%d pos=%d" % (k, 3 * k), _seq(5 + k % 9, k), b"+", b"I" * (5 + k % 9)]
        lines[role] = _u_line(role, f, k, at_end)
        cur.append(b"".join(x + (nl if r == role else b"\n") for r, x in enumerate(lines)))
        cur.append(_rec(b"@s%d pos=-%d" % (k, k), _seq(3 + k % 5, k)))
        bad += inv
        k += 1
    files.append((b"".join(cur), bad))
    return files


class _Filler:
    """ASCII filler records; exact() pads the header to an exact record size."""

    def __init__(self, seed):
        rng = np.random.default_rng(seed)
        self.pool = bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 1 << 16)])
        self.lens = [int(x) for x in rng.integers(60, 250, 4099)]
        self.k = 0

    def record(self, m=None, pad=None):
        i = self.k
        self.k += 1
        m = self.lens[i % 4099] if m is None else m
        a = (i * 977) % ((1 << 16) - 256)
        h = b"@f%d pos=%d" % (i, (i * 7919) % 1000003)
        if pad is not None:
            h += b" " + b"x" * pad
        return _rec(h, self.pool[a:a + m])

    def exact(self, nbytes):
        k = self.k
        base = len(self.record(60, 0))
        self.k = k
        assert nbytes >= base, (nbytes, base)
        r = self.record(60, nbytes - base)
        assert len(r) == nbytes
        return r


class _Text:
    def __init__(self, seed):
        self.f, self.parts, self.n = _Filler(seed), [], 0

    def add(self, b):
        self.parts.append(b)
        self.n += len(b)

    def fill_to(self, target):
        """Filler records up to exactly byte `target` (a record boundary)."""
        assert target - self.n >= 400, (target, self.n)
        while target - self.n > 1400:
            self.add(self.f.record())
        self.add(self.f.exact(target - self.n))
        assert self.n == target

    def bytes(self):
        return b"".join(self.parts)


def _bad(k):
    return b"bad%d " % k + U_INVALID[k % len(U_INVALID)] + b" line\n"


def family_u():
    out = [Case("U_forms%d" % i, "U", d, info={"errors": bad}) for i, (d, bad) in enumerate(_u_files())]
    assert sum(c.info["errors"] == 10 for c in out) >= 4 and all(c.info["errors"] <= 10 for c in out)
    body = b"".join(_rec(b"@v%d pos=%d" % (k, k), _seq(20 + k, k)) for k in range(30))
    # the 11th invalid line
    out.append(Case("U_err_first", "U", b"".join(_bad(k) for k in range(11)) + body,
                    info={"code": E_INVALID, "err_line": 0}))
    mid = b"".join(_rec(b"@w%d pos=%d" % (k, k), _seq(9, k)) + _bad(k) for k in range(10))
    out.append(Case("U_err_same_span", "U", body + mid + body + b"@x pos=1\n" + _bad(10) + body,
                    info={"code": E_INVALID, "err_line": 120 + 40 + 120 + 1}))
    t, bad_at = _Text(101), []
    for k in range(10):
        t.fill_to(90_000 * (k + 1))
        bad_at.append(t.n)
        t.add(_bad(k))
    t.fill_to(SPAN + 5000)
    t.add(b"@y pos=4\nACGT\n")
    bad_at.append(t.n)
    t.add(_bad(10) + body)
    assert bad_at[9] + len(_bad(9)) < SPAN < bad_at[10]  # the count is carried from the first span to the second
    out.append(Case("U_err_next_span", "U", t.bytes(), block=CUT_BLOCK, info={"code": E_INVALID, "bad_at": bad_at}))
    # a too-long read and the 11th invalid line in one span: whichever comes first in the file
    long_rec = _rec(b"@long pos=1", _seq(300))
    out.append(Case("U_long_before_err", "U", body + mid + long_rec + body + _bad(10) + body,
                    info={"code": E_RANGE, "err_line": 120 + 40 + 2}))
    out.append(Case("U_long_between", "U", long_rec.join([body + mid[:len(mid) // 2], mid[len(mid) // 2:] + _bad(10)]),
                    info={"code": E_RANGE}))
    out.append(Case("U_long_after_err", "U", body + mid + _bad(10) + body + long_rec + body,
                    info={"code": E_INVALID, "err_line": 120 + 40}))
    return out


# --- E: line ends -----------------------------------------------------------
def family_e():
    a = _rec(b"@a pos=1", b"ACGT")
    s32 = _seq(32)
    raw = {
        "E_cr_eof_seq": a + b"@b pos=2\nACGT\r",            # the read is the 5 bytes ACGT\r
        "E_cr_eof_header": a + b"@b pos=2\r",
        "E_cr_eof_quality": a + b"@b pos=2\nAC\n+\nII\r",
        "E_cr_eof_crlf_file": a.replace(b"\n", b"\r\n") + b"@b pos=2\r\nACGT\r",
        "E_crcrlf": a + b"@b pos=2\r\r\nACGT\r\r\n+\nIIII\r\r\n" + a,
        "E_crlf_only_lines": a + b"\r\n" + b"\r\n" + b"\r\n" + b"\r\n" + a + b"@c pos=3\r\n\r\n+\r\n\r\n" + a,
        "E_lone_cr": a + b"@b\rpos=2\nAC\rGT\n+\nII\rII\n\rACGT\nAC\r\n+\nII\n",
        "E_single_nl": b"\n",
        "E_single_cr": b"\r",
        "E_cr_only_seq_eof": b"@b pos=5\n\r",                # the read is the 1 byte \r
        "E_empty_seq_crlf": b"@a pos=1\r\n\r\n+\r\n\r\n@b pos=2\r\nAC\r\n+\r\nII\r\n",
        "E_stride_crlf": a + _rec(b"@b pos=2", s32, b"\r\n") + a,
        "E_stride_plus1_crlf": a + _rec(b"@b pos=2", s32 + b"A", b"\r\n") + a,
        "E_stride_cr_eof": a + b"@b pos=2\n" + s32 + b"\r",   # 33 bytes: too long
        "E_stride_crlf_eof": a + b"@b pos=2\n" + s32[:31] + b"\r",  # 32 bytes with its \r
    }
    codes = {"E_stride_plus1_crlf": E_RANGE, "E_stride_cr_eof": E_RANGE}
    return [Case(n, "E", d, stride=32, block=7, info={"code": codes.get(n, 0)}) for n, d in raw.items()]


# --- C: span cuts -----------------------------------------------------------
def _situations():
    """(label, bytes before the cut, bytes after it)."""
    S = _seq(48)
    tail = S + b"\n+\n" + b"I" * 48 + b"\n"
    sit = [
        ("after_header_over_60", b"@long " + b"y" * 64 + b" pos=4242\n", tail),
        # a multi-byte header: the span's closing header is found through vline
        ("after_header_negative", b"@neg \xc3\xa9 pos=-77\n", tail),
        ("after_header_no_tag", b"@notag\n", tail),
        ("inside_digits", b"@dig pos=12", b"345 t\n" + tail),
        ("between_cr_and_lf", b"@crlf pos=9\r\n" + S + b"\r", b"\n+\r\n" + b"I" * 48 + b"\r\n"),
        ("after_sequence", b"@s pos=5\n" + S + b"\n", b"+\n" + b"I" * 48 + b"\n"),
        ("after_plus", b"@p pos=6\n" + S + b"\n+\n", b"I" * 48 + b"\n"),
        ("after_quality", _rec(b"@q pos=7", S), _rec(b"@nx pos=31", S[:20])),
    ]
    for c in range(1, 18):  # every b.begin & 15
        sit.append(("mid_sequence_%d" % c, b"@m%d pos=%d\n" % (c, 1000 + c) + S[:c], S[c:] + b"\n+\n" + b"I" * 48 + b"\n"))
    sit += [
        # inside a valid 3-byte character; the header's rest, in the next span, is ASCII
        ("inside_utf8_char", b"@u \xe4\xb8", b"\xad pos=66\n" + tail),
        # the only high bytes of the next span's text are in the carried part
        ("utf8_carried", b"@u \xe4\xb8\xad po", b"s=67\n" + tail),
        # an extra, invalid line (skipped, not counted)
        ("inside_invalid_line", b"junk \xff\xfe", b" more\n" + _rec(b"@g pos=8", S)),
    ]
    return sit


def family_c():
    sit = _situations()
    assert len(sit) == 28
    groups = [(sit[2 * k:2 * k + 2], None) for k in range(13)] + [([sit[26]], "nl"), ([sit[27]], "no_nl")]
    out = []
    for gi, (ss, end) in enumerate(groups):
        t, marks = _Text(200 + gi), []
        for i, (label, pre, post) in enumerate(ss):
            cut = (i + 1) * SPAN
            t.fill_to(cut - len(pre))
            t.add(pre)
            t.add(post)
            marks.append((cut, pre, post))
        if end is None:
            for _ in range(3):
                t.add(t.f.record())
            data = t.bytes()
        else:  # the text ends exactly where a span would
            t.fill_to((len(ss) + 1) * SPAN + (end == "no_nl"))
            data = t.bytes() if end == "nl" else t.bytes()[:-1]
            assert len(data) == (len(ss) + 1) * SPAN and (data[-1:] == b"\n") == (end == "nl")
        c = Case("C_" + "+".join(s[0] for s in ss) + ("+end_" + end if end else ""), "C", data, block=CUT_BLOCK,
                 marks=marks, info={"labels": [s[0] for s in ss], "end": end})
        check_cuts(c)
        out.append(c)
    return out


def check_cuts(c: Case):
    """Each chosen byte pair sits on the two sides of a cut the reader makes."""
    assert c.cuts == [m[0] for m in c.marks], (c.name, c.cuts)
    for cut, pre, post in c.marks:
        assert c.data[cut - len(pre):cut] == pre and c.data[cut:cut + len(post)] == post, (c.name, cut)


@functools.lru_cache(maxsize=None)
def family(f):
    return tuple({"P": family_p, "U": family_u, "E": family_e, "C": family_c}[f]())


def cases(families="PUEC"):
    return [c for f in families for c in family(f)]


@functools.lru_cache(maxsize=None)
def _reference(name, with_pos):
    c = {c.name: c for c in cases()}[name]
    return reference_parse(c.data, c.stride, with_pos)


def reference(c: Case, with_pos=True) -> Parsed:
    """reference_parse of a case, computed once and shared (leave it unchanged)."""
    return _reference(c.name, with_pos)
