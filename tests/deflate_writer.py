"""A token-level DEFLATE (RFC 1951) writer, an independent interpreter of its
tokens, and the corpus of hand-built streams that no compressor emits.

The token list is the ground truth of a case: `interpret` gives the bytes it
stands for (a byte-at-a-time loop that shares nothing with the encoder),
tests/test_deflate_writer.py confirms every case against zlib on the CPU, and
tests/test_gpu_inflate_streams.py feeds the same cases to msw_inflate.hip.

Tokens: ("lit", b), ("match", len, dist), ("eob",), ("stored", bytes) and the
raw escapes ("ll_sym", sym, extra), ("d_sym", sym, extra), ("bits", v, n).
"""
import functools
import struct
import zlib
from collections import namedtuple
from dataclasses import dataclass, field

import numpy as np

from mini_parallel_amd.synthetic import BGZF_EOF

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
            227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
             4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [k for k in range(1, 14) for _ in (0, 1)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32


class BitWriter:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, v, n):  # a field: least significant bit first
        assert 0 <= v < (1 << n) or n == 0
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, n):  # a Huffman code: most significant bit first
        self.bits(int(format(c, "0%db" % n)[::-1], 2) if n else 0, n)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def raw(self, data):
        assert self.n == 0
        self.out += data

    def bitlen(self):
        return 8 * len(self.out) + self.n

    def getvalue(self):
        return bytes(self.out) + (bytes([self.acc]) if self.n else b"")


def canon_codes(lens):
    """Canonical codes (RFC 1951 3.2.2) of a list of code lengths, as
    (code, length) or None per symbol.  An over-subscribed list still gets
    codes (cut to their length): the error cases need to write them."""
    top = max(lens, default=0)
    cnt = [0] * (top + 2)
    for l in lens:
        if l:
            cnt[l] += 1
    nxt, code = [0] * (top + 2), 0
    for b in range(1, top + 1):
        code = (code + cnt[b - 1]) << 1
        nxt[b] = code
    out = []
    for l in lens:
        if l:
            out.append((nxt[l] & ((1 << l) - 1), l))
            nxt[l] += 1
        else:
            out.append(None)
    return out


def balanced_lens(n):
    """Lengths of a complete code over n >= 2 symbols, as flat as possible."""
    assert n >= 2
    d = (n - 1).bit_length()
    short = (1 << d) - n
    return [d - 1] * short + [d] * (n - short)


def random_code(rng, n_syms, max_len):
    """A complete code: from one leaf, split random leaves shorter than
    max_len until there are n_syms (half the time a deepest one, so that long
    codes appear).  Returns the lengths in random symbol order."""
    assert 2 <= n_syms <= (1 << max_len)
    leaves = [0]
    while len(leaves) < n_syms:
        ok = [i for i, l in enumerate(leaves) if l < max_len]
        if rng.random() < 0.5:
            deep = max(leaves[i] for i in ok)
            ok = [i for i in ok if leaves[i] == deep]
        i = ok[int(rng.integers(len(ok)))]
        leaves[i] += 1
        leaves.append(leaves[i])
    assert sum(1 << (max_len - l) for l in leaves) == 1 << max_len
    return [int(leaves[i]) for i in rng.permutation(n_syms)]


def len_sym(length):
    if length == 258:
        return 285, 0
    i = max(k for k in range(28) if LEN_BASE[k] <= length)
    return 257 + i, length - LEN_BASE[i]


def dist_sym(dist):
    i = max(k for k in range(30) if DIST_BASE[k] <= dist)
    return i, dist - DIST_BASE[i]


def ll_extra_bits(sym):
    return LEN_EXTRA[sym - 257] if 257 <= sym <= 285 else 0


def d_extra_bits(sym):
    return DIST_EXTRA[sym] if sym <= 29 else 0


def token_syms(tokens):
    """(lit/len symbols, distance symbols) a token list uses."""
    ll, d = set(), set()
    for t in tokens:
        if t[0] == "lit":
            ll.add(t[1])
        elif t[0] == "match":
            ll.add(len_sym(t[1])[0])
            d.add(dist_sym(t[2])[0])
        elif t[0] == "eob":
            ll.add(256)
        elif t[0] == "ll_sym":
            ll.add(t[1])
        elif t[0] == "d_sym":
            d.add(t[1])
    return ll, d


def lens_over(used, n):
    """n code lengths: a flat complete code over the symbols in `used`."""
    used = sorted(used)
    out = [0] * n
    for s, l in zip(used, balanced_lens(len(used))):
        out[s] = l
    return out


def auto_lens(tokens):
    """Lit/len and distance lengths that cover a token list (end of block
    included): flat complete codes; no distance code -> one zero length, one
    distance symbol -> a single 1-bit code (both legal, inftrees.c)."""
    ll, d = token_syms(tokens)
    ll.add(256)
    if len(ll) < 2:
        ll.add(0)
    ll_lens = lens_over(ll, max(max(ll) + 1, 257))
    if not d:
        d_lens = [0]
    elif len(d) == 1:
        d_lens = [0] * max(d) + [1]
    else:
        d_lens = lens_over(d, max(d) + 1)
    return ll_lens, d_lens


def plain_cl_syms(lens):
    return [(l, 0) for l in lens]


def rle_cl_syms(lens):
    """The lengths as code-length symbols with greedy 16/17/18 runs over the
    joined sequence (so a run crosses from the lit/len into the distance
    lengths wherever the values allow it)."""
    out, i, n = [], 0, len(lens)
    while i < n:
        v, run = lens[i], 1
        while i + run < n and lens[i + run] == v:
            run += 1
        if v == 0 and run >= 3:
            r = min(run, 138)
            out.append((18, r - 11) if r >= 11 else (17, r - 3))
        elif i > 0 and v == lens[i - 1] and run >= 3:
            r = min(run, 6)
            out.append((16, r - 3))
        else:
            r = 1
            out.append((v, 0))
        i += r
    return out


def expand_cl_syms(cl_syms):
    out = []
    for s, x in cl_syms:
        if s < 16:
            out.append(s)
        elif s == 16:
            out += [out[-1]] * (3 + x)
        elif s == 17:
            out += [0] * (3 + x)
        else:
            out += [0] * (11 + x)
    return out


def cl_features(cl_syms, nlen):
    """What the code-length symbol sequence of a header exercises."""
    tags, idx, prev, last = set(), 0, None, 0
    for s, x in cl_syms:
        rep = 1 if s < 16 else 3 + x if s < 18 else 11 + x
        last = s if s < 16 else last if s == 16 else 0  # the length this symbol writes
        if s >= 16 and idx < nlen < idx + rep:
            tags.add("rep%d_crosses_nlen" % s)
            if s == 16 and last != 0:
                tags.add("rep16_nonzero_crosses_nlen")
        if s == 16 and prev == 18:
            tags.add("rep16_after_rep18")
        if (s, rep) in ((16, 6), (17, 10), (18, 138)):
            tags.add("max_rep%d" % s)
        idx += rep
        prev = s
    return tags


Ev = namedtuple("Ev", "kind bit bits ll_len d_len out dist opos")  # a Huffman token as written: where, how long


class Stream:
    """One raw deflate stream in the making: the bits and the token list."""

    def __init__(self):
        self.w = BitWriter()
        self.tokens = []
        self.tags = set()
        self.stored_at = []  # (bit alignment of the block header, LEN, output position)
        self.ll_code_bits = 0  # longest lit/len and distance codes written
        self.d_code_bits = 0
        self.opos = 0  # output bytes so far (lengths only; the bytes are interpret's business)
        self._pend = 0
        self.blocks = []  # per block: its Huffman tokens as Ev records (window_paths), None for a stored block

    def _tokens(self, tokens, ll, d):
        w = self.w
        events = []
        self.blocks.append(events)
        for t in tokens:
            k = t[0]
            bit0, opos0 = w.bitlen(), self.opos
            if k == "lit":
                w.code(*ll[t[1]])
                self.ll_code_bits = max(self.ll_code_bits, ll[t[1]][1])
            elif k == "eob":
                w.code(*ll[256])
            elif k == "match":
                s, x = len_sym(t[1])
                w.code(*ll[s])
                w.bits(x, ll_extra_bits(s))
                ds, dx = dist_sym(t[2])
                w.code(*d[ds])
                w.bits(dx, d_extra_bits(ds))
                self.ll_code_bits = max(self.ll_code_bits, ll[s][1])
                self.d_code_bits = max(self.d_code_bits, d[ds][1])
            elif k == "ll_sym":
                w.code(*ll[t[1]])
                w.bits(t[2], ll_extra_bits(t[1]))
            elif k == "d_sym":
                w.code(*d[t[1]])
                w.bits(t[2], d_extra_bits(t[1]))
            elif k == "bits":
                w.bits(t[1], t[2])
            else:
                raise ValueError(t)
            if k == "lit" or (k == "ll_sym" and t[1] < 256):
                self.opos += 1
            elif k == "match":
                self.opos += t[1]
            elif k == "ll_sym" and 257 <= t[1] <= 285:
                self._pend = LEN_BASE[t[1] - 257] + t[2]
            elif k == "d_sym":
                self.opos, self._pend = self.opos + self._pend, 0
            if k == "lit":
                events.append(Ev("lit", bit0, w.bitlen() - bit0, ll[t[1]][1], 0, 1, 0, opos0))
            elif k == "match":
                events.append(Ev("match", bit0, w.bitlen() - bit0, ll[len_sym(t[1])[0]][1], d[dist_sym(t[2])[0]][1],
                                 t[1], t[2], opos0))
            else:  # the model stops at anything else (end of block) or refuses it (raw escapes)
                events.append(Ev(k, bit0, w.bitlen() - bit0, 0, 0, 0, 0, opos0))
            self.tokens.append(t)

    def fixed(self, tokens, final=False, eob=True):
        self.w.bits(int(final), 1)
        self.w.bits(1, 2)
        self._tokens(list(tokens) + ([("eob",)] if eob else []), canon_codes(FIXED_LL), canon_codes(FIXED_D))
        return self

    def dynamic(self, tokens, final=False, eob=True, ll_lens=None, d_lens=None, cl_lens=None, hclen=None,
                cl_syms=None, check=True):
        """A dynamic block.  Everything the header holds may be given; what is
        not is derived: lengths from the tokens (auto_lens), the code-length
        symbols as a plain sequence, a flat code-length code over the symbols
        that sequence uses, the smallest HCLEN that holds it."""
        tokens = list(tokens) + ([("eob",)] if eob else [])
        if ll_lens is None or d_lens is None:
            a, b = auto_lens(tokens)
            ll_lens = a if ll_lens is None else ll_lens
            d_lens = b if d_lens is None else d_lens
        if cl_syms is None:
            cl_syms = plain_cl_syms(list(ll_lens) + list(d_lens))
        if check:
            assert expand_cl_syms(cl_syms) == list(ll_lens) + list(d_lens)
        if cl_lens is None:
            used = {s for s, _ in cl_syms}
            if len(used) < 2:
                used.add(0 if 0 not in used else 1)
            cl_lens = lens_over(used, 19)
        if hclen is None:
            hclen = max([4] + [i + 1 for i, s in enumerate(CL_ORDER) if cl_lens[s]])
        w = self.w
        w.bits(int(final), 1)
        w.bits(2, 2)
        w.bits(len(ll_lens) - 257, 5)
        w.bits(len(d_lens) - 1, 5)
        w.bits(hclen - 4, 4)
        for i in range(hclen):
            w.bits(cl_lens[CL_ORDER[i]], 3)
        cl = canon_codes(cl_lens)
        for s, x in cl_syms:
            w.code(*cl[s])
            w.bits(x, {16: 2, 17: 3, 18: 7}.get(s, 0))
        self.tags |= cl_features(cl_syms, len(ll_lens))
        self.tags |= {"hclen%d" % hclen, "nlen%d" % len(ll_lens), "ndist%d" % len(d_lens),
                      "cl_maxlen%d" % max(cl_lens)}
        self._tokens(tokens, canon_codes(ll_lens), canon_codes(d_lens))
        return self

    def stored(self, data, final=False, nlen=None):
        w = self.w
        self.stored_at.append((w.bitlen() % 8, len(data), self.opos))
        self.blocks.append(None)
        self.opos += len(data)
        w.bits(int(final), 1)
        w.bits(0, 2)
        w.align()
        w.bits(len(data), 16)
        w.bits((~len(data) & 0xFFFF) if nlen is None else nlen, 16)
        w.raw(data)
        self.tokens.append(("stored", bytes(data)))
        return self

    def filler(self, n):
        """Bytes after an offending token, so that the error is no truncation."""
        self.w.align()
        self.w.raw(b"\0" * n)
        return self

    def raw(self):
        return self.w.getvalue()


def _walk(tokens):
    """The independent interpreter: (bytes, matches) of a token list, the
    matches as (opos, len, dist).  One byte at a time."""
    out, matches, pend = bytearray(), [], None
    for t in tokens:
        k = t[0]
        length = dist = None
        if k == "lit":
            out.append(t[1])
        elif k == "stored":
            for b in t[1]:
                out.append(b)
        elif k == "match":
            length, dist = t[1], t[2]
        elif k == "ll_sym":
            if t[1] < 256:
                out.append(t[1])
            elif 257 <= t[1] <= 285:
                pend = LEN_BASE[t[1] - 257] + t[2]
        elif k == "d_sym" and pend is not None and t[1] <= 29:
            length, dist, pend = pend, DIST_BASE[t[1]] + t[2], None
        if length is not None:
            if dist > len(out):
                raise ValueError("distance %d at output position %d" % (dist, len(out)))
            matches.append((len(out), length, dist))
            for _ in range(length):
                out.append(out[-dist])
    return bytes(out), matches


def interpret(tokens):
    return _walk(tokens)[0]


def classify(tokens, ring=2048):
    """Each match as (opos, len, dist, classes), the classes as
    msw_inflate.hip's comments define them: overlap = "dist < len" (copy_near's
    reciprocal branch); near = "dist + len <= kRing" (copy_match), else far
    (the flushed output in L2); reaches_start = the window's "dist <= opos" at
    its edge; crosses_flush = the copy completes a 256-byte chunk ("every
    completed 256-byte chunk is flushed"); crosses_ring_wrap = its destination
    or its ring-resident source passes a multiple of the ring size."""
    out = []
    for opos, length, dist in _walk(tokens)[1]:
        c = set()
        if dist < length:
            c.add("overlap")
        c.add("near" if dist + length <= ring else "far")
        if dist == opos:
            c.add("reaches_start")
        if (opos + length) // 256 > opos // 256:
            c.add("crosses_flush")
        src = opos - dist
        if opos // ring != (opos + length - 1) // ring or \
                ("near" in c and src // ring != (src + min(length, dist) - 1) // ring):
            c.add("crosses_ring_wrap")
        out.append((opos, length, dist, c))
    return out


def window_paths(s, coff=0):
    """Which decode path of msw_inflate.hip takes each match of Stream s when
    its deflate data starts at byte `coff` of the compressed buffer (only
    coff mod 4 matters): a model of the token loop's control flow, from the
    kernel's comments and code.  Returns (path, opos, len, dist, lane) per
    match, path one of
      "window": lane-parallel emission; `lane` is the window lane of the
                match's first byte, so byte j of it is made by lane + j with
                off = j in the window's off mod d multiply;
      "walk":   the window's serial walk (copy_match), W > 64;
      "scalar": the one-token scalar step (copy_match).
    The rules modelled: a window starts at a token while the member has >= 112
    bits left, in the kernel's dword arithmetic (pw, pb against ew, eb); its
    chain takes tokens while the next starts below bit 64 and is simple: a
    lit/len code of at most kFastBits = 9 bits (a literal entry packs up to
    three literals whose codes fit in 9 bits together), for a match also a
    distance code of at most kFastDBits = 7 bits and dist <= opos at the
    window's START; the chain's output W <= 64 is emitted by the lanes, W > 64
    walked serially; a token that ends the chain below bit 64 goes to the
    scalar step, which takes one table entry.  Raw escapes are not modelled."""
    cend = coff + len(s.raw())
    ew, eb = cend >> 2, 8 * (cend & 3)
    found = []

    def entry(ev, j, opos0):  # tokens the table entry at token j resolves (0: not simple)
        t = ev[j]
        if t.kind == "match":
            return int(t.ll_len <= 9 and t.d_len <= 7 and (opos0 is None or t.dist <= opos0))
        if t.kind != "lit" or t.ll_len > 9:
            return 0
        n, used = 1, t.ll_len
        while n < 3 and j + n < len(ev) and ev[j + n].kind == "lit" and used + ev[j + n].ll_len <= 9:
            used += ev[j + n].ll_len
            n += 1
        return n

    for ev in s.blocks:
        i = 0
        while ev is not None and i < len(ev):
            pos = 8 * coff + ev[i].bit
            pw, pb = pos >> 5, pos & 31
            if pw < ew - 4 or (pw == ew - 4 and eb + 16 >= pb):
                opos0, k, width, j, chain = ev[i].opos, 0, 0, i, []
                while k < 64 and j < len(ev):
                    n = entry(ev, j, opos0)
                    if not n:
                        break
                    if ev[j].kind == "match":
                        chain.append((ev[j], width))
                    k += sum(e.bits for e in ev[j:j + n])
                    width += sum(e.out for e in ev[j:j + n])
                    j += n
                for t, lane in chain:
                    found.append(("window" if width <= 64 else "walk", t.opos, t.out, t.dist, lane if width <= 64 else None))
                i = j
                if k >= 64:
                    continue
            # the scalar step: one table entry at token i
            t = ev[i]
            if t.kind == "lit":
                i += max(1, entry(ev, i, None))  # a code longer than 9 bits: one literal
            elif t.kind == "match":
                found.append(("scalar", t.opos, t.out, t.dist, None))
                i += 1
            elif t.kind == "eob":
                i = len(ev)
            else:
                raise NotImplementedError(t.kind)
    return found


def bgzf_member(raw, plain, isize=None, crc=None):
    """Raw deflate as a BGZF member (header and trailer as in
    mini_parallel_amd.synthetic.bgzf_compress)."""
    assert len(raw) + 25 <= 0xFFFF
    return struct.pack("<4BIBBH2BHH", 0x1F, 0x8B, 8, 4, 0, 0, 0xFF, 6, ord("B"), ord("C"), 2, len(raw) + 25) + raw \
        + struct.pack("<II", (zlib.crc32(plain) & 0xFFFFFFFF) if crc is None else crc,
                      len(plain) if isize is None else isize)


# ---------------------------------------------------------------------------
# The corpus
# ---------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    family: str
    raw: bytes
    plain: bytes            # valid: the whole output; error: the bytes before the error
    tokens: list
    kind: str = "valid"     # "valid" | "error" (zlib rejects the stream) | "trailer" (valid deflate, wrong trailer)
    zlib_msg: str = ""      # error: how zlib's message ends
    text: str = ""          # error / trailer: the project's status text
    isize: int = None
    crc: int = None
    tags: set = field(default_factory=set)
    stream: Stream = None

    def member(self):
        return bgzf_member(self.raw, self.plain, self.isize, self.crc)


def _case(name, family, s, **kw):
    toks = s.tokens
    plain = kw.pop("plain", None)
    if plain is None:
        plain = interpret(toks)
    tags = set(s.tags) | kw.pop("tags", set())
    return Case(name, family, s.raw(), plain, toks, tags=tags, stream=s, **kw)


def _lits(data):
    return [("lit", b) for b in data]


def _rand(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


TAIL = _lits(b"tail-of-sixteen.")  # 128 bits behind the token under test: a window can start there (>= 112 left)


def family_a():
    """Overlap sweep with the fixed code: d seed literals in a block of their
    own, then a block of k literals, the match and the tail.  The window that
    holds the match starts at that block's first token with d bytes of output
    behind it, so the match resolves in the window, k lanes in: lengths 3 and 4
    are emitted by the lanes, the longer ones (with the tail W > 64) take the
    serial walk and, where d < len, copy_near's reciprocal branch."""
    out = []
    for d in range(1, 67):
        seed = _rand(1000 + d, d + 3)
        for length in (3, 4, 63, 64, 65, 258):
            for k in range(4):
                s = Stream().fixed(_lits(seed[:d])).fixed(_lits(seed[d:d + k]) + [("match", length, d)] + TAIL, final=True)
                out.append(_case("A_d%d_len%d_k%d" % (d, length, k), "A", s, tags={"A:%d:%d:%d" % (d, length, k)}))
    return out


W_FORMS = ((0, 64), (1, 63), (2, 62), (3, 61), (0, 58), (1, 60))  # (literals before the match in its window, length)


def family_w():
    """The window's lane-parallel emission at every (d, off): d + 3 seed
    literals in a block of their own, then a block of p literals, the match
    and nothing else (end of block is not simple, so the window's chain ends
    there with W = p + len <= 64), then the tail in a third block.  With
    (p, len) = (0, 64) lane j makes byte j of the match: off = 0..63 against
    every d in 1..63 (the off mod d multiply), 64..66 (d >= 64: lane 0's
    M = 0); with p > 0 the match also reads the window's own literals where
    d <= p (pointer jumping)."""
    out = []
    for d in range(1, 67):
        seed = _rand(3000 + d, d + 6)
        for p, length in W_FORMS:
            s = Stream().fixed(_lits(seed[:d + 3])).fixed(_lits(seed[d + 3:d + 3 + p]) + [("match", length, d)])
            s.fixed(TAIL + TAIL, final=True)
            out.append(_case("W_d%d_p%d_len%d" % (d, p, length), "W", s, tags={"W:%d:%d:%d" % (d, p, length)}))
    return out


B_POS = (4096, 4097, 4095, 2560, 2561, 2559)  # >= 2050 + 258: the walk placement's window starts with d bytes behind it


def b_matches():
    m = [(t - length, length) for length in (3, 64, 258) for t in (2047, 2048, 2049)]
    m += [(d, 3) for d in range(2046, 2051)]
    m += [(d, length) for d in sorted(set(range(190, 331, 35)) | {255, 256, 257}) for length in (64, 258)]
    return sorted(set(m))


B_PLACES = ("first", "after2", "walk", "scalar")


def b_path(place, length):
    """The decode path a placement of family B gives a match of this length
    (tests/test_deflate_writer.py holds window_paths to it)."""
    if place in ("walk", "scalar"):
        return place
    return "window" if length + (2 if place == "after2" else 0) <= 64 else "walk"


def family_b():
    """Ring and flush edges behind a stored prefix.  Each match is placed
    first in a window and alone in its block (W = len: emitted by the lanes up
    to 64 bytes, lane j's source at -d + j from the window's start), after two
    literals (the source relative to the window's start is no longer -d), behind
    a 258-byte match (W > 64: the serial walk), and as the member's last token
    (fewer than 112 bits left: the scalar step)."""
    out = []
    for d, length in b_matches():
        for pos in B_POS:
            pre = _rand(d * 7 + pos, pos)
            for place in B_PLACES:
                s = Stream()
                if place == "first":
                    s.stored(pre).fixed([("match", length, d)]).fixed(TAIL, final=True)
                elif place == "after2":
                    s.stored(pre[:-2]).fixed(_lits(pre[-2:]) + [("match", length, d)]).fixed(TAIL, final=True)
                elif place == "walk":
                    s.stored(pre[:-258]).fixed([("match", 258, 500), ("match", length, d)] + TAIL, final=True)
                else:
                    s.stored(pre).fixed([("match", length, d)], final=True)
                out.append(_case("B_d%d_len%d_at%d_%s" % (d, length, pos, place), "B", s,
                                 tags={"B:%d:%d:%d:%s" % (d, length, pos, place)}))
    return out


def family_c():
    """Far distances and matches that reach byte 0 of the member; members of
    1, 2 and 3 bytes in between shift the output offset through all of mod 4."""
    out, n = [], 0

    def tiny():
        nonlocal n
        n += 1
        k = 1 + n % 3
        return _case("C_tiny%d_%d" % (k, n), "C", Stream().fixed(_lits(_rand(n, k)), final=True), tags={"C:tiny%d" % k})

    for d in (4096, 16384, 32767, 32768):
        for opos in (d, d + 1):
            for length in (3, 258):
                s = Stream().stored(_rand(d + opos + length, opos)).fixed([("match", length, d)] + TAIL, final=True)
                out += [tiny(), _case("C_far_d%d_at%d_len%d" % (d, opos, length), "C", s,
                                      tags={"C:far:%d:%d:%d" % (d, opos - d, length)})]
    for opos in range(1, 71):
        length = (3, 64, 258, 10, 65)[opos % 5]
        s = Stream().fixed(_lits(_rand(300 + opos, opos)) + [("match", length, opos)] + TAIL, final=True)
        out.append(_case("C_start_at%d_len%d" % (opos, length), "C", s, tags={"C:start:%d" % opos}))
        if opos % 9 == 0:
            out.append(tiny())
    s = Stream().stored(_rand(77, 65000)).fixed(
        [("match", 258, 32768), ("match", 258, 4096), ("match", 20, 32768)], final=True)
    out.append(_case("C_full_65536", "C", s, tags={"C:full"}))
    assert len(out[-1].plain) == 65536
    return out


EDGE_LENS = (3, 4, 63, 64, 65, 257, 258)
EDGE_DISTS = (1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 1790, 1791, 1984, 2044, 2045, 2046, 2047, 2048, 2049, 2050,
              4096, 16384, 32767, 32768)


def random_tokens(rng, size):
    """A token stream of about `size` output bytes: literal runs and matches,
    half of the lengths and distances on the boundary values of A-C."""
    toks, opos = [], 0
    alpha = rng.integers(0, 256, int(rng.integers(2, 40)))
    while opos < size:
        if opos == 0 or rng.random() < 0.3:
            n = int(rng.integers(1, 9))
            lits = alpha[rng.integers(0, len(alpha), n)] if rng.random() < 0.8 else rng.integers(0, 256, n)
            toks += [("lit", int(b)) for b in lits]
            opos += n
            continue
        length = int(rng.choice(EDGE_LENS)) if rng.random() < 0.5 else int(rng.integers(3, 259))
        if rng.random() < 0.5:
            cand = [d for d in EDGE_DISTS + (opos, 2048 - length, 2049 - length) if 1 <= d <= min(opos, 32768)]
            dist = int(cand[int(rng.integers(len(cand)))])
        else:
            dist = int(min(opos, 32768, 1 + int(2 ** (rng.random() * 15))))
        length = min(length, 65536 - opos)
        if length < 3:
            break
        toks.append(("match", length, dist))
        opos += length
    return toks


def family_d():
    out = []
    for i in range(150):
        rng = np.random.default_rng(5000 + i)
        size = 65000 if i % 30 == 0 else int(rng.integers(20000, 40000) if i % 10 == 0 else rng.integers(200, 6000))
        toks = random_tokens(rng, size)
        out.append(_case("D%d_fixed" % i, "D", Stream().fixed(toks, final=True)))
        used_ll, used_d = token_syms(toks)
        while True:  # redraw until the stream writes a lit/len code over kFastBits and a distance code over kFastDBits
            ll_lens, d_lens = random_code(rng, 286, 15), random_code(rng, 30, 15)
            if max(ll_lens[x] for x in used_ll) > 9 and max(d_lens[x] for x in used_d) > 7:
                break
        out.append(_case("D%d_longcodes" % i, "D", Stream().dynamic(toks, final=True, ll_lens=ll_lens, d_lens=d_lens)))
        # split at random token positions into fixed, dynamic, stored and empty blocks
        s, p = Stream(), 0
        while p < len(toks):
            q = min(len(toks), p + int(rng.integers(1, max(2, len(toks) // 4))))
            how = int(rng.integers(5))
            if how == 0 and toks[p][0] == "lit":
                q = p
                while q < len(toks) and toks[q][0] == "lit" and q - p < 300:
                    q += 1
                s.stored(bytes(t[1] for t in toks[p:q]))
            elif how == 1:
                s.dynamic(toks[p:q], cl_syms=None)
            elif how == 2:
                a, b = auto_lens(toks[p:q] + [("eob",)])
                s.dynamic(toks[p:q], ll_lens=a, d_lens=b, cl_syms=rle_cl_syms(a + b))
            elif how == 3:
                s.fixed([]) if rng.random() < 0.5 else s.stored(b"")
                q = p
            else:
                s.fixed(toks[p:q])
            p = q
        s.fixed([], final=True)
        c = _case("D%d_split" % i, "D", s)
        assert c.plain == out[-1].plain
        out.append(c)
    return out


def family_e():
    """Header forms zlib's compressor never writes."""
    out = []
    z138, z118 = (18, 127), (18, 107)
    eob_only = dict(ll_lens=[0] * 256 + [1], d_lens=[0], cl_syms=[z138, z118, (1, 0), (0, 0)])
    out.append(_case("E_eob_only_empty_member", "E", Stream().dynamic([], final=True, **eob_only), tags={"E:eob_only"}))
    s = Stream().fixed(_lits(b"before")).dynamic([], **eob_only).fixed(_lits(b"after") + [("match", 5, 11)], final=True)
    out.append(_case("E_eob_only_between_blocks", "E", s, tags={"E:eob_only_between"}))
    s = Stream().dynamic(_lits(b"no distance codes at all, literals only " * 3), final=True)
    assert "ndist1" in s.tags
    out.append(_case("E_no_distance_codes", "E", s, tags={"E:no_dist"}))
    s = Stream().dynamic(_lits(b"abc") + [("match", 40, 1), ("lit", 120), ("match", 3, 1)] + TAIL, final=True)
    out.append(_case("E_one_distance_code_sym0", "E", s, tags={"E:one_dist"}))
    s = Stream().dynamic(_lits(b"abcdefgh") + [("match", 40, 5), ("lit", 120), ("match", 258, 6)] + TAIL, final=True)
    out.append(_case("E_one_distance_code_sym4", "E", s, tags={"E:one_dist"}))
    rng = np.random.default_rng(60)
    toks = random_tokens(rng, 3000)
    s = Stream().dynamic(toks, final=True, ll_lens=random_code(rng, 286, 15), d_lens=random_code(rng, 30, 15))
    out.append(_case("E_nlen286_ndist30", "E", s, tags={"E:full_sets"}))
    # HCLEN = 5 is the smallest that can describe a code (4 names only 16, 17, 18 and 0: all lengths zero,
    # see the error family): 256 lit/len codes of 8 bits, no distance code
    ll = [8] * 255 + [0, 8]
    s = Stream().dynamic(_lits(b"hclen five"), final=True, ll_lens=ll, d_lens=[0], cl_lens=lens_over({0, 8}, 19),
                         cl_syms=plain_cl_syms(ll + [0]))
    out.append(_case("E_hclen5", "E", s, tags={"E:hclen_min"}))
    # HCLEN = 19: the last entry of the order (15) is used, by one 15-bit lit/len code pair
    ll = [0] * 257
    for sym, l in zip([65, 66, 67, 68, 69, 70, 71, 72, 73, 74, 75, 76, 77, 78, 79, 256], list(range(1, 15)) + [15, 15]):
        ll[sym] = l
    s = Stream().dynamic(_lits(b"ABCDEFGHIJKLMNOONM"), final=True, ll_lens=ll, d_lens=[0], cl_syms=rle_cl_syms(ll + [0]))
    out.append(_case("E_hclen19_len15", "E", s, tags={"E:hclen19"}))
    # code-length codes of 7 bits
    ll = lens_over({65, 66, 67, 68, 256, 257, 258, 259}, 260)  # eight 3-bit codes
    dl = [2, 2, 2, 2]
    cl = [0] * 19
    for sym, l in zip([0, 18, 17, 1, 4, 16, 3, 2], [1, 2, 3, 4, 5, 6, 7, 7]):  # the 7-bit ones (3, 2) are used
        cl[sym] = l
    syms = rle_cl_syms(ll + dl)
    assert {3, 2, 16} <= {sy for sy, _ in syms}
    s = Stream().dynamic(_lits(b"ABCD") + [("match", 3, 1), ("match", 4, 2), ("match", 5, 3), ("match", 3, 4)] + _lits(b"DCBA" * 4),
                         final=True, ll_lens=ll, d_lens=dl, cl_lens=cl, cl_syms=syms)
    out.append(_case("E_cl_codes_of_7_bits", "E", s, tags={"E:cl7"}))
    # repeat 16 of a non-zero length from the lit/len lengths into the distance lengths
    ll = [0] * 259
    ll[65], ll[66], ll[256], ll[257], ll[258] = 3, 3, 2, 2, 2
    dl = [2, 2, 2, 2]
    syms = rle_cl_syms(ll[:257]) + [(16, 3)]
    s = Stream().dynamic(_lits(b"ABBA") + [("match", 3, 1), ("match", 4, 2), ("match", 3, 3), ("match", 4, 4)]
                         + _lits(b"AB" * 8), final=True, ll_lens=ll, d_lens=dl, cl_syms=syms)
    out.append(_case("E_rep16_crosses_nlen", "E", s))
    # repeat 18 from the lit/len lengths into the distance lengths
    ll = [0] * 270
    ll[65], ll[256], ll[257] = 1, 2, 2
    dl = [0, 0, 0, 0, 1, 1]
    syms = rle_cl_syms(ll[:258]) + [(18, 5), (1, 0), (1, 0)]
    s = Stream().dynamic(_lits(b"AAAAAAAA") + [("match", 3, 5), ("match", 3, 8)] + _lits(b"A" * 16), final=True,
                         ll_lens=ll, d_lens=dl, cl_syms=syms)
    out.append(_case("E_rep18_crosses_nlen", "E", s))
    # repeat 16 directly after repeat 18 (it repeats the zero), after 17 and after 16; the maximal runs 6, 10, 138
    ll = [0] * 138 + [0] * 6 + [3, 3, 3, 3, 3, 3, 3] + [0] * 10 + [0] * 6 + [0] * 89 + [3]
    assert len(ll) == 257 and sum(1 for l in ll if l) == 8
    syms = [(18, 127), (16, 3), (3, 0), (16, 3), (17, 7), (16, 3), (18, 78), (3, 0)]
    s = Stream().dynamic(_lits(bytes(range(144, 151)) * 4), final=True, ll_lens=ll, d_lens=[0], cl_syms=syms + [(0, 0)])
    out.append(_case("E_rep16_after_rep18_max_runs", "E", s))
    # 258 spelled both ways
    s = Stream().fixed(_lits(b"xyz") + [("ll_sym", 284, 31), ("d_sym", 2, 0), ("match", 258, 3)] + TAIL, final=True)
    out.append(_case("E_len258_as_284_31_fixed", "E", s, tags={"E:284+31"}))
    toks = _lits(b"xyzw") + [("ll_sym", 284, 31), ("d_sym", 3, 0), ("match", 258, 4), ("ll_sym", 284, 30),
                             ("d_sym", 0, 0)] + TAIL
    s = Stream().dynamic(toks, final=True)
    out.append(_case("E_len258_as_284_31_dynamic", "E", s, tags={"E:284+31"}))
    return out


# 65505: the longest stored block a BGZF member can hold (BSIZE is 16 bits: a member is at most 65536 bytes,
# 26 of them header and trailer, 5 the block's own header), in place of the format's 65535
F_MAX_STORED = 65536 - 26 - 5
F_LENS = (0, 1, 2, 3, 4, 5, 255, 256, 257, 2047, 2048, 2049, F_MAX_STORED)


def family_f():
    """Block framing."""
    out = []
    for nine in range(8):  # block of 10 + 8a + 9b bits: the stored header starts at bit (2 + b) mod 8
        for n in (0, 1, 5, 300):
            s = Stream().fixed([]).fixed(_lits(b"ab") + _lits(bytes([200 + nine] * nine)))
            s.stored(_rand(nine * 400 + n, n)).fixed(_lits(b"end"), final=True)
            out.append(_case("F_align%d_len%d" % (s.stored_at[0][0], n), "F", s))
    for n in F_LENS:
        if n == F_MAX_STORED:
            s = Stream().stored(_rand(n, n), final=True)
        else:
            s = Stream().stored(_rand(n, n)).fixed(_lits(b"!"), final=(n != 3))
        if n == 3:
            s.stored(b"", final=True)
        out.append(_case("F_stored_len%d" % n, "F", s, tags={"F:len%d" % n}))
    for at in (256, 257, 255, 512, 1):
        seed = _rand(at, 40)
        toks = _lits(seed) + [("match", 258, 40)] * ((at - 40) // 258) + [("match", (at - 40) % 258, 7)] * ((at - 40) % 258 >= 3)
        if at == 1:
            toks = [("lit", 9)]
        s = Stream().fixed(toks).stored(_rand(at + 1, 700)).fixed([("match", 30, 700)], final=True)
        assert len(interpret(toks)) == at
        out.append(_case("F_stored_after_huffman_at%d" % at, "F", s, tags={"F:after%d" % (at % 256)}))
    s = Stream()
    for _ in range(50):
        s.fixed([])
    out.append(_case("F_50_empty_fixed_blocks", "F", s.fixed(_lits(b"data at last") + [("match", 20, 4)], final=True),
                     tags={"F:50empty"}))
    s = Stream().fixed(_lits(b"fixed one ")).stored(b"stored").fixed([("match", 12, 16)] + _lits(b" fixed two"), final=True)
    out.append(_case("F_fixed_stored_fixed", "F", s, tags={"F:fsf"}))
    s = Stream().dynamic(_lits(b"dynamic one ") + [("match", 9, 3)]).fixed(_lits(b"fixed") + [("match", 7, 20)])
    s.dynamic(_lits(b"owt cimanyd") + [("match", 30, 11)], final=True)
    out.append(_case("F_dynamic_fixed_dynamic", "F", s, tags={"F:dfd"}))
    return out


def family_g():
    """The member's end: the hand-over from the window to the scalar step at
    112 bits, and members that never see a window."""
    out = []
    body = _lits(b"GATTACA-") + [("match", 20, 8), ("lit", 200), ("match", 3, 1), ("match", 64, 30)] + _lits(b"end") \
        + [("match", 5, 2), ("lit", 201), ("lit", 65)]
    for n in range(25):  # alternately 8- and 9-bit literals in front: every byte and bit phase of the end
        pre = [("lit", 65 if j % 2 == 0 else 210) for j in range(n)]
        out.append(_case("G_pre%d" % n, "G", Stream().fixed(pre + body, final=True), tags={"G:pre%d" % n}))
    for k in range(39):
        c = _case("G_clen%d" % (2 + k), "G", Stream().fixed(_lits(b % 144 for b in _rand(900 + k, k)), final=True))
        assert len(c.raw) == 2 + k
        c.tags.add("G:clen%d" % len(c.raw))
        out.append(c)
    for nine in range(8):
        s = Stream().fixed(_lits(b % 144 for b in _rand(950 + nine, 30)) + _lits(bytes([150 + nine] * nine)), final=True)
        out.append(_case("G_eob_ends_at_bit%d" % (s.w.bitlen() % 8), "G", s, tags={"G:endbit%d" % (s.w.bitlen() % 8)}))
    order = np.random.default_rng(70).permutation(len(out))
    return [out[i] for i in order]


def family_h():
    """The CRC kernel: output sizes 0..520, each once, back to back."""
    return [_case("H_size%d" % n, "H", Stream().stored(_rand(2000 + n, n), final=True), tags={"H:%d" % n})
            for n in range(521)]


H_BAD = (1, 3, 256, 257, 520)  # members of family H whose one stored byte changes (size >= 1)


def h_bad_blob(k):
    """Family H's file with one stored byte of member k changed: the member's
    trailer no longer matches.  Returns (blob, members before it in the file)."""
    cs = family("H")
    m = bytearray(cs[k].member())
    m[18 + 5] ^= 0x40  # first byte of the stored data (18 header, 5 block header)
    return b"".join(c.member() for c in cs[:k]) + bytes(m) + b"".join(c.member() for c in cs[k + 1:]) + BGZF_EOF, k


T_BTYPE = "invalid block type"
T_STORED = "invalid stored block lengths"
T_HEADER = "invalid dynamic block header"
T_CODES = "invalid code lengths set"
T_SYMBOL = "invalid literal/length or distance code"
T_DIST = "invalid distance too far back"
T_OVERRUN = "more data than the member's ISIZE"
T_TRUNC = "truncated deflate data"
T_SIZE = "less data than the member's ISIZE"
# zlib's message -> the project's status text (msw_gfastq.cpp status_text)
ZLIB_TO_TEXT = {
    "invalid block type": T_BTYPE,
    "invalid stored block lengths": T_STORED,
    "invalid distance too far back": T_DIST,
    "too many length or distance symbols": T_HEADER,
    "invalid bit length repeat": T_HEADER,
    "invalid code lengths set": T_CODES,
    "invalid literal/lengths set": T_CODES,
    "invalid distances set": T_CODES,
    "invalid code -- missing end-of-block": T_CODES,
    "invalid literal/length code": T_SYMBOL,
    "invalid distance code": T_SYMBOL,
    "incomplete or truncated stream": T_TRUNC,
}
FILL = 40  # filler bytes after the offending token (>= 16; the all-zero code-length code reads 258 bits of them)


def family_err():
    """Streams zlib rejects, and valid streams under a wrong trailer.  Each
    comment names the line of msw_inflate.hip that rejects the stream."""
    out = []

    def err(name, s, zmsg, plain=None):
        toks = list(s.tokens)
        if plain is None:
            try:
                plain = interpret(toks)
            except ValueError:  # the offending match itself
                plain = interpret(toks[:-1])
        s.filler(FILL)
        out.append(Case("X_" + name, "X", s.raw(), plain, toks, kind="error", zlib_msg=zmsg, text=ZLIB_TO_TEXT[zmsg],
                        tags=set(s.tags) | {"X:" + name}, stream=s))

    head = _lits(b"some output first")
    # `if (btype == 3) err = GZ_E_BTYPE` in the block loop
    s = Stream().fixed(head)
    s.w.bits(0, 1), s.w.bits(3, 2)
    err("btype3", s, "invalid block type")
    # stored block: `if (len != (~nlen & 0xFFFFu)) err = GZ_E_STORED`
    err("stored_len_nlen", Stream().fixed(head).stored(b"abcdef", nlen=0x1234), "invalid stored block lengths",
        plain=bytes(t[1] for t in head))
    # dynamic header: `if (nlen > 286 || ndist > 30) err = GZ_E_HEADER`, before anything is stored
    for hlit in (30, 31):
        s = Stream().fixed(head).dynamic([], ll_lens=[0] * (257 + hlit), d_lens=[0], eob=False, cl_lens=[1, 1] + [0] * 17,
                                         cl_syms=[], check=False)
        err("hlit%d" % hlit, s, "too many length or distance symbols")
    for hdist in (30, 31):
        s = Stream().fixed(head).dynamic([], ll_lens=[0] * 257, d_lens=[0] * (hdist + 1), eob=False,
                                         cl_lens=[1, 1] + [0] * 17, cl_syms=[], check=False)
        err("hdist%d" % hdist, s, "too many length or distance symbols")
    # code-length loop: `if (idx == 0) err = GZ_E_HEADER` for symbol 16
    s = Stream().fixed(head).dynamic([], ll_lens=[0] * 257, d_lens=[0], eob=False, cl_syms=[(16, 0), (1, 0)], check=False)
    err("rep16_at_index0", s, "invalid bit length repeat")
    # `if (idx + rep > total) err = GZ_E_HEADER`: no length is stored past nlen + ndist = 258 (lens holds 320)
    z256 = [(18, 127), (18, 107)]
    for name, tail in (("rep16", [(1, 0), (16, 3)]), ("rep17", [(1, 0), (17, 0)]), ("rep18", [(1, 0), (18, 0)])):
        s = Stream().fixed(head).dynamic([], ll_lens=[0] * 257, d_lens=[0], eob=False, cl_syms=z256 + tail, check=False)
        err(name + "_past_total", s, "invalid bit length repeat")
    # code-length code: build_code(kind 0) `if (left < 0) return false` / `if (left > 0 && (kind == 0 || ...`
    # -> `err = GZ_E_CODES` at its call
    hdr = dict(ll_lens=[0] * 257, d_lens=[0], eob=False, cl_syms=[], check=False)
    err("cl_oversubscribed", Stream().fixed(head).dynamic([], cl_lens=[1, 1, 1] + [0] * 16, **hdr), "invalid code lengths set")
    err("cl_incomplete", Stream().fixed(head).dynamic([], cl_lens=[1] + [0] * 18, **hdr), "invalid code lengths set")
    # all zero: build_code returns true with lim = 0, the first decode_sym finds no code: `if (sym < 0) err =
    # GZ_E_CODES`; zlib reads a zero length from every bit and then misses the end-of-block code
    err("cl_all_zero", Stream().fixed(head).dynamic([], cl_lens=[0] * 19, hclen=7, **hdr),
        "invalid code -- missing end-of-block")
    # HCLEN = 4 can name only 16, 17, 18 and 0, so every length is zero: `lens[256] == 0` -> GZ_E_CODES
    s = Stream().fixed(head).dynamic([], ll_lens=[0] * 257, d_lens=[0], eob=False, cl_lens=lens_over({0, 18}, 19),
                                     cl_syms=z256 + [(0, 0), (0, 0)])
    assert "hclen4" in s.tags
    err("hclen4_all_lengths_zero", s, "invalid code -- missing end-of-block")
    # `if (lens[256] == 0) err = GZ_E_CODES`
    ll = [1, 1] + [0] * 255
    err("no_end_of_block_code", Stream().fixed(head).dynamic([], ll_lens=ll, d_lens=[0], eob=False),
        "invalid code -- missing end-of-block")
    # build_code(kind 1) false -> GZ_E_CODES
    ll = [1, 1] + [0] * 254 + [1]
    err("ll_oversubscribed", Stream().fixed(head).dynamic([], ll_lens=ll, d_lens=[0], eob=False), "invalid literal/lengths set")
    ll = [2] + [0] * 255 + [2]
    err("ll_incomplete", Stream().fixed(head).dynamic([], ll_lens=ll, d_lens=[0], eob=False), "invalid literal/lengths set")
    # build_code(kind 2) false -> GZ_E_CODES
    ll = [1] + [0] * 255 + [1]
    err("d_oversubscribed", Stream().fixed(head).dynamic([], ll_lens=ll, d_lens=[1, 1, 1], eob=False), "invalid distances set")
    err("d_incomplete_one_2bit", Stream().fixed(head).dynamic([], ll_lens=ll, d_lens=[2], eob=False), "invalid distances set")
    # fixed 286 / 287: build_fast gives kFastLong, slow_ll `if (sym > 285) return kFastBadE` -> GZ_E_SYMBOL
    for sym in (286, 287):
        err("fixed_ll%d" % sym, Stream().fixed(head + [("ll_sym", sym, 0)], eob=False), "invalid literal/length code")
    # fixed distance 30 / 31: build_fast keeps kFastDLong for d > 29, the scalar step `if (d > 29) bad = GZ_E_SYMBOL`
    # (dbase = ~0, so `dist > opos` holds and nothing is copied)
    for sym in (30, 31):
        err("fixed_dist%d" % sym, Stream().fixed(head + [("ll_sym", 257, 0), ("d_sym", sym, 0)], eob=False),
            "invalid distance code")
    # the unused half of a 1-bit distance code: lim_d covers only the first bit 0, the ballot is empty, d = 31
    ll = lens_over({97, 256, 257}, 258)
    s = Stream().dynamic(_lits(b"aaaa") + [("match", 3, 1), ("ll_sym", 257, 0), ("bits", 1, 1)], ll_lens=ll, d_lens=[1],
                         eob=False)
    err("unused_half_of_1bit_distance_code", s, "invalid distance code")
    # a length code under an empty distance set: lim_d = 0, the same path
    s = Stream().dynamic(_lits(b"aaaa") + [("ll_sym", 257, 0), ("bits", 0, 1)], ll_lens=ll, d_lens=[0], eob=False)
    err("length_code_without_distance_codes", s, "invalid distance code")
    # dist == opos + 1: the window's `dist <= opos` fails, the scalar step `if (dist > opos) bad = GZ_E_DIST`
    for opos in (0, 1, 63, 64, 2048, 32767):
        s = Stream()
        pre = _rand(4000 + opos, opos)
        if opos > 64:
            s.stored(pre).fixed([("match", 3, opos + 1)], eob=False)
        else:
            s.fixed(_lits(pre) + [("match", 3, opos + 1)], eob=False)
        err("dist_opos_plus_1_at%d" % opos, s, "invalid distance too far back", plain=pre)
    # a stored block whose LEN runs past the member: `if (p + rest > mem.coff + mem.clen) err = GZ_E_TRUNC`;
    # ISIZE is what LEN promises, so that the earlier `opos + len > isize` is not the diagnosis
    s = Stream().fixed(head).stored(b"x" * 100, final=True)
    data = interpret(s.tokens)
    out.append(Case("X_stored_len_past_member", "X", s.raw()[:-30], data, s.tokens, kind="error",
                    zlib_msg="incomplete or truncated stream", text=T_TRUNC, tags={"X:stored_len_past_member"}))

    # valid deflate, wrong ISIZE: output N under ISIZE N - x / N + 1
    def trailer(name, s, isize, text):
        data = interpret(s.tokens)
        out.append(Case("X_" + name, "X", s.raw(), data, s.tokens, kind="trailer", text=text, isize=isize,
                        crc=zlib.crc32(data[:isize]) & 0xFFFFFFFF, tags={"X:" + name}, stream=s))

    big = _lits(_rand(88, 50)) + [("match", 258, 50)] * 15 + _lits(b"z" * 80)  # 4000 bytes
    assert len(interpret(big)) == 4000
    for x in (1, 255, 256, 257, 3000):
        # `if (opos > isize) bad = GZ_E_OVERRUN` where a chunk would be flushed (window, walk and scalar step),
        # or `if (opos > isize) err = GZ_E_OVERRUN` at the member's end
        trailer("isize_plus%d" % x, Stream().fixed(big, final=True), 4000 - x, T_OVERRUN)
    # stored block: `if (opos + len > isize) err = GZ_E_OVERRUN` before a byte is copied
    trailer("isize_plus1_stored", Stream().stored(_rand(89, 600), final=True), 599, T_OVERRUN)
    # `else if (opos != isize) err = GZ_E_SIZE`
    trailer("isize_minus1", Stream().fixed(big, final=True), 4001, T_SIZE)
    # no deflate data at all: the block loop reads the trailer as a block header; whatever that decodes to,
    # the member's end finds the bit position past clen (`err = GZ_E_TRUNC`).  Any error will do.
    out.append(Case("X_clen0", "X", b"", b"", [], kind="clen0", tags={"X:clen0"}))
    return out


_FAMILIES = dict(A=family_a, W=family_w, B=family_b, C=family_c, D=family_d, E=family_e, F=family_f, G=family_g, H=family_h,
                 X=family_err)
VALID_FAMILIES = "AWBCDEFGH"


@functools.lru_cache(maxsize=None)
def family(f):
    return tuple(_FAMILIES[f]())


def cases():
    """The whole corpus, valid families first, then the error cases."""
    return [c for f in _FAMILIES for c in family(f)]


def blob_of(cs):
    """Members back to back, then the BGZF EOF block, and the bytes they stand for."""
    return b"".join(c.member() for c in cs) + BGZF_EOF, b"".join(c.plain for c in cs)


def error_blob(c):
    """The bad member behind one to three valid ones (and one after it), and its index."""
    front = family("H")[5:5 + 1 + family("X").index(c) % 3]
    return blob_of(list(front) + [c] + [family("H")[9]])[0], len(front)
