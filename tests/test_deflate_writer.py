"""tests/deflate_writer.py against zlib, on the CPU: every hand-built stream
of the corpus that tests/test_gpu_inflate_streams.py feeds to msw_inflate.hip
means what its token list says (zlib inflates it to the interpreter's bytes,
or rejects it with the stated message), and the corpus holds every edge it is
there for -- a corpus that silently loses one fails here, without a GPU."""
import gzip
import zlib

import numpy as np
import pytest

import deflate_writer as dw

CLASSES = {"overlap", "near", "far", "reaches_start", "crosses_flush", "crosses_ring_wrap"}


def test_bit_writer_and_canonical_codes():
    w = dw.BitWriter()
    w.bits(0b101, 3)       # LSB first
    w.code(0b110, 3)       # MSB first: 1, 1, 0 -> stream bits 3, 4, 5
    assert w.bitlen() == 6 and w.getvalue() == bytes([0b011101])
    # RFC 1951 3.2.2's example: lengths (3, 3, 3, 3, 3, 2, 4, 4) -> 010 011 100 101 110 00 1110 1111
    assert dw.canon_codes([3, 3, 3, 3, 3, 2, 4, 4]) == [(2, 3), (3, 3), (4, 3), (5, 3), (6, 3), (0, 2), (14, 4), (15, 4)]
    assert dw.canon_codes([1, 0, 1, 1])[1] is None  # over-subscribed lists still get codes
    assert [dw.len_sym(n) for n in (3, 10, 11, 257, 258)] == [(257, 0), (264, 0), (265, 0), (284, 30), (285, 0)]
    assert [dw.dist_sym(n) for n in (1, 4, 5, 24577, 32768)] == [(0, 0), (3, 0), (4, 0), (29, 0), (29, 8191)]


def test_random_code_is_complete_and_bounded():
    rng = np.random.default_rng(1)
    for n, top in ((2, 1), (19, 7), (30, 15), (286, 15), (286, 9), (512, 9)):
        lens = dw.random_code(rng, n, top)
        assert len(lens) == n and 1 <= min(lens) and max(lens) <= top
        assert sum(2.0 ** -l for l in lens) == 1.0


def test_writer_round_trips_zlibs_own_streams():
    """The interpreter and the encoder on ordinary data: tokens from a simple
    greedy matcher, written with every block type, inflate (zlib) to the input."""
    data = (b"GATTACA" * 40 + bytes(range(256)) + b"A" * 600) * 3
    toks, i = [], 0
    while i < len(data):
        j = data.rfind(data[i:i + 3], max(0, i - 300), i + 2) if i + 3 <= len(data) else -1
        if j >= 0 and j < i:
            n = 3
            while n < 258 and i + n < len(data) and data[j + n] == data[i + n]:
                n += 1
            toks.append(("match", n, i - j))
            i += n
        else:
            toks.append(("lit", data[i]))
            i += 1
    assert dw.interpret(toks) == data and any(t[0] == "match" for t in toks)
    half = len(toks) // 2
    a, b = dw.auto_lens(toks[half:] + [("eob",)])
    s = dw.Stream().fixed(toks[:half]).stored(b"").dynamic(toks[half:], ll_lens=a, d_lens=b, cl_syms=dw.rle_cl_syms(a + b))
    s.stored(b"tail", final=True)
    assert zlib.decompress(s.raw(), -15) == data + b"tail" == dw.interpret(s.tokens)
    m = dw.bgzf_member(s.raw(), data + b"tail")
    assert gzip.decompress(m + dw.BGZF_EOF) == data + b"tail"


@pytest.mark.parametrize("fam", list(dw.VALID_FAMILIES))
def test_valid_cases_equal_zlib(fam):
    cs = dw.family(fam)
    assert cs and all(c.kind == "valid" for c in cs)
    assert len({c.name for c in cs}) == len(cs)
    for c in cs:
        d = zlib.decompressobj(-15)
        got = d.decompress(c.raw)
        assert got == dw.interpret(c.tokens) == c.plain, c.name
        assert d.unused_data == b"" and d.eof, c.name
        assert len(c.plain) <= 65536 and c.isize is None and c.crc is None, c.name
    blob, plain = dw.blob_of(cs)
    assert gzip.decompress(blob) == plain


def test_error_cases_are_rejected_by_zlib_with_their_message():
    cs = dw.family("X")
    assert len({c.name for c in cs}) == len(cs)
    for c in cs:
        if c.kind == "error":
            assert dw.ZLIB_TO_TEXT[c.zlib_msg] == c.text, c.name
            with pytest.raises(zlib.error) as e:
                if c.zlib_msg == "incomplete or truncated stream":
                    zlib.decompress(c.raw, -15)  # a decompressobj waits for more input instead
                else:
                    zlib.decompressobj(-15).decompress(c.raw)
            assert str(e.value).endswith(c.zlib_msg), (c.name, str(e.value))
            # what zlib made before the error begins the trailer's bytes (the call that fails keeps its own
            # last bytes, so zlib can show a prefix only; the interpreter has them all)
            if c.zlib_msg != "incomplete or truncated stream":
                d = zlib.decompressobj(-15)
                got = b""
                try:  # one output byte per call, or the bytes of the failing call are lost with it
                    got += d.decompress(c.raw, 1)
                    while d.unconsumed_tail:
                        got += d.decompress(d.unconsumed_tail, 1)
                except zlib.error:
                    pass
                assert c.plain.startswith(got) and len(got) >= len(c.plain) - 8, c.name
                assert dw.FILL >= 16 and c.raw.endswith(b"\0" * dw.FILL), c.name
        elif c.kind == "trailer":  # zlib has no ISIZE: the stream is valid, the trailer is not
            d = zlib.decompressobj(-15)
            assert d.decompress(c.raw) == c.plain and d.eof and d.unused_data == b"", c.name
            assert c.isize != len(c.plain) and c.text in (dw.T_OVERRUN, dw.T_SIZE), c.name
            assert (c.text == dw.T_OVERRUN) == (len(c.plain) > c.isize), c.name
            with pytest.raises(gzip.BadGzipFile):
                gzip.decompress(c.member())
        else:
            assert c.kind == "clen0" and c.raw == b"" and len(c.member()) == 26


def test_crc_cases_change_one_member():
    for k in dw.H_BAD:
        blob, idx = dw.h_bad_blob(k)
        good = dw.blob_of(dw.family("H"))[0]
        assert idx == k and len(blob) == len(good) and sum(a != b for a, b in zip(blob, good)) == 1
        with pytest.raises(gzip.BadGzipFile, match="CRC check failed"):
            gzip.decompress(blob)


def _tags(fam):
    return set().union(*(c.tags for c in dw.family(fam)))


def _the_match(c, at):
    """The one match of case c that starts at output position `at`."""
    m = [x for x in dw.classify(c.tokens) if x[0] == at]
    assert len(m) == 1, c.name
    return m[0]


def test_classify_on_known_matches():
    toks = dw._lits(bytes(300)) + [("match", 5, 300), ("match", 258, 1), ("match", 3, 2046), ("match", 3, 2045)]
    pre = ("stored", bytes(2048 - 300 - 5 - 258))
    got = dw.classify([pre] + toks)
    assert [g[:3] for g in got] == [(2048 - 263, 5, 300), (2048 - 258, 258, 1), (2048, 3, 2046), (2051, 3, 2045)]
    assert got[0][3] == {"near"}
    assert got[1][3] == {"near", "overlap", "crosses_flush"}
    assert got[2][3] == {"far"}                               # 2046 + 3 > 2048
    assert dw.classify([("stored", bytes(2047)), ("match", 3, 10)])[0][3] == {"near", "crosses_flush", "crosses_ring_wrap"}
    assert dw.classify([("stored", bytes(2058)), ("match", 20, 20)])[0][3] == {"near", "crosses_ring_wrap"}  # its source
    assert got[3][3] == {"near"}
    assert dw.classify(dw._lits(b"ab") + [("match", 3, 2)])[0][3] == {"near", "overlap", "reaches_start"}
    assert "far" in dw.classify([pre] + toks, ring=256)[0][3]


def test_corpus_covers_every_class_and_listed_edge():
    seen = {f: set() for f in dw.VALID_FAMILIES}
    for f in dw.VALID_FAMILIES:
        for c in dw.family(f):
            for *_, cl in dw.classify(c.tokens):
                seen[f] |= cl
    assert set().union(*seen.values()) == CLASSES
    assert seen["D"] == CLASSES and seen["B"] >= {"near", "far", "overlap", "crosses_flush", "crosses_ring_wrap"}

    # A: every (d, len, k), the match where the sweep says, overlapping exactly when d < len
    a = {c.name: c for c in dw.family("A")}
    assert len(a) == 66 * 6 * 4
    for d in range(1, 67):
        for n in (3, 4, 63, 64, 65, 258):
            for k in range(4):
                opos, length, dist, cl = _the_match(a["A_d%d_len%d_k%d" % (d, n, k)], d + k)
                assert (length, dist) == (n, d) and ("overlap" in cl) == (d < n) and "near" in cl

    # B: every match at every position in every placement; near exactly when d + len <= 2048
    b = {c.name: c for c in dw.family("B")}
    ms = dw.b_matches()
    for n in (3, 64, 258):
        assert {d + n for d, ln in ms if ln == n} >= {2047, 2048, 2049}
    assert {d for d, ln in ms if ln == 3} >= set(range(2046, 2051))
    assert {d for d, _ in ms} >= {190, 255, 256, 257, 330}
    assert {p % 256 for p in dw.B_POS} == {0, 1, 255} and {p % 2048 for p in dw.B_POS} >= {0, 1, 2047}
    assert len(b) == len(ms) * len(dw.B_POS) * len(dw.B_PLACES)
    for d, n in ms:
        for pos in dw.B_POS:
            for place in dw.B_PLACES:
                c = b["B_d%d_len%d_at%d_%s" % (d, n, pos, place)]
                opos, length, dist, cl = _the_match(c, pos)
                assert (length, dist) == (n, d) and ("near" in cl) == (d + n <= 2048), c.name

    # C: far distances at opos = d and d + 1, byte 0 reached from 1..70, all output offsets mod 4, a full member
    c_all = dw.family("C")
    t = _tags("C")
    assert t >= {"C:far:%d:%d:%d" % (d, o, n) for d in (4096, 16384, 32767, 32768) for o in (0, 1) for n in (3, 258)}
    assert t >= {"C:start:%d" % o for o in range(1, 71)} | {"C:tiny1", "C:tiny2", "C:tiny3", "C:full"}
    ooff, far_off, start_off = 0, set(), set()
    for c in c_all:
        for opos, length, dist, cl in dw.classify(c.tokens):
            if "C:far" in "".join(c.tags):
                assert "far" in cl and dist >= 4096 and opos - dist in (0, 1), c.name
                far_off.add(ooff % 4)
            if "C:start" in "".join(c.tags):
                assert "reaches_start" in cl and dist == opos <= 70, c.name
                start_off.add(ooff % 4)
        ooff += len(c.plain)
    assert far_off == start_off == {0, 1, 2, 3}
    assert max(len(c.plain) for c in c_all) == 65536

    # D: three encodings per stream; the long codes are really written
    d_all = dw.family("D")
    assert len(d_all) == 450 and max(len(c.plain) for c in d_all) <= 65536
    assert sorted(len(c.plain) for c in d_all)[len(d_all) // 2] < 8192
    lc = [c for c in d_all if c.name.endswith("_longcodes")]
    assert len(lc) == 150 and all(c.stream.ll_code_bits > 9 and c.stream.d_code_bits > 7 for c in lc)
    sp = [c for c in d_all if c.name.endswith("_split")]
    assert sum(1 for c in sp for t in c.tokens if t[0] == "stored") > 150
    assert {"nlen286", "ndist30"} <= _tags("D")

    # E: the header forms
    assert _tags("E") >= {"E:eob_only", "E:eob_only_between", "E:no_dist", "E:one_dist", "E:full_sets", "E:hclen_min",
                          "E:hclen19", "E:cl7", "E:284+31", "hclen5", "hclen19", "cl_maxlen7", "nlen286", "ndist30",
                          "ndist1", "rep16_crosses_nlen", "rep16_nonzero_crosses_nlen", "rep18_crosses_nlen",
                          "rep16_after_rep18", "max_rep16", "max_rep17", "max_rep18"}
    e = {c.name: c for c in dw.family("E")}
    assert e["E_eob_only_empty_member"].plain == b"" and len(e["E_len258_as_284_31_fixed"].plain) == 3 + 258 + 258 + 16
    assert ("ll_sym", 284, 31) in e["E_len258_as_284_31_fixed"].tokens
    assert ("match", 258, 3) in e["E_len258_as_284_31_fixed"].tokens

    # F: block framing
    f_all = dw.family("F")
    st = [x for c in f_all for x in c.stream.stored_at]
    assert {a for a, _, _ in st} == set(range(8))
    assert {n for _, n, _ in st} >= set(dw.F_LENS)
    assert {o % 256 for c in f_all if "F:after" in "".join(c.tags) for _, _, o in c.stream.stored_at} >= {0, 1, 255}
    assert _tags("F") >= {"F:50empty", "F:fsf", "F:dfd"}

    # G: the member's end at every byte and bit phase, every coff mod 4
    g_all = dw.family("G")
    assert _tags("G") >= {"G:pre%d" % n for n in range(25)} | {"G:clen%d" % n for n in range(2, 41)} \
        | {"G:endbit%d" % n for n in range(8)}
    coff, seen_c, seen_e = 0, set(), set()
    pre_bits = set()
    for c in g_all:
        coff += 18
        seen_c.add(coff % 4)
        seen_e.add((coff + len(c.raw)) % 4)
        if "G:pre" in "".join(c.tags):
            pre_bits.add((c.stream.w.bitlen() % 8, (coff + len(c.raw)) % 4))
        coff += len(c.raw) + 8
    assert seen_c == seen_e == {0, 1, 2, 3} and len(pre_bits) >= 16
    assert min(len(c.raw) for c in g_all if "G:pre" in "".join(c.tags)) * 8 > 112  # the window runs, then hands over

    # H: every size 0..520 once
    assert [len(c.plain) for c in dw.family("H")] == list(range(521))

    # the error cases of the issue, by name
    x = {c.name[2:] for c in dw.family("X")}
    assert x >= {"btype3", "stored_len_nlen", "hlit30", "hlit31", "hdist30", "hdist31", "rep16_at_index0",
                 "rep16_past_total", "rep17_past_total", "rep18_past_total", "cl_oversubscribed", "cl_incomplete",
                 "cl_all_zero", "hclen4_all_lengths_zero", "no_end_of_block_code", "ll_oversubscribed", "ll_incomplete",
                 "d_oversubscribed", "d_incomplete_one_2bit", "fixed_ll286", "fixed_ll287", "fixed_dist30",
                 "fixed_dist31", "unused_half_of_1bit_distance_code", "length_code_without_distance_codes",
                 "stored_len_past_member", "isize_minus1", "isize_plus1_stored", "clen0"} \
        | {"dist_opos_plus_1_at%d" % o for o in (0, 1, 63, 64, 2048, 32767)} \
        | {"isize_plus%d" % n for n in (1, 255, 256, 257, 3000)}
    texts = {c.text for c in dw.family("X")}
    assert texts >= {dw.T_BTYPE, dw.T_STORED, dw.T_HEADER, dw.T_CODES, dw.T_SYMBOL, dw.T_DIST, dw.T_OVERRUN,
                     dw.T_TRUNC, dw.T_SIZE}
    assert {c.zlib_msg for c in dw.family("X") if c.kind == "error"} == set(dw.ZLIB_TO_TEXT)
    # the bad member sits behind one to three valid ones
    assert {dw.error_blob(c)[1] for c in dw.family("X")} == {1, 2, 3}


def _paths(c, coff):
    return {(opos, n, d): (path, lane) for path, opos, n, d, lane in dw.window_paths(c.stream, coff)}


def test_window_model_on_known_streams():
    """window_paths on streams small enough to follow by hand (fixed code:
    literals below 144 take 8 bits, a length-3 match at distance 1 7 + 5)."""
    s = dw.Stream().fixed(dw._lits(b"abcd")).fixed([("match", 3, 1)]).fixed(dw.TAIL + dw.TAIL, final=True)
    assert dw.window_paths(s) == [("window", 4, 3, 1, 0)]
    # literals of the match's own window in front: dist > opos at the window's start -> the scalar step
    s = dw.Stream().fixed(dw._lits(b"abcd") + [("match", 3, 4)] + dw.TAIL + dw.TAIL, final=True)
    assert dw.window_paths(s) == [("scalar", 4, 3, 4, None)]
    # the same match behind two literals of its window, and with more than 64 bytes in the window
    s = dw.Stream().fixed(dw._lits(b"abcd")).fixed(dw._lits(b"ef") + [("match", 3, 4)]).fixed(dw.TAIL + dw.TAIL, final=True)
    assert dw.window_paths(s) == [("window", 6, 3, 4, 2)]
    s = dw.Stream().fixed(dw._lits(b"abcd")).fixed([("match", 60, 4)] + dw._lits(b"efghi")).fixed(dw.TAIL + dw.TAIL, final=True)
    assert dw.window_paths(s) == [("walk", 4, 60, 4, None)]
    # the member's last 112 bits: no window, at any alignment of the data
    s = dw.Stream().fixed(dw._lits(b"abcd")).fixed([("match", 3, 1)], final=True)
    assert all(dw.window_paths(s, coff) == [("scalar", 4, 3, 1, None)] for coff in range(4))
    # 112 bits left in the kernel's dword arithmetic: 14 bytes after the token decide with coff
    s = dw.Stream().fixed(dw._lits(b"abcd")).fixed([("match", 3, 1)]).fixed(dw._lits(b"0123456789"), final=True)
    assert {dw.window_paths(s, coff)[0][0] for coff in range(4)} == {"window", "scalar"}
    # codes beyond the fast tables are not simple
    ll = [0] * 258
    for sym, n in zip([65, 66, 67, 68, 69, 70, 71, 72, 73, 256, 257], [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 10]):
        ll[sym] = n
    s = dw.Stream().fixed(dw._lits(b"abcd")).dynamic([("lit", 65), ("match", 3, 1)], ll_lens=ll, d_lens=[1, 1])
    s.fixed(dw.TAIL + dw.TAIL, final=True)
    assert dw.window_paths(s) == [("scalar", 5, 3, 1, None)]


def test_corpus_matches_take_the_decode_path_they_are_there_for():
    """The model of the kernel's token loop (dw.window_paths) on the families
    whose point is a decode path, at all four alignments of the deflate data:
    W reaches the lane-parallel emission with every (d, off) of the window's
    off mod d multiply, A and B reach the paths their docstrings name."""
    for coff in range(4):
        # W: the match is emitted by the lanes, p lanes in; off = 0..63 for every d in 1..66
        offs = {d: set() for d in range(1, 67)}
        lanes = {d: set() for d in range(1, 67)}
        for c in dw.family("W"):
            d, p, n = (int(x) for x in c.name[3:].replace("p", "").replace("len", "").split("_"))
            assert dw.window_paths(c.stream, coff) == [("window", d + 3 + p, n, d, p)], c.name
            offs[d] |= set(range(n))
            lanes[d].add(p)
        assert all(offs[d] == set(range(64)) and lanes[d] == {0, 1, 2, 3} for d in offs)
        # A: k lanes into its window; lengths 3 and 4 by the lanes, the longer ones by the serial walk
        for c in dw.family("A"):
            d, n, k = (int(x) for x in c.name[3:].replace("len", "").replace("k", "").split("_"))
            want = ("window", k) if n <= 4 else ("walk", None)
            assert _paths(c, coff) == {(d + k, n, d): want}, c.name
        # B: each placement's path
        for c in dw.family("B"):
            d, n, pos, place = c.name[3:].replace("len", "").replace("at", "").split("_")
            d, n, pos = int(d), int(n), int(pos)
            got = _paths(c, coff)
            path = dw.b_path(place, n)
            assert got[(pos, n, d)] == (path, (2 if place == "after2" else 0) if path == "window" else None), c.name
            if place == "walk":
                assert got[(pos - 258, 258, 500)] == ("walk", None), c.name
        assert {dw.b_path(p, n) for p in dw.B_PLACES for _, n in dw.b_matches()} == {"window", "walk", "scalar"}
    # the ring and far edges are reached on every path that can hold them
    for path in ("window", "walk", "scalar"):
        sums = {d + n for d, n in dw.b_matches() for p in dw.B_PLACES if dw.b_path(p, n) == path}
        assert sums >= {2047, 2048, 2049, 2050, 2051, 2052, 2053}, path
