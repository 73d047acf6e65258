"""BGZF deflate on the GPU (msw_deflate.hip) against zlib: every member is
parsed by hand (magic, 'BC' field, BSIZE, ISIZE, CRC-32) and its payload
inflated with zlib; the inputs are the smallest at which a part of the kernel
can go wrong (window, block and distance edges, the 15-bit length limit, the
single-symbol and empty distance alphabets, the stored fallback)."""
import ctypes
import functools
import struct
import zlib

import numpy as np
import pytest

from mini_parallel_amd import bgzf_deflate, bgzf_inflate
from mini_parallel_amd import synthetic as syn
from mini_parallel_amd._lib import MSW_E_INVALID, MSW_E_RANGE, lib

pytestmark = pytest.mark.gpu

BLOCK = 65280
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
LENGTHS = (0, 1, 3, 4, 5, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1)


def members(blob):
    """[(member size, inflated payload, payload size)] of a BGZF file, each member checked."""
    out, p = [], 0
    while p < len(blob):
        assert blob[p:p + 4] == b"\x1f\x8b\x08\x04" and blob[p + 10:p + 16] == b"\x06\x00BC\x02\x00"
        size = struct.unpack_from("<H", blob, p + 16)[0] + 1
        assert 26 <= size <= 65536 and p + size <= len(blob)
        crc, isize = struct.unpack_from("<II", blob, p + size - 8)
        d = zlib.decompressobj(-15)
        plain = d.decompress(blob[p + 18:p + size - 8])
        assert d.eof and not d.unused_data
        assert len(plain) == isize <= BLOCK and zlib.crc32(plain) == crc
        out.append((size, plain, size - 26))
        p += size
    return out


def text(n, seed=7):
    rng = np.random.default_rng(seed)
    words = [bytes(rng.integers(97, 123, int(k)).astype(np.uint8)) for k in rng.integers(2, 9, 300)]
    s = b" ".join(words[i] for i in rng.integers(0, 300, n // 3 + 2))
    return s[:n]


def planted(gap, quiet=False):
    """Random bytes with a 200-byte motif whose second copy starts gap bytes after the first; quiet: zeros
    around the two copies, which leave the first copy's entries in a hashed table alone."""
    a = np.random.default_rng(200).integers(0, 256, BLOCK).astype(np.uint8)
    if quiet:
        a[200:] = 0
    a[gap:gap + 200] = a[:200]
    return a.tobytes()


def skewed():
    fib = [1, 1]
    while len(fib) < 22:
        fib.append(fib[-1] + fib[-2])
    a = np.repeat(np.arange(22, dtype=np.uint8) + 65, fib)
    return np.random.default_rng(22).permutation(a).tobytes()


def distinct_4grams():
    """Every 4-gram once: a counter in base 251 with a fixed byte 255 in front of each digit group."""
    k = np.arange(3000)
    return np.stack([np.full(3000, 255), k % 251, k // 251, np.full(3000, 254)], 1).astype(np.uint8).tobytes()


@functools.lru_cache(None)
def fastq(qual):
    """~1 MB of FASTQ text: 1,200 lane reads of 400 bases."""
    g = syn.wgs_genome()
    b, pos, rng = syn._lane_reads(g, 0, 1200, 400, 2.0, 1004)
    return syn._lane_records(b, pos, rng, b"SYN", 1, qual)


CASES = {f"len{n}": lambda n=n: text(n) for n in LENGTHS}
CASES.update({
    "equal": lambda: b"a" * 70000,
    "period2": lambda: b"ab" * 35000,
    "period3": lambda: b"abc" * 23334,
    "period259": lambda: bytes(np.random.default_rng(259).integers(0, 256, 259).astype(np.uint8)) * 271,
    "motif200": lambda: planted(200), "motif32767": lambda: planted(32767), "motif32768": lambda: planted(32768),
    "motif32769": lambda: planted(32769),
    # the same between zeros: no stored form, and nothing evicts the first copy, so a taken copy shows in the size
    "near32767": lambda: planted(32767, True), "near32768": lambda: planted(32768, True),
    "random": lambda: np.random.default_rng(5).integers(0, 256, BLOCK).astype(np.uint8).tobytes(),
    "skewed": skewed,
    "one_literal": lambda: b"z" * 5000,
    "no_match": distinct_4grams,
    "fastq_illumina": lambda: fastq("illumina"), "fastq_binned": lambda: fastq("binned"),
})


@pytest.mark.parametrize("name,eof", [(n, True) for n in CASES] + [(n, False) for n in CASES if n.startswith("len")])
def test_deflate_against_zlib(gpu_ctx, name, eof):
    data = CASES[name]()
    blob = bgzf_deflate(gpu_ctx, data, eof=eof)
    if eof:
        assert blob.endswith(EOF)
        blob = blob[:-len(EOF)]
    ms = members(blob)
    assert b"".join(m[1] for m in ms) == data
    assert [len(m[1]) for m in ms] == [min(BLOCK, len(data) - k) for k in range(0, len(data), BLOCK)]
    if name == "equal":
        assert ms[0][0] <= 1024  # 254 tokens of <= 30 bits, plus the header
    if name == "random":
        assert ms[0][0] <= 65311  # the stored form
    if name.startswith("near"):
        # a copy 32,768 back or nearer is taken: 200 literals saved against the copy one too far, which
        # costs them at more than four bits each (over 100 distinct values)
        far = members(bgzf_deflate(gpu_ctx, planted(32769, True), eof=False))
        assert far[0][1] == planted(32769, True) and ms[0][0] <= far[0][0] - 100
    if name.startswith("fastq"):
        z = 0
        for k in range(0, len(data), BLOCK):
            c = zlib.compressobj(1, zlib.DEFLATED, -15)
            z += len(c.compress(data[k:k + BLOCK]) + c.flush())
        ratio = sum(m[2] for m in ms) / z
        print(f"{name}: {len(data)} bytes, payload / zlib level 1 = {ratio:.4f}")
        assert ratio <= 1.10


@pytest.mark.parametrize("n", LENGTHS)
def test_inflate_round_trip(gpu_ctx, n):
    x = text(n, seed=11)
    assert bgzf_inflate(gpu_ctx, bgzf_deflate(gpu_ctx, x)) == x


def test_deterministic(gpu_ctx):
    x = fastq("illumina")
    assert bgzf_deflate(gpu_ctx, x) == bgzf_deflate(gpu_ctx, x)


@pytest.mark.parametrize("short,flags,code", ((1, 0, MSW_E_RANGE), (0, 2, MSW_E_INVALID)))
def test_argument_errors(gpu_ctx, short, flags, code):
    src = np.frombuffer(text(1000), np.uint8)
    cap = lib().msw_bgzf_deflate_bound(len(src)) - short
    out = np.zeros(cap, np.uint8)
    n = ctypes.c_uint64()
    assert lib().msw_bgzf_deflate(gpu_ctx.handle, src.ctypes.data, len(src), out.ctypes.data, cap, ctypes.byref(n),
                                  flags) == code
