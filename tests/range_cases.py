"""Case generators shared by tests/test_gpu_wide.py and tests/test_gpu_ranges.py
(GPU) and checked on their own, against the oracle alone, by
tests/test_range_cases.py (CPU): reads of 257-384 bases on the packed
kernels' wide instances (KR 17..24), and batches that sit on the numeric
limits of the two cell domains (f16: H < 2048; u16: every value below 0x7C00).

Every batch is tiny -- a wave of the pairs layout holds 8 pairs at G = 16, so
9 pairs are one full wave and a second wave of one pair beside an empty slot.
A pair's window is random A/C/G/T and carries its read: an exact copy, a copy
with one substitution, a copy with one deletion, or a copy with a few
substitutions and one deletion.  Row padding past a read or window is random
A/C/G/T too, never zero: a kernel that scores a padding byte is caught."""
import dataclasses

import numpy as np

from mini_parallel_amd import Scoring

ACGT = np.frombuffer(b"ACGT", np.uint8)
KINDS = ("exact", "noisy", "sub", "del")

# the four scoring kinds of the packed kernels (linear / affine x score-only /
# best cell); THREE is the set the staging tests use
FOUR = {
    "linear": Scoring(),
    "linear+cell": Scoring(want_coords=True),
    "affine": Scoring(gap_open=3, gap_extend=1, affine=True),
    "affine+cell": Scoring(gap_open=3, gap_extend=1, affine=True, want_coords=True),
}
THREE = {k: FOUR[k] for k in ("linear", "linear+cell", "affine+cell")}


def with_scheme(scorings, **kw):
    """The same scoring kinds under another match / mismatch / gap scheme."""
    return {k: dataclasses.replace(sc, **kw) for k, sc in scorings.items()}


class Batch:
    def __init__(self, key, reads, read_len, wins, win_len, kinds):
        self.key = key  # names the batch (oracle results are shared by key)
        self.reads, self.read_len, self.wins, self.win_len = reads, read_len, wins, win_len
        self.kinds = list(kinds)
        self.n_pairs = int(reads.shape[0])

    @property
    def exact(self):
        """Pairs whose read is an exact substring of the window, or whose
        window is an exact substring of the read: score = match x min(m, n)."""
        return np.array([k == "exact" for k in self.kinds], bool)

    def copy(self, key):
        return Batch(key, self.reads.copy(), self.read_len.copy(), self.wins.copy(), self.win_len.copy(), self.kinds)


def other_base(b):
    """A different base for each of A/C/G/T (a substitution always mismatches)."""
    return ACGT[(np.searchsorted(ACGT, b) + 1) % 4]


def planted(key, read_lens, win_lens, read_stride, win_stride, seed, kinds=None, at_end=()):
    """One pair per entry of read_lens / win_lens.  kinds[i] (default: KINDS in
    rotation, so neighbouring pairs -- the two packed halves of a lane group
    -- always differ) says how read i derives from its window; a window
    shorter than the read is planted in the read instead (kind "exact": the
    whole window matches; any other kind becomes "sub", one substitution
    inside the planted copy).  The kinds as built are in the batch.  Pairs
    listed in at_end have their copy end at the window's last column (the
    score then depends on the window's last chunk), the others anywhere."""
    n = len(read_lens)
    kinds = list(kinds) if kinds is not None else [KINDS[i % len(KINDS)] for i in range(n)]
    rng = np.random.default_rng(seed)
    rl = np.asarray(read_lens, np.uint16)
    wl = np.asarray(win_lens, np.uint16)
    assert rl.max() <= read_stride and wl.max() <= win_stride and len(kinds) == n == len(wl)
    reads = ACGT[rng.integers(0, 4, (n, read_stride))]
    wins = ACGT[rng.integers(0, 4, (n, win_stride))]
    for i in range(n):
        m, w, kind = int(rl[i]), int(wl[i]), kinds[i]
        cut = kind in ("del", "noisy")
        need = m + (1 if cut else 0)
        if need > w:  # the whole window lies inside the read
            at = int(rng.integers(0, m - w + 1))
            reads[i, at:at + w] = wins[i, :w]
            if kind != "exact":  # one substitution inside the planted copy
                kinds[i] = "sub"
                reads[i, at + w // 3] = other_base(reads[i, at + w // 3])
            continue
        at = int(rng.integers(0, w - need + 1))
        if i in at_end:
            at = w - need
        r = wins[i, at:at + need].copy()
        if cut:
            r = np.delete(r, need // 2)
        if kind == "sub":
            r[m // 3] = other_base(r[m // 3])
        if kind == "noisy":
            hit = np.nonzero(rng.random(m) < 0.02)[0]
            r[hit] = other_base(r[hit])
        reads[i, :m] = r
    return Batch(key, reads, rl, wins, wl, kinds)


# ---------------------------------------------------------------------------
# A: reads of 257-384 bases (KR 17..24 at G = 16)
# ---------------------------------------------------------------------------
WIDE_KRS = list(range(17, 25))
WIDE_READ_STRIDE, WIDE_WIN_STRIDE = 384, 768


def kr_batch(kr, g=16, n=9):
    """Reads on the three edges of a rows-per-lane count: g (kr - 1) + 1,
    g kr - 1 and g kr bases, windows of 2m, strides of the longest shape."""
    lens = [g * (kr - 1) + 1, g * kr - 1, g * kr]
    rl = [lens[i % 3] for i in range(n)]
    return planted(("kr", kr, g, n), rl, [2 * m for m in rl], WIDE_READ_STRIDE, WIDE_WIN_STRIDE, seed=1000 + 31 * kr + g)


def fallback_batches():
    """17 pairs of 300 x 600 (three waves).  `inside`: an N in one window of
    the second wave and a lower-case base in the window of the third;
    `padded`: the same bytes (and more) only in the row padding past each
    window's end."""
    clean = planted("fb-clean", [300] * 17, [600] * 17, 304, 640, seed=2001)
    inside = clean.copy("fb-inside")
    inside.wins[11, 599] = ord("N")
    inside.wins[16, 0] = ord("a")
    padded = clean.copy("fb-padded")
    padded.wins[:, 600:] = np.resize(np.frombuffer(b"Nacgt\x00\xff", np.uint8), 40)
    return clean, inside, padded


ROUND_WIN_LENS = [511, 512, 513, 527, 528, 529, 767, 768, 1023, 1024, 1025, 4095, 4096, 1, 16, 255]


def round_batches():
    """Window lengths around the staging rounds (512 columns at G = 16), the
    16-byte chunk and the row's end, and windows shorter than the read; reads
    of 300 and 384 bases; and two batches whose every window is as long as its
    row (strides 768 and 4096): the last chunk of the last row ends at the
    buffer's last byte, in a later round.  There every read lies at its
    window's end, and so does every second one of the mixed batch."""
    n = 2 * len(ROUND_WIN_LENS)
    wl = [ROUND_WIN_LENS[i % len(ROUND_WIN_LENS)] for i in range(n)]
    rl = [(300, 384)[(i + i // len(ROUND_WIN_LENS)) % 2] for i in range(n)]
    mixed = planted("rounds-mixed", rl, wl, 384, 4096, seed=3001, at_end=range(0, n, 2))
    full768 = planted("rounds-768", [300, 384] * 4 + [384], [768] * 9, 384, 768, seed=3002, at_end=range(9))
    full4096 = planted("rounds-4096", [384, 300] * 4 + [300], [4096] * 9, 384, 4096, seed=3003, at_end=range(9))
    return mixed, full768, full4096


def bucket_edge_batch():
    """Lengths 241..384: three pairs on each edge of every rows-per-lane
    bucket from 16 to 24, shuffled; windows 2m."""
    rng = np.random.default_rng(4001)
    lens = [m for kr in range(16, 25) for m in (16 * (kr - 1) + 1, 16 * kr - 1, 16 * kr)] * 3
    rl = rng.permutation(np.array(lens))
    return planted("bucket-edges", rl, 2 * rl, WIDE_READ_STRIDE, WIDE_WIN_STRIDE, seed=4002)


def narrow_batch(max_m, g=13):
    """Reads on the rows-per-lane edges below max_m at G = g, the longest
    max_m itself."""
    kr = -(-max_m // g)
    lens = [g * (kr - 1) + 1, max_m - 1, max_m]
    rl = [lens[i % 3] for i in range(9)]
    return planted(("narrow", max_m, g), rl, [2 * m for m in rl], 320, 640, seed=5000 + max_m)


# ---------------------------------------------------------------------------
# B1: the f16 bound match (min(max_m, max_n) + 2) < 2048, from both sides
# ---------------------------------------------------------------------------
# (match, mismatch, L): L is the longest read the f16 domain takes under match
F16_EDGES = [(6, -4, 339), (7, -4, 290), (8, -4, 253), (10, -4, 202), (12, -4, 168), (16, -4, 125), (32, -4, 61),
             (64, 0, 29)]
F16_ALWAYS = (5, -4, 384)  # fits at every packed read length; tops out at 1920


def stride16(n):
    return -(-n // 16) * 16


def f16_edge_batch(match, length):
    """9 pairs of `length` x 2 `length`: exact copies (score match x length),
    single substitutions and single deletions, in rotation."""
    kinds = [("exact", "sub", "del")[i % 3] for i in range(9)]
    return planted(("f16", length), [length] * 9, [2 * length] * 9, stride16(length), stride16(2 * length),
                   seed=6000 + length, kinds=kinds)


def mirrored_batch(win):
    """Reads of 384 bases against windows of `win` < 384 planted in them: the
    window is the shorter side of the bound."""
    return planted(("mirror", win), [384] * 9, [win] * 9, 384, stride16(win), seed=6500 + win)


def top_gap_schemes(match, mismatch, length):
    """Affine penalties that matter at the top of the f16 range: a gap opened
    out of the best cell (match x length) stays positive by 10; and open +
    extend either side of the f16 domain's cap of 2047."""
    top = match * length
    return {
        "affine top-40+30": Scoring(match, mismatch, top - 40, 30, True, True),
        "affine 2046+1": Scoring(match, mismatch, 2046, 1, True, True),
        "affine 2047+1": Scoring(match, mismatch, 2047, 1, True, False),
    }


# ---------------------------------------------------------------------------
# B2: the u16 ceiling, 64 (384 + 1) + 1280 = 25920 < 0x7C00
# ---------------------------------------------------------------------------
def ceiling_batch(length):
    """Identical pairs (window == read: score match x length) and
    near-identical ones (one substitution; one deletion against a window one
    base longer), in rotation, so the two packed halves of a lane group never
    hold the same values."""
    kinds = [("exact", "sub", "del")[i % 3] for i in range(9)]
    wl = [length + (1 if k == "del" else 0) for k in kinds]
    return planted(("ceiling", length), [length] * 9, wl, stride16(length), stride16(length + 1), seed=7000 + length,
                   kinds=kinds)


def ceiling_schemes():
    out = {}
    for ge in (0, 1, 1024):
        out[f"64/0 linear {ge}"] = Scoring(64, 0, 0, ge, False, ge != 1)
    for go, ge in ((0, 0), (3, 1), (30000, 1024), (0, 1024)):
        out[f"64/0 affine {go}+{ge}"] = Scoring(64, 0, go, ge, True, go != 3)
    out["64/0 linear 1 cell"] = Scoring(64, 0, 0, 1, False, True)
    out["64/0 affine 3+1 cell"] = Scoring(64, 0, 3, 1, True, True)
    out["1/-63 linear"] = Scoring(1, -63, 0, 2, False, True)
    out["1/-63 affine"] = Scoring(1, -63, 3, 1, True, False)
    out["33/-31 linear"] = Scoring(33, -31, 0, 2, False, False)
    out["33/-31 affine"] = Scoring(33, -31, 30000, 1024, True, True)
    return out


# ---------------------------------------------------------------------------
# the oracle's results, computed once per (batch, scheme) and shared
# ---------------------------------------------------------------------------
_WANT = {}


def want(oracle, b, sc):
    k = (b.key, sc.match, sc.mismatch, sc.affine, sc.gap_open if sc.affine else 0, sc.gap_extend)
    if k not in _WANT:
        _WANT[k] = oracle.sw_batch(b.reads, b.read_len, b.wins, b.win_len, match=sc.match, mismatch=sc.mismatch,
                                   gap_open=sc.gap_open, gap_extend=sc.gap_extend, affine=sc.affine, threads=4)
    return _WANT[k]


# ---------------------------------------------------------------------------
# MSW_WAVE_TRACE records (msw_runtime.cpp traced_launch, msw_device.h
# trace_end): {n_blocks, layout | G << 8 | pairs_blocks << 16}, then four u64
# per block; word 2 holds fast in bit 40, split in bit 41 and KR from bit 48;
# blocks that were not launched are all zero.
# ---------------------------------------------------------------------------
LAYOUT_NAMES = {0: "pairs", 1: "split", 2: "mixed"}


class Launch:
    def __init__(self, hdr, blk):
        self.layout = LAYOUT_NAMES[hdr & 0xFF]
        self.group_lanes = (hdr >> 8) & 0xFF
        used = blk[blk[:, 1] != 0]
        info = used[:, 2].astype(np.uint64)
        self.blocks = int(used.shape[0])
        self.fast = ((info >> np.uint64(40)) & np.uint64(1)).astype(int).tolist()
        self.split = ((info >> np.uint64(41)) & np.uint64(1)).astype(int).tolist()
        self.kr = ((info >> np.uint64(48)) & np.uint64(0xFF)).astype(int).tolist()


class WaveTrace:
    """Reads the records a context appends to its MSW_WAVE_TRACE file."""

    def __init__(self, path):
        self.path, self.seen = str(path), 0

    def new(self):
        """The launches recorded since the last call."""
        raw = np.fromfile(self.path, dtype=np.uint64)
        out, k = [], self.seen
        while k < raw.size:
            n = int(raw[k])
            out.append(Launch(int(raw[k + 1]), raw[k + 2:k + 2 + 4 * n].reshape(n, 4)))
            k += 2 + 4 * n
        self.seen = k
        return out

    def one(self):
        launches = self.new()
        assert len(launches) == 1, f"{len(launches)} launches recorded, expected one"
        return launches[0]


ENV = ("MSW_LAYOUT", "MSW_GROUP_LANES", "MSW_NO_MULTI", "MSW_NO_F16", "MSW_WAVE_TRACE", "MSW_HOST_TRACE")


def set_env(monkeypatch, tmp_path=None, **env):
    """The switches of the context about to be made (read once, at its
    creation); with tmp_path, its wave trace."""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    if tmp_path is None:
        return None
    path = tmp_path / "wave.trace"
    path.write_bytes(b"")
    monkeypatch.setenv("MSW_WAVE_TRACE", str(path))
    return WaveTrace(path)
