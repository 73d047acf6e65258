"""Placing reads restated on the host (include/msw.h, "Placing reads").

TEST INFRASTRUCTURE ONLY.  A sort-based restatement of the k-mer index, the
seeding of one orientation, the orientation rule and the placement.  It never
builds a 4^k table: the index is the sorted list of the codes that occur, so it
runs at k = 14 as well (``dense_off`` makes the table for the small k at which
a test compares the device arrays).

    codes(seq, k) -> (code int64[len - k + 1], coded bool[...])
    Index(genome, k, max_occ): .ucode, .start, .count, .pos, .n_masked
    dense_off(index) -> uint32[4^k + 1]
    seed_one(index, read, band, cap, step) -> (d0, votes, hits, truncated)
    place(index, reads, read_len, both, band, cap, step, min_votes, window)
        -> (win_pos int64, votes uint32, hits uint32, flags uint8)
"""
import numpy as np

import strand_oracle as so

BIAS = 65536
MAX_WIN = 4096
_CODE = np.full(256, -1, np.int64)
for _k, _c in enumerate(b"ACGT"):
    _CODE[_c] = _k


def _arr(seq):
    if isinstance(seq, str):
        seq = seq.encode("latin-1")
    if isinstance(seq, (bytes, bytearray)):
        return np.frombuffer(bytes(seq), np.uint8)
    return np.ascontiguousarray(seq, dtype=np.uint8)


def codes(seq, k):
    """The code of every k-mer of seq and whether it has one."""
    s = _arr(seq)
    n = s.shape[0] - k + 1
    if n <= 0:
        return np.zeros(0, np.int64), np.zeros(0, bool)
    c = _CODE[s]
    code = np.zeros(n, np.int64)
    coded = np.ones(n, bool)
    for j in range(k):
        part = c[j:j + n]
        coded &= part >= 0
        code = code * 4 + np.maximum(part, 0)
    return code, coded


class Index:
    """ucode: the codes with a non-empty stored bucket, ascending; start /
    count: each one's slice of pos; pos: the positions, ascending per bucket."""

    def __init__(self, genome, k, max_occ):
        assert 4 <= k <= 14 and 1 <= max_occ <= 64
        g = _arr(genome)
        assert g.shape[0] <= 0xFFFF0000
        self.k, self.max_occ, self.n = k, max_occ, int(g.shape[0])
        code, coded = codes(g, k)
        p = np.flatnonzero(coded)
        order = np.argsort(code[p], kind="stable")      # by code, then by position
        p, c = p[order], code[p][order]
        ucode, first, count = np.unique(c, return_index=True, return_counts=True)
        keep = count <= max_occ
        self.n_masked = int((~keep).sum())
        self.ucode, self.count = ucode[keep], count[keep].astype(np.int64)
        self.pos = (np.concatenate([p[f:f + n] for f, n in zip(first[keep], count[keep])])
                    if keep.any() else np.zeros(0, np.int64)).astype(np.uint32)
        self.start = np.concatenate([[0], np.cumsum(self.count)])[:-1].astype(np.int64)

    def lookup(self, code, coded):
        """(start, count) of each k-mer's bucket; count 0 where there is none."""
        at = np.searchsorted(self.ucode, code)
        at = np.minimum(at, max(self.ucode.shape[0] - 1, 0))
        hit = coded & (self.ucode[at] == code) if self.ucode.shape[0] else np.zeros(code.shape, bool)
        cnt = np.where(hit, self.count[at], 0) if self.ucode.shape[0] else np.zeros(code.shape, np.int64)
        st = np.where(hit, self.start[at], 0) if self.ucode.shape[0] else np.zeros(code.shape, np.int64)
        return st, cnt


def dense_off(index):
    """off u32[4^k + 1] as the device stores it (small k only)."""
    cnt = np.zeros(4 ** index.k + 1, np.int64)
    cnt[index.ucode] = index.count
    off = np.concatenate([[0], np.cumsum(cnt[:-1])])
    assert off[-1] == index.pos.shape[0]
    return off.astype(np.uint32)


def seed_one(index, read, band, cap, step):
    """One orientation: (d0, votes, hits, truncated); votes 0: no diagonal
    (d0 is then None)."""
    assert band >= 1 and 1 <= cap <= 8192 and step >= 1
    code, coded = codes(read, index.k)
    if code.shape[0] == 0:
        return None, 0, 0, False
    coded = coded & (np.arange(code.shape[0]) % step == 0)
    st, cnt = index.lookup(code, coded)
    P = np.cumsum(cnt)
    truncated = bool(P[-1] > cap)
    diags = []
    for i in np.flatnonzero((cnt > 0) & (P <= cap)):
        diags.append(index.pos[st[i]:st[i] + cnt[i]].astype(np.int64) - int(i))
    if not diags:
        return None, 0, 0, truncated
    D = np.sort(np.concatenate(diags))
    score = np.searchsorted(D, D + band, side="left") - np.searchsorted(D, D, side="left")
    best = int(np.argmax(score))                      # the first maximum: the smallest d0
    return int(D[best]), int(score[best]), int(D.shape[0]), truncated


def window_want(window, L):
    return window if window else min(2 * L, MAX_WIN)


def place_one(index, read, both, band, cap, step, min_votes, window):
    """(win_pos, votes, hits, flags) of one read (bytes)."""
    assert min_votes >= 1
    read = _arr(read).tobytes()
    d0, votes, hits, trunc = seed_one(index, read, band, cap, step)
    rev = 0
    if both:
        r = seed_one(index, so.revcomp(read), band, cap, step)
        if r[1] > votes:                              # strictly: a tie goes forward
            (d0, votes, hits, trunc), rev = r, 1
    L = len(read)
    win_pos = -1
    if votes >= min_votes and votes > 0:
        pad = max(0, window_want(window, L) - (L + band - 1)) // 2
        win_pos = max(0, d0 - pad)
    return win_pos, votes, hits, rev | (2 if trunc else 0)


def place(index, reads, read_len, both=True, band=16, cap=4096, step=1, min_votes=1, window=0):
    """place_one over the rows of a padded batch."""
    n = len(read_len)
    out = (np.empty(n, np.int64), np.empty(n, np.uint32), np.empty(n, np.uint32), np.empty(n, np.uint8))
    for p in range(n):
        row = reads[p][:int(read_len[p])]
        for a, v in zip(out, place_one(index, row, both, band, cap, step, min_votes, window)):
            a[p] = v
    return out
