"""Staging edges of the scoring kernels' prologue: the length loads, the read
bytes and the first round of 16-byte window chunks leave together, the
window chunks clamped by the row alone (the length-bucketed grid and the
genome instances keep the per-pair clamp).  Every pair of every case against
the oracle, bit-exact, on the smallest shapes at which that can go wrong:
window lengths around the 16-byte chunk and the 192-column round, read
lengths around a lane's rows at G = 12 and 16, partial waves, buffers of
exactly n_pairs x stride bytes.  Run with -m gpu."""
import numpy as np
import pytest

from mini_parallel_amd import Scoring
from mini_parallel_amd.synthetic import config_batch

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", np.uint8)
WIN_LENS = [1, 15, 16, 17, 31, 32, 33, 191, 192, 193, 300, 304]
READ_LENS = [1, 3, 4, 5, 12, 13, 14, 147, 148, 149, 150, 151, 152, 155, 156]
PAIR_COUNTS = [1, 9, 10, 11, 21]
WIN_STRIDE, READ_STRIDE = 304, 156
SCORINGS = {
    "linear": Scoring(),
    "linear+cell": Scoring(want_coords=True),
    "affine+cell": Scoring(gap_open=3, gap_extend=1, affine=True, want_coords=True),
}
LAYOUTS = ["auto", "pairs:12", "pairs:16", "pairs:8", "split:11", "mixed"]


class Batch:
    def __init__(self, reads, read_len, wins, win_len):
        self.reads, self.read_len, self.wins, self.win_len = reads, read_len, wins, win_len
        self.n_pairs = int(reads.shape[0])


def edge_batch(n, shift=0, read_stride=READ_STRIDE, win_stride=WIN_STRIDE, seed=7):
    """n pairs whose lengths walk WIN_LENS / READ_LENS with coprime steps, so
    one wave mixes them and 21 pairs hold every length; each window carries
    its read (a few substitutions, one deletion) where it fits.  The row
    padding past a read or window is random A/C/G/T, never zero: a kernel that
    scores a padding byte is caught."""
    rng = np.random.default_rng(seed + 131 * n + shift)
    rl = np.array([READ_LENS[(7 * i + shift) % len(READ_LENS)] for i in range(n)], np.uint16)
    wl = np.array([WIN_LENS[(5 * i + shift) % len(WIN_LENS)] for i in range(n)], np.uint16)
    reads = ACGT[rng.integers(0, 4, (n, read_stride))]
    wins = ACGT[rng.integers(0, 4, (n, win_stride))]
    for i in range(n):
        m, w = int(rl[i]), int(wl[i])
        r = reads[i, :m].copy()
        r[rng.random(m) < 0.03] = ord("A")
        if m > 20:
            r = np.delete(r, m // 2)
        k = min(len(r), w)
        at = int(rng.integers(0, w - k + 1))
        wins[i, at:at + k] = r[:k]
    return Batch(reads, rl, wins, wl)


_WANT = {}


def want(oracle, key, b, sc):
    """Oracle results, computed once per (batch, scheme) and shared."""
    k = (key, sc.affine, sc.gap_open, sc.gap_extend)
    if k not in _WANT:
        _WANT[k] = oracle.sw_batch(b.reads, b.read_len, b.wins, b.win_len, match=sc.match, mismatch=sc.mismatch,
                                   gap_open=sc.gap_open, gap_extend=sc.gap_extend, affine=sc.affine, threads=4)
    return _WANT[k]


def dev_run(ctx, b, sc, read_off=0, win_off=0, max_m=None, max_n=None):
    """msw_align_batch_device over buffers of exactly n x stride bytes (plus
    the byte offset asked for): identity slot order, the benchmark's path."""
    import torch
    dev = torch.device("cuda", 0)
    n, rs, ws = b.n_pairs, b.reads.shape[1], b.wins.shape[1]
    dr = torch.zeros(n * rs + read_off, dtype=torch.uint8, device=dev)
    dw = torch.zeros(n * ws + win_off, dtype=torch.uint8, device=dev)
    dr[read_off:] = torch.from_numpy(np.ascontiguousarray(b.reads).reshape(-1)).to(dev)
    dw[win_off:] = torch.from_numpy(np.ascontiguousarray(b.wins).reshape(-1)).to(dev)
    rl = torch.from_numpy(np.ascontiguousarray(b.read_len).view(np.int16)).to(dev)
    wl = torch.from_numpy(np.ascontiguousarray(b.win_len).view(np.int16)).to(dev)
    score = torch.full((n,), -7, dtype=torch.int32, device=dev)
    ei = torch.full((n,), -7, dtype=torch.int16, device=dev)
    ej = torch.full((n,), -7, dtype=torch.int16, device=dev)
    ctx.align_batch_device(dr.data_ptr() + read_off, rl.data_ptr(), dw.data_ptr() + win_off, wl.data_ptr(), rs, ws, n,
                           score.data_ptr(), max_m or int(b.read_len.max()), max_n or int(b.win_len.max()), sc,
                           ei.data_ptr() if sc.want_coords else 0, ej.data_ptr() if sc.want_coords else 0,
                           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return score.cpu().numpy(), ei.cpu().numpy(), ej.cpu().numpy()


def assert_same(got, exp, coords, what=""):
    s, i, j = got
    ws, wi, wj = exp
    bad = np.nonzero(s != ws)[0]
    assert bad.size == 0, f"{what}: {bad.size} score mismatches, first {bad[:5]}: gpu {s[bad[:5]]} oracle {ws[bad[:5]]}"
    if coords:
        bad = np.nonzero((i != wi) | (j != wj))[0]
        assert bad.size == 0, (f"{what}: {bad.size} best-cell mismatches, first {bad[:5]}: gpu "
                               f"{list(zip(i[bad[:5]], j[bad[:5]]))} oracle {list(zip(wi[bad[:5]], wj[bad[:5]]))}")


def set_layout(monkeypatch, layout):
    for k in ("MSW_LAYOUT", "MSW_GROUP_LANES", "MSW_NO_MULTI", "MSW_NO_F16"):
        monkeypatch.delenv(k, raising=False)
    if layout != "auto":
        lay, _, g = layout.partition(":")
        monkeypatch.setenv("MSW_LAYOUT", lay)
        if g:
            monkeypatch.setenv("MSW_GROUP_LANES", g)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_length_edges(fresh_ctx, oracle, monkeypatch, layout):
    """Every window / read length edge, in partial waves of 1, 9, 10, 11 and
    21 pairs, under the three scoring kinds; the launch's length bounds are
    the strides' (304 / 156: 13 rows per lane at G = 12, 10 at G = 16)."""
    set_layout(monkeypatch, layout)
    for n in PAIR_COUNTS:
        b = edge_batch(n, shift=n)
        for name, sc in SCORINGS.items():
            got = dev_run(fresh_ctx, b, sc, max_m=READ_STRIDE, max_n=WIN_STRIDE)
            assert_same(got, want(oracle, ("edge", n), b, sc), sc.want_coords, f"{layout} n={n} {name}")


@pytest.mark.parametrize("layout", ["auto", "pairs:12", "split:11"])
def test_full_stride_windows(fresh_ctx, oracle, monkeypatch, layout):
    """Every window as long as its row (304 = 19 chunks): the last chunk of
    the batch's last row ends at the buffer's last byte."""
    set_layout(monkeypatch, layout)
    b = edge_batch(11, shift=3)
    b.win_len[:] = WIN_STRIDE
    for name, sc in SCORINGS.items():
        assert_same(dev_run(fresh_ctx, b, sc), want(oracle, "full", b, sc), sc.want_coords, f"{layout} {name}")


@pytest.mark.parametrize("layout", ["auto", "pairs:16", "split:11"])
def test_window_bytes(fresh_ctx, oracle, monkeypatch, layout):
    """An N or a lower-case base inside a window: its wave falls back to the
    integer path and stays exact.  The same bytes only in the row padding past
    the window's end: results equal those of clean padding (and the oracle's)."""
    set_layout(monkeypatch, layout)
    clean = edge_batch(21, shift=1)
    inside = Batch(clean.reads, clean.read_len, clean.wins.copy(), clean.win_len)
    padded = Batch(clean.reads, clean.read_len, clean.wins.copy(), clean.win_len)
    for i in range(21):
        w = int(clean.win_len[i])
        if i % 3 == 0:
            inside.wins[i, (w - 1) * (i % 2)] = ord("N") if i % 2 else ord("a")
        padded.wins[i, w:] = np.resize(np.frombuffer(b"Nacgt\x00\xff", np.uint8), WIN_STRIDE - w)
    for name, sc in SCORINGS.items():
        ref = dev_run(fresh_ctx, clean, sc, max_m=READ_STRIDE, max_n=WIN_STRIDE)
        assert_same(ref, want(oracle, "clean", clean, sc), sc.want_coords, f"{layout} clean {name}")
        got = dev_run(fresh_ctx, padded, sc, max_m=READ_STRIDE, max_n=WIN_STRIDE)
        assert_same(got, ref, sc.want_coords, f"{layout} padding {name}")
        got = dev_run(fresh_ctx, inside, sc, max_m=READ_STRIDE, max_n=WIN_STRIDE)
        assert_same(got, want(oracle, "inside", inside, sc), sc.want_coords, f"{layout} inside {name}")


@pytest.mark.parametrize("layout", ["auto", "pairs:12", "split:11"])
def test_read_bytes_and_alignment(fresh_ctx, oracle, monkeypatch, layout):
    """Non-ACGT read bytes (N, lower case, bytes whose class collides with a
    base, high-bit bytes) in reads and in the padding past them; then the same
    batch from a read buffer one byte off alignment, and with a read stride
    that is no multiple of 4 (157)."""
    set_layout(monkeypatch, layout)
    rng = np.random.default_rng(3)
    b = edge_batch(21, shift=2)
    zoo = np.frombuffer(b"NacgtEBDHS\x00\xc1\xc3", np.uint8)
    hit = rng.random(b.reads.shape) < 0.08
    b.reads[hit] = rng.choice(zoo, int(hit.sum()))
    odd = Batch(np.concatenate([b.reads, rng.choice(zoo, (21, 1))], axis=1), b.read_len, b.wins, b.win_len)
    assert odd.reads.shape[1] == 157
    for name, sc in SCORINGS.items():
        exp = want(oracle, "zoo", b, sc)
        assert_same(dev_run(fresh_ctx, b, sc), exp, sc.want_coords, f"{layout} aligned {name}")
        assert_same(dev_run(fresh_ctx, b, sc, read_off=1), exp, sc.want_coords, f"{layout} reads+1 {name}")
        assert_same(dev_run(fresh_ctx, odd, sc), exp, sc.want_coords, f"{layout} stride 157 {name}")
        assert_same(dev_run(fresh_ctx, odd, sc, read_off=1), exp, sc.want_coords, f"{layout} stride 157 +1 {name}")


@pytest.mark.parametrize("layout", ["auto", "pairs:12", "split:11"])
def test_unaligned_windows(fresh_ctx, oracle, monkeypatch, layout):
    """A window buffer one byte off 16-byte alignment: the scalar staging path
    (byte loads), on ACGT windows and with an N inside one."""
    set_layout(monkeypatch, layout)
    b = edge_batch(21, shift=4)
    n_in = Batch(b.reads, b.read_len, b.wins.copy(), b.win_len)
    n_in.wins[5, 0] = ord("N")
    for name, sc in SCORINGS.items():
        got = dev_run(fresh_ctx, b, sc, win_off=1, max_m=READ_STRIDE, max_n=WIN_STRIDE)
        assert_same(got, want(oracle, "unal", b, sc), sc.want_coords, f"{layout} {name}")
        got = dev_run(fresh_ctx, n_in, sc, win_off=1, max_m=READ_STRIDE, max_n=WIN_STRIDE)
        assert_same(got, want(oracle, "unal_n", n_in, sc), sc.want_coords, f"{layout} N {name}")


@pytest.mark.parametrize("multi", [True, False])
def test_planned_mixed_lengths_small(fresh_ctx, oracle, monkeypatch, multi):
    """A few hundred pairs of 75 to 250 bp through the plan: the
    length-bucketed launch, which keeps the per-pair window clamp, and the
    plan's order through the single-bucket kernels (MSW_NO_MULTI)."""
    import torch
    set_layout(monkeypatch, "auto")
    if not multi:
        monkeypatch.setenv("MSW_NO_MULTI", "1")
    b = config_batch(5, n_pairs=300, seed_offset=9)
    dev = torch.device("cuda", 0)
    d = {k: torch.from_numpy(np.ascontiguousarray(getattr(b, k))).to(dev) for k in ("reads", "wins")}
    rl = torch.from_numpy(np.ascontiguousarray(b.read_len).view(np.int16)).to(dev)
    wl = torch.from_numpy(np.ascontiguousarray(b.win_len).view(np.int16)).to(dev)
    for name, sc in SCORINGS.items():
        score = torch.full((b.n_pairs,), -7, dtype=torch.int32, device=dev)
        ei = torch.zeros(b.n_pairs, dtype=torch.int16, device=dev)
        ej = torch.zeros(b.n_pairs, dtype=torch.int16, device=dev)
        step = fresh_ctx.prepare_planned_launch(d["reads"].data_ptr(), rl.data_ptr(), d["wins"].data_ptr(),
                                                wl.data_ptr(), b.reads.shape[1], b.wins.shape[1], b.read_len,
                                                b.win_len, score.data_ptr(), sc, ei.data_ptr(), ej.data_ptr(),
                                                torch.cuda.current_stream().cuda_stream)
        step()
        torch.cuda.synchronize()
        step.close()
        got = (score.cpu().numpy(), ei.cpu().numpy(), ej.cpu().numpy())
        assert_same(got, want(oracle, "planned", b, sc), sc.want_coords, f"multi={multi} {name}")


def test_genome_windows_at_both_ends(fresh_ctx, oracle, monkeypatch):
    """align_reads on a small genome: windows that start at its first byte,
    end at its last byte, and run past it (clipped), at odd byte positions."""
    set_layout(monkeypatch, "auto")
    rng = np.random.default_rng(11)
    glen, n, m, w = 5003, 40, 150, 300
    g = ACGT[rng.integers(0, 4, glen)]
    pos = rng.integers(0, glen - w, n).astype(np.int64)
    pos[:6] = [0, 0, glen - w, glen - w + 1, glen - 17, glen - 1]
    wl = np.full(n, w, np.uint16)
    wl[1] = 16
    rl = np.array([READ_LENS[i % len(READ_LENS)] for i in range(n)], np.uint16)
    reads = ACGT[rng.integers(0, 4, (n, 160))]
    wins = np.zeros((n, 304), np.uint8)
    clipped = np.zeros(n, np.uint16)
    for i in range(n):
        k = int(min(wl[i], glen - pos[i]))
        clipped[i] = k
        wins[i, :k] = g[pos[i]:pos[i] + k]
        r = min(int(rl[i]), k)
        reads[i, :r] = wins[i, k - r:k]  # the read lies at its window's end
    b = Batch(reads, rl, wins, clipped)
    gen = fresh_ctx.load_genome(g)
    try:
        for name, sc in SCORINGS.items():
            got = fresh_ctx.align_reads(gen, reads, rl, pos, wl, scoring=sc)
            assert_same(got, want(oracle, "genome", b, sc), sc.want_coords, name)
    finally:
        gen.close()
