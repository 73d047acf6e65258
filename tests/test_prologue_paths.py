"""How a scoring wave reads its rows (msw_device.h): as aligned dwords
realigned by the lane's start offset where the batch allows it, else as
bytes -- at every row start residue, read length and row end, with bytes
outside A/C/G/T in the reads -- and, since the f16 tables, the integer codes
and the window staging all hang on those rows, every window length round the
16-column chunks.

24 pairs per batch -- at G = 12 waves of 10, 10 and 4 pairs, so the last wave
has empty slots -- every pair bit-exact against the oracle, scores and best
cell, under config 2's scheme (linear, score only) and affine + best cell; the
launch trace says which layout, rows per lane, arithmetic path and read arm
(dwords or bytes) ran.  Run with -m gpu."""
import numpy as np
import pytest

import range_cases as rc
from mini_parallel_amd.synthetic import config_batch
from test_gpu_staging import assert_same, dev_run

pytestmark = pytest.mark.gpu

N_PAIRS = 24
READ_STRIDE, WIN_STRIDE, MAX_M = 160, 304, 152
SCHEMES = {k: rc.FOUR[k] for k in ("linear", "affine+cell")}
# (layout, G, rows per lane at MAX_M, pairs per wave).  Lane starts l * KR hit
# every residue mod 4 at KR 13 and KR 19, 0 and 2 only at KR 10; the split
# layout's halves start at multiples of KR 7.
LAYOUTS = [("pairs", 12, 13, 10), ("pairs", 8, 19, 16), ("pairs", 16, 10, 8), ("split", 12, 7, 5)]
LAYOUT_IDS = ["G12-KR13", "G8-KR19", "G16-KR10", "split-G12-KR7"]


def read_arms(trace):
    """Bit 42 of word 2 of every block of the record trace.one() reads next
    (msw_device.h, trace_end): 1 if the block loaded its read rows as dwords."""
    raw = np.fromfile(trace.path, dtype=np.uint64)
    n = int(raw[trace.seen])
    blk = raw[trace.seen + 2:trace.seen + 2 + 4 * n].reshape(n, 4)
    used = blk[blk[:, 1] != 0]
    return ((used[:, 2] >> np.uint64(42)) & np.uint64(1)).astype(int).tolist()


def run(ctx, trace, b, sc, layout, what, fast=None, max_n=WIN_STRIDE, vec=1, **kw):
    """One launch of batch b; the trace must show the layout asked for, the
    read arm (vec: 1 dwords, 0 bytes) and, where given, the arithmetic path
    of every block (one value, or a list)."""
    lay, g, kr, per_wave = layout
    got = dev_run(ctx, b, sc, max_m=MAX_M, max_n=max_n, **kw)
    arms = read_arms(trace)
    launch = trace.one()
    blocks = -(-b.n_pairs // per_wave)
    assert arms == [vec] * blocks, (what, arms)
    assert launch.layout == lay and launch.group_lanes == g, (what, launch.layout, launch.group_lanes)
    assert launch.kr == [kr] * blocks, (what, launch.kr)
    if fast is not None:
        assert launch.fast == (fast if isinstance(fast, list) else [fast] * blocks), (what, launch.fast)
    return got


def env(monkeypatch, tmp_path, layout):
    return rc.set_env(monkeypatch, tmp_path, MSW_LAYOUT=layout[0], MSW_GROUP_LANES=layout[1])


def read_length_batches(kr):
    """Reads of every length at which a lane's rows end inside a dword, at a
    dword's end or with the lane (1..5, KR - 1, KR, KR + 1, 2 KR + 1, 148..152);
    pairs 0 and 1 -- one lane group -- hold 1 and 152 bases.  `mix`: rows of
    160 bytes; `full`: rows of exactly the longest read, 152 bytes, so a lane's
    last dword is its row's last, every fourth read 152 bases long."""
    lens = [1, 152, 2, 3, 4, 5, kr - 1, kr, kr + 1, 2 * kr + 1, 148, 149, 150, 151, 152]
    rl = [lens[i % len(lens)] for i in range(N_PAIRS)]
    mix = rc.planted(("prologue-mix", kr), rl, [300] * N_PAIRS, READ_STRIDE, WIN_STRIDE, seed=9100 + kr)
    rl = [152 if i % 4 == 0 else 148 + i % 5 for i in range(N_PAIRS)]
    full = rc.planted(("prologue-full", kr), rl, [300] * N_PAIRS, MAX_M, WIN_STRIDE, seed=9200 + kr)
    return mix, full


@pytest.mark.parametrize("name", list(SCHEMES))
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_read_lengths_and_row_ends(fresh_ctx, oracle, monkeypatch, tmp_path, layout, name):
    trace = env(monkeypatch, tmp_path, layout)
    sc = SCHEMES[name]
    for b in read_length_batches(layout[2]):
        what = f"{layout} {name} {b.key}"
        got = run(fresh_ctx, trace, b, sc, layout, what, fast=1)
        assert_same(got, rc.want(oracle, b, sc), sc.want_coords, what)


ODD_BYTES = (ord("N"), ord("a"), 0x00, 0xFF)


def odd_byte_batch(kr):
    """Reads of 149..152 bases whose windows are clean.  Pair i carries one of
    N, a, 0x00 and 0xFF at one of the four byte positions of a dword (16
    combinations over 24 pairs): in the first row of a lane whose start has
    that residue, in the last row of a lane that ends on it, in one more row
    of that residue, and in the read's last base."""
    rl = [149 + i % 4 for i in range(N_PAIRS)]
    b = rc.planted(("prologue-odd", kr), rl, [300] * N_PAIRS, READ_STRIDE, WIN_STRIDE, seed=9300 + kr)
    for i in range(N_PAIRS):
        byte, res, m = ODD_BYTES[i % 4], (i // 4) % 4, rl[i]
        firsts = [p for p in range(0, m, kr) if p % 4 == res]
        lasts = [p for p in range(kr - 1, m, kr) if p % 4 == res]
        spots = {res + 4 * (1 + i % 7), m - 1}
        if firsts:
            spots.add(firsts[i % len(firsts)])
        if lasts:
            spots.add(lasts[i % len(lasts)])
        b.reads[i, sorted(spots)] = byte
    return b


@pytest.mark.parametrize("name", list(SCHEMES))
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_other_read_bytes_keep_the_f16_path(fresh_ctx, oracle, monkeypatch, tmp_path, layout, name):
    """A read byte outside A/C/G/T never sends a wave to the integer path
    (only window bytes do); its row scores as all mismatch, like the
    oracle's byte compare."""
    trace = env(monkeypatch, tmp_path, layout)
    sc = SCHEMES[name]
    b = odd_byte_batch(layout[2])
    what = f"{layout} {name}"
    got = run(fresh_ctx, trace, b, sc, layout, what, fast=1)
    assert_same(got, rc.want(oracle, b, sc), sc.want_coords, what)


@pytest.mark.parametrize("name", list(SCHEMES))
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_byte_load_arm(fresh_ctx, oracle, monkeypatch, tmp_path, layout, name):
    """Batches that do not allow dword loads -- a read stride of 153 or 157,
    a read buffer 1, 2 or 3 bytes off alignment -- give what the aligned
    batch gives."""
    trace = env(monkeypatch, tmp_path, layout)
    sc = SCHEMES[name]
    mix, _ = read_length_batches(layout[2])
    odd = odd_byte_batch(layout[2])
    rng = np.random.default_rng(17)
    for b in (mix, odd):
        ref = run(fresh_ctx, trace, b, sc, layout, f"{layout} {name} {b.key} aligned", fast=1)
        assert_same(ref, rc.want(oracle, b, sc), sc.want_coords, f"{layout} {name} {b.key} aligned")
        for off in (1, 2, 3):
            what = f"{layout} {name} {b.key} reads + {off}"
            assert_same(run(fresh_ctx, trace, b, sc, layout, what, fast=1, vec=0, read_off=off), ref, sc.want_coords, what)
        for stride in (153, 157):
            wide = b.copy((b.key, stride))
            wide.reads = np.concatenate([b.reads[:, :MAX_M], rc.ACGT[rng.integers(0, 4, (N_PAIRS, stride - MAX_M))]],
                                        axis=1)
            what = f"{layout} {name} {b.key} stride {stride}"
            assert_same(run(fresh_ctx, trace, wide, sc, layout, what, fast=1, vec=0), ref, sc.want_coords, what)


WIN_LENS = [1, 15, 16, 17, 31, 32, 33] + list(range(289, 305))


def window_batch(n):
    rl = [148 + i % 5 for i in range(N_PAIRS)]
    return rc.planted(("prologue-win", n), rl, [n] * N_PAIRS, READ_STRIDE, WIN_STRIDE, seed=9400 + n,
                      at_end=range(0, N_PAIRS, 2))


@pytest.mark.parametrize("name", list(SCHEMES))
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_window_masks(fresh_ctx, oracle, monkeypatch, tmp_path, layout, name):
    """Every window of a batch n columns long, with every second read at its
    window's end; group partners of 300 and 17 columns; and one N in a
    window, which sends that wave alone to the integer path (its codes come
    from the same row dwords)."""
    trace = env(monkeypatch, tmp_path, layout)
    sc = SCHEMES[name]
    per_wave = layout[3]
    for n in WIN_LENS:
        b = window_batch(n)
        what = f"{layout} {name} n={n}"
        assert_same(run(fresh_ctx, trace, b, sc, layout, what, fast=1, max_n=n), rc.want(oracle, b, sc),
                    sc.want_coords, what)
    rl = [148 + i % 5 for i in range(N_PAIRS)]
    partners = rc.planted("prologue-partners", rl, [300 if i % 2 == 0 else 17 for i in range(N_PAIRS)], READ_STRIDE,
                          WIN_STRIDE, seed=9500, at_end=range(N_PAIRS))
    what = f"{layout} {name} partners 300 / 17"
    assert_same(run(fresh_ctx, trace, partners, sc, layout, what, fast=1), rc.want(oracle, partners, sc),
                sc.want_coords, what)
    with_n = window_batch(300).copy(("prologue-win-N", per_wave))
    # an even pair of the second wave (its read ends at the window's end), the window's last column
    with_n.wins[per_wave + per_wave % 2, 299] = ord("N")
    blocks = -(-N_PAIRS // per_wave)
    what = f"{layout} {name} N in a window"
    got = run(fresh_ctx, trace, with_n, sc, layout, what, fast=[int(k != 1) for k in range(blocks)])
    assert_same(got, rc.want(oracle, with_n, sc), sc.want_coords, what)


def test_genome_and_planned_launches(fresh_ctx, oracle, monkeypatch):
    """The other instances that share the helpers: reads against a resident
    genome at unaligned window positions, and a planned, length-bucketed
    launch over reads of 75 to 250 bases."""
    import torch
    rc.set_env(monkeypatch)
    rng = np.random.default_rng(23)
    glen, w = 3001, 300
    g = rc.ACGT[rng.integers(0, 4, glen)]
    pos = rng.integers(0, glen - w, N_PAIRS).astype(np.int64)
    pos[:4] = [1, 2, 3, glen - w - 1]
    rl = np.array([1, 152] + [148 + i % 5 for i in range(N_PAIRS - 2)], np.uint16)
    wl = np.full(N_PAIRS, w, np.uint16)
    reads = rc.ACGT[rng.integers(0, 4, (N_PAIRS, READ_STRIDE))]
    wins = np.zeros((N_PAIRS, WIN_STRIDE), np.uint8)
    for i in range(N_PAIRS):
        wins[i, :w] = g[pos[i]:pos[i] + w]
        reads[i, :rl[i]] = wins[i, w - rl[i]:w]  # the read lies at its window's end
    reads[5, 3] = ord("N")
    b = rc.Batch("prologue-genome", reads, rl, wins, wl, ["exact"] * N_PAIRS)
    gen = fresh_ctx.load_genome(g)
    try:
        for name, sc in SCHEMES.items():
            got = fresh_ctx.align_reads(gen, reads, rl, pos, wl, scoring=sc)
            assert_same(got, rc.want(oracle, b, sc), sc.want_coords, f"genome {name}")
    finally:
        gen.close()

    c5 = config_batch(5, n_pairs=96, seed_offset=13)
    b = rc.Batch("prologue-planned", c5.reads, c5.read_len, c5.wins, c5.win_len, ["noisy"] * c5.n_pairs)
    dev = torch.device("cuda", 0)
    d = {k: torch.from_numpy(np.ascontiguousarray(getattr(b, k))).to(dev) for k in ("reads", "wins")}
    dl = {k: torch.from_numpy(np.ascontiguousarray(getattr(b, k)).view(np.int16)).to(dev) for k in ("read_len", "win_len")}
    for name, sc in SCHEMES.items():
        score = torch.full((b.n_pairs,), -7, dtype=torch.int32, device=dev)
        ei = torch.zeros(b.n_pairs, dtype=torch.int16, device=dev)
        ej = torch.zeros(b.n_pairs, dtype=torch.int16, device=dev)
        step = fresh_ctx.prepare_planned_launch(d["reads"].data_ptr(), dl["read_len"].data_ptr(), d["wins"].data_ptr(),
                                                dl["win_len"].data_ptr(), b.reads.shape[1], b.wins.shape[1],
                                                b.read_len, b.win_len, score.data_ptr(), sc, ei.data_ptr(),
                                                ej.data_ptr(), torch.cuda.current_stream().cuda_stream)
        step()
        torch.cuda.synchronize()
        step.close()
        got = (score.cpu().numpy(), ei.cpu().numpy(), ej.cpu().numpy())
        assert_same(got, rc.want(oracle, b, sc), sc.want_coords, f"planned {name}")
