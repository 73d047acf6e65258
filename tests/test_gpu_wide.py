"""Reads of 257-384 bases on the packed kernels: sw_kernel<17..24> (the wide
single-bucket instances) and sw_multi_kernel<.., WIDE>, on both cell domains,
every pair bit-exact against the oracle.  The generators are in
tests/range_cases.py (checked on the CPU by tests/test_range_cases.py).

A case that claims a domain, a rows-per-lane count (KR) or a group width (G)
reads it back: device-API launches from the context's MSW_WAVE_TRACE records
(the `fast` flag, KR and G of every launched block), host-path launches from
MSW_HOST_TRACE.  Run with -m gpu."""
import numpy as np
import pytest

import range_cases as rc
from test_gpu_staging import assert_same, dev_run

pytestmark = pytest.mark.gpu

def check_launch(launch, what, fast, kr=None, g=16, blocks=None, layout="pairs"):
    assert launch.layout == layout and launch.group_lanes == g, (what, launch.layout, launch.group_lanes)
    assert launch.blocks == blocks, (what, launch.blocks, blocks)
    assert launch.fast == ([fast] * blocks if isinstance(fast, int) else fast), (what, launch.fast)
    if kr is not None:
        assert launch.kr == [kr] * blocks, (what, launch.kr)


@pytest.mark.parametrize("domain", ["f16", "u16"])
def test_every_wide_kr_single_bucket(fresh_ctx, oracle, monkeypatch, tmp_path, domain):
    """sw_kernel<KR> for KR = 17..24 as one launch in identity order: reads of
    16 (KR - 1) + 1, 16 KR - 1 and 16 KR bases in one batch, windows of 2m, all
    four scoring kinds.  f16: the default scheme runs the f16 domain (fast = 1
    in every block) and 9/-9, outside the f16 set, the integer domain; u16:
    MSW_NO_F16 sends the default scheme there too."""
    trace = rc.set_env(monkeypatch, tmp_path, **({"MSW_NO_F16": 1} if domain == "u16" else {}))
    schemes = [("2/-1", rc.FOUR, int(domain == "f16"))]
    if domain == "f16":
        schemes.append(("9/-9", rc.with_scheme(rc.FOUR, match=9, mismatch=-9), 0))
    for kr in rc.WIDE_KRS:
        b = rc.kr_batch(kr)
        for tag, scorings, fast in schemes:
            for name, sc in scorings.items():
                what = f"{domain} KR={kr} {tag} {name}"
                got = dev_run(fresh_ctx, b, sc)
                check_launch(trace.one(), what, fast, kr=kr, blocks=2)
                assert_same(got, rc.want(oracle, b, sc), sc.want_coords, what)


def test_wave_level_fallback(fresh_ctx, oracle, monkeypatch, tmp_path):
    """17 pairs of 300 x 600, three waves: an N in a window of the second and
    a lower-case base in the window of the third send exactly those waves to
    the integer domain.  The same bytes only in the row padding past the
    windows' ends change nothing: every wave stays on the f16 domain and the
    results equal those of clean padding."""
    trace = rc.set_env(monkeypatch, tmp_path)
    clean, inside, padded = rc.fallback_batches()
    for name, sc in rc.FOUR.items():
        ref = dev_run(fresh_ctx, clean, sc)
        check_launch(trace.one(), f"clean {name}", 1, kr=19, blocks=3)
        assert_same(ref, rc.want(oracle, clean, sc), sc.want_coords, f"clean {name}")
        got = dev_run(fresh_ctx, inside, sc)
        check_launch(trace.one(), f"inside {name}", [1, 0, 0], kr=19, blocks=3)
        assert_same(got, rc.want(oracle, inside, sc), sc.want_coords, f"inside {name}")
        got = dev_run(fresh_ctx, padded, sc)
        check_launch(trace.one(), f"padding {name}", 1, kr=19, blocks=3)
        assert_same(got, ref, sc.want_coords, f"padding {name}")


@pytest.mark.parametrize("domain", ["f16", "u16"])
def test_later_window_rounds_and_buffer_ends(fresh_ctx, oracle, monkeypatch, tmp_path, domain):
    """Identity-order launches clamp their window loads by the row alone, and
    at G = 16 one staging round covers 512 columns: windows of 511..4096
    columns under reads of 300 and 384 bases need later rounds.  Window lengths
    on the round, chunk and row edges and shorter than the read, from buffers
    of exactly n x stride bytes; every window as long as its row (768 and
    4096), where the last chunk of the last row ends at the buffer's last byte
    in a later round; and the same from a window buffer one byte off 16-byte
    alignment (staged by byte loads; the f16 domain is still taken)."""
    trace = rc.set_env(monkeypatch, tmp_path, **({"MSW_NO_F16": 1} if domain == "u16" else {}))
    fast = int(domain == "f16")
    for b in rc.round_batches():
        for name, sc in rc.THREE.items():
            for off in (0, 1):
                what = f"{domain} {b.key} {name} windows+{off}"
                got = dev_run(fresh_ctx, b, sc, win_off=off)
                check_launch(trace.one(), what, fast, kr=24, blocks=-(-b.n_pairs // 8))
                assert_same(got, rc.want(oracle, b, sc), sc.want_coords, what)


def host_plan(capfd):
    line = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("[msw host]")][-1]
    plan = line.split("last_launch(")[1].split(")")[0]
    return line, plan.split("layout=")[1].split()[0], int(plan.split("G=")[1].split()[0]), \
        int(plan.split("KR=")[1].split()[0])


def planned_twice(ctx, b, sc):
    import torch
    dev = torch.device("cuda", 0)
    d = {k: torch.from_numpy(np.ascontiguousarray(getattr(b, k))).to(dev) for k in ("reads", "wins")}
    rl = torch.from_numpy(np.ascontiguousarray(b.read_len).view(np.int16)).to(dev)
    wl = torch.from_numpy(np.ascontiguousarray(b.win_len).view(np.int16)).to(dev)
    score = torch.full((b.n_pairs,), -7, dtype=torch.int32, device=dev)
    ei = torch.full((b.n_pairs,), -7, dtype=torch.int16, device=dev)
    ej = torch.full((b.n_pairs,), -7, dtype=torch.int16, device=dev)
    step = ctx.prepare_planned_launch(d["reads"].data_ptr(), rl.data_ptr(), d["wins"].data_ptr(), wl.data_ptr(),
                                      b.reads.shape[1], b.wins.shape[1], b.read_len, b.win_len, score.data_ptr(), sc,
                                      ei.data_ptr(), ej.data_ptr(), torch.cuda.current_stream().cuda_stream)
    step()
    step()
    torch.cuda.synchronize()
    step.close()
    return score.cpu().numpy(), ei.cpu().numpy(), ej.cpu().numpy()


@pytest.mark.parametrize("multi", [True, False], ids=["multi", "no_multi"])
def test_length_bucketed_wide(fresh_ctx, oracle, monkeypatch, capfd, multi):
    """Host align_batch over 241..384 bp reads on every bucket edge, shuffled:
    one call, chunks of 7 pairs, asynchronous, and a plan run twice.  multi:
    the eight KR 17..24 buckets run as one launch of the wide instance, so the
    last single-bucket launch the host trace names is that of the 241..256 bp
    bucket (at the layout model's choice);
    under match 6 (7) the f16 bound holds up to 339 (290) bases, so the wide
    buckets of that one launch differ in f16_ok.  MSW_NO_MULTI: every bucket
    gets its own launch, the last one sw_kernel<24>."""
    rc.set_env(monkeypatch, MSW_HOST_TRACE=1, **({} if multi else {"MSW_NO_MULTI": 1}))
    b = rc.bucket_edge_batch()
    for tag, kw in (("2/-1", {}), ("6/-4", dict(match=6, mismatch=-4)), ("7/-4", dict(match=7, mismatch=-4))):
        for name, sc in rc.with_scheme(rc.FOUR, **kw).items():
            what = f"multi={multi} {tag} {name}"
            exp = rc.want(oracle, b, sc)
            capfd.readouterr()
            got = fresh_ctx.align_batch(b.reads, b.read_len, b.wins, b.win_len, sc)
            line, lay, g, kr = host_plan(capfd)
            if multi:  # the last launch of a single bucket held reads of at most 256 bases
                assert kr * g * (2 if lay == "split" else 1) <= 256, (what, line)
            else:
                assert lay == "pairs" and g == 16 and kr == 24, (what, line)
            assert_same(got, exp, sc.want_coords, what)
            got = fresh_ctx.align_batch(b.reads, b.read_len, b.wins, b.win_len, sc, chunk_pairs=7)
            assert_same(got, exp, sc.want_coords, what + " chunks of 7")
            if not multi:  # the last chunk ends with the batch's last pair, its last launch is that pair's or wider
                assert b.read_len[-1] > 256 and host_plan(capfd)[3] >= -(-int(b.read_len[-1]) // 16), what
            pend = fresh_ctx.align_batch(b.reads, b.read_len, b.wins, b.win_len, sc, asynchronous=True)
            assert_same(pend.wait(), exp, sc.want_coords, what + " async")
            assert_same(planned_twice(fresh_ctx, b, sc), exp, sc.want_coords, what + " planned")


def test_forced_13_lane_groups(fresh_ctx, oracle, monkeypatch, tmp_path):
    """MSW_LAYOUT=pairs with MSW_GROUP_LANES=13: four groups of 13 lanes that
    straddle the DPP rows, 8 pairs per wave, and 17 / 20 / 24 rows per lane on
    reads of up to 221 / 260 / 312 bases -- G and KR read back from the trace
    -- on both domains (default scheme, and 9/-9 outside the f16 set)."""
    trace = rc.set_env(monkeypatch, tmp_path, MSW_LAYOUT="pairs", MSW_GROUP_LANES=13)
    for max_m, kr in ((221, 17), (260, 20), (312, 24)):
        b = rc.narrow_batch(max_m)
        for tag, scorings, fast in (("2/-1", rc.FOUR, 1), ("9/-9", rc.with_scheme(rc.THREE, match=9, mismatch=-9), 0)):
            for name, sc in scorings.items():
                what = f"G=13 m<={max_m} {tag} {name}"
                got = dev_run(fresh_ctx, b, sc)
                check_launch(trace.one(), what, fast, kr=kr, g=13, blocks=2)
                assert_same(got, rc.want(oracle, b, sc), sc.want_coords, what)


def test_genome_form_wide_reads(fresh_ctx, oracle, monkeypatch):
    """align_reads with reads of 257..384 bases on a small genome: outside the
    genome instances (KR <= 16), so the windows are cut first.  Windows that
    start at the genome's first byte, end at its last byte, and run past it
    (clipped), at odd byte positions."""
    rc.set_env(monkeypatch)
    rng = np.random.default_rng(13)
    glen, n, w = 4099, 19, 600
    g = rc.ACGT[rng.integers(0, 4, glen)]
    pos = rng.integers(0, glen - w, n).astype(np.int64)
    pos[:6] = [0, 0, glen - w, glen - w + 1, glen - 301, glen - 1]
    wl = np.full(n, w, np.uint16)
    wl[1] = 16
    rl = np.array([(300, 257, 384, 383, 369)[i % 5] for i in range(n)], np.uint16)
    reads = rc.ACGT[rng.integers(0, 4, (n, 384))]
    wins = np.zeros((n, 608), np.uint8)
    clipped = np.zeros(n, np.uint16)
    for i in range(n):
        k = int(min(wl[i], glen - pos[i]))
        clipped[i] = k
        wins[i, :k] = g[pos[i]:pos[i] + k]
        r = min(int(rl[i]), k)
        reads[i, :r] = wins[i, k - r:k]  # the read (or its head) lies at its window's end
        if r > 40:
            reads[i, r // 2] = rc.other_base(reads[i, r // 2])
    b = rc.Batch("genome-wide", reads, rl, wins, clipped, ["noisy"] * n)
    gen = fresh_ctx.load_genome(g)
    try:
        for name, sc in rc.THREE.items():
            got = fresh_ctx.align_reads(gen, reads, rl, pos, wl, scoring=sc)
            assert_same(got, rc.want(oracle, b, sc), sc.want_coords, name)
    finally:
        gen.close()
