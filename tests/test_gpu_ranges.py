"""The numeric limits of the packed kernels' two cell domains, every pair
bit-exact against the oracle.

f16 domain: cells hold H x 2^-11, exact only below 2048; the runtime takes it
when match x (min(max_m, max_n) + 2) < 2048.  The batches sit on that bound
from both sides with the top score match x L reached (the binade [1024, 2048),
where a cell uses all 11 significand bits), and the wave trace shows which
domain ran.  u16 domain: the three-way max runs on the bit patterns, so every
value stays below 0x7C00; the largest, 64 (384 + 1) + 1280 = 25920, is reached.
The generators are in tests/range_cases.py (checked on the CPU by
tests/test_range_cases.py).  Run with -m gpu."""
import pytest

import mini_parallel_amd as mpa
import range_cases as rc
from mini_parallel_amd import Scoring
from test_gpu_staging import assert_same, dev_run

pytestmark = pytest.mark.gpu


def layouts_for(max_m):
    """The `layout` values of tests/test_gpu_parity.py that hold reads of
    max_m bases as they say: the split layout has at most 8 packed rows per
    lane (2G rows each), the mixed grid an even number of at most 16 rows per
    lane, narrower pairs groups at most 24 rows."""
    out = ["auto", "pairs"]
    if max_m <= 256:
        out.append("split")
    if max_m <= 256 and -(-max_m // 16) % 2 == 0:
        out.append("mixed")
    if -(-max_m // 12) <= 24:
        out.append("pairs:12")
    if -(-max_m // 22) <= 8:
        out.append("split:11")
    return out


def layout_env(layout):
    if layout == "auto":
        return {}
    lay, _, g = layout.partition(":")
    return {"MSW_LAYOUT": lay, **({"MSW_GROUP_LANES": g} if g else {})}


def check_domain(launch, what, layout, fast):
    """Every launched block ran the domain the case claims, on the layout and
    group width its name says."""
    assert launch.blocks > 0 and launch.fast == [fast] * launch.blocks, (what, launch.fast)
    if layout != "auto":
        lay, _, g = layout.partition(":")
        assert launch.layout == lay and launch.group_lanes == int(g or 16), (what, launch.layout, launch.group_lanes)


def run_case(ctx, trace, oracle, b, sc, what, layout, fast, **bounds):
    got = dev_run(ctx, b, sc, **bounds)
    check_domain(trace.one(), what, layout, fast)
    exp = rc.want(oracle, b, sc)
    assert_same(got, exp, sc.want_coords, what)
    return got


ALL_LAYOUTS = ["auto", "pairs", "split", "mixed", "pairs:12", "split:11"]


@pytest.mark.parametrize("layout", ALL_LAYOUTS)
def test_f16_bound_both_sides(fresh_ctx, oracle, monkeypatch, tmp_path, layout):
    """For each (match, L) with match (L + 2) < 2048 <= match (L + 3): a batch
    of L-base reads runs the f16 domain (fast = 1) and one of L + 1 bases the
    integer domain (fast = 0), windows of twice the read; exact copies score
    match x L -- up to 2034 of 2047 -- besides equalling the oracle.  All four
    scoring kinds, then affine penalties that matter at the top: open + extend
    10 below the top score, and 2047 / 2048, either side of the f16 cap."""
    trace = rc.set_env(monkeypatch, tmp_path, **layout_env(layout))
    ran = 0
    for match, mis, length in rc.F16_EDGES + [rc.F16_ALWAYS]:
        for m, fast in ((length, 1), (length + 1, 0)):
            if m > 384 or layout not in layouts_for(m):
                continue
            b = rc.f16_edge_batch(match, m)
            schemes = dict(rc.with_scheme(rc.FOUR, match=match, mismatch=mis))
            schemes.update(rc.top_gap_schemes(match, mis, m))
            for name, sc in schemes.items():
                what = f"{layout} {match}/{mis} L={m} {name}"
                got = run_case(fresh_ctx, trace, oracle, b, sc, what, layout, fast)
                assert (got[0][b.exact] == match * m).all(), (what, got[0])
                ran += 1
    assert ran >= 4 * 2 * 7  # even split:11 (reads up to 176 bases) holds four table rows, both sides


def test_f16_bound_mirrored(fresh_ctx, oracle, monkeypatch, tmp_path):
    """The window as the shorter side: reads of 384 bases under match 8
    against windows of 253 (f16: 8 x 255 < 2048, top score 2024) and 254
    (integer), on sw_kernel<24>."""
    trace = rc.set_env(monkeypatch, tmp_path)
    for win, fast in ((253, 1), (254, 0)):
        b = rc.mirrored_batch(win)
        schemes = dict(rc.with_scheme(rc.FOUR, match=8, mismatch=-4))
        schemes.update(rc.top_gap_schemes(8, -4, win))
        for name, sc in schemes.items():
            what = f"8/-4 384 x {win} {name}"
            got = run_case(fresh_ctx, trace, oracle, b, sc, what, "pairs", fast)
            assert (got[0][b.exact] == 8 * win).all(), (what, got[0])


@pytest.mark.parametrize("layout", ["auto", "pairs", "split", "mixed", "pairs:12"])
def test_u16_ceiling(fresh_ctx, oracle, monkeypatch, tmp_path, layout):
    """match 64 / mismatch 0 on identical and near-identical pairs of 256 and
    384 bases: scores of 16384 and 24576, under gap penalties from 0 to the
    largest accepted (affine 30000 + 1024: bias 1280, the largest value a
    register holds 25920 < 0x7C00), score-only and best cell; match 1 /
    mismatch -63 and 33 / -31, integer only.  The two pairs packed into one
    register always differ (exact copy / substitution / deletion in rotation),
    so a carry from the low half into the high half shows in the neighbour's
    score."""
    trace = rc.set_env(monkeypatch, tmp_path, **layout_env(layout))
    for m in (256, 384):
        if layout not in layouts_for(m):
            continue
        b = rc.ceiling_batch(m)
        for name, sc in rc.ceiling_schemes().items():
            what = f"{layout} m={m} {name}"
            got = run_case(fresh_ctx, trace, oracle, b, sc, what, layout, 0)
            assert (got[0][b.exact] == sc.match * m).all(), (what, got[0])


SMALL = None


def small_batch():
    global SMALL
    if SMALL is None:
        SMALL = rc.planted("limits-small", [40, 33, 17] * 3, [80, 66, 40] * 3, 48, 80, seed=8001)
    return SMALL


ACCEPTED = {
    "match 64": Scoring(match=64, mismatch=0),
    "mismatch match-64": Scoring(match=2, mismatch=-62, want_coords=True),
    "match 64 affine": Scoring(match=64, mismatch=0, gap_open=1, gap_extend=1, affine=True),
    "gap_extend 1024": Scoring(gap_extend=1024, want_coords=True),
    "gap_extend 1024 affine": Scoring(gap_open=0, gap_extend=1024, affine=True),
    "gap_open 30000": Scoring(gap_open=30000, gap_extend=1, affine=True, want_coords=True),
    "all at once": Scoring(match=64, mismatch=0, gap_open=30000, gap_extend=1024, affine=True, want_coords=True),
}
REFUSED = {
    "match 65": Scoring(match=65, mismatch=0),
    "match 0": Scoring(match=0, mismatch=0),
    "mismatch match-65": Scoring(match=2, mismatch=-63),
    "mismatch match-65 at 64": Scoring(match=64, mismatch=-1),
    "mismatch 1": Scoring(mismatch=1),
    "gap_extend 1025": Scoring(gap_extend=1025),
    "gap_extend 1025 affine": Scoring(gap_open=3, gap_extend=1025, affine=True),
    "gap_open 30001": Scoring(gap_open=30001, gap_extend=1, affine=True),
    "gap_extend -1": Scoring(gap_extend=-1),
    "gap_open -1": Scoring(gap_open=-1, gap_extend=1, affine=True),
}


@pytest.mark.parametrize("name", list(ACCEPTED), ids=lambda v: v.replace(" ", "_"))
def test_scheme_limits_accepted(gpu_ctx, oracle, name):
    """The largest values a scheme may hold each score correctly."""
    b, sc = small_batch(), ACCEPTED[name]
    got = gpu_ctx.align_batch(b.reads, b.read_len, b.wins, b.win_len, sc)
    assert_same(got, rc.want(oracle, b, sc), sc.want_coords, name)


@pytest.mark.parametrize("name", list(REFUSED), ids=lambda v: v.replace(" ", "_"))
def test_scheme_limits_refused(gpu_ctx, name):
    """One past each limit, and negative penalties, raise MswError on the host
    path, the device path and the plan alike (nothing is launched)."""
    b, sc = small_batch(), REFUSED[name]
    with pytest.raises(mpa.MswError):
        gpu_ctx.align_batch(b.reads, b.read_len, b.wins, b.win_len, sc)
    with pytest.raises(mpa.MswError):
        gpu_ctx.align_batch_device(0, 0, 0, 0, 48, 80, 9, 0, 40, 80, sc)
    with pytest.raises(mpa.MswError):
        gpu_ctx.prepare_planned_launch(0, 0, 0, 0, 48, 80, b.read_len, b.win_len, 0, sc)
