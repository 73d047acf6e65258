"""The explicitly scheduled f16 loops of the linear pairs instances keep their
LDS address and the best-cell column index by hand, four wavefront steps per
iteration (msw_device.h, kPaired): a slip would show at an iteration boundary.
So: every remainder of the step count n + G - 1 modulo the steps per
iteration, on the odd-KR and the even-KR score fold, score-only and with the
best cell, every pair bit-exact against the oracle -- and the same batches
with one N per wave, which sends each wave through the integer loop of the
same instance.  Run with -m gpu."""
import numpy as np
import pytest

import range_cases as rc
from test_gpu_staging import assert_same, dev_run

pytestmark = pytest.mark.gpu

N_PAIRS = 24  # G = 12: waves of 10, 10 and 4 pairs; G = 16: three waves of 8
READ_STRIDE, WIN_STRIDE, MAX_M = 160, 304, 152
# n + G - 1 rounded up to a multiple of 4 (or 2): 289..304 cover every remainder
# four times over, the short windows the first iterations
WIN_LENS = [1, 2, 3, 4, 5, 8, 9] + list(range(289, 305))
LINEAR = {k: rc.FOUR[k] for k in ("linear", "linear+cell")}  # config 2's scheme


def batches(n, per_wave):
    """24 pairs, reads of 148..152 bases, every window n columns; and a copy
    with one N in one window of each wave (column 0: inside every window)."""
    rl = [148 + i % 5 for i in range(N_PAIRS)]
    clean = rc.planted(("aligned-loop", n), rl, [n] * N_PAIRS, READ_STRIDE, WIN_STRIDE, seed=8000 + n)
    with_n = clean.copy(("aligned-loop-N", n, per_wave))
    for first in range(0, N_PAIRS, per_wave):
        with_n.wins[first, 0] = ord("N")
    return clean, with_n


@pytest.mark.parametrize("name", list(LINEAR))
@pytest.mark.parametrize("g,kr", [(12, 13), (16, 10)], ids=["G12-KR13", "G16-KR10"])
def test_iteration_boundaries(fresh_ctx, oracle, monkeypatch, tmp_path, g, kr, name):
    trace = rc.set_env(monkeypatch, tmp_path, MSW_LAYOUT="pairs", MSW_GROUP_LANES=g)
    sc = LINEAR[name]
    per_wave = 2 * (64 // g)
    blocks = -(-N_PAIRS // per_wave)
    for n in WIN_LENS:
        for b, fast in zip(batches(n, per_wave), (1, 0)):
            what = f"G={g} KR={kr} {name} n={n} {'f16' if fast else 'integer'}"
            got = dev_run(fresh_ctx, b, sc, max_m=MAX_M, max_n=n)
            launch = trace.one()
            assert launch.layout == "pairs" and launch.group_lanes == g, (what, launch.layout, launch.group_lanes)
            assert launch.kr == [kr] * blocks and launch.fast == [fast] * blocks, (what, launch.kr, launch.fast)
            assert_same(got, rc.want(oracle, b, sc), sc.want_coords, what)
