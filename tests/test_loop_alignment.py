"""Where the 8-byte instructions of the f16 DP loops sit in the built library
(tools/loop_align.py, no GPU): a lone wave pays for every 8-byte instruction
that straddles an 8-byte boundary ("Loop alignment"), so in the
explicitly scheduled f16 loops of the linear pairs instances -- score-only and
with the best cell, every KR the launch units instantiate, the genome
instances included -- the 4-byte instructions stand in pairs and the header is
aligned: no 8-byte instruction at 4 mod 8."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "mini_parallel_amd", "libmsw.so")
# sw_kernel<KR, AFFINE = false, COORDS, SPLIT = false, GEN>
LINEAR_PAIRS = r"\bsw_kernel<(\d+), false, (true|false), false, (true|false)>"
# pairs_lin + pairs_wide (KR 1..24) and genome_lin (KR 1..16), each score-only and with the best cell
EXPECTED = {(kr, coords, gen) for gen, top in ((False, 24), (True, 16)) for kr in range(1, top + 1)
            for coords in (False, True)}


def load_tool():
    spec = importlib.util.spec_from_file_location("loop_align", os.path.join(ROOT, "tools", "loop_align.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def f16_loops():
    """{(KR, COORDS, GEN): the report row of the instance's f16 DP loop}."""
    tool = load_tool()
    if not tool.have_tools():
        pytest.skip("ROCm's llvm-objdump / llvm-objcopy not found: the library cannot be disassembled")
    if not os.path.exists(LIB):
        pytest.skip(f"{LIB} is not built (build() makes it)")
    # the loops of KR 1..4 hold fewer than the tool's default of 100 instructions
    out = {}
    for r in tool.scan(LIB, kernels=LINEAR_PAIRS, min_body=16):
        if r["kind"] != "f16" or not r["max3"]:
            continue
        kr, coords, gen = re.search(LINEAR_PAIRS, r["kernel"]).groups()
        key = (int(kr), coords == "true", gen == "true")
        assert key not in out, f"two f16 DP loops in {r['kernel']}"
        out[key] = r
    return out


def test_every_linear_pairs_instance_is_reported(f16_loops):
    assert set(f16_loops) == EXPECTED, (sorted(EXPECTED - set(f16_loops)), sorted(set(f16_loops) - EXPECTED))


def test_no_eight_byte_instruction_straddles(f16_loops):
    bad = {k: (r["header_mod8"], r["n8_at4"], r["four_byte"]) for k, r in sorted(f16_loops.items())
           if r["header_mod8"] != 0 or r["n8_at4"] != 0 or r["other_size"] != 0}
    assert not bad, f"(KR, COORDS, GEN): (header mod 8, 8-byte instructions at 4 mod 8, the 4-byte ones) {bad}"


def test_valu_per_iteration(f16_loops):
    """Config 2's instance, four steps of 13 rows: 244 VALU (bench.py's
    CYCLES_PER_ROW_STEP rests on it) -- the pairing added none."""
    assert f16_loops[(13, False, False)]["valu"] == 244
