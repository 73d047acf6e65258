"""``write_vcf(..., insertions=)``: the majority rule that turns ``<INS>``
into a real ALT (mini_parallel_amd.write_vcf's docstring)."""
import numpy as np
import pytest

from test_variant_format import GENOME, HET, HOM, ROWS, VCF, variants
import variant_oracle as vo

TGA = 3 | 2 << 2 | 0 << 4


def sites(*rows):
    """rows: (pos, events, alleles, best_count, second_count, best_len, seq)"""
    from mini_parallel_amd import INS_SITE_DTYPE
    return np.array([r[:6] + (0, r[6]) for r in rows], INS_SITE_DTYPE)


def test_ins_sequence():
    from mini_parallel_amd import MswError, ins_sequence
    assert ins_sequence(3, TGA) == b"TGA" and ins_sequence(0, 0) == b""
    assert ins_sequence(32, (1 << 64) - 1) == b"T" * 32
    with pytest.raises(MswError):
        ins_sequence(33, 0)


@pytest.mark.parametrize("site, alt", [
    ((4, 20, 3, 11, 9, 3, TGA), "ATGA"),     # 11 of 20: above half
    ((4, 20, 2, 10, 10, 3, TGA), "<INS>"),   # exactly 2 * best == events
    ((4, 20, 1, 0, 0, 0, 0), "<INS>"),       # no allele without flags
    ((5, 20, 1, 20, 0, 3, TGA), "<INS>"),    # the table has no site at the record's position
])
def test_majority_rule(tmp_path, site, alt):
    from mini_parallel_amd import write_vcf
    rows = [(4, vo.INS, ord("A"), 0) + HOM, (7, vo.SNV, ord("T"), ord("C")) + HET]
    write_vcf(tmp_path / "v.vcf", variants(rows), GENOME, insertions=sites(site))
    text = open(tmp_path / "v.vcf").read()
    body = [ln.split("\t") for ln in text.splitlines() if not ln.startswith("#")]
    assert [(b[1], b[3], b[4]) for b in body] == [("5", "A", alt), ("8", "T", "C")]
    assert ("##ALT=<ID=INS" in text) == (alt == "<INS>")


def test_without_a_table_the_file_is_as_before(tmp_path):
    from mini_parallel_amd import write_vcf
    write_vcf(tmp_path / "v.vcf", variants(ROWS), GENOME, contig="chr9", sample="NA1", insertions=None)
    assert open(tmp_path / "v.vcf").read() == VCF
