// Writes argv[1]: .aln blocks with and without the mapq / sub_score arrays
// (flag bit 1), with and without strand bytes, made by the CLI's encoder
// (cli_aln_block.h); tests/test_mapq_format.py holds the same arrays and
// compares the file with mini_parallel_amd/alnfile.py.
#include <cstdio>

#include "cli_aln_block.h"

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    const uint32_t M = 0, I = 1, S = 4;
    std::vector<uint8_t> out;

    // reads 0..2: strand bytes and mapq (one pad byte each)
    const int64_t a_ref[] = {1000, 2001, -1};
    const int32_t a_score[] = {300, 251, 0}, a_nm[] = {0, 3, 0};
    const int16_t a_ei[] = {149, 148, -1}, a_ej[] = {149, 299, -1};
    const uint32_t a_off[] = {0, 1, 4, 4};
    const uint32_t a_ops[] = {150u << 4 | M, 100u << 4 | M, 2u << 4 | I, 47u << 4 | M};
    const uint8_t a_strand[] = {1, 0, 0}, a_mapq[] = {60, 17, 0};
    const int32_t a_sub[] = {0, 208, -5};
    append_aln_block(out, 0, 3, a_ref, a_score, a_nm, a_off, a_ei, a_ej, a_ops, 4, a_strand, a_mapq, a_sub);

    // read 3: neither
    const int64_t b_ref[] = {70000};
    const int32_t b_score[] = {77}, b_nm[] = {2};
    const int16_t b_ei[] = {149}, b_ej[] = {290};
    const uint32_t b_off[] = {0, 3};
    const uint32_t b_ops[] = {5u << 4 | S, 140u << 4 | M, 5u << 4 | S};
    append_aln_block(out, 3, 1, b_ref, b_score, b_nm, b_off, b_ei, b_ej, b_ops, 3);

    // an empty block with both flags: nothing but a header
    const uint8_t none[] = {0};
    const int32_t none32[] = {0};
    append_aln_block(out, 4, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, none, none, none32);

    // reads 4..8: mapq without strand bytes (five reads: three pad bytes)
    const int64_t c_ref[] = {-1, -1, -1, -1, 5};
    const int32_t c_score[] = {0, 0, 0, 0, 16}, c_nm[] = {0, 0, 0, 0, 0};
    const int16_t c_ei[] = {-1, -1, -1, -1, 7}, c_ej[] = {-1, -1, -1, -1, 9};
    const uint32_t c_off[] = {0, 0, 0, 0, 0, 1};
    const uint32_t c_ops[] = {8u << 4 | M};
    const uint8_t c_mapq[] = {0, 0, 0, 0, 59};
    const int32_t c_sub[] = {0, 0, 0, 0, 2147483647};
    append_aln_block(out, 4, 5, c_ref, c_score, c_nm, c_off, c_ei, c_ej, c_ops, 1, nullptr, c_mapq, c_sub);

    FILE* f = fopen(argv[1], "wb");
    if (!f || fwrite(out.data(), 1, out.size(), f) != out.size() || fclose(f) != 0) return 1;
    return 0;
}
