// Writes argv[1]: four .aln blocks made by the CLI's encoder (cli_aln_block.h)
// from the arrays below; tests/test_aln_format.py holds the same arrays and
// compares the file with mini_parallel_amd/alnfile.py, the format's owner.
#include <cstdio>

#include "cli_aln_block.h"

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    const uint32_t M = 0, I = 1, D = 2, S = 4;
    std::vector<uint8_t> out;

    // reads 3..4, first in the file; read 4 did not align: no ops, ref_pos -1
    const int64_t b_ref[] = {70000, -1};
    const int32_t b_score[] = {77, 0}, b_nm[] = {2, 0};
    const int16_t b_ei[] = {149, -1}, b_ej[] = {290, -1};
    const uint32_t b_off[] = {0, 3, 3};
    const uint32_t b_ops[] = {5u << 4 | S, 140u << 4 | M, 5u << 4 | S};
    append_aln_block(out, 3, 2, b_ref, b_score, b_nm, b_off, b_ei, b_ej, b_ops, 3);

    // reads 0..2, second in the file
    const int64_t a_ref[] = {1000, 2001, 3002};
    const int32_t a_score[] = {300, 251, 12}, a_nm[] = {0, 3, 1};
    const int16_t a_ei[] = {149, 148, 9}, a_ej[] = {149, 299, 30};
    const uint32_t a_off[] = {0, 1, 4, 6};
    const uint32_t a_ops[] = {150u << 4 | M, 100u << 4 | M, 2u << 4 | I, 47u << 4 | M, 6u << 4 | M, 144u << 4 | S};
    append_aln_block(out, 0, 3, a_ref, a_score, a_nm, a_off, a_ei, a_ej, a_ops, 6);

    // an empty block at read 5: nothing but a header
    append_aln_block(out, 5, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0);

    // reads 5..6 at the fields' limits
    const int64_t d_ref[] = {(1ll << 40) + 12345, (1ll << 40) - 1};
    const int32_t d_score[] = {2147483647, -2147483647 - 1}, d_nm[] = {-1, 2147483647};
    const int16_t d_ei[] = {-1, 32767}, d_ej[] = {-1, -32768};
    const uint32_t d_off[] = {0, 2, 3};
    const uint32_t d_ops[] = {4095u << 4 | D, 1u << 4 | M, 0xFFFFFFFFu};
    append_aln_block(out, 5, 2, d_ref, d_score, d_nm, d_off, d_ei, d_ej, d_ops, 3);

    FILE* f = fopen(argv[1], "wb");
    if (!f || fwrite(out.data(), 1, out.size(), f) != out.size() || fclose(f) != 0) return 1;
    return 0;
}
