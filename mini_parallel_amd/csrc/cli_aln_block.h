// cli_aln_block.h -- one block of an `.aln` file (the format's
// owner is mini_parallel_amd/alnfile.py).  Little-endian host; no GPU headers.
//
//   header, 32 B   u32 magic "MSWA", u32 version = 1, u64 first_read,
//                  u32 n_reads, u32 n_ops, 8 B zero
//   n_reads x 24 B i64 ref_pos, i32 score, i32 nm, u32 n_ops, i16 end_i, i16 end_j
//   n_ops x u32    packed ops in read order
#pragma once

#include <cstdint>
#include <cstring>
#include <vector>

// Appends the block of reads first_read .. first_read + n to `out`.  off[i] ..
// off[i + 1] are read i's ops within `ops` (n + 1 offsets; not read when n is
// 0); n_ops = off[n] is the block's op count.
inline void append_aln_block(std::vector<uint8_t>& out, uint64_t first_read, uint64_t n, const int64_t* ref_pos,
                             const int32_t* score, const int32_t* nm, const uint32_t* off, const int16_t* end_i,
                             const int16_t* end_j, const uint32_t* ops, uint64_t n_ops) {
    const size_t at = out.size();
    out.resize(at + 32 + n * 24 + n_ops * 4);
    uint8_t* b = out.data() + at;
    const uint32_t head[4] = {0x4157534Du /* "MSWA" */, 1u, (uint32_t)n, (uint32_t)n_ops};
    memset(b, 0, 32);
    memcpy(b, head, 8);
    memcpy(b + 8, &first_read, 8);
    memcpy(b + 16, head + 2, 8);
    uint8_t* q = b + 32;
    for (uint64_t i = 0; i < n; ++i, q += 24) {
        const uint32_t read_ops = off[i + 1] - off[i];
        memcpy(q, ref_pos + i, 8);
        memcpy(q + 8, score + i, 4);
        memcpy(q + 12, nm + i, 4);
        memcpy(q + 16, &read_ops, 4);
        memcpy(q + 20, end_i + i, 2);
        memcpy(q + 22, end_j + i, 2);
    }
    if (n_ops) memcpy(q, ops, n_ops * 4);
}
