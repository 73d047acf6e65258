// cli_aln_block.h -- one block of an `.aln` file (the format's
// owner is mini_parallel_amd/alnfile.py).  Little-endian host; no GPU headers.
//
//   header, 32 B   u32 magic "MSWA", u32 version = 1, u64 first_read,
//                  u32 n_reads, u32 n_ops, u32 flags, 4 B zero
//   n_reads x 24 B i64 ref_pos, i32 score, i32 nm, u32 n_ops, i16 end_i, i16 end_j
//   n_ops x u32    packed ops in read order
//   flags bit 0:   n_reads x u8 strand (0 / 1), zero-padded to a multiple of 4 B
//   flags bit 1:   n_reads x u8 mapq (0 .. 60), zero-padded to a multiple of 4 B,
//                  then n_reads x i32 sub_score
#pragma once

#include <cstdint>
#include <cstring>
#include <vector>

// Appends the block of reads first_read .. first_read + n to `out`.  off[i] ..
// off[i + 1] are read i's ops within `ops` (n + 1 offsets; not read when n is
// 0); n_ops = off[n] is the block's op count.  With `strand` (n bytes, 0 / 1)
// the block carries flag bit 0 and the strand bytes; without it the block is
// byte for byte the unflagged one.  With `mapq` and `sub_score` (n each, both or
// neither) the block carries flag bit 1 and both arrays after the strand bytes.
inline void append_aln_block(std::vector<uint8_t>& out, uint64_t first_read, uint64_t n, const int64_t* ref_pos,
                             const int32_t* score, const int32_t* nm, const uint32_t* off, const int16_t* end_i,
                             const int16_t* end_j, const uint32_t* ops, uint64_t n_ops,
                             const uint8_t* strand = nullptr, const uint8_t* mapq = nullptr,
                             const int32_t* sub_score = nullptr) {
    const size_t at = out.size();
    const size_t strand_bytes = strand ? (size_t)((n + 3) / 4 * 4) : 0;
    const size_t mapq_pad = mapq ? (size_t)((n + 3) / 4 * 4) : 0, mapq_bytes = mapq ? mapq_pad + n * 4 : 0;
    out.resize(at + 32 + n * 24 + n_ops * 4 + strand_bytes + mapq_bytes);
    uint8_t* b = out.data() + at;
    const uint32_t head[4] = {0x4157534Du /* "MSWA" */, 1u, (uint32_t)n, (uint32_t)n_ops};
    const uint32_t flags = (strand ? 1u : 0u) | (mapq ? 2u : 0u);
    memset(b, 0, 32);
    memcpy(b, head, 8);
    memcpy(b + 8, &first_read, 8);
    memcpy(b + 16, head + 2, 8);
    memcpy(b + 24, &flags, 4);
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
    q += n_ops * 4;
    if (strand_bytes) {
        memset(q, 0, strand_bytes);
        memcpy(q, strand, n);
        q += strand_bytes;
    }
    if (mapq_bytes) {
        memset(q, 0, mapq_pad);
        memcpy(q, mapq, n);
        memcpy(q + mapq_pad, sub_score, n * 4);
    }
}
