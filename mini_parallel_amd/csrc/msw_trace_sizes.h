// msw_trace_sizes.h -- host arithmetic of the traceback launches (internal;
// plain C++, no HIP, so tools/trace_long_sizes.cpp checks it on any host).
#pragma once
#include <stdint.h>

namespace msw {

constexpr uint32_t kTraceStripR = 6;              // rows per lane: strips of 64 * 6 = 384 rows
constexpr uint32_t kTraceLongLimit = 32767;       // = kMaxLongLen
constexpr uint64_t kTraceSlabBudget = 256ull << 20;  // global scratch of one traceback launch
constexpr uint32_t kTraceLongLdsOps = 4096;       // reverse ops kept in LDS (16 KiB); more: the block's scratch

// The grid of a traceback launch whose blocks need `block_bytes` of global
// scratch each: what the CUs hold at once, what the budget holds, at least one
// block; block_bytes == 0 is one block per pair.  `fixed` (MSW_TRACE_BLOCKS)
// caps it further.
inline uint64_t trace_grid_cap(uint64_t n_pairs, uint64_t resident, uint64_t block_bytes, uint64_t fixed) {
    uint64_t blocks = n_pairs;
    if (block_bytes) {
        uint64_t fit = kTraceSlabBudget / block_bytes;
        if (fit < 1) fit = 1;
        const uint64_t cap = resident < fit ? resident : fit;
        if (cap < blocks) blocks = cap;
    }
    if (fixed && fixed < blocks) blocks = fixed;
    return blocks;
}

// sw_trace_long_kernel (msw_trace_long.hip): LDS and per-block scratch for
// bounds max_rows x max_cols (each 1..kTraceLongLimit).
//   scratch = [checkpoint rows | strip slab | reverse ops]
//   checkpoint rows: (strips - 1) x ckpt_cols i32, x2 affine (H then F);
//     ckpt_cols = max_cols rounded up to 64, + 128: lane 0 loads whole
//     64-column blocks up to step max_cols + 62
//   strip slab: 64 R rows x slab_w direction words (16 / 8 columns per word)
//   reverse ops: ops_cap words when they do not fit LDS
// Worst bounds (32767 x 32767, affine): 85 rows x 32896 x 8 B = 22.4 MB,
// 384 x 4096 x 4 B = 6.3 MB, 65534 x 4 B = 0.3 MB: 28.9 MB per block, 9 blocks
// in the 256 MiB budget.
struct TraceLongLayout {
    uint32_t rows_per_lane;   // R
    uint32_t strips;          // ceil(max_rows / 64 R)
    uint32_t ckpt_cols;
    uint32_t slab_w;          // direction words per slab row
    uint32_t ops_cap;         // min(cigar_stride, max_rows + max_cols)
    uint32_t ops_in_lds;
    uint32_t win_bytes;       // LDS: [64 pad | max_cols bytes | 64 pad], rounded to 16
    uint32_t lds_bytes;       // win_bytes + the ops when they are in LDS
    uint64_t slab_off, ops_off;  // byte offsets in a block's scratch
    uint64_t block_bytes;
};

inline TraceLongLayout trace_long_layout(bool affine, uint32_t max_rows, uint32_t max_cols, uint32_t cigar_stride) {
    TraceLongLayout l;
    uint32_t r = (max_rows + 63u) / 64u;
    l.rows_per_lane = r < 1 ? 1 : (r > kTraceStripR ? kTraceStripR : r);
    const uint32_t strip_rows = 64u * l.rows_per_lane;
    l.strips = max_rows ? (max_rows + strip_rows - 1) / strip_rows : 1;
    l.ckpt_cols = ((max_cols + 63u) & ~63u) + 128u;
    const uint32_t cpw = affine ? 8u : 16u;
    l.slab_w = (max_cols + cpw - 1) / cpw;
    if (l.slab_w < 1) l.slab_w = 1;
    const uint64_t most = (uint64_t)max_rows + max_cols;  // the walk emits at most rows + cols ops
    l.ops_cap = cigar_stride < most ? cigar_stride : (uint32_t)most;
    l.ops_in_lds = l.ops_cap <= kTraceLongLdsOps;
    l.win_bytes = (max_cols + 128u + 15u) & ~15u;
    l.lds_bytes = l.win_bytes + (l.ops_in_lds ? l.ops_cap * 4u : 0u);
    const uint64_t ckpt = (uint64_t)(l.strips - 1) * l.ckpt_cols * (affine ? 2u : 1u) * 4u;
    const uint64_t slab = (uint64_t)strip_rows * l.slab_w * 4u;
    l.slab_off = (ckpt + 255u) & ~(uint64_t)255u;
    l.ops_off = (l.slab_off + slab + 255u) & ~(uint64_t)255u;
    l.block_bytes = (l.ops_off + (l.ops_in_lds ? 0u : (uint64_t)l.ops_cap * 4u) + 255u) & ~(uint64_t)255u;
    return l;
}

// sw_band_kernel (msw_band.hip): one wave per block; a group of G lanes owns
// the 2G diagonals of one pair's band, so a wave carries 64 / G pairs.
//   LDS = [byte tiles | direction codes]
//   byte tiles: per group kBandTile read bytes + kBandTile window bytes, the
//     bytes of the next 64 rows' anti-diagonals (64 + G each, <= kBandTile)
//   direction codes (traced calls only): per group max_rows rows of G bytes,
//     one 4-bit code per band cell, [row][diagonal], two diagonals per byte;
//     64 / G groups x G bytes = 64 bytes per row for the block whatever w is
// A block's LDS is capped at 64 KiB, so a traced call holds
// (65536 - 1024) / 64 = 1008 rows: kBandTraceMaxRows.
constexpr uint32_t kBandMaxW = 63;
constexpr uint32_t kBandTile = 128;
constexpr uint32_t kBandTileBytes = 2u * kBandTile * 4u;  // at most four groups: 1 KiB
constexpr uint32_t kBandTraceMaxRows = (65536u - kBandTileBytes) / 64u;

// lanes per pair for half-width w: 16 (B <= 32), 32 (B <= 64), 64 (B <= 127)
inline uint32_t band_group_lanes(uint32_t w) { return w <= 15 ? 16u : (w <= 31 ? 32u : 64u); }
// dynamic LDS bytes of a launch
inline uint32_t band_lds_bytes(uint32_t max_rows, bool trace) {
    return kBandTileBytes + (trace ? 64u * max_rows : 0u);
}

}  // namespace msw
