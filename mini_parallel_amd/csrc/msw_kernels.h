// msw_kernels.h -- device-side parameter block and launchers (internal).
#pragma once
#include <cstdlib>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "msw.h"  // msw_call_params_t, msw_variant_t (Variants)

namespace msw {

// Substitution codes: a real byte b becomes b << code_shift (< 0x4000), so two
// different bytes XOR to >= 2^code_shift >= delta and min(x, delta) is exactly
// the mismatch penalty.  Sentinels XOR to >= 0x4000 with every real code and
// with each other, i.e. they always mismatch (padding never scores).
constexpr uint32_t kReadSentinel = 0x8000u;
constexpr uint32_t kWinSentinel = 0x4000u;
constexpr uint32_t kWinSentinel2 = 0x40004000u;

constexpr int kGroupLanes = 16;        // one DPP row
constexpr int kPairsPerWave = 8;       // 4 groups x 2 packed pairs
constexpr int kMaxRowsPerLane = 24;    // pairs layout, any G (17..24 in narrow groups: large batches only)
constexpr int kMaxMultiKR = 16;        // sw_multi_kernel's rows-per-lane range
constexpr int kMaxReadLen = 384;       // 16 x 24
constexpr int kMaxWinLen = 4096;
constexpr int kLead = 32;
// Pairs with a read > kMaxReadLen or a window > kMaxWinLen go to the long-pair
// kernel (msw_long.hip): i32 cells, any length up to kMaxLongLen (the i16
// best-cell coordinates of msw_out_t).
constexpr int kMaxLongLen = 32767;
constexpr int kLongMaxR = 8;           // rows per lane; strips of 64 * R rows              // sentinel words in front of each window stream

// u32 words per lane-group stream: kLead + (max_win + 31) steps rounded to even
// + 4 lookahead,
// rounded so that the four groups of a wave start 16 banks apart (== 16 mod 32).
inline uint32_t stream_stride(uint32_t max_win_len) {
    uint32_t words = kLead + max_win_len + 2 * kGroupLanes + 5;
    words = (words + 31u) & ~31u;
    return words + 16u;
}

struct SwParams {
    const uint8_t* reads;
    const uint8_t* wins;
    const uint16_t* read_len;
    const uint16_t* win_len;
    const uint32_t* order;    // kernel slot -> pair index; nullptr = identity
    int32_t* score;
    int16_t* end_i;           // nullptr unless coordinates are wanted
    int16_t* end_j;
    uint64_t read_stride;
    uint64_t win_stride;
    uint32_t n_slots;
    uint32_t lds_stride;      // u32 words per lane-group window stream
    uint32_t code_shift;
    uint32_t win_vec;         // 1: win_stride % 16 == 0 and wins 16-byte aligned
    uint32_t read_vec;        // 1: read_stride % 4 == 0 and reads 4-byte aligned
    uint32_t pairs_blocks;    // mixed grid: leading blocks that use the pairs layout
    uint32_t slot_base;       // first slot index of this (sub)grid when order == nullptr
    uint32_t match2;          // match, duplicated into both u16 halves
    uint32_t delta2;          // match - mismatch
    uint32_t gap2;            // linear: gap penalty; affine: gap_extend
    uint32_t open_ext2;       // affine: gap_open + gap_extend + K
    uint32_t bias2;           // affine: K = 256 + gap_extend (see msw_kernels.hip)
    uint64_t* trace;          // diagnostics (MSW_WAVE_TRACE): 4 words per block, or nullptr
    uint32_t group_lanes;     // G: lanes per lane group (8..16)
    uint32_t groups;          // lane groups per wave = 64 / G (lanes past groups * G idle)
    // f16 fast path (ACGT windows): cell values H * 2^-11 as packed f16.
    uint32_t f16_ok;          // 1: the scheme and this launch's bound fit (msw_runtime.cpp)
    uint32_t f16_hi;          // high byte of f16(+match) | high byte of f16(mismatch) << 8
    uint32_t f16_ngap2;       // f16(-gap) (linear) / f16(-gap_extend) (affine), both halves
    uint32_t f16_noe2;        // affine: f16(-(gap_open + gap_extend)), both halves
    // Results by slot (needs order): score[out_slot_base + slot] instead of
    // score[pair], so each wave's stores are contiguous; the caller restores
    // pair order (msw_runtime.cpp: the host drain, or launch_gather_results).
    uint32_t out_by_slot;
    uint32_t out_slot_base;
    // Optional lengths in slot order, read_len | win_len << 16 per slot (index
    // out_slot_base + slot): planned batches read them contiguously instead of
    // gathering two 2-byte lengths per pair through the order array.
    const uint32_t* slot_lens;
    // Long pairs (sw_long_kernel, msw_long.hip): per-block boundary rows,
    // long_cols i32 columns each (x2 for affine: H then F).
    int32_t* long_scratch;
    uint32_t long_cols;
    // sw_long_kernel work queue (zeroed u32, or null): with fewer blocks than
    // slots, a block that finishes a slot takes the next unclaimed one
    // (gridDim.x + counter) instead of striding by gridDim.x
    uint32_t* long_next;
    // Genome-resident windows (instances with GEN = true: pairs layout, KR <=
    // 16): the window of pair p is win_src[win_pos[p] ..], win_len[p] bytes
    // (clipped by the host), read straight from the resident genome at any
    // alignment instead of from a cut slab (wins / win_stride unused); the
    // genome allocation extends >= 20 bytes past every window (kGenomePad).
    const uint8_t* win_src;
    const int64_t* win_pos;
};

// f16 bits of the cell value v * 2^-11 (|v| < 2048: exact, normal or zero).
inline uint32_t f16_cell_bits(int32_t v) {
    if (v == 0) return 0u;
    const uint32_t sign = v < 0 ? 0x8000u : 0u;
    uint32_t a = (uint32_t)(v < 0 ? -v : v);
    int e = 31 - __builtin_clz(a);  // a = 1.f * 2^e
    const uint32_t mant = (a << (10 - e)) & 0x3FFu;
    return sign | ((uint32_t)(e + 4) << 10) | mant;  // exponent bias 15, scale 2^-11
}

// Packed rows per lane for a read-length bound: ceil(m / 16) in the pairs
// layout, ceil(m / 32) in the split layout (each packed row holds two rows).
inline int rows_per_lane(uint32_t max_read_len, bool split, uint32_t group_lanes = kGroupLanes) {
    const uint32_t per = split ? 2 * group_lanes : group_lanes;
    int kr = (int)((max_read_len + per - 1) / per);
    return kr < 1 ? 1 : kr;
}

// Pairs one wave scores: two per group (pairs layout) or one (split).
__host__ __device__ inline uint32_t pairs_per_wave(bool split, uint32_t groups) { return split ? groups : 2 * groups; }

// 16-byte vector loads of the window rows are legal.
inline uint32_t vec_ok(const void* base, uint64_t stride) {
    return (stride >= 16 && stride % 16 == 0 && ((uintptr_t)base & 15) == 0) ? 1u : 0u;
}

// Dword loads of the read rows are legal (every row starts 4-byte aligned
// and holds a whole number of dwords).
inline uint32_t read_vec_ok(const void* base, uint64_t stride) {
    return (stride >= 4 && stride % 4 == 0 && ((uintptr_t)base & 3) == 0) ? 1u : 0u;
}

// Dynamic LDS bytes for one 64-lane block (one window stream per group).
inline size_t lds_bytes(uint32_t lds_stride, uint32_t groups) { return (size_t)groups * lds_stride * sizeof(uint32_t); }

enum class Layout { kPairs, kSplit, kMixed };

// Length-bucketed grid (sw_multi_kernel): bucket b holds the slots
// [slot_begin[b], slot_begin[b] + count[b]) of the order array, all with
// rows_per_lane(read length) <= kr[b], and owns blocks
// [b ? block_end[b - 1] : 0, block_end[b]) of ONE launch (pairs layout, G = 16,
// 8 pairs per block).  Buckets are listed heaviest first, so the long waves
// are dispatched first and the short ones fill the tail.
constexpr int kMaxBuckets = 16;
struct MultiTable {
    uint32_t n_buckets;
    uint32_t block_end[kMaxBuckets];
    uint32_t slot_begin[kMaxBuckets];
    uint32_t count[kMaxBuckets];
    uint32_t kr[kMaxBuckets];
    uint32_t lds_stride[kMaxBuckets];
    uint32_t f16_ok[kMaxBuckets];
};

hipError_t launch_sw(const SwParams& p, bool affine, bool coords, uint32_t max_read_len, Layout layout,
                     hipStream_t stream);

// Blocks (waves) per CU of the instance launch_sw / launch_sw_multi would run
// for these arguments (its VGPRs and p's LDS), without launching; the query
// loads the instance's code object (HIP loads a module on its first use).
// 0 on error.  cut_blocks_per_cu: the same for the window cut kernel.
int sw_blocks_per_cu(const SwParams& p, bool affine, bool coords, uint32_t max_read_len, Layout layout);
int sw_multi_blocks_per_cu(const SwParams& p, const MultiTable& t, bool affine, bool coords);
int cut_blocks_per_cu();

// All buckets of `t` in one launch; p.order is required (slot -> pair), the
// per-bucket fields of p (n_slots, lds_stride, f16_ok) come from the table.
hipError_t launch_sw_multi(const SwParams& p, const MultiTable& t, bool affine, bool coords,
                           hipStream_t stream);

// Genome-resident windows: out[p * ws ..] = genome[pos[p], pos[p] + len),
// len = want[p] clipped to the genome (0 outside it), zero-padded to ws;
// out_len[p] = len when out_len != nullptr.  ws % 16 == 0, genome allocation
// padded by >= 20 bytes past its end.
constexpr uint32_t kGenomePad = 64;
// The window rule (include/msw.h, "The window of a pair"), in one place:
// window p is genome[pos, pos + len), len = the requested length clipped at
// the genome end; a position outside [0, glen) -- negative ones wrap past
// glen -- is an empty window.
__host__ __device__ inline uint32_t genome_window_len(uint64_t glen, int64_t pos, uint32_t want) {
    const uint64_t start = (uint64_t)pos;
    const uint64_t room = start < glen ? glen - start : 0;
    return (uint32_t)(want < room ? want : room);
}
// The requested length of a device-resident read's window: `window`, or
// 2 x read length capped at kMaxWinLen when window is 0.
__host__ __device__ inline uint32_t reads_window_want(uint32_t window, uint32_t rlen) {
    return window ? window : (2u * rlen < (uint32_t)kMaxWinLen ? 2u * rlen : (uint32_t)kMaxWinLen);
}
hipError_t launch_cut_windows(const uint8_t* genome, uint64_t glen, const int64_t* pos, const uint16_t* want,
                              uint8_t* out, uint16_t* out_len, uint32_t ws, uint64_t n, hipStream_t stream);
// Same, for device-resident reads: want = window, or 2 x rlen[p] capped at
// kMaxWinLen when window is 0 (msw_align_reads_device).
hipError_t launch_cut_windows_for_reads(const uint8_t* genome, uint64_t glen, const int64_t* pos,
                                        const uint16_t* rlen, uint32_t window, uint8_t* out, uint16_t* out_len,
                                        uint32_t ws, uint64_t n, hipStream_t stream);

// dst[i] = src[inv[i]] for score (and end_i / end_j when non-null): pair
// order restored from slot-ordered results (one thread per pair, coalesced
// stores; the slot-ordered source is small enough to stay in L2).
// bytes from device memory to pinned host memory (dst: its device address),
// as a kernel on `stream` (msw_memcpy_d2h_async)
hipError_t launch_d2h_copy(void* dst, const void* src, uint64_t bytes, hipStream_t stream);
// Up to kPullRanges ranges copied by ONE kernel on `stream`: a one-chunk
// host call pulls its pinned rows and metadata into the slot's device
// buffers on its compute stream (no DMA engine, no cross-queue event between
// the upload and the scoring launch).  Sources are device addresses of
// pinned host memory; each range's source and destination share their
// alignment mod 16 (16-byte loads between a byte head and tail).
constexpr int kPullRanges = 3;
struct PullRanges {
    uint8_t* dst[kPullRanges];
    const uint8_t* src[kPullRanges];
    uint64_t bytes[kPullRanges];  // 0: unused
};
hipError_t launch_pull_copy(const PullRanges& r, hipStream_t stream);
hipError_t launch_gather_results(const uint32_t* inv, const int32_t* src_score, const int16_t* src_i,
                                 const int16_t* src_j, int32_t* score, int16_t* end_i, int16_t* end_j, uint64_t n,
                                 hipStream_t stream);

// Long pairs: R = rows per lane for a read-length bound (the fewest strips of
// <= 512 rows, rows spread evenly over them); scratch columns per block; LDS bytes.
int long_rows_per_lane(uint32_t max_read_len);
uint32_t long_scratch_cols(uint32_t max_win_len);
// Blocks (waves) of the long-pair launch one CU holds at once (registers and
// LDS of the kernel instance these bounds select).
int long_blocks_per_cu(bool affine, bool coords, uint32_t max_read_len, uint32_t max_win_len);
size_t long_lds_bytes(uint32_t max_win_len);
// One wave per pair, `blocks` blocks striding over p.n_slots (order / slot
// results as in launch_sw).  p.long_scratch must hold blocks x long_cols
// (x2 affine) i32 when the read bound exceeds 64 * R rows.
hipError_t launch_sw_long(const SwParams& p, bool affine, bool coords, uint32_t max_read_len, uint32_t max_win_len,
                          uint32_t blocks, hipStream_t stream);

// Traceback (sw_trace_kernel, msw_trace.hip): one wave per pair refills the
// rectangle rows 0..end_i x columns 0..end_j with i32 cells, records a
// direction code per cell (2 bits linear, 4 bits affine, packed into u32
// words), and walks the codes back from the end cell.
constexpr int kTraceMaxR = 6;                    // rows per lane: 64 * 6 = kMaxReadLen
constexpr uint32_t kTraceLdsWords = 8192;        // direction words kept in LDS (32 KiB); larger rectangles: global slab
struct TraceParams {
    const uint8_t* reads;
    const uint8_t* wins;
    const uint16_t* read_len;
    const uint16_t* win_len;
    const int16_t* end_i;     // the scoring call's best cell per pair; < 0: no alignment
    const int16_t* end_j;
    int16_t* start_i;
    int16_t* start_j;
    int32_t* n_cigar;
    uint32_t* cigar;          // [n_pairs][cigar_stride]
    uint64_t read_stride;
    uint64_t win_stride;
    uint32_t cigar_stride;
    uint32_t n_slots;
    uint32_t max_rows;        // the call's length bounds: larger rectangles are not traced
    uint32_t max_cols;
    int32_t match, mismatch, gap, goe;  // gap: linear penalty / affine gap_extend; goe = gap_open + gap_extend
    uint32_t win_bytes;       // LDS layout: [window | ops | direction words]
    uint32_t ops_cap;         // run-length ops the LDS buffer holds (<= cigar_stride)
    uint32_t lds_words;       // direction words in LDS
    uint32_t* slab;           // per-block global direction words (slab_words each), or null
    uint64_t slab_words;
    uint32_t* next;           // work queue counter (zeroed), or null: one block per slot
    // Windows straight from the genome (msw_trace_reads_device): genome != null
    // replaces wins / win_len / win_stride by genome + win_pos[p] and the
    // window rule (genome_window_len over reads_window_want).
    const uint8_t* genome;
    uint64_t glen;
    const int64_t* win_pos;
    uint32_t window;
};
int trace_rows_per_lane(uint32_t max_read_len);
// direction words of a rows x cols rectangle (16 cells per word linear, 8 affine)
__host__ __device__ inline uint64_t trace_words(bool affine, uint32_t rows, uint32_t cols) {
    const uint32_t cpw = affine ? 8u : 16u;
    return (uint64_t)rows * ((cols + cpw - 1) / cpw);
}
// fills p.win_bytes / ops_cap / lds_words from the bounds; returns the dynamic LDS bytes
size_t trace_lds_layout(TraceParams& p, bool affine);
int trace_blocks_per_cu(bool affine, uint32_t max_read_len, size_t lds_bytes);
hipError_t launch_sw_trace(const TraceParams& p, bool affine, uint32_t blocks, size_t lds_bytes, hipStream_t stream);

// Alignment records (msw_aln.hip, msw_aln_pack_device): per read the genome
// coordinate, the edit distance and the soft-clipped op count; an exclusive
// prefix sum of the counts; a gather of the ops into one packed stream.
struct AlnParams {
    const uint8_t* genome;
    uint64_t glen;
    const uint8_t* reads;
    const uint16_t* read_len;
    uint64_t read_stride;
    const int64_t* win_pos;
    uint64_t n;
    const int32_t* score;
    const int16_t* end_i;
    const int16_t* start_i;
    const int16_t* start_j;
    const int32_t* n_cigar;
    const uint32_t* rows;     // the trace's [n][cigar_stride] op rows
    uint32_t cigar_stride;
    int64_t* ref_pos;
    int32_t* nm;
    uint32_t* cigar_off;      // [n + 1]
    uint32_t* cigar;
    uint64_t cigar_cap;
    uint32_t* n_overflow;
};
// Items one scan block covers: a scan of `count` items has one level per
// factor of kAlnScanTile (1 level up to the tile, 2 up to its square, ...).
constexpr uint32_t kAlnScanTile = 1024;
// Everything enqueued on `stream`; the scan's block sums are allocated and
// freed stream-ordered.
hipError_t launch_aln_pack(const AlnParams& p, hipStream_t stream);
// The scan itself: the exclusive prefix sum of data[0, count) in place,
// enqueued on `st`; tmp holds the block sums of every level (the sum, over
// c = ceil(count / kAlnScanTile), ceil(c / kAlnScanTile), ... while c > 1, of c
// words).  No block waits for another: the levels are separate launches.
hipError_t scan_in_place(uint32_t* data, uint64_t count, uint32_t* tmp, hipStream_t st);

// Pileup (msw_pileup.hip; the contract is in include/msw.h, "Pileup").  The
// state of one pileup and, for an add, one batch of records.  Channel ch of
// position pos is counts[pos * pos_mul + ch * ch_mul]: rows of eight
// (pos_mul 8, ch_mul 1) or eight planes (pos_mul 1, ch_mul glen).
constexpr uint32_t kPileupReadSlots = 32;
constexpr uint32_t kPileupReadSlotWords = 16;  // u64 words between two counters
struct PileupParams {
    const uint8_t* genome;
    uint64_t glen;
    uint32_t* counts;
    uint64_t pos_mul, ch_mul;
    uint32_t* d_all;          // [glen + 1] differences of the M-column depth, modulo 2^32
    uint32_t* d_rev;          // [glen + 1] the same for strand-1 reads
    uint32_t* mism;           // [glen] M columns whose read byte differs from the genome byte
    // reads used / skipped: kPileupReadSlots slots of two counters, each counter on a 128-byte line of its own
    // (counter c of slot s at reads[(s * 2 + c) * kPileupReadSlotWords]); a block adds to slot blockIdx % slots
    unsigned long long* reads;
    // the batch (launch_pileup_add only)
    const uint8_t* rows;
    const uint16_t* read_len;
    uint64_t row_stride;
    uint64_t n;
    const int64_t* ref_pos;
    const int32_t* nm;
    const uint32_t* cigar_off;  // [n + 1]
    const uint32_t* cigar;      // op k of the stream is cigar[k - cigar_base]
    uint32_t cigar_base;        // reads whose ops start before it are skipped
    uint64_t cigar_cap;         // reads whose ops end past it are skipped
    const uint8_t* strand;      // or null
    const uint8_t* mapq;        // or null
    uint32_t min_mapq;
    uint32_t orient;            // 1: the rows are the reads as given; a strand-1 row is read as its reverse complement
};
// u32 words of scan temporaries pileup_finish needs for a genome of glen bases
uint64_t pileup_scan_tmp_words(uint64_t glen);
hipError_t launch_pileup_add(const PileupParams& p, hipStream_t stream);
// The base-quality filter of an add (msw.h, "Base qualities"): a kernel instance of its own takes it
// beside the params, so the plain add's arguments and code stay as they are.
struct PileupQual {
    const uint8_t* quals;       // quals[n][qual_stride], rows in the order of the reads as given
    uint32_t qual_stride;
    uint32_t min_baseq;         // 1..93
    // low-quality columns: kPileupReadSlots counters, one per 128-byte line (slot s at lowq[s * kPileupReadSlotWords])
    unsigned long long* lowq;
};
hipError_t launch_pileup_add_qual(const PileupParams& p, const PileupQual& q, hipStream_t stream);
// Quality sums beside the counts (msw.h, "Quality sums and weighted genotypes"): the state of a
// MSW_PILEUP_QSUM pileup, taken beside the params by a third kernel instance.  min_baseq may be 0 here.
struct PileupQsum : PileupQual {
    uint32_t* d_q;              // [glen + 1] differences of the summed Phred values of counted M columns, modulo 2^32
    uint32_t* qmis;             // [glen] the summed Phred values of counted columns whose read byte differs from the genome byte
    uint32_t* qsum;             // [glen][4], rows of four
};
hipError_t launch_pileup_add_qsum(const PileupParams& p, const PileupQsum& q, hipStream_t stream);
// blocks per CU of pileup_add_kernel; the query loads the module
int pileup_blocks_per_cu();
// scans d_all and d_rev in place and folds them and mism into counts
hipError_t launch_pileup_finish(const PileupParams& p, uint32_t* scan_tmp, hipStream_t stream);
// the same, then one more scan over q.d_q and its fold with q.qmis into q.qsum (the quality fields of q are not read)
hipError_t launch_pileup_finish_qsum(const PileupParams& p, const PileupQsum& q, uint32_t* scan_tmp, hipStream_t stream);
// stats[4] (device): covered, depth_sum, minority_ref, max_depth of finished counts
hipError_t launch_pileup_summary(const PileupParams& p, uint32_t min_depth, unsigned long long* stats,
                                 hipStream_t stream);
// out[m][8] = the rows of positions [pos0, pos0 + m), whatever the layout
hipError_t launch_pileup_rows(const PileupParams& p, uint64_t pos0, uint64_t m, uint32_t* out, hipStream_t stream);

// Variants (msw_call.hip; the contract is in include/msw.h, "Variants").  One
// call over positions [0, m) of a counts slab: channel ch of position k is
// counts[k * pos_mul + ch * ch_mul] (both pileup layouts, or a plain [m][8]
// slab), genome[k] its byte, and `rows` >= m the rows that may be read:
// m + 1 when the slab carries a look-ahead row for depth(m), else depth(m) is 0.
constexpr uint32_t kCallTile = 256;  // positions per block, one per thread
struct CallParams {
    const uint8_t* genome;
    const uint32_t* counts;
    uint64_t pos_mul, ch_mul;
    uint64_t m, rows;
    uint64_t pos0;             // added to a record's pos
    msw_call_params_t q;
    uint32_t* tile_off;        // [tiles + 1]: per-tile record counts, scanned in place; entry `tiles` is the total
    msw_variant_t* out;        // [cap], or null with cap 0
    uint64_t cap;
    unsigned long long* n_total;  // device, or null
    // the weighted calls only (msw.h, "Quality sums and weighted genotypes"): qsum[k * 4 + c], 16-byte aligned
    const uint32_t* qsum;
    uint32_t q_scale, q_third;
};
inline uint64_t call_tiles(uint64_t m) { return (m + kCallTile - 1) / kCallTile; }
// u32 words of tile_off plus the scan's temporaries behind it
uint64_t call_tmp_words(uint64_t m);
// count pass, scan, then the emit pass when cap > 0; *n_total = the total either way.  p.tile_off holds
// call_tmp_words(m) words.
hipError_t launch_call(const CallParams& p, hipStream_t stream);
// the stages apart: msw_call_counts reads a chunk's total between the scan and the emit pass
hipError_t launch_call_count(const CallParams& p, hipStream_t stream);
hipError_t launch_call_scan(const CallParams& p, hipStream_t stream);
hipError_t launch_call_emit(const CallParams& p, hipStream_t stream);
// Every launch above runs the weighted instances when p.qsum != nullptr.

// Placing reads (msw_seed.hip; the contract is in include/msw.h).
constexpr uint32_t kSeedMaxCap = 8192;      // keys one read's LDS array holds (32 KiB)
constexpr uint32_t kSeedMaxOcc = 64;
constexpr uint64_t kSeedMaxGenome = 0xFFFF0000ull;
struct SeedParams {
    const uint32_t* off;      // the index: [4^k + 1]
    const uint32_t* pos;
    const uint8_t* reads;
    const uint8_t* rc_reads;  // the reverse complements' rows, or null: forward only
    const uint16_t* read_len;
    uint64_t read_stride;
    uint64_t rc_stride;
    uint64_t n;
    uint32_t k, band, cap, step, min_votes, window;
    int64_t* win_pos;
    uint32_t* votes;
    uint32_t* hits;
    uint8_t* flags;
};
// u32 words of scan temporaries an index of 4^k = `buckets` buckets needs
uint64_t index_scan_tmp_words(uint64_t buckets);
// Steps 1-3 of the build: off[buckets + 1] = the masked counts, scanned;
// *n_masked = the buckets over max_occ.  ev[0..3] are recorded around the
// count, the mask and the scan.
hipError_t launch_index_count(const uint8_t* genome, uint64_t glen, uint32_t k, uint32_t max_occ, uint32_t* off,
                              uint32_t* n_masked, uint32_t* scan_tmp, hipEvent_t* ev, hipStream_t st);
// Steps 4-5: pos[off[buckets]] filled (cursor: buckets words of scratch) and
// every bucket sorted ascending.  ev[0..2] around the fill and the sort.
hipError_t launch_index_fill(const uint8_t* genome, uint64_t glen, uint32_t k, const uint32_t* off, uint32_t* cursor,
                             uint32_t* pos, hipEvent_t* ev, hipStream_t st);
size_t seed_lds_bytes(uint32_t cap);
hipError_t launch_seed_reads(const SeedParams& p, hipStream_t stream);
// blocks per CU of seed_reads_kernel at this cap; the query loads the module
int seed_blocks_per_cu(uint32_t cap);

// Candidates and mapping quality (the contract is in include/msw.h).
// seed_candidates_kernel (msw_seed.hip): s is what seed_reads_kernel takes and
// its four outputs are written as that kernel writes them; sep 0 = the read's
// max(W, band), else sep >= band.  Same LDS as launch_seed_reads.
struct SeedCandParams {
    SeedParams s;
    uint32_t sep;
    int64_t* win_pos1;
    uint32_t* votes1;
    uint8_t* flags1;
};
hipError_t launch_seed_candidates(const SeedCandParams& q, hipStream_t stream);
int seed_candidates_blocks_per_cu(uint32_t cap);
// mapq_select_kernel (msw_mapq.hip).  Per read the alternate wins iff
// score_a > score: its score, end cell, win_len, strand, win_pos and oriented
// row then replace the primary's (row copy: both slabs 16-byte aligned, the one
// stride a multiple of 16); sub_score is the loser's score, cand 0 / 1, mapq the
// header's formula.  end_i / end_j (with their _a) null: score only; strand and
// oriented (with their _a) null: one strand, no row traffic; win_len null: not
// moved.
struct MapqSelectParams {
    int32_t* score;
    int16_t* end_i;
    int16_t* end_j;
    uint16_t* win_len;
    uint8_t* strand;
    uint8_t* oriented;
    int64_t* win_pos;
    const int32_t* score_a;
    const int16_t* end_i_a;
    const int16_t* end_j_a;
    const uint16_t* win_len_a;
    const uint8_t* strand_a;
    const uint8_t* oriented_a;
    const int64_t* win_pos_a;
    const uint16_t* read_len;
    uint64_t oriented_stride;
    uint64_t n;
    int32_t match;
    int32_t* sub_score;
    uint8_t* mapq;
    uint8_t* cand;
};
hipError_t launch_mapq_select(const MapqSelectParams& p, hipStream_t stream);
int mapq_blocks_per_cu();

// Both strands (msw_strand.hip; the contract is in include/msw.h).
// out[p][0, read_len[p]) = the reverse complement of read row p, zeros up to
// out_stride: every byte of every output row is written.  out 16-byte
// aligned, out_stride a multiple of 16 (else hipErrorInvalidValue, nothing
// launched); the read rows at any alignment and stride.
hipError_t launch_revcomp_rows(const uint8_t* reads, const uint16_t* read_len, uint32_t read_stride, uint64_t n,
                               uint8_t* out, uint32_t out_stride, hipStream_t stream);
// strand[p] = score_r[p] > score[p]; where it is 1 the reverse results move
// into score / end_i / end_j (the end arrays may all be null), where it is 0
// the forward read row replaces row p of `oriented` (which holds the reverse
// complements on entry), zero padded.
hipError_t launch_strand_select(const uint8_t* reads, const uint16_t* read_len, uint32_t read_stride, uint64_t n,
                                uint8_t* oriented, uint32_t oriented_stride, int32_t* score, int16_t* end_i,
                                int16_t* end_j, const int32_t* score_r, const int16_t* end_i_r,
                                const int16_t* end_j_r, uint8_t* strand, hipStream_t stream);
// blocks per CU of the two kernels (the smaller); the query loads the module
int strand_blocks_per_cu();

// smith_waterman_align restated: result must be zeroed before the launch.
hipError_t launch_compat(const uint8_t* s1, const uint8_t* s2, int32_t* result, uint64_t L,
                         uint32_t W, uint64_t G, hipStream_t stream);

}  // namespace msw
