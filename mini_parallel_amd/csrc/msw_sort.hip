// msw_sort.hip -- a stable device-wide key-value radix sort (msw_sort_pairs_device,
// include/msw.h "Sorting and duplicates"): u64 keys, u32 values, LSD, 8 bits a
// pass, ceil(key_bits / 8) passes that ping-pong between the caller's arrays and
// one temporary pair; an odd pass count ends with one copy back.
//
// A pass is three steps, all enqueued on the caller's stream.  No block ever
// waits for another: the steps are separate launches.
//  1. sort_hist_kernel, one block per tile of kSortTile keys: per-wave private
//     LDS counters (LDS atomics: a count does not depend on their order), summed
//     over the block's four waves into counts[digit * tiles + tile], digit-major,
//     so that one exclusive scan of the whole array gives every (digit, tile)
//     run its place in the output.
//  2. scan_in_place (msw_aln.hip) over the 256 x tiles counts.
//  3. sort_scatter_kernel, one block per tile.  Wave w owns elements
//     [1024 w, 1024 (w + 1)) of the tile and takes them in 16 rounds of 64
//     consecutive keys, so rounds and waves are in input order.  In a round,
//     eight ballots (one per digit bit) give each lane the mask of the lanes
//     that hold its digit; its rank among them is the population count of that
//     mask below the lane, and the mask's lowest lane adds the mask's size to
//     the wave's counter of that digit in LDS -- after every lane has read the
//     counter's earlier value, which is the rank of the round among the wave's
//     earlier rounds.  No rank comes from an atomic.  Thread d then turns the
//     four waves' counts of digit d into offsets in wave order and the block
//     scans the digit totals, so every key knows its place in the sorted tile;
//     the keys go there in LDS, and the block reads the tile back in order:
//     thread t stores positions t, t + 256, ..., so the run of a digit leaves
//     as contiguous stores at counts[digit, tile] + its rank.  The values follow
//     through the same LDS bytes once the keys have left.
//
// LDS and occupancy.  kSortTile = 4096: the exchange holds 4096 x 8 = 32 KiB
// (the values reuse its first 16 KiB), the wave counters 4 x 256 x 4 = 4 KiB,
// the digit starts and global offsets 2 KiB, the block scan 16 bytes: 38 KiB +
// 16, four blocks in a CU's 160 KiB, i.e. four waves per SIMD, enough to hide
// the tile's one load and one store phase behind the other blocks' ranking.  A
// tile of 8192 would leave two blocks per CU; a tile of 2048 doubles the
// counts array (256 words per tile: 6 % of a pass's traffic at 4096) and its scan.
// Registers: 16 keys (32 VGPRs) or, once those are in LDS, 16 values; 16 places
// packed two a word (8) and 16 digits packed four a word (4): under 128, which
// four waves per SIMD allow.
#include <algorithm>

#include "msw_kernels.h"

namespace msw {
namespace {

constexpr int kSortThreads = 256;
constexpr int kSortWaves = kSortThreads / 64;
constexpr int kSortItems = (int)kSortTile / kSortThreads;       // 16 keys per thread
constexpr uint32_t kSortWaveSpan = kSortTile / kSortWaves;      // 1024 consecutive keys per wave
static_assert(kSortItems * kSortThreads == (int)kSortTile && kSortItems * 64 == (int)kSortWaveSpan, "tile shape");
constexpr uint32_t kRadix = 256;
static_assert(kRadix == kSortThreads, "thread d owns digit d");

__global__ __launch_bounds__(kSortThreads) void sort_hist_kernel(const uint64_t* __restrict__ keys, uint64_t n,
                                                                 uint32_t shift, uint32_t dmask,
                                                                 uint32_t* __restrict__ counts, uint32_t tiles) {
    __shared__ uint32_t wcnt[kSortWaves][kRadix];
    const uint32_t tid = threadIdx.x, w = tid >> 6;
#pragma unroll
    for (int k = 0; k < kSortWaves; ++k) wcnt[k][tid] = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * kSortTile;
    const uint32_t tile_n = (uint32_t)std::min<uint64_t>(kSortTile, n - base);
#pragma unroll
    for (int k = 0; k < kSortItems; ++k) {
        const uint32_t e = (uint32_t)k * kSortThreads + tid;
        if (e < tile_n) atomicAdd(&wcnt[w][(uint32_t)(keys[base + e] >> shift) & dmask], 1u);
    }
    __syncthreads();
    uint32_t sum = 0;
#pragma unroll
    for (int k = 0; k < kSortWaves; ++k) sum += wcnt[k][tid];
    counts[(uint64_t)tid * tiles + blockIdx.x] = sum;
}

template <bool kVals>
__global__ __launch_bounds__(kSortThreads) void sort_scatter_kernel(const uint64_t* __restrict__ kin,
                                                                    const uint32_t* __restrict__ vin,
                                                                    uint64_t* __restrict__ kout,
                                                                    uint32_t* __restrict__ vout, uint64_t n,
                                                                    uint32_t shift, uint32_t dmask,
                                                                    const uint32_t* __restrict__ offs,
                                                                    uint32_t tiles) {
    __shared__ uint64_t xch[kSortTile];
    __shared__ uint32_t wcnt[kSortWaves][kRadix];
    __shared__ uint32_t dstart[kRadix];  // where the digit's run starts in the sorted tile
    __shared__ uint32_t gdelta[kRadix];  // the run's place in the output minus dstart, modulo 2^32
    __shared__ uint32_t wsum[kSortWaves];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
#pragma unroll
    for (int k = 0; k < kSortWaves; ++k) wcnt[k][tid] = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * kSortTile;
    const uint32_t tile_n = (uint32_t)std::min<uint64_t>(kSortTile, n - base);
    const uint64_t below_me = (1ull << lane) - 1ull;

    uint64_t key[kSortItems];
    uint32_t val[kSortItems];
    uint32_t place[kSortItems / 2] = {};  // two 16-bit places a word: a place is below 4096
    const auto place_of = [&](int k) { return place[k >> 1] >> (16 * (k & 1)) & 0xFFFFu; };
    const auto set_place = [&](int k, uint32_t v) {
        place[k >> 1] = (place[k >> 1] & (0xFFFF0000u >> (16 * (k & 1)))) | v << (16 * (k & 1));
    };
#pragma unroll
    for (int k = 0; k < kSortItems; ++k) {
        const uint32_t e = w * kSortWaveSpan + (uint32_t)k * 64u + lane;
        key[k] = e < tile_n ? kin[base + e] : 0ull;
    }
    // ranks inside the wave, round by round
#pragma unroll
    for (int k = 0; k < kSortItems; ++k) {
        const uint32_t e = w * kSortWaveSpan + (uint32_t)k * 64u + lane;
        const bool valid = e < tile_n;
        const uint32_t d = (uint32_t)(key[k] >> shift) & dmask;
        uint64_t peers = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const uint64_t m = __ballot(bit);
            peers &= bit ? m : ~m;
        }
        const uint32_t before = (uint32_t)__popcll(peers & below_me);
        const uint32_t prior = wcnt[w][d];
        __builtin_amdgcn_wave_barrier();  // every lane has read the counter before the mask's first lane moves it
        if (valid && before == 0) wcnt[w][d] = prior + (uint32_t)__popcll(peers);
        __builtin_amdgcn_wave_barrier();
        set_place(k, prior + before);
    }
    __syncthreads();
    // digit `tid`: the waves' counts become offsets in wave order, the totals a block-wide exclusive scan
    {
        uint32_t run = 0;
#pragma unroll
        for (int k = 0; k < kSortWaves; ++k) {
            const uint32_t c = wcnt[k][tid];
            wcnt[k][tid] = run;
            run += c;
        }
        uint32_t inc = run;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t t = __shfl_up(inc, off, 64);
            if (lane >= (uint32_t)off) inc += t;
        }
        if (lane == 63) wsum[w] = inc;
        __syncthreads();
        uint32_t start = inc - run;
#pragma unroll
        for (int k = 0; k < kSortWaves; ++k)
            if ((uint32_t)k < w) start += wsum[k];
        dstart[tid] = start;
        gdelta[tid] = offs[(uint64_t)tid * tiles + blockIdx.x] - start;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kSortItems; ++k) {
        const uint32_t e = w * kSortWaveSpan + (uint32_t)k * 64u + lane;
        const uint32_t d = (uint32_t)(key[k] >> shift) & dmask;
        set_place(k, place_of(k) + dstart[d] + wcnt[w][d]);  // < tile_n for a valid key
        if (e < tile_n) xch[place_of(k)] = key[k];
    }
    // the values are asked for now that the keys' registers are free; they arrive while the keys leave
    if (kVals) {
#pragma unroll
        for (int k = 0; k < kSortItems; ++k) {
            const uint32_t e = w * kSortWaveSpan + (uint32_t)k * 64u + lane;
            val[k] = e < tile_n ? vin[base + e] : 0u;
        }
    }
    __syncthreads();
    uint32_t digit[kSortItems / 4] = {};  // of the key at position k * 256 + tid, a byte each: its place in the output
#pragma unroll
    for (int k = 0; k < kSortItems; ++k) {
        const uint32_t i = (uint32_t)k * kSortThreads + tid;
        if (i < tile_n) {
            const uint64_t x = xch[i];
            const uint32_t d = (uint32_t)(x >> shift) & dmask;
            digit[k >> 2] |= d << (8 * (k & 3));
            kout[gdelta[d] + i] = x;
        }
    }
    if (kVals) {
        uint32_t* xv = reinterpret_cast<uint32_t*>(xch);
        __syncthreads();  // the keys have left the exchange
#pragma unroll
        for (int k = 0; k < kSortItems; ++k) {
            const uint32_t e = w * kSortWaveSpan + (uint32_t)k * 64u + lane;
            if (e < tile_n) xv[place_of(k)] = val[k];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kSortItems; ++k) {
            const uint32_t i = (uint32_t)k * kSortThreads + tid;
            if (i < tile_n) vout[gdelta[digit[k >> 2] >> (8 * (k & 3)) & 255u] + i] = xv[i];
        }
    }
}

// the copy back after an odd number of passes (a kernel: the sort may be captured into a graph as it is)
__global__ __launch_bounds__(256) void sort_copy_kernel(const uint64_t* __restrict__ kin, const uint32_t* __restrict__ vin,
                                                        uint64_t* __restrict__ kout, uint32_t* __restrict__ vout,
                                                        uint64_t n) {
    const uint64_t step = (uint64_t)gridDim.x * 256u;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += step) {
        kout[i] = kin[i];
        if (vin) vout[i] = vin[i];
    }
}

uint64_t up256(uint64_t b) { return (b + 255) & ~(uint64_t)255; }
uint64_t scan_tiles(uint64_t c) { return (c + kAlnScanTile - 1) / kAlnScanTile; }
uint64_t sort_tiles(uint64_t n) { return (n + kSortTile - 1) / kSortTile; }

}  // namespace

uint64_t sort_tmp_bytes(uint64_t n, bool vals) {
    const uint64_t counts = kRadix * sort_tiles(n);
    uint64_t scan_words = 0;
    for (uint64_t c = scan_tiles(counts); c > 1; c = scan_tiles(c)) scan_words += c;
    return up256(n * 8) + (vals ? up256(n * 4) : 0) + up256(counts * 4) + up256(scan_words * 4);
}

hipError_t launch_sort_pairs(uint64_t* keys, uint32_t* vals, uint64_t n, uint32_t key_bits, void* tmp,
                             hipStream_t st) {
    if (n == 0) return hipSuccess;
    if (key_bits < 1 || key_bits > 64 || n > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const uint32_t tiles = (uint32_t)sort_tiles(n);
    const uint64_t counts_n = (uint64_t)kRadix * tiles;
    uint8_t* at = static_cast<uint8_t*>(tmp);
    uint64_t* keys2 = reinterpret_cast<uint64_t*>(at);
    at += up256(n * 8);
    uint32_t* vals2 = vals ? reinterpret_cast<uint32_t*>(at) : nullptr;
    at += vals ? up256(n * 4) : 0;
    uint32_t* counts = reinterpret_cast<uint32_t*>(at);
    at += up256(counts_n * 4);
    uint32_t* scan_tmp = reinterpret_cast<uint32_t*>(at);

    uint64_t *kin = keys, *kout = keys2;
    uint32_t *vin = vals, *vout = vals2;
    for (uint32_t shift = 0; shift < key_bits; shift += 8) {
        const uint32_t dmask = key_bits - shift >= 8 ? 255u : (1u << (key_bits - shift)) - 1u;
        hipLaunchKernelGGL(sort_hist_kernel, dim3(tiles), dim3(kSortThreads), 0, st, (const uint64_t*)kin, n, shift,
                           dmask, counts, tiles);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = scan_in_place(counts, counts_n, scan_tmp, st);
        if (e != hipSuccess) return e;
        if (vals)
            hipLaunchKernelGGL(sort_scatter_kernel<true>, dim3(tiles), dim3(kSortThreads), 0, st,
                               (const uint64_t*)kin, (const uint32_t*)vin, kout, vout, n, shift, dmask,
                               (const uint32_t*)counts, tiles);
        else
            hipLaunchKernelGGL(sort_scatter_kernel<false>, dim3(tiles), dim3(kSortThreads), 0, st,
                               (const uint64_t*)kin, (const uint32_t*)nullptr, kout, (uint32_t*)nullptr, n, shift,
                               dmask, (const uint32_t*)counts, tiles);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        std::swap(kin, kout);
        std::swap(vin, vout);
    }
    if (kin != keys) {
        const unsigned blocks = (unsigned)std::min<uint64_t>((n + 255) / 256, 1u << 16);
        hipLaunchKernelGGL(sort_copy_kernel, dim3(blocks), dim3(256), 0, st, (const uint64_t*)kin,
                           (const uint32_t*)vin, keys, vals, n);
        return hipGetLastError();
    }
    return hipSuccess;
}

}  // namespace msw
