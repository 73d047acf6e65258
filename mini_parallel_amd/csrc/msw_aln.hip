// msw_aln.hip -- alignment records from a trace (msw_aln_pack_device,
// include/msw.h "Alignment records"): genome coordinate, edit distance and a
// packed, soft-clipped CIGAR stream in place of the padded [n][cigar_stride]
// rows.
//
// Three steps, all enqueued on the caller's stream:
//  1. aln_count_kernel, one wave per read: ref_pos = win_pos + start_j, the
//     op count (leading clip + traced ops + trailing clip) into cigar_off[p],
//     and NM: the wave takes the ops in order (wave-uniform); for an M run the
//     lanes compare read[i0 + k] with genome[g0 + k], k = lane, lane + 64, ...,
//     and a ballot's popcount adds the mismatches; I and D add their lengths.
//  2. an exclusive prefix sum of cigar_off[0 .. n] in place (entry n enters as
//     0 and leaves as the total).  Per-block sums, a scan of the block sums
//     (recursing: one level per factor of kAlnScanTile), then an apply pass
//     that rescans each tile and adds its block's offset.  No block ever
//     waits for another block: the levels are separate launches.
//  3. aln_gather_kernel, one thread per packed op: a binary search in
//     cigar_off finds the op's read, consecutive threads store consecutive
//     words.  Ops at or past cigar_cap are not written.
#include <algorithm>

#include "msw_kernels.h"

namespace msw {
namespace {

constexpr int kScanThreads = 256;
constexpr int kScanItems = (int)kAlnScanTile / kScanThreads;
static_assert(kScanItems * kScanThreads == (int)kAlnScanTile, "tile = threads x items");

constexpr uint32_t kOpS = 4;  // BAM soft clip

__global__ __launch_bounds__(256) void aln_count_kernel(AlnParams p) {
    const int lane = (int)(threadIdx.x & 63u);
    const uint64_t wave = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    const uint64_t waves = (uint64_t)gridDim.x * 4u;
    if (wave == 0 && lane == 0) p.cigar_off[p.n] = 0;  // the scan turns it into the total
    for (uint64_t r = wave; r < p.n; r += waves) {
        const int32_t nc = p.n_cigar[r];
        const int si = p.start_i[r], sj = p.start_j[r], ei = p.end_i[r];
        const int rl = p.read_len[r];
        const int64_t pos = p.win_pos[r];
        // wave-uniform: every lane loaded the same words
        const bool aligned = p.score[r] > 0 && nc > 0 && si >= 0 && sj >= 0 && ei >= si && ei < rl;
        const bool over = aligned && (uint32_t)nc > p.cigar_stride;
        int64_t ref = -1;
        int32_t nm = 0;
        uint32_t count = 0;
        if (aligned) ref = pos + sj;
        if (over) nm = -1;
        if (aligned && !over) {
            const uint8_t* rd = p.reads + r * p.read_stride;
            const uint32_t* row = p.rows + r * (uint64_t)p.cigar_stride;
            int i = si;
            int64_t g = ref;
            for (int32_t q = 0; q < nc; ++q) {
                const uint32_t op = row[q];
                const int len = (int)(op >> 4);
                const uint32_t code = op & 15u;
                if (code == 0) {
                    for (int k0 = 0; k0 < len; k0 += 64) {
                        const int k = k0 + lane;
                        // the bounds hold for a trace of these inputs; anything else reads nothing
                        const bool in = k < len && i + k < rl && g + k >= 0 && (uint64_t)(g + k) < p.glen;
                        const bool diff = in && rd[i + k] != p.genome[g + k];
                        nm += (int32_t)__popcll(__ballot(diff));
                    }
                    i += len;
                    g += len;
                } else {
                    nm += len;
                    if (code == 1) i += len;
                    else g += len;
                }
            }
            count = (uint32_t)nc + (si > 0 ? 1u : 0u) + (rl - 1 - ei > 0 ? 1u : 0u);
        }
        if (lane == 0) {
            p.ref_pos[r] = ref;
            p.nm[r] = nm;
            p.cigar_off[r] = count;
            if (over) atomicAdd(p.n_overflow, 1u);
        }
    }
}

// exclusive prefix of v over the block's threads; *total = the block's sum
__device__ __forceinline__ uint32_t block_exclusive(uint32_t v, uint32_t* total) {
    __shared__ uint32_t wsum[kScanThreads / 64];
    const int lane = (int)(threadIdx.x & 63u), w = (int)(threadIdx.x >> 6);
    uint32_t inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t t = __shfl_up(inc, off, 64);
        if (lane >= off) inc += t;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    uint32_t base = 0, all = 0;
#pragma unroll
    for (int k = 0; k < kScanThreads / 64; ++k) {
        if (k < w) base += wsum[k];
        all += wsum[k];
    }
    *total = all;
    return base + inc - v;
}

// sums[b] = sum of tile b of in[0, count)
__global__ __launch_bounds__(kScanThreads) void scan_sums_kernel(const uint32_t* __restrict__ in, uint64_t count,
                                                                 uint32_t* __restrict__ sums) {
    const uint64_t base = (uint64_t)blockIdx.x * kAlnScanTile + (uint64_t)threadIdx.x * kScanItems;
    uint32_t v = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k)
        if (base + k < count) v += in[base + k];
    uint32_t total;
    (void)block_exclusive(v, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// data[0, count) -> its exclusive prefix sum per tile, plus offs[b] (the
// scanned block sums) when given; in place
__global__ __launch_bounds__(kScanThreads) void scan_apply_kernel(uint32_t* __restrict__ data, uint64_t count,
                                                                  const uint32_t* __restrict__ offs) {
    const uint64_t base = (uint64_t)blockIdx.x * kAlnScanTile + (uint64_t)threadIdx.x * kScanItems;
    uint32_t x[kScanItems], v = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
        x[k] = base + k < count ? data[base + k] : 0u;
        v += x[k];
    }
    uint32_t total;
    uint32_t run = block_exclusive(v, &total) + (offs ? offs[blockIdx.x] : 0u);
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
        if (base + k < count) data[base + k] = run;
        run += x[k];
    }
}

__global__ __launch_bounds__(256) void aln_gather_kernel(AlnParams p) {
    const uint64_t total = p.cigar_off[p.n];
    const uint64_t end = total < p.cigar_cap ? total : p.cigar_cap;
    const uint64_t step = (uint64_t)gridDim.x * 256u;
    for (uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x; k < end; k += step) {
        // the read of op k: the last r with cigar_off[r] <= k (reads without ops share their successor's offset)
        uint64_t lo = 0, hi = p.n;  // cigar_off[lo] <= k < cigar_off[hi]
        while (hi - lo > 1) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (p.cigar_off[mid] <= k) lo = mid;
            else hi = mid;
        }
        const uint64_t r = lo;
        uint32_t q = (uint32_t)(k - p.cigar_off[r]);
        const int si = p.start_i[r];
        uint32_t op;
        if (si > 0 && q == 0) {
            op = (uint32_t)si << 4 | kOpS;
        } else {
            if (si > 0) --q;
            const uint32_t nc = (uint32_t)p.n_cigar[r];
            op = q < nc ? p.rows[r * (uint64_t)p.cigar_stride + q]
                        : (uint32_t)((int)p.read_len[r] - 1 - (int)p.end_i[r]) << 4 | kOpS;
        }
        p.cigar[k] = op;
    }
}

uint64_t tiles(uint64_t count) { return (count + kAlnScanTile - 1) / kAlnScanTile; }

}  // namespace

// exclusive scan of data[0, count) in place; tmp holds the block sums of every level
hipError_t scan_in_place(uint32_t* data, uint64_t count, uint32_t* tmp, hipStream_t st) {
    const uint64_t blocks = tiles(count);
    if (blocks <= 1) {
        hipLaunchKernelGGL(scan_apply_kernel, dim3(1), dim3(kScanThreads), 0, st, data, count,
                           (const uint32_t*)nullptr);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(scan_sums_kernel, dim3((unsigned)blocks), dim3(kScanThreads), 0, st, data, count, tmp);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if ((e = scan_in_place(tmp, blocks, tmp + blocks, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(scan_apply_kernel, dim3((unsigned)blocks), dim3(kScanThreads), 0, st, data, count,
                       (const uint32_t*)tmp);
    return hipGetLastError();
}

hipError_t launch_aln_pack(const AlnParams& p, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(p.n_overflow, 0, sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    const uint64_t count = p.n + 1;  // offsets to scan
    uint64_t tmp_words = 0;
    for (uint64_t c = tiles(count); c > 1; c = tiles(c)) tmp_words += c;
    uint32_t* tmp = nullptr;
    if (tmp_words && (e = hipMallocAsync((void**)&tmp, tmp_words * sizeof(uint32_t), stream)) != hipSuccess) return e;
    // a wave per read, grid-stride past 2^20 blocks
    const uint64_t cblocks = std::min<uint64_t>((p.n + 3) / 4 + (p.n == 0), 1u << 20);
    hipLaunchKernelGGL(aln_count_kernel, dim3((unsigned)cblocks), dim3(256), 0, stream, p);
    e = hipGetLastError();
    if (e == hipSuccess) e = scan_in_place(p.cigar_off, count, tmp, stream);
    if (e == hipSuccess && p.cigar_cap && p.n) {
        // the total is known on the device only: a grid sized by what the rows can hold, striding
        const uint64_t most = std::min<uint64_t>(p.cigar_cap, p.n * ((uint64_t)p.cigar_stride + 2));
        const uint64_t gblocks = std::min<uint64_t>(std::max<uint64_t>(1, (most + 255) / 256), 1u << 16);
        hipLaunchKernelGGL(aln_gather_kernel, dim3((unsigned)gblocks), dim3(256), 0, stream, p);
        e = hipGetLastError();
    }
    if (tmp) {
        const hipError_t ef = hipFreeAsync(tmp, stream);
        if (e == hipSuccess) e = ef;
    }
    return e;
}

}  // namespace msw
