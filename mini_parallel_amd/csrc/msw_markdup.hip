// msw_markdup.hip -- duplicate flags and coordinate order (msw_markdup_device,
// msw_aln_order_device; the rules are in include/msw.h, "Sorting and
// duplicates").  Everything is enqueued on the caller's stream; the sort is
// msw_sort.hip's, the scan msw_aln.hip's.
//
//  1. markdup_key_kernel, one thread per fragment: walks the CIGAR of its read
//     (or of its two mates) for the leading clip, the trailing clip and the
//     reference span, and writes the fragment's keys (K1, K2), its packed
//     quality `quality << 31 | (2^31 - 1 - fragment)` and which rows are keyed;
//     order[f] = f.  A thread's work is its own ops, never a group's.
//  2. the order: single-end one sort of (K1, order); pairs a sort of
//     (K2, order), a gather of K1 through order, and a second, stable sort.
//  3. markdup_head_kernel: step[t] = 1 where rank t + 1 starts a new (K1, K2)
//     run; its exclusive scan is the run id of every rank.  The same kernel
//     clears best[] and *n_dup (no memset: the call may be captured).
//  4. markdup_best_kernel: best[run] = the 64-bit max of the packed qualities of
//     the run.  A max does not depend on the order its atomics run in; a wave
//     whose 64 ranks lie in one run folds them with shuffles and issues ONE
//     atomic, so a pile a million deep costs 16 K atomics on its word, not 1 M.
//  5. markdup_flag_kernel: a keyed fragment whose packed quality is not its
//     run's best is a duplicate: its keyed rows get 1, every other row 0, and
//     the count goes up by a wave's ballot at a time.
#include <algorithm>

#include "msw_kernels.h"

namespace msw {
namespace {

constexpr uint32_t kOpM = 0, kOpD = 2, kOpS = 4;
constexpr uint64_t kIdxMask = 0x7FFFFFFFull;

// the key of read r, or p.k_none
__device__ __forceinline__ uint64_t read_key(const MarkdupParams& p, uint64_t r) {
    const int64_t pos = p.ref_pos[r];
    // pos beyond the genome and its clips cannot give a key below k_none (and must not overflow below)
    if (pos < 0 || (uint64_t)pos > (p.k_none >> 1) || p.score[r] <= 0 || p.nm[r] < 0) return p.k_none;
    const uint32_t lo = p.cigar_off[r], hi = p.cigar_off[r + 1];
    if (hi < lo || hi > p.cigar_cap) return p.k_none;  // ops outside the stream: nothing to walk
    int64_t lead = 0, trail = 0, span = 0;
    for (uint32_t q = lo; q < hi; ++q) {
        const uint32_t op = p.cigar[q];
        const int64_t len = (int64_t)(op >> 4);
        const uint32_t code = op & 15u;
        if (code == kOpS) {
            if (q == lo) lead = len;
            else if (q + 1 == hi) trail = len;
        } else if (code == kOpM || code == kOpD) {
            span += len;
        }
    }
    const uint64_t s = p.strand && p.strand[r] ? 1u : 0u;
    const int64_t u5 = s ? pos + span - 1 + trail : pos - lead;
    const int64_t v = u5 + 32768;
    if (v < 0) return p.k_none;
    const uint64_t k = (uint64_t)v << 1 | s;
    return k < p.k_none ? k : p.k_none;
}

__global__ __launch_bounds__(256) void markdup_key_kernel(MarkdupParams p) {
    const uint64_t step = (uint64_t)gridDim.x * 256u;
    for (uint64_t f = (uint64_t)blockIdx.x * 256u + threadIdx.x; f < p.frags; f += step) {
        uint64_t quality = 0;
        uint32_t keyed = 0;
        if (!p.pairs) {
            const uint64_t k = read_key(p, f);
            if (k != p.k_none) {
                keyed = 1;
                quality = (uint64_t)p.score[f];
            }
            p.work[f] = k;
        } else {
            const uint64_t ka = read_key(p, 2 * f), kb = read_key(p, 2 * f + 1);
            if (ka != p.k_none) {
                keyed |= 1u;
                quality += (uint64_t)p.score[2 * f];
            }
            if (kb != p.k_none) {
                keyed |= 2u;
                quality += (uint64_t)p.score[2 * f + 1];
            }
            const uint64_t hi = ka > kb ? ka : kb;
            p.k1[f] = ka < kb ? ka : kb;
            p.k2[f] = hi;
            p.work[f] = hi;
        }
        // quality <= 2 (2^31 - 1) takes 33 bits, the index 31
        p.pk[f] = quality << 31 | (kIdxMask - f);
        p.km[f] = (uint8_t)keyed;
        p.order[f] = (uint32_t)f;
    }
}

__global__ __launch_bounds__(256) void markdup_gather_kernel(MarkdupParams p) {
    const uint64_t step = (uint64_t)gridDim.x * 256u;
    for (uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x; t < p.frags; t += step) p.work[t] = p.k1[p.order[t]];
}

__global__ __launch_bounds__(256) void markdup_head_kernel(MarkdupParams p) {
    const uint64_t step = (uint64_t)gridDim.x * 256u;
    if (p.n_dup && blockIdx.x == 0 && threadIdx.x == 0) *p.n_dup = 0;
    for (uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x; t < p.frags; t += step) {
        bool differs = false;
        if (t + 1 < p.frags) {
            differs = p.work[t] != p.work[t + 1];
            if (!differs && p.pairs) differs = p.k2[p.order[t]] != p.k2[p.order[t + 1]];
        }
        p.rid[t] = differs ? 1u : 0u;
        p.best[t] = 0;
    }
}

__global__ __launch_bounds__(256) void markdup_best_kernel(MarkdupParams p) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t step = (uint64_t)gridDim.x * 256u;
    // whole waves run every trip: the shuffles below need all 64 lanes
    const uint64_t trips = (p.frags + step - 1) / step;
    for (uint64_t trip = 0; trip < trips; ++trip) {
        const uint64_t t = trip * step + (uint64_t)blockIdx.x * 256u + threadIdx.x;
        const bool active = t < p.frags && p.work[t] != p.k_none;
        const uint32_t run = active ? p.rid[t] : 0u;
        unsigned long long v = active ? p.pk[p.order[t]] : 0ull;
        const uint64_t am = __ballot(active);
        if (am == 0) continue;
        const int first = __ffsll((unsigned long long)am) - 1;
        const uint32_t run0 = (uint32_t)__shfl((int)run, first, 64);
        if (__ballot(active && run != run0) == 0) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const unsigned long long o = __shfl_xor(v, off, 64);
                v = o > v ? o : v;
            }
            if ((int)lane == first) atomicMax(&p.best[run0], v);
        } else if (active) {
            atomicMax(&p.best[run], v);
        }
    }
}

__global__ __launch_bounds__(256) void markdup_flag_kernel(MarkdupParams p) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t step = (uint64_t)gridDim.x * 256u;
    const uint64_t trips = (p.frags + step - 1) / step;
    for (uint64_t trip = 0; trip < trips; ++trip) {
        const uint64_t t = trip * step + (uint64_t)blockIdx.x * 256u + threadIdx.x;
        bool isdup = false;
        if (t < p.frags) {
            const uint64_t f = p.order[t];
            isdup = p.work[t] != p.k_none && p.best[p.rid[t]] != p.pk[f];
            if (!p.pairs) {
                p.dup[f] = isdup ? 1 : 0;
            } else {
                const uint32_t m = p.km[f];
                p.dup[2 * f] = isdup && (m & 1u) ? 1 : 0;
                p.dup[2 * f + 1] = isdup && (m & 2u) ? 1 : 0;
            }
        }
        const uint64_t dm = __ballot(isdup);
        if (p.n_dup && lane == 0 && dm) atomicAdd(p.n_dup, (unsigned long long)__popcll(dm));
    }
}

__global__ __launch_bounds__(256) void order_key_kernel(const int64_t* __restrict__ ref_pos,
                                                        const uint8_t* __restrict__ strand, uint64_t n, uint64_t k_last,
                                                        uint64_t* __restrict__ work, uint32_t* __restrict__ order) {
    const uint64_t step = (uint64_t)gridDim.x * 256u;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += step) {
        const int64_t pos = ref_pos[i];
        uint64_t k = k_last;
        if (pos >= 0 && (uint64_t)pos < (k_last >> 1)) k = (uint64_t)pos << 1 | (strand && strand[i] ? 1u : 0u);
        work[i] = k;
        order[i] = (uint32_t)i;
    }
}

uint64_t up256(uint64_t b) { return (b + 255) & ~(uint64_t)255; }
uint64_t scan_words(uint64_t count) {
    uint64_t words = 0;
    for (uint64_t c = (count + kAlnScanTile - 1) / kAlnScanTile; c > 1; c = (c + kAlnScanTile - 1) / kAlnScanTile)
        words += c;
    return words;
}
unsigned grid_for(uint64_t n) { return (unsigned)std::min<uint64_t>(std::max<uint64_t>(1, (n + 255) / 256), 1u << 16); }

}  // namespace

uint64_t markdup_tmp_bytes(uint64_t frags, bool pairs) {
    return up256(frags * 8) * (pairs ? 5 : 3) + up256(frags) + up256(frags * 4) + up256(scan_words(frags) * 4) +
           sort_tmp_bytes(frags, true);
}

hipError_t launch_markdup(MarkdupParams p, uint32_t key_bits, void* tmp, hipStream_t st) {
    const uint64_t F = p.frags;
    if (F == 0) {  // the head kernel clears the count and touches nothing else
        if (p.n_dup) hipLaunchKernelGGL(markdup_head_kernel, dim3(1), dim3(256), 0, st, p);
        return hipGetLastError();
    }
    uint8_t* at = static_cast<uint8_t*>(tmp);
    const auto take = [&](uint64_t bytes) {
        uint8_t* r = at;
        at += up256(bytes);
        return r;
    };
    p.work = reinterpret_cast<uint64_t*>(take(F * 8));
    p.pk = reinterpret_cast<uint64_t*>(take(F * 8));
    p.best = reinterpret_cast<unsigned long long*>(take(F * 8));
    p.k1 = p.pairs ? reinterpret_cast<uint64_t*>(take(F * 8)) : nullptr;
    p.k2 = p.pairs ? reinterpret_cast<uint64_t*>(take(F * 8)) : nullptr;
    p.km = take(F);
    p.rid = reinterpret_cast<uint32_t*>(take(F * 4));
    uint32_t* scan_tmp = reinterpret_cast<uint32_t*>(take(scan_words(F) * 4));
    void* sort_tmp = at;
    const unsigned grid = grid_for(F);

    hipLaunchKernelGGL(markdup_key_kernel, dim3(grid), dim3(256), 0, st, p);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = launch_sort_pairs(p.work, p.order, F, key_bits, sort_tmp, st);
    if (e == hipSuccess && p.pairs) {
        hipLaunchKernelGGL(markdup_gather_kernel, dim3(grid), dim3(256), 0, st, p);
        e = hipGetLastError();
        if (e == hipSuccess) e = launch_sort_pairs(p.work, p.order, F, key_bits, sort_tmp, st);
    }
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(markdup_head_kernel, dim3(grid), dim3(256), 0, st, p);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = scan_in_place(p.rid, F, scan_tmp, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(markdup_best_kernel, dim3(grid), dim3(256), 0, st, p);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(markdup_flag_kernel, dim3(grid), dim3(256), 0, st, p);
    return hipGetLastError();
}

uint64_t aln_order_tmp_bytes(uint64_t n) { return up256(n * 8) + sort_tmp_bytes(n, true); }

hipError_t launch_aln_order(const int64_t* ref_pos, const uint8_t* strand, uint64_t n, uint64_t k_last,
                            uint32_t key_bits, uint32_t* order, void* tmp, hipStream_t st) {
    uint64_t* work = static_cast<uint64_t*>(tmp);
    hipLaunchKernelGGL(order_key_kernel, dim3(grid_for(n)), dim3(256), 0, st, ref_pos, strand, n, k_last, work, order);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_sort_pairs(work, order, n, key_bits, static_cast<uint8_t*>(tmp) + up256(n * 8), st);
}

}  // namespace msw
