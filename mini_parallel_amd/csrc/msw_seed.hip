// msw_seed.hip -- placing reads (include/msw.h, "Placing reads"): the k-mer
// index of the resident genome and the seed-and-vote kernel.
//
// Index build, five launches on one stream (a one-off cost, kept plain):
//  1. index_count_kernel, a thread per genome position: u32 atomics into cnt;
//  2. index_mask_kernel, a thread per bucket: counts over max_occ become 0;
//  3. scan_in_place (msw_aln.hip): cnt -> off, the exclusive prefix sum;
//  4. index_fill_kernel, a thread per position: a returning atomic cursor per
//     bucket hands out the slots of pos;
//  5. index_sort_kernel, a thread per bucket: an insertion sort of its <= 64
//     positions, so the index does not depend on the order the atomics ran in.
//
// seed_reads_kernel, one wave per read (a block is one wave and owns the
// dynamic LDS): lanes take the k-mer offsets lane, lane + 64, ...; a wave-wide
// scan of the bucket sizes with a running base over the rounds gives the cap
// rule's P_i and each k-mer's slot range in the LDS key array, so the layout
// is the same on every run and needs no atomics.  Keys are diagonals biased by
// 65536, padded with 0xFFFFFFFF to a power of two sized by this read's own
// hits; a bitonic sort, a binary search per key for the first key >= key +
// band, and a wave maximum of (score << 32 | ~key): the best score, then the
// smallest diagonal.
#include <algorithm>

#include "msw_kernels.h"

namespace msw {
namespace {

constexpr uint32_t kNoCode = 0xFFFFFFFFu;
constexpr uint32_t kPadKey = 0xFFFFFFFFu;

// the code of s[0, k), or kNoCode when a byte is none of A C G T
__device__ __forceinline__ uint32_t kmer_code(const uint8_t* s, int k) {
    uint32_t code = 0;
    bool ok = true;
    for (int j = 0; j < k; ++j) {
        const uint32_t b = s[j];
        // A 0x41, C 0x43, G 0x47, T 0x54: bits 2..1 give 0, 1, 3, 2
        const uint32_t two = (b >> 1) & 3u;
        ok = ok && (b == 'A' || b == 'C' || b == 'G' || b == 'T');
        code = (code << 2) | (two ^ (two >> 1));
    }
    return ok ? code : kNoCode;
}

__global__ __launch_bounds__(256) void index_count_kernel(const uint8_t* __restrict__ g, uint64_t n_kmers, int k,
                                                          uint32_t* __restrict__ cnt) {
    const uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (p >= n_kmers) return;
    const uint32_t c = kmer_code(g + p, k);
    if (c != kNoCode) atomicAdd(&cnt[c], 1u);
}

// cnt[buckets] is the scan's extra entry: it enters as 0 and leaves as the total
__global__ __launch_bounds__(256) void index_mask_kernel(uint32_t* __restrict__ cnt, uint64_t buckets,
                                                         uint32_t max_occ, uint32_t* __restrict__ n_masked) {
    const uint64_t c = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (c > buckets) return;
    if (c == buckets) {
        cnt[c] = 0;
        return;
    }
    if (cnt[c] > max_occ) {
        cnt[c] = 0;
        atomicAdd(n_masked, 1u);
    }
}

__global__ __launch_bounds__(256) void index_fill_kernel(const uint8_t* __restrict__ g, uint64_t n_kmers, int k,
                                                         const uint32_t* __restrict__ off,
                                                         uint32_t* __restrict__ cursor, uint32_t* __restrict__ pos) {
    const uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (p >= n_kmers) return;
    const uint32_t c = kmer_code(g + p, k);
    if (c == kNoCode) return;
    const uint32_t s = off[c], e = off[c + 1];
    if (e == s) return;  // empty or masked
    const uint32_t slot = atomicAdd(&cursor[c], 1u);
    if (slot < e - s) pos[s + slot] = (uint32_t)p;  // always: the count pass saw the same positions
}

__global__ __launch_bounds__(256) void index_sort_kernel(const uint32_t* __restrict__ off, uint64_t buckets,
                                                         uint32_t* __restrict__ pos) {
    const uint64_t c = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (c >= buckets) return;
    const uint32_t s = off[c], e = off[c + 1];
    for (uint32_t a = s + 1; a < e; ++a) {
        const uint32_t v = pos[a];
        uint32_t b = a;
        while (b > s && pos[b - 1] > v) {
            pos[b] = pos[b - 1];
            --b;
        }
        pos[b] = v;
    }
}

struct SeedResult {
    uint64_t best;     // votes << 32 | (0xFFFFFFFF - key); 0: no diagonal
    uint32_t hits;
    uint32_t truncated;
};

// One orientation of one read, by the whole wave (every lane returns the same
// result).  keys: the block's LDS array, next_pow2(cap) words.  ALT
// (seed_candidates_kernel): *best2 is the orientation's second band, the same
// packing, over the keys admissible against the first band at `sep`.
template <bool ALT>
__device__ SeedResult seed_orientation(const SeedParams& p, const uint8_t* row, int L, uint32_t* keys, int lane,
                                       uint32_t sep, uint64_t* best2) {
    const int k = (int)p.k;
    const int n_kmers = L >= k ? L - k + 1 : 0;
    uint32_t run = 0;  // P of the last offset handled so far (wave-uniform)
    uint32_t hits = 0;
    for (int base = 0; base < n_kmers && run <= p.cap; base += 64) {
        const int i = base + lane;
        uint32_t start = 0, c = 0;
        if (i < n_kmers && (uint32_t)i % p.step == 0) {
            const uint32_t code = kmer_code(row + i, k);
            if (code != kNoCode) {
                start = p.off[code];
                c = p.off[code + 1] - start;
            }
        }
        uint32_t inc = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t t = __shfl_up(inc, d, 64);
            if (lane >= d) inc += t;
        }
        const uint32_t P = run + inc;  // <= cap + 64 * 64: no overflow
        const bool in = P <= p.cap;    // P is monotone: the contributing offsets are a prefix
        if (in) {
            const uint32_t slot = P - c;
            for (uint32_t t = 0; t < c; ++t) keys[slot + t] = p.pos[start + t] - (uint32_t)i + 65536u;
        }
        const int n_in = (int)__popcll(__ballot(in));  // the lanes [0, n_in)
        if (n_in) hits = __builtin_amdgcn_readfirstlane(__shfl(P, n_in - 1, 64));
        run = __builtin_amdgcn_readfirstlane(__shfl(P, 63, 64));
    }
    SeedResult r;
    r.best = 0;
    r.hits = hits;
    r.truncated = run > p.cap ? 1u : 0u;
    if constexpr (ALT) *best2 = 0;
    if (hits == 0) return r;  // wave-uniform
    uint32_t m = 1;
    while (m < hits) m <<= 1;
    for (uint32_t t = hits + (uint32_t)lane; t < m; t += 64) keys[t] = kPadKey;
    __syncthreads();
    // bitonic sort of keys[0, m), ascending
    for (uint32_t size = 2; size <= m; size <<= 1) {
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            for (uint32_t t = (uint32_t)lane; t < (m >> 1); t += 64) {
                const uint32_t lo = 2 * t - (t & (stride - 1));  // bit `stride` clear
                const uint32_t hi = lo + stride;
                const uint32_t a = keys[lo], b = keys[hi];
                const bool up = (lo & size) == 0;
                if ((a > b) == up) {
                    keys[lo] = b;
                    keys[hi] = a;
                }
            }
            __syncthreads();
        }
    }
    uint64_t best = 0;
    for (uint32_t t = (uint32_t)lane; t < hits; t += 64) {
        const uint32_t key = keys[t];
        const uint64_t want = (uint64_t)key + p.band;
        uint32_t lo = t + 1, hi = hits;  // the first index in (t, hits] whose key >= want
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if ((uint64_t)keys[mid] >= want) hi = mid;
            else lo = mid + 1;
        }
        const uint64_t v = (uint64_t)(lo - t) << 32 | (uint64_t)(0xFFFFFFFFu - key);
        best = v > best ? v : best;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const uint64_t o = __shfl_xor(best, d, 64);
        best = o > best ? o : best;
    }
    if constexpr (ALT) {
        // The second band, over the same sorted keys: a key is admissible iff
        // it is at least sep away from the first band's.  sep >= band, so a
        // band that starts below the excluded keys ends before the admissible
        // keys above them: clipping its upper bound is all it takes.
        const int64_t key0 = (int64_t)(0xFFFFFFFFu - (uint32_t)best);
        const int64_t below = key0 - (int64_t)sep, above = key0 + (int64_t)sep;  // admissible: <= below, >= above
        uint64_t b2 = 0;
        for (uint32_t t = (uint32_t)lane; t < hits; t += 64) {
            const uint32_t key = keys[t];
            const int64_t k64 = (int64_t)key;
            if (k64 > below && k64 < above) continue;
            uint64_t want = (uint64_t)key + p.band;
            if (k64 <= below && want > (uint64_t)below + 1u) want = (uint64_t)below + 1u;  // below >= k64 >= 0
            uint32_t lo = t + 1, hi = hits;
            while (lo < hi) {
                const uint32_t mid = lo + ((hi - lo) >> 1);
                if ((uint64_t)keys[mid] >= want) hi = mid;
                else lo = mid + 1;
            }
            const uint64_t v = (uint64_t)(lo - t) << 32 | (uint64_t)(0xFFFFFFFFu - key);
            b2 = v > b2 ? v : b2;
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            const uint64_t o = __shfl_xor(b2, d, 64);
            b2 = o > b2 ? o : b2;
        }
        *best2 = b2;
    }
    __syncthreads();  // the next orientation or read refills keys
    r.best = best;
    return r;
}

__global__ __launch_bounds__(64) void seed_reads_kernel(SeedParams p) {
    extern __shared__ __attribute__((aligned(16))) uint32_t keys[];
    const int lane = (int)threadIdx.x;
    for (uint64_t r = blockIdx.x; r < p.n; r += gridDim.x) {
        const uint32_t rl = p.read_len[r];
        const int L = (int)min((uint64_t)rl, p.read_stride);
        SeedResult f = seed_orientation<false>(p, p.reads + r * p.read_stride, L, keys, lane, 0u, nullptr);
        uint32_t flags = 0;
        if (p.rc_reads) {
            const int Lr = (int)min((uint64_t)rl, p.rc_stride);
            const SeedResult v = seed_orientation<false>(p, p.rc_reads + r * p.rc_stride, Lr, keys, lane, 0u, nullptr);
            if ((v.best >> 32) > (f.best >> 32)) {  // strictly more votes: ties go forward
                f = v;
                flags = 1;
            }
        }
        if (lane == 0) {
            const uint32_t votes = (uint32_t)(f.best >> 32);
            int64_t wp = -1;
            if (votes != 0 && votes >= p.min_votes) {
                const int64_t d0 = (int64_t)(0xFFFFFFFFu - (uint32_t)f.best) - 65536;
                const int64_t W = (int64_t)reads_window_want(p.window, rl);
                const int64_t slack = W - ((int64_t)rl + (int64_t)p.band - 1);
                const int64_t pad = slack > 0 ? slack / 2 : 0;
                wp = d0 - pad > 0 ? d0 - pad : 0;
            }
            p.win_pos[r] = wp;
            p.votes[r] = votes;
            p.hits[r] = f.hits;
            p.flags[r] = (uint8_t)(flags | f.truncated << 1);
        }
    }
}

// win_pos of a band that starts at the biased diagonal `key` (the placement rule)
__device__ __forceinline__ int64_t seed_place(uint32_t key, uint32_t rl, uint32_t window, uint32_t band) {
    const int64_t d0 = (int64_t)key - 65536;
    const int64_t W = (int64_t)reads_window_want(window, rl);
    const int64_t slack = W - ((int64_t)rl + (int64_t)band - 1);
    const int64_t pad = slack > 0 ? slack / 2 : 0;
    return d0 - pad > 0 ? d0 - pad : 0;
}

// Candidates (include/msw.h, "Candidates and mapping quality"): candidate 0 is
// what seed_reads_kernel writes; candidate 1 is the best of the other bands
// (the chosen orientation's second, the other orientation's two) that has
// min_votes and lies sep or more from candidate 0's diagonal.
__global__ __launch_bounds__(64) void seed_candidates_kernel(SeedCandParams q) {
    extern __shared__ __attribute__((aligned(16))) uint32_t keys[];
    const SeedParams& p = q.s;
    const int lane = (int)threadIdx.x;
    for (uint64_t r = blockIdx.x; r < p.n; r += gridDim.x) {
        const uint32_t rl = p.read_len[r];
        const int L = (int)min((uint64_t)rl, p.read_stride);
        const uint32_t W = reads_window_want(p.window, rl);
        const uint32_t sep = q.sep ? q.sep : (W > p.band ? W : p.band);
        uint64_t own2 = 0, oth1 = 0, oth2 = 0;
        SeedResult f = seed_orientation<true>(p, p.reads + r * p.read_stride, L, keys, lane, sep, &own2);
        uint32_t flags = 0;
        if (p.rc_reads) {
            const int Lr = (int)min((uint64_t)rl, p.rc_stride);
            const SeedResult v = seed_orientation<true>(p, p.rc_reads + r * p.rc_stride, Lr, keys, lane, sep, &oth2);
            oth1 = v.best;
            if ((v.best >> 32) > (f.best >> 32)) {  // strictly more votes: ties go forward
                oth1 = f.best;
                f = v;
                const uint64_t t = own2;
                own2 = oth2;
                oth2 = t;
                flags = 1;
            }
        }
        if (lane == 0) {
            const uint32_t votes = (uint32_t)(f.best >> 32);
            const uint32_t key0 = 0xFFFFFFFFu - (uint32_t)f.best;
            p.win_pos[r] = votes != 0 && votes >= p.min_votes ? seed_place(key0, rl, p.window, p.band) : -1;
            p.votes[r] = votes;
            p.hits[r] = f.hits;
            p.flags[r] = (uint8_t)(flags | f.truncated << 1);
            // votes << 33 | forward << 32 | ~key: the most votes, then forward, then the smaller diagonal
            uint64_t pick = 0;
            const uint64_t band3[3] = {own2, oth1, oth2};
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const uint64_t b = band3[c];
                const uint32_t v = (uint32_t)(b >> 32), key = 0xFFFFFFFFu - (uint32_t)b;
                const uint32_t orient = c == 0 ? flags : flags ^ 1u;
                const int64_t gap = (int64_t)key - (int64_t)key0;
                const bool ok = votes != 0 && v != 0 && v >= p.min_votes && (gap < 0 ? -gap : gap) >= (int64_t)sep;
                const uint64_t rank = (uint64_t)v << 33 | (uint64_t)(orient ^ 1u) << 32 | (uint64_t)(uint32_t)b;
                if (ok && rank > pick) pick = rank;
            }
            const uint32_t v1 = (uint32_t)(pick >> 33);
            q.win_pos1[r] = v1 ? seed_place(0xFFFFFFFFu - (uint32_t)pick, rl, p.window, p.band) : -1;
            q.votes1[r] = v1;
            q.flags1[r] = v1 ? (uint8_t)(((pick >> 32) & 1u) ^ 1u) : (uint8_t)0;
        }
    }
}

unsigned blocks256(uint64_t items) { return (unsigned)((items + 255u) / 256u); }

}  // namespace

uint64_t index_scan_tmp_words(uint64_t buckets) {
    uint64_t words = 0;
    const auto tiles = [](uint64_t count) { return (count + kAlnScanTile - 1) / kAlnScanTile; };
    for (uint64_t c = tiles(buckets + 1); c > 1; c = tiles(c)) words += c;  // as launch_aln_pack sizes its own
    return words;
}

hipError_t launch_index_count(const uint8_t* genome, uint64_t glen, uint32_t k, uint32_t max_occ, uint32_t* off,
                              uint32_t* n_masked, uint32_t* scan_tmp, hipEvent_t* ev, hipStream_t st) {
    const uint64_t buckets = 1ull << (2 * k);
    const uint64_t n_kmers = glen >= k ? glen - k + 1 : 0;
    hipError_t e = hipMemsetAsync(off, 0, (buckets + 1) * sizeof(uint32_t), st);
    if (e == hipSuccess) e = hipMemsetAsync(n_masked, 0, sizeof(uint32_t), st);
    if (e == hipSuccess) e = hipEventRecord(ev[0], st);
    if (e != hipSuccess) return e;
    if (n_kmers)
        hipLaunchKernelGGL(index_count_kernel, dim3(blocks256(n_kmers)), dim3(256), 0, st, genome, n_kmers, (int)k,
                           off);
    if ((e = hipGetLastError()) != hipSuccess || (e = hipEventRecord(ev[1], st)) != hipSuccess) return e;
    hipLaunchKernelGGL(index_mask_kernel, dim3(blocks256(buckets + 1)), dim3(256), 0, st, off, buckets, max_occ,
                       n_masked);
    if ((e = hipGetLastError()) != hipSuccess || (e = hipEventRecord(ev[2], st)) != hipSuccess) return e;
    if ((e = scan_in_place(off, buckets + 1, scan_tmp, st)) != hipSuccess) return e;
    return hipEventRecord(ev[3], st);
}

hipError_t launch_index_fill(const uint8_t* genome, uint64_t glen, uint32_t k, const uint32_t* off, uint32_t* cursor,
                             uint32_t* pos, hipEvent_t* ev, hipStream_t st) {
    const uint64_t buckets = 1ull << (2 * k);
    const uint64_t n_kmers = glen >= k ? glen - k + 1 : 0;
    hipError_t e = hipMemsetAsync(cursor, 0, buckets * sizeof(uint32_t), st);
    if (e == hipSuccess) e = hipEventRecord(ev[0], st);
    if (e != hipSuccess) return e;
    if (n_kmers)
        hipLaunchKernelGGL(index_fill_kernel, dim3(blocks256(n_kmers)), dim3(256), 0, st, genome, n_kmers, (int)k, off,
                           cursor, pos);
    if ((e = hipGetLastError()) != hipSuccess || (e = hipEventRecord(ev[1], st)) != hipSuccess) return e;
    hipLaunchKernelGGL(index_sort_kernel, dim3(blocks256(buckets)), dim3(256), 0, st, off, buckets, pos);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return hipEventRecord(ev[2], st);
}

size_t seed_lds_bytes(uint32_t cap) {
    uint32_t m = 1;
    while (m < cap) m <<= 1;
    return (size_t)m * sizeof(uint32_t);
}

hipError_t launch_seed_reads(const SeedParams& p, hipStream_t stream) {
    if (p.n == 0) return hipSuccess;
    if (p.cap == 0 || p.cap > kSeedMaxCap || p.step == 0 || p.band == 0 || p.k < 4 || p.k > 14)
        return hipErrorInvalidValue;
    // a wave per read; past 2^20 blocks the grid strides
    const unsigned blocks = (unsigned)std::min<uint64_t>(p.n, 1u << 20);
    hipLaunchKernelGGL(seed_reads_kernel, dim3(blocks), dim3(64), seed_lds_bytes(p.cap), stream, p);
    return hipGetLastError();
}

hipError_t launch_seed_candidates(const SeedCandParams& q, hipStream_t stream) {
    const SeedParams& p = q.s;
    if (p.n == 0) return hipSuccess;
    if (p.cap == 0 || p.cap > kSeedMaxCap || p.step == 0 || p.band == 0 || p.k < 4 || p.k > 14 ||
        (q.sep != 0 && q.sep < p.band))
        return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)std::min<uint64_t>(p.n, 1u << 20);
    hipLaunchKernelGGL(seed_candidates_kernel, dim3(blocks), dim3(64), seed_lds_bytes(p.cap), stream, q);
    return hipGetLastError();
}

int seed_candidates_blocks_per_cu(uint32_t cap) {
    int a = 0;
    const hipError_t e =
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&a, seed_candidates_kernel, 64, seed_lds_bytes(cap));
    return e == hipSuccess ? a : 0;
}

int seed_blocks_per_cu(uint32_t cap) {
    int a = 0;
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&a, seed_reads_kernel, 64, seed_lds_bytes(cap));
    return e == hipSuccess ? a : 0;
}

}  // namespace msw
