// msw_pileup.hip -- per-base allele counts from alignment records
// (msw_pileup_*, include/msw.h "Pileup").
//
// The difference form: almost every aligned column shows the reference base,
// so a read does not add to counts[g + k][code] per column.  Per M run it adds
// +1 / -1 at the two ends of the run's counted range in a difference array
// (d_all, and d_rev for a strand-1 read), and only the columns whose read byte
// differs from the genome byte add to counts[pos][code(read byte)] and to
// mism[pos]: about 2 + NM atomics per read instead of one per column.
// pileup_finish_kernel folds the state once: after an exclusive scan of the
// difference arrays (scan_in_place, msw_aln.hip) entry pos + 1 is the number of
// M columns over pos, and counts[pos][code(genome[pos])] += that - mism[pos].
// Every add is an integer add, so the result is a function of the set of
// records alone, whatever order the atomics ran in.
//
// pileup_add_kernel is one wave per read like aln_count_kernel: every lane
// loads the same record words and the same ops (the walk is wave-uniform, there
// is no ballot or shuffle), and the lanes split the columns of a run.  With a
// base-quality threshold (msw_pileup_add_qual*) a second instance of the kernel
// runs, which also reads one quality byte per column.
#include <algorithm>
#include <type_traits>

#include "msw_kernels.h"

namespace msw {
namespace {

// A 0, C 1, G 2, T 3 (upper case only), anything else 4: the k-mer codes of
// "Placing reads" plus the "other" channel.
__device__ __forceinline__ uint32_t base_code(uint32_t b) {
    return b == 'A' ? 0u : b == 'C' ? 1u : b == 'G' ? 2u : b == 'T' ? 3u : 4u;
}

// comp of "Both strands": A<->T, C<->G, a<->t, c<->g, every other byte as it is
__device__ __forceinline__ uint32_t comp_byte(uint32_t b) {
    const uint32_t u = b & ~0x20u;
    const uint32_t c = u == 'A' ? 'T' : u == 'T' ? 'A' : u == 'C' ? 'G' : u == 'G' ? 'C' : 0u;
    return c ? c | (b & 0x20u) : b;
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// QUAL: the base-quality filter (msw.h, "Base qualities").  The ranges in the
// difference arrays stay whole; a column under the threshold takes itself out
// again with one add to mism[pos] -- whether its byte matches the genome or
// not, the "same" fold d_all - mism then comes out without it, and a
// mismatching one simply adds to no channel -- and, for a strand-1 read, one
// wrapped -1 on channel 7, which the fold's += d_rev brings back in range.
// Q is empty (the plain add: its arguments and code are what they were without
// the filter) or one PileupQual.
//
// QSUM (a PileupQsum in Q; msw.h, "Quality sums and weighted genotypes"): the
// Phred sums in the same difference form.  With e_k the Phred value of column k
// of the run's range [lo, hi) when it counts and 0 when it is dropped, the lane
// of column k adds e_k - e_(k-1) to d_q[g + k] (e_(lo-1) = 0; the neighbour's
// byte is a second load, not a shuffle) and the lane of column hi - 1 adds
// -e_(hi-1) to d_q[g + hi]: a stretch of one quality value costs no atomic.  A
// counted mismatching column also adds e_k to qmis[pos] and, where its code is
// below 4, to qsum[pos][code]; the fold is qsum[pos][code(genome[pos])] +=
// scanned d_q[pos + 1] - qmis[pos].  Here min_baseq may be 0: a column counts
// when t < qual_stride and its Phred value is at least min_baseq.
__device__ __forceinline__ const PileupQual& qual_of(const PileupQual& q) { return q; }
__device__ __forceinline__ const PileupQsum& qsum_of(const PileupQsum& q) { return q; }
__device__ __forceinline__ uint32_t phred_of(uint32_t b) { return b >= 33u ? b - 33u : 0u; }

template <typename... Q>
__global__ __launch_bounds__(256) void pileup_add_kernel(PileupParams p, Q... qual) {
    constexpr bool QUAL = sizeof...(Q) == 1;
    constexpr bool QSUM = (std::is_same<Q, PileupQsum>::value || ...);
    __shared__ uint32_t tally[4][QUAL ? 3 : 2];
    const int lane = (int)(threadIdx.x & 63u);
    const uint64_t wave = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    const uint64_t waves = (uint64_t)gridDim.x * 4u;
    const int64_t glen = (int64_t)p.glen;
    uint32_t used = 0, skipped = 0;
    [[maybe_unused]] uint32_t lowq = 0;  // this lane's columns under the threshold
    for (uint64_t r = wave; r < p.n; r += waves) {
        // wave-uniform: every lane loads the same words
        const int64_t ref = p.ref_pos[r];
        const uint32_t o0 = p.cigar_off[r], o1 = p.cigar_off[r + 1];
        const bool counted = ref >= 0 && p.nm[r] >= 0 && o1 > o0 && o0 >= p.cigar_base &&
                             (uint64_t)o1 <= p.cigar_cap && (!p.mapq || p.mapq[r] >= p.min_mapq);
        if (!counted) {
            ++skipped;
            continue;
        }
        ++used;
        const int64_t rl = p.read_len[r];
        const bool rev = p.strand && p.strand[r] != 0;
        const bool flip = rev && p.orient;  // the row holds the read as given: read its reverse complement
        const uint8_t* rd = p.rows + r * p.row_stride;
        const uint32_t* ops = p.cigar + (o0 - p.cigar_base);
        [[maybe_unused]] const uint8_t* qrow = nullptr;
        if constexpr (QUAL) qrow = qual_of(qual...).quals + r * qual_of(qual...).qual_stride;
        int64_t i = 0, g = ref;
        // g only grows: past glen nothing counts any more (an I run at g == glen still marks glen - 1)
        for (uint32_t q = 0; q < o1 - o0 && g <= glen; ++q) {
            const uint32_t op = ops[q];
            const int64_t len = (int64_t)(op >> 4);
            const uint32_t code = op & 15u;
            if (code == 0) {
                // columns k with 0 <= g + k < glen and i + k < rl: one range [lo, hi)
                const int64_t lo = g < 0 ? -g : 0;
                const int64_t hi = std::min(len, std::min(glen - g, rl - i));
                if (lo < hi) {
                    if (lane == 0) {
                        atomicAdd(p.d_all + (g + lo), 1u);
                        atomicAdd(p.d_all + (g + hi), 0xFFFFFFFFu);
                        if (rev) {
                            atomicAdd(p.d_rev + (g + lo), 1u);
                            atomicAdd(p.d_rev + (g + hi), 0xFFFFFFFFu);
                        }
                    }
                    for (int64_t k = lo + lane; k < hi; k += 64) {
                        const uint32_t rb = flip ? comp_byte(rd[rl - 1 - (i + k)]) : (uint32_t)rd[i + k];
                        if constexpr (QSUM) {
                            const PileupQsum& qs = qsum_of(qual...);
                            const int64_t t = rev ? rl - 1 - (i + k) : i + k;
                            const uint32_t ph = t < (int64_t)qs.qual_stride ? phred_of(qrow[t]) : 0u;
                            const bool keep = t < (int64_t)qs.qual_stride && ph >= qs.min_baseq;
                            const uint32_t e = keep ? ph : 0u;
                            // column k - 1 of the same range: lo <= k - 1, so its index is in [0, rl) too
                            uint32_t prev = 0;
                            if (k > lo) {
                                const int64_t tp = rev ? t + 1 : t - 1;
                                if (tp < (int64_t)qs.qual_stride) {
                                    const uint32_t pp = phred_of(qrow[tp]);
                                    prev = pp >= qs.min_baseq ? pp : 0u;
                                }
                            }
                            if (e != prev) atomicAdd(qs.d_q + (g + k), e - prev);
                            if (k == hi - 1 && e) atomicAdd(qs.d_q + (g + hi), 0u - e);
                            if (!keep) {
                                ++lowq;
                                atomicAdd(p.mism + (g + k), 1u);
                                if (rev) atomicAdd(p.counts + (uint64_t)(g + k) * p.pos_mul + 7u * p.ch_mul, 0xFFFFFFFFu);
                            } else if (rb != p.genome[g + k]) {
                                const uint32_t c = base_code(rb);
                                atomicAdd(p.counts + (uint64_t)(g + k) * p.pos_mul + c * p.ch_mul, 1u);
                                atomicAdd(p.mism + (g + k), 1u);
                                if (e) {
                                    atomicAdd(qs.qmis + (g + k), e);
                                    if (c < 4u) atomicAdd(qs.qsum + (uint64_t)(g + k) * 4u + c, e);
                                }
                            }
                            continue;
                        } else if constexpr (QUAL) {
                            // 0 <= i + k < rl here, so t is in [0, rl) either way; the quality rows are in the
                            // order of the reads as given, whatever the orientation of `rows`
                            const int64_t t = rev ? rl - 1 - (i + k) : i + k;
                            const uint32_t b = t < (int64_t)qual_of(qual...).qual_stride ? (uint32_t)qrow[t] : 0u;
                            if ((b >= 33u ? b - 33u : 0u) < qual_of(qual...).min_baseq) {
                                ++lowq;
                                atomicAdd(p.mism + (g + k), 1u);
                                if (rev) atomicAdd(p.counts + (uint64_t)(g + k) * p.pos_mul + 7u * p.ch_mul, 0xFFFFFFFFu);
                                continue;
                            }
                        }
                        if (rb != p.genome[g + k]) {
                            atomicAdd(p.counts + (uint64_t)(g + k) * p.pos_mul + base_code(rb) * p.ch_mul, 1u);
                            atomicAdd(p.mism + (g + k), 1u);
                        }
                    }
                }
                i += len;
                g += len;
            } else if (code == 2) {
                const int64_t lo = g < 0 ? -g : 0;
                const int64_t hi = std::min(len, glen - g);
                for (int64_t k = lo + lane; k < hi; k += 64)
                    atomicAdd(p.counts + (uint64_t)(g + k) * p.pos_mul + 5u * p.ch_mul, 1u);
                g += len;
            } else if (code == 1) {
                if (lane == 0 && g >= 1 && g - 1 < glen)
                    atomicAdd(p.counts + (uint64_t)(g - 1) * p.pos_mul + 6u * p.ch_mul, 1u);
                i += len;
            } else if (code == 4) {
                i += len;
            }
        }
    }
    // One add per block and counter, into the block's slot: adds to one
    // address run one after the other (a counter word per wave measured as the
    // whole launch time, ~12 ns each), adds to different lines side by side.
    [[maybe_unused]] unsigned long long low_wave = 0;
    if constexpr (QUAL) low_wave = wave_sum(lowq);  // every lane of the wave is here
    if (lane == 0) {
        tally[threadIdx.x >> 6][0] = used;
        tally[threadIdx.x >> 6][1] = skipped;
        if constexpr (QUAL) tally[threadIdx.x >> 6][2] = (uint32_t)low_wave;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const uint32_t v = tally[0][threadIdx.x] + tally[1][threadIdx.x] + tally[2][threadIdx.x] + tally[3][threadIdx.x];
        if (v)
            atomicAdd(p.reads + ((blockIdx.x % kPileupReadSlots) * 2u + threadIdx.x) * kPileupReadSlotWords,
                      (unsigned long long)v);
    }
    if constexpr (QUAL) {
        if (threadIdx.x == 2) {
            const unsigned long long v = (unsigned long long)tally[0][2] + tally[1][2] + tally[2][2] + tally[3][2];
            if (v) atomicAdd(qual_of(qual...).lowq + (blockIdx.x % kPileupReadSlots) * kPileupReadSlotWords, v);
        }
    }
}


// counts[pos][code(genome[pos])] += d_all[pos + 1] - mism[pos]; counts[pos][7] += d_rev[pos + 1]
// (the difference arrays scanned: exclusive, so the inclusive value sits one entry on).
// Rows of eight: the two halves of a row as 16-byte loads and stores.
__global__ __launch_bounds__(256) void pileup_finish_kernel(PileupParams p) {
    const uint64_t step = (uint64_t)gridDim.x * 256u;
    for (uint64_t pos = (uint64_t)blockIdx.x * 256u + threadIdx.x; pos < p.glen; pos += step) {
        const uint32_t c = base_code(p.genome[pos]);
        const uint32_t same = p.d_all[pos + 1] - p.mism[pos];
        const uint32_t rev = p.d_rev[pos + 1];
        if (p.pos_mul == 8) {
            uint4* row = reinterpret_cast<uint4*>(p.counts + pos * 8u);
            uint4 a = row[0], b = row[1];
            a.x += c == 0 ? same : 0u;
            a.y += c == 1 ? same : 0u;
            a.z += c == 2 ? same : 0u;
            a.w += c == 3 ? same : 0u;
            b.x += c == 4 ? same : 0u;
            b.w += rev;
            row[0] = a;
            row[1] = b;
        } else {
            p.counts[pos * p.pos_mul + c * p.ch_mul] += same;
            p.counts[pos * p.pos_mul + 7u * p.ch_mul] += rev;
        }
    }
}

// qsum[pos][code(genome[pos])] += d_q[pos + 1] - qmis[pos] where that code is below 4 (d_q scanned)
__global__ __launch_bounds__(256) void pileup_finish_qsum_kernel(PileupParams p, PileupQsum q) {
    const uint64_t step = (uint64_t)gridDim.x * 256u;
    for (uint64_t pos = (uint64_t)blockIdx.x * 256u + threadIdx.x; pos < p.glen; pos += step) {
        const uint32_t c = base_code(p.genome[pos]);
        if (c < 4u) q.qsum[pos * 4u + c] += q.d_q[pos + 1] - q.qmis[pos];
    }
}

// stats: [0] covered, [1] depth_sum, [2] minority_ref, [3] max_depth
__global__ __launch_bounds__(256) void pileup_summary_kernel(PileupParams p, uint32_t min_depth,
                                                             unsigned long long* stats) {
    __shared__ unsigned long long part[4][4];
    const uint64_t step = (uint64_t)gridDim.x * 256u;
    unsigned long long covered = 0, sum = 0, minority = 0, mx = 0;
    for (uint64_t pos = (uint64_t)blockIdx.x * 256u + threadIdx.x; pos < p.glen; pos += step) {
        uint32_t ch[6];
        if (p.pos_mul == 8) {
            const uint4 a = *reinterpret_cast<const uint4*>(p.counts + pos * 8u);
            const uint2 b = *reinterpret_cast<const uint2*>(p.counts + pos * 8u + 4u);
            ch[0] = a.x, ch[1] = a.y, ch[2] = a.z, ch[3] = a.w, ch[4] = b.x, ch[5] = b.y;
        } else {
#pragma unroll
            for (int k = 0; k < 6; ++k) ch[k] = p.counts[pos * p.pos_mul + (uint64_t)k * p.ch_mul];
        }
        const unsigned long long depth = (unsigned long long)ch[0] + ch[1] + ch[2] + ch[3] + ch[4] + ch[5];
        const uint32_t c = base_code(p.genome[pos]);
        const unsigned long long ref = c == 0 ? ch[0] : c == 1 ? ch[1] : c == 2 ? ch[2] : c == 3 ? ch[3] : ch[4];
        covered += depth > 0;
        sum += depth;
        mx = depth > mx ? depth : mx;
        minority += depth >= min_depth && 2 * ref < depth;
    }
    // every lane of every wave takes part in the shuffles
    covered = wave_sum(covered);
    sum = wave_sum(sum);
    minority = wave_sum(minority);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_down(mx, off, 64);
        mx = o > mx ? o : mx;
    }
    const int lane = (int)(threadIdx.x & 63u), w = (int)(threadIdx.x >> 6);
    if (lane == 0) {
        part[w][0] = covered;
        part[w][1] = sum;
        part[w][2] = minority;
        part[w][3] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t[4] = {0, 0, 0, 0};
        for (int k = 0; k < 4; ++k) {
            t[0] += part[k][0];
            t[1] += part[k][1];
            t[2] += part[k][2];
            t[3] = part[k][3] > t[3] ? part[k][3] : t[3];
        }
        if (t[0]) atomicAdd(stats + 0, t[0]);
        if (t[1]) atomicAdd(stats + 1, t[1]);
        if (t[2]) atomicAdd(stats + 2, t[2]);
        if (t[3]) atomicMax(stats + 3, t[3]);
    }
}

// out[pos - pos0][ch] = counts of positions [pos0, pos0 + m) in the public row order
__global__ __launch_bounds__(256) void pileup_rows_kernel(PileupParams p, uint64_t pos0, uint64_t m, uint32_t* out) {
    const uint64_t step = (uint64_t)gridDim.x * 256u;
    for (uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x; k < m * 8u; k += step)
        out[k] = p.counts[(pos0 + (k >> 3)) * p.pos_mul + (k & 7u) * p.ch_mul];
}

unsigned grid_for(uint64_t items) {
    return (unsigned)std::min<uint64_t>(std::max<uint64_t>(1, (items + 255) / 256), 1u << 16);
}

}  // namespace

uint64_t pileup_scan_tmp_words(uint64_t glen) {
    uint64_t words = 0;
    for (uint64_t c = (glen + 1 + kAlnScanTile - 1) / kAlnScanTile; c > 1; c = (c + kAlnScanTile - 1) / kAlnScanTile)
        words += c;
    return words;
}

int pileup_blocks_per_cu() {
    int a = 0;
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(&a, pileup_add_kernel<>, 256, 0) == hipSuccess ? a : 0;
}

hipError_t launch_pileup_add(const PileupParams& p, hipStream_t stream) {
    if (p.n == 0) return hipSuccess;
    // a wave per read, grid-stride past 2^20 blocks
    const uint64_t blocks = std::min<uint64_t>((p.n + 3) / 4, 1u << 20);
    hipLaunchKernelGGL(pileup_add_kernel<>, dim3((unsigned)blocks), dim3(256), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_pileup_add_qual(const PileupParams& p, const PileupQual& q, hipStream_t stream) {
    if (p.n == 0) return hipSuccess;
    const uint64_t blocks = std::min<uint64_t>((p.n + 3) / 4, 1u << 20);
    hipLaunchKernelGGL(pileup_add_kernel<PileupQual>, dim3((unsigned)blocks), dim3(256), 0, stream, p, q);
    return hipGetLastError();
}

hipError_t launch_pileup_add_qsum(const PileupParams& p, const PileupQsum& q, hipStream_t stream) {
    if (p.n == 0) return hipSuccess;
    const uint64_t blocks = std::min<uint64_t>((p.n + 3) / 4, 1u << 20);
    hipLaunchKernelGGL(pileup_add_kernel<PileupQsum>, dim3((unsigned)blocks), dim3(256), 0, stream, p, q);
    return hipGetLastError();
}

hipError_t launch_pileup_finish_qsum(const PileupParams& p, const PileupQsum& q, uint32_t* scan_tmp,
                                     hipStream_t stream) {
    hipError_t e = launch_pileup_finish(p, scan_tmp, stream);
    if (e == hipSuccess) e = scan_in_place(q.d_q, p.glen + 1, scan_tmp, stream);
    if (e != hipSuccess || p.glen == 0) return e;
    hipLaunchKernelGGL(pileup_finish_qsum_kernel, dim3(grid_for(p.glen)), dim3(256), 0, stream, p, q);
    return hipGetLastError();
}

hipError_t launch_pileup_finish(const PileupParams& p, uint32_t* scan_tmp, hipStream_t stream) {
    hipError_t e = scan_in_place(p.d_all, p.glen + 1, scan_tmp, stream);
    if (e == hipSuccess) e = scan_in_place(p.d_rev, p.glen + 1, scan_tmp, stream);
    if (e != hipSuccess || p.glen == 0) return e;
    hipLaunchKernelGGL(pileup_finish_kernel, dim3(grid_for(p.glen)), dim3(256), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_pileup_summary(const PileupParams& p, uint32_t min_depth, unsigned long long* stats,
                                 hipStream_t stream) {
    hipError_t e = hipMemsetAsync(stats, 0, 4 * sizeof(unsigned long long), stream);
    if (e != hipSuccess || p.glen == 0) return e;
    // a few positions per thread: one add per block and field
    hipLaunchKernelGGL(pileup_summary_kernel, dim3(grid_for((p.glen + 7) / 8)), dim3(256), 0, stream, p, min_depth,
                       stats);
    return hipGetLastError();
}

hipError_t launch_pileup_rows(const PileupParams& p, uint64_t pos0, uint64_t m, uint32_t* out, hipStream_t stream) {
    if (m == 0) return hipSuccess;
    hipLaunchKernelGGL(pileup_rows_kernel, dim3(grid_for(m * 8)), dim3(256), 0, stream, p, pos0, m, out);
    return hipGetLastError();
}

}  // namespace msw
