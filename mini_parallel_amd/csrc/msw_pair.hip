// msw_pair.hip -- read pairs (include/msw.h, "Pairs"): the choice among the
// candidate combinations of two mates, the rescue plan, and the insert-size
// histogram.  Rows 2p and 2p + 1 of every per-read array are the mates of pair
// p.  The choice itself is one __device__ function, pair_choose, that the plan
// and the select both call: the plan runs it over two candidates per mate and
// the select over two or three, so the two kernels cannot disagree on it.
#include <algorithm>

#include "msw_kernels.h"

namespace msw {
namespace {

constexpr uint32_t kPairLanes = 16;  // lanes that own one mate's row, as in mapq_select_kernel

// One mate's K candidates as the scoring calls left them, and what the rule
// needs of them.  Index K is "none": it always exists and scores 0.
template <int K>
struct Mate {
    int64_t s[K + 1];
    bool ex[K + 1];
    int64_t left[K], right[K];  // the unclipped span [left_u, right_u)
    uint32_t t[K];              // strand
    int64_t wp[K];
    int16_t ei[K], ej[K];
};

// left_u = win_pos + end_j - end_i: the genome coordinate at which base 0 of
// the oriented read stands when the alignment is continued gap-free from the
// best cell; right_u = left_u + L.  A candidate exists iff win_pos >= 0 and
// score > 0.
// P: the kernel's parameter struct; its c[k] are read with constant k, so the
// pointers stay in scalar registers.
template <int K, class P>
__device__ __forceinline__ Mate<K> load_mate(const P& p, uint64_t r, int64_t L) {
    Mate<K> m;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int32_t s = p.c[k].score[r];
        m.wp[k] = p.c[k].win_pos[r];
        m.ei[k] = p.c[k].end_i[r];
        m.ej[k] = p.c[k].end_j[r];
        m.t[k] = p.c[k].strand[r] != 0 ? 1u : 0u;
        m.s[k] = s;
        m.ex[k] = m.wp[k] >= 0 && s > 0;
        m.left[k] = m.wp[k] + (int64_t)m.ej[k] - (int64_t)m.ei[k];
        m.right[k] = m.left[k] + L;
    }
    m.s[K] = 0;
    m.ex[K] = true;
    return m;
}

// second ? b : a, member by member
template <int K>
__device__ __forceinline__ Mate<K> either(bool second, const Mate<K>& a, const Mate<K>& b) {
    Mate<K> m;
#pragma unroll
    for (int k = 0; k <= K; ++k) {
        m.s[k] = second ? b.s[k] : a.s[k];
        m.ex[k] = second ? b.ex[k] : a.ex[k];
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        m.left[k] = second ? b.left[k] : a.left[k];
        m.right[k] = second ? b.right[k] : a.right[k];
        m.t[k] = second ? b.t[k] : a.t[k];
        m.wp[k] = second ? b.wp[k] : a.wp[k];
        m.ei[k] = second ? b.ei[k] : a.ei[k];
        m.ej[k] = second ? b.ej[k] : a.ej[k];
    }
    return m;
}

// Candidate i of a mate as the select moves it; i = K ("none") is all zeros.
struct Won {
    int64_t s, left, right, wp;
    uint32_t t;
    int16_t ei, ej;
};
template <int K>
__device__ __forceinline__ Won won(const Mate<K>& m, int i) {  // i is a constant once the loops are unrolled
    Won w = {0, 0, 0, 0, 0u, 0, 0};
    if (i < K) w = Won{m.s[i], m.left[i], m.right[i], m.wp[i], m.t[i], m.ei[i], m.ej[i]};
    return w;
}
__device__ __forceinline__ Won either(bool second, const Won& a, const Won& b) {
    return Won{second ? b.s : a.s,   second ? b.left : a.left, second ? b.right : a.right, second ? b.wp : a.wp,
               second ? b.t : a.t,   second ? b.ei : a.ei,     second ? b.ej : a.ej};
}

struct Choice {
    int c[2];        // the chosen candidate of each mate, K: "none"
    Won w[2];        // and what it holds
    int64_t best;    // S of the chosen combination
    int64_t alt[2];  // the largest S among the combinations in which mate m uses another candidate, -1: none
    bool proper;
    bool opposite;   // both chosen candidates exist and their strands differ
    int64_t tlen;    // right_u(r) - left_u(f) of the chosen combination where `opposite`
};

// All (K + 1)^2 combinations in lexicographic order (0 < 1 < 2 < none), a
// strictly larger S replacing the best so far: the smallest (c1, c2) wins a
// tie.  Unrolled and branch-free: a combination with a missing candidate
// carries S = -1 and (none, none), S = 0, is always there.
template <int K>
__device__ __forceinline__ Choice pair_choose(const Mate<K>& a, const Mate<K>& b, const PairRule& q) {
    int64_t S[(K + 1) * (K + 1)];
    Choice ch;
    ch.c[0] = ch.c[1] = K;
    ch.w[0] = ch.w[1] = Won{0, 0, 0, 0, 0u, 0, 0};
    ch.best = -1;
    ch.proper = ch.opposite = false;
    ch.tlen = 0;
#pragma unroll
    for (int i = 0; i <= K; ++i) {
#pragma unroll
        for (int j = 0; j <= K; ++j) {
            bool opp = false, prop = false;
            int64_t tl = 0;
            if (i < K && j < K) {  // known at compile time: "none" is never proper
                opp = a.ex[i] && b.ex[j] && a.t[i] != b.t[j];
                const bool af = a.t[i] == 0;  // f is the strand-0 candidate, r the strand-1 one
                const int64_t lf = af ? a.left[i] : b.left[j], lr = af ? b.left[j] : a.left[i];
                const int64_t rf = af ? a.right[i] : b.right[j], rr = af ? b.right[j] : a.right[i];
                tl = rr - lf;
                prop = opp && lf <= lr && rf <= rr && tl >= (int64_t)q.min_ins && tl <= (int64_t)q.max_ins;
            }
            const bool valid = a.ex[i] && b.ex[j];
            const int64_t s = valid ? a.s[i] + b.s[j] + (prop ? (int64_t)q.pair_bonus : 0) : -1;
            S[i * (K + 1) + j] = s;
            const bool take = s > ch.best;
            ch.best = take ? s : ch.best;
            ch.c[0] = take ? i : ch.c[0];
            ch.c[1] = take ? j : ch.c[1];
            ch.w[0] = either(take, ch.w[0], won<K>(a, i));
            ch.w[1] = either(take, ch.w[1], won<K>(b, j));
            ch.proper = take ? prop : ch.proper;
            ch.opposite = take ? opp : ch.opposite;
            ch.tlen = take ? tl : ch.tlen;
        }
    }
    ch.alt[0] = ch.alt[1] = -1;
#pragma unroll
    for (int i = 0; i <= K; ++i) {
#pragma unroll
        for (int j = 0; j <= K; ++j) {
            const int64_t s = S[i * (K + 1) + j];
            ch.alt[0] = i != ch.c[0] && s > ch.alt[0] ? s : ch.alt[0];
            ch.alt[1] = j != ch.c[1] && s > ch.alt[1] ? s : ch.alt[1];
        }
    }
    return ch;
}

// min(60, 120 (S_best - S_alt) / (match L)); 0 when the mate's own chosen score
// is <= 0 or match L == 0.  S_alt <= S_best, and "none" is an alternative of
// every existing candidate, so the operands are >= 0 where the division runs.
__device__ __forceinline__ uint32_t pair_mapq(int64_t own, int64_t best, int64_t alt, int32_t match, uint32_t L) {
    const int64_t den = (int64_t)match * (int64_t)L;
    if (own <= 0 || den <= 0 || alt < 0) return 0u;
    const int64_t q = 120ll * (best - alt) / den;
    return (uint32_t)(q < 60 ? q : 60);
}

__device__ __forceinline__ int32_t saturate_i32(int64_t v) {
    return (int32_t)(v > 2147483647ll ? 2147483647ll : (v < -2147483647ll ? -2147483647ll : v));
}

// One thread per pair: the K = 2 choice, then where each mate's rescue window
// starts.  Mate m is to be rescued iff the chosen combination is not proper
// and its partner's chosen candidate a exists with s_a >= rescue_min_score;
// the window is where a proper mate of a would lie.
__global__ __launch_bounds__(256) void pair_plan_kernel(PairPlanParams p) {
    const uint64_t pr = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (pr >= p.n_pairs) return;
    const uint64_t r0 = 2 * pr;
    const int64_t L[2] = {(int64_t)p.read_len[r0], (int64_t)p.read_len[r0 + 1]};
    const Mate<2> a = load_mate<2>(p, r0, L[0]), b = load_mate<2>(p, r0 + 1, L[1]);
    const Choice ch = pair_choose<2>(a, b, p.rule);
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const Won& o = ch.w[1 - m];  // the partner's chosen candidate, the anchor of mate m's window
        const int64_t la = o.left, ra = o.right;
        const uint32_t ta = o.t;
        const bool go = !ch.proper && ch.c[1 - m] < 2 && o.s >= (int64_t)p.rule.rescue_min_score;
        // t_a = 0: right_u(m) in [left_u(a) + min_ins, left_u(a) + max_ins];
        // t_a = 1: left_u(m) in [right_u(a) - max_ins, right_u(a) - min_ins]
        int64_t wp = ta == 0 ? la + p.rule.min_ins - L[m] - p.rule.slack : ra - p.rule.max_ins - p.rule.slack;
        wp = wp < 0 ? 0 : wp;
        p.rescue_pos[r0 + m] = go ? wp : -1;
    }
}

// Sixteen adjacent lanes own a mate's row, so thirty-two own a pair: they sit
// in one wave, load both mates' candidates with the same instructions and come
// to the same choice, and every load is waited for by that choice before lane 0
// of a mate replaces candidate 0's scalars.  Rows move in 16-byte chunks and
// only where candidate 1 or 2 won: a losing row is never read, a winning
// candidate 0's row never written.
template <int K>
__global__ __launch_bounds__(256) void pair_select_kernel(PairSelectParams p, uint32_t chunks) {
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint64_t r = t / kPairLanes, pr = r >> 1;
    if (pr >= p.n_pairs) return;
    const uint32_t lane = (uint32_t)(t % kPairLanes), m = (uint32_t)(r & 1);
    const uint64_t r0 = 2 * pr;
    const uint32_t L0 = p.read_len[r0], L1 = p.read_len[r0 + 1];
    const Mate<K> a = load_mate<K>(p, r0, (int64_t)L0), b = load_mate<K>(p, r0 + 1, (int64_t)L1);
    const Choice ch = pair_choose<K>(a, b, p.rule);
    const Mate<K> me = either<K>(m != 0, a, b);
    const int c = m ? ch.c[1] : ch.c[0];
    const Won w = either(m != 0, ch.w[0], ch.w[1]);
    const bool exists = c < K;
    if (lane == 0) {
        int64_t sub = 0;  // the best of the mate's other existing candidates
#pragma unroll
        for (int k = 0; k < K; ++k) sub = k != c && me.ex[k] && me.s[k] > sub ? me.s[k] : sub;
        const int64_t own = w.s;
        p.sub_score[r] = (int32_t)sub;
        p.cand[r] = (uint8_t)(exists ? c : 0);
        p.mapq[r] = (uint8_t)pair_mapq(own, ch.best, m ? ch.alt[1] : ch.alt[0], p.match, m ? L1 : L0);
        if (!exists) {
            p.c[0].score[r] = 0;
        } else if (c > 0) {
            p.c[0].score[r] = (int32_t)own;
            p.c[0].win_pos[r] = w.wp;
            p.c[0].end_i[r] = w.ei;
            p.c[0].end_j[r] = w.ej;
            p.c[0].strand[r] = (uint8_t)w.t;
            p.c[0].win_len[r] = (K == 3 && c == 2 ? p.c[K - 1].win_len : p.c[1].win_len)[r];
        }
        if (m == 0) {
            p.pair_flags[pr] = (uint8_t)((ch.proper ? 1u : 0u) | (K == 3 && ch.c[0] == 2 ? 2u : 0u) |
                                         (K == 3 && ch.c[1] == 2 ? 4u : 0u));
            p.tlen[pr] = ch.opposite ? saturate_i32(ch.tlen) : 0;
        }
    }
    if (!exists || c == 0) return;
    const uint8_t* from = K == 3 && c == 2 ? p.c[K - 1].oriented : p.c[1].oriented;
    const uint4* src = reinterpret_cast<const uint4*>(from + r * p.oriented_stride);
    uint4* dst = reinterpret_cast<uint4*>(p.c[0].oriented + r * p.oriented_stride);
    for (uint32_t k = lane; k < chunks; k += kPairLanes) dst[k] = src[k];
}

// 4096 bins privatised in LDS (16 KB a block): the pairs of a block add with
// ds_add_u32, and after the barrier every thread flushes its 16 bins with a
// global atomic add, zero bins skipped.  Integer adds commute: the histogram
// is the same whatever order they ran in.
__global__ __launch_bounds__(256) void insert_hist_kernel(const int32_t* tlen, const uint8_t* mapq, uint64_t n,
                                                          uint32_t min_mapq, uint32_t* hist) {
    __shared__ uint32_t bins[kInsertBins];
    for (uint32_t k = threadIdx.x; k < kInsertBins; k += 256u) bins[k] = 0u;
    __syncthreads();
    const uint64_t step = (uint64_t)gridDim.x * 256u;
    for (uint64_t pr = (uint64_t)blockIdx.x * 256u + threadIdx.x; pr < n; pr += step) {
        // tlen != 0 only where both chosen candidates exist on opposite strands
        const int32_t tl = tlen[pr];
        const uint32_t q0 = mapq[2 * pr], q1 = mapq[2 * pr + 1];
        if (tl > 0 && tl < (int32_t)kInsertBins && q0 >= min_mapq && q1 >= min_mapq) atomicAdd(&bins[tl], 1u);
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < kInsertBins; k += 256u) {
        const uint32_t v = bins[k];
        if (v) atomicAdd(&hist[k], v);
    }
}

bool rows_ok(const uint8_t* rows, uint64_t stride) {
    return rows && stride != 0 && stride % 16 == 0 && ((uintptr_t)rows & 15) == 0 && stride / 16 <= 0xFFFFFFFFull;
}

}  // namespace

hipError_t launch_pair_plan(const PairPlanParams& p, hipStream_t stream) {
    if (p.n_pairs == 0) return hipSuccess;
    const uint64_t nb = (p.n_pairs + 255u) / 256u;
    if (nb > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pair_plan_kernel, dim3((unsigned)nb), dim3(256), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_pair_select(const PairSelectParams& p, hipStream_t stream) {
    if (p.n_pairs == 0) return hipSuccess;
    if (p.k != 2 && p.k != 3) return hipErrorInvalidValue;
    for (uint32_t k = 0; k < p.k; ++k)
        if (!rows_ok(p.c[k].oriented, p.oriented_stride)) return hipErrorInvalidValue;
    const uint32_t chunks = (uint32_t)(p.oriented_stride / 16);
    if (p.n_pairs > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const uint64_t nb = (p.n_pairs * 2 * kPairLanes + 255u) / 256u;
    if (nb > 0x7FFFFFFFull) return hipErrorInvalidValue;
    if (p.k == 2) hipLaunchKernelGGL(pair_select_kernel<2>, dim3((unsigned)nb), dim3(256), 0, stream, p, chunks);
    else hipLaunchKernelGGL(pair_select_kernel<3>, dim3((unsigned)nb), dim3(256), 0, stream, p, chunks);
    return hipGetLastError();
}

hipError_t launch_insert_hist(const int32_t* tlen, const uint8_t* mapq, uint64_t n_pairs, uint32_t min_mapq,
                              uint32_t* hist, hipStream_t stream) {
    if (n_pairs == 0) return hipSuccess;
    if (n_pairs > 0x7FFFFFFFull) return hipErrorInvalidValue;
    // grid-stride: enough blocks to fill the device, few enough that the flush stays small
    const uint64_t nb = std::min<uint64_t>((n_pairs + 255u) / 256u, 1024u);
    hipLaunchKernelGGL(insert_hist_kernel, dim3((unsigned)nb), dim3(256), 0, stream, tlen, mapq, n_pairs, min_mapq,
                       hist);
    return hipGetLastError();
}

}  // namespace msw
