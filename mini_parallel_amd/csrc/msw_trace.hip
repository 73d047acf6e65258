// msw_trace.hip -- traceback: start cell and CIGAR of the canonical alignment
// that ends at the best cell a scoring call reported (include/msw.h, "The
// canonical alignment").
//
// Mapping (one wave64 per pair, in the style of msw_long.hip; one block per
// slot, or a capped grid taking slots from a work queue when the direction
// words need a global slab):
//  * only the rectangle rows 0..end_i x columns 0..end_j is filled: nothing
//    outside it can lie on a path into the end cell;
//  * lane l owns rows [l*R, l*R+R) (R = ceil(max read length / 64) <= 6, one
//    strip) and sweeps the columns with the one-column-per-lane skew: at step
//    t it scores column t-l, its top row taking H (and Gotoh's F) of lane
//    l-1's bottom row from the previous step through one DPP wave_shr:1;
//  * i32 cells, exactly the oracle's recurrence (oracle/sw_oracle.c);
//  * per cell a direction code, computed with the contract's precedence
//    (diagonal > I > D, open > extend):
//      linear, 2 bits : 3 stop (H == 0), 2 diagonal, 1 up (I), 0 left (D)
//      affine, 4 bits : bits 0-1 the H source (3 stop, 2 diagonal, 1 F, 0 E),
//                       bit 2 F opened here (F == H[i-1][j] - goe),
//                       bit 3 E opened here (E == H[i][j-1] - goe)
//    The source falls out of the max itself: each candidate enters it as
//    value * 4 + tag, the tags in precedence order (0 * 4 + 3 is the stop
//    candidate), so one max gives H = x >> 2 and the source = x & 3, ties
//    resolved as the contract says, with no compare chain;
//  * a lane ORs the codes of 16 (linear) / 8 (affine) consecutive columns of
//    a row into one u32 and stores it when the word is complete or the row
//    ends: word (i, j / 16 or j / 8) of a row-major [rows][W] array;
//  * that array lives in LDS when the pair's rectangle fits the launch's
//    budget (kTraceLdsWords), else in the block's slab of global scratch; the
//    choice is per pair and wave-uniform, one templated path over both;
//  * lane 0 walks the codes back from (end_i, end_j), run-length merging the
//    ops into an LDS buffer in reverse; the wave then stores them forward to
//    the pair's CIGAR row and lane 0 stores the start cell and the op count.
//    A pair that needs more ops than the row holds keeps its count only.
#include "msw_kernels.h"

namespace msw {
namespace {

constexpr int32_t kNeg = -(1 << 27);  // -inf for E/F: kNeg * 4 and what 4096 steps subtract stay inside i32
constexpr int32_t kNoMatch = 0x100;   // read code past the rectangle: equals no window byte

// lane l <- src of lane l-1; lane 0 <- lane0 (DPP wave_shr:1, bound_ctrl off)
__device__ __forceinline__ int32_t shr1_or(int32_t src, int32_t lane0) {
    return __builtin_amdgcn_update_dpp(lane0, src, 0x138, 0xF, 0xF, false);
}

// direction words written by other lanes of this wave: global ones are read
// past the vector L1 (which may still hold the previous pair's lines)
template <bool GLOBAL>
__device__ __forceinline__ uint32_t dir_load(const uint32_t* p) {
    if (GLOBAL) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return *p;
}

struct Walked {
    int32_t n_ops, start_i, start_j;
};

// Fill rows x cols (the window is in lds_win) and walk back from its last cell.
template <int R, bool AFFINE, bool GLOBAL>
__device__ __forceinline__ Walked trace_pair(const TraceParams& p, const uint8_t* rd, const uint8_t* lds_win,
                                             uint32_t* lds_ops, uint32_t* dirs, int rows, int cols) {
    constexpr int BITS = AFFINE ? 4 : 2, CPW = 32 / BITS, LOG = AFFINE ? 3 : 4;
    const int lane = (int)threadIdx.x;
    const int W = (cols + CPW - 1) / CPW;
    const int32_t gap = p.gap, goe = p.goe;
    const int row0 = lane * R;
    int32_t rb[R], h[R], ee[R];
    uint32_t acc[R];
#pragma unroll
    for (int k = 0; k < R; ++k) {
        rb[k] = row0 + k < rows ? (int32_t)rd[row0 + k] : kNoMatch;
        h[k] = 0;
        ee[k] = kNeg;
        acc[k] = 0;
    }
    int32_t hb = 0, fb = kNeg, dg = 0;  // bottom row H / F of the last step; the top row's diagonal
    const int steps = cols + (rows - 1) / R;  // the last lane with a row finishes column cols - 1
    // the substitution values live in VGPRs (v_cndmask operands), loaded once
    // (linear: already as tagged diagonal candidates, s * 4 + 2)
    int32_t vmatch, vmismatch;
    asm volatile("v_mov_b32 %0, %1" : "=v"(vmatch) : "s"(AFFINE ? p.match : p.match * 4 + 2));
    asm volatile("v_mov_b32 %0, %1" : "=v"(vmismatch) : "s"(AFFINE ? p.mismatch : p.mismatch * 4 + 2));
    const int32_t up4 = 1 - 4 * gap, left4 = -4 * gap;  // linear: (v - gap) * 4 + tag = v * 4 + these
    // the window byte is read one step ahead, so its LDS latency hides under
    // the step's arithmetic (index <= cols + 127 < win_bytes)
    int32_t wnext = lds_win[64 - lane];
    for (int t = 0; t < steps; ++t) {
        const int32_t up0 = shr1_or(hb, 0);
        int32_t fu = kNeg;
        if (AFFINE) fu = shr1_or(fb, kNeg);
        const int j = t - lane;
        const int32_t w = wnext;
        wnext = lds_win[64 + j + 1];
        const bool ok = (uint32_t)j < (uint32_t)cols;
        const int sh = (j & (CPW - 1)) * BITS;
        int32_t up = up0, diag = dg;
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const int32_t left = h[k];
            const int32_t sub = rb[k] == w ? vmatch : vmismatch;
            int32_t x;  // H * 4 + source
            uint32_t code = 0;
            if (AFFINE) {
                const int32_t eopen = left - goe, fopen = up - goe;
                ee[k] = max(ee[k] - gap, eopen);
                fu = max(fu - gap, fopen);
                x = max(max((diag + sub) * 4 + 2, fu * 4 + 1), max(ee[k] * 4, 3));
                code = (fu == fopen ? 4u : 0u) | (ee[k] == eopen ? 8u : 0u);
            } else {
                x = max(max(diag * 4 + sub, up * 4 + up4), max(left * 4 + left4, 3));
            }
            // columns outside [0, cols) hold H = 0, so column 0 sees the
            // boundary; their codes are never read: a word starts from zero
            // at its first column (sh == 0) and is stored by a column < cols
            x = ok ? x : 3;
            code |= (uint32_t)x & 3u;
            acc[k] = (sh == 0 ? 0u : acc[k]) | code << sh;
            diag = left;
            up = x >> 2;
            h[k] = up;
        }
        dg = up0;
        hb = h[R - 1];
        if (AFFINE) fb = fu;
        if (ok && ((j & (CPW - 1)) == CPW - 1 || j == cols - 1)) {
#pragma unroll
            for (int k = 0; k < R; ++k) {
                if (row0 + k < rows) dirs[(row0 + k) * W + (j >> LOG)] = acc[k];
            }
        }
    }
    if (GLOBAL) __threadfence();
    __syncthreads();  // every direction word is stored before lane 0 reads them

    int32_t n_ops = 0, si = -1, sj = -1;
    if (lane == 0) {
        const uint32_t cap = p.ops_cap;
        uint32_t cur_op = 3, cur_len = 0;
        auto emit = [&](uint32_t op) {
            if (op == cur_op) {
                ++cur_len;
                return;
            }
            if (cur_len) {
                if ((uint32_t)n_ops < cap) lds_ops[n_ops] = cur_len << 4 | cur_op;
                ++n_ops;
            }
            cur_op = op;
            cur_len = 1;
        };
        int i = rows - 1, j = cols - 1, state = 0;  // state: 0 H, 1 F, 2 E
        while (i >= 0 && j >= 0) {
            const uint32_t c = dir_load<GLOBAL>(dirs + i * W + (j >> LOG)) >> ((j & (CPW - 1)) * BITS);
            if (state == 0) {
                const uint32_t src = c & 3u;
                if (src == 3) break;
                if (src == 2) {
                    emit(0);
                    si = i;
                    sj = j;
                    --i;
                    --j;
                    continue;
                }
                if (!AFFINE) {
                    emit(src == 1 ? 1u : 2u);
                    if (src == 1) --i;
                    else --j;
                    continue;
                }
                state = src == 1 ? 1 : 2;
            }
            if (state == 1) {
                emit(1);
                --i;
                if (c & 4u) state = 0;
            } else {
                emit(2);
                --j;
                if (c & 8u) state = 0;
            }
        }
        if (cur_len) {
            if ((uint32_t)n_ops < cap) lds_ops[n_ops] = cur_len << 4 | cur_op;
            ++n_ops;
        }
    }
    Walked r;
    r.n_ops = __builtin_amdgcn_readfirstlane(n_ops);
    r.start_i = __builtin_amdgcn_readfirstlane(si);
    r.start_j = __builtin_amdgcn_readfirstlane(sj);
    return r;
}

template <int R, bool AFFINE>
__global__ __launch_bounds__(64) void sw_trace_kernel(TraceParams p) {
    extern __shared__ uint8_t lds[];  // [64 pad | window | 64 pad] [ops] [direction words]
    uint8_t* const lds_win = lds;
    uint32_t* const lds_ops = reinterpret_cast<uint32_t*>(lds + p.win_bytes);
    uint32_t* const lds_dirs = lds_ops + p.ops_cap;
    uint32_t* const slab = p.slab ? p.slab + (size_t)blockIdx.x * p.slab_words : nullptr;
    const int lane = (int)threadIdx.x;

    auto next_slot = [&](uint32_t slot) {
        if (!p.next) return slot + gridDim.x;
        uint32_t k = 0;
        if (lane == 0) k = atomicAdd(p.next, 1u);
        return gridDim.x + (uint32_t)__builtin_amdgcn_readfirstlane((int)k);
    };
    for (uint32_t pair = blockIdx.x; pair < p.n_slots; pair = next_slot(pair)) {
        const int m = p.read_len[pair];
        // the pair's window: its row of the caller's slab, or (wave-uniform
        // select) the genome at win_pos[pair] under the window rule
        const uint8_t* wn;
        int n;
        if (p.genome) {
            const int64_t pos = p.win_pos[pair];
            n = (int)genome_window_len(p.glen, pos, reads_window_want(p.window, (uint32_t)m));
            wn = p.genome + pos;  // read only below n bytes: never when the position is outside the genome
        } else {
            n = p.win_len[pair];
            wn = p.wins + (size_t)pair * p.win_stride;
        }
        // wave-uniform; a best cell outside the pair or the call's bounds is not traced
        int rows = (int)p.end_i[pair] + 1, cols = (int)p.end_j[pair] + 1;
        rows = __builtin_amdgcn_readfirstlane(rows);
        cols = __builtin_amdgcn_readfirstlane(cols);
        const uint64_t words = trace_words(AFFINE, (uint32_t)rows, (uint32_t)cols);
        const bool in_lds = words <= p.lds_words;
        bool traced = rows > 0 && cols > 0 && rows <= m && cols <= n && rows <= 64 * R &&
                      (uint32_t)rows <= p.max_rows && (uint32_t)cols <= p.max_cols &&
                      (in_lds || (slab && words <= p.slab_words));
        Walked r = {0, -1, -1};
        __syncthreads();  // the previous pair's LDS reads are done
        if (traced) {
            const uint8_t* rd = p.reads + (size_t)pair * p.read_stride;
            for (int k = lane; k < cols; k += 64) lds_win[64 + k] = wn[k];
            __syncthreads();
            r = in_lds ? trace_pair<R, AFFINE, false>(p, rd, lds_win, lds_ops, lds_dirs, rows, cols)
                       : trace_pair<R, AFFINE, true>(p, rd, lds_win, lds_ops, slab, rows, cols);
            __syncthreads();  // lane 0's ops are in LDS
            if ((uint32_t)r.n_ops <= p.ops_cap) {
                uint32_t* row = p.cigar + (size_t)pair * p.cigar_stride;
                for (int k = lane; k < r.n_ops; k += 64) row[k] = lds_ops[r.n_ops - 1 - k];
            }
        }
        if (lane == 0) {
            p.start_i[pair] = (int16_t)r.start_i;
            p.start_j[pair] = (int16_t)r.start_j;
            p.n_cigar[pair] = r.n_ops;
        }
    }
}

template <int R>
hipError_t go(const TraceParams& p, bool affine, uint32_t blocks, size_t shm, hipStream_t stream) {
    const dim3 grid(blocks), block(64);
    if (affine) hipLaunchKernelGGL((sw_trace_kernel<R, true>), grid, block, shm, stream, p);
    else hipLaunchKernelGGL((sw_trace_kernel<R, false>), grid, block, shm, stream, p);
    return hipGetLastError();
}

template <int R>
int resident(bool affine, size_t shm) {
    int nb = 0;
    const hipError_t e = affine ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, sw_trace_kernel<R, true>, 64, shm)
                                : hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, sw_trace_kernel<R, false>, 64, shm);
    return e == hipSuccess && nb > 0 ? nb : 0;
}

}  // namespace

int trace_rows_per_lane(uint32_t max_read_len) {
    const int r = (int)((max_read_len + 63u) / 64u);
    return r < 1 ? 1 : (r > kTraceMaxR ? kTraceMaxR : r);
}

size_t trace_lds_layout(TraceParams& p, bool affine) {
    p.win_bytes = (p.max_cols + 128u + 15u) & ~15u;
    // the walk emits at most rows + cols ops
    p.ops_cap = p.cigar_stride < p.max_rows + p.max_cols ? p.cigar_stride : p.max_rows + p.max_cols;
    const uint64_t need = trace_words(affine, p.max_rows, p.max_cols);
    p.lds_words = need < kTraceLdsWords ? (uint32_t)need : kTraceLdsWords;
    return (size_t)p.win_bytes + ((size_t)p.ops_cap + p.lds_words) * sizeof(uint32_t);
}

int trace_blocks_per_cu(bool affine, uint32_t max_read_len, size_t lds_bytes) {
    switch (trace_rows_per_lane(max_read_len)) {
        case 1: return resident<1>(affine, lds_bytes);
        case 2: return resident<2>(affine, lds_bytes);
        case 3: return resident<3>(affine, lds_bytes);
        case 4: return resident<4>(affine, lds_bytes);
        case 5: return resident<5>(affine, lds_bytes);
        default: return resident<6>(affine, lds_bytes);
    }
}

hipError_t launch_sw_trace(const TraceParams& p, bool affine, uint32_t blocks, size_t lds_bytes, hipStream_t stream) {
    if (p.n_slots == 0 || blocks == 0) return hipSuccess;
    if (p.max_rows > (uint32_t)kMaxReadLen || p.max_cols > (uint32_t)kMaxWinLen || lds_bytes > 64u * 1024u)
        return hipErrorInvalidValue;
    switch (trace_rows_per_lane(p.max_rows)) {
        case 1: return go<1>(p, affine, blocks, lds_bytes, stream);
        case 2: return go<2>(p, affine, blocks, lds_bytes, stream);
        case 3: return go<3>(p, affine, blocks, lds_bytes, stream);
        case 4: return go<4>(p, affine, blocks, lds_bytes, stream);
        case 5: return go<5>(p, affine, blocks, lds_bytes, stream);
        default: return go<6>(p, affine, blocks, lds_bytes, stream);
    }
}

}  // namespace msw
