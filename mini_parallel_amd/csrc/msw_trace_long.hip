// msw_trace_long.hip -- traceback for pairs past the packed range (read > 384
// or window > 4096, each up to kMaxLongLen): the canonical alignment of
// include/msw.h, bit-exact with sw_trace_kernel (msw_trace.hip), without that
// kernel's full [rows][cols] direction array (268 / 537 MB at 32767 x 32767).
//
// Strip checkpointing, one wave64 per pair, blocks taking slots from the work
// queue (the grid is capped by the scratch budget, msw_trace_sizes.h):
//  * only rows 0..end_i x columns 0..end_j are touched; the rows are cut into
//    strips of 64 R rows; lane l owns rows [l R, l R + R) of the strip and
//    sweeps the columns with the one-column-per-lane skew, H (and Gotoh's F)
//    handed down by one DPP wave_shr:1 each (msw_long.hip's mapping);
//  * forward pass, strips 0..S-2: score-only (no codes, no best cell, one max
//    per cell); lane 63's bottom row is collected by wave_shl:1 and stored 64
//    columns at a time into the block's checkpoint row ckpt[s] (affine: H and
//    F).  Lane 0 of the next strip takes its top input from that row, loaded
//    64 columns at a time into one VGPR and rotated down by wave_shl:1.  Every
//    strip's row is kept;
//  * backward pass, s = S-1 .. 0: strip s is refilled from ckpt[s-1] (zeros
//    for strip 0) with msw_trace.hip's tagged-max direction codes (2 bits
//    linear, 4 affine; 16 / 8 columns per u32) into the block's strip slab
//    [64 R][W]; lane 0 walks the codes from the current (i, j, state) until it
//    stops or i leaves the strip at the top.  The state (an I gap in state F
//    may span strips), the open run (a run crossing the boundary is one op)
//    and the start cell are carried; strip s-1 is refilled for columns 0..j
//    only; a walk that stopped skips the remaining strips;
//  * ops are emitted in reverse into LDS, or into the block's scratch when
//    ops_cap words do not fit, and stored forward by the whole wave at the end;
//  * the direction words always live in the global slab: a strip's rectangle
//    of a long pair (384 rows x the columns left of j) passes any LDS budget
//    except for windows of a few hundred columns;
//  * words one lane writes and another reads through global memory (checkpoint
//    rows, slab words, ops) are read with agent-scope loads past the vector
//    L1, a fence and a barrier between writer and reader: scratch is reused
//    across strips and pairs.
#include "msw_kernels.h"

namespace msw {
namespace {

// -inf for E / F.  Cells reach at most 64 * 32767 < 2^21.  A gap value that is
// never reopened loses gap_extend (<= 1024) per step: over 32767 steps
// kNeg - 32767 * 1024 - goe (<= 31024) > -2^27 - 2^25 - 2^15 > -2^28, and the
// tagged form value * 4 + tag of that is > -2^30: inside i32, as is 2^21 * 4.
constexpr int32_t kNeg = -(1 << 27);
constexpr int32_t kNoMatch = 0x100;  // read code past the rectangle: equals no window byte

// lane l <- src of lane l-1; lane 0 keeps lane0's value of lane 0 (DPP wave_shr:1, bound_ctrl off)
__device__ __forceinline__ int32_t shr1_or(int32_t src, int32_t lane0) {
    return __builtin_amdgcn_update_dpp(lane0, src, 0x138, 0xF, 0xF, false);
}
// lane l <- src of lane l+1; lane 63 keeps in63's value of lane 63 (DPP wave_shl:1, bound_ctrl off)
__device__ __forceinline__ int32_t shl1_or(int32_t src, int32_t in63) {
    return __builtin_amdgcn_update_dpp(in63, src, 0x130, 0xF, 0xF, false);
}
template <class T>
__device__ __forceinline__ T coherent_load(const T* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One strip: rows [0, srows) of `rd` (the strip's first read byte; rows past
// `srows` score as mismatches and are never stored) x columns [0, ccols) of
// the window in lds_win.  top_h / top_f: the checkpoint row above the strip,
// or null (the matrix boundary).  CODED: direction words into dirs[srows][W],
// W = ceil(ccols / columns per word).  Score-only (srows == 64 R): the bottom
// row into out_h / out_f.
template <int R, bool AFFINE, bool CODED>
__device__ __forceinline__ void fill_strip(const TraceParams& p, const uint8_t* rd, int srows, int ccols,
                                           const uint8_t* lds_win, const int32_t* top_h, const int32_t* top_f,
                                           int32_t* out_h, int32_t* out_f, uint32_t* dirs) {
    constexpr int BITS = AFFINE ? 4 : 2, CPW = 32 / BITS, LOG = AFFINE ? 3 : 4;
    const int lane = (int)threadIdx.x;
    const int W = (ccols + CPW - 1) / CPW;
    const bool bin = top_h != nullptr;  // wave-uniform
    const int32_t gap = p.gap, goe = p.goe;
    const int row0 = lane * R;
    int32_t rb[R], h[R], ee[R];
    uint32_t acc[R];
#pragma unroll
    for (int k = 0; k < R; ++k) {
        rb[k] = row0 + k < srows ? (int32_t)rd[row0 + k] : kNoMatch;
        h[k] = 0;
        ee[k] = kNeg;
        acc[k] = 0;
    }
    int32_t hb = 0, fb = kNeg, dg = 0;  // bottom row H / F of the last step; the top row's diagonal
    int32_t bo_h = 0, bo_f = kNeg;      // lane 63's bottom row of the last 64 steps (oldest in lane 0)
    // coded: the last lane with a row finishes column ccols - 1; score-only: lane 63 does
    const int steps = ccols + (CODED ? (srows - 1) / R : 63);
    // substitution values in VGPRs (v_cndmask operands); coded linear: already
    // the tagged diagonal candidates s * 4 + 2
    const bool tagged = CODED && !AFFINE;
    int32_t vmatch, vmismatch;
    asm volatile("v_mov_b32 %0, %1" : "=v"(vmatch) : "s"(tagged ? p.match * 4 + 2 : p.match));
    asm volatile("v_mov_b32 %0, %1" : "=v"(vmismatch) : "s"(tagged ? p.mismatch * 4 + 2 : p.mismatch));
    const int32_t up4 = 1 - 4 * gap, left4 = -4 * gap;  // linear: (v - gap) * 4 + tag = v * 4 + these
    // the window byte is read one step ahead (index 1 .. ccols + 127 < win_bytes)
    int32_t wnext = lds_win[64 - lane];
    for (int tb = 0; tb < steps; tb += 64) {
        // the row above the strip, columns [tb, tb + 64) (< ckpt_cols); lane 0 holds column t
        int32_t bi_h = 0, bi_f = kNeg;
        if (bin) {
            bi_h = coherent_load(top_h + tb + lane);
            if (AFFINE) bi_f = coherent_load(top_f + tb + lane);
        }
        const int te = min(tb + 64, steps);
        for (int t = tb; t < te; ++t) {
            const int32_t up0 = shr1_or(hb, bi_h);
            int32_t fu = kNeg;
            if (AFFINE) fu = shr1_or(fb, bi_f);
            if (bin) {
                bi_h = shl1_or(bi_h, 0);
                if (AFFINE) bi_f = shl1_or(bi_f, kNeg);
            }
            const int j = t - lane;
            const int32_t w = wnext;
            wnext = lds_win[64 + j + 1];
            const bool ok = (uint32_t)j < (uint32_t)ccols;
            const int sh = (j & (CPW - 1)) * BITS;
            int32_t up = up0, diag = dg;
#pragma unroll
            for (int k = 0; k < R; ++k) {
                const int32_t left = h[k];
                const int32_t sub = rb[k] == w ? vmatch : vmismatch;
                if (CODED) {
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
                    // columns outside [0, ccols) hold H = 0; their codes are never
                    // read: a word starts from zero at its first column and is
                    // stored by a column < ccols
                    x = ok ? x : 3;
                    code |= (uint32_t)x & 3u;
                    acc[k] = (sh == 0 ? 0u : acc[k]) | code << sh;
                    up = x >> 2;
                } else {
                    int32_t x;
                    if (AFFINE) {
                        ee[k] = max(ee[k] - gap, left - goe);
                        fu = max(fu - gap, up - goe);
                        x = max(max(diag + sub, ee[k]), max(fu, 0));
                    } else {
                        x = max(max(diag + sub, max(up, left) - gap), 0);
                    }
                    up = ok ? x : 0;
                }
                diag = left;
                h[k] = up;
            }
            dg = up0;
            hb = h[R - 1];
            if (AFFINE) fb = fu;
            if (CODED) {
                if (ok && ((j & (CPW - 1)) == CPW - 1 || j == ccols - 1)) {
#pragma unroll
                    for (int k = 0; k < R; ++k) {
                        if (row0 + k < srows) dirs[(row0 + k) * W + (j >> LOG)] = acc[k];
                    }
                }
            } else {
                // lane 63 scored column c = t - 63 of the strip's bottom row
                const int c = t - 63;
                bo_h = shl1_or(bo_h, hb);
                if (AFFINE) bo_f = shl1_or(bo_f, fb);
                if ((c & 63) == 63 && c >= 63) {  // lanes hold columns [c - 63, c]
                    out_h[c - 63 + lane] = bo_h;
                    if (AFFINE) out_f[c - 63 + lane] = bo_f;
                }
            }
        }
    }
    if (!CODED && (ccols & 63) != 0 && ccols - 64 + lane >= 0) {  // lanes hold columns [ccols - 64, ccols - 1]
        out_h[ccols - 64 + lane] = bo_h;
        if (AFFINE) out_f[ccols - 64 + lane] = bo_f;
    }
    __threadfence();
    __syncthreads();  // the strip's words are stored before another lane loads them
}

// The walk, carried from strip to strip (wave-uniform copies of lane 0's values).
struct Walk {
    int32_t i, j, state;      // state: 0 H, 1 F, 2 E
    int32_t n_ops, si, sj;
    uint32_t cur_op, cur_len;  // the open run
    int32_t done;
};

#ifndef MSW_TRACE_LONG_NO_WALK
// lane 0: from (w.i, w.j, w.state) through the strip whose first row is `base`
template <bool AFFINE>
__device__ __forceinline__ void walk_strip(Walk& w, const uint32_t* dirs, int W, int base, uint32_t* ops,
                                           uint32_t cap) {
    constexpr int BITS = AFFINE ? 4 : 2, CPW = 32 / BITS, LOG = AFFINE ? 3 : 4;
    int i = w.i, j = w.j, state = w.state;
    int32_t n_ops = w.n_ops, si = w.si, sj = w.sj;
    uint32_t cur_op = w.cur_op, cur_len = w.cur_len;
    bool stop = false;
    auto emit = [&](uint32_t op) {
        if (op == cur_op) {
            ++cur_len;
            return;
        }
        if (cur_len) {
            if ((uint32_t)n_ops < cap) ops[n_ops] = cur_len << 4 | cur_op;
            ++n_ops;
        }
        cur_op = op;
        cur_len = 1;
    };
    while (i >= base && j >= 0) {
        const uint32_t c = coherent_load(dirs + (i - base) * W + (j >> LOG)) >> ((j & (CPW - 1)) * BITS);
        if (state == 0) {
            const uint32_t src = c & 3u;
            if (src == 3) {
                stop = true;
                break;
            }
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
    if (stop || i < 0 || j < 0) {  // the walk is over: close the open run
        if (cur_len) {
            if ((uint32_t)n_ops < cap) ops[n_ops] = cur_len << 4 | cur_op;
            ++n_ops;
        }
        w.done = 1;
    }
    w.i = i;
    w.j = j;
    w.state = state;
    w.n_ops = n_ops;
    w.si = si;
    w.sj = sj;
    w.cur_op = cur_op;
    w.cur_len = cur_len;
}
#endif

template <int R, bool AFFINE>
__global__ __launch_bounds__(64) void sw_trace_long_kernel(TraceLongParams q) {
    extern __shared__ uint8_t lds[];  // [64 pad | window | 64 pad] [ops, when they fit]
    const TraceParams& p = q.t;
    constexpr int SR = 64 * R;  // rows per strip
    constexpr int CPW = AFFINE ? 8 : 16;
    uint8_t* const lds_win = lds;
    uint8_t* const mine = q.scratch + (size_t)blockIdx.x * q.block_bytes;
    int32_t* const ckpt = reinterpret_cast<int32_t*>(mine);
    const size_t ckpt_row = (size_t)q.ckpt_cols * (AFFINE ? 2u : 1u);
    uint32_t* const slab = reinterpret_cast<uint32_t*>(mine + q.slab_off);
    uint32_t* const ops = q.ops_in_lds ? reinterpret_cast<uint32_t*>(lds + p.win_bytes)
                                       : reinterpret_cast<uint32_t*>(mine + q.ops_off);
    const int lane = (int)threadIdx.x;

    auto next_slot = [&](uint32_t slot) {
        if (!p.next) return slot + gridDim.x;
        uint32_t k = 0;
        if (lane == 0) k = atomicAdd(p.next, 1u);
        return gridDim.x + (uint32_t)__builtin_amdgcn_readfirstlane((int)k);
    };
    for (uint32_t pair = blockIdx.x; pair < p.n_slots; pair = next_slot(pair)) {
        const int m = p.read_len[pair];
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
        const bool traced = rows > 0 && cols > 0 && rows <= m && cols <= n && (uint32_t)rows <= p.max_rows &&
                            (uint32_t)cols <= p.max_cols && (uint32_t)(cols + CPW - 1) / CPW <= q.slab_w;
        Walk w = {rows - 1, cols - 1, 0, 0, -1, -1, 3u, 0u, 0};
        __syncthreads();  // the previous pair's LDS reads are done
        if (traced) {
            const uint8_t* rd = p.reads + (size_t)pair * p.read_stride;
            for (int k = lane; k < cols; k += 64) lds_win[64 + k] = wn[k];
            __syncthreads();
            const int S = (rows + SR - 1) / SR;  // <= the bound's strips: S - 1 checkpoint rows exist
            for (int s = 0; s + 1 < S; ++s) {
                int32_t* out = ckpt + (size_t)s * ckpt_row;
                const int32_t* top = s ? out - ckpt_row : nullptr;
                fill_strip<R, AFFINE, false>(p, rd + s * SR, SR, cols, lds_win, top, top ? top + q.ckpt_cols : nullptr,
                                             out, out + q.ckpt_cols, nullptr);
            }
            for (int s = S - 1; s >= 0 && !w.done; --s) {
                const int base = s * SR, srows = min(SR, rows - base), ccols = w.j + 1;
                const int32_t* top = s ? ckpt + (size_t)(s - 1) * ckpt_row : nullptr;
                fill_strip<R, AFFINE, true>(p, rd + base, srows, ccols, lds_win, top, top ? top + q.ckpt_cols : nullptr,
                                            nullptr, nullptr, slab);
#ifndef MSW_TRACE_LONG_NO_WALK
                if (lane == 0) walk_strip<AFFINE>(w, slab, (ccols + CPW - 1) / CPW, base, ops, p.ops_cap);
#else
                if (lane == 0) {  // measurement build: every fill, no walk (the outputs are not an alignment)
                    w.i = base - 1;
                    w.done = s == 0;
                }
#endif
                w.i = __builtin_amdgcn_readfirstlane(w.i);
                w.j = __builtin_amdgcn_readfirstlane(w.j);
                w.done = __builtin_amdgcn_readfirstlane(w.done);
                __syncthreads();  // lane 0 has read the slab before the next strip overwrites it
            }
            w.n_ops = __builtin_amdgcn_readfirstlane(w.n_ops);
            w.si = __builtin_amdgcn_readfirstlane(w.si);
            w.sj = __builtin_amdgcn_readfirstlane(w.sj);
            __threadfence();
            __syncthreads();  // lane 0's ops are stored
            if ((uint32_t)w.n_ops <= p.ops_cap) {
                uint32_t* row = p.cigar + (size_t)pair * p.cigar_stride;
                for (int k = lane; k < w.n_ops; k += 64)
                    row[k] = q.ops_in_lds ? ops[w.n_ops - 1 - k] : coherent_load(ops + (w.n_ops - 1 - k));
            }
        }
        if (lane == 0) {
            p.start_i[pair] = (int16_t)w.si;
            p.start_j[pair] = (int16_t)w.sj;
            p.n_cigar[pair] = w.n_ops;
        }
    }
}

template <int R>
hipError_t go(const TraceLongParams& p, bool affine, uint32_t blocks, size_t shm, hipStream_t stream) {
    const dim3 grid(blocks), block(64);
    if (affine) hipLaunchKernelGGL((sw_trace_long_kernel<R, true>), grid, block, shm, stream, p);
    else hipLaunchKernelGGL((sw_trace_long_kernel<R, false>), grid, block, shm, stream, p);
    return hipGetLastError();
}

template <int R>
int resident(bool affine, size_t shm) {
    int nb = 0;
    const hipError_t e =
        affine ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, sw_trace_long_kernel<R, true>, 64, shm)
               : hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, sw_trace_long_kernel<R, false>, 64, shm);
    return e == hipSuccess && nb > 0 ? nb : 0;
}

}  // namespace

int trace_long_blocks_per_cu(bool affine, uint32_t max_read_len, size_t lds_bytes) {
    switch (trace_rows_per_lane(max_read_len)) {
        case 1: return resident<1>(affine, lds_bytes);
        case 2: return resident<2>(affine, lds_bytes);
        case 3: return resident<3>(affine, lds_bytes);
        case 4: return resident<4>(affine, lds_bytes);
        case 5: return resident<5>(affine, lds_bytes);
        default: return resident<6>(affine, lds_bytes);
    }
}

hipError_t launch_sw_trace_long(const TraceLongParams& p, bool affine, uint32_t blocks, size_t lds_bytes,
                                hipStream_t stream) {
    if (p.t.n_slots == 0 || blocks == 0) return hipSuccess;
    if (p.t.max_rows > (uint32_t)kMaxLongLen || p.t.max_cols > (uint32_t)kMaxLongLen || lds_bytes > 64u * 1024u ||
        !p.scratch)
        return hipErrorInvalidValue;
    switch (trace_rows_per_lane(p.t.max_rows)) {
        case 1: return go<1>(p, affine, blocks, lds_bytes, stream);
        case 2: return go<2>(p, affine, blocks, lds_bytes, stream);
        case 3: return go<3>(p, affine, blocks, lds_bytes, stream);
        case 4: return go<4>(p, affine, blocks, lds_bytes, stream);
        case 5: return go<5>(p, affine, blocks, lds_bytes, stream);
        default: return go<6>(p, affine, blocks, lds_bytes, stream);
    }
}

}  // namespace msw
