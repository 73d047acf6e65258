// msw_band.hip -- banded Smith-Waterman (include/msw.h, "Banded alignment";
// DESIGN.md 4.22).
//
// The mapping.  A band of half-width w has B = 2w + 1 diagonals
// k = j - i - c + w in [0, B).  A group of G lanes (16, 32 or 64, the smallest
// with 2G >= B) serves one pair; lane q of the group owns the two adjacent
// diagonals 2q and 2q + 1, one H (and E, F) register each.  A wave carries
// 64 / G pairs and is a block of its own.
//
// Anti-diagonal stepping.  Step s = 2h + parity handles the cells with
// i + j = s + c - w; every lane computes its diagonal of the step's parity, and
// on both steps of one h its row is i = h - q.  So the read length is a step
// count: there are no row registers and no 384 limit.
//   - the diagonal neighbour (i-1, j-1) is the lane's own value of step s - 2;
//   - even step, k = 2q:     up (i-1, j) is the lane's own odd register,
//                            left (i, j-1) is lane q-1's odd register: one DPP
//                            wave_shr:1;
//   - odd step, k = 2q + 1:  left is the lane's own even register, up is lane
//                            q+1's even register: one DPP wave_shl:1.
// Affine E travels with left and F with up, by the same moves: there is no
// in-row dependency and no scan.  A lane at a group's edge takes "no cell"
// instead of its neighbour group's value.
//
// Cells that do not exist (row or column outside the pair, diagonal outside the
// band) get H = 0.  Their E and F need no mask: left of a row's cells and above
// a column's cells every H is 0, so E and F stay <= 0 there by induction, and
// what lies right of a row's cells or below a column's feeds only cells that do
// not exist either.  A non-positive E or F never reaches an H, a best cell or a
// direction code that the walk reads.
//
// Bytes.  Every 64 rows the group stages the 64 + G read bytes and 64 + G + 1
// window bytes of the next 128 steps into LDS (bytes outside the pair as 0),
// read or genome bytes where they lie; a step reads its two bytes from there.
//
// Traceback.  The traced variant packs one 4-bit code per band cell
// ([row][G bytes], the lane's two diagonals in one byte, written once per h):
// bits 0-1 the source of H (0 stop, 1 diagonal, 2 F / up, 3 E / left), bit 2 F
// opened, bit 3 E opened.  Lane 0 of the group then walks them from the best
// cell twice, counting the runs and then writing them in forward order, so the
// row it writes is sw_trace_kernel's: run-length-merged ops, n_cigar beyond the
// stride with nothing written, start_i / start_j.
#include <hip/hip_runtime.h>

#include "msw_kernels.h"
#include "msw_trace_sizes.h"

namespace msw {
namespace {

constexpr int kNeg = -(1 << 29);
constexpr int kCentreClamp = 1 << 20;  // |c| beyond any pair: no cell exists

// lane l <- src of lane l-1 (DPP wave_shr:1); lane 0 keeps `edge`
__device__ __forceinline__ int from_lower(int src, int edge) {
    return __builtin_amdgcn_update_dpp(edge, src, 0x138, 0xF, 0xF, false);
}
// lane l <- src of lane l+1 (DPP wave_shl:1); lane 63 keeps `edge`
__device__ __forceinline__ int from_upper(int src, int edge) {
    return __builtin_amdgcn_update_dpp(edge, src, 0x130, 0xF, 0xF, false);
}

// The direction code of a cell with value h (0 for a cell that does not exist).
template <bool AFF>
__device__ __forceinline__ uint32_t cell_code(int h, int diag, int f, int e, int f_open, int e_open) {
    uint32_t c = h == 0 ? 0u : (h == diag ? 1u : (h == f ? 2u : 3u));
    if (AFF) c |= (f == f_open ? 4u : 0u) | (e == e_open ? 8u : 0u);
    return c;
}

template <int G, bool AFF, int MODE>
__global__ __launch_bounds__(64) void sw_band_kernel(const BandParams p) {
    extern __shared__ uint8_t lds[];
    constexpr int NG = 64 / G;
    const int lane = (int)threadIdx.x;
    const int g = lane / G, q = lane % G;
    const int w = (int)p.w, B = 2 * w + 1;
    const uint64_t pair = (uint64_t)blockIdx.x * NG + g;
    const bool live = pair < p.n_pairs;

    // the pair: L rows, W columns starting at seq, centre c relative to seq
    int L = 0, W = 0, c = 0;
    int64_t origin = 0;
    const uint8_t* seq = nullptr;
    const uint8_t* read = nullptr;
    if (live) {
        L = p.read_len[pair];
        if (L > (int)p.max_rows) L = 0;
        read = p.reads + pair * p.read_stride;
        if (p.genome) {
            const int64_t c64 = p.diag64[pair];
            if (c64 == INT64_MIN) {
                L = 0;
                origin = -1;
            } else if (c64 < -(int64_t)kCentreClamp) {
                c = -kCentreClamp;
            } else {
                origin = c64 > w ? c64 - w : 0;
                c = (int)(c64 - origin);  // min(c64, w)
                const int64_t glen = (int64_t)p.glen;
                const int64_t hi = c64 >= glen ? glen : (c64 + L + w < glen ? c64 + L + w : glen);
                W = hi > origin ? (int)(hi - origin) : 0;
                seq = p.genome + origin;
            }
        } else {
            W = min((int)p.win_len[pair], kMaxLongLen);  // end_j is an int16
            seq = p.wins + pair * p.win_stride;
            const int c32 = p.diag32[pair];
            c = c32 < -kCentreClamp ? -kCentreClamp : (c32 > kCentreClamp ? kCentreClamp : c32);
        }
    }
    // rows h - q for h in [0, L + w): the last cell is (L - 1, diagonal 2w) at h = L - 1 + w
    int nh = (L > 0 && W > 0) ? L + w : 0;
    for (int off = G; off < 64; off <<= 1) nh = max(nh, __shfl_xor(nh, off, 64));
    nh = __builtin_amdgcn_readfirstlane(nh);

    uint8_t* const rt = lds + g * (2 * (int)kBandTile);
    uint8_t* const wt = rt + kBandTile;
    uint8_t* const codes = lds + kBandTileBytes + (size_t)g * p.max_rows * G;

    const int cj = c - w + 2 * q;  // column of the even diagonal in row i: i + cj
    const unsigned We = 2 * q < B ? (unsigned)W : 0u, Wo = 2 * q + 1 < B ? (unsigned)W : 0u;
    const bool first = q == 0, last = q == G - 1;

    int He = 0, Ho = 0, Ee = kNeg, Eo = kNeg, Fe = kNeg, Fo = kNeg;
    int best = 0, best_s = 0;

    for (int h0 = 0; h0 < nh; h0 += 64) {
        __syncthreads();
        for (int t = q; t < (int)kBandTile; t += G) {
            const int i = h0 - (G - 1) + t, j = h0 + c - w + t;
            rt[t] = (unsigned)i < (unsigned)L ? read[i] : (uint8_t)0;
            wt[t] = (unsigned)j < (unsigned)W ? seq[j] : (uint8_t)0;
        }
        __syncthreads();
        const int hend = min(64, nh - h0);
        int wb_e = wt[q];
        for (int hh = 0; hh < hend; ++hh) {
            const int i = h0 + hh - q;
            const int rb = rt[hh + (G - 1 - q)];
            const int wb_o = wt[hh + q + 1];
            const bool row = (unsigned)i < (unsigned)L;
            uint32_t code = 0;
            {  // even step: diagonal 2q
                const bool ok = row && (unsigned)(i + cj) < We;
                int hl = from_lower(Ho, 0);
                hl = first ? 0 : hl;
                const int diag = He + (rb == wb_e ? p.match : p.mismatch);
                int hn, e = 0, f = 0, e_open = 0, f_open = 0;
                if (AFF) {
                    int el = from_lower(Eo, kNeg);
                    el = first ? kNeg : el;
                    e_open = hl - p.goe;
                    f_open = Ho - p.goe;
                    e = max(e_open, el - p.gap);
                    f = max(f_open, Fo - p.gap);
                    Ee = e;
                    Fe = f;
                    hn = max(max(0, diag), max(e, f));
                } else {
                    f = Ho - p.gap;
                    e = hl - p.gap;
                    hn = max(max(0, diag), max(e, f));
                }
                hn = ok ? hn : 0;
                if (MODE == 0) {
                    best = max(best, hn);
                } else if (hn > best) {
                    best = hn;
                    best_s = 2 * (h0 + hh);
                }
                if (MODE == 2) code = cell_code<AFF>(hn, diag, f, e, f_open, e_open);
                He = hn;
            }
            {  // odd step: diagonal 2q + 1
                const bool ok = row && (unsigned)(i + cj + 1) < Wo;
                // the group's last lane: diagonal 2G - 1 is never in the band, so its H is masked
                // anyway, but its F is not, and the even step of diagonal 2G - 2 reads that F as
                // its up neighbour: it must not be made of the next group's values
                int hu = from_upper(He, 0);
                hu = last ? 0 : hu;
                const int diag = Ho + (rb == wb_o ? p.match : p.mismatch);
                int hn, e = 0, f = 0, e_open = 0, f_open = 0;
                if (AFF) {
                    int fu = from_upper(Fe, kNeg);
                    fu = last ? kNeg : fu;
                    e_open = He - p.goe;
                    f_open = hu - p.goe;
                    e = max(e_open, Ee - p.gap);
                    f = max(f_open, fu - p.gap);
                    Eo = e;
                    Fo = f;
                    hn = max(max(0, diag), max(e, f));
                } else {
                    e = He - p.gap;
                    f = hu - p.gap;
                    hn = max(max(0, diag), max(e, f));
                }
                hn = ok ? hn : 0;
                if (MODE == 0) {
                    best = max(best, hn);
                } else if (hn > best) {
                    best = hn;
                    best_s = 2 * (h0 + hh) + 1;
                }
                if (MODE == 2) code |= cell_code<AFF>(hn, diag, f, e, f_open, e_open) << 4;
                Ho = hn;
            }
            if (MODE == 2 && row) codes[(size_t)i * G + q] = (uint8_t)code;
            wb_e = wb_o;
        }
    }

    // the group's best cell: max score, then smallest i, then smallest j
    int score = best, ei = -1, ek = 0;
    if (MODE == 0) {
        for (int off = G / 2; off > 0; off >>= 1) score = max(score, __shfl_xor(score, off, G));
    } else {
        const int bi = (best_s >> 1) - q, bk = 2 * q + (best_s & 1), bj = bi + c - w + bk;
        uint64_t key = best > 0 ? ((uint64_t)best << 32) | ((uint64_t)(0x7FFF - bi) << 16) | (uint64_t)(0xFFFF - bj) : 0;
        for (int off = G / 2; off > 0; off >>= 1) key = max(key, (uint64_t)__shfl_xor(key, off, G));
        score = (int)(key >> 32);
        if (score > 0) {
            ei = 0x7FFF - (int)((key >> 16) & 0xFFFF);
            ek = (0xFFFF - (int)(key & 0xFFFF)) - ei - c + w;
        }
    }
    if (live && first) {
        p.score[pair] = score;
        if (MODE >= 1) {
            p.end_i[pair] = (int16_t)ei;
            p.end_j[pair] = (int16_t)(score > 0 ? ei + c - w + ek : -1);
        }
        if (p.genome) {
            if (p.win_pos_out) p.win_pos_out[pair] = origin;
            if (p.win_len_out) p.win_len_out[pair] = (uint16_t)W;
        }
    }
    if (MODE != 2) return;

    __syncthreads();
    if (!(live && first)) return;
    int n = 0, si = -1, sj = -1;
    uint32_t* const row_out = p.cigar + pair * p.cigar_stride;
    for (int pass = 0; pass < 2 && score > 0; ++pass) {
        int i = ei, k = ek, state = 0, run_op = -1, run_len = 0, r = 0;
        // every emitted op lowers i or j: at most L + W of them, and one more turn per gap for the state change
        for (int turn = 0; turn < 2 * (L + W) + 2; ++turn) {
            const int j = i + c - w + k;
            if (i < 0 || j < 0 || k < 0 || k >= B) break;
            const uint32_t code = (codes[(size_t)i * G + (k >> 1)] >> ((k & 1) * 4)) & 15u;
            int op;
            if (state == 0) {
                const uint32_t src = code & 3u;
                if (src == 0) break;
                if (src == 1) {
                    op = 0;
                    si = i;
                    sj = j;
                    --i;
                } else if (!AFF) {
                    op = src == 2 ? 1 : 2;
                    if (src == 2) {
                        --i;
                        ++k;
                    } else {
                        --k;
                    }
                } else {
                    state = src == 2 ? 1 : 2;
                    continue;
                }
            } else if (state == 1) {
                op = 1;
                state = (code & 4u) ? 0 : 1;
                --i;
                ++k;
            } else {
                op = 2;
                state = (code & 8u) ? 0 : 2;
                --k;
            }
            if (op == run_op) {
                ++run_len;
            } else {
                if (run_op >= 0) {
                    if (pass) row_out[n - 1 - r] = (uint32_t)run_len << 4 | (uint32_t)run_op;
                    ++r;
                }
                run_op = op;
                run_len = 1;
            }
        }
        if (run_op >= 0) {
            if (pass) row_out[n - 1 - r] = (uint32_t)run_len << 4 | (uint32_t)run_op;
            ++r;
        }
        if (!pass) {
            n = r;
            if ((uint32_t)n > p.cigar_stride) break;  // overflow: the count alone
        }
    }
    p.start_i[pair] = (int16_t)si;
    p.start_j[pair] = (int16_t)sj;
    p.n_cigar[pair] = n;
}

template <int G>
hipError_t launch_g(const BandParams& p, bool affine, int mode, hipStream_t stream) {
    const uint32_t per = 64 / G;
    const dim3 grid((p.n_pairs + per - 1) / per), block(64);
    const size_t shm = band_lds_bytes(p.max_rows, mode == 2);
#define MSW_BAND_LAUNCH(AFF, MODE) \
    hipLaunchKernelGGL((sw_band_kernel<G, AFF, MODE>), grid, block, shm, stream, p)
    if (affine) {
        if (mode == 0) MSW_BAND_LAUNCH(true, 0);
        else if (mode == 1) MSW_BAND_LAUNCH(true, 1);
        else MSW_BAND_LAUNCH(true, 2);
    } else {
        if (mode == 0) MSW_BAND_LAUNCH(false, 0);
        else if (mode == 1) MSW_BAND_LAUNCH(false, 1);
        else MSW_BAND_LAUNCH(false, 2);
    }
#undef MSW_BAND_LAUNCH
    return hipGetLastError();
}

}  // namespace

hipError_t launch_sw_band(const BandParams& p, bool affine, int mode, hipStream_t stream) {
    if (p.n_pairs == 0) return hipSuccess;
    if (p.w > kBandMaxW || mode < 0 || mode > 2) return hipErrorInvalidValue;
    if (mode == 2 && p.max_rows > kBandTraceMaxRows) return hipErrorInvalidValue;
    const uint32_t lanes = band_group_lanes(p.w);
    return lanes == 16 ? launch_g<16>(p, affine, mode, stream)
                       : (lanes == 32 ? launch_g<32>(p, affine, mode, stream) : launch_g<64>(p, affine, mode, stream));
}

}  // namespace msw
