// msw_e2e.hip -- banded end-to-end alignment (include/msw.h, "Banded end-to-end
// alignment"): the whole read, window ends free, no floor at 0.
//
// The mapping is sw_band_kernel's (msw_band.hip): a group of G lanes (16, 32 or
// 64, the smallest with 2G >= B = 2w + 1) serves one pair, lane q owns the
// diagonals 2q and 2q + 1, step s = 2h + parity runs along an anti-diagonal, on
// both steps of one h the lane's row is i = h - q, left and up arrive by one DPP
// move each, and every 64 rows the group stages the bytes of the next 128 steps
// into LDS.  The cell lattice is this kernel's own.
//
// Three kinds of row.  i < -1: no cell.  i = -1: the virtual start row, H = 0
// where the lane's column lies in [-1, W) and its diagonal in the band, "no
// cell" elsewhere; the two values are per-lane constants (se, so), so the row
// costs one compare and two selects per h.  0 <= i < L: the recurrence, with "no
// cell" outside the window or the band.  Lane q reaches row -1 at h = q - 1: lane
// 0 starts on it, which is the registers' initial state.
//
// "No cell" is the sentinel kNeg = -2^29, and H of a cell that does not exist
// is EXACTLY kNeg (one select per step, where the local kernel writes its 0).
// E and F take no select of their own:
//   - a gap can reach an existing cell from a missing one only across the
//     band's two edges, the window's column -1 or the start row.  The edge
//     lanes of a group take kNeg there as the DPP move's `old` operand (for
//     G = 16 the move is row_shr / row_shl, whose row is the group; for G = 64 it
//     is wave_shr / wave_shl; G = 32 alone pays a select);
//   - everywhere else in the missing region every H is kNeg, so E and F are
//     max(kNeg - goe, previous - gap_extend) there: at most kNeg, at least
//     kNeg - goe - 128 gap_extend for E (a row's chain is 2G <= 128 cells long
//     and starts over in every row), at least kNeg - goe for F (the first term
//     holds it).  F of the start row is made of row -2, so it is one of these,
//     and E of the start row is read by no cell of row 0.
// Why the sentinel can neither drift into range nor wrap.  An existing cell
// that no path reaches is made of sentinels only; it gains at most `match` and
// loses at most `-mismatch` per row since the last exact kNeg on its diagonal,
// and a gap term loses goe + gap_extend per cell of a chain that a missing cell
// (exact kNeg) ends, so with match <= 64, mismatch >= -63, gap_open <= 30,000,
// gap_extend <= 1,024 and rows <= 32,767 every such value lies within
// 32,767 x 64 + 31,024 + 128 x 1,024 < 2.3 x 10^6 of kNeg = -5.4 x 10^8.  A cell
// that a path reaches holds a true value: at most 64 L, and at least the score
// of L diagonal steps and one gap inside the band, above -2.3 x 10^6.  The two
// ranges are 5 x 10^8 apart and both far inside an i32, so a true value always
// wins a max against a sentinel, `v > kNeg / 2` tells them apart, and the
// comparisons that make the direction codes never match across them.
//
// Result.  Nothing is tracked in the loop: a lane latches its two H on the one
// h where its row is L - 1, and the group reduces one key, (score + 2^30) << 32
// | (0xFFFF - j): maximum score, then smallest j; key 0 is "row L - 1 has no
// reachable cell" and reports MSW_E2E_NONE.
//
// Traceback.  The codes are sw_band_kernel's ([row][G] bytes in LDS, 4 bits per
// cell, no row for the start row): bits 0-1 the source of H (1 diagonal, 2 F /
// up, 3 E / left; 0 is not written), bit 2 F opened, bit 3 E opened.  Lane 0 of
// the group walks them from (L - 1, end_j) until it steps into row -1, twice,
// counting the runs and then writing them forward.
#include <hip/hip_runtime.h>

#include "msw_kernels.h"
#include "msw_trace_sizes.h"

namespace msw {
namespace {

constexpr int kNeg = -(1 << 29);
constexpr int kReach = kNeg / 2;        // above: a true value; below: a sentinel
constexpr int kBias = 1 << 30;          // score + kBias > 0 for every true value
constexpr int kNone = -2147483647 - 1;  // MSW_E2E_NONE
constexpr int kCentreClamp = 1 << 20;   // |c| beyond any pair: no cell exists

// lane q of a group <- src of lane q - 1; lane 0 of the group gets `edge`
template <int G>
__device__ __forceinline__ int from_lower(int src, int edge, bool first) {
    if (G == 16) return __builtin_amdgcn_update_dpp(edge, src, 0x111, 0xF, 0xF, false);  // row_shr:1
    const int v = __builtin_amdgcn_update_dpp(edge, src, 0x138, 0xF, 0xF, false);        // wave_shr:1
    return G == 64 ? v : (first ? edge : v);
}
// lane q of a group <- src of lane q + 1; lane G - 1 of the group gets `edge`
template <int G>
__device__ __forceinline__ int from_upper(int src, int edge, bool last) {
    if (G == 16) return __builtin_amdgcn_update_dpp(edge, src, 0x101, 0xF, 0xF, false);  // row_shl:1
    const int v = __builtin_amdgcn_update_dpp(edge, src, 0x130, 0xF, 0xF, false);        // wave_shl:1
    return G == 64 ? v : (last ? edge : v);
}

template <bool AFF>
__device__ __forceinline__ uint32_t cell_code(int h, int diag, int f, int e, int f_open, int e_open) {
    uint32_t c = h == diag ? 1u : (h == f ? 2u : 3u);
    if (AFF) c |= (f == f_open ? 4u : 0u) | (e == e_open ? 8u : 0u);
    return c;
}

template <int G, bool AFF, int MODE>
__global__ __launch_bounds__(64) void sw_band_e2e_kernel(const BandParams p) {
    extern __shared__ uint8_t lds[];
    constexpr int NG = 64 / G;
    const int lane = (int)threadIdx.x;
    const int g = lane / G, q = lane % G;
    const int w = (int)p.w, B = 2 * w + 1;
    const uint64_t pair = (uint64_t)blockIdx.x * NG + g;
    const bool live = pair < p.n_pairs;

    // the pair: L rows, W columns starting at seq, centre c relative to seq (as in sw_band_kernel)
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
    // the start row's cells of the two diagonals: (-1, cj - 1) and (-1, cj), columns in [-1, W)
    const int se = (2 * q < B && (unsigned)cj <= (unsigned)W) ? 0 : kNeg;
    const int so = (2 * q + 1 < B && (unsigned)(cj + 1) <= (unsigned)W) ? 0 : kNeg;
    // a group that runs along with its wave without a read of its own latches nothing
    const int last_row = L > 0 ? L - 1 : -(2 * G);

    // before h = 0 the lane stands on row -1 - q: lane 0 on the start row
    int He = first ? se : kNeg, Ho = first ? so : kNeg;
    int Ee = kNeg, Eo = kNeg, Fe = kNeg, Fo = kNeg;
    int lat_e = kNeg, lat_o = kNeg;

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
            const bool seed = i == -1;
            const int none_e = seed ? se : kNeg, none_o = seed ? so : kNeg;
            uint32_t code = 0;
            {  // even step: diagonal 2q; up is the own odd register, left comes from lane q - 1
                const bool ok = row && (unsigned)(i + cj) < We;
                const int hl = from_lower<G>(Ho, kNeg, first);
                const int diag = He + (rb == wb_e ? p.match : p.mismatch);
                int hn, e, f, e_open = 0, f_open = 0;
                if (AFF) {
                    const int el = from_lower<G>(Eo, kNeg, first);
                    e_open = hl - p.goe;
                    f_open = Ho - p.goe;
                    e = max(e_open, el - p.gap);
                    f = max(f_open, Fo - p.gap);
                    Ee = e;
                    Fe = f;
                } else {
                    f = Ho - p.gap;
                    e = hl - p.gap;
                }
                hn = max(diag, max(e, f));
                if (MODE == 2) code = cell_code<AFF>(hn, diag, f, e, f_open, e_open);
                He = ok ? hn : none_e;
            }
            {  // odd step: diagonal 2q + 1; left is the own even register, up comes from lane q + 1
                const bool ok = row && (unsigned)(i + cj + 1) < Wo;
                const int hu = from_upper<G>(He, kNeg, last);
                const int diag = Ho + (rb == wb_o ? p.match : p.mismatch);
                int hn, e, f, e_open = 0, f_open = 0;
                if (AFF) {
                    const int fu = from_upper<G>(Fe, kNeg, last);
                    e_open = He - p.goe;
                    f_open = hu - p.goe;
                    e = max(e_open, Ee - p.gap);
                    f = max(f_open, fu - p.gap);
                    Eo = e;
                    Fo = f;
                } else {
                    e = He - p.gap;
                    f = hu - p.gap;
                }
                hn = max(diag, max(e, f));
                if (MODE == 2) code |= cell_code<AFF>(hn, diag, f, e, f_open, e_open) << 4;
                Ho = ok ? hn : none_o;
            }
            if (i == last_row) {
                lat_e = He;
                lat_o = Ho;
            }
            if (MODE == 2 && row) codes[(size_t)i * G + q] = (uint8_t)code;
            wb_e = wb_o;
        }
    }

    // the group's result: the maximum of row L - 1, then the smallest j
    int score = kNone, ei = -1, ej = -1;
    if (MODE == 0) {
        int v = max(lat_e, lat_o);
        for (int off = G / 2; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, G));
        if (v > kReach) score = v;
    } else {
        const int je = last_row + cj;  // a latched value above kReach is an existing cell's: 0 <= j < W
        uint64_t key = lat_e > kReach ? ((uint64_t)(uint32_t)(lat_e + kBias) << 32) | (uint64_t)(0xFFFF - je) : 0;
        const uint64_t ko = lat_o > kReach ? ((uint64_t)(uint32_t)(lat_o + kBias) << 32) | (uint64_t)(0xFFFE - je) : 0;
        key = max(key, ko);
        for (int off = G / 2; off > 0; off >>= 1) key = max(key, (uint64_t)__shfl_xor(key, off, G));
        if (key) {
            score = (int)(uint32_t)(key >> 32) - kBias;
            ei = L - 1;
            ej = 0xFFFF - (int)(key & 0xFFFF);
        }
    }
    if (live && first) {
        p.score[pair] = score;
        if (MODE >= 1) {
            p.end_i[pair] = (int16_t)ei;
            p.end_j[pair] = (int16_t)ej;
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
    for (int pass = 0; pass < 2 && ei >= 0; ++pass) {
        int i = ei, k = ej - ei - c + w, state = 0, run_op = -1, run_len = 0, r = 0;
        // every emitted op lowers i or j: at most L + W of them, and one more turn per gap for the state change
        for (int turn = 0; turn < 2 * (L + W) + 2 && i >= 0; ++turn) {
            if (k < 0 || k >= B) break;  // never on a reachable cell's codes; keeps a wrong code inside LDS
            const uint32_t code = (codes[(size_t)i * G + (k >> 1)] >> ((k & 1) * 4)) & 15u;
            int op;
            if (state == 0) {
                const uint32_t src = code & 3u;
                if (src == 1) {
                    op = 0;
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
            si = 0;
            sj = c - w + k;  // the walk stepped into (-1, j0), j0 = -1 + c - w + k: start_j = j0 + 1
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
    // the codes of rows 0 .. max_rows - 1 only: the start row keeps none, so the local kernel's sizes hold
    const size_t shm = band_lds_bytes(p.max_rows, mode == 2);
#define MSW_E2E_LAUNCH(AFF, MODE) \
    hipLaunchKernelGGL((sw_band_e2e_kernel<G, AFF, MODE>), grid, block, shm, stream, p)
    if (affine) {
        if (mode == 0) MSW_E2E_LAUNCH(true, 0);
        else if (mode == 1) MSW_E2E_LAUNCH(true, 1);
        else MSW_E2E_LAUNCH(true, 2);
    } else {
        if (mode == 0) MSW_E2E_LAUNCH(false, 0);
        else if (mode == 1) MSW_E2E_LAUNCH(false, 1);
        else MSW_E2E_LAUNCH(false, 2);
    }
#undef MSW_E2E_LAUNCH
    return hipGetLastError();
}

}  // namespace

hipError_t launch_sw_band_e2e(const BandParams& p, bool affine, int mode, hipStream_t stream) {
    if (p.n_pairs == 0) return hipSuccess;
    if (p.w > kBandMaxW || mode < 0 || mode > 2) return hipErrorInvalidValue;
    if (mode == 2 && p.max_rows > kBandTraceMaxRows) return hipErrorInvalidValue;
    const uint32_t lanes = band_group_lanes(p.w);
    return lanes == 16 ? launch_g<16>(p, affine, mode, stream)
                       : (lanes == 32 ? launch_g<32>(p, affine, mode, stream) : launch_g<64>(p, affine, mode, stream));
}

}  // namespace msw
