// msw_call.hip -- variant calls from finished pileup counts
// (msw_pileup_call*, msw_call_counts; include/msw.h "Variants").
//
// One thread per position, a tile of kCallTile positions per block, three
// stages:
//   call_count_kernel  evaluates both site kinds of every position and writes
//                      the tile's number of records into tile_off[tile];
//   scan_in_place      (msw_aln.hip) makes them offsets; entry `tiles` is the total;
//   call_emit_kernel   evaluates again and writes each record at tile offset +
//                      wave offset (LDS wave totals) + lane offset (ballots);
//                      a tile whose two offsets are equal has nothing to write
//                      and its block leaves at once.
// No block waits for another and no atomic decides an output position, so the
// records and their order are a function of the counts alone.
//
// A position's row is read once per pass; depth(pos + 1) of the insertion kind
// comes from the neighbouring lane (__shfl_down), and only a wave's last lane
// or the last position loads a further row.  Every lane reaches every ballot
// and shuffle: the tail is a predicate, never an early return.
#include <algorithm>

#include "msw_kernels.h"

namespace msw {
namespace {

typedef unsigned long long u64;

__device__ __forceinline__ uint32_t base_code(uint32_t b) {
    return b == 'A' ? 0u : b == 'C' ? 1u : b == 'G' ? 2u : b == 'T' ? 3u : 4u;
}

__device__ __forceinline__ uint32_t sat32(u64 v) { return v > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)v; }

struct Row {
    uint32_t c[8];
};

// the row of position k: two 16-byte loads from rows of eight, else eight strided words
__device__ __forceinline__ Row load_row(const CallParams& p, uint64_t k) {
    Row r;
    if (p.pos_mul == 8 && p.ch_mul == 1) {
        const uint4* row = reinterpret_cast<const uint4*>(p.counts + k * 8u);
        const uint4 a = row[0], b = row[1];
        r.c[0] = a.x, r.c[1] = a.y, r.c[2] = a.z, r.c[3] = a.w;
        r.c[4] = b.x, r.c[5] = b.y, r.c[6] = b.z, r.c[7] = b.w;
    } else {
#pragma unroll
        for (int ch = 0; ch < 8; ++ch) r.c[ch] = p.counts[k * p.pos_mul + (uint64_t)ch * p.ch_mul];
    }
    return r;
}

__device__ __forceinline__ u64 row_depth(const Row& r) {
    return (u64)r.c[0] + r.c[1] + r.c[2] + r.c[3] + r.c[4] + r.c[5];
}

// Candidate, genotypes and emission of one site (ref, a, n); fills the record's
// numbers when v != nullptr.  All products in 64 bits, as the header states them.
// W (msw.h, "Quality sums and weighted genotypes"): walt and wref stand for
// a * q_miss and ref * q_miss, the cost of the alternative's observations under
// 0/0 and of the reference's under 1/1; without W they are not read.
template <bool W>
__device__ __forceinline__ bool call_site(const msw_call_params_t& q, u64 n, u64 ref, u64 a, u64 wref, u64 walt,
                                          msw_variant_t* v) {
    if (!(n >= q.min_depth && a >= q.min_alt && 1000ull * a >= (u64)q.min_alt_permille * n)) return false;
    const u64 raw0 = ref * q.q_hit + (W ? walt : a * q.q_miss);
    const u64 raw1 = (ref + a) * q.q_het;
    const u64 raw2 = (W ? wref : ref * q.q_miss) + a * q.q_hit;
    const u64 post0 = raw0, post1 = raw1 + q.prior_het, post2 = raw2 + q.prior_hom;
    uint32_t gt = 0;
    u64 best = post0;
    if (post1 < best) best = post1, gt = 1;
    if (post2 < best) best = post2, gt = 2;
    if (gt == 0) return false;
    const u64 qual = std::min<u64>((post0 - best + 50) / 100, 0xFFFFFFFFull);
    if (qual < q.min_qual) return false;
    if (v) {
        // the second smallest of three: the largest of the pairwise minima
        const u64 second = std::max(std::max(std::min(post0, post1), std::min(post0, post2)), std::min(post1, post2));
        const u64 rmin = std::min(raw0, std::min(raw1, raw2));
        v->qual = (uint32_t)qual;
        v->pl[0] = (uint32_t)std::min<u64>((raw0 - rmin + 50) / 100, 0xFFFFFFFFull);
        v->pl[1] = (uint32_t)std::min<u64>((raw1 - rmin + 50) / 100, 0xFFFFFFFFull);
        v->pl[2] = (uint32_t)std::min<u64>((raw2 - rmin + 50) / 100, 0xFFFFFFFFull);
        v->gt = (uint8_t)gt;
        v->gq = (uint8_t)std::min<u64>(99, (second - best + 50) / 100);
        v->depth = sat32(n);
        v->ref_count = sat32(ref);
        v->alt_count = sat32(a);
    }
    return true;
}

// Both kinds of one position.  Returns bit 0: a column record, bit 1: an
// insertion record; with EMIT the records go to col / ins.
// W: the position's row of quality sums is one 16-byte load beside the counts row.
template <bool EMIT, bool W>
__device__ __forceinline__ uint32_t call_position(const CallParams& p, const Row& r, u64 depth, u64 depth_next,
                                                  uint32_t gbyte, uint64_t pos, msw_variant_t* col,
                                                  msw_variant_t* ins) {
    uint32_t bits = 0;
    const uint32_t rc = base_code(gbyte);
    if (rc < 4) {
        const u64 n = (u64)r.c[0] + r.c[1] + r.c[2] + r.c[3] + r.c[5];
        const uint32_t ref = rc == 0 ? r.c[0] : rc == 1 ? r.c[1] : rc == 2 ? r.c[2] : r.c[3];
        // channels 0, 1, 2, 3 without rc, then 5: the highest count, the lowest index on a tie
        uint32_t a = 0, alt_ch = 8;
#pragma unroll
        for (uint32_t ch = 0; ch < 4; ++ch)
            if (ch != rc && (alt_ch == 8 || r.c[ch] > a)) a = r.c[ch], alt_ch = ch;
        if (r.c[5] > a) a = r.c[5], alt_ch = 5;
        u64 wref = 0, walt = 0;
        if constexpr (W) {
            const uint4 qs = *reinterpret_cast<const uint4*>(p.qsum + (pos - p.pos0) * 4u);
            const uint32_t qr = rc == 0 ? qs.x : rc == 1 ? qs.y : rc == 2 ? qs.z : qs.w;
            const uint32_t qa = alt_ch == 0 ? qs.x : alt_ch == 1 ? qs.y : alt_ch == 2 ? qs.z : qs.w;
            wref = (u64)p.q_scale * qr + (u64)p.q_third * ref;
            // a deleted base has no quality
            walt = alt_ch == 5 ? (u64)a * p.q.q_miss : (u64)p.q_scale * qa + (u64)p.q_third * a;
        }
        if (call_site<W>(p.q, n, ref, a, wref, walt, EMIT ? col : nullptr)) {
            bits |= 1u;
            if (EMIT) {
                col->pos = pos;
                col->kind = alt_ch == 5 ? MSW_VAR_DEL : MSW_VAR_SNV;
                col->ref = (uint8_t)gbyte;
                col->alt = alt_ch == 0 ? 'A' : alt_ch == 1 ? 'C' : alt_ch == 2 ? 'G' : alt_ch == 3 ? 'T' : 0;
            }
        }
    }
    {
        const u64 a = r.c[6];
        const u64 span = std::min(depth, depth_next);
        const u64 ref = span > a ? span - a : 0;
        if (call_site<false>(p.q, ref + a, ref, a, 0, 0, EMIT ? ins : nullptr)) {
            bits |= 2u;
            if (EMIT) {
                ins->pos = pos;
                ins->kind = MSW_VAR_INS;
                ins->ref = (uint8_t)gbyte;
                ins->alt = 0;
            }
        }
    }
    return bits;
}

// What both passes share: the thread's row and genome byte (zeros past m), and
// depth(pos + 1) from the next lane; the wave's last lane and the last position
// load row pos + 1 themselves when the slab holds it.
template <bool EMIT, bool W>
__device__ __forceinline__ uint32_t call_thread(const CallParams& p, uint64_t k, msw_variant_t* col,
                                                msw_variant_t* ins) {
    const bool live = k < p.m;
    // the look-ahead row's loads are issued beside the row's own, not behind the shuffle: one memory round trip
    const bool edge = live && ((threadIdx.x & 63u) == 63u || k + 1 == p.m);
    Row r = {};
    uint32_t gbyte = 0;
    u64 depth_edge = 0;
    if (live) {
        r = load_row(p, k);
        gbyte = p.genome[k];
    }
    if (edge && k + 1 < p.rows) {
        if (p.pos_mul == 8 && p.ch_mul == 1) {
            const uint4 a = *reinterpret_cast<const uint4*>(p.counts + (k + 1) * 8u);
            const uint2 b = *reinterpret_cast<const uint2*>(p.counts + (k + 1) * 8u + 4u);
            depth_edge = (u64)a.x + a.y + a.z + a.w + b.x + b.y;
        } else {
#pragma unroll
            for (int ch = 0; ch < 6; ++ch) depth_edge += p.counts[(k + 1) * p.pos_mul + (uint64_t)ch * p.ch_mul];
        }
    }
    const u64 depth = row_depth(r);
    u64 depth_next = __shfl_down(depth, 1, 64);  // all 64 lanes, live or not
    if (edge) depth_next = depth_edge;
    return live ? call_position<EMIT, W>(p, r, depth, depth_next, gbyte, p.pos0 + k, col, ins) : 0u;
}

template <bool W>
__global__ __launch_bounds__(kCallTile) void call_count_kernel(CallParams p) {
    __shared__ uint32_t wave_n[kCallTile / 64];
    const uint64_t k = (uint64_t)blockIdx.x * kCallTile + threadIdx.x;
    const uint32_t bits = call_thread<false, W>(p, k, nullptr, nullptr);
    const uint32_t n = (uint32_t)__popcll(__ballot(bits & 1u)) + (uint32_t)__popcll(__ballot(bits & 2u));
    if ((threadIdx.x & 63u) == 0) wave_n[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
#pragma unroll
        for (uint32_t w = 0; w < kCallTile / 64; ++w) t += wave_n[w];
        p.tile_off[blockIdx.x] = t;
        // the entry behind the last tile scans into the total
        if (blockIdx.x + 1 == gridDim.x) p.tile_off[gridDim.x] = 0;
    }
}

template <bool W>
__global__ __launch_bounds__(kCallTile) void call_emit_kernel(CallParams p) {
    __shared__ uint32_t wave_n[kCallTile / 64];
    const uint64_t k = (uint64_t)blockIdx.x * kCallTile + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    // a tile without records (most of them: variants are sparse) is not read again; the whole block leaves together
    if (p.tile_off[blockIdx.x + 1] == p.tile_off[blockIdx.x]) return;
    msw_variant_t col = {}, ins = {};  // the padding stays zero
    const uint32_t bits = call_thread<true, W>(p, k, &col, &ins);
    const u64 mc = __ballot(bits & 1u), mi = __ballot(bits & 2u);
    const u64 below = lane ? ~0ull >> (64u - lane) : 0ull;
    if (lane == 0) wave_n[wave] = (uint32_t)__popcll(mc) + (uint32_t)__popcll(mi);
    __syncthreads();
    uint64_t at = p.tile_off[blockIdx.x];
#pragma unroll
    for (uint32_t w = 0; w < kCallTile / 64; ++w) at += w < wave ? wave_n[w] : 0u;
    at += (uint32_t)__popcll(mc & below) + (uint32_t)__popcll(mi & below);
    if (bits & 1u) {
        if (at < p.cap) p.out[at] = col;
        ++at;
    }
    if ((bits & 2u) && at < p.cap) p.out[at] = ins;
}

// *n_total = the scanned total
__global__ void call_total_kernel(const uint32_t* tile_off, uint64_t tiles, unsigned long long* n_total) {
    *n_total = tile_off[tiles];
}

}  // namespace

uint64_t call_tmp_words(uint64_t m) {
    const uint64_t count = call_tiles(m) + 1;
    uint64_t words = count;
    for (uint64_t c = (count + kAlnScanTile - 1) / kAlnScanTile; c > 1; c = (c + kAlnScanTile - 1) / kAlnScanTile)
        words += c;
    return words;
}

hipError_t launch_call_count(const CallParams& p, hipStream_t stream) {
    if (p.m == 0) return hipMemsetAsync(p.tile_off, 0, sizeof(uint32_t), stream);
    if (p.qsum) hipLaunchKernelGGL(call_count_kernel<true>, dim3((unsigned)call_tiles(p.m)), dim3(kCallTile), 0, stream, p);
    else hipLaunchKernelGGL(call_count_kernel<false>, dim3((unsigned)call_tiles(p.m)), dim3(kCallTile), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_call_scan(const CallParams& p, hipStream_t stream) {
    const uint64_t count = call_tiles(p.m) + 1;
    hipError_t e = scan_in_place(p.tile_off, count, p.tile_off + count, stream);
    if (e != hipSuccess || !p.n_total) return e;
    hipLaunchKernelGGL(call_total_kernel, dim3(1), dim3(1), 0, stream, (const uint32_t*)p.tile_off, call_tiles(p.m),
                       p.n_total);
    return hipGetLastError();
}

hipError_t launch_call_emit(const CallParams& p, hipStream_t stream) {
    if (p.m == 0 || p.cap == 0) return hipSuccess;
    if (p.qsum) hipLaunchKernelGGL(call_emit_kernel<true>, dim3((unsigned)call_tiles(p.m)), dim3(kCallTile), 0, stream, p);
    else hipLaunchKernelGGL(call_emit_kernel<false>, dim3((unsigned)call_tiles(p.m)), dim3(kCallTile), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_call(const CallParams& p, hipStream_t stream) {
    hipError_t e = launch_call_count(p, stream);
    if (e == hipSuccess) e = launch_call_scan(p, stream);
    if (e == hipSuccess) e = launch_call_emit(p, stream);
    return e;
}

}  // namespace msw
