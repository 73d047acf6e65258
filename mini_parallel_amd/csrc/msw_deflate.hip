// msw_deflate.hip -- BGZF deflate (RFC 1951 DEFLATE, RFC 1952 framing) on
// gfx950, one wave per BGZF block: the output-side twin of msw_inflate.hip.
//
// A block is <= 65,280 input bytes and becomes one gzip member holding one
// DEFLATE block.  The wave makes two passes:
//  1. parse, 64 positions per window.  Lane l stands at p0 + l, reads its four
//     bytes (two aligned dwords + v_alignbyte), hashes them into a head table
//     in LDS and extends the candidate found there dword-wise (xor + trailing
//     zero count) up to 258 bytes, inside the block and a distance of 32,768.
//     Candidates come from earlier windows only: every lane reads the table
//     first, then all insert their position with an LDS max, so the table
//     never depends on which lane's write lands last.  The greedy token chain
//     (next start = p + len[p], or p + 1) is walked by the scalar unit with
//     v_readlane, a match that leaves the window carrying its rest into the
//     next one; chain lanes append their token to the wave's token buffer
//     (ballot + popcount, coalesced) and count their symbols into the two
//     histograms in LDS (integer adds: the order does not matter);
//  2. codes and emission.  The used symbols are sorted by count in LDS (a
//     bitonic network over the wave), lane 0 runs the in-place two-queue merge
//     (Moffat & Katajainen) and the 15-bit limit on the length counts, the
//     wave assigns lengths by rank and canonical codes by ballots, bit-reversed
//     for DEFLATE's LSB-first packing.  The dynamic size is then known, so the
//     stored form is chosen here when it is not larger.  The token buffer is
//     read back 64 tokens per step: each lane forms its token's <= 48 bits, a
//     DPP scan of the bit counts places them, the lanes OR them into a staging
//     area in LDS (OR commutes: deterministic) and the completed dwords go out
//     with vector stores.
// The CRC-32 of the trailer is msw_inflate.hip's wave-parallel CRC, written
// instead of compared (launch_gz_crc_put).  Members are built at a 64 KiB
// stride and gathered back to back after a scan of their sizes; no block
// waits for another.  Nothing but vector stores and LDS operations writes.
#include <algorithm>

#include "msw_gz.h"

namespace msw {
namespace {

constexpr uint32_t kBlock = kDeflateBlock, kSlot = kDeflateSlot;
constexpr uint32_t kHashBits = 13, kHeads = 1u << kHashBits;
constexpr uint32_t kMinMatch = 4, kMaxMatch = 258, kMaxDist = 32768;
constexpr uint32_t kLit = 286, kDist = 30, kDistAt = 288, kSyms = 320, kEob = 256;
constexpr uint32_t kMaxBits = 15;
constexpr uint32_t kStage = 128;  // dwords: a step places <= 31 + 64 * 48 bits
constexpr uint32_t kMatchTok = 0x80000000u;

// ds_max has no 16-bit form, so a head entry is a dword (position + 1, 0 = empty).
struct Lds {
    uint32_t head[kHeads];   // 32 KiB
    uint32_t hist[kSyms];    // literal/length counts at 0, distance counts at kDistAt
    uint32_t code[kSyms];    // bit-reversed code | length << 16, same places
    uint32_t key[512];       // sort keys: count << 9 | symbol
    uint32_t tree[512];      // the merge's working array: counts, parents, depths
    uint32_t stage[kStage];
    uint32_t blc[16], next[16];
};

// v of the lane the DPP control names, 0 where there is none or the row is masked off
template <int kCtrl, int kRows>
__device__ __forceinline__ uint32_t dpp(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, kCtrl, kRows, 0xF, true);
}

// inclusive prefix sum over the wave: row_shr 1/2/4/8 inside each row of 16,
// then row_bcast:15 into rows 1 and 3 and row_bcast:31 into rows 2 and 3
__device__ __forceinline__ uint32_t wave_inclusive(uint32_t v) {
    v += dpp<0x111, 0xF>(v);
    v += dpp<0x112, 0xF>(v);
    v += dpp<0x114, 0xF>(v);
    v += dpp<0x118, 0xF>(v);
    v += dpp<0x142, 0xA>(v);
    v += dpp<0x143, 0xC>(v);
    return v;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_readlane((int)wave_inclusive(v), 63);
}

// Bytes q .. q + 3 of the block (q < n) from its aligned dwords w.  Only dwords
// that hold a byte of the block are read; bytes at or past n are unspecified.
__device__ __forceinline__ uint32_t load4(const uint32_t* __restrict__ w, uint32_t q, uint32_t last) {
    const uint32_t i = q >> 2;
    const uint32_t lo = w[min(i, last)], hi = w[min(i + 1, last)];
    return __builtin_amdgcn_alignbyte(hi, lo, q & 3);
}

// length - 3 -> length code (symbol - 257), its extra-bit count and value
__device__ __forceinline__ void len_code(uint32_t l, uint32_t& c, uint32_t& eb, uint32_t& ev) {
    if (l < 8) {
        c = l, eb = 0, ev = 0;
    } else if (l == 255) {
        c = 28, eb = 0, ev = 0;
    } else {
        eb = 29u - (uint32_t)__clz((int)l);  // floor(log2 l) - 2
        c = 4 * eb + 4 + ((l >> eb) & 3);
        ev = l & ((1u << eb) - 1);
    }
}
// distance - 1 -> distance code, its extra-bit count and value
__device__ __forceinline__ void dist_code(uint32_t d, uint32_t& c, uint32_t& eb, uint32_t& ev) {
    if (d < 4) {
        c = d, eb = 0, ev = 0;
    } else {
        const uint32_t lg = 31u - (uint32_t)__clz((int)d);
        eb = lg - 1;
        c = 2 * lg + ((d >> eb) & 1);
        ev = d & ((1u << eb) - 1);
    }
}
__device__ __forceinline__ uint32_t lit_extra(uint32_t sym) { return sym >= 265 && sym < 285 ? (sym - 261) >> 2 : 0; }
__device__ __forceinline__ uint32_t dist_extra(uint32_t c) { return c >= 4 ? (c >> 1) - 1 : 0; }

// Length-limited canonical Huffman code of the N-padded alphabet
// hist[base, base + nsym) into code[base ...].  At least two symbols are used.
template <uint32_t N>
__device__ void build_codes(Lds& L, uint32_t base, uint32_t nsym, uint32_t lane) {
    // keys of the used symbols, ascending by count (ties by symbol), unused last
    uint32_t nu = 0;
    for (uint32_t i0 = 0; i0 < N; i0 += 64) {
        const uint32_t i = i0 + lane;
        const uint32_t f = i < nsym ? L.hist[base + i] : 0u;
        if (i < N) L.key[i] = f ? f << 9 | i : 0xFFFFFFFFu;
        nu += (uint32_t)__popcll(__ballot(f != 0));
        if (i < nsym) L.code[base + i] = 0;
    }
    if (lane < 16) L.blc[lane] = 0;
    __syncthreads();
#pragma unroll 1
    for (uint32_t k = 2; k <= N; k <<= 1)
#pragma unroll 1
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = lane; t < N / 2; t += 64) {
                const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const uint32_t a = L.key[i], b = L.key[l];
                if ((a > b) == ((i & k) == 0)) L.key[i] = b, L.key[l] = a;
            }
            __syncthreads();
        }
    for (uint32_t i = lane; i < nu; i += 64) L.tree[i] = L.key[i] >> 9;
    __syncthreads();
    if (lane == 0) {
        // in-place minimum-redundancy code lengths of the sorted counts
        // (Moffat & Katajainen 1995): merge, parent depths, leaf depths
        uint32_t* A = L.tree;
        const int n = (int)nu;
        A[0] += A[1];
        int root = 0, leaf = 2, next;
        for (next = 1; next < n - 1; ++next) {
            if (leaf >= n || A[root] < A[leaf]) A[next] = A[root], A[root++] = (uint32_t)next;
            else A[next] = A[leaf++];
            if (leaf >= n || (root < next && A[root] < A[leaf])) A[next] += A[root], A[root++] = (uint32_t)next;
            else A[next] += A[leaf++];
        }
        A[n - 2] = 0;
        for (next = n - 3; next >= 0; --next) A[next] = A[A[next]] + 1;
        int avbl = 1, used = 0, dpth = 0;
        root = n - 2, next = n - 1;
        while (avbl > 0) {
            while (root >= 0 && (int)A[root] == dpth) ++used, --root;
            while (avbl > used) A[next--] = (uint32_t)dpth, --avbl;
            avbl = 2 * used, ++dpth, used = 0;
        }
    }
    __syncthreads();
    for (uint32_t i = lane; i < nu; i += 64) atomicAdd(&L.blc[min(L.tree[i], kMaxBits)], 1u);
    __syncthreads();
    if (lane == 0) {
        // the 15-bit limit on the counts per length: while the clamped set is
        // over-subscribed, one code leaves the deepest level and a shallower
        // leaf becomes two
        uint32_t total = 0;
        for (uint32_t i = 1; i <= kMaxBits; ++i) total += L.blc[i] << (kMaxBits - i);
        while (total > (1u << kMaxBits)) {
            L.blc[kMaxBits]--;
            for (uint32_t i = kMaxBits - 1; i > 0; --i)
                if (L.blc[i]) {
                    L.blc[i]--;
                    L.blc[i + 1] += 2;
                    break;
                }
            --total;
        }
        uint32_t c = 0;
        for (uint32_t i = 1; i <= kMaxBits; ++i) {
            c = (c + L.blc[i - 1]) << 1;
            L.next[i] = c;
        }
    }
    __syncthreads();
    // lengths by rank: the most frequent symbols take the shortest codes
    for (uint32_t i = lane; i < nu; i += 64) {
        const uint32_t r = nu - 1 - i;
        uint32_t len = 1, cum = L.blc[1];
        while (cum <= r && len < kMaxBits) cum += L.blc[++len];
        L.code[base + (L.key[i] & 511u)] = len << 16;
    }
    __syncthreads();
    // canonical codes in symbol order, 64 symbols per step
    const uint64_t below = (1ull << lane) - 1;
    for (uint32_t s0 = 0; s0 < nsym; s0 += 64) {
        const uint32_t s = s0 + lane;
        const uint32_t len = s < nsym ? L.code[base + s] >> 16 : 0u;
        uint32_t cd = 0, add = 0;
#pragma unroll 1
        for (uint32_t b = 1; b <= kMaxBits; ++b) {
            const uint64_t m = __ballot(len == b);
            if (len == b) cd = L.next[b] + (uint32_t)__popcll(m & below);
            if (lane == b) add = (uint32_t)__popcll(m);
        }
        __syncthreads();
        if (lane >= 1 && lane <= kMaxBits) L.next[lane] += add;
        if (len) L.code[base + s] = len << 16 | (__brev(cd) >> (32 - len));
        __syncthreads();
    }
}

// Place nb bits v of every lane after bitpos: OR into the staging dwords,
// store the completed ones, keep the partial one.
__device__ __forceinline__ void emit(Lds& L, uint32_t* __restrict__ outw, uint32_t& bitpos, uint64_t v, uint32_t nb,
                                     uint32_t lane) {
    const uint32_t inc = wave_inclusive(nb);
    const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
    const uint32_t first = bitpos & 31;
    if (nb) {
        const uint32_t off = first + inc - nb, d = off >> 5, s = off & 31;
        const uint64_t lo = v << s;
        const uint32_t w0 = (uint32_t)lo, w1 = (uint32_t)(lo >> 32), w2 = s ? (uint32_t)(v >> (64 - s)) : 0u;
        if (w0) atomicOr(&L.stage[d], w0);
        if (w1) atomicOr(&L.stage[d + 1], w1);
        if (w2) atomicOr(&L.stage[d + 2], w2);
    }
    __syncthreads();
    const uint32_t done = (first + total) >> 5, base = bitpos >> 5;
    for (uint32_t i = lane; i < done; i += 64) outw[base + i] = L.stage[i];
    const uint32_t part = L.stage[done];
    __syncthreads();
    if (done) {
        L.stage[lane] = 0;
        L.stage[lane + 64] = 0;
        __syncthreads();
        if (lane == 0) L.stage[0] = part;
        __syncthreads();
    }
    bitpos += total;
}

__global__ __launch_bounds__(64) void gz_deflate_kernel(const uint8_t* __restrict__ data, uint64_t len, uint32_t nblocks,
                                                        uint8_t* __restrict__ slots, uint32_t* __restrict__ sizes,
                                                        uint32_t* __restrict__ tokens) {
    __shared__ Lds L;
    const uint32_t lane = threadIdx.x;
    const uint64_t below = (1ull << lane) - 1;
    uint32_t* __restrict__ tok = tokens + (size_t)blockIdx.x * kBlock;
    if (blockIdx.x == 0 && lane == 0) sizes[nblocks] = 0;  // the scan turns it into the total
    for (uint32_t b = blockIdx.x; b < nblocks; b += gridDim.x) {
        const uint64_t boff = (uint64_t)b * kBlock;
        const uint32_t n = (uint32_t)min((uint64_t)kBlock, len - boff);  // >= 1
        const uint32_t* __restrict__ w = (const uint32_t*)(data + boff);
        const uint8_t* __restrict__ bytes = data + boff;
        const uint32_t last = (n - 1) >> 2;
        uint8_t* __restrict__ slot = slots + (size_t)b * kSlot;
        uint32_t* __restrict__ outw = (uint32_t*)slot;

        for (uint32_t i = lane; i < kHeads; i += 64) L.head[i] = 0;
        for (uint32_t i = lane; i < kSyms; i += 64) L.hist[i] = 0;
        L.stage[lane] = 0;
        L.stage[lane + 64] = 0;
        __syncthreads();

        // ---- pass 1: parse ------------------------------------------------
        uint32_t ntok = 0, carry = 0;
        for (uint32_t p0 = 0; p0 < n; p0 += 64) {
            const uint32_t p = p0 + lane;
            const bool hv = p + kMinMatch <= n;
            uint32_t v = 0, h = 0, mlen = 1, mdist = 0;
            if (hv) {
                v = load4(w, p, last);
                h = (v * 0x9E3779B1u) >> (32 - kHashBits);
            } else if (p < n) {
                v = bytes[p];
            }
            const bool skip = carry >= 64;  // the whole window lies inside a match
            if (!skip && hv) {
                const uint32_t c1 = L.head[h];
                const uint32_t dist = p + 1 - c1;  // c1 = candidate + 1
                if (c1 && dist <= kMaxDist) {
                    const uint32_t c = c1 - 1, maxl = min(kMaxMatch, n - p);
                    uint32_t m = 0;
                    while (m < maxl) {
                        const uint32_t x = load4(w, p + m, last) ^ load4(w, c + m, last);
                        if (x) {
                            m += (uint32_t)__builtin_ctz(x) >> 3;
                            break;
                        }
                        m += 4;
                    }
                    m = min(m, maxl);
                    if (m >= kMinMatch) mlen = m, mdist = dist;
                }
            }
            __syncthreads();  // every lane has read the table
            if (hv) atomicMax(&L.head[h], p + 1);
            __syncthreads();
            if (skip) {
                carry -= 64;
                continue;
            }
            const uint32_t wend = min(64u, n - p0);
            uint64_t starts = 0;
            uint32_t pos = (uint32_t)__builtin_amdgcn_readfirstlane((int)carry);
            while (pos < wend) {  // the scalar walk of the token chain
                starts |= 1ull << pos;
                pos += (uint32_t)__builtin_amdgcn_readlane((int)mlen, (int)pos);
            }
            carry = pos - wend;
            if ((starts >> lane) & 1) {
                uint32_t t;
                if (mlen >= kMinMatch) {
                    t = kMatchTok | (mlen - 3) << 16 | (mdist - 1);
                    uint32_t c, eb, ev;
                    len_code(mlen - 3, c, eb, ev);
                    atomicAdd(&L.hist[257 + c], 1u);
                    dist_code(mdist - 1, c, eb, ev);
                    atomicAdd(&L.hist[kDistAt + c], 1u);
                } else {
                    t = v & 0xFFu;
                    atomicAdd(&L.hist[t], 1u);
                }
                tok[ntok + (uint32_t)__popcll(starts & below)] = t;
            }
            ntok += (uint32_t)__popcll(starts);
        }
        if (lane == 0) L.hist[kEob] = 1;
        __threadfence_block();  // pass 2 reads the tokens other lanes wrote
        __syncthreads();

        // ---- codes --------------------------------------------------------
        // the real counts stay in registers: lane l owns symbols l, l + 64, ...
        uint32_t cnt[5], dcnt = lane < kDist ? L.hist[kDistAt + lane] : 0u, nlit = 0;
        for (uint32_t k = 0; k < 5; ++k) {
            const uint32_t s = lane + 64 * k;
            cnt[k] = s < kLit ? L.hist[s] : 0u;
            const uint64_t m = __ballot(cnt[k] != 0);
            if (m) nlit = 64 * k + 64 - (uint32_t)__clzll((long long)m);
        }
        // like zlib, at least two distance codes, so that the code is complete
        uint32_t nd = (uint32_t)__popcll(__ballot(dcnt != 0));
        __syncthreads();
        if (lane == 0)
            for (uint32_t k = 0; nd < 2; ++k)
                if (L.hist[kDistAt + k] == 0) L.hist[kDistAt + k] = 1, ++nd;
        __syncthreads();
        const uint64_t dm = __ballot(lane < kDist && L.hist[kDistAt + lane] != 0);
        const uint32_t ndist = 64 - (uint32_t)__clzll((long long)dm);
        build_codes<512>(L, 0, kLit, lane);
        build_codes<32>(L, kDistAt, kDist, lane);

        uint32_t bits = 0;
        for (uint32_t k = 0; k < 5; ++k) {
            const uint32_t s = lane + 64 * k;
            if (cnt[k]) bits += cnt[k] * ((L.code[s] >> 16) + lit_extra(s));
        }
        if (dcnt) bits += dcnt * ((L.code[kDistAt + lane] >> 16) + dist_extra(lane));
        const uint32_t dyn_bits = 17 + 57 + 4 * (nlit + ndist) + wave_sum(bits);
        const uint32_t dyn_bytes = (dyn_bits + 7) >> 3;
        const bool stored = dyn_bytes >= n + 5;
        const uint32_t total = 18 + (stored ? n + 5 : dyn_bytes) + 8;

        // ---- framing: the 16 fixed header bytes as dwords -----------------
        if (lane < 4) {
            const uint32_t hd = lane == 0 ? 0x04088B1Fu : lane == 1 ? 0u : lane == 2 ? 0x0006FF00u : 0x00024342u;
            outw[lane] = hd;
        }
        uint32_t pend;  // payload end
        if (stored) {
            // BSIZE, the stored block's header and the first input byte by
            // byte stores; input byte 1 on lies at the slot's byte 24
            if (lane < 8) {
                const uint32_t hb = lane == 0   ? (total - 1) & 0xFF
                                    : lane == 1 ? (total - 1) >> 8
                                    : lane == 2 ? 1u
                                    : lane == 3 ? n & 0xFF
                                    : lane == 4 ? n >> 8
                                    : lane == 5 ? ~n & 0xFF
                                    : lane == 6 ? (~n >> 8) & 0xFF
                                                : (uint32_t)bytes[0];
                slot[16 + lane] = (uint8_t)hb;
            }
            const uint32_t nd4 = (n - 1) >> 2;  // whole dwords of input bytes 1 ..
            for (uint32_t i = lane; i < nd4; i += 64) outw[6 + i] = load4(w, 1 + 4 * i, last);
            for (uint32_t q = 1 + 4 * nd4 + lane; q < n; q += 64) slot[23 + q] = bytes[q];
            pend = 23 + n;
        } else {
            uint32_t bitpos = 16 * 8;
            if (lane == 0) L.stage[0] = total - 1;  // BSIZE: bytes 16 and 17
            __syncthreads();
            bitpos += 16;
            // block header: BFINAL, BTYPE = 10, HLIT, HDIST, HCLEN = 15; then the
            // code-length code in its transmission order: symbols 0..15 take
            // four bits each, 16 / 17 / 18 none
            {
                uint64_t v = 0;
                uint32_t nb = 0;
                if (lane == 0) v = 1u | 2u << 1 | (nlit - 257) << 3 | (ndist - 1) << 8 | 15u << 13, nb = 17;
                else if (lane < 20) v = lane >= 4 ? 4 : 0, nb = 3;
                emit(L, outw, bitpos, v, nb, lane);
            }
            for (uint32_t s0 = 0; s0 < nlit; s0 += 64) {
                const uint32_t s = s0 + lane;
                emit(L, outw, bitpos, s < nlit ? __brev(L.code[s] >> 16) >> 28 : 0u, s < nlit ? 4 : 0, lane);
            }
            emit(L, outw, bitpos, lane < ndist ? __brev(L.code[kDistAt + lane] >> 16) >> 28 : 0u, lane < ndist ? 4 : 0,
                 lane);
            // ---- pass 2: the tokens ---------------------------------------
            for (uint32_t t0 = 0; t0 < ntok; t0 += 64) {
                uint64_t v = 0;
                uint32_t nb = 0;
                if (t0 + lane < ntok) {
                    const uint32_t t = tok[t0 + lane];
                    if (t & kMatchTok) {
                        uint32_t lc, le, lx, dc, de, dx;
                        len_code((t >> 16) & 0xFF, lc, le, lx);
                        dist_code(t & 0x7FFF, dc, de, dx);
                        const uint32_t e1 = L.code[257 + lc], e2 = L.code[kDistAt + dc];
                        const uint32_t n1 = e1 >> 16, n2 = e2 >> 16;
                        v = (uint64_t)(e1 & 0xFFFF) | (uint64_t)lx << n1 | (uint64_t)(e2 & 0xFFFF) << (n1 + le) |
                            (uint64_t)dx << (n1 + le + n2);
                        nb = n1 + le + n2 + de;
                    } else {
                        const uint32_t e = L.code[t];
                        v = e & 0xFFFF, nb = e >> 16;
                    }
                }
                emit(L, outw, bitpos, v, nb, lane);
            }
            {
                const uint32_t e = L.code[kEob];
                emit(L, outw, bitpos, lane == 0 ? e & 0xFFFF : 0u, lane == 0 ? e >> 16 : 0u, lane);
            }
            // the last partial dword, byte by byte (the trailer follows unaligned)
            pend = (bitpos + 7) >> 3;
            const uint32_t q = (bitpos >> 5) * 4 + lane;
            if (lane < 4 && q < pend) slot[q] = (uint8_t)(L.stage[0] >> (8 * lane));
            __syncthreads();
        }
        // ISIZE; the CRC-32 in front of it is launch_gz_crc_put's
        if (lane < 4) slot[pend + 4 + lane] = (uint8_t)(n >> (8 * lane));
        if (lane == 0) sizes[b] = pend + 8;
        __syncthreads();
    }
}

// Members from their slots to out, back to back: off = the scanned sizes
// (off[n] the group's total), base = the bytes of the groups before.
__global__ __launch_bounds__(256) void gz_gather_kernel(const uint8_t* __restrict__ slots,
                                                        const uint32_t* __restrict__ off, uint32_t n,
                                                        const uint64_t* __restrict__ base, uint8_t* __restrict__ out) {
    const uint64_t o0 = base ? *base : 0;
    for (uint32_t b = blockIdx.x; b < n; b += gridDim.x) {
        const uint32_t size = off[b + 1] - off[b];
        const uint8_t* __restrict__ src = slots + (size_t)b * kSlot;
        const uint32_t* __restrict__ srcw = (const uint32_t*)src;
        uint8_t* __restrict__ dst = out + o0 + off[b];
        const uint32_t head = min(size, (4u - (uint32_t)((uintptr_t)dst & 3)) & 3u);
        const uint32_t nd = (size - head) >> 2;
        if (threadIdx.x < head) dst[threadIdx.x] = src[threadIdx.x];
        for (uint32_t i = threadIdx.x; i < nd; i += 256) {
            const uint32_t q = head + 4 * i;
            const uint32_t lo = srcw[q >> 2], hi = srcw[min((q >> 2) + 1, kSlot / 4 - 1)];
            *(uint32_t*)(dst + q) = __builtin_amdgcn_alignbyte(hi, lo, q & 3);
        }
        for (uint32_t q = head + 4 * nd + threadIdx.x; q < size; q += 256) dst[q] = src[q];
    }
}

// After a group: its bytes join *base; after the last one the EOF member and *out_len.
__global__ __launch_bounds__(64) void gz_finish_kernel(const uint32_t* __restrict__ total, uint64_t* __restrict__ base,
                                                       int first, int last, uint32_t flags, uint8_t* __restrict__ out,
                                                       uint64_t* __restrict__ out_len) {
    static const uint8_t kEof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43,
                                     2,    0,    0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0,    0,    0};
    uint64_t t = (first ? 0 : *base) + (total ? *total : 0u);
    if (!last) {
        if (threadIdx.x == 0) *base = t;
        return;
    }
    if (!(flags & 1u)) {
        if (threadIdx.x < 28) out[t + threadIdx.x] = kEof[threadIdx.x];
        t += 28;
    }
    if (threadIdx.x == 0) *out_len = t;
}

}  // namespace

hipError_t launch_gz_deflate(const uint8_t* data, uint64_t len, uint32_t nblocks, uint32_t waves, uint8_t* slots,
                             uint32_t* sizes, uint32_t* tokens, hipStream_t stream) {
    if (nblocks == 0) return hipSuccess;
    hipLaunchKernelGGL(gz_deflate_kernel, dim3(std::min(nblocks, waves)), dim3(64), 0, stream, data, len, nblocks, slots,
                       sizes, tokens);
    return hipGetLastError();
}

hipError_t launch_gz_gather(const uint8_t* slots, const uint32_t* off, uint32_t nblocks, const uint64_t* base,
                            uint8_t* out, hipStream_t stream) {
    if (nblocks == 0) return hipSuccess;
    hipLaunchKernelGGL(gz_gather_kernel, dim3(std::min(nblocks, 1u << 16)), dim3(256), 0, stream, slots, off, nblocks,
                       base, out);
    return hipGetLastError();
}

hipError_t launch_gz_finish(const uint32_t* total, uint64_t* base, bool first, bool last, uint32_t flags, uint8_t* out,
                            uint64_t* out_len, hipStream_t stream) {
    hipLaunchKernelGGL(gz_finish_kernel, dim3(1), dim3(64), 0, stream, total, base, first ? 1 : 0, last ? 1 : 0, flags,
                       out, out_len);
    return hipGetLastError();
}

}  // namespace msw
