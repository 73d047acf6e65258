// msw_strand.hip -- both strands (include/msw.h, "Both strands"): the reverse
// complement of a slab of read rows, and the choice between the two
// orientations' scoring results.  Byte movers beside the DP kernels: a thread
// owns 16-byte chunks of an output row, so every row store is a whole uint4 and
// consecutive threads write consecutive chunks of a row (as cut_windows_kernel).
#include <algorithm>

#include "msw_kernels.h"

namespace msw {
namespace {

// 0x80 in every byte of z that is zero (exact: no carry crosses a byte).
__device__ __forceinline__ uint32_t zero_bytes(uint32_t z) {
    return ~(((z & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | z) & 0x80808080u;
}

// comp() of four bytes at once: A <-> T and a <-> t differ by 0x15, C <-> G
// and c <-> g by 0x04; every other byte value stays.  The case bit is folded
// away for the comparison only.
__device__ __forceinline__ uint32_t comp4(uint32_t w) {
    const uint32_t v = w & ~0x20202020u;
    const uint32_t at = zero_bytes(v ^ 0x41414141u) | zero_bytes(v ^ 0x54545454u);
    const uint32_t cg = zero_bytes(v ^ 0x43434343u) | zero_bytes(v ^ 0x47474747u);
    return w ^ ((at >> 7) * 0x15u) ^ ((cg >> 7) * 0x04u);
}

// the low nb bytes of v (nb <= 0: nothing, nb >= 4: all)
__device__ __forceinline__ uint32_t keep_bytes(uint32_t v, int nb) {
    return nb >= 4 ? v : (nb > 0 ? v & ((1u << (8 * nb)) - 1u) : 0u);
}

// out[p][k] = comp(reads[p][L - 1 - k]) for k < L = read_len[p], 0 up to the
// stride.  The 16 output bytes of chunk c come from the source bytes
// [a, a + 16), a = L - 16 - 16 c, backwards.  VEC (rows 4-byte aligned, a whole
// number of dwords long): the five aligned dwords round them, each index
// clamped to the row's last whole dword and a dword in front of the row taken
// as zero, so a chunk that holds the read's first bytes (a < 0) needs no arm
// of its own: the zeros shift in where the read has no byte, and comp(0) = 0.
// One v_alignbyte_b32 and one v_perm_b32 per output dword.  Otherwise byte
// loads, packed into the same dwords.
template <bool VEC>
__global__ __launch_bounds__(256) void revcomp_rows_kernel(const uint8_t* __restrict__ reads,
                                                           const uint16_t* __restrict__ read_len,
                                                           uint64_t read_stride, uint8_t* __restrict__ out,
                                                           uint64_t out_stride, uint32_t chunks, uint64_t n) {
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint64_t p = t / chunks;
    if (p >= n) return;
    const uint32_t c = (uint32_t)(t - p * chunks);
    const int L = (int)min((uint64_t)read_len[p], read_stride);
    const uint8_t* row = reads + p * read_stride;
    const int a = L - 16 - 16 * (int)c;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (a > -16) {
        if constexpr (VEC) {
            const uint32_t* src = reinterpret_cast<const uint32_t*>(row);
            const int last = (int)(read_stride >> 2) - 1, i0 = a >> 2;  // arithmetic shift: floor
            uint32_t x[5];
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                const uint32_t v = src[min(max(i0 + k, 0), last)];
                x[k] = i0 + k < 0 ? 0u : v;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint32_t s = __builtin_amdgcn_alignbyte(x[4 - e], x[3 - e], (uint32_t)a & 3u);
                w[e] = comp4(__builtin_amdgcn_perm(0u, s, 0x00010203u));
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                uint32_t s = 0u;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int i = L - 1 - (16 * (int)c + 4 * e + j);
                    const uint32_t b = row[max(i, 0)];
                    s |= (i >= 0 ? b : 0u) << (8 * j);
                }
                w[e] = comp4(s);
            }
        }
    }
    *reinterpret_cast<uint4*>(out + p * out_stride + 16ull * c) = make_uint4(w[0], w[1], w[2], w[3]);
}

// Source arm of the forward copy: 16-byte loads, dword loads or byte loads.
enum : int { kSrc16 = 0, kSrc4 = 1, kSrc1 = 2 };

// Per read: strand[p] = score_r > score_f (ties: forward).  Reverse wins: its
// results replace the forward ones in score / end_i / end_j, and the oriented
// row already holds the reverse complement.  Forward wins: the forward row
// replaces row p of `oriented`, zero padded.  Sixteen adjacent lanes own a
// read and share its 16-byte chunks; they sit in one wave, so all of them
// have the forward score (one load instruction, waited for by the branch
// below) before the first of them replaces it.
constexpr uint32_t kSelectLanes = 16;
template <int SRC>
__global__ __launch_bounds__(256) void strand_select_kernel(const uint8_t* __restrict__ reads,
                                                            const uint16_t* __restrict__ read_len,
                                                            uint64_t read_stride, uint8_t* __restrict__ oriented,
                                                            uint64_t out_stride, uint32_t chunks, uint64_t n,
                                                            int32_t* score, int16_t* __restrict__ end_i,
                                                            int16_t* __restrict__ end_j,
                                                            const int32_t* __restrict__ score_r,
                                                            const int16_t* __restrict__ end_i_r,
                                                            const int16_t* __restrict__ end_j_r,
                                                            uint8_t* __restrict__ strand) {
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint64_t p = t / kSelectLanes;
    if (p >= n) return;
    const uint32_t lane = (uint32_t)(t % kSelectLanes);
    const int32_t sr = score_r[p];
    const bool rev = sr > score[p];
    if (lane == 0) {
        strand[p] = rev ? 1 : 0;
        if (rev) {
            score[p] = sr;
            if (end_i) {
                end_i[p] = end_i_r[p];
                end_j[p] = end_j_r[p];
            }
        }
    }
    if (rev) return;
    const int L = (int)min((uint64_t)read_len[p], read_stride);
    const uint8_t* row = reads + p * read_stride;
    for (uint32_t c = lane; c < chunks; c += kSelectLanes) {
        const int rem = L - 16 * (int)c;
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        if (rem > 0) {
            if constexpr (SRC == kSrc16) {
                const uint4 v = *reinterpret_cast<const uint4*>(row + 16ull * c);  // rem > 0: inside the row
                w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
            } else if constexpr (SRC == kSrc4) {
                const uint32_t* src = reinterpret_cast<const uint32_t*>(row);
                const int last = (int)(read_stride >> 2) - 1;
#pragma unroll
                for (int e = 0; e < 4; ++e) w[e] = src[min(4 * (int)c + e, last)];
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int i = 16 * (int)c + 4 * e + j;
                        w[e] |= (uint32_t)row[min(i, L - 1)] << (8 * j);
                    }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) w[e] = keep_bytes(w[e], rem - 4 * e);
        }
        *reinterpret_cast<uint4*>(oriented + p * out_stride + 16ull * c) = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// one thread per 16-byte chunk of n rows of `stride` bytes, 256 per block
bool chunk_grid(uint64_t n, uint32_t stride, uint32_t* chunks, unsigned* blocks) {
    *chunks = stride / 16u;
    const uint64_t nb = (n * *chunks + 255u) / 256u;
    *blocks = (unsigned)nb;
    return nb <= 0x7FFFFFFFull;
}

}  // namespace

hipError_t launch_revcomp_rows(const uint8_t* reads, const uint16_t* read_len, uint32_t read_stride, uint64_t n,
                               uint8_t* out, uint32_t out_stride, hipStream_t stream) {
    uint32_t chunks;
    unsigned blocks;
    if (n == 0) return hipSuccess;
    if (out_stride == 0 || out_stride % 16 != 0 || ((uintptr_t)out & 15) != 0 || read_stride == 0 ||
        !chunk_grid(n, out_stride, &chunks, &blocks))
        return hipErrorInvalidValue;
    if (read_vec_ok(reads, read_stride))
        hipLaunchKernelGGL(revcomp_rows_kernel<true>, dim3(blocks), dim3(256), 0, stream, reads, read_len,
                           (uint64_t)read_stride, out, (uint64_t)out_stride, chunks, n);
    else
        hipLaunchKernelGGL(revcomp_rows_kernel<false>, dim3(blocks), dim3(256), 0, stream, reads, read_len,
                           (uint64_t)read_stride, out, (uint64_t)out_stride, chunks, n);
    return hipGetLastError();
}

hipError_t launch_strand_select(const uint8_t* reads, const uint16_t* read_len, uint32_t read_stride, uint64_t n,
                                uint8_t* oriented, uint32_t oriented_stride, int32_t* score, int16_t* end_i,
                                int16_t* end_j, const int32_t* score_r, const int16_t* end_i_r,
                                const int16_t* end_j_r, uint8_t* strand, hipStream_t stream) {
    uint32_t chunks;
    unsigned blocks;
    if (n == 0) return hipSuccess;
    if (oriented_stride == 0 || oriented_stride % 16 != 0 || ((uintptr_t)oriented & 15) != 0 || read_stride == 0 ||
        !chunk_grid(n, oriented_stride, &chunks, &blocks))
        return hipErrorInvalidValue;
    blocks = (unsigned)((n * kSelectLanes + 255u) / 256u);  // n <= 2^31 - 1 (chunk_grid): fits
#define MSW_SELECT(SRC)                                                                                          \
    hipLaunchKernelGGL(strand_select_kernel<SRC>, dim3(blocks), dim3(256), 0, stream, reads, read_len,          \
                       (uint64_t)read_stride, oriented, (uint64_t)oriented_stride, chunks, n, score, end_i, end_j, \
                       score_r, end_i_r, end_j_r, strand)
    if (vec_ok(reads, read_stride)) MSW_SELECT(kSrc16);
    else if (read_vec_ok(reads, read_stride)) MSW_SELECT(kSrc4);
    else MSW_SELECT(kSrc1);
#undef MSW_SELECT
    return hipGetLastError();
}

int strand_blocks_per_cu() {
    int a = 0, b = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&a, revcomp_rows_kernel<true>, 256, 0) != hipSuccess) return 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, strand_select_kernel<kSrc16>, 256, 0) != hipSuccess)
        return 0;
    return std::min(a, b);
}

}  // namespace msw
