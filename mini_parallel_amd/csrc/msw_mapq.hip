// msw_mapq.hip -- the choice between a read's two candidate loci
// (include/msw.h, "Candidates and mapping quality").  A byte mover shaped like
// strand_select_kernel (msw_strand.hip): sixteen adjacent lanes own a read and
// share the 16-byte chunks of its oriented row.
#include "msw_kernels.h"

namespace msw {
namespace {

constexpr uint32_t kMapqLanes = 16;

// min(60, 120 (s1 - s2) / (match L)), s2 = clamp(sub, 0, s1); 0 when s1 <= 0
// or match L == 0.  Every operand is >= 0 where the division runs, so the
// truncating division is the floor.
__device__ __forceinline__ uint32_t mapq_of(int32_t s1, int32_t sub, int32_t match, uint32_t L) {
    const int64_t den = (int64_t)match * (int64_t)L;
    if (s1 <= 0 || den <= 0) return 0u;
    const int64_t s2 = sub < 0 ? 0 : (sub > s1 ? s1 : sub);
    const int64_t q = 120ll * ((int64_t)s1 - s2) / den;
    return (uint32_t)(q < 60 ? q : 60);
}

// The sixteen lanes of a read sit in one wave and load both scores with the
// same two instructions, waited for by the comparison below, before lane 0
// replaces the primary score.  A losing alternate's row is never read, a
// winning primary's row never written.
__global__ __launch_bounds__(256) void mapq_select_kernel(MapqSelectParams p, uint32_t chunks) {
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint64_t r = t / kMapqLanes;
    if (r >= p.n) return;
    const uint32_t lane = (uint32_t)(t % kMapqLanes);
    const int32_t sp = p.score[r], sa = p.score_a[r];
    const bool alt = sa > sp;  // ties keep candidate 0
    if (lane == 0) {
        const int32_t s1 = alt ? sa : sp, sub = alt ? sp : sa;
        p.sub_score[r] = sub;
        p.cand[r] = alt ? 1 : 0;
        p.mapq[r] = (uint8_t)mapq_of(s1, sub, p.match, p.read_len[r]);
        if (alt) {
            p.score[r] = sa;
            p.win_pos[r] = p.win_pos_a[r];
            if (p.end_i) {
                p.end_i[r] = p.end_i_a[r];
                p.end_j[r] = p.end_j_a[r];
            }
            if (p.win_len) p.win_len[r] = p.win_len_a[r];
            if (p.strand) p.strand[r] = p.strand_a[r];
        }
    }
    if (!alt || !p.oriented) return;
    const uint4* src = reinterpret_cast<const uint4*>(p.oriented_a + r * p.oriented_stride);
    uint4* dst = reinterpret_cast<uint4*>(p.oriented + r * p.oriented_stride);
    for (uint32_t c = lane; c < chunks; c += kMapqLanes) dst[c] = src[c];
}

}  // namespace

hipError_t launch_mapq_select(const MapqSelectParams& p, hipStream_t stream) {
    if (p.n == 0) return hipSuccess;
    uint32_t chunks = 0;
    if (p.oriented) {
        if (p.oriented_stride == 0 || p.oriented_stride % 16 != 0 || ((uintptr_t)p.oriented & 15) != 0 ||
            ((uintptr_t)p.oriented_a & 15) != 0 || p.oriented_stride / 16 > 0xFFFFFFFFull)
            return hipErrorInvalidValue;
        chunks = (uint32_t)(p.oriented_stride / 16);
    }
    const uint64_t nb = (p.n * kMapqLanes + 255u) / 256u;
    if (nb > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mapq_select_kernel, dim3((unsigned)nb), dim3(256), 0, stream, p, chunks);
    return hipGetLastError();
}

int mapq_blocks_per_cu() {
    int a = 0;
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(&a, mapq_select_kernel, 256, 0) == hipSuccess ? a : 0;
}

}  // namespace msw
