// Host-side check of the long-pair traceback's sizing (msw_trace_sizes.h): for
// bounds from 385 x 1 to 32767 x 32767, both schemes and several cigar strides
// it checks the strip count, the scratch layout, ops_cap, the LDS bytes and the
// grid cap, and that every value the kernel parameters keep in 32 bits fits.
// No GPU.  Build with the host compiler and sanitizers, e.g.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -Imini_parallel_amd/csrc tools/trace_long_sizes.cpp -o /tmp/trace_long_sizes && /tmp/trace_long_sizes
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "msw_trace_sizes.h"

#define CHECK(c)                                                                                        \
    do {                                                                                                \
        if (!(c)) {                                                                                     \
            std::fprintf(stderr, "FAILED %s (rows %u cols %u affine %d stride %u)\n", #c, m, n, (int)aff, cs); \
            return 1;                                                                                   \
        }                                                                                               \
    } while (0)

int main() {
    using namespace msw;
    const uint32_t lens[] = {1, 2, 15, 16, 17, 63, 64, 65, 384, 385, 767, 768, 769, 4096, 4097, 4160, 4161,
                             8191, 16384, 32703, 32704, 32705, 32766, 32767};
    uint64_t cases = 0, worst = 0;
    for (bool aff : {false, true})
        for (uint32_t m : lens)
            for (uint32_t n : lens)
                for (uint32_t cs : {0u, 1u, 64u, 4096u, 4097u, 65534u, 0xFFFFFFFFu}) {
                    const TraceLongLayout l = trace_long_layout(aff, m, n, cs);
                    const uint32_t strip = 64u * l.rows_per_lane, cpw = aff ? 8u : 16u;
                    CHECK(l.rows_per_lane >= 1 && l.rows_per_lane <= kTraceStripR);
                    CHECK((uint64_t)l.strips * strip >= m && (uint64_t)(l.strips - 1) * strip < m);
                    CHECK(m <= 384 ? l.strips == 1 : l.rows_per_lane == 6);
                    // lane 0 loads whole 64-column blocks up to step n + 62
                    CHECK(l.ckpt_cols % 64 == 0 && l.ckpt_cols >= ((n + 62u) | 63u) + 1u && l.ckpt_cols <= 32768u + 128u);
                    CHECK((uint64_t)l.slab_w * cpw >= n && l.slab_w <= 4096u);
                    CHECK(l.ops_cap <= cs && l.ops_cap <= m + n && (l.ops_cap == cs || l.ops_cap == m + n));
                    CHECK(l.win_bytes >= n + 128u && l.win_bytes % 16 == 0);
                    CHECK(l.lds_bytes == l.win_bytes + (l.ops_in_lds ? 4u * l.ops_cap : 0u) && l.lds_bytes <= 64u * 1024u);
                    // the three areas in order, disjoint, inside the block
                    const uint64_t ckpt = (uint64_t)(l.strips - 1) * l.ckpt_cols * (aff ? 8u : 4u);
                    const uint64_t slab = (uint64_t)strip * l.slab_w * 4u;
                    const uint64_t ops = l.ops_in_lds ? 0u : 4ull * l.ops_cap;
                    CHECK(ckpt <= l.slab_off && l.slab_off + slab <= l.ops_off && l.ops_off + ops <= l.block_bytes);
                    CHECK(l.slab_off % 256 == 0 && l.ops_off % 256 == 0 && l.block_bytes % 256 == 0);
                    // in-kernel 32-bit indices: slab words of a strip, i32 of a checkpoint row
                    CHECK((uint64_t)strip * l.slab_w < (1ull << 31) && 2ull * l.ckpt_cols < (1ull << 31));
                    for (uint64_t pairs : {1ull, 9ull, 100000ull, 0x7FFFFFFFull})
                        for (uint64_t resident : {1ull, 256ull * 8})
                            for (uint64_t fixed : {0ull, 1ull, 3ull}) {
                                const uint64_t b = trace_grid_cap(pairs, resident, l.block_bytes, fixed);
                                CHECK(b >= 1 && b <= pairs && b <= resident && (!fixed || b <= fixed));
                                CHECK(b == 1 || b * l.block_bytes <= kTraceSlabBudget);
                                CHECK(b <= 0x7FFFFFFFull && b * l.block_bytes + 256 < (1ull << 40));
                            }
                    if (l.block_bytes > worst) worst = l.block_bytes;
                    ++cases;
                }
    const TraceLongLayout w = trace_long_layout(true, kTraceLongLimit, kTraceLongLimit, 0xFFFFFFFFu);
    std::printf("%llu layouts checked; worst block %llu bytes (32767 x 32767 affine: %u strips, %llu bytes, %llu blocks "
                "in the budget)\n",
                (unsigned long long)cases, (unsigned long long)worst, w.strips, (unsigned long long)w.block_bytes,
                (unsigned long long)trace_grid_cap(1000, 2048, w.block_bytes, 0));
    return worst == w.block_bytes ? 0 : 1;
}
