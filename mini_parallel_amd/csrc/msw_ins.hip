// msw_ins.hip -- the inserted sequences of a pileup (msw_pileup_ins_*,
// include/msw.h "Pileup", "Inserted sequences").
//
// Two stages.  ins_capture_kernel runs behind every add of a MSW_PILEUP_INS
// pileup and appends one 16-byte event per I run to a log; the vote, enqueued
// by msw_pileup_finish, groups the log by position and writes one
// msw_ins_site_t per position that has events.
//
// Capture.  About one read in 50 to 100 carries an I run, so the add's wave per
// read would idle here: one LANE owns one read and walks its few ops alone,
// with the add's own count rule and walk.  The bases are then read by the wave
// together: while any lane holds a pending run (a ballot, so the loop is
// wave-uniform) the lowest such lane broadcasts (i, len, pos, read_len, flip),
// lanes 0..31 load one inserted byte each -- 32 consecutive bytes of the row,
// mirrored and complemented under flip -- and three ballots make the event:
// the low and the high bit of the 32 base codes as two 32-bit planes, and
// "some base is not upper-case ACGT or lies past the read".  Lane 0 takes the
// slots of a round's events with one returning add on the log's cursor and
// stores each event as one 16-byte store.  The cursor counts every event met,
// stored or not, so the events dropped by a full log are cursor - capacity: no
// counter of their own.
//
// Vote.  Channel 6 of the counts is the number of events per position, so its
// exclusive scan (scan_in_place, msw_aln.hip) is where each site's events go;
// ins_fill_kernel moves them there (an atomic per event picks the place inside
// the site's range: the order inside a site depends on the race, nothing that
// is computed from it does).  Flag, scan, write gives the sites in position
// order.  ins_vote_kernel then runs one wave per site and needs no sort: the
// count of an event's allele is the number of events of the site equal to it,
// and an event stands for its allele when no equal event sits before it.
//   up to 64 events: one event per lane, one v_readlane round of the three key
//     words per event of the site;
//   deeper: the site goes through LDS in tiles of kInsVoteTile events per
//     wave; a lane holds kInsOwn events of its own in registers and sweeps
//     every tile by broadcast reads, pass after pass until every event of the
//     site has been an "own" event once.  Exact at any depth, and quadratic in
//     it.
// Each lane keeps the best allele it has seen (count, then the shorter, then
// the smaller sequence) and the highest count among the others; one butterfly
// merge over the wave gives the site's winner and second_count.
#include <algorithm>

#include "msw_kernels.h"

namespace msw {
namespace {

// as in msw_pileup.hip: A 0, C 1, G 2, T 3 (upper case only), anything else 4
__device__ __forceinline__ uint32_t base_code(uint32_t b) {
    return b == 'A' ? 0u : b == 'C' ? 1u : b == 'G' ? 2u : b == 'T' ? 3u : 4u;
}

// comp of "Both strands"
__device__ __forceinline__ uint32_t comp_byte(uint32_t b) {
    const uint32_t u = b & ~0x20u;
    const uint32_t c = u == 'A' ? 'T' : u == 'T' ? 'A' : u == 'C' ? 'G' : u == 'G' ? 'C' : 0u;
    return c ? c | (b & 0x20u) : b;
}

// the value lane `src` holds; src is wave-uniform
__device__ __forceinline__ uint32_t from_lane(uint32_t v, uint32_t src) {
    return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)src);
}

constexpr uint32_t kLenMask = 0x0FFFFFFFu;  // an op's length has 28 bits; the event's flags sit above them

__global__ __launch_bounds__(256) void ins_capture_kernel(PileupParams p, PileupIns ins) {
    const uint32_t lane = threadIdx.x & 63u;
    const int64_t glen = (int64_t)p.glen;
    const uint64_t step = (uint64_t)gridDim.x * 256u;
    // r0: the wave's first read, so every loop around the ballots is wave-uniform
    for (uint64_t r0 = (uint64_t)blockIdx.x * 256u + (threadIdx.x & ~63u); r0 < p.n; r0 += step) {
        const uint64_t r = r0 + lane;
        uint32_t nops = 0, q = 0, rl = 0, flip = 0;
        const uint32_t* ops = p.cigar;
        int64_t i = 0, g = 0;
        if (r < p.n) {
            const int64_t ref = p.ref_pos[r];
            const uint32_t o0 = p.cigar_off[r], o1 = p.cigar_off[r + 1];
            const bool counted = ref >= 0 && p.nm[r] >= 0 && o1 > o0 && o0 >= p.cigar_base &&
                                 (uint64_t)o1 <= p.cigar_cap && (!p.mapq || p.mapq[r] >= p.min_mapq);
            if (counted) {
                nops = o1 - o0;
                ops = p.cigar + (o0 - p.cigar_base);
                rl = p.read_len[r];
                flip = p.strand && p.strand[r] != 0 && p.orient;
                g = ref;
            }
        }
        for (;;) {
            // this lane's walk, on to its next I run that yields an event
            bool pend = false;
            uint32_t ei = 0, elen = 0, epos = 0;
            while (q < nops && g <= glen && !pend) {
                const uint32_t op = ops[q++];
                const int64_t len = (int64_t)(op >> 4);
                const uint32_t code = op & 15u;
                if (code == 0) {
                    i += len;
                    g += len;
                } else if (code == 2) {
                    g += len;
                } else if (code == 1) {
                    if (g >= 1 && g - 1 < glen) {
                        pend = true;
                        // read_len is below 65536: a clamped i keeps every base past the read
                        ei = (uint32_t)std::min<int64_t>(i, 65535);
                        elen = (uint32_t)len;
                        epos = (uint32_t)(g - 1);
                    }
                    i += len;
                } else if (code == 4) {
                    i += len;
                }
            }
            uint64_t mask = __ballot(pend);
            if (!mask) break;
            // one returning add per round: the round's events take consecutive slots (an add per event
            // measured as the whole launch, ~12 ns each on the one address)
            unsigned long long slot = 0;
            if (lane == 0) slot = atomicAdd(ins.cursor, (unsigned long long)__popcll(mask));
            slot = __shfl(slot, 0, 64);
            for (; mask; ++slot) {
                const uint32_t src = (uint32_t)__builtin_ctzll(mask);
                mask &= mask - 1;
                const uint32_t si = from_lane(ei, src), slen = from_lane(elen, src), spos = from_lane(epos, src);
                const uint32_t srl = from_lane(rl, src), sflip = from_lane(flip, src);
                const uint8_t* row = p.rows + (r0 + src) * p.row_stride;
                // base `lane` of the run; t < srl <= row_stride keeps the load inside the row
                const uint32_t t = si + lane;
                const bool mine = lane < std::min(slen, 32u);
                uint32_t c = 4u;
                if (mine && t < srl) c = base_code(sflip ? comp_byte(row[srl - 1u - t]) : (uint32_t)row[t]);
                const uint32_t plane0 = (uint32_t)__ballot(mine && (c & 1u));
                const uint32_t plane1 = (uint32_t)__ballot(mine && (c & 2u));
                const bool other = __ballot(mine && c == 4u) != 0;
                const uint32_t flags = (other ? 1u : 0u) | (slen > 32u ? 2u : 0u);
                if (lane == 0 && slot < ins.cap)
                    ins.log[slot] = make_uint4(spos, slen | flags << 28, flags ? 0u : plane0, flags ? 0u : plane1);
            }
        }
    }
}

// A log that dropped events gives no table: every kernel of the vote sees it and leaves.
__device__ __forceinline__ bool log_whole(const InsVote& v) { return *v.cursor <= v.cap; }

__device__ __forceinline__ uint32_t site_events(const InsVote& v, uint64_t pos) {
    return v.counts[pos * v.pos_mul + 6u * v.ch_mul];
}

// off[pos] = events at pos, sidx[pos] = 1 where there are any; both scanned afterwards
__global__ __launch_bounds__(256) void ins_offsets_kernel(InsVote v) {
    const uint64_t step = (uint64_t)gridDim.x * 256u;
    for (uint64_t pos = (uint64_t)blockIdx.x * 256u + threadIdx.x; pos <= v.glen; pos += step) {
        const uint32_t c = pos < v.glen ? site_events(v, pos) : 0u;
        v.off[pos] = c;
        v.sidx[pos] = c != 0;
    }
}

// every event into its site's range; afterwards off[pos] is the END of the range of pos
__global__ __launch_bounds__(256) void ins_fill_kernel(InsVote v) {
    if (!log_whole(v)) return;
    const uint64_t n = *v.cursor, step = (uint64_t)gridDim.x * 256u;
    for (uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x; e < n; e += step) {
        const uint4 ev = v.log[e];
        const uint32_t j = atomicAdd(v.off + ev.x, 1u);
        if (j < v.cap) v.sorted[j] = ev;
    }
}

// the sites in position order: pos, events, and (in `alleles`, until the vote) where the site's events start
__global__ __launch_bounds__(256) void ins_sites_kernel(InsVote v) {
    const bool whole = log_whole(v);
    if (blockIdx.x == 0 && threadIdx.x == 0) *v.n_sites = whole ? v.sidx[v.glen] : 0ull;
    if (!whole) return;
    const uint64_t step = (uint64_t)gridDim.x * 256u;
    for (uint64_t pos = (uint64_t)blockIdx.x * 256u + threadIdx.x; pos < v.glen; pos += step) {
        const uint32_t c = site_events(v, pos), s = v.sidx[pos];
        if (c == 0 || s >= v.sites_cap) continue;
        msw_ins_site_t rec{};
        rec.pos = (uint32_t)pos;
        rec.events = c;
        rec.alleles = v.off[pos] - c;
        v.sites[s] = rec;
    }
}

// bit k of x to bit 2k
__device__ __forceinline__ uint64_t spread_bits(uint32_t x) {
    uint64_t w = x;
    w = (w | w << 16) & 0x0000FFFF0000FFFFull;
    w = (w | w << 8) & 0x00FF00FF00FF00FFull;
    w = (w | w << 4) & 0x0F0F0F0F0F0F0F0Full;
    w = (w | w << 2) & 0x3333333333333333ull;
    w = (w | w << 1) & 0x5555555555555555ull;
    return w;
}

// What a lane, and after the merge the wave, knows of a site: the best allele with flags == 0 (cnt 0: none
// yet), the highest count among the other such alleles, and the number of alleles of any kind.
struct Tally {
    uint32_t cnt = 0, len = 0;
    uint64_t seq = 0;
    uint32_t second = 0, alleles = 0;
};

__device__ __forceinline__ bool beats(uint32_t cnt, uint32_t len, uint64_t seq, const Tally& t) {
    return cnt != t.cnt ? cnt > t.cnt : len != t.len ? len < t.len : seq < t.seq;
}

// one allele, seen through the one event that stands for it
__device__ __forceinline__ void note(Tally& t, const uint4& ev, uint32_t cnt) {
    ++t.alleles;
    if (ev.y >> 28) return;
    const uint32_t len = ev.y & kLenMask;
    const uint64_t seq = spread_bits(ev.z) | spread_bits(ev.w) << 1;
    if (beats(cnt, len, seq, t)) {
        t.second = std::max(t.second, t.cnt);
        t.cnt = cnt;
        t.len = len;
        t.seq = seq;
    } else {
        t.second = std::max(t.second, cnt);
    }
}

// Two tallies over disjoint sets of alleles.  Two different alleles never tie, so both lanes of a butterfly
// step come to the same result.
__device__ __forceinline__ Tally merged(const Tally& a, const Tally& b) {
    Tally t = beats(b.cnt, b.len, b.seq, a) ? b : a;
    t.second = std::max(std::max(a.second, b.second), std::min(a.cnt, b.cnt));
    t.alleles = a.alleles + b.alleles;
    return t;
}

__device__ __forceinline__ bool same_allele(const uint4& a, uint32_t y, uint32_t z, uint32_t w) {
    return a.y == y && a.z == z && a.w == w;
}

constexpr uint32_t kInsOwn = 4;  // events of its own a lane holds per pass over a deep site

__global__ __launch_bounds__(256) void ins_vote_kernel(InsVote v) {
    // the three key words of a tile's events, per wave
    __shared__ uint32_t tile[4][3][kInsVoteTile];
    if (!log_whole(v)) return;
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint64_t n_sites = std::min<uint64_t>(*v.n_sites, v.sites_cap);
    for (uint64_t s = (uint64_t)blockIdx.x * 4u + w; s < n_sites; s += (uint64_t)gridDim.x * 4u) {
        // wave-uniform: every lane reads the same record
        const msw_ins_site_t site = v.sites[s];
        const uint64_t start = site.alleles;
        // the events of the site lie inside sorted[0, cap) whenever channel 6 and the log agree
        const uint32_t n = (uint32_t)std::min<uint64_t>(site.events, start < v.cap ? v.cap - start : 0);
        const uint4* ev = v.sorted + start;
        Tally t;
        if (n <= 64u) {
            const bool act = lane < n;
            const uint4 mine = act ? ev[lane] : make_uint4(0, 0, 0, 0);
            uint32_t cnt = 0;
            bool first = act;
            for (uint32_t r = 0; r < n; ++r) {
                const bool eq = act && same_allele(mine, from_lane(mine.y, r), from_lane(mine.z, r), from_lane(mine.w, r));
                cnt += eq;
                first = first && !(eq && r < lane);
            }
            if (first) note(t, mine, cnt);
        } else {
            for (uint32_t own0 = 0; own0 < n; own0 += 64u * kInsOwn) {
                uint4 mine[kInsOwn];
                uint32_t cnt[kInsOwn];
                bool first[kInsOwn];
#pragma unroll
                for (uint32_t k = 0; k < kInsOwn; ++k) {
                    const uint32_t idx = own0 + k * 64u + lane;
                    first[k] = idx < n;
                    mine[k] = first[k] ? ev[idx] : make_uint4(0, 0, 0, 0);
                    cnt[k] = 0;
                }
                for (uint32_t t0 = 0; t0 < n; t0 += kInsVoteTile) {
                    const uint32_t m = std::min(kInsVoteTile, n - t0);
                    // the wave's own lanes wrote and will read this tile: no other wave touches it
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    for (uint32_t j = lane; j < m; j += 64u) {
                        const uint4 e = ev[t0 + j];
                        tile[w][0][j] = e.y;
                        tile[w][1][j] = e.z;
                        tile[w][2][j] = e.w;
                    }
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    __builtin_amdgcn_wave_barrier();
#pragma unroll 4
                    for (uint32_t j = 0; j < m; ++j) {
                        const uint32_t y = tile[w][0][j], z = tile[w][1][j], x = tile[w][2][j];
#pragma unroll
                        for (uint32_t k = 0; k < kInsOwn; ++k) {
                            const uint32_t idx = own0 + k * 64u + lane;
                            const bool eq = idx < n && same_allele(mine[k], y, z, x);
                            cnt[k] += eq;
                            first[k] = first[k] && !(eq && t0 + j < idx);
                        }
                    }
                }
#pragma unroll
                for (uint32_t k = 0; k < kInsOwn; ++k)
                    if (first[k]) note(t, mine[k], cnt[k]);
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            Tally o;
            o.cnt = __shfl_xor(t.cnt, off, 64);
            o.len = __shfl_xor(t.len, off, 64);
            o.seq = __shfl_xor(t.seq, off, 64);
            o.second = __shfl_xor(t.second, off, 64);
            o.alleles = __shfl_xor(t.alleles, off, 64);
            t = merged(t, o);
        }
        if (lane == 0) {
            msw_ins_site_t rec{};
            rec.pos = site.pos;
            rec.events = site.events;
            rec.alleles = t.alleles;
            rec.best_count = t.cnt;
            rec.second_count = t.second;
            rec.best_len = t.cnt ? (uint16_t)t.len : (uint16_t)0;
            rec.seq = t.cnt ? t.seq : 0ull;
            v.sites[s] = rec;
        }
    }
}

unsigned grid_for(uint64_t items, uint64_t most) {
    return (unsigned)std::min<uint64_t>(std::max<uint64_t>(1, (items + 255) / 256), most);
}

}  // namespace

hipError_t launch_ins_capture(const PileupParams& p, const PileupIns& ins, hipStream_t stream) {
    if (p.n == 0) return hipSuccess;
    // a lane per read, grid-stride past 2^20 blocks
    hipLaunchKernelGGL(ins_capture_kernel, dim3(grid_for(p.n, 1u << 20)), dim3(256), 0, stream, p, ins);
    return hipGetLastError();
}

hipError_t launch_ins_vote(const InsVote& v, uint32_t* scan_tmp, hipStream_t stream) {
    hipLaunchKernelGGL(ins_offsets_kernel, dim3(grid_for(v.glen + 1, 1u << 16)), dim3(256), 0, stream, v);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = scan_in_place(v.off, v.glen + 1, scan_tmp, stream);
    if (e == hipSuccess) e = scan_in_place(v.sidx, v.glen + 1, scan_tmp, stream);
    if (e != hipSuccess) return e;
    // the numbers of events and of sites are on the device: fixed grids that stride over them
    hipLaunchKernelGGL(ins_fill_kernel, dim3(grid_for(v.cap, 2048)), dim3(256), 0, stream, v);
    hipLaunchKernelGGL(ins_sites_kernel, dim3(grid_for(std::max<uint64_t>(v.glen, 1), 1u << 16)), dim3(256), 0, stream, v);
    hipLaunchKernelGGL(ins_vote_kernel, dim3(grid_for(v.sites_cap * 64, 4096)), dim3(256), 0, stream, v);
    return hipGetLastError();
}

}  // namespace msw
