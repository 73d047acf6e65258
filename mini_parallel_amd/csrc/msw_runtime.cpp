// msw_runtime.cpp -- device runtime and C ABI (include/msw.h) for the
// MI355X-native batched Smith-Waterman scorer.
//
// Replaces (smith_waterman/src/):
//   gpu.rs:33-132        OpenCL discovery + Mutex'd context singleton
//                        -> msw_device_count/info, one msw_ctx per device
//   aligner.rs:410-532   gpu_align: per-call JIT, buffer build, blocking finish
//                        -> msw_align_compat (kernels compiled ahead of time)
//   aligner.rs:269-289   per-chunk concat + gpu_align loop
//                        -> msw_align_batch: pinned double-buffered staging, H2D
//                           on a copy stream overlapped with the kernels
//   system_info.rs:236-243  80 % memory cap -> hipMemGetInfo
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <deque>
#include <functional>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/msw.h"
#include "msw_kernels.h"

namespace {

thread_local std::string g_last_error;

int fail(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

}  // namespace

namespace msw_detail {
int set_error(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}
}  // namespace msw_detail

namespace {

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail(MSW_E_DEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),   \
                        __FILE__, __LINE__);                                                   \
    } while (0)

inline uint32_t dup16(uint32_t v) { return (v & 0xFFFFu) | ((v & 0xFFFFu) << 16); }

// The library's run-time switches, read ONCE when a context is created
// (msw_ctx_create -> read_options) and kept in the context: no call or launch
// path reads the environment.  Every one forces a code path the tests cover
// (INTEGRATION.md section 4), or turns a diagnostic trace on.
struct Options {
    bool no_f16 = false;          // MSW_NO_F16: the integer path for every launch
    bool force_long = false;      // MSW_FORCE_LONG=1: every pair on the long-pair kernel
    uint64_t long_blocks = 0;     // MSW_LONG_BLOCKS: a fixed long-pair block count (work-queue grids)
    uint64_t trace_blocks = 0;    // MSW_TRACE_BLOCKS: a fixed traceback block count (work-queue grids)
    bool layout_set = false;      // MSW_LAYOUT given (per-bucket launches then)
    bool force_pairs = false, force_split = false, force_mixed = false;  // its value
    bool group_set = false;       // MSW_GROUP_LANES given
    uint32_t group_lanes = 0;     // its value (8..16)
    bool no_multi = false;        // MSW_NO_MULTI: one launch per bucket
    bool host_trace = false;      // MSW_HOST_TRACE: per-call host phase times on stderr
    std::string wave_trace;       // MSW_WAVE_TRACE=file: per-block placement records
    uint64_t chunk = 65536;       // GPU_CHUNK_SIZE_READS: default pairs per staged chunk (aligner.rs:9-15)
    uint64_t gz_group_bytes = 1024ull << 20;  // MSW_GZ_GROUP_MB: output bytes per msw_bgzf_inflate launch
    bool pileup_planes = false;   // MSW_PILEUP_PLANES=1: a pileup's device counts as eight planes, not rows of eight
};

Options read_options() {
    Options o;
    auto has = [](const char* k) { return getenv(k) != nullptr; };
    o.no_f16 = has("MSW_NO_F16");
    const char* fl = getenv("MSW_FORCE_LONG");
    o.force_long = fl && *fl == '1';
    const char* lb = getenv("MSW_LONG_BLOCKS");
    o.long_blocks = lb && atoll(lb) > 0 ? (uint64_t)atoll(lb) : 0;
    const char* tb = getenv("MSW_TRACE_BLOCKS");
    o.trace_blocks = tb && atoll(tb) > 0 ? (uint64_t)atoll(tb) : 0;
    const char* lay = getenv("MSW_LAYOUT");
    o.layout_set = lay != nullptr;
    o.force_pairs = lay && !strcmp(lay, "pairs");
    o.force_split = lay && !strcmp(lay, "split");
    o.force_mixed = lay && !strcmp(lay, "mixed");
    const char* g = getenv("MSW_GROUP_LANES");
    o.group_set = g != nullptr;
    o.group_lanes = g ? (uint32_t)atoi(g) : 0u;
    o.no_multi = has("MSW_NO_MULTI");
    o.host_trace = has("MSW_HOST_TRACE");
    const char* wt = getenv("MSW_WAVE_TRACE");
    o.wave_trace = wt ? wt : "";
    const char* v = getenv("GPU_CHUNK_SIZE_READS");
    if (v && *v) {
        char* end = nullptr;
        const unsigned long long n = strtoull(v, &end, 10);
        if (end && *end == '\0' && n > 0) o.chunk = n;
    }
    const char* gz = getenv("MSW_GZ_GROUP_MB");
    if (gz && atoll(gz) > 0) o.gz_group_bytes = (uint64_t)atoll(gz) << 20;
    const char* pp = getenv("MSW_PILEUP_PLANES");
    o.pileup_planes = pp && *pp == '1';
    return o;
}

const Options kDefaultOptions{};

// Validated kernel constants for one scoring scheme.
struct Scheme {
    const Options* opt = &kDefaultOptions;  // the context's switches
    bool affine, coords;
    uint32_t match2, delta2, gap2, open_ext2, bias2, code_shift;
    int32_t match;
    uint32_t bias;  // affine value bias K (0 for linear)
    // f16 fast path: match and mismatch are f16 values with a zero low byte
    // (the v_perm tables hold high bytes only); per-launch bound in f16_fits.
    bool f16_scheme;
    uint32_t f16_hi, f16_ngap2, f16_noe2;
};

int make_scheme(const msw_scoring_t* sc, const Options& opt, Scheme* s) {
    if (!sc) return fail(MSW_E_INVALID, "scoring is NULL");
    s->opt = &opt;
    if (sc->match < 1 || sc->match > 64)
        return fail(MSW_E_RANGE, "match=%d outside [1, 64]", sc->match);
    if (sc->mismatch > 0 || sc->match - sc->mismatch > 64)
        return fail(MSW_E_RANGE, "mismatch=%d outside [match-64, 0]", sc->mismatch);
    if (sc->gap_extend < 0 || sc->gap_open < 0)
        return fail(MSW_E_RANGE, "negative gap penalty (open=%d extend=%d)", sc->gap_open,
                    sc->gap_extend);
    if (sc->gap_extend > 1024 || sc->gap_open > 30000)
        return fail(MSW_E_RANGE, "gap penalty too large (gap_extend <= 1024, gap_open <= 30000)");
    s->affine = sc->affine != 0;
    s->coords = sc->want_coords != 0;
    s->match = sc->match;
    const uint32_t delta = (uint32_t)(sc->match - sc->mismatch);
    uint32_t shift = 0;
    while ((1u << shift) < delta) ++shift;
    s->code_shift = shift;
    s->match2 = dup16((uint32_t)sc->match);
    s->delta2 = dup16(delta);
    s->gap2 = dup16((uint32_t)sc->gap_extend);
    // Affine kernels keep H/E/F biased by K = 256 + gap_extend (msw_kernels.hip):
    // K > 0xFF, the largest substitution penalty (fast-path padding columns).
    s->bias = s->affine ? 256u + (uint32_t)sc->gap_extend : 0u;
    s->bias2 = dup16(s->bias);
    s->open_ext2 = dup16((uint32_t)(sc->gap_open + sc->gap_extend) + s->bias);
    // f16 domain (cells H * 2^-11, exact below 2048): gaps of 2048 or more
    // zero any cell, exactly as 2047 does, so they are capped there.
    const uint32_t mb = msw::f16_cell_bits(sc->match), xb = msw::f16_cell_bits(sc->mismatch);
    s->f16_scheme = (mb & 0xFFu) == 0 && (xb & 0xFFu) == 0;
    s->f16_hi = (mb >> 8) | ((xb >> 8) << 8);
    const int32_t ge = std::min(sc->gap_extend, 2047);
    const int32_t oe = std::min(sc->affine ? sc->gap_open + sc->gap_extend : sc->gap_extend, 2047);
    s->f16_ngap2 = dup16(msw::f16_cell_bits(-ge));
    s->f16_noe2 = dup16(msw::f16_cell_bits(-oe));
    return MSW_OK;
}

// The f16 path holds every cell value (<= match * min(m, n)) below 2048.
bool f16_fits(const Scheme& s, uint32_t max_m, uint32_t max_n) {
    if (s.opt->no_f16) return false;  // tests: force the integer path
    return s.f16_scheme && (uint64_t)s.match * (std::min(max_m, max_n) + 2u) < 2048u;
}

// Length limits: pairs up to kMaxReadLen x kMaxWinLen run on the packed
// 16-bit kernels (every cell value, <= match * (384 + 1) + bias <= 64 * 385 +
// 1280 = 25920 < 0x7C00, is a finite non-negative f16 bit pattern for
// v_pk_maximum3_f16; tests/test_gpu_ranges.py reaches it); longer reads
// or windows, up to kMaxLongLen (the i16 coordinates), on the i32 long-pair
// kernel (msw_long.hip).
int check_bounds(const Scheme& s, uint32_t max_m, uint32_t max_n) {
    (void)s;
    if (max_m > (uint32_t)msw::kMaxLongLen)
        return fail(MSW_E_RANGE, "read length %u > %d", max_m, msw::kMaxLongLen);
    if (max_n > (uint32_t)msw::kMaxLongLen)
        return fail(MSW_E_RANGE, "window length %u > %d", max_n, msw::kMaxLongLen);
    return MSW_OK;
}

// A pair (or a bound) beyond the packed kernels' limits.
inline bool is_long(uint32_t m, uint32_t n) {
    return m > (uint32_t)msw::kMaxReadLen || n > (uint32_t)msw::kMaxWinLen;
}
// MSW_FORCE_LONG=1 (Options::force_long) sends every pair to the long-pair
// kernel (tests and tools/long_bench.py run it on the packed kernels' shapes).

// Long-pair launch (p's pointers, order and output fields set by the caller):
// one wave per pair, one block per slot: the dispatcher fills every wave slot
// the kernel's registers and LDS allow and refills freed ones in slot order,
// so with the slots of spread lengths sorted heaviest first (`spread`,
// bucket_chunk) that is longest-job-first over the SIMDs (tools/long_bench.py
// mixed 257-2000: 2.4 -> 3.9 TCUPS).  Equal pairs whose last round would be a
// short tail (<= 1/8 of the resident waves, running almost alone) are spread
// evenly over the fewest rounds instead (150 x 5000: 3.0 -> 3.6 TCUPS; with
// larger tails keeping full occupancy measured faster).  Past a block cap
// (boundary-row scratch <= 1 GiB), finished blocks take the next slot from a
// work queue.  Scratch and queue counter are allocated stream-ordered on
// `st`, so calls on any stream stay independent.
int launch_long(const Scheme& sch, msw::SwParams p, uint64_t n, uint32_t max_m, uint32_t max_n, bool spread,
                int cu_count, hipStream_t st) {
    if (n == 0) return MSW_OK;
    p.n_slots = (uint32_t)n;
    const bool strips = max_m > 64u * (uint32_t)msw::long_rows_per_lane(max_m);
    const size_t per_block = strips ? (size_t)msw::long_scratch_cols(max_n) * (sch.affine ? 2u : 1u) * sizeof(int32_t) : 0;
    const uint64_t resident =
        (uint64_t)(cu_count > 0 ? cu_count : 256) * (uint64_t)msw::long_blocks_per_cu(sch.affine, sch.coords, max_m, max_n);
    uint64_t blocks = n;
    if (!spread && n > resident && n % resident != 0 && (n % resident) * 8 <= resident) {
        const uint64_t rounds = (n + resident - 1) / resident;
        blocks = (n + rounds - 1) / rounds;
    }
    blocks = std::min<uint64_t>(blocks, per_block ? std::max<uint64_t>(resident, (1ull << 30) / per_block) : 1ull << 20);
    if (sch.opt->long_blocks) blocks = std::min<uint64_t>(n, sch.opt->long_blocks);  // tests: a fixed block count
    const bool queue = n > blocks;
    const size_t scratch_bytes = (size_t)blocks * per_block;
    uint8_t* mem = nullptr;
    if (strips || queue) {
        HIP_TRY(hipMallocAsync((void**)&mem, scratch_bytes + 256, st));
        p.long_scratch = strips ? reinterpret_cast<int32_t*>(mem) : nullptr;
        p.long_cols = strips ? msw::long_scratch_cols(max_n) : 0u;
        if (queue) {
            p.long_next = reinterpret_cast<uint32_t*>(mem + scratch_bytes);
            HIP_TRY(hipMemsetAsync(p.long_next, 0, sizeof(uint32_t), st));
        }
    }
    const hipError_t e = msw::launch_sw_long(p, sch.affine, sch.coords, max_m, max_n, (uint32_t)blocks, st);
    if (mem) HIP_TRY(hipFreeAsync(mem, st));
    HIP_TRY(e);
    return MSW_OK;
}

msw::SwParams base_params(const Scheme& s) {
    msw::SwParams p;
    memset(&p, 0, sizeof(p));
    p.code_shift = s.code_shift;
    p.match2 = s.match2;
    p.delta2 = s.delta2;
    p.gap2 = s.gap2;
    p.open_ext2 = s.open_ext2;
    p.bias2 = s.bias2;
    p.f16_hi = s.f16_hi;
    p.f16_ngap2 = s.f16_ngap2;
    p.f16_noe2 = s.f16_noe2;
    return p;
}

// Device + pinned buffers for one in-flight chunk.  The per-pair metadata of a
// chunk (window positions, read and window lengths, slot order) is one block,
// [pos i64 | rlen u16 | wlen u16 | order u32] x n, uploaded by ONE copy of the
// part the chunk uses (pairs mode skips the positions, a chunk in input order
// the order); the results [score i32 | end_i i16 | end_j i16] come back by one
// copy, or are written by the kernels straight into the pinned block (a
// one-chunk call: no copy and no event between the kernel and the host).
struct Slot {
    size_t cap_pairs = 0, cap_read = 0, cap_win = 0;
    uint8_t *d_reads = nullptr, *d_wins = nullptr, *d_meta = nullptr, *d_res = nullptr;
    uint8_t *h_reads = nullptr, *h_wins = nullptr, *h_meta = nullptr, *h_res = nullptr;
    // device addresses of the pinned staging blocks (one-chunk calls pull from them)
    const uint8_t *g_reads = nullptr, *g_wins = nullptr, *g_meta = nullptr;
    // views into d_meta / h_meta and d_res / h_res
    int64_t *d_pos = nullptr, *h_pos = nullptr;
    uint32_t *d_order = nullptr, *h_order = nullptr;
    uint16_t *d_rlen = nullptr, *d_wlen = nullptr, *h_rlen = nullptr, *h_wlen = nullptr;
    int32_t *d_score = nullptr, *h_score = nullptr;
    int16_t *d_ei = nullptr, *d_ej = nullptr, *h_ei = nullptr, *h_ej = nullptr;
    // where this chunk's kernels store results: the device block or the host one
    int32_t* k_score = nullptr;
    int16_t *k_ei = nullptr, *k_ej = nullptr;
    hipEvent_t uploaded = nullptr, computed = nullptr, done = nullptr;
    // timing events around the chunk's scoring launches; a chunk whose kernels
    // write the host block directly ends on k_end (done is not recorded)
    hipEvent_t k_start = nullptr, k_end = nullptr;
    bool busy = false;
    bool by_slot = false;  // results in slot order: the drain scatters them through h_order
    bool direct_out = false;  // the kernels wrote h_res themselves; k_end marks completion
    uint64_t ticket = 0;  // msw_align_*_async call that owns the chunk in flight
    uint64_t seq = 0;     // submission order of the chunk (drains go in this order)
    // Pending readback bookkeeping.
    uint64_t first = 0, count = 0;
    msw_out_t out{};
};

constexpr size_t kMetaBytesPerPair = 8 + 2 + 2 + 4;
constexpr size_t kResBytesPerPair = 4 + 2 + 2;

// Views of the metadata / result blocks for a chunk of n pairs (each array
// packed at n entries, so one copy moves exactly the chunk's bytes).
void set_views(Slot& s, uint64_t n) {
    auto views = [n](uint8_t* meta, uint8_t* res, int64_t*& pos, uint32_t*& order, uint16_t*& rlen, uint16_t*& wlen,
                     int32_t*& score, int16_t*& ei, int16_t*& ej) {
        pos = reinterpret_cast<int64_t*>(meta);
        rlen = reinterpret_cast<uint16_t*>(meta + 8 * n);
        wlen = reinterpret_cast<uint16_t*>(meta + 10 * n);
        order = reinterpret_cast<uint32_t*>(meta + 12 * n);
        score = reinterpret_cast<int32_t*>(res);
        ei = reinterpret_cast<int16_t*>(res + 4 * n);
        ej = reinterpret_cast<int16_t*>(res + 6 * n);
    };
    views(s.d_meta, s.d_res, s.d_pos, s.d_order, s.d_rlen, s.d_wlen, s.d_score, s.d_ei, s.d_ej);
    views(s.h_meta, s.h_res, s.h_pos, s.h_order, s.h_rlen, s.h_wlen, s.h_score, s.h_ei, s.h_ej);
}

void free_slot(Slot& s) {
    for (void* p : {(void*)s.d_reads, (void*)s.d_wins, (void*)s.d_meta, (void*)s.d_res})
        if (p) (void)hipFree(p);
    for (void* p : {(void*)s.h_reads, (void*)s.h_wins, (void*)s.h_meta, (void*)s.h_res})
        if (p) (void)hipHostFree(p);
    s = Slot{};
}

}  // namespace

struct msw_ctx {
    int device = 0;
    int cu_count = 256;
    Options opt;  // the environment's switches, read at creation
    // compute: created with the context; the others too, unless the context
    // is lean (MSW_CTX_LEAN: made by the first call that uses them,
    // aux_streams): a stream costs 3-30 ms to create (the first few each make
    // a hardware queue) and as much to destroy, and the --full-wgs GPU-reader
    // workers never use them (profiles/r06/c3f/)
    hipStream_t compute = nullptr, copy = nullptr, d2h = nullptr;
    // multi-chunk calls alternate their chunks' kernels over compute and
    // compute2, so chunk k+1's waves start under chunk k's tail (one stream
    // would idle the CUs the tail leaves)
    hipStream_t compute2 = nullptr;
    hipStream_t side = nullptr;  // long-pair launches beside packed ones (fork_side)
    // Staging slots, used round robin by successive chunks (and calls): with
    // three, the host stages chunk k+1 while k runs and k-1 drains, so the
    // uploads of k+1 finish under kernel k.
    static constexpr int kSlots = 3;
    Slot slots[kSlots];
    uint64_t next_ticket = 1, done_ticket = 0;
    uint64_t slot_seq = 0;  // chunks submitted (slot = slot_seq % kSlots)
    msw_stats_t stats{};    // msw_ctx_stats: host-batch calls since creation / the last reset
    // Origin of the kernel-time interval union (recorded at creation, moved
    // forward every ~second of GPU time so float ms offsets stay fine-grained:
    // epoch_next is recorded, and once it has completed becomes the epoch)
    hipEvent_t epoch = nullptr, epoch_next = nullptr;
    double busy_until = 0.0;     // ms after epoch at which the counted scoring intervals end
    // pinned_cached: the most recently used (address, bytes) ranges asked
    // about, most recent first (move to front on a hit).  16: a --full-wgs
    // worker's two result sets x five copies per batch, plus a call's reads /
    // windows, stay cached (the 8-entry FIFO missed every one).
    struct PinnedRange {
        const void* p = nullptr;
        size_t bytes = 0;
        bool pinned = false;
        const uint8_t* dev = nullptr;  // its device address (pinned ranges)
    };
    static constexpr unsigned kPinnedRanges = 16;
    PinnedRange pinned_ranges[kPinnedRanges];
    unsigned pinned_used = 0;
    uint64_t pinned_epoch = 0;           // g_host_free_epoch when the cache was last valid
    uint64_t pinned_hits = 0, pinned_misses = 0;  // MSW_HOST_TRACE
    // compat buffers
    uint8_t *c_s1 = nullptr, *c_s2 = nullptr;
    int32_t* c_res = nullptr;
    size_t c_cap = 0;
    hipEvent_t c_k0 = nullptr, c_k1 = nullptr;  // timing of the compat launch (msw_ctx_stats)
    // msw_align_reads_device scratch: the cut windows and their clipped lengths
    // msw_align_reads_device's window slab and lengths, one set per stream
    // it is called on (calls on two streams run concurrently)
    struct ReadsScratch {
        hipStream_t st = nullptr;
        uint8_t* wins = nullptr;
        uint16_t* wlen = nullptr;
        size_t wins_cap = 0, wlen_cap = 0;
        // both strands: the reverse pass's results [score i32 | end_i i16 | end_j i16]
        uint8_t* rev = nullptr;
        size_t rev_cap = 0;
    };
    std::vector<ReadsScratch> rscratch;
    // streams made by msw_stream_create (synchronised by msw_synchronize,
    // destroyed with the context if the caller has not)
    std::vector<hipStream_t> user_streams;
    // timing events of msw_align_reads_device launches not yet harvested
    struct DevTiming {
        hipEvent_t k0, k1;
        uint64_t pairs;
    };
    std::deque<DevTiming> dev_timings;
    std::vector<hipEvent_t> free_events;
    // free_events and fences: msw_fence_wait may run on several threads at
    // once (--full-wgs settles its last two batches on two)
    std::mutex ev_mu;
    // the plan of the last single-bucket launch of a host chunk or of a
    // planned call (issue_schedule; MSW_HOST_TRACE prints it)
    msw::Layout last_layout = msw::Layout::kPairs;
    uint32_t last_group_lanes = 0, last_kr = 0;
    std::unordered_map<uint64_t, hipEvent_t> fences;  // msw_fence_record, not yet waited on
    uint64_t next_fence = 1;
};

struct msw_genome {
    const msw_ctx* ctx = nullptr;  // identity only
    int device = 0;
    uint8_t* d_seq = nullptr;      // len + kGenomePad bytes (cut kernel over-reads <= 20)
    uint64_t len = 0;
};

struct msw_index {
    const msw_ctx* ctx = nullptr;  // identity only
    int device = 0;
    uint32_t k = 0, max_occ = 0;
    uint64_t buckets = 0, n_pos = 0, n_masked = 0;
    uint32_t* d_off = nullptr;     // [buckets + 1]
    uint32_t* d_pos = nullptr;     // [max(n_pos, 1)]
    double build_ms[5] = {0, 0, 0, 0, 0};
};

// Internal accessors for the other units of the library (msw_gfastq.cpp).
namespace msw_detail {
int ctx_device(const msw_ctx* c) { return c->device; }
hipStream_t ctx_compute_stream(const msw_ctx* c) { return c->compute; }
uint64_t ctx_gz_group_bytes(const msw_ctx* c) { return c->opt.gz_group_bytes; }
}  // namespace msw_detail

namespace {

int set_device(msw_ctx* ctx) {
    int cur = -1;
    if (hipGetDevice(&cur) == hipSuccess && cur == ctx->device) return MSW_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    return MSW_OK;
}

// The stream of a device-API call: the caller's, or the context's compute stream.
inline hipStream_t call_stream(const msw_ctx* ctx, void* stream) {
    return stream ? (hipStream_t)stream : ctx->compute;
}

// The streams a context creates on first use (compute is made with it).
int aux_streams(msw_ctx* ctx) {
    for (hipStream_t* st : {&ctx->compute2, &ctx->copy, &ctx->d2h, &ctx->side})
        if (!*st) HIP_TRY(hipStreamCreateWithFlags(st, hipStreamNonBlocking));
    return MSW_OK;
}

hipEvent_t take_event(msw_ctx* ctx) {
    {
        std::lock_guard<std::mutex> lk(ctx->ev_mu);
        if (!ctx->free_events.empty()) {
            hipEvent_t e = ctx->free_events.back();
            ctx->free_events.pop_back();
            return e;
        }
    }
    hipEvent_t e = nullptr;
    return hipEventCreate(&e) == hipSuccess ? e : nullptr;
}

// A finished scoring interval [k0, k1] into ctx->stats.kernel_ms as part of
// the union of all of them: chunks alternate over two compute streams and
// overlap, so each interval adds only its part after everything counted so
// far ends.  Durations come from elapsed(k0, k1) (exact), the overlap from
// offsets against the context's epoch event.  Intervals arrive in
// submission order, i.e. in start order but for a chunk that starts before
// its predecessor, which is then undercounted, never counted twice.
// Callers hand intervals over oldest chunk first (drain_through), so each
// starts no earlier than the previous one save for the two compute streams'
// overlap, which is exactly what the union removes.
void add_kernel_interval(msw_ctx* ctx, hipEvent_t k0, hipEvent_t k1) {
    float dur = 0.f, start = 0.f;
    if (hipEventElapsedTime(&dur, k0, k1) != hipSuccess) {
        (void)hipGetLastError();
        return;
    }
    if (!ctx->epoch || hipEventElapsedTime(&start, ctx->epoch, k0) != hipSuccess) {
        (void)hipGetLastError();
        ctx->stats.kernel_ms += dur;
        return;
    }
    const double covered = std::min<double>(dur, std::max(0.0, ctx->busy_until - start));
    ctx->stats.kernel_ms += dur - covered;
    ctx->busy_until = std::max<double>(ctx->busy_until, (double)start + dur);
    // Re-base: a float offset of T ms resolves T / 2^24 -- 0.25 ms after an
    // hour -- so the epoch moves up once it is a second behind.  The new one
    // is an event on the compute stream; it takes over once it has completed
    // and its distance from the old one is known (both offsets then move by
    // it; an interval starting before it gets a negative offset, which the
    // union handles the same way).
    if (ctx->epoch_next) {
        float delta = 0.f;
        if (hipEventQuery(ctx->epoch_next) == hipSuccess &&
            hipEventElapsedTime(&delta, ctx->epoch, ctx->epoch_next) == hipSuccess) {
            ctx->busy_until -= delta;
            std::swap(ctx->epoch, ctx->epoch_next);
            (void)hipEventDestroy(ctx->epoch_next);
            ctx->epoch_next = nullptr;
        }
        (void)hipGetLastError();
    } else if (start > 1000.f) {
        if (hipEventCreate(&ctx->epoch_next) != hipSuccess || hipEventRecord(ctx->epoch_next, ctx->compute) != hipSuccess) {
            if (ctx->epoch_next) (void)hipEventDestroy(ctx->epoch_next);
            ctx->epoch_next = nullptr;
            (void)hipGetLastError();
        }
    }
}

// Kernel time of finished msw_align_reads_device launches into ctx->stats
// (wait = true: all of them, after synchronising).
void harvest_dev_timings(msw_ctx* ctx, bool wait) {
    while (!ctx->dev_timings.empty()) {
        msw_ctx::DevTiming& t = ctx->dev_timings.front();
        if (wait) (void)hipEventSynchronize(t.k1);
        else if (hipEventQuery(t.k1) != hipSuccess) break;
        add_kernel_interval(ctx, t.k0, t.k1);
        ctx->stats.launches += 1;
        ctx->stats.pairs += t.pairs;
        {
            std::lock_guard<std::mutex> lk(ctx->ev_mu);
            ctx->free_events.push_back(t.k0);
            ctx->free_events.push_back(t.k1);
        }
        ctx->dev_timings.pop_front();
    }
}

template <typename T>
int grow_dev(T** p, size_t n) {
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    if (n == 0) return MSW_OK;
    hipError_t e = hipMalloc((void**)p, n * sizeof(T));
    if (e != hipSuccess) return fail(MSW_E_NOMEM, "hipMalloc(%zu B): %s", n * sizeof(T), hipGetErrorString(e));
    return MSW_OK;
}
template <typename T>
int grow_host(T** p, size_t n, unsigned flags = hipHostMallocDefault) {
    if (*p) (void)hipHostFree(*p);
    *p = nullptr;
    if (n == 0) return MSW_OK;
    hipError_t e = hipHostMalloc((void**)p, n * sizeof(T), flags);
    if (e != hipSuccess) return fail(MSW_E_NOMEM, "hipHostMalloc(%zu B): %s", n * sizeof(T), hipGetErrorString(e));
    return MSW_OK;
}

// The device address of a pinned host block (the pull copy reads it there).
int dev_addr(const uint8_t* h, const uint8_t** out) {
    void* d = nullptr;
    HIP_TRY(hipHostGetDevicePointer(&d, (void*)h, 0));
    *out = (const uint8_t*)d;
    return MSW_OK;
}

int ensure_slot(Slot& s, size_t pairs, size_t read_bytes, size_t win_bytes) {
    int rc;
    if (!s.uploaded) {
        HIP_TRY(hipEventCreateWithFlags(&s.uploaded, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&s.computed, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
        HIP_TRY(hipEventCreate(&s.k_start));
        HIP_TRY(hipEventCreate(&s.k_end));
    }
    if (pairs > s.cap_pairs) {
        // the result block is mapped and coherent: one-chunk calls have the
        // kernels store into it directly (its device address is the host one)
        if ((rc = grow_dev(&s.d_meta, pairs * kMetaBytesPerPair)) ||
            (rc = grow_host(&s.h_meta, pairs * kMetaBytesPerPair)) ||
            (rc = grow_dev(&s.d_res, pairs * kResBytesPerPair)) ||
            (rc = grow_host(&s.h_res, pairs * kResBytesPerPair, hipHostMallocMapped | hipHostMallocCoherent)) ||
            (rc = dev_addr(s.h_meta, &s.g_meta)))
            return rc;
        s.cap_pairs = pairs;
    }
    if (read_bytes > s.cap_read) {
        if ((rc = grow_dev(&s.d_reads, read_bytes)) || (rc = grow_host(&s.h_reads, read_bytes)) ||
            (rc = dev_addr(s.h_reads, &s.g_reads)))
            return rc;
        s.cap_read = read_bytes;
    }
    if (win_bytes > s.cap_win) {
        if ((rc = grow_dev(&s.d_wins, win_bytes)) || (rc = grow_host(&s.h_wins, win_bytes)) ||
            (rc = dev_addr(s.h_wins, &s.g_wins)))
            return rc;
        s.cap_win = win_bytes;
    }
    return MSW_OK;
}

// Lane-group layout of one launch.  "pairs" scores 2 pairs per G-lane group,
// "split" 1 pair per group (rows split over the two halves; half the work per
// wave), "mixed" (G = 16) runs up to one pairs-wave per SIMD and the rest as
// split-waves.  G (8..16 lanes per group, 64 / G groups per wave) sets how many
// pairs one wave holds, so a small batch can be cut into about one wave per
// SIMD.  The choice minimises a makespan model:
//  - a wave issues steps x (a * KR + b) instructions (a, b fitted to the
//    compiled loops: tools/issue_sim.py);
//  - waves are dealt round-robin over the 4 x CU SIMDs in block order (what
//    tools/wave_trace.py observes), and a SIMD holding k waves issues one
//    instruction per r(k) cycles (measured: 5.27 alone, 4.6 for two, 3.94 at
//    eight -- a lone wave cannot issue back to back).
// MSW_LAYOUT=pairs|split|mixed and MSW_GROUP_LANES=8..16 override (tests use
// them to cover every path).
struct LaunchPlan {
    msw::Layout layout;
    uint32_t pairs_blocks;
    uint32_t group_lanes;
    uint32_t groups;
};

static double simd_cycles_per_instr(uint64_t k) {
    static const double r[] = {0.0, 5.27, 4.6, 4.3, 4.15, 4.05, 4.0, 3.97, 3.94};
    return r[k > 8 ? 8 : k];
}

LaunchPlan choose_layout(uint64_t n_pairs, uint32_t max_m, uint32_t max_n, const Scheme& sch, int cu_count) {
    const uint64_t simds = 4ull * (uint64_t)(cu_count > 0 ? cu_count : 256);
    // VALU instructions per packed row of the compiled loops:
    // f16 path 4.8 (+4.1 affine, +2.6 coordinates); integer path 5.5 (+5.2, +2.8).
    const bool f16 = f16_fits(sch, max_m, max_n);
    const double per_row = f16 ? 4.8 + (sch.affine ? 4.1 : 0.0) + (sch.coords ? 2.6 : 0.0)
                               : 5.5 + (sch.affine ? 5.2 : 0.0) + (sch.coords ? 2.8 : 0.0);
    auto wave_instr = [&](bool split, uint32_t G) {
        const int kr = msw::rows_per_lane(max_m, split, G);
        const double steps = (double)max_n + (split ? 2.0 * G : (double)G);
        const double over = (split ? 5.5 : 3.0) + (sch.affine ? 2.0 : 0.0);
        return steps * (per_row * kr + over) + 300.0;
    };
    // Round-robin dealing: SIMD i holds waves i, i + S, ...; time = its
    // instructions x r(its wave count).
    auto makespan = [&](uint64_t w1, double c1, uint64_t w2, double c2) {
        const uint64_t w = w1 + w2;
        if (w == 0) return 0.0;
        if (w2 == 0 || w1 == 0) {
            const double c = w1 ? c1 : c2;
            const uint64_t k = (w + simds - 1) / simds;
            return (double)k * c * simd_cycles_per_instr(k);
        }
        // SIMD i holds w1 / S + (i < w1 % S) first-kind waves of w / S + (i <
        // w % S): constant between the two breakpoints, so three SIMDs cover
        // every case (closed form: a loop over the waves cost ~1 ms of host
        // time per 2M-pair launch, stalling the GPU between kernels)
        const uint64_t b1 = w1 % simds, b = w % simds;
        double t = 0.0;
        for (uint64_t i : {(uint64_t)0, std::min(b1, b), std::max(b1, b)}) {
            if (i >= simds) continue;
            const uint64_t n1 = w1 / simds + (i < b1 ? 1 : 0), n = w / simds + (i < b ? 1 : 0);
            if (n == 0) continue;
            t = std::max(t, ((double)n1 * c1 + (double)(n - n1) * c2) * simd_cycles_per_instr(n));
        }
        return t;
    };
    const uint32_t stride = msw::stream_stride(max_n);
    const uint32_t force_g = sch.opt->group_lanes;
    const bool force_pairs = sch.opt->force_pairs, force_split = sch.opt->force_split;
    const bool force_mixed = sch.opt->force_mixed;

    LaunchPlan best{msw::Layout::kPairs, 0, 16, 4};
    double best_t = 1e300;
    for (int split = 0; split <= 1; ++split) {
        if ((force_pairs && split) || (force_split && !split) || force_mixed) continue;
        for (uint32_t G = 16; G >= 8; --G) {
            if (force_g ? G != force_g : ((force_pairs || force_split) && G != 16)) continue;
            const int kr = msw::rows_per_lane(max_m, split, G);
            if (kr > (split ? 8 : msw::kMaxRowsPerLane)) continue;
            const uint32_t groups = 64 / G;
            if (G != 16 && msw::lds_bytes(stride, groups) > 65536) continue;
            const uint64_t per = msw::pairs_per_wave(split, groups);
            // 17..19 rows in narrower groups (150 bp reads: G = 8 / KR = 19 or
            // G = 9 / KR = 17) fit only 2-3 waves per SIMD (VGPRs; the LDS of 7-8
            // window streams), and the makespan model does not predict where
            // they start to win (an occupancy-rounds model puts
            // them ahead at every size).  So the gate is the measured crossover
            // per instance family (tools/group_lanes_probe.py, alternating A/B
            // against G = 16, profiles/r05/ab/group_9v16.jsonl and
            // profiles/r04/ab/group_lanes_probe_sizes.jsonl):
            //  KR 17 (G = 9): 2-3 % slower at 9 waves per SIMD (131k pairs),
            //    2.4-3.5 % faster at 18, 3.5-5 % at 37, 5-6 % at 55: >= 16;
            //  KR 18..19 (G = 8): 4 % faster to 13 % slower at 16 waves per
            //    SIMD (262k), 5-6 % faster at 64 (1M): >= 48.
            // Larger rows-per-lane counts were never measured: not taken.
            const uint64_t min_waves = kr <= 17 ? 16 : 48;
            if (!split && G != 16 && kr > 16 && !force_g &&
                (kr > 19 || (n_pairs + per - 1) / per < min_waves * simds))
                continue;
            const double t = makespan((n_pairs + per - 1) / per, wave_instr(split, G), 0, 0.0);
            if (t < best_t * 0.995) {
                best_t = t;
                best = {split ? msw::Layout::kSplit : msw::Layout::kPairs, 0, G, groups};
            }
        }
    }
    // Mixed grid (G = 16, even KR): up to one pairs-wave per SIMD, then split waves.
    const int krp = msw::rows_per_lane(max_m, false);
    const bool mixed_ok = (krp % 2) == 0 && krp <= 16 && (!force_g || force_g == 16) && !force_pairs && !force_split;
    if (mixed_ok) {
        const double cp = wave_instr(false, 16), cs = wave_instr(true, 16);
        for (uint64_t k = 1; k <= 4; ++k) {
            const uint64_t pw = std::min<uint64_t>(n_pairs / 8, k * simds / 4);
            if (pw == 0) continue;
            const uint64_t rest = n_pairs - pw * 8;
            const double t = makespan(pw, cp, (rest + 3) / 4, cs);
            if (t < best_t * 0.995 || (force_mixed && best.layout != msw::Layout::kMixed)) {
                best_t = t;
                best = {msw::Layout::kMixed, (uint32_t)pw, 16, 4};
            }
        }
        if (force_mixed && best.layout != msw::Layout::kMixed)
            best = {msw::Layout::kMixed, (uint32_t)std::min<uint64_t>(n_pairs / 8, simds), 16, 4};
    } else if (force_mixed) {
        best = {msw::Layout::kSplit, 0, 16, 4};
    }
    return best;
}

// Whether one launch of n pairs under these bounds can read its windows from
// the resident genome: the GEN instances exist for the pairs layout with up
// to 16 rows per lane (the shapes of short-read chunks), not for long pairs.
bool genome_windows_ok(uint64_t n, uint32_t max_m, uint32_t max_n, const Scheme& sch, int cu_count) {
    if (is_long(max_m, max_n)) return false;
    const LaunchPlan plan = choose_layout(n, max_m, max_n, sch, cu_count);
    return plan.layout == msw::Layout::kPairs && msw::rows_per_lane(max_m, false, plan.group_lanes) <= 16;
}

// Buckets of one chunk: pairs grouped by rows-per-lane (read length / 16), and
// inside a bucket by window length, so every wave runs with tight bounds.
struct Bucket {
    uint32_t begin, count, max_m, max_n;
    bool long_pairs = false;  // beyond the packed kernels: sw_long_kernel
    bool spread = false;      // long pairs of spread lengths, sorted heaviest first
};

// lengths: the chunk's {min read, max read, min window, max window}.
// all_long: Options::force_long.
void bucket_chunk(const uint16_t* rlen, const uint16_t* wlen, uint64_t n, uint32_t* order,
                  std::vector<Bucket>& buckets, uint32_t lengths[4], bool all_long) {
    buckets.clear();
    // key = KR (1..24) * 257 + ceil(n / 16) (<= 256): counting sort; pairs
    // beyond the packed kernels' limits share the last key.
    constexpr int kLongKey = (msw::kMaxRowsPerLane + 1) * 257, kKeys = kLongKey + 1;
    auto key_of = [&](uint64_t i) {
        if (all_long || is_long(rlen[i], wlen[i])) return kLongKey;
        const int kr = msw::rows_per_lane(rlen[i], false);
        const int nb = (wlen[i] + 15) / 16;
        return kr * 257 + nb;
    };
    // One key (fixed-length reads and windows, the common case): one bucket in
    // input order, no sort -- unless they are long pairs of spread lengths,
    // which the work queue wants heaviest first.
    int kmin = kKeys, kmax = -1;
    uint32_t gm = 0, gn = 0, lm = 0xFFFF, ln = 0xFFFF;
    for (uint64_t i = 0; i < n; ++i) {
        const int k = key_of(i);
        kmin = std::min(kmin, k);
        kmax = std::max(kmax, k);
        gm = std::max<uint32_t>(gm, rlen[i]);
        gn = std::max<uint32_t>(gn, wlen[i]);
        lm = std::min<uint32_t>(lm, rlen[i]);
        ln = std::min<uint32_t>(ln, wlen[i]);
    }
    lengths[0] = lm, lengths[1] = gm, lengths[2] = ln, lengths[3] = gn;
    const bool spread_long = kmin == kLongKey && (gm - lm >= 64 || gn - ln >= 64);
    if (n && kmin == kmax && !spread_long) {
        for (uint64_t i = 0; i < n; ++i) order[i] = (uint32_t)i;
        buckets.push_back({0, (uint32_t)n, gm, gn, kmin == kLongKey});
        return;
    }
    std::vector<uint32_t> hist(kKeys + 1, 0);
    for (uint64_t i = 0; i < n; ++i) hist[key_of(i) + 1]++;
    for (int k = 0; k < kKeys; ++k) hist[k + 1] += hist[k];
    std::vector<uint32_t> pos(hist.begin(), hist.end() - 1);
    for (uint64_t i = 0; i < n; ++i) order[pos[key_of(i)]++] = (uint32_t)i;
    // max read / max window over the slots [b, e)
    auto bounds = [&](uint32_t b, uint32_t e, uint32_t& mm, uint32_t& mn) {
        mm = mn = 0;
        for (uint32_t s = b; s < e; ++s) {
            mm = std::max<uint32_t>(mm, rlen[order[s]]);
            mn = std::max<uint32_t>(mn, wlen[order[s]]);
        }
    };
    // One bucket per KR value; the window bound is the bucket's max.
    for (int kr = 1; kr <= msw::kMaxRowsPerLane; ++kr) {
        const uint32_t b = hist[kr * 257], e = hist[kr * 257 + 257];
        if (e <= b) continue;
        uint32_t mm, mn;
        bounds(b, e, mm, mn);
        buckets.push_back({b, e - b, mm, mn});
    }
    if (hist[kLongKey + 1] > hist[kLongKey]) {  // the long pairs: last in slot order
        const uint32_t b = hist[kLongKey], e = hist[kLongKey + 1];
        uint32_t mm, mn;
        bounds(b, e, mm, mn);
        // heaviest first (strips x steps at the launch's rows per lane): the
        // kernel's work queue then schedules longest-job-first
        const uint32_t strip_rows = 64u * (uint32_t)msw::long_rows_per_lane(mm);
        auto cost = [&](uint32_t i) {
            return (uint64_t)((rlen[i] + strip_rows - 1) / strip_rows) * (uint64_t)(wlen[i] + 63u);
        };
        std::stable_sort(order + b, order + e, [&](uint32_t x, uint32_t y) { return cost(x) > cost(y); });
        buckets.push_back({b, e - b, mm, mn, true, cost(order[b]) != cost(order[e - 1])});
    }
}

// The packed-kernel buckets of a list (all but a trailing long bucket).
size_t short_buckets(const std::vector<Bucket>& buckets) {
    return !buckets.empty() && buckets.back().long_pairs ? buckets.size() - 1 : buckets.size();
}

// The leading buckets sw_multi_kernel takes (KR <= 16; buckets come in KR
// order); the rest of the packed buckets (KR 17..24) launch on their own.
size_t multi_buckets(const std::vector<Bucket>& buckets) {
    const size_t n = short_buckets(buckets);
    size_t k = 0;
    while (k < n && msw::rows_per_lane(buckets[k].max_m, false) <= msw::kMaxMultiKR) ++k;
    return k;
}

// One-launch table of a bucket list (msw::MultiTable): heaviest waves first
// (rows per lane x window steps), so the tail of the grid is short waves.
// [lo, hi): the KR <= 16 buckets (sw_multi_kernel) or the KR 17..24 ones (its
// wide instance).
void fill_multi(const std::vector<Bucket>& buckets, size_t lo, size_t hi, const Scheme& sch, msw::MultiTable& t) {
    std::vector<Bucket> bs(buckets.begin() + lo, buckets.begin() + hi);
    auto cost = [](const Bucket& b) { return (uint64_t)msw::rows_per_lane(b.max_m, false) * (b.max_n + 16u); };
    std::stable_sort(bs.begin(), bs.end(), [&](const Bucket& a, const Bucket& b) { return cost(a) > cost(b); });
    memset(&t, 0, sizeof(t));
    uint32_t blocks = 0;
    for (const Bucket& b : bs) {
        const uint32_t i = t.n_buckets++;
        blocks += (b.count + msw::kPairsPerWave - 1) / msw::kPairsPerWave;
        t.block_end[i] = blocks;
        t.slot_begin[i] = b.begin;
        t.count[i] = b.count;
        t.kr[i] = (uint32_t)msw::rows_per_lane(b.max_m, false);
        t.lds_stride[i] = msw::stream_stride(b.max_n);
        t.f16_ok[i] = f16_fits(sch, b.max_m, b.max_n) ? 1u : 0u;
    }
}

// Several buckets run as one sw_multi_kernel launch, unless MSW_NO_MULTI is
// set or a layout / group width is forced (MSW_LAYOUT, MSW_GROUP_LANES): then
// each bucket gets its own launch with that layout (tests cover both).
bool use_multi(size_t n_buckets, const Options& o) {
    return n_buckets > 1 && !o.no_multi && !o.layout_set && !o.group_set;
}

// A long-pair launch next to packed launches runs on the context's side
// stream, forked from `st` and joined back after the packed launches: the
// long kernel's tail and the packed buckets' short launches (a few lone waves
// each for KR 17..24) share the CUs instead of queueing behind each other.
struct SideFork {
    hipEvent_t ev = nullptr;
    SideFork() = default;
    SideFork(const SideFork&) = delete;
    SideFork& operator=(const SideFork&) = delete;
    ~SideFork() {
        if (ev) (void)hipEventDestroy(ev);
    }
};

int fork_side(msw_ctx* ctx, hipStream_t st, SideFork& f) {
    if (!ctx->side) {
        const int rc = aux_streams(ctx);
        if (rc) return rc;
    }
    HIP_TRY(hipEventCreateWithFlags(&f.ev, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(f.ev, st));
    HIP_TRY(hipStreamWaitEvent(ctx->side, f.ev, 0));
    return MSW_OK;
}

int join_side(msw_ctx* ctx, hipStream_t st, SideFork& f) {
    HIP_TRY(hipEventRecord(f.ev, ctx->side));
    HIP_TRY(hipStreamWaitEvent(st, f.ev, 0));
    return MSW_OK;
}

// What a bucket list launches: the long bucket on the long-pair kernel, the
// KR <= 16 buckets as one sw_multi_kernel launch, the KR 17..24 buckets as one
// launch of its wide instance, every other packed bucket on its own.  Made by
// schedule_buckets (per host chunk; once per plan), issued by issue_schedule.
struct BucketSchedule {
    bool has_long = false;
    Bucket longs{};  // pairs beyond the packed kernels (sw_long_kernel): the last slots
    bool multi = false, wide = false;
    msw::MultiTable table{};       // multi: the KR <= 16 buckets
    msw::MultiTable wide_table{};  // wide: the KR 17..24 buckets
    // packed-kernel buckets launched on their own (all of them without a
    // multi table, else the KR 17..24 ones), each with its layout
    std::vector<std::pair<Bucket, LaunchPlan>> singles;
    bool packed() const { return multi || wide || !singles.empty(); }
};

// ordered: the batch is launched through an order array (slot -> pair), which
// the multi launches need.  A host chunk in input order has none: it is one
// bucket with a launch of its own.
BucketSchedule schedule_buckets(const std::vector<Bucket>& buckets, const Scheme& sch, int cu_count, bool ordered) {
    BucketSchedule s;
    const size_t n_short = short_buckets(buckets), n_multi = multi_buckets(buckets);
    if (n_short < buckets.size()) {
        s.has_long = true;
        s.longs = buckets.back();
    }
    s.multi = ordered && use_multi(n_multi, *sch.opt);
    if (s.multi) fill_multi(buckets, 0, n_multi, sch, s.table);
    // The KR 17..24 buckets as one launch of the wide instance when there are
    // several: one launch per bucket left each bucket's few waves running
    // alone and measured slower (8.5 vs 12.7 TCUPS linear).
    s.wide = ordered && use_multi(n_short - n_multi, *sch.opt);
    if (s.wide) fill_multi(buckets, n_multi, n_short, sch, s.wide_table);
    for (size_t bi = s.multi ? n_multi : 0; bi < (s.wide ? n_multi : n_short); ++bi) {
        const Bucket& b = buckets[bi];
        s.singles.push_back({b, choose_layout(b.count, b.max_m, b.max_n, sch, cu_count)});
    }
    return s;
}

// p narrowed to the slots [b.begin, b.begin + b.count) of its order array
// (without one, slot k is pair k: the pairs from b.begin on) and of its
// slot-ordered results.
msw::SwParams bucket_slots(msw::SwParams p, const Bucket& b) {
    if (p.order) p.order += b.begin;
    else p.slot_base = b.begin;
    p.out_slot_base = b.begin;
    p.n_slots = b.count;
    return p;
}

// One packed bucket's launch parameters under its plan (p: the batch's
// pointers, strides / window source, order and output fields).
msw::SwParams bucket_params(const msw::SwParams& p, const Scheme& sch, const Bucket& b, const LaunchPlan& plan) {
    msw::SwParams q = bucket_slots(p, b);
    q.lds_stride = msw::stream_stride(b.max_n);
    q.f16_ok = f16_fits(sch, b.max_m, b.max_n) ? 1u : 0u;
    q.pairs_blocks = plan.pairs_blocks;
    q.group_lanes = plan.group_lanes;
    q.groups = plan.groups;
    return q;
}

// One packed bucket on its own launch.
int launch_bucket(const msw::SwParams& p, const Scheme& sch, const Bucket& b, const LaunchPlan& plan, hipStream_t st) {
    HIP_TRY(msw::launch_sw(bucket_params(p, sch, b, plan), sch.affine, sch.coords, b.max_m, plan.layout, st));
    return MSW_OK;
}

// The launches of a schedule on `st`, in this order: the long launch (on the
// side stream if and only if packed launches follow), the multi launch, the
// wide multi launch, the single buckets in bucket order, the join back from
// the side stream.  `base` carries what the caller knows -- data pointers and
// strides, window source, outputs, the order array (or null: input order),
// out_by_slot, slot_lens; the per-launch fields are derived here.
int issue_schedule(msw_ctx* ctx, const Scheme& sch, const msw::SwParams& base, const BucketSchedule& s,
                   hipStream_t st) {
    int rc;
    SideFork side;
    if (s.has_long) {  // the long pairs: their own launch, beside any packed ones
        const Bucket& b = s.longs;
        msw::SwParams p = bucket_slots(base, b);
        p.slot_lens = nullptr;  // the long kernel reads lengths per pair, never by slot
        // only the order array puts slots of spread lengths heaviest first
        const bool spread = base.order && b.spread;
        if (s.packed() && (rc = fork_side(ctx, st, side))) return rc;
        if ((rc = launch_long(sch, p, b.count, b.max_m, b.max_n, spread, ctx->cu_count, s.packed() ? ctx->side : st)))
            return rc;
    }
    msw::SwParams m = base;  // the multi launches: slots and slot results from 0, buckets from the table
    m.out_slot_base = 0;
    m.group_lanes = 16;
    m.groups = 4;
    if (s.multi) HIP_TRY(msw::launch_sw_multi(m, s.table, sch.affine, sch.coords, st));
    if (s.wide) HIP_TRY(msw::launch_sw_multi(m, s.wide_table, sch.affine, sch.coords, st));
    for (const auto& sb : s.singles) {
        const Bucket& b = sb.first;
        const LaunchPlan& plan = sb.second;
        ctx->last_layout = plan.layout;
        ctx->last_group_lanes = plan.group_lanes;
        ctx->last_kr = (uint32_t)msw::rows_per_lane(b.max_m, plan.layout == msw::Layout::kSplit, plan.group_lanes);
        if ((rc = launch_bucket(base, sch, b, plan, st))) return rc;
    }
    if (side.ev) return join_side(ctx, st, side);
    return MSW_OK;
}

// Base parameters of a staged chunk's launches.  Its windows come from the
// slot's cut slab (win_stride), or, with a genome, straight from the resident
// genome at the slot's positions (the packed kernels only; long pairs need
// the slab).
msw::SwParams slot_params(const Scheme& sch, const Slot& s, uint32_t read_stride, uint32_t win_stride,
                          const msw_genome* g) {
    msw::SwParams p = base_params(sch);
    p.reads = s.d_reads;
    p.read_len = s.d_rlen;
    p.win_len = s.d_wlen;
    p.score = s.k_score;
    p.end_i = sch.coords ? s.k_ei : nullptr;
    p.end_j = sch.coords ? s.k_ej : nullptr;
    p.read_stride = read_stride;
    p.read_vec = msw::read_vec_ok(p.reads, p.read_stride);
    if (g) {
        p.win_src = g->d_seq;
        p.win_pos = s.d_pos;
        p.win_vec = 1;
    } else {
        p.wins = s.d_wins;
        p.win_stride = win_stride;
        p.win_vec = msw::vec_ok(p.wins, p.win_stride);
    }
    return p;
}

// Base parameters of a device-memory batch (the device API and plans).
msw::SwParams batch_params(const Scheme& sch, const msw_batch_t& b, const msw_out_t& out) {
    msw::SwParams p = base_params(sch);
    p.reads = b.reads;
    p.wins = b.wins;
    p.read_len = b.read_len;
    p.win_len = b.win_len;
    p.score = out.score;
    p.end_i = sch.coords ? out.end_i : nullptr;
    p.end_j = sch.coords ? out.end_j : nullptr;
    p.read_stride = b.read_stride;
    p.win_stride = b.win_stride;
    p.win_vec = msw::vec_ok(p.wins, p.win_stride);
    p.read_vec = msw::read_vec_ok(p.reads, p.read_stride);
    return p;
}

// The scoring launches of one staged chunk.  ordered: the chunk runs through
// the slot's order array and leaves its results in slot order (the drain
// scatters them); a chunk in input order needs neither.  g: the chunk's one
// packed bucket reads its windows from the resident genome.
int launch_buckets(msw_ctx* ctx, const Scheme& sch, const Slot& s, const std::vector<Bucket>& buckets, bool ordered,
                   uint32_t read_stride, uint32_t win_stride, hipStream_t cs, const msw_genome* g = nullptr) {
    if (g && short_buckets(buckets) < buckets.size())
        return fail(MSW_E_INVALID, "internal: long pairs need the window slab");
    if (g && (ordered || buckets.size() != 1)) return fail(MSW_E_INVALID, "internal: genome windows need one bucket");
    msw::SwParams p = slot_params(sch, s, read_stride, win_stride, g);
    p.order = ordered ? s.d_order : nullptr;
    p.out_by_slot = ordered ? 1u : 0u;
    return issue_schedule(ctx, sch, p, schedule_buckets(buckets, sch, ctx->cu_count, ordered), cs);
}

// Copy finished results of a slot into the caller's arrays; the chunk's
// kernel time goes into the context's counters.
int drain_slot(msw_ctx* ctx, Slot& s) {
    if (!s.busy) return MSW_OK;
    s.busy = false;
    HIP_TRY(hipEventSynchronize(s.direct_out ? s.k_end : s.done));
    add_kernel_interval(ctx, s.k_start, s.k_end);
    if (s.by_slot) {  // length-bucketed chunk: slot k holds pair h_order[k]
        int32_t* sc = s.out.score + s.first;
        for (uint64_t k = 0; k < s.count; ++k) sc[s.h_order[k]] = s.h_score[k];
        if (s.out.end_i) {
            int16_t *ei = s.out.end_i + s.first, *ej = s.out.end_j + s.first;
            for (uint64_t k = 0; k < s.count; ++k) {
                ei[s.h_order[k]] = s.h_ei[k];
                ej[s.h_order[k]] = s.h_ej[k];
            }
        }
        return MSW_OK;
    }
    memcpy(s.out.score + s.first, s.h_score, s.count * sizeof(int32_t));
    if (s.out.end_i) memcpy(s.out.end_i + s.first, s.h_ei, s.count * sizeof(int16_t));
    if (s.out.end_j) memcpy(s.out.end_j + s.first, s.h_ej, s.count * sizeof(int16_t));
    return MSW_OK;
}

// Drain the busy slots whose ticket is <= `ticket` (all: UINT64_MAX) oldest
// chunk first, so the kernel-time union sees its intervals in start order.
int drain_through(msw_ctx* ctx, uint64_t ticket) {
    for (;;) {
        Slot* next = nullptr;
        for (Slot& s : ctx->slots)
            if (s.busy && s.ticket <= ticket && (!next || s.seq < next->seq)) next = &s;
        if (!next) return MSW_OK;
        const int rc = drain_slot(ctx, *next);
        if (rc) return rc;
    }
}

int validate_batch(const msw_batch_t* b, const msw_out_t* out, const Scheme& sch) {
    if (!b || !out) return fail(MSW_E_INVALID, "batch/out is NULL");
    if (b->n_pairs == 0) return MSW_OK;
    if (!b->reads || !b->wins || !b->read_len || !b->win_len || !out->score)
        return fail(MSW_E_INVALID, "NULL array in batch/out");
    if (sch.coords && (!out->end_i || !out->end_j))
        return fail(MSW_E_INVALID, "want_coords set but end_i/end_j is NULL");
    if (b->n_pairs > 0xFFFFFFFFull) return fail(MSW_E_RANGE, "n_pairs > 2^32-1");
    return MSW_OK;
}

// The length bounds a device-memory call states must fit the batch's rows.
int check_strides(const msw_batch_t& b, uint32_t max_m, uint32_t max_n) {
    if (max_m > b.read_stride || max_n > b.win_stride) return fail(MSW_E_INVALID, "max length exceeds stride");
    return MSW_OK;
}

// Host-memory batch of either form: pairs (reads + windows) or reads against
// a genome-resident window source (wins == nullptr, genome + win_pos set).
struct HostBatch {
    const uint8_t* reads = nullptr;
    const uint16_t* read_len = nullptr;
    uint32_t read_stride = 0;
    const uint8_t* wins = nullptr;
    const uint16_t* win_len = nullptr;
    uint32_t win_stride = 0;
    const msw_genome* genome = nullptr;
    const int64_t* win_pos = nullptr;
    uint64_t n = 0;
};

// True when [p, p + bytes) lies in page-locked host memory (hipHostMalloc /
// hipHostRegister): such arrays are DMA'd directly, without staging.
// dev: the device address of p when pinned.
bool is_pinned(const void* p, size_t bytes, const uint8_t** dev) {
    *dev = nullptr;
    if (!p || !bytes) return false;
    for (const void* q : {p, (const void*)((const uint8_t*)p + bytes - 1)}) {
        hipPointerAttribute_t a;
        memset(&a, 0, sizeof(a));
        if (hipPointerGetAttributes(&a, q) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        if (a.type != hipMemoryTypeHost) return false;
        if (q == p) *dev = (const uint8_t*)a.devicePointer;
    }
    return true;
}

inline uint32_t round16(uint32_t v) { return (v + 15u) & ~15u; }

// Window length actually scored in genome mode: clipped at the genome end,
// empty for positions outside it.
inline uint16_t genome_window(int64_t pos, uint16_t want, uint64_t glen) {
    const uint64_t p = (uint64_t)pos;  // negative positions wrap past glen
    const uint64_t room = p < glen ? glen - p : 0;
    return (uint16_t)std::min<uint64_t>(want, room);
}

// Copy `n` rows of `len` bytes from stride `src_stride` to `dst_stride`.
void repack_rows(uint8_t* dst, uint32_t dst_stride, const uint8_t* src, uint32_t src_stride, uint64_t n) {
    if (dst_stride == src_stride) {
        memcpy(dst, src, n * src_stride);
        return;
    }
    for (uint64_t i = 0; i < n; ++i) memcpy(dst + i * dst_stride, src + i * src_stride, dst_stride);
}

// MSW_HOST_TRACE=1 (Options::host_trace): per-call host phase times on
// stderr (tools / DESIGN.md 5).
struct HostTrace {
    bool on;
    explicit HostTrace(bool enabled) : on(enabled) {}
    double scan = 0, stage = 0, submit = 0, wait = 0;
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    double lap() {
        const auto n = std::chrono::steady_clock::now();
        const double d = std::chrono::duration<double, std::micro>(n - t).count();
        t = n;
        return d;
    }
};

// Host loops compiled twice, AVX2 and baseline x86-64, picked at load time
// (the attribute means nothing to the gfx950 pass of this file).
#if defined(__HIP_DEVICE_COMPILE__)
#define MSW_HOST_SIMD
#else
#define MSW_HOST_SIMD __attribute__((target_clones("avx2", "default")))
#endif

// One pass over a chunk's per-pair arrays: the read lengths, the window
// lengths (genome mode: clipped at the genome end) and the positions into the
// slot's metadata block, and what the dispatch needs -- the length bounds and
// the cells and bytes.  Plain loops over the arrays (the compiler vectorises
// them; AVX2 where the host has it): ~10k pairs per microsecond.
struct ChunkScan {
    uint32_t lm = 0xFFFF, gm = 0, ln = 0xFFFF, gn = 0;
    uint64_t cells = 0, bytes = 0;
};

MSW_HOST_SIMD
void scan_lengths(const uint16_t* __restrict rl, const uint16_t* __restrict wl, uint64_t n, ChunkScan& c) {
    uint32_t lm = 0xFFFF, gm = 0, ln = 0xFFFF, gn = 0;
    uint64_t cells = 0, bytes = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t r = rl[i], w = wl[i];
        lm = std::min(lm, r);
        gm = std::max(gm, r);
        ln = std::min(ln, w);
        gn = std::max(gn, w);
        cells += r * w;
        bytes += r + w;
    }
    c.lm = lm, c.gm = gm, c.ln = ln, c.gn = gn, c.cells = cells, c.bytes = bytes;
}

MSW_HOST_SIMD
void clip_windows(const int64_t* __restrict pos, const uint16_t* __restrict want, uint64_t n, uint64_t glen,
                  uint16_t* __restrict out) {
    for (uint64_t i = 0; i < n; ++i) out[i] = genome_window(pos[i], want[i], glen);
}

MSW_HOST_SIMD
void max_u16(const uint16_t* __restrict a, uint64_t n, uint32_t& m) {
    uint32_t v = 0;
    for (uint64_t i = 0; i < n; ++i) v = std::max<uint32_t>(v, a[i]);
    m = v;
}

ChunkScan stage_meta(Slot& s, const HostBatch& b, uint64_t first, uint64_t cnt) {
    memcpy(s.h_rlen, b.read_len + first, cnt * sizeof(uint16_t));
    if (b.genome) {
        memcpy(s.h_pos, b.win_pos + first, cnt * sizeof(int64_t));
        clip_windows(b.win_pos + first, b.win_len + first, cnt, b.genome->len, s.h_wlen);
    } else {
        memcpy(s.h_wlen, b.win_len + first, cnt * sizeof(uint16_t));
    }
    ChunkScan c;
    scan_lengths(s.h_rlen, s.h_wlen, cnt, c);
    return c;
}

// True when every pair of the chunk has one bucket key (bucket_chunk's: rows
// per lane of its read, 16-column blocks of its window, not long) -- decided
// from the bounds alone, both keys being monotone in the lengths.
bool single_key(const ChunkScan& c, bool all_long) {
    return !all_long && !is_long(c.gm, c.gn) &&
           msw::rows_per_lane(c.lm, false) == msw::rows_per_lane(c.gm, false) &&
           (c.ln + 15) / 16 == (c.gn + 15) / 16;
}

// Pinned-ness of the caller's arrays, remembered for the most recently used
// ranges (hipPointerGetAttributes twice per array and call is a visible share
// of a small call).  msw_host_free bumps g_host_free_epoch, which empties
// every context's cache at its next lookup, so a freed msw_host_alloc block
// whose address comes back as pageable memory is never taken for pinned
// (ADVICE r05).  Memory the caller pins or unpins itself must stay as it was
// while a call uses it, as for any DMA API; a stale verdict then only changes
// how a copy is made, never what it copies (hipMemcpyAsync accepts pageable
// and pinned sources alike, and the d2h copy kernel needs a device pointer
// for the block, which an unpinned one no longer has).
std::atomic<uint64_t> g_host_free_epoch{0};

bool pinned_cached(msw_ctx* ctx, const void* p, size_t bytes, const uint8_t** dev = nullptr) {
    const uint64_t ep = g_host_free_epoch.load(std::memory_order_acquire);
    if (ep != ctx->pinned_epoch) {
        ctx->pinned_used = 0;
        ctx->pinned_epoch = ep;
    }
    msw_ctx::PinnedRange* r = ctx->pinned_ranges;
    for (unsigned k = 0; k < ctx->pinned_used; ++k)
        if (r[k].p == p && r[k].bytes == bytes && p) {
            const msw_ctx::PinnedRange hit = r[k];
            for (unsigned q = k; q > 0; --q) r[q] = r[q - 1];  // move to front
            r[0] = hit;
            ++ctx->pinned_hits;
            if (dev) *dev = hit.dev;
            return hit.pinned;
        }
    ++ctx->pinned_misses;
    const uint8_t* d = nullptr;
    const bool pinned = is_pinned(p, bytes, &d);
    const unsigned n = std::min(ctx->pinned_used + 1, msw_ctx::kPinnedRanges);  // the least recent falls off
    for (unsigned q = n - 1; q > 0; --q) r[q] = r[q - 1];
    r[0] = {p, bytes, pinned, d};
    ctx->pinned_used = n;
    if (dev) *dev = d;
    return pinned;
}


int run_batch_impl(msw_ctx* ctx, const msw_scoring_t* sc, const HostBatch& b, msw_out_t* out,
                   uint64_t chunk_pairs, bool sync) {
    Scheme sch;
    int rc;
    if ((rc = make_scheme(sc, ctx->opt, &sch))) return rc;
    if (!out) return fail(MSW_E_INVALID, "out is NULL");
    const bool gmode = b.genome != nullptr;
    const uint64_t n = b.n;
    if (n == 0) return MSW_OK;
    if (!b.reads || !b.read_len || !b.win_len || !out->score || (gmode ? !b.win_pos : !b.wins))
        return fail(MSW_E_INVALID, "NULL array in batch/out");
    if (sch.coords && (!out->end_i || !out->end_j))
        return fail(MSW_E_INVALID, "want_coords set but end_i/end_j is NULL");
    if (n > 0xFFFFFFFFull) return fail(MSW_E_RANGE, "n_pairs > 2^32-1");
    if (gmode && (b.genome->ctx != ctx)) return fail(MSW_E_INVALID, "genome belongs to another context");
    if ((rc = set_device(ctx))) return rc;
    HostTrace tr(ctx->opt.host_trace);
    // Host-side range checks over the whole batch first: fail before any launch.
    // (genome mode bounds the requested window lengths: a clipped window is
    // never longer, and the positions need not be read here)
    uint32_t gm = 0, gn = 0;
    max_u16(b.read_len, n, gm);
    max_u16(b.win_len, n, gn);
    if (gm > b.read_stride || (!gmode && gn > b.win_stride))
        return fail(MSW_E_INVALID, "length exceeds stride (max read %u / stride %u, max window %u / stride %u)",
                    gm, b.read_stride, gn, b.win_stride);
    if ((rc = check_bounds(sch, gm, gn))) return rc;

    // Direct DMA from pinned caller arrays; otherwise stage through the slot's
    // pinned buffers with rows repacked to 16-byte-rounded strides.
    const uint8_t *g_reads = nullptr, *g_wins = nullptr;  // their device addresses
    const bool d_reads = pinned_cached(ctx, b.reads, n * b.read_stride, &g_reads);
    const bool d_wins = !gmode && pinned_cached(ctx, b.wins, n * b.win_stride, &g_wins);
    const uint32_t rs = d_reads ? b.read_stride : std::min(b.read_stride, std::max(16u, round16(gm)));
    const uint32_t ws = gmode ? std::max(16u, round16(gn))
                              : (d_wins ? b.win_stride : std::min(b.win_stride, std::max(16u, round16(gn))));
    if (tr.on) tr.scan += tr.lap();

    const uint64_t chunk = chunk_pairs ? chunk_pairs : ctx->opt.chunk;
    // A multi-chunk call pipelines its own chunks: copies on the copy stream,
    // kernels alternating between the two compute streams, results back on
    // the d2h stream.  A one-chunk call keeps its kernels and results on one
    // compute stream (async calls alternate it, so consecutive calls
    // overlap; a synchronous call uploads there too) and its kernels store
    // the results straight into the slot's mapped host block (no copy, no
    // event after the kernels but the timing one).
    const bool multi_chunk = n > chunk;
    const bool alternate = multi_chunk || !sync;
    const bool direct_out = !multi_chunk;
    // the copy / second compute / d2h streams: created by the first call that uses them
    if (alternate && !ctx->copy && (rc = aux_streams(ctx))) return rc;
    // Genome mode: a chunk of one bucket that the model puts in the pairs
    // layout with <= 16 rows per lane reads its windows straight from the
    // resident genome (GEN kernel instances: no cut launch, one dependent
    // step fewer per chunk); other chunks (several buckets, long pairs, other
    // layouts) cut a window slab first.
    const bool all_long = ctx->opt.force_long;
    const bool genome_ok = gmode && !all_long;
    uint64_t fused_chunks = 0;
    std::vector<Bucket> buckets;
    uint64_t c = 0;
    // A short first chunk starts the GPU early; with chunks of more than 64k
    // pairs the chunks after it double up to `chunk`, so each chunk's upload
    // hides under the kernel of the one before (a large chunk straight after
    // a small one left the GPU idle while it uploaded) and the large ones
    // still reach the narrow lane groups.  1M config-3 pairs
    // from pinned memory, genome form (tools/h2h_sweep.py,
    // profiles/r05/h2h/chunk_ramp.jsonl): 131k / 262k / 524k chunks 8.29 /
    // 8.49 / 9.41-9.49 ms -> 7.99 / 7.97-8.02 / 8.26-8.56; at 32k the ramp's
    // extra chunk cost 1 % (7.92 -> 8.01), so smaller chunks keep the old
    // schedule.
    const bool ramp = chunk > 65536;
    uint64_t next_chunk = n > chunk ? std::max<uint64_t>(std::min<uint64_t>(chunk, 8192), chunk / 8) : chunk;
    for (uint64_t first = 0, cnt = 0; first < n; first += cnt, ++c) {
        const uint64_t this_chunk = next_chunk;
        next_chunk = ramp ? std::min<uint64_t>(chunk, 2 * next_chunk) : chunk;
        cnt = std::min(this_chunk, n - first);
        // Slots alternate across calls too, so consecutive async calls overlap.
        const uint64_t seq = ctx->slot_seq++;
        Slot& s = ctx->slots[seq % msw_ctx::kSlots];
        hipStream_t cs = (alternate && (seq & 1)) ? ctx->compute2 : ctx->compute;
        if (tr.on) tr.submit += tr.lap();
        if ((rc = drain_slot(ctx, s))) return rc;  // the slot's previous chunk must be out before reuse
        if (tr.on) tr.wait += tr.lap();
        if ((rc = ensure_slot(s, cnt, (size_t)cnt * rs, (size_t)cnt * ws))) return rc;
        set_views(s, cnt);
        // Bulk rows: DMA'd from the caller's memory when pinned, else staged.
        const uint8_t* src_reads = b.reads + first * b.read_stride;
        if (!d_reads) {
            repack_rows(s.h_reads, rs, src_reads, b.read_stride, cnt);
            src_reads = s.h_reads;
        }
        const uint8_t* src_wins = nullptr;
        if (!gmode) {
            src_wins = b.wins + first * b.win_stride;
            if (!d_wins) {
                repack_rows(s.h_wins, ws, src_wins, b.win_stride, cnt);
                src_wins = s.h_wins;
            }
        }
        // Metadata block: lengths (effective window lengths in genome mode),
        // positions; the slot order only for a chunk of several buckets.
        const ChunkScan cs_ = stage_meta(s, b, first, cnt);
        bool uniform;
        if (single_key(cs_, all_long)) {  // fixed-length reads and windows, the common case: no sort
            buckets.assign(1, Bucket{0, (uint32_t)cnt, cs_.gm, cs_.gn});
            uniform = true;
        } else {
            uint32_t lens[4];
            bucket_chunk(s.h_rlen, s.h_wlen, cnt, s.h_order, buckets, lens, all_long);
            // One read-length bucket: order only matters if windows vary a lot;
            // long pairs of spread read lengths keep their heaviest-first order.
            uniform = buckets.size() == 1 && lens[3] - lens[2] < 16 &&
                      (!buckets[0].long_pairs || lens[1] - lens[0] < 64);
        }
        const bool fused = genome_ok && uniform && genome_windows_ok(cnt, cs_.gm, cs_.gn, sch, ctx->cu_count);
        fused_chunks += fused ? 1 : 0;
        if (tr.on) tr.stage += tr.lap();
        // [pos | rlen | wlen | order]: the contiguous part this chunk uses
        const size_t meta_lo = gmode ? 0 : 8 * cnt, meta_hi = (uniform ? 12 : 16) * cnt;
        // A one-chunk call pulls its rows and metadata from pinned host
        // memory into the slot with one copy kernel on its compute stream,
        // ahead of its scoring launch: no DMA engine and no event between
        // them.  (The DMA form -- uploads on the copy stream, the kernel
        // behind an event -- ran the 10k-pair stream at 57 us per batch:
        // reads and metadata copies 33.6 + 8.0 us back to back on the DMA
        // engine and ~22 us from an upload's end to its kernel's start,
        // kernels never overlapping; profiles/r06/host/stream_trace/.)
        // Sources must share the slot buffers' alignment mod 16.
        const uint8_t* g_src_reads = d_reads ? g_reads + first * b.read_stride : s.g_reads;
        const uint8_t* g_src_wins = gmode ? nullptr : (d_wins ? g_wins + first * b.win_stride : s.g_wins);
        const bool pull = !multi_chunk && g_src_reads && (gmode || g_src_wins) &&
                          (((uintptr_t)g_src_reads ^ (uintptr_t)s.d_reads) & 15u) == 0 &&
                          (gmode || (((uintptr_t)g_src_wins ^ (uintptr_t)s.d_wins) & 15u) == 0);
        if (pull) {
            msw::PullRanges pr{};
            pr.dst[0] = s.d_reads;
            pr.src[0] = g_src_reads;
            pr.bytes[0] = cnt * rs;
            if (!gmode) {
                pr.dst[1] = s.d_wins;
                pr.src[1] = g_src_wins;
                pr.bytes[1] = cnt * ws;
            }
            pr.dst[2] = s.d_meta + meta_lo;
            pr.src[2] = s.g_meta + meta_lo;
            pr.bytes[2] = meta_hi - meta_lo;
            // (The copy on the copy stream running ahead, the kernels on one
            // compute stream behind an event: 58.3 vs 55.1 us per batch,
            // profiles/r06/host/pull_ahead_ab.jsonl.)
            HIP_TRY(msw::launch_pull_copy(pr, cs));
            if (gmode && !fused)
                HIP_TRY(msw::launch_cut_windows(b.genome->d_seq, b.genome->len, s.d_pos, s.d_wlen, s.d_wins, nullptr,
                                                ws, cnt, cs));
        } else {
            // Multi-chunk calls: H2D on the copy stream, kernels on the
            // compute streams (an event orders each kernel after its chunk's
            // upload), results back on the d2h stream -- chunk k+1's uploads
            // and chunk k-1's readback overlap chunk k's kernel.  (One-chunk
            // calls whose sources are misaligned: DMA'd on the call's own
            // stream.)
            hipStream_t up = multi_chunk ? ctx->copy : cs;
            HIP_TRY(hipMemcpyAsync(s.d_reads, src_reads, cnt * rs, hipMemcpyHostToDevice, up));
            if (!gmode) HIP_TRY(hipMemcpyAsync(s.d_wins, src_wins, cnt * ws, hipMemcpyHostToDevice, up));
            HIP_TRY(hipMemcpyAsync(s.d_meta + meta_lo, s.h_meta + meta_lo, meta_hi - meta_lo, hipMemcpyHostToDevice,
                                   up));
            if (gmode && !fused)
                HIP_TRY(msw::launch_cut_windows(b.genome->d_seq, b.genome->len, s.d_pos, s.d_wlen, s.d_wins, nullptr,
                                                ws, cnt, up));
            if (multi_chunk) {
                HIP_TRY(hipEventRecord(s.uploaded, ctx->copy));
                HIP_TRY(hipStreamWaitEvent(cs, s.uploaded, 0));
            }
        }
        if (uniform) {
            buckets.resize(1);
            buckets[0].begin = 0;
        }
        s.k_score = direct_out ? s.h_score : s.d_score;
        s.k_ei = direct_out ? s.h_ei : s.d_ei;
        s.k_ej = direct_out ? s.h_ej : s.d_ej;
        HIP_TRY(hipEventRecord(s.k_start, cs));
        if ((rc = launch_buckets(ctx, sch, s, buckets, !uniform, rs, ws, cs, fused ? b.genome : nullptr)))
            return rc;
        HIP_TRY(hipEventRecord(s.k_end, cs));
        ctx->stats.launches += 1;
        ctx->stats.pairs += cnt;
        ctx->stats.cells += cs_.cells;
        ctx->stats.alg_bytes += cs_.bytes + cnt * (sch.coords ? 8u : 4u);
        if (!direct_out) {
            hipStream_t down = cs;
            if (multi_chunk) {
                HIP_TRY(hipEventRecord(s.computed, cs));
                HIP_TRY(hipStreamWaitEvent(ctx->d2h, s.computed, 0));
                down = ctx->d2h;
            }
            HIP_TRY(hipMemcpyAsync(s.h_res, s.d_res, (sch.coords ? kResBytesPerPair : 4) * cnt,
                                   hipMemcpyDeviceToHost, down));
            HIP_TRY(hipEventRecord(s.done, down));
        }
        s.busy = true;
        s.direct_out = direct_out;
        s.by_slot = !uniform;
        s.ticket = ctx->next_ticket;  // the ticket an async call returns
        s.seq = seq;
        s.first = first;
        s.count = cnt;
        s.out = *out;
        if (!sch.coords) { s.out.end_i = nullptr; s.out.end_j = nullptr; }
    }
    if (tr.on) tr.submit += tr.lap();  // the last chunk's HIP calls
    if (sync) {
        if ((rc = drain_through(ctx, UINT64_MAX))) return rc;
        if (tr.on) tr.wait += tr.lap();
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return fail(MSW_E_DEVICE, "kernel failure: %s", hipGetErrorString(e));
    }
    if (tr.on)
        fprintf(stderr,
                "[msw host] pairs=%llu chunks=%llu direct(reads=%d wins=%d out=%d) genome_chunks=%llu rs=%u ws=%u "
                "last_launch(layout=%s G=%u KR=%u) scan=%.1fus stage=%.1fus submit=%.1fus wait=%.1fus "
                "pinned_cache(hits=%llu misses=%llu)\n",
                (unsigned long long)n, (unsigned long long)c, (int)d_reads, (int)d_wins, (int)direct_out,
                (unsigned long long)fused_chunks, rs, ws,
                ctx->last_layout == msw::Layout::kSplit ? "split" : (ctx->last_layout == msw::Layout::kMixed ? "mixed" : "pairs"),
                ctx->last_group_lanes, ctx->last_kr,
                tr.scan, tr.stage, tr.submit, tr.wait, (unsigned long long)ctx->pinned_hits,
                (unsigned long long)ctx->pinned_misses);
    return MSW_OK;
}


// A call that fails after submitting some of its chunks must not leave them
// behind: they point at the caller's output arrays, and a later msw_wait or
// slot reuse would drain them there (the caller may have freed them by then).
// The streams are synchronised, the call's chunks dropped, and its ticket
// number consumed so no later call shares it.
int run_batch(msw_ctx* ctx, const msw_scoring_t* sc, const HostBatch& b, msw_out_t* out, uint64_t chunk_pairs,
              bool sync) {
    if (!ctx) return fail(MSW_E_INVALID, "ctx is NULL");
    const uint64_t ticket = ctx->next_ticket;
    const int rc = run_batch_impl(ctx, sc, b, out, chunk_pairs, sync);
    if (rc == MSW_OK) return rc;
    bool dropped = false;
    for (Slot& s : ctx->slots) dropped = dropped || (s.busy && s.ticket == ticket);
    if (dropped) {
        const std::string msg = g_last_error;
        for (hipStream_t st : {ctx->copy, ctx->compute, ctx->compute2, ctx->d2h, ctx->side})
            if (st) (void)hipStreamSynchronize(st);
        for (Slot& s : ctx->slots)
            if (s.busy && s.ticket == ticket) s.busy = false;
        ctx->next_ticket++;
        g_last_error = msg;
    }
    return rc;
}

HostBatch pairs_batch(const msw_batch_t& b) {
    HostBatch h;
    h.reads = b.reads;
    h.read_len = b.read_len;
    h.read_stride = b.read_stride;
    h.wins = b.wins;
    h.win_len = b.win_len;
    h.win_stride = b.win_stride;
    h.n = b.n_pairs;
    return h;
}

HostBatch reads_batch(const msw_read_batch_t& b, const msw_genome* g) {
    HostBatch h;
    h.reads = b.reads;
    h.read_len = b.read_len;
    h.read_stride = b.read_stride;
    h.win_len = b.win_len;
    h.genome = g;
    h.win_pos = b.win_pos;
    h.n = b.n_pairs;
    return h;
}

}  // namespace

extern "C" {

const char* msw_last_error(void) { return g_last_error.c_str(); }

const char* msw_version(void) { return "msw 0.1.0 (gfx950, HIP)"; }

int msw_device_count(int* n) {
    if (!n) return fail(MSW_E_INVALID, "n is NULL");
    *n = 0;
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess || c == 0) return fail(MSW_E_NODEVICE, "no GPU: %s", hipGetErrorString(e));
    *n = c;
    return MSW_OK;
}

int msw_device_info(int ordinal, msw_device_info_t* out) {
    if (!out) return fail(MSW_E_INVALID, "out is NULL");
    int n = 0;
    int rc = msw_device_count(&n);
    if (rc) return rc;
    if (ordinal < 0 || ordinal >= n) return fail(MSW_E_INVALID, "device %d out of range [0,%d)", ordinal, n);
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, ordinal));
    memset(out, 0, sizeof(*out));
    snprintf(out->name, sizeof(out->name), "%s", prop.name);
    if (!out->name[0])  // the marketing name can be empty under ROCm: name the target instead
        snprintf(out->name, sizeof(out->name), "AMD Instinct GPU (%s, %d CUs)", prop.gcnArchName,
                 prop.multiProcessorCount);
    snprintf(out->arch, sizeof(out->arch), "%s", prop.gcnArchName);
    out->mem_bytes = prop.totalGlobalMem;
    out->max_wg = (uint32_t)prop.maxThreadsPerBlock;
    out->cu_count = (uint32_t)prop.multiProcessorCount;
    int cur = 0;
    (void)hipGetDevice(&cur);
    if (hipSetDevice(ordinal) == hipSuccess) {
        size_t fr = 0, tot = 0;
        if (hipMemGetInfo(&fr, &tot) == hipSuccess) out->mem_free_bytes = fr;
        (void)hipSetDevice(cur);
    }
    return MSW_OK;
}

int msw_ctx_create(int ordinal, msw_ctx** out) { return msw_ctx_create_ex(ordinal, 0u, out); }

int msw_ctx_create_ex(int ordinal, unsigned flags, msw_ctx** out) {
    if (!out) return fail(MSW_E_INVALID, "out is NULL");
    if (flags & ~MSW_CTX_LEAN) return fail(MSW_E_INVALID, "unknown context flags 0x%x", flags);
    *out = nullptr;
    int n = 0;
    int rc = msw_device_count(&n);
    if (rc) return rc;
    if (ordinal < 0 || ordinal >= n) return fail(MSW_E_INVALID, "device %d out of range [0,%d)", ordinal, n);
    msw_ctx* c = new msw_ctx();
    c->device = ordinal;
    c->opt = read_options();
    hipError_t e = hipSetDevice(ordinal);
    hipDeviceProp_t prop;
    if (e == hipSuccess && hipGetDeviceProperties(&prop, ordinal) == hipSuccess && prop.multiProcessorCount > 0)
        c->cu_count = prop.multiProcessorCount;
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->compute, hipStreamNonBlocking);
    if (e == hipSuccess && !(flags & MSW_CTX_LEAN) && aux_streams(c) != MSW_OK) e = hipErrorOutOfMemory;
    if (e == hipSuccess) e = hipEventCreate(&c->epoch);
    if (e == hipSuccess) e = hipEventRecord(c->epoch, c->compute);
    if (e != hipSuccess) {
        delete c;
        return fail(MSW_E_DEVICE, "context creation on device %d failed: %s", ordinal, hipGetErrorString(e));
    }
    *out = c;
    return MSW_OK;
}

void msw_ctx_destroy(msw_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->compute) (void)hipStreamSynchronize(ctx->compute);
    if (ctx->compute2) (void)hipStreamSynchronize(ctx->compute2);
    if (ctx->copy) (void)hipStreamSynchronize(ctx->copy);
    if (ctx->d2h) (void)hipStreamSynchronize(ctx->d2h);
    if (ctx->side) (void)hipStreamSynchronize(ctx->side);
    for (Slot& s : ctx->slots) {
        if (s.uploaded) (void)hipEventDestroy(s.uploaded);
        if (s.computed) (void)hipEventDestroy(s.computed);
        if (s.done) (void)hipEventDestroy(s.done);
        if (s.k_start) (void)hipEventDestroy(s.k_start);
        if (s.k_end) (void)hipEventDestroy(s.k_end);
        free_slot(s);
    }
    if (ctx->c_k0) (void)hipEventDestroy(ctx->c_k0);
    if (ctx->c_k1) (void)hipEventDestroy(ctx->c_k1);
    (void)hipFree(ctx->c_s1);
    (void)hipFree(ctx->c_s2);
    (void)hipFree(ctx->c_res);
    for (auto& r : ctx->rscratch) {
        (void)hipFree(r.wins);
        (void)hipFree(r.wlen);
        (void)hipFree(r.rev);
    }
    for (hipStream_t st : ctx->user_streams) {
        (void)hipStreamSynchronize(st);
        (void)hipStreamDestroy(st);
    }
    for (auto& t : ctx->dev_timings) {
        (void)hipEventDestroy(t.k0);
        (void)hipEventDestroy(t.k1);
    }
    for (hipEvent_t e : ctx->free_events) (void)hipEventDestroy(e);
    for (auto& kv : ctx->fences) (void)hipEventDestroy(kv.second);
    if (ctx->epoch) (void)hipEventDestroy(ctx->epoch);
    if (ctx->epoch_next) (void)hipEventDestroy(ctx->epoch_next);
    if (ctx->compute) (void)hipStreamDestroy(ctx->compute);
    if (ctx->compute2) (void)hipStreamDestroy(ctx->compute2);
    if (ctx->copy) (void)hipStreamDestroy(ctx->copy);
    if (ctx->d2h) (void)hipStreamDestroy(ctx->d2h);
    if (ctx->side) (void)hipStreamDestroy(ctx->side);
    delete ctx;
}

int msw_align_batch(msw_ctx* ctx, const msw_scoring_t* sc, const msw_batch_t* batch, msw_out_t* out,
                    uint64_t chunk_pairs) {
    if (!batch) return fail(MSW_E_INVALID, "batch is NULL");
    return run_batch(ctx, sc, pairs_batch(*batch), out, chunk_pairs, true);
}

int msw_align_batch_async(msw_ctx* ctx, const msw_scoring_t* sc, const msw_batch_t* batch, msw_out_t* out,
                          uint64_t chunk_pairs, uint64_t* ticket) {
    if (!ticket) return fail(MSW_E_INVALID, "ticket is NULL");
    if (!batch) return fail(MSW_E_INVALID, "batch is NULL");
    int rc = run_batch(ctx, sc, pairs_batch(*batch), out, chunk_pairs, false);
    if (rc) return rc;
    *ticket = ctx->next_ticket++;
    return MSW_OK;
}

int msw_wait(msw_ctx* ctx, uint64_t ticket) {
    if (!ctx) return fail(MSW_E_INVALID, "ctx is NULL");
    if (ticket == 0 || ticket >= ctx->next_ticket) return fail(MSW_E_INVALID, "unknown ticket %llu", (unsigned long long)ticket);
    int rc = set_device(ctx);
    if (rc) return rc;
    // Drain the chunks of this ticket and of every earlier one (tickets are
    // enqueued in order on the same streams); later calls stay in flight.
    if ((rc = drain_through(ctx, ticket))) return rc;
    ctx->done_ticket = std::max(ctx->done_ticket, ticket);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MSW_E_DEVICE, "kernel failure: %s", hipGetErrorString(e));
    return MSW_OK;
}

// Diagnostics only (MSW_WAVE_TRACE=file, read by tools/wave_trace.py): the
// launch records per-block clocks and placement and appends one record
// {u64 n_blocks, u64 layout | G << 8 | pairs_blocks << 16, n_blocks x 4 u64}
// to the file.  Synchronous.
static int traced_launch(msw::SwParams p, const Scheme& sch, uint32_t max_read_len, const LaunchPlan& plan,
                         hipStream_t st, const char* path) {
    const uint64_t n_blocks = p.n_slots / 4 + 2;  // the split layout's count bounds every grid
    uint64_t* d = nullptr;
    HIP_TRY(hipMalloc(&d, n_blocks * 4 * sizeof(uint64_t)));
    (void)hipMemsetAsync(d, 0, n_blocks * 4 * sizeof(uint64_t), st);
    p.trace = d;
    hipError_t e = msw::launch_sw(p, sch.affine, sch.coords, max_read_len, plan.layout, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    std::vector<uint64_t> h(n_blocks * 4);
    if (e == hipSuccess) e = hipMemcpy(h.data(), d, h.size() * sizeof(uint64_t), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(MSW_E_DEVICE, "traced launch: %s", hipGetErrorString(e));
    FILE* f = fopen(path, "ab");
    if (!f) return fail(MSW_E_INVALID, "cannot open MSW_WAVE_TRACE file %s", path);
    const uint64_t hdr[2] = {n_blocks, (uint64_t)plan.layout | ((uint64_t)plan.group_lanes << 8) |
                                           ((uint64_t)plan.pairs_blocks << 16)};
    fwrite(hdr, sizeof(hdr), 1, f);
    fwrite(h.data(), sizeof(uint64_t), h.size(), f);
    fclose(f);
    return MSW_OK;
}

// One packed-kernel launch of all n pairs of p (pointers and strides set,
// input order) under the given length bounds: layout from the makespan model.
static int launch_packed(msw_ctx* ctx, const Scheme& sch, const msw::SwParams& p, uint32_t n, uint32_t max_read_len,
                         uint32_t max_win_len, hipStream_t st) {
    const Bucket b{0, n, max_read_len, max_win_len};
    const LaunchPlan plan = choose_layout(n, max_read_len, max_win_len, sch, ctx->cu_count);
    if (!ctx->opt.wave_trace.empty())
        return traced_launch(bucket_params(p, sch, b, plan), sch, max_read_len, plan, st, ctx->opt.wave_trace.c_str());
    return launch_bucket(p, sch, b, plan, st);
}

int msw_align_batch_device(msw_ctx* ctx, const msw_scoring_t* sc, const msw_batch_t* b, msw_out_t* out,
                           uint32_t max_read_len, uint32_t max_win_len, void* stream) {
    if (!ctx) return fail(MSW_E_INVALID, "ctx is NULL");
    Scheme sch;
    int rc;
    if ((rc = make_scheme(sc, ctx->opt, &sch))) return rc;
    if ((rc = validate_batch(b, out, sch))) return rc;
    if (b->n_pairs == 0) return MSW_OK;
    if ((rc = check_bounds(sch, max_read_len, max_win_len))) return rc;
    if ((rc = check_strides(*b, max_read_len, max_win_len))) return rc;
    if ((rc = set_device(ctx))) return rc;
    const msw::SwParams p = batch_params(sch, *b, *out);  // input order: no order array
    hipStream_t st = call_stream(ctx, stream);
    // bounds past the packed kernels: the whole batch on the long-pair kernel
    if (ctx->opt.force_long || is_long(max_read_len, max_win_len))
        return launch_long(sch, p, b->n_pairs, max_read_len, max_win_len, false, ctx->cu_count, st);
    return launch_packed(ctx, sch, p, (uint32_t)b->n_pairs, max_read_len, max_win_len, st);
}

// Traceback supports the packed kernels' range only.
static int check_trace_bounds(uint32_t max_m, uint32_t max_n) {
    if (max_m > (uint32_t)msw::kMaxReadLen)
        return fail(MSW_E_RANGE, "traceback: read length %u > %d", max_m, msw::kMaxReadLen);
    if (max_n > (uint32_t)msw::kMaxWinLen)
        return fail(MSW_E_RANGE, "traceback: window length %u > %d", max_n, msw::kMaxWinLen);
    return MSW_OK;
}

static int validate_trace(const msw_trace_t* tr) {
    if (!tr) return fail(MSW_E_INVALID, "trace is NULL");
    if (!tr->start_i || !tr->start_j || !tr->n_cigar) return fail(MSW_E_INVALID, "NULL array in trace");
    if (tr->cigar_stride && !tr->cigar) return fail(MSW_E_INVALID, "cigar is NULL with cigar_stride > 0");
    return MSW_OK;
}

// The launch both traceback entry points share: LDS layout, LDS / slab switch,
// grid cap and work queue.  p holds the call's inputs and outputs (windows
// from a slab or from the genome); the bounds and scoring are filled here.
static int run_trace(msw_ctx* ctx, const Scheme& sch, const msw_scoring_t* sc, msw::TraceParams p, uint64_t n_pairs,
                     uint32_t max_read_len, uint32_t max_win_len, hipStream_t st) {
    p.n_slots = (uint32_t)n_pairs;
    p.max_rows = max_read_len;
    p.max_cols = max_win_len;
    p.match = sc->match;
    p.mismatch = sc->mismatch;
    p.gap = sc->gap_extend;
    p.goe = sc->gap_open + sc->gap_extend;
    const size_t shm = msw::trace_lds_layout(p, sch.affine);
    // One block per pair while the direction words fit LDS.  A bound whose
    // rectangle does not fit needs a global slab per block: the grid is then
    // capped (what the CUs hold at once, and 256 MiB of slabs) and finished
    // blocks take the next pair from a queue.  Slab and counter are allocated
    // stream-ordered on `st`, like the long-pair launch's scratch.
    const uint64_t need = msw::trace_words(sch.affine, max_read_len, max_win_len);
    const bool slab = need > p.lds_words;
    const uint64_t slab_bytes = slab ? need * sizeof(uint32_t) : 0;
    uint64_t blocks = n_pairs;
    if (slab) {
        const int per_cu = msw::trace_blocks_per_cu(sch.affine, max_read_len, shm);
        if (per_cu <= 0) return fail(MSW_E_DEVICE, "traceback kernel does not fit a CU");
        const uint64_t resident = (uint64_t)(ctx->cu_count > 0 ? ctx->cu_count : 256) * (uint64_t)per_cu;
        blocks = std::min(blocks, std::min(resident, std::max<uint64_t>(1, (256ull << 20) / slab_bytes)));
    }
    if (ctx->opt.trace_blocks) blocks = std::min<uint64_t>(blocks, ctx->opt.trace_blocks);  // tests: a fixed block count
    const bool queue = blocks < n_pairs;
    uint8_t* mem = nullptr;
    if (slab || queue) {
        HIP_TRY(hipMallocAsync((void**)&mem, blocks * slab_bytes + 256, st));
        if (slab) {
            p.slab = reinterpret_cast<uint32_t*>(mem);
            p.slab_words = need;
        }
        if (queue) {
            p.next = reinterpret_cast<uint32_t*>(mem + blocks * slab_bytes);
            const hipError_t em = hipMemsetAsync(p.next, 0, sizeof(uint32_t), st);
            if (em != hipSuccess) {
                (void)hipFreeAsync(mem, st);
                HIP_TRY(em);
            }
        }
    }
    const hipError_t e = msw::launch_sw_trace(p, sch.affine, (uint32_t)blocks, shm, st);
    if (mem) HIP_TRY(hipFreeAsync(mem, st));
    HIP_TRY(e);
    return MSW_OK;
}

static void trace_outputs(msw::TraceParams& p, const msw_out_t* ends, const msw_trace_t* tr) {
    p.end_i = ends->end_i;
    p.end_j = ends->end_j;
    p.start_i = tr->start_i;
    p.start_j = tr->start_j;
    p.n_cigar = tr->n_cigar;
    p.cigar = tr->cigar;
    p.cigar_stride = tr->cigar_stride;
}

int msw_trace_batch_device(msw_ctx* ctx, const msw_scoring_t* sc, const msw_batch_t* b, const msw_out_t* ends,
                           msw_trace_t* tr, uint32_t max_read_len, uint32_t max_win_len, void* stream) {
    if (!ctx) return fail(MSW_E_INVALID, "ctx is NULL");
    Scheme sch;
    int rc;
    if ((rc = make_scheme(sc, ctx->opt, &sch))) return rc;
    sch.coords = true;  // want_coords is not read: the ends are an input here
    if ((rc = validate_batch(b, ends, sch)) || (rc = validate_trace(tr))) return rc;
    if (b->n_pairs == 0) return MSW_OK;
    if ((rc = check_trace_bounds(max_read_len, max_win_len))) return rc;
    // one block per pair: a 1-D grid holds 2^31 - 1 blocks
    if (b->n_pairs > 0x7FFFFFFFull) return fail(MSW_E_RANGE, "traceback: n_pairs > 2^31-1 in one call");
    if ((rc = check_strides(*b, max_read_len, max_win_len))) return rc;
    if ((rc = set_device(ctx))) return rc;
    hipStream_t st = call_stream(ctx, stream);
    msw::TraceParams p;
    memset(&p, 0, sizeof(p));
    p.reads = b->reads;
    p.wins = b->wins;
    p.read_len = b->read_len;
    p.win_len = b->win_len;
    p.read_stride = b->read_stride;
    p.win_stride = b->win_stride;
    trace_outputs(p, ends, tr);
    return run_trace(ctx, sch, sc, p, b->n_pairs, max_read_len, max_win_len, st);
}

int msw_trace_reads_device(msw_ctx* ctx, const msw_scoring_t* sc, const msw_genome* g, const uint8_t* reads,
                           const uint16_t* read_len, uint32_t read_stride, const int64_t* win_pos, uint64_t n,
                           uint32_t window, uint32_t max_read_len, const msw_out_t* ends, msw_trace_t* tr,
                           void* stream) {
    if (!ctx || !g) return fail(MSW_E_INVALID, "ctx/genome is NULL");
    if (g->ctx != ctx) return fail(MSW_E_INVALID, "genome belongs to another context");
    Scheme sch;
    int rc;
    if ((rc = make_scheme(sc, ctx->opt, &sch))) return rc;
    if ((rc = validate_trace(tr))) return rc;
    if (n == 0) return MSW_OK;
    if (!reads || !read_len || !win_pos) return fail(MSW_E_INVALID, "NULL array");
    if (!ends || !ends->end_i || !ends->end_j) return fail(MSW_E_INVALID, "traceback needs end_i / end_j");
    // the window bound of msw_align_reads_device
    const uint32_t max_win = window ? window : std::min<uint32_t>(2u * max_read_len, (uint32_t)msw::kMaxWinLen);
    if ((rc = check_trace_bounds(max_read_len, max_win))) return rc;
    if (n > 0x7FFFFFFFull) return fail(MSW_E_RANGE, "traceback: n > 2^31-1 in one call");
    if (max_read_len > read_stride) return fail(MSW_E_INVALID, "max_read_len exceeds read_stride");
    if ((rc = set_device(ctx))) return rc;
    hipStream_t st = call_stream(ctx, stream);
    msw::TraceParams p;
    memset(&p, 0, sizeof(p));
    p.reads = reads;
    p.read_len = read_len;
    p.read_stride = read_stride;
    p.genome = g->d_seq;
    p.glen = g->len;
    p.win_pos = win_pos;
    p.window = window;
    trace_outputs(p, ends, tr);
    return run_trace(ctx, sch, sc, p, n, max_read_len, max_win, st);
}

static int validate_aln(const msw_aln_t* a) {
    if (!a) return fail(MSW_E_INVALID, "aln is NULL");
    if (!a->ref_pos || !a->nm || !a->cigar_off || !a->n_overflow) return fail(MSW_E_INVALID, "NULL array in aln");
    if (a->cigar_cap && !a->cigar) return fail(MSW_E_INVALID, "cigar is NULL with cigar_cap > 0");
    return MSW_OK;
}

int msw_aln_pack_device(msw_ctx* ctx, const msw_genome* g, const uint8_t* reads, const uint16_t* read_len,
                        uint32_t read_stride, const int64_t* win_pos, uint64_t n, const msw_out_t* ends,
                        const msw_trace_t* tr, msw_aln_t* aln, void* stream) {
    if (!ctx || !g) return fail(MSW_E_INVALID, "ctx/genome is NULL");
    if (g->ctx != ctx) return fail(MSW_E_INVALID, "genome belongs to another context");
    int rc;
    if ((rc = validate_aln(aln))) return rc;
    if (n > 0x7FFFFFFFull) return fail(MSW_E_RANGE, "aln pack: n > 2^31-1 in one call");
    if (n) {
        if ((rc = validate_trace(tr))) return rc;
        if (!reads || !read_len || !win_pos) return fail(MSW_E_INVALID, "NULL array");
        if (!ends || !ends->score || !ends->end_i || !ends->end_j)
            return fail(MSW_E_INVALID, "aln pack needs score / end_i / end_j");
    }
    if ((rc = set_device(ctx))) return rc;
    hipStream_t st = call_stream(ctx, stream);
    msw::AlnParams p;
    memset(&p, 0, sizeof(p));
    p.genome = g->d_seq;
    p.glen = g->len;
    p.reads = reads;
    p.read_len = read_len;
    p.read_stride = read_stride;
    p.win_pos = win_pos;
    p.n = n;
    if (n) {
        p.score = ends->score;
        p.end_i = ends->end_i;
        p.start_i = tr->start_i;
        p.start_j = tr->start_j;
        p.n_cigar = tr->n_cigar;
        p.rows = tr->cigar;
        p.cigar_stride = tr->cigar_stride;
    }
    p.ref_pos = aln->ref_pos;
    p.nm = aln->nm;
    p.cigar_off = aln->cigar_off;
    p.cigar = aln->cigar;
    p.cigar_cap = aln->cigar_cap;
    p.n_overflow = aln->n_overflow;
    HIP_TRY(msw::launch_aln_pack(p, st));
    return MSW_OK;
}

int msw_align_batch_trace(msw_ctx* ctx, const msw_scoring_t* sc, const msw_batch_t* b, msw_out_t* out,
                          msw_trace_t* tr, uint64_t chunk_pairs) {
    if (!ctx) return fail(MSW_E_INVALID, "ctx is NULL");
    if (!sc) return fail(MSW_E_INVALID, "scoring is NULL");
    msw_scoring_t scc = *sc;
    scc.want_coords = 1;
    Scheme sch;
    int rc;
    if ((rc = make_scheme(&scc, ctx->opt, &sch))) return rc;
    if ((rc = validate_batch(b, out, sch)) || (rc = validate_trace(tr))) return rc;
    const uint64_t n = b->n_pairs;
    if (n == 0) return MSW_OK;
    uint32_t max_m = 0, max_n = 0;
    max_u16(b->read_len, n, max_m);
    max_u16(b->win_len, n, max_n);
    if ((rc = check_trace_bounds(max_m, max_n))) return rc;
    if (max_m > b->read_stride || max_n > b->win_stride) return fail(MSW_E_INVALID, "a length exceeds its stride");
    if ((rc = set_device(ctx))) return rc;
    // Simple and synchronous: per chunk upload, score with coordinates, trace,
    // download (not part of the three-slot staging pipeline).
    const uint64_t chunk = std::min<uint64_t>(n, chunk_pairs ? chunk_pairs : 65536);
    const size_t rs = b->read_stride, ws = b->win_stride, cs = tr->cigar_stride;
    // [reads | wins | cigar u32 | score i32 | n_cigar i32 | rlen wlen end_i end_j start_i start_j, 2 B each]
    const size_t o_wins = (chunk * rs + 255) & ~(size_t)255, o_cig = (o_wins + chunk * ws + 255) & ~(size_t)255;
    const size_t o_score = o_cig + chunk * cs * 4, o_nc = o_score + chunk * 4, o_h = o_nc + chunk * 4;
    uint8_t* d = nullptr;
    hipError_t e = hipMalloc((void**)&d, o_h + chunk * 12 + 256);
    if (e != hipSuccess) return fail(MSW_E_NOMEM, "hipMalloc(%zu B): %s", o_h + chunk * 12, hipGetErrorString(e));
    uint16_t* d_rl = reinterpret_cast<uint16_t*>(d + o_h);
    uint16_t* d_wl = d_rl + chunk;
    int16_t *d_ei = reinterpret_cast<int16_t*>(d_wl + chunk), *d_ej = d_ei + chunk, *d_si = d_ej + chunk,
            *d_sj = d_si + chunk;
    hipStream_t st = ctx->compute;
    rc = MSW_OK;
    for (uint64_t lo = 0; lo < n && rc == MSW_OK; lo += chunk) {
        const uint64_t c = std::min(chunk, n - lo);
        uint32_t cm = 0, cn = 0;
        max_u16(b->read_len + lo, c, cm);
        max_u16(b->win_len + lo, c, cn);
        auto up = [&](void* dst, const void* src, size_t bytes) {
            if (e == hipSuccess && bytes) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st);
        };
        auto down = [&](void* dst, const void* src, size_t bytes) {
            if (e == hipSuccess && bytes) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st);
        };
        up(d, b->reads + lo * rs, c * rs);
        up(d + o_wins, b->wins + lo * ws, c * ws);
        up(d_rl, b->read_len + lo, c * 2);
        up(d_wl, b->win_len + lo, c * 2);
        if (e != hipSuccess) break;
        msw_batch_t db = {d, d + o_wins, d_rl, d_wl, (uint32_t)rs, (uint32_t)ws, c};
        msw_out_t dout = {reinterpret_cast<int32_t*>(d + o_score), d_ei, d_ej};
        msw_trace_t dtr = {d_si, d_sj, reinterpret_cast<int32_t*>(d + o_nc), reinterpret_cast<uint32_t*>(d + o_cig),
                           (uint32_t)cs};
        if ((rc = msw_align_batch_device(ctx, &scc, &db, &dout, cm, cn, st))) break;
        // same stream: the trace reads the ends the scoring launch wrote
        if ((rc = msw_trace_batch_device(ctx, &scc, &db, &dout, &dtr, cm, cn, st))) break;
        down(out->score + lo, dout.score, c * 4);
        down(out->end_i + lo, d_ei, c * 2);
        down(out->end_j + lo, d_ej, c * 2);
        down(tr->start_i + lo, d_si, c * 2);
        down(tr->start_j + lo, d_sj, c * 2);
        down(tr->n_cigar + lo, dtr.n_cigar, c * 4);
        if (cs) down(tr->cigar + lo * cs, dtr.cigar, c * cs * 4);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
    }
    if (e != hipSuccess) (void)hipStreamSynchronize(st);
    (void)hipFree(d);
    if (rc) return rc;
    if (e != hipSuccess) return fail(MSW_E_DEVICE, "traceback: %s", hipGetErrorString(e));
    return MSW_OK;
}

}  // extern "C"

struct msw_plan {
    const msw_ctx* ctx = nullptr;  // identity only: destroy must not touch the context
    int device = 0;
    Scheme sch{};
    uint64_t n = 0;
    uint32_t max_m = 0, max_n = 0;
    uint32_t* d_order = nullptr;
    // Non-identity order: the kernel writes results in slot order into d_tmp
    // (score i32 | end_i i16 | end_j i16, n each) and a gather pass puts them
    // in pair order through d_inv (pair -> slot): coalesced stores instead of
    // one scattered 4-byte store per pair.
    bool identity = true;
    uint32_t* d_inv = nullptr;
    uint8_t* d_tmp = nullptr;
    uint32_t* d_slot_lens = nullptr;  // read_len | win_len << 16 in slot order
    BucketSchedule sched;             // the launches of one call
};

extern "C" {

int msw_plan_create(msw_ctx* ctx, const msw_scoring_t* sc, const uint16_t* read_len, const uint16_t* win_len,
                    uint64_t n_pairs, msw_plan** out) {
    if (!ctx || !out) return fail(MSW_E_INVALID, "ctx/out is NULL");
    *out = nullptr;
    Scheme sch;
    int rc;
    if ((rc = make_scheme(sc, ctx->opt, &sch))) return rc;
    if (n_pairs && (!read_len || !win_len)) return fail(MSW_E_INVALID, "NULL length array");
    if (n_pairs > 0xFFFFFFFFull) return fail(MSW_E_RANGE, "n_pairs > 2^32-1");
    uint32_t gm = 0, gn = 0;
    max_u16(read_len, n_pairs, gm);
    max_u16(win_len, n_pairs, gn);
    if ((rc = check_bounds(sch, gm, gn))) return rc;
    if ((rc = set_device(ctx))) return rc;
    msw_plan* pl = new msw_plan();
    pl->ctx = ctx;
    pl->device = ctx->device;
    pl->sch = sch;
    pl->n = n_pairs;
    pl->max_m = gm;
    pl->max_n = gn;
    if (n_pairs) {
        std::vector<uint32_t> order(n_pairs);
        std::vector<Bucket> buckets;
        uint32_t lens[4];
        bucket_chunk(read_len, win_len, n_pairs, order.data(), buckets, lens, ctx->opt.force_long);
        pl->sched = schedule_buckets(buckets, sch, ctx->cu_count, true);
        rc = grow_dev(&pl->d_order, n_pairs);
        hipError_t e = rc ? hipSuccess : hipMemcpy(pl->d_order, order.data(), n_pairs * sizeof(uint32_t),
                                                   hipMemcpyHostToDevice);
        if (!rc && e != hipSuccess) rc = fail(MSW_E_DEVICE, "plan upload: %s", hipGetErrorString(e));
        for (uint64_t k = 0; k < n_pairs && pl->identity; ++k) pl->identity = order[k] == (uint32_t)k;
        if (!rc && !pl->identity) {
            std::vector<uint32_t> inv(n_pairs), lens(n_pairs);
            for (uint64_t k = 0; k < n_pairs; ++k) {
                inv[order[k]] = (uint32_t)k;
                lens[k] = (uint32_t)read_len[order[k]] | ((uint32_t)win_len[order[k]] << 16);
            }
            if (!(rc = grow_dev(&pl->d_inv, n_pairs)) && !(rc = grow_dev(&pl->d_tmp, n_pairs * kResBytesPerPair)) &&
                !(rc = grow_dev(&pl->d_slot_lens, n_pairs))) {
                e = hipMemcpy(pl->d_inv, inv.data(), n_pairs * sizeof(uint32_t), hipMemcpyHostToDevice);
                if (e == hipSuccess)
                    e = hipMemcpy(pl->d_slot_lens, lens.data(), n_pairs * sizeof(uint32_t), hipMemcpyHostToDevice);
                if (e != hipSuccess) rc = fail(MSW_E_DEVICE, "plan upload: %s", hipGetErrorString(e));
            }
        }
        if (rc) {
            msw_plan_destroy(pl);
            return rc;
        }
    }
    *out = pl;
    return MSW_OK;
}

int msw_align_batch_planned(msw_ctx* ctx, const msw_plan* plan, const msw_batch_t* b, msw_out_t* out,
                            void* stream) {
    if (!ctx || !plan) return fail(MSW_E_INVALID, "ctx/plan is NULL");
    if (plan->ctx != ctx) return fail(MSW_E_INVALID, "plan belongs to another context");
    int rc;
    if ((rc = validate_batch(b, out, plan->sch))) return rc;
    if (b->n_pairs != plan->n)
        return fail(MSW_E_INVALID, "batch has %llu pairs, plan %llu", (unsigned long long)b->n_pairs,
                    (unsigned long long)plan->n);
    if (plan->n == 0) return MSW_OK;
    if ((rc = check_strides(*b, plan->max_m, plan->max_n))) return rc;
    if ((rc = set_device(ctx))) return rc;
    const Scheme& sch = plan->sch;
    msw::SwParams p = batch_params(sch, *b, *out);
    p.order = plan->d_order;  // also when it is the identity: the multi launches need one
    hipStream_t st = call_stream(ctx, stream);
    const uint64_t n = plan->n;
    int32_t* t_score = reinterpret_cast<int32_t*>(plan->d_tmp);
    int16_t* t_i = reinterpret_cast<int16_t*>(plan->d_tmp + 4 * n);
    int16_t* t_j = reinterpret_cast<int16_t*>(plan->d_tmp + 6 * n);
    if (!plan->identity) {  // slot-ordered lengths and results, gathered below
        p.out_by_slot = 1;
        p.slot_lens = plan->d_slot_lens;
        p.score = t_score;
        p.end_i = sch.coords ? t_i : nullptr;
        p.end_j = sch.coords ? t_j : nullptr;
    }
    if ((rc = issue_schedule(ctx, sch, p, plan->sched, st))) return rc;
    if (!plan->identity)
        HIP_TRY(msw::launch_gather_results(plan->d_inv, t_score, t_i, t_j, out->score, sch.coords ? out->end_i : nullptr,
                                           sch.coords ? out->end_j : nullptr, n, st));
    return MSW_OK;
}

void msw_plan_destroy(msw_plan* plan) {
    if (!plan) return;
    if (plan->d_order || plan->d_inv || plan->d_tmp || plan->d_slot_lens) {
        (void)hipSetDevice(plan->device);
        for (void* q : {(void*)plan->d_order, (void*)plan->d_inv, (void*)plan->d_tmp, (void*)plan->d_slot_lens})
            if (q) (void)hipFree(q);
    }
    delete plan;
}

int msw_align_compat(msw_ctx* ctx, const uint8_t* s1, size_t n1, const uint8_t* s2, size_t n2, uint32_t wg,
                     uint32_t max_groups, int32_t* score) {
    if (!ctx || !score) return fail(MSW_E_INVALID, "ctx/score is NULL");
    *score = 0;
    const size_t L = std::min(n1, n2);
    if (L == 0) return MSW_OK;                                 // aligner.rs:414-416
    if (!s1 || !s2) return fail(MSW_E_INVALID, "NULL sequence");
    int rc = set_device(ctx);
    if (rc) return rc;
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, ctx->device));
    const uint32_t W = wg ? wg : std::min<uint32_t>((uint32_t)prop.maxThreadsPerBlock, 1024u);  // aligner.rs:422
    const uint64_t G = std::min<uint64_t>((L + W - 1) / W, max_groups ? max_groups : 1000000u);  // :423-424
    // aligner.rs:436-456: min(1,000,000 * 1024 work items, 80 % of memory / 3).
    size_t fr = 0, tot = 0;
    HIP_TRY(hipMemGetInfo(&fr, &tot));
    const uint64_t cap = std::min<uint64_t>(1024000000ull, (uint64_t)(tot * 0.8) / 3);
    if (L > cap)
        return fail(MSW_E_RANGE, "Sequence too large (%zu bytes), max allowed: %llu bytes (%llu MB)", L,
                    (unsigned long long)cap, (unsigned long long)(cap / (1024 * 1024)));
    if (L > ctx->c_cap) {
        if ((rc = grow_dev(&ctx->c_s1, L)) || (rc = grow_dev(&ctx->c_s2, L))) return rc;
        ctx->c_cap = L;
    }
    if (!ctx->c_res && (rc = grow_dev(&ctx->c_res, 1))) return rc;
    HIP_TRY(hipMemcpyAsync(ctx->c_s1, s1, L, hipMemcpyHostToDevice, ctx->compute));
    HIP_TRY(hipMemcpyAsync(ctx->c_s2, s2, L, hipMemcpyHostToDevice, ctx->compute));
    HIP_TRY(hipMemsetAsync(ctx->c_res, 0, sizeof(int32_t), ctx->compute));
    if (!ctx->c_k0) {
        HIP_TRY(hipEventCreate(&ctx->c_k0));
        HIP_TRY(hipEventCreate(&ctx->c_k1));
    }
    HIP_TRY(hipEventRecord(ctx->c_k0, ctx->compute));
    HIP_TRY(msw::launch_compat(ctx->c_s1, ctx->c_s2, ctx->c_res, L, W, G, ctx->compute));
    HIP_TRY(hipEventRecord(ctx->c_k1, ctx->compute));
    HIP_TRY(hipMemcpyAsync(score, ctx->c_res, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->compute));
    HIP_TRY(hipStreamSynchronize(ctx->compute));
    add_kernel_interval(ctx, ctx->c_k0, ctx->c_k1);
    ctx->stats.launches += 1;
    ctx->stats.alg_bytes += 2ull * L + 4;
    return MSW_OK;
}

int msw_genome_create(msw_ctx* ctx, const uint8_t* seq, uint64_t len, msw_genome** out) {
    if (!ctx || !out) return fail(MSW_E_INVALID, "ctx/out is NULL");
    *out = nullptr;
    if (len && !seq) return fail(MSW_E_INVALID, "seq is NULL");
    int rc = set_device(ctx);
    if (rc) return rc;
    msw_genome* g = new msw_genome();
    g->ctx = ctx;
    g->device = ctx->device;
    g->len = len;
    hipError_t e = hipMalloc((void**)&g->d_seq, len + msw::kGenomePad);
    if (e != hipSuccess) {
        delete g;
        return fail(MSW_E_NOMEM, "hipMalloc(%llu B) for the genome: %s", (unsigned long long)len, hipGetErrorString(e));
    }
    // on the compute stream (the call is synchronous; a --full-wgs worker
    // then never creates its copy stream)
    e = hipMemsetAsync(g->d_seq + len, 0, msw::kGenomePad, ctx->compute);
    if (e == hipSuccess && len) e = hipMemcpyAsync(g->d_seq, seq, len, hipMemcpyHostToDevice, ctx->compute);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->compute);
    if (e != hipSuccess) {
        msw_genome_destroy(g);
        return fail(MSW_E_DEVICE, "genome upload: %s", hipGetErrorString(e));
    }
    *out = g;
    return MSW_OK;
}

void msw_genome_destroy(msw_genome* g) {
    if (!g) return;
    if (g->d_seq) {
        (void)hipSetDevice(g->device);
        (void)hipFree(g->d_seq);
    }
    delete g;
}

uint64_t msw_genome_length(const msw_genome* g) { return g ? g->len : 0; }

int msw_genome_cut_device(msw_ctx* ctx, const msw_genome* g, const int64_t* win_pos, const uint16_t* win_len,
                          uint64_t n, uint8_t* wins, uint32_t win_stride, uint16_t* win_len_out, void* stream) {
    if (!ctx || !g) return fail(MSW_E_INVALID, "ctx/genome is NULL");
    if (g->ctx != ctx) return fail(MSW_E_INVALID, "genome belongs to another context");
    if (n == 0) return MSW_OK;
    if (!win_pos || !win_len || !wins) return fail(MSW_E_INVALID, "NULL array");
    if (win_stride == 0 || win_stride % 16 != 0 || ((uintptr_t)wins & 15) != 0)
        return fail(MSW_E_INVALID, "win_stride must be a non-zero multiple of 16 and wins 16-byte aligned");
    int rc = set_device(ctx);
    if (rc) return rc;
    hipStream_t st = call_stream(ctx, stream);
    HIP_TRY(msw::launch_cut_windows(g->d_seq, g->len, win_pos, win_len, wins, win_len_out, win_stride, n, st));
    return MSW_OK;
}

int msw_align_reads(msw_ctx* ctx, const msw_scoring_t* sc, const msw_genome* g, const msw_read_batch_t* batch,
                    msw_out_t* out, uint64_t chunk_pairs) {
    if (!batch || !g) return fail(MSW_E_INVALID, "batch/genome is NULL");
    return run_batch(ctx, sc, reads_batch(*batch, g), out, chunk_pairs, true);
}

int msw_align_reads_async(msw_ctx* ctx, const msw_scoring_t* sc, const msw_genome* g,
                          const msw_read_batch_t* batch, msw_out_t* out, uint64_t chunk_pairs, uint64_t* ticket) {
    if (!ticket) return fail(MSW_E_INVALID, "ticket is NULL");
    if (!batch || !g) return fail(MSW_E_INVALID, "batch/genome is NULL");
    int rc = run_batch(ctx, sc, reads_batch(*batch, g), out, chunk_pairs, false);
    if (rc) return rc;
    *ticket = ctx->next_ticket++;
    return MSW_OK;
}

// The window cut of the device-resident reads calls: the windows of n reads
// into the stream's scratch slab; b gets the slab, the clipped lengths and the
// stride (its reads stay the caller's), *max_win_out the window bound.
static int cut_reads_windows(msw_ctx* ctx, const msw_genome* g, const uint16_t* read_len, const int64_t* win_pos,
                             uint64_t n, uint32_t window, uint32_t max_read_len, uint16_t* win_len_out,
                             hipStream_t st, msw_batch_t* b, uint32_t* max_win_out) {
    int rc;
    const uint32_t max_win = window ? window : std::min<uint32_t>(2u * max_read_len, (uint32_t)msw::kMaxWinLen);
    harvest_dev_timings(ctx, false);
    const uint32_t ws = std::max<uint32_t>(16u, (max_win + 15u) & ~15u);
    const size_t wbytes = (size_t)n * ws;
    msw_ctx::ReadsScratch* rs = nullptr;
    for (auto& r : ctx->rscratch)
        if (r.st == st) rs = &r;
    if (!rs) {
        ctx->rscratch.emplace_back();
        rs = &ctx->rscratch.back();
        rs->st = st;
    }
    if (wbytes > rs->wins_cap) {
        if ((rc = grow_dev(&rs->wins, wbytes + wbytes / 4))) return rc;
        rs->wins_cap = wbytes + wbytes / 4;
    }
    uint16_t* wlen = win_len_out;
    if (!wlen) {
        if (n > rs->wlen_cap) {
            if ((rc = grow_dev(&rs->wlen, (size_t)n + n / 4))) return rc;
            rs->wlen_cap = (size_t)n + n / 4;
        }
        wlen = rs->wlen;
    }
    HIP_TRY(msw::launch_cut_windows_for_reads(g->d_seq, g->len, win_pos, read_len, window, rs->wins, wlen, ws, n,
                                              st));
    b->wins = rs->wins;
    b->read_len = read_len;
    b->win_len = wlen;
    b->win_stride = ws;
    b->n_pairs = n;
    *max_win_out = max_win;
    return MSW_OK;
}

// One scoring pass of a device-resident reads call over the cut windows,
// between the timing events msw_ctx_stats harvests.
static int score_reads_batch(msw_ctx* ctx, const msw_scoring_t* sc, const msw_batch_t* b, msw_out_t* out,
                             uint32_t max_read_len, uint32_t max_win, void* stream, hipStream_t st) {
    int rc;
    msw_ctx::DevTiming t{take_event(ctx), take_event(ctx), b->n_pairs};
    if (!t.k0 || !t.k1) return fail(MSW_E_DEVICE, "hipEventCreate failed");
    HIP_TRY(hipEventRecord(t.k0, st));
    if ((rc = msw_align_batch_device(ctx, sc, b, out, max_read_len, max_win, stream))) return rc;
    HIP_TRY(hipEventRecord(t.k1, st));
    ctx->dev_timings.push_back(t);
    return MSW_OK;
}

int msw_align_reads_device(msw_ctx* ctx, const msw_scoring_t* sc, const msw_genome* g, const uint8_t* reads,
                           const uint16_t* read_len, uint32_t read_stride, const int64_t* win_pos, uint64_t n,
                           uint32_t window, uint32_t max_read_len, msw_out_t* out, uint16_t* win_len_out,
                           void* stream) {
    if (!ctx || !g) return fail(MSW_E_INVALID, "ctx/genome is NULL");
    if (g->ctx != ctx) return fail(MSW_E_INVALID, "genome belongs to another context");
    if (n == 0) return MSW_OK;
    if (!reads || !read_len || !win_pos || !out || !out->score) return fail(MSW_E_INVALID, "NULL array");
    if (window > (uint32_t)msw::kMaxLongLen) return fail(MSW_E_RANGE, "window %u > %d", window, msw::kMaxLongLen);
    int rc = set_device(ctx);
    if (rc) return rc;
    hipStream_t st = call_stream(ctx, stream);
    msw_batch_t b{reads, nullptr, read_len, nullptr, read_stride, 0, n};
    uint32_t max_win = 0;
    if ((rc = cut_reads_windows(ctx, g, read_len, win_pos, n, window, max_read_len, win_len_out, st, &b, &max_win)))
        return rc;
    return score_reads_batch(ctx, sc, &b, out, max_read_len, max_win, stream, st);
}

static int check_oriented(const void* strand, const void* oriented, uint32_t oriented_stride, uint32_t max_read_len) {
    if (!strand || !oriented) return fail(MSW_E_INVALID, "strand/oriented is NULL");
    if (((uintptr_t)oriented & 15) != 0 || oriented_stride == 0 || oriented_stride % 16 != 0)
        return fail(MSW_E_INVALID, "oriented must be 16-byte aligned and oriented_stride a non-zero multiple of 16");
    if (oriented_stride < max_read_len) return fail(MSW_E_INVALID, "oriented_stride is below max_read_len");
    return MSW_OK;
}

// Both orientations of the device batch b (windows cut) on one stream:
// reverse complements into `oriented`, forward scoring into `out`, reverse
// scoring into the stream's own scratch, then the choice per read.  `score`
// is one scoring pass (both go through msw_align_batch_device).
using ScorePass = std::function<int(const msw_batch_t*, msw_out_t*)>;
static int score_both_strands(msw_ctx* ctx, const msw_scoring_t* sc, const msw_batch_t* b, msw_out_t* out, uint8_t* strand,
                              uint8_t* oriented, uint32_t oriented_stride, hipStream_t st, const ScorePass& score) {
    const uint64_t n = b->n_pairs;
    int rc;
    HIP_TRY(msw::launch_revcomp_rows(b->reads, b->read_len, b->read_stride, n, oriented, oriented_stride, st));
    if ((rc = score(b, out))) return rc;
    const bool coords = sc->want_coords != 0;
    // [score i32 | end_i i16 | end_j i16], n each, in the stream's own scratch:
    // everything that touches it is ordered on `st`
    msw_ctx::ReadsScratch* rs = nullptr;
    for (auto& r : ctx->rscratch)
        if (r.st == st) rs = &r;
    if (!rs) {
        ctx->rscratch.emplace_back();
        rs = &ctx->rscratch.back();
        rs->st = st;
    }
    const size_t need = n * 8 + 16;
    if (need > rs->rev_cap) {
        if ((rc = grow_dev(&rs->rev, need + need / 4))) return rc;
        rs->rev_cap = need + need / 4;
    }
    uint8_t* tmp = rs->rev;
    msw_out_t rout = {reinterpret_cast<int32_t*>(tmp), nullptr, nullptr};
    if (coords) {
        rout.end_i = reinterpret_cast<int16_t*>(tmp + n * 4);
        rout.end_j = rout.end_i + n;
    }
    msw_batch_t rb = *b;
    rb.reads = oriented;
    rb.read_stride = oriented_stride;
    rc = score(&rb, &rout);
    hipError_t e = hipSuccess;
    if (rc == MSW_OK)
        e = msw::launch_strand_select(b->reads, b->read_len, b->read_stride, n, oriented, oriented_stride, out->score,
                                      coords ? out->end_i : nullptr, coords ? out->end_j : nullptr, rout.score,
                                      rout.end_i, rout.end_j, strand, st);
    if (rc) return rc;
    HIP_TRY(e);
    return MSW_OK;
}

int msw_revcomp_device(msw_ctx* ctx, const uint8_t* reads, const uint16_t* read_len, uint32_t read_stride, uint64_t n,
                       uint8_t* out, uint32_t out_stride, void* stream) {
    if (!ctx) return fail(MSW_E_INVALID, "ctx is NULL");
    if (n == 0) return MSW_OK;
    if (!reads || !read_len || !out) return fail(MSW_E_INVALID, "NULL array");
    if (read_stride == 0) return fail(MSW_E_INVALID, "read_stride is 0");
    if (((uintptr_t)out & 15) != 0 || out_stride == 0 || out_stride % 16 != 0)
        return fail(MSW_E_INVALID, "out must be 16-byte aligned and out_stride a non-zero multiple of 16");
    if (n > 0x7FFFFFFFull || n * (out_stride / 16u) > (0x7FFFFFFFull << 8))
        return fail(MSW_E_RANGE, "revcomp: too many rows in one call");
    int rc = set_device(ctx);
    if (rc) return rc;
    HIP_TRY(msw::launch_revcomp_rows(reads, read_len, read_stride, n, out, out_stride, call_stream(ctx, stream)));
    return MSW_OK;
}

int msw_align_reads_strands_device(msw_ctx* ctx, const msw_scoring_t* sc, const msw_genome* g, const uint8_t* reads,
                                   const uint16_t* read_len, uint32_t read_stride, const int64_t* win_pos, uint64_t n,
                                   uint32_t window, uint32_t max_read_len, msw_out_t* out, uint16_t* win_len_out,
                                   uint8_t* strand, uint8_t* oriented, uint32_t oriented_stride, void* stream) {
    if (!ctx || !g) return fail(MSW_E_INVALID, "ctx/genome is NULL");
    if (g->ctx != ctx) return fail(MSW_E_INVALID, "genome belongs to another context");
    if (!sc) return fail(MSW_E_INVALID, "scoring is NULL");
    if (n == 0) return MSW_OK;
    if (!reads || !read_len || !win_pos || !out || !out->score) return fail(MSW_E_INVALID, "NULL array");
    if (sc->want_coords && (!out->end_i || !out->end_j)) return fail(MSW_E_INVALID, "want_coords needs end_i / end_j");
    int rc;
    if ((rc = check_oriented(strand, oriented, oriented_stride, max_read_len))) return rc;
    if (window > (uint32_t)msw::kMaxLongLen) return fail(MSW_E_RANGE, "window %u > %d", window, msw::kMaxLongLen);
    if (max_read_len > read_stride) return fail(MSW_E_INVALID, "max_read_len exceeds read_stride");
    if (n > 0x7FFFFFFFull || n * (oriented_stride / 16u) > (0x7FFFFFFFull << 8))
        return fail(MSW_E_RANGE, "both strands: too many rows in one call");
    // scheme and bounds before anything is enqueued (the scoring passes check them again)
    Scheme sch;
    if ((rc = make_scheme(sc, ctx->opt, &sch))) return rc;
    const uint32_t bound_win = window ? window : std::min<uint32_t>(2u * max_read_len, (uint32_t)msw::kMaxWinLen);
    if ((rc = check_bounds(sch, max_read_len, bound_win))) return rc;
    if ((rc = set_device(ctx))) return rc;
    hipStream_t st = call_stream(ctx, stream);
    msw_batch_t b{reads, nullptr, read_len, nullptr, read_stride, 0, n};
    uint32_t max_win = 0;
    if ((rc = cut_reads_windows(ctx, g, read_len, win_pos, n, window, max_read_len, win_len_out, st, &b, &max_win)))
        return rc;
    return score_both_strands(ctx, sc, &b, out, strand, oriented, oriented_stride, st,
                              [&](const msw_batch_t* pb, msw_out_t* po) {
                                  return score_reads_batch(ctx, sc, pb, po, max_read_len, max_win, stream, st);
                              });
}

// The body of msw_align_reads_trace (strand == NULL: aln required) and of
// msw_align_reads_strands (strand != NULL: both orientations are scored, the
// trace and the pack read the oriented rows, and aln may be NULL for scores
// alone, with coordinates as sc says).
static int reads_records(msw_ctx* ctx, const msw_scoring_t* sc, const msw_genome* g, const msw_read_batch_t* b,
                         msw_out_t* out, msw_aln_t* aln, uint8_t* strand, bool both, uint64_t chunk_pairs) {
    if (!ctx || !g) return fail(MSW_E_INVALID, "ctx/genome is NULL");
    if (g->ctx != ctx) return fail(MSW_E_INVALID, "genome belongs to another context");
    if (!sc || !b) return fail(MSW_E_INVALID, "scoring/batch is NULL");
    msw_scoring_t scc = *sc;
    if (aln) scc.want_coords = 1;
    const bool coords = scc.want_coords != 0;
    Scheme sch;
    int rc;
    if ((rc = make_scheme(&scc, ctx->opt, &sch))) return rc;
    if ((aln || !both) && (rc = validate_aln(aln))) return rc;
    const uint64_t n = b->n_pairs;
    if (aln) {
        *aln->n_overflow = 0;
        aln->cigar_off[0] = 0;
    }
    if (n == 0) return MSW_OK;
    if (!b->reads || !b->read_len || !b->win_pos || !b->win_len) return fail(MSW_E_INVALID, "NULL array in batch");
    if (both && !strand) return fail(MSW_E_INVALID, "strand is NULL");
    if (aln) {
        if (!out || !out->score || !out->end_i || !out->end_j)
            return fail(MSW_E_INVALID, "traceback needs score / end_i / end_j");
    } else if (!out || !out->score || (coords && (!out->end_i || !out->end_j))) {
        return fail(MSW_E_INVALID, "NULL array in out");
    }
    if (n > 0x7FFFFFFFull) return fail(MSW_E_RANGE, "traceback: n_pairs > 2^31-1 in one call");
    uint32_t max_m = 0, max_n = 0;
    max_u16(b->read_len, n, max_m);
    max_u16(b->win_len, n, max_n);
    if (aln) {
        if ((rc = check_trace_bounds(max_m, max_n))) return rc;
    } else if ((rc = check_bounds(sch, max_m, max_n))) {
        return rc;
    }
    if (max_m > b->read_stride) return fail(MSW_E_INVALID, "a length exceeds its stride");
    if ((rc = set_device(ctx))) return rc;
    // Simple and synchronous, like msw_align_batch_trace: per chunk upload,
    // cut, score with coordinates, trace, pack, download.  The trace stride is
    // exact (no alignment has more ops than rows + columns), so no read
    // overflows; the packed ops of a chunk are pulled once its total is known.
    const uint64_t chunk = std::min<uint64_t>(n, chunk_pairs ? chunk_pairs : 65536);
    const size_t rs = b->read_stride, ws = std::max<size_t>(16, (max_n + 15u) & ~15u),
                 cs = aln ? (size_t)max_m + max_n : 0;
    auto up256 = [](size_t x) { return (x + 255) & ~(size_t)255; };
    // [reads | wins | rows u32 | pos i64 | ref i64 | score nc nm i32 | off u32 [c+1] + ovf | 7 x 2 B arrays]
    const size_t o_wins = up256(chunk * rs), o_rows = up256(o_wins + chunk * ws), o_pos = up256(o_rows + chunk * cs * 4);
    const size_t o_ref = o_pos + chunk * 8, o_score = o_ref + chunk * 8, o_nc = o_score + chunk * 4,
                 o_nm = o_nc + chunk * 4, o_off = o_nm + chunk * 4, o_h = o_off + (chunk + 2) * 4;
    const size_t total_bytes = o_h + chunk * 14 + 256;
    uint8_t* d = nullptr;
    hipError_t e = hipMalloc((void**)&d, total_bytes);
    if (e != hipSuccess) return fail(MSW_E_NOMEM, "hipMalloc(%zu B): %s", total_bytes, hipGetErrorString(e));
    uint32_t* d_ops = nullptr;  // the chunk's packed ops; grown to a chunk's total when it does not fit
    uint64_t ops_cap = aln ? chunk * 8 : 1;
    e = hipMalloc((void**)&d_ops, ops_cap * 4);
    if (e != hipSuccess) {
        (void)hipFree(d);
        return fail(MSW_E_NOMEM, "hipMalloc(%llu B): %s", (unsigned long long)ops_cap * 4, hipGetErrorString(e));
    }
    // both strands: the chunk's oriented rows [chunk][ors] and its strand bytes
    const size_t ors = std::max<size_t>(16, (max_m + 15u) & ~15u);
    uint8_t *d_or = nullptr, *d_strand = nullptr;
    if (both) {
        e = hipMalloc((void**)&d_or, chunk * ors + chunk + 16);
        if (e != hipSuccess) {
            (void)hipFree(d);
            (void)hipFree(d_ops);
            return fail(MSW_E_NOMEM, "hipMalloc(%zu B): %s", chunk * ors + chunk, hipGetErrorString(e));
        }
        d_strand = d_or + chunk * ors;
    }
    uint16_t* d_rl = reinterpret_cast<uint16_t*>(d + o_h);
    uint16_t *d_want = d_rl + chunk, *d_wl = d_want + chunk;
    int16_t *d_ei = reinterpret_cast<int16_t*>(d_wl + chunk), *d_ej = d_ei + chunk, *d_si = d_ej + chunk,
            *d_sj = d_si + chunk;
    int64_t *d_pos = reinterpret_cast<int64_t*>(d + o_pos), *d_ref = reinterpret_cast<int64_t*>(d + o_ref);
    uint32_t* d_off = reinterpret_cast<uint32_t*>(d + o_off);
    hipStream_t st = ctx->compute;
    std::vector<uint32_t> off(chunk + 1);
    uint64_t base = 0;  // ops of the chunks before this one
    rc = MSW_OK;
    for (uint64_t lo = 0; lo < n && rc == MSW_OK && e == hipSuccess; lo += chunk) {
        const uint64_t c = std::min(chunk, n - lo);
        uint32_t cm = 0, cn = 0;
        max_u16(b->read_len + lo, c, cm);
        max_u16(b->win_len + lo, c, cn);
        auto up = [&](void* dst, const void* src, size_t bytes) {
            if (e == hipSuccess && bytes) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st);
        };
        auto down = [&](void* dst, const void* src, size_t bytes) {
            if (e == hipSuccess && bytes) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st);
        };
        up(d, b->reads + lo * rs, c * rs);
        up(d_rl, b->read_len + lo, c * 2);
        up(d_want, b->win_len + lo, c * 2);
        up(d_pos, b->win_pos + lo, c * 8);
        if (e != hipSuccess) break;
        if ((rc = msw_genome_cut_device(ctx, g, d_pos, d_want, c, d + o_wins, (uint32_t)ws, d_wl, st))) break;
        msw_batch_t db = {d, d + o_wins, d_rl, d_wl, (uint32_t)rs, (uint32_t)ws, c};
        msw_out_t dout = {reinterpret_cast<int32_t*>(d + o_score), d_ei, d_ej};
        msw_trace_t dtr = {d_si, d_sj, reinterpret_cast<int32_t*>(d + o_nc), reinterpret_cast<uint32_t*>(d + o_rows),
                           (uint32_t)cs};
        if (both) {
            rc = score_both_strands(ctx, &scc, &db, &dout, d_strand, d_or, (uint32_t)ors, st,
                                    [&](const msw_batch_t* pb, msw_out_t* po) {
                                        return msw_align_batch_device(ctx, &scc, pb, po, cm, cn, st);
                                    });
            if (rc) break;
            down(strand + lo, d_strand, c);
            // from here on the reads are the oriented rows
            db.reads = d_or;
            db.read_stride = (uint32_t)ors;
            if (!aln) {
                down(out->score + lo, dout.score, c * 4);
                if (coords) {
                    down(out->end_i + lo, d_ei, c * 2);
                    down(out->end_j + lo, d_ej, c * 2);
                }
                if (e == hipSuccess) e = hipStreamSynchronize(st);
                continue;
            }
        } else if ((rc = msw_align_batch_device(ctx, &scc, &db, &dout, cm, cn, st))) {
            break;
        }
        if ((rc = msw_trace_batch_device(ctx, &scc, &db, &dout, &dtr, cm, cn, st))) break;
        uint64_t total = 0;
        for (int pass = 0; pass < 2; ++pass) {
            msw_aln_t da = {d_ref, reinterpret_cast<int32_t*>(d + o_nm), d_off, d_ops, ops_cap, d_off + c + 1};
            if ((rc = msw_aln_pack_device(ctx, g, db.reads, d_rl, db.read_stride, d_pos, c, &dout, &dtr, &da, st)))
                break;
            down(off.data(), d_off, (c + 1) * 4);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e != hipSuccess) break;
            total = off[c];
            if (total <= ops_cap) break;
            (void)hipFree(d_ops);
            d_ops = nullptr;
            ops_cap = total;
            e = hipMalloc((void**)&d_ops, ops_cap * 4);
        }
        if (rc || e != hipSuccess) break;
        down(out->score + lo, dout.score, c * 4);
        down(out->end_i + lo, d_ei, c * 2);
        down(out->end_j + lo, d_ej, c * 2);
        down(aln->ref_pos + lo, d_ref, c * 8);
        down(aln->nm + lo, d + o_nm, c * 4);
        const uint64_t room = aln->cigar_cap > base ? aln->cigar_cap - base : 0;
        down(aln->cigar + base, d_ops, std::min(total, room) * 4);
        // one prefix sum over the whole batch: this chunk's offsets start at `base`
        for (uint64_t k = 0; k <= c; ++k) aln->cigar_off[lo + k] = (uint32_t)(base + off[k]);
        base += total;
        if (e == hipSuccess) e = hipStreamSynchronize(st);
    }
    if (e != hipSuccess) (void)hipStreamSynchronize(st);
    (void)hipFree(d);
    if (d_ops) (void)hipFree(d_ops);
    if (d_or) (void)hipFree(d_or);
    if (rc) return rc;
    if (e != hipSuccess) return fail(MSW_E_DEVICE, "alignment records: %s", hipGetErrorString(e));
    return MSW_OK;
}

int msw_align_reads_trace(msw_ctx* ctx, const msw_scoring_t* sc, const msw_genome* g, const msw_read_batch_t* b,
                          msw_out_t* out, msw_aln_t* aln, uint64_t chunk_pairs) {
    return reads_records(ctx, sc, g, b, out, aln, nullptr, false, chunk_pairs);
}

int msw_align_reads_strands(msw_ctx* ctx, const msw_scoring_t* sc, const msw_genome* g, const msw_read_batch_t* b,
                            msw_out_t* out, uint8_t* strand, msw_aln_t* aln, uint64_t chunk_pairs) {
    return reads_records(ctx, sc, g, b, out, aln, strand, true, chunk_pairs);
}

// Placing reads (include/msw.h, "Placing reads"; the kernels: msw_seed.hip).
int msw_index_create(msw_ctx* ctx, const msw_genome* g, uint32_t k, uint32_t max_occ, msw_index** out) {
    if (!ctx || !out) return fail(MSW_E_INVALID, "ctx/out is NULL");
    *out = nullptr;
    if (!g) return fail(MSW_E_INVALID, "genome is NULL");
    if (g->ctx != ctx) return fail(MSW_E_INVALID, "genome belongs to another context");
    if (k < 4 || k > 14) return fail(MSW_E_RANGE, "index: k %u outside [4, 14]", k);
    if (max_occ < 1 || max_occ > msw::kSeedMaxOcc)
        return fail(MSW_E_RANGE, "index: max_occ %u outside [1, %u]", max_occ, msw::kSeedMaxOcc);
    if (g->len > msw::kSeedMaxGenome)
        return fail(MSW_E_RANGE, "index: genome of %llu bases > %llu", (unsigned long long)g->len,
                    (unsigned long long)msw::kSeedMaxGenome);
    int rc = set_device(ctx);
    if (rc) return rc;
    msw_index* x = new msw_index();
    x->ctx = ctx;
    x->device = ctx->device;
    x->k = k;
    x->max_occ = max_occ;
    x->buckets = 1ull << (2 * k);
    // plain hipMalloc for the temporaries: a one-off, synchronous build
    uint32_t *tmp = nullptr, *cursor = nullptr, *d_masked = nullptr;
    hipEvent_t ev[7] = {};
    hipStream_t st = ctx->compute;
    const uint64_t tmp_words = msw::index_scan_tmp_words(x->buckets);
    uint32_t h_masked = 0, total = 0;
    int err = MSW_OK;
    hipError_t e = hipMalloc((void**)&x->d_off, (x->buckets + 1) * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void**)&tmp, (tmp_words + 1) * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void**)&d_masked, sizeof(uint32_t));
    if (e != hipSuccess) err = fail(MSW_E_NOMEM, "index: hipMalloc for 4^%u buckets: %s", k, hipGetErrorString(e));
    for (int i = 0; i < 7 && e == hipSuccess; ++i) e = hipEventCreate(&ev[i]);
    if (e == hipSuccess)
        e = msw::launch_index_count(g->d_seq, g->len, k, max_occ, x->d_off, d_masked, tmp, ev, st);
    if (e == hipSuccess) e = hipMemcpyAsync(&total, x->d_off + x->buckets, 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(&h_masked, d_masked, 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) {
        x->n_pos = total;
        x->n_masked = h_masked;
        e = hipMalloc((void**)&x->d_pos, std::max<uint64_t>(total, 1) * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMalloc((void**)&cursor, x->buckets * sizeof(uint32_t));
        if (e != hipSuccess)
            err = fail(MSW_E_NOMEM, "index: hipMalloc for %u positions: %s", total, hipGetErrorString(e));
    }
    if (e == hipSuccess) e = msw::launch_index_fill(g->d_seq, g->len, k, x->d_off, cursor, x->d_pos, ev + 4, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) {
        // ev: [count | mask | scan |] then [fill | sort |]
        const int a[5] = {0, 1, 2, 4, 5};
        for (int i = 0; i < 5; ++i) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, ev[a[i]], ev[a[i] + 1]) == hipSuccess) x->build_ms[i] = ms;
        }
    } else {
        (void)hipStreamSynchronize(st);
    }
    for (hipEvent_t v : ev)
        if (v) (void)hipEventDestroy(v);
    (void)hipFree(tmp);
    (void)hipFree(cursor);
    (void)hipFree(d_masked);
    if (e != hipSuccess) {
        msw_index_destroy(x);
        return err ? err : fail(MSW_E_DEVICE, "index build: %s", hipGetErrorString(e));
    }
    *out = x;
    return MSW_OK;
}

void msw_index_destroy(msw_index* x) {
    if (!x) return;
    (void)hipSetDevice(x->device);
    if (x->d_off) (void)hipFree(x->d_off);
    if (x->d_pos) (void)hipFree(x->d_pos);
    delete x;
}

int msw_index_info(const msw_index* x, msw_index_info_t* out) {
    if (!x || !out) return fail(MSW_E_INVALID, "index/out is NULL");
    out->k = x->k;
    out->max_occ = x->max_occ;
    out->n_buckets = x->buckets;
    out->n_pos = x->n_pos;
    out->n_masked = x->n_masked;
    out->off = x->d_off;
    out->pos = x->d_pos;
    for (int i = 0; i < 5; ++i) out->build_ms[i] = x->build_ms[i];
    return MSW_OK;
}

static int check_seed_params(const msw_seed_params_t* sp, uint32_t max_read_len) {
    if (!sp) return fail(MSW_E_INVALID, "seed params is NULL");
    if (sp->band < 1) return fail(MSW_E_RANGE, "seed: band must be >= 1");
    if (sp->cap < 1 || sp->cap > msw::kSeedMaxCap)
        return fail(MSW_E_RANGE, "seed: cap %u outside [1, %u]", sp->cap, msw::kSeedMaxCap);
    if (sp->step < 1) return fail(MSW_E_RANGE, "seed: step must be >= 1");
    if (sp->min_votes < 1) return fail(MSW_E_RANGE, "seed: min_votes must be >= 1");
    if (sp->window > (uint32_t)msw::kMaxLongLen)
        return fail(MSW_E_RANGE, "seed: window %u > %d", sp->window, msw::kMaxLongLen);
    if (max_read_len > (uint32_t)msw::kMaxLongLen)
        return fail(MSW_E_RANGE, "seed: max_read_len %u > %d", max_read_len, msw::kMaxLongLen);
    return MSW_OK;
}

// The checks of the device seeding calls and the kernel's parameters; *go is
// false where the call has nothing to launch (n == 0).
static int seed_device_params(msw_ctx* ctx, const msw_index* x, const uint8_t* reads, const uint8_t* rc_reads,
                              const uint16_t* read_len, uint32_t read_stride, uint32_t rc_stride, uint64_t n,
                              uint32_t max_read_len, const msw_seed_params_t* sp, const msw_seed_out_t* out,
                              msw::SeedParams* pp, bool* go) {
    msw::SeedParams& p = *pp;
    *go = false;
    if (!ctx || !x) return fail(MSW_E_INVALID, "ctx/index is NULL");
    if (x->ctx != ctx) return fail(MSW_E_INVALID, "index belongs to another context");
    int rc;
    if ((rc = check_seed_params(sp, max_read_len))) return rc;
    if (n == 0) return MSW_OK;
    if (!reads || !read_len || !out || !out->win_pos || !out->votes || !out->hits || !out->flags)
        return fail(MSW_E_INVALID, "NULL array");
    if (read_stride == 0 || max_read_len > read_stride) return fail(MSW_E_INVALID, "max_read_len exceeds read_stride");
    if (rc_reads && (rc_stride == 0 || max_read_len > rc_stride))
        return fail(MSW_E_INVALID, "max_read_len exceeds rc_stride");
    if ((rc = set_device(ctx))) return rc;
    p.off = x->d_off;
    p.pos = x->d_pos;
    p.reads = reads;
    p.rc_reads = rc_reads;
    p.read_len = read_len;
    p.read_stride = read_stride;
    p.rc_stride = rc_stride;
    p.n = n;
    p.k = x->k;
    p.band = sp->band;
    p.cap = sp->cap;
    p.step = sp->step;
    p.min_votes = sp->min_votes;
    p.window = sp->window;
    p.win_pos = out->win_pos;
    p.votes = out->votes;
    p.hits = out->hits;
    p.flags = out->flags;
    *go = true;
    return MSW_OK;
}

int msw_seed_reads_device(msw_ctx* ctx, const msw_index* x, const uint8_t* reads, const uint8_t* rc_reads,
                          const uint16_t* read_len, uint32_t read_stride, uint32_t rc_stride, uint64_t n,
                          uint32_t max_read_len, const msw_seed_params_t* sp, const msw_seed_out_t* out, void* stream) {
    msw::SeedParams p;
    bool go;
    int rc = seed_device_params(ctx, x, reads, rc_reads, read_len, read_stride, rc_stride, n, max_read_len, sp, out, &p,
                                &go);
    if (rc || !go) return rc;
    HIP_TRY(msw::launch_seed_reads(p, call_stream(ctx, stream)));
    return MSW_OK;
}

int msw_seed_reads(msw_ctx* ctx, const msw_index* x, const msw_read_batch_t* b, int both,
                   const msw_seed_params_t* sp, const msw_seed_out_t* out, uint64_t chunk_reads) {
    if (!ctx || !x) return fail(MSW_E_INVALID, "ctx/index is NULL");
    if (x->ctx != ctx) return fail(MSW_E_INVALID, "index belongs to another context");
    if (!b) return fail(MSW_E_INVALID, "batch is NULL");
    const uint64_t n = b->n_pairs;
    uint32_t max_m = 0;
    if (n && !b->read_len) return fail(MSW_E_INVALID, "NULL array");
    max_u16(b->read_len, n, max_m);
    int rc;
    if ((rc = check_seed_params(sp, max_m))) return rc;
    if (n == 0) return MSW_OK;
    if (!b->reads || !out || !out->win_pos || !out->votes || !out->hits || !out->flags)
        return fail(MSW_E_INVALID, "NULL array");
    if (b->read_stride == 0 || max_m > b->read_stride) return fail(MSW_E_INVALID, "a length exceeds its stride");
    if ((rc = set_device(ctx))) return rc;
    // Simple and synchronous, like msw_align_batch_trace: per chunk upload,
    // reverse complement, seed, download.
    const uint64_t chunk = std::min<uint64_t>(n, chunk_reads ? chunk_reads : 65536);
    const size_t rs = b->read_stride, os = round16((uint32_t)std::max<uint32_t>(max_m, 1));
    // [reads | rc rows | win_pos i64 | votes u32 | hits u32 | read_len u16 | flags u8]
    const size_t o_rc = (chunk * rs + 255) & ~(size_t)255, o_wp = (o_rc + (both ? chunk * os : 0) + 255) & ~(size_t)255;
    const size_t o_votes = o_wp + chunk * 8, o_hits = o_votes + chunk * 4, o_rl = o_hits + chunk * 4,
                 o_fl = o_rl + chunk * 2;
    uint8_t* d = nullptr;
    hipError_t e = hipMalloc((void**)&d, o_fl + chunk + 256);
    if (e != hipSuccess) return fail(MSW_E_NOMEM, "hipMalloc(%zu B): %s", o_fl + chunk, hipGetErrorString(e));
    hipStream_t st = ctx->compute;
    rc = MSW_OK;
    for (uint64_t lo = 0; lo < n && rc == MSW_OK; lo += chunk) {
        const uint64_t c = std::min(chunk, n - lo);
        uint16_t* d_rl = reinterpret_cast<uint16_t*>(d + o_rl);
        msw_seed_out_t dout = {reinterpret_cast<int64_t*>(d + o_wp), reinterpret_cast<uint32_t*>(d + o_votes),
                               reinterpret_cast<uint32_t*>(d + o_hits), d + o_fl};
        e = hipMemcpyAsync(d, b->reads + lo * rs, c * rs, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(d_rl, b->read_len + lo, c * 2, hipMemcpyHostToDevice, st);
        if (e != hipSuccess) break;
        if (both && (rc = msw_revcomp_device(ctx, d, d_rl, (uint32_t)rs, c, d + o_rc, (uint32_t)os, st))) break;
        if ((rc = msw_seed_reads_device(ctx, x, d, both ? d + o_rc : nullptr, d_rl, (uint32_t)rs, (uint32_t)os, c, max_m,
                                        sp, &dout, st)))
            break;
        e = hipMemcpyAsync(out->win_pos + lo, dout.win_pos, c * 8, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(out->votes + lo, dout.votes, c * 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(out->hits + lo, dout.hits, c * 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(out->flags + lo, dout.flags, c, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) break;
    }
    if (e != hipSuccess || rc) (void)hipStreamSynchronize(st);
    (void)hipFree(d);
    if (rc) return rc;
    if (e != hipSuccess) return fail(MSW_E_DEVICE, "seeding: %s", hipGetErrorString(e));
    return MSW_OK;
}

// Candidates and mapping quality (include/msw.h; the kernels: msw_seed.hip,
// msw_mapq.hip).
int msw_seed_candidates_device(msw_ctx* ctx, const msw_index* x, const uint8_t* reads, const uint8_t* rc_reads,
                               const uint16_t* read_len, uint32_t read_stride, uint32_t rc_stride, uint64_t n,
                               uint32_t max_read_len, const msw_seed_params_t* sp, uint32_t sep,
                               const msw_seed_out_t* out, const msw_seed_alt_t* alt, void* stream) {
    msw::SeedCandParams q;
    bool go;
    int rc = seed_device_params(ctx, x, reads, rc_reads, read_len, read_stride, rc_stride, n, max_read_len, sp, out,
                                &q.s, &go);
    if (rc) return rc;
    if (sep != 0 && sep < sp->band) return fail(MSW_E_RANGE, "candidates: sep %u is below band %u", sep, sp->band);
    if (!go) return MSW_OK;
    if (!alt || !alt->win_pos || !alt->votes || !alt->flags) return fail(MSW_E_INVALID, "NULL array in alt");
    q.sep = sep;
    q.win_pos1 = alt->win_pos;
    q.votes1 = alt->votes;
    q.flags1 = alt->flags;
    HIP_TRY(msw::launch_seed_candidates(q, call_stream(ctx, stream)));
    return MSW_OK;
}

int msw_seed_candidates(msw_ctx* ctx, const msw_index* x, const msw_read_batch_t* b, int both,
                        const msw_seed_params_t* sp, uint32_t sep, const msw_seed_out_t* out,
                        const msw_seed_alt_t* alt, uint64_t chunk_reads) {
    if (!ctx || !x) return fail(MSW_E_INVALID, "ctx/index is NULL");
    if (x->ctx != ctx) return fail(MSW_E_INVALID, "index belongs to another context");
    if (!b) return fail(MSW_E_INVALID, "batch is NULL");
    const uint64_t n = b->n_pairs;
    uint32_t max_m = 0;
    if (n && !b->read_len) return fail(MSW_E_INVALID, "NULL array");
    max_u16(b->read_len, n, max_m);
    int rc;
    if ((rc = check_seed_params(sp, max_m))) return rc;
    if (sep != 0 && sep < sp->band) return fail(MSW_E_RANGE, "candidates: sep %u is below band %u", sep, sp->band);
    if (n == 0) return MSW_OK;
    if (!b->reads || !out || !out->win_pos || !out->votes || !out->hits || !out->flags || !alt || !alt->win_pos ||
        !alt->votes || !alt->flags)
        return fail(MSW_E_INVALID, "NULL array");
    if (b->read_stride == 0 || max_m > b->read_stride) return fail(MSW_E_INVALID, "a length exceeds its stride");
    if ((rc = set_device(ctx))) return rc;
    const uint64_t chunk = std::min<uint64_t>(n, chunk_reads ? chunk_reads : 65536);
    const size_t rs = b->read_stride, os = round16((uint32_t)std::max<uint32_t>(max_m, 1));
    // [reads | rc rows | win_pos, win_pos1 i64 | votes, hits, votes1 u32 | read_len u16 | flags, flags1 u8]
    const size_t o_rc = (chunk * rs + 255) & ~(size_t)255, o_wp = (o_rc + (both ? chunk * os : 0) + 255) & ~(size_t)255;
    const size_t o_wp1 = o_wp + chunk * 8, o_votes = o_wp1 + chunk * 8, o_hits = o_votes + chunk * 4,
                 o_votes1 = o_hits + chunk * 4, o_rl = o_votes1 + chunk * 4, o_fl = o_rl + chunk * 2,
                 o_fl1 = o_fl + chunk;
    uint8_t* d = nullptr;
    hipError_t e = hipMalloc((void**)&d, o_fl1 + chunk + 256);
    if (e != hipSuccess) return fail(MSW_E_NOMEM, "hipMalloc(%zu B): %s", o_fl1 + chunk, hipGetErrorString(e));
    hipStream_t st = ctx->compute;
    rc = MSW_OK;
    for (uint64_t lo = 0; lo < n && rc == MSW_OK; lo += chunk) {
        const uint64_t c = std::min(chunk, n - lo);
        uint16_t* d_rl = reinterpret_cast<uint16_t*>(d + o_rl);
        msw_seed_out_t dout = {reinterpret_cast<int64_t*>(d + o_wp), reinterpret_cast<uint32_t*>(d + o_votes),
                               reinterpret_cast<uint32_t*>(d + o_hits), d + o_fl};
        msw_seed_alt_t dalt = {reinterpret_cast<int64_t*>(d + o_wp1), reinterpret_cast<uint32_t*>(d + o_votes1),
                               d + o_fl1};
        e = hipMemcpyAsync(d, b->reads + lo * rs, c * rs, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(d_rl, b->read_len + lo, c * 2, hipMemcpyHostToDevice, st);
        if (e != hipSuccess) break;
        if (both && (rc = msw_revcomp_device(ctx, d, d_rl, (uint32_t)rs, c, d + o_rc, (uint32_t)os, st))) break;
        if ((rc = msw_seed_candidates_device(ctx, x, d, both ? d + o_rc : nullptr, d_rl, (uint32_t)rs, (uint32_t)os, c,
                                             max_m, sp, sep, &dout, &dalt, st)))
            break;
        auto down = [&](void* dst, const void* src, size_t bytes) {
            if (e == hipSuccess) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st);
        };
        down(out->win_pos + lo, dout.win_pos, c * 8);
        down(out->votes + lo, dout.votes, c * 4);
        down(out->hits + lo, dout.hits, c * 4);
        down(out->flags + lo, dout.flags, c);
        down(alt->win_pos + lo, dalt.win_pos, c * 8);
        down(alt->votes + lo, dalt.votes, c * 4);
        down(alt->flags + lo, dalt.flags, c);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) break;
    }
    if (e != hipSuccess || rc) (void)hipStreamSynchronize(st);
    (void)hipFree(d);
    if (rc) return rc;
    if (e != hipSuccess) return fail(MSW_E_DEVICE, "candidates: %s", hipGetErrorString(e));
    return MSW_OK;
}

int msw_mapq_select_device(msw_ctx* ctx, const msw_cand_t* pr, const msw_cand_t* al, uint32_t oriented_stride,
                           const uint16_t* read_len, uint64_t n, int32_t match, int32_t* sub_score, uint8_t* mapq,
                           uint8_t* cand, void* stream) {
    if (!ctx) return fail(MSW_E_INVALID, "ctx is NULL");
    if (match < 0 || match > 64) return fail(MSW_E_RANGE, "mapq select: match=%d outside [0, 64]", match);
    if (n == 0) return MSW_OK;
    if (!pr || !al || !pr->score || !al->score || !pr->win_pos || !al->win_pos || !read_len || !sub_score || !mapq ||
        !cand)
        return fail(MSW_E_INVALID, "NULL array");
    const bool coords = pr->end_i || pr->end_j || al->end_i || al->end_j;
    if (coords && (!pr->end_i || !pr->end_j || !al->end_i || !al->end_j))
        return fail(MSW_E_INVALID, "end_i / end_j must be given for both candidates or for neither");
    const bool rows = pr->strand || pr->oriented || al->strand || al->oriented;
    if (rows && (!pr->strand || !pr->oriented || !al->strand || !al->oriented))
        return fail(MSW_E_INVALID, "strand / oriented must be given for both candidates or for neither");
    if ((pr->win_len != nullptr) != (al->win_len != nullptr))
        return fail(MSW_E_INVALID, "win_len must be given for both candidates or for neither");
    if (rows && (((uintptr_t)pr->oriented & 15) != 0 || ((uintptr_t)al->oriented & 15) != 0 || oriented_stride == 0 ||
                 oriented_stride % 16 != 0))
        return fail(MSW_E_INVALID, "oriented must be 16-byte aligned and oriented_stride a non-zero multiple of 16");
    if (n > 0x7FFFFFFFull) return fail(MSW_E_RANGE, "mapq select: too many reads in one call");
    int rc = set_device(ctx);
    if (rc) return rc;
    msw::MapqSelectParams p;
    p.score = pr->score, p.end_i = pr->end_i, p.end_j = pr->end_j, p.win_len = pr->win_len, p.strand = pr->strand;
    p.oriented = pr->oriented, p.win_pos = pr->win_pos;
    p.score_a = al->score, p.end_i_a = al->end_i, p.end_j_a = al->end_j, p.win_len_a = al->win_len;
    p.strand_a = al->strand, p.oriented_a = al->oriented, p.win_pos_a = al->win_pos;
    p.read_len = read_len;
    p.oriented_stride = oriented_stride;
    p.n = n;
    p.match = match;
    p.sub_score = sub_score, p.mapq = mapq, p.cand = cand;
    HIP_TRY(msw::launch_mapq_select(p, call_stream(ctx, stream)));
    return MSW_OK;
}

int msw_map_reads(msw_ctx* ctx, const msw_scoring_t* sc, const msw_genome* g, const msw_index* x,
                  const msw_read_batch_t* b, int both, const msw_seed_params_t* sp, uint32_t sep, msw_out_t* out,
                  uint8_t* strand, msw_aln_t* aln, const msw_mapq_t* mq, uint64_t chunk_pairs) {
    if (!ctx || !g || !x) return fail(MSW_E_INVALID, "ctx/genome/index is NULL");
    if (g->ctx != ctx) return fail(MSW_E_INVALID, "genome belongs to another context");
    if (x->ctx != ctx) return fail(MSW_E_INVALID, "index belongs to another context");
    if (!sc || !b) return fail(MSW_E_INVALID, "scoring/batch is NULL");
    msw_scoring_t scc = *sc;
    scc.want_coords = 1;
    Scheme sch;
    int rc;
    if ((rc = make_scheme(&scc, ctx->opt, &sch))) return rc;
    if ((rc = validate_aln(aln))) return rc;
    const uint64_t n = b->n_pairs;
    uint32_t max_m = 0;
    if (n && !b->read_len) return fail(MSW_E_INVALID, "NULL array in batch");
    max_u16(b->read_len, n, max_m);
    if ((rc = check_seed_params(sp, max_m))) return rc;
    if (sep != 0 && sep < sp->band) return fail(MSW_E_RANGE, "candidates: sep %u is below band %u", sep, sp->band);
    *aln->n_overflow = 0;
    aln->cigar_off[0] = 0;
    if (n == 0) return MSW_OK;
    if (!b->reads) return fail(MSW_E_INVALID, "NULL array in batch");
    if (both && !strand) return fail(MSW_E_INVALID, "strand is NULL");
    if (!out || !out->score || !out->end_i || !out->end_j)
        return fail(MSW_E_INVALID, "traceback needs score / end_i / end_j");
    if (!mq || !mq->mapq || !mq->sub_score || !mq->cand) return fail(MSW_E_INVALID, "NULL array in mapq");
    if (n > 0x7FFFFFFFull) return fail(MSW_E_RANGE, "traceback: n_pairs > 2^31-1 in one call");
    const uint32_t window = sp->window;
    const uint32_t max_n = window ? window : std::min<uint32_t>(2u * max_m, (uint32_t)msw::kMaxWinLen);
    if ((rc = check_trace_bounds(max_m, max_n))) return rc;
    if (b->read_stride == 0 || max_m > b->read_stride) return fail(MSW_E_INVALID, "a length exceeds its stride");
    if ((rc = set_device(ctx))) return rc;
    // Simple and synchronous, like msw_align_reads_trace.  Per chunk, all on
    // the compute stream: upload, (reverse complement,) candidates, the two
    // scoring calls, the selection, then trace and pack on the winner.
    const uint64_t chunk = std::min<uint64_t>(n, chunk_pairs ? chunk_pairs : 65536);
    const size_t rs = b->read_stride, ors = round16(std::max<uint32_t>(max_m, 1)), cs = (size_t)max_m + max_n;
    auto up256 = [](size_t v) { return (v + 255) & ~(size_t)255; };
    // [reads | rc rows | oriented 0 | oriented 1 | trace rows u32 | 3 x i64 | 8 x 4 B | off u32[c + 2] |
    //  9 x 2 B | 6 x 1 B]
    const size_t o_rc = up256(chunk * rs), o_or0 = up256(o_rc + (both ? chunk * ors : 0)),
                 o_or1 = up256(o_or0 + (both ? chunk * ors : 0)), o_rows = up256(o_or1 + (both ? chunk * ors : 0)),
                 o_q = up256(o_rows + chunk * cs * 4), o_w = o_q + chunk * 24, o_off = o_w + chunk * 32,
                 o_h = o_off + (chunk + 2) * 4, o_b = up256(o_h + chunk * 18);
    const size_t total_bytes = o_b + chunk * 6 + 256;
    uint8_t* d = nullptr;
    hipError_t e = hipMalloc((void**)&d, total_bytes);
    if (e != hipSuccess) return fail(MSW_E_NOMEM, "hipMalloc(%zu B): %s", total_bytes, hipGetErrorString(e));
    uint32_t* d_ops = nullptr;  // the chunk's packed ops; grown to a chunk's total when it does not fit
    uint64_t ops_cap = chunk * 8;
    e = hipMalloc((void**)&d_ops, ops_cap * 4);
    if (e != hipSuccess) {
        (void)hipFree(d);
        return fail(MSW_E_NOMEM, "hipMalloc(%llu B): %s", (unsigned long long)ops_cap * 4, hipGetErrorString(e));
    }
    int64_t *d_wp0 = reinterpret_cast<int64_t*>(d + o_q), *d_wp1 = d_wp0 + chunk, *d_ref = d_wp1 + chunk;
    int32_t* w32 = reinterpret_cast<int32_t*>(d + o_w);
    int32_t *d_s0 = w32, *d_s1 = w32 + chunk, *d_sub = w32 + 2 * chunk, *d_nc = w32 + 3 * chunk, *d_nm = w32 + 4 * chunk;
    uint32_t *d_votes = reinterpret_cast<uint32_t*>(w32 + 5 * chunk), *d_hits = d_votes + chunk,
             *d_votes1 = d_hits + chunk;
    uint32_t* d_off = reinterpret_cast<uint32_t*>(d + o_off);
    uint16_t* d_rl = reinterpret_cast<uint16_t*>(d + o_h);
    uint16_t *d_wl0 = d_rl + chunk, *d_wl1 = d_wl0 + chunk;
    int16_t *d_ei0 = reinterpret_cast<int16_t*>(d_wl1 + chunk), *d_ej0 = d_ei0 + chunk, *d_ei1 = d_ej0 + chunk,
            *d_ej1 = d_ei1 + chunk, *d_si = d_ej1 + chunk, *d_sj = d_si + chunk;
    uint8_t *d_fl = d + o_b, *d_fl1 = d_fl + chunk, *d_st0 = d_fl1 + chunk, *d_st1 = d_st0 + chunk,
            *d_mapq = d_st1 + chunk, *d_cand = d_mapq + chunk;
    uint8_t *d_rc = d + o_rc, *d_or0 = d + o_or0, *d_or1 = d + o_or1;
    hipStream_t st = ctx->compute;
    std::vector<uint32_t> off(chunk + 1);
    uint64_t base = 0;  // ops of the chunks before this one
    rc = MSW_OK;
    for (uint64_t lo = 0; lo < n && rc == MSW_OK && e == hipSuccess; lo += chunk) {
        const uint64_t c = std::min(chunk, n - lo);
        auto up = [&](void* dst, const void* src, size_t bytes) {
            if (e == hipSuccess && bytes) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st);
        };
        auto down = [&](void* dst, const void* src, size_t bytes) {
            if (e == hipSuccess && bytes) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st);
        };
        up(d, b->reads + lo * rs, c * rs);
        up(d_rl, b->read_len + lo, c * 2);
        if (e != hipSuccess) break;
        if (both && (rc = msw_revcomp_device(ctx, d, d_rl, (uint32_t)rs, c, d_rc, (uint32_t)ors, st))) break;
        const msw_seed_out_t so = {d_wp0, d_votes, d_hits, d_fl};
        const msw_seed_alt_t sa = {d_wp1, d_votes1, d_fl1};
        if ((rc = msw_seed_candidates_device(ctx, x, d, both ? d_rc : nullptr, d_rl, (uint32_t)rs, (uint32_t)ors, c,
                                             max_m, sp, sep, &so, &sa, st)))
            break;
        msw_out_t o0 = {d_s0, d_ei0, d_ej0}, o1 = {d_s1, d_ei1, d_ej1};
        if (both) {
            if ((rc = msw_align_reads_strands_device(ctx, &scc, g, d, d_rl, (uint32_t)rs, d_wp0, c, window, max_m, &o0,
                                                     d_wl0, d_st0, d_or0, (uint32_t)ors, st)) ||
                (rc = msw_align_reads_strands_device(ctx, &scc, g, d, d_rl, (uint32_t)rs, d_wp1, c, window, max_m, &o1,
                                                     d_wl1, d_st1, d_or1, (uint32_t)ors, st)))
                break;
        } else if ((rc = msw_align_reads_device(ctx, &scc, g, d, d_rl, (uint32_t)rs, d_wp0, c, window, max_m, &o0,
                                                d_wl0, st)) ||
                   (rc = msw_align_reads_device(ctx, &scc, g, d, d_rl, (uint32_t)rs, d_wp1, c, window, max_m, &o1,
                                                d_wl1, st))) {
            break;
        }
        const msw_cand_t c0 = {d_s0, d_ei0, d_ej0, d_wl0, both ? d_st0 : nullptr, both ? d_or0 : nullptr, d_wp0};
        const msw_cand_t c1 = {d_s1, d_ei1, d_ej1, d_wl1, both ? d_st1 : nullptr, both ? d_or1 : nullptr, d_wp1};
        if ((rc = msw_mapq_select_device(ctx, &c0, &c1, (uint32_t)ors, d_rl, c, scc.match, d_sub, d_mapq, d_cand, st)))
            break;
        // from here on the reads are the winner's oriented rows
        const uint8_t* rows = both ? d_or0 : d;
        const uint32_t rstride = both ? (uint32_t)ors : (uint32_t)rs;
        msw_trace_t dtr = {d_si, d_sj, d_nc, reinterpret_cast<uint32_t*>(d + o_rows), (uint32_t)cs};
        if ((rc = msw_trace_reads_device(ctx, &scc, g, rows, d_rl, rstride, d_wp0, c, window, max_m, &o0, &dtr, st)))
            break;
        uint64_t total = 0;
        for (int pass = 0; pass < 2; ++pass) {
            msw_aln_t da = {d_ref, d_nm, d_off, d_ops, ops_cap, d_off + c + 1};
            if ((rc = msw_aln_pack_device(ctx, g, rows, d_rl, rstride, d_wp0, c, &o0, &dtr, &da, st))) break;
            down(off.data(), d_off, (c + 1) * 4);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e != hipSuccess) break;
            total = off[c];
            if (total <= ops_cap) break;
            (void)hipFree(d_ops);
            d_ops = nullptr;
            ops_cap = total;
            if (hipMalloc((void**)&d_ops, ops_cap * 4) != hipSuccess) {
                d_ops = nullptr;
                rc = fail(MSW_E_NOMEM, "hipMalloc(%llu B) for the packed ops", (unsigned long long)ops_cap * 4);
                break;
            }
        }
        if (rc || e != hipSuccess) break;
        down(out->score + lo, d_s0, c * 4);
        down(out->end_i + lo, d_ei0, c * 2);
        down(out->end_j + lo, d_ej0, c * 2);
        if (both) down(strand + lo, d_st0, c);
        down(mq->mapq + lo, d_mapq, c);
        down(mq->sub_score + lo, d_sub, c * 4);
        down(mq->cand + lo, d_cand, c);
        down(aln->ref_pos + lo, d_ref, c * 8);
        down(aln->nm + lo, d_nm, c * 4);
        const uint64_t room = aln->cigar_cap > base ? aln->cigar_cap - base : 0;
        down(aln->cigar + base, d_ops, std::min(total, room) * 4);
        for (uint64_t k = 0; k <= c; ++k) aln->cigar_off[lo + k] = (uint32_t)(base + off[k]);
        base += total;
        if (e == hipSuccess) e = hipStreamSynchronize(st);
    }
    if (e != hipSuccess || rc) (void)hipStreamSynchronize(st);
    (void)hipFree(d);
    if (d_ops) (void)hipFree(d_ops);
    if (rc) return rc;
    if (e != hipSuccess) return fail(MSW_E_DEVICE, "map reads: %s", hipGetErrorString(e));
    return MSW_OK;
}

// Pileup (include/msw.h, "Pileup"; the kernels: msw_pileup.hip).
struct msw_pileup {
    const msw_ctx* ctx = nullptr;  // identity only
    int device = 0;
    // one allocation: counts [glen][8] | the read counters' slots + stats u64[4] + the low-quality column counter's
    // slots | d_all [glen + 1] | d_rev [glen + 1] | mism [glen] | the scan's block sums
    // and with MSW_PILEUP_QSUM: | qsum [glen][4] | d_q [glen + 1] | qmis [glen]
    uint8_t* d_state = nullptr;
    msw::PileupParams p{};         // the state's part; an add fills in its batch
    uint32_t flags = 0;
    msw::PileupQsum qs{};          // the state's part (d_q, qmis, qsum, lowq), with MSW_PILEUP_QSUM
    unsigned long long* d_stats = nullptr;
    unsigned long long* d_lowq = nullptr;  // PileupQual::lowq
    uint32_t* d_scan_tmp = nullptr;
    bool finished = false;
    hipEvent_t fin = nullptr;      // recorded behind the fold
};

static int check_pileup(const msw_ctx* ctx, const msw_pileup* pile) {
    if (!ctx || !pile) return fail(MSW_E_INVALID, "ctx/pileup is NULL");
    if (pile->ctx != ctx) return fail(MSW_E_INVALID, "pileup belongs to another context");
    return MSW_OK;
}

int msw_pileup_create(msw_ctx* ctx, const msw_genome* g, msw_pileup** out) {
    return msw_pileup_create_ex(ctx, g, 0, out);
}

int msw_pileup_create_ex(msw_ctx* ctx, const msw_genome* g, uint32_t flags, msw_pileup** out) {
    if (!ctx || !g || !out) return fail(MSW_E_INVALID, "ctx/genome/out is NULL");
    *out = nullptr;
    if (flags & ~MSW_PILEUP_QSUM) return fail(MSW_E_INVALID, "pileup create: unknown flag in 0x%x", flags);
    const bool qsum = (flags & MSW_PILEUP_QSUM) != 0;
    if (g->ctx != ctx) return fail(MSW_E_INVALID, "genome belongs to another context");
    int rc = set_device(ctx);
    if (rc) return rc;
    const uint64_t glen = g->len;
    auto up16 = [](uint64_t x) { return (x + 15) & ~(uint64_t)15; };
    const uint64_t read_words = (uint64_t)msw::kPileupReadSlots * 2 * msw::kPileupReadSlotWords;
    const uint64_t lowq_words = (uint64_t)msw::kPileupReadSlots * msw::kPileupReadSlotWords;
    const uint64_t o_reads = (glen * 32 + 127) & ~(uint64_t)127, o_all = o_reads + (read_words + 16 + lowq_words) * 8,
                   o_rev = o_all + up16((glen + 1) * 4),
                   o_mism = o_rev + up16((glen + 1) * 4), o_tmp = o_mism + up16(glen * 4),
                   o_qsum = o_tmp + up16(msw::pileup_scan_tmp_words(glen) * 4) + 16,
                   o_dq = o_qsum + (qsum ? glen * 16 : 0), o_qmis = o_dq + (qsum ? up16((glen + 1) * 4) : 0),
                   total = o_qmis + (qsum ? up16(glen * 4) + 16 : 0);
    msw_pileup* pile = new msw_pileup();
    pile->ctx = ctx;
    pile->flags = flags;
    pile->device = ctx->device;
    hipError_t e = hipMalloc((void**)&pile->d_state, total);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        delete pile;
        return fail(MSW_E_NOMEM, "hipMalloc(%llu B) for the pileup of %llu bases: %s", (unsigned long long)total,
                    (unsigned long long)glen, hipGetErrorString(e));
    }
    msw::PileupParams& p = pile->p;
    p.genome = g->d_seq;
    p.glen = glen;
    p.counts = reinterpret_cast<uint32_t*>(pile->d_state);
    const bool planes = ctx->opt.pileup_planes;
    p.pos_mul = planes ? 1 : 8;
    p.ch_mul = planes ? glen : 1;
    p.reads = reinterpret_cast<unsigned long long*>(pile->d_state + o_reads);
    pile->d_stats = p.reads + read_words;
    pile->d_lowq = pile->d_stats + 16;
    p.d_all = reinterpret_cast<uint32_t*>(pile->d_state + o_all);
    p.d_rev = reinterpret_cast<uint32_t*>(pile->d_state + o_rev);
    p.mism = reinterpret_cast<uint32_t*>(pile->d_state + o_mism);
    pile->d_scan_tmp = reinterpret_cast<uint32_t*>(pile->d_state + o_tmp);
    if (qsum) {
        pile->qs.lowq = pile->d_lowq;
        pile->qs.qsum = reinterpret_cast<uint32_t*>(pile->d_state + o_qsum);
        pile->qs.d_q = reinterpret_cast<uint32_t*>(pile->d_state + o_dq);
        pile->qs.qmis = reinterpret_cast<uint32_t*>(pile->d_state + o_qmis);
    }
    // the kernels' code object, loaded here rather than inside the first add (HIP loads a module on first use)
    (void)msw::pileup_blocks_per_cu();
    e = hipEventCreateWithFlags(&pile->fin, hipEventDisableTiming);
    if (e == hipSuccess) e = hipMemsetAsync(pile->d_state, 0, total, ctx->compute);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->compute);
    if (e != hipSuccess) {
        msw_pileup_destroy(pile);
        return fail(MSW_E_DEVICE, "pileup state: %s", hipGetErrorString(e));
    }
    *out = pile;
    return MSW_OK;
}

void msw_pileup_destroy(msw_pileup* pile) {
    if (!pile) return;
    (void)hipSetDevice(pile->device);
    if (pile->fin) (void)hipEventDestroy(pile->fin);
    if (pile->d_state) (void)hipFree(pile->d_state);
    delete pile;
}

// a MSW_PILEUP_QSUM pileup takes no add without qualities
static int check_pileup_qsum_add(const msw_ctx* ctx, const msw_pileup* pile, const uint8_t* quals) {
    if (ctx && pile && pile->ctx == ctx && (pile->flags & MSW_PILEUP_QSUM) && !quals)
        return fail(MSW_E_INVALID, "pileup add: a MSW_PILEUP_QSUM pileup needs quals (msw_pileup_add_qual*)");
    return MSW_OK;
}

// the checks both add forms share; *go = false: nothing to do
static int check_pileup_add(msw_ctx* ctx, msw_pileup* pile, const uint8_t* rows, const uint16_t* read_len,
                            uint32_t row_stride, uint64_t n, const msw_aln_t* aln, uint32_t min_mapq, bool* go) {
    *go = false;
    int rc;
    if ((rc = check_pileup(ctx, pile))) return rc;
    if (!aln) return fail(MSW_E_INVALID, "aln is NULL");
    if (pile->finished) return fail(MSW_E_INVALID, "pileup is finished: it takes no more reads");
    if (n > 0x7FFFFFFFull) return fail(MSW_E_RANGE, "pileup add: n > 2^31-1 in one call");
    if (min_mapq > 255u) return fail(MSW_E_RANGE, "pileup add: min_mapq %u > 255", min_mapq);
    if (n == 0) return MSW_OK;
    if (!rows || !read_len) return fail(MSW_E_INVALID, "NULL array");
    if (row_stride == 0) return fail(MSW_E_INVALID, "row_stride is 0");
    if (!aln->ref_pos || !aln->nm || !aln->cigar_off) return fail(MSW_E_INVALID, "NULL array in aln");
    if (aln->cigar_cap && !aln->cigar) return fail(MSW_E_INVALID, "cigar is NULL with cigar_cap > 0");
    *go = true;
    return MSW_OK;
}

int msw_pileup_add_device(msw_ctx* ctx, msw_pileup* pile, const uint8_t* rows, const uint16_t* read_len,
                          uint32_t row_stride, uint64_t n, const msw_aln_t* aln, const uint8_t* strand,
                          const uint8_t* mapq, uint32_t min_mapq, void* stream) {
    return msw_pileup_add_qual_device(ctx, pile, rows, read_len, row_stride, n, aln, strand, mapq, min_mapq, nullptr, 0,
                                      0, stream);
}

int msw_pileup_add_qual_device(msw_ctx* ctx, msw_pileup* pile, const uint8_t* rows, const uint16_t* read_len,
                               uint32_t row_stride, uint64_t n, const msw_aln_t* aln, const uint8_t* strand,
                               const uint8_t* mapq, uint32_t min_mapq, const uint8_t* quals, uint32_t qual_stride,
                               uint32_t min_baseq, void* stream) {
    if (min_baseq > 93u) return fail(MSW_E_RANGE, "pileup add: min_baseq %u > 93", min_baseq);
    int rc;
    bool go;
    if ((rc = check_pileup_qsum_add(ctx, pile, quals))) return rc;
    if ((rc = check_pileup_add(ctx, pile, rows, read_len, row_stride, n, aln, min_mapq, &go)) || !go) return rc;
    if ((rc = set_device(ctx))) return rc;
    msw::PileupParams p = pile->p;
    p.rows = rows;
    p.read_len = read_len;
    p.row_stride = row_stride;
    p.n = n;
    p.ref_pos = aln->ref_pos;
    p.nm = aln->nm;
    p.cigar_off = aln->cigar_off;
    p.cigar = aln->cigar;
    p.cigar_cap = aln->cigar_cap;
    p.strand = strand;
    p.mapq = mapq;
    p.min_mapq = min_mapq;
    if (pile->flags & MSW_PILEUP_QSUM) {
        msw::PileupQsum q = pile->qs;
        q.quals = quals;
        q.qual_stride = qual_stride;
        q.min_baseq = min_baseq;
        HIP_TRY(msw::launch_pileup_add_qsum(p, q, call_stream(ctx, stream)));
    } else if (quals && min_baseq) {  // else the plain add
        const msw::PileupQual q{quals, qual_stride, min_baseq, pile->d_lowq};
        HIP_TRY(msw::launch_pileup_add_qual(p, q, call_stream(ctx, stream)));
    } else {
        HIP_TRY(msw::launch_pileup_add(p, call_stream(ctx, stream)));
    }
    return MSW_OK;
}

int msw_pileup_add(msw_ctx* ctx, msw_pileup* pile, const uint8_t* reads, const uint16_t* read_len, uint32_t read_stride,
                   uint64_t n, const msw_aln_t* aln, const uint8_t* strand, const uint8_t* mapq, uint32_t min_mapq,
                   uint64_t chunk_reads) {
    return msw_pileup_add_qual(ctx, pile, reads, read_len, read_stride, n, aln, strand, mapq, min_mapq, nullptr, 0, 0,
                               chunk_reads);
}

int msw_pileup_add_qual(msw_ctx* ctx, msw_pileup* pile, const uint8_t* reads, const uint16_t* read_len,
                        uint32_t read_stride, uint64_t n, const msw_aln_t* aln, const uint8_t* strand,
                        const uint8_t* mapq, uint32_t min_mapq, const uint8_t* quals, uint32_t qual_stride,
                        uint32_t min_baseq, uint64_t chunk_reads) {
    if (min_baseq > 93u) return fail(MSW_E_RANGE, "pileup add: min_baseq %u > 93", min_baseq);
    int rc;
    bool go;
    if ((rc = check_pileup_qsum_add(ctx, pile, quals))) return rc;
    const bool qsum = ctx && pile && pile->ctx == ctx && (pile->flags & MSW_PILEUP_QSUM);
    if (min_baseq == 0 && !qsum) quals = nullptr;  // the plain add
    if (!quals) qual_stride = 0;
    if ((rc = check_pileup_add(ctx, pile, reads, read_len, read_stride, n, aln, min_mapq, &go)) || !go) return rc;
    const uint64_t chunk = std::min<uint64_t>(n, chunk_reads ? chunk_reads : 65536);
    // the offsets decide what is uploaded: they must be a prefix sum inside the capacity
    uint64_t max_ops = 0;
    for (uint64_t lo = 0; lo < n; lo += chunk) {
        const uint64_t hi = std::min(n, lo + chunk);
        for (uint64_t k = lo; k < hi; ++k)
            if (aln->cigar_off[k + 1] < aln->cigar_off[k])
                return fail(MSW_E_INVALID, "pileup add: cigar_off decreases at read %llu", (unsigned long long)k);
        max_ops = std::max<uint64_t>(max_ops, aln->cigar_off[hi] - aln->cigar_off[lo]);
    }
    if (aln->cigar_off[n] > aln->cigar_cap)
        return fail(MSW_E_INVALID, "pileup add: the reads hold %u ops, cigar_cap is %llu", aln->cigar_off[n],
                    (unsigned long long)aln->cigar_cap);
    for (uint64_t k = 0; k < n; ++k)
        if (read_len[k] > read_stride) return fail(MSW_E_INVALID, "a length exceeds its stride");
    if ((rc = set_device(ctx))) return rc;
    auto up16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
    // [ref i64 | nm i32 | off u32 [c + 1] | ops | rlen u16 | strand | mapq | rows | quals]
    const size_t rs = read_stride, qs = qual_stride;
    const size_t o_nm = chunk * 8, o_off = o_nm + chunk * 4, o_ops = up16(o_off + (chunk + 1) * 4),
                 o_rl = up16(o_ops + max_ops * 4), o_st = up16(o_rl + chunk * 2), o_mq = up16(o_st + chunk),
                 o_rows = up16(o_mq + chunk), o_q = up16(o_rows + chunk * rs),
                 total = o_q + chunk * qs + 16;
    uint8_t* d = nullptr;
    hipError_t e = hipMalloc((void**)&d, total);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(MSW_E_NOMEM, "hipMalloc(%zu B): %s", total, hipGetErrorString(e));
    }
    hipStream_t st = ctx->compute;
    msw::PileupParams p = pile->p;
    p.rows = d + o_rows;
    p.read_len = reinterpret_cast<const uint16_t*>(d + o_rl);
    p.row_stride = rs;
    p.ref_pos = reinterpret_cast<const int64_t*>(d);
    p.nm = reinterpret_cast<const int32_t*>(d + o_nm);
    p.cigar_off = reinterpret_cast<const uint32_t*>(d + o_off);
    p.cigar = reinterpret_cast<const uint32_t*>(d + o_ops);
    p.cigar_cap = aln->cigar_cap;
    p.strand = strand ? d + o_st : nullptr;
    p.mapq = mapq ? d + o_mq : nullptr;
    p.min_mapq = min_mapq;
    p.orient = strand ? 1u : 0u;
    const msw::PileupQual q{d + o_q, qual_stride, min_baseq, pile->d_lowq};
    msw::PileupQsum qq = pile->qs;
    qq.quals = q.quals;
    qq.qual_stride = qual_stride;
    qq.min_baseq = min_baseq;
    for (uint64_t lo = 0; lo < n && e == hipSuccess; lo += chunk) {
        const uint64_t c = std::min(chunk, n - lo);
        auto up = [&](size_t at, const void* src, size_t bytes) {
            if (e == hipSuccess && bytes) e = hipMemcpyAsync(d + at, src, bytes, hipMemcpyHostToDevice, st);
        };
        const uint32_t o0 = aln->cigar_off[lo], o1 = aln->cigar_off[lo + c];
        up(0, aln->ref_pos + lo, c * 8);
        up(o_nm, aln->nm + lo, c * 4);
        up(o_off, aln->cigar_off + lo, (c + 1) * 4);
        up(o_ops, aln->cigar + o0, (size_t)(o1 - o0) * 4);
        up(o_rl, read_len + lo, c * 2);
        if (strand) up(o_st, strand + lo, c);
        if (mapq) up(o_mq, mapq + lo, c);
        up(o_rows, reads + lo * rs, c * rs);
        if (quals) up(o_q, quals + lo * qs, c * qs);
        p.n = c;
        p.cigar_base = o0;
        if (e == hipSuccess)
            e = qsum ? msw::launch_pileup_add_qsum(p, qq, st)
                     : quals ? msw::launch_pileup_add_qual(p, q, st) : msw::launch_pileup_add(p, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);  // the buffers are the next chunk's
    }
    if (e != hipSuccess) (void)hipStreamSynchronize(st);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(MSW_E_DEVICE, "pileup add: %s", hipGetErrorString(e));
    return MSW_OK;
}

int msw_pileup_finish(msw_ctx* ctx, msw_pileup* pile, void* stream) {
    int rc;
    if ((rc = check_pileup(ctx, pile))) return rc;
    if (pile->finished) return MSW_OK;
    if ((rc = set_device(ctx))) return rc;
    hipStream_t st = call_stream(ctx, stream);
    if (pile->flags & MSW_PILEUP_QSUM) HIP_TRY(msw::launch_pileup_finish_qsum(pile->p, pile->qs, pile->d_scan_tmp, st));
    else HIP_TRY(msw::launch_pileup_finish(pile->p, pile->d_scan_tmp, st));
    HIP_TRY(hipEventRecord(pile->fin, st));
    pile->finished = true;
    return MSW_OK;
}

int msw_pileup_counts_device(msw_ctx* ctx, msw_pileup* pile, const uint32_t** counts, uint64_t* pos_stride,
                             uint64_t* ch_stride) {
    int rc;
    if ((rc = check_pileup(ctx, pile))) return rc;
    if (!counts || !pos_stride || !ch_stride) return fail(MSW_E_INVALID, "NULL output");
    *counts = pile->p.counts;
    *pos_stride = pile->p.pos_mul;
    *ch_stride = pile->p.ch_mul;
    return MSW_OK;
}

int msw_pileup_counts(msw_ctx* ctx, msw_pileup* pile, uint32_t* host_out) {
    int rc;
    if ((rc = check_pileup(ctx, pile))) return rc;
    if (!pile->finished) return fail(MSW_E_INVALID, "pileup counts before msw_pileup_finish");
    const uint64_t glen = pile->p.glen;
    if (glen == 0) return MSW_OK;
    if (!host_out) return fail(MSW_E_INVALID, "host_out is NULL");
    if ((rc = set_device(ctx))) return rc;
    HIP_TRY(hipEventSynchronize(pile->fin));
    hipStream_t st = ctx->compute;
    if (pile->p.pos_mul == 8) {
        HIP_TRY(hipMemcpyAsync(host_out, pile->p.counts, glen * 32, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return MSW_OK;
    }
    // planes: rows are made on the GPU, a bounce buffer of them at a time
    const uint64_t step = std::min<uint64_t>(glen, 1u << 20);
    uint32_t* bounce = nullptr;
    hipError_t e = hipMalloc((void**)&bounce, step * 32);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(MSW_E_NOMEM, "hipMalloc(%llu B): %s", (unsigned long long)step * 32, hipGetErrorString(e));
    }
    for (uint64_t pos = 0; pos < glen && e == hipSuccess; pos += step) {
        const uint64_t m = std::min(step, glen - pos);
        e = msw::launch_pileup_rows(pile->p, pos, m, bounce, st);
        if (e == hipSuccess) e = hipMemcpyAsync(host_out + pos * 8, bounce, m * 32, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
    }
    if (e != hipSuccess) (void)hipStreamSynchronize(st);
    (void)hipFree(bounce);
    if (e != hipSuccess) return fail(MSW_E_DEVICE, "pileup counts: %s", hipGetErrorString(e));
    return MSW_OK;
}

int msw_pileup_summary(msw_ctx* ctx, msw_pileup* pile, uint32_t min_depth, msw_pileup_summary_t* out) {
    int rc;
    if ((rc = check_pileup(ctx, pile))) return rc;
    if (!out) return fail(MSW_E_INVALID, "out is NULL");
    if (min_depth == 0) return fail(MSW_E_INVALID, "pileup summary: min_depth is 0");
    if (!pile->finished) return fail(MSW_E_INVALID, "pileup summary before msw_pileup_finish");
    if ((rc = set_device(ctx))) return rc;
    HIP_TRY(hipEventSynchronize(pile->fin));
    hipStream_t st = ctx->compute;
    HIP_TRY(msw::launch_pileup_summary(pile->p, min_depth, pile->d_stats, st));
    // the read counters' slots, then covered, depth_sum, minority_ref, max_depth
    constexpr uint32_t kWords = msw::kPileupReadSlots * 2 * msw::kPileupReadSlotWords;
    std::vector<unsigned long long> h(kWords + 4);
    HIP_TRY(hipMemcpyAsync(h.data(), pile->p.reads, h.size() * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    memset(out, 0, sizeof(*out));
    for (uint32_t s = 0; s < msw::kPileupReadSlots; ++s) {
        out->reads_used += h[(s * 2 + 0) * msw::kPileupReadSlotWords];
        out->reads_skipped += h[(s * 2 + 1) * msw::kPileupReadSlotWords];
    }
    out->covered = h[kWords];
    out->depth_sum = h[kWords + 1];
    out->minority_ref = h[kWords + 2];
    out->max_depth = (uint32_t)h[kWords + 3];
    return MSW_OK;
}

int msw_pileup_lowq_columns(msw_ctx* ctx, msw_pileup* pile, uint64_t* out) {
    int rc;
    if ((rc = check_pileup(ctx, pile))) return rc;
    if (!out) return fail(MSW_E_INVALID, "out is NULL");
    if ((rc = set_device(ctx))) return rc;
    // adds may have been enqueued on any stream: wait for all of them
    HIP_TRY(hipDeviceSynchronize());
    constexpr uint32_t kWords = msw::kPileupReadSlots * msw::kPileupReadSlotWords;
    std::vector<unsigned long long> h(kWords);
    HIP_TRY(hipMemcpy(h.data(), pile->d_lowq, h.size() * 8, hipMemcpyDeviceToHost));
    *out = 0;
    for (uint32_t s = 0; s < msw::kPileupReadSlots; ++s) *out += h[s * msw::kPileupReadSlotWords];
    return MSW_OK;
}

// Quality sums (include/msw.h, "Quality sums and weighted genotypes").
static int check_pileup_qsum(const msw_ctx* ctx, const msw_pileup* pile, const char* what) {
    int rc;
    if ((rc = check_pileup(ctx, pile))) return rc;
    if (!(pile->flags & MSW_PILEUP_QSUM)) return fail(MSW_E_INVALID, "%s: the pileup was created without MSW_PILEUP_QSUM", what);
    return MSW_OK;
}

int msw_pileup_qsums_device(msw_ctx* ctx, msw_pileup* pile, const uint32_t** qsums, uint64_t* pos_stride,
                            uint64_t* ch_stride) {
    int rc;
    if ((rc = check_pileup_qsum(ctx, pile, "pileup qsums"))) return rc;
    if (!qsums || !pos_stride || !ch_stride) return fail(MSW_E_INVALID, "NULL output");
    *qsums = pile->qs.qsum;
    *pos_stride = 4;
    *ch_stride = 1;
    return MSW_OK;
}

int msw_pileup_qsums(msw_ctx* ctx, msw_pileup* pile, uint32_t* host_out) {
    int rc;
    if ((rc = check_pileup_qsum(ctx, pile, "pileup qsums"))) return rc;
    if (!pile->finished) return fail(MSW_E_INVALID, "pileup qsums before msw_pileup_finish");
    const uint64_t glen = pile->p.glen;
    if (glen == 0) return MSW_OK;
    if (!host_out) return fail(MSW_E_INVALID, "host_out is NULL");
    if ((rc = set_device(ctx))) return rc;
    HIP_TRY(hipEventSynchronize(pile->fin));
    hipStream_t st = ctx->compute;
    HIP_TRY(hipMemcpyAsync(host_out, pile->qs.qsum, glen * 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return MSW_OK;
}

// Variants (include/msw.h, "Variants"; the kernels: msw_call.hip).
void msw_call_qparams_default(msw_call_qparams_t* q) {
    if (!q) return;
    *q = msw_call_qparams_t{100, 477};
}

static int check_call_qparams(const msw_call_qparams_t* qparams, msw::CallParams* p) {
    msw_call_qparams_t q;
    if (qparams) q = *qparams;
    else msw_call_qparams_default(&q);
    if (q.q_scale > 65535u || q.q_third > 65535u)
        return fail(MSW_E_INVALID, "call qparams: q_scale or q_third above 65535");
    p->q_scale = q.q_scale;
    p->q_third = q.q_third;
    return MSW_OK;
}

void msw_call_params_default(msw_call_params_t* q) {
    if (!q) return;
    *q = msw_call_params_t{4, 2, 200, 20, 4, 2477, 304, 3000, 3301};
}

static int check_call_params(const msw_call_params_t* params, msw_call_params_t* q) {
    if (params) *q = *params;
    else msw_call_params_default(q);
    if (q->q_hit > 65535u || q->q_miss > 65535u || q->q_het > 65535u)
        return fail(MSW_E_INVALID, "call params: a q_* cost above 65535");
    if (q->min_depth == 0) return fail(MSW_E_INVALID, "call params: min_depth is 0");
    if (q->min_alt_permille > 1000u) return fail(MSW_E_INVALID, "call params: min_alt_permille %u > 1000", q->min_alt_permille);
    return MSW_OK;
}

static_assert(sizeof(msw_variant_t) == 48, "msw_variant_t is 48 bytes, in memory and in the .var file");

// both device forms; weighted: the call of "Quality sums and weighted genotypes"
static int pileup_call_device(msw_ctx* ctx, msw_pileup* pile, const msw_call_params_t* params, bool weighted,
                              const msw_call_qparams_t* qparams, msw_variant_t* out_dev, uint64_t cap,
                              uint64_t* n_total_dev, void* stream) {
    int rc;
    msw::CallParams p{};
    if ((rc = weighted ? check_pileup_qsum(ctx, pile, "pileup call") : check_pileup(ctx, pile))) return rc;
    if ((rc = check_call_params(params, &p.q))) return rc;
    if (weighted && (rc = check_call_qparams(qparams, &p))) return rc;
    if (!pile->finished) return fail(MSW_E_INVALID, "pileup call before msw_pileup_finish");
    if (cap && !out_dev) return fail(MSW_E_INVALID, "out is NULL with cap > 0");
    if (pile->p.glen > 0x7FFFFFFFull) return fail(MSW_E_RANGE, "pileup call: genome above 2^31-1 bases");
    if ((rc = set_device(ctx))) return rc;
    hipStream_t st = call_stream(ctx, stream);
    // behind the fold, whatever stream it ran on
    HIP_TRY(hipStreamWaitEvent(st, pile->fin, 0));
    p.genome = pile->p.genome;
    p.counts = pile->p.counts;
    p.pos_mul = pile->p.pos_mul;
    p.ch_mul = pile->p.ch_mul;
    p.m = p.rows = pile->p.glen;
    p.out = out_dev;
    p.cap = cap;
    p.n_total = reinterpret_cast<unsigned long long*>(n_total_dev);
    p.qsum = weighted ? pile->qs.qsum : nullptr;
    HIP_TRY(hipMallocAsync((void**)&p.tile_off, msw::call_tmp_words(p.m) * sizeof(uint32_t), st));
    hipError_t e = msw::launch_call(p, st);
    const hipError_t ef = hipFreeAsync(p.tile_off, st);
    if (e == hipSuccess) e = ef;
    if (e != hipSuccess) return fail(MSW_E_DEVICE, "pileup call: %s", hipGetErrorString(e));
    return MSW_OK;
}

int msw_pileup_call_device(msw_ctx* ctx, msw_pileup* pile, const msw_call_params_t* params, msw_variant_t* out_dev,
                           uint64_t cap, uint64_t* n_total_dev, void* stream) {
    return pileup_call_device(ctx, pile, params, false, nullptr, out_dev, cap, n_total_dev, stream);
}

int msw_pileup_call_qual_device(msw_ctx* ctx, msw_pileup* pile, const msw_call_params_t* params,
                                const msw_call_qparams_t* qparams, msw_variant_t* out_dev, uint64_t cap,
                                uint64_t* n_total_dev, void* stream) {
    return pileup_call_device(ctx, pile, params, true, qparams, out_dev, cap, n_total_dev, stream);
}

static int pileup_call(msw_ctx* ctx, msw_pileup* pile, const msw_call_params_t* params, bool weighted,
                       const msw_call_qparams_t* qparams, msw_variant_t* out_host, uint64_t cap, uint64_t* n_total) {
    int rc;
    if ((rc = weighted ? check_pileup_qsum(ctx, pile, "pileup call") : check_pileup(ctx, pile))) return rc;
    if (!n_total) return fail(MSW_E_INVALID, "n_total is NULL");
    if (cap && !out_host) return fail(MSW_E_INVALID, "out is NULL with cap > 0");
    if ((rc = set_device(ctx))) return rc;
    // at most two records per base
    const uint64_t dcap = std::min<uint64_t>(cap, pile->p.glen * 2);
    uint8_t* d = nullptr;
    hipError_t e = hipMalloc((void**)&d, 16 + dcap * sizeof(msw_variant_t));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(MSW_E_NOMEM, "hipMalloc(%llu B): %s", (unsigned long long)(16 + dcap * sizeof(msw_variant_t)),
                    hipGetErrorString(e));
    }
    hipStream_t st = ctx->compute;
    msw_variant_t* d_out = reinterpret_cast<msw_variant_t*>(d + 16);
    rc = pileup_call_device(ctx, pile, params, weighted, qparams, dcap ? d_out : nullptr, dcap,
                            reinterpret_cast<uint64_t*>(d), st);
    if (rc == MSW_OK) {
        uint64_t total = 0;
        e = hipMemcpyAsync(&total, d, 8, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        const uint64_t have = std::min(total, dcap);
        if (e == hipSuccess && have) e = hipMemcpyAsync(out_host, d_out, have * sizeof(msw_variant_t), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) rc = fail(MSW_E_DEVICE, "pileup call: %s", hipGetErrorString(e));
        else *n_total = total;
    } else {
        (void)hipStreamSynchronize(st);
    }
    (void)hipFree(d);
    return rc;
}

int msw_pileup_call(msw_ctx* ctx, msw_pileup* pile, const msw_call_params_t* params, msw_variant_t* out_host,
                    uint64_t cap, uint64_t* n_total) {
    return pileup_call(ctx, pile, params, false, nullptr, out_host, cap, n_total);
}

int msw_pileup_call_qual(msw_ctx* ctx, msw_pileup* pile, const msw_call_params_t* params,
                         const msw_call_qparams_t* qparams, msw_variant_t* out_host, uint64_t cap, uint64_t* n_total) {
    return pileup_call(ctx, pile, params, true, qparams, out_host, cap, n_total);
}

static int call_counts(msw_ctx* ctx, const uint8_t* genome_host, uint64_t glen, const uint32_t* counts_host,
                       bool weighted, const uint32_t* qsums_host, const msw_call_params_t* params,
                       const msw_call_qparams_t* qparams, uint64_t chunk_pos, msw_variant_t* out_host, uint64_t cap,
                       uint64_t* n_total) {
    int rc;
    msw::CallParams p{};
    if (!ctx) return fail(MSW_E_INVALID, "ctx is NULL");
    if (!n_total) return fail(MSW_E_INVALID, "n_total is NULL");
    if ((rc = check_call_params(params, &p.q))) return rc;
    if (weighted && (rc = check_call_qparams(qparams, &p))) return rc;
    if (cap && !out_host) return fail(MSW_E_INVALID, "out is NULL with cap > 0");
    if (chunk_pos > (1ull << 24)) return fail(MSW_E_RANGE, "call counts: chunk_pos above 2^24");
    *n_total = 0;
    if (glen == 0) return MSW_OK;
    if (!genome_host || !counts_host || (weighted && !qsums_host)) return fail(MSW_E_INVALID, "NULL array");
    if ((rc = set_device(ctx))) return rc;
    const uint64_t chunk = std::min<uint64_t>(glen, chunk_pos ? chunk_pos : 1ull << 20);
    auto up16 = [](uint64_t x) { return (x + 15) & ~(uint64_t)15; };
    // [rows of chunk + 1 positions | genome bytes | total u64 | tile offsets and scan words | weighted: rows of four]
    const uint64_t o_gen = (chunk + 1) * 32, o_tot = o_gen + up16(chunk), o_tile = o_tot + 16,
                   o_qsum = o_tile + up16(msw::call_tmp_words(chunk) * 4), bytes = o_qsum + (weighted ? chunk * 16 : 0);
    uint8_t* d = nullptr;
    hipError_t e = hipMalloc((void**)&d, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(MSW_E_NOMEM, "hipMalloc(%llu B): %s", (unsigned long long)bytes, hipGetErrorString(e));
    }
    hipStream_t st = ctx->compute;
    p.counts = reinterpret_cast<const uint32_t*>(d);
    p.genome = d + o_gen;
    p.pos_mul = 8;
    p.ch_mul = 1;
    p.n_total = reinterpret_cast<unsigned long long*>(d + o_tot);
    p.tile_off = reinterpret_cast<uint32_t*>(d + o_tile);
    p.qsum = weighted ? reinterpret_cast<const uint32_t*>(d + o_qsum) : nullptr;
    msw_variant_t* d_out = nullptr;  // grows to the largest chunk's records that still fit cap
    uint64_t d_out_cap = 0, total = 0, written = 0;
    bool nomem = false;
    for (uint64_t lo = 0; lo < glen && e == hipSuccess; lo += chunk) {
        const uint64_t m = std::min(chunk, glen - lo);
        p.m = m;
        p.rows = lo + m < glen ? m + 1 : m;  // the look-ahead row
        p.pos0 = lo;
        p.out = nullptr;
        p.cap = 0;
        e = hipMemcpyAsync(d, counts_host + lo * 8, p.rows * 32, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(d + o_gen, genome_host + lo, m, hipMemcpyHostToDevice, st);
        if (e == hipSuccess && weighted)
            e = hipMemcpyAsync(d + o_qsum, qsums_host + lo * 4, m * 16, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = msw::launch_call_count(p, st);
        if (e == hipSuccess) e = msw::launch_call_scan(p, st);
        uint64_t t = 0;
        if (e == hipSuccess) e = hipMemcpyAsync(&t, p.n_total, 8, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) break;
        const uint64_t want = std::min(t, cap - written);
        if (want) {
            if (want > d_out_cap) {
                if (d_out) (void)hipFree(d_out);
                d_out = nullptr;
                d_out_cap = 0;
                e = hipMalloc((void**)&d_out, want * sizeof(msw_variant_t));
                if (e != hipSuccess) {
                    (void)hipGetLastError();
                    nomem = true;
                    break;
                }
                d_out_cap = want;
            }
            p.out = d_out;
            p.cap = want;
            e = msw::launch_call_emit(p, st);
            if (e == hipSuccess)
                e = hipMemcpyAsync(out_host + written, d_out, want * sizeof(msw_variant_t), hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);  // the buffers are the next chunk's
            written += want;
        }
        total += t;
    }
    if (e != hipSuccess) (void)hipStreamSynchronize(st);
    if (d_out) (void)hipFree(d_out);
    (void)hipFree(d);
    if (nomem) return fail(MSW_E_NOMEM, "hipMalloc for a chunk's records: %s", hipGetErrorString(e));
    if (e != hipSuccess) return fail(MSW_E_DEVICE, "call counts: %s", hipGetErrorString(e));
    *n_total = total;
    return MSW_OK;
}

int msw_call_counts(msw_ctx* ctx, const uint8_t* genome_host, uint64_t glen, const uint32_t* counts_host,
                    const msw_call_params_t* params, uint64_t chunk_pos, msw_variant_t* out_host, uint64_t cap,
                    uint64_t* n_total) {
    return call_counts(ctx, genome_host, glen, counts_host, false, nullptr, params, nullptr, chunk_pos, out_host, cap,
                       n_total);
}

int msw_call_counts_qual(msw_ctx* ctx, const uint8_t* genome_host, uint64_t glen, const uint32_t* counts_host,
                         const uint32_t* qsums_host, const msw_call_params_t* params,
                         const msw_call_qparams_t* qparams, uint64_t chunk_pos, msw_variant_t* out_host, uint64_t cap,
                         uint64_t* n_total) {
    return call_counts(ctx, genome_host, glen, counts_host, true, qsums_host, params, qparams, chunk_pos, out_host, cap,
                       n_total);
}

int msw_memcpy_d2h_async(msw_ctx* ctx, void* dst, const void* src, size_t bytes, void* stream) {
    if (!ctx) return fail(MSW_E_INVALID, "ctx is NULL");
    int rc = set_device(ctx);
    if (rc) return rc;
    hipStream_t st = call_stream(ctx, stream);
    // Into pinned host memory the copy is a kernel on the caller's stream,
    // not a DMA: the copy engines serve every stream of the process from
    // shared in-order rings, so a DMA that waits on its stream's scoring
    // kernel holds up the copies other workers queued behind it (config 3
    // from FASTQ: one worker's result copies 2 ms late, behind the other's
    // next batch).  Source and destination that differ in
    // alignment mod 16 go by DMA: the kernel would copy them byte by byte
    // (ADVICE r05).
    if (bytes && (((uintptr_t)dst ^ (uintptr_t)src) & 15) == 0 && pinned_cached(ctx, dst, bytes)) {
        void* dp = nullptr;
        if (hipHostGetDevicePointer(&dp, dst, 0) == hipSuccess && dp) {
            HIP_TRY(msw::launch_d2h_copy(dp, src, bytes, st));
            return MSW_OK;
        }
        (void)hipGetLastError();
    }
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st));
    return MSW_OK;
}

void* msw_host_alloc(size_t bytes) {
    void* p = nullptr;
    // portable: the --full-wgs readers fill slabs that any GPU's context DMAs
    if (hipHostMalloc(&p, bytes, hipHostMallocPortable) != hipSuccess) {
        fail(MSW_E_NOMEM, "hipHostMalloc(%zu) failed", bytes);
        return nullptr;
    }
    return p;
}

void msw_host_free(void* p) {
    if (!p) return;
    (void)hipHostFree(p);
    g_host_free_epoch.fetch_add(1, std::memory_order_release);  // every context's pinned cache is stale
}

void* msw_dev_alloc(msw_ctx* ctx, size_t bytes) {
    if (!ctx || set_device(ctx)) return nullptr;
    void* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) {
        fail(MSW_E_NOMEM, "hipMalloc(%zu) failed", bytes);
        return nullptr;
    }
    return p;
}

void msw_dev_free(msw_ctx* ctx, void* p) {
    if (ctx) (void)hipSetDevice(ctx->device);
    if (p) (void)hipFree(p);
}

int msw_memcpy_h2d(msw_ctx* ctx, void* dst, const void* src, size_t bytes) {
    if (!ctx) return fail(MSW_E_INVALID, "ctx is NULL");
    int rc = set_device(ctx);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return MSW_OK;
}

int msw_memcpy_d2h(msw_ctx* ctx, void* dst, const void* src, size_t bytes) {
    if (!ctx) return fail(MSW_E_INVALID, "ctx is NULL");
    int rc = set_device(ctx);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return MSW_OK;
}

int msw_ctx_prepare(msw_ctx* ctx, const msw_scoring_t* sc) {
    if (!ctx) return fail(MSW_E_INVALID, "ctx is NULL");
    Scheme sch;
    int rc;
    if ((rc = make_scheme(sc, ctx->opt, &sch))) return rc;
    if ((rc = set_device(ctx))) return rc;
    // one occupancy query per kernel module (translation unit): the query
    // loads the module; the shapes are any valid ones of that unit
    msw::SwParams p = base_params(sch);
    p.n_slots = 1;
    p.lds_stride = msw::stream_stride(300);
    p.group_lanes = 16;
    p.groups = 4;
    p.pairs_blocks = 1;
    int ok = 1;
    ok &= msw::sw_blocks_per_cu(p, sch.affine, sch.coords, 16, msw::Layout::kPairs) > 0;    // pairs, KR <= 16
    ok &= msw::sw_blocks_per_cu(p, sch.affine, sch.coords, 300, msw::Layout::kPairs) > 0;   // pairs, KR 17..24
    ok &= msw::sw_blocks_per_cu(p, sch.affine, sch.coords, 32, msw::Layout::kSplit) > 0;    // split
    ok &= msw::sw_blocks_per_cu(p, sch.affine, sch.coords, 32, msw::Layout::kMixed) > 0;    // mixed grid
    msw::MultiTable t;
    memset(&t, 0, sizeof(t));
    t.n_buckets = 1;
    t.block_end[0] = 1;
    t.count[0] = 1;
    t.lds_stride[0] = p.lds_stride;
    static const uint32_t dummy_order = 0;
    p.order = &dummy_order;  // never dereferenced: nothing launches
    for (uint32_t kr : {1u, 17u}) {  // the bucketed grid and its wide instance
        t.kr[0] = kr;
        ok &= msw::sw_multi_blocks_per_cu(p, t, sch.affine, sch.coords) > 0;
    }
    p.order = nullptr;
    static const uint8_t dummy_genome = 0;
    p.win_src = &dummy_genome;  // genome-window instances
    ok &= msw::sw_blocks_per_cu(p, sch.affine, sch.coords, 16, msw::Layout::kPairs) > 0;
    p.win_src = nullptr;
    ok &= msw::long_blocks_per_cu(sch.affine, sch.coords, 600, 600) > 0;
    ok &= msw::cut_blocks_per_cu() > 0;
    ok &= msw::strand_blocks_per_cu() > 0;  // both strands
    ok &= msw::seed_blocks_per_cu(4096) > 0;  // placing reads
    msw::TraceParams tp;
    memset(&tp, 0, sizeof(tp));
    tp.max_rows = 150;
    tp.max_cols = 300;
    tp.cigar_stride = 64;
    ok &= msw::trace_blocks_per_cu(sch.affine, tp.max_rows, msw::trace_lds_layout(tp, sch.affine)) > 0;  // traceback
    (void)hipGetLastError();
    return ok ? MSW_OK : fail(MSW_E_DEVICE, "kernel module load failed");
}

int msw_ctx_stats(msw_ctx* ctx, msw_stats_t* out, int reset) {
    if (!ctx || !out) return fail(MSW_E_INVALID, "ctx/out is NULL");
    if (set_device(ctx) == MSW_OK) harvest_dev_timings(ctx, true);
    *out = ctx->stats;
    if (reset) ctx->stats = msw_stats_t{};
    return MSW_OK;
}

int msw_fence_record(msw_ctx* ctx, void* stream, uint64_t* fence) {
    if (!ctx || !fence) return fail(MSW_E_INVALID, "ctx/fence is NULL");
    int rc = set_device(ctx);
    if (rc) return rc;
    hipEvent_t e = take_event(ctx);
    if (!e) return fail(MSW_E_DEVICE, "hipEventCreate failed");
    std::lock_guard<std::mutex> lk(ctx->ev_mu);
    if (hipEventRecord(e, call_stream(ctx, stream)) != hipSuccess) {
        ctx->free_events.push_back(e);
        return fail(MSW_E_DEVICE, "hipEventRecord failed");
    }
    *fence = ctx->next_fence++;
    ctx->fences.emplace(*fence, e);
    return MSW_OK;
}

int msw_fence_wait(msw_ctx* ctx, uint64_t fence) {
    if (!ctx) return fail(MSW_E_INVALID, "ctx is NULL");
    hipEvent_t e = nullptr;
    {
        std::lock_guard<std::mutex> lk(ctx->ev_mu);
        auto it = ctx->fences.find(fence);
        if (it == ctx->fences.end()) return fail(MSW_E_INVALID, "unknown fence %llu", (unsigned long long)fence);
        e = it->second;
        ctx->fences.erase(it);
    }
    int rc = set_device(ctx);
    if (rc) return rc;
    const hipError_t err = hipEventSynchronize(e);
    {
        std::lock_guard<std::mutex> lk(ctx->ev_mu);
        ctx->free_events.push_back(e);
    }
    if (err != hipSuccess) return fail(MSW_E_DEVICE, "GPU error before the fence: %s", hipGetErrorString(err));
    return MSW_OK;
}

int msw_synchronize(msw_ctx* ctx) {
    if (!ctx) return fail(MSW_E_INVALID, "ctx is NULL");
    int rc = set_device(ctx);
    if (rc) return rc;
    for (hipStream_t st : {ctx->compute, ctx->compute2, ctx->copy, ctx->d2h, ctx->side})
        if (st) HIP_TRY(hipStreamSynchronize(st));
    for (hipStream_t st : ctx->user_streams) HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipGetLastError());
    return MSW_OK;
}

int msw_stream_create(msw_ctx* ctx, void** out) {
    if (!ctx || !out) return fail(MSW_E_INVALID, "ctx/out is NULL");
    *out = nullptr;
    int rc = set_device(ctx);
    if (rc) return rc;
    hipStream_t st = nullptr;
    HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    ctx->user_streams.push_back(st);
    *out = st;
    return MSW_OK;
}

int msw_stream_destroy(msw_ctx* ctx, void* stream) {
    if (!ctx || !stream) return fail(MSW_E_INVALID, "ctx/stream is NULL");
    auto it = std::find(ctx->user_streams.begin(), ctx->user_streams.end(), (hipStream_t)stream);
    if (it == ctx->user_streams.end()) return fail(MSW_E_INVALID, "stream was not made by msw_stream_create on this context");
    int rc = set_device(ctx);
    if (rc) return rc;
    ctx->user_streams.erase(it);
    // its per-stream scratch goes too (a later stream may reuse the handle)
    for (size_t i = 0; i < ctx->rscratch.size(); ++i)
        if (ctx->rscratch[i].st == (hipStream_t)stream) {
            HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
            (void)hipFree(ctx->rscratch[i].wins);
            (void)hipFree(ctx->rscratch[i].wlen);
            ctx->rscratch.erase(ctx->rscratch.begin() + (long)i);
            break;
        }
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    HIP_TRY(hipStreamDestroy((hipStream_t)stream));
    return MSW_OK;
}

}  // extern "C"
