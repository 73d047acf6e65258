// msw_runtime_internal.h -- what the runtime's translation units share:
//   msw_runtime.cpp    context, staging pipeline, scoring calls, plans, compat,
//                      genome, reads and strands scoring, memory and streams
//   msw_rt_trace.cpp   traceback, alignment records
//   msw_rt_map.cpp     index, seeds, candidates, MAPQ, pairs, the map drivers
//   msw_rt_pileup.cpp  pileup, variant calls
//   msw_rt_band.cpp    banded alignment
//   msw_rt_sort.cpp    sorting and duplicates
//   msw_rt_deflate.cpp BGZF deflate (include/msw_fastq.h)
// Each section of include/msw.h is implemented in one of them; nothing but
// this header is shared between them.  Not installed, not part of the C ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <deque>
#include <functional>
#include <initializer_list>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/msw.h"
#include "msw_kernels.h"

namespace msw_detail {

// Sets msw_last_error() and returns `code`.
int fail(int code, const char* fmt, ...);

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return ::msw_detail::fail(MSW_E_DEVICE, "%s failed: %s (%s:%d)", #expr,            \
                                      hipGetErrorString(e_), __FILE__, __LINE__);              \
    } while (0)

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

extern const Options kDefaultOptions;

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

int make_scheme(const msw_scoring_t* sc, const Options& opt, Scheme* s);

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

}  // namespace msw_detail

struct msw_ctx {
    int device = 0;
    int cu_count = 256;
    msw_detail::Options opt;  // the environment's switches, read at creation
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
    msw_detail::Slot slots[kSlots];
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

namespace msw_detail {

// --- msw_runtime.cpp -------------------------------------------------------

int set_device(msw_ctx* ctx);

// The stream of a device-API call: the caller's, or the context's compute stream.
inline hipStream_t call_stream(const msw_ctx* ctx, void* stream) {
    return stream ? (hipStream_t)stream : ctx->compute;
}

void max_u16(const uint16_t* a, uint64_t n, uint32_t& m);

inline uint32_t round16(uint32_t v) { return (v + 15u) & ~15u; }

// A pair (or a bound) beyond the packed kernels' limits.
inline bool is_long(uint32_t m, uint32_t n) {
    return m > (uint32_t)msw::kMaxReadLen || n > (uint32_t)msw::kMaxWinLen;
}

int check_bounds(const Scheme& s, uint32_t max_m, uint32_t max_n);
int validate_batch(const msw_batch_t* b, const msw_out_t* out, const Scheme& sch);
int check_strides(const msw_batch_t& b, uint32_t max_m, uint32_t max_n);

// Both orientations of a device batch on one stream (strands scoring);
// `score` is one scoring pass.
using ScorePass = std::function<int(const msw_batch_t*, msw_out_t*)>;
int score_both_strands(msw_ctx* ctx, const msw_scoring_t* sc, const msw_batch_t* b, msw_out_t* out, uint8_t* strand,
                       uint8_t* oriented, uint32_t oriented_stride, hipStream_t st, const ScorePass& score);

// --- msw_rt_trace.cpp ------------------------------------------------------

int check_trace_bounds(uint32_t max_m, uint32_t max_n);
int check_trace_bounds(const Scheme& sch, uint32_t max_m, uint32_t max_n, bool long_pairs);
int validate_trace(const msw_trace_t* tr);
int validate_aln(const msw_aln_t* a);

// --- the chunked host drivers' three pieces --------------------------------

// One device allocation carved into typed arrays.  Plan with take() (every
// array starts 256-byte aligned), then alloc() once; a slice converts to its
// pointer from then on.  The destructor frees, so a driver must have drained
// its stream by then (ChunkCopy::finish).  The allocation ends in kTail spare
// bytes: the kernels read rows in 16-byte pieces, past the last element of
// an array whose length is no multiple of 16, and any array may be the last.
class DeviceArena {
public:
    static constexpr size_t kAlign = 256, kTail = 256;
    template <class T>
    struct Slice {
        const DeviceArena* arena;
        size_t at;
        operator T*() const { return reinterpret_cast<T*>(arena->base_ + at); }
    };
    DeviceArena() = default;
    DeviceArena(const DeviceArena&) = delete;
    DeviceArena& operator=(const DeviceArena&) = delete;
    ~DeviceArena() { (void)hipFree(base_); }
    template <class T>
    Slice<T> take(size_t count) {
        const size_t at = bytes_;
        bytes_ = (at + count * sizeof(T) + kAlign - 1) & ~(kAlign - 1);
        return {this, at};
    }
    size_t bytes() const { return bytes_ + kTail; }
    int alloc() {
        const hipError_t e = hipMalloc((void**)&base_, bytes());
        if (e == hipSuccess) return MSW_OK;
        base_ = nullptr;
        (void)hipGetLastError();
        return fail(MSW_E_NOMEM, "hipMalloc(%zu B): %s", bytes(), hipGetErrorString(e));
    }

private:
    uint8_t* base_ = nullptr;
    size_t bytes_ = 0;
};

// Temporaries of one call on `st`: allocated before its launches, freed behind them.
struct StreamTmp {
    void* p = nullptr;
    hipStream_t st;
    explicit StreamTmp(hipStream_t s) : st(s) {}
    StreamTmp(const StreamTmp&) = delete;
    StreamTmp& operator=(const StreamTmp&) = delete;
    ~StreamTmp() {
        if (p) (void)hipFreeAsync(p, st);
    }
    int alloc(uint64_t bytes) {
        const hipError_t e = hipMallocAsync(&p, bytes + DeviceArena::kTail, st);
        if (e == hipSuccess) return MSW_OK;
        p = nullptr;
        (void)hipGetLastError();
        return fail(MSW_E_NOMEM, "hipMallocAsync(%llu B): %s", (unsigned long long)bytes, hipGetErrorString(e));
    }
};

// The copies of a chunked driver on one stream, with a sticky error: after a
// failure every later call is a no-op and finish() reports it.
struct ChunkCopy {
    hipStream_t st;
    hipError_t e = hipSuccess;
    explicit ChunkCopy(hipStream_t s) : st(s) {}
    bool ok() const { return e == hipSuccess; }
    void up(void* dst, const void* src, size_t bytes) {
        if (e == hipSuccess && bytes) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st);
    }
    void down(void* dst, const void* src, size_t bytes) {
        if (e == hipSuccess && bytes) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st);
    }
    void sync() { note(hipStreamSynchronize(st)); }
    // A launch (or any HIP call) between the copies.
    void note(hipError_t x) { e = e == hipSuccess ? x : e; }
    // The end of a driver, with rc the first failing msw call's code: on any
    // error the stream is drained before the caller's arena frees what the
    // work in flight uses.
    int finish(int rc, const char* what) {
        if (rc || e != hipSuccess) (void)hipStreamSynchronize(st);
        if (rc) return rc;
        if (e != hipSuccess) return fail(MSW_E_DEVICE, "%s: %s", what, hipGetErrorString(e));
        return MSW_OK;
    }
};

// The packed ops of a records driver across its chunks: the device buffer
// (grown to a chunk's total when it does not fit), the ops of the chunks
// before the current one, and the current chunk's offsets on the host.
struct RecordOps {
    uint32_t* d_ops = nullptr;
    uint64_t cap = 0, base = 0;
    std::vector<uint32_t> off;
    RecordOps() = default;
    RecordOps(const RecordOps&) = delete;
    RecordOps& operator=(const RecordOps&) = delete;
    ~RecordOps() { (void)hipFree(d_ops); }
    int alloc(uint64_t ops);  // a buffer of `ops` ops in place of the present one; MSW_E_NOMEM
};

// One chunk's device arrays as pack_chunk_records reads and writes them.
struct ChunkRecords {
    const uint8_t* rows;  // the reads as aligned (oriented rows where there are any)
    uint32_t row_stride;
    const uint16_t* read_len;
    const int64_t* win_pos;
    const msw_out_t* ends;
    const msw_trace_t* tr;
    int64_t* ref_pos;  // [c]
    int32_t* nm;       // [c]
    uint32_t* off;     // [c + 2]: the offsets and the overflow count
};
struct ChunkPull {
    void* dst;
    const void* src;
    size_t bytes;
};

// Rows [lo, lo + c) of a records driver, traced: packs them, pulls the
// offsets, regrows ops once when the chunk's total exceeds it and packs
// again; then enqueues the driver's own downloads `first`, those of ref_pos,
// nm and of the ops that fit the room left under aln->cigar_cap, writes
// aln->cigar_off[lo .. lo + c] rebased onto the batch, and advances
// ops.base.  The caller synchronises.  Returns the first failing msw call's
// code (a failed regrow: MSW_E_NOMEM); a failed copy stays in cp.
int pack_chunk_records(msw_ctx* ctx, const msw_genome* g, ChunkCopy& cp, RecordOps& ops, const ChunkRecords& r,
                       uint64_t lo, uint64_t c, std::initializer_list<ChunkPull> first, msw_aln_t* aln);

}  // namespace msw_detail
