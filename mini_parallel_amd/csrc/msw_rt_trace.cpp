// msw_rt_trace.cpp -- traceback and alignment records (include/msw.h,
// "Traceback", "Traceback for long pairs", "Alignment records" and the host
// call of "Both strands"): the trace grid and its launches, the device calls,
// the pack, and the chunked host drivers msw_align_batch_trace* and
// msw_align_reads_trace* / msw_align_reads_strands.  The kernels:
// msw_trace.hip, msw_trace_long.hip, msw_aln.hip.
#include "msw_runtime_internal.h"

using namespace msw_detail;

namespace msw_detail {

// Traceback on sw_trace_kernel supports the packed kernels' range only; the
// *_long calls take bounds up to kMaxLongLen (check_bounds).
int check_trace_bounds(uint32_t max_m, uint32_t max_n) {
    if (max_m > (uint32_t)msw::kMaxReadLen)
        return fail(MSW_E_RANGE, "traceback: read length %u > %d", max_m, msw::kMaxReadLen);
    if (max_n > (uint32_t)msw::kMaxWinLen)
        return fail(MSW_E_RANGE, "traceback: window length %u > %d", max_n, msw::kMaxWinLen);
    return MSW_OK;
}
int check_trace_bounds(const Scheme& sch, uint32_t max_m, uint32_t max_n, bool long_pairs) {
    return long_pairs ? check_bounds(sch, max_m, max_n) : check_trace_bounds(max_m, max_n);
}

int validate_trace(const msw_trace_t* tr) {
    if (!tr) return fail(MSW_E_INVALID, "trace is NULL");
    if (!tr->start_i || !tr->start_j || !tr->n_cigar) return fail(MSW_E_INVALID, "NULL array in trace");
    if (tr->cigar_stride && !tr->cigar) return fail(MSW_E_INVALID, "cigar is NULL with cigar_stride > 0");
    return MSW_OK;
}

int validate_aln(const msw_aln_t* a) {
    if (!a) return fail(MSW_E_INVALID, "aln is NULL");
    if (!a->ref_pos || !a->nm || !a->cigar_off || !a->n_overflow) return fail(MSW_E_INVALID, "NULL array in aln");
    if (a->cigar_cap && !a->cigar) return fail(MSW_E_INVALID, "cigar is NULL with cigar_cap > 0");
    return MSW_OK;
}

int RecordOps::alloc(uint64_t ops) {
    if (d_ops) (void)hipFree(d_ops);
    d_ops = nullptr;
    cap = 0;
    const hipError_t e = hipMalloc((void**)&d_ops, ops * 4);
    if (e != hipSuccess) {
        d_ops = nullptr;
        (void)hipGetLastError();
        return fail(MSW_E_NOMEM, "hipMalloc(%llu B) for the packed ops: %s", (unsigned long long)ops * 4,
                    hipGetErrorString(e));
    }
    cap = ops;
    return MSW_OK;
}

// Two passes at the most: the first tells the chunk's total, and where that
// exceeds the buffer the second packs into one of exactly that size.  The
// trace stride is exact, so no read overflows and off[c] is the true total.
int pack_chunk_records(msw_ctx* ctx, const msw_genome* g, ChunkCopy& cp, RecordOps& ops, const ChunkRecords& r,
                       uint64_t lo, uint64_t c, std::initializer_list<ChunkPull> first, msw_aln_t* aln) {
    uint64_t total = 0;
    if (ops.off.size() < c + 1) ops.off.resize(c + 1);
    for (int pass = 0; pass < 2; ++pass) {
        msw_aln_t da = {r.ref_pos, r.nm, r.off, ops.d_ops, ops.cap, r.off + c + 1};
        int rc = msw_aln_pack_device(ctx, g, r.rows, r.read_len, r.row_stride, r.win_pos, c, r.ends, r.tr, &da, cp.st);
        if (rc) return rc;
        cp.down(ops.off.data(), r.off, (c + 1) * 4);
        cp.sync();
        if (!cp.ok()) return MSW_OK;  // cp.finish reports it
        total = ops.off[c];
        if (total <= ops.cap) break;
        if ((rc = ops.alloc(total))) return rc;
    }
    for (const ChunkPull& p : first) cp.down(p.dst, p.src, p.bytes);
    cp.down(aln->ref_pos + lo, r.ref_pos, c * 8);
    cp.down(aln->nm + lo, r.nm, c * 4);
    const uint64_t room = aln->cigar_cap > ops.base ? aln->cigar_cap - ops.base : 0;
    cp.down(aln->cigar + ops.base, ops.d_ops, std::min(total, room) * 4);
    // one prefix sum over the whole batch: this chunk's offsets start at ops.base
    for (uint64_t k = 0; k <= c; ++k) aln->cigar_off[lo + k] = (uint32_t)(ops.base + ops.off[k]);
    ops.base += total;
    return MSW_OK;
}

}  // namespace msw_detail

extern "C" {

// What both traceback kernels' launches share.  p holds the call's inputs and
// outputs (windows from a slab or from the genome); this fills the bounds and
// the scoring.
static void trace_call_params(msw::TraceParams& p, const msw_scoring_t* sc, uint64_t n_pairs, uint32_t max_read_len,
                              uint32_t max_win_len) {
    p.n_slots = (uint32_t)n_pairs;
    p.max_rows = max_read_len;
    p.max_cols = max_win_len;
    p.match = sc->match;
    p.mismatch = sc->mismatch;
    p.gap = sc->gap_extend;
    p.goe = sc->gap_open + sc->gap_extend;
}

// The grid and its global scratch: one block per pair while a block needs no
// scratch (block_bytes == 0); else the grid is capped (what the CUs hold at
// once -- per_cu() is asked only then -- and 256 MiB of scratch) and finished
// blocks take the next pair from a queue.  Scratch and counter are allocated
// stream-ordered on `st`, like the long-pair launch's scratch; launch(mem,
// next, blocks) enqueues the kernel.
extern "C++" {
template <class PerCu, class Launch>
static int trace_grid_launch(msw_ctx* ctx, uint64_t n_pairs, uint64_t block_bytes, hipStream_t st, PerCu per_cu,
                             Launch launch) {
    uint64_t resident = 0;
    if (block_bytes) {
        const int k = per_cu();
        if (k <= 0) return fail(MSW_E_DEVICE, "traceback kernel does not fit a CU");
        resident = (uint64_t)(ctx->cu_count > 0 ? ctx->cu_count : 256) * (uint64_t)k;
    }
    // MSW_TRACE_BLOCKS: tests fix the block count
    const uint64_t blocks = msw::trace_grid_cap(n_pairs, resident, block_bytes, ctx->opt.trace_blocks);
    const bool queue = blocks < n_pairs;
    uint8_t* mem = nullptr;
    uint32_t* next = nullptr;
    if (block_bytes || queue) {
        HIP_TRY(hipMallocAsync((void**)&mem, blocks * block_bytes + 256, st));
        if (queue) {
            next = reinterpret_cast<uint32_t*>(mem + blocks * block_bytes);
            const hipError_t em = hipMemsetAsync(next, 0, sizeof(uint32_t), st);
            if (em != hipSuccess) {
                (void)hipFreeAsync(mem, st);
                HIP_TRY(em);
            }
        }
    }
    const hipError_t e = launch(block_bytes ? mem : nullptr, next, (uint32_t)blocks);
    if (mem) HIP_TRY(hipFreeAsync(mem, st));
    HIP_TRY(e);
    return MSW_OK;
}
}  // extern "C++"

// sw_trace_kernel: the direction words of the whole rectangle, in LDS while
// the bound's rectangle fits, else in a global slab per block.
static int run_trace(msw_ctx* ctx, const Scheme& sch, const msw_scoring_t* sc, msw::TraceParams p, uint64_t n_pairs,
                     uint32_t max_read_len, uint32_t max_win_len, hipStream_t st) {
    trace_call_params(p, sc, n_pairs, max_read_len, max_win_len);
    const size_t shm = msw::trace_lds_layout(p, sch.affine);
    const uint64_t need = msw::trace_words(sch.affine, max_read_len, max_win_len);
    const uint64_t slab_bytes = need > p.lds_words ? need * sizeof(uint32_t) : 0;
    return trace_grid_launch(
        ctx, n_pairs, slab_bytes, st, [&] { return msw::trace_blocks_per_cu(sch.affine, max_read_len, shm); },
        [&](uint8_t* mem, uint32_t* next, uint32_t blocks) {
            p.slab = reinterpret_cast<uint32_t*>(mem);
            p.slab_words = mem ? need : 0;
            p.next = next;
            return msw::launch_sw_trace(p, sch.affine, blocks, shm, st);
        });
}

// sw_trace_long_kernel: bounds past the packed range (or MSW_FORCE_LONG);
// every block has its checkpoint rows, strip slab and op buffer in scratch.
static int run_trace_long(msw_ctx* ctx, const Scheme& sch, const msw_scoring_t* sc, msw::TraceParams p,
                          uint64_t n_pairs, uint32_t max_read_len, uint32_t max_win_len, hipStream_t st) {
    trace_call_params(p, sc, n_pairs, max_read_len, max_win_len);
    const msw::TraceLongLayout l = msw::trace_long_layout(sch.affine, max_read_len, max_win_len, p.cigar_stride);
    p.win_bytes = l.win_bytes;
    p.ops_cap = l.ops_cap;
    msw::TraceLongParams q;
    memset(&q, 0, sizeof(q));
    q.block_bytes = l.block_bytes;
    q.slab_off = l.slab_off;
    q.ops_off = l.ops_off;
    q.ckpt_cols = l.ckpt_cols;
    q.slab_w = l.slab_w;
    q.ops_in_lds = l.ops_in_lds;
    return trace_grid_launch(
        ctx, n_pairs, l.block_bytes, st,
        [&] { return msw::trace_long_blocks_per_cu(sch.affine, max_read_len, l.lds_bytes); },
        [&](uint8_t* mem, uint32_t* next, uint32_t blocks) {
            q.t = p;
            q.t.next = next;
            q.scratch = mem;
            return msw::launch_sw_trace_long(q, sch.affine, blocks, l.lds_bytes, st);
        });
}

// The kernel a traceback call runs on: the *_long calls leave the packed range
// (or take MSW_FORCE_LONG) as msw_align_batch_device does for scoring.
static int run_trace_any(msw_ctx* ctx, const Scheme& sch, const msw_scoring_t* sc, const msw::TraceParams& p,
                         uint64_t n_pairs, uint32_t max_read_len, uint32_t max_win_len, hipStream_t st,
                         bool long_pairs) {
    if (long_pairs && (ctx->opt.force_long || is_long(max_read_len, max_win_len)))
        return run_trace_long(ctx, sch, sc, p, n_pairs, max_read_len, max_win_len, st);
    return run_trace(ctx, sch, sc, p, n_pairs, max_read_len, max_win_len, st);
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

static int trace_batch_device(msw_ctx* ctx, const msw_scoring_t* sc, const msw_batch_t* b, const msw_out_t* ends,
                              msw_trace_t* tr, uint32_t max_read_len, uint32_t max_win_len, void* stream,
                              bool long_pairs) {
    if (!ctx) return fail(MSW_E_INVALID, "ctx is NULL");
    Scheme sch;
    int rc;
    if ((rc = make_scheme(sc, ctx->opt, &sch))) return rc;
    sch.coords = true;  // want_coords is not read: the ends are an input here
    if ((rc = validate_batch(b, ends, sch)) || (rc = validate_trace(tr))) return rc;
    if (b->n_pairs == 0) return MSW_OK;
    if ((rc = check_trace_bounds(sch, max_read_len, max_win_len, long_pairs))) return rc;
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
    return run_trace_any(ctx, sch, sc, p, b->n_pairs, max_read_len, max_win_len, st, long_pairs);
}

int msw_trace_batch_device(msw_ctx* ctx, const msw_scoring_t* sc, const msw_batch_t* b, const msw_out_t* ends,
                           msw_trace_t* tr, uint32_t max_read_len, uint32_t max_win_len, void* stream) {
    return trace_batch_device(ctx, sc, b, ends, tr, max_read_len, max_win_len, stream, false);
}

int msw_trace_long_batch_device(msw_ctx* ctx, const msw_scoring_t* sc, const msw_batch_t* b, const msw_out_t* ends,
                                msw_trace_t* tr, uint32_t max_read_len, uint32_t max_win_len, void* stream) {
    return trace_batch_device(ctx, sc, b, ends, tr, max_read_len, max_win_len, stream, true);
}

static int trace_reads_device(msw_ctx* ctx, const msw_scoring_t* sc, const msw_genome* g, const uint8_t* reads,
                              const uint16_t* read_len, uint32_t read_stride, const int64_t* win_pos, uint64_t n,
                              uint32_t window, uint32_t max_read_len, const msw_out_t* ends, msw_trace_t* tr,
                              void* stream, bool long_pairs) {
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
    if ((rc = check_trace_bounds(sch, max_read_len, max_win, long_pairs))) return rc;
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
    return run_trace_any(ctx, sch, sc, p, n, max_read_len, max_win, st, long_pairs);
}

int msw_trace_reads_device(msw_ctx* ctx, const msw_scoring_t* sc, const msw_genome* g, const uint8_t* reads,
                           const uint16_t* read_len, uint32_t read_stride, const int64_t* win_pos, uint64_t n,
                           uint32_t window, uint32_t max_read_len, const msw_out_t* ends, msw_trace_t* tr,
                           void* stream) {
    return trace_reads_device(ctx, sc, g, reads, read_len, read_stride, win_pos, n, window, max_read_len, ends, tr,
                              stream, false);
}

int msw_trace_reads_long_device(msw_ctx* ctx, const msw_scoring_t* sc, const msw_genome* g, const uint8_t* reads,
                                const uint16_t* read_len, uint32_t read_stride, const int64_t* win_pos, uint64_t n,
                                uint32_t window, uint32_t max_read_len, const msw_out_t* ends, msw_trace_t* tr,
                                void* stream) {
    return trace_reads_device(ctx, sc, g, reads, read_len, read_stride, win_pos, n, window, max_read_len, ends, tr,
                              stream, true);
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

static int align_batch_trace(msw_ctx* ctx, const msw_scoring_t* sc, const msw_batch_t* b, msw_out_t* out,
                             msw_trace_t* tr, uint64_t chunk_pairs, bool long_pairs) {
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
    if ((rc = check_trace_bounds(sch, max_m, max_n, long_pairs))) return rc;
    if (max_m > b->read_stride || max_n > b->win_stride) return fail(MSW_E_INVALID, "a length exceeds its stride");
    if ((rc = set_device(ctx))) return rc;
    // Simple and synchronous: per chunk upload, score with coordinates, trace,
    // download (not part of the three-slot staging pipeline).
    const uint64_t chunk = std::min<uint64_t>(n, chunk_pairs ? chunk_pairs : 65536);
    const size_t rs = b->read_stride, ws = b->win_stride, cs = tr->cigar_stride;
    DeviceArena a;
    const auto d_reads = a.take<uint8_t>(chunk * rs), d_wins = a.take<uint8_t>(chunk * ws);
    const auto d_cig = a.take<uint32_t>(chunk * cs);
    const auto d_score = a.take<int32_t>(chunk), d_nc = a.take<int32_t>(chunk);
    const auto d_rl = a.take<uint16_t>(chunk), d_wl = a.take<uint16_t>(chunk);
    const auto d_ei = a.take<int16_t>(chunk), d_ej = a.take<int16_t>(chunk), d_si = a.take<int16_t>(chunk),
               d_sj = a.take<int16_t>(chunk);
    if ((rc = a.alloc())) return rc;
    ChunkCopy cp(ctx->compute);
    hipStream_t st = cp.st;
    for (uint64_t lo = 0; lo < n && rc == MSW_OK && cp.ok(); lo += chunk) {
        const uint64_t c = std::min(chunk, n - lo);
        uint32_t cm = 0, cn = 0;
        max_u16(b->read_len + lo, c, cm);
        max_u16(b->win_len + lo, c, cn);
        cp.up(d_reads, b->reads + lo * rs, c * rs);
        cp.up(d_wins, b->wins + lo * ws, c * ws);
        cp.up(d_rl, b->read_len + lo, c * 2);
        cp.up(d_wl, b->win_len + lo, c * 2);
        if (!cp.ok()) break;
        msw_batch_t db = {d_reads, d_wins, d_rl, d_wl, (uint32_t)rs, (uint32_t)ws, c};
        msw_out_t dout = {d_score, d_ei, d_ej};
        msw_trace_t dtr = {d_si, d_sj, d_nc, d_cig, (uint32_t)cs};
        if ((rc = msw_align_batch_device(ctx, &scc, &db, &dout, cm, cn, st))) break;
        // same stream: the trace reads the ends the scoring launch wrote
        if ((rc = trace_batch_device(ctx, &scc, &db, &dout, &dtr, cm, cn, st, long_pairs))) break;
        cp.down(out->score + lo, d_score, c * 4);
        cp.down(out->end_i + lo, d_ei, c * 2);
        cp.down(out->end_j + lo, d_ej, c * 2);
        cp.down(tr->start_i + lo, d_si, c * 2);
        cp.down(tr->start_j + lo, d_sj, c * 2);
        cp.down(tr->n_cigar + lo, d_nc, c * 4);
        if (cs) cp.down(tr->cigar + lo * cs, d_cig, c * cs * 4);
        cp.sync();
    }
    return cp.finish(rc, "traceback");
}

int msw_align_batch_trace(msw_ctx* ctx, const msw_scoring_t* sc, const msw_batch_t* b, msw_out_t* out,
                          msw_trace_t* tr, uint64_t chunk_pairs) {
    return align_batch_trace(ctx, sc, b, out, tr, chunk_pairs, false);
}

int msw_align_batch_trace_long(msw_ctx* ctx, const msw_scoring_t* sc, const msw_batch_t* b, msw_out_t* out,
                               msw_trace_t* tr, uint64_t chunk_pairs) {
    return align_batch_trace(ctx, sc, b, out, tr, chunk_pairs, true);
}

// The body of msw_align_reads_trace (strand == NULL: aln required) and of
// msw_align_reads_strands (strand != NULL: both orientations are scored, the
// trace and the pack read the oriented rows, and aln may be NULL for scores
// alone, with coordinates as sc says).
static int reads_records(msw_ctx* ctx, const msw_scoring_t* sc, const msw_genome* g, const msw_read_batch_t* b,
                         msw_out_t* out, msw_aln_t* aln, uint8_t* strand, bool both, uint64_t chunk_pairs,
                         bool long_pairs = false) {
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
        if ((rc = check_trace_bounds(sch, max_m, max_n, long_pairs))) return rc;
    } else if ((rc = check_bounds(sch, max_m, max_n))) {
        return rc;
    }
    if (max_m > b->read_stride) return fail(MSW_E_INVALID, "a length exceeds its stride");
    if ((rc = set_device(ctx))) return rc;
    // Simple and synchronous, like msw_align_batch_trace: per chunk upload,
    // cut, score with coordinates, trace, pack, download.  The trace stride is
    // exact (no alignment has more ops than rows + columns), so no read
    // overflows; the packed ops of a chunk are pulled once its total is known.
    const size_t rs = b->read_stride, ws = std::max<size_t>(16, (max_n + 15u) & ~15u),
                 cs = aln ? (size_t)max_m + max_n : 0;
    uint64_t chunk = std::min<uint64_t>(n, chunk_pairs ? chunk_pairs : 65536);
    // past the packed range the exact stride reaches 65,534 ops: a chunk's trace rows stay within 1 GiB
    if (long_pairs && is_long(max_m, max_n))
        chunk = std::min<uint64_t>(chunk, std::max<uint64_t>(1, (1ull << 30) / (cs * 4)));
    DeviceArena a;
    const auto d_reads = a.take<uint8_t>(chunk * rs), d_wins = a.take<uint8_t>(chunk * ws);
    const auto d_rows = a.take<uint32_t>(chunk * cs);
    const auto d_pos = a.take<int64_t>(chunk), d_ref = a.take<int64_t>(chunk);
    const auto d_score = a.take<int32_t>(chunk), d_nc = a.take<int32_t>(chunk), d_nm = a.take<int32_t>(chunk);
    const auto d_off = a.take<uint32_t>(chunk + 2);
    const auto d_rl = a.take<uint16_t>(chunk), d_want = a.take<uint16_t>(chunk), d_wl = a.take<uint16_t>(chunk);
    const auto d_ei = a.take<int16_t>(chunk), d_ej = a.take<int16_t>(chunk), d_si = a.take<int16_t>(chunk),
               d_sj = a.take<int16_t>(chunk);
    // both strands: the chunk's oriented rows [chunk][ors] and its strand bytes
    const size_t ors = std::max<size_t>(16, (max_m + 15u) & ~15u);
    const auto d_or = a.take<uint8_t>(both ? chunk * ors : 0), d_strand = a.take<uint8_t>(both ? chunk : 0);
    RecordOps ops;
    if ((rc = a.alloc()) || (rc = ops.alloc(aln ? chunk * 8 : 1))) return rc;
    ChunkCopy cp(ctx->compute);
    hipStream_t st = cp.st;
    for (uint64_t lo = 0; lo < n && rc == MSW_OK && cp.ok(); lo += chunk) {
        const uint64_t c = std::min(chunk, n - lo);
        uint32_t cm = 0, cn = 0;
        max_u16(b->read_len + lo, c, cm);
        max_u16(b->win_len + lo, c, cn);
        cp.up(d_reads, b->reads + lo * rs, c * rs);
        cp.up(d_rl, b->read_len + lo, c * 2);
        cp.up(d_want, b->win_len + lo, c * 2);
        cp.up(d_pos, b->win_pos + lo, c * 8);
        if (!cp.ok()) break;
        if ((rc = msw_genome_cut_device(ctx, g, d_pos, d_want, c, d_wins, (uint32_t)ws, d_wl, st))) break;
        msw_batch_t db = {d_reads, d_wins, d_rl, d_wl, (uint32_t)rs, (uint32_t)ws, c};
        msw_out_t dout = {d_score, d_ei, d_ej};
        msw_trace_t dtr = {d_si, d_sj, d_nc, d_rows, (uint32_t)cs};
        if (both) {
            rc = score_both_strands(ctx, &scc, &db, &dout, d_strand, d_or, (uint32_t)ors, st,
                                    [&](const msw_batch_t* pb, msw_out_t* po) {
                                        return msw_align_batch_device(ctx, &scc, pb, po, cm, cn, st);
                                    });
            if (rc) break;
            cp.down(strand + lo, d_strand, c);
            // from here on the reads are the oriented rows
            db.reads = d_or;
            db.read_stride = (uint32_t)ors;
            if (!aln) {
                cp.down(out->score + lo, d_score, c * 4);
                if (coords) {
                    cp.down(out->end_i + lo, d_ei, c * 2);
                    cp.down(out->end_j + lo, d_ej, c * 2);
                }
                cp.sync();
                continue;
            }
        } else if ((rc = msw_align_batch_device(ctx, &scc, &db, &dout, cm, cn, st))) {
            break;
        }
        if ((rc = trace_batch_device(ctx, &scc, &db, &dout, &dtr, cm, cn, st, long_pairs))) break;
        const ChunkRecords rec = {db.reads, db.read_stride, d_rl, d_pos, &dout, &dtr, d_ref, d_nm, d_off};
        if ((rc = pack_chunk_records(ctx, g, cp, ops, rec, lo, c,
                                     {{out->score + lo, d_score, c * 4},
                                      {out->end_i + lo, d_ei, c * 2},
                                      {out->end_j + lo, d_ej, c * 2}},
                                     aln)))
            break;
        cp.sync();
    }
    return cp.finish(rc, "alignment records");
}

int msw_align_reads_trace(msw_ctx* ctx, const msw_scoring_t* sc, const msw_genome* g, const msw_read_batch_t* b,
                          msw_out_t* out, msw_aln_t* aln, uint64_t chunk_pairs) {
    return reads_records(ctx, sc, g, b, out, aln, nullptr, false, chunk_pairs);
}

int msw_align_reads_trace_long(msw_ctx* ctx, const msw_scoring_t* sc, const msw_genome* g,
                               const msw_read_batch_t* b, msw_out_t* out, msw_aln_t* aln, uint64_t chunk_pairs) {
    return reads_records(ctx, sc, g, b, out, aln, nullptr, false, chunk_pairs, true);
}

int msw_align_reads_strands(msw_ctx* ctx, const msw_scoring_t* sc, const msw_genome* g, const msw_read_batch_t* b,
                            msw_out_t* out, uint8_t* strand, msw_aln_t* aln, uint64_t chunk_pairs) {
    return reads_records(ctx, sc, g, b, out, aln, strand, true, chunk_pairs);
}

}  // extern "C"
