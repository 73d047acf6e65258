// msw_rt_band.cpp -- banded alignment (include/msw.h, "Banded alignment" and
// "Banded end-to-end alignment"): the limit checks, the two device calls and
// their chunked host drivers, each once for both modes (`e2e` picks the
// kernel).  The kernels: msw_band.hip, msw_e2e.hip.
#include "msw_runtime_internal.h"
#include "msw_trace_sizes.h"

using namespace msw_detail;

// What every banded call checks before it touches the device.
static int check_band(const msw_scoring_t* sc, const msw_out_t* out, const msw_trace_t* tr, uint32_t w,
                      uint32_t max_read_len, bool* coords) {
    if (!sc) return fail(MSW_E_INVALID, "scoring is NULL");
    if (!out || !out->score) return fail(MSW_E_INVALID, "out->score is NULL");
    *coords = sc->want_coords != 0 || tr;
    if (*coords && (!out->end_i || !out->end_j)) return fail(MSW_E_INVALID, "end_i / end_j is NULL");
    int rc;
    if (tr && (rc = validate_trace(tr))) return rc;
    if (w > msw::kBandMaxW) return fail(MSW_E_RANGE, "banded: w %u > %u", w, msw::kBandMaxW);
    if (max_read_len > (uint32_t)msw::kMaxLongLen || max_read_len + 2 * w > (uint32_t)msw::kMaxLongLen)
        return fail(MSW_E_RANGE, "banded: read length %u + 2 x %u > %d", max_read_len, w, msw::kMaxLongLen);
    if (tr && max_read_len > msw::kBandTraceMaxRows)
        return fail(MSW_E_RANGE, "banded traceback: read length %u > %u (direction codes are kept in LDS)",
                    max_read_len, msw::kBandTraceMaxRows);
    return MSW_OK;
}

static void band_call_params(msw::BandParams& p, const msw_scoring_t* sc, uint64_t n, uint32_t w,
                             uint32_t max_read_len, const msw_out_t* out, const msw_trace_t* tr, bool coords) {
    p.n_pairs = (uint32_t)n;
    p.w = w;
    p.max_rows = max_read_len;
    p.match = sc->match;
    p.mismatch = sc->mismatch;
    p.gap = sc->gap_extend;
    p.goe = sc->gap_open + sc->gap_extend;
    p.score = out->score;
    p.end_i = coords ? out->end_i : nullptr;
    p.end_j = coords ? out->end_j : nullptr;
    if (tr) {
        p.start_i = tr->start_i;
        p.start_j = tr->start_j;
        p.n_cigar = tr->n_cigar;
        p.cigar = tr->cigar;
        p.cigar_stride = tr->cigar_stride;
    }
}

static hipError_t launch_band(const msw::BandParams& p, bool e2e, bool affine, int mode, hipStream_t st) {
    return e2e ? msw::launch_sw_band_e2e(p, affine, mode, st) : msw::launch_sw_band(p, affine, mode, st);
}

static int batch_banded_device(bool e2e, msw_ctx* ctx, const msw_scoring_t* sc, const msw_batch_t* b,
                               const int32_t* diag, uint32_t w, msw_out_t* out, msw_trace_t* tr,
                               uint32_t max_read_len, void* stream) {
    if (!ctx) return fail(MSW_E_INVALID, "ctx is NULL");
    if (!b) return fail(MSW_E_INVALID, "batch is NULL");
    bool coords = false;
    Scheme sch;
    int rc;
    if ((rc = check_band(sc, out, tr, w, max_read_len, &coords)) || (rc = make_scheme(sc, ctx->opt, &sch))) return rc;
    if (b->n_pairs == 0) return MSW_OK;
    if (!b->reads || !b->wins || !b->read_len || !b->win_len || !diag) return fail(MSW_E_INVALID, "NULL array");
    if (b->n_pairs > 0x7FFFFFFFull) return fail(MSW_E_RANGE, "banded: n_pairs > 2^31-1 in one call");
    if (max_read_len > b->read_stride) return fail(MSW_E_INVALID, "max_read_len exceeds read_stride");
    if ((rc = set_device(ctx))) return rc;
    msw::BandParams p;
    memset(&p, 0, sizeof(p));
    p.reads = b->reads;
    p.read_len = b->read_len;
    p.read_stride = b->read_stride;
    p.wins = b->wins;
    p.win_len = b->win_len;
    p.win_stride = b->win_stride;
    p.diag32 = diag;
    band_call_params(p, sc, b->n_pairs, w, max_read_len, out, tr, coords);
    HIP_TRY(launch_band(p, e2e, sch.affine, tr ? 2 : (coords ? 1 : 0), call_stream(ctx, stream)));
    return MSW_OK;
}

static int reads_banded_device(bool e2e, msw_ctx* ctx, const msw_scoring_t* sc, const msw_genome* g,
                               const uint8_t* reads, const uint16_t* read_len, uint32_t read_stride,
                               const int64_t* diag, uint64_t n, uint32_t w, uint32_t max_read_len, msw_out_t* out,
                               int64_t* win_pos_out, uint16_t* win_len_out, msw_trace_t* tr, void* stream) {
    if (!ctx || !g) return fail(MSW_E_INVALID, "ctx/genome is NULL");
    if (g->ctx != ctx) return fail(MSW_E_INVALID, "genome belongs to another context");
    bool coords = false;
    Scheme sch;
    int rc;
    if ((rc = check_band(sc, out, tr, w, max_read_len, &coords)) || (rc = make_scheme(sc, ctx->opt, &sch))) return rc;
    if (n == 0) return MSW_OK;
    if (!reads || !read_len || !diag) return fail(MSW_E_INVALID, "NULL array");
    if (n > 0x7FFFFFFFull) return fail(MSW_E_RANGE, "banded: n > 2^31-1 in one call");
    if (max_read_len > read_stride) return fail(MSW_E_INVALID, "max_read_len exceeds read_stride");
    if ((rc = set_device(ctx))) return rc;
    msw::BandParams p;
    memset(&p, 0, sizeof(p));
    p.reads = reads;
    p.read_len = read_len;
    p.read_stride = read_stride;
    p.genome = g->d_seq;
    p.glen = g->len;
    p.diag64 = diag;
    p.win_pos_out = win_pos_out;
    p.win_len_out = win_len_out;
    band_call_params(p, sc, n, w, max_read_len, out, tr, coords);
    HIP_TRY(launch_band(p, e2e, sch.affine, tr ? 2 : (coords ? 1 : 0), call_stream(ctx, stream)));
    return MSW_OK;
}

// Both host drivers: per chunk upload, one launch, download; simple and
// synchronous like msw_align_batch_trace.  g == NULL: the padded form.
static int banded_host(bool e2e, msw_ctx* ctx, const msw_scoring_t* sc, const msw_genome* g, const uint8_t* reads,
                       const uint16_t* read_len, size_t rs, const uint8_t* wins, const uint16_t* win_len, size_t ws,
                       const int32_t* diag32, const int64_t* diag64, uint64_t n, uint32_t w, msw_out_t* out,
                       int64_t* win_pos_out, uint16_t* win_len_out, msw_trace_t* tr, uint64_t chunk_pairs) {
    if (!ctx) return fail(MSW_E_INVALID, "ctx is NULL");
    uint32_t max_m = 0;
    if (n && !read_len) return fail(MSW_E_INVALID, "NULL array in batch");
    max_u16(read_len, n, max_m);
    bool coords = false;
    int rc;
    if ((rc = check_band(sc, out, tr, w, max_m, &coords))) return rc;
    if (n == 0) return MSW_OK;
    if (!reads || (g ? !diag64 : (!wins || !win_len || !diag32))) return fail(MSW_E_INVALID, "NULL array in batch");
    if (max_m > rs) return fail(MSW_E_INVALID, "a length exceeds its stride");
    if (!g) {
        uint32_t max_n = 0;
        max_u16(win_len, n, max_n);
        if (max_n > ws) return fail(MSW_E_INVALID, "a length exceeds its stride");
    }
    if ((rc = set_device(ctx))) return rc;
    const uint64_t chunk = std::min<uint64_t>(n, chunk_pairs ? chunk_pairs : 65536);
    const size_t cs = tr ? tr->cigar_stride : 0;
    DeviceArena a;
    const auto d_reads = a.take<uint8_t>(chunk * rs), d_wins = a.take<uint8_t>(g ? 0 : chunk * ws);
    const auto d_cig = a.take<uint32_t>(chunk * cs);
    const auto d_d64 = a.take<int64_t>(g ? chunk : 0), d_pos = a.take<int64_t>(g ? chunk : 0);
    const auto d_d32 = a.take<int32_t>(g ? 0 : chunk);
    const auto d_score = a.take<int32_t>(chunk), d_nc = a.take<int32_t>(chunk);
    const auto d_rl = a.take<uint16_t>(chunk), d_wl = a.take<uint16_t>(chunk);
    const auto d_ei = a.take<int16_t>(chunk), d_ej = a.take<int16_t>(chunk), d_si = a.take<int16_t>(chunk),
               d_sj = a.take<int16_t>(chunk);
    if ((rc = a.alloc())) return rc;
    ChunkCopy cp(ctx->compute);
    hipStream_t st = cp.st;
    for (uint64_t lo = 0; lo < n && rc == MSW_OK && cp.ok(); lo += chunk) {
        const uint64_t c = std::min(chunk, n - lo);
        uint32_t cm = 0;
        max_u16(read_len + lo, c, cm);
        cp.up(d_reads, reads + lo * rs, c * rs);
        cp.up(d_rl, read_len + lo, c * 2);
        if (g) {
            cp.up(d_d64, diag64 + lo, c * 8);
        } else {
            cp.up(d_wins, wins + lo * ws, c * ws);
            cp.up(d_wl, win_len + lo, c * 2);
            cp.up(d_d32, diag32 + lo, c * 4);
        }
        if (!cp.ok()) break;
        msw_out_t dout = {d_score, d_ei, d_ej};
        msw_trace_t dtr = {d_si, d_sj, d_nc, d_cig, (uint32_t)cs};
        if (g) {
            rc = reads_banded_device(e2e, ctx, sc, g, d_reads, d_rl, (uint32_t)rs, d_d64, c, w, cm, &dout, d_pos, d_wl,
                                     tr ? &dtr : nullptr, st);
        } else {
            msw_batch_t db = {d_reads, d_wins, d_rl, d_wl, (uint32_t)rs, (uint32_t)ws, c};
            rc = batch_banded_device(e2e, ctx, sc, &db, d_d32, w, &dout, tr ? &dtr : nullptr, cm, st);
        }
        if (rc) break;
        cp.down(out->score + lo, d_score, c * 4);
        if (coords) {
            cp.down(out->end_i + lo, d_ei, c * 2);
            cp.down(out->end_j + lo, d_ej, c * 2);
        }
        if (g && win_pos_out) cp.down(win_pos_out + lo, d_pos, c * 8);
        if (g && win_len_out) cp.down(win_len_out + lo, d_wl, c * 2);
        if (tr) {
            cp.down(tr->start_i + lo, d_si, c * 2);
            cp.down(tr->start_j + lo, d_sj, c * 2);
            cp.down(tr->n_cigar + lo, d_nc, c * 4);
            if (cs) cp.down(tr->cigar + lo * cs, d_cig, c * cs * 4);
        }
        cp.sync();
    }
    return cp.finish(rc, "banded alignment");
}

static int batch_banded_host(bool e2e, msw_ctx* ctx, const msw_scoring_t* sc, const msw_batch_t* b,
                             const int32_t* diag, uint32_t w, msw_out_t* out, msw_trace_t* tr, uint64_t chunk_pairs) {
    if (!b) return fail(MSW_E_INVALID, "batch is NULL");
    return banded_host(e2e, ctx, sc, nullptr, b->reads, b->read_len, b->read_stride, b->wins, b->win_len,
                       b->win_stride, diag, nullptr, b->n_pairs, w, out, nullptr, nullptr, tr, chunk_pairs);
}

static int reads_banded_host(bool e2e, msw_ctx* ctx, const msw_scoring_t* sc, const msw_genome* g,
                             const msw_read_batch_t* b, uint32_t w, msw_out_t* out, int64_t* win_pos_out,
                             uint16_t* win_len_out, msw_trace_t* tr, uint64_t chunk_pairs) {
    if (!g) return fail(MSW_E_INVALID, "genome is NULL");
    if (!b) return fail(MSW_E_INVALID, "batch is NULL");
    return banded_host(e2e, ctx, sc, g, b->reads, b->read_len, b->read_stride, nullptr, nullptr, 0, nullptr,
                       b->win_pos, b->n_pairs, w, out, win_pos_out, win_len_out, tr, chunk_pairs);
}

extern "C" {

int msw_align_batch_banded_device(msw_ctx* ctx, const msw_scoring_t* sc, const msw_batch_t* b, const int32_t* diag,
                                  uint32_t w, msw_out_t* out, msw_trace_t* tr, uint32_t max_read_len, void* stream) {
    return batch_banded_device(false, ctx, sc, b, diag, w, out, tr, max_read_len, stream);
}
int msw_align_batch_banded_e2e_device(msw_ctx* ctx, const msw_scoring_t* sc, const msw_batch_t* b,
                                      const int32_t* diag, uint32_t w, msw_out_t* out, msw_trace_t* tr,
                                      uint32_t max_read_len, void* stream) {
    return batch_banded_device(true, ctx, sc, b, diag, w, out, tr, max_read_len, stream);
}

int msw_align_reads_banded_device(msw_ctx* ctx, const msw_scoring_t* sc, const msw_genome* g, const uint8_t* reads,
                                  const uint16_t* read_len, uint32_t read_stride, const int64_t* diag, uint64_t n,
                                  uint32_t w, uint32_t max_read_len, msw_out_t* out, int64_t* win_pos_out,
                                  uint16_t* win_len_out, msw_trace_t* tr, void* stream) {
    return reads_banded_device(false, ctx, sc, g, reads, read_len, read_stride, diag, n, w, max_read_len, out,
                               win_pos_out, win_len_out, tr, stream);
}
int msw_align_reads_banded_e2e_device(msw_ctx* ctx, const msw_scoring_t* sc, const msw_genome* g,
                                      const uint8_t* reads, const uint16_t* read_len, uint32_t read_stride,
                                      const int64_t* diag, uint64_t n, uint32_t w, uint32_t max_read_len,
                                      msw_out_t* out, int64_t* win_pos_out, uint16_t* win_len_out, msw_trace_t* tr,
                                      void* stream) {
    return reads_banded_device(true, ctx, sc, g, reads, read_len, read_stride, diag, n, w, max_read_len, out,
                               win_pos_out, win_len_out, tr, stream);
}

int msw_align_batch_banded(msw_ctx* ctx, const msw_scoring_t* sc, const msw_batch_t* b, const int32_t* diag,
                           uint32_t w, msw_out_t* out, msw_trace_t* tr, uint64_t chunk_pairs) {
    return batch_banded_host(false, ctx, sc, b, diag, w, out, tr, chunk_pairs);
}
int msw_align_batch_banded_e2e(msw_ctx* ctx, const msw_scoring_t* sc, const msw_batch_t* b, const int32_t* diag,
                               uint32_t w, msw_out_t* out, msw_trace_t* tr, uint64_t chunk_pairs) {
    return batch_banded_host(true, ctx, sc, b, diag, w, out, tr, chunk_pairs);
}

int msw_align_reads_banded(msw_ctx* ctx, const msw_scoring_t* sc, const msw_genome* g, const msw_read_batch_t* b,
                           uint32_t w, msw_out_t* out, int64_t* win_pos_out, uint16_t* win_len_out, msw_trace_t* tr,
                           uint64_t chunk_pairs) {
    return reads_banded_host(false, ctx, sc, g, b, w, out, win_pos_out, win_len_out, tr, chunk_pairs);
}
int msw_align_reads_banded_e2e(msw_ctx* ctx, const msw_scoring_t* sc, const msw_genome* g,
                               const msw_read_batch_t* b, uint32_t w, msw_out_t* out, int64_t* win_pos_out,
                               uint16_t* win_len_out, msw_trace_t* tr, uint64_t chunk_pairs) {
    return reads_banded_host(true, ctx, sc, g, b, w, out, win_pos_out, win_len_out, tr, chunk_pairs);
}

}  // extern "C"
