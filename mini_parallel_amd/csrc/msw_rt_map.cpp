// msw_rt_map.cpp -- placing reads (include/msw.h, "Placing reads",
// "Candidates and mapping quality", "Pairs"): the k-mer index, seeding, the
// candidates and their MAPQ selection, the pair calls, and the chunked host
// drivers msw_seed_reads, msw_seed_candidates, msw_map_reads, msw_map_pairs.
// The kernels: msw_seed.hip, msw_mapq.hip, msw_pair.hip.
#include "msw_runtime_internal.h"

using namespace msw_detail;

extern "C" {

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

// The body of msw_seed_reads (alt == NULL) and of msw_seed_candidates (cands):
// simple and synchronous, like msw_align_batch_trace: per chunk upload,
// reverse complement, seed, download.
static int seed_host(msw_ctx* ctx, const msw_index* x, const msw_read_batch_t* b, int both,
                     const msw_seed_params_t* sp, bool cands, uint32_t sep, const msw_seed_out_t* out,
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
    if (cands && sep != 0 && sep < sp->band)
        return fail(MSW_E_RANGE, "candidates: sep %u is below band %u", sep, sp->band);
    if (n == 0) return MSW_OK;
    if (!b->reads || !out || !out->win_pos || !out->votes || !out->hits || !out->flags ||
        (cands && (!alt || !alt->win_pos || !alt->votes || !alt->flags)))
        return fail(MSW_E_INVALID, "NULL array");
    if (b->read_stride == 0 || max_m > b->read_stride) return fail(MSW_E_INVALID, "a length exceeds its stride");
    if ((rc = set_device(ctx))) return rc;
    const uint64_t chunk = std::min<uint64_t>(n, chunk_reads ? chunk_reads : 65536), alt_chunk = cands ? chunk : 0;
    const size_t rs = b->read_stride, os = round16((uint32_t)std::max<uint32_t>(max_m, 1));
    DeviceArena a;
    const auto d_reads = a.take<uint8_t>(chunk * rs), d_rc = a.take<uint8_t>(both ? chunk * os : 0);
    const auto d_wp = a.take<int64_t>(chunk), d_wp1 = a.take<int64_t>(alt_chunk);
    const auto d_votes = a.take<uint32_t>(chunk), d_hits = a.take<uint32_t>(chunk), d_votes1 = a.take<uint32_t>(alt_chunk);
    const auto d_rl = a.take<uint16_t>(chunk);
    const auto d_fl = a.take<uint8_t>(chunk), d_fl1 = a.take<uint8_t>(alt_chunk);
    if ((rc = a.alloc())) return rc;
    ChunkCopy cp(ctx->compute);
    hipStream_t st = cp.st;
    for (uint64_t lo = 0; lo < n && rc == MSW_OK && cp.ok(); lo += chunk) {
        const uint64_t c = std::min(chunk, n - lo);
        const msw_seed_out_t dout = {d_wp, d_votes, d_hits, d_fl};
        const msw_seed_alt_t dalt = {d_wp1, d_votes1, d_fl1};
        const uint8_t* rc_rows = both ? (const uint8_t*)d_rc : nullptr;
        cp.up(d_reads, b->reads + lo * rs, c * rs);
        cp.up(d_rl, b->read_len + lo, c * 2);
        if (!cp.ok()) break;
        if (both && (rc = msw_revcomp_device(ctx, d_reads, d_rl, (uint32_t)rs, c, d_rc, (uint32_t)os, st))) break;
        rc = cands ? msw_seed_candidates_device(ctx, x, d_reads, rc_rows, d_rl, (uint32_t)rs, (uint32_t)os, c, max_m, sp,
                                                sep, &dout, &dalt, st)
                   : msw_seed_reads_device(ctx, x, d_reads, rc_rows, d_rl, (uint32_t)rs, (uint32_t)os, c, max_m, sp, &dout,
                                           st);
        if (rc) break;
        cp.down(out->win_pos + lo, d_wp, c * 8);
        cp.down(out->votes + lo, d_votes, c * 4);
        cp.down(out->hits + lo, d_hits, c * 4);
        cp.down(out->flags + lo, d_fl, c);
        if (cands) {
            cp.down(alt->win_pos + lo, d_wp1, c * 8);
            cp.down(alt->votes + lo, d_votes1, c * 4);
            cp.down(alt->flags + lo, d_fl1, c);
        }
        cp.sync();
    }
    return cp.finish(rc, cands ? "candidates" : "seeding");
}

int msw_seed_reads(msw_ctx* ctx, const msw_index* x, const msw_read_batch_t* b, int both,
                   const msw_seed_params_t* sp, const msw_seed_out_t* out, uint64_t chunk_reads) {
    return seed_host(ctx, x, b, both, sp, false, 0, out, nullptr, chunk_reads);
}

// Host memory, synchronous, chunked like msw_seed_reads.
int msw_seed_candidates(msw_ctx* ctx, const msw_index* x, const msw_read_batch_t* b, int both,
                        const msw_seed_params_t* sp, uint32_t sep, const msw_seed_out_t* out,
                        const msw_seed_alt_t* alt, uint64_t chunk_reads) {
    return seed_host(ctx, x, b, both, sp, true, sep, out, alt, chunk_reads);
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

// Pairs (include/msw.h, "Pairs"; the kernels: msw_pair.hip).
void msw_pair_params_default(msw_pair_params_t* p) {
    if (!p) return;
    *p = msw_pair_params_t{1u, 1000u, 17, 60, 16u};
}

static bool rescue_on(const msw_pair_params_t& q) { return q.rescue_min_score != 0 || q.slack != 0; }

static int check_pair_params(const msw_pair_params_t* q, msw::PairRule* r) {
    if (!q) return fail(MSW_E_INVALID, "pair params is NULL");
    if (q->min_ins < 1 || q->min_ins > q->max_ins || q->max_ins > 4095)
        return fail(MSW_E_RANGE, "pairs: insert bounds [%u, %u] outside 1 <= min <= max <= 4095", q->min_ins,
                    q->max_ins);
    if (q->pair_bonus < 0 || q->rescue_min_score < 0)
        return fail(MSW_E_RANGE, "pairs: pair_bonus / rescue_min_score below 0");
    if (q->slack > 4096) return fail(MSW_E_RANGE, "pairs: slack %u > 4096", q->slack);
    *r = msw::PairRule{(int32_t)q->min_ins, (int32_t)q->max_ins, q->pair_bonus, q->rescue_min_score, (int32_t)q->slack};
    return MSW_OK;
}

// W_r of the contract; 0 when rescue is off
static int rescue_window(const msw_pair_params_t& q, uint32_t max_read_len, uint32_t* w) {
    *w = 0;
    if (!rescue_on(q)) return MSW_OK;
    const uint64_t wr = (uint64_t)q.max_ins - q.min_ins + max_read_len + 2ull * q.slack;
    if (wr > (uint64_t)msw::kMaxWinLen)
        return fail(MSW_E_RANGE, "pairs: rescue window %llu > %d", (unsigned long long)wr, msw::kMaxWinLen);
    *w = (uint32_t)wr;
    return MSW_OK;
}

static msw::PairCand pair_cand(const msw_cand_t& c) {
    return msw::PairCand{c.score, c.end_i, c.end_j, c.win_len, c.strand, c.oriented, c.win_pos};
}

int msw_pair_plan_device(msw_ctx* ctx, const msw_cand_t* cand, const uint16_t* read_len, uint64_t n_pairs,
                         const msw_pair_params_t* params, int64_t* rescue_pos, void* stream) {
    if (!ctx) return fail(MSW_E_INVALID, "ctx is NULL");
    msw::PairPlanParams p;
    int rc;
    if ((rc = check_pair_params(params, &p.rule))) return rc;
    if (n_pairs == 0) return MSW_OK;
    if (!cand || !read_len || !rescue_pos) return fail(MSW_E_INVALID, "NULL array");
    for (int k = 0; k < 2; ++k) {
        if (!cand[k].score || !cand[k].end_i || !cand[k].end_j || !cand[k].strand || !cand[k].win_pos)
            return fail(MSW_E_INVALID, "NULL array in candidate %d", k);
        p.c[k] = pair_cand(cand[k]);
    }
    if (n_pairs > 0x3FFFFFFFull) return fail(MSW_E_RANGE, "pair plan: too many pairs in one call");
    if ((rc = set_device(ctx))) return rc;
    p.read_len = read_len;
    p.n_pairs = n_pairs;
    p.rescue_pos = rescue_pos;
    HIP_TRY(msw::launch_pair_plan(p, call_stream(ctx, stream)));
    return MSW_OK;
}

int msw_pair_select_device(msw_ctx* ctx, const msw_cand_t* cand, uint32_t K, uint32_t oriented_stride,
                           const uint16_t* read_len, uint64_t n_pairs, int32_t match,
                           const msw_pair_params_t* params, int32_t* sub_score, uint8_t* mapq, uint8_t* cand_out,
                           uint8_t* pair_flags, int32_t* tlen, void* stream) {
    if (!ctx) return fail(MSW_E_INVALID, "ctx is NULL");
    msw::PairSelectParams p;
    memset(&p, 0, sizeof(p));
    int rc;
    if ((rc = check_pair_params(params, &p.rule))) return rc;
    if (match < 0 || match > 64) return fail(MSW_E_RANGE, "pair select: match=%d outside [0, 64]", match);
    if (K != 2 && K != 3) return fail(MSW_E_INVALID, "pair select: K=%u is neither 2 nor 3", K);
    if (n_pairs == 0) return MSW_OK;
    if (!cand || !read_len || !sub_score || !mapq || !cand_out || !pair_flags || !tlen)
        return fail(MSW_E_INVALID, "NULL array");
    for (uint32_t k = 0; k < K; ++k) {
        const msw_cand_t& c = cand[k];
        if (!c.score || !c.end_i || !c.end_j || !c.win_len || !c.strand || !c.oriented || !c.win_pos)
            return fail(MSW_E_INVALID, "NULL array in candidate %u", k);
        if (((uintptr_t)c.oriented & 15) != 0 || oriented_stride == 0 || oriented_stride % 16 != 0)
            return fail(MSW_E_INVALID, "oriented must be 16-byte aligned and oriented_stride a non-zero multiple of 16");
        p.c[k] = pair_cand(c);
    }
    if (n_pairs > 0x3FFFFFFFull) return fail(MSW_E_RANGE, "pair select: too many pairs in one call");
    if ((rc = set_device(ctx))) return rc;
    p.k = K;
    p.read_len = read_len;
    p.oriented_stride = oriented_stride;
    p.n_pairs = n_pairs;
    p.match = match;
    p.sub_score = sub_score, p.mapq = mapq, p.cand = cand_out, p.pair_flags = pair_flags, p.tlen = tlen;
    HIP_TRY(msw::launch_pair_select(p, call_stream(ctx, stream)));
    return MSW_OK;
}

int msw_insert_hist_device(msw_ctx* ctx, const int32_t* tlen, const uint8_t* mapq, uint64_t n_pairs,
                           uint32_t min_mapq, uint32_t* hist, void* stream) {
    if (!ctx) return fail(MSW_E_INVALID, "ctx is NULL");
    if (min_mapq > 255) return fail(MSW_E_RANGE, "insert hist: min_mapq %u > 255", min_mapq);
    if (n_pairs == 0) return MSW_OK;
    if (!tlen || !mapq || !hist) return fail(MSW_E_INVALID, "NULL array");
    if (n_pairs > 0x3FFFFFFFull) return fail(MSW_E_RANGE, "insert hist: too many pairs in one call");
    int rc = set_device(ctx);
    if (rc) return rc;
    HIP_TRY(msw::launch_insert_hist(tlen, mapq, n_pairs, min_mapq, hist, call_stream(ctx, stream)));
    return MSW_OK;
}

int msw_insert_bounds(const uint32_t* hist, uint32_t* lo, uint32_t* hi, uint32_t* median) {
    if (!hist || !lo || !hi || !median) return fail(MSW_E_INVALID, "NULL argument");
    uint64_t total = 0;
    for (uint32_t k = 0; k < msw::kInsertBins; ++k) total += hist[k];
    if (total == 0) return fail(MSW_E_INVALID, "insert bounds: the histogram is empty");
    const uint64_t need[3] = {(total + 3) / 4, (total + 1) / 2, (3 * total + 3) / 4};
    uint32_t q[3] = {0, 0, 0};
    uint64_t cum = 0;
    int at = 0;
    for (uint32_t k = 0; k < msw::kInsertBins && at < 3; ++k) {
        cum += hist[k];
        while (at < 3 && cum >= need[at]) q[at++] = k;
    }
    const int64_t iqr = (int64_t)q[2] - q[0];
    *lo = (uint32_t)std::max<int64_t>(1, (int64_t)q[0] - 3 * iqr);
    *hi = (uint32_t)std::min<int64_t>(4095, (int64_t)q[2] + 3 * iqr);
    *median = q[1];
    return MSW_OK;
}

// What msw_map_reads and msw_map_pairs share: their argument checks, and the
// carve of one candidate's arrays.

// msw_map_pairs' own arguments, checked among the shared ones in the places
// where it has always checked them.
struct PairArgs {
    const msw_pair_params_t* pp;
    const uint8_t* pair_flags;
    const int32_t* tlen;
    msw::PairRule rule;  // out
    uint32_t wr;         // out: W_r, 0 with rescue off
};

struct MapArgs {  // out
    msw_scoring_t scc;  // the scoring with want_coords set
    uint64_t n;         // rows
    uint32_t max_m, max_n, window;
};

// *go = false: nothing to do (no rows; the empty aln is written).
static int check_map_args(msw_ctx* ctx, const msw_scoring_t* sc, const msw_genome* g, const msw_index* x,
                          const msw_read_batch_t* b, bool need_strand, const msw_seed_params_t* sp, uint32_t sep,
                          const msw_out_t* out, const uint8_t* strand, msw_aln_t* aln, const msw_mapq_t* mq,
                          PairArgs* pair, MapArgs* m, bool* go) {
    *go = false;
    if (!ctx || !g || !x) return fail(MSW_E_INVALID, "ctx/genome/index is NULL");
    if (g->ctx != ctx) return fail(MSW_E_INVALID, "genome belongs to another context");
    if (x->ctx != ctx) return fail(MSW_E_INVALID, "index belongs to another context");
    if (!sc || !b) return fail(MSW_E_INVALID, "scoring/batch is NULL");
    m->scc = *sc;
    m->scc.want_coords = 1;
    Scheme sch;
    int rc;
    if ((rc = make_scheme(&m->scc, ctx->opt, &sch))) return rc;
    if ((rc = validate_aln(aln))) return rc;
    const uint64_t n = m->n = b->n_pairs;
    if (pair && (n & 1)) return fail(MSW_E_INVALID, "pairs: %llu rows is an odd number", (unsigned long long)n);
    uint32_t max_m = 0;
    if (n && !b->read_len) return fail(MSW_E_INVALID, "NULL array in batch");
    max_u16(b->read_len, n, max_m);
    if ((rc = check_seed_params(sp, max_m))) return rc;
    if (sep != 0 && sep < sp->band) return fail(MSW_E_RANGE, "candidates: sep %u is below band %u", sep, sp->band);
    if (pair && ((rc = check_pair_params(pair->pp, &pair->rule)) || (rc = rescue_window(*pair->pp, max_m, &pair->wr))))
        return rc;
    *aln->n_overflow = 0;
    aln->cigar_off[0] = 0;
    if (n == 0) return MSW_OK;
    if (!b->reads) return fail(MSW_E_INVALID, "NULL array in batch");
    if (need_strand && !strand) return fail(MSW_E_INVALID, "strand is NULL");
    if (!out || !out->score || !out->end_i || !out->end_j)
        return fail(MSW_E_INVALID, "traceback needs score / end_i / end_j");
    if (!mq || !mq->mapq || !mq->sub_score || !mq->cand) return fail(MSW_E_INVALID, "NULL array in mapq");
    if (pair && (!pair->pair_flags || !pair->tlen)) return fail(MSW_E_INVALID, "pair_flags / tlen is NULL");
    if (n > 0x7FFFFFFFull) return fail(MSW_E_RANGE, "traceback: n_pairs > 2^31-1 in one call");
    m->max_m = max_m;
    m->window = sp->window;
    m->max_n = m->window ? m->window : std::min<uint32_t>(2u * max_m, (uint32_t)msw::kMaxWinLen);
    if ((rc = check_trace_bounds(max_m, m->max_n))) return rc;
    if (b->read_stride == 0 || max_m > b->read_stride) return fail(MSW_E_INVALID, "a length exceeds its stride");
    if ((rc = set_device(ctx))) return rc;
    *go = true;
    return MSW_OK;
}

// One candidate's arrays of a chunk; without `oriented` (one strand) it has
// neither strand bytes nor rows.
struct CandAt {
    DeviceArena::Slice<int64_t> wp;
    DeviceArena::Slice<int32_t> s;
    DeviceArena::Slice<int16_t> ei, ej;
    DeviceArena::Slice<uint16_t> wl;
    DeviceArena::Slice<uint8_t> st, rows;
    bool oriented;
    msw_cand_t cand() const {  // once the arena is allocated
        return msw_cand_t{s, ei, ej, wl, oriented ? (uint8_t*)st : nullptr, oriented ? (uint8_t*)rows : nullptr, wp};
    }
};

static CandAt take_cand(DeviceArena& a, uint64_t chunk, size_t ors, bool oriented) {
    return CandAt{a.take<int64_t>(chunk),  a.take<int32_t>(chunk),
                  a.take<int16_t>(chunk),  a.take<int16_t>(chunk),
                  a.take<uint16_t>(chunk), a.take<uint8_t>(oriented ? chunk : 0),
                  a.take<uint8_t>(oriented ? chunk * ors : 0), oriented};
}

int msw_map_reads(msw_ctx* ctx, const msw_scoring_t* sc, const msw_genome* g, const msw_index* x,
                  const msw_read_batch_t* b, int both, const msw_seed_params_t* sp, uint32_t sep, msw_out_t* out,
                  uint8_t* strand, msw_aln_t* aln, const msw_mapq_t* mq, uint64_t chunk_pairs) {
    MapArgs m;
    bool go;
    int rc = check_map_args(ctx, sc, g, x, b, both != 0, sp, sep, out, strand, aln, mq, nullptr, &m, &go);
    if (rc || !go) return rc;
    const msw_scoring_t& scc = m.scc;
    const uint64_t n = m.n;
    const uint32_t max_m = m.max_m, max_n = m.max_n, window = m.window;
    // Simple and synchronous, like msw_align_reads_trace.  Per chunk, all on
    // the compute stream: upload, (reverse complement,) candidates, the two
    // scoring calls, the selection, then trace and pack on the winner.
    const uint64_t chunk = std::min<uint64_t>(n, chunk_pairs ? chunk_pairs : 65536);
    const size_t rs = b->read_stride, ors = round16(std::max<uint32_t>(max_m, 1)), cs = (size_t)max_m + max_n;
    DeviceArena a;
    const auto d_reads = a.take<uint8_t>(chunk * rs), d_rc = a.take<uint8_t>(both ? chunk * ors : 0);
    const CandAt ca[2] = {take_cand(a, chunk, ors, both != 0), take_cand(a, chunk, ors, both != 0)};
    const auto d_rows = a.take<uint32_t>(chunk * cs);
    const auto d_ref = a.take<int64_t>(chunk);
    const auto d_sub = a.take<int32_t>(chunk), d_nc = a.take<int32_t>(chunk), d_nm = a.take<int32_t>(chunk);
    const auto d_votes = a.take<uint32_t>(chunk), d_hits = a.take<uint32_t>(chunk), d_votes1 = a.take<uint32_t>(chunk),
               d_off = a.take<uint32_t>(chunk + 2);
    const auto d_rl = a.take<uint16_t>(chunk);
    const auto d_si = a.take<int16_t>(chunk), d_sj = a.take<int16_t>(chunk);
    const auto d_fl = a.take<uint8_t>(chunk), d_fl1 = a.take<uint8_t>(chunk), d_mapq = a.take<uint8_t>(chunk),
               d_cand = a.take<uint8_t>(chunk);
    RecordOps ops;
    if ((rc = a.alloc()) || (rc = ops.alloc(chunk * 8))) return rc;
    const msw_cand_t cand[2] = {ca[0].cand(), ca[1].cand()};
    msw_out_t co[2] = {{cand[0].score, cand[0].end_i, cand[0].end_j}, {cand[1].score, cand[1].end_i, cand[1].end_j}};
    ChunkCopy cp(ctx->compute);
    hipStream_t st = cp.st;
    for (uint64_t lo = 0; lo < n && rc == MSW_OK && cp.ok(); lo += chunk) {
        const uint64_t c = std::min(chunk, n - lo);
        cp.up(d_reads, b->reads + lo * rs, c * rs);
        cp.up(d_rl, b->read_len + lo, c * 2);
        if (!cp.ok()) break;
        if (both && (rc = msw_revcomp_device(ctx, d_reads, d_rl, (uint32_t)rs, c, d_rc, (uint32_t)ors, st))) break;
        const msw_seed_out_t so = {cand[0].win_pos, d_votes, d_hits, d_fl};
        const msw_seed_alt_t sa = {cand[1].win_pos, d_votes1, d_fl1};
        if ((rc = msw_seed_candidates_device(ctx, x, d_reads, both ? (const uint8_t*)d_rc : nullptr, d_rl, (uint32_t)rs,
                                             (uint32_t)ors, c, max_m, sp, sep, &so, &sa, st)))
            break;
        for (int k = 0; k < 2 && rc == MSW_OK; ++k)
            rc = both ? msw_align_reads_strands_device(ctx, &scc, g, d_reads, d_rl, (uint32_t)rs, cand[k].win_pos, c,
                                                       window, max_m, &co[k], cand[k].win_len, cand[k].strand,
                                                       cand[k].oriented, (uint32_t)ors, st)
                      : msw_align_reads_device(ctx, &scc, g, d_reads, d_rl, (uint32_t)rs, cand[k].win_pos, c, window,
                                               max_m, &co[k], cand[k].win_len, st);
        if (rc) break;
        if ((rc = msw_mapq_select_device(ctx, &cand[0], &cand[1], (uint32_t)ors, d_rl, c, scc.match, d_sub, d_mapq,
                                         d_cand, st)))
            break;
        // from here on the reads are the winner's oriented rows
        const uint8_t* rows = both ? cand[0].oriented : (const uint8_t*)d_reads;
        const uint32_t rstride = both ? (uint32_t)ors : (uint32_t)rs;
        msw_trace_t dtr = {d_si, d_sj, d_nc, d_rows, (uint32_t)cs};
        if ((rc = msw_trace_reads_device(ctx, &scc, g, rows, d_rl, rstride, cand[0].win_pos, c, window, max_m, &co[0],
                                         &dtr, st)))
            break;
        const ChunkRecords rec = {rows, rstride, d_rl, cand[0].win_pos, &co[0], &dtr, d_ref, d_nm, d_off};
        if ((rc = pack_chunk_records(ctx, g, cp, ops, rec, lo, c,
                                     {{out->score + lo, cand[0].score, c * 4},
                                      {out->end_i + lo, cand[0].end_i, c * 2},
                                      {out->end_j + lo, cand[0].end_j, c * 2},
                                      {both ? strand + lo : nullptr, cand[0].strand, both ? c : 0},
                                      {mq->mapq + lo, d_mapq, c},
                                      {mq->sub_score + lo, d_sub, c * 4},
                                      {mq->cand + lo, d_cand, c}},
                                     aln)))
            break;
        cp.sync();
    }
    return cp.finish(rc, "map reads");
}

int msw_map_pairs(msw_ctx* ctx, const msw_scoring_t* sc, const msw_genome* g, const msw_index* x,
                  const msw_read_batch_t* b, const msw_seed_params_t* sp, uint32_t sep, const msw_pair_params_t* pp,
                  msw_out_t* out, uint8_t* strand, msw_aln_t* aln, const msw_mapq_t* mq, uint8_t* pair_flags,
                  int32_t* tlen, uint32_t* hist, uint64_t chunk_pairs) {
    MapArgs m;
    PairArgs pa = {pp, pair_flags, tlen, {}, 0};
    bool go;
    int rc = check_map_args(ctx, sc, g, x, b, true, sp, sep, out, strand, aln, mq, &pa, &m, &go);
    if (rc || !go) return rc;
    const msw_scoring_t& scc = m.scc;
    const uint64_t n = m.n;  // rows
    const uint32_t max_m = m.max_m, max_n = m.max_n, window = m.window, wr = pa.wr;
    const bool rescue = wr != 0;
    const int K = rescue ? 3 : 2;
    // The trace reads a window only up to the best cell's column, so its
    // window argument is a bound and one call serves both window lengths: with
    // rescue it is the larger of the two, without it what msw_map_reads passes.
    const uint32_t trace_window = rescue ? std::max(max_n, wr) : window;
    const uint32_t trace_n = rescue ? trace_window : max_n;
    // msw_map_reads with `both`, on whole pairs, with the plan and the rescue
    // scoring between the two candidate scorings and the select.
    const uint64_t chunk = std::min<uint64_t>(n, 2 * (chunk_pairs ? chunk_pairs : 32768));
    const size_t rs = b->read_stride, ors = round16(std::max<uint32_t>(max_m, 1)), cs = (size_t)max_m + trace_n;
    DeviceArena a;
    const auto d_reads = a.take<uint8_t>(chunk * rs), d_rc = a.take<uint8_t>(chunk * ors);
    const auto d_rows = a.take<uint32_t>(chunk * cs);
    const auto d_ref = a.take<int64_t>(chunk);
    const auto d_sub = a.take<int32_t>(chunk), d_nc = a.take<int32_t>(chunk), d_nm = a.take<int32_t>(chunk),
               d_tlen = a.take<int32_t>(chunk / 2);
    const auto d_votes = a.take<uint32_t>(chunk), d_hits = a.take<uint32_t>(chunk), d_votes1 = a.take<uint32_t>(chunk),
               d_off = a.take<uint32_t>(chunk + 2), d_hist = a.take<uint32_t>(msw::kInsertBins);
    const auto d_rl = a.take<uint16_t>(chunk);
    const auto d_si = a.take<int16_t>(chunk), d_sj = a.take<int16_t>(chunk);
    const auto d_fl = a.take<uint8_t>(chunk), d_fl1 = a.take<uint8_t>(chunk), d_mapq = a.take<uint8_t>(chunk),
               d_cand = a.take<uint8_t>(chunk), d_pf = a.take<uint8_t>(chunk / 2);
    CandAt ca[3];
    for (int k = 0; k < K; ++k) ca[k] = take_cand(a, chunk, ors, true);
    RecordOps ops;
    if ((rc = a.alloc()) || (rc = ops.alloc(chunk * 8))) return rc;
    msw_cand_t cand[3];
    msw_out_t co[3];
    for (int k = 0; k < K; ++k) {
        cand[k] = ca[k].cand();
        co[k] = msw_out_t{cand[k].score, cand[k].end_i, cand[k].end_j};
    }
    ChunkCopy cp(ctx->compute);
    hipStream_t st = cp.st;
    if (hist) cp.note(hipMemsetAsync(d_hist, 0, msw::kInsertBins * 4, st));
    for (uint64_t lo = 0; lo < n && rc == MSW_OK && cp.ok(); lo += chunk) {
        const uint64_t c = std::min(chunk, n - lo);
        cp.up(d_reads, b->reads + lo * rs, c * rs);
        cp.up(d_rl, b->read_len + lo, c * 2);
        if (!cp.ok()) break;
        if ((rc = msw_revcomp_device(ctx, d_reads, d_rl, (uint32_t)rs, c, d_rc, (uint32_t)ors, st))) break;
        const msw_seed_out_t so = {cand[0].win_pos, d_votes, d_hits, d_fl};
        const msw_seed_alt_t sa = {cand[1].win_pos, d_votes1, d_fl1};
        if ((rc = msw_seed_candidates_device(ctx, x, d_reads, d_rc, d_rl, (uint32_t)rs, (uint32_t)ors, c, max_m, sp,
                                             sep, &so, &sa, st)))
            break;
        for (int k = 0; k < 2 && rc == MSW_OK; ++k)
            rc = msw_align_reads_strands_device(ctx, &scc, g, d_reads, d_rl, (uint32_t)rs, cand[k].win_pos, c, window,
                                                max_m, &co[k], cand[k].win_len, cand[k].strand, cand[k].oriented,
                                                (uint32_t)ors, st);
        if (rc) break;
        if (rescue) {
            // every row is scored at W_r; a row that is not to be rescued is an empty window
            if ((rc = msw_pair_plan_device(ctx, cand, d_rl, c / 2, pp, cand[2].win_pos, st)) ||
                (rc = msw_align_reads_strands_device(ctx, &scc, g, d_reads, d_rl, (uint32_t)rs, cand[2].win_pos, c, wr,
                                                     max_m, &co[2], cand[2].win_len, cand[2].strand, cand[2].oriented,
                                                     (uint32_t)ors, st)))
                break;
        }
        if ((rc = msw_pair_select_device(ctx, cand, (uint32_t)K, (uint32_t)ors, d_rl, c / 2, scc.match, pp, d_sub,
                                         d_mapq, d_cand, d_pf, d_tlen, st)))
            break;
        if (hist && (rc = msw_insert_hist_device(ctx, d_tlen, d_mapq, c / 2, 0u, d_hist, st))) break;
        // from here on the reads are the winners' oriented rows, in candidate 0's arrays
        msw_trace_t dtr = {d_si, d_sj, d_nc, d_rows, (uint32_t)cs};
        if ((rc = msw_trace_reads_device(ctx, &scc, g, cand[0].oriented, d_rl, (uint32_t)ors, cand[0].win_pos, c,
                                         trace_window, max_m, &co[0], &dtr, st)))
            break;
        const ChunkRecords rec = {cand[0].oriented, (uint32_t)ors, d_rl, cand[0].win_pos, &co[0], &dtr, d_ref, d_nm,
                                  d_off};
        if ((rc = pack_chunk_records(ctx, g, cp, ops, rec, lo, c,
                                     {{out->score + lo, cand[0].score, c * 4},
                                      {out->end_i + lo, cand[0].end_i, c * 2},
                                      {out->end_j + lo, cand[0].end_j, c * 2},
                                      {strand + lo, cand[0].strand, c},
                                      {mq->mapq + lo, d_mapq, c},
                                      {mq->sub_score + lo, d_sub, c * 4},
                                      {mq->cand + lo, d_cand, c},
                                      {pair_flags + lo / 2, d_pf, c / 2},
                                      {tlen + lo / 2, d_tlen, c / 2 * 4}},
                                     aln)))
            break;
        cp.sync();
    }
    if (hist && rc == MSW_OK && cp.ok()) {
        std::vector<uint32_t> h(msw::kInsertBins);
        cp.down(h.data(), d_hist, msw::kInsertBins * 4);
        cp.sync();
        if (cp.ok())
            for (uint32_t k = 0; k < msw::kInsertBins; ++k) hist[k] += h[k];
    }
    return cp.finish(rc, "map pairs");
}

}  // extern "C"
