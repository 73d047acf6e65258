// msw_rt_pileup.cpp -- pileup and variant calls (include/msw.h, "Pileup",
// "Variants", "Base qualities", "Quality sums and weighted genotypes"): the
// pileup state, the adds, the fold, the counts and sums, and the calls from a
// pileup or from host counts.  The kernels: msw_pileup.hip, msw_call.hip.
#include "msw_runtime_internal.h"

using namespace msw_detail;

extern "C" {

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
    hipEvent_t fin = nullptr;      // recorded behind the fold (and the vote)
    // with MSW_PILEUP_INS ("Inserted sequences"; the kernels: msw_ins.hip): the log, an allocation of its own; its
    // cursor and the number of sites are words 8 and 9 of the sixteen at d_stats
    msw::PileupIns ins{};
    bool added = false;            // an add has been enqueued: the log's capacity is fixed
    msw_ins_site_t* d_sites = nullptr;  // the table, allocated by the finish
    uint64_t sites_cap = 0;
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
    if (flags & ~(MSW_PILEUP_QSUM | MSW_PILEUP_INS)) return fail(MSW_E_INVALID, "pileup create: unknown flag in 0x%x", flags);
    const bool qsum = (flags & MSW_PILEUP_QSUM) != 0;
    if (g->ctx != ctx) return fail(MSW_E_INVALID, "genome belongs to another context");
    int rc = set_device(ctx);
    if (rc) return rc;
    const uint64_t glen = g->len;
    if ((flags & MSW_PILEUP_INS) && glen > 0xFFFFFFFFull)
        return fail(MSW_E_RANGE, "pileup create: MSW_PILEUP_INS over a genome above 2^32-1 bases");
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
    if (e == hipSuccess && (flags & MSW_PILEUP_INS)) {
        pile->ins.cursor = pile->d_stats + 8;
        pile->ins.cap = std::max<uint64_t>(1ull << 20, glen / 4);
        e = hipMalloc((void**)&pile->ins.log, pile->ins.cap * sizeof(uint4));
    }
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
    if (pile->ins.log) (void)hipFree(pile->ins.log);
    if (pile->d_sites) (void)hipFree(pile->d_sites);
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
    pile->added = true;
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
    if (pile->flags & MSW_PILEUP_INS) HIP_TRY(msw::launch_ins_capture(p, pile->ins, call_stream(ctx, stream)));
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
    pile->added = true;
    const bool ins = (pile->flags & MSW_PILEUP_INS) != 0;
    const size_t rs = read_stride, qs = qual_stride;
    DeviceArena a;
    const auto d_ref = a.take<int64_t>(chunk);
    const auto d_nm = a.take<int32_t>(chunk);
    const auto d_off = a.take<uint32_t>(chunk + 1), d_ops = a.take<uint32_t>(max_ops);
    const auto d_rl = a.take<uint16_t>(chunk);
    const auto d_st = a.take<uint8_t>(chunk), d_mq = a.take<uint8_t>(chunk), d_rows = a.take<uint8_t>(chunk * rs),
               d_q = a.take<uint8_t>(chunk * qs);
    if ((rc = a.alloc())) return rc;
    ChunkCopy cp(ctx->compute);
    hipStream_t st = cp.st;
    msw::PileupParams p = pile->p;
    p.rows = d_rows;
    p.read_len = d_rl;
    p.row_stride = rs;
    p.ref_pos = d_ref;
    p.nm = d_nm;
    p.cigar_off = d_off;
    p.cigar = d_ops;
    p.cigar_cap = aln->cigar_cap;
    p.strand = strand ? (const uint8_t*)d_st : nullptr;
    p.mapq = mapq ? (const uint8_t*)d_mq : nullptr;
    p.min_mapq = min_mapq;
    p.orient = strand ? 1u : 0u;
    const msw::PileupQual q{d_q, qual_stride, min_baseq, pile->d_lowq};
    msw::PileupQsum qq = pile->qs;
    qq.quals = q.quals;
    qq.qual_stride = qual_stride;
    qq.min_baseq = min_baseq;
    for (uint64_t lo = 0; lo < n && cp.ok(); lo += chunk) {
        const uint64_t c = std::min(chunk, n - lo);
        const uint32_t o0 = aln->cigar_off[lo], o1 = aln->cigar_off[lo + c];
        cp.up(d_ref, aln->ref_pos + lo, c * 8);
        cp.up(d_nm, aln->nm + lo, c * 4);
        cp.up(d_off, aln->cigar_off + lo, (c + 1) * 4);
        cp.up(d_ops, aln->cigar + o0, (size_t)(o1 - o0) * 4);
        cp.up(d_rl, read_len + lo, c * 2);
        if (strand) cp.up(d_st, strand + lo, c);
        if (mapq) cp.up(d_mq, mapq + lo, c);
        cp.up(d_rows, reads + lo * rs, c * rs);
        if (quals) cp.up(d_q, quals + lo * qs, c * qs);
        p.n = c;
        p.cigar_base = o0;
        if (cp.ok())
            cp.note(qsum ? msw::launch_pileup_add_qsum(p, qq, st)
                         : quals ? msw::launch_pileup_add_qual(p, q, st) : msw::launch_pileup_add(p, st));
        if (ins && cp.ok()) cp.note(msw::launch_ins_capture(p, pile->ins, st));
        cp.sync();  // the buffers are the next chunk's
    }
    return cp.finish(MSW_OK, "pileup add");
}

// The vote of "Inserted sequences" behind the fold: the table is allocated here and kept, the glen-sized offsets and
// the grouped events live for these launches only; everything is stream-ordered.
static int pileup_ins_vote(msw_pileup* pile, hipStream_t st) {
    const msw::PileupParams& p = pile->p;
    auto up16 = [](uint64_t x) { return (x + 15) & ~(uint64_t)15; };
    msw::InsVote v{};
    v.counts = p.counts;
    v.pos_mul = p.pos_mul;
    v.ch_mul = p.ch_mul;
    v.glen = p.glen;
    v.log = pile->ins.log;
    v.cap = pile->ins.cap;
    v.cursor = pile->ins.cursor;
    v.n_sites = pile->ins.cursor + 1;
    // a site has at least one event, and a position at most one site
    v.sites_cap = pile->sites_cap = std::max<uint64_t>(1, std::min(v.cap, p.glen));
    HIP_TRY(hipMallocAsync((void**)&pile->d_sites, v.sites_cap * sizeof(msw_ins_site_t), st));
    v.sites = pile->d_sites;
    const uint64_t words = up16((p.glen + 1) * 4);
    uint8_t* tmp = nullptr;
    HIP_TRY(hipMallocAsync((void**)&tmp, 2 * words + v.cap * sizeof(uint4), st));
    v.off = reinterpret_cast<uint32_t*>(tmp);
    v.sidx = reinterpret_cast<uint32_t*>(tmp + words);
    v.sorted = reinterpret_cast<uint4*>(tmp + 2 * words);
    hipError_t e = msw::launch_ins_vote(v, pile->d_scan_tmp, st);
    const hipError_t ef = hipFreeAsync(tmp, st);
    if (e == hipSuccess) e = ef;
    if (e != hipSuccess) return fail(MSW_E_DEVICE, "pileup finish, inserted sequences: %s", hipGetErrorString(e));
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
    if ((pile->flags & MSW_PILEUP_INS) && (rc = pileup_ins_vote(pile, st))) return rc;
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

// Inserted sequences (include/msw.h, "Inserted sequences"; the kernels: msw_ins.hip).
static int check_pileup_ins(const msw_ctx* ctx, const msw_pileup* pile, const char* what) {
    int rc;
    if ((rc = check_pileup(ctx, pile))) return rc;
    if (!(pile->flags & MSW_PILEUP_INS)) return fail(MSW_E_INVALID, "%s: the pileup was created without MSW_PILEUP_INS", what);
    return MSW_OK;
}

static_assert(sizeof(msw_ins_site_t) == 32, "msw_ins_site_t is 32 bytes");

int msw_pileup_ins_capacity(msw_ctx* ctx, msw_pileup* pile, uint64_t events) {
    int rc;
    if ((rc = check_pileup_ins(ctx, pile, "pileup ins capacity"))) return rc;
    if (pile->added || pile->finished) return fail(MSW_E_INVALID, "pileup ins capacity: after the first add");
    if (events == 0 || events > 0x7FFFFFFFull) return fail(MSW_E_RANGE, "pileup ins capacity: %llu events", (unsigned long long)events);
    if (events == pile->ins.cap) return MSW_OK;
    if ((rc = set_device(ctx))) return rc;
    uint4* log = nullptr;
    const hipError_t e = hipMalloc((void**)&log, events * sizeof(uint4));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(MSW_E_NOMEM, "hipMalloc(%llu B) for the insertion log: %s", (unsigned long long)(events * sizeof(uint4)),
                    hipGetErrorString(e));
    }
    (void)hipFree(pile->ins.log);
    pile->ins.log = log;
    pile->ins.cap = events;
    return MSW_OK;
}

// cursor and n_sites, once the device (all = true) or the finish has drained
static int pileup_ins_words(msw_ctx* ctx, msw_pileup* pile, bool all, unsigned long long h[2]) {
    int rc;
    if ((rc = set_device(ctx))) return rc;
    // adds may have been enqueued on any stream
    if (all) HIP_TRY(hipDeviceSynchronize());
    else HIP_TRY(hipEventSynchronize(pile->fin));
    HIP_TRY(hipMemcpy(h, pile->ins.cursor, 16, hipMemcpyDeviceToHost));
    return MSW_OK;
}

int msw_pileup_ins_info(msw_ctx* ctx, msw_pileup* pile, msw_ins_info_t* out) {
    int rc;
    if ((rc = check_pileup_ins(ctx, pile, "pileup ins info"))) return rc;
    if (!out) return fail(MSW_E_INVALID, "out is NULL");
    unsigned long long h[2];
    if ((rc = pileup_ins_words(ctx, pile, true, h))) return rc;
    out->events = h[0];
    out->dropped = h[0] > pile->ins.cap ? h[0] - pile->ins.cap : 0;
    out->sites = pile->finished ? h[1] : 0;
    out->capacity = pile->ins.cap;
    return MSW_OK;
}

int msw_pileup_ins_sites_device(msw_ctx* ctx, msw_pileup* pile, const msw_ins_site_t** sites, uint64_t* n) {
    int rc;
    if ((rc = check_pileup_ins(ctx, pile, "pileup ins sites"))) return rc;
    if (!sites || !n) return fail(MSW_E_INVALID, "NULL output");
    if (!pile->finished) return fail(MSW_E_INVALID, "pileup ins sites before msw_pileup_finish");
    unsigned long long h[2];
    if ((rc = pileup_ins_words(ctx, pile, false, h))) return rc;
    if (h[0] > pile->ins.cap)
        return fail(MSW_E_RANGE, "pileup ins sites: the log of %llu events dropped %llu (msw_pileup_ins_capacity)",
                    (unsigned long long)pile->ins.cap, h[0] - pile->ins.cap);
    *sites = pile->d_sites;
    *n = h[1];
    return MSW_OK;
}

int msw_pileup_ins_sites(msw_ctx* ctx, msw_pileup* pile, msw_ins_site_t* host_out, uint64_t cap, uint64_t* n_total) {
    int rc;
    if ((rc = check_pileup_ins(ctx, pile, "pileup ins sites"))) return rc;
    if (!n_total) return fail(MSW_E_INVALID, "n_total is NULL");
    if (cap && !host_out) return fail(MSW_E_INVALID, "host_out is NULL with cap > 0");
    const msw_ins_site_t* d = nullptr;
    uint64_t n = 0;
    if ((rc = msw_pileup_ins_sites_device(ctx, pile, &d, &n))) return rc;
    const uint64_t have = std::min(cap, n);
    if (have) HIP_TRY(hipMemcpy(host_out, d, have * sizeof(msw_ins_site_t), hipMemcpyDeviceToHost));
    *n_total = n;
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
    // rows of chunk + 1 positions (the look-ahead row), and with `weighted` rows of four sums
    DeviceArena a;
    const auto d_counts = a.take<uint32_t>((chunk + 1) * 8), d_tile = a.take<uint32_t>(msw::call_tmp_words(chunk)),
               d_qsum = a.take<uint32_t>(weighted ? chunk * 4 : 0);
    const auto d_gen = a.take<uint8_t>(chunk);
    const auto d_tot = a.take<unsigned long long>(1);
    if ((rc = a.alloc())) return rc;
    ChunkCopy cp(ctx->compute);
    hipStream_t st = cp.st;
    p.counts = d_counts;
    p.genome = d_gen;
    p.pos_mul = 8;
    p.ch_mul = 1;
    p.n_total = d_tot;
    p.tile_off = d_tile;
    p.qsum = weighted ? (const uint32_t*)d_qsum : nullptr;
    msw_variant_t* d_out = nullptr;  // grows to the largest chunk's records that still fit cap
    uint64_t d_out_cap = 0, total = 0, written = 0;
    for (uint64_t lo = 0; lo < glen && rc == MSW_OK && cp.ok(); lo += chunk) {
        const uint64_t m = std::min(chunk, glen - lo);
        p.m = m;
        p.rows = lo + m < glen ? m + 1 : m;  // the look-ahead row
        p.pos0 = lo;
        p.out = nullptr;
        p.cap = 0;
        cp.up(d_counts, counts_host + lo * 8, p.rows * 32);
        cp.up(d_gen, genome_host + lo, m);
        if (weighted) cp.up(d_qsum, qsums_host + lo * 4, m * 16);
        if (cp.ok()) cp.note(msw::launch_call_count(p, st));
        if (cp.ok()) cp.note(msw::launch_call_scan(p, st));
        uint64_t t = 0;
        cp.down(&t, p.n_total, 8);
        cp.sync();
        if (!cp.ok()) break;
        const uint64_t want = std::min(t, cap - written);
        if (want) {
            if (want > d_out_cap) {
                if (d_out) (void)hipFree(d_out);
                d_out = nullptr;
                d_out_cap = 0;
                const hipError_t e = hipMalloc((void**)&d_out, want * sizeof(msw_variant_t));
                if (e != hipSuccess) {
                    (void)hipGetLastError();
                    d_out = nullptr;
                    rc = fail(MSW_E_NOMEM, "hipMalloc for a chunk's records: %s", hipGetErrorString(e));
                    break;
                }
                d_out_cap = want;
            }
            p.out = d_out;
            p.cap = want;
            cp.note(msw::launch_call_emit(p, st));
            cp.down(out_host + written, d_out, want * sizeof(msw_variant_t));
            cp.sync();  // the buffers are the next chunk's
            written += want;
        }
        total += t;
    }
    rc = cp.finish(rc, "call counts");
    if (d_out) (void)hipFree(d_out);
    if (rc == MSW_OK) *n_total = total;
    return rc;
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

}  // extern "C"
