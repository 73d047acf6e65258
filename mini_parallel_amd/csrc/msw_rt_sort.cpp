// msw_rt_sort.cpp -- sorting and duplicates (include/msw.h, "Sorting and
// duplicates"): the limit checks, the three device calls with their
// stream-ordered temporaries, and the one-shot host forms.
// The kernels: msw_sort.hip, msw_markdup.hip.
#include "msw_runtime_internal.h"

using namespace msw_detail;

namespace {

constexpr uint64_t kMaxRefLen = 1ull << 61;

uint32_t bit_length(uint64_t v) {
    uint32_t b = 0;
    for (; v; v >>= 1) ++b;
    return b;
}

int check_markdup(msw_ctx* ctx, const msw_aln_t* aln, const int32_t* score, uint64_t n_rows, uint64_t ref_len,
                  int pairs, const uint32_t* order, const uint8_t* dup) {
    if (!ctx) return fail(MSW_E_INVALID, "ctx is NULL");
    if (!aln) return fail(MSW_E_INVALID, "aln is NULL");
    if (ref_len > kMaxRefLen) return fail(MSW_E_RANGE, "mark duplicates: ref_len > 2^61");
    if (n_rows > 0x7FFFFFFFull) return fail(MSW_E_RANGE, "mark duplicates: n_rows > 2^31-1 in one call");
    if (pairs && (n_rows & 1)) return fail(MSW_E_INVALID, "mark duplicates: pairs with an odd row count");
    if (n_rows && (!aln->ref_pos || !aln->nm || !aln->cigar_off || !score || !order || !dup))
        return fail(MSW_E_INVALID, "NULL array");
    return MSW_OK;
}

int check_order(msw_ctx* ctx, const int64_t* ref_pos, uint64_t n, uint64_t ref_len, const uint32_t* order) {
    if (!ctx) return fail(MSW_E_INVALID, "ctx is NULL");
    if (ref_len > kMaxRefLen) return fail(MSW_E_RANGE, "coordinate order: ref_len > 2^61");
    if (n > 0x7FFFFFFFull) return fail(MSW_E_RANGE, "coordinate order: n > 2^31-1 in one call");
    if (n && (!ref_pos || !order)) return fail(MSW_E_INVALID, "NULL array");
    return MSW_OK;
}

}  // namespace

extern "C" {

int msw_sort_pairs_device(msw_ctx* ctx, uint64_t* keys, uint32_t* vals, uint64_t n, uint32_t key_bits, void* stream) {
    if (!ctx) return fail(MSW_E_INVALID, "ctx is NULL");
    if (key_bits < 1 || key_bits > 64) return fail(MSW_E_RANGE, "sort: key_bits %u outside 1..64", key_bits);
    if (n > 0x7FFFFFFFull) return fail(MSW_E_RANGE, "sort: n > 2^31-1 in one call");
    if (n == 0) return MSW_OK;
    if (!keys) return fail(MSW_E_INVALID, "keys is NULL");
    int rc;
    if ((rc = set_device(ctx))) return rc;
    StreamTmp tmp(call_stream(ctx, stream));
    if ((rc = tmp.alloc(msw::sort_tmp_bytes(n, vals != nullptr)))) return rc;
    HIP_TRY(msw::launch_sort_pairs(keys, vals, n, key_bits, tmp.p, tmp.st));
    return MSW_OK;
}

int msw_markdup_device(msw_ctx* ctx, const msw_aln_t* aln, const uint8_t* strand, const int32_t* score,
                       uint64_t n_rows, uint64_t ref_len, int pairs, uint32_t* order, uint8_t* dup, uint64_t* n_dup,
                       void* stream) {
    int rc;
    if ((rc = check_markdup(ctx, aln, score, n_rows, ref_len, pairs, order, dup))) return rc;
    if ((rc = set_device(ctx))) return rc;
    hipStream_t st = call_stream(ctx, stream);
    msw::MarkdupParams p;
    memset(&p, 0, sizeof(p));
    p.ref_pos = aln->ref_pos;
    p.nm = aln->nm;
    p.cigar_off = aln->cigar_off;
    p.cigar = aln->cigar;
    p.cigar_cap = aln->cigar ? aln->cigar_cap : 0;
    p.strand = strand;
    p.score = score;
    p.frags = pairs ? n_rows / 2 : n_rows;
    p.k_none = (ref_len + 65536) << 1;
    p.pairs = pairs ? 1u : 0u;
    p.order = order;
    p.dup = dup;
    p.n_dup = reinterpret_cast<unsigned long long*>(n_dup);
    StreamTmp tmp(st);
    // no fragments: nothing to flag, but the count is still the call's to write
    if (p.frags && (rc = tmp.alloc(msw::markdup_tmp_bytes(p.frags, pairs != 0)))) return rc;
    HIP_TRY(msw::launch_markdup(p, bit_length(p.k_none), tmp.p, st));
    return MSW_OK;
}

int msw_aln_order_device(msw_ctx* ctx, const int64_t* ref_pos, const uint8_t* strand, uint64_t n, uint64_t ref_len,
                         uint32_t* order, void* stream) {
    int rc;
    if ((rc = check_order(ctx, ref_pos, n, ref_len, order))) return rc;
    if (n == 0) return MSW_OK;
    if ((rc = set_device(ctx))) return rc;
    const uint64_t k_last = ref_len ? ref_len << 1 : 1ull << 63;
    StreamTmp tmp(call_stream(ctx, stream));
    if ((rc = tmp.alloc(msw::aln_order_tmp_bytes(n)))) return rc;
    HIP_TRY(msw::launch_aln_order(ref_pos, strand, n, k_last, bit_length(k_last), order, tmp.p, tmp.st));
    return MSW_OK;
}

int msw_markdup(msw_ctx* ctx, const msw_aln_t* aln, const uint8_t* strand, const int32_t* score, uint64_t n_rows,
                uint64_t ref_len, int pairs, uint32_t* order, uint8_t* dup, uint64_t* n_dup) {
    int rc;
    if ((rc = check_markdup(ctx, aln, score, n_rows, ref_len, pairs, order, dup))) return rc;
    if (n_dup) *n_dup = 0;
    if (n_rows == 0) return MSW_OK;
    // the offsets decide what is uploaded: they must be a prefix sum inside the capacity
    for (uint64_t k = 0; k < n_rows; ++k)
        if (aln->cigar_off[k + 1] < aln->cigar_off[k])
            return fail(MSW_E_INVALID, "mark duplicates: cigar_off decreases at read %llu", (unsigned long long)k);
    const uint64_t ops = aln->cigar_off[n_rows];
    if (ops > aln->cigar_cap)
        return fail(MSW_E_INVALID, "mark duplicates: the reads hold %u ops, cigar_cap is %llu",
                    aln->cigar_off[n_rows], (unsigned long long)aln->cigar_cap);
    if (ops && !aln->cigar) return fail(MSW_E_INVALID, "NULL array");
    if ((rc = set_device(ctx))) return rc;
    const uint64_t frags = pairs ? n_rows / 2 : n_rows;
    DeviceArena a;
    const auto d_ref = a.take<int64_t>(n_rows);
    const auto d_cnt = a.take<uint64_t>(1);
    const auto d_nm = a.take<int32_t>(n_rows), d_score = a.take<int32_t>(n_rows);
    const auto d_off = a.take<uint32_t>(n_rows + 1), d_ops = a.take<uint32_t>(ops), d_order = a.take<uint32_t>(frags);
    const auto d_strand = a.take<uint8_t>(strand ? n_rows : 0), d_dup = a.take<uint8_t>(n_rows);
    if ((rc = a.alloc())) return rc;
    ChunkCopy cp(ctx->compute);
    cp.up(d_ref, aln->ref_pos, n_rows * 8);
    cp.up(d_nm, aln->nm, n_rows * 4);
    cp.up(d_score, score, n_rows * 4);
    cp.up(d_off, aln->cigar_off, (n_rows + 1) * 4);
    cp.up(d_ops, aln->cigar, ops * 4);
    if (strand) cp.up(d_strand, strand, n_rows);
    if (cp.ok()) {
        msw_aln_t dev = {d_ref, d_nm, d_off, d_ops, ops, nullptr};
        rc = msw_markdup_device(ctx, &dev, strand ? (const uint8_t*)d_strand : nullptr, d_score, n_rows, ref_len,
                                pairs, d_order, d_dup, d_cnt, cp.st);
    }
    if (rc == MSW_OK) {
        cp.down(order, d_order, frags * 4);
        cp.down(dup, d_dup, n_rows);
        if (n_dup) cp.down(n_dup, d_cnt, 8);
        cp.sync();
    }
    return cp.finish(rc, "mark duplicates");
}

int msw_aln_order(msw_ctx* ctx, const int64_t* ref_pos, const uint8_t* strand, uint64_t n, uint64_t ref_len,
                  uint32_t* order) {
    int rc;
    if ((rc = check_order(ctx, ref_pos, n, ref_len, order))) return rc;
    if (n == 0) return MSW_OK;
    if ((rc = set_device(ctx))) return rc;
    DeviceArena a;
    const auto d_ref = a.take<int64_t>(n);
    const auto d_order = a.take<uint32_t>(n);
    const auto d_strand = a.take<uint8_t>(strand ? n : 0);
    if ((rc = a.alloc())) return rc;
    ChunkCopy cp(ctx->compute);
    cp.up(d_ref, ref_pos, n * 8);
    if (strand) cp.up(d_strand, strand, n);
    if (cp.ok())
        rc = msw_aln_order_device(ctx, d_ref, strand ? (const uint8_t*)d_strand : nullptr, n, ref_len, d_order, cp.st);
    if (rc == MSW_OK) {
        cp.down(order, d_order, n * 4);
        cp.sync();
    }
    return cp.finish(rc, "coordinate order");
}

}  // extern "C"
