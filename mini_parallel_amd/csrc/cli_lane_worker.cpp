// cli_lane_worker.cpp -- one worker of the GPU lane reader (`rustseq_mini
// --full-wgs`, sw mode, BGZF lane files): it takes whole files, has them
// inflated, parsed and scored on its GPU, and sums / writes the per-read
// results on the host, one batch behind the GPU over two result sets.
#include <fcntl.h>

#include "cli_aln_block.h"
#include "cli_wgs.h"
#include "msw_fastq.h"

namespace {

// What the alignment steps need of their worker.
struct LaneEnv {
    msw_ctx* ctx;
    const msw_scoring_t* sc;
    msw_genome* gen;
    const Args* a;
    uint64_t batch;
    int gi;
    msw_pileup* pile;  // --pileup-out: this worker's pileup, else null
    uint32_t min_baseq;  // --pileup-min-baseq; above 0 the reader keeps quality rows
    bool qsum;           // --call-baseq: the pileup carries quality sums, every add goes with the quality rows
};

// The pinned result block of a set: score i32 | ei i16 | ej i16 | rlen u16 | wlen u16, each [batch]
struct HostResults {
    int32_t* score = nullptr;
    int16_t *end_i = nullptr, *end_j = nullptr;
    uint16_t *read_len = nullptr, *win_len = nullptr;
    static size_t bytes(uint64_t batch) { return batch * (4 + 2 + 2 + 2 + 2); }
    HostResults() = default;
    HostResults(uint8_t* base, uint64_t batch)
        : score((int32_t*)base), end_i((int16_t*)(base + batch * 4)), end_j(end_i + batch),
          read_len((uint16_t*)(end_j + batch)), win_len(read_len + batch) {}
};

// The pinned alignment block of a set: ref_pos i64 [batch] | nm i32 [batch] |
// off u32 [batch + 2], the overflow count being off[batch + 1] as on the device
struct HostAln {
    int64_t* ref_pos = nullptr;
    int32_t* nm = nullptr;
    uint32_t *off = nullptr, *overflow = nullptr;
    static size_t bytes(uint64_t batch) { return batch * 12 + (batch + 2) * 4; }
    HostAln() = default;
    HostAln(uint8_t* base, uint64_t batch)
        : ref_pos((int64_t*)base), nm((int32_t*)(base + batch * 8)), off((uint32_t*)(base + batch * 12)),
          overflow(off + batch + 1) {}
};

// --alignments-out: a batch's trace, its records and packed ops.
struct AlnSet {
    int16_t *d_si = nullptr, *d_sj = nullptr;
    int32_t *d_nc = nullptr, *d_nm = nullptr;
    int64_t* d_ref = nullptr;
    uint32_t* d_off = nullptr;    // [batch + 2]: offsets, then the overflow count at [batch + 1]
    uint32_t* d_rows = nullptr;   // [batch][aln_stride]
    uint32_t* d_exact = nullptr;  // rows at the exact stride, made by the first batch that needs them
    uint64_t exact_words = 0;
    uint32_t *d_ops = nullptr, *h_ops = nullptr;  // packed ops, device / pinned
    uint64_t ops_cap = 0;
    HostAln h;
    msw_dev_reads_t d{};  // the batch's device arrays (valid until the reader's call after next)
    const uint8_t* quals = nullptr;  // --pileup-min-baseq: the batch's quality rows, of the same lifetime
    uint32_t qual_stride = 0;
    void* stream = nullptr;
    uint32_t stride = 0;  // of the rows the offsets on the host were packed from
    const uint32_t* rows = nullptr;
    uint64_t fence = 0, n_ops = 0;
    bool pending = false, ok = false;
    std::vector<uint8_t> block;  // the .aln block of the batch

    void alloc(const LaneEnv& e, uint32_t aln_stride) {
        const uint64_t batch = e.batch;
        d_si = (int16_t*)msw_dev_alloc(e.ctx, batch * 2);
        d_sj = (int16_t*)msw_dev_alloc(e.ctx, batch * 2);
        d_nc = (int32_t*)msw_dev_alloc(e.ctx, batch * 4);
        d_nm = (int32_t*)msw_dev_alloc(e.ctx, batch * 4);
        d_ref = (int64_t*)msw_dev_alloc(e.ctx, batch * 8);
        d_off = (uint32_t*)msw_dev_alloc(e.ctx, (batch + 2) * 4);
        d_rows = (uint32_t*)msw_dev_alloc(e.ctx, batch * aln_stride * 4);
        // every read within the stride: at most stride + 2 ops each
        ops_cap = batch * ((uint64_t)aln_stride + 2);
        d_ops = (uint32_t*)msw_dev_alloc(e.ctx, ops_cap * 4);
        h_ops = (uint32_t*)msw_host_alloc(ops_cap * 4);
        uint8_t* ha = (uint8_t*)msw_host_alloc(HostAln::bytes(batch));
        if (!d_si || !d_sj || !d_nc || !d_nm || !d_ref || !d_off || !d_rows || !d_ops || !h_ops || !ha)
            die(std::string("GPU lane reader alignment buffers: ") + msw_last_error());
        h = HostAln(ha, batch);
        block.reserve(32 + batch * 24 + batch * 12);
    }

    // GPU side of a batch on its stream: trace straight from the genome (or
    // only pack again, into grown buffers), pack, and copy back the records
    // and offsets -- the packed ops follow once the host knows how many
    // there are.  o: the batch's scores and end cells on the device.
    bool run(const LaneEnv& e, const msw_out_t& o, uint32_t stride_, uint32_t* rows_, bool trace) {
        msw_trace_t tr{d_si, d_sj, d_nc, rows_, stride_};
        msw_aln_t al{d_ref, d_nm, d_off, d_ops, ops_cap, d_off + e.batch + 1};
        stride = stride_;
        rows = rows_;
        return (!trace || msw_trace_reads_device(e.ctx, e.sc, e.gen, d.reads, d.read_len, d.read_stride, d.pos, d.n,
                                                 window_for(*e.a, 0), d.max_len, &o, &tr, stream) == MSW_OK) &&
               msw_aln_pack_device(e.ctx, e.gen, d.reads, d.read_len, d.read_stride, d.pos, d.n, &o, &tr, &al,
                                   stream) == MSW_OK &&
               msw_memcpy_d2h_async(e.ctx, h.ref_pos, d_ref, d.n * 8, stream) == MSW_OK &&
               msw_memcpy_d2h_async(e.ctx, h.nm, d_nm, d.n * 4, stream) == MSW_OK &&
               msw_memcpy_d2h_async(e.ctx, h.off, d_off, (d.n + 1) * 4, stream) == MSW_OK &&
               msw_memcpy_d2h_async(e.ctx, h.overflow, d_off + e.batch + 1, 4, stream) == MSW_OK &&
               msw_fence_record(e.ctx, stream, &fence) == MSW_OK;
    }

    // Rows for one more trace of the batch's n reads at the exact stride: no
    // alignment has more ops than rows + columns.  0 when they cannot be had.
    uint32_t exact_rows(const LaneEnv& e, uint64_t n) {
        const uint32_t s = d.max_len + window_for(*e.a, d.max_len);
        if (n * s > exact_words) {
            if (d_exact) msw_dev_free(e.ctx, d_exact);
            exact_words = n * s;
            d_exact = (uint32_t*)msw_dev_alloc(e.ctx, exact_words * 4);
            if (!d_exact) {
                exact_words = 0;
                return 0;
            }
        }
        return s;
    }

    void grow_ops(const LaneEnv& e, uint64_t cap) {
        msw_dev_free(e.ctx, d_ops);
        msw_host_free(h_ops);
        ops_cap = cap;
        d_ops = (uint32_t*)msw_dev_alloc(e.ctx, ops_cap * 4);
        h_ops = (uint32_t*)msw_host_alloc(ops_cap * 4);
        if (!d_ops || !h_ops) die(std::string("GPU lane reader alignment buffers: ") + msw_last_error());
    }

    // Host side, while the batch's n reads are still on the device (before
    // the reader's call after next): a batch with reads past the stride is
    // traced and packed once more at the exact stride, so the file's
    // alignments are always complete; then the packed ops actually used are
    // copied back and set_fence covers everything settle reads.
    // With --pileup-out the settled records go into the worker's pileup
    // here, on the batch's stream: after the retrace and the ops growth, so
    // every read has its final ops exactly once, and before the ops copy-back
    // (strand / mapq: the set's bytes on the device, or null).
    void finish(const LaneEnv& e, const msw_out_t& o, uint64_t n, FileState& f, uint64_t* set_fence,
                const uint8_t* strand, const uint8_t* mapq) {
        if (!pending) return;
        pending = false;
        ok = false;
        n_ops = 0;
        bool good = true, exact = false;
        for (;;) {
            if (!(good = msw_fence_wait(e.ctx, fence) == MSW_OK)) break;
            if (*h.overflow != 0 && !exact) {
                exact = true;
                const uint32_t s = exact_rows(e, n);
                if (!(good = s != 0 && run(e, o, s, d_exact, true))) break;
                continue;
            }
            if (h.off[n] > ops_cap) {  // after an exact trace only: grow, pack again
                grow_ops(e, h.off[n]);
                if (!(good = run(e, o, stride, const_cast<uint32_t*>(rows), false))) break;
                continue;
            }
            break;
        }
        if (good && e.pile) {
            const msw_aln_t al{d_ref, d_nm, d_off, d_ops, ops_cap, d_off + e.batch + 1};
            // the quality rows are the reader's, in the order of the file, whichever way d.reads is oriented
            good = (e.min_baseq || e.qsum ? msw_pileup_add_qual_device(e.ctx, e.pile, d.reads, d.read_len, d.read_stride, n, &al,
                                                             strand, mapq, (uint32_t)e.a->pileup_min_mapq, quals,
                                                             qual_stride, e.min_baseq, stream)
                                : msw_pileup_add_device(e.ctx, e.pile, d.reads, d.read_len, d.read_stride, n, &al, strand,
                                                        mapq, (uint32_t)e.a->pileup_min_mapq, stream)) == MSW_OK;
        }
        if (good) {
            n_ops = h.off[n];
            good = (n_ops == 0 || msw_memcpy_d2h_async(e.ctx, h_ops, d_ops, n_ops * 4, stream) == MSW_OK);
        }
        if (!good) {
            fprintf(stderr, "  GPU %d alignment records error: %s\n", e.gi, msw_last_error());
            f.failed = true;
            (void)msw_synchronize(e.ctx);
        }
        ok = good;
        // what settle waits on
        if (msw_fence_record(e.ctx, stream, set_fence) != MSW_OK) {
            f.failed = true;
            ok = false;
            *set_fence = 0;
        }
    }
};

// One of a worker's two result sets: batch k's copy-back lands while batch k+1 runs.
struct ResultSet {
    int32_t* d_score = nullptr;
    int16_t *d_ei = nullptr, *d_ej = nullptr;
    uint16_t* d_wlen = nullptr;
    HostResults h;
    uint64_t n = 0, first = 0;
    size_t fi = 0;
    uint64_t fence = 0;  // after the batch's copy-back (msw_fence_record)
    bool live = false;
    uint64_t* rec = nullptr;  // --scores-out: the batch's records (recbuf)
    // --both-strands: the batch's oriented rows [batch][read_stride()] and
    // strand bytes.  They belong to the set, not to the reader, so the trace
    // and a second trace at the exact stride read them while the set is live.
    uint8_t *d_oriented = nullptr, *d_strand = nullptr, *h_strand = nullptr;
    // --map: the batch's seeded window positions (they take the place of the
    // reader's pos array in the scoring call, the trace and the pack), votes,
    // hits and flags; the votes come back to count the placed reads
    int64_t* d_wpos = nullptr;
    uint32_t *d_votes = nullptr, *d_hits = nullptr, *h_votes = nullptr;
    uint8_t* d_flags = nullptr;
    // --mapq: the second candidate's positions, votes and flags, its scoring
    // results (and with --both-strands its strand bytes and oriented rows),
    // and what the selection writes.  The selection leaves the winner in the
    // set's own arrays above, so everything after it reads those as before.
    int64_t* d_wpos1 = nullptr;
    uint32_t* d_votes1 = nullptr;
    uint8_t* d_flags1 = nullptr;
    int32_t* d_score1 = nullptr;
    int16_t *d_ei1 = nullptr, *d_ej1 = nullptr;
    uint16_t* d_wlen1 = nullptr;
    uint8_t *d_strand1 = nullptr, *d_oriented1 = nullptr;
    uint8_t *d_mapq = nullptr, *d_cand = nullptr, *h_mapq = nullptr;
    int32_t *d_sub = nullptr, *h_sub = nullptr;
    AlnSet aln;
    msw_out_t out() const { return msw_out_t{d_score, d_ei, d_ej}; }
    msw_out_t out1() const { return msw_out_t{d_score1, d_ei1, d_ej1}; }
};

class LaneWorker {
   public:
    LaneWorker(LaneRun& lanes, int wi);
    void run();

   private:
    bool open_next(size_t* fi_out);
    void reader_done(size_t fi);
    void maybe_finish(size_t fi);
    void finish_alignments(ResultSet& r);
    bool next_batch(size_t fi, void* stream, msw_dev_reads_t* d);
    void settle(ResultSet& r);
    void write_aln_block(ResultSet& r, FileState& f);
    void collect_pileup();
    bool score(ResultSet& r, const msw_dev_reads_t& d, const int64_t* pos, bool alt, void* stream);
    bool submit(ResultSet& r, const msw_dev_reads_t& d, size_t fi, void* stream);
    int open_out(const std::string& dir, const FileState& f, const char* ext);

    LaneRun& lanes_;
    WgsRun& run_;
    const Args& a_;
    const int wi_, gi_;
    const bool aln_, both_, map_, mapq_;
    const uint64_t batch_;
    Clock::time_point ts0_;
    Ctx ctx_;
    void* streams_[2] = {nullptr, nullptr};
    msw_gfastq* gr_ = nullptr;  // one reader per worker, reset per file (buffers kept)
    size_t pending_ = LaneRun::kNone;  // the file claimed ahead and prefetched
    msw_scoring_t sc_;
    msw_genome* gen_ = nullptr;
    msw_index* idx_ = nullptr;  // --map
    msw_pileup* pile_ = nullptr;  // --pileup-out
    uint32_t min_baseq_ = 0;      // --pileup-min-baseq (0: the reader keeps no qualities, unless qsum_)
    bool qsum_ = false;           // --call-baseq: quality rows and a MSW_PILEUP_QSUM pileup
    const uint8_t* batch_quals_ = nullptr;  // the quality rows of the batch next_batch returned last
    msw_seed_params_t seed_{};
    LaneEnv env_;
    ResultSet res_[2];
    uint32_t aln_stride_ = 16;  // ops per read the first trace's rows hold (tests set 1 to force the second trace)
    std::unique_ptr<uint64_t[]> recbuf_;
    unsigned long long alg_local_ = 0;
    // per file this worker has open: batches in flight, reader done
    std::map<size_t, std::pair<int, bool>> open_files_;
    int cur_ = 0;
};

// Setup, before the clock: context and streams, lane reader, the first file's
// prefetch, genome, kernels, result sets.
LaneWorker::LaneWorker(LaneRun& lanes, int wi)
    : lanes_(lanes), run_(lanes.run), a_(lanes.run.a), wi_(wi), gi_(wi % lanes.run.ngpu), aln_(lanes.aln),
      both_(lanes.both), map_(lanes.run.a.map), mapq_(lanes.run.a.mapq), batch_(lanes.batch), ts0_(Clock::now()),
      // lean: a GPU-reader worker scores device-resident batches
      // only, so its context makes just the compute stream
      ctx_(lanes.run.devices[gi_].ordinal, MSW_CTX_LEAN) {
    // With per-read records (256k-read batches) the batches
    // alternate over two streams (with the two result sets), so
    // one batch's read emit and window cut run beside the other
    // batch's scoring instead of between two launches: config 3
    // from FASTQ 13.67-13.99 -> 13.25-13.74 ms.  Sums only (1 M-read
    // batches that fill the GPU alone) keep one stream: config 4
    // measured 3 % slower on two.
    if (lanes_.per_read && msw_stream_create(ctx_.h, &streams_[1]) != MSW_OK)
        die(std::string("GPU stream: ") + msw_last_error());
    const double t_ctx = ms_since(ts0_);
    // --pileup-min-baseq above 0: the reader keeps the records' quality lines beside the reads
    min_baseq_ = lanes_.pileup && a_.pileup_min_baseq > 0 ? (uint32_t)a_.pileup_min_baseq : 0u;
    // --call-baseq: the quality lines too, at --pileup-min-baseq 0 as well
    qsum_ = lanes_.pileup && a_.call_baseq;
    if ((min_baseq_ || qsum_ ? msw_gfastq_open_ex(ctx_.h, nullptr, read_stride(), batch_, MSW_GFASTQ_POS | MSW_GFASTQ_QUAL, 0, &gr_)
                    : msw_gfastq_open(ctx_.h, nullptr, read_stride(), batch_, 1, 0, &gr_)) != MSW_OK)
        die(std::string("GPU lane reader: ") + msw_last_error());
    const double t_rd = ms_since(ts0_) - t_ctx;
    // the first file: claimed now and opened / pinned on the
    // reader's thread (msw_gfastq_prefetch) while this worker
    // uploads the genome and allocates its result sets, so its
    // first window is ready when the clock starts (the same work
    // on a helper thread beside the reader's buffers measured
    // equal, and starting the prefetch later cost ~0.5 ms of the
    // timed region: profiles/r06/c3f/setup_ab.jsonl)
    pending_ = lanes_.claim();
    if (pending_ != LaneRun::kNone) (void)msw_gfastq_prefetch(gr_, run_.st[pending_]->path.c_str());
    sc_ = scoring_of(a_, lanes_.per_read);
    const auto tg0 = Clock::now();
    const std::string& ref_seq = run_.genome();
    if (msw_genome_create(ctx_.h, (const uint8_t*)ref_seq.data(), ref_seq.size(), &gen_) != MSW_OK)
        die(std::string("GPU genome upload error: ") + msw_last_error());
    const double t_gen = ms_since(tg0);
    // --map: the k-mer index of the genome just uploaded, before the clock
    const auto ti0 = Clock::now();
    if (map_) {
        if (msw_index_create(ctx_.h, gen_, (uint32_t)a_.seed_k, (uint32_t)a_.seed_max_occ, &idx_) != MSW_OK)
            die(std::string("GPU k-mer index error: ") + msw_last_error());
        seed_ = msw_seed_params_t{(uint32_t)a_.seed_band, 4096u, 1u, 1u, window_for(a_, 0)};
    }
    const double t_ix = map_ ? ms_since(ti0) : 0.0;
    // the scoring kernels' modules, loaded now rather than at the first batch
    const auto tk0 = Clock::now();
    if (msw_ctx_prepare(ctx_.h, &sc_) != MSW_OK) die(std::string("GPU kernel load: ") + msw_last_error());
    const double t_kl = ms_since(tk0);
    const auto tres0 = Clock::now();
    // --pileup-out: this worker's pileup of the genome just uploaded, before the clock
    if (lanes_.pileup && msw_pileup_create_ex(ctx_.h, gen_, qsum_ ? MSW_PILEUP_QSUM : 0u, &pile_) != MSW_OK)
        die(std::string("GPU pileup error: ") + msw_last_error());
    env_ = LaneEnv{ctx_.h, &sc_, gen_, &a_, batch_, gi_, pile_, min_baseq_, qsum_};
    if (aln_) aln_stride_ = (uint32_t)std::min(4480L, std::max(1L, atol(env_or("MSW_CLI_CIGAR_STRIDE", "16").c_str())));
    for (ResultSet& r : res_) {
        r.d_score = (int32_t*)msw_dev_alloc(ctx_.h, batch_ * 4);
        r.d_ei = (int16_t*)msw_dev_alloc(ctx_.h, batch_ * 2);
        r.d_ej = (int16_t*)msw_dev_alloc(ctx_.h, batch_ * 2);
        r.d_wlen = (uint16_t*)msw_dev_alloc(ctx_.h, batch_ * 2);
        uint8_t* h = (uint8_t*)msw_host_alloc(HostResults::bytes(batch_));
        if (!r.d_score || !r.d_ei || !r.d_ej || !r.d_wlen || !h)
            die(std::string("GPU lane reader buffers: ") + msw_last_error());
        r.h = HostResults(h, batch_);
        if (both_) {
            r.d_oriented = (uint8_t*)msw_dev_alloc(ctx_.h, batch_ * read_stride());
            r.d_strand = (uint8_t*)msw_dev_alloc(ctx_.h, batch_);
            r.h_strand = (uint8_t*)msw_host_alloc(batch_);
            if (!r.d_oriented || !r.d_strand || !r.h_strand)
                die(std::string("GPU lane reader strand buffers: ") + msw_last_error());
        }
        if (map_) {
            r.d_wpos = (int64_t*)msw_dev_alloc(ctx_.h, batch_ * 8);
            r.d_votes = (uint32_t*)msw_dev_alloc(ctx_.h, batch_ * 4);
            r.d_hits = (uint32_t*)msw_dev_alloc(ctx_.h, batch_ * 4);
            r.d_flags = (uint8_t*)msw_dev_alloc(ctx_.h, batch_);
            r.h_votes = (uint32_t*)msw_host_alloc(batch_ * 4);
            if (!r.d_wpos || !r.d_votes || !r.d_hits || !r.d_flags || !r.h_votes)
                die(std::string("GPU lane reader seed buffers: ") + msw_last_error());
        }
        if (mapq_) {
            r.d_wpos1 = (int64_t*)msw_dev_alloc(ctx_.h, batch_ * 8);
            r.d_votes1 = (uint32_t*)msw_dev_alloc(ctx_.h, batch_ * 4);
            r.d_flags1 = (uint8_t*)msw_dev_alloc(ctx_.h, batch_);
            r.d_score1 = (int32_t*)msw_dev_alloc(ctx_.h, batch_ * 4);
            r.d_ei1 = (int16_t*)msw_dev_alloc(ctx_.h, batch_ * 2);
            r.d_ej1 = (int16_t*)msw_dev_alloc(ctx_.h, batch_ * 2);
            r.d_wlen1 = (uint16_t*)msw_dev_alloc(ctx_.h, batch_ * 2);
            r.d_mapq = (uint8_t*)msw_dev_alloc(ctx_.h, batch_);
            r.d_cand = (uint8_t*)msw_dev_alloc(ctx_.h, batch_);
            r.d_sub = (int32_t*)msw_dev_alloc(ctx_.h, batch_ * 4);
            r.h_mapq = (uint8_t*)msw_host_alloc(batch_);
            r.h_sub = (int32_t*)msw_host_alloc(batch_ * 4);
            if (both_) {
                r.d_strand1 = (uint8_t*)msw_dev_alloc(ctx_.h, batch_);
                r.d_oriented1 = (uint8_t*)msw_dev_alloc(ctx_.h, batch_ * read_stride());
            }
            if (!r.d_wpos1 || !r.d_votes1 || !r.d_flags1 || !r.d_score1 || !r.d_ei1 || !r.d_ej1 || !r.d_wlen1 ||
                !r.d_mapq || !r.d_cand || !r.d_sub || !r.h_mapq || !r.h_sub ||
                (both_ && (!r.d_strand1 || !r.d_oriented1)))
                die(std::string("GPU lane reader candidate buffers: ") + msw_last_error());
        }
    }
    // per-read records of a batch, built here and written from here:
    // allocated and touched in setup (a fresh 2 MB buffer per batch
    // page-faulted inside the last batch's settle, after the GPU)
    if (!a_.scores_out.empty()) {
        recbuf_.reset(new uint64_t[2 * batch_]);  // one half per result set
        memset(recbuf_.get(), 0, 2 * batch_ * sizeof(uint64_t));
        res_[0].rec = recbuf_.get();
        res_[1].rec = recbuf_.get() + batch_;
    }
    if (aln_)
        for (ResultSet& r : res_) r.aln.alloc(env_, aln_stride_);
    run_.setup_phase(t_ctx, t_gen, ms_since(tres0), t_rd, t_kl, t_ix);
}

void LaneWorker::maybe_finish(size_t fi) {
    auto it = open_files_.find(fi);
    if (it == open_files_.end() || it->second.first > 0 || !it->second.second) return;
    open_files_.erase(it);
    run_.finish_file(fi);
}

// the reader's stats of the file it just finished
void LaneWorker::reader_done(size_t fi) {
    uint64_t bi = 0, bo = 0;
    msw_gfastq_stats(gr_, nullptr, nullptr, nullptr, nullptr, &bi, &bo);
    lanes_.gz_in += bi;
    lanes_.gz_out += bo;
    run_.st[fi]->reader_done = true;
    open_files_[fi].second = true;
    maybe_finish(fi);
}

int LaneWorker::open_out(const std::string& dir, const FileState& f, const char* ext) {
    const std::string out = out_path(dir, f.path, ext);
    const int fd = open(out.c_str(), O_CREAT | O_TRUNC | O_WRONLY, 0644);
    if (fd < 0) die("error: cannot create " + out);
    return fd;
}

// next file for this worker: reset the reader (its compressed
// bytes start loading in the background), false when none is
// left.  The worker claims the file after it at the same time
// and has the reader pin that file's first window now
// (msw_gfastq_prefetch), so the next switch does not wait on it.
bool LaneWorker::open_next(size_t* fi_out) {
    constexpr size_t kNone = LaneRun::kNone;
    for (;;) {
        size_t fi = pending_ != kNone ? pending_ : lanes_.claim();
        pending_ = kNone;
        if (fi == kNone) {  // nothing left to claim: another worker's pending file
            for (size_t k : run_.todo)
                if (lanes_.started[k].load() == 0 && lanes_.start_file(k)) {
                    fi = k;
                    break;
                }
            if (fi == kNone) return false;
        } else if (!lanes_.start_file(fi)) {
            continue;  // taken by an idle worker meanwhile
        }
        FileState& f = *run_.st[fi];
        f.t0 = Clock::now();
        open_files_[fi] = {0, false};
        if (!a_.scores_out.empty()) f.scores_fd = open_out(a_.scores_out, f, ".scores");
        if (aln_) f.aln_fd = open_out(a_.alignments_out, f, ".aln");
        printf("  Processing file %zu/%zu: %s (GPU inflate)\n", run_.gidx[fi] + 1, run_.n_lane_files, f.path.c_str());
        fflush(stdout);
        if (msw_gfastq_reset(gr_, f.path.c_str()) != MSW_OK) {
            f.error = msw_last_error();
            fprintf(stderr, "  Error reading %s: %s\n", f.path.c_str(), f.error.c_str());
            f.failed = true;
            reader_done(fi);
            continue;
        }
        pending_ = lanes_.claim();
        if (pending_ != kNone) (void)msw_gfastq_prefetch(gr_, run_.st[pending_]->path.c_str());
        *fi_out = fi;
        return true;
    }
}

void LaneWorker::finish_alignments(ResultSet& r) {
    if (aln_ && r.live)
        r.aln.finish(env_, r.out(), r.n, *run_.st[r.fi], &r.fence, both_ ? r.d_strand : nullptr,
                     mapq_ ? r.d_mapq : nullptr);
}

// The reader's next batch of file fi on `stream`; false (after reader_done)
// on an error and at the end of the file.
bool LaneWorker::next_batch(size_t fi, void* stream, msw_dev_reads_t* d) {
    FileState& f = *run_.st[fi];
    if (msw_gfastq_next(gr_, stream, d) != MSW_OK) {
        f.error = msw_last_error();
        fprintf(stderr, "  Error reading %s: %s\n", f.path.c_str(), f.error.c_str());
        f.failed = true;
        reader_done(fi);
        return false;
    }
    batch_quals_ = nullptr;
    if ((min_baseq_ || qsum_) && msw_gfastq_quals(gr_, &batch_quals_) != MSW_OK) batch_quals_ = nullptr;
    run_.trace_ev(wi_, "batch", d->n);
    if (d->n == 0) reader_done(fi);
    return d->n != 0;
}

// one self-contained block: header, records, packed ops
void LaneWorker::write_aln_block(ResultSet& r, FileState& f) {
    std::vector<uint8_t>& block = r.aln.block;
    block.clear();
    append_aln_block(block, r.first, r.n, r.aln.h.ref_pos, r.h.score, r.aln.h.nm, r.aln.h.off, r.h.end_i, r.h.end_j,
                     r.aln.h_ops, r.aln.n_ops, both_ ? r.h_strand : nullptr, mapq_ ? r.h_mapq : nullptr,
                     mapq_ ? r.h_sub : nullptr);
    size_t done = 0;
    while (done < block.size()) {
        const ssize_t w = write(f.aln_fd, block.data() + done, block.size() - done);
        if (w <= 0) break;
        done += (size_t)w;
    }
    if (done != block.size()) {
        fprintf(stderr, "  error writing alignments for %s\n", f.path.c_str());
        f.failed = true;
    }
}

// --pileup-out, after the clock has stopped: fold this worker's pileup (every
// add has finished: both sets are settled), copy the counts out and add them
// to the run's.
void LaneWorker::collect_pileup() {
    const size_t words = (size_t)msw_genome_length(gen_) * 8;
    std::vector<uint32_t> mine(words);
    msw_pileup_summary_t s;
    uint64_t lowq = 0;
    std::vector<uint32_t> mine_q(qsum_ ? words / 2 : 0);
    const bool ok = msw_pileup_finish(ctx_.h, pile_, nullptr) == MSW_OK &&
                    msw_pileup_counts(ctx_.h, pile_, mine.data()) == MSW_OK &&
                    (!qsum_ || msw_pileup_qsums(ctx_.h, pile_, mine_q.data()) == MSW_OK) &&
                    msw_pileup_summary(ctx_.h, pile_, 1, &s) == MSW_OK &&
                    (!min_baseq_ || msw_pileup_lowq_columns(ctx_.h, pile_, &lowq) == MSW_OK);
    if (!ok) fprintf(stderr, "  GPU %d pileup error: %s\n", gi_, msw_last_error());
    std::lock_guard<std::mutex> lk(lanes_.pile_mu);
    if (!ok) {
        lanes_.pile_failed = true;
        return;
    }
    if (lanes_.pile_sum.empty()) {
        lanes_.pile_sum.swap(mine);
    } else {
        uint32_t* sum = lanes_.pile_sum.data();
        for (size_t k = 0; k < words; ++k) sum[k] += mine[k];
    }
    if (qsum_) {
        if (lanes_.qsum_sum.empty()) {
            lanes_.qsum_sum.swap(mine_q);
        } else {
            uint32_t* sum = lanes_.qsum_sum.data();
            for (size_t k = 0; k < mine_q.size(); ++k) sum[k] += mine_q[k];
        }
    }
    lanes_.pile_used += s.reads_used;
    lanes_.pile_skipped += s.reads_skipped;
    lanes_.pile_lowq += lowq;
}

// host side of a finished batch: sums, cells, per-read records, then this
// worker's file table
void LaneWorker::settle(ResultSet& r) {
    if (!r.live) return;
    finish_alignments(r);
    r.live = false;
    FileState& f = *run_.st[r.fi];
    run_.trace_ev(wi_, "settle-wait", r.n);
    if (msw_fence_wait(ctx_.h, r.fence) != MSW_OK) {
        fprintf(stderr, "  GPU %d alignment error: %s\n", gi_, msw_last_error());
        f.failed = true;
    } else {
        const HostResults& h = r.h;
        long long sum = 0;
        unsigned long long cl = 0, nb = 0, nw = 0;
        // records [score i32 | end_i i16 | end_j i16], built as whole
        // words in the same pass as the sums
        uint64_t* rec = f.scores_fd >= 0 ? r.rec : nullptr;
        for (uint64_t i = 0; i < r.n; ++i) {
            sum += h.score[i];
            cl += (unsigned long long)h.read_len[i] * h.win_len[i];
            nb += h.read_len[i];
            nw += h.win_len[i];
            if (rec) rec[i] = score_record(h.score[i], h.end_i[i], h.end_j[i]);
        }
        alg_local_ += nb + nw + (sc_.want_coords ? 8ull : 4ull) * r.n;
        f.score += sum;
        f.bases += nb;
        f.reads += r.n;
        run_.cells += cl;
        if (both_) {
            unsigned long long rev = 0;
            for (uint64_t i = 0; i < r.n; ++i) rev += r.h_strand[i];
            run_.reverse_reads += rev;
        }
        if (map_) {
            unsigned long long placed = 0;
            for (uint64_t i = 0; i < r.n; ++i) placed += r.h_votes[i] >= seed_.min_votes;  // win_pos >= 0
            run_.placed_reads += placed;
        }
        if (mapq_) {
            unsigned long long hist[4] = {0, 0, 0, 0};
            for (uint64_t i = 0; i < r.n; ++i) {
                const uint8_t q = r.h_mapq[i];
                hist[q == 0 ? 0 : q < 30 ? 1 : q < 60 ? 2 : 3] += 1;
            }
            for (int k = 0; k < 4; ++k) run_.mapq_hist[k] += hist[k];
        }
        if (rec && pwrite(f.scores_fd, rec, r.n * 8, (off_t)(r.first * 8)) != (ssize_t)(r.n * 8)) {
            fprintf(stderr, "  error writing scores for %s\n", f.path.c_str());
            f.failed = true;
        }
        if (f.aln_fd >= 0 && r.aln.ok) write_aln_block(r, f);
    }
    open_files_[r.fi].first -= 1;
    maybe_finish(r.fi);
    run_.trace_ev(wi_, "settled", r.n);
}

// One scoring call of batch d at the window positions `pos`, into the set's
// own result arrays or (alt) into its second candidate's.
bool LaneWorker::score(ResultSet& r, const msw_dev_reads_t& d, const int64_t* pos, bool alt, void* stream) {
    msw_out_t o = alt ? r.out1() : r.out();
    uint16_t* wlen = alt ? r.d_wlen1 : r.d_wlen;
    return (both_ ? msw_align_reads_strands_device(ctx_.h, &sc_, gen_, d.reads, d.read_len, d.read_stride, pos, d.n,
                                                   window_for(a_, 0), d.max_len, &o, wlen,
                                                   alt ? r.d_strand1 : r.d_strand, alt ? r.d_oriented1 : r.d_oriented,
                                                   read_stride(), stream)
                  : msw_align_reads_device(ctx_.h, &sc_, gen_, d.reads, d.read_len, d.read_stride, pos, d.n,
                                           window_for(a_, 0), d.max_len, &o, wlen, stream)) == MSW_OK;
}

// Batch d of file fi into result set r on `stream`: scoring, the copy-back
// of the per-read results and, with --alignments-out, the trace and pack on
// the same stream (finish_alignments records r.fence after the packed ops).
// On an error everything in flight is waited for and the other set's
// alignments are finished while its reads are in place; false.
bool LaneWorker::submit(ResultSet& r, const msw_dev_reads_t& d, size_t fi, void* stream) {
    FileState& f = *run_.st[fi];
    msw_out_t o = r.out();
    // the reads the trace and the pack see: the reader's rows, or with
    // --both-strands the set's oriented rows
    msw_dev_reads_t da = d;
    if (both_) {
        da.reads = r.d_oriented;
        da.read_stride = read_stride();
    }
    // --map: seed on this batch's stream, in front of the scoring call; the
    // seeded positions then stand wherever the reader's stood
    const int64_t* pos = d.pos;
    bool seeded = true;
    if (map_) {
        const msw_seed_out_t so{r.d_wpos, r.d_votes, r.d_hits, r.d_flags};
        const msw_seed_alt_t sa{r.d_wpos1, r.d_votes1, r.d_flags1};
        const uint8_t* rc_rows = both_ ? r.d_oriented : nullptr;
        const uint32_t rc_stride = both_ ? read_stride() : 0;
        seeded = (!both_ || msw_revcomp_device(ctx_.h, d.reads, d.read_len, d.read_stride, d.n, r.d_oriented,
                                               read_stride(), stream) == MSW_OK) &&
                 // --mapq: the candidates call in the seeding call's place
                 (mapq_ ? msw_seed_candidates_device(ctx_.h, idx_, d.reads, rc_rows, d.read_len, d.read_stride, rc_stride,
                                                     d.n, d.max_len, &seed_, (uint32_t)a_.seed_sep, &so, &sa, stream)
                        : msw_seed_reads_device(ctx_.h, idx_, d.reads, rc_rows, d.read_len, d.read_stride, rc_stride, d.n,
                                                d.max_len, &seed_, &so, stream)) == MSW_OK &&
                 msw_memcpy_d2h_async(ctx_.h, r.h_votes, r.d_votes, d.n * 4, stream) == MSW_OK;
        pos = r.d_wpos;
        da.pos = r.d_wpos;
    }
    // --mapq: both candidates are scored and the selection leaves the better
    // one in the set's own arrays (scores, end cells, window lengths and
    // positions, strand bytes, oriented rows), before anything is copied back
    bool selected = true;
    if (seeded && mapq_) {
        const bool ends = sc_.want_coords != 0;
        const msw_cand_t c0{r.d_score, ends ? r.d_ei : nullptr, ends ? r.d_ej : nullptr, r.d_wlen,
                            both_ ? r.d_strand : nullptr, both_ ? r.d_oriented : nullptr, r.d_wpos};
        const msw_cand_t c1{r.d_score1, ends ? r.d_ei1 : nullptr, ends ? r.d_ej1 : nullptr, r.d_wlen1,
                            both_ ? r.d_strand1 : nullptr, both_ ? r.d_oriented1 : nullptr, r.d_wpos1};
        selected = score(r, d, r.d_wpos, false, stream) && score(r, d, r.d_wpos1, true, stream) &&
                   msw_mapq_select_device(ctx_.h, &c0, &c1, read_stride(), d.read_len, d.n, sc_.match, r.d_sub, r.d_mapq,
                                          r.d_cand, stream) == MSW_OK &&
                   msw_memcpy_d2h_async(ctx_.h, r.h_mapq, r.d_mapq, d.n, stream) == MSW_OK &&
                   msw_memcpy_d2h_async(ctx_.h, r.h_sub, r.d_sub, d.n * 4, stream) == MSW_OK;
    }
    if (!seeded || !selected || (!mapq_ && !score(r, d, pos, false, stream)) ||
        (both_ && msw_memcpy_d2h_async(ctx_.h, r.h_strand, r.d_strand, d.n, stream) != MSW_OK) ||
        msw_memcpy_d2h_async(ctx_.h, r.h.score, r.d_score, d.n * 4, stream) != MSW_OK ||
        // end cells only feed --scores-out records
        (sc_.want_coords && (msw_memcpy_d2h_async(ctx_.h, r.h.end_i, r.d_ei, d.n * 2, stream) != MSW_OK ||
                             msw_memcpy_d2h_async(ctx_.h, r.h.end_j, r.d_ej, d.n * 2, stream) != MSW_OK)) ||
        msw_memcpy_d2h_async(ctx_.h, r.h.read_len, d.read_len, d.n * 2, stream) != MSW_OK ||
        msw_memcpy_d2h_async(ctx_.h, r.h.win_len, r.d_wlen, d.n * 2, stream) != MSW_OK ||
        (aln_ ? (r.aln.d = da, r.aln.quals = batch_quals_, r.aln.qual_stride = d.read_stride, r.aln.stream = stream,
                 !r.aln.run(env_, o, aln_stride_, r.aln.d_rows, true))
              : msw_fence_record(ctx_.h, stream, &r.fence) != MSW_OK)) {
        fprintf(stderr, "  GPU %d alignment error: %s\n", gi_, msw_last_error());
        f.failed = true;
        (void)msw_synchronize(ctx_.h);
        finish_alignments(res_[cur_ ^ 1]);
        reader_done(fi);
        return false;
    }
    run_.trace_ev(wi_, "submitted", d.n);
    r.n = d.n;
    r.first = d.first_read;
    r.fi = fi;
    r.live = true;
    r.aln.pending = aln_;
    open_files_[fi].first += 1;
    return true;
}

// One loop over the batches of all of this worker's files: a
// file's last batches are settled after the next file's first
// batch is launched, so the next file's read, inflate and parse
// (reader stream) run beside this file's scoring (compute stream).
//
// The order the two result sets are held to:
//   1. a set's alignments are finished before the reader's call after next:
//      the reader's next batch reuses the slab of the batch before last,
//      which is the batch this set still traces from;
//   2. a set is settled before it is used again (the batch before last
//      used it), and not earlier: its host work runs beside the other
//      set's batch on the GPU;
//   3. when a submit fails, the other set's alignments are finished at
//      once, while its reads are in place (submit does it).
void LaneWorker::run() {
    run_.gate.arrive();
    size_t fi = 0;
    bool have = open_next(&fi);
    while (have) {
        ResultSet& r = res_[cur_];
        void* const stream = streams_[cur_];  // this batch's stream
        msw_dev_reads_t d;
        finish_alignments(r);
        if (!next_batch(fi, stream, &d)) {
            have = open_next(&fi);
            continue;
        }
        settle(r);
        if (!submit(r, d, fi, stream)) {
            have = open_next(&fi);
            continue;
        }
        cur_ ^= 1;
    }
    // (the last two batches' host work on two threads measured
    // equal: config 3 from FASTQ 13.22-13.42 vs 13.16-13.26 ms)
    settle(res_[cur_]);
    settle(res_[cur_ ^ 1]);
    run_.mark_done();
    if (pile_) collect_pileup();
    msw_ctx_stats(ctx_.h, &lanes_.gstats[(size_t)wi_], 0);
    lanes_.gstats[(size_t)wi_].alg_bytes = alg_local_;
    // the reader, result sets, genome and context stay allocated:
    // the process exits (_exit in main) once the record is written
    ctx_.keep = true;
}

}  // namespace

void lane_worker(LaneRun& lanes, int wi) {
    LaneWorker w(lanes, wi);
    w.run();
}
