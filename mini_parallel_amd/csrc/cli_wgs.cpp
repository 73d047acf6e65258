// cli_wgs.cpp -- `rustseq_mini --full-wgs`: the run's shared state (WgsRun),
// the GPU lane reader's start-up (its worker is cli_lane_worker.cpp) and the
// host-reader path: reader threads fill read slabs, a bounded queue hands
// chunks to one host thread per GPU (own msw_ctx), results are summed per file.
#include <deque>
#include <fstream>
#include <sstream>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>

#include "cli_wgs.h"
#include "msw_fastq.h"

std::string json_escape(const std::string& s) {
    std::string o;
    for (char c : s) {
        if (c == '"' || c == '\\') { o += '\\'; o += c; }
        else if ((unsigned char)c < 0x20) { char b[8]; snprintf(b, sizeof(b), "\\u%04x", c); o += b; }
        else o += c;
    }
    return o;
}

void Checkpoint::save() const {
    std::ostringstream o;
    size_t done = 0;
    for (auto& kv : files) done += kv.second.completed;
    o << "{\n  \"run_id\": \"" << json_escape(run_id) << "\",\n  \"files\": [";
    bool first = true;
    for (auto& kv : files) {
        const FileCheckpoint& f = kv.second;
        o << (first ? "\n" : ",\n") << "    {\"file_path\": \"" << json_escape(f.file_path)
          << "\", \"file_index\": " << f.file_index << ", \"score\": " << f.score
          << ", \"processing_time_ms\": " << f.processing_time_ms << ", \"total_bases\": " << f.total_bases
          << ", \"total_reads\": " << f.total_reads << ", \"completed\": " << (f.completed ? "true" : "false")
          << "}";
        first = false;
    }
    o << "\n  ],\n  \"total_files\": " << total_files << ",\n  \"completed_files\": " << done << "\n}\n";
    const std::string tmp = path + ".tmp";
    {
        std::ofstream f(tmp);
        f << o.str();
    }
    rename(tmp.c_str(), path.c_str());  // atomic replace
}

bool Checkpoint::load() {
    std::ifstream f(path);
    if (!f) return false;
    std::stringstream ss;
    ss << f.rdbuf();
    const std::string s = ss.str();
    size_t p = 0;
    while ((p = s.find("{\"file_path\": \"", p)) != std::string::npos) {
        FileCheckpoint c;
        size_t q = s.find('"', p + 15);
        c.file_path = s.substr(p + 15, q - (p + 15));
        auto num = [&](const char* key) -> std::string {
            size_t k = s.find(key, q);
            if (k == std::string::npos) return "0";
            k += strlen(key);
            size_t e = s.find_first_of(",}", k);
            return s.substr(k, e - k);
        };
        c.file_index = strtoull(num("\"file_index\": ").c_str(), nullptr, 10);
        c.score = strtoll(num("\"score\": ").c_str(), nullptr, 10);
        c.processing_time_ms = atof(num("\"processing_time_ms\": ").c_str());
        c.total_bases = strtoull(num("\"total_bases\": ").c_str(), nullptr, 10);
        c.total_reads = strtoull(num("\"total_reads\": ").c_str(), nullptr, 10);
        c.completed = num("\"completed\": ").find("true") != std::string::npos;
        files[c.file_index] = c;
        p = q;
    }
    return true;
}

// ---------------------------------------------------------------------------
// Reference genome (FASTA) for sw mode.
// ---------------------------------------------------------------------------
// The sequence lines concatenated (header lines and '\r' dropped): the file is
// mapped and scanned with memchr (about 2x the line-by-line rate).  Returns
// false when the file cannot be read.
static bool load_fasta(const std::string& path, std::string* seq) {
    const int fd = open(path.c_str(), O_RDONLY);
    if (fd < 0) return false;
    struct stat sb;
    if (fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode)) {
        close(fd);
        return false;
    }
    seq->clear();
    const size_t n = (size_t)sb.st_size;
    void* m = n ? mmap(nullptr, n, PROT_READ, MAP_PRIVATE | MAP_POPULATE, fd, 0) : nullptr;
    close(fd);
    if (n && m == MAP_FAILED) return false;
    seq->reserve(n);
    const char* p = (const char*)m;
    const char* end = p + n;
    while (p < end) {
        const char* nl = (const char*)memchr(p, '\n', (size_t)(end - p));
        const char* e = nl ? nl : end;
        const char* le = (e > p && e[-1] == '\r') ? e - 1 : e;
        if (le > p && *p != '>') seq->append(p, (size_t)(le - p));
        p = e + 1;
    }
    if (n) munmap(m, n);
    return true;
}

void ReferenceLoad::start(const std::string& p) {
    path = p;
    th = std::thread([this]() {
        const auto t = Clock::now();
        ok = load_fasta(path, &seq);
        ms = ms_since(t);
    });
}

const std::string& ReferenceLoad::get() {
    std::call_once(joined, [this]() {
        if (th.joinable()) th.join();
    });
    if (!ok) die("error: cannot open reference " + path);
    return seq;
}

// ---------------------------------------------------------------------------
// WgsRun
// ---------------------------------------------------------------------------
WgsRun::WgsRun(const Args& a_, const std::vector<Device>& devices_, const std::vector<std::string>& files_,
               const std::vector<size_t>& gidx_, size_t n_lane_files_, Checkpoint& ckpt_, ReferenceLoad& ref_)
    : a(a_), devices(devices_), files(files_), gidx(gidx_), n_lane_files(n_lane_files_), ckpt(ckpt_), ref(ref_),
      chunk(get_chunk_size_reads()), sw(a_.score_mode == "sw"), ngpu((int)devices_.size()), st(files_.size()),
      cli_trace(getenv("MSW_CLI_TRACE") != nullptr) {
    if (sw && a.reference.empty()) die("error: --score-mode sw with --full-wgs needs --reference <FASTA>");
    // the reference: loading since the top of main, beside the HIP runtime
    // init (which takes longer), so this wait is normally over at once; a
    // reference that cannot be read fails here, before any worker starts
    if (sw) printf("Loaded reference: %zu bases\n", ref.get().size());
    for (size_t i = 0; i < files.size(); ++i) {
        st[i].reset(new FileState());
        st[i]->path = files[i];
        auto it = ckpt.files.find(gidx[i]);
        if (it != ckpt.files.end() && it->second.completed && it->second.file_path == files[i]) {
            printf("  Skipping completed file %zu/%zu: %s (score %lld)\n", gidx[i] + 1, n_lane_files,
                   files[i].c_str(), it->second.score);
        } else {
            todo.push_back(i);
        }
    }
    t_setup = Clock::now();
    t_all = t_setup;
}

void WgsRun::setup_phase(double c, double g, double r, double rd, double kl, double ix) {
    std::lock_guard<std::mutex> lk(setup_mu);
    ph_index = std::max(ph_index, ix);
    ph_ctx = std::max(ph_ctx, c);
    ph_gen = std::max(ph_gen, g);
    ph_res = std::max(ph_res, r);
    ph_reader = std::max(ph_reader, rd);
    ph_kl = std::max(ph_kl, kl);
}

void WgsRun::mark_done() {
    const long long t = Clock::now().time_since_epoch().count();
    long long cur = t_done_ns.load();
    while (t > cur && !t_done_ns.compare_exchange_weak(cur, t)) {
    }
}

void WgsRun::trace_ev(int wi, const char* what, uint64_t n) const {
    if (cli_trace)
        fprintf(stderr, "[cli trace] worker %d %s n=%llu t=%.3f ms\n", wi, what, (unsigned long long)n,
                ms_since(t_all));
}

void WgsRun::start_clock(int n) {
    gate.release_when(n);
    t_all = Clock::now();
}

void WgsRun::finish_file(size_t fi) {
    FileState& f = *st[fi];
    if (f.finished.exchange(true)) return;  // exactly once (reader or GPU thread)
    f.ms = ms_since(f.t0);
    if (f.scores_fd >= 0) {
        close(f.scores_fd);
        f.scores_fd = -1;
    }
    if (f.aln_fd >= 0) {
        close(f.aln_fd);
        f.aln_fd = -1;
    }
    FileCheckpoint c;
    c.file_path = f.path;
    c.file_index = gidx[fi];
    c.score = f.score.load();
    c.processing_time_ms = f.ms;
    c.total_bases = f.bases.load();
    c.total_reads = f.reads.load();
    c.completed = !f.failed.load();
    std::lock_guard<std::mutex> lk(ck_mu);
    ckpt.files[gidx[fi]] = c;
    ckpt.save();
    printf("  File %zu done: %s score=%lld reads=%llu bases=%llu time=%.2fs%s\n", gidx[fi] + 1, f.path.c_str(),
           c.score, c.total_reads, c.total_bases, f.ms / 1000.0, c.completed ? "" : " (FAILED)");
    fflush(stdout);
}

// After the threads have joined: every file finished (a no-op for those
// already finished), then the record of the run.  gpu[i] is worker i's
// stats; worker i runs on devices[i % ngpu].
WgsReport WgsRun::report(int readers, int host_threads, const std::vector<msw_stats_t>& gpu, bool gpu_inflate,
                         unsigned long long gz_in, unsigned long long gz_out) {
    for (size_t fi : todo) finish_file(fi);
    WgsReport rep;
    rep.setup_ms = std::chrono::duration<double, std::milli>(t_all - t_setup).count();
    rep.reference_load_ms = ref.ms;
    rep.context_ms = ph_ctx;
    rep.genome_ms = ph_gen;
    rep.result_sets_ms = ph_res;
    rep.lane_reader_ms = ph_reader;
    rep.kernel_load_ms = ph_kl;
    rep.gz_in = gz_in;
    rep.gz_out = gz_out;
    const double total = ms_since(t_all);
    const long long d = t_done_ns.load();
    rep.wall_ms = d ? std::chrono::duration<double, std::milli>(Clock::time_point(Clock::duration(d)) - t_all).count()
                    : total;
    rep.pileup = pileup;
    rep.variants = variants;
    rep.teardown_ms = total - rep.wall_ms - pileup.ms - variants.ms;
    rep.cells = cells.load();
    rep.both_strands = a.both_strands;
    rep.reverse_reads = reverse_reads.load();
    rep.map = a.map;
    rep.placed_reads = placed_reads.load();
    rep.index_ms = ph_index;
    rep.mapq = a.mapq;
    for (int k = 0; k < 4; ++k) rep.mapq_hist[k] = mapq_hist[k].load();
    rep.readers = readers;
    rep.host_threads = host_threads;
    rep.gpu = gpu;
    for (size_t wi = 0; wi < gpu.size(); ++wi) rep.gpu_dev.push_back(devices[wi % (size_t)ngpu].ordinal);
    rep.gpu_inflate = gpu_inflate;
    for (size_t i = 0; i < files.size(); ++i)
        if (ckpt.files.count(gidx[i])) rep.results.push_back(ckpt.files[gidx[i]]);
    return rep;
}

// ---------------------------------------------------------------------------
// GPU lane reader (sw mode, every lane file BGZF, MSW_GPU_INFLATE != 0):
// each worker takes whole files; the host reads compressed bytes only and
// inflate, parse, window cut and scoring run on the worker's GPU
// (msw_gfastq_* + msw_align_reads_device).  Per-read results come back to
// the host for the i64 sums and --scores-out, one batch behind the GPU.
// ---------------------------------------------------------------------------
LaneRun::LaneRun(WgsRun& run_, bool aln_, bool per_read_, bool both_, uint64_t batch_, int nworkers_)
    : run(run_), aln(aln_), per_read(per_read_), both(both_), batch(batch_), nworkers(nworkers_),
      started(new std::atomic<int>[run_.st.size()]), gstats((size_t)nworkers_, msw_stats_t{}),
      pileup(run_.a.wants_pileup()) {
    for (size_t i = 0; i < run.st.size(); ++i) started[i] = 0;
}

// --pileup-out, after the workers have joined: the summary of the summed
// counts (include/msw.h, "Pileup") and the .mpu file -- a 32-byte header
// ("MSWPILE1", u32 version 1, u32 channels 8, u64 genome length, u64
// reads_used), then the rows.  The phase runs from the stop of the clock.
static void write_pileup(WgsRun& run, LaneRun& lanes) {
    const std::string& g = run.genome();
    const uint64_t glen = g.size();
    std::vector<uint32_t>& c = lanes.pile_sum;
    if (lanes.pile_failed || c.size() != glen * 8) die("error: the pileup could not be read back from the GPUs");
    PileupReport& p = run.pileup;
    p.on = true;
    p.reads_used = lanes.pile_used;
    p.reads_skipped = lanes.pile_skipped;
    p.lowq_columns = lanes.pile_lowq;
    const unsigned long long min_depth = (unsigned long long)run.a.pileup_min_depth;
    for (uint64_t pos = 0; pos < glen; ++pos) {
        const uint32_t* row = c.data() + pos * 8;
        const unsigned long long depth = (unsigned long long)row[0] + row[1] + row[2] + row[3] + row[4] + row[5];
        const char b = g[pos];
        const int code = b == 'A' ? 0 : b == 'C' ? 1 : b == 'G' ? 2 : b == 'T' ? 3 : 4;
        p.covered += depth > 0;
        p.depth_sum += depth;
        p.max_depth = std::max(p.max_depth, depth);
        p.minority_ref += depth >= min_depth && 2ull * row[code] < depth;
    }
    FILE* f = fopen(run.a.pileup_out.c_str(), "wb");
    if (!f) die("error: cannot create " + run.a.pileup_out);
    unsigned char head[32];
    memcpy(head, "MSWPILE1", 8);
    const uint32_t version = 1, channels = 8;
    const uint64_t used = p.reads_used;
    memcpy(head + 8, &version, 4);
    memcpy(head + 12, &channels, 4);
    memcpy(head + 16, &glen, 8);
    memcpy(head + 24, &used, 8);
    const bool ok = fwrite(head, 1, 32, f) == 32 && fwrite(c.data(), 4, c.size(), f) == c.size();
    if (fclose(f) != 0 || !ok) die("error: writing " + run.a.pileup_out);
    const long long d = run.t_done_ns.load();
    p.ms = d ? std::chrono::duration<double, std::milli>(Clock::now() - Clock::time_point(Clock::duration(d))).count() : 0.0;
}

// --variants-out, after the workers have joined and the pileup's phase: one
// context on the run's first device calls on the summed counts
// (msw_call_counts: a count call, then a call that fills the records) and the
// .var file is written -- a 72-byte header ("MSWVARS1", u32 version 1, u32
// record size 48, u64 genome length, u64 record count, the nine u32 of
// msw_call_params_t, u32 zero), then the records.
static void write_variants(WgsRun& run, LaneRun& lanes) {
    const auto t0 = Clock::now();
    const long long d = run.t_done_ns.load();
    // without --pileup-out the phase runs from the stop of the clock
    const auto from = run.pileup.on || !d ? t0 : Clock::time_point(Clock::duration(d));
    const std::string& g = run.genome();
    const uint64_t glen = g.size();
    if (lanes.pile_failed || lanes.pile_sum.size() != glen * 8) die("error: the pileup could not be read back from the GPUs");
    const msw_call_params_t q = run.a.call_params();
    // --call-baseq: the weighted call on the summed quality sums (msw_call_counts_qual), an MSWVARQ1 file -- the 72
    // bytes above, then q_scale, q_third and two zero words -- and, with --qsum-out, the .mqs file: a 32-byte header
    // ("MSWQSUM1", u32 version 1, u32 channels 4, u64 genome length, u64 reads_used), then the rows of four
    const bool weighted = run.a.call_baseq;
    msw_call_qparams_t qq;
    msw_call_qparams_default(&qq);
    if (weighted && lanes.qsum_sum.size() != glen * 4) die("error: the quality sums could not be read back from the GPUs");
    std::vector<msw_variant_t> recs;
    {
        Ctx ctx(run.devices[0].ordinal, MSW_CTX_LEAN);
        uint64_t n = 0, again = 0;
        const uint8_t* gb = reinterpret_cast<const uint8_t*>(g.data());
        auto call = [&](msw_variant_t* out, uint64_t cap, uint64_t* total) {
            return weighted ? msw_call_counts_qual(ctx.h, gb, glen, lanes.pile_sum.data(), lanes.qsum_sum.data(), &q, &qq, 0,
                                                   out, cap, total)
                            : msw_call_counts(ctx.h, gb, glen, lanes.pile_sum.data(), &q, 0, out, cap, total);
        };
        if (call(nullptr, 0, &n) != MSW_OK) die(std::string("GPU variant call error: ") + msw_last_error());
        recs.resize(n);
        if (n && (call(recs.data(), n, &again) != MSW_OK || again != n))
            die(std::string("GPU variant call error: ") + msw_last_error());
    }
    VariantsReport& v = run.variants;
    v.on = true;
    v.lowq_columns = lanes.pile_lowq;
    v.total = recs.size();
    for (const msw_variant_t& r : recs) {
        if (r.kind < 3) ++v.by_kind[r.kind];
        if (r.gt < 3) ++v.by_gt[r.gt];
    }
    FILE* f = fopen(run.a.variants_out.c_str(), "wb");
    if (!f) die("error: cannot create " + run.a.variants_out);
    unsigned char head[88] = {0};
    const size_t head_bytes = weighted ? 88 : 72;
    memcpy(head, weighted ? "MSWVARQ1" : "MSWVARS1", 8);
    const uint32_t version = 1, rsize = (uint32_t)sizeof(msw_variant_t);
    const uint64_t count = recs.size();
    memcpy(head + 8, &version, 4);
    memcpy(head + 12, &rsize, 4);
    memcpy(head + 16, &glen, 8);
    memcpy(head + 24, &count, 8);
    memcpy(head + 32, &q, 36);
    if (weighted) memcpy(head + 72, &qq, 8);
    static_assert(sizeof(msw_call_params_t) == 36 && sizeof(msw_variant_t) == 48 && sizeof(msw_call_qparams_t) == 8,
                  "the .var layout");
    const bool ok = fwrite(head, 1, head_bytes, f) == head_bytes &&
                    fwrite(recs.data(), sizeof(msw_variant_t), recs.size(), f) == recs.size();
    if (fclose(f) != 0 || !ok) die("error: writing " + run.a.variants_out);
    if (!run.a.qsum_out.empty()) {
        FILE* fq = fopen(run.a.qsum_out.c_str(), "wb");
        if (!fq) die("error: cannot create " + run.a.qsum_out);
        unsigned char qh[32];
        memcpy(qh, "MSWQSUM1", 8);
        const uint32_t channels = 4;
        const uint64_t used = lanes.pile_used;
        memcpy(qh + 8, &version, 4);
        memcpy(qh + 12, &channels, 4);
        memcpy(qh + 16, &glen, 8);
        memcpy(qh + 24, &used, 8);
        const std::vector<uint32_t>& w = lanes.qsum_sum;
        const bool okq = fwrite(qh, 1, 32, fq) == 32 && fwrite(w.data(), 4, w.size(), fq) == w.size();
        if (fclose(fq) != 0 || !okq) die("error: writing " + run.a.qsum_out);
    }
    v.ms = std::chrono::duration<double, std::milli>(Clock::now() - from).count();
}

static WgsReport run_gpu_lanes(WgsRun& run, bool aln, bool per_read) {
    // reads per scoring launch; wide slabs (MSW_MAX_READ_LEN) keep a batch's
    // slab near 256 MiB (two per worker)
    // per-read records (--scores-out) are host work per read: batches of
    // 256k reads, so one batch's records are written while the next one
    // scores (config 3 from FASTQ: 17.4-18.0 -> 16.3-16.4 ms per 1 M reads,
    // profiles/r05/c3f/c3f_batch_ab.jsonl); sums only: 1 M-read batches
    const uint64_t batch_default = per_read ? (1u << 18) : (1u << 20);
    const uint64_t batch = std::max<uint64_t>(
        run.chunk, std::min<uint64_t>(strtoull(env_or("MSW_GFASTQ_BATCH", std::to_string(batch_default)).c_str(),
                                               nullptr, 10),
                                      (256ull << 20) / read_stride()));
    // two workers (contexts) per GPU by default: one file's inflate and
    // host reads overlap the other's scoring
    // (three or four workers per GPU measured slower: DESIGN.md 5)
    const int per_gpu = 2;
    LaneRun lanes(run, aln, per_read, run.a.both_strands, batch, run.ngpu * per_gpu);
    std::vector<std::thread> workers;
    for (int wi = 0; wi < lanes.nworkers; ++wi) workers.emplace_back(lane_worker, std::ref(lanes), wi);
    run.start_clock(lanes.nworkers);
    for (auto& t : workers) t.join();
    if (!run.a.pileup_out.empty()) write_pileup(run, lanes);
    if (!run.a.variants_out.empty()) write_variants(run, lanes);
    return run.report(0, lanes.nworkers, lanes.gstats, true, lanes.gz_in.load(), lanes.gz_out.load());
}

// ---------------------------------------------------------------------------
// Host-reader path (compat mode, gzip lane files, MSW_GPU_INFLATE=0).
// ---------------------------------------------------------------------------
namespace {

// Read slabs in pinned memory (msw_host_alloc = hipHostMalloc): the FASTQ
// readers parse straight into them and msw_align_reads DMAs them to the GPU
// without staging.  Recycled through a free list; one block per slab:
// [reads cap x read_stride() | pos i64 x cap | rlen u16 x cap].
class SlabPool {
   public:
    struct Slab {
        uint8_t* base = nullptr;
        uint8_t* reads = nullptr;
        int64_t* pos = nullptr;
        uint16_t* rlen = nullptr;
        bool pinned = false;
    };
    explicit SlabPool(uint64_t cap) : cap_(cap) {}
    ~SlabPool() {
        for (Slab* s : free_) release(s);
    }
    Slab* get() {
        {
            std::lock_guard<std::mutex> lk(m_);
            if (!free_.empty()) {
                Slab* s = free_.back();
                free_.pop_back();
                return s;
            }
        }
        Slab* s = new Slab();
        const size_t bytes = cap_ * (read_stride() + 8 + 2);
        s->base = (uint8_t*)msw_host_alloc(bytes);
        s->pinned = s->base != nullptr;
        if (!s->base) s->base = (uint8_t*)malloc(bytes);  // pageable fallback: staged by the runtime
        if (!s->base) die("error: out of host memory for read slabs");
        s->reads = s->base;
        s->pos = (int64_t*)(s->base + cap_ * read_stride());
        s->rlen = (uint16_t*)(s->base + cap_ * (read_stride() + 8));
        return s;
    }
    void put(Slab* s) {
        std::lock_guard<std::mutex> lk(m_);
        free_.push_back(s);
    }

   private:
    static void release(Slab* s) {
        if (s->pinned) msw_host_free(s->base);
        else free(s->base);
        delete s;
    }
    uint64_t cap_;
    std::mutex m_;
    std::vector<Slab*> free_;
};

struct Chunk {
    size_t file_index = 0;
    SlabPool* pool = nullptr;
    SlabPool::Slab* slab = nullptr;  // sw: reads n x read_stride(), rlen, pos
    std::vector<uint8_t> cat;        // compat: the chunk's sequences back to back (any read length)
    uint64_t n = 0;
    uint64_t first_read = 0;         // index of the chunk's first read in its file
    bool last = false;               // last chunk of its file
    const uint8_t* reads() const { return slab->reads; }
    const uint16_t* rlen() const { return slab->rlen; }
    const int64_t* pos() const { return slab->pos; }
    ~Chunk() {
        if (slab) pool->put(slab);
    }
};

class ChunkQueue {
   public:
    explicit ChunkQueue(size_t cap) : cap_(cap) {}
    void push(std::unique_ptr<Chunk> c) {
        std::unique_lock<std::mutex> lk(m_);
        cv_space_.wait(lk, [&] { return q_.size() < cap_; });
        q_.push_back(std::move(c));
        cv_item_.notify_one();
    }
    std::unique_ptr<Chunk> pop() {
        std::unique_lock<std::mutex> lk(m_);
        cv_item_.wait(lk, [&] { return !q_.empty() || closed_; });
        if (q_.empty()) return nullptr;
        auto c = std::move(q_.front());
        q_.pop_front();
        cv_space_.notify_one();
        return c;
    }
    void close() {
        std::lock_guard<std::mutex> lk(m_);
        closed_ = true;
        cv_item_.notify_all();
    }

   private:
    std::mutex m_;
    std::condition_variable cv_item_, cv_space_;
    std::deque<std::unique_ptr<Chunk>> q_;
    size_t cap_;
    bool closed_ = false;
};

// What the host path's reader and GPU threads share beyond the run.
struct HostRun {
    WgsRun& run;
    ChunkQueue queue;
    SlabPool slabs;
    std::atomic<size_t> next_file{0};
    std::atomic<int> readers_left;
    std::vector<msw_stats_t> gstats;  // per GPU thread
    HostRun(WgsRun& r, int nreaders)
        : run(r), queue(2 * (size_t)r.ngpu + 2), slabs(r.chunk), readers_left(nreaders), gstats((size_t)r.ngpu) {}
};

// The next chunk of a file into c; false on a read error.  c.n == 0: end of file.
bool read_chunk(HostRun& h, msw_fastq* fq, Chunk& c) {
    const uint64_t chunk = h.run.chunk;
    if (h.run.sw) {
        c.pool = &h.slabs;
        c.slab = h.slabs.get();
        return msw_fastq_next(fq, c.slab->reads, c.slab->rlen, read_stride(), chunk, &c.n, c.slab->pos) == MSW_OK;
    }
    // compat: exactly `chunk` reads of any length, concatenated
    // (aligner.rs:270); the buffer grows when a read does not fit
    bool ok = true;
    std::vector<uint8_t>& cat = c.cat;
    cat.resize((size_t)std::min<uint64_t>(chunk, 65536) * 160);
    std::vector<uint32_t> lens((size_t)std::min<uint64_t>(chunk, 65536));
    uint64_t used = 0;
    while (ok && c.n < chunk) {
        uint64_t got = 0, nb = 0, need = 0;
        const uint64_t want = std::min<uint64_t>(chunk - c.n, lens.size());
        ok = msw_fastq_next_packed(fq, cat.data() + used, cat.size() - used, lens.data(), want, &got, &nb, &need) ==
             MSW_OK;
        used += nb;
        c.n += got;
        if (ok && need) cat.resize(std::max(2 * cat.size(), (size_t)(used + need)));
        else if (ok && got < want) break;  // end of file
    }
    cat.resize((size_t)used);
    return ok;
}

void host_reader_thread(HostRun& h) {
    WgsRun& run = h.run;
    run.gate.wait_open();
    for (;;) {
        const size_t k = h.next_file.fetch_add(1);
        if (k >= run.todo.size()) break;
        const size_t fi = run.todo[k];
        FileState& f = *run.st[fi];
        f.t0 = Clock::now();
        if (run.sw && !run.a.scores_out.empty()) {
            const std::string out = out_path(run.a.scores_out, f.path, ".scores");
            f.scores_fd = open(out.c_str(), O_CREAT | O_TRUNC | O_WRONLY, 0644);
            if (f.scores_fd < 0) die("error: cannot create " + out);
        }
        printf("  Processing file %zu/%zu: %s\n", run.gidx[fi] + 1, run.n_lane_files, f.path.c_str());
        fflush(stdout);
        msw_fastq* fq = nullptr;
        if (msw_fastq_open(f.path.c_str(), &fq) != MSW_OK) {
            f.error = msw_last_error();
            f.failed = true;
            f.reader_done = true;
            if (f.outstanding.load() == 0) run.finish_file(fi);
            continue;
        }
        uint64_t reads_so_far = 0;
        for (;;) {
            std::unique_ptr<Chunk> c(new Chunk());
            c->file_index = fi;
            c->first_read = reads_so_far;
            if (!read_chunk(h, fq, *c)) {
                f.error = msw_last_error();
                fprintf(stderr, "  Error reading %s: %s\n", f.path.c_str(), f.error.c_str());
                f.failed = true;
                break;
            }
            if (c->n == 0) break;
            reads_so_far += c->n;
            f.outstanding.fetch_add(1);
            h.queue.push(std::move(c));
        }
        msw_fastq_close(fq);
        f.reader_done = true;
        // A file with no chunks in flight is finished here; otherwise by the GPU thread.
        if (f.outstanding.load() == 0) run.finish_file(fi);
    }
    if (h.readers_left.fetch_sub(1) == 1) h.queue.close();
}

// Up to three chunks in flight (msw_align_reads_async; msw_wait on the
// oldest ticket before a fourth is staged): the context's three
// staging slots keep uploads of chunk k+1 under kernel k.
struct InFlight {
    std::unique_ptr<Chunk> c;
    std::vector<uint16_t> want;
    std::vector<int32_t> score;
    std::vector<int16_t> ei, ej;
    uint64_t ticket = 0;
    unsigned long long cells = 0, bases = 0;
    bool failed = false;

    // sw: the chunk's windows and cells, then its scoring on GPU thread g.
    // window = reference[pos : pos + W] (W = --window, at most
    // 32767, or 2 x read length capped at 4096), clipped at the genome end
    InFlight(WgsRun& run, msw_ctx* ctx, int g, const msw_scoring_t& sc, msw_genome* gen, uint64_t gsize,
             std::unique_ptr<Chunk> chunk, unsigned long long nb)
        : c(std::move(chunk)), want(c->n), score(c->n, 0), ei(c->n, 0), ej(c->n, 0), bases(nb) {
        for (uint64_t i = 0; i < c->n; ++i) {
            const uint32_t w = std::min<uint32_t>(window_for(run.a, c->rlen()[i]), 32767u);
            want[i] = (uint16_t)w;
            const int64_t p = c->pos()[i];
            if (p >= 0 && (uint64_t)p < gsize)
                cells += (unsigned long long)std::min<uint64_t>(w, gsize - (uint64_t)p) * c->rlen()[i];
        }
        msw_read_batch_t rb{c->reads(), c->rlen(), read_stride(), c->pos(), want.data(), c->n};
        msw_out_t o{score.data(), ei.data(), ej.data()};
        if (msw_align_reads_async(ctx, &sc, gen, &rb, &o, 0, &ticket) != MSW_OK) {
            fprintf(stderr, "  GPU %d alignment error: %s\n", g, msw_last_error());
            failed = true;
        }
    }

    void settle(WgsRun& run, msw_ctx* ctx, int g) {
        FileState& f = *run.st[c->file_index];
        long long chunk_score = 0;
        if (!failed && ticket && msw_wait(ctx, ticket) != MSW_OK) {
            fprintf(stderr, "  GPU %d alignment error: %s\n", g, msw_last_error());
            failed = true;
        }
        if (failed) {
            f.failed = true;
        } else {
            for (uint64_t i = 0; i < c->n; ++i) chunk_score += score[i];
            run.cells += cells;
            if (f.scores_fd >= 0) {
                // chunks of one file may finish on different GPUs in any
                // order: each lands at its reads' own offset
                std::vector<uint64_t> rec(c->n);
                for (uint64_t i = 0; i < c->n; ++i) rec[i] = score_record(score[i], ei[i], ej[i]);
                if (pwrite(f.scores_fd, rec.data(), rec.size() * 8, (off_t)(c->first_read * 8)) !=
                    (ssize_t)(rec.size() * 8)) {
                    fprintf(stderr, "  error writing scores for %s\n", f.path.c_str());
                    f.failed = true;
                }
            }
        }
        f.score += chunk_score;
        f.bases += bases;
        f.reads += c->n;
        if (f.outstanding.fetch_sub(1) == 1 && f.reader_done.load()) run.finish_file(c->file_index);
        c.reset();
    }
};

// compat: chunk concat self-aligned (aligner.rs:269-276, :365-373)
void score_compat_chunk(WgsRun& run, msw_ctx* ctx, int g, const Chunk& c) {
    FileState& f = *run.st[c.file_index];
    long long chunk_score = 0;
    const std::vector<uint8_t>& cat = c.cat;
    if (cat.size() >= 1000) {
        int32_t s = 0;
        if (msw_align_compat(ctx, cat.data(), cat.size(), cat.data(), cat.size(),
                             std::min<uint32_t>(run.devices[g].max_wg, 1024), 1000000, &s) != MSW_OK) {
            fprintf(stderr, "  GPU %d alignment error: %s\n", g, msw_last_error());
            f.failed = true;
        }
        chunk_score = s;
    }
    f.score += chunk_score;
    f.bases += cat.size();
    f.reads += c.n;
    if (f.outstanding.fetch_sub(1) == 1 && f.reader_done.load()) run.finish_file(c.file_index);
}

void host_gpu_worker(HostRun& h, int g) {
    WgsRun& run = h.run;
    const auto ts0 = Clock::now();
    Ctx ctx(run.devices[g].ordinal);
    const double t_ctx = ms_since(ts0);
    const msw_scoring_t sc = scoring_of(run.a, !run.a.scores_out.empty());
    // sw mode: the reference genome lives in this GPU's HBM; a chunk
    // ships reads + window positions, windows are cut on the GPU.
    msw_genome* gen = nullptr;
    const uint64_t gsize = run.sw ? run.genome().size() : 0;
    if (run.sw && msw_genome_create(ctx.h, (const uint8_t*)run.genome().data(), gsize, &gen) != MSW_OK)
        die(std::string("GPU genome upload error: ") + msw_last_error());
    const double t_gen = ms_since(ts0);
    if (msw_ctx_prepare(ctx.h, &sc) != MSW_OK) die(std::string("GPU kernel load: ") + msw_last_error());
    run.setup_phase(t_ctx, t_gen - t_ctx, 0.0, 0.0, ms_since(ts0) - t_gen);
    run.gate.arrive();
    std::deque<std::unique_ptr<InFlight>> pending;
    constexpr size_t kDepth = 3;
    for (;;) {
        std::unique_ptr<Chunk> c = h.queue.pop();
        if (!c) break;
        if (!run.sw) {
            score_compat_chunk(run, ctx.h, g, *c);
            continue;
        }
        unsigned long long nb = 0;
        for (uint64_t i = 0; i < c->n; ++i) nb += c->rlen()[i];
        pending.emplace_back(new InFlight(run, ctx.h, g, sc, gen, gsize, std::move(c), nb));
        if (pending.size() >= kDepth) {
            pending.front()->settle(run, ctx.h, g);
            pending.pop_front();
        }
    }
    while (!pending.empty()) {
        pending.front()->settle(run, ctx.h, g);
        pending.pop_front();
    }
    run.mark_done();
    msw_ctx_stats(ctx.h, &h.gstats[(size_t)g], 0);
    ctx.keep = true;  // like the genome, left to the process exit
}

WgsReport run_host_readers(WgsRun& run) {
    // Readers: one thread per lane file in flight (a gzip stream inflates on
    // one core; zlib gives ~0.5-0.75 M reads/s per thread, far below what one
    // GPU scores, so the host side wants every file open at once):
    // min(files, MSW_HOST_THREADS), by default the CPUs this process may use
    // (usable_cpus()).
    const int host_threads = std::max(1, atoi(env_or("MSW_HOST_THREADS", std::to_string(usable_cpus())).c_str()));
    const int nreaders =
        std::max(1, std::min<int>((int)run.todo.size(), std::max(host_threads, 2 * run.ngpu)));
    // Fewer files than the CPU share: BGZF blocks of one file inflate on
    // several threads (msw_fastq.cpp; MSW_INFLATE_THREADS overrides).
    if (!getenv("MSW_INFLATE_THREADS")) {
        const std::string per = std::to_string(std::max(1, host_threads / nreaders));
        setenv("MSW_INFLATE_THREADS", per.c_str(), 0);
    }
    HostRun h(run, nreaders);
    std::vector<std::thread> readers, workers;
    for (int r = 0; r < nreaders; ++r) readers.emplace_back(host_reader_thread, std::ref(h));
    for (int g = 0; g < run.ngpu; ++g) workers.emplace_back(host_gpu_worker, std::ref(h), g);
    run.start_clock(run.ngpu);
    for (auto& t : readers) t.join();
    for (auto& t : workers) t.join();
    return run.report(nreaders, host_threads, h.gstats, false, 0, 0);
}

}  // namespace

WgsReport run_full_wgs(const Args& a, const std::vector<Device>& devices, const std::vector<std::string>& files,
                       const std::vector<size_t>& gidx, size_t n_lane_files, Checkpoint& ckpt, ReferenceLoad& ref) {
    WgsRun run(a, devices, files, gidx, n_lane_files, ckpt, ref);
    bool gpu_reader = run.sw && env_or("MSW_GPU_INFLATE", "1") != "0" && !run.todo.empty();
    for (size_t fi : run.todo) gpu_reader = gpu_reader && msw_is_bgzf(files[fi].c_str());
    const bool aln = !a.alignments_out.empty();
    if (aln && !run.todo.empty() && !gpu_reader)
        die("error: --alignments-out needs BGZF lane files (the GPU lane reader); the host reader does not write "
            "alignments");
    if (a.both_strands && !run.todo.empty() && !gpu_reader)
        die("error: --both-strands needs BGZF lane files (the GPU lane reader); the host reader scores the reads as "
            "given");
    if (a.map && !run.todo.empty() && !gpu_reader)
        die("error: --map needs BGZF lane files (the GPU lane reader); the host reader takes the positions from the "
            "headers");
    return gpu_reader ? run_gpu_lanes(run, aln, !a.scores_out.empty() || aln) : run_host_readers(run);
}
