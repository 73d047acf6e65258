// cli_wgs.h -- the --full-wgs run: what main hands it (checkpoint, reference
// load), what it hands back (WgsReport), and the run's state shared by its
// threads (WgsRun; LaneRun for the GPU lane reader's workers).
#pragma once

#include <atomic>
#include <condition_variable>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "cli_common.h"

// ---------------------------------------------------------------------------
// Checkpoint / resume (aligner.rs:22-104 schema, with the bugs fixed: one
// stable file name per run id, i64 scores, resume skips completed files).
// ---------------------------------------------------------------------------
struct FileCheckpoint {
    std::string file_path;
    size_t file_index = 0;
    long long score = 0;
    double processing_time_ms = 0;
    unsigned long long total_bases = 0, total_reads = 0;
    bool completed = false;
};

std::string json_escape(const std::string& s);

struct Checkpoint {
    std::string run_id, path;
    size_t total_files = 0;
    std::map<size_t, FileCheckpoint> files;
    void save() const;
    bool load();  // minimal parser for the file this program writes
};

// The reference, loaded on a thread of its own from the start of main, beside
// the HIP runtime init; run_full_wgs takes it before the workers start.
struct ReferenceLoad {
    std::string path, seq;
    double ms = 0;
    bool ok = false;
    std::thread th;
    void start(const std::string& p);
    // the sequence; exits like the other setup errors when it could not be read
    const std::string& get();
    ~ReferenceLoad() {
        if (th.joinable()) th.join();
    }
    std::once_flag joined;
};

struct FileState {
    std::string path;
    std::atomic<long long> score{0};
    std::atomic<unsigned long long> bases{0}, reads{0};
    std::atomic<int> outstanding{0};
    std::atomic<bool> reader_done{false}, failed{false}, finished{false};
    int scores_fd = -1;  // --scores-out: per-read records, written at the read's offset
    int aln_fd = -1;     // --alignments-out: blocks appended as the batches settle
    Clock::time_point t0;
    double ms = 0;
    std::string error;
};

// Workers set up (context, genome upload, staging buffers) before the clock
// starts: the run record's wall time covers the data, like the reference's
// per-file processing times; setup_ms reports the rest.
struct StartGate {
    std::mutex m;
    std::condition_variable cv;
    int arrived = 0;
    bool open = false;
    void arrive() {
        std::unique_lock<std::mutex> lk(m);
        ++arrived;
        cv.notify_all();
        cv.wait(lk, [&] { return open; });
    }
    void wait_open() {
        std::unique_lock<std::mutex> lk(m);
        cv.wait(lk, [&] { return open; });
    }
    void release_when(int n) {
        std::unique_lock<std::mutex> lk(m);
        cv.wait(lk, [&] { return arrived >= n; });
        open = true;
        cv.notify_all();
    }
};

// --pileup-out: the summary of the run's pileup and the time of its phase
// (fold, copy-out, sum over the workers, summary, file), after the clock.
struct PileupReport {
    bool on = false;
    unsigned long long reads_used = 0, reads_skipped = 0, covered = 0, depth_sum = 0, max_depth = 0, minority_ref = 0;
    unsigned long long lowq_columns = 0;  // --pileup-min-baseq: M columns under the threshold, over the workers
    double ms = 0;
};

// --variants-out: the calls' totals by kind (SNV, DEL, INS) and genotype (index 1: 0/1, 2: 1/1) and the time of the
// phase (the call on the summed counts, the file), after the pileup's phase.
struct VariantsReport {
    bool on = false;
    unsigned long long total = 0, by_kind[3] = {0, 0, 0}, by_gt[3] = {0, 0, 0};
    unsigned long long lowq_columns = 0;  // as PileupReport's (a run may have --variants-out alone)
    double ms = 0;
};

struct WgsReport {
    std::vector<FileCheckpoint> results;
    PileupReport pileup;
    VariantsReport variants;
    double wall_ms = 0;
    unsigned long long cells = 0;
    int readers = 0;
    int host_threads = 0;
    std::vector<msw_stats_t> gpu;  // per worker: kernel time and algorithmic bytes (msw_ctx_stats)
    std::vector<int> gpu_dev;      // device ordinal of each gpu[] entry (workers may share a GPU)
    bool gpu_inflate = false;      // lane files inflated and parsed on the GPUs
    double setup_ms = 0;           // worker setup before the clock started (contexts, genome, buffers)
    double teardown_ms = 0;        // release after the last results, outside the clock
    // setup split (JSON "setup_phases", each phase's max over the workers):
    // reference_load on its own thread from the start of main, beside hip_init
    // (run_full_wgs waits for it before setup); context / genome upload /
    // result sets / lane reader
    // inside setup_ms (workers run them side by side); hip_init is filled in
    // by main (the first HIP call, before setup_ms)
    double reference_load_ms = 0, context_ms = 0, genome_ms = 0, result_sets_ms = 0, lane_reader_ms = 0;
    double kernel_load_ms = 0;  // msw_ctx_prepare: the scoring kernels' code objects, before the clock
    unsigned long long gz_in = 0, gz_out = 0;  // compressed / inflated bytes (GPU lane reader)
    bool both_strands = false;                 // --both-strands
    unsigned long long reverse_reads = 0;      // reads of this run whose reverse complement won (strand 1)
    bool map = false;                          // --map
    unsigned long long placed_reads = 0;       // --map: reads the seeding gave a window (win_pos >= 0)
    double index_ms = 0;                       // --map: the k-mer index build, a phase of the setup split
    bool mapq = false;                         // --mapq
    unsigned long long mapq_hist[4] = {0, 0, 0, 0};  // --mapq: reads with MAPQ 0, 1-29, 30-59, 60
};

// The window of a read of `len` bases: --window, else 2 x read length capped
// at 4096.  len = 0 gives --window or 0, the library's "use your own rule".
inline uint32_t window_for(const Args& a, uint32_t len) {
    return a.window > 0 ? (uint32_t)a.window : std::min<uint32_t>(2u * len, 4096u);
}

// dir/<lane file's base name><ext>
inline std::string out_path(const std::string& dir, const std::string& lane_file, const char* ext) {
    const size_t slash = lane_file.find_last_of('/');
    return dir + "/" + (slash == std::string::npos ? lane_file : lane_file.substr(slash + 1)) + ext;
}

// One .scores record as a whole word: i32 score | i16 end_i | i16 end_j, little-endian.
inline uint64_t score_record(int32_t score, int16_t end_i, int16_t end_j) {
    return (uint64_t)(uint32_t)score | (uint64_t)(uint16_t)end_i << 32 | (uint64_t)(uint16_t)end_j << 48;
}

// One --full-wgs run: its inputs and what its reader and worker threads share.
struct WgsRun {
    const Args& a;
    const std::vector<Device>& devices;  // already worker_devices(): one host-path worker per entry
    // files: this process's lane files; gidx[i]: file i's index in the whole
    // lane set (WGS_FILE_SHARD takes a subset), used for messages and the checkpoint
    const std::vector<std::string>& files;
    const std::vector<size_t>& gidx;
    const size_t n_lane_files;
    Checkpoint& ckpt;
    ReferenceLoad& ref;  // the reference FASTA, already loading (sw mode; main starts it)
    const uint64_t chunk;
    const bool sw;
    const int ngpu;
    std::vector<std::unique_ptr<FileState>> st;
    std::vector<size_t> todo;  // indices into files / st of the files not completed by an earlier run
    std::mutex ck_mu;
    std::atomic<unsigned long long> cells{0};
    std::atomic<unsigned long long> reverse_reads{0};  // --both-strands: strand-1 reads
    std::atomic<unsigned long long> placed_reads{0};   // --map: reads with a window
    std::atomic<unsigned long long> mapq_hist[4] = {};  // --mapq: reads with MAPQ 0, 1-29, 30-59, 60
    PileupReport pileup;  // --pileup-out: filled after the workers have joined
    VariantsReport variants;  // --variants-out: likewise
    StartGate gate;
    Clock::time_point t_setup, t_all;
    // the clock stops when the last worker has its last results on the host;
    // teardown (reader / context / genome release) is reported apart, like setup
    std::atomic<long long> t_done_ns{0};
    std::mutex setup_mu;
    double ph_ctx = 0, ph_gen = 0, ph_res = 0, ph_reader = 0, ph_kl = 0, ph_index = 0;  // max over workers
    // MSW_CLI_TRACE=1: per worker, ms since the start gate of each batch's
    // arrival from the reader, its submission, and its settle (stderr)
    const bool cli_trace;

    WgsRun(const Args& a, const std::vector<Device>& devices, const std::vector<std::string>& files,
           const std::vector<size_t>& gidx, size_t n_lane_files, Checkpoint& ckpt, ReferenceLoad& ref);
    const std::string& genome() { return ref.get(); }
    void finish_file(size_t fi);  // exactly once per file: checkpoint entry and the "File done" line
    void mark_done();
    void trace_ev(int wi, const char* what, uint64_t n) const;
    void setup_phase(double ctx, double genome, double result_sets, double reader, double kernel_load,
                     double index = 0.0);
    // opens the gate once n workers have arrived; the clock starts here
    void start_clock(int n);
    WgsReport report(int readers, int host_threads, const std::vector<msw_stats_t>& gpu, bool gpu_inflate,
                     unsigned long long gz_in, unsigned long long gz_out);
};

// What the GPU lane reader's workers share beyond the run.
struct LaneRun {
    WgsRun& run;
    const bool aln;       // --alignments-out
    const bool per_read;  // per-read output of either kind: best cells, 256k-read batches, two streams
    const bool both;      // --both-strands
    const uint64_t batch;  // reads per scoring launch
    const int nworkers;
    std::atomic<size_t> next_file{0};
    // A claimed file is pending (prefetched by its claimer) until a worker
    // starts it; a worker left with nothing to claim takes another
    // worker's pending file instead of idling (with few or
    // uneven files the claim-ahead could leave one worker a whole file
    // of work at the end).  0 = pending, 1 = started; indexed like st.
    std::unique_ptr<std::atomic<int>[]> started;
    std::atomic<unsigned long long> gz_in{0}, gz_out{0};
    std::vector<msw_stats_t> gstats;  // per worker
    // --pileup-out or --variants-out: the workers' finished counts [glen][8] summed on the host, and their read counters
    const bool pileup;
    std::mutex pile_mu;
    std::vector<uint32_t> pile_sum;
    std::vector<uint32_t> qsum_sum;   // --call-baseq: the workers' quality sums [glen][4], summed beside the counts
    unsigned long long pile_used = 0, pile_skipped = 0, pile_lowq = 0;
    bool pile_failed = false;

    static constexpr size_t kNone = ~(size_t)0;
    LaneRun(WgsRun& run, bool aln, bool per_read, bool both, uint64_t batch, int nworkers);
    size_t claim() {
        const size_t k = next_file.fetch_add(1);
        return k < run.todo.size() ? run.todo[k] : kNone;
    }
    bool start_file(size_t fi) {
        int e = 0;
        return started[fi].compare_exchange_strong(e, 1);
    }
};

// cli_lane_worker.cpp: the body of worker thread wi
void lane_worker(LaneRun& lanes, int wi);

// cli_wgs.cpp
WgsReport run_full_wgs(const Args& a, const std::vector<Device>& devices, const std::vector<std::string>& files,
                       const std::vector<size_t>& gidx, size_t n_lane_files, Checkpoint& ckpt, ReferenceLoad& ref);
