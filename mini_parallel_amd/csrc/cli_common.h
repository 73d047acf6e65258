// cli_common.h -- what every source of `rustseq_mini` uses: exit and
// environment helpers, the clock, the parsed arguments, a GPU and a context.
#pragma once

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <sched.h>
#include <unistd.h>

#include "msw.h"

using Clock = std::chrono::steady_clock;

inline double ms_since(Clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
}

// Exit 1 with a message.  _exit: a worker thread may die while others are
// still inside HIP calls, and exit()'s static destructors (the HIP runtime's
// teardown) would race them.
[[noreturn]] inline void die(const std::string& msg) {
    fflush(stdout);
    fprintf(stderr, "%s\n", msg.c_str());
    fflush(stderr);
    _exit(1);
}

inline std::string env_or(const char* k, const std::string& d) {
    const char* v = getenv(k);
    return v ? std::string(v) : d;
}

// CPUs this process may use: the affinity mask, capped by the cgroup v2 CPU
// quota (cpu.max) when there is one.  The GPU boxes grant a 16-CPU quota on a
// 256-CPU affinity mask, so hardware_concurrency() alone overstates it 16x.
inline int usable_cpus() {
    int n = 0;
    cpu_set_t set;
    CPU_ZERO(&set);
    if (sched_getaffinity(0, sizeof(set), &set) == 0) n = CPU_COUNT(&set);
    if (n <= 0) n = (int)std::thread::hardware_concurrency();
    if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
        char q[64] = {0};
        double period = 0;
        if (fscanf(f, "%63s %lf", q, &period) == 2 && strcmp(q, "max") != 0 && period > 0) {
            const int quota = (int)(atof(q) / period);
            if (quota >= 1) n = std::min(n, quota);
        }
        fclose(f);
    }
    return std::max(1, n);
}

// aligner.rs:9-15
inline uint64_t get_chunk_size_reads() {
    const char* v = getenv("GPU_CHUNK_SIZE_READS");
    if (!v) die("error: GPU_CHUNK_SIZE_READS not set in .env file");
    char* end = nullptr;
    unsigned long long n = strtoull(v, &end, 10);
    if (!*v || *end || n == 0) die(std::string("error: Invalid GPU_CHUNK_SIZE_READS value '") + v + "'");
    return n;
}

struct Args {
    std::string seq1, seq2;
    bool has_seq1 = false, has_seq2 = false, files = false, gpu = false, test_wgs = false, full_wgs = false;
    bool cigar = false;
    bool both_strands = false;  // --both-strands: --full-wgs sw scores each read and its reverse complement
    // --map: --full-wgs sw places each read on the genome itself (k-mer index, seed voting) instead of
    // taking the window position from a pos= tag of the FASTQ header
    bool map = false;
    int seed_k = 12, seed_max_occ = 64, seed_band = 16;
    // --mapq: --map scores a second candidate locus per read as well, keeps the better one and gives every
    // record a sub-optimal score and a mapping quality; --seed-sep: the least distance of the second
    // candidate's diagonal from the first (0: the read's window length)
    bool mapq = false, has_seed_sep = false;
    int seed_sep = 0;
    // --pileup-out: the per-base allele counts of the run's records (one .mpu file); reads below
    // --pileup-min-mapq do not count, --pileup-min-depth is the summary's least depth
    std::string pileup_out;
    bool has_pileup_min_mapq = false, has_pileup_min_depth = false;
    int pileup_min_mapq = 0, pileup_min_depth = 4;
    // --pileup-min-baseq: M columns whose base quality (Phred, from the lane file's quality line) is below it
    // do not count; above 0 the workers' readers keep the quality lines (MSW_GFASTQ_QUAL)
    bool has_pileup_min_baseq = false;
    int pileup_min_baseq = 0;
    // --variants-out: the variant calls of the run's pileup (one .var file; include/msw.h, "Variants"), with the
    // thresholds of --call-min-depth / -alt / -alt-permille / -qual over msw_call_params_default
    std::string variants_out;
    bool has_call_flag = false;
    long call_min_depth = 4, call_min_alt = 2, call_min_alt_permille = 200, call_min_qual = 20;
    msw_call_params_t call_params() const {
        msw_call_params_t q;
        msw_call_params_default(&q);
        q.min_depth = (uint32_t)call_min_depth;
        q.min_alt = (uint32_t)call_min_alt;
        q.min_alt_permille = (uint32_t)call_min_alt_permille;
        q.min_qual = (uint32_t)call_min_qual;
        return q;
    }
    // --call-baseq: the calls weigh every observation by its base quality (include/msw.h, "Quality sums and
    // weighted genotypes"): the workers' readers keep the quality lines whatever --pileup-min-baseq says, their
    // pileups carry quality sums, and the .var file is an MSWVARQ1 one; --qsum-out: the summed quality sums (.mqs)
    bool call_baseq = false;
    std::string qsum_out;
    // the workers keep pileups for either output
    bool wants_pileup() const { return !pileup_out.empty() || !variants_out.empty(); }
    long chunk_size = 1, num_files = -1;
    std::string score_mode = "compat", gap_model = "linear", reference, checkpoint_dir = ".", json, scores_out, alignments_out;
    int match = 2, mismatch = -1, gap_open = 3, gap_extend = -1, window = 0, num_gpus = 1;
};

// Best cells cost ~1.5x the score-only kernel; --full-wgs needs them only for
// --scores-out records (the per-file results are score sums), pair mode prints
// them.
inline msw_scoring_t scoring_of(const Args& a, bool want_coords) {
    msw_scoring_t sc;
    sc.match = a.match;
    sc.mismatch = a.mismatch;
    sc.gap_open = a.gap_model == "affine" ? a.gap_open : 0;
    sc.gap_extend = a.gap_extend;
    sc.affine = a.gap_model == "affine";
    sc.want_coords = want_coords ? 1 : 0;
    return sc;
}

struct Device {
    int ordinal;
    std::string name;
    double memory_gb;
    uint32_t max_wg;
};

struct Ctx {
    msw_ctx* h = nullptr;
    // --full-wgs workers leave their context (and buffers) to the process
    // exit: main ends the process with _exit once the run record and the
    // checkpoint are written, so releasing them one by one (50-60 ms of
    // unregisters and frees after the last results) is work the OS redoes
    bool keep = false;
    explicit Ctx(int ordinal, unsigned flags = 0) {
        if (msw_ctx_create_ex(ordinal, flags, &h) != MSW_OK) die(std::string("GPU context error: ") + msw_last_error());
    }
    ~Ctx() {
        if (!keep) msw_ctx_destroy(h);
    }
};

// Read slab stride of sw mode: MSW_MAX_READ_LEN (default 256, the packed
// kernels' read limit; up to 32767 -- longer reads then score on the
// long-pair kernel, with either lane reader).
// (read on first use, so a bad value fails the run that needs it, not --help)
inline uint32_t read_stride() {
    static const uint32_t stride = [] {
        const long v = atol(env_or("MSW_MAX_READ_LEN", "256").c_str());
        if (v < 1 || v > 32767) die("error: MSW_MAX_READ_LEN must be in [1, 32767]");
        return std::max<uint32_t>(16u, ((uint32_t)v + 15u) & ~15u);
    }();
    return stride;
}
