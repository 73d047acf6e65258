// cli.cpp -- `rustseq_mini`, the reference CLI (smith_waterman/src/main.rs)
// rebuilt over the MI355X scorer's C ABI (include/msw.h, include/msw_fastq.h).
//
// Flags of main.rs:11-46 are kept (-1/--seq1, -2/--seq2, -f/--files,
// -c/--chunk-size (unused, as in the reference), -g/--gpu, -n/--num-files
// (unused), -t/--test-wgs, --full-wgs), plus:
//   --score-mode compat|sw   compat (default) = the kernel the reference launches
//                            (smith_waterman.cl:11-71); sw = Smith-Waterman
//   --gap-model linear|affine, --match/--mismatch/--gap-open/--gap-extend
//   --reference FASTA        sw --full-wgs: read i is scored against
//                            reference[pos : pos + window], pos from the
//                            "pos=" tag of its FASTQ header
//   --window N               window length (default 2 x read length)
//   --num-gpus N             --full-wgs: lane files sharded over N GPUs
//   --checkpoint-dir DIR     checkpoint_<run_id>.json written per file, resumed
//   --json PATH              run record (benchmark.rs:17-34 fields + GCUPS)
// Environment (.env loaded like dotenv, main.rs:50): WGS_DATA_DIR,
// WGS_SAMPLE_ID, WGS_LANES, WGS_READS_PER_LANE (aligner.rs:184-195),
// GPU_CHUNK_SIZE_READS (mandatory for chunked modes, aligner.rs:9-15),
// WGS_RUN_ID (stable checkpoint id).
//
// This file: arguments, main, the pair and -f modes.  The --full-wgs run is
// cli_wgs.cpp (its GPU lane reader's worker cli_lane_worker.cpp).
#include <ctime>
#include <fstream>
#include <functional>
#include <sstream>

#include "cli_wgs.h"
#include "msw_fastq.h"

namespace {

// dotenv::dotenv().ok() (main.rs:50): KEY=VALUE lines of ./.env, existing
// variables win, missing file is fine.
void load_dotenv() {
    std::ifstream f(".env");
    std::string line;
    while (std::getline(f, line)) {
        if (line.empty() || line[0] == '#') continue;
        const size_t eq = line.find('=');
        if (eq == std::string::npos) continue;
        std::string k = line.substr(0, eq), v = line.substr(eq + 1);
        while (!k.empty() && isspace((unsigned char)k.back())) k.pop_back();
        while (!v.empty() && isspace((unsigned char)v.front())) v.erase(v.begin());
        if (v.size() >= 2 && (v.front() == '"' || v.front() == '\'') && v.back() == v.front())
            v = v.substr(1, v.size() - 2);
        setenv(k.c_str(), v.c_str(), 0);
    }
}

void usage() {
    printf(
        "High-performance sequence alignment for genome-scale data (MI355X)\n\n"
        "Usage: rustseq_mini [OPTIONS]\n\n"
        "Options:\n"
        "  -1, --seq1 <SEQ1>            first sequence or file path\n"
        "  -2, --seq2 <SEQ2>            second sequence or file path\n"
        "  -f, --files                  treat inputs as file paths instead of direct sequences\n"
        "  -c, --chunk-size <N>         chunk size in MB (accepted, unused as in the reference)\n"
        "  -g, --gpu                    use GPU acceleration if available\n"
        "  -n, --num-files <N>          number of files (accepted, unused as in the reference)\n"
        "  -t, --test-wgs               count bases of the first lane's files\n"
        "      --full-wgs               process the full WGS dataset\n"
        "      --score-mode <compat|sw> compat = reference kernel semantics (default), sw = Smith-Waterman\n"
        "      --cigar                  --score-mode sw, one pair: also print the alignment's start and CIGAR\n"
        "                               (read <= 384, window <= 4096; with -f the pair is the two files' bases)\n"
        "      --gap-model <linear|affine>\n"
        "      --match N --mismatch N --gap-open N --gap-extend N\n"
        "      --reference <FASTA>      reference genome for --full-wgs --score-mode sw\n"
        "      --window N               window length (default 2 x read length)\n"
        "      --num-gpus N             GPUs for --full-wgs\n"
        "      --checkpoint-dir DIR     where checkpoint_<run_id>.json lives (default .)\n"
        "      --scores-out DIR         --full-wgs sw: per-read results, one <lane file>.scores per file\n"
        "                               (8 bytes per read in file order: i32 score, i16 end_i, i16 end_j)\n"
        "      --alignments-out DIR     --full-wgs sw, BGZF lane files read on the GPU: per-read alignments, one\n"
        "                               <lane file>.aln per file (genome position, score, NM, CIGAR with soft\n"
        "                               clips; blocks of reads, see DESIGN.md 4.10).  Reads <= 384 and windows\n"
        "                               <= 4096 bases.  Not available with the host (gzip) lane reader.\n"
        "      --both-strands           --full-wgs sw, BGZF lane files read on the GPU: score each read and its\n"
        "                               reverse complement against the window and keep the better (ties: the read\n"
        "                               as given); .aln blocks then carry a strand byte per read, and a strand-1\n"
        "                               record's end_i and CIGAR are in the reverse complement's coordinates\n"
        "      --map                    --full-wgs sw, BGZF lane files read on the GPU: place each read on the\n"
        "                               reference with a k-mer index and seed voting instead of a pos= tag in its\n"
        "                               header (an unplaced read scores 0, ref_pos -1).  With --scores-out it\n"
        "                               needs --alignments-out too: end cells are relative to the seeded window\n"
        "      --seed-k N               --map: k-mer length, 4..14 (default 12)\n"
        "      --seed-max-occ N         --map: k-mers with more occurrences are ignored, 1..64 (default 64)\n"
        "      --seed-band N            --map: width of the diagonal band that votes together (default 16)\n"
        "      --mapq                   --map: score a second candidate locus per read as well (the best other\n"
        "                               seed band at least --seed-sep diagonals away), keep the better-scoring one;\n"
        "                               .aln blocks then carry a mapping quality (0..60, an uncalibrated heuristic)\n"
        "                               and the other candidate's score per read\n"
        "      --seed-sep N             --mapq: least distance between the two candidates' diagonals, at least\n"
        "                               --seed-band (default 0: the read's window length)\n"
        "      --pileup-out PATH        --alignments-out: also write the pileup of the run's records, per genome\n"
        "                               base the reads showing A, C, G, T or something else, deleting it,\n"
        "                               inserting after it, and the reverse-strand share (one dense .mpu file,\n"
        "                               32 bytes per base, DESIGN.md 4.14).  One pileup covers one run: not with\n"
        "                               a checkpoint that already lists completed files\n"
        "      --pileup-min-mapq N      --pileup-out with --mapq: reads below this MAPQ do not count, 0..60\n"
        "                               (default 0)\n"
        "      --pileup-min-baseq N     --pileup-out or --variants-out: M columns whose base quality (Phred+33 in\n"
        "                               the lane file's quality line) is below this do not count, 0..93\n"
        "                               (default 0: the quality lines are not read)\n"
        "      --pileup-min-depth N     --pileup-out: least depth of a position in the summary's minority_ref\n"
        "                               (default 4)\n"
        "      --variants-out PATH      --alignments-out: also call variants from the run's pileup (with or without\n"
        "                               --pileup-out) and write them as one .var file: SNVs, deleted bases and\n"
        "                               insertion sites with a genotype (DESIGN.md 4.15).  --pileup-min-mapq\n"
        "                               applies.  Like a pileup, the calls cover one run\n"
        "      --call-min-depth N       --variants-out: least observations at a site, at least 1 (default 4)\n"
        "      --call-min-alt N         --variants-out: least observations of the alternative (default 2)\n"
        "      --call-min-alt-permille N  --variants-out: least share of the alternative, 0..1000 (default 200)\n"
        "      --call-min-qual N        --variants-out: least quality of a call (default 20)\n"
        "      --call-baseq             --variants-out: weigh every observation by its base quality (the lane\n"
        "                               files' quality lines are read; the .var file is an MSWVARQ1 one)\n"
        "      --qsum-out PATH          --call-baseq: write the per-base quality sums (.mqs)\n"
        "      --json PATH              write a JSON run record\n"
        "  -h, --help\n");
}

Args parse_args(int argc, char** argv) {
    Args a;
    auto need = [&](int& i) -> std::string {
        if (i + 1 >= argc) die(std::string("error: a value is required for '") + argv[i] + "'");
        return argv[++i];
    };
    for (int i = 1; i < argc; ++i) {
        std::string s = argv[i];
        std::string val;
        const size_t eq = s.find('=');
        if (s.rfind("--", 0) == 0 && eq != std::string::npos) { val = s.substr(eq + 1); s = s.substr(0, eq); }
        auto v = [&]() { return val.empty() ? need(i) : val; };
        if (s == "-1" || s == "--seq1") { a.seq1 = v(); a.has_seq1 = true; }
        else if (s == "-2" || s == "--seq2") { a.seq2 = v(); a.has_seq2 = true; }
        else if (s == "-f" || s == "--files") a.files = true;
        else if (s == "-c" || s == "--chunk-size") a.chunk_size = atol(v().c_str());
        else if (s == "-g" || s == "--gpu") a.gpu = true;
        else if (s == "-n" || s == "--num-files") a.num_files = atol(v().c_str());
        else if (s == "-t" || s == "--test-wgs") a.test_wgs = true;
        else if (s == "--full-wgs") a.full_wgs = true;
        else if (s == "--score-mode") a.score_mode = v();
        else if (s == "--cigar") a.cigar = true;
        else if (s == "--gap-model") a.gap_model = v();
        else if (s == "--match") a.match = atoi(v().c_str());
        else if (s == "--mismatch") a.mismatch = atoi(v().c_str());
        else if (s == "--gap-open") a.gap_open = atoi(v().c_str());
        else if (s == "--gap-extend") a.gap_extend = atoi(v().c_str());
        else if (s == "--reference") a.reference = v();
        else if (s == "--window") a.window = atoi(v().c_str());
        else if (s == "--num-gpus") a.num_gpus = atoi(v().c_str());
        else if (s == "--checkpoint-dir") a.checkpoint_dir = v();
        else if (s == "--json") a.json = v();
        else if (s == "--scores-out") a.scores_out = v();
        else if (s == "--alignments-out") a.alignments_out = v();
        else if (s == "--both-strands") a.both_strands = true;
        else if (s == "--map") a.map = true;
        else if (s == "--seed-k") a.seed_k = atoi(v().c_str());
        else if (s == "--seed-max-occ") a.seed_max_occ = atoi(v().c_str());
        else if (s == "--seed-band") a.seed_band = atoi(v().c_str());
        else if (s == "--mapq") a.mapq = true;
        else if (s == "--seed-sep") { a.seed_sep = atoi(v().c_str()); a.has_seed_sep = true; }
        else if (s == "--pileup-out") a.pileup_out = v();
        else if (s == "--pileup-min-mapq") { a.pileup_min_mapq = atoi(v().c_str()); a.has_pileup_min_mapq = true; }
        else if (s == "--pileup-min-baseq") { a.pileup_min_baseq = atoi(v().c_str()); a.has_pileup_min_baseq = true; }
        else if (s == "--pileup-min-depth") { a.pileup_min_depth = atoi(v().c_str()); a.has_pileup_min_depth = true; }
        else if (s == "--variants-out") a.variants_out = v();
        else if (s == "--call-min-depth") { a.call_min_depth = atol(v().c_str()); a.has_call_flag = true; }
        else if (s == "--call-min-alt") { a.call_min_alt = atol(v().c_str()); a.has_call_flag = true; }
        else if (s == "--call-min-alt-permille") { a.call_min_alt_permille = atol(v().c_str()); a.has_call_flag = true; }
        else if (s == "--call-min-qual") { a.call_min_qual = atol(v().c_str()); a.has_call_flag = true; }
        else if (s == "--call-baseq") a.call_baseq = true;
        else if (s == "--qsum-out") a.qsum_out = v();
        else if (s == "-h" || s == "--help") { usage(); exit(0); }
        else die("error: unexpected argument '" + s + "' found\n\nFor more information, try '--help'.");
    }
    if (a.score_mode != "compat" && a.score_mode != "sw") die("error: --score-mode must be compat or sw");
    if (a.gap_model != "linear" && a.gap_model != "affine") die("error: --gap-model must be linear or affine");
    if (a.gap_extend < 0) a.gap_extend = a.gap_model == "affine" ? 1 : 2;
    if (a.cigar && (a.score_mode != "sw" || a.full_wgs || a.test_wgs))
        die("error: --cigar needs --score-mode sw and one pair of sequences (-1 / -2, direct or with -f)");
    if (!a.alignments_out.empty()) {
        // traceback's range (include/msw.h): refused here, before any file is opened
        if (!a.full_wgs || a.score_mode != "sw") die("error: --alignments-out needs --full-wgs --score-mode sw");
        if (a.window > 4096) die("error: --alignments-out traces windows of at most 4096 bases (--window)");
        if (atol(env_or("MSW_MAX_READ_LEN", "256").c_str()) > 384)
            die("error: --alignments-out traces reads of at most 384 bases (MSW_MAX_READ_LEN)");
        if (env_or("MSW_GPU_INFLATE", "1") == "0")
            die("error: --alignments-out needs the GPU lane reader (MSW_GPU_INFLATE=0 selects the host reader)");
    }
    if (a.both_strands) {
        // refused here, before any file is opened, like --alignments-out
        if (!a.full_wgs || a.score_mode != "sw") die("error: --both-strands needs --full-wgs --score-mode sw");
        if (env_or("MSW_GPU_INFLATE", "1") == "0")
            die("error: --both-strands needs the GPU lane reader (MSW_GPU_INFLATE=0 selects the host reader)");
    }
    if (a.map) {
        // refused here, before any file is opened, like --both-strands
        if (!a.full_wgs || a.score_mode != "sw") die("error: --map needs --full-wgs --score-mode sw");
        if (env_or("MSW_GPU_INFLATE", "1") == "0")
            die("error: --map needs the GPU lane reader (MSW_GPU_INFLATE=0 selects the host reader)");
        if (!a.scores_out.empty() && a.alignments_out.empty())
            die("error: --map with --scores-out needs --alignments-out (end cells are relative to the seeded window)");
        if (a.seed_k < 4 || a.seed_k > 14) die("error: --seed-k must be 4..14");
        if (a.seed_max_occ < 1 || a.seed_max_occ > 64) die("error: --seed-max-occ must be 1..64");
        if (a.seed_band < 1) die("error: --seed-band must be at least 1");
    }
    // refused here, before any file is opened, like --map
    if (a.mapq && !a.map) die("error: --mapq needs --map");
    if (a.has_seed_sep && !a.mapq) die("error: --seed-sep needs --mapq");
    if (a.mapq && a.seed_sep != 0 && a.seed_sep < a.seed_band)
        die("error: --seed-sep must be 0 (the window length) or at least --seed-band");
    // refused here, before any file is opened, like --mapq
    if (!a.pileup_out.empty() && a.alignments_out.empty())
        die("error: --pileup-out needs --alignments-out (the records are made there)");
    if (!a.variants_out.empty() && a.alignments_out.empty())
        die("error: --variants-out needs --alignments-out (the records are made there)");
    if (a.has_pileup_min_mapq && (!a.wants_pileup() || !a.mapq))
        die("error: --pileup-min-mapq needs --pileup-out and --mapq");
    if (a.has_pileup_min_mapq && (a.pileup_min_mapq < 0 || a.pileup_min_mapq > 60))
        die("error: --pileup-min-mapq must be 0..60");
    if (a.has_pileup_min_baseq && !a.wants_pileup()) die("error: --pileup-min-baseq needs --pileup-out or --variants-out");
    if (a.has_pileup_min_baseq && (a.pileup_min_baseq < 0 || a.pileup_min_baseq > 93))
        die("error: --pileup-min-baseq must be 0..93");
    if (a.call_baseq && a.variants_out.empty()) die("error: --call-baseq needs --variants-out");
    if (!a.qsum_out.empty() && !a.call_baseq) die("error: --qsum-out needs --call-baseq");
    if (a.has_pileup_min_depth && a.pileup_out.empty()) die("error: --pileup-min-depth needs --pileup-out");
    if (a.has_pileup_min_depth && a.pileup_min_depth < 1) die("error: --pileup-min-depth must be at least 1");
    if (a.has_call_flag && a.variants_out.empty()) die("error: the --call-* thresholds need --variants-out");
    if (a.call_min_depth < 1 || a.call_min_depth > 0xFFFFFFFFl) die("error: --call-min-depth must be 1..4294967295");
    if (a.call_min_alt < 0 || a.call_min_alt > 0xFFFFFFFFl) die("error: --call-min-alt must be 0..4294967295");
    if (a.call_min_alt_permille < 0 || a.call_min_alt_permille > 1000) die("error: --call-min-alt-permille must be 0..1000");
    if (a.call_min_qual < 0 || a.call_min_qual > 0xFFFFFFFFl) die("error: --call-min-qual must be 0..4294967295");
    return a;
}

bool is_gpu_available() {
    int n = 0;
    return msw_device_count(&n) == MSW_OK && n > 0;
}

std::vector<Device> get_gpu_devices() {
    std::vector<Device> out;
    int n = 0;
    if (msw_device_count(&n) != MSW_OK) return out;
    for (int i = 0; i < n; ++i) {
        msw_device_info_t info;
        if (msw_device_info(i, &info) != MSW_OK) continue;
        out.push_back({i, info.name, info.mem_bytes / 1073741824.0, info.max_wg});
    }
    return out;
}

// gpu_align (aligner.rs:410-532) through msw_align_compat.
int32_t gpu_align(Ctx& ctx, const std::string& s1, const std::string& s2, const Device& dev, bool* ok,
                  std::string* err) {
    int32_t score = 0;
    const uint32_t wg = std::min<uint32_t>(dev.max_wg, 1024);
    const int rc = msw_align_compat(ctx.h, (const uint8_t*)s1.data(), s1.size(), (const uint8_t*)s2.data(),
                                    s2.size(), wg, 1000000, &score);
    *ok = rc == MSW_OK;
    if (!*ok && err) *err = msw_last_error();
    return score;
}

// A FASTQ file as chunks of concatenated sequences (the Vec<String> + concat
// of aligner.rs:270 / :392-393).
int for_each_fastq_chunk(const std::string& path, uint64_t chunk, const std::function<int(std::string&)>& fn,
                         uint64_t* bases = nullptr, uint64_t* reads = nullptr) {
    msw_fastq* fq = nullptr;
    if (msw_fastq_open(path.c_str(), &fq) != MSW_OK) return -1;
    constexpr uint32_t kStride = 4096;
    std::vector<uint8_t> slab((size_t)std::min<uint64_t>(chunk, 65536) * kStride);
    std::vector<uint16_t> lens(std::min<uint64_t>(chunk, 65536));
    std::string cat;
    uint64_t in_chunk = 0, nb = 0, nr = 0;
    int rc = 0;
    for (;;) {
        uint64_t want = std::min<uint64_t>(chunk - in_chunk, lens.size()), got = 0;
        rc = msw_fastq_next(fq, slab.data(), lens.data(), kStride, want, &got, nullptr);
        if (rc) break;
        for (uint64_t i = 0; i < got; ++i) {
            cat.append((const char*)slab.data() + i * kStride, lens[i]);
            nb += lens[i];
        }
        nr += got;
        in_chunk += got;
        if (got == 0 || in_chunk == chunk) {
            if (in_chunk > 0) {
                rc = fn(cat);
                if (rc) break;
            }
            cat.clear();
            in_chunk = 0;
            if (got == 0) break;
        }
    }
    msw_fastq_close(fq);
    if (bases) *bases = nb;
    if (reads) *reads = nr;
    return rc;
}

// GPU contexts of the --full-wgs workers: --num-gpus N of the visible devices,
// or the ordinals listed in MSW_DEVICES (comma separated; an ordinal may
// repeat: "0,0" runs two workers, each with its own context, on GPU 0 -- the
// multi-worker path on a one-GPU box).
std::vector<Device> worker_devices(const std::vector<Device>& devs, int n) {
    std::vector<Device> pool;
    const char* v = getenv("MSW_DEVICES");
    if (v && *v) {
        std::stringstream ss(v);
        std::string tok;
        while (std::getline(ss, tok, ',')) {
            char* end = nullptr;
            const long k = strtol(tok.c_str(), &end, 10);
            if (tok.empty() || *end || k < 0 || k >= (long)devs.size())
                die("error: MSW_DEVICES entry '" + tok + "' is not a visible GPU ordinal");
            pool.push_back(devs[(size_t)k]);
        }
    } else {
        pool = devs;
    }
    if (n < 1) die("error: --num-gpus must be >= 1");
    if (n > (int)pool.size())
        die("error: --num-gpus " + std::to_string(n) + " but only " + std::to_string(pool.size()) +
            " GPU context(s) available (visible GPUs, or MSW_DEVICES)");
    pool.resize((size_t)n);
    return pool;
}

std::string stable_run_id(const std::string& dir, const std::string& sample, const Args& a) {
    const char* v = getenv("WGS_RUN_ID");
    if (v && *v) return v;
    // FNV-1a over the inputs that define the run: same dataset + mode -> same id.
    // The scoring scheme and window are part of it: a checkpoint written under
    // other parameters is never resumed into this run.
    std::string key = dir + "|" + sample + "|" + a.score_mode + "|" + a.gap_model + "|" + a.reference + "|" +
                      env_or("GPU_CHUNK_SIZE_READS", "") + "|" + std::to_string(a.match) + "|" +
                      std::to_string(a.mismatch) + "|" + std::to_string(a.gap_open) + "|" +
                      std::to_string(a.gap_extend) + "|" + std::to_string(a.window) + "|" +
                      env_or("WGS_FILE_SHARD", "");
    // a run on both strands never resumes a one-strand checkpoint, nor the other way round
    if (a.both_strands) key += "|both-strands";
    // nor does a mapped run resume one that took its positions from the headers, or other seed parameters
    if (a.map)
        key += "|map|" + std::to_string(a.seed_k) + "|" + std::to_string(a.seed_max_occ) + "|" +
               std::to_string(a.seed_band);
    // nor does a run with a second candidate and MAPQ resume one without, or one with another separation
    if (a.mapq) key += "|mapq|" + std::to_string(a.seed_sep);
    // a pileup covers the files of one run: its run never resumes one without, or one with another threshold
    if (!a.pileup_out.empty()) key += "|pileup|" + std::to_string(a.pileup_min_mapq);
    // nor do calls, which come from that pileup: the least MAPQ of its reads and the four thresholds
    if (!a.variants_out.empty())
        key += "|variants|" + std::to_string(a.pileup_min_mapq) + "," + std::to_string(a.call_min_depth) + "," +
               std::to_string(a.call_min_alt) + "," + std::to_string(a.call_min_alt_permille) + "," +
               std::to_string(a.call_min_qual);
    // nor does either with a base-quality threshold resume one without, or one with another (0 is the run without)
    if (a.wants_pileup() && a.pileup_min_baseq > 0) key += "|baseq|" + std::to_string(a.pileup_min_baseq);
    // nor does a run with quality-weighted calls resume one without
    if (a.call_baseq) key += "|callq";
    uint64_t h = 1469598103934665603ull;
    for (unsigned char c : key) { h ^= c; h *= 1099511628211ull; }
    char buf[32];
    snprintf(buf, sizeof(buf), "wgs_%016llx", (unsigned long long)h);
    return buf;
}

void write_json(const std::string& path, const std::string& body) {
    if (path.empty()) return;
    std::ofstream f(path);
    f << body;
}

// CLOCK_REALTIME in ns: the run record's process timeline (t_main_unix_ns,
// t_record_unix_ns), so a parent can split its child's wall into start-up
// (exec -> main), main -> record and exit (record -> reaped).
long long unix_ns() {
    timespec t;
    clock_gettime(CLOCK_REALTIME, &t);
    return (long long)t.tv_sec * 1000000000ll + t.tv_nsec;
}

// This process's lane files (aligner.rs:184-195 names) and, in gidx, each
// one's index in the whole lane set of *n_lane_files files.
std::vector<std::string> lane_files(const std::string& dir, const std::string& sample, std::vector<size_t>* gidx,
                                    size_t* n_lane_files) {
    const int lanes = atoi(env_or("WGS_LANES", "8").c_str()) > 0 ? atoi(env_or("WGS_LANES", "8").c_str()) : 8;
    const int rpl = atoi(env_or("WGS_READS_PER_LANE", "2").c_str()) > 0
                        ? atoi(env_or("WGS_READS_PER_LANE", "2").c_str()) : 2;
    std::vector<std::string> files;
    for (int lane = 1; lane <= lanes; ++lane)
        for (int r = 1; r <= rpl; ++r) {
            char name[512];
            snprintf(name, sizeof(name), "%s/%s_L%03d_R%d_001.fastq.gz", dir.c_str(), sample.c_str(), lane, r);
            files.push_back(name);
        }
    *n_lane_files = files.size();
    gidx->resize(files.size());
    for (size_t i = 0; i < gidx->size(); ++i) (*gidx)[i] = i;
    // WGS_FILE_SHARD=r/N: this process takes lane files r, r+N, r+2N, ...
    // (one process per GPU, e.g. bench.py's config-4 leg under
    // torch.distributed.run; the reference has no multi-GPU path, gpu.rs:117,125)
    const std::string shard = env_or("WGS_FILE_SHARD", "");
    if (!shard.empty()) {
        int r = -1, n = 0;
        char tail = 0;
        if (sscanf(shard.c_str(), "%d/%d%c", &r, &n, &tail) != 2 || n < 1 || r < 0 || r >= n)
            die("error: WGS_FILE_SHARD must be r/N with 0 <= r < N, got '" + shard + "'");
        std::vector<std::string> mine;
        std::vector<size_t> mine_idx;
        for (size_t i = (size_t)r; i < files.size(); i += (size_t)n) {
            mine.push_back(files[i]);
            mine_idx.push_back(i);
        }
        files.swap(mine);
        gidx->swap(mine_idx);
        printf("File shard %d/%d: %zu lane file(s)\n", r, n, files.size());
    }
    return files;
}

// Sums over a run's files, as printed and recorded.
struct WgsTotals {
    long long score = 0;
    unsigned long long reads = 0, bases = 0;
};

// What the run record takes from main beside the report.
struct RecordInputs {
    std::string run_id;
    size_t total_files = 0, num_gpus = 0;
    double hip_init_ms = 0;
    long long t_main_ns = 0;
};

// Run record: the reference's BenchmarkResult fields (tools/benchmark.rs:17-34;
// its fake gpu_utilization_avg / gpu_memory_used_mb are dropped) plus GCUPS
// (kernel and end to end), HBM GB/s and roofline fractions.
void write_run_record(const Args& a, const std::vector<Device>& devices, const WgsReport& rep, const WgsTotals& tot,
                      const RecordInputs& in) {
    const unsigned long long reads = tot.reads, bases = tot.bases;
    const double secs = std::max(rep.wall_ms / 1000.0, 1e-9);
    char ts[64];
    {
        const time_t now = time(nullptr);
        struct tm tmv;
        gmtime_r(&now, &tmv);
        strftime(ts, sizeof(ts), "%Y-%m-%dT%H:%M:%SZ", &tmv);
    }
    double ram_gb = 0;
    {
        std::ifstream mi("/proc/meminfo");
        std::string k;
        double v = 0;
        if (mi >> k >> v && k == "MemTotal:") ram_gb = v / (1024.0 * 1024.0);
    }
    const double gcups_e2e = rep.cells ? rep.cells / (rep.wall_ms * 1e6) : 0.0;
    // Kernel rate: the job's cells over the busiest GPU's kernel time
    // (HIP events around every chunk's scoring launch, msw_ctx_stats),
    // the kernel time of the workers sharing a GPU summed.
    double kmax = 0, ksum = 0;
    unsigned long long alg = 0;
    std::map<int, double> per_dev;
    for (size_t i = 0; i < rep.gpu.size(); ++i) {
        per_dev[i < rep.gpu_dev.size() ? rep.gpu_dev[i] : (int)i] += rep.gpu[i].kernel_ms;
        ksum += rep.gpu[i].kernel_ms;
        alg += rep.gpu[i].alg_bytes;
    }
    for (const auto& kv : per_dev) kmax = std::max(kmax, kv.second);
    const int ng = (int)per_dev.size();  // physical GPUs
    const bool sw_mode = a.score_mode == "sw";
    const double gcups = kmax > 0 && sw_mode ? rep.cells / (kmax * 1e6) : 0.0;
    const double hbm_gbps = kmax > 0 ? alg / (kmax * 1e6) : 0.0;
    // Per-GPU ceilings: 8 TB/s HBM; VALU issue of the loop that ran (128
    // cells per 19.16 / 30.28 / 35.88 / 46.99 cycles per packed row-step for
    // linear / +coords / affine / +coords, x 1024 SIMDs x 2.4 GHz; bench.py
    // CYCLES_PER_ROW_STEP).
    const bool coords = !a.scores_out.empty();
    const double valu_ceiling = a.gap_model == "affine" ? (coords ? 6694.5 : 8767.6)
                                                        : (coords ? 10389.5 : 16418.2);
    const double frac_hbm = ng ? hbm_gbps / (8000.0 * ng) : 0.0;
    const double frac_valu = ng && sw_mode ? gcups / (valu_ceiling * ng) : 0.0;
    // Scoring time per GPU over the wall: each worker's kernel_ms is the
    // union of its own launches, but two workers on one GPU overlap, so
    // their sum can exceed the wall -- capped at 1 (an upper bound then).
    const double busy = ng && rep.wall_ms > 0 ? std::min(1.0, ksum / (ng * rep.wall_ms)) : 0.0;
    std::ostringstream j;
    j << "{\"timestamp\": \"" << ts << "\", \"run_id\": \"" << in.run_id << "\", \"mode\": \"full_wgs\""
      << ", \"score_mode\": \"" << a.score_mode << "\", \"files_processed\": " << rep.results.size()
      << ", \"total_files\": " << in.total_files << ", \"total_reads\": " << reads << ", \"total_bases\": " << bases
      << ", \"total_score\": " << tot.score << ", \"total_time_seconds\": " << secs << ", \"wall_ms\": " << rep.wall_ms
      << ", \"throughput_reads_per_second\": " << reads / secs
      << ", \"throughput_bases_per_second\": " << bases / secs << ", \"chunk_size\": " << get_chunk_size_reads()
      << ", \"cpu_cores_used\": " << usable_cpus() << ", \"host_reader_threads\": " << rep.readers
      << ", \"parallel_files\": " << (rep.readers > 1 || rep.host_threads > 1 ? "true" : "false")
      << ", \"system_info\": {\"gpu_name\": \"" << json_escape(devices.empty() ? "" : devices[0].name)
      << "\", \"gpu_memory_gb\": " << (devices.empty() ? 0.0 : devices[0].memory_gb)
      << ", \"cpu_cores\": " << std::thread::hardware_concurrency() << ", \"total_ram_gb\": " << ram_gb << "}"
      << ", \"num_gpus\": " << in.num_gpus << ", \"physical_gpus\": " << ng << ", \"host_cores\": " << std::thread::hardware_concurrency()
      << ", \"host_cpus_usable\": " << usable_cpus() << ", \"host_threads\": " << rep.host_threads
      << ", \"cells\": " << rep.cells << ", \"gcups\": " << gcups << ", \"gcups_end_to_end\": " << gcups_e2e
      << ", \"kernel_ms\": " << kmax << ", \"gpu_busy_fraction\": " << busy
      << ", \"alg_bytes\": " << alg << ", \"hbm_gbps\": " << hbm_gbps
      << ", \"roofline_fraction_hbm\": " << frac_hbm << ", \"roofline_fraction_valu\": " << frac_valu
      << ", \"gpu_inflate\": " << (rep.gpu_inflate ? "true" : "false") << ", \"setup_ms\": " << rep.setup_ms
      << ", \"setup_phases\": {\"hip_init_ms\": " << in.hip_init_ms << ", \"reference_load_ms\": " << rep.reference_load_ms
      << ", \"context_ms\": " << rep.context_ms << ", \"genome_ms\": " << rep.genome_ms
      << ", \"result_sets_ms\": " << rep.result_sets_ms << ", \"lane_reader_ms\": " << rep.lane_reader_ms
      << ", \"kernel_load_ms\": " << rep.kernel_load_ms << ", \"index_ms\": " << rep.index_ms << "}"
      << ", \"teardown_ms\": " << rep.teardown_ms
      << ", \"both_strands\": " << (rep.both_strands ? "true" : "false") << ", \"reverse_reads\": " << rep.reverse_reads
      << ", \"map\": " << (rep.map ? "true" : "false") << ", \"seed_k\": " << (rep.map ? a.seed_k : 0)
      << ", \"placed_reads\": " << rep.placed_reads;
    // --mapq only: reads with MAPQ 0, 1-29, 30-59, 60
    if (rep.mapq)
        j << ", \"mapq\": true, \"seed_sep\": " << a.seed_sep << ", \"mapq_histogram\": {\"0\": " << rep.mapq_hist[0]
          << ", \"1-29\": " << rep.mapq_hist[1] << ", \"30-59\": " << rep.mapq_hist[2] << ", \"60\": " << rep.mapq_hist[3]
          << "}";
    // --pileup-out only
    if (rep.pileup.on) {
        const PileupReport& p = rep.pileup;
        j << ", \"pileup\": {\"path\": \"" << json_escape(a.pileup_out) << "\", \"min_mapq\": " << a.pileup_min_mapq
          << ", \"min_depth\": " << a.pileup_min_depth << ", \"reads_used\": " << p.reads_used
          << ", \"reads_skipped\": " << p.reads_skipped << ", \"covered\": " << p.covered
          << ", \"depth_sum\": " << p.depth_sum << ", \"max_depth\": " << p.max_depth
          << ", \"minority_ref\": " << p.minority_ref;
        // --pileup-min-baseq above 0 only: the threshold and the M columns it dropped, over the workers
        if (a.pileup_min_baseq > 0) j << ", \"min_baseq\": " << a.pileup_min_baseq << ", \"lowq_columns\": " << p.lowq_columns;
        j << ", \"pileup_ms\": " << p.ms << "}";
    }
    // --variants-out only
    if (rep.variants.on) {
        const VariantsReport& v = rep.variants;
        const msw_call_params_t q = a.call_params();
        j << ", \"variants\": {\"path\": \"" << json_escape(a.variants_out) << "\", \"min_mapq\": " << a.pileup_min_mapq
          << ", \"params\": {\"min_depth\": " << q.min_depth << ", \"min_alt\": " << q.min_alt
          << ", \"min_alt_permille\": " << q.min_alt_permille << ", \"min_qual\": " << q.min_qual
          << ", \"q_hit\": " << q.q_hit << ", \"q_miss\": " << q.q_miss << ", \"q_het\": " << q.q_het
          << ", \"prior_het\": " << q.prior_het << ", \"prior_hom\": " << q.prior_hom << "}, \"records\": " << v.total
          << ", \"snv\": " << v.by_kind[0] << ", \"del\": " << v.by_kind[1] << ", \"ins\": " << v.by_kind[2]
          << ", \"het\": " << v.by_gt[1] << ", \"hom\": " << v.by_gt[2];
        if (a.pileup_min_baseq > 0) j << ", \"min_baseq\": " << a.pileup_min_baseq << ", \"lowq_columns\": " << v.lowq_columns;
        // --call-baseq only
        if (a.call_baseq) {
            msw_call_qparams_t qq;
            msw_call_qparams_default(&qq);
            j << ", \"baseq_weighted\": true, \"q_scale\": " << qq.q_scale << ", \"q_third\": " << qq.q_third;
        }
        j << ", \"variants_ms\": " << v.ms << "}";
    }
    j
      << ", \"inflate_bytes_in\": " << rep.gz_in << ", \"inflate_bytes_out\": " << rep.gz_out
      << ", \"reads_per_second\": " << reads / secs << ", \"t_main_unix_ns\": " << in.t_main_ns
      << ", \"t_record_unix_ns\": " << unix_ns() << "}\n";
    write_json(a.json, j.str());
}

// --full-wgs: the lane files, the checkpoint, the run, its summary and record.
[[noreturn]] void full_wgs_mode(const Args& a, const std::vector<Device>& devices, ReferenceLoad& ref,
                                double hip_init_ms, long long t_main_ns) {
    printf("Processing FULL WGS dataset...\n");
    if (!a.gpu || !is_gpu_available()) die("error: gpu acceleration is required for full WGS processing");
    const std::string dir = env_or("WGS_DATA_DIR", "/path/to/wgs/data");
    const std::string sample = env_or("WGS_SAMPLE_ID", "SAMPLE_ID");
    std::vector<size_t> gidx;
    size_t n_lane_files = 0;
    const std::vector<std::string> files = lane_files(dir, sample, &gidx, &n_lane_files);
    Checkpoint ck;
    ck.run_id = stable_run_id(dir, sample, a);
    ck.path = a.checkpoint_dir + "/checkpoint_" + ck.run_id + ".json";
    ck.total_files = files.size();
    if (ck.load()) printf("Resuming run %s from %s\n", ck.run_id.c_str(), ck.path.c_str());
    if (a.wants_pileup())
        for (const auto& kv : ck.files)
            if (kv.second.completed)
                die(std::string("error: ") + (a.pileup_out.empty() ? "--variants-out" : "--pileup-out") +
                    " covers the files of one run, but " + ck.path +
                    " already lists a completed file: remove the checkpoint to run all files again");
    const std::vector<Device> workers = worker_devices(devices, a.num_gpus);
    const WgsReport rep = run_full_wgs(a, workers, files, gidx, n_lane_files, ck, ref);
    WgsTotals tot;
    bool all_ok = true;
    printf("\nFULL WGS PROCESSING COMPLETE\n==========================================\n");
    printf("Total files processed: %zu\n", rep.results.size());
    for (const auto& r : rep.results) {
        printf("File %zu: Score=%lld, Time=%.2fs\n", r.file_index + 1, r.score, r.processing_time_ms / 1000.0);
        tot.score += r.score;
        tot.reads += r.total_reads;
        tot.bases += r.total_bases;
        all_ok = all_ok && r.completed;
    }
    printf("Total reads: %llu, total bases: %llu, total score: %lld\n", tot.reads, tot.bases, tot.score);
    if (rep.both_strands) printf("Both strands: %llu reverse reads\n", rep.reverse_reads);
    if (rep.map) printf("Mapped (k = %d): %llu of %llu reads placed\n", a.seed_k, rep.placed_reads, tot.reads);
    if (rep.mapq)
        printf("MAPQ: %llu reads at 0, %llu at 1-29, %llu at 30-59, %llu at 60\n", rep.mapq_hist[0], rep.mapq_hist[1],
               rep.mapq_hist[2], rep.mapq_hist[3]);
    if (rep.pileup.on)
        printf("Pileup: %llu reads used, %llu skipped, %llu bases covered, depth sum %llu, max depth %llu, %llu "
               "positions with the reference base in the minority at depth >= %d, %.1f ms -> %s\n",
               rep.pileup.reads_used, rep.pileup.reads_skipped, rep.pileup.covered, rep.pileup.depth_sum,
               rep.pileup.max_depth, rep.pileup.minority_ref, a.pileup_min_depth, rep.pileup.ms, a.pileup_out.c_str());
    if (rep.variants.on)
        printf("Variants: %llu records (%llu SNV, %llu DEL, %llu INS; %llu 0/1, %llu 1/1), %.1f ms -> %s\n",
               rep.variants.total, rep.variants.by_kind[0], rep.variants.by_kind[1], rep.variants.by_kind[2],
               rep.variants.by_gt[1], rep.variants.by_gt[2], rep.variants.ms, a.variants_out.c_str());
    printf("Wall time: %.2f s", rep.wall_ms / 1000.0);
    if (rep.cells) printf(", %.1f GCUPS end-to-end", rep.cells / (rep.wall_ms * 1e6));
    printf("\n");
    write_run_record(a, devices, rep, tot, RecordInputs{ck.run_id, files.size(), workers.size(), hip_init_ms, t_main_ns});
    // Records, scores files and checkpoint are written and closed: end the
    // process here.  The workers' contexts, genomes and pinned buffers are
    // released by the exit itself (Ctx::keep), not call by call.
    // Under rocprofv3 (its tool library is named in the environment) the
    // ordinary exit runs, so the profiler's exit handlers write its
    // output; the contexts are still left to the runtime's own exit.
    fflush(stdout);
    fflush(stderr);
    if (getenv("ROCP_TOOL_LIBRARIES") || getenv("ROCPROF_OUTPUT_PATH")) exit(all_ok ? 0 : 1);
    _exit(all_ok ? 0 : 1);
}

int test_wgs_mode() {
    printf("Testing WGS file reading from configured directory...\n");
    const std::string dir = env_or("WGS_DATA_DIR", "/path/to/wgs/data");
    const std::string sample = env_or("WGS_SAMPLE_ID", "SAMPLE_ID");
    for (const char* rr : {"R1", "R2"}) {
        const std::string file = sample + "_L001_" + rr + "_001.fastq.gz";
        const std::string full = dir + "/" + file;
        printf("Testing: %s\n", full.c_str());
        uint64_t bases = 0, reads = 0;
        get_chunk_size_reads();  // count_bases_in_fastq needs it (aligner.rs:538)
        if (msw_fastq_count_bases(full.c_str(), &bases, &reads) == MSW_OK)
            printf("✅ Successfully counted %llu bases in %s\n", (unsigned long long)bases, file.c_str());
        else
            printf("❌ Error counting bases in %s: %s\n", file.c_str(), msw_last_error());
    }
    return 0;
}

// --cigar with -f: the pair is the bases of file 1 (its reads in file
// order, concatenated) against the bases of file 2; it then runs as a
// direct pair.  Reading stops once a file is past every limit.
// False (after the message) when a file cannot be read.
bool load_cigar_files(Args& a) {
    for (std::string* seq : {&a.seq1, &a.seq2}) {
        const std::string path = *seq;
        std::string bases;
        const int rc = for_each_fastq_chunk(path, 64, [&](std::string& c) {
            bases += c;
            return bases.size() > 32767 ? 2 : 0;
        });
        if (rc != 0 && rc != 2) {
            fprintf(stderr, "GPU alignment error: %s\n", msw_last_error());
            return false;
        }
        if (rc == 0) printf("Loaded %llu bases from %s\n", (unsigned long long)bases.size(), path.c_str());
        *seq = bases;
    }
    a.files = false;
    return true;
}

// gpu_align_pair (aligner.rs:376-407)
int files_mode(const Args& a, Ctx& ctx, const Device& dev) {
    uint64_t b1 = 0, b2 = 0, r = 0;
    const uint64_t chunk = get_chunk_size_reads();
    if (msw_fastq_count_bases(a.seq1.c_str(), &b1, &r) || msw_fastq_count_bases(a.seq2.c_str(), &b2, &r)) {
        fprintf(stderr, "GPU alignment error: %s\n", msw_last_error());
        return 1;
    }
    printf("Loaded %llu bases from %s\n", (unsigned long long)b1, a.seq1.c_str());
    printf("Loaded %llu bases from %s\n", (unsigned long long)b2, a.seq2.c_str());
    const auto t0 = Clock::now();
    // File 2's chunks are cached (the reference re-decompresses file 2 once
    // per chunk of file 1, aligner.rs:390-398; the sum is identical).
    std::vector<std::string> chunks2;
    for_each_fastq_chunk(a.seq2, chunk, [&](std::string& c) { chunks2.push_back(c); return 0; });
    int32_t total = 0;  // i32 sum, wrapping like a release build
    std::string err;
    const int rc = for_each_fastq_chunk(a.seq1, chunk, [&](std::string& c1) {
        for (const auto& c2 : chunks2) {
            bool ok = false;
            const int32_t s = gpu_align(ctx, c1, c2, dev, &ok, &err);
            if (!ok) return 1;
            total = (int32_t)((uint32_t)total + (uint32_t)s);
        }
        return 0;
    });
    if (rc) {
        fprintf(stderr, "GPU alignment error: %s\n", err.empty() ? msw_last_error() : err.c_str());
        return 1;
    }
    printf("GPU Alignment Result:\n  Score: %d\n  Processing time: %.2f ms\n  GPU device: %s\n", total,
           (double)(long long)ms_since(t0), dev.name.c_str());
    return 0;
}

// --score-mode sw, one direct pair: score and best cell, with --cigar the alignment.
int sw_pair_mode(const Args& a, Ctx& ctx) {
    msw_scoring_t sc = scoring_of(a, true);
    const size_t rs = std::max<size_t>(16, (a.seq1.size() + 15) / 16 * 16);
    const size_t ws = std::max<size_t>(16, (a.seq2.size() + 15) / 16 * 16);
    std::vector<uint8_t> r(rs, 0), w(ws, 0);
    memcpy(r.data(), a.seq1.data(), a.seq1.size());
    memcpy(w.data(), a.seq2.data(), a.seq2.size());
    if (a.seq1.size() > 32767 || a.seq2.size() > 32767) {
        fprintf(stderr, "GPU alignment error: sequence of %zu / %zu bases exceeds the kernel limits "
                        "(read <= 32767, window <= 32767)\n", a.seq1.size(), a.seq2.size());
        return 1;
    }
    uint16_t rl = (uint16_t)a.seq1.size(), wl = (uint16_t)a.seq2.size();
    int32_t score = 0;
    int16_t ei = -1, ej = -1;
    msw_batch_t b{r.data(), w.data(), &rl, &wl, (uint32_t)rs, (uint32_t)ws, 1};
    msw_out_t o{&score, &ei, &ej};
    int16_t si = -1, sj = -1;
    int32_t n_ops = 0;
    std::vector<uint32_t> ops;
    if (a.cigar) {
        // one pass sized for the common case, a second with the count the pair needs
        for (uint32_t stride = 64;; stride = (uint32_t)n_ops) {
            ops.assign(stride, 0);
            msw_trace_t tr{&si, &sj, &n_ops, ops.data(), stride};
            if (msw_align_batch_trace(ctx.h, &sc, &b, &o, &tr, 0) != MSW_OK) {
                fprintf(stderr, "GPU alignment error: %s\n", msw_last_error());
                return 1;
            }
            if (n_ops <= (int32_t)stride) break;
        }
    } else if (msw_align_batch(ctx.h, &sc, &b, &o, 0) != MSW_OK) {
        fprintf(stderr, "GPU alignment error: %s\n", msw_last_error());
        return 1;
    }
    printf("GPU Alignment score: %d\n", score);
    printf("Best cell: read %d, window %d\n", ei, ej);
    if (a.cigar) {
        std::string text;
        for (int32_t k = 0; k < n_ops; ++k) text += std::to_string(ops[k] >> 4) + "MID?"[std::min<uint32_t>(ops[k] & 15u, 3u)];
        printf("Alignment start: read %d, window %d\n", si, sj);
        printf("CIGAR: %s\n", n_ops ? text.c_str() : "*");
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    const long long t_main_ns = unix_ns();
    load_dotenv();
    Args a = parse_args(argc, argv);
    // --full-wgs sw: the reference loads beside the HIP runtime init
    // (setup_phases.reference_load_ms is its own duration)
    ReferenceLoad ref;
    if (a.full_wgs && a.score_mode == "sw" && !a.reference.empty()) ref.start(a.reference);
    const auto t_hip = Clock::now();
    const auto devices = get_gpu_devices();  // the first HIP call: runtime init
    const double hip_init_ms = ms_since(t_hip);
    printf("Detecting system information...\n");
    for (const auto& d : devices) printf("  GPU %d: %s (%.1f GB)\n", d.ordinal, d.name.c_str(), d.memory_gb);
    if (devices.empty()) printf("  No GPU detected\n");

    if (a.full_wgs) full_wgs_mode(a, devices, ref, hip_init_ms, t_main_ns);
    if (a.test_wgs) return test_wgs_mode();

    if (!a.has_seq1) die("--seq1 is required when not in test mode");
    if (!a.has_seq2) die("--seq2 is required when not in test mode");
    if (!a.gpu || !is_gpu_available()) die("error: gpu acceleration is required and no compatible gpu was found");
    printf("GPU acceleration enabled\n");
    for (const auto& d : devices) printf("  Found GPU: %s (%g GB)\n", d.name.c_str(), d.memory_gb);
    const Device& dev = devices[0];
    Ctx ctx(dev.ordinal);

    if (a.files && a.cigar && !load_cigar_files(a)) return 1;
    if (a.files) return files_mode(a, ctx, dev);
    if (a.score_mode == "sw") return sw_pair_mode(a, ctx);
    bool ok = false;
    std::string err;
    const int32_t score = gpu_align(ctx, a.seq1, a.seq2, dev, &ok, &err);
    if (!ok) {
        fprintf(stderr, "GPU alignment error: %s\n", err.c_str());
        return 1;
    }
    printf("GPU Alignment score: %d\n", score);
    return 0;
}

