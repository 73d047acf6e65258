/*
 * msw.h -- C ABI of the MI355X-native batched Smith-Waterman scorer.
 *
 * This is the drop-in boundary for the `smith_waterman` crate's scoring path
 * (bmwoolf/mini_parallel, package `rustseq_mini`).  The reference has no FFI
 * layer of its own (binary-only crate, Cargo.toml:7-17); each entry point
 * below names the Rust item it replaces (file:line under smith_waterman/src/).
 * A Rust crate binds it with a plain `extern "C"` block.
 *
 * Contract
 *  - C99 POD only; no C++ exceptions cross this boundary; every int-returning
 *    call returns MSW_OK (0) or a negative MSW_E* code, and msw_last_error()
 *    returns the thread-local message (mirrors Result<_, String>, e.g.
 *    aligner.rs:452-455).
 *  - One msw_ctx per GPU, used by one host thread at a time.  Contexts on
 *    different GPUs run concurrently.  The library owns all device memory and
 *    streams; the caller owns every host array it passes in.
 *  - Byte semantics follow the reference kernel: substitution is byte
 *    equality (smith_waterman.cl:43,114), case-sensitive, 'N' == 'N'.
 *  - Score = global max cell, >= 0.  Coordinates = 0-based (i in read, j in
 *    window) of the best cell, smallest i then smallest j on ties; (-1,-1)
 *    when the score is 0 or the pair is empty.
 *  - Supported by the GPU kernels: read and window lengths <= 32767 (pairs
 *    up to 384 x 4096 run on the packed 16-bit kernels, longer ones on the
 *    i32 long-pair kernel, in the same call), 1 <= match <= 64,
 *    match - 64 <= mismatch <= 0, 0 <= gap_extend <= 1024,
 *    0 <= gap_open <= 30000.  Anything else -> MSW_E_RANGE.
 *    There is no CPU fallback: without a usable GPU every call fails.
 */
#ifndef MSW_H
#define MSW_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSW_OK 0
#define MSW_E_INVALID (-1)   /* bad argument / NULL pointer              */
#define MSW_E_RANGE (-2)     /* length or scoring outside kernel limits  */
#define MSW_E_DEVICE (-3)    /* HIP runtime / launch failure             */
#define MSW_E_NODEVICE (-4)  /* no GPU (is_gpu_available() == false)     */
#define MSW_E_NOMEM (-5)     /* device or pinned allocation failed       */

/* Replaces GpuDevice{name, memory_gb, max_work_group_size} (gpu.rs:17-22). */
typedef struct {
    char name[256];
    uint64_t mem_bytes;
    uint64_t mem_free_bytes;    /* hipMemGetInfo; replaces system_info.rs:236-243 */
    uint32_t max_wg;            /* max work-group size (gpu.rs:62)           */
    uint32_t cu_count;
    char arch[64];              /* e.g. "gfx950"                             */
} msw_device_info_t;

/* Scoring.  Reference constants: match +2, mismatch -1, gap 2
 * (smith_waterman.cl:5-7).  Linear gap: affine = 0, gap_extend = gap penalty,
 * gap_open ignored.  Affine (Gotoh): a gap of length k costs
 * gap_open + k * gap_extend.  want_coords = 1 fills end_i / end_j. */
typedef struct {
    int32_t match;
    int32_t mismatch;
    int32_t gap_open;
    int32_t gap_extend;
    int32_t affine;
    int32_t want_coords;
} msw_scoring_t;

/* A padded SoA batch: pair p uses reads[p*read_stride ..][0, read_len[p]) and
 * wins[p*win_stride ..][0, win_len[p]).  In msw_align_batch the pointers are
 * host memory (pageable or msw_host_alloc'ed); in msw_align_batch_device they
 * are device memory.  Replaces the Vec<String> chunk handed to the loader
 * callback (aligner.rs:107-108, :128-147). */
typedef struct {
    const uint8_t* reads;
    const uint8_t* wins;
    const uint16_t* read_len;
    const uint16_t* win_len;
    uint32_t read_stride;
    uint32_t win_stride;
    uint64_t n_pairs;
} msw_batch_t;

/* Caller-owned outputs (host in msw_align_batch, device in _device).
 * end_i / end_j may be NULL when want_coords == 0. */
typedef struct {
    int32_t* score;
    int16_t* end_i;
    int16_t* end_j;
} msw_out_t;

typedef struct msw_ctx msw_ctx;

/* gpu.rs:33-45 is_gpu_available / gpu.rs:48-94 get_gpu_devices. */
int msw_device_count(int* n);
int msw_device_info(int ordinal, msw_device_info_t* out);

/* gpu.rs:97-132 get_opencl_context/init_opencl: one context per device with
 * compute, copy and readback streams and three pinned staging slots (up to
 * three chunks in flight). */
int msw_ctx_create(int ordinal, msw_ctx** out);
/* msw_ctx_create with flags.  MSW_CTX_LEAN: only the compute stream up
 * front; the copy / second compute / readback / side streams are made by the
 * first call that needs them (host-batch calls, long pairs beside packed
 * ones).  A stream costs 3-30 ms to create -- the first few of a process each
 * make a hardware queue -- and the --full-wgs GPU-reader workers, which
 * score device-resident batches only, never use them.  Without the flag all
 * five streams are made here, before any the caller creates, so they land
 * on their own hardware queues.  The library reads its environment switches
 *  once, here. */
#define MSW_CTX_LEAN 1u
int msw_ctx_create_ex(int ordinal, unsigned flags, msw_ctx** out);
void msw_ctx_destroy(msw_ctx* ctx);

/* Batched scoring from host memory, synchronous.  Streams the batch through
 * pinned staging in chunks of `chunk_pairs` (0 = GPU_CHUNK_SIZE_READS env, or
 * 65536) with H2D copies on the copy stream overlapped with the kernels (a
 * one-chunk call keeps its copies and kernels on one compute stream; async
 * one-chunk calls alternate two, so consecutive calls overlap).
 * Pageable arrays are staged (rows repacked to 16-byte-rounded strides, so
 * padding does not cross PCIe); arrays in pinned memory (msw_host_alloc or
 * hipHostRegister) are copied to the GPU directly.
 * Replaces the per-chunk gpu_align loop of aligner.rs:269-289 / :390-398. */
int msw_align_batch(msw_ctx* ctx, const msw_scoring_t* sc, const msw_batch_t* batch,
                    msw_out_t* out, uint64_t chunk_pairs);

/* Same, asynchronous: returns a ticket; host arrays must stay alive and
 * unmodified until msw_wait(ticket) returns. */
int msw_align_batch_async(msw_ctx* ctx, const msw_scoring_t* sc, const msw_batch_t* batch,
                          msw_out_t* out, uint64_t chunk_pairs, uint64_t* ticket);
int msw_wait(msw_ctx* ctx, uint64_t ticket);

/* Device-resident batch: pointers in `batch` and `out` are device memory.
 * Enqueued on `stream` (a hipStream_t; NULL = the context's compute stream),
 * no host synchronisation.  max_read_len / max_win_len bound the batch (the
 * caller knows them; they select the kernel instance and the LDS size). */
int msw_align_batch_device(msw_ctx* ctx, const msw_scoring_t* sc, const msw_batch_t* batch,
                           msw_out_t* out, uint32_t max_read_len, uint32_t max_win_len,
                           void* stream);

/* Traceback: the alignment itself -- its first cell and its CIGAR.
 *
 * The canonical alignment (unique, so a second implementation can be
 * compared op for op):
 *  - it ends at the best cell as defined above (max score, smallest i, then
 *    smallest j); H, E, F are the recurrence of the scorer, byte-equality
 *    substitution s(i,j), H[-1][*] = H[*][-1] = 0, E = F = -inf outside;
 *  - the walk starts at (end_i, end_j) in state H.
 *    Linear, at (i, j):  H == 0 -> stop (the cell is not part of the
 *    alignment); H == H[i-1][j-1] + s(i,j) -> emit M, go to (i-1, j-1);
 *    else H == H[i-1][j] - gap -> emit I (a read base against nothing), go to
 *    (i-1, j); else emit D, go to (i, j-1).
 *    Affine (goe = gap_open + gap_extend), state H:  H == 0 -> stop;
 *    H == H[i-1][j-1] + s -> emit M, go to (i-1, j-1); else H == F[i][j] ->
 *    state F at the same cell; else state E at the same cell.
 *    State F: emit I, go to (i-1, j); the next state is H if
 *    F[i][j] == H[i-1][j] - goe (opening preferred), else F.
 *    State E: emit D, go to (i, j-1); the next state is H if
 *    E[i][j] == H[i][j-1] - goe, else E.
 *    Precedence: diagonal > I > D, open > extend.
 *  - start_i / start_j: the cell of the last M emitted (the first aligned
 *    cell); the CIGAR: the ops in forward order, run-length merged, encoded
 *    like BAM as len << 4 | op with M = 0, I = 1, D = 2.  Score 0 or an empty
 *    pair: start (-1, -1) and 0 ops.  The first and last ops are M, adjacent
 *    ops differ, every length is >= 1.
 *
 * Range: traceback supports the packed kernels' range only, read <= 384 and
 * window <= 4096; a longer pair (or bound) in a traceback call returns
 * MSW_E_RANGE (scoring such pairs stays available through the calls above).
 *
 * Overflow: when a pair needs more than cigar_stride ops, n_cigar[p] still
 * holds the count it needs, its cigar row is unspecified (nothing is written
 * past the row), and start_i / start_j are valid. */
typedef struct {
    int16_t* start_i;      /* first aligned read base, -1 when score == 0 */
    int16_t* start_j;
    int32_t* n_cigar;      /* ops the pair needs */
    uint32_t* cigar;       /* [n_pairs][cigar_stride], len << 4 | op, M=0 I=1 D=2 */
    uint32_t cigar_stride;
} msw_trace_t;

/* Device-resident: every pointer in `batch`, `ends` and `tr` is device memory.
 * `ends` holds the score / end_i / end_j already computed for this batch and
 * scheme (msw_align_batch_device with want_coords = 1); the trace refills only
 * rows 0..end_i and columns 0..end_j of each pair and does not search for the
 * maximum again.  sc->want_coords is not read.  Enqueued on `stream` (NULL =
 * the context's compute stream), no host synchronisation. */
int msw_trace_batch_device(msw_ctx* ctx, const msw_scoring_t* sc, const msw_batch_t* batch, const msw_out_t* ends,
                           msw_trace_t* tr, uint32_t max_read_len, uint32_t max_win_len, void* stream);
/* Host memory, synchronous: scores with coordinates (want_coords is forced),
 * then traces, in chunks of `chunk_pairs` (0 = 65536).  All of out->score,
 * out->end_i and out->end_j are required. */
int msw_align_batch_trace(msw_ctx* ctx, const msw_scoring_t* sc, const msw_batch_t* batch, msw_out_t* out,
                          msw_trace_t* tr, uint64_t chunk_pairs);

/* Length-bucketed plan for a device-resident batch of mixed lengths (BASELINE
 * config 5).  Built on the host from host copies of the length arrays (the
 * FASTQ loader has them): pairs are grouped by rows per lane (read length /
 * 16) and by window length, and the slot -> pair order is uploaded once;
 * msw_align_batch_planned then scores the whole batch in ONE kernel launch,
 * heaviest bucket first, enqueued on `stream` like msw_align_batch_device.
 * A plan belongs to its context and fixes the scoring scheme and the lengths:
 * reuse it for every pass over the same batch.  This is the device-resident
 * form of msw_align_batch's per-chunk bucketing (which replaces the
 * one-string-per-call gpu_align loop, aligner.rs:269-289). */
typedef struct msw_plan msw_plan;
int msw_plan_create(msw_ctx* ctx, const msw_scoring_t* sc, const uint16_t* read_len,
                    const uint16_t* win_len, uint64_t n_pairs, msw_plan** out);
int msw_align_batch_planned(msw_ctx* ctx, const msw_plan* plan, const msw_batch_t* batch,
                            msw_out_t* out, void* stream);
void msw_plan_destroy(msw_plan* plan);

/* == gpu_align(seq1, seq2, device) (aligner.rs:410-532): the kernel the
 * reference actually launches (smith_waterman.cl:11-71) with its host geometry
 * W = min(max_wg, 1024) (aligner.rs:422), G = min(ceil(L/W), max_groups)
 * (:423-424; reference max_groups = 1,000,000, gpu.rs:10), L = min(n1, n2),
 * L == 0 -> 0 (:414-416), L > 1,024,000,000 or > 0.8*mem/3 -> MSW_E_RANGE
 * (:436-456).  wg == 0 -> device max work-group size capped at 1024. */
int msw_align_compat(msw_ctx* ctx, const uint8_t* s1, size_t n1, const uint8_t* s2, size_t n2,
                     uint32_t wg, uint32_t max_groups, int32_t* score);

/* Pinned host memory (hipHostMalloc); replaces USE_PINNED_MEMORY /
 * alloc_host_ptr (aligner.rs:466-475). */
void* msw_host_alloc(size_t bytes);
void msw_host_free(void* p);

/* Reference genome resident in HBM.  The --full-wgs sw driver scores each
 * read against a window of the reference genome; the reference crate builds
 * every input on the host per chunk (aligner.rs:269-289).  Here the genome is
 * uploaded once per GPU and windows are cut on the GPU from (position,
 * length), so a chunk ships reads + 8-byte positions over PCIe instead of
 * reads + windows (~2.7x fewer bytes at 150 bp x 300 bp).  A genome belongs to
 * the context it was created on; destroy it before that context. */
typedef struct msw_genome msw_genome;
int msw_genome_create(msw_ctx* ctx, const uint8_t* seq, uint64_t len, msw_genome** out);
void msw_genome_destroy(msw_genome* g);
uint64_t msw_genome_length(const msw_genome* g);

/* Device-resident form: cut the windows of n (position, requested length)
 * pairs (device arrays) into a device slab wins[n][win_stride] (win_stride a
 * multiple of 16, wins 16-byte aligned; zero-padded), writing the clipped
 * lengths to win_len_out (may be NULL) -- the input msw_align_batch_device /
 * msw_align_batch_planned take.  Enqueued on `stream` (NULL = the context's
 * compute stream).  Windows are also clipped at win_stride. */
int msw_genome_cut_device(msw_ctx* ctx, const msw_genome* g, const int64_t* win_pos, const uint16_t* win_len,
                          uint64_t n, uint8_t* wins, uint32_t win_stride, uint16_t* win_len_out, void* stream);

/* Reads against genome windows: pair p scores reads[p*read_stride ..][0,
 * read_len[p]) against genome[win_pos[p], win_pos[p] + win_len[p]), the
 * window clipped at the genome end; win_pos < 0 or >= the genome length is an
 * empty window (score 0, coordinates (-1,-1)).  The requested win_len is
 * bounded like a window length (<= 4096).  Host arrays as in
 * msw_align_batch (pageable or msw_host_alloc'ed: pinned arrays are copied to
 * the GPU directly, without staging). */
typedef struct {
    const uint8_t* reads;
    const uint16_t* read_len;
    uint32_t read_stride;
    const int64_t* win_pos;
    const uint16_t* win_len;
    uint64_t n_pairs;
} msw_read_batch_t;

int msw_align_reads(msw_ctx* ctx, const msw_scoring_t* sc, const msw_genome* g, const msw_read_batch_t* batch,
                    msw_out_t* out, uint64_t chunk_pairs);
/* Same, asynchronous (completes with msw_wait; host arrays must stay alive). */
int msw_align_reads_async(msw_ctx* ctx, const msw_scoring_t* sc, const msw_genome* g,
                          const msw_read_batch_t* batch, msw_out_t* out, uint64_t chunk_pairs, uint64_t* ticket);

/* Device-resident reads against genome windows (the GPU lane reader's
 * batches, msw_gfastq_next): read p = reads[p * read_stride ..][0,
 * read_len[p]) scores against genome[win_pos[p], win_pos[p] + W), W = window,
 * or 2 x read_len[p] when window is 0 (the CLI's --window rule), capped at
 * 4096 and clipped at the genome end.  Windows are cut into a context scratch
 * slab on the GPU; everything is enqueued on `stream` (NULL = the context's
 * compute stream), no host synchronisation.  All arrays are device memory;
 * win_len_out (may be NULL) receives the clipped window lengths.
 * max_read_len bounds read_len (it selects the kernel instance). */
int msw_align_reads_device(msw_ctx* ctx, const msw_scoring_t* sc, const msw_genome* g, const uint8_t* reads,
                           const uint16_t* read_len, uint32_t read_stride, const int64_t* win_pos, uint64_t n,
                           uint32_t window, uint32_t max_read_len, msw_out_t* out, uint16_t* win_len_out,
                           void* stream);

/* The window of a pair in the device-resident genome calls
 * (msw_align_reads_device, msw_trace_reads_device): window p is
 * genome[win_pos[p], win_pos[p] + W), W = `window`, or 2 x read_len[p] capped
 * at 4096 when `window` is 0, clipped at the genome end; win_pos[p] < 0 or
 * >= the genome length is an empty window.
 *
 * Traceback straight from the genome: arguments and windows are those of
 * msw_align_reads_device, `ends` is what that call wrote with want_coords = 1
 * for the same arguments, and `tr` is filled as by msw_trace_batch_device
 * (overflow contract included; start_j and end_j are window-relative).  The
 * windows are read from the genome itself: the call needs no cut slab and
 * nothing an earlier call left behind.  Range as for traceback:
 * max_read_len <= 384 and the window bound (window, or 2 x max_read_len capped
 * at 4096) <= 4096, else MSW_E_RANGE.  Enqueued on `stream`, no host
 * synchronisation. */
int msw_trace_reads_device(msw_ctx* ctx, const msw_scoring_t* sc, const msw_genome* g, const uint8_t* reads,
                           const uint16_t* read_len, uint32_t read_stride, const int64_t* win_pos, uint64_t n,
                           uint32_t window, uint32_t max_read_len, const msw_out_t* ends, msw_trace_t* tr,
                           void* stream);

/* Alignment records: what a consumer of alignments needs beside the trace,
 * and the CIGARs packed into one stream instead of [n][cigar_stride] rows.
 * Per read with score > 0 whose trace did not overflow:
 *  - ops: S start_i when start_i > 0, the traced ops, S (read_len - 1 - end_i)
 *    when that is > 0, so a packed CIGAR consumes exactly read_len read bases;
 *  - nm (SAM's NM): the I lengths plus the D lengths plus the M columns whose
 *    read byte differs from the genome byte (byte equality, as the scorer),
 *    walking the ops from (start_i, ref_pos).
 * Score 0 or an empty pair: ref_pos -1, nm 0, no ops.  A read whose trace
 * overflowed (n_cigar > cigar_stride): nm -1, no ops, counted in n_overflow;
 * its ref_pos is valid.  When the total exceeds cigar_cap, cigar_off is still
 * complete and nothing is written at or past cigar + cigar_cap. */
typedef struct {
    int64_t*  ref_pos;    /* [n]   genome coordinate of the first aligned base = win_pos + start_j; -1 when score == 0 */
    int32_t*  nm;         /* [n]   edit distance; 0 when score == 0; -1 when the read's trace overflowed */
    uint32_t* cigar_off;  /* [n+1] exclusive prefix sum of ops per read, soft clips included; [n] = total */
    uint32_t* cigar;      /* packed ops, len << 4 | op, M=0 I=1 D=2 S=4 (BAM codes) */
    uint64_t  cigar_cap;  /* ops `cigar` holds */
    uint32_t* n_overflow; /* [1] reads with n_cigar > cigar_stride in the trace: they contribute 0 ops */
} msw_aln_t;

/* Device-resident: every array is device memory; `ends` and `tr` are the
 * scoring and trace results of these reads (n <= 2^31 - 1).  Enqueued on
 * `stream` with no host synchronisation; temporaries are stream-ordered. */
int msw_aln_pack_device(msw_ctx* ctx, const msw_genome* g, const uint8_t* reads, const uint16_t* read_len,
                        uint32_t read_stride, const int64_t* win_pos, uint64_t n, const msw_out_t* ends,
                        const msw_trace_t* tr, msw_aln_t* aln, void* stream);

/* Host memory, synchronous (like msw_align_batch_trace): scores batch (as
 * msw_align_reads, coordinates forced), traces and packs, in chunks of
 * `chunk_pairs` (0 = 65536); cigar_off is one prefix sum over the whole
 * batch.  The trace stride used inside is exact, so *n_overflow is 0.  A
 * cigar_cap below cigar_off[n] still returns MSW_OK with cigar_off complete;
 * `cigar` is then unspecified.  Reads <= 384, requested windows <= 4096. */
int msw_align_reads_trace(msw_ctx* ctx, const msw_scoring_t* sc, const msw_genome* g, const msw_read_batch_t* batch,
                          msw_out_t* out, msw_aln_t* aln, uint64_t chunk_pairs);

/* Both strands.
 *
 * Reverse complement of a read of length L: rc[k] = comp(read[L-1-k]), where
 * comp maps A<->T, C<->G, a<->t, c<->g and leaves every other byte value as
 * it is ('N' included): the scorer compares bytes, so comp is defined on bytes.
 *
 * Both-strand scoring of read p against its window: score_f is the result
 * for the read as given, score_r the result for rc(read) against the same
 * window; strand[p] = 1 exactly when score_r > score_f, else 0 (ties go to
 * the forward strand, 0 == 0 and empty reads and windows included).  The
 * reported score and end cell are the winner's.  end_i, the later start_i and
 * the CIGAR are in the coordinates of the ORIENTED read: the read itself for
 * strand 0, its reverse complement for strand 1.  end_j, start_j and ref_pos
 * are window and genome coordinates as in the one-strand calls, so for strand
 * 1 ref_pos is still the leftmost genome base of the alignment and the CIGAR
 * runs left to right along the genome (what SAM stores with flag 0x10).
 *
 * Oriented slab: row p of oriented[n][oriented_stride] holds the oriented
 * read in bytes [0, read_len[p]) and zeros up to the stride;
 * msw_trace_reads_device and msw_aln_pack_device then run unchanged with
 * `oriented` / oriented_stride in place of reads / read_stride. */

/* out[p * out_stride ..] = rc(reads[p * read_stride ..][0, read_len[p])),
 * zeros up to out_stride (every byte of every output row is written).  Device
 * arrays; the read rows at any alignment and any stride >= the longest read;
 * `out` 16-byte aligned and out_stride a non-zero multiple of 16, else
 * MSW_E_INVALID.  Enqueued on `stream`, no host synchronisation. */
int msw_revcomp_device(msw_ctx* ctx, const uint8_t* reads, const uint16_t* read_len, uint32_t read_stride,
                       uint64_t n, uint8_t* out, uint32_t out_stride, void* stream);

/* msw_align_reads_device on both strands: same arguments, window rule and
 * errors; strand is u8[n], oriented the slab above (16-byte aligned,
 * oriented_stride a multiple of 16 and >= max_read_len, else MSW_E_INVALID,
 * as for a NULL strand or oriented).  On the one stream: one window cut shared
 * by both orientations, the reverse complements, forward scoring into `out`,
 * reverse scoring into scratch the context keeps per stream, the choice.  With
 * want_coords = 0, end_i / end_j may be NULL. */
int msw_align_reads_strands_device(msw_ctx* ctx, const msw_scoring_t* sc, const msw_genome* g, const uint8_t* reads,
                                   const uint16_t* read_len, uint32_t read_stride, const int64_t* win_pos, uint64_t n,
                                   uint32_t window, uint32_t max_read_len, msw_out_t* out, uint16_t* win_len_out,
                                   uint8_t* strand, uint8_t* oriented, uint32_t oriented_stride, void* stream);

/* Host memory, synchronous, chunked like msw_align_reads_trace (requested
 * window lengths from batch->win_len); strand is u8[n_pairs].  aln == NULL:
 * scores only, coordinates as sc says.  With aln: coordinates are forced, the
 * oriented rows are traced at the exact stride and packed; ranges and
 * MSW_E_RANGE as for msw_align_reads_trace. */
int msw_align_reads_strands(msw_ctx* ctx, const msw_scoring_t* sc, const msw_genome* g, const msw_read_batch_t* batch,
                            msw_out_t* out, uint8_t* strand, msw_aln_t* aln, uint64_t chunk_pairs);

/* Placing reads: a k-mer index of the resident genome and seed voting.
 *
 * Everything is defined on bytes and integers, so a plain restatement
 * (tests/seed_oracle.py) can be compared value for value.
 *
 * k-mers.  Codes are A 0, C 1, G 2, T 3, upper case only (the scorer compares
 * bytes).  A k-mer that contains any other byte has no code and is skipped.
 * The code of s[i .. i+k) is the base-4 number with s[i] most significant.
 * 4 <= k <= 14.
 *
 * Index over a genome g of length n (n <= 0xFFFF0000, else MSW_E_RANGE:
 * positions are u32 and diagonals are stored biased by 65536).  cnt[c] is the
 * number of positions p in [0, n-k] whose k-mer has code c.  A bucket with
 * cnt[c] > max_occ is masked: it is stored as empty (1 <= max_occ <= 64).
 * off u32[4^k + 1] is the exclusive prefix sum of the masked counts, and
 * pos u32[off[4^k]] holds each bucket's positions in ascending order, so the
 * index is bit-reproducible whatever order the build's atomics ran in.
 *
 * Seeding one orientation of one read r of length L, with band >= 1, cap in
 * [1, 8192] and step >= 1:
 *  1. for each offset i in [0, L-k] with i % step == 0 and a coded k-mer, c_i
 *     is the size of its bucket; otherwise c_i = 0;
 *  2. P_i = the sum of c_j over j <= i; offset i contributes its c_i hits iff
 *     P_i <= cap; the read is truncated iff the last P exceeds cap;
 *  3. every contributing hit (i, p) gives a diagonal d = p - i, signed (it is
 *     negative where a read overhangs the genome start);
 *  4. for each d0 in the multiset D of diagonals, score(d0) is the number of
 *     d in D with d0 <= d < d0 + band;
 *  5. the seed is the d0 of maximal score, the smallest such d0 on ties;
 *     votes is that score and hits is |D|;
 *  6. no diagonal at all (L < k, no coded k-mer, every bucket empty or
 *     masked) gives votes = 0.
 *
 * Orientation.  With a reverse-complement slab (rows as msw_revcomp_device
 * writes them) both orientations are seeded, and the reverse one is chosen
 * iff its votes is strictly greater: a tie goes to forward, as in the strand
 * rule above.  Without the slab the orientation is forward.
 *
 * Placement.  W is the window rule of the device-resident genome calls
 * (`window`, or 2 x L capped at 4096 when `window` is 0);
 * pad = max(0, (W - (L + band - 1)) / 2); win_pos = max(0, d0 - pad); and
 * win_pos = -1 when votes < min_votes (min_votes >= 1): the existing "empty
 * window, score 0" case, so nothing downstream needs a new rule.
 *
 * Composition.  win_pos feeds the reads-against-genome calls unchanged.
 * msw_align_reads_strands_device scores both orientations against the seeded
 * window and the right one wins there by score: bit 0 of flags is a hint, not
 * the record's strand. */
typedef struct msw_index msw_index;
typedef struct {
    uint32_t k;
    uint32_t max_occ;
    uint64_t n_buckets;       /* 4^k */
    uint64_t n_pos;           /* stored positions = off[4^k] */
    uint64_t n_masked;        /* buckets over max_occ */
    const uint32_t* off;      /* device, [n_buckets + 1]; read-only, for tests and tools */
    const uint32_t* pos;      /* device, [n_pos] */
    double build_ms[5];       /* GPU time of the count, mask, scan, fill and sort passes */
} msw_index_info_t;

/* Builds the index of `genome` on the GPU, synchronously.  An index belongs
 * to the context of its genome; it keeps nothing of the genome itself, and is
 * destroyed before that context. */
int msw_index_create(msw_ctx* ctx, const msw_genome* genome, uint32_t k, uint32_t max_occ, msw_index** out);
void msw_index_destroy(msw_index* idx);
int msw_index_info(const msw_index* idx, msw_index_info_t* out);

typedef struct {
    uint32_t band;
    uint32_t cap;
    uint32_t step;
    uint32_t min_votes;
    uint32_t window;          /* the `window` argument the scoring call will get */
} msw_seed_params_t;

/* Per read: the placement, the chosen orientation's votes and hits, and
 * flags: bit 0 the reverse orientation was chosen, bit 1 the chosen
 * orientation was truncated. */
typedef struct {
    int64_t*  win_pos;
    uint32_t* votes;
    uint32_t* hits;
    uint8_t*  flags;
} msw_seed_out_t;

/* Device-resident: every array is device memory; rc_reads (may be NULL:
 * forward only) holds the reverse complements in rows of rc_stride bytes.
 * Rows at any alignment and stride >= max_read_len (else MSW_E_INVALID);
 * max_read_len <= 32767 and window <= 32767, band / cap / step / min_votes as
 * above, else MSW_E_RANGE.  Enqueued on `stream` (NULL = the context's compute
 * stream) with no host synchronisation; n = 0 launches nothing. */
int msw_seed_reads_device(msw_ctx* ctx, const msw_index* idx, const uint8_t* reads, const uint8_t* rc_reads,
                          const uint16_t* read_len, uint32_t read_stride, uint32_t rc_stride, uint64_t n,
                          uint32_t max_read_len, const msw_seed_params_t* params, const msw_seed_out_t* out,
                          void* stream);

/* Host memory, synchronous, in chunks of `chunk_reads` (0 = 65536): per chunk
 * it uploads the rows, makes the reverse complements on the GPU when `both`
 * is non-zero, seeds and downloads.  batch->win_pos and batch->win_len are
 * not read. */
int msw_seed_reads(msw_ctx* ctx, const msw_index* idx, const msw_read_batch_t* batch, int both,
                   const msw_seed_params_t* params, const msw_seed_out_t* out, uint64_t chunk_reads);

/* Candidates and mapping quality.
 *
 * Defined on integers, like "Placing reads" (tests/mapq_oracle.py restates
 * it).  A read gets up to two candidate loci; both are scored, the better one
 * becomes the read's record, and the other one's score is the sub-optimal
 * score that the mapping quality is made of.
 *
 * Per orientation.  D is the multiset of contributing diagonals and (d1, v1)
 * the seed of "Placing reads".  With sep >= band, a diagonal e is admissible
 * against d iff |e - d| >= sep.  The orientation's second band (d2, v2) is the
 * seed rule (steps 4-6) applied to the subset of D admissible against d1; no
 * admissible diagonal gives v2 = 0.
 *
 * Per read.  Candidate 0 is exactly what msw_seed_reads_device reports: the
 * same orientation rule, win_pos, votes, hits and flags, bit for bit; d0 is
 * its diagonal.  Candidate 1 is chosen among the other bands, up to three: the
 * chosen orientation's second band, and the other orientation's first and
 * second bands.  A band is eligible iff its votes >= min_votes and its
 * diagonal is admissible against d0.  The most votes win; on a tie the forward
 * orientation goes before the reverse one, then the smaller diagonal.  No
 * eligible band (candidate 0 without a diagonal included) gives win_pos1 = -1,
 * votes1 = 0, flags1 = 0.  win_pos1 follows the placement formula of "Placing
 * reads".  sep = 0 means max(W, band), W the window rule's length for that
 * read; a sep that is neither 0 nor >= band is MSW_E_RANGE.
 *
 * This is NOT the globally second-best band over both orientations: a band
 * that is third in its own orientation is never seen, and the other
 * orientation's second band is the one admissible against that orientation's
 * own first band, which is then tested against d0.  The rule is what one pass
 * over each orientation's sorted diagonals can give without a second key array
 * or a re-expansion of the first orientation.
 *
 * Selection.  s_p and s_a are the scores of candidates 0 and 1 (the both-strand
 * score where both strands are scored; an empty window scores 0).  The
 * alternate wins iff s_a > s_p; ties keep candidate 0.  The winner's score,
 * end cell, win_len, strand, oriented row and win_pos become the read's;
 * sub_score is the loser's score and cand is 0 or 1.
 *
 * Mapping quality, with s1 the winner's score and L the read length:
 * mapq = 0 when s1 <= 0 or match * L == 0; otherwise
 * mapq = min(60, 120 * (s1 - s2) / (match * L)), floor division in 64-bit
 * integers, s2 = clamp(sub_score, 0, s1).  This is an uncalibrated heuristic:
 * a monotone function of the score gap per best-possible score, not a
 * probability, and not comparable with another mapper's MAPQ. */
typedef struct {
    int64_t*  win_pos;        /* [n] candidate 1's window position, -1: none */
    uint32_t* votes;          /* [n] its votes, 0: none */
    uint8_t*  flags;          /* [n] bit 0: it comes from the reverse orientation */
} msw_seed_alt_t;

/* msw_seed_reads_device with the second candidate: the same arguments, checks
 * and errors; `out` is written as that call writes it.  Enqueued on `stream`,
 * no host synchronisation. */
int msw_seed_candidates_device(msw_ctx* ctx, const msw_index* idx, const uint8_t* reads, const uint8_t* rc_reads,
                               const uint16_t* read_len, uint32_t read_stride, uint32_t rc_stride, uint64_t n,
                               uint32_t max_read_len, const msw_seed_params_t* params, uint32_t sep,
                               const msw_seed_out_t* out, const msw_seed_alt_t* alt, void* stream);

/* Host memory, synchronous, chunked like msw_seed_reads. */
int msw_seed_candidates(msw_ctx* ctx, const msw_index* idx, const msw_read_batch_t* batch, int both,
                        const msw_seed_params_t* params, uint32_t sep, const msw_seed_out_t* out,
                        const msw_seed_alt_t* alt, uint64_t chunk_reads);

/* One candidate's scoring results, device arrays of n.  end_i / end_j NULL
 * (in both candidates): scores only.  strand / oriented NULL (in both): one
 * strand, no rows.  win_len NULL (in both): not moved. */
typedef struct {
    int32_t*  score;
    int16_t*  end_i;
    int16_t*  end_j;
    uint16_t* win_len;
    uint8_t*  strand;
    uint8_t*  oriented;       /* [n][oriented_stride], as msw_align_reads_strands_device writes it */
    int64_t*  win_pos;
} msw_cand_t;

/* The selection above, in place: where the alternate wins its results and its
 * oriented row (zero padding included) replace the primary's; elsewhere the
 * primary's arrays are not written and the alternate's row is not read.
 * sub_score i32[n], mapq u8[n], cand u8[n] are written for every read.  With
 * rows: both slabs 16-byte aligned and oriented_stride a non-zero multiple of
 * 16, else MSW_E_INVALID; match outside [0, 64] is MSW_E_RANGE.  Enqueued on
 * `stream`, no host synchronisation. */
int msw_mapq_select_device(msw_ctx* ctx, const msw_cand_t* primary, const msw_cand_t* alt, uint32_t oriented_stride,
                           const uint16_t* read_len, uint64_t n, int32_t match, int32_t* sub_score, uint8_t* mapq,
                           uint8_t* cand, void* stream);

typedef struct {
    uint8_t* mapq;            /* [n] */
    int32_t* sub_score;       /* [n] */
    uint8_t* cand;            /* [n] 0: candidate 0 is the record's locus, 1: candidate 1 */
} msw_mapq_t;

/* Host memory, synchronous, in chunks of `chunk_pairs` (0 = 65536): per chunk
 * the candidates, the scoring of both (msw_align_reads_strands_device twice
 * when `both` is non-zero, else msw_align_reads_device twice), the selection,
 * then the trace and the pack of the winner's rows at the winner's positions.
 * batch->win_pos and batch->win_len are not read: the window is
 * params->window.  out, strand (required when `both`, else may be NULL) and
 * aln (required) are filled as by msw_align_reads_strands; ranges and
 * MSW_E_RANGE as for msw_align_reads_trace. */
int msw_map_reads(msw_ctx* ctx, const msw_scoring_t* sc, const msw_genome* g, const msw_index* idx,
                  const msw_read_batch_t* batch, int both, const msw_seed_params_t* params, uint32_t sep,
                  msw_out_t* out, uint8_t* strand, msw_aln_t* aln, const msw_mapq_t* mq, uint64_t chunk_pairs);

/* Pileup: per genome base, what the reads aligned over it show.
 *
 * Everything is integers and bytes, so a plain restatement
 * (tests/pileup_oracle.py) can be compared value for value.
 *
 * Counts.  counts[glen][8], uint32, one row per genome base:
 *   0..3  the aligned read byte is A, C, G, T (upper case only: the k-mer
 *         codes of "Placing reads")
 *   4     the aligned read byte is anything else (N, lower case, 0)
 *   5     the base is deleted in the read (a column of a D run)
 *   6     an I run follows this base: +1 per run, at g - 1, g being the genome
 *         coordinate at which the walk stands when it meets the run
 *   7     the columns of M runs that come from strand-1 reads (a subset of 0..4)
 * depth(pos) is the sum of channels 0..5.
 *
 * Which reads count.  Read p of a batch counts when ref_pos[p] >= 0,
 * nm[p] >= 0 (an overflowed trace has no ops), cigar_off[p + 1] > cigar_off[p]
 * and, where a mapq array is given, mapq[p] >= min_mapq.  In the device form a
 * read whose ops end past aln->cigar_cap does not count either.  A read that
 * counts adds 1 to reads_used, every other read 1 to reads_skipped.
 *
 * The walk.  i = 0 and g = ref_pos[p]; the packed ops
 * cigar[cigar_off[p] .. cigar_off[p + 1]) in order:
 *   S len  i += len;
 *   M len  column k of [0, len) counts when 0 <= g + k < glen and
 *          i + k < read_len[p]: its channel is the code of rows[p][i + k], and
 *          channel 7 gets +1 too when strand != NULL and strand[p] != 0; then
 *          i += len, g += len;
 *   I len  channel 6 at g - 1 when 0 <= g - 1 < glen; then i += len;
 *   D len  channel 5 at g + k for the k of [0, len) with 0 <= g + k < glen;
 *          then g += len;
 *   any other op code is skipped without effect.
 * rows are the rows the CIGARs refer to: the oriented slab after a both-strands
 * call, the reads themselves otherwise.  The column rules make every access
 * in-bounds for any records (read_len[p] <= row_stride is the caller's), not
 * only for what msw_aln_pack_device wrote.
 *
 * Summary of finished counts for a min_depth >= 1: covered = the positions
 * with depth > 0; depth_sum; max_depth; minority_ref = the positions with
 * depth >= min_depth and 2 * counts[pos][code(genome[pos])] < depth (the code
 * of a genome byte that is not upper-case ACGT is 4).
 *
 * Base qualities (msw_pileup_add_qual[_device]).  quals[n][qual_stride] holds
 * one byte per base, and its rows are always in the order of the file: byte t
 * of row p belongs to base t of read p AS GIVEN, in both add forms.  The Phred
 * value of a byte b is b >= 33 ? b - 33 : 0.  Column k of an M run stands at
 * read offset i + k of the row the CIGAR refers to; its quality index is
 * t = i + k for a strand-0 read (or strand == NULL) and
 * t = read_len[p] - 1 - (i + k) for a strand-1 read, whether `rows` is the
 * oriented slab (device form) or the reads as given (host form).  A column
 * that passes the range rules of the walk counts only if t < qual_stride and
 * phred(quals[p][t]) >= min_baseq.  One that passes the range rules and fails
 * this test adds to no channel, neither 0..4 nor 7, and adds 1 to the
 * pileup's low-quality column count (msw_pileup_lowq_columns).  D runs, I
 * runs, reads_used and reads_skipped are as without qualities.
 * min_baseq == 0 or quals == NULL is exactly msw_pileup_add[_device];
 * min_baseq > 93 is MSW_E_RANGE.
 *
 * The result is a function of the set of records (with qualities and
 * threshold, where given) alone: it is bit-reproducible whatever order the
 * batches and the GPU's atomics ran in.
 *
 * State: about 44 bytes of device memory per genome base (the 32-byte row, two
 * 4-byte difference arrays and a 4-byte mismatch count), so
 * 176 MB for a 4 Mbase genome; a MSW_PILEUP_QSUM pileup ("Quality sums and
 * weighted genotypes" below) holds 24 bytes per base more, about 68 in all and
 * 272 MB for 4 Mbase.  A pileup belongs to the context of its genome and is
 * destroyed before it. */
typedef struct msw_pileup msw_pileup;
typedef struct {
    uint64_t covered;
    uint64_t depth_sum;
    uint64_t minority_ref;
    uint64_t reads_used;
    uint64_t reads_skipped;
    uint32_t max_depth;
    uint32_t reserved;
} msw_pileup_summary_t;

/* An empty pileup over `genome` (the state is zeroed); synchronous.
 * MSW_E_NOMEM when the state cannot be allocated. */
int msw_pileup_create(msw_ctx* ctx, const msw_genome* genome, msw_pileup** out);
void msw_pileup_destroy(msw_pileup* pile);

/* Adds the records of n reads.  Device arrays: rows[n][row_stride] with
 * read_len as above, aln->ref_pos / nm / cigar_off / cigar / cigar_cap as
 * msw_aln_pack_device wrote them (aln->n_overflow is not read); strand and
 * mapq may be NULL.  Enqueued on `stream` (NULL = the context's compute
 * stream), no host synchronisation; adds on several streams may run at once.
 * n > 2^31 - 1 is MSW_E_RANGE, min_mapq > 255 too; after msw_pileup_finish
 * MSW_E_INVALID. */
int msw_pileup_add_device(msw_ctx* ctx, msw_pileup* pile, const uint8_t* rows, const uint16_t* read_len,
                          uint32_t row_stride, uint64_t n, const msw_aln_t* aln, const uint8_t* strand,
                          const uint8_t* mapq, uint32_t min_mapq, void* stream);

/* The same from host memory, synchronous, in chunks of `chunk_reads` (0 =
 * 65536).  `reads` are the reads AS GIVEN to msw_align_reads_strands or
 * msw_map_reads, and `strand` the bytes that call returned: the reverse
 * complement of a strand-1 read is taken on the GPU.  With strand == NULL the
 * rows are what the CIGARs refer to, as in the device form.  aln->cigar_off
 * must not decrease and the ops of every read must lie inside aln->cigar_cap,
 * else MSW_E_INVALID. */
int msw_pileup_add(msw_ctx* ctx, msw_pileup* pile, const uint8_t* reads, const uint16_t* read_len,
                   uint32_t read_stride, uint64_t n, const msw_aln_t* aln, const uint8_t* strand,
                   const uint8_t* mapq, uint32_t min_mapq, uint64_t chunk_reads);

/* Both adds with the base-quality threshold of "Base qualities" above.  quals
 * is device memory in the device form (e.g. msw_gfastq_quals, msw_fastq.h) and
 * host memory in the host form; a quality path of its own runs only when
 * quals != NULL and min_baseq > 0, otherwise these are the calls above (a
 * MSW_PILEUP_QSUM pileup has rules of its own: "Quality sums and weighted
 * genotypes" below). */
int msw_pileup_add_qual_device(msw_ctx* ctx, msw_pileup* pile, const uint8_t* rows, const uint16_t* read_len,
                               uint32_t row_stride, uint64_t n, const msw_aln_t* aln, const uint8_t* strand,
                               const uint8_t* mapq, uint32_t min_mapq, const uint8_t* quals, uint32_t qual_stride,
                               uint32_t min_baseq, void* stream);
int msw_pileup_add_qual(msw_ctx* ctx, msw_pileup* pile, const uint8_t* reads, const uint16_t* read_len,
                        uint32_t read_stride, uint64_t n, const msw_aln_t* aln, const uint8_t* strand,
                        const uint8_t* mapq, uint32_t min_mapq, const uint8_t* quals, uint32_t qual_stride,
                        uint32_t min_baseq, uint64_t chunk_reads);
/* The M columns dropped by the threshold so far; synchronous (it waits for the
 * device), valid before or after msw_pileup_finish. */
int msw_pileup_lowq_columns(msw_ctx* ctx, msw_pileup* pile, uint64_t* out);

/* Folds the state into the counts, once, enqueued on `stream`: every add must
 * have been enqueued on that stream or have finished.  Afterwards both add
 * forms return MSW_E_INVALID; a second finish is a no-op. */
int msw_pileup_finish(msw_ctx* ctx, msw_pileup* pile, void* stream);

/* The finished counts into host_out[glen][8]; synchronous (it waits for the
 * finish).  Before msw_pileup_finish: MSW_E_INVALID. */
int msw_pileup_counts(msw_ctx* ctx, msw_pileup* pile, uint32_t* host_out);
/* The counts on the device: channel ch of position pos is
 * (*counts)[pos * *pos_stride + ch * *ch_stride] (rows of eight: 8 and 1).
 * Valid at any time; the values are final once the finish has run. */
int msw_pileup_counts_device(msw_ctx* ctx, msw_pileup* pile, const uint32_t** counts, uint64_t* pos_stride,
                             uint64_t* ch_stride);
/* The summary above, computed on the GPU; synchronous, only after
 * msw_pileup_finish (else MSW_E_INVALID); min_depth == 0 is MSW_E_INVALID. */
int msw_pileup_summary(msw_ctx* ctx, msw_pileup* pile, uint32_t min_depth, msw_pileup_summary_t* out);

/* Variants: the sites of finished pileup counts at which the sample differs
 * from the genome, with a genotype.
 *
 * Everything is integers, so a plain restatement (tests/variant_oracle.py) can
 * be compared value for value, and the result is a function of the counts, the
 * genome bytes and the parameters alone.
 *
 * Input.  Finished counts c[glen][8] (the channels of "Pileup") and the genome
 * bytes.  code() is the pileup's: A 0, C 1, G 2, T 3, anything else 4.
 * depth(pos) is the sum of channels 0..5 as a 64-bit value; depth(glen) is 0.
 *
 * Site kinds.  A position yields at most two records, the column record first.
 *   Column (MSW_VAR_SNV 0, MSW_VAR_DEL 1), only where r = code(genome[pos]) < 4:
 *     n = c[0] + c[1] + c[2] + c[3] + c[5] (channel 4 says nothing), ref = c[r];
 *     the alternative is the channel of {0, 1, 2, 3} \ {r} + {5} with the highest
 *     count, the lowest channel index on a tie, and a is its count.  Channel 5
 *     makes the record a DEL (alt 0), any other an SNV with alt the base letter.
 *   Insertion (MSW_VAR_INS 2), for any genome byte: a = c[6],
 *     span = min(depth(pos), depth(pos + 1)), ref = span > a ? span - a : 0,
 *     n = ref + a.  The inserted sequence is not in the pileup: alt is 0.
 *   The record's depth is n, its ref_count ref, its alt_count a.
 *
 * Candidate.  n >= min_depth, a >= min_alt and
 * 1000 * a >= min_alt_permille * n, all in 64 bits.
 *
 * Genotypes.  g: 0 = 0/0, 1 = 0/1, 2 = 1/1; all u64.
 *   raw[0] = ref * q_hit + a * q_miss
 *   raw[1] = (ref + a) * q_het
 *   raw[2] = ref * q_miss + a * q_hit
 *   (third alleles cost the same under every genotype and are left out)
 *   post = raw + {0, prior_het, prior_hom}
 *   gt = argmin post, the lowest g on a tie
 *   pl[g] = min((raw[g] - min raw + 50) / 100, 2^32 - 1)
 *   qual  = min((post[0] - min post + 50) / 100, 2^32 - 1)
 *   gq    = min(99, (second smallest post - smallest post + 50) / 100)
 *
 * Emission.  A candidate with gt != 0 and qual >= min_qual becomes a record.
 * Records are ordered by pos, then kind.
 *
 * The costs are -1000 * log10(p) for an error rate e = 0.01: q_hit for an
 * observation of a homozygous genotype's allele (p = 1 - e), q_miss for one of
 * the other allele (p = e / 3), q_het for either allele of a heterozygote
 * (p = (1 - e) / 2 + e / 6); the priors are in the same unit. */
#define MSW_VAR_SNV 0
#define MSW_VAR_DEL 1
#define MSW_VAR_INS 2
typedef struct {
    uint32_t min_depth;        /* 4 */
    uint32_t min_alt;          /* 2 */
    uint32_t min_alt_permille; /* 200 */
    uint32_t min_qual;         /* 20 */
    uint32_t q_hit;            /* 4 */
    uint32_t q_miss;           /* 2477 */
    uint32_t q_het;            /* 304 */
    uint32_t prior_het;        /* 3000 */
    uint32_t prior_hom;        /* 3301 */
} msw_call_params_t;
/* One record, 48 bytes, the same bytes in memory and in the .var file
 * (little-endian). */
typedef struct {
    uint64_t pos;
    uint32_t depth;      /* n, saturated at 2^32 - 1 */
    uint32_t ref_count;  /* ref, saturated */
    uint32_t alt_count;  /* a, saturated */
    uint32_t qual;
    uint32_t pl[3];
    uint8_t kind;        /* MSW_VAR_* */
    uint8_t ref;         /* the genome byte */
    uint8_t alt;         /* SNV: 'A', 'C', 'G' or 'T'; else 0 */
    uint8_t gt;          /* 1 = 0/1, 2 = 1/1 */
    uint8_t gq;
    uint8_t pad[7];      /* zeros */
} msw_variant_t;

/* Fills *params with the defaults noted beside the fields. */
void msw_call_params_default(msw_call_params_t* params);

/* In every call below: params == NULL selects the defaults; a q_* above 65535,
 * min_depth == 0 or min_alt_permille above 1000 is MSW_E_INVALID.  Records
 * past `cap` are not written; the total is always reported.
 *
 * Calls on a finished pileup's own counts and genome, enqueued on `stream`
 * (NULL = the context's compute stream, behind the finish), no host
 * synchronisation: out_dev[cap] records and *n_total_dev (u64) are device
 * memory.  out_dev == NULL with cap == 0 runs the count pass alone.  Before
 * msw_pileup_finish: MSW_E_INVALID.  A genome above 2^31 - 1 bases is
 * MSW_E_RANGE (a call's record offsets are 32 bits: at most two per base). */
int msw_pileup_call_device(msw_ctx* ctx, msw_pileup* pile, const msw_call_params_t* params, msw_variant_t* out_dev,
                           uint64_t cap, uint64_t* n_total_dev, void* stream);
/* The same into host memory, synchronous.  out_host == NULL with cap == 0 runs
 * the count pass alone and returns the total. */
int msw_pileup_call(msw_ctx* ctx, msw_pileup* pile, const msw_call_params_t* params, msw_variant_t* out_host,
                    uint64_t cap, uint64_t* n_total);
/* Calls on any host counts_host[glen][8] over genome_host[glen], for example
 * the sum of several pileups; synchronous.  The rows go through a bounded
 * device buffer in chunks of chunk_pos positions (0 = 2^20; above 2^24 is
 * MSW_E_RANGE), each chunk with one row of look-ahead for depth(pos + 1):
 * record order and totals do not depend on chunk_pos.  glen and the total are
 * 64-bit and have no other limit. */
int msw_call_counts(msw_ctx* ctx, const uint8_t* genome_host, uint64_t glen, const uint32_t* counts_host,
                    const msw_call_params_t* params, uint64_t chunk_pos, msw_variant_t* out_host, uint64_t cap,
                    uint64_t* n_total);

/* Quality sums and weighted genotypes: per base and allele the summed Phred
 * values of the observations, and a caller that charges an observation by its
 * own error rate instead of one fixed rate.
 *
 * Integers throughout; tests/pileup_qsum_oracle.py and
 * tests/variant_qual_oracle.py restate this section.
 *
 * Quality sums.  A pileup created with msw_pileup_create_ex(ctx, genome,
 * MSW_PILEUP_QSUM, &out) carries qsum[glen][4], uint32, beside its counts.
 * qsum[pos][c] is the sum of phred(quals[p][t]) over the M columns that count
 * at pos and whose read byte has code c < 4.  "Count" is the walk, the range
 * rules and the min_baseq rule of "Base qualities" above, unchanged, with the
 * same quality index t and the same t < qual_stride rule: a column adds to
 * qsum exactly when it adds to channel c < 4 of the counts.  A dropped column,
 * or one whose read byte has code 4, adds nothing; D and I runs add nothing.
 * Sums are modulo 2^32, like the counts.  The result is a function of the set
 * of records, qualities and threshold alone.
 *
 * Calls on a MSW_PILEUP_QSUM pileup.  msw_pileup_add_qual[_device] needs
 * quals != NULL (else MSW_E_INVALID, for any n) and accepts min_baseq == 0:
 * the quality path runs, because the sums need it, and then a column counts
 * when t < qual_stride.  msw_pileup_add[_device] returns MSW_E_INVALID.
 * msw_pileup_create_ex with flags 0 is msw_pileup_create; an unknown flag is
 * MSW_E_INVALID.  On a pileup without the flag every call of "Pileup" behaves
 * exactly as described there.
 *
 * Weighted genotypes.  Site kinds, candidate rule, choice of the alternative
 * (the highest count), emission, pl, qual, gq, record layout and order are
 * those of "Variants".  Only raw[] of a COLUMN site changes.  With
 * r = code(genome[pos]), alt_ch the alternative's channel, all values u64:
 *   Wref = q_scale * qsum[pos][r] + q_third * ref
 *   Walt = alt_ch < 4 ? q_scale * qsum[pos][alt_ch] + q_third * a
 *                     : a * q_miss          (a DEL has no base quality)
 *   raw[0] = ref * q_hit + Walt
 *   raw[1] = (ref + a) * q_het
 *   raw[2] = Wref + a * q_hit
 * Insertion sites keep the formula of "Variants".  The cost of an observation
 * with Phred value Q under the other homozygote is
 * -1000 * log10(10^(-Q/10) / 3) = 100 * Q + 477; at Q20 that is the 2477 of
 * q_miss, so with every counted base at Phred 20 and the default weights the
 * records are those of "Variants".  q_hit and q_het stay fixed: they depend
 * on e too, but for Q20 and better -1000 * log10(1 - e) lies between 0 and 4
 * and -1000 * log10((1 - e) / 2 + e / 6) between 301 and 304, so the fixed
 * values are off by a few units per read (what decides a genotype,
 * q_het - q_hit, by under 3), against the hundreds to thousands per read of
 * the weighted term.
 *
 * State: the flag adds 24 bytes of device memory per genome base (16 for
 * qsum, a 4-byte difference array and a 4-byte sum over mismatching columns),
 * allocated only with the flag: about 68 bytes per base, 272 MB for a 4 Mbase
 * genome. */
#define MSW_PILEUP_QSUM 1u
typedef struct {
    uint32_t q_scale; /* 100 */
    uint32_t q_third; /* 477 */
} msw_call_qparams_t;
/* Fills *qparams with the defaults noted beside the fields. */
void msw_call_qparams_default(msw_call_qparams_t* qparams);

/* msw_pileup_create with flags: 0 or MSW_PILEUP_QSUM. */
int msw_pileup_create_ex(msw_ctx* ctx, const msw_genome* genome, uint32_t flags, msw_pileup** out);
/* The finished quality sums into host_out[glen][4]; synchronous (it waits for
 * the finish).  Before msw_pileup_finish, or on a pileup without
 * MSW_PILEUP_QSUM: MSW_E_INVALID. */
int msw_pileup_qsums(msw_ctx* ctx, msw_pileup* pile, uint32_t* host_out);
/* The sums on the device: channel c of position pos is
 * (*qsums)[pos * *pos_stride + c * *ch_stride] (rows of four: 4 and 1, in
 * either layout of the counts).  Valid at any time; the values are final once
 * the finish has run.  Without MSW_PILEUP_QSUM: MSW_E_INVALID. */
int msw_pileup_qsums_device(msw_ctx* ctx, msw_pileup* pile, const uint32_t** qsums, uint64_t* pos_stride,
                            uint64_t* ch_stride);

/* The three calls of "Variants" with weighted genotypes; their error rules,
 * cap, totals and chunking are the same.  qparams == NULL selects the
 * defaults; a q_scale or q_third above 65535 is MSW_E_INVALID.  The pileup
 * forms take a finished MSW_PILEUP_QSUM pileup (without the flag:
 * MSW_E_INVALID); msw_call_counts_qual takes qsums_host[glen][4] beside
 * counts_host and streams it in the same chunks (the sums need no look-ahead
 * row). */
int msw_pileup_call_qual_device(msw_ctx* ctx, msw_pileup* pile, const msw_call_params_t* params,
                                const msw_call_qparams_t* qparams, msw_variant_t* out_dev, uint64_t cap,
                                uint64_t* n_total_dev, void* stream);
int msw_pileup_call_qual(msw_ctx* ctx, msw_pileup* pile, const msw_call_params_t* params,
                         const msw_call_qparams_t* qparams, msw_variant_t* out_host, uint64_t cap, uint64_t* n_total);
int msw_call_counts_qual(msw_ctx* ctx, const uint8_t* genome_host, uint64_t glen, const uint32_t* counts_host,
                         const uint32_t* qsums_host, const msw_call_params_t* params,
                         const msw_call_qparams_t* qparams, uint64_t chunk_pos, msw_variant_t* out_host, uint64_t cap,
                         uint64_t* n_total);

/* Device memory helpers for callers that keep batches resident in HBM. */
void* msw_dev_alloc(msw_ctx* ctx, size_t bytes);
void msw_dev_free(msw_ctx* ctx, void* p);
int msw_memcpy_h2d(msw_ctx* ctx, void* dst, const void* src, size_t bytes);
int msw_memcpy_d2h(msw_ctx* ctx, void* dst, const void* src, size_t bytes);
/* enqueued on `stream` (NULL = the context's compute stream); dst should be
 * pinned: into pinned memory the copy runs as a kernel on that stream (not a
 * DMA on the process-wide copy-engine rings, where a copy waiting on one
 * stream holds up the copies of others); pageable dst: hipMemcpyAsync. */
int msw_memcpy_d2h_async(msw_ctx* ctx, void* dst, const void* src, size_t bytes, void* stream);
int msw_synchronize(msw_ctx* ctx);
/* A host-waitable point in `stream`'s work (NULL = the context's compute
 * stream): msw_fence_wait blocks until everything enqueued on that stream
 * before msw_fence_record has finished, without waiting for what came after
 * (msw_synchronize drains all of the context's streams).  A fence is waited
 * on once; the context keeps unwaited fences until it is destroyed.  Several
 * threads may wait on (different) fences of one context at once. */
int msw_fence_record(msw_ctx* ctx, void* stream, uint64_t* fence);
int msw_fence_wait(msw_ctx* ctx, uint64_t fence);
/* A stream of the context's device for callers that keep two batches in
 * flight (e.g. --full-wgs alternates its batches over the compute stream and
 * one of these, so one batch's read emit and window cut run beside the other
 * batch's scoring).  Any call taking `void* stream` accepts it; calls on two
 * streams may run concurrently.  msw_synchronize drains it; msw_ctx_destroy
 * destroys any the caller has not.  (The reference scores one batch at a
 * time on one queue: gpu.rs:117-125.) */
int msw_stream_create(msw_ctx* ctx, void** out);
int msw_stream_destroy(msw_ctx* ctx, void* stream);

/* Counters of the host-batch calls (msw_align_batch*, msw_align_reads*) on a
 * context, for run records (the reference's BenchmarkResult,
 * tools/benchmark.rs:17-34, reports only wall-clock rates):
 * kernel_ms = GPU time covered by the scoring launches: the union of their
 * [start, end] intervals (HIP events around each chunk's launch on its
 * compute stream -- a multi-chunk call alternates two compute streams, whose
 * launches overlap -- added when the chunk is drained; and around
 * msw_align_reads_device launches, added when they have finished),
 * alg_bytes = read + window bytes + 4 B score (+ 4 B coordinates) per pair,
 * the kernel's algorithmic HBM traffic.  reset != 0 zeroes them after the copy. */
typedef struct {
    double kernel_ms;
    uint64_t launches;
    uint64_t pairs;
    uint64_t cells;
    uint64_t alg_bytes;
} msw_stats_t;
int msw_ctx_stats(msw_ctx* ctx, msw_stats_t* out, int reset);

/* Optional, before a timed region: load the code objects of every scoring
 * kernel module a call under this scheme may use (the packed layouts, the
 * length-bucketed grid, genome windows, long pairs, the window cut, both
 * strands, traceback, the seed kernels).  HIP
 * loads a module on its first launch, ~1-2 ms each, which a short run --
 * one lane file per worker -- would otherwise pay inside its first batch
 * (the reference has no analogue: it JIT-builds its OpenCL program on every
 * gpu_align call, aligner.rs:504-508).  Launches nothing. */
int msw_ctx_prepare(msw_ctx* ctx, const msw_scoring_t* scoring);

/* Thread-local message of the last failing call on this thread. */
const char* msw_last_error(void);

/* Library version string (also names the compiled GPU target). */
const char* msw_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MSW_H */
