/* muscato_hip.h -- C ABI of libmuscato_hip.so: muscato's seed-and-extend hot path
 * (muscato_screen -> muscato_confirm [-> per-read best+MMTol]) on AMD MI355X (gfx950).
 *
 * The reference (kshedden/muscato, pure Go) has no in-process plugin/FFI interface for
 * this path: its boundary is two executables joined by snappy text files in TempDir,
 *     exec.Command("muscato_screen",  config.json)        cmd/muscato/main.go:306-316
 *     GNU sort of bmatch_k -> smatch_k                    cmd/muscato/main.go:318-385
 *     exec.Command("muscato_confirm", config.json, k)     cmd/muscato/main.go:387-420
 * with inputs  reads_sorted.txt.sz (unique reads), GeneFileName (one target per line,
 * gene number = line index) and outputs rmatch_k.txt.sz, lines
 * "read \t targetsub \t pos \t nmiss \t %011d"   (cmd/muscato_confirm/main.go:221-230).
 * This header is the boundary a cgo (or any FFI) host binds instead of spawning those
 * processes; INTEGRATION.md shows the cgo stub.  Each entry point names the reference
 * code it replaces.
 *
 * Conventions
 *   - plain C types only; no HIP / torch types cross the boundary.
 *   - every function returning int returns 0 on success, non-zero on error; the text of
 *     the last error of a context is musc_last_error(ctx).  Nothing aborts or throws
 *     across the boundary (the reference convention is exit status != 0,
 *     cmd/muscato/main.go:313-315, 411-415 -- the CLI maps errors to that).
 *   - ownership: inputs are borrowed for the duration of the call; outputs returned
 *     through musc_hit** are owned by the library until musc_free_hits().
 *   - threading: one musc_ctx per GPU; calls on one ctx must be serialised by the caller;
 *     different ctxs may be driven from different host threads (a Go caller must
 *     runtime.LockOSThread() around a call sequence: HIP's current device is per thread).
 *   - there is NO CPU fallback: if no gfx950 device is usable musc_init fails.
 */
#ifndef MUSCATO_HIP_H
#define MUSCATO_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MUSC_ABI_VERSION 3
#define MUSC_MAX_WINDOWS 16

typedef struct musc_ctx musc_ctx;

/* One accepted placement: read `read_idx` (index into the loaded unique reads) matches
 * target `gene_idx` (line index of the gene file) at target offset `pos` with `nmiss`
 * mismatches.  Equivalent to one rmatch_k / matches.txt line
 * (cmd/muscato_confirm/main.go:221-230). */
typedef struct {
  uint32_t read_idx;
  uint32_t gene_idx;
  uint32_t pos;
  uint32_t nmiss;
} musc_hit;

/* The part of utils.Config (utils/config.go:10-101) the hot path reads. */
typedef struct {
  int32_t n_windows;                 /* len(Config.Windows), 1..MUSC_MAX_WINDOWS       */
  int32_t windows[MUSC_MAX_WINDOWS]; /* Config.Windows: start of each window in a read */
  int32_t window_width;              /* Config.WindowWidth                             */
  double pmatch;                     /* Config.PMatch; nmiss = int((1-PMatch)*len)     */
  int32_t min_dinuc;                 /* Config.MinDinuc (utils/entropy.go:5-40 gate)   */
  int32_t max_read_length;           /* Config.MaxReadLength                           */
  int32_t max_matches;               /* Config.MaxMatches (per window-key block)       */
  int32_t match_mode;                /* 0 = "best", 1 = "first" (Config.MatchMode)     */
  int32_t mmtol;                     /* Config.MMTol                                   */
  /* 0: return every accepted tuple = set-union of rmatch_0..W-1 (output of muscato_confirm
   *    after combine_filter | sort -u, cmd/muscato/main.go:441-463);
   * 1: additionally keep, per read, only nmiss <= best+MMTol = matches.txt
   *    (cmd/muscato_combine_windows/main.go:36-60). */
  int32_t apply_mmtol;
  /* Addition (the reference has no such flag; BASELINE.json's --MaxMismatch): 0 = budget from
   * PMatch as above; v > 0 = every read may have at most v-1 mismatches. */
  int32_t max_mismatch_p1;
  /* 1 = skip the per-block MaxMatches check (musc_stats.n_overflow_blocks becomes ~0) */
  int32_t skip_block_check;
  /* > 1 when this context only sees 1/n_shards of the reads of a (window,key) block: the
   * MaxMatches check then uses MaxMatches / n_shards, so that "no overflow on any shard"
   * proves "no overflow" (SURVEY.md 8e caveat) */
  int32_t n_shards;
  int32_t reserved[2];
} musc_params;

/* Counters and device timings of the last musc_match* call on a context.
 *
 * What each counter counts, per path (tests/stats_model.py recounts every one of them on the CPU from the oracle's
 * window gate, k-mer index and fit rule; tests/test_gpu_stats.py holds each path to it).  "Fused" = context buckets
 * (index_kind 1 and 2: k_match_t, k_match_g), "two-kernel" = k_screen / k_screen_t -> k_confirm (index_kind 0 and 3).
 * Every counter is that of ONE pass over the reads: a batch that is repeated after its buffers grew, a pass that starts
 * over on smaller batches, and the exact repeat of a pass whose MaxMatches screening was inconclusive are counted
 * once, and a sized pass, a hipGraph replay and a streamed pass report what the first, careful pass reports.
 *   a PROBE     a (read, window) pair with len >= Windows[k] + WindowWidth and CountDinuc(window) >= MinDinuc.  Fused: less
 *               the read windows that hold an X (they never probe; a read with more X than its xpos word lists -- four,
 *               wide buckets three -- has no probe at all).  Two-kernel: a window with an X does probe.
 *   a CANDIDATE an index entry of the bucket a probe fetches.  On a direct table (bucket = key) these are the window
 *               starts of the database with the probe's key -- a window that would cross its target's end is never
 *               indexed, and context buckets do not index a window that holds an X; on a hashed table also the entries
 *               of the keys that share the bucket.
 *   FITS        p = jx - Windows[k] >= 0 and p + len <= target length, or, at jx == 0, len <= min(100 - WindowWidth, target
 *               length) (cmd/muscato_screen/main.go:294-316, :347-353, cmd/muscato_confirm/main.go:201-203).
 * With several partitions every counter but n_reads, n_hits and n_overflow_blocks is the SUM over the partitions'
 * passes: each pass probes every read window again (n_read_windows = probes x partitions), finds the candidates of its
 * own index, and writes its own tuples (with apply_mmtol the best + MMTol among that partition's targets: the bytes bill
 * those, which may be more than n_hits). */
typedef struct {
  uint64_t n_reads;         /* unique reads loaded (several partitions: once)                                   */
  uint64_t n_read_windows;  /* probes                                                                           */
  uint64_t n_candidates;    /* candidates: the sum over the probes of their bucket's entry count                */
  uint64_t n_pairs;         /* fused: the candidates that fit -- every one of them is compared with the read.
                             * two-kernel: the candidates that fit AND pass the flank filter (the min(Windows[k], 8) read
                             * bases left of the window and the min(len - Windows[k] - WindowWidth, 8) right of it differ from
                             * the target's in at most the read's mismatch budget), per (read, window, placement) -- the
                             * reference's smatch/win join output minus what the flank filter rules out: what reaches
                             * k_confirm, a two-window descriptor counting twice.  The screen never compares the key
                             * itself, so on a hashed table an entry of a colliding key that fits and passes the flank
                             * filter is a pair too (k_confirm rejects it)                                  */
  uint64_t n_accepted;      /* distinct (read, target, position) with nmiss <= budget: the union over the windows, before
                             * the best + MMTol selection, whatever apply_mmtol is                      */
  uint64_t n_hits;          /* tuples returned (apply_mmtol = 0: n_accepted)                             */
  /* (window,key) blocks whose accepted pairs may exceed MaxMatches: 0 = proven none (the
   * reference's truncation, cmd/muscato_confirm/main.go:233-242, 424-448, never triggered and
   * the tuples are exact); > 0 = upper bound; ~0 = check skipped */
  uint64_t n_overflow_blocks;
  uint64_t confirm_bytes;   /* two-kernel: algorithmic bytes of the confirm launches: n_descriptors x (12 B descriptor +
                             * ceil(2L/8) B record + ceil(2L/8) + 1 B target span; 63 B at L = 100) + 16 B per
                             * tuple written, L = the longest loaded read.  Fused: 0                         */
  uint32_t confirm_launches; /* two-kernel: k_confirm launches, <= n_batches and equal when every batch has a descriptor
                             * (a careful pass skips the launch for a batch without one).  Fused: 0              */
  uint32_t n_batches;       /* batches of the pass: ceil(n_reads / batch) uniform ones, or those of musc_stream_plan
                             * when the pass consumes a streamed load (the exact repeat of such a pass finds the
                             * reads resident and runs, and reports, uniform batches)                          */
  float ms_screen;          /* HIP-event time of each kernel family, summed over batches:  */
  float ms_scan;            /*   k_screen (index_kind 0) or k_match (1) | scan | (see match_variant) |
                             *   k_confirm (index_kind 0 only) | scan+k_compact            */
  uint32_t match_variant;   /* (ABI 3; the slot was an unused float) which fused kernel ran on context buckets:
                             * 0 = none (two-kernel path), 2 = k_match_t, general
                             * instance, 3 = k_match_t specialised for the run's geometry (SpecGeom<1>),
                             * 4 = k_match_g (three waves per SIMD, LDS-DMA), general, 5 = k_match_g specialised */
  float ms_confirm;
  float ms_select;
  float ms_total;           /* first launch to last completion on the context's stream  */
  float ms_index_build;     /* last musc_db_build_index                                 */
  float ms_read_prep;       /* last musc_reads_sort_unique (device time)                   */
  uint64_t n_descriptors;   /* two-kernel: descriptors k_screen wrote.  Line buckets (index_kind 3): one per pair,
                             * n_descriptors = n_pairs.  64-byte buckets: one descriptor stands for windows 2j and 2j + 1
                             * of a read when both found the placement among their buckets' inline entries (then it is two
                             * pairs), so distinct (read, window pair, placement) <= n_descriptors <= n_pairs, and
                             * n_pairs - n_descriptors = the two-window descriptors.  Fused: 0 (no descriptors exist) */
  /* ---- since ABI version 2 */
  uint32_t index_kind;      /* index the pass ran on: 0 = 64-byte window-start buckets + target
                             * gather (k_screen -> k_confirm), 3 = the same on 128-byte line
                             * buckets (dense databases; k_screen_t -> k_confirm), 1 = context
                             * buckets, 120 bases (k_match_t or k_match), 2 = wide context
                             * buckets, 200 bases (k_match_t)                                */
  uint32_t match_launches;  /* fused: launches of the match kernel = n_batches.  Two-kernel: 0     */
  uint64_t n_overflow_entries; /* fused: the sum over the probes of max(0, bucket count - 3) (wide buckets: - 2), the
                             * entries beyond a bucket's inline ones, all of which are walked.  Two-kernel: 0 (not counted) */
  uint64_t match_bytes;     /* fused: algorithmic bytes of the match launches: n_reads x ceil(2L/8) B of records (L = the
                             * longest loaded read) + one 128-B bucket line per probe + 40 B (wide: 60) per overflow entry
                             * + 16 B per tuple staged.  Two-kernel: 0                         */
  uint64_t match_bytes_strict; /* the same with a probe billed for what it uses of its line: 8 B header + 40 B
                             * (wide: 60) per entry, inline or not: n_reads x ceil(2L/8) + 8 x n_read_windows + 40 x
                             * n_candidates + 16 per tuple staged                                  */
  uint64_t index_bytes;     /* device memory the resident index holds: (buckets + 1) x the bucket size (context and line
                             * buckets 128 B, window-start buckets 64 B; a direct table has 4^WindowWidth buckets) + the overflow
                             * array as allocated -- context buckets: whole 128-B lines of three entries (wide: two) for the
                             * overflow entries + 16; 64-byte buckets: 16 B x (overflow entries + 16); line buckets: 16 B x
                             * (8 x the overflow lines of eight slots, used or not, + 16).  The build's temporaries,
                             * released when the build ends, are not included.  Several partitions: the last partition's
                             * index.  (tests/stats_model.py models the context tables only.)                       */
} musc_stats;

int musc_abi_version(void);

/* Create / destroy a context bound to HIP device `device_ordinal` (one per GPU). */
int musc_init(int device_ordinal, musc_ctx** out);
void musc_destroy(musc_ctx* ctx);
const char* musc_last_error(musc_ctx* ctx); /* ctx may be NULL: error of a failed musc_init */
/* The MUSC_* environment knobs (tests, A/B runs: MUSC_INDEX, MUSC_MATCH, MUSC_GRAPH ...) are read once, by
 * musc_init; a pass never calls getenv.  This re-reads them for a live context (a test hook; the next pass sizes
 * its buffers again).  The reference has no counterpart: its knobs are the Config fields.
 * The rule: every MUSC_* knob is latched when the context is made.  Setting or clearing one in the environment of a
 * live context changes nothing until musc_reload_env, which latches all of them again -- except MUSC_BATCH_READS,
 * which keeps its value of musc_init (a streamed load in flight was planned with it), and MUSC_RCCL_LIB, which is
 * read once per process.  musc_reload_env also lets a MUSC_GRAPH whose capture failed once be tried again. */
int musc_reload_env(musc_ctx* ctx);

/* ---- target database: replaces muscato_screen's scan of GeneFileName
 * (cmd/muscato_screen/main.go:408-452; gene number = sequence index). --------------------
 *
 * A failed call of any loader (musc_db_load_ascii, musc_db_load_packed, musc_db_load_text) leaves no database: the
 * next pass answers "no database loaded".  (The first two refuse a NULL argument before they touch the database in hand.)
 *
 * ASCII form: `seqs` holds nseq sequences back to back, sequence i = bytes
 * [offsets[i], offsets[i+1]).  'A','C','G','T' are bases, every other byte is the
 * reference's 'X' (cmd/muscato_prep_targets/main.go:68-80).  on_device != 0 means both
 * pointers are device pointers.  A target may have any length (an empty one included) on a database below 2^32
 * bases; context buckets on a database with X take targets below 2^31 bases (longer ones run on the window-start
 * buckets), and tuples report positions in 32 bits whatever the index kind. */
int musc_db_load_ascii(musc_ctx* ctx, const char* seqs, const uint64_t* offsets, uint32_t nseq,
                       int on_device);
/* Packed form: 2 bits per base (A=0 C=1 G=2 T=3), base j of the concatenated stream in bits
 * [2j%8, 2j%8+2) of byte j/4; nmask (may be NULL) has 1 bit per base, bit j%8 of byte j/8, set
 * where the base is 'X' (the 2-bit code under a set mask bit is ignored).  seq_offsets are in
 * bases, nseq+1 entries.  Host pointers. */
int musc_db_load_packed(musc_ctx* ctx, const uint8_t* bases2bit, const uint8_t* nmask,
                        const uint64_t* seq_offsets, uint32_t nseq);
/* Build the k-mer -> target position index for WindowWidth (done lazily by musc_match if the
 * width changed).  One-off per (database, width); replaces the per-run Bloom sketch + full
 * database scan of cmd/muscato_screen/main.go:116-207, 256-366 (result-equivalent: SURVEY.md
 * 8a note H). */
int musc_db_build_index(musc_ctx* ctx, int32_t window_width);
/* The same for a whole parameter block: builds the index musc_match* will pick for `params` and
 * reads of at most max_read_len bases (0 = params->max_read_length) -- context buckets (128-byte
 * buckets that carry each placement's 120 surrounding target bases, so that screen and confirm
 * are one kernel and no target gather is needed, or 200 bases for two placements per bucket; see
 * kernels_match.hpp) when the run fits them -- a database with X included: its entries whose
 * context holds an X are flagged and compared as cmd/muscato_confirm/main.go:151-159 does -- the
 * window-start-bucket index of musc_db_build_index otherwise.  musc_match* does this lazily;
 * calling it first only moves the one-off cost out of the first match.  MUSC_INDEX=classic in
 * the environment forces the window-start buckets, MUSC_NO_X_CONTEXT=1 only for runs with X. */
int musc_db_build_index_for(musc_ctx* ctx, const musc_params* params, int32_t max_read_len);

/* Partitions (an addition: the reference streams the database from disk and has no index to fit).  A database whose
 * index does not fit the device is matched in partitions: contiguous ranges of whole targets, each of whose index is
 * built in turn while the packed database stays resident; every pass runs over all reads, and the tuples are merged
 * on the device into exactly what one pass over an index of the whole database returns -- the same tuples (with
 * apply_mmtol the global best + MMTol), read-major (within a read: partition order), gene_idx the global target
 * number, and the same MaxMatches verdict (n_overflow_blocks, musc_overflow_probes) over the whole database.
 * With one partition -- the default whenever the index fits -- nothing changes.  With several, musc_stats sums the
 * counters, bytes and times (ms_index_build included) over the partitions; n_hits and n_overflow_blocks are those of
 * the merged result, index_kind / match_variant / index_bytes those of the partitions (one kind and table size per
 * pass).
 * musc_db_set_partition_bases: at most max_bases target bases per partition (a longer target is a partition of its
 * own); 0 = automatic (the default: one partition if the index fits, else the fewest ranges of about equal bases
 * whose index does).  It takes effect at the next build or match; musc_db_build_index_for then builds the first
 * partition's index.  More than 4096 partitions is an error. */
int musc_db_set_partition_bases(musc_ctx* ctx, uint64_t max_bases);
/* The plan of the last build or match: *n partitions, partition p = targets [first_target[p], first_target[p+1]);
 * n + 1 boundaries are written when first_target is not NULL (cap = room for boundaries).  *n = 0 before any. */
int musc_db_partitions(musc_ctx* ctx, uint32_t* first_target, uint32_t cap, uint32_t* n);

/* ---- reads: replaces reading reads_sorted.txt.sz (cmd/muscato_screen/main.go:120-191,
 * cmd/muscato_window_reads/main.go:94-141).  Reads must already be prepared as the
 * reference does (non-ACGT -> X, truncated to MaxReadLength, de-duplicated); read_idx in the
 * hits is the index into this array.
 * One rule for every loader below (and the two read-prep calls): a load replaces the reads in hand, and after a load
 * that failed, at whatever point, the context holds no reads: musc_match* answers 4, "no reads loaded", until a load
 * succeeds. --------------------------------------------------------------------------- */
int musc_reads_load_ascii(musc_ctx* ctx, const char* seqs, const uint64_t* offsets,
                          uint64_t nreads, int on_device);
int musc_reads_load_packed(musc_ctx* ctx, const uint8_t* bases2bit, const uint8_t* nmask,
                           const uint64_t* read_offsets, uint64_t nreads);
/* The same with 32-bit lengths instead of 64-bit offsets (`const uint32_t*
 * lengths_or_offsets`): lengths[i] = bases of read i, or lengths == NULL: every read has fixed_len
 * bases (nothing but the bases crosses PCIe then).  The reads sit back to back in the 2-bit stream.
 * async != 0 (fixed length, no mask): the call returns once the upload is QUEUED -- in pieces, on a
 * copy stream of its own -- and the next musc_match* on the context packs and matches each batch of
 * reads as its piece arrives, so that upload and matching overlap (the reference's equivalent is
 * muscato_screen reading reads_sorted.txt.sz while it hashes, cmd/muscato_screen/main.go:116-207).
 * The caller's buffer must then stay valid until that musc_match* call (or musc_destroy) returns;
 * pinned memory makes the upload asynchronous in fact. */
int musc_reads_load_packed32(musc_ctx* ctx, const uint8_t* bases2bit, const uint8_t* nmask,
                             const uint32_t* lengths, uint32_t fixed_len, uint64_t nreads, int async);

/* Read prep on the GPU: replaces the bytewise sort of the prepared reads (sortReads in
 * cmd/muscato/main.go: GNU sort of the `seq\tname` lines under LC_ALL=C) and the collapse of
 * identical sequences (cmd/muscato_uniqify/main.go:83-135) for the sequence column.
 * Input: nreads reads as they leave muscato_prep_reads (non-ACGT -> X, length filter, truncated),
 * in input order, ASCII + offsets like musc_reads_load_ascii.
 * Afterwards the context's reads are the DISTINCT sequences in bytewise order (a proper prefix
 * first), exactly as if the first column of reads_sorted.txt.sz had been loaded, and
 *   order[nreads]       input read numbers sorted by sequence, ties in input order
 *   ustart[*nunique+1]  distinct sequence g = the input reads order[ustart[g] .. ustart[g+1])
 * so the host can write `seq\tcount\tnames` (count = group size; the reference's name order within
 * a group is the bytewise order of the names, which the caller applies).  Both arrays are
 * malloc'ed by the library: musc_free_u32. */
int musc_reads_sort_unique(musc_ctx* ctx, const char* seqs, const uint64_t* offsets, uint64_t nreads,
                           int on_device, uint32_t** order, uint32_t** ustart, uint64_t* nunique);

/* FASTQ parsing on the GPU, in front of the sort above: replaces utils/fastq.go:35-61 (records of four lines under
 * bufio.ScanLines: one trailing '\r' of a line is dropped, a last line without '\n' is a line, an incomplete last
 * record of 1, 2 or 3 lines is dropped) and cmd/muscato_prep_reads/main.go:46-92 (a read whose raw length is below
 * MinReadLength goes; every byte that is none of A C G T becomes X; the rest is cut at MaxReadLength).
 * text = the nbytes raw bytes of the read file (on_device != 0: a device pointer, any alignment; bytes outside
 * [text, text + nbytes) are never read).  min_read_len <= 0 keeps every record; max_read_len < 0 is an error (2).
 * Afterwards the context's reads are the distinct PREPARED sequences in bytewise order, exactly what
 * musc_reads_sort_unique leaves for the same prepared reads (a prepared read of more than 65535 bases fails as it does
 * there), stats.ms_read_prep covers the whole device stage (parse + sort + collapse), and `out` describes the kept
 * reads, numbered in file order: spans into the caller's text, and order / ustart as musc_reads_sort_unique returns
 * them.  No complete record (nbytes == 0 included): zero reads, and arrays that are valid and empty.
 * What stays with the caller: the 1000-byte rule for a read's name (cmd/muscato_prep_reads/main.go:76-79: name_len is
 * the length before it), the cut of a name at its first tab and the 1000-byte rule of the joined names
 * (cmd/muscato_uniqify/main.go:83-135), and the order of the names within a group (the bytewise order of the names).
 * Not enforced: the reference's 1 MiB line limit (utils/fastq.go:25-27 gives its scanner a 1 MiB buffer and panics on a
 * longer line; the host path of this project does not enforce it either).
 * A device allocation that fails returns 10, the library's code for a failed HIP call ("out of memory" in the text);
 * after that, as after every failed call here, the context holds no reads and `out` is all zero.
 * The arrays are malloc'ed by the library: musc_fastq_prep_free (which zeroes the struct; a zeroed struct is fine).
 * MUSC_ABI_VERSION is unchanged: these are additions. */
typedef struct musc_fastq_prep {
  uint64_t n_records, n_short, n_reads, n_unique;  /* n_reads = n_records - n_short */
  uint32_t max_len, reserved;      /* max_len: the longest prepared read                        */
  uint64_t *name_off, *seq_off;    /* [n_reads] byte offsets into the caller's text            */
  uint32_t *name_len, *seq_len;    /* [n_reads] name: after the \r rule, before the 1000 rule; */
                                   /*           seq: the prepared length                       */
  uint32_t *order, *ustart;        /* as musc_reads_sort_unique, over the kept reads           */
} musc_fastq_prep;
int  musc_reads_prep_fastq(musc_ctx* ctx, const char* text, uint64_t nbytes, int on_device,
                           int32_t min_read_len, int32_t max_read_len, musc_fastq_prep* out);
void musc_fastq_prep_free(musc_fastq_prep* p);

/* ---- the names of the reads on the device (additions; MUSC_ABI_VERSION is unchanged) -------------------------------
 * What musc_reads_prep_fastq leaves to the caller, done in place on the raw text: a name of more than 1000 bytes becomes
 * its first 995 and "..." (cmd/muscato_prep_reads/main.go:76-79); the members of a group of identical prepared reads
 * are ordered by that clipped name bytewise (unsigned bytes, a proper prefix first, equal names in file order: the
 * `sort` of the seq\tname lines under LC_ALL=C); a name ends at its first tab, the names of a group are joined with ';'
 * and a join of more than 1000 bytes becomes its first 996 and "..." (cmd/muscato_uniqify/main.go:83-135).
 * Groups of up to 64 members are ranked by counting; the members of larger groups by W + 2 stable radix-sort passes
 * over 64-bit keys (clipped length and read number; the W 8-byte words of the longest clipped name, last to first; the
 * group number).  No sort under a comparator runs.
 *
 * musc_reads_names_order: the ranking alone, on hand-fed groups.  text, name_off, name_len, order, ustart are what
 * musc_reads_prep_fastq takes and returns (on_device != 0: text is a device pointer; the arrays are host arrays);
 * n = the kept reads, nu = the groups, ranked_out[n] = the kept reads group by group in name order.  The arrays are
 * checked before anything is indexed by them (a name outside the text, a member >= n, groups that are empty or do not
 * span the n places: 2).  Needs no loaded reads and leaves the context's reads and texts alone. */
int musc_reads_names_order(musc_ctx* ctx, const char* text, uint64_t nbytes, int on_device, const uint64_t* name_off,
                           const uint32_t* name_len, uint64_t n, const uint32_t* order, const uint32_t* ustart, uint64_t nu,
                           uint32_t* ranked_out);
/* musc_reads_prep_fastq_names: musc_reads_prep_fastq with the text kept resident until the records count\tJ of all groups
 * are rendered; they are left as the context's read text exactly as musc_results_set_read_text of the same bytes would
 * leave them.  `out` as musc_reads_prep_fastq fills it (musc_fastq_prep_free); `info` as below, ranked[n_reads] =
 * the kept reads group by group in name order, malloc'ed by the library: musc_free_u32.  After a failed call the context
 * holds no reads and no read text, and both structs are all zero. */
typedef struct musc_read_names {
  uint64_t text_bytes, line_bytes;         /* of all records count\tJ / of all lines seq\tcount\tJ\n   */
  uint64_t n_single, n_counted, n_sorted;  /* groups of 1 / of 2 to 64 / of more members              */
  uint64_t n_pairs;                        /* members of the groups that went through the key passes  */
  uint32_t key_passes;                     /* W + 2, or 0 when no group has more than 64 members      */
  float ms_names;                          /* device time of the stage behind the sort + collapse     */
  uint32_t* ranked;
} musc_read_names;
int musc_reads_prep_fastq_names(musc_ctx* ctx, const char* text, uint64_t nbytes, int on_device, int32_t min_read_len,
                                int32_t max_read_len, musc_fastq_prep* out, musc_read_names* info);
/* Records [rec0, rec0 + nrec) (clipped at the end) of the texts the call above left: which = 0, the records count\tJ;
 * which = 1, the lines seq\tcount\tJ\n, which are reads_sorted.txt byte for byte.  dst, capacity, dst_on_device and
 * *nbytes as musc_results_text.  Refused (2) once the reads or the read text have been replaced. */
int musc_reads_names_text(musc_ctx* ctx, int which, uint64_t rec0, uint64_t nrec, char* dst, uint64_t capacity, int dst_on_device,
                          uint64_t* nbytes);

/* ---- the hot path: screen + confirm (+ per-read best filter) -------------------------
 * musc_match_device leaves the hits in device memory (count in *nhits);
 * musc_hits_copy copies them to `dst` (host, or device if dst_on_device) -- capacity in
 * hits; musc_match = both, into a library-owned host array.  Hit order is unspecified. */
int musc_match_device(musc_ctx* ctx, const musc_params* params, uint64_t* nhits);
int musc_hits_copy(musc_ctx* ctx, musc_hit* dst, uint64_t capacity, int dst_on_device);
/* The same tuples as one u64 each, for the wire (gather to rank 0 over RCCL/xGMI) or for keeping
 * them compact: (read_idx + read_base) in the top bits, then gene_idx, pos, nmiss, with
 * bits[4] = the widths of read, gene, pos, nmiss (each 1..32, sum <= 64).  The numeric order of
 * the words is the lexicographic order of the tuples.  Fails with code 8 if a field of some
 * tuple does not fit its width.  musc_hits_unpack inverts it (src and dst both on the device or
 * both on the host). */
int musc_hits_copy_packed(musc_ctx* ctx, uint64_t* dst, uint64_t capacity, int dst_on_device,
                          uint64_t read_base, const int32_t* bits);
int musc_hits_unpack(musc_ctx* ctx, const uint64_t* src, uint64_t n, int on_device, const int32_t* bits,
                     musc_hit* dst);
/* The most compact wire form (5 bytes per tuple at one tuple per read, against 8 and 16): the hit
 * list is read-major -- a read's tuples are contiguous and reads come in increasing order -- so the
 * read index travels as counts[r] = number of tuples of read r (one byte per loaded read) and a
 * tuple is one u32 word gene | pos | nmiss with bits[3] = the widths of gene, pos, nmiss (sum <= 32).
 * Fails with code 8 if a field does not fit or a read has more than 255 tuples (use the 8-byte
 * form then).  words: room for nhits words, counts: room for the loaded reads. */
int musc_hits_copy_compact(musc_ctx* ctx, uint32_t* words, uint64_t words_capacity, uint8_t* counts,
                           uint64_t counts_capacity, int dst_on_device, const int32_t* bits);
int musc_match(musc_ctx* ctx, const musc_params* params, musc_hit** hits, uint64_t* nhits);
void musc_free_hits(musc_hit* hits);

int musc_get_stats(musc_ctx* ctx, musc_stats* out);

/* ---- results.txt from the resident tuples: replaces the post-chain of cmd/muscato/main.go:422-676 (combine_windows,
 * the gene-id join, `sort -k1`, the read join).  A line is
 *     read \t targetsub \t pos \t nmiss \t name \t len \t count \t names \n
 * with targetsub = target[pos : pos + len(read)] clipped at the target's end; the lines are ordered bytewise on
 * their first six columns (cmd/muscato/main.go:657).  Reads, database and tuples are resident; the two texts below
 * are what the device cannot know.  MUSC_ABI_VERSION is unchanged: these are additions.
 * targetsub is rendered and ordered from the packed database (2 bits a base + the X plane): every target byte that is
 * none of A C G T comes out as 'X', as musc_db_load_ascii reads it.  A host whose targets hold other letters (an 'N'
 * that muscato_prep_targets left in the last FASTA record, cmd/muscato_prep_targets/main.go:204-212) and that must
 * quote them literally keeps its own post-chain for that run, as the CLI does. */
/* Gene g's `name\tlen` (what follows the gene number on its line of the id file, the join of
 * cmd/muscato/main.go:524-611) = bytes [offsets[g], offsets[g + 1]) of text, nseq = the loaded targets.  absent (may be
 * NULL): absent[g] != 0 = the id file has no line for gene g, and its tuples vanish as unpairable lines do in `join`.
 * Uploads the text and ranks the genes' texts bytewise (equal texts share a rank).  A database load forgets it. */
int musc_results_set_gene_text(musc_ctx* ctx, const char* text, const uint64_t* offsets, const uint8_t* absent, uint32_t nseq);
/* Read r's `count\tnames` (columns 2 and 3 of reads_sorted.txt.sz, joined at cmd/muscato/main.go:659) = bytes
 * [offsets[r], offsets[r + 1]); nreads = the loaded reads.  A read load forgets it.  Without it the lines end after
 * the sixth column. */
int musc_results_set_read_text(musc_ctx* ctx, const char* text, const uint64_t* offsets, uint64_t nreads);
/* Order n tuples (hits == NULL: the list the last musc_match* left on the device, n ignored; on_device != 0: hits is
 * a device pointer) as `sort -k1` orders their lines (cmd/muscato/main.go:657), without the tuples of absent genes,
 * and compute every line's byte offset: *nlines lines, *nbytes bytes in all.  The tuples are expected to be the
 * selection that reaches results.txt (matches.txt: apply_mmtol = 1).  A tuple with read_idx >= the loaded reads,
 * gene_idx >= the loaded targets, pos > its target's length or nmiss > 65535 fails the call (code 2) before anything
 * is loaded through it.  Needs the gene text; setting either text afterwards invalidates the order.
 * A device list must be 16-byte aligned (it is read one tuple per 16-byte load; hipMalloc'ed memory is).  hits == NULL
 * needs the list of a pass over the reads and the database in hand: after a read or database load the call fails
 * (code 2) until the next musc_match*. */
int musc_results_order(musc_ctx* ctx, const musc_hit* hits, uint64_t n, int on_device, uint64_t* nlines, uint64_t* nbytes);
/* The ordered tuples (capacity in tuples): the lines of matches.txt (cmd/muscato_combine_windows/main.go:36-60) with
 * their gene number still in place, in the order `sort -k1` gives their results lines (cmd/muscato/main.go:657). */
int musc_results_hits(musc_ctx* ctx, musc_hit* dst, uint64_t capacity, int dst_on_device);
/* The bytes of lines [line0, line0 + nlines) of the last order, clipped at its end (a range past it: 0 bytes), into
 * dst -- a host buffer is filled through a bounded device staging buffer.  *nbytes = bytes of the range; dst == NULL
 * only reports them.  capacity < the range: code 2, nothing is written, *nbytes = 0.  The concatenation over
 * consecutive ranges is ResultsFileName.  Code 11: a line no longer fits the data in hand (nothing of the range is to
 * be used). */
int musc_results_text(musc_ctx* ctx, uint64_t line0, uint64_t nlines, char* dst, uint64_t capacity, int dst_on_device,
                      uint64_t* nbytes);
/* HIP-event time of the last musc_results_order and of all musc_results_text calls since (the reference logs wall
 * time per stage of this chain only: cmd/muscato/main.go:1041-1056). */
int musc_results_last_ms(musc_ctx* ctx, float* ms_order, float* ms_text);
/* "pos \t nmiss" of a line as one integer that compares as that text does under `sort` (cmd/muscato/main.go:657):
 * each decimal digit is 4 bits (digit + 1), left-aligned and zero-padded, ten digits of pos above five of nmiss.
 * Needs no device; 2 for nmiss > 99999. */
int musc_results_number_key(uint32_t pos, uint32_t nmiss, uint64_t* key);

/* ---- the three side outputs from the resident tuples.  They replace what the reference reads back
 * from results.txt: the nonmatch FASTQ of cmd/muscato_nonmatch/main.go:95-114 (an exact set for its Bloom filter),
 * `*_genestats` of cmd/muscato/main.go:94-150 + cmd/muscato_genestats/main.go, and `*_readstats` of
 * cmd/muscato_readstats/main.go (the gene set of a line in bytewise order).  Whitespace is C isspace.  The token of
 * a read is the second field of its text `count\tnames` (the first name), its count the first field.
 *   nonmatch:  the loaded reads in order, without those that have a kept tuple or an empty token:
 *              token#count \n SEQ \n + \n !(len times) \n
 *   genestats: name \t N \t \n per distinct gene NAME with a kept tuple, N = the kept tuples of all genes of that
 *              name, in bytewise name order
 *   readstats: the matched reads that have a token, in read order; consecutive ones with equal tokens are a run;
 *              token \t then name; per distinct gene name among the run's kept tuples, bytewise, then \n
 * MUSC_ABI_VERSION is unchanged: these are additions. */
enum { MUSC_SIDE_NONMATCH = 0, MUSC_SIDE_GENESTATS = 1, MUSC_SIDE_READSTATS = 2 };
/* Build the record lists of the three texts from the last successful musc_results_order of this context:
 * nrecords[3] and nbytes[3] (either may be NULL) per text.  Code 2: no such order, no read text, or anything since
 * that invalidates the order (a read or database load, a new gene or read text, a musc_match*).  Code 12: the gene
 * text is not in the simple form the device needs -- every present gene's text exactly `name\tlen` with one tab, both
 * sides non-empty and every other byte above 0x20 (what muscato_prep_targets writes; checked when the text is set).
 * Code 12 is a refusal, not a fault: the context stays as it was, and the caller keeps its host path. */
int musc_side_prepare(musc_ctx* ctx, uint64_t* nrecords, uint64_t* nbytes);
/* The bytes of records [rec0, rec0 + nrec) of text `which`, clipped at its end (a range past it: 0 bytes), into dst
 * -- a host buffer is filled through a bounded device staging buffer, a device buffer may have any alignment.
 * *nbytes = bytes of the range; dst == NULL only reports them.  capacity < the range: code 2, nothing is written.
 * The concatenation over consecutive ranges is the file.  Code 11: a record no longer fits the data in hand. */
int musc_side_text(musc_ctx* ctx, int which, uint64_t rec0, uint64_t nrec, char* dst, uint64_t capacity, int dst_on_device,
                   uint64_t* nbytes);
/* HIP-event time of the last musc_side_prepare and of all musc_side_text calls since. */
int musc_side_last_ms(musc_ctx* ctx, float* ms_prepare, float* ms_text);

/* Which kernel instances the last musc_match* launched (tests: a pass that silently took another instance than the
 * one a test was written for is noticed).  The host resolves every kernel through a table whose entries hold the
 * function pointer and its descriptor side by side; these words are the descriptors of the entries the last pass took.
 *   out[0]  the fused kernel (0: the pass ran the two-kernel path)
 *             MUSC_INST_MATCH_T  k_match_t<RW, W, XM, WIDE, SG>
 *             MUSC_INST_MATCH_G  k_match_g<RW, SG>
 *   out[1]  the screen kernel of the two-kernel path (0: a fused pass)
 *             MUSC_INST_SCREEN   k_screen<RW, mask, one, lines>
 *             MUSC_INST_SCREEN_T k_screen_t<RW>
 *   out[2]  MUSC_INST_CONFIRM    k_confirm<RW, mask, w2>  (0: a fused pass, or no batch reached the confirm stage)
 *   out[3]  bits 0-7 the MaxMatches block mode of the last pass (0 none, 1 screening, 2 exact counters); bit 8: that
 *           pass was the exact repeat of a pass whose screening was inconclusive
 * A descriptor: bits 0-7 the family, 8-15 RW (0: the runtime-stride instance), then one template argument per
 * field, in the order written above: bits 16-19, 20-23, 24-27, 28-31 (k_match_g: SG in 28-31).
 * After a partitioned pass: the instances of the last partition. */
#define MUSC_INSTANCE_WORDS 4
#define MUSC_INST_MATCH_T 1u
#define MUSC_INST_MATCH_G 2u
#define MUSC_INST_SCREEN 3u
#define MUSC_INST_SCREEN_T 4u
#define MUSC_INST_CONFIRM 5u
int musc_last_instance(const musc_ctx* ctx, uint32_t* out);
/* Every descriptor the library's resolvers can return (needs no device): *n their number, the first `capacity` of
 * them in `out` (may be NULL with capacity 0). */
int musc_instances(uint32_t* out, uint32_t capacity, uint32_t* n);

/* The schedule of a streamed load (musc_reads_load_packed32 with async = 1) and of the pass that consumes it (needs no
 * device): the upload is queued in *n pieces, piece i ending before read ends[i]; is_batch_end[i] != 0 where the pass
 * launches a batch that ends with piece i.  Full batches of batch_reads (rounded up to 64) while two of them remain,
 * then batches of half of what is left, down to a last batch of at most max(64, batch_reads / 16 rounded up to 64)
 * reads; every end but the last is a multiple of 64.  *planned_batches: the batch count the MaxMatches screening
 * threshold of that pass is divided by.  The first `capacity` entries are written (ends / is_batch_end may be NULL);
 * 1 for fixed_len > 65535 or nreads >= 2^32 - 16.  batch_reads outside 1..2^24: the default, 2^24. */
int musc_stream_plan(uint64_t nreads, uint32_t fixed_len, uint32_t batch_reads, uint64_t* ends, uint8_t* is_batch_end,
                     uint64_t capacity, uint64_t* n, uint64_t* planned_batches);

/* When the last musc_match* left n_overflow_blocks > 0: the (read, window) probes whose
 * (window, key) block may hold more than MaxMatches accepted pairs -- the blocks for which
 * cmd/muscato_confirm/main.go:233-242, 424-448 keep an order-dependent subset.  The library
 * returns every accepted tuple; a host that must reproduce the truncation literally re-derives
 * those blocks from this list (muscato_host.hpp: apply_maxmatches).  Arrays are library-owned
 * until musc_free_u32(); n = 0 when nothing overflowed. */
int musc_overflow_probes(musc_ctx* ctx, uint32_t** read_idx, uint32_t** window, uint64_t* n);
void musc_free_u32(uint32_t* p);

/* ---- the MaxMatches truncation replayed on the device: what apply_maxmatches of muscato_host.hpp does
 * on the host from the downloaded tuples and musc_overflow_probes, without either leaving the device.  Needs the list
 * of a musc_match* on this context with apply_mmtol = 0 (and n_shards <= 1, and the MaxMatches check not skipped) over
 * the reads and the database in hand, and uses that pass's parameters: otherwise code 2.  The list of the pass becomes
 * the reference's selection -- in every (window, key) block with more than MaxMatches accepted pairs the pairs that
 * cmd/muscato_confirm/main.go:183-244, 424-448 keep (candidates in the bytewise order of their smatch line, reads in
 * that of their win_k_sorted line; "first": the first MaxMatches + 1; "best": the sift-up heap cut at MaxMatches), and
 * the union over the windows rebuilt for the reads of those blocks -- and, with apply_mmtol != 0, of that per read the
 * tuples with nmiss <= best + MMTol (matches.txt).  It stays resident and read-major as "the list of the last pass":
 * musc_hits_copy*, musc_results_order(hits = NULL), musc_results_hits and the side stage read it; a read or database
 * load or a musc_match* replaces it as usual, and a second call without a new pass returns 2.
 * *n_suspect_probes = the probes musc_overflow_probes would name, *n_truncated_blocks = the blocks that really held
 * more than MaxMatches pairs (the others are false alarms of the hashed counters and are left alone), *nhits = the
 * tuples of the new list; each pointer may be NULL.  No suspect probe: apply_mmtol = 0 changes nothing, apply_mmtol
 * != 0 applies the per-read selection only.
 * Code 10: a device allocation failed; the list of the pass stays as it was.  Code 12 is a refusal that leaves the
 * context untouched (as musc_side_prepare's): the longest loaded read has more than MUSC_MM_MAX_READ_LEN bases (the
 * flanks the lines are ordered by are compared base by base), WindowWidth is above that bound, MaxMatches is negative,
 * or there are 2^32 - 16 tuples or 2^30 - 2 suspect probes or more.  The caller keeps its host path then.
 * MUSC_DEBUG_MM_HEAP_LDS=<entries> (tests only, read by musc_init) lowers the LDS capacity of the replay kernel's heap,
 * so that the path with the heap in global memory runs at small MaxMatches.  MUSC_ABI_VERSION is unchanged: additions. */
#define MUSC_MM_MAX_READ_LEN 1024
int musc_maxmatches_apply(musc_ctx* ctx, int apply_mmtol, uint64_t* nhits, uint64_t* n_suspect_probes,
                          uint64_t* n_truncated_blocks);
/* HIP-event time of the last successful musc_maxmatches_apply (allocations included). */
int musc_maxmatches_last_ms(musc_ctx* ctx, float* ms);
/* Of the same call: the accepted pairs the truncated blocks held (what the replay kernel walked), and the HIP-event
 * time of that kernel, k_mm_replay, alone.  Either pointer may be NULL. */
int musc_maxmatches_last_detail(musc_ctx* ctx, uint64_t* n_pairs, float* ms_replay);

/* ---- several GPUs in one process (a Go host driving one ctx per GPU from locked threads):
 * concatenate the device-resident hits of ctxs[0..n) in rank order into one host array,
 * adding read_base[i] to the read_idx of shard i.  (The one-process-per-GPU path gathers
 * over RCCL instead: muscato_amd/dist.py.) */
int musc_gather(musc_ctx* const* ctxs, int n, const uint64_t* read_base, musc_hit** hits,
                uint64_t* nhits);
/* The same over RCCL: the tuples of ctxs[1..n) travel to ctxs[0]'s GPU over xGMI (ncclSend /
 * ncclRecv, all of them in one ncclGroupStart/End so that the links run side by side), are
 * rebased there and leave the node's GPUs in ONE device-to-host copy -- the concatenation step
 * of the reference (combineWindows, cmd/muscato/main.go:422-505) without N host copies.  One
 * clique per device list is created on first use (ncclCommInitAll) and kept for the process.
 * librccl is loaded at run time on the first call with n > 1: a return code of 20 means it
 * could not be used (the text says why) and musc_gather is the alternative.  The contexts must
 * sit on distinct devices. */
int musc_gather_rccl(musc_ctx* const* ctxs, int n, const uint64_t* read_base, musc_hit** hits,
                     uint64_t* nhits);
/* Whether musc_gather_rccl can load librccl in this process: 0 = yes, 20 = no, with the reason
 * copied into msg (at most cap bytes, NUL-terminated; msg may be NULL).  Needs no GPU.  The library
 * is looked up once per process: MUSC_RCCL_LIB names it, else the ROCm tree's, else the loader's. */
int musc_rccl_probe(char* msg, uint64_t cap);

/* ---- the gene file from its raw bytes (additions; MUSC_ABI_VERSION is unchanged) -----------------------------------
 * The reference writes GeneFileName through snappy's framed writer (cmd/muscato_prep_targets/main.go:246-258) and reads
 * it back under bufio.ScanLines (cmd/muscato_screen/main.go:408-452).  These two calls do on the device what the host
 * chain slurp -> sz_decode -> split_lines -> cut at the first tab -> concat -> musc_db_load_ascii does.
 *
 * musc_sz_decode: `bytes` is a framed snappy stream in host memory.  *nout = the decoded length; dst == NULL only
 * sizes (the chunk headers are walked, no block is decoded).  Otherwise the decoded bytes go to dst (host, or device at
 * any alignment when dst_on_device != 0), capacity >= *nout bytes.  A failed call leaves dst as it was.
 *
 * musc_db_load_text: `bytes` is the raw gene file.  framed = 1: a framed stream; 0: plain text; -1: a framed stream
 * exactly when it begins with the ten-byte stream identifier.  A framed stream must be a host pointer (on_device != 0
 * with one: 2).  Plain text may be a device pointer at any alignment; bytes outside [bytes, bytes + nbytes) are never
 * read.  Lines are bufio's: a line ends at '\n', one trailing '\r' is dropped, an unterminated last line is kept,
 * there is no empty line after a final '\n'.  The target is the line up to its first tab (a '\r' in front of that
 * tab is data).  Afterwards the context holds exactly the database musc_db_load_ascii holds for those targets.
 *
 * Codes: 2 bad arguments, and no line at all ("database has no sequences"); 10 a HIP failure ("out of memory" in the
 * text when an allocation failed); 12 a refusal: a chunk declares more than 65 536 uncompressed bytes, which the
 * framing format forbids (the caller falls back to its host decoder); 13 a bad stream: a framing, block or checksum
 * error -- the text names the chunk's index (counting every chunk of the stream from 0) and the error. */
typedef struct musc_db_text_info {
  uint64_t n_targets, n_bases;      /* lines, and bases over all of them                          */
  uint64_t n_odd;                   /* target bytes that are none of A C G T X                    */
  uint32_t first_odd_target, reserved;
  uint64_t n_text_bytes, n_chunks;  /* decoded text; data chunks of the stream (0 for plain text) */
  float ms_decode, ms_parse;        /* device time: frames -> text; text -> planes + seq_off      */
} musc_db_text_info;
int musc_sz_decode(musc_ctx* ctx, const uint8_t* bytes, uint64_t nbytes, uint8_t* dst, uint64_t capacity,
                   int dst_on_device, uint64_t* nout);
int musc_db_load_text(musc_ctx* ctx, const uint8_t* bytes, uint64_t nbytes, int on_device, int framed,
                      musc_db_text_info* out);

/* ---- target preparation from the raw file (additions; MUSC_ABI_VERSION is unchanged) --------------------------------
 * cmd/muscato_prep_targets/main.go turns a FASTA file (processFasta, :143-213) or id<TAB>sequence text (processText,
 * :82-141) into two texts -- the sequences, one per line, and the id lines "%011d\tname\tlen" -- and writes both through
 * snappy's framed writer (:246-258).  These calls do on the device what the host chain slurp -> split_lines -> concat
 * -> subx -> revcomp -> snprintf -> sz_encode does; the host functions stay the specification and the fallback.
 *
 * musc_targets_prep (replaces :82-213 with :48-80): `bytes` is the plain text, in host memory or (on_device != 0) in
 * device memory at any alignment; bytes outside [bytes, bytes + nbytes) are never read.  Lines are bufio's, as for
 * musc_db_load_text.  fasta = 0: the records are the lines in front of the first stop line -- a line that is empty or
 * does not hold exactly one tab; the name is what stands before the tab, the sequence what follows it, every byte that
 * is none of A C G T made X.  fasta = 1: an empty line fails the call (14); a line that begins with '>' is a header,
 * its record the lines up to the next header, its name the whole header line; lines in front of the first header form
 * a record with the empty name; a record without bases is dropped and takes no number; every record is substituted
 * EXCEPT the one that reaches the end of the input with bases (:204-212).  rev = 1: every record is followed by its
 * reverse complement (A<->T, C<->G, X->X, any other byte -> 0x00), named name_r; numbers count both strands.  The two
 * texts stay resident in the context until the next musc_targets_prep, musc_targets_prep_free or musc_destroy; no
 * other call touches them and they touch no other state.  A failed call leaves no prepared texts, those of an earlier
 * call included.  nbytes == 0 succeeds with two empty texts.
 *
 * musc_targets_prep_text: bytes [off, off + nbytes) of one text (which: 0 sequences, 1 ids) to dst -- host memory, or
 * device memory at any alignment; nothing outside [dst, dst + nbytes) is written.  A range beyond the text: 2.
 *
 * musc_targets_prep_load (replaces the write of :246-258 and the read back of cmd/muscato_screen/main.go:408-452): the
 * resident sequence text becomes the context's database, exactly as musc_db_load_text(on_device = 1, framed = 0) on
 * that buffer.  Without a prepared text: 2.  The prepared texts survive the load.
 *
 * musc_sz_frame (replaces snappy.NewBufferedWriter of :246-258): byte for byte the stream the host writer makes -- the
 * ten identifier bytes, then uncompressed chunks of 65 536 bytes, the last one shorter, each with the masked CRC-32C of
 * its data.  `bytes` in host or device memory at any alignment, dst likewise.  dst == NULL only sizes:
 * *nout = 10 + 8 * chunks + nbytes.  A failed call leaves dst as it was.
 *
 * Codes: 2 bad arguments (fasta or rev outside 0 / 1, a NULL pointer with bytes, a range or capacity that does not
 * fit); 10 a HIP failure ("out of memory" in the text when an allocation failed); 12 a refusal: 0xFFFFFFF0 targets or
 * more, both strands counted (the caller keeps its host chain); 14 a bad text:
 * "musc_targets_prep: empty line in FASTA input (line N)", N the 0-based number of the first empty line. */
typedef struct musc_targets_prep_info {
  uint64_t n_lines;       /* input lines                                                     */
  uint64_t n_records;     /* kept records (one strand)                                       */
  uint64_t n_targets;     /* lines of the sequence text = n_records * (rev ? 2 : 1)          */
  uint64_t n_dropped;     /* FASTA records without bases                                     */
  uint64_t stop_line;     /* text format: the first stop line, ~0 when the input ran out     */
  uint64_t n_subx;        /* bytes that subx changed                                         */
  uint64_t n_seq_bytes, n_id_bytes;
  float ms;               /* device time of the stage                                        */
  uint32_t reserved;
} musc_targets_prep_info;
int musc_targets_prep(musc_ctx* ctx, const uint8_t* bytes, uint64_t nbytes, int on_device, int fasta, int rev,
                      musc_targets_prep_info* out);
int musc_targets_prep_text(musc_ctx* ctx, int which, uint64_t off, uint64_t nbytes, uint8_t* dst, int dst_on_device);
int musc_targets_prep_load(musc_ctx* ctx, musc_db_text_info* out);
int musc_targets_prep_free(musc_ctx* ctx);
int musc_sz_frame(musc_ctx* ctx, const uint8_t* bytes, uint64_t nbytes, int on_device, uint8_t* dst, uint64_t capacity,
                  int dst_on_device, uint64_t* nout);

/* ---- The compressing writer (additions, MUSC_ABI_VERSION stays 3)
 *
 * musc_sz_compress: `bytes` as a framed snappy stream whose chunks (65 536 bytes of data, the last one shorter) are
 * compressed by the rule of csrc/sz_compress_plan.hpp, or stored where a chunk's block would take n - n / 8 bytes or
 * more: byte for byte what the host writer makes with MUSC_SZ_WRITE=compressed (host/sz.hpp, sz_encode_compressed).
 * musc_sz_decode, musc_db_load_text and golang/snappy's reader take the stream.  `bytes` and dst in host or device
 * memory at any alignment.  dst == NULL only sizes, and unlike musc_sz_frame's its answer is a bound, not the length:
 * *nout = 10 + 8 * chunks + nbytes, which no stream exceeds.  Otherwise capacity must be at least that bound, and
 * *nout = the stream's length.  Everything is allocated before a byte of dst is written: a failed call leaves dst as
 * it was.  Nothing outside [dst, dst + *nout) is written.
 *
 * musc_targets_prep_sz: a resident prepared text (which: 0 sequences, 1 ids) framed where it lies -- compressed = 1 as
 * musc_sz_compress, compressed = 0 as musc_sz_frame (dst == NULL sizes as that call does).  Without a prepared
 * text: 2.
 *
 * Codes: 2 bad arguments (a NULL pointer with bytes, a capacity below the bound, which or compressed outside 0 / 1,
 * no prepared text); 10 a HIP failure ("out of memory" in the text when an allocation failed). */
int musc_sz_compress(musc_ctx* ctx, const uint8_t* bytes, uint64_t nbytes, int on_device, uint8_t* dst, uint64_t capacity,
                     int dst_on_device, uint64_t* nout);
int musc_targets_prep_sz(musc_ctx* ctx, int which, int compressed, uint8_t* dst, uint64_t capacity, int dst_on_device,
                         uint64_t* nout);

#ifdef __cplusplus
}
#endif
#endif /* MUSCATO_HIP_H */
