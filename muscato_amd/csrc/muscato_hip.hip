// libmuscato_hip.so -- muscato's seed-and-extend hot path on MI355X (gfx950, wave64).
//
// Path (reference file:line, kshedden/muscato):
//   screen : cmd/muscato_screen/main.go:116-207 (read k-mer sketch), :256-366 (target scan)
//   join   : cmd/muscato/main.go:318-385 (sort) + cmd/muscato_confirm/main.go:375-416 (merge)
//   confirm: cmd/muscato_confirm/main.go:151-159 (cdiff), :171-250 (searchpairs)
//   select : cmd/muscato_combine_windows/main.go:36-60 (per-read best + MMTol)
//
// MI355X design: the target database stays resident in HBM as one 2-bit
// stream plus a k-mer -> (gene, offset) table of 64-byte buckets built once per (database,
// WindowWidth); reads are fixed-stride 2-bit records.  One pass = k_screen (window keys probe
// the table, candidates filtered from the index entry alone) -> k_confirm (XOR/popcount Hamming
// distance, then per-read best + MMTol and MaxMatches accounting in the same workgroup; bound by
// the cache lines it gathers) -> tile scan -> k_compact (tuples in read order).  Read prep
// (bytewise sort + collapse, muscato_prep.hpp) is a separate entry point.  The Bloom sketch of
// the reference only prunes work and cannot change results
// (SURVEY.md 8a note H): every candidate is verified exactly in k_confirm, including its
// window key.
//
// There is no CPU fallback in this library.

#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rccl/rccl.h>  // types and prototypes only: the library is resolved at run time (rccl_api)
#include <dlfcn.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/muscato_hip.h"
#include "../../include/muscato_sam.h"
#include "../../include/muscato_cov.h"

#include "ctx_state.hpp"
#include "dev_mem.hpp"
#include "index_plan.hpp"
#include "launch_plan.hpp"
#include "load_plan.hpp"

#include "kernels_common.hpp"
#include "kernels_index.hpp"
#include "kernels_screen.hpp"
#include "kernels_confirm.hpp"
#include "kernels_match.hpp"
#include "kernels_match_lane_inst.hpp"  // k_match_t: declaration only (defined in match_lane_rw*.hip)
#include "kernels_screen_lane.hpp"
#include "kernels_partition.hpp"
#include "kernels_results.hpp"
#include "side_names.hpp"
#include "kernels_side.hpp"
#include "kernels_sam.hpp"
#include "kernels_cov.hpp"
#include "kernels_maxmatches.hpp"
#include "kernels_fastq.hpp"
MUSC_LANE_INSTANCES_4(extern)
MUSC_LANE_INSTANCES_8(extern)
MUSC_LANE_INSTANCES_12(extern)
MUSC_LANE_INSTANCES_8W(extern)
MUSC_LANE_INSTANCES_12W(extern)
MUSC_LANE_INSTANCES_16W(extern)
MUSC_LANE_INSTANCES_SPEC(extern)
MUSC_DMA_INSTANCES(extern)

// ------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------

namespace {

thread_local std::string g_init_error;  // musc_init may run on one host thread per GPU

// roctx ranges around the kernel families (the reference's tracing hook is the
// CPUProfile flag, cmd/muscato_screen/main.go:530-538): visible in `rocprofv3 --marker-trace`.
// The marker library is resolved at run time; without it the ranges are no-ops.
struct Roctx {
  int (*push)(const char*) = nullptr;
  int (*pop)() = nullptr;
  Roctx() {
    for (const char* name : {"librocprofiler-sdk-roctx.so.1", "librocprofiler-sdk-roctx.so", "libroctx64.so.4", "libroctx64.so"}) {
      if (void* h = dlopen(name, RTLD_NOW | RTLD_LOCAL)) {
        push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
        pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
        if (push && pop) return;
        push = nullptr;
        pop = nullptr;
      }
    }
  }
};
const Roctx& roctx() {
  static const Roctx r;
  return r;
}
struct Range {
  bool on;
  explicit Range(const char* name) : on(roctx().push != nullptr) {
    if (on) (void)roctx().push(name);
  }
  ~Range() {
    if (on) (void)roctx().pop();
  }
};

// A stream capture in progress is ended on every exit path: an early return between
// hipStreamBeginCapture and hipStreamEndCapture would leave the stream capturing, and every later
// call on the context would fail until it is destroyed.
struct CaptureGuard {
  hipStream_t st = nullptr;
  bool active = false;
  hipError_t begin(hipStream_t s) {
    const hipError_t e = hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal);
    if (e == hipSuccess) {
      st = s;
      active = true;
    }
    return e;
  }
  hipError_t end(hipGraph_t* g) {
    active = false;
    return hipStreamEndCapture(st, g);
  }
  ~CaptureGuard() {
    if (!active) return;
    hipGraph_t g = nullptr;
    (void)hipStreamEndCapture(st, &g);
    if (g) (void)hipGraphDestroy(g);
    (void)hipGetLastError();
  }
};

}  // namespace

// the size rules of the loaders (load_plan.hpp): the record shape, and the schedule of a streamed load, which the pass
// that consumes it follows
using musc_load::RecShape;
using musc_load::StreamPlan;
using musc_load::stream_plan;
using musc_load::stream_plan_batch;

// The MUSC_* environment knobs (tests, A/B runs, experiments), read ONCE per context at musc_init -- a pass
// never calls getenv -- and again only on musc_reload_env (tests that flip a knob on a live context).
// (MUSC_INDEX, MUSC_DEBUG_INDEX_BITS, MUSC_DEBUG_CTX_DIRECT and MUSC_DEBUG_INDEX_BUDGET_MB are musc_index::Knobs: what the
// index decisions of index_plan.hpp read)
struct EnvKnobs : musc_index::Knobs {
  bool match_dma = false;     // MUSC_MATCH = dma: k_match_g (kernels_match_dma.hpp) where it is built for the run, k_match_t elsewhere
  bool screen_wg = false;     // MUSC_SCREEN = wg: k_screen on line buckets instead of k_screen_t
  int context = 0;            // MUSC_CONTEXT = narrow (1) | wide (2)
  bool no_x_context = false;  // MUSC_NO_X_CONTEXT
  bool force_wide = false;    // MUSC_DEBUG_FORCE_WIDE
  int debug_grid = 0;         // MUSC_DEBUG_GRID (0: not set)
  bool debug_sync = false;    // MUSC_DEBUG_SYNC
  int graph = -1;             // MUSC_GRAPH: -1 not set, else its value
  bool pipeline = false;      // MUSC_PIPELINE > 0
  bool no_spec = false;       // MUSC_NO_SPEC: never pick a geometry-specialised kernel instance
  long batch_reads = 0;       // MUSC_BATCH_READS (0: not set)
  uint64_t stage_bytes = 64ull << 20;  // MUSC_DEBUG_STAGE_BYTES: device staging of a text call for a host destination (tests)
  uint64_t stage_lines = 1ull << 20;   // MUSC_DEBUG_STAGE_LINES: record offsets such a call fetches to the host at a time (tests)
  long mm_heap_lds = 0;                // MUSC_DEBUG_MM_HEAP_LDS: LDS heap entries of k_mm_replay, lowered (tests; 0: not set)
  uint64_t stage_grid = 0;             // MUSC_DEBUG_STAGE_GRID: the cap of every stage grid, lowered (tests; 0: not set)
  void read() {
    *this = EnvKnobs();
    auto is = [](const char* v, const char* w) { return v && !strcmp(v, w); };
    const char* e = getenv("MUSC_INDEX");
    index = is(e, "classic") ? musc_index::IDX_CLASSIC : is(e, "lines") ? musc_index::IDX_LINES : is(e, "classic64") ? musc_index::IDX_CLASSIC64 : musc_index::IDX_AUTO;
    e = getenv("MUSC_MATCH");
    match_dma = is(e, "dma");
    screen_wg = is(getenv("MUSC_SCREEN"), "wg");
    e = getenv("MUSC_CONTEXT");
    context = is(e, "narrow") ? 1 : is(e, "wide") ? 2 : 0;
    no_x_context = getenv("MUSC_NO_X_CONTEXT") != nullptr;
    force_wide = getenv("MUSC_DEBUG_FORCE_WIDE") != nullptr;
    if ((e = getenv("MUSC_DEBUG_INDEX_BITS"))) index_bits = atoi(e);
    ctx_direct = (e = getenv("MUSC_DEBUG_CTX_DIRECT")) && atoi(e) > 0;
    if ((e = getenv("MUSC_DEBUG_GRID"))) debug_grid = atoi(e);
    debug_sync = getenv("MUSC_DEBUG_SYNC") != nullptr;
    if ((e = getenv("MUSC_GRAPH"))) graph = atoi(e);
    if ((e = getenv("MUSC_PIPELINE"))) pipeline = atoi(e) > 0;
    no_spec = getenv("MUSC_NO_SPEC") != nullptr;
    if ((e = getenv("MUSC_BATCH_READS"))) batch_reads = atol(e);
    if ((e = getenv("MUSC_DEBUG_INDEX_BUDGET_MB"))) index_budget_mb = atol(e);
    if ((e = getenv("MUSC_DEBUG_STAGE_BYTES")) && atoll(e) > 0) stage_bytes = (uint64_t)atoll(e);
    if ((e = getenv("MUSC_DEBUG_STAGE_LINES")) && atoll(e) > 0) stage_lines = (uint64_t)atoll(e);
    if ((e = getenv("MUSC_DEBUG_MM_HEAP_LDS"))) mm_heap_lds = atol(e);
    if ((e = getenv("MUSC_DEBUG_STAGE_GRID")) && atoll(e) > 0) stage_grid = std::min<uint64_t>((uint64_t)atoll(e), musc_launch::KNOB_MAX);
  }
};

struct musc_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  EnvKnobs env;
  // what is still valid (ctx_state.hpp); the caches of a pass below carry st.g.pass_inputs (in a PassKey, or as `gen`)
  musc_state::State st;

  // database
  DevPtr<uint32_t> db2;
  DevPtr<uint32_t> dbm2;     // null when the database holds no X (or an all-zero plane made for reads that do)
  bool db_has_x = false;     // the database holds an X
  bool reads_have_x = false; // some loaded read holds an X
  // reads with X on context buckets (k_match_t<.., XM = 1 | 2>): where each read's X are (k_read_xpos), and
  // whether the reads in hand fit that form under a given mismatch budget (k_xpos_check), cached
  DevBuf<uint32_t> rdx;
  struct { uint64_t gen = 0; int wide = -1; } rdx_of;  // wide: the format of rdx, XPos<false> or XPos<true>
  struct { uint64_t gen = 0; double pmatch = -1.0; int32_t mmp1 = -1; bool ok = false; } xok;
  DevPtr<uint32_t> dbx;      // with dbm2: one bit per 64-base block that holds an X
  uint64_t max_tlen = 0;     // longest target (context buckets flag an entry in bit 31 of its position)
  // a database with X on context buckets (k_match_t<.., XM = 2>): whether the reads in hand keep their X
  // out of the run's windows and within their xpos words (k_xpos_check_db), cached per read set and windows
  struct { uint64_t gen = 0; int32_t key[CTX_MAX_W + 3] = {0}; bool ok = false; } xokdb;
  DevPtr<uint64_t> seq_off;
  uint32_t nseq = 0;
  uint64_t nbases = 0;
  uint64_t db_words = 0;
  std::vector<uint64_t> h_seq_off;  // seq_off on the host: the partition planner cuts at target boundaries

  // Partitions: a database whose index does not fit is matched one range of whole targets at a time;
  // the packed database stays resident, each range's index is built in turn and the tuples are merged on the device
  uint64_t part_bases = 0;           // musc_db_set_partition_bases: most bases per partition, 0 = automatic
  std::vector<uint32_t> part_first;  // the plan of the last pass: partition p = targets [part_first[p], part_first[p + 1])
  musc_index::Kind part_kind = musc_index::K_CLASSIC64;  // several partitions: the index kind all of them build, settled on the largest
  uint64_t part_size = 0;            // bases of the largest partition: the size-dependent choices are made on it
  uint32_t cur_part = 0;             // the partition ensure_index builds
  // (the buffers of the merge below live for one partitioned pass: match_partitioned releases them)
  DevBuf<musc_hit> pacc;             // the partitions' tuple lists, appended segment after segment
  DevBuf<uint32_t> pbest;            // per read: fewest mismatches over the partitions so far
  DevBuf<uint64_t> pcnt, padj;       // per read: survivors -> output cursor; run offset of the segment in hand
  DevBuf<uint32_t> pflags, pflags_tmp;  // one segment's survivor flags and their scan
  DevBuf<uint32_t> block_acc;        // the exact MaxMatches block counters summed over the partitions

  // index (muscato_index.hpp)
  musc_index::Resident idx;  // the index in hand: kind, width, table shape and the targets it covers; ww == 0: none
  int wide = 0;  // database >= 2^32 bases: 40-bit positions, gene numbers < 2^24
  // only one kind is resident at a time: the window-start index (2^bits + 1 Bucket or LineBucket, uint4 overflow
  // entries) or context buckets (CtxBucket, CtxEntry / CtxEntryW: kernels_match.hpp)
  DevMem idx_T, idx_E, ctx_T, ctx_E;  // (DevMem::grow: exact sizes -- DevBuf's growth by half is wrong for a 64 GiB table)
  unsigned scrt_resident = 0;  // k_screen_t: waves resident at once (queried once per record stride)
  int scrt_rw = 0;
  uint64_t idx_novf = 0;    // overflow entries of the index in hand
  DevPtr<PathParams> d_pp;      // k_screen / k_confirm / k_hot_probes: the run's parameters
  PathParams h_pp;              // what d_pp holds
  bool h_pp_valid = false;
  DevPtr<MatchParams> d_mp;     // k_match's parameter block
  MatchParams h_mp;             // what d_mp holds
  bool h_mp_valid = false;
  int spec_geom = 0;            // the geometry-specialised k_match_t instance this pass launches (SpecGeom<n>), 0 = the general one
  DevBuf<uint4> spill;          // k_match: reported candidates beyond a tile's LDS list

  // reads: nreads, rw and max_len are committed together, with the records allocated (reads_records)
  DevPtr<uint32_t> rd;
  uint64_t rd_cap = 0;      // bytes of rd when a fixed-length load made it (kept from load to load), 0: sized for the reads in hand
  DevPtr<uint32_t> rdm;     // null when no read holds an X
  uint64_t nreads = 0;
  int rw = 0;
  uint32_t max_len = 0;
  bool reads_failed = false;  // the last load failed: no pass until one succeeds

  // musc_reads_load_packed32(async): reads of one length on their way from the host -- the 2-bit
  // stream goes to `stage` in pieces on the copy stream s_up, an event per piece; a pass packs the
  // records of a batch (k_pack_reads_fixed) when the batch's pieces have arrived.  stream_plan decides
  // the pieces and the batches of the pass that consumes them.
  struct Upload {
    DevPtr<uint32_t> stage;            // (grown when a load needs more, never shrunk)
    hipStream_t s_up = nullptr;
    std::vector<hipEvent_t> ev;
    StreamPlan plan;                   // piece ends and batch ends of this upload, in reads
    uint64_t next_piece = 0;           // the first piece whose records are still missing
    uint64_t packed_upto = 0;          // reads whose records exist
    uint32_t L = 0;
    bool active = false;               // records are still missing
  } up;

  // per-batch work buffers
  // what k_screen hands to k_confirm, twice: in a pipelined pass k_screen fills one set on the
  // screen stream while k_confirm and k_compact drain the other on the confirm stream
  struct BatchSet {
    DevBuf<uint32_t> wb, rvalid, tbase, tcount;
    DevBuf<uint4> cdesc;
  } bs[2];
  int cur = 0;                     // the set the next launches use
  hipStream_t stream2 = nullptr;   // confirm stream of a pipelined pass
  hipStream_t s_confirm = nullptr; // where k_confirm .. k_advance go in the pass in flight
  hipEvent_t ev_ready[2] = {nullptr, nullptr}, ev_free[2] = {nullptr, nullptr}, ev_join = nullptr;
  DevBuf<uint32_t> scan_tmp, tcount2, tpre;
  DevBuf<uint4> stage;
  DevBuf<uint32_t> p_nx;
  DevBuf<uint16_t> nmiss_tab;
  DevBuf<uint32_t> block_table;
  bool force_exact_blocks = false;
  // the MaxMatches screening of these reads, database and parameters was inconclusive once: later passes over the same
  // combination start with the exact per-block counters instead of screening, failing and repeating
  struct { musc_state::PassKey key; } exact;
  PathParams last_pp;          // of the last musc_match_device
  uint32_t last_max_matches = 0;
  uint32_t last_inst[MUSC_INSTANCE_WORDS] = {0, 0, 0, 0};  // musc_last_instance: what the resolvers of the last pass returned
  bool last_exact_blocks = false;  // block_table holds exact counters of that pass
  DevPtr<unsigned long long> counters;     // CNT_WORDS u64: the pass block and the batch block (kernels_common.hpp)
  PinnedPtr<uint64_t> h_pinned;            // their pinned mirror ...
  PinnedWords scalars;                     // ... and, between passes, the words a Readback brings scalars back through

  DevBuf<musc_hit> hits;
  uint64_t nhits = 0;
  DevBuf<uint64_t> packed;      // staging of musc_hits_copy_packed / musc_hits_unpack for host pointers
  std::vector<hipEvent_t> dl_ev;  // download_chunks: one event per chunk
  DevBuf<musc_hit> gathered;    // musc_gather_rccl: every context's tuples on this device
  DevPtr<uint32_t> d_flag;      // one device word for kernels that report "does not fit"

  // results.txt on the device: the texts the lines quote, and the ordered list of the last
  // musc_results_order with its line offsets (valid: st.ordered_current())
  DevPtr<char> res_gtext;           // every gene's name\tlen (musc_results_set_gene_text); released with the database
  DevPtr<uint64_t> res_goff;        // nseq + 1 byte offsets into it
  DevPtr<uint32_t> res_rank;        // per gene: rank of its text among all genes' texts, RES_ABSENT without an id line
  DevPtr<char> res_ttext;           // every read's count\tnames (musc_results_set_read_text); released with the reads
  DevPtr<uint64_t> res_toff;        // nreads + 1 byte offsets into it
  DevPtr<uint64_t> rn_loff;         // nreads + 1 byte offsets of the lines seq\tcount\tnames\n, when the read-name stage made the text
  float rn_ms_text = 0;             // event time of the musc_reads_names_text calls that rendered
  DevBuf<musc_hit> res_hits;        // the ordered tuples
  DevBuf<uint64_t> res_off;         // res_n + 1 line offsets
  DevBuf<unsigned char> res_stage;  // musc_results_text: the bytes on their way to a host buffer
  uint64_t res_n = 0, res_bytes = 0;
  float res_ms_order = 0, res_ms_text = 0;

  // the side outputs on the device: what musc_side_prepare leaves for musc_side_text (valid: st.may_side_text())
  DevPtr<uint32_t> side_nrank;      // per gene: rank of its name among all names, RES_ABSENT without an id line
  DevPtr<uint2> side_names;         // per name rank: a gene with that name, the name's bytes
  uint32_t side_nnames = 0;
  bool side_form_ok = false;        // every present gene's text is name\tlen in the simple form
  uint32_t side_bad_gene = 0;       // the first gene whose text is not
  DevBuf<uint4> side_tok;           // per read: count span and token span of its tail
  DevBuf<uint32_t> side_cnt;        // per name rank: kept tuples
  DevBuf<uint32_t> side_idx[2];     // nonmatch: the reads of the records; genestats: the name ranks of the lines
  DevBuf<uint64_t> side_off[3];     // per text: nrec + 1 byte offsets
  DevBuf<uint64_t> side_el, side_eloff;       // readstats: run << 32 | name rank per element, nel + 1 byte offsets
  DevBuf<uint32_t> side_first, side_runread;  // readstats: per run its first element, its first read
  uint64_t side_nel = 0;
  uint64_t side_nrec[3] = {0, 0, 0}, side_nbytes[3] = {0, 0, 0};
  float side_ms_prepare = 0, side_ms_text = 0;

  // SAM output on the device: what musc_sam_prepare leaves for musc_sam_text (valid: st.may_sam_text())
  DevBuf<uint4> sam_tok;            // per read: bytes of the count, QNAME's first byte within the tail and its bytes
  DevBuf<uint2> sam_gname;          // per gene: the RNAME token's first byte within its text and its bytes
  DevBuf<uint4> sam_info;           // per line: NM, bytes of MD, NH, HI
  DevBuf<uint64_t> sam_off, sam_hoff;  // res_n + 1 record offsets; nseq + 3 offsets of the header's slots
  uint64_t sam_n = 0, sam_bytes = 0, sam_hbytes = 0;
  uint32_t sam_rev = 0;
  float sam_ms_prepare = 0, sam_ms_text = 0;

  // coverage on the device: what musc_cov_prepare leaves for musc_cov_text (valid: st.may_cov_text())
  DevBuf<uint2> cov_gname;                     // per gene: the RNAME token, as sam_gname (SAM's own stays untouched)
  DevBuf<uint32_t> cov_run_f, cov_run_d;       // per run: its target, its depth
  DevBuf<uint64_t> cov_run_s, cov_run_e;       // ... its first base and the one behind its last
  DevBuf<uint64_t> cov_off, cov_soff;          // cov_nruns + 1 offsets of the bedGraph records; cov_nt + 1 of the summary's
  DevBuf<uint32_t> cov_target;                 // per summary record: its target
  DevBuf<uint32_t> cov_numreads, cov_maxdepth; // per target
  DevBuf<uint64_t> cov_covbases, cov_sumdepth;
  uint64_t cov_nruns = 0, cov_bytes = 0, cov_nt = 0, cov_sbytes = 0;
  uint32_t cov_flags = 0;
  float cov_ms_prepare = 0, cov_ms_text = 0;

  // the MaxMatches replay on the device
  musc_params mm_params;            // of the last musc_match* that succeeded (its list may be replayed: st.may_replay())
  float mm_ms = 0, mm_ms_replay = 0;  // event time of the last musc_maxmatches_apply; of its k_mm_replay
  uint64_t mm_pairs = 0;            // pairs in the blocks which that call truncated

  // target preparation on the device: the two texts of the last musc_targets_prep (0 sequences, 1 ids),
  // until the next one, musc_targets_prep_free or musc_destroy; no other call touches them
  DevPtr<unsigned char> tp_text[2];
  uint64_t tp_bytes[2] = {0, 0};
  bool tp_have = false;

  uint32_t batch_reads = 16u << 20;
  // A pass over the same reads, database and parameters as the last completed one needs no
  // sizing: its buffers are known to suffice, so it runs without host round trips.
  struct { musc_state::PassKey key; uint32_t bsz = 0; } sized;  // of the last completed pass (block_mode: 2 or 0); its reads per batch
  musc_stats stats;
  // MUSC_GRAPH=1: the sized pass on context buckets as a hipGraph (one launch instead of seven per
  // batch; no per-kernel timing in that mode)
  struct {
    hipGraphExec_t exec = nullptr;
    musc_state::PassKey key;
    uint32_t batches = 0;
    bool failed = false;  // capture or instantiation failed once: sized passes run launch by launch
    void drop() { if (exec) (void)hipGraphExecDestroy(exec); exec = nullptr; }
  } graph;
  // timing events are created once and reused by every pass (creating and destroying a pair per
  // kernel family per batch cost more than the kernels of a small pass)
  std::vector<hipEvent_t> ev_pool;
  size_t ev_used = 0;
  // the mismatch-budget table on the device is valid for these inputs
  struct { double pmatch = -1.0; int32_t mmp1 = -1; uint32_t maxlen = 0xFFFFFFFFu; } nm;
  musc_state::PassKey pass_key(const musc_params& P, int block_mode) const { return musc_state::PassKey{st.g.pass_inputs, P, block_mode}; }
};

// p[i] = i: the item numbers a sort by key passes starts from (KeyPasses)
MUSC_KERNEL void k_prep_iota(uint32_t* __restrict__ p, uint64_t n) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
    p[i] = (uint32_t)i;
}

namespace {

int fail(musc_ctx* c, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (c) c->err = buf; else g_init_error = buf;
  return code;
}

// (a failed call also leaves its error as the thread's last error: cleared here, so that the next call on the
// context -- a smaller plan after an index that did not fit -- does not report it again)
#define HIPCHK(c, expr)                                                                 \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess) {                                                             \
      (void)hipGetLastError();                                                          \
      return fail((c), 10, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    }                                                                                   \
  } while (0)

template <class T>
int ensure(musc_ctx* c, DevBuf<T>& b, uint64_t n, bool keep = false) {
  if (n <= b.cap && b.p) return 0;
  const uint64_t ncap = grown_cap(n, b.cap);
  T* np = nullptr;
  HIPCHK(c, hipMalloc((void**)&np, grown_bytes(ncap, sizeof(T))));
  if (keep && b.p && b.cap) {
    hipError_t e = hipMemcpyAsync(np, b.p, b.cap * sizeof(T), hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
      (void)hipFree(np);
      return fail(c, 10, "hit buffer grow failed: %s", hipGetErrorString(e));
    }
  }
  b.release();
  b.p = np;
  b.cap = ncap;
  return 0;
}

// blocks of b threads covering n elements; a dispatch must stay below 2^32 work-items, callers
// with potentially larger n use grid-stride kernels instead
inline unsigned nblk(uint64_t n, unsigned b) { return (unsigned)((n + b - 1) / b); }

// The grid of a persistent stage kernel (launch_plan.hpp): `wanted` blocks under the launch's cap, or under
// MUSC_DEBUG_STAGE_GRID.  Every capped launch of the host drivers but the pass's own (muscato_pass.hpp) comes through here.
static_assert(musc_launch::CAP_GRID == MAX_GRID && musc_launch::SCAN_TILE_ELEMS == SCAN_TILE, "launch_plan.hpp restates two constants of kernels_common.hpp");
inline dim3 stage_grid(const musc_ctx* c, uint64_t wanted, uint64_t cap) { return dim3(musc_launch::stage_blocks(wanted, cap, c->env.stage_grid)); }

// the grid of a grid-stride kernel over k items
inline dim3 grid(const musc_ctx* c, uint64_t k) { return stage_grid(c, (k + 255) / 256, musc_launch::CAP_GRID); }

// ---- what the host drivers share: the scans, tmp_alloc / staged, KeyPasses; Readback is dev_mem.hpp's

using musc_launch::scan_tmp_elems;  // (the scratch plan of the recursion below: launch_plan.hpp)

// The host recursion of both scans: `top` scans the tiles of the level in hand and leaves their sums in tmp, which are
// scanned in turn (exclusive, by `below`) and added back.
template <class T>
int scan_levels(musc_ctx* c, const T* in, T* out, uint64_t n, T* tmp, hipStream_t st, void (*top)(const T*, T*, T*, uint64_t),
                void (*below)(const T*, T*, T*, uint64_t), void (*add)(T*, const T*, uint64_t)) {
  const uint64_t nb = musc_launch::scan_tiles(n);
  if (nb > 0x7FFFFFFFull) return fail(c, 11, "scan too large");
  T* const sums = nb <= 1 ? nullptr : tmp;
  hipLaunchKernelGGL(top, dim3(sums ? (unsigned)nb : 1u), dim3(SCAN_BLOCK), 0, st, in, out, sums, n);
  HIPCHK(c, hipGetLastError());
  if (!sums) return 0;
  const int rc = scan_levels(c, (const T*)sums, sums, nb, tmp + musc_launch::scan_next_level(nb), st, below, below, add);
  if (rc) return rc;
  hipLaunchKernelGGL(add, dim3((unsigned)nb), dim3(SCAN_BLOCK), 0, st, out, (const T*)sums, n);
  HIPCHK(c, hipGetLastError());
  return 0;
}

// u32 scan of n elements (in may equal out).  tmp must hold scan_tmp_elems(n).
int scan_u32(musc_ctx* c, const uint32_t* in, uint32_t* out, uint64_t n, bool inclusive, uint32_t* tmp, hipStream_t st = nullptr) {
  return scan_levels<uint32_t>(c, in, out, n, tmp, st ? st : c->stream, inclusive ? k_scan_block<true> : k_scan_block<false>, k_scan_block<false>, k_scan_add);
}

// exclusive u64 scan (in place allowed); tmp must hold scan_tmp_elems(n) u64
int scan_u64(musc_ctx* c, const uint64_t* in, uint64_t* out, uint64_t n, uint64_t* tmp) {
  return scan_levels<uint64_t>(c, in, out, n, tmp, c->stream, k_scan64_block, k_scan64_block, k_scan64_add);
}

// A temporary of the public call `who`: a failed device allocation is the library's code for a failed HIP call, and the
// text says whose, how large and why ("out of memory").
template <class T>
int tmp_alloc(musc_ctx* c, const char* who, TmpBufs& B, T** ptr, uint64_t bytes) {
  const hipError_t e = B.alloc(ptr, bytes);
  if (e == hipSuccess) return 0;
  (void)hipGetLastError();
  return fail(c, 10, "%s: device allocation of %llu bytes failed: %s", who, (unsigned long long)bytes, hipGetErrorString(e));
}

// An input of `bytes` bytes on the device: the caller's pointer where it is there already, else a temporary of B with
// `slack` spare bytes behind the input and the copy queued on the context's stream (*d_ptr is device memory either way).
template <class T>
int staged(musc_ctx* c, const char* who, TmpBufs& B, const T* ptr, uint64_t bytes, int on_device, uint64_t slack, const T** d_ptr) {
  *d_ptr = ptr;
  if (on_device) return 0;
  T* d = nullptr;
  const int rc = tmp_alloc(c, who, B, &d, bytes + slack);
  if (rc) return rc;
  if (bytes) HIPCHK(c, hipMemcpyAsync(d, ptr, bytes, hipMemcpyHostToDevice, c->stream));
  *d_ptr = d;
  return 0;
}

// The stable sort of n items by passes of 64-bit keys, least significant pass first: LSD over (key, item number) pairs
// with rocPRIM's device radix sort (a library primitive, not part of the hot path).  start() takes the buffers as
// temporaries of its own B, sized for the largest of the end bits the passes will name, and numbers the items;
// pass(end_bit, fill) has `fill(order, keys)` queue the kernel that writes keys[i] = the key of item order[i] and sorts
// bits [0, end_bit) of them (the end bit decides how many radix passes the primitive runs); order() is the permutation
// after the passes so far.  Everything is queued on the context's stream; nothing waits.
struct KeyPasses {
  TmpBufs B;  // (the caller may add temporaries that live as long as the sort's)
  int start(musc_ctx* ctx, const char* who, uint64_t items, std::initializer_list<unsigned> end_bits) {
    c = ctx, n = items;
    int rc;
    if ((rc = tmp_alloc(c, who, B, &k0, n * 8)) || (rc = tmp_alloc(c, who, B, &k1, n * 8)) || (rc = tmp_alloc(c, who, B, &p0, n * 4)) ||
        (rc = tmp_alloc(c, who, B, &p1, n * 4)))
      return rc;
    for (unsigned end : end_bits) {
      size_t tb = 0;
      HIPCHK(c, sort(nullptr, tb, end));
      tmp_bytes = std::max(tmp_bytes, tb);
    }
    if ((rc = tmp_alloc(c, who, B, &tmp, tmp_bytes))) return rc;
    hipLaunchKernelGGL(k_prep_iota, grid(c, n), dim3(256), 0, c->stream, p0, n);
    HIPCHK(c, hipGetLastError());
    return 0;
  }
  template <class Fill>
  int pass(unsigned end_bit, Fill fill) {
    fill((const uint32_t*)p0, k0);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, sort(tmp, tmp_bytes, end_bit));
    std::swap(p0, p1);
    return 0;
  }
  const uint32_t* order() const { return p0; }
  hipError_t sort(void* t, size_t& bytes, unsigned end_bit) {
    return rocprim::radix_sort_pairs(t, bytes, k0, k1, p0, p1, (size_t)n, 0u, end_bit, c->stream);
  }
  musc_ctx* c = nullptr;
  uint64_t n = 0;
  uint64_t *k0 = nullptr, *k1 = nullptr;
  uint32_t *p0 = nullptr, *p1 = nullptr;
  void* tmp = nullptr;
  size_t tmp_bytes = 0;
};

void free_index(musc_ctx* c);  // muscato_index.hpp

// the gene text of the results stage belongs to a database, the read text to a read set
void drop_gene_text(musc_ctx* c) {
  for (DevMem* m : std::initializer_list<DevMem*>{&c->res_gtext, &c->res_goff, &c->res_rank, &c->side_nrank, &c->side_names}) m->release();
  c->side_nnames = 0;
  c->side_form_ok = false;
  c->st.gene_text_dropped();
}
void drop_read_text(musc_ctx* c) {
  c->res_ttext.release();
  c->res_toff.release();
  c->rn_loff.release();
  c->st.read_text_dropped();
}

void free_db(musc_ctx* c) {
  free_index(c);
  drop_gene_text(c);
  for (DevMem* m : std::initializer_list<DevMem*>{&c->db2, &c->dbm2, &c->dbx, &c->seq_off}) m->release();
  c->db_has_x = false;
  c->nseq = 0;
  c->nbases = 0;
  c->h_seq_off.clear();
  c->part_first.clear();
  c->st.db_freed();
}

// Forget the reads in hand.  keep_rd: the record buffer stays allocated for the fixed-length load that follows
// (reads_load_fixed: a hipFree waits for the device, and freeing and allocating 1.4 GB again before every load kept
// the link idle at the start of each streamed step)
void drop_reads(musc_ctx* c, bool keep_rd) {
  if (c->up.active) {  // an upload nobody matched: the caller's buffer is borrowed until it ends
    (void)hipStreamSynchronize(c->up.s_up);
    c->up.active = false;
  }
  if (!(keep_rd && c->rd_cap)) {
    c->rd.release();
    c->rd_cap = 0;
  }
  c->rdm.release();
  drop_read_text(c);
  c->reads_have_x = false;
  c->reads_failed = false;
  c->nreads = 0;
  c->rw = 0;
  c->st.reads_dropped();
}
void free_reads(musc_ctx* c) { drop_reads(c, false); }

// The one rule for a load that failed, wherever it failed: nothing of it stays, and musc_match* answers 4, "no reads
// loaded", until a load succeeds.  (The message of the failure stays the context's last error.)
int reads_load_done(musc_ctx* c, int rc) {
  if (rc) {
    // (pieces of a fixed-length load, kernels and copies of the failed call may still be queued: none of them is when this returns)
    if (c->up.s_up) (void)hipStreamSynchronize(c->up.s_up);
    (void)hipStreamSynchronize(c->stream);
    free_reads(c);
    c->reads_failed = true;
  }
  return rc;
}

struct EvPair {
  hipEvent_t a, b;
};

// an event of the context's pool (created on first use, destroyed with the context)
hipEvent_t pool_event(musc_ctx* c) {
  if (c->ev_used == c->ev_pool.size()) {
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    c->ev_pool.push_back(e);
  }
  return c->ev_pool[c->ev_used++];
}

// Up to three points in time on the context's stream, for a call that reports the time between them: it starts from an
// empty pool, marks each point where it passes it, and reads a span once the stream has been waited for.
struct Marks {
  hipEvent_t e[3] = {nullptr, nullptr, nullptr};
  int start(musc_ctx* c) {
    c->ev_used = 0;
    for (hipEvent_t& x : e)
      if (!(x = pool_event(c))) return fail(c, 10, "hipEventCreate failed");
    return 0;
  }
  hipError_t mark(musc_ctx* c, int i) const { return hipEventRecord(e[i], c->stream); }
  float ms(int a, int b) const {
    float t = 0;
    (void)hipEventElapsedTime(&t, e[a], e[b]);
    return t;
  }
};

// `body()` between two such marks: *ms = the time between them.  The stream is waited for on every path, so nothing of
// a failed body is still queued when its temporaries go; *ms is written on success only.
template <class Body>
int timed(musc_ctx* c, float* ms, Body body) {
  Marks m;
  if (const int e = m.start(c)) return e;
  HIPCHK(c, m.mark(c, 0));
  const int rc = body();
  const hipError_t er = m.mark(c, 1);
  const hipError_t es = hipStreamSynchronize(c->stream);
  if (rc) return rc;
  HIPCHK(c, er);
  HIPCHK(c, es);
  *ms = m.ms(0, 1);
  return 0;
}

// HIP-event timing of the kernel families of one pass; the events belong to the context's pool
struct Timer {
  musc_ctx* c;
  bool off = false;  // while a pass is captured into a hipGraph no events are recorded
  std::vector<EvPair> ev[5];
  explicit Timer(musc_ctx* ctx) : c(ctx) { c->ev_used = 0; }
  int begin(int fam, hipStream_t s = nullptr) {
    if (off) return 0;
    EvPair p;
    p.a = pool_event(c);
    p.b = pool_event(c);
    if (!p.a || !p.b) return 1;
    (void)hipEventRecord(p.a, s ? s : c->stream);
    ev[fam].push_back(p);
    return 0;
  }
  void end(int fam, hipStream_t s = nullptr) {
    if (!off && !ev[fam].empty()) (void)hipEventRecord(ev[fam].back().b, s ? s : c->stream);
  }
  float total(int fam) {
    float t = 0;
    for (auto& p : ev[fam]) {
      float ms = 0;
      if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) t += ms;
    }
    return t;
  }
};

int check_params(musc_ctx* c, const musc_params* P) {
  if (!P) return fail(c, 2, "params is NULL");
  if (P->n_windows < 1 || P->n_windows > MUSC_MAX_WINDOWS)
    return fail(c, 2, "n_windows=%d outside 1..%d", P->n_windows, MUSC_MAX_WINDOWS);
  if (P->window_width < 1 || P->window_width > 4096) return fail(c, 2, "bad window_width=%d", P->window_width);
  for (int k = 0; k < P->n_windows; k++)
    if (P->windows[k] < 0 || P->windows[k] > 60000) return fail(c, 2, "bad window start %d", P->windows[k]);
  if (!(P->pmatch >= 0.0 && P->pmatch <= 1.0)) return fail(c, 2, "PMatch=%g outside [0,1]", P->pmatch);
  if (P->match_mode != 0 && P->match_mode != 1) return fail(c, 2, "match_mode must be 0 (best) or 1 (first)");
  if (P->mmtol < 0) return fail(c, 2, "MMTol < 0");
  if (P->max_mismatch_p1 < 0) return fail(c, 2, "max_mismatch_p1 < 0");
  return 0;
}

}  // namespace

extern "C" {

int musc_abi_version(void) { return MUSC_ABI_VERSION; }

const char* musc_last_error(musc_ctx* ctx) { return ctx ? ctx->err.c_str() : g_init_error.c_str(); }

int musc_init(int device_ordinal, musc_ctx** out) {
  if (!out) return fail(nullptr, 2, "musc_init: out is NULL");
  *out = nullptr;
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev == 0)
    return fail(nullptr, 3, "musc_init: no HIP device (%s); this library has no CPU fallback",
                e == hipSuccess ? "device count 0" : hipGetErrorString(e));
  if (device_ordinal < 0 || device_ordinal >= ndev)
    return fail(nullptr, 2, "musc_init: device %d outside 0..%d", device_ordinal, ndev - 1);
  hipDeviceProp_t prop;
  if ((e = hipGetDeviceProperties(&prop, device_ordinal)) != hipSuccess)
    return fail(nullptr, 3, "musc_init: hipGetDeviceProperties: %s", hipGetErrorString(e));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(nullptr, 3, "musc_init: device %d is %s; this library is built for gfx950 only",
                device_ordinal, prop.gcnArchName);
  if ((e = hipSetDevice(device_ordinal)) != hipSuccess)
    return fail(nullptr, 3, "musc_init: hipSetDevice: %s", hipGetErrorString(e));
  musc_ctx* c = new musc_ctx();
  c->device = device_ordinal;
  memset(&c->stats, 0, sizeof c->stats);
  if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess ||
      (e = hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking)) != hipSuccess ||
      (e = hipEventCreateWithFlags(&c->ev_ready[0], hipEventDisableTiming)) != hipSuccess ||
      (e = hipEventCreateWithFlags(&c->ev_ready[1], hipEventDisableTiming)) != hipSuccess ||
      (e = hipEventCreateWithFlags(&c->ev_free[0], hipEventDisableTiming)) != hipSuccess ||
      (e = hipEventCreateWithFlags(&c->ev_free[1], hipEventDisableTiming)) != hipSuccess ||
      (e = hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming)) != hipSuccess ||
      (e = c->counters.alloc(CNT_WORDS * sizeof(unsigned long long))) != hipSuccess ||
      (e = c->d_flag.alloc(4)) != hipSuccess ||
      (e = c->d_mp.alloc(sizeof(MatchParams))) != hipSuccess ||
      (e = c->d_pp.alloc(sizeof(PathParams))) != hipSuccess ||
      (e = c->h_pinned.alloc(CNT_WORDS * sizeof(uint64_t))) != hipSuccess) {
    fail(nullptr, 3, "musc_init: %s", hipGetErrorString(e));
    musc_destroy(c);
    return 3;
  }
  c->scalars.w = c->h_pinned;
  c->scalars.n = CNT_WORDS;
  c->env.read();
  if (c->env.batch_reads >= 1 && c->env.batch_reads <= (16l << 20)) c->batch_reads = (uint32_t)c->env.batch_reads;  // tests: many small batches
  *out = c;
  return 0;
}

// Re-read the MUSC_* knobs (musc_init reads them once; MUSC_BATCH_READS stays as it was read then).  A test hook:
// a knob that changes which index or kernel a pass takes makes the next pass size itself again, and a MUSC_GRAPH
// whose capture failed once is tried again.
int musc_reload_env(musc_ctx* c) {
  if (!c) return 1;
  c->env.read();
  c->sized.key = musc_state::PassKey();
  c->graph.failed = false;
  return 0;
}

void musc_destroy(musc_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  for (hipStream_t s : {c->stream, c->stream2})
    if (s) (void)hipStreamSynchronize(s);
  if (c->up.active && c->up.s_up) (void)hipStreamSynchronize(c->up.s_up);  // (an upload nobody matched)
  c->graph.drop();
  for (hipEvent_t ev : {c->ev_ready[0], c->ev_ready[1], c->ev_free[0], c->ev_free[1], c->ev_join})
    if (ev) (void)hipEventDestroy(ev);
  for (const std::vector<hipEvent_t>* v : {&c->ev_pool, &c->up.ev, &c->dl_ev})
    for (hipEvent_t ev : *v) (void)hipEventDestroy(ev);
  for (hipStream_t s : {c->up.s_up, c->stream2, c->stream})
    if (s) (void)hipStreamDestroy(s);
  delete c;  // (every buffer goes with its owner)
}

}  // extern "C"

// the loaders: databases and reads from packed or ASCII input, then from text (FASTQ; the gene file); target
// preparation from the raw FASTA or id<TAB>sequence file, whose sequence text the gene-file loader takes
#include "muscato_load.hpp"
#include "muscato_prep.hpp"
#include "muscato_db_text.hpp"
#include "muscato_targets_prep.hpp"
#include "muscato_sz_compress.hpp"

// the index layer: the build driver, eligibility, the partition planner, ensure_index, musc_db_build_index*
#include "muscato_index.hpp"

extern "C" {

// ---------------------------------------------------------------- hot path

static int match_partitioned(musc_ctx* c, const musc_params* P, uint64_t* nhits);

}  // extern "C"

// the pass driver and musc_match_device (C++: templates of kernel instances)
#include "muscato_pass.hpp"

extern "C" {

// A partitioned pass: for each partition in turn its index is built and the per-index pass runs over
// every read, with exact MaxMatches block counters (summed over the partitions, so that a block whose accepted pairs
// are split counts in full).  Each partition's read-major list is appended to `pacc` and folded into the per-read best;
// after the last one, the survivors of the global best + MMTol selection go read-major into `hits`.  The index of each
// partition is a new data epoch, so no sized-pass or hipGraph shortcut ever replays one partition's pass for another.
static int match_partitions_run(musc_ctx* c, const musc_params* P, uint64_t* nhits) {
  const uint32_t np = (uint32_t)c->part_first.size() - 1;
  const uint64_t nr = c->nreads;
  const bool check_blocks = !P->skip_block_check;
  const uint32_t BT = 1u << BLOCK_TABLE_BITS;
  int rc = 0;
  if ((rc = ensure(c, c->pbest, nr + 1))) return rc;
  HIPCHK(c, hipMemsetAsync(c->pbest.p, 0xFF, (nr + 1) * 4, c->stream));
  if (check_blocks) {
    if ((rc = ensure(c, c->block_acc, BT))) return rc;
    HIPCHK(c, hipMemsetAsync(c->block_acc.p, 0, (uint64_t)BT * 4, c->stream));
  }
  musc_stats sum;
  memset(&sum, 0, sizeof sum);
  std::vector<uint64_t> seg(np + 1, 0);
  for (uint32_t p = 0; p < np && !rc; p++) {
    c->cur_part = p;
    uint64_t nh = 0;
    if ((rc = ensure_index(c, P, c->max_len))) break;
    const float build_ms = c->stats.ms_index_build;
    if ((rc = match_index_pass(c, P, &nh))) break;
    const musc_stats& s = c->stats;
    sum.n_read_windows += s.n_read_windows;
    sum.n_candidates += s.n_candidates;
    sum.n_pairs += s.n_pairs;
    sum.n_accepted += s.n_accepted;
    sum.confirm_bytes += s.confirm_bytes;
    sum.confirm_launches += s.confirm_launches;
    sum.n_batches += s.n_batches;
    sum.ms_screen += s.ms_screen;
    sum.ms_scan += s.ms_scan;
    sum.ms_confirm += s.ms_confirm;
    sum.ms_select += s.ms_select;
    sum.ms_total += s.ms_total;
    sum.ms_index_build += build_ms;
    sum.n_descriptors += s.n_descriptors;
    sum.match_launches += s.match_launches;
    sum.n_overflow_entries += s.n_overflow_entries;
    sum.match_bytes += s.match_bytes;
    sum.match_bytes_strict += s.match_bytes_strict;
    sum.index_kind = s.index_kind;        // (equal for every partition: plan_partitions settles the kind)
    sum.match_variant = s.match_variant;
    sum.index_bytes = s.index_bytes;
    if (nh) {
      if ((rc = ensure(c, c->pacc, seg[p] + nh, true))) break;
      HIPCHK(c, hipMemcpyAsync(c->pacc.p + seg[p], c->hits.p, nh * sizeof(musc_hit), hipMemcpyDeviceToDevice, c->stream));
      hipLaunchKernelGGL(k_part_best, stage_grid(c, nblk(nh, 256), musc_launch::CAP_TILES), dim3(256), 0, c->stream,
                         reinterpret_cast<const uint4*>(c->pacc.p + seg[p]), nh, c->pbest.p);
      HIPCHK(c, hipGetLastError());
    }
    if (check_blocks) {
      hipLaunchKernelGGL(k_add_u32, dim3(nblk(BT, 256)), dim3(256), 0, c->stream, c->block_acc.p, c->block_table.p, (uint64_t)BT);
      HIPCHK(c, hipGetLastError());
    }
    seg[p + 1] = seg[p] + nh;
  }
  if (rc) return rc;

  // the merge: survivors per read -> output offsets -> each segment's survivors to their places, in partition order
  Range rg("partition merge");
  hipEvent_t ev0 = pool_event(c), ev1 = pool_event(c);
  if (!ev0 || !ev1) return fail(c, 10, "hipEventCreate failed");
  HIPCHK(c, hipEventRecord(ev0, c->stream));
  const uint64_t total_in = seg[np];
  const uint32_t mmtol = P->mmtol > 0xFFFF ? 0xFFFFu : (uint32_t)P->mmtol;
  uint64_t max_seg = 0;
  for (uint32_t p = 0; p < np; p++) max_seg = std::max(max_seg, seg[p + 1] - seg[p]);
  if (max_seg >= 0xFFFFFFFFull) return fail(c, 6, "one partition returned %llu tuples (>= 2^32)", (unsigned long long)max_seg);
  if ((rc = ensure(c, c->pcnt, nr + 1)) || (rc = ensure(c, c->padj, nr + 1)) ||
      (rc = ensure(c, c->pflags, max_seg + 1)) || (rc = ensure(c, c->pflags_tmp, scan_tmp_elems(max_seg + 1))))
    return rc;
  if (scan_tmp_elems(nr + 1) * 2 > c->pflags_tmp.cap && (rc = ensure(c, c->pflags_tmp, scan_tmp_elems(nr + 1) * 2)))
    return rc;  // (scan_u64 borrows it too, in u64 units)
  HIPCHK(c, hipMemsetAsync(c->pcnt.p, 0, (nr + 1) * 8, c->stream));
  if (total_in) {
    hipLaunchKernelGGL(k_part_count, stage_grid(c, nblk(total_in, 256), musc_launch::CAP_TILES), dim3(256), 0, c->stream,
                       reinterpret_cast<const uint4*>(c->pacc.p), total_in, c->pbest.p, mmtol, P->apply_mmtol,
                       reinterpret_cast<unsigned long long*>(c->pcnt.p));
    HIPCHK(c, hipGetLastError());
  }
  if ((rc = scan_u64(c, c->pcnt.p, c->pcnt.p, nr + 1, reinterpret_cast<uint64_t*>(c->pflags_tmp.p)))) return rc;
  Readback R(c->scalars, c->stream);
  uint64_t total = 0;
  HIPCHK(c, R.get(c->pcnt.p + nr, &total).wait());
  if ((rc = ensure(c, c->hits, total ? total : 1))) return rc;
  HIPCHK(c, hipMemsetAsync(c->d_flag, 0, 4, c->stream));
  for (uint32_t p = 0; p < np; p++) {
    const uint64_t n = seg[p + 1] - seg[p];
    if (!n) continue;
    const uint4* const h = reinterpret_cast<const uint4*>(c->pacc.p + seg[p]);
    const dim3 sgrid = stage_grid(c, nblk(n + 1, 256), musc_launch::CAP_TILES);
    hipLaunchKernelGGL(k_part_flags, sgrid, dim3(256), 0, c->stream, h, n, c->pbest.p, mmtol, P->apply_mmtol, c->pflags.p);
    HIPCHK(c, hipGetLastError());
    if ((rc = scan_u32(c, c->pflags.p, c->pflags.p, n + 1, false, c->pflags_tmp.p, c->stream))) return rc;
    hipLaunchKernelGGL(k_part_head, sgrid, dim3(256), 0, c->stream, h, n, c->pflags.p, c->pcnt.p, c->padj.p);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(k_part_scatter, sgrid, dim3(256), 0, c->stream, h, n, c->pflags.p, c->padj.p, c->pcnt.p,
                       reinterpret_cast<uint4*>(c->hits.p), total, c->d_flag);
    HIPCHK(c, hipGetLastError());
  }
  // the MaxMatches verdict of the whole database: the summed exact counters, then the usual count of full blocks
  if (check_blocks) {
    HIPCHK(c, hipMemcpyAsync(c->block_table.p, c->block_acc.p, (uint64_t)BT * 4, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(c->counters + CNT_OVF_BLOCKS, 0, 8, c->stream));
    hipLaunchKernelGGL(k_block_overflow, dim3(1024), dim3(256), 0, c->stream, c->block_table.p, c->last_max_matches, c->counters);
    HIPCHK(c, hipGetLastError());
  }
  HIPCHK(c, hipEventRecord(ev1, c->stream));
  uint64_t ovf_blocks = 0;
  uint32_t overran = 0;
  HIPCHK(c, R.get(c->counters + CNT_OVF_BLOCKS, &ovf_blocks).get(c->d_flag.get(), &overran).wait());
  if (overran) return fail(c, 12, "internal: the partition merge overran its %llu tuples", (unsigned long long)total);
  float merge_ms = 0;
  (void)hipEventElapsedTime(&merge_ms, ev0, ev1);
  sum.ms_select += merge_ms;
  sum.ms_total += merge_ms;
  sum.n_reads = nr;
  sum.n_hits = c->nhits = total;
  sum.n_overflow_blocks = check_blocks ? ovf_blocks : ~0ull;
  c->stats = sum;
  c->last_exact_blocks = check_blocks;
  if (nhits) *nhits = total;
  return 0;
}

// Every partition runs with exact block counters; on every exit the context's own setting comes back and the merge's
// buffers are released, so that the next plan sees the memory it reserved for them (merge_reserve)
static int match_partitioned(musc_ctx* c, const musc_params* P, uint64_t* nhits) {
  const bool keep_force = c->force_exact_blocks;
  c->force_exact_blocks = true;
  const int rc = match_partitions_run(c, P, nhits);
  c->force_exact_blocks = keep_force;
  (void)hipStreamSynchronize(c->stream);  // (an error path may leave merge kernels queued)
  c->pacc.release(); c->pbest.release(); c->pcnt.release(); c->padj.release(); c->pflags.release(); c->pflags_tmp.release();
  c->block_acc.release();
  return rc;
}

int musc_hits_copy(musc_ctx* c, musc_hit* dst, uint64_t capacity, int dst_on_device) {
  if (!c) return 1;
  if (capacity < c->nhits) return fail(c, 2, "musc_hits_copy: capacity %llu < %llu hits",
                                       (unsigned long long)capacity, (unsigned long long)c->nhits);
  if (c->nhits == 0) return 0;
  if (!dst) return fail(c, 2, "musc_hits_copy: dst is NULL");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(dst, c->hits.p, c->nhits * sizeof(musc_hit),
                           dst_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

}  // extern "C"

// results.txt and the side outputs as text from the resident tuples (musc_results_*, musc_side_*)
#include "muscato_text.hpp"
#include "muscato_cov.hpp"
// the MaxMatches truncation replayed on the device (musc_maxmatches_*)
#include "muscato_maxmatches.hpp"
#include "muscato_read_names.hpp"

extern "C" {

// Tuples that are packed on the device on their way to the host (musc_hits_copy_compact, musc_hits_copy_packed): the
// pack kernel runs at memory speed, the copy at link speed, so packing everything first keeps the link idle for the
// whole kernel.  Instead the list goes in chunks: `pack(t0, t1)` launches the kernel for tuples [t0, t1) on the
// context's stream, and the copy of those `elem`-byte words follows on the copy stream behind an event while the next
// chunk is packed.  The first chunk is 1/32 of the list (what the link waits for), each later one four times the one
// before: the pack of a chunk is over long before the copy of the previous one.  Queues only; download_end waits.
extern "C++" {
template <class Pack>
static int download_chunks(musc_ctx* c, uint64_t n, size_t elem, const void* src, void* dst, Pack pack) {
  if (!c->up.s_up) HIPCHK(c, hipStreamCreateWithFlags(&c->up.s_up, hipStreamNonBlocking));
  const uint64_t smallest = std::min<uint64_t>(c->batch_reads, 1u << 18);  // (MUSC_BATCH_READS: several chunks of a test-sized list)
  uint64_t sz = std::max<uint64_t>(n / 32, smallest);
  size_t k = 0;
  for (uint64_t t0 = 0; t0 < n; k++, sz *= 4) {
    const uint64_t t1 = n - t0 <= sz + sz / 2 ? n : t0 + sz;
    if (k == c->dl_ev.size()) {
      hipEvent_t e = nullptr;
      HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
      c->dl_ev.push_back(e);
    }
    pack(t0, t1);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->dl_ev[k], c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->up.s_up, c->dl_ev[k], 0));
    HIPCHK(c, hipMemcpyAsync((char*)dst + t0 * elem, (const char*)src + t0 * elem, (t1 - t0) * elem, hipMemcpyDeviceToHost, c->up.s_up));
    t0 = t1;
  }
  return 0;
}
}  // extern "C++"

// The end of such a download: the kernels' verdict word to *h_bad (pinned), `tail_bytes` more bytes that are complete
// only after the last chunk's kernel (the count bytes) behind the chunks on the copy stream, then both streams are
// waited for -- on every path, so that nothing is still being written to the caller's buffers when the call returns.
static int download_end(musc_ctx* c, uint32_t* h_bad, void* tail_dst, const void* tail_src, uint64_t tail_bytes) {
  hipError_t e = hipMemcpyAsync(h_bad, c->d_flag, 4, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess && tail_bytes) {
    hipStream_t st = c->up.s_up ? c->up.s_up : c->stream;
    if (st != c->stream && (e = hipEventRecord(c->ev_join, c->stream)) == hipSuccess) e = hipStreamWaitEvent(st, c->ev_join, 0);
    if (e == hipSuccess) e = hipMemcpyAsync(tail_dst, tail_src, tail_bytes, hipMemcpyDeviceToHost, st);
  }
  const hipError_t e1 = hipStreamSynchronize(c->stream);
  const hipError_t e2 = c->up.s_up ? hipStreamSynchronize(c->up.s_up) : hipSuccess;
  if (e == hipSuccess) e = e1 != hipSuccess ? e1 : e2;
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(c, 10, "copying the tuples to the host failed: %s", hipGetErrorString(e));
  }
  return 0;
}

static int check_pack_bits(musc_ctx* c, const int32_t* bits, PackBits* b) {
  if (!bits) return fail(c, 2, "bits is NULL");
  int sum = 0;
  for (int i = 0; i < 4; i++) {
    if (bits[i] < 1 || bits[i] > 32) return fail(c, 2, "field width %d outside 1..32", bits[i]);
    sum += bits[i];
  }
  if (sum > 64) return fail(c, 2, "field widths add up to %d > 64 bits", sum);
  *b = PackBits{bits[0], bits[1], bits[2], bits[3]};
  return 0;
}

int musc_hits_copy_packed(musc_ctx* c, uint64_t* dst, uint64_t capacity, int dst_on_device, uint64_t read_base,
                          const int32_t* bits) {
  if (!c) return 1;
  PackBits b;
  int rc = check_pack_bits(c, bits, &b);
  if (rc) return rc;
  if (capacity < c->nhits) return fail(c, 2, "musc_hits_copy_packed: capacity %llu < %llu hits",
                                       (unsigned long long)capacity, (unsigned long long)c->nhits);
  if (c->nhits == 0) return 0;
  if (!dst) return fail(c, 2, "musc_hits_copy_packed: dst is NULL");
  HIPCHK(c, hipSetDevice(c->device));
  uint64_t* out = dst;
  if (!dst_on_device) {
    if ((rc = ensure(c, c->packed, c->nhits))) return rc;
    out = c->packed.p;
  }
  HIPCHK(c, hipMemsetAsync(c->d_flag, 0, 4, c->stream));
  const uint4* const hits = reinterpret_cast<const uint4*>(c->hits.p);
  auto pack = [&](uint64_t t0, uint64_t t1) {
    hipLaunchKernelGGL(k_pack_hits, grid(c, t1 - t0), dim3(256), 0, c->stream, hits + t0, t1 - t0,
                       read_base, b, out + t0, c->d_flag);
  };
  uint32_t* const h_bad = reinterpret_cast<uint32_t*>(c->h_pinned.get());
  if (dst_on_device) {
    pack(0, c->nhits);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h_bad, c->d_flag, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  } else {
    rc = download_chunks(c, c->nhits, 8, out, dst, pack);
    const int rc_end = download_end(c, h_bad, nullptr, nullptr, 0);
    if (rc || rc_end) return rc ? rc : rc_end;
  }
  const uint32_t bad = *h_bad;
  if (bad) return fail(c, 8, "musc_hits_copy_packed: a tuple field does not fit its width (%d/%d/%d/%d bits)",
                       b.read, b.gene, b.pos, b.nmiss);
  return 0;
}

int musc_hits_copy_compact(musc_ctx* c, uint32_t* words, uint64_t words_cap, uint8_t* counts, uint64_t counts_cap,
                           int dst_on_device, const int32_t* bits) {
  if (!c) return 1;
  if (!bits) return fail(c, 2, "bits is NULL");
  int sum = 0;
  for (int i = 0; i < 3; i++) {
    if (bits[i] < 1 || bits[i] > 30) return fail(c, 2, "field width %d outside 1..30", bits[i]);
    sum += bits[i];
  }
  if (sum > 32) return fail(c, 2, "field widths add up to %d > 32 bits", sum);
  if (words_cap < c->nhits) return fail(c, 2, "musc_hits_copy_compact: room for %llu tuples < %llu",
                                        (unsigned long long)words_cap, (unsigned long long)c->nhits);
  if (counts_cap < c->nreads) return fail(c, 2, "musc_hits_copy_compact: room for %llu reads < %llu",
                                          (unsigned long long)counts_cap, (unsigned long long)c->nreads);
  if ((c->nhits && !words) || (c->nreads && !counts)) return fail(c, 2, "musc_hits_copy_compact: NULL destination");
  HIPCHK(c, hipSetDevice(c->device));
  const PackBits b{0, bits[0], bits[1], bits[2]};
  uint32_t* dw = words;
  uint8_t* dc = counts;
  if (!dst_on_device) {  // stage on the device, then one copy each
    int rc = ensure(c, c->packed, (c->nhits * 4 + c->nreads + 15) / 8 + 2);
    if (rc) return rc;
    dw = reinterpret_cast<uint32_t*>(c->packed.p);
    dc = reinterpret_cast<uint8_t*>(dw + c->nhits);
  }
  HIPCHK(c, hipMemsetAsync(c->d_flag, 0, 4, c->stream));
  if (c->nreads) HIPCHK(c, hipMemsetAsync(dc, 0, c->nreads, c->stream));
  const uint4* const hits = reinterpret_cast<const uint4*>(c->hits.p);
  uint32_t* const h_bad = reinterpret_cast<uint32_t*>(c->h_pinned.get());
  if (dst_on_device) {
    if (c->nhits) {
      hipLaunchKernelGGL(k_pack_compact, grid(c, c->nhits), dim3(256), 0, c->stream, hits, c->nhits,
                         b, dw, dc, c->d_flag);
      HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipMemcpyAsync(h_bad, c->d_flag, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  } else {
    // the words chunk by chunk, then the count bytes: a count is final only when the chunk that holds the head of its
    // read's run has been packed, and the counts are the smaller copy
    int rc = download_chunks(c, c->nhits, 4, dw, words, [&](uint64_t t0, uint64_t t1) {
      hipLaunchKernelGGL(k_pack_compact_range, grid(c, t1 - t0), dim3(256), 0, c->stream, hits,
                         c->nhits, t0, t1, b, dw, dc, c->d_flag);
    });
    const int rc_end = download_end(c, h_bad, counts, dc, c->nreads);
    if (rc || rc_end) return rc ? rc : rc_end;
  }
  const uint32_t bad = *h_bad;
  if (bad & 4u) return fail(c, 12, "internal: the hit list is not read-major");
  if (bad) return fail(c, 8, "musc_hits_copy_compact: %s", (bad & 1u) ? "a tuple field does not fit its width"
                                                                      : "a read has more than 255 tuples");
  return 0;
}

int musc_hits_unpack(musc_ctx* c, const uint64_t* src, uint64_t n, int on_device, const int32_t* bits, musc_hit* dst) {
  if (!c) return 1;
  PackBits b;
  int rc = check_pack_bits(c, bits, &b);
  if (rc) return rc;
  if (n == 0) return 0;
  if (!src || !dst) return fail(c, 2, "musc_hits_unpack: NULL pointer");
  if (!on_device) {  // host to host: plain loop, same layout
    for (uint64_t i = 0; i < n; i++) {
      uint64_t v = src[i];
      dst[i].nmiss = (uint32_t)(v & ((1ull << b.nmiss) - 1ull));
      v >>= b.nmiss;
      dst[i].pos = (uint32_t)(v & ((1ull << b.pos) - 1ull));
      v >>= b.pos;
      dst[i].gene_idx = (uint32_t)(v & ((1ull << b.gene) - 1ull));
      v >>= b.gene;
      dst[i].read_idx = (uint32_t)v;
    }
    return 0;
  }
  HIPCHK(c, hipSetDevice(c->device));
  hipLaunchKernelGGL(k_unpack_hits, grid(c, n), dim3(256), 0, c->stream, src, n, b,
                     reinterpret_cast<uint4*>(dst));
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

int musc_match(musc_ctx* c, const musc_params* P, musc_hit** hits, uint64_t* nhits) {
  if (!c) return 1;
  if (!hits || !nhits) return fail(c, 2, "musc_match: NULL output pointer");
  *hits = nullptr;
  *nhits = 0;
  uint64_t n = 0;
  int rc = musc_match_device(c, P, &n);
  if (rc) return rc;
  musc_hit* h = (musc_hit*)malloc(sizeof(musc_hit) * (n ? n : 1));
  if (!h) return fail(c, 7, "out of host memory for %llu hits", (unsigned long long)n);
  rc = musc_hits_copy(c, h, n, 0);
  if (rc) {
    free(h);
    return rc;
  }
  *hits = h;
  *nhits = n;
  return 0;
}

void musc_free_hits(musc_hit* hits) { free(hits); }

int musc_overflow_probes(musc_ctx* c, uint32_t** read_idx, uint32_t** window, uint64_t* n) {
  if (!c) return 1;
  if (!read_idx || !window || !n) return fail(c, 2, "musc_overflow_probes: NULL output pointer");
  *read_idx = *window = nullptr;
  *n = 0;
  if (c->stats.n_overflow_blocks == 0 || c->stats.n_overflow_blocks == ~0ull) return 0;
  if (!c->last_exact_blocks || !c->block_table.p) return fail(c, 4, "no exact block counters from the last pass");
  HIPCHK(c, hipSetDevice(c->device));
  DevPtr<uint2> d_out;  // the probes on the device, released on every return
  uint64_t found = 0;
  const int rc = hot_probes_device(c, &d_out, &found);
  if (rc) return rc;
  std::vector<uint2> h(found ? found : 1);
  if (found) {
    const hipError_t e = hipMemcpy(h.data(), d_out, found * sizeof(uint2), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(c, 10, "musc_overflow_probes: %s", hipGetErrorString(e));
  }
  uint32_t* r = (uint32_t*)malloc(sizeof(uint32_t) * (found ? found : 1));
  uint32_t* w = (uint32_t*)malloc(sizeof(uint32_t) * (found ? found : 1));
  if (!r || !w) {
    free(r);
    free(w);
    return fail(c, 7, "musc_overflow_probes: out of host memory");
  }
  for (uint64_t j = 0; j < found; j++) {
    r[j] = h[j].x;
    w[j] = h[j].y;
  }
  *read_idx = r;
  *window = w;
  *n = found;
  return 0;
}

void musc_free_u32(uint32_t* p) { free(p); }

int musc_get_stats(musc_ctx* c, musc_stats* out) {
  if (!c || !out) return 1;
  *out = c->stats;
  return 0;
}

int musc_last_instance(const musc_ctx* c, uint32_t* out) {
  if (!c || !out) return 1;
  for (int i = 0; i < MUSC_INSTANCE_WORDS; i++) out[i] = c->last_inst[i];
  return 0;
}

// Every descriptor the resolvers can return, read out of the resolvers themselves over every argument they take
// (no GPU, no context): the tests compare their case lists with it, so an instance without a case is noticed.
int musc_instances(uint32_t* out, uint32_t capacity, uint32_t* n) {
  if (!n) return 1;
  std::vector<uint32_t> ids;
  auto add = [&](uint32_t id) {
    if (id && std::find(ids.begin(), ids.end(), id) == ids.end()) ids.push_back(id);
  };
  static const int strides[] = {4, 8, 12, 16, 20};  // (20: a stride without instances of its own, the runtime-stride ones)
  for (int rw : strides) {
    for (int kind : {MK_LANE, MK_DMA})
      for (int sg = 0; sg <= MUSC_SPEC_GEOMS; sg++)
        for (int wide = 0; wide < 2; wide++)
          for (int W = 1; W <= CTX_MAX_W; W++)
            for (int xm = 0; xm < 3; xm++) add(match_instance(kind, sg, rw, wide != 0, W, xm).id);
    add(screen_t_instance(rw).id);
    for (int mask = 0; mask < 2; mask++)
      for (int W = 2; W <= 3; W++) {
        for (int lines = 0; lines < 2; lines++) add(screen_instance(rw, mask != 0, W, lines != 0).id);
        add(confirm_instance(rw, mask != 0, W).id);
      }
  }
  *n = (uint32_t)ids.size();
  if (out)
    for (uint32_t i = 0; i < capacity && i < ids.size(); i++) out[i] = ids[i];
  return 0;
}

// stream_plan as the loader and the passes use it (no GPU, no context): the tests check its rules over read counts
// no test could upload.
int musc_stream_plan(uint64_t nreads, uint32_t fixed_len, uint32_t batch_reads, uint64_t* ends, uint8_t* is_batch_end,
                     uint64_t capacity, uint64_t* n, uint64_t* planned_batches) {
  if (!n || fixed_len > 65535 || nreads >= 0xFFFFFFF0ull) return 1;  // (no read index / record for these)
  if (batch_reads < 1 || batch_reads > (16u << 20)) batch_reads = 16u << 20;  // (as musc_init reads MUSC_BATCH_READS)
  StreamPlan sp;
  stream_plan(nreads, batch_reads, &sp);
  *n = sp.piece_end.size();
  if (planned_batches) *planned_batches = std::max<uint64_t>(sp.batch_end.size(), 1);
  size_t b = 0;
  for (size_t i = 0; i < sp.piece_end.size() && i < capacity; i++) {
    if (ends) ends[i] = sp.piece_end[i];
    while (b < sp.batch_end.size() && sp.batch_end[b] < sp.piece_end[i]) b++;
    if (is_batch_end) is_batch_end[i] = b < sp.batch_end.size() && sp.batch_end[b] == sp.piece_end[i];
  }
  return 0;
}

int musc_gather(musc_ctx* const* ctxs, int n, const uint64_t* read_base, musc_hit** hits, uint64_t* nhits) {
  if (!ctxs || n < 1 || !hits || !nhits) return 1;
  uint64_t total = 0;
  for (int i = 0; i < n; i++) {
    if (!ctxs[i]) return 1;
    total += ctxs[i]->nhits;
  }
  musc_hit* h = (musc_hit*)malloc(sizeof(musc_hit) * (total ? total : 1));
  if (!h) return fail(ctxs[0], 7, "musc_gather: out of host memory");
  uint64_t o = 0;
  for (int i = 0; i < n; i++) {
    musc_ctx* c = ctxs[i];
    int rc = musc_hits_copy(c, h + o, c->nhits, 0);
    if (rc) {
      free(h);
      return rc;
    }
    const uint64_t base = read_base ? read_base[i] : 0;
    for (uint64_t j = 0; j < c->nhits; j++) h[o + j].read_idx += (uint32_t)base;
    o += c->nhits;
  }
  *hits = h;
  *nhits = total;
  return 0;
}

// ---- RCCL, resolved at run time: a single-GPU user never loads the library, and a box without
// it still runs everything but musc_gather_rccl
namespace {
struct RcclApi {
  void* lib = nullptr;
  decltype(&ncclCommInitAll) CommInitAll = nullptr;
  decltype(&ncclCommDestroy) CommDestroy = nullptr;
  decltype(&ncclGroupStart) GroupStart = nullptr;
  decltype(&ncclGroupEnd) GroupEnd = nullptr;
  decltype(&ncclSend) Send = nullptr;
  decltype(&ncclRecv) Recv = nullptr;
  decltype(&ncclGetErrorString) GetErrorString = nullptr;
  std::string err;
  std::map<std::vector<int>, std::vector<ncclComm_t>> comms;  // one clique per device list, kept for the process
};
std::mutex g_rccl_mu;

RcclApi* rccl_api() {
  static RcclApi api;
  if (api.lib || !api.err.empty()) return &api;
  // MUSC_RCCL_LIB names the library (tests point it at a missing file); otherwise the one next to the
  // HIP runtime this library links against, then whatever the loader finds
  std::string first_err;
  std::vector<std::string> names;
  if (const char* e = getenv("MUSC_RCCL_LIB")) names.push_back(e);
  else names = {"/opt/rocm/lib/librccl.so.1", "librccl.so.1", "librccl.so"};
  for (const std::string& name : names) {
    (void)dlerror();
    api.lib = dlopen(name.c_str(), RTLD_NOW | RTLD_LOCAL);
    if (api.lib) break;
    const char* e = dlerror();  // (one call: it returns the message and clears it)
    if (first_err.empty()) first_err = e ? e : "not found";
  }
  if (!api.lib) {
    api.err = std::string("cannot load librccl: ") + first_err;
    return &api;
  }
#define MUSC_RCCL_SYM(FIELD, NAME)                                   \
  api.FIELD = reinterpret_cast<decltype(api.FIELD)>(dlsym(api.lib, NAME)); \
  if (!api.FIELD && api.err.empty()) api.err = std::string("librccl lacks ") + NAME;
  MUSC_RCCL_SYM(CommInitAll, "ncclCommInitAll")
  MUSC_RCCL_SYM(CommDestroy, "ncclCommDestroy")
  MUSC_RCCL_SYM(GroupStart, "ncclGroupStart")
  MUSC_RCCL_SYM(GroupEnd, "ncclGroupEnd")
  MUSC_RCCL_SYM(Send, "ncclSend")
  MUSC_RCCL_SYM(Recv, "ncclRecv")
  MUSC_RCCL_SYM(GetErrorString, "ncclGetErrorString")
#undef MUSC_RCCL_SYM
  return &api;
}
}  // namespace

int musc_rccl_probe(char* msg, uint64_t cap) {
  std::lock_guard<std::mutex> lock(g_rccl_mu);
  RcclApi* api = rccl_api();
  if (msg && cap) {
    strncpy(msg, api->err.c_str(), cap - 1);
    msg[cap - 1] = 0;
  }
  return api->err.empty() ? 0 : 20;
}

__global__ void k_rebase_reads(uint4* __restrict__ h, uint64_t n, uint32_t base) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) h[i].x += base;
}

int musc_gather_rccl(musc_ctx* const* ctxs, int n, const uint64_t* read_base, musc_hit** hits, uint64_t* nhits) {
  if (!ctxs || n < 1 || !hits || !nhits) return 1;
  *hits = nullptr;
  *nhits = 0;
  uint64_t total = 0;
  std::vector<uint64_t> off(n + 1, 0);
  std::vector<int> devs(n);
  for (int i = 0; i < n; i++) {
    if (!ctxs[i]) return 1;
    devs[i] = ctxs[i]->device;
    off[i] = total;
    total += ctxs[i]->nhits;
  }
  off[n] = total;
  musc_ctx* c0 = ctxs[0];
  for (int i = 0; i < n; i++)
    for (int j = i + 1; j < n; j++)
      if (devs[i] == devs[j]) return fail(c0, 2, "musc_gather_rccl: contexts %d and %d share device %d", i, j, devs[i]);
  std::lock_guard<std::mutex> lock(g_rccl_mu);
  std::vector<ncclComm_t>* comms = nullptr;
  RcclApi* api = nullptr;
  if (n > 1) {
    api = rccl_api();
    if (!api->err.empty()) return fail(c0, 20, "musc_gather_rccl: %s", api->err.c_str());
    auto it = api->comms.find(devs);
    if (it == api->comms.end()) {
      std::vector<ncclComm_t> cs(n);
      const ncclResult_t r = api->CommInitAll(cs.data(), n, devs.data());
      if (r != ncclSuccess) return fail(c0, 20, "musc_gather_rccl: ncclCommInitAll: %s", api->GetErrorString(r));
      it = api->comms.emplace(devs, cs).first;
    }
    comms = &it->second;
  }
  HIPCHK(c0, hipSetDevice(c0->device));
  int rc = ensure(c0, c0->gathered, total ? total : 1);
  if (rc) return rc;
  // the destination's own tuples never touch a link; everything else arrives over xGMI, all
  // transfers in ONE group so that the links run side by side
  if (c0->nhits)
    HIPCHK(c0, hipMemcpyAsync(c0->gathered.p, c0->hits.p, c0->nhits * sizeof(musc_hit), hipMemcpyDeviceToDevice, c0->stream));
  if (n > 1) {
    ncclResult_t r = api->GroupStart();
    for (int i = 1; i < n && r == ncclSuccess; i++) {
      if (!ctxs[i]->nhits) continue;
      const size_t bytes = ctxs[i]->nhits * sizeof(musc_hit);
      (void)hipSetDevice(ctxs[i]->device);
      r = api->Send(ctxs[i]->hits.p, bytes, ncclUint8, 0, (*comms)[i], ctxs[i]->stream);
      if (r != ncclSuccess) break;
      (void)hipSetDevice(c0->device);
      r = api->Recv(c0->gathered.p + off[i], bytes, ncclUint8, i, (*comms)[0], c0->stream);
    }
    const ncclResult_t r2 = api->GroupEnd();
    if (r == ncclSuccess) r = r2;
    if (r != ncclSuccess) return fail(c0, 20, "musc_gather_rccl: %s", api->GetErrorString(r));
  }
  HIPCHK(c0, hipSetDevice(c0->device));
  for (int i = 0; i < n; i++) {
    const uint64_t base = read_base ? read_base[i] : 0;
    if (!base || !ctxs[i]->nhits) continue;
    hipLaunchKernelGGL(k_rebase_reads, grid(c0, ctxs[i]->nhits), dim3(256), 0, c0->stream,
                       reinterpret_cast<uint4*>(c0->gathered.p + off[i]), ctxs[i]->nhits, (uint32_t)base);
    HIPCHK(c0, hipGetLastError());
  }
  for (int i = 1; i < n; i++) {  // the senders' streams
    HIPCHK(ctxs[i], hipSetDevice(ctxs[i]->device));
    HIPCHK(ctxs[i], hipStreamSynchronize(ctxs[i]->stream));
  }
  HIPCHK(c0, hipSetDevice(c0->device));
  musc_hit* h = (musc_hit*)malloc(sizeof(musc_hit) * (total ? total : 1));
  if (!h) return fail(c0, 7, "musc_gather_rccl: out of host memory");
  hipError_t e = hipSuccess;
  if (total) e = hipMemcpyAsync(h, c0->gathered.p, total * sizeof(musc_hit), hipMemcpyDeviceToHost, c0->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c0->stream);
  if (e != hipSuccess) {
    free(h);
    return fail(c0, 10, "musc_gather_rccl: %s", hipGetErrorString(e));
  }
  *hits = h;
  *nhits = total;
  return 0;
}

}  // extern "C"
