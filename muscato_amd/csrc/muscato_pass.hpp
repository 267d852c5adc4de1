// muscato_pass.hpp -- the host side of musc_match_device: the kernel-instance resolvers and launchers of both paths, and
// the pass driver (set-up, batches, finish, retries).  Part of libmuscato_hip.so: included by muscato_hip.hip after
// muscato_index.hpp (ensure_index, plan_partitions; the resident index is read through c->idx) and muscato_load.hpp,
// whose upload and database code it calls (upload_prepare, db_xblocks).
#pragma once

namespace {

inline bool idx_is_ctx(const musc_ctx* c) { return musc_index::is_ctx(c->idx.kind); }
inline bool idx_is_wide(const musc_ctx* c) { return c->idx.kind == musc_index::K_CTXW; }
inline bool idx_is_lines(const musc_ctx* c) { return c->idx.kind == musc_index::K_LINES; }

// Which of the two fused kernels on context buckets runs
enum MatchKind { MK_LANE = 2, MK_DMA = 3 };
// MK_LANE = k_match_t (kernels_match_lane.hpp): every run on context buckets.  MK_DMA = k_match_g
// (kernels_match_dma.hpp): the same comparisons at three to four waves per SIMD, everything from memory by LDS-DMA --
// built for two windows on 120-base buckets, records of 8 words, no X on either side (BASELINE configs 2-4).  It is
// the second implementation (MUSC_MATCH=dma; the parity tests run both): on cfg3 its launch takes as long as
// k_match_t's.
int match_kind(const musc_ctx* c, int W) {
  if (c->env.match_dma && W == 2 && c->rw == 8 && c->idx.kind == musc_index::K_CTX && !c->db_has_x && !c->reads_have_x) return MK_DMA;
  return MK_LANE;
}

// line buckets without X anywhere, record strides k_screen_t is built for: the wave-autonomous screen
// (kernels_screen_lane.hpp); MUSC_SCREEN=wg keeps k_screen (A/B runs)
bool screen_lane(const musc_ctx* c, bool mask) {
  return idx_is_lines(c) && !mask && !c->rdm && (c->rw == 4 || c->rw == 8 || c->rw == 12 || c->rw == 16) && !c->env.screen_wg;
}

// f(std::integral_constant<int, RW>{}) for the record strides that have kernel instances of their own (RW = 0: any other)
template <class F>
auto by_rw(int rw, F&& f) {
  switch (rw) {
    case 4: return f(std::integral_constant<int, 4>{});
    case 8: return f(std::integral_constant<int, 8>{});
    case 12: return f(std::integral_constant<int, 12>{});
    case 16: return f(std::integral_constant<int, 16>{});
    default: return f(std::integral_constant<int, 0>{});
  }
}

// The instance of each two-kernel-path kernel a run launches: one resolver per kernel, which the launch
// (and for k_screen_t the occupancy query of screen_grid) takes it from.  A resolver returns the function pointer
// TOGETHER with its descriptor (musc_last_instance, include/muscato_hip.h): both come from one table entry, written
// by one macro from one list of template arguments, so what a pass reports is what it launched.
typedef decltype(&k_screen_t<8>) screen_t_fn;
typedef decltype(&k_screen<0, false, false, false>) screen_fn;
typedef decltype(&k_confirm<0, false, false>) confirm_fn;
template <class Fn>
struct Inst {
  Fn fn;
  uint32_t id;  // MUSC_INST_* family and template arguments; 0 with fn == nullptr
};
constexpr uint32_t inst_id(uint32_t family, int rw, int a = 0, int b = 0, int c = 0, int d = 0) {
  return family | (uint32_t)rw << 8 | (uint32_t)a << 16 | (uint32_t)b << 20 | (uint32_t)c << 24 | (uint32_t)d << 28;
}
#define INST_SCREEN_T(RW) Inst<screen_t_fn>{k_screen_t<RW>, inst_id(MUSC_INST_SCREEN_T, RW)}
#define INST_SCREEN(RW, M, ONE, LN) Inst<screen_fn>{k_screen<RW, M, ONE, LN>, inst_id(MUSC_INST_SCREEN, RW, M, ONE, LN)}
#define INST_CONFIRM(RW, M, W2) Inst<confirm_fn>{k_confirm<RW, M, W2>, inst_id(MUSC_INST_CONFIRM, RW, M, W2)}

Inst<screen_t_fn> screen_t_instance(int rw) {  // (screen_lane: only the strides k_screen_t is built for)
  return by_rw(rw, [](auto r) -> Inst<screen_t_fn> {
    if constexpr (decltype(r)::value != 0) return INST_SCREEN_T(decltype(r)::value);
    else return Inst<screen_t_fn>{nullptr, 0};
  });
}

Inst<screen_fn> screen_instance(int rw, bool mask, int W, bool lines) {
  const int m = mask, one = W <= 2, ln = lines;
  return by_rw(rw, [&](auto r) -> Inst<screen_fn> {
    constexpr int RW = decltype(r)::value;
    static const Inst<screen_fn> k[2][2][2] = {
        {{INST_SCREEN(RW, false, false, false), INST_SCREEN(RW, false, false, true)}, {INST_SCREEN(RW, false, true, false), INST_SCREEN(RW, false, true, true)}},
        {{INST_SCREEN(RW, true, false, false), INST_SCREEN(RW, true, false, true)}, {INST_SCREEN(RW, true, true, false), INST_SCREEN(RW, true, true, true)}}};
    return k[m][one][ln];
  });
}

Inst<confirm_fn> confirm_instance(int rw, bool mask, int W) {
  const int m = mask, w2 = W <= 2;
  return by_rw(rw, [&](auto r) -> Inst<confirm_fn> {
    constexpr int RW = decltype(r)::value;
    static const Inst<confirm_fn> k[2][2] = {{INST_CONFIRM(RW, false, false), INST_CONFIRM(RW, false, true)}, {INST_CONFIRM(RW, true, false), INST_CONFIRM(RW, true, true)}};
    return k[m][w2];
  });
}

// workgroups of the screen stage: the descriptor buffer is cut into that many regions.  k_screen_t's
// workgroups are single waves that stay for the whole launch: as many as are resident at once (a
// second, thinner round of them would cost what a full one does).
unsigned screen_grid(musc_ctx* c, uint32_t n, bool mask) {
  unsigned g = std::min(nblk(n, TILE), MAX_GRID);
  if (screen_lane(c, mask)) {
    if (!c->scrt_resident || c->scrt_rw != c->rw) {
      int per_cu = 0, ncu = 0;
      const void* fn = reinterpret_cast<const void*>(screen_t_instance(c->rw).fn);
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, 64, 0) != hipSuccess || per_cu < 1) { (void)hipGetLastError(); per_cu = 8; }
      if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess || ncu < 1) ncu = 256;
      c->scrt_resident = (unsigned)per_cu * (unsigned)ncu;
      c->scrt_rw = c->rw;
    }
    g = std::min(g, std::min(c->scrt_resident, MAX_GRID));
  }
  return g;
}

// ---------------------------------------------------------------- the pass
// match_index_pass is the ONLY place that repeats a pass: an attempt = pass_setup, then pass_fused or pass_two_kernel,
// each ending in pass_close and pass_verdict; what the attempt came to goes back to the loop as a PassOutcome.
enum PassOutcome {
  PASS_DONE = 0,
  PASS_RERUN_CAREFUL,   // a guard fired on a sized pass: it did not fit after all
  PASS_RERUN_EXACT,     // MaxMatches screening inconclusive: a hot sketch cell, or more launches than the threshold assumed
  PASS_RERUN_NO_GRAPH,  // capture or instantiation failed
};

// What pass_setup settles for one attempt; both paths read it
struct PassPlan {
  const musc_params* P = nullptr;
  PathParams pp;
  uint64_t max_matches = 0, planned_batches = 0;
  int block_mode = 0;      // MaxMatches accounting (see k_confirm): 0 off, 1 screening sketch, 2 exact per-block counters
  uint32_t block_thr = 0;  // mode 1: what one workgroup-launch may add to a sketch cell
  // A pass over the same reads, database, parameters and block mode as the last completed one is known to fit: it runs
  // without host round trips; every kernel still guards its writes, and the flags are checked once at the end.
  bool sized = false;
  match_kernel_t kern = nullptr;  // fused path: the instance, and the workgroups of it that are resident at once
  unsigned resident = 0;
  bool mask = false;              // two-kernel path: an X on either side
};

// How many reads the batch at r0 takes: from the upload's schedule (a pass that starts with an upload in flight, every
// attempt of it: stream_plan -- whole pieces, tapered towards the end), else uniform batches of bsz reads.  A streamed
// pass sizes itself (the reads are new) and leaves the context UNSIZED: a later pass over the same reads finds them
// resident, sizes itself on uniform batches and is the one later passes replay -- the tapered schedule is never
// replayed against resident reads, where small batches only cost.
struct BatchCursor {
  const StreamPlan* plan = nullptr;
  uint32_t bsz = 0;
  uint32_t reads_at(uint64_t r0, uint64_t nreads) const {
    return (uint32_t)(plan ? stream_plan_batch(*plan, r0) : std::min<uint64_t>(bsz, nreads - r0));
  }
  void halve(uint32_t n) {  // the batch of n reads passed 2^31 offsets: uniform batches of half of it from here on
    bsz = n / 2;
    plan = nullptr;
  }
};
constexpr uint64_t BATCH_OFFSET_CAP = 1ull << 31;  // tuple and descriptor offsets within a batch are u32

// What a first (careful) pass provides per batch of n reads before it has seen a count: tuples staged per read on the
// fused path, descriptors per read (and at least) on the two-kernel path.  tests/test_stats_model.py:
// test_heavy_reads_outgrow_a_first_pass restates these figures so that the growing case of tests/test_gpu_stats.py
// does grow -- keep the two in step.
constexpr uint64_t FIRST_PASS_TUPLES_PER_READ = 2, FIRST_PASS_DESC_PER_READ = 4, FIRST_PASS_DESC_MIN = 1024;

// the events of one attempt: per-kernel-family pairs and the two around the whole pass
struct PassClock {
  Timer tm;
  hipEvent_t ev0, ev1;
  explicit PassClock(musc_ctx* c) : tm(c), ev0(pool_event(c)), ev1(pool_event(c)) {}
};

void launch_screen(musc_ctx* c, const PassPlan& pl, uint64_t r0, uint32_t n) {
  const dim3 sgrid(screen_grid(c, n, pl.mask));
  auto& b = c->bs[c->cur];
  if (screen_lane(c, pl.mask)) {
    const auto k = screen_t_instance(c->rw);
    c->last_inst[1] = k.id;
    hipLaunchKernelGGL(k.fn, sgrid, dim3(64), 0, c->stream, c->rd, r0, n, c->d_pp, c->nmiss_tab.p,
                       static_cast<const LineBucket*>(c->idx_T.p), static_cast<const uint4*>(c->idx_E.p), b.cdesc.p, b.cdesc.cap, b.rvalid.p, b.wb.p,
                       b.tbase.p, b.tcount.p, c->counters + CNT_BATCH, c->counters + CNT_FLAGS);
  } else {
    const auto k = screen_instance(c->rw, c->rdm != nullptr, pl.pp.W, idx_is_lines(c));
    c->last_inst[1] = k.id;
    hipLaunchKernelGGL(k.fn, sgrid, dim3(TILE), 0, c->stream, c->rd, c->rdm, r0, n, c->rw, c->d_pp,
                       c->nmiss_tab.p, static_cast<const Bucket*>(c->idx_T.p), static_cast<const uint4*>(c->idx_E.p), b.cdesc.p, b.cdesc.cap, b.rvalid.p, b.wb.p, b.tbase.p, b.tcount.p,
                       c->counters + CNT_BATCH, c->counters + CNT_FLAGS);
  }
}

void launch_confirm(musc_ctx* c, const PassPlan& pl, uint64_t r0, uint32_t n) {
  // persistent over tiles; the MaxMatches screening threshold assumes at most MAX_GRID workgroups
  const dim3 grid(std::min(nblk(n, TILE), MAX_GRID));
  static_assert((1u << 24) / TILE / MAX_GRID <= CONF_TILES, "a k_confirm workgroup keeps its tile list in LDS");
  const size_t lds = pl.block_mode ? (size_t)TILE * pl.pp.W * 4 : 0;
  auto& b = c->bs[c->cur];
  const auto k = confirm_instance(c->rw, pl.mask, pl.pp.W);
  c->last_inst[2] = k.id;
  hipLaunchKernelGGL(k.fn, grid, dim3(TILE), lds, c->s_confirm, c->rd, c->rdm, c->db2, c->dbm2,
                     c->dbx, r0, n, c->rw, c->d_pp, c->nmiss_tab.p, b.cdesc.p, b.rvalid.p, c->p_nx.p, b.tbase.p, b.tcount.p,
                     b.wb.p, pl.block_mode, pl.block_thr, c->block_table.p, c->seq_off, c->stage.p, c->tcount2.p,
                     c->counters);
}

}  // namespace

static size_t match_dyn_lds(int kind, int W, int block_mode) {
  // per-(window, read) counters of the wave-tile in hand (k_match_t: of two wave-tiles), then (mode 1) the sketch
  if (kind == MK_DMA) return block_mode == 1 ? (size_t)(4u << MATCHG_SKETCH_BITS) : 0u;  // (its per-(window, read) counters are registers)
  const size_t wcnt = (size_t)TILE * W * 4 * (kind == MK_LANE ? 2 : 1);  // TILE = 4 waves x 64
  return block_mode ? wcnt + (block_mode == 1 ? (4u << MATCH_SKETCH_BITS) : 0u) : 0u;
}

// The fused-kernel instance a pass launches (nullptr: none is built for the run); the occupancy query and the launch
// both take it from here.  Instances (kernels_match_lane_inst.hpp): k_match_t on 120-base buckets for records of 4, 8,
// 12 words and on wide ones for 4 to 16, each for 1-4 windows and three X modes; the geometry-specialised
// k_match_t<8, 2, 0, false, 1>; k_match_g<8, 0 | 1>.
typedef Inst<match_kernel_t> MatchInst;  // pointer and descriptor from one table entry, as on the two-kernel path
#define INST_T(RW, W, XM, WD, SG) MatchInst{k_match_t<RW, W, XM, WD, SG>, inst_id(MUSC_INST_MATCH_T, RW, W, XM, WD, SG)}
#define INST_G(RW, SG) MatchInst{k_match_g<RW, SG>, inst_id(MUSC_INST_MATCH_G, RW, 0, 0, 0, SG)}
template <int RW, bool WD>
static MatchInst lane_instance(int W, int xm) {
  static const MatchInst k[4][3] = {
      {INST_T(RW, 1, 0, WD, 0), INST_T(RW, 1, 1, WD, 0), INST_T(RW, 1, 2, WD, 0)},
      {INST_T(RW, 2, 0, WD, 0), INST_T(RW, 2, 1, WD, 0), INST_T(RW, 2, 2, WD, 0)},
      {INST_T(RW, 3, 0, WD, 0), INST_T(RW, 3, 1, WD, 0), INST_T(RW, 3, 2, WD, 0)},
      {INST_T(RW, 4, 0, WD, 0), INST_T(RW, 4, 1, WD, 0), INST_T(RW, 4, 2, WD, 0)}};
  return k[(W >= 1 && W <= 3 ? W : 4) - 1][xm];
}

// (kind, spec_geom: what match_kind and spec_geom_matches decided for the run)
static MatchInst match_instance(int kind, int spec_geom, int rw, bool wide, int W, int xm) {
  if (kind == MK_DMA) return spec_geom == 1 ? INST_G(8, 1) : INST_G(8, 0);
  if (spec_geom == 1) return INST_T(8, 2, 0, false, 1);  // (chosen by spec_geom_matches: every specialised quantity equals the run's)
  return by_rw(rw, [&](auto r) -> MatchInst {
    constexpr int RW = decltype(r)::value;
    if constexpr (RW == 0) return MatchInst{nullptr, 0};
    else if (wide) return lane_instance<RW, true>(W, xm);
    else if constexpr (RW <= 12) return lane_instance<RW, false>(W, xm);
    else return MatchInst{nullptr, 0};
  });
}

// workgroups of the kernel that are resident at once on this device: the persistent grid
static unsigned match_resident(musc_ctx* c, match_kernel_t kern, int W, int block_mode) {
  int per_cu = 0, ncu = 0;
  const size_t lds = match_dyn_lds(match_kind(c, W), W, block_mode);
  const void* fn = reinterpret_cast<const void*>(kern);
  hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, TILE, lds);
  if (e != hipSuccess || per_cu < 1) { (void)hipGetLastError(); per_cu = 2; }
  // The occupancy query counts LDS to the byte; the hardware hands it out in larger pieces
  // (measured on gfx950: 3 x 54 208 B did not fit a CU's 160 KB, 3 x 52 160 B did), and a grid one
  // workgroup per CU too large runs its last third as a second round (+45 % on cfg3).  Bound the
  // count with 2 KB pieces.
  hipFuncAttributes fa;
  if (hipFuncGetAttributes(&fa, fn) == hipSuccess) {
    const size_t total = ((size_t)fa.sharedSizeBytes + lds + 2047) / 2048 * 2048;
    const int fit = total ? (int)((160u << 10) / total) : per_cu;
    if (fit >= 1 && fit < per_cu) per_cu = fit;
  } else {
    (void)hipGetLastError();
  }
  if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess || ncu < 1) ncu = 256;
  unsigned resident = (unsigned)per_cu * (unsigned)ncu;
  if (c->env.debug_grid >= 1 && (unsigned)c->env.debug_grid < resident) resident = (unsigned)c->env.debug_grid;  // tests: a small grid makes every wave walk many wave-tiles of a small input
  return resident;
}

static void launch_match(musc_ctx* c, const PassPlan& pl, uint64_t r0, uint32_t n, unsigned ngrid) {
  const size_t lds = match_dyn_lds(match_kind(c, pl.pp.W), pl.pp.W, pl.block_mode);
  const uint32_t* const rdx = c->reads_have_x ? (const uint32_t*)c->rdx.p : (const uint32_t*)nullptr;
  hipLaunchKernelGGL(pl.kern, dim3(ngrid), dim3(TILE), lds, c->stream, c->rd, r0, n, c->d_mp, c->nmiss_tab.p, static_cast<const CtxBucket*>(c->ctx_T.p),
                     static_cast<const CtxEntry*>(c->ctx_E.p), c->stage.p, c->stage.cap, c->spill.p, c->spill.cap, c->bs[0].tbase.p, c->tcount2.p,
                     pl.block_mode, pl.block_thr, c->block_table.p, c->counters, rdx);
}

// The geometry-specialised instance a pass may launch: SpecGeom<g> is taken only when EVERY quantity it turns into
// a constant equals the run's -- window width, window starts, context offset, MinDinuc, the first-window sets, and
// the TABLE: a direct table of 2 * ww bits (cfg2's 10^8-base database gets a hashed 2^27-bucket table for the same
// ww: the general instance) -- and the instance exists for this record stride / bucket width / X mode.  Reads of
// other lengths than the geometry's are fine: the instance falls back to per-lane length masks for such a tile.
// MUSC_NO_SPEC=1 keeps every pass on the general instances (A/B runs, tests).
template <int SG>
static bool spec_geom_equals(const MatchParams& mp) {
  typedef SpecGeom<SG> G;
  if (mp.W != G::nwin || mp.ww != G::ww || mp.CL != G::CL || mp.min_dinuc != G::min_dinuc || mp.direct != 1 || mp.bits != 2 * G::ww) return false;
  for (int k = 0; k < G::nwin; k++)
    if (mp.win[k] != G::win[k] || mp.need[k] != (1u << k) - 1u) return false;
  return true;
}
static int spec_geom_matches(const musc_ctx* c, const MatchParams& mp) {
  if (c->env.no_spec) return 0;
  if (c->rw != 8 || idx_is_wide(c) || c->db_has_x || c->reads_have_x) return 0;  // the instances that exist: <8, 2, 0, false, g>
  return spec_geom_equals<1>(mp) ? 1 : 0;
}

// The fused path's share of the set-up: the run's parameter block (and with it the kernel instance: it
// depends on c->spec_geom), the instance, its persistent grid
static int match_setup(musc_ctx* c, PassPlan* pl) {
  const PathParams& pp = pl->pp;
  if (c->rw != 4 && c->rw != 8 && c->rw != 12 && !(c->rw == 16 && idx_is_wide(c)))
    return fail(c, 12, "internal: record stride %d on the context path", c->rw);
  static thread_local MatchParams mp;  // 16 KB with its mask tables: not on the stack
  memset(&mp, 0, sizeof mp);
  mp.W = pp.W; mp.ww = pp.ww; mp.min_dinuc = pp.min_dinuc; mp.bits = pp.bits; mp.direct = pp.direct;
  mp.mmtol = pp.mmtol; mp.apply_mmtol = pp.apply_mmtol; mp.max_len = pp.max_len; mp.CL = c->idx.CL;
  mp.q1zero_mask = pp.q1zero_mask;
  mp.seq_off = c->db_has_x ? c->seq_off : nullptr;
  mp.dbm2 = c->db_has_x ? c->dbm2 : nullptr;
  for (int k = 0; k < pp.W && k < CTX_MAX_W; k++) mp.win[k] = pp.win[k];
  match_tables(mp);
  c->spec_geom = spec_geom_matches(c, mp);
  c->stats.match_variant = (match_kind(c, pp.W) == MK_DMA ? 4u : 2u) + (c->spec_geom ? 1u : 0u);
  if (!c->h_mp_valid || memcmp(&mp, &c->h_mp, sizeof mp) != 0) {
    c->h_mp = mp;
    HIPCHK(c, hipMemcpyAsync(c->d_mp, &c->h_mp, sizeof mp, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->h_mp_valid = true;
  }
  // the persistent grid = the workgroups that are resident at once (every wave then sees many
  // wave-tiles and the end-of-kernel atomics stay few)
  // (a grid of 2 to 16 times the resident workgroups, dispatched dynamically, is slower: 1.03 to 1.11 ms against 0.98-0.99 on
  // cfg3, profiles/r04_ab_shape_spec_dma.txt -- the waves that finish early leave their share of the memory system to the slow ones)
  const int xm = c->db_has_x ? 2 : c->reads_have_x ? 1 : 0;
  const MatchInst inst = match_instance(match_kind(c, pp.W), c->spec_geom, c->rw, idx_is_wide(c), pp.W, xm);
  pl->kern = inst.fn;
  c->last_inst[0] = inst.id;
  if (!pl->kern) return fail(c, 12, "internal: no fused kernel instance for record stride %d, %d windows", c->rw, pp.W);
  pl->resident = match_resident(c, pl->kern, pp.W, pl->block_mode);
  return 0;
}

// Everything an attempt settles before its first batch, the same way on both paths: fresh stats, the
// parameter blocks and the nmiss table on the device, a cleared pass block, the MaxMatches block mode, whether the
// pass is sized, and where its batches come from.
static int pass_setup(musc_ctx* c, const musc_params* P, PassPlan* pl, BatchCursor* cur) {
  int rc = 0;
  const float keep_index_ms = c->stats.ms_index_build;
  memset(&c->stats, 0, sizeof c->stats);
  c->stats.ms_index_build = keep_index_ms;
  c->stats.n_reads = c->nreads;
  c->nhits = 0;

  pl->P = P;
  PathParams& pp = pl->pp;
  memset(&pp, 0, sizeof pp);
  pp.W = P->n_windows;
  pp.ww = P->window_width;
  pp.min_dinuc = P->min_dinuc;
  pp.bits = c->idx.bits;
  pp.direct = c->idx.direct;
  pp.mmtol = P->mmtol > 0xFFFF ? 0xFFFF : P->mmtol;
  pp.apply_mmtol = P->apply_mmtol;
  pp.wide = c->wide;
  pp.max_len = (int32_t)c->max_len;
  for (int k = 0; k < pp.W; k++) {
    pp.win[k] = P->windows[k];
    if (P->windows[k] == 0) pp.q1zero_mask |= 1u << k;
  }

  if (c->nm.pmatch != P->pmatch || c->nm.mmp1 != P->max_mismatch_p1 || c->nm.maxlen != c->max_len || !c->nmiss_tab.p) {
    const std::vector<uint16_t> tab = nmiss_budget(P, c->max_len);
    if ((rc = ensure(c, c->nmiss_tab, tab.size()))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->nmiss_tab.p, tab.data(), tab.size() * 2, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // tab goes out of scope
    c->nm.pmatch = P->pmatch;
    c->nm.mmp1 = P->max_mismatch_p1;
    c->nm.maxlen = c->max_len;
  }

  HIPCHK(c, hipMemsetAsync(c->counters, 0, CNT_PASS_WORDS * sizeof(unsigned long long), c->stream));
  // MaxMatches accounting (see k_confirm): screening first, exact only if inconclusive
  // (a pass that starts with an upload in flight runs on the upload's schedule, stream_plan: its batch count)
  pl->planned_batches = c->up.active ? std::max<uint64_t>(c->up.plan.batch_end.size(), 1)
                                     : (c->nreads + c->batch_reads - 1) / c->batch_reads + 1;
  pl->max_matches = P->max_matches > 0 ? (uint64_t)P->max_matches : 0x7FFFFFFFull;
  if (P->n_shards > 1) pl->max_matches /= (uint64_t)P->n_shards;  // this context sees one shard of each block
  // The screening threshold is per workgroup-launch, so it follows the grid -- and the two paths bound their grids
  // differently on purpose: k_confirm's by the host constant MAX_GRID, a fused kernel's by the workgroups resident at
  // once (match_setup, further down: it needs the block mode decided here for the kernel's LDS).
  auto thr_for = [&](uint64_t grid) { return (uint32_t)std::min<uint64_t>(pl->max_matches / (pl->planned_batches * grid), 0x7FFFFFFFull); };
  const uint32_t thr_host = thr_for(MAX_GRID);
  const bool known_exact = c->exact.key == c->pass_key(*P, 2);
  pl->block_mode = P->skip_block_check ? 0 : (c->force_exact_blocks || known_exact || thr_host < 2 ? 2 : 1);
  if (pl->block_mode == 2) {
    if ((rc = ensure(c, c->block_table, 1ull << BLOCK_TABLE_BITS))) return rc;
    HIPCHK(c, hipMemsetAsync(c->block_table.p, 0, (1ull << BLOCK_TABLE_BITS) * 4, c->stream));
  }
  if (!c->h_pp_valid || memcmp(&pp, &c->h_pp, sizeof pp) != 0) {
    c->h_pp = pp;
    HIPCHK(c, hipMemcpyAsync(c->d_pp, &c->h_pp, sizeof pp, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->h_pp_valid = true;
  }
  c->stats.index_kind = c->idx.kind;
  c->last_inst[0] = c->last_inst[1] = c->last_inst[2] = 0;  // (the resolvers of this pass fill them in)
  c->last_inst[3] = (uint32_t)pl->block_mode | (c->force_exact_blocks ? 0x100u : 0u);
  c->stats.index_bytes = ((1ull << c->idx.bits) + 1) * musc_index::bucket_bytes(c->idx.kind) +
                         (idx_is_ctx(c) ? ctx_entries_bytes(c->idx_novf + 16, idx_is_wide(c)) : (c->idx_novf + 16) * sizeof(uint4));
  if (idx_is_ctx(c)) {
    if ((rc = match_setup(c, pl))) return rc;
    const uint32_t thr_resident = thr_for(pl->resident);
    if (pl->block_mode == 1 && thr_resident < 2) {  // (the pass clears the table with its batch block)
      pl->block_mode = 2;
      c->last_inst[3] = 2u | (c->force_exact_blocks ? 0x100u : 0u);
      if (!c->block_table.p && (rc = ensure(c, c->block_table, 1ull << BLOCK_TABLE_BITS))) return rc;
    }
    pl->block_thr = thr_resident;
  } else {
    pl->block_thr = thr_host;
  }
  pl->mask = c->reads_have_x || c->db_has_x;  // (a stale all-zero plane of an earlier batch does not count)

  pl->sized = c->sized.key == c->pass_key(*P, pl->block_mode == 2 ? 2 : 0) && !c->env.debug_sync;
  cur->bsz = pl->sized ? c->sized.bsz : c->batch_reads;
  cur->plan = c->up.active && !pl->sized ? &c->up.plan : nullptr;
  return 0;
}

// all CNT_WORDS counters into the pinned mirror, now (a careful pass, after each batch)
static int pass_peek(musc_ctx* c) {
  HIPCHK(c, hipMemcpyAsync(c->h_pinned, c->counters, CNT_WORDS * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

// a careful pass: room for the per-tile words of a batch of ntiles tiles (both paths scan and compact the same way)
static int ensure_tiles(musc_ctx* c, musc_ctx::BatchSet& b, uint32_t ntiles) {
  int rc;
  if ((rc = ensure(c, b.tbase, (uint64_t)ntiles + 1)) || (rc = ensure(c, c->scan_tmp, scan_tmp_elems((uint64_t)ntiles + 1))) ||
      (rc = ensure(c, c->tcount2, (uint64_t)ntiles + 1)) || (rc = ensure(c, c->tpre, (uint64_t)ntiles + 1)))
    return rc;
  return 0;
}

// scan of the per-tile tuple counts -> the staged tuples to their place in `hits` -> the hit cursor moves on
static int launch_compact(musc_ctx* c, Timer& tm, decltype(&k_compact) compact, dim3 grid, uint32_t ntiles, const uint32_t* tbase,
                          hipStream_t st) {
  tm.begin(4, st);
  tm.begin(1, st);
  const int rc = scan_u32(c, c->tcount2.p, c->tpre.p, (uint64_t)ntiles + 1, false, c->scan_tmp.p, st);
  if (rc) return rc;
  tm.end(1, st);
  hipLaunchKernelGGL(compact, grid, dim3(256), 0, st, ntiles, tbase, c->tcount2.p, c->tpre.p, c->stage.p,
                     reinterpret_cast<uint4*>(c->hits.p), c->hits.cap, c->counters);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_advance, dim3(1), dim3(64), 0, st, c->tpre.p, ntiles, c->counters);
  HIPCHK(c, hipGetLastError());
  tm.end(4, st);
  return 0;
}

// The last launches of a pass: the count of full blocks (mode 2), the closing event (not inside a capture), the read-back
static int pass_close(musc_ctx* c, const PassPlan& pl, hipEvent_t ev1) {
  if (pl.block_mode == 2) {
    hipLaunchKernelGGL(k_block_overflow, dim3(1024), dim3(256), 0, c->stream, c->block_table.p, (uint32_t)pl.max_matches,
                       c->counters);
    HIPCHK(c, hipGetLastError());
  }
  if (ev1) HIPCHK(c, hipEventRecord(ev1, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->h_pinned, c->counters, CNT_WORDS * 8, hipMemcpyDeviceToHost, c->stream));
  return 0;
}

// The end of an attempt on either path: wait for the read-back, read the flags, fill the stats, judge the MaxMatches
// screening, and leave the sizing behind.  tot: the batch-block totals a careful pass added up (a sized pass reads
// them from the block itself, which it cleared once).
static int pass_verdict(musc_ctx* c, const PassPlan& pl, const BatchCursor& cur, const uint64_t* tot, PassClock& clk,
                        PassOutcome* what) {
  const bool fused = idx_is_ctx(c);
  c->last_pp = pl.pp;
  c->last_max_matches = (uint32_t)pl.max_matches;
  c->last_exact_blocks = pl.block_mode == 2;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const uint64_t* h = c->h_pinned;
  if (h[CNT_FLAGS] & FLAG_SPEC_REFUSED)
    return fail(c, 12, "internal: the kernel instance specialised for geometry %d refused this run's parameters", c->spec_geom);
  if (h[CNT_FLAGS]) {
    if (!pl.sized) return fail(c, 12, "internal: a capacity guard fired although every batch was sized (flags %llu)",
                               (unsigned long long)h[CNT_FLAGS]);
    *what = PASS_RERUN_CAREFUL;
    return 0;
  }
  if (pl.sized) tot = h + CNT_BATCH;  // the batch block accumulated over the whole pass
  c->stats.n_accepted = h[CNT_ACCEPTED];
  c->stats.n_hits = c->nhits = h[CNT_HITS];
  c->stats.n_overflow_blocks = pl.block_mode ? h[CNT_OVF_BLOCKS] : ~0ull;
  if (pl.block_mode == 1 && (h[CNT_HOT] || c->stats.n_batches > pl.planned_batches)) {
    *what = PASS_RERUN_EXACT;
    return 0;
  }
  c->stats.ms_screen = clk.tm.total(0);
  c->stats.ms_scan = clk.tm.total(1);
  c->stats.ms_confirm = clk.tm.total(3);
  c->stats.ms_select = clk.tm.total(4);
  (void)hipEventElapsedTime(&c->stats.ms_total, clk.ev0, clk.ev1);
  const uint64_t rec_b = (2 * (uint64_t)c->max_len + 7) / 8;
  c->stats.n_candidates = tot[fused ? MB_CAND : SB_CAND];
  c->stats.n_read_windows = tot[fused ? MB_WINDOWS : SB_WINDOWS];
  if (fused) {
    c->stats.n_pairs = tot[MB_CMP];
    c->stats.n_overflow_entries = tot[MB_OVF];
    const uint64_t ent_b = idx_is_wide(c) ? sizeof(CtxEntryW) : sizeof(CtxEntry);
    c->stats.match_bytes = c->nreads * rec_b + tot[MB_WINDOWS] * sizeof(CtxBucket) + tot[MB_OVF] * ent_b + 16 * c->stats.n_hits;
    c->stats.match_bytes_strict = c->nreads * rec_b + tot[MB_WINDOWS] * 8 + tot[MB_CAND] * ent_b + 16 * c->stats.n_hits;
  } else {
    c->stats.n_descriptors = tot[SB_PAIRS];
    c->stats.n_pairs = tot[SB_PAIRS] + tot[SB_TWO];  // a two-window descriptor is two of the reference's candidate pairs
    // (billed per DESCRIPTOR: one that stands for two windows is two of the reference's pairs but is fetched once;
    // the formulas of all three byte counts: musc_stats, include/muscato_hip.h)
    c->stats.confirm_bytes = c->stats.n_descriptors * (12 + rec_b + rec_b + 1) + 16 * c->stats.n_hits;
    if (!pl.sized && c->env.pipeline) {  // the second batch set gets the capacities the first one ended up with
      int rc;
      if ((rc = ensure(c, c->bs[1].wb, c->bs[0].wb.cap)) || (rc = ensure(c, c->bs[1].rvalid, c->bs[0].rvalid.cap)) ||
          (rc = ensure(c, c->bs[1].tbase, c->bs[0].tbase.cap)) || (rc = ensure(c, c->bs[1].tcount, c->bs[0].tcount.cap)) ||
          (rc = ensure(c, c->bs[1].cdesc, c->bs[0].cdesc.cap)))
        return rc;
    }
  }
  // (a streamed pass leaves the context unsized: BatchCursor)
  c->sized.key = cur.plan ? musc_state::PassKey() : c->pass_key(*pl.P, pl.block_mode == 2 ? 2 : 0);
  c->sized.bsz = cur.bsz;
  return 0;
}

// One attempt on context buckets: per batch k_match (screen + confirm + select, tuples staged per
// workgroup) -> scan of the per-tile tuple counts -> k_compact_w.  The only data-dependent
// capacities are the staging region and the spill region of a workgroup; a careful pass sizes them: a batch that does
// not fit makes the WHOLE pass start over with larger buffers (its kernels have already added the batch to the pass
// block), at most 40 times.
static int pass_fused(musc_ctx* c, const PassPlan& pl, BatchCursor cur, PassOutcome* what) {
  int rc = 0;
  const bool sized = pl.sized;
  // A sized pass can be replayed as a hipGraph (MUSC_GRAPH=1): its launches, the counter memsets
  // and the final readback are captured once per (reads, database, parameters) and then cost one
  // launch per pass.  Every buffer of a sized pass is fixed, so the captured arguments stay valid;
  // any pass that sizes drops the graph.
  const bool use_graph = sized && c->env.graph > 0 && !c->graph.failed;
  if (!sized) c->graph.drop();
  // A batch's staged tuples go to their place in `hits` by a k_compact_w of their own.  (r02 / r03 moved them from inside
  // the NEXT batch's match launch instead; r04's A/B on cfg3 / the cfg4 shard, profiles/r04_ab_shape_spec_dma.txt: the pass
  // takes the same time either way, but the match launch grows by work its algorithmic bytes do not bill.)
  for (int attempt = 0;; attempt++) {
    if (attempt > 40) return fail(c, 12, "internal: the context pass did not converge on buffer sizes");
    PassClock clk(c);
    if (!clk.ev0 || !clk.ev1) return fail(c, 10, "hipEventCreate failed");
    const bool replay = use_graph && c->graph.exec && c->graph.key == c->pass_key(*pl.P, pl.block_mode);
    const bool capture = use_graph && !replay;
    if (capture) c->graph.drop();
    clk.tm.off = capture || replay;
    CaptureGuard cap;  // (ends the capture if this attempt leaves early)
    if (capture) {
      if (cap.begin(c->stream) != hipSuccess) {  // no capture on this stream: the plain sized pass
        (void)hipGetLastError();
        *what = PASS_RERUN_NO_GRAPH;
        return 0;
      }
    } else if (!replay) {
      HIPCHK(c, hipEventRecord(clk.ev0, c->stream));
    }
    uint64_t tot[CNT_BATCH_WORDS] = {0}, r0 = 0;
    c->stats.n_batches = c->stats.match_launches = 0;
    bool again = false;
    if (!replay) {
      HIPCHK(c, hipMemsetAsync(c->counters, 0, CNT_WORDS * sizeof(unsigned long long), c->stream));
      if (pl.block_mode == 2) HIPCHK(c, hipMemsetAsync(c->block_table.p, 0, (1ull << BLOCK_TABLE_BITS) * 4, c->stream));
    }
    while (!replay && r0 < c->nreads) {
      const uint32_t n = cur.reads_at(r0, c->nreads);
      const uint32_t ntiles = nblk(n, WT);  // wave-tiles of 64 reads
      const uint64_t sgrid = std::min<uint64_t>(nblk(n, TILE), pl.resident);
      const uint64_t swaves = sgrid * (TILE / 64);  // regions of stage and spill are per wave
      if (!sized) {
        if ((rc = ensure_tiles(c, c->bs[0], ntiles)) ||
            (rc = ensure(c, c->stage, std::max<uint64_t>(FIRST_PASS_TUPLES_PER_READ * n, swaves * 64))) ||
            (rc = ensure(c, c->spill, swaves * 32)))
          return rc;
        HIPCHK(c, hipMemsetAsync(c->counters + CNT_BATCH, 0, CNT_BATCH_WORDS * sizeof(unsigned long long), c->stream));
      }
      if ((rc = upload_prepare(c, r0, n, c->stream))) return rc;  // (reads still on their way from the host)
      clk.tm.begin(0);
      {
        Range rg("k_match");
        launch_match(c, pl, r0, n, (unsigned)sgrid);
      }
      HIPCHK(c, hipGetLastError());
      clk.tm.end(0);
      c->stats.match_launches++;
      c->stats.n_batches++;
      if (!sized) {
        if ((rc = pass_peek(c))) return rc;
        const uint64_t* h = c->h_pinned;
        // (k_match_t keeps a spill region per wave and wave-tile parity)
        const uint64_t need_stage = h[CNT_BATCH + MB_STAGE_MAX] * swaves, need_spill = 2 * h[CNT_BATCH + MB_SPILL_MAX] * swaves;
        if (need_stage > BATCH_OFFSET_CAP) {
          if (n == 1) return fail(c, 6, "one read has %llu tuples (> 2^31)", (unsigned long long)h[CNT_BATCH + MB_STAGE_MAX]);
          cur.halve(n);
          again = true;
          break;
        }
        if (h[CNT_FLAGS] & FLAG_SPEC_REFUSED)
          return fail(c, 12, "internal: the kernel instance specialised for geometry %d refused this run's parameters", c->spec_geom);
        if (h[CNT_FLAGS] || need_stage > c->stage.cap || need_spill > c->spill.cap) {
          // room for every workgroup's tuples / spilled candidates, then the pass starts over
          if (need_stage > c->stage.cap && (rc = ensure(c, c->stage, need_stage + need_stage / 4 + swaves))) return rc;
          if (need_spill > c->spill.cap && (rc = ensure(c, c->spill, need_spill + need_spill / 4 + swaves))) return rc;
          again = true;
          break;
        }
        for (int i = 0; i < CNT_BATCH_WORDS; i++) tot[i] += h[CNT_BATCH + i];  // (the *_MAX slots mean nothing in tot)
        if ((rc = ensure(c, c->hits, h[CNT_HITS] + h[CNT_BATCH + MB_TUPLES], true))) return rc;
      }
      Range rgc("scan + k_compact_w");
      const dim3 cgrid(std::min(nblk(ntiles, 4), 4u * MAX_GRID));
      if ((rc = launch_compact(c, clk.tm, k_compact_w, cgrid, ntiles, c->bs[0].tbase.p, c->stream))) return rc;
      r0 += n;
    }
    if (again) continue;
    if (!replay && (rc = pass_close(c, pl, capture ? nullptr : clk.ev1))) return rc;
    if (capture) {
      hipGraph_t g = nullptr;
      hipError_t ge = cap.end(&g);
      if (ge == hipSuccess) ge = hipGraphInstantiate(&c->graph.exec, g, nullptr, nullptr, 0);
      if (g) (void)hipGraphDestroy(g);
      if (ge != hipSuccess) {  // the graph is an optimisation: without it the pass runs launch by launch
        (void)hipGetLastError();
        c->graph.exec = nullptr;
        *what = PASS_RERUN_NO_GRAPH;
        return 0;
      }
      c->graph.key = c->pass_key(*pl.P, pl.block_mode);
      c->graph.batches = c->stats.n_batches;
    }
    if (capture || replay) {
      c->stats.n_batches = c->stats.match_launches = c->graph.batches;
      HIPCHK(c, hipEventRecord(clk.ev0, c->stream));
      HIPCHK(c, hipGraphLaunch(c->graph.exec, c->stream));
      HIPCHK(c, hipEventRecord(clk.ev1, c->stream));
    }
    return pass_verdict(c, pl, cur, tot, clk, what);
  }
}

// One attempt on the two-kernel path.  Per batch: k_screen claims descriptor space as it goes; if a batch of a careful
// pass needs more than the buffer holds it reports how much, and the BATCH is repeated after growing the buffer (the
// pass block is untouched by k_screen but for the flag word, which is cleared).
static int pass_two_kernel(musc_ctx* c, const PassPlan& pl, BatchCursor cur, PassOutcome* what) {
  int rc = 0;
  PassClock clk(c);
  if (!clk.ev0 || !clk.ev1) return fail(c, 10, "hipEventCreate failed");
  HIPCHK(c, hipEventRecord(clk.ev0, c->stream));

  // a mask plane on only one side: allocate the missing all-zero plane once
  if (pl.mask && !c->rdm && c->nreads) {
    const uint64_t words = c->nreads * (uint64_t)c->rw;
    HIPCHK(c, c->rdm.alloc(words * 4 + 256));
    HIPCHK(c, hipMemsetAsync(c->rdm, 0, words * 4 + 256, c->stream));
  }
  if (pl.mask && !c->dbm2) {
    HIPCHK(c, c->dbm2.alloc((c->db_words + 64) * 4));
    // (the index stays valid: bucket_of treats a null and an all-zero mask plane alike)
    HIPCHK(c, hipMemsetAsync(c->dbm2, 0, (c->db_words + 64) * 4, c->stream));
    if ((rc = db_xblocks(c))) return rc;
  }

  const bool sized = pl.sized;
  uint64_t tot[CNT_BATCH_WORDS] = {0}, r0 = 0;
  if (sized) HIPCHK(c, hipMemsetAsync(c->counters + CNT_BATCH, 0, CNT_BATCH_WORDS * sizeof(unsigned long long), c->stream));
  // MUSC_PIPELINE=1: a sized pass of several batches is pipelined over two streams, k_screen of
  // batch b+1 beside k_confirm + k_compact of batch b, alternating between the two batch sets.
  // Off by default: measured on cfg3 / cfg4 / cfg5 shards the pass moves ~5.6 TB/s of cache lines
  // through HBM either way (both kernels are bound by the lines they fetch), so overlapping them
  // gains nothing (5.66 vs 5.44 ms on cfg3) and the second set costs memory.
  const bool piped = sized && c->env.pipeline && c->nreads > cur.bsz && c->bs[1].cdesc.cap >= c->bs[0].cdesc.cap;
  hipStream_t sA = c->stream, sB = piped ? c->stream2 : c->stream;
  c->s_confirm = sB;
  c->cur = 0;
  if (piped) {  // the confirm stream starts after the memsets above
    HIPCHK(c, hipEventRecord(c->ev_join, sA));
    HIPCHK(c, hipStreamWaitEvent(sB, c->ev_join, 0));
  }
  uint32_t batch_no = 0;
  while (r0 < c->nreads) {
    const uint32_t n = cur.reads_at(r0, c->nreads);
    if (piped) {
      c->cur = (int)(batch_no & 1u);
      // the set is free once the batch before last has been compacted
      if (batch_no >= 2) HIPCHK(c, hipStreamWaitEvent(sA, c->ev_free[c->cur], 0));
    }
    auto& b = c->bs[c->cur];
    const uint32_t ntiles = nblk(n, TILE);
    uint64_t total = 1;  // pairs of this batch (unknown on a sized pass)
    if (!sized) {
      if ((rc = ensure_tiles(c, b, ntiles)) || (rc = ensure(c, b.tcount, (uint64_t)ntiles + 1)) ||
          (rc = ensure(c, b.wb, (uint64_t)n * pl.pp.W)) || (rc = ensure(c, b.rvalid, (uint64_t)n + 1)) ||
          (rc = ensure(c, b.cdesc, std::max<uint64_t>(FIRST_PASS_DESC_PER_READ * n, FIRST_PASS_DESC_MIN))))
        return rc;
      HIPCHK(c, hipMemsetAsync(c->counters + CNT_BATCH, 0, CNT_BATCH_WORDS * sizeof(unsigned long long), c->stream));
    }

    if ((rc = upload_prepare(c, r0, n, c->stream))) return rc;  // (reads still on their way from the host)
    clk.tm.begin(0);
    {
      Range rg("k_screen");
      launch_screen(c, pl, r0, n);
    }
    HIPCHK(c, hipGetLastError());
    clk.tm.end(0);
    if (piped) {
      HIPCHK(c, hipEventRecord(c->ev_ready[c->cur], sA));
      HIPCHK(c, hipStreamWaitEvent(sB, c->ev_ready[c->cur], 0));
    }
    if (!sized) {
      if ((rc = pass_peek(c))) return rc;
      const uint64_t* h = c->h_pinned;
      total = h[CNT_BATCH + SB_PAIRS];
      const uint64_t sgrid = screen_grid(c, n, pl.mask);
      const uint64_t region = h[CNT_BATCH + SB_DESC_MAX], need = region * sgrid;  // every workgroup region as large as the fullest
      if (need > BATCH_OFFSET_CAP || region > b.cdesc.cap / sgrid) {
        if (need > BATCH_OFFSET_CAP) {  // too many pairs for one launch: this range again with half the reads
          if (n == 1) return fail(c, 6, "one read has %llu candidate pairs (> 2^31)", (unsigned long long)total);
          cur.halve(n);
        } else if ((rc = ensure(c, b.cdesc, need + need / 8 + sgrid))) {  // room for every workgroup's pairs
          return rc;
        }
        HIPCHK(c, hipMemsetAsync(c->counters + CNT_FLAGS, 0, 8, c->stream));
        continue;  // repeat the batch
      }
      for (int i = 0; i < CNT_BATCH_WORDS; i++) tot[i] += h[CNT_BATCH + i];  // (the *_MAX slots mean nothing in tot)
      if ((rc = ensure(c, c->p_nx, b.cdesc.cap))) return rc;
      if ((rc = ensure(c, c->stage, b.cdesc.cap))) return rc;
      if ((rc = ensure(c, c->hits, h[CNT_HITS] + total, true))) return rc;
    }
    c->stats.n_batches++;

    if (total) {
      clk.tm.begin(3, sB);
      {
        Range rg("k_confirm");
        launch_confirm(c, pl, r0, n);
      }
      HIPCHK(c, hipGetLastError());
      clk.tm.end(3, sB);
      c->stats.confirm_launches++;

      Range rgc("scan + k_compact");
      const dim3 cgrid(std::min(nblk(n, TILE), MAX_GRID));
      if ((rc = launch_compact(c, clk.tm, k_compact, cgrid, ntiles, b.tbase.p, sB))) return rc;
    }
    if (piped) HIPCHK(c, hipEventRecord(c->ev_free[c->cur], sB));
    r0 += n;
    batch_no++;
  }
  if (piped) {  // join: everything below is ordered after both streams
    HIPCHK(c, hipEventRecord(c->ev_join, sB));
    HIPCHK(c, hipStreamWaitEvent(sA, c->ev_join, 0));
  }
  c->cur = 0;
  c->s_confirm = c->stream;
  if ((rc = pass_close(c, pl, clk.ev1))) return rc;
  return pass_verdict(c, pl, cur, tot, clk, what);
}

// One pass over the resident index (of the whole database, or of partition cur_part of a partitioned pass): attempts
// until one is done.  Every attempt starts from scratch -- ensure_index, then in pass_setup fresh stats (ms_index_build
// kept), no hits, last_inst cleared, the pass block cleared, the block table ensured and cleared in mode 2 -- and what
// a rerun changes against the attempt before it is set HERE and nowhere else.
static int match_index_pass(musc_ctx* c, const musc_params* P, uint64_t* nhits) {
  bool forced_exact = false;
  int rc = 0;
  for (;;) {
    PassPlan pl;
    BatchCursor cur;
    PassOutcome what = PASS_DONE;
    if ((rc = ensure_index(c, P, c->max_len))) break;
    if (nhits) *nhits = 0;
    if ((rc = pass_setup(c, P, &pl, &cur))) break;
    rc = idx_is_ctx(c) ? pass_fused(c, pl, cur, &what) : pass_two_kernel(c, pl, cur, &what);
    if (rc || what == PASS_DONE) break;
    if (what == PASS_RERUN_CAREFUL) {
      c->sized.key = musc_state::PassKey();
    } else if (what == PASS_RERUN_NO_GRAPH) {
      c->graph.failed = true;
    } else {  // PASS_RERUN_EXACT: this attempt chain runs exact, and later passes over the same inputs start exact
      c->force_exact_blocks = forced_exact = true;
      c->exact.key = c->pass_key(*P, 2);
    }
  }
  if (forced_exact) c->force_exact_blocks = false;
  if (!rc && nhits) *nhits = c->nhits;
  return rc;
}

static int match_device_impl(musc_ctx* c, const musc_params* P, uint64_t* nhits) {
  Range rg_pass("musc_match_device");
  int rc = check_params(c, P);
  if (rc) return rc;
  if (!c->db2) return fail(c, 4, "no database loaded");
  if (c->reads_failed || !c->rw) return fail(c, 4, "no reads loaded");  // (rw == 0: no load yet; a load of zero reads sets it)
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = plan_partitions(c, P, c->max_len))) return rc;
  c->cur_part = 0;
  if (c->part_first.size() > 2) return match_partitioned(c, P, nhits);
  return match_index_pass(c, P, nhits);
}

// musc_reads_load_packed32(async = 1) borrows the caller's host buffer "until the next musc_match* returns": that holds
// on every exit -- a pass that fails early (parameters, no database, an index that cannot be built, a HIP error in a
// batch) waits for the copies still queued on the upload stream before it returns.  The pieces stay valid on the
// device, so a later pass packs and matches them.
extern "C" int musc_match_device(musc_ctx* c, const musc_params* P, uint64_t* nhits) {
  if (!c) return 1;
  c->st.list_changes();  // (an order taken before is not this pass's; a pass that fails leaves no list)
  const int rc = match_device_impl(c, P, nhits);
  if (rc != 0 && c->up.active && c->up.s_up) (void)hipStreamSynchronize(c->up.s_up);
  if (rc == 0) {
    c->st.list_made(musc_state::LIST_PASS);
    c->mm_params = *P;  // musc_maxmatches_apply: the list and the parameters it replays
  }
  return rc;
}
