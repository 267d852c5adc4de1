// muscato_index.hpp -- the device side of the index layer: the one build driver and its three layouts, context-bucket
// eligibility, the partition planner and ensure_index, and the musc_db_build_index* / musc_db_*partition* entry points.
// It owns the resident index (musc_ctx::idx and the four tables) and acts on what index_plan.hpp decides: the planner
// and the builds ask the same cascade.  Part of libmuscato_hip.so: included by muscato_hip.hip after the context, the
// scans and the event pool it calls (fail, HIPCHK, ensure, TmpBufs, Readback, scan_u64, pool_event, check_params), behind the
// loaders (muscato_load.hpp: the database it indexes).
#pragma once

namespace mi = musc_index;

static_assert(sizeof(Bucket) == mi::BUCKET_BYTES && sizeof(LineBucket) == mi::LINE_BUCKET_BYTES && sizeof(uint4) == mi::ENTRY_BYTES,
              "index_plan.hpp sizes the window-start index with these");
static_assert(sizeof(CtxBucket) == mi::CTX_BUCKET_BYTES && sizeof(CtxEntry) == mi::CTX_ENTRY_BYTES && sizeof(CtxEntryW) == mi::CTX_ENTRYW_BYTES,
              "index_plan.hpp sizes the context index with these");

namespace {

void free_index(musc_ctx* c) {
  // (the allocations stay for the next build; musc_destroy releases them)
  c->idx = mi::Resident();
  c->st.index_freed();
}

// The targets (and their bases) an index build covers, and the base count its size-dependent choices are made on:
// the whole database, or one partition of a pass (then `size` is the largest partition's, so that every partition
// builds the same kind and size of table)
struct IdxRange {
  uint32_t g0, g1;
  uint64_t b0, b1, size;
};
IdxRange whole_db(const musc_ctx* c) { return IdxRange{0, c->nseq, 0, c->nbases, c->nbases}; }

// Device memory an index may take before the reserves: what is free plus what the resident tables hold.  Asked once per
// plan_partitions / ensure_index call.
uint64_t index_avail(const musc_ctx* c) {
  size_t mfree = 0, mtotal = 0;
  if (hipMemGetInfo(&mfree, &mtotal) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return (uint64_t)mfree + c->idx_T.bytes + c->idx_E.bytes + c->ctx_T.bytes + c->ctx_E.bytes;
}

// One index build over a table T of nb + 1 buckets of bucket_b bytes with overflow entries E, the same steps for every
// layout: count per bucket -> overflow sizes -> u64 scan (a 10 Gbp database has billions of overflow entries) ->
// offsets, then E is grown to the total and the entries are filled in.  The caller brings the launches -- count(cursor),
// sizes(tmp), set(tmp), fill(cursor) -- and cap(&novf, &bytes): the overflow total as entries and the bytes of E for
// them (an error code if they cannot be numbered).  cursors: one more zeroed u32 per bucket for count and fill.
// soft: an allocation that fails means "does not fit" (100: the caller falls back) instead of error 10.
template <class Count, class Sizes, class Set, class Cap, class Fill>
int build_index_table(musc_ctx* c, int bits, uint64_t bucket_b, bool cursors, bool soft, DevMem& T, DevMem& E,
                      Count count, Sizes sizes, Set set, Cap cap, Fill fill) {
  const uint64_t nb = 1ull << bits;
  auto no_mem = [&](hipError_t e, const char* what) {
    (void)hipGetLastError();
    return soft ? 100 : fail(c, 10, "hipMalloc of %s failed: %s", what, hipGetErrorString(e));
  };
  c->ev_used = 0;
  hipEvent_t e0 = pool_event(c), e1 = pool_event(c), e2 = pool_event(c), e3 = pool_event(c);
  if (!e0 || !e1 || !e2 || !e3) return fail(c, 10, "hipEventCreate failed");
  hipError_t e = T.grow((nb + 1) * bucket_b);
  if (e != hipSuccess) return no_mem(e, "the index table");
  TmpBufs B, Bc;
  uint64_t *tmp = nullptr, *stmp = nullptr;
  uint32_t* cursor = nullptr;
  if ((e = B.alloc(&tmp, (nb + 1 + 16) * 8)) != hipSuccess || (e = B.alloc(&stmp, scan_tmp_elems(nb + 1) * 8)) != hipSuccess ||
      (cursors && (e = Bc.alloc(&cursor, (nb + 1) * 4)) != hipSuccess))
    return no_mem(e, "the index build's temporaries");
  // timed: the device work (allocation above and below is host time, seconds for a 64 GiB table
  // the first time, and not repeated)
  HIPCHK(c, hipEventRecord(e0, c->stream));
  HIPCHK(c, hipMemsetAsync(T.p, 0, (nb + 1) * bucket_b, c->stream));
  if (cursor) HIPCHK(c, hipMemsetAsync(cursor, 0, (nb + 1) * 4, c->stream));
  count(cursor);
  HIPCHK(c, hipGetLastError());
  sizes(tmp);
  HIPCHK(c, hipGetLastError());
  int rc = scan_u64(c, tmp, tmp, nb + 1, stmp);
  if (rc) return rc;
  uint64_t novf = 0, e_bytes = 0;
  Readback R(c->scalars, c->stream);
  R.get(tmp + nb, &novf);
  set(tmp);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipEventRecord(e2, c->stream));
  HIPCHK(c, R.wait());
  B.release();  // 8 bytes per bucket: returned before the overflow array is allocated
  if ((rc = cap(&novf, &e_bytes))) return rc;
  c->idx_novf = novf;
  if ((e = E.grow(e_bytes)) != hipSuccess) return no_mem(e, "the index's overflow entries");
  HIPCHK(c, hipEventRecord(e3, c->stream));
  fill(cursor);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipEventRecord(e1, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  float ms = 0, ms2 = 0;
  (void)hipEventElapsedTime(&ms, e0, e2);
  (void)hipEventElapsedTime(&ms2, e3, e1);
  c->stats.ms_index_build = ms + ms2;
  return 0;
}

// The window-start index (kernels_index.hpp) over the targets of R, on 64-byte buckets or line buckets
template <class BT>
int build_window_index(musc_ctx* c, const mi::Resident& w, const IdxRange& R) {
  const uint64_t nb = 1ull << w.bits;
  const dim3 blocks = stage_grid(c, (R.b1 - R.b0 + 255) / 256, musc_launch::CAP_INDEX);
  auto T = [c] { return static_cast<BT*>(c->idx_T.p); };
  auto index = [&](auto filling, uint4* E) {
    if (R.b1 > R.b0)
      hipLaunchKernelGGL((k_index<decltype(filling)::value, BT>), blocks, dim3(256), 0, c->stream, c->db2, c->dbm2, c->seq_off, c->nseq,
                         R.b0, R.b1, w.ww, w.bits, w.direct, c->wide, T(), E);
  };
  return build_index_table(
      c, w.bits, sizeof(BT), false, false, c->idx_T, c->idx_E, [&](uint32_t*) { index(std::false_type{}, (uint4*)nullptr); },
      [&](uint64_t* tmp) { hipLaunchKernelGGL((k_index_ovf_count<BT>), dim3(nblk(nb + 1, 256)), dim3(256), 0, c->stream, T(), nb, tmp); },
      [&](uint64_t* tmp) { hipLaunchKernelGGL((k_index_ovf_set<BT>), dim3(nblk(nb, 256)), dim3(256), 0, c->stream, T(), nb, tmp); },
      [&](uint64_t* novf, uint64_t* bytes) {  // the total counts entries (64-byte buckets) or lines of eight entries (line buckets)
        if (std::is_same<BT, LineBucket>::value) {
          if (*novf >= 0xFFFFFFF0ull) return fail(c, 5, "internal: %llu overflow lines do not fit 32-bit numbers", (unsigned long long)*novf);
          *novf *= 8;
        }
        *bytes = (*novf + 16) * sizeof(uint4);
        return 0;
      },
      [&](uint32_t*) { index(std::true_type{}, static_cast<uint4*>(c->idx_E.p)); });
}

// Context buckets (kernels_match.hpp) for window width w.ww and w.CL bases of left context.  100: an allocation failed
int build_ctx_index(musc_ctx* c, const mi::Resident& w, const IdxRange& R) {
  const uint64_t nb = 1ull << w.bits;
  const bool wide = w.kind == mi::K_CTXW;
  const dim3 blocks = stage_grid(c, (R.b1 - R.b0 + 255) / 256, musc_launch::CAP_INDEX);
  // a database with X: its windows with an X stay out, entries whose context touches one are flagged
  const uint32_t* const xm2 = c->db_has_x ? c->dbm2 : nullptr;
  const uint32_t* const xbl = c->db_has_x ? c->dbx : nullptr;
  auto T = [c] { return static_cast<CtxBucket*>(c->ctx_T.p); };
  auto index = [&](auto kern, void* E, uint32_t* cursor) {
    if (R.b1 > R.b0)
      hipLaunchKernelGGL(kern, blocks, dim3(256), 0, c->stream, c->db2, xm2, xbl, c->seq_off, c->nseq, c->nbases, R.b0, R.b1, w.ww,
                         w.bits, w.direct, w.CL, T(), E, cursor);
  };
  return build_index_table(
      c, w.bits, sizeof(CtxBucket), true, true, c->ctx_T, c->ctx_E,
      // (the counting pass does not look at the entries: one instance serves both layouts)
      [&](uint32_t* cursor) { index(k_index_ctx<false, false>, nullptr, cursor); },
      [&](uint64_t* tmp) {
        hipLaunchKernelGGL(k_ctx_ovf_count, dim3(nblk(nb + 1, 256)), dim3(256), 0, c->stream, T(), nb, (uint32_t)(wide ? CTXW_INLINE : CTX_INLINE), tmp);
      },
      [&](uint64_t* tmp) { hipLaunchKernelGGL(k_ctx_ovf_set, dim3(nblk(nb, 256)), dim3(256), 0, c->stream, T(), nb, tmp); },
      [&](uint64_t* novf, uint64_t* bytes) {
        if (*novf >= 0xFFFFFFF0ull) return fail(c, 5, "internal: %llu overflow entries do not fit 32-bit offsets", (unsigned long long)*novf);
        *bytes = ctx_entries_bytes(*novf + 16, wide);  // (entries sit line-aligned: ctx_entry_word)
        return 0;
      },
      [&](uint32_t* cursor) {
        if (wide) index(k_index_ctx<true, true>, c->ctx_E.p, cursor);
        else index(k_index_ctx<true, false>, c->ctx_E.p, cursor);
      });
}

// Build the index `want` over R in place of the one in hand; one index kind is resident at a time, so the other
// kind's tables go first.  100: a context build whose allocation failed (nothing is resident then).
int build_index(musc_ctx* c, const mi::Resident& want, const IdxRange& R) {
  free_index(c);
  int rc;
  if (mi::is_ctx(want.kind)) {
    c->idx_T.release();
    c->idx_E.release();
    rc = build_ctx_index(c, want, R);
  } else {
    c->ctx_T.release();
    c->ctx_E.release();
    rc = want.kind == mi::K_LINES ? build_window_index<LineBucket>(c, want, R) : build_window_index<Bucket>(c, want, R);
  }
  if (!rc) c->idx = want;
  return rc;
}

// The xpos words of the reads in hand, in the format of the bucket width
bool reads_xpos(musc_ctx* c, int wide) {
  if (c->rdx_of.gen == c->st.g.pass_inputs && c->rdx_of.wide == wide) return true;
  if (ensure(c, c->rdx, c->nreads)) return false;
  if (wide)
    hipLaunchKernelGGL(k_read_xpos<true>, dim3(nblk(c->nreads, 256)), dim3(256), 0, c->stream, c->rd, c->rdm, c->nreads, c->rw, c->rdx.p);
  else
    hipLaunchKernelGGL(k_read_xpos<false>, dim3(nblk(c->nreads, 256)), dim3(256), 0, c->stream, c->rd, c->rdm, c->nreads, c->rw, c->rdx.p);
  if (hipGetLastError() != hipSuccess) return false;
  c->rdx_of.gen = c->st.g.pass_inputs;
  c->rdx_of.wide = wide;
  c->xok.gen = c->xokdb.gen = 0;
  return true;
}

// nmiss budget per read length 0 .. max_len + 1: int((1-PMatch)*float64(len)), IEEE double, truncation
// (cmd/muscato_confirm/main.go:198) -- evaluated on the host exactly as Go does; --MaxMismatch replaces it.
std::vector<uint16_t> nmiss_budget(const musc_params* P, uint32_t max_len) {
  std::vector<uint16_t> tab((size_t)max_len + 2);
  for (uint32_t L = 0; L < tab.size(); L++) {
    volatile double a = 1.0 - P->pmatch;
    volatile double b = a * (double)L;
    long long v = (long long)b;
    if (P->max_mismatch_p1 > 0) v = P->max_mismatch_p1 - 1;
    tab[L] = (uint16_t)std::min<long long>(std::max<long long>(v, 0), 0xFFFE);
  }
  return tab;
}

// Reads with X fit the context path if every read that holds more of them than its xpos word lists
// (XPos<wide>: four on 120-base buckets, three on wide ones) could not match anyway (that many
// mismatches exceed its budget int((1 - PMatch) * len)).  One small kernel and a 4-byte readback
// per (read set, bucket width, PMatch, MaxMismatch).
bool reads_x_fit(musc_ctx* c, const musc_params* P, uint32_t max_len, int wide) {
  if (!c->rdm || !c->rd || !c->nreads) return false;
  if (c->env.no_x_context) return false;
  if (!reads_xpos(c, wide)) return false;
  // (the budget table covers the reads in hand whatever length the caller planned the index for)
  max_len = std::max(max_len, c->max_len);
  if (c->xok.gen == c->st.g.pass_inputs && c->xok.pmatch == P->pmatch && c->xok.mmp1 == P->max_mismatch_p1) return c->xok.ok;
  const std::vector<uint16_t> tab = nmiss_budget(P, max_len);  // the budget musc_match_device applies
  TmpBufs B;
  uint16_t* d_tab = nullptr;
  uint32_t bad = 1;
  if (B.alloc(&d_tab, tab.size() * 2) != hipSuccess) return false;
  if (hipMemcpyAsync(d_tab, tab.data(), tab.size() * 2, hipMemcpyHostToDevice, c->stream) != hipSuccess) return false;
  if (hipMemsetAsync(c->d_flag, 0, 4, c->stream) != hipSuccess) return false;
  hipLaunchKernelGGL(k_xpos_check, dim3(nblk(c->nreads, 256)), dim3(256), 0, c->stream, c->rd, c->rdx.p, c->nreads, c->rw, d_tab,
                     max_len, wide ? XPos<true>::MAX : XPos<false>::MAX, c->d_flag);
  if (Readback(c->scalars, c->stream).get(c->d_flag.get(), &bad).wait() != hipSuccess) return false;
  c->xok.ok = bad == 0;
  c->xok.gen = c->st.g.pass_inputs;
  c->xok.pmatch = P->pmatch;
  c->xok.mmp1 = P->max_mismatch_p1;
  return c->xok.ok;
}

// Reads with X against a DATABASE with X fit the context path if every read lists all its X in its
// xpos word and none of them falls into one of the run's windows (k_xpos_check_db).
bool reads_x_fit_db(musc_ctx* c, const musc_params* P, int wide) {
  if (!c->rdm || !c->rd || !c->nreads) return false;
  if (!reads_xpos(c, wide)) return false;
  int32_t key[CTX_MAX_W + 3] = {P->n_windows, P->window_width, wide};
  XWins wn;
  memset(&wn, 0, sizeof wn);
  wn.n = P->n_windows;
  wn.ww = P->window_width;
  for (int k = 0; k < P->n_windows && k < CTX_MAX_W; k++) key[3 + k] = wn.q1[k] = P->windows[k];
  if (c->xokdb.gen == c->st.g.pass_inputs && std::equal(key, key + CTX_MAX_W + 3, c->xokdb.key)) return c->xokdb.ok;
  uint32_t bad = 1;
  if (hipMemsetAsync(c->d_flag, 0, 4, c->stream) != hipSuccess) return false;
  if (wide) hipLaunchKernelGGL(k_xpos_check_db<true>, dim3(nblk(c->nreads, 256)), dim3(256), 0, c->stream, c->rdx.p, c->nreads, wn, c->d_flag);
  else hipLaunchKernelGGL(k_xpos_check_db<false>, dim3(nblk(c->nreads, 256)), dim3(256), 0, c->stream, c->rdx.p, c->nreads, wn, c->d_flag);
  if (Readback(c->scalars, c->stream).get(c->d_flag.get(), &bad).wait() != hipSuccess) return false;
  c->xokdb.ok = bad == 0;
  c->xokdb.gen = c->st.g.pass_inputs;
  std::copy(key, key + CTX_MAX_W + 3, c->xokdb.key);
  return c->xokdb.ok;
}

// Which index a run with these parameters and reads of at most max_len bases uses: context
// buckets when every read fits the context around each of at most CTX_MAX_W windows -- 120 bases
// (three entries per bucket line) or, where k_match_t runs, 200 bases (two per line: *wide = 1) --
// the database holds no X (the context has no mask plane; reads may hold some where
// k_match_t runs, see reads_x_fit) and positions fit 32 bits.
bool ctx_eligible(musc_ctx* c, const musc_params* P, uint32_t max_len, int* CL, int* wide) {
  if (c->env.index != mi::IDX_AUTO) return false;  // the two-kernel path
  // (the planes themselves may exist without an X: an all-zero one is made for the side that has
  // none when the other side does, and the database's stays for the context's lifetime)
  // a database with X: k_match_t only (an entry whose context holds an X is flagged in bit 31 of its
  // position, the X's place or "several: see the mask plane" in the top byte of its target number)
  if (c->db_has_x && (c->max_tlen >= 0x80000000ull || c->nseq > (1u << 24) || c->env.no_x_context)) return false;
  if (c->nbases >= 0xFFFFFFF0ull || c->env.force_wide) return false;
  if (P->n_windows > CTX_MAX_W) return false;
  int q1min = P->windows[0], q1max = P->windows[0];
  for (int k = 1; k < P->n_windows; k++) {
    q1min = std::min(q1min, P->windows[k]);
    q1max = std::max(q1max, P->windows[k]);
  }
  const int64_t span = (int64_t)q1max - q1min + (int64_t)max_len;
  const int wenv = c->env.context;  // experiments: "narrow" (1) keeps runs beyond 120 bases on the two-kernel path, "wide" (2) puts every run on wide buckets
  *CL = q1max;
  *wide = 0;
  if (span > CTX_BASES || q1max > CTX_BASES || wenv == 2) {
    // wide buckets: k_match_t only; records of up to 16 words hold 200-base reads and their length word
    if (wenv == 1) return false;
    if (span > CTXW_BASES || q1max > CTXW_BASES) return false;
    *wide = 1;
  }
  // reads with X: k_match_t handles them, and only while every read either lists all its X
  // in its xpos word or has more X than mismatches allowed (reads_x_fit, cached per reads + budget)
  if (c->reads_have_x && !(c->db_has_x ? reads_x_fit_db(c, P, *wide) : reads_x_fit(c, P, max_len, *wide))) return false;
  return true;
}

// ---- partitions

// What a partitioned pass holds beside the index and the usual pass buffers (match_partitioned; all of it released
// when the pass ends): 20 B per read (best, survivor count / cursor, run offset), the summed block counters, and the
// accumulated tuple lists -- 20 B per tuple (the list and one scan word), estimated from the tuple buffer of the passes
// so far and at least one tuple per read
uint64_t merge_reserve(const musc_ctx* c) {
  const uint64_t tuples = std::max<uint64_t>(c->hits.cap, c->nreads);
  return 20 * (c->nreads + 1) + (4ull << BLOCK_TABLE_BITS) + 20 * tuples;
}

// The partition plan of a pass with these parameters: one partition (the unpartitioned path) whenever the index fits,
// or the limit of musc_db_set_partition_bases allows; otherwise the fewest ranges of about equal bases whose index
// fits.  Every partition then builds the same index kind and table size, settled on the largest one.
int plan_partitions(musc_ctx* c, const musc_params* P, uint32_t max_len) {
  const int32_t ww = P->window_width;
  const std::vector<uint32_t> one = {0u, c->nseq};
  // automatic, and an index of the whole database is resident: it fits (nothing to decide, nothing to query)
  if (!c->part_bases && c->idx.ww == ww && c->idx.g0 == 0 && c->idx.g1 == c->nseq && c->nseq) {
    c->part_first = one;
    return 0;
  }
  int CL = 0, wide = 0;
  const bool ctx_ok = ctx_eligible(c, P, max_len, &CL, &wide);
  const uint64_t avail = index_avail(c);
  auto plan_for = [&](uint64_t bases, uint64_t extra, bool need_fit) {
    return mi::cascade(c->env, ww, need_fit && ctx_ok, wide != 0, bases, avail, extra, need_fit);
  };
  std::vector<uint32_t> first = one;
  uint64_t largest = c->nbases;
  mi::Plan plan{};
  if (c->part_bases) {
    if (!mi::cut_targets(c->h_seq_off, c->part_bases, &first, &largest))
      return fail(c, 5, "DbPartitionBases %llu cuts the database into more than %u partitions",
                  (unsigned long long)c->part_bases, mi::MAX_PARTITIONS);
    plan = plan_for(largest, first.size() > 2 ? merge_reserve(c) : 0, true);
    if (!plan.fits) plan = plan_for(largest, 0, false);  // (then the build reports what failed)
  } else if (!plan_for(c->nbases, 0, true).fits) {
    // the fewest partitions whose largest index fits
    auto fits = [&](uint64_t bases) { return plan_for(bases, merge_reserve(c), true).fits; };
    if (!mi::fewest_partitions(c->h_seq_off, fits, &first, &largest))
      return fail(c, 5, "the index of this database does not fit the device even in %u partitions", mi::MAX_PARTITIONS);
    plan = plan_for(largest, merge_reserve(c), true);
  }
  c->part_first = first;
  c->part_kind = plan.kind;  // (read by a partitioned pass only)
  c->part_size = first.size() > 2 ? largest : c->nbases;
  return 0;
}

// Whether the index in hand is the one `want` names.  The targets covered are part of the comparison: a partition never
// reuses another partition's table; so is the table shape: a musc_reload_env that flips MUSC_DEBUG_CTX_DIRECT or
// MUSC_DEBUG_INDEX_BITS rebuilds on the next pass.
// keep_layout: a resident window-start index for this width keeps its line / 64-byte layout.  The automatic choice
// looks at the free memory of the moment, which moves as the pass buffers grow, and a flip would mean dropping the sized
// state and rebuilding tens of gigabytes in the middle of a run.  Only an explicit MUSC_INDEX = lines | classic64 that
// contradicts the resident layout rebuilds, or a partitioned pass that has settled the other one.
bool index_in_hand(const musc_ctx* c, mi::Resident want, bool keep_layout) {
  if (keep_layout && !mi::is_ctx(want.kind) && !mi::is_ctx(c->idx.kind)) want.kind = c->idx.kind;
  return want == c->idx;
}

// The index of this request resident when it returns: of the whole database, or of partition cur_part of a partitioned
// pass (partitioned = false: the whole database whatever the last plan said).  ctx_ok / CL / wide: what ctx_eligible
// said.  Decide, then touch state: the plan comes first, and only a plan that is not in hand invalidates and builds.
int ensure_index_of(musc_ctx* c, int32_t ww, bool partitioned, bool ctx_ok, int CL, bool wide) {
  c->wide = c->nbases >= 0xFFFFFFF0ull || c->env.force_wide;  // (never on context buckets: ctx_eligible)
  if (c->wide && c->nseq >= (1u << 24))
    return fail(c, 5, "a database of 2^32 bases or more may hold at most 2^24 targets (has %u)", c->nseq);
  IdxRange R = whole_db(c);
  if (partitioned) {
    const uint32_t g0 = c->part_first[c->cur_part], g1 = c->part_first[c->cur_part + 1];
    R = IdxRange{g0, g1, c->h_seq_off[g0], c->h_seq_off[g1], c->part_size};
  }
  // the plan: the kind plan_partitions settled (on the table of the largest partition), else the cascade on the
  // whole database
  auto plan_for = [&](uint64_t avail) {
    if (!partitioned) return mi::cascade(c->env, ww, ctx_ok, wide, R.size, avail, 0, false);
    const mi::Table t = mi::table_for(c->env, ctx_ok, ww, R.size);
    return mi::Plan{c->part_kind, t.bits, t.direct, !ctx_ok || mi::index_fits(c->env, c->part_kind, t.bits, R.size, avail, 0)};
  };
  auto ident = [&](const mi::Plan& p) { return mi::Resident{p.kind, ww, mi::is_ctx(p.kind) ? CL : 0, p.bits, p.direct, R.g0, R.g1}; };
  const bool keep_layout = !partitioned && c->env.index != mi::IDX_LINES && c->env.index != mi::IDX_CLASSIC64;
  // What the plan would be with all the memory there is: if that is in hand it stays, and nothing is queried.  (A
  // resident context index is not measured against the memory of the moment either: the pass buffers grew beside it.)
  if (index_in_hand(c, ident(plan_for(~0ull)), keep_layout)) return 0;
  const mi::Plan plan = plan_for(index_avail(c));
  int rc = 100;
  if (plan.fits) {
    if (index_in_hand(c, ident(plan), keep_layout)) return 0;
    rc = build_index(c, ident(plan), R);
  }
  if (rc != 100) return rc;
  if (partitioned)
    return fail(c, 5, "the context index of partition %u (%llu bases) does not fit the device", c->cur_part,
                (unsigned long long)(R.b1 - R.b0));
  // the one runtime fallback: the estimate said the context table fits and its allocation failed.  The window-start
  // index is a quarter of the size; it is what is resident afterwards, so the next pass finds it.
  return ensure_index_of(c, ww, false, false, 0, false);
}

int ensure_index(musc_ctx* c, const musc_params* P, uint32_t max_len) {
  const bool partitioned = c->part_first.size() > 2;
  int CL = 0, wide = 0;
  const bool ctx_ok = (!partitioned || mi::is_ctx(c->part_kind)) && ctx_eligible(c, P, max_len, &CL, &wide);
  if (partitioned && mi::is_ctx(c->part_kind) && !ctx_ok) return fail(c, 12, "internal: a partition lost context-bucket eligibility");
  return ensure_index_of(c, P->window_width, partitioned, ctx_ok, CL, wide != 0);
}

}  // namespace

extern "C" {

int musc_db_build_index(musc_ctx* c, int32_t ww) {
  if (!c) return 1;
  if (!c->db2) return fail(c, 4, "no database loaded");
  if (ww < 1 || ww > 4096) return fail(c, 2, "bad window width %d", ww);
  HIPCHK(c, hipSetDevice(c->device));
  return ensure_index_of(c, ww, false, false, 0, false);
}

int musc_db_build_index_for(musc_ctx* c, const musc_params* P, int32_t max_read_len) {
  if (!c) return 1;
  int rc = check_params(c, P);
  if (rc) return rc;
  if (!c->db2) return fail(c, 4, "no database loaded");
  HIPCHK(c, hipSetDevice(c->device));
  const uint32_t ml = max_read_len > 0 ? (uint32_t)max_read_len
                                       : (P->max_read_length > 0 ? (uint32_t)P->max_read_length : c->max_len);
  if ((rc = plan_partitions(c, P, ml))) return rc;
  c->cur_part = 0;  // (several partitions: the first one's index)
  return ensure_index(c, P, ml);
}

int musc_db_set_partition_bases(musc_ctx* c, uint64_t max_bases) {
  if (!c) return 1;
  c->part_bases = max_bases;
  return 0;
}

int musc_db_partitions(musc_ctx* c, uint32_t* first_target, uint32_t cap, uint32_t* n) {
  if (!c) return 1;
  if (!n) return fail(c, 2, "musc_db_partitions: n is NULL");
  *n = c->part_first.empty() ? 0u : (uint32_t)c->part_first.size() - 1;
  if (!first_target || !*n) return 0;
  if (cap < *n + 1) return fail(c, 2, "musc_db_partitions: room for %u boundaries < %u", cap, *n + 1);
  memcpy(first_target, c->part_first.data(), (*n + 1) * sizeof(uint32_t));
  return 0;
}

}  // extern "C"
