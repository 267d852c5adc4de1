// muscato_maxmatches.hpp -- the host side of the MaxMatches replay on the device (musc_maxmatches_*).
// Part of libmuscato_hip.so: included by muscato_hip.hip after muscato_text.hpp (timed; grid, the scans and Readback are
// what the drivers share).  The kernels are in
// kernels_maxmatches.hpp, the decisions that need no device in maxmatches_plan.hpp.
#pragma once

// The suspect probes of the last pass, on the device: the (read, window) pairs whose (window, key) block counter is above
// MaxMatches.  *out holds *found pairs; k_hot_probes runs again with room for all of them when the first buffer was
// too small.
static int hot_probes_device(musc_ctx* c, DevPtr<uint2>* out, uint64_t* found) {
  *found = 0;
  uint64_t cap = 1u << 20;
  for (;;) {
    HIPCHK(c, out->alloc(cap * sizeof(uint2)));
    uint2* const d_out = out->get();
    hipError_t e = hipMemsetAsync(c->counters + CNT_BATCH, 0, 8, c->stream);
    if (e == hipSuccess) {
      by_rw(c->rw, [&](auto r) {
        hipLaunchKernelGGL((k_hot_probes<decltype(r)::value>), grid(c, c->nreads), dim3(256), 0, c->stream, c->rd, c->rdm, c->nreads, c->rw, c->d_pp,
                           c->block_table.p, c->last_max_matches, d_out, cap, c->counters + CNT_BATCH);
      });
      e = hipGetLastError();
    }
    uint64_t n = 0;
    if (e == hipSuccess) e = Readback(c->scalars, c->stream).get(c->counters + CNT_BATCH, &n).wait();
    if (e != hipSuccess) {  // (the block goes with the caller's owner)
      (void)hipGetLastError();
      return fail(c, 10, "the suspect probes: %s", hipGetErrorString(e));
    }
    if (n > cap) {  // again, with room for all of them
      cap = n + 16;
      continue;
    }
    *found = n;
    return 0;
  }
}

namespace {

MmData mm_data(const musc_ctx* c, const musc_params& P) {
  MmData D;
  D.rd = c->rd;
  D.rdm = c->reads_have_x ? c->rdm : nullptr;
  D.db2 = c->db2;
  D.dbm2 = c->db_has_x ? c->dbm2 : nullptr;
  D.seq_off = c->seq_off;
  D.nreads = c->nreads;
  D.nseq = c->nseq;
  D.rw = c->rw;
  D.W = P.n_windows;
  D.ww = P.window_width;
  D.min_dinuc = P.min_dinuc;
  D.max_read_length = P.max_read_length;
  for (int k = 0; k < MUSC_MAX_WINDOWS; k++) D.win[k] = k < P.n_windows ? P.windows[k] : 0;
  return D;
}

// rocprim::merge_sort of n uint2 under `less`, in -> out; its temporary storage goes through T
template <class Less>
int mm_sort(musc_ctx* c, TmpBufs& T, uint2* in, uint2* out, uint64_t n, Less less) {
  size_t bytes = 0;
  void* tmp = nullptr;
  HIPCHK(c, rocprim::merge_sort(nullptr, bytes, in, out, (size_t)n, less, c->stream));
  HIPCHK(c, T.alloc(&tmp, bytes));
  HIPCHK(c, rocprim::merge_sort(tmp, bytes, in, out, (size_t)n, less, c->stream));
  return 0;
}

// The stage proper, queued on the context's stream.  The pass's list is read until the last step, which copies the
// survivors over it: every failure before that leaves the list as it was.
int mm_apply_impl(musc_ctx* c, const musc_params& P, int apply_mmtol, uint64_t* n_suspect, uint64_t* n_trunc) {
  const uint64_t N = c->nhits;
  const int W = P.n_windows;
  const dim3 B256(256);
  const MmData D = mm_data(c, P);
  const uint4* const hits = reinterpret_cast<const uint4*>(c->hits.p);
  Readback R(c->scalars, c->stream);
  int rc;

  DevPtr<uint2> probes;
  uint64_t np = 0;
  if (c->stats.n_overflow_blocks != 0) {
    if (!c->last_exact_blocks || !c->block_table.p) return fail(c, 4, "musc_maxmatches_apply: no exact block counters from the last pass");
    if ((rc = hot_probes_device(c, &probes, &np))) return rc;
  }
  *n_suspect = np;
  if (np >= musc_mm::MAX_BLOCKS) return fail(c, 12, "musc_maxmatches_apply: %llu suspect probes are more than the device stage takes", (unsigned long long)np);
  if (N == 0 || (np == 0 && !apply_mmtol)) return 0;

  TmpBufs A, B;  // A: the blocks and the pairs; B: the sorts' storage and the survivors
  uint32_t* words = nullptr;
  uint64_t* sizes = nullptr;
  uint64_t ntrunc = 0;
  if (np) {
    // ---- 1. the suspect blocks: the probes in (window, key) order, one representative each
    uint2 *sorted = nullptr, *blocks = nullptr;
    uint32_t *heads = nullptr, *excl = nullptr, *stmp = nullptr;
    HIPCHK(c, A.alloc(&sorted, np * 8));
    {
      TmpBufs S;
      if ((rc = mm_sort(c, S, probes.get(), sorted, np, MmProbeLess{D}))) return rc;
      HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    HIPCHK(c, A.alloc(&heads, np * 4));
    HIPCHK(c, A.alloc(&excl, np * 4));
    HIPCHK(c, A.alloc(&stmp, scan_tmp_elems(np) * 4));
    hipLaunchKernelGGL(k_mm_heads, grid(c, np), B256, 0, c->stream, D, sorted, np, heads);
    HIPCHK(c, hipGetLastError());
    if ((rc = scan_u32(c, heads, excl, np, false, stmp))) return rc;
    uint32_t heads_before = 0, head_last = 0;
    HIPCHK(c, R.get(excl + (np - 1), &heads_before).get(heads + (np - 1), &head_last).wait());
    const uint32_t nb = heads_before + head_last;
    HIPCHK(c, A.alloc(&blocks, (uint64_t)nb * 8));
    hipLaunchKernelGGL(k_mm_blocks, grid(c, np), B256, 0, c->stream, sorted, heads, excl, np, blocks);
    HIPCHK(c, hipGetLastError());

    // ---- 2. pairs: every (tuple, window) finds its block; the blocks count what their windows emit
    uint32_t *cnt = nullptr, *fill = nullptr;
    uint64_t *off = nullptr, *tmp64 = nullptr;
    HIPCHK(c, A.alloc(&words, N * (uint64_t)W * 4));
    HIPCHK(c, A.alloc(&cnt, (uint64_t)nb * 4));
    HIPCHK(c, A.alloc(&fill, (uint64_t)nb * 4));
    HIPCHK(c, A.alloc(&sizes, ((uint64_t)nb + 1) * 8));
    HIPCHK(c, A.alloc(&off, ((uint64_t)nb + 1) * 8));
    HIPCHK(c, A.alloc(&tmp64, scan_tmp_elems((uint64_t)nb + 1) * 8));
    HIPCHK(c, hipMemsetAsync(cnt, 0, (uint64_t)nb * 4, c->stream));
    HIPCHK(c, hipMemsetAsync(fill, 0, (uint64_t)nb * 4, c->stream));
    HIPCHK(c, hipMemsetAsync(c->counters + CNT_SCRATCH, 0, 8, c->stream));
    hipLaunchKernelGGL(k_mm_pairs, grid(c, N * (uint64_t)W), B256, 0, c->stream, D, hits, N, blocks, nb, words, cnt);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(k_mm_sizes, grid(c, (uint64_t)nb + 1), B256, 0, c->stream, cnt, nb, (uint32_t)P.max_matches, sizes, c->counters + CNT_SCRATCH);
    HIPCHK(c, hipGetLastError());
    if ((rc = scan_u64(c, sizes, off, (uint64_t)nb + 1, tmp64))) return rc;
    uint64_t M = 0;
    HIPCHK(c, R.get(c->counters + CNT_SCRATCH, &ntrunc).get(off + nb, &M).wait());
    *n_trunc = ntrunc;
    c->mm_pairs = M;
    if (ntrunc == 0) {  // false alarms only
      if (!apply_mmtol) return 0;
      words = nullptr;
    } else {
      // ---- 3. order: the pairs of the truncated blocks, block-major, in the order of their lines
      uint2 *pairs = nullptr, *psorted = nullptr, *gheap = nullptr;
      HIPCHK(c, B.alloc(&pairs, M * 8));
      HIPCHK(c, A.alloc(&psorted, M * 8));
      hipLaunchKernelGGL(k_mm_fill, grid(c, N * (uint64_t)W), B256, 0, c->stream, words, N, W, sizes, off, fill, pairs);
      HIPCHK(c, hipGetLastError());
      if ((rc = mm_sort(c, B, pairs, psorted, M, MmPairLess{D, hits, blocks}))) return rc;
      // ---- 4. replay
      const uint32_t lds_cap = musc_mm::heap_lds_entries(c->env.mm_heap_lds);
      const bool in_lds = musc_mm::heap_in_lds(P.max_matches, lds_cap);
      if (!in_lds && P.match_mode == 0) HIPCHK(c, B.alloc(&gheap, M * 8));
      hipEvent_t e0 = pool_event(c), e1 = pool_event(c);
      if (e0) (void)hipEventRecord(e0, c->stream);
      hipLaunchKernelGGL(k_mm_replay, stage_grid(c, nb, musc_launch::CAP_REPLAY), dim3(64), 0, c->stream, hits, psorted, blocks, sizes, off, nb, W,
                         (uint32_t)P.max_matches, P.match_mode == 1 ? 1 : 0, lds_cap, gheap, words);
      HIPCHK(c, hipGetLastError());
      if (e1) (void)hipEventRecord(e1, c->stream);
      HIPCHK(c, hipStreamSynchronize(c->stream));
      c->mm_ms_replay = 0;
      if (e0 && e1) (void)hipEventElapsedTime(&c->mm_ms_replay, e0, e1);
      B.release();
    }
  }

  // ---- 5. survivors, the per-read selection, and the new list
  uint32_t *flags = nullptr, *excl = nullptr, *stmp = nullptr, *best = nullptr;
  HIPCHK(c, B.alloc(&flags, N * 4));
  HIPCHK(c, B.alloc(&excl, N * 4));
  HIPCHK(c, B.alloc(&stmp, scan_tmp_elems(N) * 4));
  if (apply_mmtol) {
    HIPCHK(c, B.alloc(&best, c->nreads * 4));
    HIPCHK(c, hipMemsetAsync(best, 0xFF, c->nreads * 4, c->stream));
  }
  hipLaunchKernelGGL(k_mm_survive, grid(c, N), B256, 0, c->stream, hits, N, words, W, sizes, apply_mmtol ? 1 : 0, flags, best);
  HIPCHK(c, hipGetLastError());
  if (apply_mmtol) {
    hipLaunchKernelGGL(k_mm_best, grid(c, N), B256, 0, c->stream, hits, N, best, (uint32_t)P.mmtol, flags);
    HIPCHK(c, hipGetLastError());
  }
  if ((rc = scan_u32(c, flags, excl, N, false, stmp))) return rc;
  uint64_t kept_before = 0, kept_last = 0;
  HIPCHK(c, R.get(excl + (N - 1), &kept_before).get(flags + (N - 1), &kept_last).wait());
  const uint64_t m = kept_before + kept_last;
  uint4* out = nullptr;
  HIPCHK(c, B.alloc(&out, m * 16));
  hipLaunchKernelGGL(k_mm_compact, grid(c, N), B256, 0, c->stream, hits, N, flags, excl, out);
  HIPCHK(c, hipGetLastError());
  // from here on the list changes.  (The survivors go back into the pass's own buffer: a captured graph of the pass
  // holds its address.)
  c->st.list_changes();  // (nobody's list until the copy has landed; an order taken before is not this list's)
  if (m) HIPCHK(c, hipMemcpyAsync(c->hits.p, out, m * 16, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->nhits = m;
  c->stats.n_hits = m;
  c->st.list_made(musc_state::LIST_REPLAYED);  // no longer that of a pass: a second call needs a new pass
  return 0;
}

}  // namespace

extern "C" {

int musc_maxmatches_apply(musc_ctx* c, int apply_mmtol, uint64_t* nhits, uint64_t* n_suspect_probes, uint64_t* n_truncated_blocks) {
  if (!c) return 1;
  uint64_t ns = 0, nt = 0;
  if (nhits) *nhits = 0;
  if (n_suspect_probes) *n_suspect_probes = 0;
  if (n_truncated_blocks) *n_truncated_blocks = 0;
  if (!c->st.may_replay())
    return fail(c, 2, "musc_maxmatches_apply: the resident tuple list is not that of a musc_match* over the reads and the database in hand");
  const musc_params P = c->mm_params;
  if (P.apply_mmtol != 0) return fail(c, 2, "musc_maxmatches_apply: the last pass ran with apply_mmtol = 1: its list lacks the tuples the replay needs");
  if (P.n_shards > 1) return fail(c, 2, "musc_maxmatches_apply: the last pass saw one shard of the reads (n_shards = %d)", P.n_shards);
  if (c->stats.n_overflow_blocks == ~0ull) return fail(c, 2, "musc_maxmatches_apply: the last pass skipped the MaxMatches check");
  if (const char* why = musc_mm::refusal(musc_mm::Shape{c->max_len, P.window_width, P.max_matches, c->nhits}))
    return fail(c, 12, "musc_maxmatches_apply: %s", why);
  HIPCHK(c, hipSetDevice(c->device));
  float ms = 0;
  c->mm_ms_replay = 0;
  c->mm_pairs = 0;
  const int rc = timed(c, &ms, [&]() -> int { return mm_apply_impl(c, P, apply_mmtol, &ns, &nt); });
  if (rc) return rc;
  c->mm_ms = ms;
  if (nhits) *nhits = c->nhits;
  if (n_suspect_probes) *n_suspect_probes = ns;
  if (n_truncated_blocks) *n_truncated_blocks = nt;
  return 0;
}

int musc_maxmatches_last_ms(musc_ctx* c, float* ms) {
  if (!c || !ms) return 1;
  *ms = c->mm_ms;
  return 0;
}

int musc_maxmatches_last_detail(musc_ctx* c, uint64_t* n_pairs, float* ms_replay) {
  if (!c) return 1;
  if (n_pairs) *n_pairs = c->mm_pairs;
  if (ms_replay) *ms_replay = c->mm_ms_replay;
  return 0;
}

}  // extern "C"
