// muscato_cov.hpp -- the host side of the coverage stage (musc_cov_*).  Part of libmuscato_hip.so: included
// by muscato_hip.hip after muscato_text.hpp, whose text_range, res_data and sam_names it uses, with what the drivers
// share (grid, the scans, tmp_alloc, KeyPasses, Readback, timed).  musc_cov_prepare sorts the interval ends of the
// ordered list of the last musc_results_order, sums them to depths, compacts the runs and lays out both texts;
// musc_cov_text renders a range of records of either (kernels_cov.hpp) through text_range.
#pragma once

static const int MUSC_COV_ERR_REFUSED = 12;  // the list, the database or the gene text does not allow coverage as asked

static CovData cov_data(const musc_ctx* c) {
  CovData D;
  D.R = res_data(c);
  D.gname = c->cov_gname.p;
  D.rank = c->res_rank;
  D.flags = c->cov_flags;
  return D;
}

static CovSummary cov_summary(const musc_ctx* c) {
  return CovSummary{c->cov_target.p, c->cov_numreads.p, c->cov_maxdepth.p, c->cov_covbases.p, c->cov_sumdepth.p};
}

// The temporaries of one musc_cov_prepare, all of them in one device block: want() notes an array and its place,
// alloc() takes the block and hands out the places.
struct CovArena {
  struct Want { void** p; uint64_t at; };
  std::vector<Want> wants;
  uint64_t bytes = 0;
  TmpBufs B;
  template <class T>
  void want(T** p, uint64_t elems) {
    wants.push_back(Want{reinterpret_cast<void**>(p), bytes});
    bytes += (elems * sizeof(T) + 255u) & ~(uint64_t)255u;
  }
  int alloc(musc_ctx* c, const char* who) {
    unsigned char* base = nullptr;
    const int rc = tmp_alloc(c, who, B, &base, bytes);
    if (rc) return rc;
    for (const Want& w : wants) *w.p = base + w.at;
    return 0;
  }
};

// -> 0, with the tables of both texts in the context; MUSC_COV_ERR_REFUSED with the reason as the context's error
static int cov_prepare_impl(musc_ctx* c) {
  static const char* const who = "musc_cov_prepare";
  const dim3 B256(256);
  const uint64_t m = c->res_n, n2 = 2 * m, nseq = c->nseq, nreads = c->nreads;
  const uint4* const hits = reinterpret_cast<const uint4*>(c->res_hits.p);
  const CovData D = cov_data(c);
  const bool unique = (c->cov_flags & MUSC_COV_UNIQUE) != 0u;
  int rc;
  Readback R(c->scalars, c->stream);

  // ---- the temporaries.  Three arrays take a second name once the first is dead: the flags and places of the group
  // ends become those of the breakpoints, the events' slots the breakpoints', the groups' slots the runs' lengths.
  CovArena A;
  uint32_t *first = nullptr, *last = nullptr, *evdelta = nullptr, *sum = nullptr, *flagA = nullptr, *idxA = nullptr, *gdepth = nullptr,
           *gline = nullptr, *bdepth = nullptr, *bline = nullptr, *isrun = nullptr, *ridx = nullptr, *t_nreads = nullptr, *b0 = nullptr,
           *b1 = nullptr, *has = nullptr, *tidx = nullptr, *stmp32 = nullptr;
  uint64_t *evkey = nullptr, *gkey = nullptr, *rarea = nullptr, *stmp64 = nullptr, *words = nullptr;
  if (unique) A.want(&first, nreads + 1), A.want(&last, nreads + 1);
  A.want(&evkey, n2 + 1), A.want(&evdelta, n2 + 1), A.want(&sum, n2 + 1), A.want(&flagA, n2 + 1), A.want(&idxA, n2 + 1);
  A.want(&gdepth, n2 + 1), A.want(&gkey, n2 + 1), A.want(&gline, n2 + 1);
  A.want(&bdepth, n2 + 1), A.want(&bline, n2 + 1), A.want(&isrun, n2 + 1), A.want(&ridx, n2 + 1), A.want(&rarea, n2 + 1);
  A.want(&t_nreads, nseq + 1), A.want(&b0, nseq + 1), A.want(&b1, nseq + 1), A.want(&has, nseq + 1), A.want(&tidx, nseq + 1);
  A.want(&stmp32, scan_tmp_elems(std::max(n2, nseq) + 1)), A.want(&stmp64, scan_tmp_elems(std::max(n2, nseq) + 1));
  A.want(&words, 2);  // the total weight; the flag of a tuple or a run that does not fit
  if ((rc = A.alloc(c, who))) return rc;
  uint32_t *const isend = flagA, *const gidx = idxA, *const isbreak = flagA, *const bidx = idxA;
  uint64_t *const bkey = evkey, *const rlen = gkey;
  unsigned long long* const total = reinterpret_cast<unsigned long long*>(words);
  uint32_t* const bad = reinterpret_cast<uint32_t*>(words + 1);

  // ---- events, the total weight and the refusal
  HIPCHK(c, hipMemsetAsync(words, 0, 16, c->stream));
  HIPCHK(c, hipMemsetAsync(t_nreads, 0, (nseq + 1) * 4, c->stream));
  HIPCHK(c, hipMemsetAsync(b0, 0, (nseq + 1) * 4, c->stream));
  HIPCHK(c, hipMemsetAsync(b1, 0, (nseq + 1) * 4, c->stream));
  if (m) {
    if (unique) {
      hipLaunchKernelGGL(k_sam_runs, grid(c, m), B256, 0, c->stream, hits, m, first, last);
      HIPCHK(c, hipGetLastError());
    }
    hipLaunchKernelGGL(k_cov_events, grid(c, m), B256, 0, c->stream, hits, m, D, (const uint32_t*)first, (const uint32_t*)last, evkey, evdelta,
                       t_nreads, total, bad);
    HIPCHK(c, hipGetLastError());
  }
  uint64_t weight = 0;
  uint32_t unfit = 0;
  HIPCHK(c, R.get(words, &weight).get(bad, &unfit).wait());
  if (unfit) return fail(c, 11, "%s: a tuple of the ordered list no longer fits the reads and the database in hand", who);
  if (musc_cov::total_refused(weight))
    return fail(c, MUSC_COV_ERR_REFUSED, "%s: the weights of the contributing lines add up to %llu, the depths are 32 bits wide", who,
                (unsigned long long)weight);

  // ---- the sort, the depths, and three compactions: group ends, breakpoints, runs
  uint32_t ng = 0, nb = 0, nruns = 0;
  KeyPasses S;
  if (n2) {
    const unsigned end_bit = musc_cov::sort_end_bit(c->nbases, nseq);
    if ((rc = S.start(c, who, n2, {end_bit}))) return rc;
    if ((rc = S.pass(end_bit, [&](const uint32_t* order, uint64_t* keys) {
          hipLaunchKernelGGL(k_cov_keys, grid(c, n2), B256, 0, c->stream, order, (const uint64_t*)evkey, n2, keys);
        })))
      return rc;
    const uint32_t* const order = S.order();
    hipLaunchKernelGGL(k_cov_gather, grid(c, n2 + 1), B256, 0, c->stream, order, (const uint64_t*)evkey, (const uint32_t*)evdelta, n2, sum, isend);
    HIPCHK(c, hipGetLastError());
    if ((rc = scan_u32(c, sum, sum, n2, true, stmp32)) || (rc = scan_u32(c, isend, gidx, n2 + 1, false, stmp32))) return rc;
    hipLaunchKernelGGL(k_cov_groups, grid(c, n2), B256, 0, c->stream, order, (const uint64_t*)evkey, (const uint32_t*)isend, (const uint32_t*)gidx,
                       (const uint32_t*)sum, n2, gdepth, gkey, gline);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, R.get(gidx + n2, &ng).wait());
    hipLaunchKernelGGL(k_cov_breaks, grid(c, (uint64_t)ng + 1), B256, 0, c->stream, (const uint32_t*)gdepth, (uint64_t)ng, isbreak);
    HIPCHK(c, hipGetLastError());
    if ((rc = scan_u32(c, isbreak, bidx, (uint64_t)ng + 1, false, stmp32))) return rc;
    HIPCHK(c, R.get(bidx + ng, &nb).wait());
    HIPCHK(c, hipMemsetAsync(isrun, 0, ((uint64_t)nb + 1) * 4, c->stream));
    hipLaunchKernelGGL(k_cov_break_list, grid(c, ng), B256, 0, c->stream, (const uint32_t*)isbreak, (const uint32_t*)bidx, (const uint32_t*)gdepth,
                       (const uint64_t*)gkey, (const uint32_t*)gline, (uint64_t)ng, bdepth, bkey, bline, isrun);
    HIPCHK(c, hipGetLastError());
    if ((rc = scan_u32(c, isrun, ridx, (uint64_t)nb + 1, false, stmp32))) return rc;
    HIPCHK(c, R.get(ridx + nb, &nruns).wait());
  }

  // ---- the tables that stay (an earlier call's are invalid since cov_begins and are overwritten here)
  const uint64_t nr1 = std::max<uint64_t>(nruns, 1), ns1 = std::max<uint64_t>(nseq, 1);
  if ((rc = ensure(c, c->cov_run_f, nr1)) || (rc = ensure(c, c->cov_run_d, nr1)) || (rc = ensure(c, c->cov_run_s, nr1)) ||
      (rc = ensure(c, c->cov_run_e, nr1)) || (rc = ensure(c, c->cov_off, (uint64_t)nruns + 1)) || (rc = ensure(c, c->cov_soff, nseq + 1)) ||
      (rc = ensure(c, c->cov_target, ns1)) || (rc = ensure(c, c->cov_numreads, ns1)) || (rc = ensure(c, c->cov_maxdepth, ns1)) ||
      (rc = ensure(c, c->cov_covbases, ns1)) || (rc = ensure(c, c->cov_sumdepth, ns1)))
    return rc;
  HIPCHK(c, hipMemcpyAsync(c->cov_numreads.p, t_nreads, nseq * 4, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(c->cov_maxdepth.p, 0, ns1 * 4, c->stream));
  hipLaunchKernelGGL(k_cov_runs, grid(c, (uint64_t)nb + 1), B256, 0, c->stream, hits, D, (const uint32_t*)isrun, (const uint32_t*)ridx,
                     (const uint32_t*)bdepth, (const uint64_t*)bkey, (const uint32_t*)bline, (uint64_t)nb, (uint64_t)nruns, c->cov_run_f.p,
                     c->cov_run_d.p, c->cov_run_s.p, c->cov_run_e.p, rlen, rarea, c->cov_off.p, c->cov_maxdepth.p, bad);
  HIPCHK(c, hipGetLastError());
  if (nruns) {
    hipLaunchKernelGGL(k_cov_bounds, grid(c, nruns), B256, 0, c->stream, (const uint32_t*)c->cov_run_f.p, (uint64_t)nruns, b0, b1);
    HIPCHK(c, hipGetLastError());
  }
  if ((rc = scan_u64(c, rlen, rlen, (uint64_t)nruns + 1, stmp64)) || (rc = scan_u64(c, rarea, rarea, (uint64_t)nruns + 1, stmp64)) ||
      (rc = scan_u64(c, c->cov_off.p, c->cov_off.p, (uint64_t)nruns + 1, stmp64)))
    return rc;

  // ---- the summary: one record per target with a line
  hipLaunchKernelGGL(k_cov_targets, grid(c, nseq + 1), B256, 0, c->stream, D, (const uint32_t*)b0, (const uint32_t*)b1, (const uint64_t*)rlen,
                     (const uint64_t*)rarea, c->cov_covbases.p, c->cov_sumdepth.p, has);
  HIPCHK(c, hipGetLastError());
  if ((rc = scan_u32(c, has, tidx, nseq + 1, false, stmp32))) return rc;
  uint32_t nt = 0;
  HIPCHK(c, R.get(tidx + nseq, &nt).wait());
  hipLaunchKernelGGL(k_cov_target_list, grid(c, nseq + 1), B256, 0, c->stream, D, cov_summary(c), (const uint32_t*)has, (const uint32_t*)tidx,
                     (uint64_t)nt, c->cov_target.p, c->cov_soff.p);
  HIPCHK(c, hipGetLastError());
  if ((rc = scan_u64(c, c->cov_soff.p, c->cov_soff.p, (uint64_t)nt + 1, stmp64))) return rc;
  uint64_t bytes = 0, sbytes = 0;
  HIPCHK(c, R.get(c->cov_off.p + nruns, &bytes).get(c->cov_soff.p + nt, &sbytes).get(bad, &unfit).wait());
  if (unfit) return fail(c, 11, "%s: a run does not lie within its target", who);
  c->cov_nruns = nruns;
  c->cov_bytes = bytes;
  c->cov_nt = nt;
  c->cov_sbytes = sbytes;
  return 0;
}

int musc_cov_prepare(musc_ctx* c, uint32_t flags, uint64_t* nruns, uint64_t* run_bytes, uint64_t* ntargets, uint64_t* summary_bytes) {
  if (!c) return 1;
  for (uint64_t* out : {nruns, run_bytes, ntargets, summary_bytes})
    if (out) *out = 0;
  c->st.cov_begins();
  if (!c->st.ordered_current() || !c->db2 || !c->res_gtext || !c->res_rank)
    return fail(c, 2, "musc_cov_prepare: no ordered list (musc_results_order) of the reads, the database and the texts in hand");
  if (flags & ~musc_cov::ALL_FLAGS) return fail(c, 2, "musc_cov_prepare: unknown flags (%u)", flags);
  const uint32_t rev_pairs = flags & MUSC_COV_REV_PAIRS ? 1u : 0u;
  if (musc_cov::lines_refused(c->res_n))
    return fail(c, MUSC_COV_ERR_REFUSED, "musc_cov_prepare: the ordered list has %llu lines, 2^31 or more", (unsigned long long)c->res_n);
  if (rev_pairs && (c->nseq & 1u))
    return fail(c, MUSC_COV_ERR_REFUSED, "musc_cov_prepare: rev_pairs with an odd number of targets (%u)", c->nseq);
  HIPCHK(c, hipSetDevice(c->device));
  uint32_t verdict = 0;
  int rc = sam_names(c, c->cov_gname, rev_pairs, &verdict);
  if (rc) return rc;
  if (verdict & 2u) return fail(c, MUSC_COV_ERR_REFUSED, "musc_cov_prepare: rev_pairs, and the two targets of a pair differ in length");
  if (verdict & 1u)
    return fail(c, MUSC_COV_ERR_REFUSED, "musc_cov_prepare: the gene text of a target with an id line%s has an empty first token",
                rev_pairs ? " (or of its even partner)" : "");
  c->cov_flags = flags;
  rc = timed(c, &c->cov_ms_prepare, [&] { return cov_prepare_impl(c); });
  if (rc) return rc;
  c->cov_ms_text = 0;
  c->st.cov_made();
  if (nruns) *nruns = c->cov_nruns;
  if (run_bytes) *run_bytes = c->cov_bytes;
  if (ntargets) *ntargets = c->cov_nt;
  if (summary_bytes) *summary_bytes = c->cov_sbytes;
  return 0;
}

static void launch_cov(musc_ctx* c, int which, uint64_t r0, uint64_t r1, uint64_t bytes, unsigned char* out) {
  const dim3 blocks = stage_grid(c, bytes / 256 + 1, musc_launch::CAP_TILES);
  const CovData D = cov_data(c);
  if (which == 0)
    hipLaunchKernelGGL(k_cov_render, blocks, dim3(256), 0, c->stream, (const uint32_t*)c->cov_run_f.p, (const uint32_t*)c->cov_run_d.p,
                       (const uint64_t*)c->cov_run_s.p, (const uint64_t*)c->cov_run_e.p, (const uint64_t*)c->cov_off.p, r0, r1, D, out,
                       c->d_flag.get());
  else
    hipLaunchKernelGGL(k_cov_sum_render, blocks, dim3(256), 0, c->stream, cov_summary(c), (const uint64_t*)c->cov_soff.p, r0, r1, D, out,
                       c->d_flag.get());
}

int musc_cov_text(musc_ctx* c, int which, uint64_t rec0, uint64_t nrec, char* dst, uint64_t capacity, int dst_on_device, uint64_t* nbytes) {
  if (!c) return 1;
  if (!nbytes) return fail(c, 2, "musc_cov_text: nbytes is NULL");
  *nbytes = 0;
  if (which < 0 || which > 1) return fail(c, 2, "musc_cov_text: no such text (%d)", which);
  if (!c->st.may_cov_text()) return fail(c, 2, "musc_cov_text: nothing prepared (musc_cov_prepare)");
  const TextDesc t = {which ? c->cov_soff.p : c->cov_off.p, which ? c->cov_nt : c->cov_nruns, "musc_cov_text",
                      "a record no longer fits the database or the gene text in hand", &c->cov_ms_text};
  return text_range(c, t, rec0, nrec, dst, capacity, dst_on_device, nbytes,
                    [&](uint64_t r0, uint64_t r1, uint64_t bytes, unsigned char* out) { launch_cov(c, which, r0, r1, bytes, out); });
}

int musc_cov_last_ms(musc_ctx* c, float* ms_prepare, float* ms_text) {
  if (!c) return 1;
  if (ms_prepare) *ms_prepare = c->cov_ms_prepare;
  if (ms_text) *ms_text = c->cov_ms_text;
  return 0;
}
