// muscato_read_names.hpp -- the host side of the read-name stage: the members of each group of identical
// prepared reads in the order of their clipped names, the record count\tJ of every group left as the context's read
// text, and the lines seq\tcount\tJ\n of reads_sorted.txt rendered on demand.  Part of libmuscato_hip.so: included by
// muscato_hip.hip behind muscato_text.hpp (text_range, drop_read_text) and muscato_prep.hpp (fastq_prep_run); grid,
// tmp_alloc, staged, KeyPasses and Readback are what the drivers share.
// The kernels are kernels_read_names.hpp; what a lane computes is read_names_lanes.hpp and read_names_keys.hpp.
//
// Groups of up to WAVE_GROUP_MAX members are ranked by counting.  The members of the larger ones go, as (group, kept
// read) pairs, through key_passes() stable passes of KeyPasses on (uint64_t key, uint32_t pair number), as the reads do
// in reads_sort_unique_dev.  No library sort under a comparator is instantiated here.  What the device reports back
// (the pairs, the longest clipped name) is clamped before the host sizes or loops by it.
#pragma once

#include "kernels_read_names.hpp"

// the stage's inputs, all on the device; the kept reads are numbered in file order
struct RnInput {
  musc_rn::TextBytes rd;
  musc_rn::Names N;
  const uint32_t* order;   // [n] kept reads by sequence, ties in file order
  const uint32_t* ustart;  // [nu + 1]
  uint64_t nu;
};

// ranked[n] = the kept reads group by group in name order.  gid[n] = the group of each place (left for the caller).
static int rn_rank(musc_ctx* c, const char* who, const RnInput& in, uint32_t* ranked, uint32_t* gid, uint64_t* n_pairs, uint32_t* n_passes) {
  const uint64_t n = in.N.n;
  const dim3 B256(256);
  TmpBufs B;
  *n_pairs = 0;
  *n_passes = 0;
  uint32_t *flag = nullptr, *excl = nullptr, *stmp = nullptr, *max_clip = nullptr;
  int rc = 0;
  if ((rc = tmp_alloc(c, who, B, &flag, (n + 1) * 4)) || (rc = tmp_alloc(c, who, B, &excl, (n + 1) * 4)) ||
      (rc = tmp_alloc(c, who, B, &stmp, scan_tmp_elems(n + 1) * 4)) || (rc = tmp_alloc(c, who, B, &max_clip, 4)))
    return rc;
  hipLaunchKernelGGL(k_rn_gid, grid(c, n), B256, 0, c->stream, in.ustart, (uint32_t)in.nu, n, gid);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemsetAsync(flag + n, 0, 4, c->stream));
  HIPCHK(c, hipMemsetAsync(max_clip, 0, 4, c->stream));
  hipLaunchKernelGGL(k_rn_rank, grid(c, n), B256, 0, c->stream, in.rd, in.N, in.order, in.ustart, gid, ranked, flag);
  HIPCHK(c, hipGetLastError());
  if ((rc = scan_u32(c, flag, excl, n + 1, false, stmp))) return rc;
  Readback R(c->scalars, c->stream);
  uint64_t np = 0;
  HIPCHK(c, R.get(excl + n, &np).wait());
  if (np > n) return fail(c, 11, "%s: %llu members of larger groups among %llu reads", who, (unsigned long long)np, (unsigned long long)n);
  if (np == 0) return 0;

  // ---- the pairs of the larger groups, ordered by W + 2 stable key passes
  uint2* pairs = nullptr;
  uint32_t* place = nullptr;
  KeyPasses K;
  if ((rc = tmp_alloc(c, who, B, &pairs, np * 8)) || (rc = tmp_alloc(c, who, B, &place, np * 4)) || (rc = K.start(c, who, np, {64u}))) return rc;
  hipLaunchKernelGGL(k_rn_pairs, grid(c, n), B256, 0, c->stream, flag, excl, in.order, gid, in.N, pairs, place, max_clip);
  HIPCHK(c, hipGetLastError());
  uint32_t clip = 0;
  HIPCHK(c, R.get(max_clip, &clip).wait());
  const uint32_t W = musc_rn::key_words(clip);  // (clamped: at most CMP_WORDS whatever came back)
  for (uint32_t pass = 0; pass < W + 2 && !rc; pass++)
    rc = K.pass(64u, [&](const uint32_t* ord, uint64_t* keys) { hipLaunchKernelGGL(k_rn_keys, grid(c, np), B256, 0, c->stream, in.rd, in.N, pairs, ord, np, pass, W, keys); });
  if (rc) return rc;
  hipLaunchKernelGGL(k_rn_unpairs, grid(c, np), B256, 0, c->stream, pairs, K.order(), place, np, ranked);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));  // (the temporaries go with B)
  *n_pairs = np;
  *n_passes = W + 2;
  return 0;
}

// What a caller's arrays must satisfy before a kernel indexes by them: every name inside the text, every member a kept
// read, the groups a partition of the n places.
static int rn_check_input(musc_ctx* c, const char* who, uint64_t nbytes, const uint64_t* name_off, const uint32_t* name_len, uint64_t n,
                          const uint32_t* order, const uint32_t* ustart, uint64_t nu) {
  if (nu > n || (n && !nu)) return fail(c, 2, "%s: %llu groups of %llu reads", who, (unsigned long long)nu, (unsigned long long)n);
  if (ustart[0] != 0 || ustart[nu] != n) return fail(c, 2, "%s: the groups do not span the reads", who);
  for (uint64_t g = 0; g < nu; g++)
    if (ustart[g + 1] <= ustart[g] || ustart[g + 1] > n) return fail(c, 2, "%s: group %llu is empty or out of range", who, (unsigned long long)g);
  for (uint64_t i = 0; i < n; i++) {
    if (order[i] >= n) return fail(c, 2, "%s: order[%llu] is no kept read", who, (unsigned long long)i);
    if (name_off[i] > nbytes || musc_rn::text_len(name_len[i]) > nbytes - name_off[i])
      return fail(c, 2, "%s: the name of read %llu lies outside the text", who, (unsigned long long)i);
  }
  return 0;
}

static int names_order_run(musc_ctx* c, const char* text, uint64_t nbytes, int on_device, const uint64_t* name_off, const uint32_t* name_len,
                           uint64_t n, const uint32_t* order, const uint32_t* ustart, uint64_t nu, uint32_t* ranked_out) {
  static const char* const who = "musc_reads_names_order";
  int rc = rn_check_input(c, who, nbytes, name_off, name_len, n, order, ustart, nu);
  if (rc || n == 0) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  TmpBufs B;
  RnInput in;
  const unsigned char* d_text = nullptr;
  uint32_t *ranked = nullptr, *gid = nullptr;
  if ((rc = staged(c, who, B, (const unsigned char*)text, nbytes, on_device, 16, &d_text)) ||
      (rc = staged(c, who, B, name_off, n * 8, 0, 0, &in.N.name_off)) || (rc = staged(c, who, B, name_len, n * 4, 0, 0, &in.N.name_len)) ||
      (rc = staged(c, who, B, order, n * 4, 0, 0, &in.order)) || (rc = staged(c, who, B, ustart, (nu + 1) * 4, 0, 0, &in.ustart)) ||
      (rc = tmp_alloc(c, who, B, &ranked, n * 4)) || (rc = tmp_alloc(c, who, B, &gid, n * 4)))
    return rc;
  in.rd = musc_rn::TextBytes{d_text, nbytes};
  in.N.n = n;
  in.nu = nu;
  uint64_t np = 0;
  uint32_t passes = 0;
  if ((rc = rn_rank(c, who, in, ranked, gid, &np, &passes))) {
    (void)hipStreamSynchronize(c->stream);  // (kernels may still be queued on the temporaries)
    return rc;
  }
  HIPCHK(c, hipMemcpyAsync(ranked_out, ranked, n * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int musc_reads_names_order(musc_ctx* c, const char* text, uint64_t nbytes, int on_device, const uint64_t* name_off,
                                      const uint32_t* name_len, uint64_t n, const uint32_t* order, const uint32_t* ustart, uint64_t nu,
                                      uint32_t* ranked_out) {
  if (!c) return 1;
  if (n >= musc_rn::RN_MAX_READS) return fail(c, 2, "musc_reads_names_order: too many reads for 32-bit read numbers");
  if (!ustart || (n && (!name_off || !name_len || !order || !ranked_out)) || (!text && nbytes))
    return fail(c, 2, "musc_reads_names_order: NULL argument");
  return names_order_run(c, text, nbytes, on_device, name_off, name_len, n, order, ustart, nu, ranked_out);
}

// ---------------------------------------------------------------- the whole stage behind the FASTQ prep

static void launch_rn_lines(musc_ctx* c, uint64_t r0, uint64_t r1, uint64_t bytes, unsigned char* out) {
  const dim3 blocks = stage_grid(c, bytes / 256 + 1, musc_launch::CAP_TILES);
  const musc_rn::Reads S{c->rd, c->reads_have_x ? c->rdm.get() : nullptr, c->rw};
  hipLaunchKernelGGL(k_rn_lines, blocks, dim3(256), 0, c->stream, S, c->res_ttext.get(), c->res_toff.get(), c->rn_loff.get(), r0, r1, out);
}
static void launch_rn_copy(musc_ctx* c, uint64_t r0, uint64_t r1, uint64_t bytes, unsigned char* out) {
  const dim3 blocks = stage_grid(c, bytes / 256 + 1, musc_launch::CAP_TILES);
  hipLaunchKernelGGL(k_rn_copy, blocks, dim3(256), 0, c->stream, c->res_ttext.get(), c->res_toff.get(), r0, r1, out);
}

// Behind the sort + collapse of fastq_prep_run, the text still resident: rank, measure, size, and render the records
// into the context's read text (the buffers and the stamp of musc_results_set_read_text); the line offsets stay for
// musc_reads_names_text.
static int read_names_stage(musc_ctx* c, const char* who, const unsigned char* d_text, uint64_t nbytes, const uint64_t* d_name_off,
                            const uint32_t* d_name_len, const uint32_t* d_seq_len, const musc_fastq_prep* fp, musc_read_names* info) {
  const uint64_t n = fp->n_reads, nu = fp->n_unique;
  drop_read_text(c);
  for (uint64_t g = 0; g < nu; g++) {
    const musc_rn::Path p = musc_rn::group_path(fp->ustart[g + 1] - fp->ustart[g]);
    (p == musc_rn::PATH_SINGLE ? info->n_single : p == musc_rn::PATH_WAVE ? info->n_counted : info->n_sorted)++;
  }
  HIPCHK(c, c->res_toff.alloc((nu + 1) * 8));
  HIPCHK(c, c->rn_loff.alloc((nu + 1) * 8));
  if (n == 0) {
    HIPCHK(c, c->res_ttext.alloc(16));
    HIPCHK(c, hipMemsetAsync(c->res_toff.get(), 0, 8, c->stream));
    HIPCHK(c, hipMemsetAsync(c->rn_loff.get(), 0, 8, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
  }
  float ms = 0;
  const int rc = timed(c, &ms, [&]() -> int {
    const dim3 B256(256);
    TmpBufs B;
    RnInput in;
    in.rd = musc_rn::TextBytes{d_text, nbytes};
    in.N = musc_rn::Names{d_name_off, d_name_len, n};
    in.nu = nu;
    uint32_t *ranked = nullptr, *gid = nullptr, *meta = nullptr, *tstart = nullptr, *gsum = nullptr;
    uint64_t* stmp = nullptr;
    int r = 0;
    if ((r = staged(c, who, B, (const uint32_t*)fp->order, n * 4, 0, 0, &in.order)) ||
        (r = staged(c, who, B, (const uint32_t*)fp->ustart, (nu + 1) * 4, 0, 0, &in.ustart)) || (r = tmp_alloc(c, who, B, &ranked, n * 4)) ||
        (r = tmp_alloc(c, who, B, &gid, n * 4)) || (r = tmp_alloc(c, who, B, &meta, n * 4)) || (r = tmp_alloc(c, who, B, &tstart, n * 4)) ||
        (r = tmp_alloc(c, who, B, &gsum, nu * 4)) || (r = tmp_alloc(c, who, B, &stmp, scan_tmp_elems(nu + 1) * 8)))
      return r;
    hipLaunchKernelGGL(k_rn_measure, grid(c, n), B256, 0, c->stream, in.rd, in.N, meta);
    HIPCHK(c, hipGetLastError());
    uint32_t passes = 0;
    if ((r = rn_rank(c, who, in, ranked, gid, &info->n_pairs, &passes))) return r;
    info->key_passes = passes;
    // ---- sizes per group, offsets by scan
    uint64_t *roff = c->res_toff.get(), *loff = c->rn_loff.get();
    HIPCHK(c, hipMemsetAsync(roff + nu, 0, 8, c->stream));
    HIPCHK(c, hipMemsetAsync(loff + nu, 0, 8, c->stream));
    hipLaunchKernelGGL(k_rn_sizes, grid(c, nu), B256, 0, c->stream, ranked, in.ustart, meta, d_seq_len, nu, tstart, gsum, roff, loff);
    HIPCHK(c, hipGetLastError());
    if ((r = scan_u64(c, roff, roff, nu + 1, stmp)) || (r = scan_u64(c, loff, loff, nu + 1, stmp))) return r;
    HIPCHK(c, Readback(c->scalars, c->stream).get(roff + nu, &info->text_bytes).get(loff + nu, &info->line_bytes).wait());
    // (a record is at most 10 digits, a tab and JOIN_LIMIT bytes: a total beyond that is not the sizes' own)
    if (info->text_bytes > nu * (uint64_t)(11 + musc_rn::JOIN_LIMIT))
      return fail(c, 11, "%s: %llu bytes of read text for %llu reads", who, (unsigned long long)info->text_bytes, (unsigned long long)nu);
    // ---- the records, where musc_results_set_read_text would have put them
    HIPCHK(c, c->res_ttext.alloc(info->text_bytes + 16));
    const musc_rn::Groups G{ranked, in.ustart, meta, tstart, gsum};
    const dim3 blocks = stage_grid(c, info->text_bytes / 256 + 1, musc_launch::CAP_TILES);
    hipLaunchKernelGGL(k_rn_records, blocks, B256, 0, c->stream, in.rd, in.N, G, roff, (uint64_t)0, nu,
                       reinterpret_cast<unsigned char*>(c->res_ttext.get()));
    HIPCHK(c, hipGetLastError());
    if (!(info->ranked = (uint32_t*)malloc(n * 4))) return fail(c, 7, "out of host memory for the ranked members");
    HIPCHK(c, hipMemcpyAsync(info->ranked, ranked, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // (the temporaries go with B)
    return 0;
  });
  if (rc) return rc;
  info->ms_names = ms;
  return 0;
}

extern "C" int musc_reads_prep_fastq_names(musc_ctx* c, const char* text, uint64_t nbytes, int on_device, int32_t min_read_len,
                                           int32_t max_read_len, musc_fastq_prep* out, musc_read_names* info) {
  static const char* const who = "musc_reads_prep_fastq_names";
  if (!c) return 1;
  if (out) memset(out, 0, sizeof *out);
  if (info) memset(info, 0, sizeof *info);
  if (!out || !info) return fail(c, 2, "%s: NULL output pointer", who);
  if (!text && nbytes) return fail(c, 2, "%s: NULL input", who);
  HIPCHK(c, hipSetDevice(c->device));
  free_reads(c);
  if (max_read_len < 0) return reads_load_done(c, fail(c, 2, "%s: max_read_len %d is negative", who, max_read_len));
  const int rc = fastq_prep_run(c, who, text, nbytes, on_device, min_read_len, (uint32_t)max_read_len, out, true,
                                [&](const unsigned char* d_text, const uint64_t* d_name_off, const uint32_t* d_name_len, const uint32_t* d_seq_len) {
                                  return read_names_stage(c, who, d_text, nbytes, d_name_off, d_name_len, d_seq_len, out, info);
                                });
  if (reads_load_done(c, rc)) {  // nothing stale: no reads and no read text, and behind its wait no arrays and no counts
    musc_fastq_prep_free(out);
    free(info->ranked);
    memset(info, 0, sizeof *info);
  }
  return rc;
}

extern "C" int musc_reads_names_text(musc_ctx* c, int which, uint64_t rec0, uint64_t nrec, char* dst, uint64_t capacity, int dst_on_device,
                                     uint64_t* nbytes) {
  if (!c) return 1;
  if (!nbytes) return fail(c, 2, "musc_reads_names_text: nbytes is NULL");
  *nbytes = 0;
  if (which < 0 || which > 1) return fail(c, 2, "musc_reads_names_text: no such text (%d)", which);
  if (!c->rn_loff || !c->res_toff || !c->res_ttext)
    return fail(c, 2, "musc_reads_names_text: no read names rendered (musc_reads_prep_fastq_names)");
  const TextDesc t = {which ? c->rn_loff.get() : c->res_toff.get(), c->nreads, "musc_reads_names_text",
                      "a record no longer fits the reads in hand", &c->rn_ms_text};
  return text_range(c, t, rec0, nrec, dst, capacity, dst_on_device, nbytes, [&](uint64_t r0, uint64_t r1, uint64_t bytes, unsigned char* out) {
    if (which) launch_rn_lines(c, r0, r1, bytes, out); else launch_rn_copy(c, r0, r1, bytes, out);
  });
}
