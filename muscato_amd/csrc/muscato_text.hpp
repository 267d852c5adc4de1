// muscato_text.hpp -- the host side of the texts rendered on the device: results.txt (musc_results_*) and
// the nonmatch FASTQ, genestats and readstats (musc_side_*).  Part of libmuscato_hip.so: included by
// muscato_hip.hip after the context, what the drivers share (grid, the scans, tmp_alloc, KeyPasses, Readback), the event
// marks (timed) and drop_gene_text / drop_read_text.  Both families build
// record lists with 64-bit byte offsets and render ranges of them through one driver, text_range.
#pragma once

#include "text_stage.hpp"

// A text as musc_results_text and musc_side_text see it: n records, record i = bytes [off[i], off[i + 1]) of the text.
struct TextDesc {
  const uint64_t* off;  // device, n + 1 offsets
  uint64_t n;
  const char* name;     // of the public call, for messages
  const char* unfit;    // the code-11 message: a record the kernel refused to render
  float* ms_text;       // accumulates the event time of the calls that render
};

// Records [rec0, rec0 + nrec) of a text, clipped at its end, into dst; `launch(r0, r1, bytes, out)` queues the kernel
// that renders records [r0, r1), `bytes` in all, at `out` on the device.  dst == NULL only reports the size.  A device
// destination takes one launch.  A host destination is filled through res_stage: the offsets come to the host in
// windows of MUSC_DEBUG_STAGE_LINES records, and each window goes in pieces of the most records that fit
// MUSC_DEBUG_STAGE_BYTES (text_stage.hpp), rendered, copied and waited for one after the other.
// *nbytes = the bytes of the range on success and 0 on every failure.
template <class Launch>
static int text_range(musc_ctx* c, const TextDesc& t, uint64_t rec0, uint64_t nrec, char* dst, uint64_t capacity, int dst_on_device,
                      uint64_t* nbytes, Launch launch) {
  *nbytes = 0;
  if (rec0 >= t.n || nrec == 0) return 0;
  const uint64_t r0 = rec0, r1 = nrec > t.n - rec0 ? t.n : rec0 + nrec;
  HIPCHK(c, hipSetDevice(c->device));
  uint64_t bytes = 0;
  float ms = 0;
  int rc = timed(c, &ms, [&]() -> int {
    uint64_t o0 = 0, o1 = 0;
    HIPCHK(c, Readback(c->scalars, c->stream).get(t.off + r0, &o0).get(t.off + r1, &o1).wait());
    bytes = o1 - o0;
    if (!dst) return 0;
    if (capacity < bytes)
      return fail(c, 2, "%s: capacity %llu < %llu bytes", t.name, (unsigned long long)capacity, (unsigned long long)bytes);
    HIPCHK(c, hipMemsetAsync(c->d_flag, 0, 4, c->stream));  // raised by a record the kernel refuses to render
    if (dst_on_device) {
      launch(r0, r1, bytes, reinterpret_cast<unsigned char*>(dst));
      HIPCHK(c, hipGetLastError());
      return 0;
    }
    const uint64_t stage = c->env.stage_bytes;
    std::vector<uint64_t> off;
    for (uint64_t b0 = r0; b0 < r1;) {
      const uint64_t nw = std::min(r1 - b0, c->env.stage_lines);  // this window: records [b0, b0 + nw)
      off.resize(nw + 1);
      HIPCHK(c, hipMemcpyAsync(off.data(), t.off + b0, (nw + 1) * 8, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
      for (uint64_t p0 = 0; p0 < nw;) {
        const uint64_t p1 = musc_text::stage_piece_end(off.data(), nw, p0, stage);
        const uint64_t pb = off[p1] - off[p0];
        const int re = ensure(c, c->res_stage, std::max(pb, stage));
        if (re) return re;
        launch(b0 + p0, b0 + p1, pb, c->res_stage.p);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(dst + (off[p0] - o0), c->res_stage.p, pb, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        p0 = p1;
      }
      b0 += nw;
    }
    return 0;
  });
  if (rc) return rc;
  if (dst) {
    uint32_t bad = 0;
    HIPCHK(c, Readback(c->scalars, c->stream).get(c->d_flag.get(), &bad).wait());
    if (bad) return fail(c, 11, "%s: %s", t.name, t.unfit);
    *t.ms_text += ms;
  }
  *nbytes = bytes;
  return 0;
}

// ---------------------------------------------------------------- results.txt on the device
// The post-chain of cmd/muscato/main.go:422-676 from the resident tuples: musc_results_order drops the tuples of genes
// without an id line, orders the rest as `sort -k1` orders their six-column lines and computes every line's byte
// offset; musc_results_text renders a range of lines (kernels_results.hpp).

static ResData res_data(const musc_ctx* c) {
  ResData D;
  D.rd = c->rd;
  D.rdm = c->reads_have_x ? c->rdm : nullptr;
  D.db2 = c->db2;
  D.dbm2 = c->db_has_x ? c->dbm2 : nullptr;
  D.seq_off = c->seq_off;
  D.gtext = c->res_gtext;
  D.goff = c->res_goff;
  D.ttext = c->res_ttext;
  D.toff = c->res_toff;
  D.nreads = c->nreads;
  D.nseq = c->nseq;
  D.rw = c->rw;
  return D;
}

// text + offsets of n items to the device (the offsets must not decrease; item i = bytes [offsets[i], offsets[i + 1]))
static int upload_text(musc_ctx* c, const char* what, const char* text, const uint64_t* offsets, uint64_t n, DevPtr<char>* d_text, DevPtr<uint64_t>* d_off) {
  for (uint64_t i = 0; i < n; i++)
    if (offsets[i + 1] < offsets[i]) return fail(c, 2, "%s: offsets decrease at item %llu", what, (unsigned long long)i);
  const uint64_t bytes = offsets[n];
  HIPCHK(c, d_text->alloc(bytes + 16));
  HIPCHK(c, d_off->alloc((n + 1) * 8));
  if (bytes) HIPCHK(c, hipMemcpyAsync(d_text->get(), text, bytes, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_off->get(), offsets, (n + 1) * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

int musc_results_set_gene_text(musc_ctx* c, const char* text, const uint64_t* offsets, const uint8_t* absent, uint32_t nseq) {
  if (!c) return 1;
  if (!offsets || (!text && offsets[nseq] != 0)) return fail(c, 2, "musc_results_set_gene_text: NULL input");
  if (!c->db2 || nseq != c->nseq)
    return fail(c, 2, "musc_results_set_gene_text: text of %u genes for a database of %u targets", nseq, c->nseq);
  HIPCHK(c, hipSetDevice(c->device));
  drop_gene_text(c);  // (a new text leaves the tuple list as good as it was)
  // ... and one that cannot be put in place leaves no text and no list, as it always has
  auto failed = [c](int rc) { return drop_gene_text(c), c->st.list_forgotten(), rc; };
  int rc = upload_text(c, "musc_results_set_gene_text", text, offsets, nseq, &c->res_gtext, &c->res_goff);
  if (rc) return failed(rc);
  // rank of each gene's text among all of them, bytewise; equal texts share a rank
  std::vector<uint32_t> order;
  order.reserve(nseq);
  for (uint32_t g = 0; g < nseq; g++)
    if (!absent || !absent[g]) order.push_back(g);
  auto cmp = [&](uint32_t a, uint32_t b) {
    const uint64_t la = offsets[a + 1] - offsets[a], lb = offsets[b + 1] - offsets[b];
    const int d = memcmp(text + offsets[a], text + offsets[b], (size_t)std::min(la, lb));
    return d ? d : la < lb ? -1 : la > lb ? 1 : 0;
  };
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return cmp(a, b) < 0; });
  std::vector<uint32_t> rank(nseq, RES_ABSENT);
  uint32_t rk = 0;
  for (size_t i = 0; i < order.size(); i++) {
    if (i && cmp(order[i - 1], order[i]) != 0) rk++;
    rank[order[i]] = rk;
  }
  hipError_t e = c->res_rank.alloc((uint64_t)nseq * 4 + 16);
  if (e == hipSuccess) e = hipMemcpy(c->res_rank, rank.data(), (uint64_t)nseq * 4, hipMemcpyHostToDevice);
  if (e != hipSuccess) return failed(fail(c, 10, "musc_results_set_gene_text: %s", hipGetErrorString(e)));
  // for the side outputs: the form of the texts, and the rank of each gene's name alone
  c->side_bad_gene = musc_side::first_bad_form(text, offsets, absent, nseq);
  c->side_form_ok = c->side_bad_gene == nseq;
  if (c->side_form_ok) {
    const musc_side::NameRanks R = musc_side::name_ranks(text, offsets, absent, nseq);
    std::vector<uint2> names(R.rep.size());
    for (size_t k = 0; k < names.size(); k++) names[k] = make_uint2(R.rep[k], R.len[k]);
    e = c->side_nrank.alloc((uint64_t)nseq * 4 + 16);
    if (e == hipSuccess) e = c->side_names.alloc(names.size() * 8 + 16);
    if (e == hipSuccess) e = hipMemcpy(c->side_nrank, R.rank.data(), (uint64_t)nseq * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess && !names.empty()) e = hipMemcpy(c->side_names, names.data(), names.size() * 8, hipMemcpyHostToDevice);
    if (e != hipSuccess) return failed(fail(c, 10, "musc_results_set_gene_text: %s", hipGetErrorString(e)));
    c->side_nnames = (uint32_t)names.size();
  }
  return 0;
}

int musc_results_set_read_text(musc_ctx* c, const char* text, const uint64_t* offsets, uint64_t nreads) {
  if (!c) return 1;
  if (!offsets || (!text && offsets[nreads] != 0)) return fail(c, 2, "musc_results_set_read_text: NULL input");
  if (nreads != c->nreads)
    return fail(c, 2, "musc_results_set_read_text: text of %llu reads, %llu are loaded", (unsigned long long)nreads, (unsigned long long)c->nreads);
  HIPCHK(c, hipSetDevice(c->device));
  drop_read_text(c);
  const int rc = upload_text(c, "musc_results_set_read_text", text, offsets, nreads, &c->res_ttext, &c->res_toff);
  if (rc) drop_read_text(c);
  return rc;
}

int musc_results_number_key(uint32_t pos, uint32_t nmiss, uint64_t* key) {
  if (!key || nmiss > 99999u) return 2;
  *key = res_number_key(pos, nmiss);
  return 0;
}

static int results_order_impl(musc_ctx* c, const musc_hit* hits, uint64_t n, int on_device) {
  const dim3 B256(256);
  const uint4* d_in = reinterpret_cast<const uint4*>(hits);
  TmpBufs B;
  if (!hits) {
    if (!c->st.may_order_resident())
      return fail(c, 2, "musc_results_order: the resident tuple list is not that of a pass over the reads and the database in hand");
    d_in = reinterpret_cast<const uint4*>(c->hits.p);
    n = c->nhits;
  } else if (on_device && ((uintptr_t)hits & 15u)) {
    return fail(c, 2, "musc_results_order: a device list must be 16-byte aligned");
  } else if (!on_device && n) {
    // a host list is checked here, before it is uploaded (a device list: k_results_flag)
    for (uint64_t i = 0; i < n; i++) {
      const musc_hit& h = hits[i];
      if (h.read_idx >= c->nreads || h.gene_idx >= c->nseq || h.nmiss > RES_MAX_NMISS ||
          h.pos > c->h_seq_off[(size_t)h.gene_idx + 1] - c->h_seq_off[h.gene_idx])
        return fail(c, 2, "musc_results_order: tuple %llu (read %u, gene %u, pos %u, nmiss %u) is outside the loaded reads and targets",
                    (unsigned long long)i, h.read_idx, h.gene_idx, h.pos, h.nmiss);
    }
    uint4* up = nullptr;
    HIPCHK(c, B.alloc(&up, n * 16));
    HIPCHK(c, hipMemcpyAsync(up, hits, n * 16, hipMemcpyHostToDevice, c->stream));
    d_in = up;
  }
  if (n >= 0xFFFFFFF0ull) return fail(c, 2, "musc_results_order: too many tuples for 32-bit line numbers");
  int rc;
  if ((rc = ensure(c, c->res_off, n + 1))) return rc;
  if (n == 0) {
    HIPCHK(c, hipMemsetAsync(c->res_off.p, 0, 8, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
  }

  // ---- validate, drop the tuples of absent genes
  uint32_t *keep = nullptr, *excl = nullptr, *stmp = nullptr;
  uint4* a = nullptr;
  HIPCHK(c, B.alloc(&keep, n * 4));
  HIPCHK(c, B.alloc(&excl, n * 4));
  HIPCHK(c, B.alloc(&stmp, scan_tmp_elems(n) * 4));
  HIPCHK(c, hipMemsetAsync(c->d_flag, 0, 4, c->stream));
  hipLaunchKernelGGL(k_results_flag, grid(c, n), B256, 0, c->stream, d_in, n, c->nreads, c->nseq, c->seq_off, c->res_rank, keep, c->d_flag);
  HIPCHK(c, hipGetLastError());
  if ((rc = scan_u32(c, keep, excl, n, false, stmp))) return rc;
  Readback R(c->scalars, c->stream);
  uint32_t verdict = 0;
  uint64_t kept_before = 0, kept_last = 0;
  HIPCHK(c, R.get(c->d_flag.get(), &verdict).get(excl + (n - 1), &kept_before).get(keep + (n - 1), &kept_last).wait());
  if (verdict & 1u)
    return fail(c, 2, "musc_results_order: a tuple names a read, a target or a position outside the loaded reads and targets");
  const bool read_major = !(verdict & 2u);
  const uint64_t m = kept_before + kept_last;
  if ((rc = ensure(c, c->res_hits, std::max<uint64_t>(m, 1)))) return rc;
  uint4* const out = reinterpret_cast<uint4*>(c->res_hits.p);
  if (m == 0) {
    HIPCHK(c, hipMemsetAsync(c->res_off.p, 0, 8, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
  }
  HIPCHK(c, B.alloc(&a, m * 16));
  hipLaunchKernelGGL(k_results_compact, grid(c, n), B256, 0, c->stream, d_in, keep, excl, n, a);
  HIPCHK(c, hipGetLastError());

  static const char* const who = "musc_results_order";
  // one stable pass of K over the k tuples a[idx[.]] (idx null: a itself) on the key word `what`
  auto sort_pass = [&](KeyPasses& K, const uint32_t* idx, uint64_t k, uint32_t what, unsigned end_bit) {
    return K.pass(end_bit, [&](const uint32_t* perm, uint64_t* keys) {
      hipLaunchKernelGGL(k_results_keys, grid(c, k), B256, 0, c->stream, a, idx, perm, k, what, c->res_rank, c->rd, c->rw, c->db2,
                         c->db_has_x ? c->dbm2 : (const uint32_t*)nullptr, c->seq_off, keys);
    });
  };

  // ---- a list that is not read-major (a host list in any order): one sort on read_idx first
  if (!read_major) {
    KeyPasses K;
    uint4* a2 = nullptr;
    if ((rc = K.start(c, who, m, {32u, 33u, 60u, 63u}))) return rc;
    HIPCHK(c, B.alloc(&a2, m * 16));
    if ((rc = sort_pass(K, nullptr, m, RES_KEY_READ, 32u))) return rc;
    hipLaunchKernelGGL(k_results_gather, grid(c, m), B256, 0, c->stream, a, K.order(), m, a2);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));  // (K's buffers are released at the end of this scope)
    a = a2;
  }

  // ---- read segments: a read with one tuple is in place; the others are sorted
  uint32_t *multi = nullptr, *incl = nullptr, *idx = nullptr;
  HIPCHK(c, B.alloc(&multi, m * 4));
  HIPCHK(c, B.alloc(&incl, m * 4));
  HIPCHK(c, hipMemsetAsync(c->counters + CNT_SCRATCH, 0, 8, c->stream));
  hipLaunchKernelGGL(k_results_segments, grid(c, m), B256, 0, c->stream, a, m, c->rd, c->rw, multi, c->counters + CNT_SCRATCH);
  HIPCHK(c, hipGetLastError());
  if ((rc = scan_u32(c, multi, incl, m, true, stmp))) return rc;  // (m <= n: stmp is large enough)
  uint64_t k = 0, maxlen = 0;
  HIPCHK(c, R.get(incl + (m - 1), &k).get(c->counters + CNT_SCRATCH, &maxlen).wait());
  if (k == 0) {
    HIPCHK(c, hipMemcpyAsync(out, a, m * 16, hipMemcpyDeviceToDevice, c->stream));
  } else {
    KeyPasses K;
    if ((rc = K.start(c, who, k, {32u, 33u, 60u, 63u})) || (rc = tmp_alloc(c, who, K.B, &idx, k * 4))) return rc;
    hipLaunchKernelGGL(k_results_idx, grid(c, m), B256, 0, c->stream, multi, incl, m, idx);
    HIPCHK(c, hipGetLastError());
    // least significant first: gene rank, the number word, the target words from last to first, the read
    const uint32_t nw = (uint32_t)((maxlen + RES_BASES_PER_WORD - 1) / RES_BASES_PER_WORD);
    if ((rc = sort_pass(K, idx, k, RES_KEY_RANK, 32u))) return rc;
    if ((rc = sort_pass(K, idx, k, RES_KEY_NUMBER, 60u))) return rc;
    for (uint32_t w = nw; w-- > 0;)
      if ((rc = sort_pass(K, idx, k, RES_KEY_SPAN + w, 63u))) return rc;
    if ((rc = sort_pass(K, idx, k, RES_KEY_READ, 32u))) return rc;
    hipLaunchKernelGGL(k_results_place, grid(c, m), B256, 0, c->stream, a, multi, incl, idx, K.order(), m, out);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }

  // ---- line lengths -> offsets
  uint64_t* stmp64 = nullptr;
  HIPCHK(c, B.alloc(&stmp64, scan_tmp_elems(m + 1) * 8));
  hipLaunchKernelGGL(k_results_len, grid(c, m + 1), B256, 0, c->stream, out, m, res_data(c), c->res_off.p);
  HIPCHK(c, hipGetLastError());
  if ((rc = scan_u64(c, c->res_off.p, c->res_off.p, m + 1, stmp64))) return rc;
  uint64_t res_bytes = 0;
  HIPCHK(c, R.get(c->res_off.p + m, &res_bytes).wait());
  c->res_n = m;
  c->res_bytes = res_bytes;
  return 0;
}

int musc_results_order(musc_ctx* c, const musc_hit* hits, uint64_t n, int on_device, uint64_t* nlines, uint64_t* nbytes) {
  if (!c) return 1;
  if (nlines) *nlines = 0;
  if (nbytes) *nbytes = 0;
  c->st.order_begins();  // (whatever comes of this call, the last order and what was prepared from it are gone)
  c->res_n = c->res_bytes = 0;
  if (!c->db2 || !c->res_gtext || !c->res_rank) return fail(c, 2, "musc_results_order: no gene text (musc_results_set_gene_text)");
  if (c->up.active) return fail(c, 2, "musc_results_order: a streamed read load has not been matched yet");
  HIPCHK(c, hipSetDevice(c->device));
  const int rc = timed(c, &c->res_ms_order, [&] { return results_order_impl(c, hits, n, on_device); });
  if (rc) return rc;
  c->res_ms_text = 0;
  c->st.order_made();
  if (nlines) *nlines = c->res_n;
  if (nbytes) *nbytes = c->res_bytes;
  return 0;
}

int musc_results_hits(musc_ctx* c, musc_hit* dst, uint64_t capacity, int dst_on_device) {
  if (!c) return 1;
  if (!c->st.ordered_current()) return fail(c, 2, "musc_results_hits: no ordered list (musc_results_order)");
  if (capacity < c->res_n) return fail(c, 2, "musc_results_hits: capacity %llu < %llu tuples", (unsigned long long)capacity, (unsigned long long)c->res_n);
  if (c->res_n == 0) return 0;
  if (!dst) return fail(c, 2, "musc_results_hits: dst is NULL");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(dst, c->res_hits.p, c->res_n * sizeof(musc_hit), dst_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

static void launch_render(musc_ctx* c, uint64_t l0, uint64_t l1, unsigned char* out) {
  const uint64_t nl = l1 - l0;
  const dim3 blocks = stage_grid(c, (nl + 3) / 4, musc_launch::CAP_TILES);
  hipLaunchKernelGGL(k_results_render, blocks, dim3(256), 0, c->stream, reinterpret_cast<const uint4*>(c->res_hits.p), c->res_off.p, l0, l1,
                     res_data(c), out, c->d_flag);
}

int musc_results_text(musc_ctx* c, uint64_t line0, uint64_t nlines, char* dst, uint64_t capacity, int dst_on_device, uint64_t* nbytes) {
  if (!c) return 1;
  if (!nbytes) return fail(c, 2, "musc_results_text: nbytes is NULL");
  *nbytes = 0;
  if (!c->st.ordered_current()) return fail(c, 2, "musc_results_text: no ordered list (musc_results_order)");
  const TextDesc t = {c->res_off.p, c->res_n, "musc_results_text",
                      "a line of the ordered list no longer fits the reads, the database or the texts in hand", &c->res_ms_text};
  return text_range(c, t, line0, nlines, dst, capacity, dst_on_device, nbytes,
                    [&](uint64_t l0, uint64_t l1, uint64_t, unsigned char* out) { launch_render(c, l0, l1, out); });
}

int musc_results_last_ms(musc_ctx* c, float* ms_order, float* ms_text) {
  if (!c) return 1;
  if (ms_order) *ms_order = c->res_ms_order;
  if (ms_text) *ms_text = c->res_ms_text;
  return 0;
}

// ---------------------------------------------------------------- the side outputs on the device
// The nonmatch FASTQ (cmd/muscato_nonmatch/main.go:95-114, an exact set for the Bloom filter), `*_genestats`
// (cmd/muscato/main.go:94-150 + cmd/muscato_genestats/main.go) and `*_readstats` (cmd/muscato_readstats/main.go, the
// gene set sorted) from the ordered list of the last musc_results_order: musc_side_prepare builds the record lists
// and their byte offsets, musc_side_text renders a range of records (kernels_side.hpp).

static const int MUSC_SIDE_ERR_FORM = 12;  // the gene text is not in the simple form: the caller's cue for its host path

static SideData side_data(const musc_ctx* c) {
  SideData D;
  D.rd = c->rd;
  D.rdm = c->reads_have_x ? c->rdm : nullptr;
  D.ttext = c->res_ttext;
  D.toff = c->res_toff;
  D.tok = c->side_tok.p;
  D.gtext = c->res_gtext;
  D.goff = c->res_goff;
  D.names = c->side_names;
  D.nreads = c->nreads;
  D.nseq = c->nseq;
  D.nnames = c->side_nnames;
  D.rw = c->rw;
  return D;
}

// flag / len over n + 1 items (the last one empty) -> the record list of text `which`: idx (when the text has one),
// offsets, counts.  excl and stmp are scratch for n + 1 items; len is scanned in place.
static int side_records(musc_ctx* c, int which, const uint32_t* flag, uint32_t* excl, uint64_t* len, uint64_t n, uint32_t* stmp,
                        uint64_t* stmp64) {
  int rc;
  if ((rc = scan_u32(c, flag, excl, n + 1, false, stmp))) return rc;
  if ((rc = scan_u64(c, len, len, n + 1, stmp64))) return rc;
  uint64_t nrec = 0, nbytes = 0;
  HIPCHK(c, Readback(c->scalars, c->stream).get(excl + n, &nrec).get(len + n, &nbytes).wait());
  if ((rc = ensure(c, c->side_idx[which], std::max<uint64_t>(nrec, 1)))) return rc;
  if ((rc = ensure(c, c->side_off[which], nrec + 1))) return rc;
  hipLaunchKernelGGL(k_side_compact, grid(c, n + 1), dim3(256), 0, c->stream, flag, excl, len, n, c->side_idx[which].p, c->side_off[which].p);
  HIPCHK(c, hipGetLastError());
  c->side_nrec[which] = nrec;
  c->side_nbytes[which] = nbytes;
  return 0;
}

static int side_prepare_impl(musc_ctx* c) {
  const dim3 B256(256);
  const uint64_t nreads = c->nreads, m = c->res_n, nnames = c->side_nnames;
  const uint4* const hits = reinterpret_cast<const uint4*>(c->res_hits.p);
  int rc;
  TmpBufs B;
  Readback R(c->scalars, c->stream);
  HIPCHK(c, hipMemsetAsync(c->d_flag, 0, 4, c->stream));

  // ---- tokens: once per read text
  if (!c->st.tokens_current()) {
    if ((rc = ensure(c, c->side_tok, std::max<uint64_t>(nreads, 1)))) return rc;
    hipLaunchKernelGGL(k_side_tokens, grid(c, nreads), B256, 0, c->stream, c->res_ttext, c->res_toff, nreads, c->side_tok.p, c->d_flag);
    HIPCHK(c, hipGetLastError());
  }

  // ---- mark the matched reads, count the tuples of every name
  const uint64_t nmax = std::max(std::max(nreads, nnames), m) + 1;  // items of the largest scan below
  uint32_t *matched = nullptr, *flag = nullptr, *excl = nullptr, *stmp = nullptr;
  uint64_t *len = nullptr, *stmp64 = nullptr;
  HIPCHK(c, B.alloc(&matched, (nreads + 1) * 4));
  HIPCHK(c, B.alloc(&flag, nmax * 4));
  HIPCHK(c, B.alloc(&excl, nmax * 4));
  HIPCHK(c, B.alloc(&stmp, scan_tmp_elems(nmax) * 4));
  HIPCHK(c, B.alloc(&len, nmax * 8));
  HIPCHK(c, B.alloc(&stmp64, scan_tmp_elems(nmax) * 8));
  if ((rc = ensure(c, c->side_cnt, std::max<uint64_t>(nnames, 1)))) return rc;
  HIPCHK(c, hipMemsetAsync(matched, 0, (nreads + 1) * 4, c->stream));
  HIPCHK(c, hipMemsetAsync(c->side_cnt.p, 0, std::max<uint64_t>(nnames, 1) * 4, c->stream));
  if (m) {
    hipLaunchKernelGGL(k_side_mark, grid(c, m), B256, 0, c->stream, hits, m, c->side_nrank, nreads, c->nseq, (uint32_t)nnames, matched,
                       c->side_cnt.p, c->d_flag);
    HIPCHK(c, hipGetLastError());
  }
  uint32_t bad = 0;
  HIPCHK(c, R.get(c->d_flag.get(), &bad).wait());
  if (bad) return fail(c, 11, "musc_side_prepare: a read's text is longer than 4 GiB, or the ordered list no longer fits the reads and the gene text in hand");
  c->st.tokens_made();
  const SideData D = side_data(c);

  // ---- nonmatch: the unmatched reads that have a token
  hipLaunchKernelGGL(k_side_nm_len, grid(c, nreads + 1), B256, 0, c->stream, D, matched, flag, len);
  HIPCHK(c, hipGetLastError());
  if ((rc = side_records(c, MUSC_SIDE_NONMATCH, flag, excl, len, nreads, stmp, stmp64))) return rc;

  // ---- genestats: the names with a tuple
  hipLaunchKernelGGL(k_side_gs_len, grid(c, nnames + 1), B256, 0, c->stream, D, c->side_cnt.p, flag, len);
  HIPCHK(c, hipGetLastError());
  if ((rc = side_records(c, MUSC_SIDE_GENESTATS, flag, excl, len, nnames, stmp, stmp64))) return rc;

  // ---- readstats: runs of equal tokens over the matched reads that have one
  c->side_nel = 0;
  c->side_nrec[MUSC_SIDE_READSTATS] = c->side_nbytes[MUSC_SIDE_READSTATS] = 0;
  if ((rc = ensure(c, c->side_off[MUSC_SIDE_READSTATS], 1))) return rc;
  HIPCHK(c, hipMemsetAsync(c->side_off[MUSC_SIDE_READSTATS].p, 0, 8, c->stream));
  hipLaunchKernelGGL(k_side_rs_flag, grid(c, nreads + 1), B256, 0, c->stream, matched, c->side_tok.p, nreads, flag);
  HIPCHK(c, hipGetLastError());
  if ((rc = scan_u32(c, flag, excl, nreads + 1, false, stmp))) return rc;
  uint64_t ncr = 0;
  HIPCHK(c, R.get(excl + nreads, &ncr).wait());
  if (ncr == 0 || m == 0) return 0;
  uint32_t *cr = nullptr, *head = nullptr, *incl = nullptr, *runof = nullptr;
  HIPCHK(c, B.alloc(&cr, ncr * 4));
  HIPCHK(c, B.alloc(&head, ncr * 4));
  HIPCHK(c, B.alloc(&incl, ncr * 4));
  HIPCHK(c, B.alloc(&runof, nreads * 4));
  hipLaunchKernelGGL(k_side_compact, grid(c, nreads + 1), B256, 0, c->stream, flag, excl, (const uint64_t*)nullptr, nreads, cr, (uint64_t*)nullptr);
  hipLaunchKernelGGL(k_side_rs_heads, grid(c, ncr), B256, 0, c->stream, cr, ncr, D, head);
  HIPCHK(c, hipGetLastError());
  if ((rc = scan_u32(c, head, incl, ncr, true, stmp))) return rc;
  uint64_t nruns = 0;
  HIPCHK(c, R.get(incl + (ncr - 1), &nruns).wait());
  if ((rc = ensure(c, c->side_runread, nruns))) return rc;
  if ((rc = ensure(c, c->side_first, nruns + 1))) return rc;
  if ((rc = ensure(c, c->side_off[MUSC_SIDE_READSTATS], nruns + 1))) return rc;
  HIPCHK(c, hipMemsetAsync(runof, 0xFF, nreads * 4, c->stream));
  HIPCHK(c, hipMemsetAsync(c->side_first.p, 0, (nruns + 1) * 4, c->stream));  // (every run has an element; were one without, it reads element 0)
  hipLaunchKernelGGL(k_side_rs_runs, grid(c, ncr), B256, 0, c->stream, cr, head, incl, ncr, runof, c->side_runread.p);
  HIPCHK(c, hipGetLastError());

  // one key per kept tuple, sorted; the distinct keys are the elements of the lines
  uint64_t *k0 = nullptr, *k1 = nullptr;
  void* tmp = nullptr;
  size_t tmp_bytes = 0;
  HIPCHK(c, B.alloc(&k0, m * 8));
  HIPCHK(c, B.alloc(&k1, m * 8));
  HIPCHK(c, rocprim::radix_sort_keys(nullptr, tmp_bytes, k0, k1, (size_t)m, 0u, 64u, c->stream));
  HIPCHK(c, B.alloc(&tmp, tmp_bytes));
  hipLaunchKernelGGL(k_side_rs_keys, grid(c, m), B256, 0, c->stream, hits, m, runof, c->side_nrank, k0);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, rocprim::radix_sort_keys(tmp, tmp_bytes, k0, k1, (size_t)m, 0u, 64u, c->stream));
  hipLaunchKernelGGL(k_side_rs_uniq, grid(c, m + 1), B256, 0, c->stream, k1, m, flag);
  HIPCHK(c, hipGetLastError());
  if ((rc = scan_u32(c, flag, excl, m + 1, false, stmp))) return rc;
  uint64_t nel = 0;
  HIPCHK(c, R.get(excl + m, &nel).wait());
  if (nel < nruns) return fail(c, 11, "musc_side_prepare: a run of reads without an element");
  if ((rc = ensure(c, c->side_el, nel))) return rc;
  if ((rc = ensure(c, c->side_eloff, nel + 1))) return rc;
  hipLaunchKernelGGL(k_side_rs_elems, grid(c, m), B256, 0, c->stream, k1, flag, excl, m, c->side_el.p);
  hipLaunchKernelGGL(k_side_rs_len, grid(c, nel + 1), B256, 0, c->stream, c->side_el.p, nel, (uint32_t)nruns, D, c->side_runread.p,
                     c->side_eloff.p, c->side_first.p);
  HIPCHK(c, hipGetLastError());
  if ((rc = scan_u64(c, c->side_eloff.p, c->side_eloff.p, nel + 1, stmp64))) return rc;  // (nel <= m: stmp64 is large enough)
  hipLaunchKernelGGL(k_side_rs_lines, grid(c, nruns + 1), B256, 0, c->stream, c->side_first.p, c->side_eloff.p, nruns,
                     c->side_off[MUSC_SIDE_READSTATS].p);
  HIPCHK(c, hipGetLastError());
  uint64_t rs_bytes = 0;
  HIPCHK(c, R.get(c->side_eloff.p + nel, &rs_bytes).wait());
  c->side_nel = nel;
  c->side_nrec[MUSC_SIDE_READSTATS] = nruns;
  c->side_nbytes[MUSC_SIDE_READSTATS] = rs_bytes;
  return 0;
}

int musc_side_prepare(musc_ctx* c, uint64_t* nrecords, uint64_t* nbytes) {
  if (!c) return 1;
  for (int w = 0; w < 3; w++) {
    if (nrecords) nrecords[w] = 0;
    if (nbytes) nbytes[w] = 0;
  }
  c->st.side_begins();
  switch (c->st.side_prepare_refusal(c->res_ttext != nullptr, c->side_form_ok, c->nreads)) {
    case musc_state::SIDE_OK: break;
    case musc_state::SIDE_NO_ORDER: return fail(c, 2, "musc_side_prepare: no ordered list (musc_results_order) of the reads, the database and the texts in hand");
    case musc_state::SIDE_PASS_AFTER: return fail(c, 2, "musc_side_prepare: a pass ran after the last musc_results_order: order its list first");
    case musc_state::SIDE_NO_READ_TEXT: return fail(c, 2, "musc_side_prepare: no read text (musc_results_set_read_text)");
    case musc_state::SIDE_FORM: return fail(c, MUSC_SIDE_ERR_FORM, "musc_side_prepare: gene text not in the simple form (gene %u is not name\\tlen without blanks)", c->side_bad_gene);
    case musc_state::SIDE_TOO_MANY_READS: return fail(c, 2, "musc_side_prepare: too many reads for 32-bit record numbers");
  }
  HIPCHK(c, hipSetDevice(c->device));
  const int rc = timed(c, &c->side_ms_prepare, [&] { return side_prepare_impl(c); });
  if (rc) return rc;
  c->side_ms_text = 0;
  c->st.side_made();
  for (int w = 0; w < 3; w++) {
    if (nrecords) nrecords[w] = c->side_nrec[w];
    if (nbytes) nbytes[w] = c->side_nbytes[w];
  }
  return 0;
}

static void launch_side(musc_ctx* c, int which, uint64_t r0, uint64_t r1, uint64_t bytes, unsigned char* out) {
  const dim3 blocks = stage_grid(c, bytes / 256 + 1, musc_launch::CAP_TILES);
  const SideData D = side_data(c);
  if (which == MUSC_SIDE_NONMATCH)
    hipLaunchKernelGGL(k_side_nm_render, blocks, dim3(256), 0, c->stream, c->side_idx[0].p, c->side_off[0].p, r0, r1, D, out, c->d_flag);
  else if (which == MUSC_SIDE_GENESTATS)
    hipLaunchKernelGGL(k_side_gs_render, blocks, dim3(256), 0, c->stream, c->side_idx[1].p, c->side_off[1].p, r0, r1, D, c->side_cnt.p, out,
                       c->d_flag);
  else
    hipLaunchKernelGGL(k_side_rs_render, blocks, dim3(256), 0, c->stream, c->side_el.p, c->side_nel, c->side_eloff.p, c->side_first.p,
                       (uint32_t)c->side_nrec[2], r0, r1, D, c->side_runread.p, out, c->d_flag);
}

int musc_side_text(musc_ctx* c, int which, uint64_t rec0, uint64_t nrec, char* dst, uint64_t capacity, int dst_on_device, uint64_t* nbytes) {
  if (!c) return 1;
  if (!nbytes) return fail(c, 2, "musc_side_text: nbytes is NULL");
  *nbytes = 0;
  if (which < 0 || which > 2) return fail(c, 2, "musc_side_text: no such text (%d)", which);
  if (!c->st.may_side_text()) return fail(c, 2, "musc_side_text: nothing prepared (musc_side_prepare)");
  const TextDesc t = {c->side_off[which].p, c->side_nrec[which], "musc_side_text", "a record no longer fits the reads or the texts in hand",
                      &c->side_ms_text};
  return text_range(c, t, rec0, nrec, dst, capacity, dst_on_device, nbytes,
                    [&](uint64_t r0, uint64_t r1, uint64_t bytes, unsigned char* out) { launch_side(c, which, r0, r1, bytes, out); });
}

int musc_side_last_ms(musc_ctx* c, float* ms_prepare, float* ms_text) {
  if (!c) return 1;
  if (ms_prepare) *ms_prepare = c->side_ms_prepare;
  if (ms_text) *ms_text = c->side_ms_text;
  return 0;
}

// ---------------------------------------------------------------- SAM output on the device
// One record per line of the ordered list of the last musc_results_order, and the header: musc_sam_prepare compares
// every span with its read and computes the offsets, musc_sam_text renders a range of records or of header slots
// (kernels_sam.hpp) through text_range.

static const int MUSC_SAM_ERR_REFUSED = 12;  // the database or the gene text does not allow SAM as asked: the caller's cue for its host path

static SamData sam_data(const musc_ctx* c) {
  SamData D;
  D.R = res_data(c);
  D.tok = c->sam_tok.p;
  D.gname = c->sam_gname.p;
  D.rank = c->res_rank;
  D.rev_pairs = c->sam_rev;
  return D;
}

// the refusals that need the device: the RNAME tokens of every gene, and under rev_pairs the lengths of every pair
// (into `gname`: SAM's table, or the coverage stage's own)
static int sam_names(musc_ctx* c, DevBuf<uint2>& gname, uint32_t rev_pairs, uint32_t* verdict) {
  int rc;
  if ((rc = ensure(c, gname, std::max<uint64_t>(c->nseq, 1)))) return rc;
  HIPCHK(c, hipMemsetAsync(c->d_flag, 0, 4, c->stream));
  if (c->nseq) {
    hipLaunchKernelGGL(k_sam_gnames, grid(c, c->nseq), dim3(256), 0, c->stream, c->res_gtext.get(), c->res_goff.get(), c->res_rank.get(),
                       c->seq_off.get(), c->nseq, rev_pairs, gname.p, c->d_flag.get());
    HIPCHK(c, hipGetLastError());
  }
  HIPCHK(c, Readback(c->scalars, c->stream).get(c->d_flag.get(), verdict).wait());
  return 0;
}

static int sam_prepare_impl(musc_ctx* c) {
  const dim3 B256(256);
  const uint64_t nreads = c->nreads, m = c->res_n, nh = (uint64_t)c->nseq + 2;
  const uint4* const hits = reinterpret_cast<const uint4*>(c->res_hits.p);
  static const char* const who = "musc_sam_prepare";
  int rc;
  TmpBufs B;
  Readback R(c->scalars, c->stream);
  if (c->res_ttext) {
    if ((rc = ensure(c, c->sam_tok, std::max<uint64_t>(nreads, 1)))) return rc;
    hipLaunchKernelGGL(k_sam_tokens, grid(c, nreads), B256, 0, c->stream, c->res_ttext.get(), c->res_toff.get(), nreads, c->sam_tok.p);
    HIPCHK(c, hipGetLastError());
  }
  if ((rc = ensure(c, c->sam_hoff, nh + 1)) || (rc = ensure(c, c->sam_off, m + 1)) || (rc = ensure(c, c->sam_info, std::max<uint64_t>(m, 1))))
    return rc;
  const SamData D = sam_data(c);
  uint32_t *first = nullptr, *last = nullptr;
  uint64_t* stmp64 = nullptr;
  if ((rc = tmp_alloc(c, who, B, &first, (nreads + 1) * 4)) || (rc = tmp_alloc(c, who, B, &last, (nreads + 1) * 4)) ||
      (rc = tmp_alloc(c, who, B, &stmp64, scan_tmp_elems(std::max(m, nh) + 1) * 8)))
    return rc;
  // ---- the header's slots
  hipLaunchKernelGGL(k_sam_hdr_len, grid(c, nh + 1), B256, 0, c->stream, D, c->sam_hoff.p);
  HIPCHK(c, hipGetLastError());
  if ((rc = scan_u64(c, c->sam_hoff.p, c->sam_hoff.p, nh + 1, stmp64))) return rc;
  // ---- the records: NH / HI from the runs of equal reads, NM and MD from the planes, then the offsets
  if (m) {
    hipLaunchKernelGGL(k_sam_runs, grid(c, m), B256, 0, c->stream, hits, m, first, last);
    HIPCHK(c, hipGetLastError());
  }
  hipLaunchKernelGGL(k_sam_count, grid(c, m + 1), B256, 0, c->stream, hits, m, D, first, last, c->sam_info.p, c->sam_off.p);
  HIPCHK(c, hipGetLastError());
  if ((rc = scan_u64(c, c->sam_off.p, c->sam_off.p, m + 1, stmp64))) return rc;
  uint64_t hbytes = 0, bytes = 0;
  HIPCHK(c, R.get(c->sam_hoff.p + nh, &hbytes).get(c->sam_off.p + m, &bytes).wait());
  c->sam_n = m;
  c->sam_bytes = bytes;
  c->sam_hbytes = hbytes;
  return 0;
}

int musc_sam_prepare(musc_ctx* c, int rev_pairs, uint64_t* nrecords, uint64_t* header_bytes, uint64_t* record_bytes) {
  if (!c) return 1;
  if (nrecords) *nrecords = 0;
  if (header_bytes) *header_bytes = 0;
  if (record_bytes) *record_bytes = 0;
  c->st.sam_begins();
  if (!c->st.ordered_current() || !c->db2 || !c->res_gtext || !c->res_rank)
    return fail(c, 2, "musc_sam_prepare: no ordered list (musc_results_order) of the reads, the database and the texts in hand");
  if (rev_pairs && (c->nseq & 1u))
    return fail(c, MUSC_SAM_ERR_REFUSED, "musc_sam_prepare: rev_pairs with an odd number of targets (%u)", c->nseq);
  HIPCHK(c, hipSetDevice(c->device));
  uint32_t verdict = 0;
  int rc = sam_names(c, c->sam_gname, rev_pairs ? 1u : 0u, &verdict);
  if (rc) return rc;
  if (verdict & 2u) return fail(c, MUSC_SAM_ERR_REFUSED, "musc_sam_prepare: rev_pairs, and the two targets of a pair differ in length");
  if (verdict & 1u)
    return fail(c, MUSC_SAM_ERR_REFUSED, "musc_sam_prepare: the gene text of a target with an id line%s has an empty first token",
                rev_pairs ? " (or of its even partner)" : "");
  c->sam_rev = rev_pairs ? 1u : 0u;
  rc = timed(c, &c->sam_ms_prepare, [&] { return sam_prepare_impl(c); });
  if (rc) return rc;
  c->sam_ms_text = 0;
  c->st.sam_made();
  if (nrecords) *nrecords = c->sam_n;
  if (header_bytes) *header_bytes = c->sam_hbytes;
  if (record_bytes) *record_bytes = c->sam_bytes;
  return 0;
}

static void launch_sam(musc_ctx* c, int which, uint64_t r0, uint64_t r1, uint64_t bytes, unsigned char* out) {
  const dim3 blocks = stage_grid(c, bytes / 256 + 1, musc_launch::CAP_TILES);
  const SamData D = sam_data(c);
  if (which == 0)
    hipLaunchKernelGGL(k_sam_hdr_render, blocks, dim3(256), 0, c->stream, c->sam_hoff.p, r0, r1, D, out, c->d_flag.get());
  else
    hipLaunchKernelGGL(k_sam_render, blocks, dim3(256), 0, c->stream, reinterpret_cast<const uint4*>(c->res_hits.p), c->sam_info.p,
                       c->sam_off.p, r0, r1, D, out, c->d_flag.get());
}

int musc_sam_text(musc_ctx* c, int which, uint64_t rec0, uint64_t nrec, char* dst, uint64_t capacity, int dst_on_device, uint64_t* nbytes) {
  if (!c) return 1;
  if (!nbytes) return fail(c, 2, "musc_sam_text: nbytes is NULL");
  *nbytes = 0;
  if (which < 0 || which > 1) return fail(c, 2, "musc_sam_text: no such text (%d)", which);
  if (!c->st.may_sam_text()) return fail(c, 2, "musc_sam_text: nothing prepared (musc_sam_prepare)");
  const TextDesc t = {which ? c->sam_off.p : c->sam_hoff.p, which ? c->sam_n : (uint64_t)c->nseq + 2, "musc_sam_text",
                      "a record no longer fits the reads, the database or the texts in hand", &c->sam_ms_text};
  return text_range(c, t, rec0, nrec, dst, capacity, dst_on_device, nbytes,
                    [&](uint64_t r0, uint64_t r1, uint64_t bytes, unsigned char* out) { launch_sam(c, which, r0, r1, bytes, out); });
}

int musc_sam_last_ms(musc_ctx* c, float* ms_prepare, float* ms_text) {
  if (!c) return 1;
  if (ms_prepare) *ms_prepare = c->sam_ms_prepare;
  if (ms_text) *ms_text = c->sam_ms_text;
  return 0;
}
