// muscato_db_text.hpp -- the gene file from its raw bytes to the resident database: musc_sz_decode and
// musc_db_load_text.  Included at the end of muscato_hip.hip (one translation unit: musc_ctx, db_alloc / db_finish, the
// scans and the FASTQ stage's loads are defined there).
//
// Reference: cmd/muscato_prep_targets/main.go:246-258 writes the gene file through snappy's framed writer;
// cmd/muscato_screen/main.go:408-452 reads it back line by line, the target being the line up to its first tab.  On the
// host this is slurp -> sz_decode -> split_lines -> substr -> concat -> musc_db_load_ascii (host/muscato_host.hpp).

#include "sz_plan.hpp"
#include "kernels_sz.hpp"
#include "kernels_db_text.hpp"

// a failed device allocation: the library's code for a failed HIP call, the text says which and why ("out of memory")
#define DBT_ALLOC(c, who, B, ptr, bytes)                                                                             \
  do {                                                                                                               \
    const hipError_t e_ = (B).alloc((ptr), (bytes));                                                                 \
    if (e_ != hipSuccess) {                                                                                          \
      (void)hipGetLastError();                                                                                       \
      return fail((c), 10, "%s: device allocation of %llu bytes failed: %s", (who), (unsigned long long)(bytes),     \
                  hipGetErrorString(e_));                                                                            \
    }                                                                                                                \
  } while (0)

static int sz_plan_or_fail(musc_ctx* c, const char* who, const uint8_t* bytes, uint64_t nbytes, musc_sz::Plan& plan) {
  const int rc = musc_sz::sz_plan(bytes, nbytes, plan);
  if (rc) return fail(c, rc, "%s: chunk %llu: %s", who, (unsigned long long)plan.bad_index, plan.msg.c_str());
  return 0;
}

// The planned chunks of the host stream `bytes`, decoded to the device memory d_dst (plan.n_out bytes).  Queued on the
// context's stream and waited for: 13 names the first chunk in stream order whose block or checksum is bad.
static int sz_decode_run(musc_ctx* c, const char* who, const musc_sz::Plan& plan, const uint8_t* bytes, uint64_t nbytes,
                         unsigned char* d_dst, TmpBufs& B) {
  const uint64_t nch = plan.chunks.size();
  if (nch == 0) return 0;
  if (nch >= 0xFFFFFFF0ull) return fail(c, 2, "%s: too many chunks", who);
  static const musc_sz::X2n x2n;  // (built once)
  std::vector<SzChunkDev> tab(nch);
  for (uint64_t i = 0; i < nch; i++) {
    const musc_sz::Chunk& k = plan.chunks[i];
    tab[i] = SzChunkDev{k.body, k.out_off, k.body_len, k.ulen, k.crc, k.type};
  }
  unsigned char* d_stream = nullptr;
  SzChunkDev* d_tab = nullptr;
  uint32_t *d_status = nullptr, *d_x2n = nullptr;
  DBT_ALLOC(c, who, B, &d_stream, nbytes + 16);
  DBT_ALLOC(c, who, B, &d_tab, nch * sizeof(SzChunkDev));
  DBT_ALLOC(c, who, B, &d_status, nch * 4);
  DBT_ALLOC(c, who, B, &d_x2n, sizeof x2n.t);
  HIPCHK(c, hipMemcpyAsync(d_stream, bytes, nbytes, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_tab, tab.data(), nch * sizeof(SzChunkDev), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_x2n, x2n.t, sizeof x2n.t, hipMemcpyHostToDevice, c->stream));
  const uint64_t slo = (uint64_t)((uintptr_t)d_stream & 15u);
  hipLaunchKernelGGL(k_sz_decode, dim3((unsigned)std::min<uint64_t>(nch, 8 * MAX_GRID)), dim3(SZ_BLOCK), 0, c->stream,
                     d_stream - slo, slo, d_tab, (uint32_t)nch, d_x2n, d_dst, d_status);
  HIPCHK(c, hipGetLastError());
  std::vector<uint32_t> status(nch);
  HIPCHK(c, hipMemcpyAsync(status.data(), d_status, nch * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (uint64_t i = 0; i < nch; i++)
    if (status[i])
      return fail(c, musc_sz::SZ_BAD, "%s: chunk %llu: %s", who, (unsigned long long)plan.chunks[i].index,
                  musc_sz::status_text(status[i]));
  return 0;
}

extern "C" int musc_sz_decode(musc_ctx* c, const uint8_t* bytes, uint64_t nbytes, uint8_t* dst, uint64_t capacity,
                              int dst_on_device, uint64_t* nout) {
  static const char* const who = "musc_sz_decode";
  if (!c) return 1;
  if (!nout) return fail(c, 2, "%s: NULL output pointer", who);
  *nout = 0;
  if (!bytes && nbytes) return fail(c, 2, "%s: NULL input", who);
  HIPCHK(c, hipSetDevice(c->device));
  musc_sz::Plan plan;
  int rc = sz_plan_or_fail(c, who, bytes, nbytes, plan);
  if (rc) return rc;
  *nout = plan.n_out;
  if (!dst) return 0;  // sizing
  if (capacity < plan.n_out)
    return fail(c, 2, "%s: capacity %llu below the %llu decoded bytes", who, (unsigned long long)capacity, (unsigned long long)plan.n_out);
  // decoded beside dst and copied when every chunk has passed: a failed call leaves dst as it was
  TmpBufs B;
  unsigned char* d_out = nullptr;
  DBT_ALLOC(c, who, B, &d_out, plan.n_out + 16);
  if ((rc = sz_decode_run(c, who, plan, bytes, nbytes, d_out, B))) return rc;
  if (plan.n_out) {
    HIPCHK(c, hipMemcpyAsync(dst, d_out, plan.n_out, dst_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return 0;
}

static int db_load_text_run(musc_ctx* c, const uint8_t* bytes, uint64_t nbytes, int on_device, int framed, musc_db_text_info* out) {
  static const char* const who = "musc_db_load_text";
  static const unsigned char magic[10] = {0xff, 0x06, 0x00, 0x00, 's', 'N', 'a', 'P', 'p', 'Y'};
  if (framed < 0) {  // as read_maybe_sz: a framed stream says so itself
    unsigned char head[sizeof magic] = {};
    framed = 0;
    if (nbytes >= sizeof magic) {
      if (on_device) HIPCHK(c, hipMemcpy(head, bytes, sizeof magic, hipMemcpyDeviceToHost));
      else memcpy(head, bytes, sizeof magic);
      framed = memcmp(head, magic, sizeof magic) == 0;
    }
  }
  if (framed && on_device) return fail(c, 2, "%s: a framed stream must be in host memory", who);
  c->ev_used = 0;
  hipEvent_t e0 = pool_event(c), e1 = pool_event(c), e2 = pool_event(c);
  if (!e0 || !e1 || !e2) return fail(c, 10, "hipEventCreate failed");
  TmpBufs B;  // the stream, the text and the line tables: all released when the planes stand

  // ---- frames -> text
  const unsigned char* d_text = bytes;
  uint64_t ntext = nbytes, nchunks = 0;
  if (framed) {
    musc_sz::Plan plan;
    int rc = sz_plan_or_fail(c, who, bytes, nbytes, plan);
    if (rc) return rc;
    unsigned char* dt = nullptr;
    DBT_ALLOC(c, who, B, &dt, plan.n_out + 16);
    HIPCHK(c, hipEventRecord(e0, c->stream));
    if ((rc = sz_decode_run(c, who, plan, bytes, nbytes, dt, B))) return rc;
    d_text = dt;
    ntext = plan.n_out;
    nchunks = plan.chunks.size();
  } else {
    HIPCHK(c, hipEventRecord(e0, c->stream));
    if (!on_device && nbytes) {
      unsigned char* dt = nullptr;
      DBT_ALLOC(c, who, B, &dt, nbytes + 16);
      HIPCHK(c, hipMemcpyAsync(dt, bytes, nbytes, hipMemcpyHostToDevice, c->stream));
      d_text = dt;
    }
  }
  HIPCHK(c, hipEventRecord(e1, c->stream));
  if (ntext == 0) return fail(c, 2, "database has no sequences");

  // ---- lines: newlines per tile, tile bases
  const uint64_t lo = (uint64_t)((uintptr_t)d_text & (FQ_LANE_BYTES - 1)), hi = lo + ntext;
  const unsigned char* base16 = d_text - lo;
  const uint64_t ntiles = (hi + FQ_TILE_BYTES - 1) / FQ_TILE_BYTES;
  const dim3 tgrid((unsigned)std::min<uint64_t>(ntiles, 4 * MAX_GRID));
  uint64_t *cnt = nullptr, *stmp = nullptr;
  DBT_ALLOC(c, who, B, &cnt, (ntiles + 1) * 8);
  DBT_ALLOC(c, who, B, &stmp, scan_tmp_elems(ntiles + 1) * 8);
  HIPCHK(c, hipMemsetAsync(cnt + ntiles, 0, 8, c->stream));
  hipLaunchKernelGGL(k_fq_count, tgrid, dim3(FQ_BLOCK), 0, c->stream, base16, lo, hi, ntiles, cnt);
  HIPCHK(c, hipGetLastError());
  int rc = scan_u64(c, cnt, cnt, ntiles + 1, stmp);
  if (rc) return rc;
  c->h_pinned[1] = 0;
  HIPCHK(c, hipMemcpyAsync(c->h_pinned, cnt + ntiles, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->h_pinned + 1, d_text + (ntext - 1), 1, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const uint64_t newlines = c->h_pinned[0];
  const uint32_t virt = *reinterpret_cast<const unsigned char*>(c->h_pinned + 1) != '\n';  // a last line without a newline is a line
  const uint64_t nlines = newlines + virt;
  if (nlines >= 0xFFFFFFF0ull) return fail(c, 2, "%s: too many targets for 32-bit target numbers", who);

  // ---- spans, lengths, seq_off
  uint64_t *begin = nullptr, *len = nullptr, *stmp2 = nullptr;
  unsigned long long *end = nullptr, *census = nullptr;
  DBT_ALLOC(c, who, B, &begin, nlines * 8);
  DBT_ALLOC(c, who, B, &end, nlines * 8);
  DBT_ALLOC(c, who, B, &len, (nlines + 1) * 8);
  DBT_ALLOC(c, who, B, &stmp2, scan_tmp_elems(nlines + 1) * 8);
  DBT_ALLOC(c, who, B, &census, 16);
  HIPCHK(c, hipMemsetAsync(end, 0xFF, nlines * 8, c->stream));
  hipLaunchKernelGGL(k_dbt_lines, tgrid, dim3(FQ_BLOCK), 0, c->stream, base16, lo, hi, ntiles, cnt, nlines, virt, begin, end);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_dbt_lengths, dim3(std::min(nblk(nlines + 1, 256), MAX_GRID)), dim3(256), 0, c->stream, d_text, ntext, nlines,
                     begin, end, len);
  HIPCHK(c, hipGetLastError());
  if ((rc = scan_u64(c, len, len, nlines + 1, stmp2))) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));  // (db_alloc reads the offsets with copies that do not wait for the stream)

  // ---- the planes
  if ((rc = db_alloc(c, len, (uint32_t)nlines, 1))) return rc;
  HIPCHK(c, hipMemsetAsync(census, 0, 8, c->stream));
  HIPCHK(c, hipMemsetAsync(census + 1, 0xFF, 8, c->stream));
  if (c->db_words) {
    hipLaunchKernelGGL(k_pack_db_spans, dim3(nblk(c->db_words, 256)), dim3(256), 0, c->stream, d_text, ntext, begin, c->seq_off.get(),
                       nlines, c->nbases, c->db2.get(), c->dbm2.get(), c->db_words, c->d_flag.get(), census);
    HIPCHK(c, hipGetLastError());
  }
  HIPCHK(c, hipEventRecord(e2, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->h_pinned + 2, census, 16, hipMemcpyDeviceToHost, c->stream));
  if ((rc = db_finish(c))) return rc;  // (waits for the stream)
  if (out) {
    out->n_targets = nlines;
    out->n_bases = c->nbases;
    out->n_odd = c->h_pinned[2];
    out->first_odd_target = out->n_odd ? (uint32_t)c->h_pinned[3] : 0;
    out->n_text_bytes = ntext;
    out->n_chunks = nchunks;
    (void)hipEventElapsedTime(&out->ms_decode, e0, e1);
    (void)hipEventElapsedTime(&out->ms_parse, e1, e2);
  }
  return 0;
}

extern "C" int musc_db_load_text(musc_ctx* c, const uint8_t* bytes, uint64_t nbytes, int on_device, int framed,
                                 musc_db_text_info* out) {
  if (!c) return 1;
  if (out) memset(out, 0, sizeof *out);
  HIPCHK(c, hipSetDevice(c->device));
  free_db(c);
  if (!bytes && nbytes) return fail(c, 2, "musc_db_load_text: NULL input");
  if (framed < -1 || framed > 1) return fail(c, 2, "musc_db_load_text: framed = %d is none of -1, 0, 1", framed);
  const int rc = db_load_text_run(c, bytes, nbytes, on_device, framed, out);
  if (rc) {  // a failed call leaves no database (the message stays the context's last error)
    (void)hipStreamSynchronize(c->stream);
    free_db(c);
    if (out) memset(out, 0, sizeof *out);
  }
  return rc;
}
