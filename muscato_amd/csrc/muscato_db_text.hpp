// muscato_db_text.hpp -- the gene file from its raw bytes to the resident database: musc_sz_decode and
// musc_db_load_text.  Included by muscato_hip.hip behind muscato_load.hpp and muscato_prep.hpp (one translation unit:
// musc_ctx, the scans, grid, staged, tmp_alloc and Readback; db_alloc / db_finish / db_load_done and text_lines are
// muscato_load.hpp's).
//
// Reference: cmd/muscato_prep_targets/main.go:246-258 writes the gene file through snappy's framed writer;
// cmd/muscato_screen/main.go:408-452 reads it back line by line, the target being the line up to its first tab.  On the
// host this is slurp -> sz_decode -> split_lines -> substr -> concat -> musc_db_load_ascii (host/muscato_host.hpp).

#include "sz_plan.hpp"
#include "kernels_sz.hpp"
#include "kernels_db_text.hpp"

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
  int rc = 0;
  if ((rc = tmp_alloc(c, who, B, &d_stream, nbytes + 16)) || (rc = tmp_alloc(c, who, B, &d_tab, nch * sizeof(SzChunkDev))) ||
      (rc = tmp_alloc(c, who, B, &d_status, nch * 4)) || (rc = tmp_alloc(c, who, B, &d_x2n, sizeof x2n.t)))
    return rc;
  HIPCHK(c, hipMemcpyAsync(d_stream, bytes, nbytes, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_tab, tab.data(), nch * sizeof(SzChunkDev), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_x2n, x2n.t, sizeof x2n.t, hipMemcpyHostToDevice, c->stream));
  const uint64_t slo = (uint64_t)((uintptr_t)d_stream & 15u);
  hipLaunchKernelGGL(k_sz_decode, stage_grid(c, nch, musc_launch::CAP_CHUNKS), dim3(SZ_BLOCK), 0, c->stream,
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
  if ((rc = tmp_alloc(c, who, B, &d_out, plan.n_out + 16))) return rc;
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
  Marks m;  // 0 .. 1: frames -> text (or the upload), 1 .. 2: text -> planes
  int rc = m.start(c);
  if (rc) return rc;
  TmpBufs B;  // the stream, the text and the line tables: all released when the planes stand

  // ---- frames -> text
  const unsigned char* d_text = nullptr;
  uint64_t ntext = nbytes, nchunks = 0;
  if (framed) {
    musc_sz::Plan plan;
    unsigned char* dt = nullptr;
    if ((rc = sz_plan_or_fail(c, who, bytes, nbytes, plan)) || (rc = tmp_alloc(c, who, B, &dt, plan.n_out + 16))) return rc;
    HIPCHK(c, m.mark(c, 0));
    if ((rc = sz_decode_run(c, who, plan, bytes, nbytes, dt, B))) return rc;
    d_text = dt;
    ntext = plan.n_out;
    nchunks = plan.chunks.size();
  } else {
    HIPCHK(c, m.mark(c, 0));
    // (16 spare bytes: the text's last 16-byte lane lies inside the block; fq_load16 reads no byte past the text itself)
    if ((rc = staged(c, who, B, bytes, nbytes, on_device, 16, &d_text))) return rc;
  }
  HIPCHK(c, m.mark(c, 1));
  if (ntext == 0) return fail(c, 2, "database has no sequences");

  // ---- lines: newlines per tile, tile bases
  TextLines L;
  if ((rc = text_lines(c, who, B, d_text, ntext, &L))) return rc;
  const uint64_t nlines = L.newlines + L.virt;
  if (nlines >= 0xFFFFFFF0ull) return fail(c, 2, "%s: too many targets for 32-bit target numbers", who);

  // ---- spans, lengths, seq_off
  uint64_t *begin = nullptr, *len = nullptr, *stmp2 = nullptr;
  unsigned long long *end = nullptr, *census = nullptr;
  if ((rc = tmp_alloc(c, who, B, &begin, nlines * 8)) || (rc = tmp_alloc(c, who, B, &end, nlines * 8)) ||
      (rc = tmp_alloc(c, who, B, &len, (nlines + 1) * 8)) || (rc = tmp_alloc(c, who, B, &stmp2, scan_tmp_elems(nlines + 1) * 8)) ||
      (rc = tmp_alloc(c, who, B, &census, 16)))
    return rc;
  HIPCHK(c, hipMemsetAsync(end, 0xFF, nlines * 8, c->stream));
  hipLaunchKernelGGL(k_dbt_lines, L.tgrid, dim3(FQ_BLOCK), 0, c->stream, L.base16, L.lo, L.hi, L.ntiles, L.cnt, nlines, L.virt, begin, end);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_dbt_lengths, grid(c, nlines + 1), dim3(256), 0, c->stream, d_text, ntext, nlines,
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
  HIPCHK(c, m.mark(c, 2));
  uint64_t odd[2] = {0, 0};  // how many targets hold an odd byte, the first of them
  Readback R(c->scalars, c->stream);
  if ((rc = db_finish(c, R.get_words(census, odd, 2)))) return rc;  // (waits for the stream)
  if (out) {
    out->n_targets = nlines;
    out->n_bases = c->nbases;
    out->n_odd = odd[0];
    out->first_odd_target = out->n_odd ? (uint32_t)odd[1] : 0;
    out->n_text_bytes = ntext;
    out->n_chunks = nchunks;
    out->ms_decode = m.ms(0, 1);
    out->ms_parse = m.ms(1, 2);
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
  const int rc = db_load_done(c, db_load_text_run(c, bytes, nbytes, on_device, framed, out));
  if (rc && out) memset(out, 0, sizeof *out);
  return rc;
}
