// muscato_targets_prep.hpp -- target preparation from the raw bytes of a FASTA or id<TAB>sequence file to the two
// prepared texts, resident in the context, and the framed writer: musc_targets_prep,
// musc_targets_prep_text, musc_targets_prep_load, musc_targets_prep_free and musc_sz_frame.  Included by
// muscato_hip.hip behind muscato_db_text.hpp (one translation unit: musc_ctx, the scans, staged, tmp_alloc and Readback,
// text_lines of muscato_load.hpp, db_load_text_run of muscato_db_text.hpp).  The arithmetic is targets_prep_plan.hpp's.
//
// Reference: cmd/muscato_prep_targets/main.go:82-141 (processText), :143-213 (processFasta), :48-80 (revcomp, subx),
// :246-258 (both texts through snappy's framed writer).  On the host this is prep_targets_text / prep_targets_fasta
// and sz_encode (host/muscato_host.hpp, host/sz.hpp), which stay the specification and the fallback.

#include "targets_prep_plan.hpp"
#include "kernels_targets_prep.hpp"

static void tp_free(musc_ctx* c) {
  for (int w = 0; w < 2; w++) {
    c->tp_text[w].release();
    c->tp_bytes[w] = 0;
  }
  c->tp_have = false;
}

// an owning buffer of a prepared text: whole dwords, so that the kernels' last aligned store lies inside it
static int tp_out_alloc(musc_ctx* c, const char* who, DevPtr<unsigned char>& buf, uint64_t nbytes) {
  const uint64_t bytes = ((nbytes + 3) & ~3ull) + 16;
  const hipError_t e = buf.alloc(bytes);
  if (e == hipSuccess) return 0;
  (void)hipGetLastError();
  return fail(c, 10, "%s: device allocation of %llu bytes failed: %s", who, (unsigned long long)bytes, hipGetErrorString(e));
}

static int targets_prep_run(musc_ctx* c, const uint8_t* bytes, uint64_t nbytes, int on_device, int fasta, int rev,
                            musc_targets_prep_info* out) {
  static const char* const who = "musc_targets_prep";
  musc_targets_prep_info info;
  memset(&info, 0, sizeof info);
  info.stop_line = ~0ull;
  if (nbytes == 0) {  // two empty texts
    c->tp_have = true;
    if (out) *out = info;
    return 0;
  }
  Marks m;
  int rc = m.start(c);
  if (rc) return rc;
  HIPCHK(c, m.mark(c, 0));
  Readback R(c->scalars, c->stream);
  TmpBufs B, B2;  // the text and the line tables; the record tables
  const unsigned char* d_text = nullptr;
  // (16 spare bytes: the text's last 16-byte lane lies inside the block; fq_load16 reads no byte past the text itself)
  if ((rc = staged(c, who, B, bytes, nbytes, on_device, 16, &d_text))) return rc;
  TextLines L;
  if ((rc = text_lines(c, who, B, d_text, nbytes, &L))) return rc;
  const uint64_t nlines = L.newlines + L.virt;
  info.n_lines = nlines;

  // ---- lines
  uint64_t *begin = nullptr, *eol = nullptr, *stmp = nullptr;
  unsigned long long* st = nullptr;
  if ((rc = tmp_alloc(c, who, B, &begin, nlines * 8)) || (rc = tmp_alloc(c, who, B, &eol, nlines * 8)) ||
      (rc = tmp_alloc(c, who, B, &stmp, scan_tmp_elems(nlines + 2) * 8)) || (rc = tmp_alloc(c, who, B, &st, TP_ST_WORDS * 8)))
    return rc;
  HIPCHK(c, hipMemsetAsync(st, 0xFF, TP_ST_WORDS * 8, c->stream));
  HIPCHK(c, hipMemsetAsync(st + TP_ST_SUBX, 0, 8, c->stream));
  HIPCHK(c, hipMemsetAsync(st + TP_ST_KEPT0, 0, 8, c->stream));

  // ---- records: nrec of them, fo = their nrec + 1 offsets (the scan of len + 1), where each one's bytes and name are
  uint64_t nrec = 0;
  uint64_t *fo = nullptr, *src0 = nullptr, *name_b = nullptr, *name_len = nullptr, *S = nullptr;
  if (!fasta) {
    unsigned long long *ftab = nullptr, *ltab = nullptr;
    uint64_t* a = nullptr;
    if ((rc = tmp_alloc(c, who, B, &ftab, nlines * 8)) || (rc = tmp_alloc(c, who, B, &ltab, nlines * 8)) ||
        (rc = tmp_alloc(c, who, B, &a, (nlines + 1) * 8)))
      return rc;
    HIPCHK(c, hipMemsetAsync(ftab, 0xFF, nlines * 8, c->stream));
    HIPCHK(c, hipMemsetAsync(ltab, 0, nlines * 8, c->stream));
    hipLaunchKernelGGL(k_tp_lines, L.tgrid, dim3(FQ_BLOCK), 0, c->stream, L.base16, L.lo, L.hi, L.ntiles, L.cnt, nlines, L.virt, begin, eol, ftab, ltab);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(k_tp_classify<false>, grid(c, nlines + 1), dim3(256), 0, c->stream, d_text, nbytes, nlines, begin, eol, ftab, ltab,
                       (uint64_t*)nullptr, (uint64_t*)nullptr, st);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, R.get(st + TP_ST_STOP, &info.stop_line).wait());
    nrec = std::min<uint64_t>(info.stop_line, nlines);  // the records are the lines in front of the first stop line
    if (musc_tp::refused(nrec, rev)) return fail(c, 12, "%s: %llu targets do not fit 32-bit target numbers", who, (unsigned long long)musc_tp::n_targets(nrec, rev));
    hipLaunchKernelGGL(k_tp_text_recs, grid(c, nrec + 1), dim3(256), 0, c->stream, nrec, begin, eol, ftab, ltab, a);
    HIPCHK(c, hipGetLastError());
    if ((rc = scan_u64(c, a, a, nrec + 1, stmp))) return rc;
    fo = a;
    src0 = reinterpret_cast<uint64_t*>(ltab);
    name_b = begin;
    name_len = reinterpret_cast<uint64_t*>(ftab);
  } else {
    uint64_t *hdr = nullptr, *bases = nullptr;
    if ((rc = tmp_alloc(c, who, B, &hdr, (nlines + 1) * 8)) || (rc = tmp_alloc(c, who, B, &bases, (nlines + 1) * 8))) return rc;
    hipLaunchKernelGGL(k_tp_lines, L.tgrid, dim3(FQ_BLOCK), 0, c->stream, L.base16, L.lo, L.hi, L.ntiles, L.cnt, nlines, L.virt, begin, eol,
                       (unsigned long long*)nullptr, (unsigned long long*)nullptr);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(k_tp_classify<true>, grid(c, nlines + 1), dim3(256), 0, c->stream, d_text, nbytes, nlines, begin, eol,
                       (const unsigned long long*)nullptr, (const unsigned long long*)nullptr, hdr, bases, st);
    HIPCHK(c, hipGetLastError());
    if ((rc = scan_u64(c, hdr, hdr, nlines + 1, stmp)) || (rc = scan_u64(c, bases, bases, nlines + 1, stmp))) return rc;
    S = bases;
    uint64_t empty_line = 0, nhdr = 0;
    HIPCHK(c, R.get(st + TP_ST_EMPTY, &empty_line).get(hdr + nlines, &nhdr).wait());
    if (empty_line != ~0ull) return fail(c, 14, "%s: empty line in FASTA input (line %llu)", who, (unsigned long long)empty_line);
    const uint64_t ngroups = nhdr + 1;  // group 0: the lines in front of the first header
    uint64_t *hl = nullptr, *kept = nullptr, *a = nullptr;
    if ((rc = tmp_alloc(c, who, B2, &hl, (ngroups + 1) * 8)) || (rc = tmp_alloc(c, who, B2, &kept, (ngroups + 1) * 8)) ||
        (rc = tmp_alloc(c, who, B2, &a, (ngroups + 1) * 8)) || (rc = tmp_alloc(c, who, B2, &fo, (ngroups + 1) * 8)) ||
        (rc = tmp_alloc(c, who, B2, &src0, ngroups * 8)) || (rc = tmp_alloc(c, who, B2, &name_b, ngroups * 8)) ||
        (rc = tmp_alloc(c, who, B2, &name_len, ngroups * 8)))
      return rc;
    hipLaunchKernelGGL(k_tp_hl, grid(c, nlines), dim3(256), 0, c->stream, nlines, hdr, ngroups, hl);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(k_tp_groups, grid(c, ngroups + 1), dim3(256), 0, c->stream, ngroups, hl, S, kept, a);
    HIPCHK(c, hipGetLastError());
    if ((rc = scan_u64(c, kept, kept, ngroups + 1, stmp)) || (rc = scan_u64(c, a, a, ngroups + 1, stmp))) return rc;
    hipLaunchKernelGGL(k_tp_compact, grid(c, ngroups + 1), dim3(256), 0, c->stream, ngroups, kept, a, hl, S, begin, eol, fo, src0, name_b,
                       name_len, st);
    HIPCHK(c, hipGetLastError());
    uint64_t kept0 = 0;
    HIPCHK(c, R.get(kept + ngroups, &nrec).get(st + TP_ST_KEPT0, &kept0).wait());
    info.n_dropped = nhdr - (nrec - kept0);  // headers whose record has no bases
    if (musc_tp::refused(nrec, rev)) return fail(c, 12, "%s: %llu targets do not fit 32-bit target numbers", who, (unsigned long long)musc_tp::n_targets(nrec, rev));
  }

  // ---- the id lines' lengths and offsets; the sizes of both texts
  uint64_t* ioff = nullptr;
  if ((rc = tmp_alloc(c, who, B2, &ioff, (nrec + 1) * 8))) return rc;
  hipLaunchKernelGGL(k_tp_idlen, grid(c, nrec + 1), dim3(256), 0, c->stream, nrec, fo, name_len, rev, ioff);
  HIPCHK(c, hipGetLastError());
  if ((rc = scan_u64(c, ioff, ioff, nrec + 1, stmp))) return rc;
  uint64_t fwd_bytes = 0, nid_bytes = 0;
  HIPCHK(c, R.get(fo + nrec, &fwd_bytes).get(ioff + nrec, &nid_bytes).wait());
  const uint64_t mult = rev ? 2 : 1;
  const uint64_t nseq_bytes = musc_tp::seq_fwd_off(fwd_bytes, rev);

  // ---- both texts
  DevPtr<unsigned char> seq, ids;
  if ((rc = tp_out_alloc(c, who, seq, nseq_bytes)) || (rc = tp_out_alloc(c, who, ids, nid_bytes))) return rc;
  if (nseq_bytes) {
    const dim3 g = grid(c, (nseq_bytes + 3) / 4);
    if (fasta)
      hipLaunchKernelGGL(k_tp_seq<true>, g, dim3(256), 0, c->stream, d_text, nbytes, nrec, fo, src0, S, begin, nlines, mult, nseq_bytes, seq.get(), st);
    else
      hipLaunchKernelGGL(k_tp_seq<false>, g, dim3(256), 0, c->stream, d_text, nbytes, nrec, fo, src0, S, begin, nlines, mult, nseq_bytes, seq.get(), st);
    HIPCHK(c, hipGetLastError());
    if (rev) {
      hipLaunchKernelGGL(k_tp_rev, g, dim3(256), 0, c->stream, nrec, fo, nseq_bytes, seq.get());
      HIPCHK(c, hipGetLastError());
    }
  }
  if (nid_bytes) {
    hipLaunchKernelGGL(k_tp_ids, grid(c, (nid_bytes + 3) / 4), dim3(256), 0, c->stream, d_text, nbytes, nrec, fo, ioff, name_b, name_len, rev,
                       nid_bytes, ids.get());
    HIPCHK(c, hipGetLastError());
  }
  HIPCHK(c, m.mark(c, 1));
  HIPCHK(c, R.get(st + TP_ST_SUBX, &info.n_subx).wait());
  info.n_records = nrec;
  info.n_targets = musc_tp::n_targets(nrec, rev);
  info.n_seq_bytes = nseq_bytes;
  info.n_id_bytes = nid_bytes;
  info.ms = m.ms(0, 1);
  c->tp_text[0] = std::move(seq);
  c->tp_text[1] = std::move(ids);
  c->tp_bytes[0] = nseq_bytes;
  c->tp_bytes[1] = nid_bytes;
  c->tp_have = true;
  if (out) *out = info;
  return 0;
}

extern "C" int musc_targets_prep(musc_ctx* c, const uint8_t* bytes, uint64_t nbytes, int on_device, int fasta, int rev,
                                 musc_targets_prep_info* out) {
  if (!c) return 1;
  if (out) memset(out, 0, sizeof *out);
  HIPCHK(c, hipSetDevice(c->device));
  tp_free(c);  // a failed call leaves no prepared texts, those of an earlier call included
  if (!bytes && nbytes) return fail(c, 2, "musc_targets_prep: NULL input");
  if (fasta < 0 || fasta > 1 || rev < 0 || rev > 1) return fail(c, 2, "musc_targets_prep: fasta = %d, rev = %d: both must be 0 or 1", fasta, rev);
  const int rc = targets_prep_run(c, bytes, nbytes, on_device, fasta, rev, out);
  if (rc) {
    (void)hipStreamSynchronize(c->stream);  // (kernels of the call may still be queued on its temporaries)
    tp_free(c);
    if (out) memset(out, 0, sizeof *out);
  }
  return rc;
}

extern "C" int musc_targets_prep_text(musc_ctx* c, int which, uint64_t off, uint64_t nbytes, uint8_t* dst, int dst_on_device) {
  static const char* const who = "musc_targets_prep_text";
  if (!c) return 1;
  if (which < 0 || which > 1) return fail(c, 2, "%s: which = %d is neither 0 (sequences) nor 1 (ids)", who, which);
  if (!c->tp_have) return fail(c, 2, "%s: no prepared text (musc_targets_prep first)", who);
  if (off > c->tp_bytes[which] || nbytes > c->tp_bytes[which] - off)
    return fail(c, 2, "%s: bytes [%llu, %llu + %llu) beyond the text's %llu", who, (unsigned long long)off, (unsigned long long)off,
                (unsigned long long)nbytes, (unsigned long long)c->tp_bytes[which]);
  if (nbytes == 0) return 0;
  if (!dst) return fail(c, 2, "%s: NULL output pointer", who);
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(dst, c->tp_text[which].get() + off, nbytes, dst_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int musc_targets_prep_load(musc_ctx* c, musc_db_text_info* out) {
  if (!c) return 1;
  if (out) memset(out, 0, sizeof *out);
  if (!c->tp_have) return fail(c, 2, "musc_targets_prep_load: no prepared text (musc_targets_prep first)");
  HIPCHK(c, hipSetDevice(c->device));
  free_db(c);
  // the resident sequence text is the gene file's text: one target per line (a line without a tab is its own target)
  const int rc = db_load_done(c, db_load_text_run(c, c->tp_text[0].get(), c->tp_bytes[0], 1, 0, out));
  if (rc && out) memset(out, 0, sizeof *out);
  return rc;
}

extern "C" int musc_targets_prep_free(musc_ctx* c) {
  if (!c) return 1;
  HIPCHK(c, hipSetDevice(c->device));
  tp_free(c);
  return 0;
}

// musc_sz_frame, and musc_targets_prep_sz (muscato_sz_compress.hpp) on a resident text
static int sz_frame_call(musc_ctx* c, const char* who, const uint8_t* bytes, uint64_t nbytes, int on_device, uint8_t* dst, uint64_t capacity,
                         int dst_on_device, uint64_t* nout) {
  if (!nout) return fail(c, 2, "%s: NULL output pointer", who);
  *nout = 0;
  if (!bytes && nbytes) return fail(c, 2, "%s: NULL input", who);
  const uint64_t size = musc_tp::sz_frame_size(nbytes), nch = musc_tp::sz_chunks(nbytes);
  *nout = size;
  if (!dst) return 0;  // sizing
  if (capacity < size)
    return fail(c, 2, "%s: capacity %llu below the %llu bytes of the stream", who, (unsigned long long)capacity, (unsigned long long)size);
  HIPCHK(c, hipSetDevice(c->device));
  static const musc_sz::X2n x2n;  // (built once)
  TmpBufs B;
  const unsigned char* d_src = nullptr;
  unsigned char* d_out = dst;
  uint32_t* d_x2n = nullptr;
  int rc = 0;
  // (no slack: fq_src_dword reads no byte outside [0, nbytes)); everything is allocated before a byte of dst is written
  if ((rc = staged(c, who, B, bytes, nbytes, on_device, 0, &d_src)) || (rc = tmp_alloc(c, who, B, &d_x2n, sizeof x2n.t))) return rc;
  if (!dst_on_device && (rc = tmp_alloc(c, who, B, &d_out, size))) return rc;
  HIPCHK(c, hipMemcpyAsync(d_x2n, x2n.t, sizeof x2n.t, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_sz_frame, stage_grid(c, nch, musc_launch::CAP_CHUNKS), dim3(TPF_BLOCK), 0, c->stream, d_src,
                     nbytes, nch, d_x2n, d_out);
  HIPCHK(c, hipGetLastError());
  if (!dst_on_device) HIPCHK(c, hipMemcpyAsync(dst, d_out, size, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int musc_sz_frame(musc_ctx* c, const uint8_t* bytes, uint64_t nbytes, int on_device, uint8_t* dst, uint64_t capacity,
                             int dst_on_device, uint64_t* nout) {
  if (!c) return 1;
  return sz_frame_call(c, "musc_sz_frame", bytes, nbytes, on_device, dst, capacity, dst_on_device, nout);
}
