// muscato_prep.hpp -- read prep on the GPU: bytewise sort of the prepared reads and collapse of
// identical sequences, and the FASTQ parse in front of it (kernels_fastq.hpp).
// Included by muscato_hip.hip right behind muscato_load.hpp (one translation unit: it uses musc_ctx,
// the record functions, what the drivers share -- staged, tmp_alloc, KeyPasses, Readback -- and the loaders'
// offsets_census and text_lines).
//
// Reference: cmd/muscato/main.go sortReads (GNU `sort` of the `seq\tname` lines under LC_ALL=C)
// followed by cmd/muscato_uniqify/main.go:83-135 (adjacent lines with the same sequence become
// one line `seq\tcount\tname1;name2...`).  Only the sequence column is the GPU's business: it
// returns the sort order (ties in input order; the host orders the names of a group, which is
// what comparing the whole `seq\tname` line amounts to) and the group boundaries, and leaves the
// distinct sequences loaded as the context's reads, exactly as musc_reads_load_ascii of the
// first column of reads_sorted.txt.sz would.
//
// Order: bytewise on A < C < G < T < X (ASCII 65 < 67 < 71 < 84 < 88), a proper prefix sorts
// first (the tab that follows it, 9, is below every letter).  A read becomes ceil(maxlen / 21)
// u64 key words of 3-bit codes (0 = past the end, 1..5 = A C G T other), first base most
// significant, so that comparing the words as integers from the first to the last is that
// order; the sort is LSD over the words, one stable pass of KeyPasses per word.

#define PREP_BASES_PER_WORD 21

DEV uint32_t prep_code(unsigned char ch) {
  switch (ch) {
    case 'A': return 1u;
    case 'C': return 2u;
    case 'G': return 3u;
    case 'T': return 4u;
    default: return 5u;  // prepared reads hold nothing but A C G T X (cmd/muscato_prep_reads/main.go:33-44)
  }
}

// keys[i] = key word `w` of read perm[i]
MUSC_KERNEL __launch_bounds__(256) void k_prep_keys(const unsigned char* __restrict__ s,
                                                   const uint64_t* __restrict__ off,
                                                   const uint32_t* __restrict__ perm, uint64_t n, uint32_t w,
                                                   uint64_t* __restrict__ keys) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t r = perm[i];
    const uint64_t o = off[r];
    const uint64_t len = off[r + 1] - o;
    const uint64_t first = (uint64_t)w * PREP_BASES_PER_WORD;
    uint64_t key = 0;
    for (uint32_t j = 0; j < PREP_BASES_PER_WORD; j++) {
      const uint64_t q = first + j;
      if (q >= len) break;
      key |= (uint64_t)prep_code(s[o + q]) << (60 - 3 * j);
    }
    keys[i] = key;
  }
}

// head[i] = 1 when the i-th read in sorted order differs from the one before it
MUSC_KERNEL __launch_bounds__(256) void k_prep_heads(const unsigned char* __restrict__ s,
                                                    const uint64_t* __restrict__ off,
                                                    const uint32_t* __restrict__ perm, uint64_t n,
                                                    uint32_t* __restrict__ head) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    uint32_t h = 1;
    if (i > 0) {
      const uint32_t a = perm[i], b = perm[i - 1];
      const uint64_t oa = off[a], ob = off[b];
      const uint64_t la = off[a + 1] - oa, lb = off[b + 1] - ob;
      if (la == lb) {
        h = 0;
        for (uint64_t q = 0; q < la; q++)
          if (s[oa + q] != s[ob + q]) {
            h = 1;
            break;
          }
      }
    }
    head[i] = h;
  }
}

// ustart[g] = position in sorted order where group g starts (gid = inclusive scan of head, minus 1)
MUSC_KERNEL void k_prep_starts(const uint32_t* __restrict__ head, const uint32_t* __restrict__ incl, uint64_t n,
                              uint32_t* __restrict__ ustart, uint32_t* __restrict__ uhead,
                              const uint32_t* __restrict__ perm) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    if (head[i]) {
      ustart[incl[i] - 1] = (uint32_t)i;
      uhead[incl[i] - 1] = perm[i];  // the input read that represents the group
    }
    if (i == n - 1) ustart[incl[i]] = (uint32_t)n;
  }
}

// 2-bit records of the distinct reads: record g = input read uhead[g] (k_pack_reads with one
// level of indirection)
MUSC_KERNEL void k_prep_pack(const unsigned char* __restrict__ s, const uint64_t* __restrict__ off,
                            const uint32_t* __restrict__ uhead, uint64_t nunique, int rw,
                            uint32_t* __restrict__ rd, uint32_t* __restrict__ rdm, uint32_t* __restrict__ has_x) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t g = t / rw;
  const int j = (int)(t % rw);
  if (g >= nunique) return;
  const uint32_t r = uhead[g];
  const uint64_t o = off[r];
  const uint32_t len = (uint32_t)(off[r + 1] - o);
  if (j == rw - 1) {
    uint32_t anyx = 0;
    for (uint32_t q = 0; q < len; q++) {
      uint32_t isx;
      (void)ascii_code(s[o + q], &isx);
      anyx |= isx;
    }
    rd[t] = (len & 0xFFFFu) | (anyx ? READ_HAS_X : 0u);
    rdm[t] = 0;
    return;
  }
  uint32_t v = 0, mv = 0;
  for (int b = 0; b < 16; b++) {
    const uint32_t q = (uint32_t)j * 16 + b;
    if (q < len) {
      uint32_t isx;
      const uint32_t c = ascii_code(s[o + q], &isx);
      v |= c << (2 * b);
      mv |= isx << (2 * b);
    }
  }
  rd[t] = v;
  rdm[t] = mv;
  if (mv) atomicOr(has_x, 1u);
}

// The device stage of musc_reads_sort_unique on n > 0 prepared reads that are already in device memory (d_s, d_off as
// musc_reads_load_ascii takes them), for the public call `who`.  Mark 0 has been set by the caller, in front of whatever
// device work of its own the time is to cover; mark 1 is set here.
static int reads_sort_unique_dev(musc_ctx* c, const char* who, const unsigned char* d_s, const uint64_t* d_off, const uint64_t n,
                                 const Marks& m, uint32_t** order, uint32_t** ustart, uint64_t* nunique) {
  TmpBufs B;
  RecShape shape;
  uint64_t first = 0, last = 0, maxlen = 0;
  int rc = offsets_census(c, d_off, n, &first, &last, &maxlen);
  if (rc) return rc;
  if (first != 0) return fail(c, 2, "read offsets[0] must be 0");
  if ((rc = reads_shape(c, 0, maxlen, false, &shape))) return rc;  // (the longest read alone, before anything is sorted)

  // ---- LSD sort over the key words
  const uint32_t nw = (uint32_t)std::max<uint64_t>((maxlen + PREP_BASES_PER_WORD - 1) / PREP_BASES_PER_WORD, 1);
  KeyPasses K;
  if ((rc = K.start(c, who, n, {63u}))) return rc;
  for (uint32_t w = nw; w-- > 0 && !rc;)
    rc = K.pass(63u, [&](const uint32_t* perm, uint64_t* keys) { hipLaunchKernelGGL(k_prep_keys, grid(c, n), dim3(256), 0, c->stream, d_s, d_off, perm, n, w, keys); });
  if (rc) return rc;
  const uint32_t* const p0 = K.order();

  // ---- groups of identical sequences
  uint32_t *head = nullptr, *incl = nullptr, *stmp = nullptr, *d_ustart = nullptr, *d_uhead = nullptr;
  if ((rc = tmp_alloc(c, who, B, &head, n * 4)) || (rc = tmp_alloc(c, who, B, &incl, n * 4)) ||
      (rc = tmp_alloc(c, who, B, &stmp, scan_tmp_elems(n) * 4)) || (rc = tmp_alloc(c, who, B, &d_ustart, (n + 1) * 4)) ||
      (rc = tmp_alloc(c, who, B, &d_uhead, n * 4)))
    return rc;
  hipLaunchKernelGGL(k_prep_heads, grid(c, n), dim3(256), 0, c->stream, d_s, d_off, p0, n, head);
  HIPCHK(c, hipGetLastError());
  if ((rc = scan_u32(c, head, incl, n, true, stmp))) return rc;
  hipLaunchKernelGGL(k_prep_starts, grid(c, n), dim3(256), 0, c->stream, head, incl, n, d_ustart, d_uhead, p0);
  HIPCHK(c, hipGetLastError());
  uint64_t nu = 0;
  HIPCHK(c, Readback(c->scalars, c->stream).get(incl + (n - 1), &nu).wait());

  // ---- the distinct sequences become the context's reads
  if ((rc = reads_shape(c, nu, maxlen, false, &shape)) || (rc = reads_records(c, shape, nu, maxlen, true, false))) return rc;
  const auto [rw, words] = shape;
  uint32_t* d_hasx = c->d_flag;
  HIPCHK(c, hipMemsetAsync(d_hasx, 0, 4, c->stream));
  hipLaunchKernelGGL(k_prep_pack, dim3(nblk(words, 256)), dim3(256), 0, c->stream, d_s, d_off, d_uhead, nu, rw, c->rd,
                     c->rdm, d_hasx);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, m.mark(c, 1));

  // ---- order and group boundaries for the host (names, counts)
  // (the owners free what the two copies target behind the wait alone: no return lies between the first copy and it)
  std::unique_ptr<uint32_t, decltype(&free)> h_order((uint32_t*)malloc(n * 4), free), h_ustart((uint32_t*)malloc((nu + 1) * 4), free);
  if (!h_order || !h_ustart) return fail(c, 7, "out of host memory for the sort order");
  uint32_t hasx = 0;
  hipError_t e = hipMemcpyAsync(h_order.get(), p0, n * 4, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(h_ustart.get(), d_ustart, (nu + 1) * 4, hipMemcpyDeviceToHost, c->stream);
  const hipError_t ew = Readback(c->scalars, c->stream).get(d_hasx, &hasx).wait();
  if (e == hipSuccess) e = ew;
  if (e != hipSuccess) return fail(c, 10, "musc_reads_sort_unique: %s", hipGetErrorString(e));
  reads_settle_x(c, hasx);
  c->stats.ms_read_prep = m.ms(0, 1);  // device time of the last sort + collapse
  *order = h_order.release();
  *ustart = h_ustart.release();
  *nunique = nu;
  return 0;
}

static int reads_sort_unique_run(musc_ctx* c, const char* seqs, const uint64_t* offsets, uint64_t nreads, int on_device,
                                 uint32_t** order, uint32_t** ustart, uint64_t* nunique) {
  HIPCHK(c, hipSetDevice(c->device));
  free_reads(c);
  if (nreads >= 0xFFFFFFF0ull) return fail(c, 2, "too many reads for 32-bit read numbers");
  if (nreads == 0) {
    c->rw = 4;
    *order = (uint32_t*)malloc(4);
    *ustart = (uint32_t*)calloc(1, 4);
    if (!*order || !*ustart) return fail(c, 7, "out of host memory");
    return 0;
  }
  static const char* const who = "musc_reads_sort_unique";
  Marks m;
  int rc = m.start(c);
  if (rc) return rc;
  TmpBufs B;  // the upload: released when the device stage has returned
  const unsigned char* d_s = nullptr;
  const uint64_t* d_off = nullptr;
  // (64 spare bytes behind the sequences, as behind the prepared reads of the FASTQ stage: k_prep_keys, k_prep_heads and
  // k_prep_pack read the bytes of each read only; no slack behind the offsets: nothing reads past offsets[nreads])
  if ((rc = staged(c, who, B, (const unsigned char*)seqs, on_device ? 0 : offsets[nreads], on_device, 64, &d_s)) ||
      (rc = staged(c, who, B, offsets, (nreads + 1) * 8, on_device, 0, &d_off)))
    return rc;
  HIPCHK(c, m.mark(c, 0));
  return reads_sort_unique_dev(c, who, d_s, d_off, nreads, m, order, ustart, nunique);
}

extern "C" int musc_reads_sort_unique(musc_ctx* c, const char* seqs, const uint64_t* offsets, uint64_t nreads,
                                      int on_device, uint32_t** order, uint32_t** ustart, uint64_t* nunique) {
  if (!c) return 1;
  if (!order || !ustart || !nunique) return fail(c, 2, "musc_reads_sort_unique: NULL output pointer");
  *order = *ustart = nullptr;
  *nunique = 0;
  if ((!seqs || !offsets) && nreads) return fail(c, 2, "musc_reads_sort_unique: NULL input");
  return reads_load_done(c, reads_sort_unique_run(c, seqs, offsets, nreads, on_device, order, ustart, nunique));
}

// ---------------------------------------------------------------- FASTQ text -> prepared reads (kernels_fastq.hpp)

extern "C" void musc_fastq_prep_free(musc_fastq_prep* p) {
  if (!p) return;
  free(p->name_off);
  free(p->seq_off);
  free(p->name_len);
  free(p->seq_len);
  free(p->order);
  free(p->ustart);
  memset(p, 0, sizeof *p);
}

// `after(d_text, d_name_off, d_name_len, d_seq_len)` runs behind the sort + collapse, the kept reads' spans as device
// arrays (null when no read is kept).  keep_text: the text and the record tables stay resident until it has returned
// (the read-name stage, muscato_read_names.hpp, reads the names in place); else they go before the sort as always.
template <class After>
static int fastq_prep_run(musc_ctx* c, const char* who, const char* text, uint64_t nbytes, int on_device, int32_t min_len, uint32_t max_len,
                          musc_fastq_prep* out, bool keep_text, After after) {
  Marks m;
  int rc = m.start(c);
  if (rc) return rc;
  TmpBufs P;  // the text and the record tables: released before the sort takes its own temporaries
  TmpBufs S;  // the prepared reads
  const unsigned char* d_text = nullptr;
  // (16 spare bytes: the text's last 16-byte lane lies inside the block; fq_load16 reads no byte past the text itself)
  if ((rc = staged(c, who, P, (const unsigned char*)text, nbytes, on_device, 16, &d_text))) return rc;
  HIPCHK(c, m.mark(c, 0));

  // ---- lines: newlines per tile, tile bases
  TextLines L;
  if (nbytes && (rc = text_lines(c, who, P, d_text, nbytes, &L))) return rc;
  const uint64_t nrec = (L.newlines + L.virt) / 4;  // an incomplete last record is dropped
  if (nrec >= 0xFFFFFFF0ull) return fail(c, 2, "too many reads for 32-bit read numbers");

  // ---- records: spans, the \r rule, the length rules; kept reads' numbers and offsets
  uint64_t *lines = nullptr, *len = nullptr;
  uint32_t *kidx = nullptr, *name_len = nullptr;
  uint64_t nkept = 0, total = 0;
  if (nrec) {
    uint64_t* stmp64 = nullptr;
    uint32_t* stmp32 = nullptr;
    if ((rc = tmp_alloc(c, who, P, &lines, (3 * (nrec + 1) + 2) * 8)) ||  // three tables and the two counters of k_fq_records
        (rc = tmp_alloc(c, who, P, &len, (nrec + 1) * 8)) || (rc = tmp_alloc(c, who, P, &kidx, (nrec + 1) * 4)) ||
        (rc = tmp_alloc(c, who, P, &name_len, (nrec + 1) * 4)) || (rc = tmp_alloc(c, who, P, &stmp64, scan_tmp_elems(nrec + 1) * 8)) ||
        (rc = tmp_alloc(c, who, P, &stmp32, scan_tmp_elems(nrec + 1) * 4)))
      return rc;
    uint64_t *name_begin = lines, *name_end = lines + (nrec + 1), *seq_end = lines + 2 * (nrec + 1);
    unsigned long long* st = reinterpret_cast<unsigned long long*>(lines + 3 * (nrec + 1));
    hipLaunchKernelGGL(k_fq_lines, L.tgrid, dim3(FQ_BLOCK), 0, c->stream, L.base16, L.lo, L.hi, L.ntiles, L.cnt, nrec, L.virt, L.newlines,
                       name_begin, name_end, seq_end);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemsetAsync(st, 0, 16, c->stream));
    hipLaunchKernelGGL(k_fq_records, grid(c, nrec + 1), dim3(256), 0, c->stream, d_text, nrec,
                       name_begin, name_end, seq_end, min_len, max_len, kidx, len, name_len, st);
    HIPCHK(c, hipGetLastError());
    if ((rc = scan_u32(c, kidx, kidx, nrec + 1, false, stmp32)) || (rc = scan_u64(c, len, len, nrec + 1, stmp64))) return rc;
    uint64_t census[2] = {0, 0};  // the longest kept read, the reads that were too short
    HIPCHK(c, Readback(c->scalars, c->stream).get(kidx + nrec, &nkept).get(len + nrec, &total).get_words(st, census, 2).wait());
    out->max_len = (uint32_t)census[0];
    out->n_short = census[1];
  }
  out->n_records = nrec;
  out->n_reads = nkept;
  out->name_off = (uint64_t*)malloc(std::max<uint64_t>(nkept, 1) * 8);
  out->seq_off = (uint64_t*)malloc(std::max<uint64_t>(nkept, 1) * 8);
  out->name_len = (uint32_t*)malloc(std::max<uint64_t>(nkept, 1) * 4);
  out->seq_len = (uint32_t*)malloc(std::max<uint64_t>(nkept, 1) * 4);
  if (!out->name_off || !out->seq_off || !out->name_len || !out->seq_len) return fail(c, 7, "out of host memory for the read spans");
  if (nkept == 0) {  // as musc_reads_sort_unique of no reads
    c->rw = 4;
    out->order = (uint32_t*)malloc(4);
    out->ustart = (uint32_t*)calloc(1, 4);
    if (!out->order || !out->ustart) return fail(c, 7, "out of host memory");
    return after(d_text, (const uint64_t*)nullptr, (const uint32_t*)nullptr, (const uint32_t*)nullptr);
  }

  // ---- the prepared reads, and the kept reads' spans for the host
  unsigned char* prep = nullptr;
  uint64_t *prep_off = nullptr, *o64 = nullptr;
  uint32_t* o32 = nullptr;
  if ((rc = tmp_alloc(c, who, S, &prep, total + 64)) || (rc = tmp_alloc(c, who, S, &prep_off, (nkept + 1) * 8)) ||
      (rc = tmp_alloc(c, who, P, &o64, 2 * nkept * 8)) || (rc = tmp_alloc(c, who, P, &o32, 2 * nkept * 4)))
    return rc;
  hipLaunchKernelGGL(k_fq_gather, stage_grid(c, nblk(nrec, 256 / FQ_GROUP), musc_launch::CAP_TILES), dim3(256), 0, c->stream, d_text, nbytes,
                     nrec, lines, lines + (nrec + 1), kidx, len, name_len, prep, prep_off, o64, o64 + nkept, o32, o32 + nkept);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(out->name_off, o64, nkept * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(out->seq_off, o64 + nkept, nkept * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(out->name_len, o32, nkept * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(out->seq_len, o32 + nkept, nkept * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (!keep_text) P.release();
  if ((rc = reads_sort_unique_dev(c, who, prep, prep_off, nkept, m, &out->order, &out->ustart, &out->n_unique))) return rc;
  S.release();
  return after(d_text, (const uint64_t*)o64, (const uint32_t*)o32, (const uint32_t*)(o32 + nkept));
}

extern "C" int musc_reads_prep_fastq(musc_ctx* c, const char* text, uint64_t nbytes, int on_device, int32_t min_read_len,
                                     int32_t max_read_len, musc_fastq_prep* out) {
  if (!c) return 1;
  if (!out) return fail(c, 2, "musc_reads_prep_fastq: NULL output pointer");
  memset(out, 0, sizeof *out);
  if (!text && nbytes) return fail(c, 2, "musc_reads_prep_fastq: NULL input");
  HIPCHK(c, hipSetDevice(c->device));
  free_reads(c);
  if (max_read_len < 0) return reads_load_done(c, fail(c, 2, "musc_reads_prep_fastq: max_read_len %d is negative", max_read_len));
  const int rc = reads_load_done(c, fastq_prep_run(c, "musc_reads_prep_fastq", text, nbytes, on_device, min_read_len, (uint32_t)max_read_len, out, false,
                                                   [](const unsigned char*, const uint64_t*, const uint32_t*, const uint32_t*) { return 0; }));
  if (rc) musc_fastq_prep_free(out);  // nothing stale: no reads and (behind reads_load_done's wait for the queued downloads) no arrays
  return rc;
}
