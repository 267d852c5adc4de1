// muscato_load.hpp -- the loaders: what brings a database or a read set from the caller's bytes to the resident planes
// and records.  Part of libmuscato_hip.so: included by muscato_hip.hip after the context, the scans and
// the event marks (fail, HIPCHK, grid, TmpBufs, tmp_alloc, staged, Readback, scan_u64, free_db, free_reads,
// reads_load_done, Marks), and in front of
// muscato_index.hpp and muscato_pass.hpp, which call upload_prepare, db_xblocks and the read-record functions.  The
// loaders that start from text follow it in muscato_prep.hpp (FASTQ, sort + collapse) and muscato_db_text.hpp (the gene
// file).  The arithmetic is load_plan.hpp's.
//
// Every musc_db_load_* ends in db_load_done and every musc_reads_* loader in reads_load_done: a load that failed,
// wherever it failed, leaves nothing behind.
#pragma once

// ---------------------------------------------------------------- what the loaders share

// What a loader asks of n + 1 read offsets on the device before it sizes anything: the first, the last and the longest
// read (k_max_len), read back together, with one wait.
static int offsets_census(musc_ctx* c, const uint64_t* d_off, uint64_t n, uint64_t* first, uint64_t* last, uint64_t* maxlen) {
  HIPCHK(c, hipMemsetAsync(c->counters + CNT_SCRATCH, 0, 8, c->stream));
  hipLaunchKernelGGL(k_max_len, grid(c, n), dim3(256), 0, c->stream, d_off, n, c->counters + CNT_SCRATCH);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, Readback(c->scalars, c->stream).get(c->counters + CNT_SCRATCH, maxlen).get(d_off, first).get(d_off + n, last).wait());
  return 0;
}

// The lines of a text of nbytes > 0 bytes on the device, as the FASTQ parse and the gene file take them
// (kernels_fastq.hpp): the text in 16-byte lanes of the address space, the newlines in front of each 4 096-byte tile
// (k_fq_count, scanned; cnt[ntiles] = all of them), and whether a last line without a newline adds one.  One wait.
struct TextLines {
  const unsigned char* base16 = nullptr;  // the text is its bytes [lo, hi)
  uint64_t lo = 0, hi = 0, ntiles = 0;
  dim3 tgrid;                             // of the kernels that walk the tiles again (k_fq_lines, k_dbt_lines)
  uint64_t* cnt = nullptr;                // a temporary of B
  uint64_t newlines = 0;
  uint32_t virt = 0;
};
static int text_lines(musc_ctx* c, const char* who, TmpBufs& B, const unsigned char* d_text, uint64_t nbytes, TextLines* L) {
  L->lo = (uint64_t)((uintptr_t)d_text & (FQ_LANE_BYTES - 1));
  L->hi = L->lo + nbytes;
  L->base16 = d_text - L->lo;
  L->ntiles = (L->hi + FQ_TILE_BYTES - 1) / FQ_TILE_BYTES;
  L->tgrid = stage_grid(c, L->ntiles, musc_launch::CAP_TILES);
  uint64_t* stmp = nullptr;
  int rc = 0;
  if ((rc = tmp_alloc(c, who, B, &L->cnt, (L->ntiles + 1) * 8)) || (rc = tmp_alloc(c, who, B, &stmp, scan_tmp_elems(L->ntiles + 1) * 8)))
    return rc;
  HIPCHK(c, hipMemsetAsync(L->cnt + L->ntiles, 0, 8, c->stream));
  hipLaunchKernelGGL(k_fq_count, L->tgrid, dim3(FQ_BLOCK), 0, c->stream, L->base16, L->lo, L->hi, L->ntiles, L->cnt);
  HIPCHK(c, hipGetLastError());
  if ((rc = scan_u64(c, L->cnt, L->cnt, L->ntiles + 1, stmp))) return rc;
  unsigned char last = 0;
  HIPCHK(c, Readback(c->scalars, c->stream).get(L->cnt + L->ntiles, &L->newlines).get(d_text + (nbytes - 1), &last).wait());
  L->virt = last != '\n';  // a last line without a newline is a line
  return 0;
}

// ---------------------------------------------------------------- database

// The one rule for a database load that failed, wherever it failed (the twin of reads_load_done): nothing of it stays --
// not the counts db_alloc committed, not planes that are zeroed or half packed -- and musc_match* answers "no database
// loaded" until a load succeeds.  (The message of the failure stays the context's last error.)
static int db_load_done(musc_ctx* c, int rc) {
  if (rc) {
    (void)hipStreamSynchronize(c->stream);  // (kernels of the load may still be queued on its temporaries)
    free_db(c);
  }
  return rc;
}

// the X-block bitmap of the mask plane (all zero for a plane that exists only because reads hold X)
static int db_xblocks(musc_ctx* c) {
  const uint64_t nblk64 = musc_load::dbx_blocks(c->db_words), nw = musc_load::dbx_words(c->db_words);
  HIPCHK(c, c->dbx.alloc(nw * 4));
  HIPCHK(c, hipMemsetAsync(c->dbx, 0, nw * 4, c->stream));
  hipLaunchKernelGGL(k_db_xblocks, dim3(nblk(nblk64, 256)), dim3(256), 0, c->stream, c->dbm2, c->db_words, c->dbx);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

// the pack kernel has run: whether it met an X (one wait, which also delivers what the caller has queued in R), and with
// it the mask plane's fate
static int db_finish(musc_ctx* c, Readback& R) {
  uint32_t hasx = 0;
  HIPCHK(c, R.get(c->d_flag.get(), &hasx).wait());
  c->db_has_x = hasx != 0;
  if (!hasx) {
    c->dbm2.release();
    return 0;
  }
  return db_xblocks(c);
}

// The offsets of nseq targets become the database's shape, or are refused before anything of the context changes but
// the old database, which goes first.  The offsets come to the host whole in any case (the partition planner cuts at
// target boundaries), so their first and last word and the longest target are taken from that copy: no kernel and no
// wait of their own, whichever side the caller's offsets are on.
static int db_alloc(musc_ctx* c, const uint64_t* offsets, uint32_t nseq, int on_device) {
  HIPCHK(c, hipSetDevice(c->device));
  free_db(c);
  if (nseq == 0) return fail(c, 2, "database has no sequences");
  std::vector<uint64_t> off((size_t)nseq + 1);
  if (on_device) HIPCHK(c, hipMemcpy(off.data(), offsets, off.size() * 8, hipMemcpyDeviceToHost));
  else memcpy(off.data(), offsets, off.size() * 8);
  const uint64_t last = off[nseq];
  if (off[0] != 0) return fail(c, 2, "offsets[0] must be 0");
  if (last >= (1ull << 36)) return fail(c, 2, "database larger than 2^36 bases");
  c->max_tlen = 0;
  for (uint32_t g = 0; g < nseq; g++) c->max_tlen = std::max<uint64_t>(c->max_tlen, off[g + 1] - off[g]);
  c->nseq = nseq;
  c->nbases = last;
  c->db_words = musc_load::db_words(last);
  c->h_seq_off = std::move(off);
  // DB_SLACK_WORDS of zeroed slack behind both planes (pass_two_kernel allocates a missing mask plane the same way, and
  // db_xblocks sizes dbx for db_words + 64).  What reads into it, and what bounds each access:
  //   - k_confirm<RW != 0> (pair_issue): RW <= 16 words from the word of the placement's first base, whatever the
  //     read's length -- at most 15 words past the last one.  db_span_has_x looks at the same RW * 16 bases.
  //   - k_confirm<0> (confirm_pair, runtime stride): ceil(len / 16) steps, each reading one word ahead -- at most ONE
  //     word past the word of the read's last base, and a read ends inside its target.  The bound is the read's own
  //     length: bounded by the stride of the longest read loaded it walked up to 4 099 words past the last base.
  //   - ext64 on a plane (bucket_of in the index build, res_span_word): two words past the word of its first bit,
  //     and that bit belongs to a base of the database.  ctx_words (the context index build) takes the words of a
  //     context of at most 200 bases around a window that starts inside the database.
  //   - k_results_render / the side kernels read single words of bases inside [0, nbases).
  // k_screen<0>, k_screen_t and k_hot_probes<0> never touch the planes: they read the index and the read records
  // (Rec<0>::ext = ext64 on the record: a window that takes part ends inside len, so at most two words past the
  // record's last base word -- the record's own length word, then the next record or the 256 spare bytes behind rd
  // and rdm).  The results and side kernels take c->rw only to find a record and its length word.
  const uint64_t alloc_words = musc_load::db_plane_words(c->db_words);
  HIPCHK(c, c->db2.alloc(alloc_words * 4));
  HIPCHK(c, c->dbm2.alloc(alloc_words * 4));
  HIPCHK(c, hipMemsetAsync(c->db2, 0, alloc_words * 4, c->stream));
  HIPCHK(c, hipMemsetAsync(c->dbm2, 0, alloc_words * 4, c->stream));
  HIPCHK(c, c->seq_off.alloc(((uint64_t)nseq + 1) * 8));
  HIPCHK(c, hipMemcpyAsync(c->seq_off, offsets, ((uint64_t)nseq + 1) * 8,
                           on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(c->d_flag, 0, 4, c->stream));  // raised by the packing kernel when it meets an X
  return 0;
}

static int db_load_ascii_run(musc_ctx* c, const char* seqs, const uint64_t* offsets, uint32_t nseq, int on_device) {
  int rc = db_alloc(c, offsets, nseq, on_device);
  if (rc) return rc;
  TmpBufs B;
  const unsigned char* src = nullptr;
  // (no slack: k_pack_db_ascii reads bytes [0, nbases) only)
  if ((rc = staged(c, "musc_db_load_ascii", B, (const unsigned char*)seqs, c->nbases, on_device, 0, &src))) return rc;
  if (c->db_words) {
    hipLaunchKernelGGL(k_pack_db_ascii, dim3(nblk(c->db_words, 256)), dim3(256), 0, c->stream, src, c->nbases,
                       c->db2, c->dbm2, c->db_words, c->d_flag);
    HIPCHK(c, hipGetLastError());
  }
  Readback R(c->scalars, c->stream);
  return db_finish(c, R);
}

static int db_load_packed_run(musc_ctx* c, const uint8_t* bases2bit, const uint8_t* nmask, const uint64_t* seq_offsets, uint32_t nseq) {
  static const char* const who = "musc_db_load_packed";
  int rc = db_alloc(c, seq_offsets, nseq, 0);
  if (rc) return rc;
  TmpBufs B;
  uint32_t* t2 = nullptr;
  uint16_t* tm = nullptr;
  const uint64_t w = c->db_words;
  if (w) {  // (whole zeroed words around the caller's bytes: not a staged copy)
    if ((rc = tmp_alloc(c, who, B, &t2, w * 4))) return rc;
    HIPCHK(c, hipMemsetAsync(t2, 0, w * 4, c->stream));
    HIPCHK(c, hipMemcpyAsync(t2, bases2bit, (c->nbases + 3) / 4, hipMemcpyHostToDevice, c->stream));
    if (nmask) {
      if ((rc = tmp_alloc(c, who, B, &tm, w * 2))) return rc;
      HIPCHK(c, hipMemsetAsync(tm, 0, w * 2, c->stream));
      HIPCHK(c, hipMemcpyAsync(tm, nmask, (c->nbases + 7) / 8, hipMemcpyHostToDevice, c->stream));
    }
    hipLaunchKernelGGL(k_pack_db_packed, dim3(nblk(w, 256)), dim3(256), 0, c->stream, t2, tm, c->db2, c->dbm2, w,
                       c->d_flag);
    HIPCHK(c, hipGetLastError());
  }
  Readback R(c->scalars, c->stream);
  return db_finish(c, R);
}

extern "C" int musc_db_load_ascii(musc_ctx* c, const char* seqs, const uint64_t* offsets, uint32_t nseq, int on_device) {
  if (!c) return 1;
  if (!seqs || !offsets) return fail(c, 2, "musc_db_load_ascii: NULL input");
  return db_load_done(c, db_load_ascii_run(c, seqs, offsets, nseq, on_device));
}

extern "C" int musc_db_load_packed(musc_ctx* c, const uint8_t* bases2bit, const uint8_t* nmask, const uint64_t* seq_offsets,
                                   uint32_t nseq) {
  if (!c) return 1;
  if (!bases2bit || !seq_offsets) return fail(c, 2, "musc_db_load_packed: NULL input");
  return db_load_done(c, db_load_packed_run(c, bases2bit, nmask, seq_offsets, nseq));
}

// ---------------------------------------------------------------- reads

// The records of reads [r0, r0 + n) must exist before stream `st` goes on: for the pieces of an
// asynchronous upload (reads_load_fixed) that are still missing, `st` waits for their arrival and
// packs them.  A no-op once every record exists.
static int upload_prepare(musc_ctx* c, uint64_t r0, uint64_t n, hipStream_t st) {
  musc_ctx::Upload& u = c->up;
  if (!u.active) return 0;
  const uint64_t want = std::min<uint64_t>(r0 + n, c->nreads);
  while (u.packed_upto < want && u.next_piece < u.plan.piece_end.size()) {
    const uint64_t i = u.next_piece;
    const uint64_t first = u.packed_upto, cnt = u.plan.piece_end[i] - first;
    HIPCHK(c, hipStreamWaitEvent(st, u.ev[i], 0));
    hipLaunchKernelGGL(k_pack_reads_fixed, dim3(nblk(cnt * (uint64_t)c->rw, 256)), dim3(256), 0, st, u.stage, first, cnt, u.L, c->rw, c->rd);
    HIPCHK(c, hipGetLastError());
    u.packed_upto = first + cnt;
    u.next_piece = i + 1;
  }
  if (u.packed_upto >= c->nreads) u.active = false;
  return 0;
}

// The read records, built in one way by every loader (reads_load, reads_load_fixed, reads_sort_unique_dev): a record is
// rw words -- the 2-bit bases of the longest read, then the length word, rounded up to four words -- and both planes
// end in 256 zeroed bytes (what reads past a plane's end: db_alloc).  reads_shape: rw and the words of all records
// (load_plan.hpp), or one of the three refusals in words (fixed: the wording of the fixed-length loader, which knows no
// single read to blame).
static int reads_shape(musc_ctx* c, uint64_t nreads, uint64_t maxlen, bool fixed, RecShape* s) {
  switch (musc_load::rec_shape(nreads, maxlen, s)) {
    case musc_load::TOO_MANY_READS: return fail(c, 2, "too many reads for 32-bit read_idx");
    case musc_load::READ_TOO_LONG:
      return fixed ? fail(c, 2, "read length exceeds the 65535-base record limit")
                   : fail(c, 2, "read of %llu bases exceeds the 65535-base record limit", (unsigned long long)maxlen);
    case musc_load::TOO_MANY_WORDS: return fail(c, 2, "too many read words for one dispatch (reads x record words >= 2^32)");
    case musc_load::SHAPE_OK: break;
  }
  return 0;
}
// The planes of that shape: rd -- keep: the buffer of the last fixed-length load where it is large enough, and the new
// one is kept in turn -- and, with mask, rdm.  nreads, rw and max_len are committed here, together, once the planes exist.
static int reads_records(musc_ctx* c, const RecShape& s, uint64_t nreads, uint64_t maxlen, bool mask, bool keep) {
  const uint64_t bytes = s.words * 4 + 256;
  if (!keep || c->rd_cap < bytes) {
    c->rd_cap = 0;
    HIPCHK(c, c->rd.alloc(bytes));
    if (keep) c->rd_cap = bytes;
  }
  HIPCHK(c, hipMemsetAsync(c->rd + s.words, 0, 256, c->stream));
  if (mask) {
    HIPCHK(c, c->rdm.alloc(bytes));
    HIPCHK(c, hipMemsetAsync(c->rdm + s.words, 0, 256, c->stream));
  }
  c->nreads = nreads;
  c->rw = s.rw;
  c->max_len = (uint32_t)maxlen;
  return 0;
}
// what the pack kernel left in d_flag says whether a read holds an X; a mask plane nobody needs goes
static void reads_settle_x(musc_ctx* c, uint32_t hasx) {
  c->reads_have_x = hasx != 0;
  if (!hasx) c->rdm.release();
}

// who: the public call, for the message of a temporary that does not fit
static int reads_load(musc_ctx* c, const char* who, const unsigned char* ascii, const uint8_t* bases2bit, const uint8_t* nmask,
                      const uint64_t* offsets, uint64_t nreads, int on_device, bool packed) {
  HIPCHK(c, hipSetDevice(c->device));
  free_reads(c);
  RecShape shape;
  int rc = reads_shape(c, nreads, 0, false, &shape);  // (the read count alone, before anything is uploaded)
  if (rc) return rc;
  if (nreads == 0) {
    c->rw = 4;
    return 0;
  }
  TmpBufs B;
  const uint64_t* offp = nullptr;
  uint64_t first = 0, total = 0, maxlen = 0;
  // (no slack: k_max_len and k_pack_reads read offsets [0, nreads] only)
  if ((rc = staged(c, who, B, offsets, (nreads + 1) * 8, on_device, 0, &offp)) || (rc = offsets_census(c, offp, nreads, &first, &total, &maxlen)))
    return rc;
  if (first != 0) return fail(c, 2, "read offsets[0] must be 0");
  // the mask plane only where an X can turn up: ASCII input, or packed input that comes with a mask
  if ((rc = reads_shape(c, nreads, maxlen, false, &shape)) || (rc = reads_records(c, shape, nreads, maxlen, !packed || nmask != nullptr, false)))
    return rc;
  const auto [rw, words] = shape;
  uint32_t* d_hasx = c->d_flag;
  HIPCHK(c, hipMemsetAsync(d_hasx, 0, 4, c->stream));
  if (!packed) {
    const unsigned char* src = nullptr;
    // (no slack: k_pack_reads<false> reads the bytes of each read, [0, total), only)
    if ((rc = staged(c, who, B, ascii, total, on_device, 0, &src))) return rc;
    hipLaunchKernelGGL(k_pack_reads<false>, dim3(nblk(words, 256)), dim3(256), 0, c->stream, src,
                       (const uint32_t*)nullptr, (const uint32_t*)nullptr, offp, nreads, rw, c->rd, c->rdm, d_hasx);
  } else {  // (the streams are host memory whichever side the offsets are on; whole zeroed words around them: not a staged copy)
    unsigned char *t1 = nullptr, *t2 = nullptr;
    const uint64_t b2 = ((total + 3) / 4 + 7) & ~3ull, bm = ((total + 7) / 8 + 7) & ~3ull;
    if ((rc = tmp_alloc(c, who, B, &t1, b2 + 16))) return rc;
    HIPCHK(c, hipMemsetAsync(t1, 0, b2 + 16, c->stream));
    HIPCHK(c, hipMemcpyAsync(t1, bases2bit, (total + 3) / 4, hipMemcpyHostToDevice, c->stream));
    if (nmask) {
      if ((rc = tmp_alloc(c, who, B, &t2, bm + 16))) return rc;
      HIPCHK(c, hipMemsetAsync(t2, 0, bm + 16, c->stream));
      HIPCHK(c, hipMemcpyAsync(t2, nmask, (total + 7) / 8, hipMemcpyHostToDevice, c->stream));
    }
    hipLaunchKernelGGL(k_pack_reads<true>, dim3(nblk(words, 256)), dim3(256), 0, c->stream,
                       (const unsigned char*)nullptr, (const uint32_t*)t1, (const uint32_t*)t2, offp, nreads, rw,
                       c->rd, c->rdm, d_hasx);
  }
  HIPCHK(c, hipGetLastError());
  uint32_t hasx = 0;
  HIPCHK(c, Readback(c->scalars, c->stream).get(d_hasx, &hasx).wait());
  reads_settle_x(c, hasx);
  return 0;
}

// Reads of one length without X: the 2-bit stream is all that crosses PCIe.  async: the upload is
// queued in pieces on a copy stream and the records are made batch by batch by the pass that needs
// them (upload_prepare), so that upload and matching overlap.
static int reads_load_fixed(musc_ctx* c, const uint8_t* bases2bit, uint32_t L, uint64_t nreads, int async) {
  HIPCHK(c, hipSetDevice(c->device));
  // The reads in hand go, the record buffer stays: a streamed step is bound by the link, so the first bytes are queued
  // before anything else that takes time, and in the steady state (a read set that fits the buffers of the last one)
  // this call neither frees nor allocates.
  drop_reads(c, true);
  RecShape shape;
  const int rc_shape = reads_shape(c, nreads, L, true, &shape);
  if (rc_shape) return rc_shape;
  if (nreads == 0) {
    c->rw = 4;
    return 0;
  }
  musc_ctx::Upload& u = c->up;
  const uint64_t total_bytes = musc_load::fixed_total_bytes(nreads, L);
  const uint64_t need_words = musc_load::fixed_need_words(total_bytes);  // (k_pack_reads_fixed reads up to two words past a read's last)
  HIPCHK(c, u.stage.grow(need_words * 4));
  if (!u.s_up) HIPCHK(c, hipStreamCreateWithFlags(&u.s_up, hipStreamNonBlocking));
  // the pieces: whole bytes of the stream and whole wave-tiles (64 | every end but the last), each batch of the pass
  // that consumes them a whole number of pieces -- a batch needs all of its pieces, and the next batch's pieces arrive
  // while it is matched
  stream_plan(nreads, c->batch_reads, &u.plan);
  const std::vector<uint64_t>& ends = u.plan.piece_end;
  u.L = L;
  u.packed_upto = 0;
  u.next_piece = 0;
  while (u.ev.size() < ends.size()) {
    hipEvent_t e = nullptr;
    HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    u.ev.push_back(e);
  }
  HIPCHK(c, hipMemsetAsync(u.stage + (need_words - 4), 0, 16, u.s_up));
  for (size_t i = 0; i < ends.size(); i++) {
    const auto [b0, b1] = musc_load::fixed_piece_bytes(i ? ends[i - 1] : 0, ends[i], L, total_bytes);
    HIPCHK(c, hipMemcpyAsync(reinterpret_cast<uint8_t*>(u.stage.get()) + b0, bases2bit + b0, b1 - b0, hipMemcpyHostToDevice, u.s_up));
    HIPCHK(c, hipEventRecord(u.ev[i], u.s_up));
  }
  u.active = true;
  // the records (nothing reads them before the first piece has landed): the buffer of the last fixed-length load where
  // it is large enough, its zeroed 256-byte tail at its new place
  int rc = reads_records(c, shape, nreads, L, false, true);
  if (rc) return rc;
  reads_settle_x(c, 0);
  if (!async) {
    if ((rc = upload_prepare(c, 0, nreads, c->stream))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return 0;
}

// lengths and / or a mask: offsets are made on the device (a scan of the lengths, or multiples of
// fixed_len) and the general loader takes over
static int reads_load_lengths(musc_ctx* c, const uint8_t* bases2bit, const uint8_t* nmask, const uint32_t* lengths,
                              uint32_t fixed_len, uint64_t nreads) {
  static const char* const who = "musc_reads_load_packed32";
  HIPCHK(c, hipSetDevice(c->device));
  TmpBufs B;
  uint64_t *d_off = nullptr, *stmp = nullptr;
  uint32_t* d_len = nullptr;
  int rc = tmp_alloc(c, who, B, &d_off, (nreads + 2) * 8);
  if (rc) return rc;
  if (lengths) {
    if ((rc = tmp_alloc(c, who, B, &d_len, (nreads + 1) * 4)) || (rc = tmp_alloc(c, who, B, &stmp, scan_tmp_elems(nreads + 1) * 8))) return rc;
    HIPCHK(c, hipMemcpyAsync(d_len, lengths, nreads * 4, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_widen_u32, dim3(nblk(nreads + 1, 256)), dim3(256), 0, c->stream, d_len, nreads, d_off);
    HIPCHK(c, hipGetLastError());
    if ((rc = scan_u64(c, d_off, d_off, nreads + 1, stmp))) return rc;
  } else {
    hipLaunchKernelGGL(k_iota_mul, dim3(nblk(nreads + 1, 256)), dim3(256), 0, c->stream, d_off, nreads, (uint64_t)fixed_len);
    HIPCHK(c, hipGetLastError());
  }
  return reads_load(c, who, nullptr, bases2bit, nmask, d_off, nreads, 1, true);
}

extern "C" int musc_reads_load_packed32(musc_ctx* c, const uint8_t* bases2bit, const uint8_t* nmask, const uint32_t* lengths,
                                        uint32_t fixed_len, uint64_t nreads, int async) {
  if (!c) return 1;
  if (!bases2bit && nreads) return fail(c, 2, "musc_reads_load_packed32: NULL input");
  return reads_load_done(c, !lengths && !nmask ? reads_load_fixed(c, bases2bit, fixed_len, nreads, async)
                                               : reads_load_lengths(c, bases2bit, nmask, lengths, fixed_len, nreads));
}

extern "C" int musc_reads_load_ascii(musc_ctx* c, const char* seqs, const uint64_t* offsets, uint64_t nreads, int on_device) {
  if (!c) return 1;
  if ((!seqs || !offsets) && nreads) return fail(c, 2, "musc_reads_load_ascii: NULL input");
  return reads_load_done(c, reads_load(c, "musc_reads_load_ascii", (const unsigned char*)seqs, nullptr, nullptr, offsets, nreads, on_device, false));
}

extern "C" int musc_reads_load_packed(musc_ctx* c, const uint8_t* bases2bit, const uint8_t* nmask, const uint64_t* read_offsets,
                                      uint64_t nreads) {
  if (!c) return 1;
  if ((!bases2bit || !read_offsets) && nreads) return fail(c, 2, "musc_reads_load_packed: NULL input");
  return reads_load_done(c, reads_load(c, "musc_reads_load_packed", nullptr, bases2bit, nmask, read_offsets, nreads, 0, true));
}
