// muscato_sz_compress.hpp -- the compressing writer of framed snappy streams on the device:
// musc_sz_compress and musc_targets_prep_sz.  Included by muscato_hip.hip behind muscato_targets_prep.hpp (one
// translation unit: musc_ctx, scan_u64, staged, tmp_alloc, Readback, sz_frame_call).  The rule is sz_compress_plan.hpp's,
// the kernels are k_sz_compress and k_sz_gather of kernels_sz.hpp.  On the host this is sz_encode_compressed
// (host/sz.hpp), which stays the specification and the fallback.
//
// Two launches with a scan between them: k_sz_compress leaves every chunk in its own slot of a scratch buffer and its
// length in an array, scan_u64 makes the lengths offsets, k_sz_gather moves the chunks to their places.  No workgroup
// waits for another.

// what a call needs on the device beside its input and output, all allocated before a byte of the output is written
struct SzcBufs {
  unsigned char* slots = nullptr;  // nchunks slots of musc_szc::SLOT bytes, and spare bytes for k_sz_gather's last dword
  uint64_t* lens = nullptr;        // nchunks + 1: lengths, then offsets
  uint64_t* stmp = nullptr;
  uint32_t* x2n = nullptr;
};

static int szc_alloc(musc_ctx* c, const char* who, TmpBufs& B, uint64_t nbytes, SzcBufs* b) {
  const uint64_t nch = musc_szc::chunks(nbytes);
  int rc;
  if ((rc = tmp_alloc(c, who, B, &b->slots, nch * musc_szc::SLOT + 16)) || (rc = tmp_alloc(c, who, B, &b->lens, (nch + 1) * 8)) ||
      (rc = tmp_alloc(c, who, B, &b->stmp, scan_tmp_elems(nch + 1) * 8)) || (rc = tmp_alloc(c, who, B, &b->x2n, sizeof(musc_sz::X2n::t))))
    return rc;
  return 0;
}

// d_src: nbytes bytes on the device at any alignment; d_out: room for sz_compress_bound(nbytes) on the device at any
// alignment.  *total = the stream's length.  Waits for the stream.
static int szc_run(musc_ctx* c, const SzcBufs& b, const unsigned char* d_src, uint64_t nbytes, unsigned char* d_out, uint64_t* total) {
  static const musc_sz::X2n x2n;  // (built once)
  const uint64_t nch = musc_szc::chunks(nbytes);
  HIPCHK(c, hipMemcpyAsync(b.x2n, x2n.t, sizeof x2n.t, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(b.lens, 0, (nch + 1) * 8, c->stream));
  const dim3 g = stage_grid(c, nch, musc_launch::CAP_CHUNKS);
  if (nch) {
    const uint64_t lo = (uint64_t)(uintptr_t)d_src & 15u;
    hipLaunchKernelGGL(k_sz_compress, g, dim3(SZC_BLOCK), 0, c->stream, d_src - lo, lo, nbytes, nch, b.x2n, b.slots, b.lens);
    HIPCHK(c, hipGetLastError());
    const int rc = scan_u64(c, b.lens, b.lens, nch + 1, b.stmp);
    if (rc) return rc;
  }
  hipLaunchKernelGGL(k_sz_gather, g, dim3(SZC_BLOCK), 0, c->stream, b.slots, b.lens, nch, d_out);
  HIPCHK(c, hipGetLastError());
  uint64_t sum = 0;
  Readback R(c->scalars, c->stream);
  HIPCHK(c, R.get(b.lens + nch, &sum).wait());
  *total = musc_szc::MAGIC + sum;
  return 0;
}

static int sz_compress_call(musc_ctx* c, const char* who, const uint8_t* bytes, uint64_t nbytes, int on_device, uint8_t* dst, uint64_t capacity,
                            int dst_on_device, uint64_t* nout) {
  if (!nout) return fail(c, 2, "%s: NULL output pointer", who);
  *nout = 0;
  if (!bytes && nbytes) return fail(c, 2, "%s: NULL input", who);
  const uint64_t bound = musc_szc::sz_compress_bound(nbytes);
  *nout = bound;
  if (!dst) return 0;  // sizing: the bound (the stream's length is known only once it is made)
  if (capacity < bound)
    return fail(c, 2, "%s: capacity %llu below the %llu bytes a stream of %llu bytes may take", who, (unsigned long long)capacity,
                (unsigned long long)bound, (unsigned long long)nbytes);
  HIPCHK(c, hipSetDevice(c->device));
  TmpBufs B;
  SzcBufs b;
  const unsigned char* d_src = nullptr;
  unsigned char* d_out = dst;
  int rc = 0;
  // (no slack behind the input: fq_load16 reads no byte outside it); everything is allocated before a byte of dst is written
  if ((rc = staged(c, who, B, bytes, nbytes, on_device, 0, &d_src)) || (rc = szc_alloc(c, who, B, nbytes, &b))) return rc;
  if (!dst_on_device && (rc = tmp_alloc(c, who, B, &d_out, bound))) return rc;
  uint64_t total = 0;
  if ((rc = szc_run(c, b, d_src, nbytes, d_out, &total))) {
    (void)hipStreamSynchronize(c->stream);  // (kernels of the call may still be queued on its temporaries)
    return rc;
  }
  if (!dst_on_device) {
    HIPCHK(c, hipMemcpyAsync(dst, d_out, total, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  *nout = total;
  return 0;
}

extern "C" int musc_sz_compress(musc_ctx* c, const uint8_t* bytes, uint64_t nbytes, int on_device, uint8_t* dst, uint64_t capacity,
                                int dst_on_device, uint64_t* nout) {
  if (!c) return 1;
  return sz_compress_call(c, "musc_sz_compress", bytes, nbytes, on_device, dst, capacity, dst_on_device, nout);
}

extern "C" int musc_targets_prep_sz(musc_ctx* c, int which, int compressed, uint8_t* dst, uint64_t capacity, int dst_on_device, uint64_t* nout) {
  static const char* const who = "musc_targets_prep_sz";
  if (!c) return 1;
  if (nout) *nout = 0;
  if (which < 0 || which > 1) return fail(c, 2, "%s: which = %d is neither 0 (sequences) nor 1 (ids)", who, which);
  if (compressed < 0 || compressed > 1) return fail(c, 2, "%s: compressed = %d must be 0 or 1", who, compressed);
  if (!c->tp_have) return fail(c, 2, "%s: no prepared text (musc_targets_prep first)", who);
  const uint8_t* const text = c->tp_text[which].get();  // (null with an empty text)
  return compressed ? sz_compress_call(c, who, text, c->tp_bytes[which], 1, dst, capacity, dst_on_device, nout)
                    : sz_frame_call(c, who, text, c->tp_bytes[which], 1, dst, capacity, dst_on_device, nout);
}
