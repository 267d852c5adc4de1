// kernels_sz.hpp -- framed snappy on the GPU.  Included by muscato_hip.hip behind kernels_fastq.hpp, whose
// aligned 16-byte loads it reuses.  The chunk table comes from sz_plan (sz_plan.hpp), on the host.
//
// k_sz_decode: one workgroup per data chunk.  The chunk's output, at most 65 536 bytes, is built in LDS: a copy element
// reads bytes that an earlier element of the same chunk wrote, and LDS orders those accesses inside a workgroup with a
// barrier and no cache argument.  With the 4 KiB window of the body and the CRC table a workgroup holds 70 KiB, so a CU
// (160 KiB) takes two chunks.
//   - The tag walk is uniform over the workgroup: every lane reads the same tag and operand bytes from the window.
//   - A literal is a cooperative copy from the body; a copy element is out[pos + i] = out[pos - off + i mod off], i < len,
//     whose sources all lie before pos -- the overlapping (run-length) form is as parallel as the plain one.  A barrier
//     is needed only where a copy reads what was written since the last one (dirty_lo).
//   - Every element is checked before a byte of it is written: operand bytes inside the body, the literal inside the body
//     and inside the declared length, 1 <= off <= pos, pos + len <= the declared length; a chunk ends with pos == the
//     declared length.  So a chunk reads nothing outside [body, body + body_len) and writes nothing outside
//     [out_off, out_off + ulen), whatever its bytes say.  The first check that fails is the chunk's status (sz.hpp's
//     decoder, which appends first and compares lengths last, may name a later one).
//   - CRC-32C from LDS: each lane takes a slice of an odd number of dwords (no two lanes of a wave on one bank), the
//     slices' CRCs are joined by multiplication by x^(8 bytes behind the slice) mod P (sz_plan.hpp), masked as mask_crc
//     does and compared with the stored word.
//   - Only then is the chunk written out: whole dwords where the output address allows, bytes at the edges.

#define SZ_BLOCK 256u
#define SZ_WIN_UNITS 256u  // 16-byte units of the body window

struct SzChunkDev {
  uint64_t body;     // offset in the stream
  uint64_t out_off;  // offset in the output
  uint32_t body_len, ulen, crc, type;
};

DEV uint32_t sz_gf2_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
#pragma unroll 8
  for (uint32_t m = 0x80000000u; m; m >>= 1) {
    p ^= (a & m) ? b : 0u;
    b = (b >> 1) ^ ((b & 1u) ? 0x82F63B78u : 0u);
  }
  return p;
}

// stream16 = the stream's address rounded down to 16, slo = the stream's first byte in that space.  dst == nullptr: decode
// and check only.  status[chunk] = musc_sz::Status.
MUSC_KERNEL __launch_bounds__(SZ_BLOCK) void k_sz_decode(const unsigned char* __restrict__ stream16, uint64_t slo,
                                                        const SzChunkDev* __restrict__ chunks, uint32_t nchunks,
                                                        const uint32_t* __restrict__ x2n, unsigned char* __restrict__ dst,
                                                        uint32_t* __restrict__ status) {
  __shared__ uint32_t s_out[65536 / 4];
  __shared__ uint4 s_win[SZ_WIN_UNITS];
  __shared__ uint32_t s_tab[256];
  __shared__ uint32_t s_red[SZ_BLOCK / 64];
  unsigned char* const out = reinterpret_cast<unsigned char*>(s_out);
  const unsigned char* const win = reinterpret_cast<const unsigned char*>(s_win);
  const uint32_t tid = threadIdx.x;
  {
    uint32_t c = tid;
#pragma unroll
    for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ 0x82F63B78u : c >> 1;
    s_tab[tid] = c;
  }
  for (uint32_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    const SzChunkDev C = chunks[ch];
    const uint64_t lo = slo + C.body, hi = lo + C.body_len;  // the body in the aligned address space
    const uint32_t n = C.body_len, ulen = C.ulen;
    uint32_t st = 0;
    __syncthreads();  // (the previous chunk's output and window are done with)
    if (C.type == 1) {
      for (uint32_t i = tid; i < ulen; i += SZ_BLOCK) out[i] = stream16[lo + i];
    } else {
      uint32_t p = 0, pos = 0, dirty_lo = 0;
      uint64_t win_j = ~0ull;  // first unit in the window; none yet
      while (p < n) {
        // the tag and its operand bytes (at most five) in the window
        const uint64_t a = lo + p;
        if (win_j == ~0ull || a < win_j * 16 || a + 5 > (win_j + SZ_WIN_UNITS) * 16) {
          __syncthreads();
          win_j = a / 16;
          if ((win_j + tid) * 16 < hi) s_win[tid] = fq_load16(stream16, win_j + tid, lo, hi);
          __syncthreads();
          dirty_lo = pos;
        }
        const unsigned char* w = win + (a - win_j * 16);
        const uint32_t tag = w[0], t = tag & 3u;
        uint32_t len, off = 0;
        p++;
        if (t == 0) {
          uint64_t l = tag >> 2;
          if (l >= 60) {
            const uint32_t nb = (uint32_t)l - 59;
            if (nb > n - p) { st = musc_sz::ST_TRUNC_LITLEN; break; }
            l = 0;
            for (uint32_t i = 0; i < nb; i++) l |= (uint64_t)w[1 + i] << (8 * i);
            p += nb;
          }
          l += 1;
          if (l > n - p) { st = musc_sz::ST_TRUNC_LITERAL; break; }
          if (l > ulen - pos) { st = musc_sz::ST_LENGTH; break; }
          len = (uint32_t)l;
          for (uint32_t i = tid; i < len; i += SZ_BLOCK) out[pos + i] = stream16[lo + p + i];
          p += len;
        } else {
          const uint32_t nb = t == 1 ? 1u : t == 2 ? 2u : 4u;
          if (nb > n - p) { st = musc_sz::ST_TRUNC_COPY; break; }
          if (t == 1) {
            len = ((tag >> 2) & 7u) + 4;
            off = ((tag >> 5) << 8) | w[1];
          } else {
            len = (tag >> 2) + 1;
            off = w[1] | ((uint32_t)w[2] << 8);
            if (t == 3) off |= ((uint32_t)w[3] << 16) | ((uint32_t)w[4] << 24);
          }
          p += nb;
          if (off == 0 || off > pos) { st = musc_sz::ST_BAD_OFFSET; break; }
          if (len > ulen - pos) { st = musc_sz::ST_LENGTH; break; }
          const uint32_t src = pos - off, src_end = src + (off < len ? off : len);
          if (src_end > dirty_lo) {  // reads what was written since the last barrier
            __syncthreads();
            dirty_lo = pos;
          }
          if (tid < len) out[pos + tid] = out[src + tid % off];  // (len <= 64)
        }
        pos += len;
      }
      if (st == 0 && pos != ulen) st = musc_sz::ST_LENGTH;
    }
    __syncthreads();

    // ---- CRC-32C of out[0, ulen)
    if (st == 0) {
      const uint32_t sd = ((ulen + 4 * SZ_BLOCK - 1) / (4 * SZ_BLOCK)) | 1u;  // dwords per slice, odd
      const uint32_t b0 = tid * sd * 4;
      const uint32_t b1 = b0 + sd * 4 < ulen ? b0 + sd * 4 : ulen;
      uint32_t c = 0;
      if (b0 < ulen) {
        c = 0xFFFFFFFFu;
        uint32_t i = b0;
        for (; i + 4 <= b1; i += 4) {
          uint32_t v = s_out[i >> 2];
#pragma unroll
          for (int k = 0; k < 4; k++, v >>= 8) c = s_tab[(c ^ v) & 0xFFu] ^ (c >> 8);
        }
        for (; i < b1; i++) c = s_tab[(c ^ out[i]) & 0xFFu] ^ (c >> 8);
        c ^= 0xFFFFFFFFu;
        // times x^(8 * bytes behind the slice)
        uint32_t m = 0x80000000u;
        uint32_t behind = ulen - b1;
        for (uint32_t k = 3; behind; behind >>= 1, k++)
          if (behind & 1u) m = sz_gf2_mul(x2n[k], m);
        c = sz_gf2_mul(m, c);
      }
#pragma unroll
      for (int d = 32; d; d >>= 1) c ^= __shfl_xor(c, d);
      if ((tid & 63u) == 0) s_red[tid >> 6] = c;
      __syncthreads();
      c = 0;
#pragma unroll
      for (uint32_t k = 0; k < SZ_BLOCK / 64; k++) c ^= s_red[k];
      const uint32_t masked = ((c >> 15) | (c << 17)) + 0xa282ead8u;
      if (masked != C.crc) st = musc_sz::ST_CHECKSUM;
    }
    if (tid == 0) status[ch] = st;

    // ---- the chunk's bytes to dst + out_off: whole dwords where the address allows, bytes at the edges
    if (st == 0 && dst) {
      unsigned char* const d = dst + C.out_off;
      const uint32_t mis = (4u - ((uint32_t)(uintptr_t)d & 3u)) & 3u;
      const uint32_t head = mis < ulen ? mis : ulen;
      const uint32_t nd = (ulen - head) >> 2;
      for (uint32_t k = tid; k < nd; k += SZ_BLOCK) {
        const uint32_t q = head + 4 * k;
        uint32_t v;
        if (head == 0) v = s_out[k];
        else v = __builtin_amdgcn_alignbyte(s_out[(q >> 2) + 1], s_out[q >> 2], head);
        *reinterpret_cast<uint32_t*>(d + q) = v;
      }
      const uint32_t tail0 = head + 4 * nd;
      if (tid < head) d[tid] = out[tid];
      else if (tid >= 4 && tail0 + (tid - 4) < ulen) d[tail0 + (tid - 4)] = out[tail0 + (tid - 4)];
    }
  }
}
