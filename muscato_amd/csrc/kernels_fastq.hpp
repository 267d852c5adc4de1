// kernels_fastq.hpp -- FASTQ parsing on the GPU: from the raw bytes of the read file to the prepared reads that
// musc_reads_sort_unique orders and collapses.  Included by muscato_hip.hip next to muscato_prep.hpp.
//
// Reference: utils/fastq.go:35-61 (records of four lines under bufio.ScanLines: a line ends at '\n', one trailing '\r'
// is dropped, a last line without '\n' is a line, an incomplete last record is dropped) and
// cmd/muscato_prep_reads/main.go:46-92 (MinReadLength on the raw length, every byte that is none of A C G T becomes
// X, MaxReadLength).  The name rules of the latter (1000 bytes) stay with the caller.
//
// Passes.  Every byte position and every line ordinal is 64-bit.
//   k_fq_count    newlines per 4096-byte tile (a lane owns 16 bytes, a workgroup a tile)
//   scan_u64      tile bases
//   k_fq_lines    the same load again; every newline gets its global ordinal k and, with p its position,
//                   k % 4 == 0  ends a name:      name_end[k / 4] = p  (the sequence begins at p + 1)
//                   k % 4 == 1  ends a sequence:  seq_end[k / 4] = p
//                   k % 4 == 3  starts a name:    name_begin[k / 4 + 1] = p + 1
//   k_fq_records  one lane per record: the '\r' rule, raw length, kept flag, prepared length
//   scan_u32/u64  the kept reads' numbers and the offsets of their prepared sequences
//   k_fq_gather   16 lanes per record: the prepared bytes, assembled as whole aligned dwords
//
// A lane's 16 bytes are 16-byte aligned in the ADDRESS space: with lo = the text's address modulo 16, chunk j holds
// the text's bytes [16 j - lo, 16 j + 16 - lo).  A chunk that lies inside the text is one 16-byte load; the first and
// the last chunk of a text whose address or end is not a multiple of 16 are read byte by byte, the bytes outside the
// text never.

#define FQ_LANE_BYTES 16u
#define FQ_BLOCK 256u
#define FQ_TILE_BYTES (FQ_LANE_BYTES * FQ_BLOCK)
#define FQ_GROUP 16u  // lanes that write one read in k_fq_gather

// 0x80 in every byte of v that equals the byte replicated in c4, 0 in the others (no carry crosses a byte)
DEV uint32_t fq_eq_bytes(uint32_t v, uint32_t c4) {
  const uint32_t x = v ^ c4;
  return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
}

// bit b set where byte b of the 16 is '\n' (the four 0x80 flags of a dword gathered by one multiplication: the
// partial products land on distinct bits, so nothing carries)
DEV uint32_t fq_nl_mask(uint4 v) {
  const uint32_t a = ((fq_eq_bytes(v.x, 0x0A0A0A0Au) >> 7) * 0x00204081u) >> 21 & 0xFu;
  const uint32_t b = ((fq_eq_bytes(v.y, 0x0A0A0A0Au) >> 7) * 0x00204081u) >> 21 & 0xFu;
  const uint32_t c = ((fq_eq_bytes(v.z, 0x0A0A0A0Au) >> 7) * 0x00204081u) >> 21 & 0xFu;
  const uint32_t d = ((fq_eq_bytes(v.w, 0x0A0A0A0Au) >> 7) * 0x00204081u) >> 21 & 0xFu;
  return a | (b << 4) | (c << 8) | (d << 12);
}

DEV uint32_t fq_edge_dword(const unsigned char* __restrict__ p, uint64_t a, uint64_t lo, uint64_t hi) {
  uint32_t w = 0;
#pragma unroll
  for (uint32_t b = 0; b < 4; b++)
    if (a + b >= lo && a + b < hi) w |= (uint32_t)p[a + b] << (8 * b);
  return w;
}

// chunk j of the aligned address space that starts at base16; the text is its bytes [lo, hi).  Bytes outside the text
// are not read and come back as 0.
DEV uint4 fq_load16(const unsigned char* __restrict__ base16, uint64_t j, uint64_t lo, uint64_t hi) {
  const uint64_t a = j * FQ_LANE_BYTES;
  if (a >= lo && a + FQ_LANE_BYTES <= hi) return *reinterpret_cast<const uint4*>(base16 + a);
  uint4 v;
  v.x = fq_edge_dword(base16, a, lo, hi);
  v.y = fq_edge_dword(base16, a + 4, lo, hi);
  v.z = fq_edge_dword(base16, a + 8, lo, hi);
  v.w = fq_edge_dword(base16, a + 12, lo, hi);
  return v;
}

// cnt[t] = newlines of tile t
MUSC_KERNEL __launch_bounds__(FQ_BLOCK) void k_fq_count(const unsigned char* __restrict__ base16, uint64_t lo, uint64_t hi,
                                                       uint64_t ntiles, uint64_t* __restrict__ cnt) {
  __shared__ uint32_t s_wave[FQ_BLOCK / 64];
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t j = t * FQ_BLOCK + threadIdx.x;
    uint32_t n = 0;
    if (j * FQ_LANE_BYTES < hi) n = (uint32_t)__popc(fq_nl_mask(fq_load16(base16, j, lo, hi)));
#pragma unroll
    for (int d = 32; d; d >>= 1) n += __shfl_xor(n, d);
    if ((threadIdx.x & 63u) == 0) s_wave[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t s = 0;
#pragma unroll
      for (uint32_t w = 0; w < FQ_BLOCK / 64; w++) s += s_wave[w];
      cnt[t] = s;
    }
    __syncthreads();
  }
}

// newline number k at text position p (see the table at the top); nrec = complete records
DEV void fq_emit(uint64_t k, uint64_t p, uint64_t nrec, uint64_t* __restrict__ name_begin, uint64_t* __restrict__ name_end,
                 uint64_t* __restrict__ seq_end) {
  const uint64_t r = k >> 2;
  const uint32_t m = (uint32_t)k & 3u;
  if (m == 0) {
    if (r < nrec) name_end[r] = p;
  } else if (m == 1) {
    if (r < nrec) seq_end[r] = p;
  } else if (m == 3) {
    if (r + 1 < nrec) name_begin[r + 1] = p + 1;
  }
}

// tile_base = the exclusive scan of k_fq_count's counts.  virt != 0: the text does not end in '\n', and its last line
// is closed by one virtual newline, number virt_k, at position hi - lo (the text's length).
MUSC_KERNEL __launch_bounds__(FQ_BLOCK) void k_fq_lines(const unsigned char* __restrict__ base16, uint64_t lo, uint64_t hi,
                                                       uint64_t ntiles, const uint64_t* __restrict__ tile_base, uint64_t nrec,
                                                       uint32_t virt, uint64_t virt_k, uint64_t* __restrict__ name_begin,
                                                       uint64_t* __restrict__ name_end, uint64_t* __restrict__ seq_end) {
  __shared__ uint32_t s_wave[FQ_BLOCK / 64];
  const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
  if (blockIdx.x == 0 && threadIdx.x == 0 && nrec) {
    name_begin[0] = 0;
    if (virt) fq_emit(virt_k, hi - lo, nrec, name_begin, name_end, seq_end);
  }
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t j = t * FQ_BLOCK + threadIdx.x;
    uint32_t m = 0;
    if (j * FQ_LANE_BYTES < hi) m = fq_nl_mask(fq_load16(base16, j, lo, hi));
    const uint32_t c = (uint32_t)__popc(m);
    uint32_t inc = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t o = __shfl_up(inc, d);
      if (lane >= (uint32_t)d) inc += o;
    }
    if (lane == 63) s_wave[wid] = inc;
    __syncthreads();
    uint32_t wave_off = 0;
#pragma unroll
    for (uint32_t w = 0; w < FQ_BLOCK / 64; w++)
      if (w < wid) wave_off += s_wave[w];
    uint64_t k = tile_base[t] + wave_off + inc - c;
    while (m) {
      const uint32_t b = (uint32_t)__ffs((int)m) - 1u;
      m &= m - 1u;
      fq_emit(k++, j * FQ_LANE_BYTES + b - lo, nrec, name_begin, name_end, seq_end);
    }
    __syncthreads();
  }
}

// One lane per record.  kept[r] = 1 when the read stays, len[r] = its prepared length (0 when it goes); both get one
// more element, 0, so that their exclusive scans end in the totals.  st[0] = the longest prepared length,
// st[1] = the reads below min_len.
MUSC_KERNEL __launch_bounds__(256) void k_fq_records(const unsigned char* __restrict__ text, uint64_t nrec,
                                                    const uint64_t* __restrict__ name_begin, const uint64_t* __restrict__ name_end,
                                                    const uint64_t* __restrict__ seq_end, int32_t min_len, uint32_t max_len,
                                                    uint32_t* __restrict__ kept, uint64_t* __restrict__ len,
                                                    uint32_t* __restrict__ name_len, unsigned long long* __restrict__ st) {
  unsigned long long longest = 0, nshort = 0;
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r <= nrec; r += (uint64_t)gridDim.x * blockDim.x) {
    if (r == nrec) {
      kept[r] = 0;
      len[r] = 0;
      break;
    }
    const uint64_t b = name_begin[r], s = name_end[r] + 1;
    uint64_t e = name_end[r], q = seq_end[r];
    if (e > b && text[e - 1] == '\r') e--;  // dropCR: one trailing \r of the line, any other is data
    if (q > s && text[q - 1] == '\r') q--;
    const uint64_t raw = q - s;
    const bool keep = min_len <= 0 || raw >= (uint64_t)min_len;
    const uint64_t l = keep ? (raw < max_len ? raw : (uint64_t)max_len) : 0;
    kept[r] = keep ? 1u : 0u;
    len[r] = l;
    name_len[r] = (uint32_t)(e - b < 0xFFFFFFFFull ? e - b : 0xFFFFFFFFull);
    longest = l > longest ? l : longest;
    nshort += keep ? 0u : 1u;
  }
#pragma unroll
  for (int d = 32; d; d >>= 1) {
    const unsigned long long o = __shfl_xor(longest, d);
    longest = o > longest ? o : longest;
    nshort += __shfl_xor(nshort, d);
  }
  if ((threadIdx.x & 63u) == 0) {
    if (longest) atomicMax(st, longest);
    if (nshort) atomicAdd(st + 1, nshort);
  }
}

// every byte that is none of A C G T becomes X (cmd/muscato_prep_reads/main.go:33-44), four bytes at a time
DEV uint32_t fq_subx4(uint32_t v) {
  const uint32_t ok = fq_eq_bytes(v, 0x41414141u) | fq_eq_bytes(v, 0x43434343u) | fq_eq_bytes(v, 0x47474747u) |
                      fq_eq_bytes(v, 0x54545454u);
  const uint32_t m = (ok >> 7) * 0xFFu;  // 0xFF in the bytes that stay
  return (v & m) | (0x58585858u & ~m);
}
DEV unsigned char fq_subx1(unsigned char ch) { return (ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T') ? ch : (unsigned char)'X'; }

// the text's bytes [q, q + 4) as one dword (q + 4 <= nbytes): two aligned dword loads and a byte alignment where both
// lie inside the text, byte loads at its edges
DEV uint32_t fq_src_dword(const unsigned char* __restrict__ text, uint64_t nbytes, uint64_t q) {
  const unsigned char* p = text + q;
  const uint32_t sh = (uint32_t)(uintptr_t)p & 3u;
  if (sh == 0) return *reinterpret_cast<const uint32_t*>(p);
  if (q >= sh && q - sh + 8 <= nbytes) {
    const uint32_t* a = reinterpret_cast<const uint32_t*>(p - sh);
    return __builtin_amdgcn_alignbyte(a[1], a[0], sh);
  }
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// Sixteen lanes per record.  kidx / off = the exclusive scans of k_fq_records' kept / len (nrec + 1 elements).  Kept
// read i = kidx[r] gets its row of the span table and its prepared bytes at out + off[r]: the dwords of out that the
// read covers whole are assembled and stored aligned, the up to three bytes before and after them one lane each (the
// shape of k_results_render).  out is 4-byte aligned.
MUSC_KERNEL __launch_bounds__(256) void k_fq_gather(const unsigned char* __restrict__ text, uint64_t nbytes, uint64_t nrec,
                                                   const uint64_t* __restrict__ name_begin, const uint64_t* __restrict__ name_end,
                                                   const uint32_t* __restrict__ kidx, const uint64_t* __restrict__ off,
                                                   const uint32_t* __restrict__ name_len, unsigned char* __restrict__ out,
                                                   uint64_t* __restrict__ out_off, uint64_t* __restrict__ o_name_off,
                                                   uint64_t* __restrict__ o_seq_off, uint32_t* __restrict__ o_name_len,
                                                   uint32_t* __restrict__ o_seq_len) {
  const uint32_t sub = threadIdx.x & (FQ_GROUP - 1u);
  const uint64_t ngroups = (uint64_t)gridDim.x * (blockDim.x / FQ_GROUP);
  if (blockIdx.x == 0 && threadIdx.x == 0) out_off[kidx[nrec]] = off[nrec];
  for (uint64_t r = (uint64_t)blockIdx.x * (blockDim.x / FQ_GROUP) + threadIdx.x / FQ_GROUP; r < nrec; r += ngroups) {
    const uint32_t i = kidx[r];
    if (kidx[r + 1] == i) continue;  // not kept
    const uint64_t o = off[r], s = name_end[r] + 1;
    const uint32_t len = (uint32_t)(off[r + 1] - o);
    if (sub == 0) {
      out_off[i] = o;
      o_name_off[i] = name_begin[r];
      o_seq_off[i] = s;
      o_name_len[i] = name_len[r];
      o_seq_len[i] = len;
    }
    unsigned char* const p = out + o;
    const uint32_t mis = (4u - ((uint32_t)o & 3u)) & 3u;
    const uint32_t head = mis < len ? mis : len;
    const uint32_t nd = (len - head) >> 2;
    for (uint32_t d = sub; d < nd; d += FQ_GROUP) {
      const uint32_t k = head + 4 * d;
      *reinterpret_cast<uint32_t*>(p + k) = fq_subx4(fq_src_dword(text, nbytes, s + k));
    }
    const uint32_t tail0 = head + 4 * nd;
    if (sub < head) p[sub] = fq_subx1(text[s + sub]);
    else if (sub >= 4 && tail0 + (sub - 4) < len) p[tail0 + (sub - 4)] = fq_subx1(text[s + tail0 + (sub - 4)]);
  }
}
