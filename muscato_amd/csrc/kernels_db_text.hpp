// kernels_db_text.hpp -- the gene file's text on the GPU: lines, the cut at the first tab, and the 2-bit planes
// (DESIGN.md 21).  Included by muscato_hip.hip behind kernels_fastq.hpp: the text is read with fq_load16 under its
// alignment rule (a lane's 16 bytes are aligned in the address space; bytes outside the text are never read), and the
// newline count per 4 096-byte tile is k_fq_count itself.
//
// Reference: the gene file is read with bufio.Scanner's ScanLines (cmd/muscato_screen/main.go:408-452): a line ends at
// '\n', one trailing '\r' is dropped, a last line without '\n' is a line, and there is no empty line behind a final
// '\n'; the target is the line up to its first tab.  A '\r' that the cut leaves in front of a tab is data.
//
// Passes (positions and line numbers are 64-bit):
//   k_fq_count        newlines per tile
//   scan_u64          tile bases
//   k_dbt_lines       the same load again: newline number k at p gives end[k] <= p and begin[k + 1] = p + 1; a tab at q
//                     in line k gives end[k] <= q.  end[] starts at ~0 and only ever sees atomicMin, so the line's end is
//                     its first tab or its newline, whoever comes first, and no lane walks a long line.
//   k_dbt_lengths     one lane per line: the '\r' rule, the target's length
//   scan_u64          seq_off
//   k_pack_db_spans   one lane per word of 16 bases: both planes, the X flag, the census of odd bytes

// bit b set where byte b of the 16 equals the byte replicated in c4 (fq_nl_mask for any byte)
DEV uint32_t dbt_mask(uint4 v, uint32_t c4) {
  const uint32_t a = ((fq_eq_bytes(v.x, c4) >> 7) * 0x00204081u) >> 21 & 0xFu;
  const uint32_t b = ((fq_eq_bytes(v.y, c4) >> 7) * 0x00204081u) >> 21 & 0xFu;
  const uint32_t c = ((fq_eq_bytes(v.z, c4) >> 7) * 0x00204081u) >> 21 & 0xFu;
  const uint32_t d = ((fq_eq_bytes(v.w, c4) >> 7) * 0x00204081u) >> 21 & 0xFu;
  return a | (b << 4) | (c << 8) | (d << 12);
}

// tile_base = the exclusive scan of k_fq_count's counts; nlines = newlines + virt.  virt != 0: the text does not end in
// '\n' and its last line ends at the text's length.  end[] holds ~0 on entry.
MUSC_KERNEL __launch_bounds__(FQ_BLOCK) void k_dbt_lines(const unsigned char* __restrict__ base16, uint64_t lo, uint64_t hi,
                                                        uint64_t ntiles, const uint64_t* __restrict__ tile_base,
                                                        uint64_t nlines, uint32_t virt, uint64_t* __restrict__ begin,
                                                        unsigned long long* __restrict__ end) {
  __shared__ uint32_t s_wave[FQ_BLOCK / 64];
  const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
  if (blockIdx.x == 0 && threadIdx.x == 0 && nlines) {
    begin[0] = 0;
    if (virt) atomicMin(&end[nlines - 1], (unsigned long long)(hi - lo));
  }
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t j = t * FQ_BLOCK + threadIdx.x;
    uint32_t m = 0, tabs = 0;
    if (j * FQ_LANE_BYTES < hi) {
      const uint4 v = fq_load16(base16, j, lo, hi);
      m = fq_nl_mask(v);
      tabs = dbt_mask(v, 0x09090909u);
      // (bytes outside the text come back as 0: neither)
    }
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
    const uint64_t k0 = tile_base[t] + wave_off + inc - c;  // newlines in front of this lane's bytes = its first line
    const uint64_t p0 = j * FQ_LANE_BYTES - lo;             // (wraps for the bytes in front of the text: never used)
    while (tabs) {
      const uint32_t b = (uint32_t)__ffs((int)tabs) - 1u;
      tabs &= tabs - 1u;
      const uint64_t k = k0 + (uint32_t)__popc(m & ((1u << b) - 1u));
      if (k < nlines) atomicMin(&end[k], (unsigned long long)(p0 + b));
    }
    uint64_t k = k0;
    while (m) {
      const uint32_t b = (uint32_t)__ffs((int)m) - 1u;
      m &= m - 1u;
      atomicMin(&end[k], (unsigned long long)(p0 + b));  // (k < newlines <= nlines)
      if (k + 1 < nlines) begin[k + 1] = p0 + b + 1;
      k++;
    }
    __syncthreads();
  }
}

// One lane per line.  len[k] = the target's length; len[nlines] = 0, so that the exclusive scan ends in the total.
MUSC_KERNEL __launch_bounds__(256) void k_dbt_lengths(const unsigned char* __restrict__ text, uint64_t nbytes, uint64_t nlines,
                                                     const uint64_t* __restrict__ begin, const unsigned long long* __restrict__ end,
                                                     uint64_t* __restrict__ len) {
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k <= nlines; k += (uint64_t)gridDim.x * blockDim.x) {
    if (k == nlines) {
      len[k] = 0;
      break;
    }
    const uint64_t b = begin[k];
    uint64_t e = end[k];
    if (e > nbytes) e = nbytes;  // (every line has its newline or the text's end: a guard, not a case)
    const bool cut = e < nbytes && text[e] == '\t';
    if (!cut && e > b && text[e - 1] == '\r') e--;  // dropCR: one trailing \r of the line; in front of a tab it is data
    len[k] = e - b;
  }
}

// One lane per word of 16 bases.  The targets a word covers are found by binary search in seq_off (a word may hold
// several short or empty ones); every base comes from its line's span, begin[t] + (base - seq_off[t]).  Writes both
// planes and raises has_x as k_pack_db_ascii does; census[0] += the bytes that are none of A C G T X, census[1] = the
// lowest target number that holds one (~0 on entry).
MUSC_KERNEL __launch_bounds__(256) void k_pack_db_spans(const unsigned char* __restrict__ text, uint64_t nbytes,
                                                       const uint64_t* __restrict__ begin, const uint64_t* __restrict__ seq_off,
                                                       uint64_t nseq, uint64_t nbases, uint32_t* __restrict__ db2,
                                                       uint32_t* __restrict__ dbm2, uint64_t nwords, uint32_t* __restrict__ has_x,
                                                       unsigned long long* __restrict__ census) {
  const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long nodd = 0, first = ~0ull;
  if (w < nwords) {
    const uint64_t b0 = w * 16;
    // t = the last target with seq_off[t] <= b0: the one that holds base b0 (b0 < nbases = seq_off[nseq])
    uint64_t lo = 0, hi = nseq;
    while (hi - lo > 1) {
      const uint64_t mid = lo + (hi - lo) / 2;
      if (seq_off[mid] <= b0) lo = mid; else hi = mid;
    }
    uint64_t t = lo, t_off = seq_off[t], t_end = seq_off[t + 1], t_begin = begin[t];
    uint32_t v = 0, mv = 0;
    if (b0 + 16 <= t_end) {  // the whole word in one target: four dwords of its span
      const uint64_t q = t_begin + (b0 - t_off);
#pragma unroll
      for (uint32_t d = 0; d < 4; d++) {
        uint32_t x = fq_src_dword(text, nbytes, q + 4 * d);
#pragma unroll
        for (uint32_t j = 0; j < 4; j++, x >>= 8) {
          const unsigned char ch = (unsigned char)(x & 0xFFu);
          uint32_t isx;
          const uint32_t code = ascii_code(ch, &isx);
          v |= code << (2 * (4 * d + j));
          mv |= isx << (2 * (4 * d + j));
          nodd += (isx && ch != 'X') ? 1u : 0u;
        }
      }
      if (nodd) first = t;
    } else {
      for (uint32_t j = 0; j < 16; j++) {
        const uint64_t b = b0 + j;
        if (b >= nbases) break;
        while (b >= t_end) {  // (empty targets are stepped over)
          t++;
          t_off = t_end;
          t_end = seq_off[t + 1];
          t_begin = begin[t];
        }
        const unsigned char ch = text[t_begin + (b - t_off)];
        uint32_t isx;
        const uint32_t code = ascii_code(ch, &isx);
        v |= code << (2 * j);
        mv |= isx << (2 * j);
        if (isx && ch != 'X') {
          nodd++;
          if (first == ~0ull) first = t;
        }
      }
    }
    db2[w] = v;
    dbm2[w] = mv;
    if (mv) atomicOr(has_x, 1u);
  }
  if (first != ~0ull) atomicMin(census + 1, first);
  block_add_u64(nodd, census);
}
