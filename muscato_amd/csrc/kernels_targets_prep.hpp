// kernels_targets_prep.hpp -- target preparation on the GPU: records out of FASTA or id<TAB>sequence
// text, the reverse complements, the id text, and the framed writer.  Included by muscato_hip.hip behind
// kernels_db_text.hpp: the text is read with fq_load16 / fq_src_dword under their rule (bytes outside the text are
// never read), the newline count per tile is k_fq_count itself, and the CRC by parts is k_sz_decode's.
//
// Reference: cmd/muscato_prep_targets/main.go:48-213.  Lines are bufio.ScanLines' (kernels_db_text.hpp).
//
// Passes (every position, line and record number is 64-bit; no lane's work grows with a line, a record or a name):
//   k_fq_count, scan_u64   newlines per tile, tile bases (text_lines)
//   k_tp_lines             every newline number k at p: nl[k] = p, begin[k + 1] = p + 1; every tab at q in line k:
//                          ftab[k] <= q (atomicMin), ltab[k] >= q + 1 (atomicMax).  One tab: ftab + 1 == ltab.
//   k_tp_classify          one lane per line: the '\r' rule; text format: the stop flag into a global minimum;
//                          FASTA: the first empty line (a global minimum), the header flag, the line's bases
//   text format            k_tp_text_recs (lines below the stop line are the records), scan of len + 1
//   FASTA                  scans of the header flags and of the bases (S); k_tp_hl the header lines; k_tp_groups one
//                          lane per header: len = S[next header] - S[header]; scans of len > 0 and of len + 1;
//                          k_tp_compact the kept records
//   k_tp_seq               one lane per dword of the sequence text: its record by binary search in the offsets, its
//                          source line by binary search in S; whole dwords through fq_subx4, bytes where a dword
//                          straddles a line or a record; counts what subx changed
//   k_tp_rev               one lane per dword again, over the prepared forward lines: a dword of the complement is
//                          the forward dword byte-swapped and complemented in registers
//   k_tp_idlen, scan_u64   bytes of each record's id lines, their offsets
//   k_tp_ids               one lane per dword of the id text
//   k_sz_frame             one workgroup per chunk of 65 536 bytes: CRC-32C by parts from global memory, the eight
//                          header bytes, the data

#define TP_ST_STOP 0     // text format: the first stop line (~0: none)
#define TP_ST_EMPTY 1    // FASTA: the first empty line (~0: none)
#define TP_ST_SUBX 2     // bytes that subx changed
#define TP_ST_EXEMPT 3   // FASTA: the record that reaches the end of the input with bases (~0: none)
#define TP_ST_KEPT0 4    // FASTA: 1 when the lines in front of the first header form a record
#define TP_ST_WORDS 8

// tile_base = the exclusive scan of k_fq_count's counts; nlines = newlines + virt (k_dbt_lines).  ftab[] holds ~0 and
// ltab[] 0 on entry (text format), or both are null (FASTA).
MUSC_KERNEL __launch_bounds__(FQ_BLOCK) void k_tp_lines(const unsigned char* __restrict__ base16, uint64_t lo, uint64_t hi,
                                                       uint64_t ntiles, const uint64_t* __restrict__ tile_base,
                                                       uint64_t nlines, uint32_t virt, uint64_t* __restrict__ begin,
                                                       uint64_t* __restrict__ nl, unsigned long long* __restrict__ ftab,
                                                       unsigned long long* __restrict__ ltab) {
  __shared__ uint32_t s_wave[FQ_BLOCK / 64];
  const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
  if (blockIdx.x == 0 && threadIdx.x == 0 && nlines) {
    begin[0] = 0;
    if (virt) nl[nlines - 1] = hi - lo;
  }
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t j = t * FQ_BLOCK + threadIdx.x;
    uint32_t m = 0, tabs = 0;
    if (j * FQ_LANE_BYTES < hi) {
      const uint4 v = fq_load16(base16, j, lo, hi);
      m = fq_nl_mask(v);
      if (ftab) tabs = dbt_mask(v, 0x09090909u);
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
      if (k < nlines) {
        atomicMin(&ftab[k], (unsigned long long)(p0 + b));
        atomicMax(&ltab[k], (unsigned long long)(p0 + b + 1));
      }
    }
    uint64_t k = k0;
    while (m) {
      const uint32_t b = (uint32_t)__ffs((int)m) - 1u;
      m &= m - 1u;
      if (k < nlines) nl[k] = p0 + b;  // (k < newlines <= nlines: a guard, not a case)
      if (k + 1 < nlines) begin[k + 1] = p0 + b + 1;
      k++;
    }
    __syncthreads();
  }
}

// One lane per line: nl[k] becomes the line's end under the '\r' rule.  Text format: a stop line lowers st[TP_ST_STOP].
// FASTA: an empty line lowers st[TP_ST_EMPTY]; hdr[k] = 1 for a header, bases[k] = the bytes a data line adds to its
// record; both get one more element, 0, so that their exclusive scans end in the totals.
template <bool FASTA>
MUSC_KERNEL __launch_bounds__(256) void k_tp_classify(const unsigned char* __restrict__ text, uint64_t nbytes, uint64_t nlines,
                                                     const uint64_t* __restrict__ begin, uint64_t* __restrict__ nl,
                                                     const unsigned long long* __restrict__ ftab,
                                                     const unsigned long long* __restrict__ ltab, uint64_t* __restrict__ hdr,
                                                     uint64_t* __restrict__ bases, unsigned long long* __restrict__ st) {
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k <= nlines; k += (uint64_t)gridDim.x * blockDim.x) {
    if (k == nlines) {
      if (FASTA) hdr[k] = 0, bases[k] = 0;
      break;
    }
    const uint64_t b = begin[k];
    uint64_t e = nl[k];
    if (e > nbytes) e = nbytes;  // (every line has its newline or the text's end: a guard, not a case)
    if (e < b) e = b;
    if (e > b && text[e - 1] == '\r') e--;  // dropCR
    nl[k] = e;
    const uint64_t len = e - b;
    if (FASTA) {
      if (len == 0) atomicMin(st + TP_ST_EMPTY, (unsigned long long)k);
      const bool h = len != 0 && text[b] == '>';
      hdr[k] = h ? 1u : 0u;
      bases[k] = h ? 0u : len;
    } else {
      const unsigned long long ft = ftab[k];
      if (len == 0 || ft == ~0ull || ft + 1 != ltab[k]) atomicMin(st + TP_ST_STOP, (unsigned long long)k);
    }
  }
}

// Text format, one lane per record = line k < nrec: a[k] = the sequence's length + 1 (a[nrec] = 0), and in place
// ftab[k] -> the name's length, ltab[k] -> where the sequence begins.  The name begins at begin[k].
MUSC_KERNEL __launch_bounds__(256) void k_tp_text_recs(uint64_t nrec, const uint64_t* __restrict__ begin, const uint64_t* __restrict__ eol,
                                                      unsigned long long* __restrict__ ftab, unsigned long long* __restrict__ ltab,
                                                      uint64_t* __restrict__ a) {
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k <= nrec; k += (uint64_t)gridDim.x * blockDim.x) {
    if (k == nrec) {
      a[k] = 0;
      break;
    }
    const uint64_t ft = ftab[k];
    a[k] = eol[k] - ft;  // (the tab lies inside the line: eol > ft)
    ltab[k] = ft + 1;
    ftab[k] = ft - begin[k];
  }
}

// FASTA.  hs = the exclusive scan of the header flags (nlines + 1 elements).  hl[g], g = 1 .. nhdr: the line of header
// g; hl[0] = 0 and hl[nhdr + 1] = nlines, so that group g -- the lines in front of the first header for g = 0 -- holds
// the bases S[hl[g + 1]] - S[hl[g]] (a header adds none).
MUSC_KERNEL __launch_bounds__(256) void k_tp_hl(uint64_t nlines, const uint64_t* __restrict__ hs, uint64_t ngroups, uint64_t* __restrict__ hl) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    hl[0] = 0;
    hl[ngroups] = nlines;
  }
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < nlines; k += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t g = hs[k];
    if (hs[k + 1] != g && g + 1 < ngroups) hl[g + 1] = k;
  }
}

// One lane per group: kept[g] = 1 and a[g] = len + 1 for a group with bases, 0 and 0 otherwise and for g = ngroups.
MUSC_KERNEL __launch_bounds__(256) void k_tp_groups(uint64_t ngroups, const uint64_t* __restrict__ hl, const uint64_t* __restrict__ S,
                                                   uint64_t* __restrict__ kept, uint64_t* __restrict__ a) {
  for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g <= ngroups; g += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t len = 0;
    if (g < ngroups) len = S[hl[g + 1]] - S[hl[g]];
    kept[g] = len ? 1u : 0u;
    a[g] = len ? len + 1 : 0u;
  }
}

// One lane per group.  kidx / fg = the exclusive scans of kept / a.  Kept group g is record t = kidx[g]: its offset,
// the number of its first base among all bases (its source in S), its name (the header line; none for group 0).
MUSC_KERNEL __launch_bounds__(256) void k_tp_compact(uint64_t ngroups, const uint64_t* __restrict__ kidx, const uint64_t* __restrict__ fg,
                                                    const uint64_t* __restrict__ hl, const uint64_t* __restrict__ S,
                                                    const uint64_t* __restrict__ begin, const uint64_t* __restrict__ eol,
                                                    uint64_t* __restrict__ fo, uint64_t* __restrict__ src0,
                                                    uint64_t* __restrict__ name_b, uint64_t* __restrict__ name_len,
                                                    unsigned long long* __restrict__ st) {
  for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g <= ngroups; g += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t t = kidx[g];
    if (g == ngroups) {
      fo[t] = fg[g];
      break;
    }
    if (kidx[g + 1] == t) continue;  // no bases: dropped
    const uint64_t h = hl[g];
    fo[t] = fg[g];
    src0[t] = S[h];
    name_b[t] = g ? begin[h] : 0;
    name_len[t] = g ? eol[h] - begin[h] : 0;
    if (g == 0) st[TP_ST_KEPT0] = 1;
    if (g + 1 == ngroups) st[TP_ST_EXEMPT] = t;  // it reaches the end of the input with bases: not substituted
  }
}

// the largest i in [0, n) with a[i] * mult <= v (a[0] * mult <= v; a does not fall)
DEV uint64_t tp_find(const uint64_t* __restrict__ a, uint64_t n, uint64_t mult, uint64_t v) {
  uint64_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (a[mid] * mult <= v) lo = mid; else hi = mid;
  }
  return lo;
}

// where byte j of record t stands in the text, and how many bytes from there on are consecutive in the text (room).
// Text format: src0[t] is where the sequence begins.  FASTA: src0[t] + j is the number of the base among all bases,
// and the line that holds it is the last L with S[L] <= that number (S[L + 1] is greater: the line has bases).
template <bool FASTA>
DEV uint64_t tp_src(const uint64_t* __restrict__ src0, uint64_t t, uint64_t j, const uint64_t* __restrict__ S,
                    const uint64_t* __restrict__ begin, uint64_t nlines, uint64_t* room) {
  if (!FASTA) {
    *room = ~0ull;
    return src0[t] + j;
  }
  const uint64_t x = src0[t] + j;
  const uint64_t L = tp_find(S, nlines, 1, x);
  *room = S[L + 1] - x;
  return begin[L] + (x - S[L]);
}

// bytes of v that differ from w
DEV uint32_t tp_diff_bytes(uint32_t v, uint32_t w) { return 4u - (uint32_t)__popc(fq_eq_bytes(v ^ w, 0u)); }

// One lane per dword of the sequence text (total bytes, out 4-byte aligned with room for the last whole dword).
// fo = the nrec + 1 offsets of the records (the scan of len + 1); mult = 2 with reverse complements, whose bytes this
// kernel leaves alone: record t's forward line is at mult * fo[t], its newline behind it, and with mult = 2 the
// complement and a second newline follow.  st[TP_ST_SUBX] += the bytes subx changed.
template <bool FASTA>
MUSC_KERNEL __launch_bounds__(256) void k_tp_seq(const unsigned char* __restrict__ text, uint64_t nbytes, uint64_t nrec,
                                                const uint64_t* __restrict__ fo, const uint64_t* __restrict__ src0,
                                                const uint64_t* __restrict__ S, const uint64_t* __restrict__ begin, uint64_t nlines,
                                                uint64_t mult, uint64_t total, unsigned char* __restrict__ out,
                                                unsigned long long* __restrict__ st) {
  const uint64_t exempt = FASTA ? st[TP_ST_EXEMPT] : ~0ull;
  const uint64_t nwords = (total + 3) / 4;
  unsigned long long nsub = 0;
  for (uint64_t w0 = (uint64_t)blockIdx.x * blockDim.x; w0 < nwords; w0 += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t w = w0 + threadIdx.x;
    if (w < nwords) {
      const uint64_t p0 = 4 * w;
      uint64_t t = tp_find(fo, nrec, mult, p0);
      uint64_t r = p0 - mult * fo[t], len = fo[t + 1] - fo[t] - 1;
      uint64_t room = 0;
      bool whole = false;
      if (r + 4 <= len) {  // four bytes of one forward line: one dword when they are consecutive in the text
        const uint64_t q = tp_src<FASTA>(src0, t, r, S, begin, nlines, &room);
        if (room >= 4) {
          const uint32_t v = fq_src_dword(text, nbytes, q);
          const uint32_t s = t == exempt ? v : fq_subx4(v);
          nsub += tp_diff_bytes(v, s);
          *reinterpret_cast<uint32_t*>(out + p0) = s;
          whole = true;
        }
      }
      if (!whole) {
        for (uint32_t b = 0; b < 4; b++) {
          const uint64_t p = p0 + b;
          if (p >= total) break;
          while (p >= mult * fo[t + 1]) t++;  // (a record has a byte at least: four steps at most)
          r = p - mult * fo[t];
          len = fo[t + 1] - fo[t] - 1;
          if (r < len) {
            const unsigned char ch = text[tp_src<FASTA>(src0, t, r, S, begin, nlines, &room)];
            const unsigned char s = t == exempt ? ch : fq_subx1(ch);
            nsub += s != ch ? 1u : 0u;
            out[p] = s;
          } else if (r == len || r == 2 * len + 1) {
            out[p] = '\n';
          }
        }
      }
    }
  }
  block_add_u64(nsub, st + TP_ST_SUBX);
}

// A T C G X -> T A G C X, any other byte -> 0 (cmd/muscato_prep_targets/main.go:48-66), four bytes at a time
DEV uint32_t tp_comp4(uint32_t v) {
  const uint32_t a = (fq_eq_bytes(v, 0x41414141u) >> 7) * 0xFFu, t = (fq_eq_bytes(v, 0x54545454u) >> 7) * 0xFFu;
  const uint32_t c = (fq_eq_bytes(v, 0x43434343u) >> 7) * 0xFFu, g = (fq_eq_bytes(v, 0x47474747u) >> 7) * 0xFFu;
  const uint32_t x = (fq_eq_bytes(v, 0x58585858u) >> 7) * 0xFFu;
  return (a & 0x54545454u) | (t & 0x41414141u) | (c & 0x47474747u) | (g & 0x43434343u) | (x & 0x58585858u);
}
DEV unsigned char tp_comp1(unsigned char ch) {
  return ch == 'A' ? 'T' : ch == 'T' ? 'A' : ch == 'C' ? 'G' : ch == 'G' ? 'C' : ch == 'X' ? 'X' : 0;
}

// One lane per dword of the sequence text again, after k_tp_seq: the complements, from the forward lines in `out`
// itself.  Byte i of record t's complement is the complement of byte len - 1 - i of its forward line, so an aligned
// dword of the complement is a (mostly unaligned) dword of the forward line, byte-swapped.  Every byte this kernel
// reads is a forward byte and every byte it writes a complement byte: the aligned loads of fq_src_dword may carry
// neighbouring bytes that another lane writes, which are shifted out.
MUSC_KERNEL __launch_bounds__(256) void k_tp_rev(uint64_t nrec, const uint64_t* __restrict__ fo, uint64_t total, unsigned char* out) {
  const uint64_t nwords = (total + 3) / 4;
  for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < nwords; w += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t p0 = 4 * w;
    uint64_t t = tp_find(fo, nrec, 2, p0);
    uint64_t base = 2 * fo[t], len = fo[t + 1] - fo[t] - 1;
    uint64_t r = p0 - base;
    if (r > len && r - len - 1 + 4 <= len) {
      const uint64_t i = r - len - 1;  // complement bytes [i, i + 4) = forward bytes [len - 4 - i, len - i), reversed
      const uint32_t v = fq_src_dword(out, total, base + (len - 4 - i));
      *reinterpret_cast<uint32_t*>(out + p0) = tp_comp4(__builtin_bswap32(v));
      continue;
    }
    for (uint32_t b = 0; b < 4; b++) {
      const uint64_t p = p0 + b;
      if (p >= total) break;
      while (p >= 2 * fo[t + 1]) t++;
      base = 2 * fo[t];
      len = fo[t + 1] - fo[t] - 1;
      r = p - base;
      if (r > len && r - len - 1 < len) out[p] = tp_comp1(out[base + (len - 1 - (r - len - 1))]);
    }
  }
}

// One lane per record: idb[t] = the bytes of its id lines (idb[nrec] = 0).
MUSC_KERNEL __launch_bounds__(256) void k_tp_idlen(uint64_t nrec, const uint64_t* __restrict__ fo, const uint64_t* __restrict__ name_len,
                                                  int rev, uint64_t* __restrict__ idb) {
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t <= nrec; t += (uint64_t)gridDim.x * blockDim.x)
    idb[t] = t < nrec ? musc_tp::id_rec_len(name_len[t], fo[t + 1] - fo[t] - 1, rev) : 0;
}

// digit number d (0 = the last) of v
DEV unsigned char tp_digit(uint64_t v, uint32_t d) {
  for (; d; d--) v /= 10;
  return (unsigned char)('0' + v % 10);
}

// One lane per dword of the id text: ioff = the scan of k_tp_idlen.  A dword that lies inside a name is one dword of
// the text; every other byte is worked out from its place in the line "%011d \t name [_r] \t len \n".
MUSC_KERNEL __launch_bounds__(256) void k_tp_ids(const unsigned char* __restrict__ text, uint64_t nbytes, uint64_t nrec,
                                                const uint64_t* __restrict__ fo, const uint64_t* __restrict__ ioff,
                                                const uint64_t* __restrict__ name_b, const uint64_t* __restrict__ name_len,
                                                int rev, uint64_t total, unsigned char* __restrict__ out) {
  const uint64_t nwords = (total + 3) / 4;
  for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < nwords; w += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t p0 = 4 * w;
    uint64_t t = tp_find(ioff, nrec, 1, p0);
    uint32_t v = 0;
    for (uint32_t b = 0; b < 4; b++) {
      const uint64_t p = p0 + b;
      if (p >= total) break;
      while (p >= ioff[t + 1]) t++;  // (an id line has fifteen bytes at least: one step at most)
      const uint64_t nlen = name_len[t], len = fo[t + 1] - fo[t] - 1;
      const uint64_t line0 = musc_tp::id_line_len(nlen, len, 0);
      uint64_t r = p - ioff[t];
      const uint32_t strand = rev && r >= line0 ? 1u : 0u;
      if (strand) r -= line0;
      const uint64_t name_end = musc_tp::ID_NUM_DIGITS + 1 + nlen;
      if (b == 0 && r >= musc_tp::ID_NUM_DIGITS + 1 && r + 4 <= name_end) {
        v = fq_src_dword(text, nbytes, name_b[t] + (r - (musc_tp::ID_NUM_DIGITS + 1)));
        break;
      }
      const uint64_t tab2 = name_end + 2 * strand;
      const uint32_t nd = musc_tp::dec_digits(len);
      unsigned char ch;
      if (r < musc_tp::ID_NUM_DIGITS) ch = tp_digit((rev ? 2 * t : t) + strand, musc_tp::ID_NUM_DIGITS - 1 - (uint32_t)r);
      else if (r == musc_tp::ID_NUM_DIGITS) ch = '\t';
      else if (r < name_end) ch = text[name_b[t] + (r - (musc_tp::ID_NUM_DIGITS + 1))];
      else if (r < tab2) ch = r == name_end ? '_' : 'r';
      else if (r == tab2) ch = '\t';
      else if (r <= tab2 + nd) ch = tp_digit(len, nd - (uint32_t)(r - tab2));
      else ch = '\n';
      v |= (uint32_t)ch << (8 * b);
    }
    if (p0 + 4 <= total) {
      *reinterpret_cast<uint32_t*>(out + p0) = v;
    } else {
      for (uint32_t b = 0; p0 + b < total; b++) out[p0 + b] = (unsigned char)(v >> (8 * b));
    }
  }
}

// One workgroup per chunk of `src` (nbytes > 0 bytes at any alignment): chunk i is src[65536 i, ...), at most 65 536
// bytes.  CRC-32C by parts as in k_sz_decode, the data read from global memory: every lane takes a slice of an odd
// number of dwords, and the slices' CRCs are joined by multiplication by x^(8 bytes behind the slice) mod P.  Then the
// chunk's eight header bytes and its data go to dst + 10 + 65544 i (dst at any alignment): whole dwords where the
// address allows, bytes at the edges.  The workgroup of chunk 0 writes the stream identifier.
#define TPF_BLOCK 256u
MUSC_KERNEL __launch_bounds__(TPF_BLOCK) void k_sz_frame(const unsigned char* __restrict__ src, uint64_t nbytes, uint64_t nchunks,
                                                        const uint32_t* __restrict__ x2n, unsigned char* __restrict__ dst) {
  __shared__ uint32_t s_tab[256];
  __shared__ uint32_t s_red[TPF_BLOCK / 64];
  const uint32_t tid = threadIdx.x;
  sz_crc_table(s_tab, tid);
  if (blockIdx.x == 0 && tid < 10)  // ff 06 00 00 "sNaPpY", out of two constants (no table in memory)
    dst[tid] = tid < 8 ? (unsigned char)(0x50614e73000006ffull >> (8 * tid)) : (unsigned char)(0x5970u >> (8 * (tid - 8)));
  __syncthreads();
  for (uint64_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    const uint64_t off = ch * musc_tp::SZ_CHUNK;
    const uint32_t ulen = musc_tp::sz_chunk_len(nbytes, ch);
    const uint32_t c = sz_crc_slice(ulen, tid, TPF_BLOCK, s_tab, x2n, [&](uint32_t i) { return fq_src_dword(src, nbytes, off + i); },
                                    [&](uint32_t i) { return (uint32_t)src[off + i]; });
    const uint32_t masked = sz_crc_join(c, s_red, tid);
    __syncthreads();  // (s_red is written again for the next chunk)
    unsigned char* const h = dst + musc_tp::sz_chunk_pos(ch);
    if (tid < 8) {
      const uint32_t len = ulen + 4;
      h[tid] = tid == 0 ? (unsigned char)0x01 : tid < 4 ? (unsigned char)(len >> (8 * (tid - 1))) : (unsigned char)(masked >> (8 * (tid - 4)));
    }
    unsigned char* const d = h + musc_tp::SZ_HEAD;
    const uint32_t mis = (4u - ((uint32_t)(uintptr_t)d & 3u)) & 3u;
    const uint32_t head = mis < ulen ? mis : ulen;
    const uint32_t nd = (ulen - head) >> 2;
    for (uint32_t k = tid; k < nd; k += TPF_BLOCK) {
      const uint32_t q = head + 4 * k;
      *reinterpret_cast<uint32_t*>(d + q) = fq_src_dword(src, nbytes, off + q);
    }
    const uint32_t tail0 = head + 4 * nd;
    if (tid < head) d[tid] = src[off + tid];
    else if (tid >= 4 && tid < 8 && tail0 + (tid - 4) < ulen) d[tail0 + (tid - 4)] = src[off + tail0 + (tid - 4)];
  }
}
