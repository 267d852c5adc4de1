// kernels_side.hpp -- the nonmatch FASTQ and the two stats files from the resident tuples.
// Part of libmuscato_hip.so: included by muscato_hip.hip (one translation unit), after kernels_results.hpp.
//
// Reference: cmd/muscato_nonmatch/main.go:95-114 (the reads without a results line, as FASTQ records),
// cmd/muscato/main.go:94-150 + cmd/muscato_genestats/main.go (`sort -k5`, runs of column 5 counted) and
// cmd/muscato_readstats/main.go (runs of column 8, the set of column 5).  Everything those programs read back from
// results.txt is on the device already: the kept, ordered tuples give (read, gene) of every line, the read records
// the sequences, the gene text the names and the read text count and names.
//
// Every text is a list of records with 64-bit byte offsets, rendered one wave per record (per element for readstats)
// the way k_results_render renders a line (wave_id, wave_store: kernels_results.hpp).  No LDS, no atomics but the
// per-name tuple counter, nothing waits on another workgroup.
#pragma once

#define SIDE_NONE 0xFFFFFFFFu  // a read that belongs to no readstats run

DEV bool side_isspace(uint32_t b) { return b == 0x20u || b - 9u <= 4u; }  // C isspace in the C locale

struct SideData {
  const uint32_t* rd;
  const uint32_t* rdm;     // null: no read holds an X
  const char* ttext;       // every read's count\tnames
  const uint64_t* toff;
  const uint4* tok;        // per read: count span (x = first byte within the tail, y = bytes), token span (z, w)
  const char* gtext;       // every gene's name\tlen
  const uint64_t* goff;
  const uint2* names;      // per name rank: x = a gene with that name, y = bytes of the name
  uint64_t nreads;
  uint32_t nseq, nnames;
  int rw;
};

// ---- tokens -------------------------------------------------------------------------------------------------------
// The first two whitespace-separated fields of each read's tail: its count and the first of its names (bytes.Fields).
MUSC_KERNEL __launch_bounds__(256) void k_side_tokens(const char* __restrict__ ttext, const uint64_t* __restrict__ toff, uint64_t nreads,
                                                     uint4* __restrict__ tok, uint32_t* __restrict__ flag) {
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < nreads; r += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t t0 = toff[r], T64 = toff[r + 1] - t0;
    uint4 t = make_uint4(0u, 0u, 0u, 0u);
    if (T64 > 0xFFFFFFFFull) {
      atomicOr(flag, 1u);  // a tail that 32-bit spans cannot describe
    } else {
      const unsigned char* const p = reinterpret_cast<const unsigned char*>(ttext) + t0;
      const uint32_t T = (uint32_t)T64;
      uint32_t i = 0;
      while (i < T && side_isspace(p[i])) i++;
      t.x = i;
      while (i < T && !side_isspace(p[i])) i++;
      t.y = i - t.x;
      while (i < T && side_isspace(p[i])) i++;
      t.z = i;
      while (i < T && !side_isspace(p[i])) i++;
      t.w = i - t.z;
    }
    tok[r] = t;
  }
}

// ---- mark and count -----------------------------------------------------------------------------------------------
// matched[r] = read r has a kept tuple (a plain store: every writer stores 1); cnt[name rank] += 1 per kept tuple
MUSC_KERNEL __launch_bounds__(256) void k_side_mark(const uint4* __restrict__ hits, uint64_t m, const uint32_t* __restrict__ nrank,
                                                   uint64_t nreads, uint32_t nseq, uint32_t nnames, uint32_t* __restrict__ matched,
                                                   uint32_t* __restrict__ cnt, uint32_t* __restrict__ flag) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint4 h = hits[i];
    const uint32_t k = (uint64_t)h.x < nreads && h.y < nseq ? nrank[h.y] : SIDE_NONE;
    if (k >= nnames) {
      atomicOr(flag, 1u);
      continue;
    }
    matched[h.x] = 1u;
    atomicAdd(&cnt[k], 1u);
  }
}

// The records of a text are the items with flag set: idx[j] = the j-th of them, off[j] = its first byte (excl = the
// exclusive scan of flag, lenscan that of the lengths, both over n + 1 items of which the last is empty).
MUSC_KERNEL __launch_bounds__(256) void k_side_compact(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ excl,
                                                      const uint64_t* __restrict__ lenscan, uint64_t n, uint32_t* __restrict__ idx,
                                                      uint64_t* __restrict__ off) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += (uint64_t)gridDim.x * blockDim.x) {
    if (i == n) {
      if (off) off[excl[n]] = lenscan[n];
    } else if (flag[i]) {
      idx[excl[i]] = (uint32_t)i;
      if (off) off[excl[i]] = lenscan[i];
    }
  }
}

// ---- nonmatch -----------------------------------------------------------------------------------------------------
// token#count \n SEQ \n + \n !...! \n
struct SideNm {
  uint32_t L, TL, CL, read_x;
  uint64_t rrec, tokp, cntp;  // first word of the read's record; first byte of the token, of the count, in the text
  DEV uint64_t total() const { return (uint64_t)TL + 1 + CL + 1 + L + 3 + L + 1; }
};

DEV SideNm side_nm(const SideData& D, uint32_t r) {
  SideNm s;
  s.rrec = (uint64_t)r * (uint64_t)D.rw;
  const uint32_t lw = D.rd[s.rrec + (uint64_t)(D.rw - 1)];
  s.L = lw & 0xFFFFu;
  s.read_x = (lw & READ_HAS_X) && D.rdm;
  const uint4 t = D.tok[r];
  const uint64_t t0 = D.toff[r];
  s.CL = t.y;
  s.TL = t.w;
  s.cntp = t0 + t.x;
  s.tokp = t0 + t.z;
  return s;
}

// byte k of a record, k < s.total(): one text byte and one plane word are loaded whatever piece k is in (a clamped
// place inside the tail, inside the record), as in res_line_byte
DEV uint32_t side_nm_byte(const SideData& D, const SideNm& s, uint64_t k) {
  const uint64_t s_cnt = (uint64_t)s.TL + 1, s_seq = s_cnt + s.CL + 1, s_plus = s_seq + s.L + 1, s_q = s_plus + 2;
  const bool in_tok = k < s.TL, in_cnt = k >= s_cnt && k - s_cnt < s.CL, in_seq = k >= s_seq && k - s_seq < s.L,
             in_q = k >= s_q && k - s_q < s.L;
  const uint32_t tb = (unsigned char)D.ttext[in_tok ? s.tokp + k : s.cntp + (in_cnt ? k - s_cnt : 0ull)];
  const uint64_t b = s.rrec * 16ull + (in_seq ? k - s_seq : 0ull);
  const uint32_t sh = 2u * ((uint32_t)b & 15u);
  const uint32_t code = (D.rd[b >> 4] >> sh) & 3u;
  const uint32_t isx = s.read_x ? (D.rdm[b >> 4] >> sh) & 1u : 0u;
  if (in_tok || in_cnt) return tb;
  if (in_seq) return res_base_char(code, isx);
  if (in_q) return (uint32_t)'!';
  if (k == s.TL) return (uint32_t)'#';
  if (k == s_plus) return (uint32_t)'+';
  return (uint32_t)'\n';
}

// flag[i] = read i is a nonmatch record, len[i] = its bytes (0 when it is skipped: matched, or no token); item nreads is empty
MUSC_KERNEL __launch_bounds__(256) void k_side_nm_len(SideData D, const uint32_t* __restrict__ matched, uint32_t* __restrict__ flag,
                                                     uint64_t* __restrict__ len) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= D.nreads; i += (uint64_t)gridDim.x * blockDim.x) {
    bool keep = false;
    uint64_t l = 0;
    if (i < D.nreads && !matched[i] && D.tok[i].w) {
      keep = true;
      l = side_nm(D, (uint32_t)i).total();
    }
    flag[i] = keep;
    len[i] = l;
  }
}

// records [r0, r1) into `out`, record j at byte off[j] - off[r0]; one wave per record.  The read index and the record's
// length are checked again before anything is loaded through them: a record that fails is not rendered and fails the
// call through *flag (a plain store: every writer stores the same word).
MUSC_KERNEL __launch_bounds__(256) void k_side_nm_render(const uint32_t* __restrict__ idx, const uint64_t* __restrict__ off, uint64_t r0,
                                                        uint64_t r1, SideData D, unsigned char* __restrict__ out,
                                                        uint32_t* __restrict__ flag) {
  const WaveId w = wave_id(threadIdx.x, blockIdx.x, blockDim.x, gridDim.x);
  const uint64_t base = off[r0];
  for (uint64_t j = r0 + w.wave; j < r1; j += w.nwaves) {
    const uint32_t r = __builtin_amdgcn_readfirstlane(idx[j]);
    if ((uint64_t)r >= D.nreads) {
      if (w.lane == 0) *flag = 1u;
      continue;
    }
    const SideNm s = side_nm(D, r);
    const uint64_t total = off[j + 1] - off[j];
    if (total != s.total() || s.TL == 0u) {
      if (w.lane == 0) *flag = 1u;
      continue;
    }
    wave_store(out + (off[j] - base), total, w.lane, [&](uint64_t k) { return side_nm_byte(D, s, k); });
  }
}

// ---- genestats ----------------------------------------------------------------------------------------------------
// name \t N \t \n per name rank with a kept tuple
MUSC_KERNEL __launch_bounds__(256) void k_side_gs_len(SideData D, const uint32_t* __restrict__ cnt, uint32_t* __restrict__ flag,
                                                     uint64_t* __restrict__ len) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= D.nnames; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t c = i < D.nnames ? cnt[i] : 0u;
    flag[i] = c != 0u;
    len[i] = c ? (uint64_t)D.names[i].y + 1 + res_ndigits(c) + 2 : 0ull;
  }
}

MUSC_KERNEL __launch_bounds__(256) void k_side_gs_render(const uint32_t* __restrict__ idx, const uint64_t* __restrict__ off, uint64_t r0,
                                                        uint64_t r1, SideData D, const uint32_t* __restrict__ cnt,
                                                        unsigned char* __restrict__ out, uint32_t* __restrict__ flag) {
  const WaveId w = wave_id(threadIdx.x, blockIdx.x, blockDim.x, gridDim.x);
  const uint64_t base = off[r0];
  for (uint64_t j = r0 + w.wave; j < r1; j += w.nwaves) {
    const uint32_t k = __builtin_amdgcn_readfirstlane(idx[j]);
    if (k >= D.nnames || D.names[k].x >= D.nseq) {
      if (w.lane == 0) *flag = 1u;
      continue;
    }
    const uint2 nm = D.names[k];
    const uint32_t c = cnt[k], nd = res_ndigits(c);
    const uint64_t g0 = D.goff[nm.x], G = D.goff[nm.x + 1] - g0;
    const uint64_t total = off[j + 1] - off[j], NL = nm.y;
    if (total != NL + 1 + nd + 2 || NL >= G || c == 0u) {
      if (w.lane == 0) *flag = 1u;
      continue;
    }
    const char* const name = D.gtext + g0;
    wave_store(out + (off[j] - base), total, w.lane, [&](uint64_t q) -> uint32_t {
      const bool in_name = q < NL, in_num = q > NL && q - NL - 1 < nd;
      const uint32_t tb = (unsigned char)name[in_name ? q : 0ull];
      const uint32_t dg = res_digit_char(c, nd, in_num ? (uint32_t)(q - NL - 1) : 0u);
      return in_name ? tb : in_num ? dg : q + 1 == total ? (uint32_t)'\n' : (uint32_t)'\t';
    });
  }
}

// ---- readstats ----------------------------------------------------------------------------------------------------
// flag[i] = read i is matched and has a token (the reads whose results lines have eight fields); item nreads is empty
MUSC_KERNEL __launch_bounds__(256) void k_side_rs_flag(const uint32_t* __restrict__ matched, const uint4* __restrict__ tok, uint64_t nreads,
                                                      uint32_t* __restrict__ flag) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= nreads; i += (uint64_t)gridDim.x * blockDim.x)
    flag[i] = i < nreads && matched[i] && tok[i].w;
}

// head[j] = the j-th of those reads starts a run: its token differs from its predecessor's
MUSC_KERNEL __launch_bounds__(256) void k_side_rs_heads(const uint32_t* __restrict__ cr, uint64_t ncr, SideData D, uint32_t* __restrict__ head) {
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < ncr; j += (uint64_t)gridDim.x * blockDim.x) {
    uint32_t h = 1u;
    if (j > 0) {
      const uint32_t a = cr[j - 1], b = cr[j];
      const uint4 ta = D.tok[a], tb = D.tok[b];
      if (ta.w == tb.w) {
        const char* const pa = D.ttext + D.toff[a] + ta.z;
        const char* const pb = D.ttext + D.toff[b] + tb.z;
        uint32_t q = 0;
        while (q < ta.w && pa[q] == pb[q]) q++;
        h = q < ta.w;
      }
    }
    head[j] = h;
  }
}

// runof[read] = its run, runread[run] = the run's first read (incl = the inclusive scan of head)
MUSC_KERNEL __launch_bounds__(256) void k_side_rs_runs(const uint32_t* __restrict__ cr, const uint32_t* __restrict__ head,
                                                      const uint32_t* __restrict__ incl, uint64_t ncr, uint32_t* __restrict__ runof,
                                                      uint32_t* __restrict__ runread) {
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < ncr; j += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t run = incl[j] - 1u;
    runof[cr[j]] = run;
    if (head[j]) runread[run] = cr[j];
  }
}

// one key per kept tuple: run << 32 | name rank; all ones for the tuple of a read without a token
MUSC_KERNEL __launch_bounds__(256) void k_side_rs_keys(const uint4* __restrict__ hits, uint64_t m, const uint32_t* __restrict__ runof,
                                                      const uint32_t* __restrict__ nrank, uint64_t* __restrict__ keys) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint4 h = hits[i];  // (read and gene were checked by k_side_mark of the same prepare)
    const uint32_t run = runof[h.x];
    keys[i] = run == SIDE_NONE ? ~0ull : ((uint64_t)run << 32) | nrank[h.y];
  }
}

// flag[i] = sorted key i is the first of its value and names a run; item m is empty
MUSC_KERNEL __launch_bounds__(256) void k_side_rs_uniq(const uint64_t* __restrict__ keys, uint64_t m, uint32_t* __restrict__ flag) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= m; i += (uint64_t)gridDim.x * blockDim.x)
    flag[i] = i < m && keys[i] != ~0ull && (i == 0 || keys[i] != keys[i - 1]);
}

MUSC_KERNEL __launch_bounds__(256) void k_side_rs_elems(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ flag,
                                                       const uint32_t* __restrict__ excl, uint64_t m, uint64_t* __restrict__ el) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x)
    if (flag[i]) el[excl[i]] = keys[i];
}

// An element is one `name;` of a line; the first of a run also carries `token \t`, the last the newline.
struct SideEl {
  uint32_t run, rank, head, tail;
};
DEV SideEl side_el(const uint64_t* __restrict__ el, uint64_t nel, uint64_t k) {
  SideEl e;
  const uint64_t v = el[k];
  e.run = (uint32_t)(v >> 32);
  e.rank = (uint32_t)v;
  e.head = k == 0 || (uint32_t)(el[k - 1] >> 32) != e.run;
  e.tail = k + 1 == nel || (uint32_t)(el[k + 1] >> 32) != e.run;
  return e;
}

// len[k] = bytes of element k (item nel is empty); first[run] = the run's first element, first[nruns] = nel
MUSC_KERNEL __launch_bounds__(256) void k_side_rs_len(const uint64_t* __restrict__ el, uint64_t nel, uint32_t nruns, SideData D,
                                                     const uint32_t* __restrict__ runread, uint64_t* __restrict__ len,
                                                     uint32_t* __restrict__ first) {
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k <= nel; k += (uint64_t)gridDim.x * blockDim.x) {
    if (k == nel) {
      len[k] = 0;
      first[nruns] = (uint32_t)nel;
      continue;
    }
    const SideEl e = side_el(el, nel, k);
    uint64_t l = (uint64_t)D.names[e.rank].y + 1;
    if (e.head) {
      l += (uint64_t)D.tok[runread[e.run]].w + 1;
      first[e.run] = (uint32_t)k;
    }
    len[k] = l + e.tail;
  }
}

// loff[run] = first byte of the run's line (run <= nruns)
MUSC_KERNEL __launch_bounds__(256) void k_side_rs_lines(const uint32_t* __restrict__ first, const uint64_t* __restrict__ eloff, uint64_t nruns,
                                                       uint64_t* __restrict__ loff) {
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r <= nruns; r += (uint64_t)gridDim.x * blockDim.x)
    loff[r] = eloff[first[r]];
}

// lines [r0, r1): the elements first[r0] .. first[r1], one wave per element -- a read with ten thousand genes is ten
// thousand waves, not one
MUSC_KERNEL __launch_bounds__(256) void k_side_rs_render(const uint64_t* __restrict__ el, uint64_t nel, const uint64_t* __restrict__ eloff,
                                                        const uint32_t* __restrict__ first, uint32_t nruns, uint64_t r0, uint64_t r1,
                                                        SideData D, const uint32_t* __restrict__ runread, unsigned char* __restrict__ out,
                                                        uint32_t* __restrict__ flag) {
  const WaveId w = wave_id(threadIdx.x, blockIdx.x, blockDim.x, gridDim.x);
  const uint64_t e0 = first[r0], e1 = first[r1];
  if (e0 > e1 || e1 > nel) {
    if (threadIdx.x == 0) *flag = 1u;
    return;
  }
  const uint64_t base = eloff[e0];
  for (uint64_t k = e0 + w.wave; k < e1; k += w.nwaves) {
    SideEl e = side_el(el, nel, k);
    e.run = __builtin_amdgcn_readfirstlane(e.run);
    e.rank = __builtin_amdgcn_readfirstlane(e.rank);
    if (e.run >= nruns || e.rank >= D.nnames || D.names[e.rank].x >= D.nseq || (uint64_t)runread[e.run] >= D.nreads) {
      if (w.lane == 0) *flag = 1u;
      continue;
    }
    const uint2 nm = D.names[e.rank];
    const uint32_t r = runread[e.run];
    const uint64_t TL = e.head ? (uint64_t)D.tok[r].w + 1 : 0ull, NL = nm.y;  // token and its tab
    const uint64_t g0 = D.goff[nm.x], G = D.goff[nm.x + 1] - g0;
    const uint64_t total = eloff[k + 1] - eloff[k];
    if (total != TL + NL + 1 + e.tail || NL >= G) {
      if (w.lane == 0) *flag = 1u;
      continue;
    }
    const char* const name = D.gtext + g0;
    const char* const tokp = D.ttext + D.toff[r] + D.tok[r].z;
    wave_store(out + (eloff[k] - base), total, w.lane, [&](uint64_t q) -> uint32_t {
      const bool in_tok = q + 1 < TL, in_name = q >= TL && q - TL < NL;
      const uint32_t tb = (unsigned char)(in_tok ? tokp[q] : name[in_name ? q - TL : 0ull]);
      if (in_tok || in_name) return tb;
      if (q + 1 == TL) return (uint32_t)'\t';
      return q == TL + NL ? (uint32_t)';' : (uint32_t)'\n';
    });
  }
}
