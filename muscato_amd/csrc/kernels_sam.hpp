// kernels_sam.hpp -- SAM records and header from the resident tuples.
// Part of libmuscato_hip.so: included by muscato_hip.hip (one translation unit), after kernels_side.hpp.
//
// One record per line of results.txt, in the same order, from what musc_results_order left on the device: the ordered
// tuples, the 2-bit and X planes of the reads and of the database, seq_off, the gene text and the read tails.  The
// format and its size rules are sam_plan.hpp's; this file adds the two things no other stage does: the comparison of
// every span with its read (NM, and the places MD is made of), 32 bases a step by XOR on the 2-bit words with the X
// planes folded in, and MD as variable-length text.
//
// The counting pass is one thread per line; the render kernels are one wave per record (wave_id, wave_store:
// kernels_results.hpp).  Every byte of a record but MD is arithmetic in the byte index and goes through wave_store;
// MD is written by the same wave, a lane per 32-base word of the span, placed by two wave scans.  No LDS, no atomics
// but the refusal flag, nothing waits on another workgroup.
#pragma once

#include "sam_plan.hpp"

struct SamData {
  ResData R;
  const uint4* tok;     // per read: x = bytes of the count (0: no XC), y = first byte of QNAME within the tail, z = its bytes
  const uint2* gname;   // per gene: x = first byte of the RNAME token within its text, y = its bytes
  const uint32_t* rank; // per gene: RES_ABSENT without an id line
  uint32_t rev_pairs;
};

// ---- names ------------------------------------------------------------------------------------------------------------
MUSC_KERNEL __launch_bounds__(256) void k_sam_tokens(const char* __restrict__ ttext, const uint64_t* __restrict__ toff, uint64_t nreads,
                                                    uint4* __restrict__ tok) {
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < nreads; r += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t t0 = toff[r];
    const musc_sam::TailSpans t = musc_sam::tail_spans(reinterpret_cast<const unsigned char*>(ttext) + t0, toff[r + 1] - t0);
    tok[r] = make_uint4(t.count_len, t.q0, t.qlen, 0u);
  }
}

// gname[g] = the RNAME token of gene g.  *flag: bit 0 = a gene with an id line has an empty token (under rev_pairs: or
// its even partner has no id line), bit 1 = under rev_pairs the two targets of a pair differ in length.
MUSC_KERNEL __launch_bounds__(256) void k_sam_gnames(const char* __restrict__ gtext, const uint64_t* __restrict__ goff,
                                                    const uint32_t* __restrict__ rank, const uint64_t* __restrict__ seq_off, uint32_t nseq,
                                                    uint32_t rev_pairs, uint2* __restrict__ gname, uint32_t* __restrict__ flag) {
  for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < nseq; g += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t g0 = goff[g];
    const musc_sam::NameSpan s = musc_sam::rname_span(reinterpret_cast<const unsigned char*>(gtext) + g0, goff[g + 1] - g0);
    gname[g] = make_uint2(s.n0, s.len);
    uint32_t f = 0;
    if (rank[g] != RES_ABSENT) {
      if (rev_pairs && (g & 1u)) {
        const uint64_t e0 = goff[g - 1];
        const musc_sam::NameSpan e = musc_sam::rname_span(reinterpret_cast<const unsigned char*>(gtext) + e0, g0 - e0);
        if (rank[g - 1] == RES_ABSENT || e.len == 0u) f |= 1u;
      } else if (s.len == 0u) {
        f |= 1u;
      }
    }
    if (rev_pairs && (g & 1u) && seq_off[g + 1] - seq_off[g] != seq_off[g] - seq_off[g - 1]) f |= 2u;
    if (f) atomicOr(flag, f);
  }
}

// ---- the header -------------------------------------------------------------------------------------------------------
// Slots: 0 = @HD, 1 + t = the @SQ line of target t (empty when it has none: no id line, or odd under rev_pairs),
// nseq + 1 = @PG.  len[nseq + 2] = 0, so that the exclusive scan over nseq + 3 items ends with the total.
DEV bool sam_has_sq(const SamData& D, uint32_t t) { return D.rank[t] != RES_ABSENT && !(D.rev_pairs && (t & 1u)); }

MUSC_KERNEL __launch_bounds__(256) void k_sam_hdr_len(SamData D, uint64_t* __restrict__ len) {
  const uint64_t n = (uint64_t)D.R.nseq + 2;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t l = 0;
    if (i == 0) l = musc_sam::HD_BYTES;
    else if (i + 1 == n) l = musc_sam::PG_BYTES;
    else if (i < n && sam_has_sq(D, (uint32_t)(i - 1)))
      l = musc_sam::sq_bytes(D.gname[i - 1].y, D.R.seq_off[i] - D.R.seq_off[i - 1]);
    len[i] = l;
  }
}

__device__ const uint64_t SAM_POW10[20] = {1ull, 10ull, 100ull, 1000ull, 10000ull, 100000ull, 1000000ull, 10000000ull, 100000000ull,
                                           1000000000ull, 10000000000ull, 100000000000ull, 1000000000000ull, 10000000000000ull,
                                           100000000000000ull, 1000000000000000ull, 10000000000000000ull, 100000000000000000ull,
                                           1000000000000000000ull, 10000000000000000000ull};
DEV uint32_t sam_digit_char(uint64_t v, uint32_t nd, uint32_t j) { return (uint32_t)'0' + (uint32_t)((v / SAM_POW10[nd - 1u - j]) % 10ull); }

// up to eight bytes of fixed text as one integer, the first byte lowest
constexpr uint64_t sam_lit(const char* s, int n) {
  uint64_t v = 0;
  for (int i = 0; i < n; i++) v |= (uint64_t)(unsigned char)s[i] << (8 * i);
  return v;
}
// (a template argument: the integer is made by the compiler, never by the kernel)
#define SAM_LIT(s) std::integral_constant<uint64_t, sam_lit(s, (int)sizeof(s) - 1)>::value, (uint32_t)sizeof(s) - 1u

// Byte k of a run of pieces: every piece either owns k (and says what the byte is) or takes its length off k
struct SamPick {
  uint64_t k;
  uint32_t out;
  bool done;
  DEV explicit SamPick(uint64_t k_) : k(k_), out((uint32_t)'\n'), done(false) {}
  DEV bool take(uint64_t n) {
    if (done) return false;
    if (k < n) return done = true;
    k -= n;
    return false;
  }
  DEV void lit(uint64_t packed, uint32_t n) {
    if (take(n)) out = (uint32_t)(packed >> (8u * (uint32_t)k)) & 0xFFu;
  }
  DEV void num(uint32_t v) {
    const uint32_t nd = res_ndigits(v);
    if (take(nd)) out = res_digit_char(v, nd, (uint32_t)k);
  }
  DEV void num64(uint64_t v) {  // POS and LN: a target may reach 2^32 bases
    const uint32_t nd = musc_sam::ndigits(v);
    if (take(nd)) out = sam_digit_char(v, nd, (uint32_t)k);
  }
  DEV void text(const char* p, uint64_t n) {
    if (take(n)) out = (unsigned char)p[k];
  }
};

MUSC_KERNEL __launch_bounds__(256) void k_sam_hdr_render(const uint64_t* __restrict__ off, uint64_t r0, uint64_t r1, SamData D,
                                                        unsigned char* __restrict__ out, uint32_t* __restrict__ flag) {
  const WaveId w = wave_id(threadIdx.x, blockIdx.x, blockDim.x, gridDim.x);
  const uint64_t base = off[r0], n = (uint64_t)D.R.nseq + 2;
  for (uint64_t i = r0 + w.wave; i < r1; i += w.nwaves) {
    const uint64_t total = off[i + 1] - off[i];
    unsigned char* const p = out + (off[i] - base);
    if (i >= n) {
      if (w.lane == 0) *flag = 1u;
    } else if (i == 0 || i + 1 == n) {
      if (total != (i == 0 ? musc_sam::HD_BYTES : musc_sam::PG_BYTES)) {
        if (w.lane == 0) *flag = 1u;
        continue;
      }
      wave_store(p, total, w.lane, [&](uint64_t k) -> uint32_t {  // musc_sam::HD_LINE and PG_LINE, eight bytes a piece
        SamPick q(k);
        if (i == 0) {
          static_assert(musc_sam::HD_BYTES == 8 + 8 + 8 + 7 + 1, "@HD is restated here");
          q.lit(SAM_LIT("@HD\tVN:1"));
          q.lit(SAM_LIT(".6\tSO:un"));
          q.lit(SAM_LIT("sorted\tG"));
          q.lit(SAM_LIT("O:query"));
        } else {
          static_assert(musc_sam::PG_BYTES == 8 + 8 + 8 + 8 + 1 + 1, "@PG is restated here");
          q.lit(SAM_LIT("@PG\tID:m"));
          q.lit(SAM_LIT("uscato_a"));
          q.lit(SAM_LIT("md\tPN:mu"));
          q.lit(SAM_LIT("scato_am"));
          q.lit(SAM_LIT("d"));
        }
        return q.out;  // (the newline is what is left)
      });
    } else {
      const uint32_t t = (uint32_t)(i - 1);
      if (!sam_has_sq(D, t)) {
        if (total != 0 && w.lane == 0) *flag = 1u;
        continue;
      }
      const uint2 nm = D.gname[t];
      const uint64_t g0 = D.R.goff[t], G = D.R.goff[t + 1] - g0, tl = D.R.seq_off[t + 1] - D.R.seq_off[t];
      if (total != musc_sam::sq_bytes(nm.y, tl) || (uint64_t)nm.x + nm.y > G) {
        if (w.lane == 0) *flag = 1u;
        continue;
      }
      const char* const name = D.R.gtext + g0 + nm.x;
      wave_store(p, total, w.lane, [&](uint64_t k) -> uint32_t {
        SamPick q(k);
        q.lit(SAM_LIT("@SQ\tSN:"));
        q.text(name, nm.y);
        q.lit(SAM_LIT("\tLN:"));
        q.num64(tl);
        return q.out;  // (the newline is what is left)
      });
    }
  }
}

// ---- the comparison -----------------------------------------------------------------------------------------------------
// Bases [32 k, 32 k + 32) of a line's span against the read: bit 2 j set = base 32 k + j differs (A C G T X, X equals X).
// Two 64-bit extracts of the 2-bit planes at whatever phase the read record and the database place have (ext64 reads
// at most two words past the first: both planes end with spare words), two more of the X planes where there is an X.
DEV uint64_t sam_diff_word(const ResData& D, const ResLine& l, uint32_t k) {
  const uint64_t EVEN = 0x5555555555555555ull;
  const uint32_t j0 = 32u * k, nb = l.S - j0 < 32u ? l.S - j0 : 32u;
  const uint64_t rb = 2ull * (l.rrec * 16ull + j0), tb = 2ull * (l.gbase + j0);
  const uint64_t x = ext64(D.rd, rb) ^ ext64(D.db2, tb);
  const uint64_t cd = (x | (x >> 1)) & EVEN;
  const uint64_t xr = l.read_x ? ext64(D.rdm, rb) & EVEN : 0ull;
  const uint64_t xt = D.dbm2 ? ext64(D.dbm2, tb) & EVEN : 0ull;
  return ((xr ^ xt) | (cd & ~(xr | xt))) & lowmask64(2 * (int)nb);
}

struct SamRec {
  ResLine l;
  uint32_t rev, f;         // reverse strand; the target RNAME and POS speak of
  uint64_t tlen;           // bases of target g
  uint32_t qlen, clen;     // bytes of QNAME (0: `*`), of the count (0: no XC)
  uint64_t qp, cp, np;     // first byte of QNAME and of the count in the read text, of RNAME in the gene text
  uint32_t nlen;
};

DEV SamRec sam_rec(const SamData& D, uint4 h) {
  SamRec s;
  s.l = res_line(D.R, h);
  s.rev = D.rev_pairs && (h.y & 1u);
  s.f = s.rev ? h.y - 1u : h.y;
  s.tlen = D.R.seq_off[h.y + 1] - D.R.seq_off[h.y];
  const uint4 t = s.l.has_tail ? D.tok[h.x] : make_uint4(0u, 0u, 0u, 0u);
  s.clen = t.x;
  s.qlen = t.z;
  s.cp = s.l.toff;
  s.qp = s.l.toff + t.y;
  const uint2 nm = D.gname[s.f];
  s.np = D.R.goff[s.f] + nm.x;
  s.nlen = nm.y;
  return s;
}

DEV uint64_t sam_rec_bytes(const SamRec& s, uint4 info, uint32_t nmiss) {
  musc_sam::RecordSizes z;
  z.qname = s.qlen ? s.qlen : 1u;
  z.flag = musc_sam::flag(s.rev, info.w == 1u);
  z.rname = s.nlen;
  z.pos1 = musc_sam::pos1(s.rev, s.tlen, s.l.pos, s.l.S);
  z.L = s.l.L;
  z.S = s.l.S;
  z.d = info.x;
  z.md = info.y;
  z.nh = info.z;
  z.hi = info.w;
  z.nmiss = nmiss;
  z.count_len = s.clen;
  return musc_sam::record_bytes(z);
}

// ---- the counting pass --------------------------------------------------------------------------------------------------
// first[r] / last[r] = the first and the last line of read r in the ordered (read-major) list
MUSC_KERNEL __launch_bounds__(256) void k_sam_runs(const uint4* __restrict__ hits, uint64_t m, uint32_t* __restrict__ first,
                                                  uint32_t* __restrict__ last) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t r = hits[i].x;
    if (i == 0 || hits[i - 1].x != r) first[r] = (uint32_t)i;
    if (i + 1 == m || hits[i + 1].x != r) last[r] = (uint32_t)i;
  }
}

// info[i] = (NM, bytes of MD, NH, HI) of line i, len[i] = the bytes of its record; len[m] = 0
MUSC_KERNEL __launch_bounds__(256) void k_sam_count(const uint4* __restrict__ hits, uint64_t m, SamData D, const uint32_t* __restrict__ first,
                                                   const uint32_t* __restrict__ last, uint4* __restrict__ info, uint64_t* __restrict__ len) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= m; i += (uint64_t)gridDim.x * blockDim.x) {
    if (i == m) {
      len[i] = 0;
      continue;
    }
    const uint4 h = hits[i];
    const SamRec s = sam_rec(D, h);
    musc_sam::MdSize md;
    uint32_t d = 0;
    for (uint32_t k = 0; 32u * k < s.l.S; k++) {
      uint64_t diff = sam_diff_word(D.R, s.l, k);  // a word without a mismatch costs this line and the next
      d += (uint32_t)__popcll(diff);
      while (diff) {
        md.mismatch(32u * k + ((uint32_t)__builtin_ctzll(diff) >> 1));
        diff &= diff - 1;
      }
    }
    const uint32_t f0 = first[h.x];
    const uint4 in = make_uint4(d, md.finish(s.l.S), last[h.x] - f0 + 1u, (uint32_t)i - f0 + 1u);
    info[i] = in;
    len[i] = sam_rec_bytes(s, in, h.w);
  }
}

// ---- the render kernel ----------------------------------------------------------------------------------------------------
DEV uint32_t sam_base_char(uint32_t code, uint32_t isx, uint32_t rev) {
  return isx ? (uint32_t)'N' : (0x54474341u >> (8u * (rev ? 3u - code : code))) & 0xFFu;  // "ACGT"
}

// `v` in decimal at p[at ..], every byte inside [0, end)
DEV void sam_put_num(unsigned char* p, uint32_t at, uint32_t end, uint32_t v, uint32_t nd) {
  for (uint32_t j = 0; j < nd; j++)
    if (at + j < end) p[at + j] = (unsigned char)res_digit_char(v, nd, j);
}

// MD of a record into p[0, mdlen), by one wave.  The span is taken 64 words (2048 bases) a round, a word a lane.  In
// span order mismatch i, at place m_i, owns the piece `digits(m_i - m_(i-1) - 1) base`; the pieces are laid out by an
// exclusive scan of their lengths, which needs the place of the last mismatch before each lane's word: a max scan.  On
// the forward strand the piece stands at its offset from the front and the last run's digits end the text.  On the
// reverse strand the same piece is read backwards (`base digits`, the base complemented) at the same offset from the
// end, and the last run's digits open the text.  Every store is held inside [0, mdlen).
DEV void sam_md_store(unsigned char* p, uint32_t mdlen, const ResData& D, const ResLine& l, uint32_t rev, uint32_t lane) {
  const uint32_t S = l.S, nw = (S + 31u) >> 5;
  int32_t carry_last = -1;
  uint32_t carry_off = 0;
  for (uint32_t w0 = 0; w0 < nw; w0 += 64u) {
    const uint32_t k = w0 + lane;
    const uint64_t diff = k < nw ? sam_diff_word(D, l, k) : 0ull;
    int32_t mine = diff ? (int32_t)(32u * k + ((63u - (uint32_t)__builtin_clzll(diff)) >> 1)) : -1;
    for (int dl = 1; dl < 64; dl <<= 1) {
      const int32_t o = __shfl_up(mine, dl);
      if ((int)lane >= dl && o > mine) mine = o;
    }
    int32_t prev = __shfl_up(mine, 1);
    if (lane == 0 || prev < carry_last) prev = carry_last;
    uint32_t bytes = 0;
    int32_t last = prev;
    for (uint64_t dd = diff; dd; dd &= dd - 1) {
      const int32_t j = (int32_t)(32u * k + ((uint32_t)__builtin_ctzll(dd) >> 1));
      bytes += musc_sam::ndigits((uint32_t)(j - last - 1)) + 1u;
      last = j;
    }
    uint32_t incl = bytes;
    for (int dl = 1; dl < 64; dl <<= 1) {
      const uint32_t o = __shfl_up(incl, dl);
      if ((int)lane >= dl) incl += o;
    }
    uint32_t at = carry_off + incl - bytes;
    last = prev;
    for (uint64_t dd = diff; dd; dd &= dd - 1) {
      const int32_t j = (int32_t)(32u * k + ((uint32_t)__builtin_ctzll(dd) >> 1));
      const uint32_t run = (uint32_t)(j - last - 1), nd = musc_sam::ndigits(run);
      const uint64_t b = l.gbase + (uint64_t)j;
      const uint32_t sh = 2u * ((uint32_t)b & 15u);
      const uint32_t ch = sam_base_char((D.db2[b >> 4] >> sh) & 3u, D.dbm2 ? (D.dbm2[b >> 4] >> sh) & 1u : 0u, rev);
      if (at + nd + 1u <= mdlen) {
        if (!rev) {
          sam_put_num(p, at, mdlen, run, nd);
          p[at + nd] = (unsigned char)ch;
        } else {
          const uint32_t q = mdlen - at - nd - 1u;
          p[q] = (unsigned char)ch;
          sam_put_num(p, q + 1u, mdlen, run, nd);
        }
      }
      at += nd + 1u;
      last = j;
    }
    carry_off += __shfl(incl, 63);
    const int32_t wl = __shfl(mine, 63);
    if (wl > carry_last) carry_last = wl;
  }
  if (lane == 0) {
    const uint32_t run = (uint32_t)((int32_t)S - carry_last - 1), nd = musc_sam::ndigits(run);
    if (carry_off + nd <= mdlen) sam_put_num(p, rev ? 0u : mdlen - nd, mdlen, run, nd);
  }
}

// Records [r0, r1) of the ordered list into `out`, record i at byte off[i] - off[r0]; one wave per record.  The tuple
// is checked again before anything is loaded through it, and the record's length against the one its offsets were
// made from: a record that fails is not rendered and fails the call through *flag.
MUSC_KERNEL __launch_bounds__(256) void k_sam_render(const uint4* __restrict__ hits, const uint4* __restrict__ info,
                                                    const uint64_t* __restrict__ off, uint64_t r0, uint64_t r1, SamData D,
                                                    unsigned char* __restrict__ out, uint32_t* __restrict__ flag) {
  const WaveId w = wave_id(threadIdx.x, blockIdx.x, blockDim.x, gridDim.x);
  const uint64_t base = off[r0];
  for (uint64_t i = r0 + w.wave; i < r1; i += w.nwaves) {
    uint4 h = hits[i], in = info[i];
    h.x = __builtin_amdgcn_readfirstlane(h.x);
    h.y = __builtin_amdgcn_readfirstlane(h.y);
    h.z = __builtin_amdgcn_readfirstlane(h.z);
    h.w = __builtin_amdgcn_readfirstlane(h.w);
    in.x = __builtin_amdgcn_readfirstlane(in.x);
    in.y = __builtin_amdgcn_readfirstlane(in.y);
    in.z = __builtin_amdgcn_readfirstlane(in.z);
    in.w = __builtin_amdgcn_readfirstlane(in.w);
    if ((uint64_t)h.x >= D.R.nreads || h.y >= D.R.nseq || (uint64_t)h.z > D.R.seq_off[h.y + 1] - D.R.seq_off[h.y]) {
      if (w.lane == 0) *flag = 1u;
      continue;
    }
    const SamRec s = sam_rec(D, h);
    const ResLine& l = s.l;
    const uint64_t total = off[i + 1] - off[i];
    if (total != sam_rec_bytes(s, in, h.w) || (uint64_t)in.y > total) {
      if (w.lane == 0) *flag = 1u;
      continue;
    }
    const uint32_t L = l.L, S = l.S, rev = s.rev, mdlen = in.y;
    const uint32_t fl = musc_sam::flag(rev, in.w == 1u);
    const uint64_t p1 = musc_sam::pos1(rev, s.tlen, l.pos, S);
    // the bytes after MD: the fixed tags, XC and the newline
    const uint64_t after = 6ull + musc_sam::ndigits(in.z) + 6 + musc_sam::ndigits(in.w) + 6 + musc_sam::ndigits(h.w) +
                           (s.clen ? 6ull + s.clen : 0ull) + 1;
    const uint64_t before = total - after - mdlen;
    unsigned char* const p = out + (off[i] - base);
    wave_store(p, before, w.lane, [&](uint64_t k) -> uint32_t {
      SamPick q(k);
      if (s.qlen) q.text(D.R.ttext + s.qp, s.qlen);
      else q.lit(SAM_LIT("*"));
      q.lit(SAM_LIT("\t"));
      q.num(fl);
      q.lit(SAM_LIT("\t"));
      q.text(D.R.gtext + s.np, s.nlen);
      q.lit(SAM_LIT("\t"));
      q.num64(p1);
      q.lit(SAM_LIT("\t255\t"));
      if (S == 0u) {
        q.lit(SAM_LIT("*"));
      } else {
        if (rev && L > S) q.num(L - S), q.lit(SAM_LIT("S"));
        q.num(S);
        q.lit(SAM_LIT("M"));
        if (!rev && L > S) q.num(L - S), q.lit(SAM_LIT("S"));
      }
      q.lit(SAM_LIT("\t*\t0\t0\t"));
      if (L == 0u) {
        q.lit(SAM_LIT("*"));
      } else if (q.take(L)) {
        const uint64_t b = l.rrec * 16ull + (rev ? (uint64_t)L - 1 - q.k : q.k);
        const uint32_t sh = 2u * ((uint32_t)b & 15u);
        q.out = sam_base_char((D.R.rd[b >> 4] >> sh) & 3u, l.read_x ? (D.R.rdm[b >> 4] >> sh) & 1u : 0u, rev);
      }
      q.lit(SAM_LIT("\t*\tNM:i:"));
      q.num(in.x);
      q.lit(SAM_LIT("\tMD:Z:"));
      return q.out;
    });
    sam_md_store(p + before, mdlen, D.R, l, rev, w.lane);
    wave_store(p + before + mdlen, after, w.lane, [&](uint64_t k) -> uint32_t {
      SamPick q(k);
      q.lit(SAM_LIT("\tNH:i:"));
      q.num(in.z);
      q.lit(SAM_LIT("\tHI:i:"));
      q.num(in.w);
      q.lit(SAM_LIT("\tXM:i:"));
      q.num(h.w);
      if (s.clen) {
        q.lit(SAM_LIT("\tXC:i:"));
        q.text(D.R.ttext + s.cp, s.clen);
      }
      return q.out;  // (the newline is what is left)
    });
  }
}
