// kernels_results.hpp -- the order and the bytes of results.txt from the resident tuples.
// Part of libmuscato_hip.so: included by muscato_hip.hip (one translation unit).
//
// Reference: the post-chain of cmd/muscato/main.go:422-676 -- combine_windows, the gene-id join (sort -k5 | join | cut,
// :524-611), `sort -k1` of the six-column lines (:657) and the join with reads_sorted (:659).  A line is
//     read \t targetsub \t pos \t nmiss \t name \t len [\t count \t names] \n
// and the lines are ordered bytewise on the first six columns.  On the device that order is the order of the key
//     read_idx | targetsub as 3-bit codes, 21 to a u64 | pos and nmiss as decimal text, 4 bits a digit | rank of name\tlen
// (most significant first): the loaded reads are the distinct sequences in bytewise order, and a tab is below every
// base letter and every digit, so a field that ends compares below one that goes on.
#pragma once

#include <rocprim/device/device_radix_sort.hpp>  // the sort of (key word, permutation) pairs, as in muscato_prep.hpp

#define RES_ABSENT 0xFFFFFFFFu     // rank of a gene without an id line: its tuples vanish
#define RES_BASES_PER_WORD 21      // as PREP_BASES_PER_WORD: 3-bit codes, 0 = past the end, 1..5 = A C G T X
#define RES_MAX_NMISS 65535u       // a read has at most 65535 bases; five decimal digits in the number key

// what k_results_keys builds
#define RES_KEY_RANK 0u
#define RES_KEY_NUMBER 1u
#define RES_KEY_READ 2u
#define RES_KEY_SPAN 3u            // + the word number

__host__ __device__ inline uint32_t res_ndigits(uint32_t v) {
  uint32_t n = 1;
  while (v >= 10u) {
    v /= 10u;
    n++;
  }
  return n;
}

// `v` as decimal text in `width` 4-bit cells: digit + 1, the first digit in the top cell, zero below the last one
__host__ __device__ inline uint64_t res_digit_cells(uint32_t v, uint32_t width) {
  const uint32_t nd = res_ndigits(v);
  uint64_t f = 0;
  for (uint32_t j = 0; j < nd; j++) {
    f |= (uint64_t)(v % 10u + 1u) << (4u * (width - nd + j));
    v /= 10u;
  }
  return f;
}

// "pos \t nmiss" as one integer that compares as the text does: ten cells of pos, five of nmiss (nmiss <= 99999)
__host__ __device__ inline uint64_t res_number_key(uint32_t pos, uint32_t nmiss) {
  return (res_digit_cells(pos, 10) << 20) | res_digit_cells(nmiss, 5);
}

// What a line is made of.  Every index in here has been checked by k_results_flag before the tuple reached an
// ordered list; the render kernel checks read and gene again (a uniform compare) before it loads through them.
struct ResLine {
  uint32_t r, g, pos, nmiss;
  uint32_t L, S;        // bases of the read, of the target span (clipped at the target's end)
  uint32_t np, nm;      // decimal digits of pos, nmiss
  uint64_t gbase;       // database position of the span's first base
  uint64_t rrec;        // first word of the read's record
  uint64_t goff, toff;  // first byte of the gene's text, of the read's tail
  uint64_t G, T;        // bytes of the gene's text, of the tail
  uint32_t has_tail, read_x;
  DEV uint64_t total() const { return (uint64_t)L + 1 + S + 1 + np + 1 + nm + 1 + G + (has_tail ? 1 + T : 0) + 1; }
};

struct ResData {
  const uint32_t* rd;
  const uint32_t* rdm;   // null: no read holds an X
  const uint32_t* db2;
  const uint32_t* dbm2;  // null: the database holds no X
  const uint64_t* seq_off;
  const char* gtext;
  const uint64_t* goff;
  const char* ttext;     // null: no read text, the lines end after the sixth column
  const uint64_t* toff;
  uint64_t nreads;
  uint32_t nseq;
  int rw;
};

DEV ResLine res_line(const ResData& D, uint4 h) {
  ResLine l;
  l.r = h.x;
  l.g = h.y;
  l.pos = h.z;
  l.nmiss = h.w;
  l.rrec = (uint64_t)h.x * (uint64_t)D.rw;
  const uint32_t lw = D.rd[l.rrec + (uint64_t)(D.rw - 1)];
  l.L = lw & 0xFFFFu;
  l.read_x = (lw & READ_HAS_X) && D.rdm;
  const uint64_t t0 = D.seq_off[h.y], t1 = D.seq_off[h.y + 1];
  const uint64_t left = t1 - t0 - (uint64_t)h.z;  // pos <= the target's length: checked
  l.S = left < (uint64_t)l.L ? (uint32_t)left : l.L;
  l.gbase = t0 + h.z;
  l.np = res_ndigits(h.z);
  l.nm = res_ndigits(h.w);
  l.goff = D.goff[h.y];
  l.G = D.goff[h.y + 1] - l.goff;
  l.has_tail = D.ttext != nullptr;
  l.toff = l.has_tail ? D.toff[h.x] : 0;
  l.T = l.has_tail ? D.toff[h.x + 1] - l.toff : 0;
  return l;
}

DEV uint32_t res_base_char(uint32_t code, uint32_t isx) { return isx ? (uint32_t)'X' : (0x54474341u >> (8u * code)) & 0xFFu; }  // "ACGT"

__device__ const uint32_t RES_POW10[10] = {1u, 10u, 100u, 1000u, 10000u, 100000u, 1000000u, 10000000u, 100000000u, 1000000000u};

DEV uint32_t res_digit_char(uint32_t v, uint32_t nd, uint32_t j) { return (uint32_t)'0' + (v / RES_POW10[nd - 1u - j]) % 10u; }

// Byte k of a line, k < l.total().  Which piece the byte belongs to is arithmetic; the loads are unconditional -- one
// plane word (the read's record or the database, at a clamped base inside the piece's own range) and one text byte (the
// gene's text or the tail, likewise) -- so that the four bytes of a dword, and the lanes of a wave that sit in different
// pieces, wait for memory once instead of once per piece.
DEV uint32_t res_line_byte(const ResData& D, const ResLine& l, uint64_t k) {
  const uint64_t s_span = (uint64_t)l.L + 1, s_pos = s_span + l.S + 1, s_nm = s_pos + l.np + 1, s_g = s_nm + l.nm + 1,
                 s_t = s_g + l.G + 1;
  const bool in_read = k < l.L, in_span = k >= s_span && k - s_span < l.S, in_pos = k >= s_pos && k - s_pos < l.np,
             in_nm = k >= s_nm && k - s_nm < l.nm, in_g = k >= s_g && k - s_g < l.G,
             in_t = l.has_tail && k >= s_t && k - s_t < l.T;
  // a base: the read's word or the database's (neither piece: the first word of the span's place, which exists)
  const uint32_t* const p2 = in_read ? D.rd : D.db2;
  const uint32_t* const pm = in_read ? (l.read_x ? D.rdm : nullptr) : D.dbm2;
  const uint64_t b = in_read ? l.rrec * 16ull + k : l.gbase + (in_span ? k - s_span : 0ull);
  const uint32_t sh = 2u * ((uint32_t)b & 15u);
  const uint32_t code = (p2[b >> 4] >> sh) & 3u;
  const uint32_t isx = pm ? (pm[b >> 4] >> sh) & 1u : 0u;
  // a text byte (neither piece: the first byte of the gene's place; the buffers end with 16 spare bytes)
  const char* const tp = in_t ? D.ttext + l.toff + (k - s_t) : D.gtext + l.goff + (in_g ? k - s_g : 0ull);
  const uint32_t tb = (unsigned char)*tp;
  // a digit
  const uint32_t v = in_pos ? l.pos : l.nmiss, nd = in_pos ? l.np : l.nm;
  const uint32_t j = in_pos ? (uint32_t)(k - s_pos) : in_nm ? (uint32_t)(k - s_nm) : 0u;
  const uint32_t dg = res_digit_char(v, nd, j);
  if (in_read || in_span) return res_base_char(code, isx);
  if (in_g || in_t) return tb;
  if (in_pos || in_nm) return dg;
  return k + 1 == l.total() ? (uint32_t)'\n' : (uint32_t)'\t';
}

// ---- validation and selection ---------------------------------------------------------------------------------
// keep[i] = the tuple's gene has an id line.  *flag: bit 0 = some tuple names a read, a gene or a position that does
// not exist (nothing is loaded through such an index), bit 1 = the list is not read-major in increasing read order.
MUSC_KERNEL __launch_bounds__(256) void k_results_flag(const uint4* __restrict__ in, uint64_t n, uint64_t nreads, uint32_t nseq,
                                                      const uint64_t* __restrict__ seq_off, const uint32_t* __restrict__ rank,
                                                      uint32_t* __restrict__ keep, uint32_t* __restrict__ flag) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint4 h = in[i];
    bool bad = (uint64_t)h.x >= nreads || h.y >= nseq || h.w > RES_MAX_NMISS;
    if (!bad) bad = (uint64_t)h.z > seq_off[h.y + 1] - seq_off[h.y];
    uint32_t k = 0, f = bad ? 1u : 0u;
    if (!bad) k = rank[h.y] != RES_ABSENT;
    if (i > 0 && in[i - 1].x > h.x) f |= 2u;
    keep[i] = k;
    if (f) atomicOr(flag, f);
  }
}

MUSC_KERNEL __launch_bounds__(256) void k_results_compact(const uint4* __restrict__ in, const uint32_t* __restrict__ keep,
                                                         const uint32_t* __restrict__ excl, uint64_t n, uint4* __restrict__ out) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
    if (keep[i]) out[excl[i]] = in[i];
}

MUSC_KERNEL __launch_bounds__(256) void k_results_gather(const uint4* __restrict__ in, const uint32_t* __restrict__ perm, uint64_t n,
                                                        uint4* __restrict__ out) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) out[i] = in[perm[i]];
}

// multi[i] = tuple i of the read-major list shares its read with a neighbour (singletons are already in place);
// *maxlen = the longest read among those
MUSC_KERNEL __launch_bounds__(256) void k_results_segments(const uint4* __restrict__ a, uint64_t m, const uint32_t* __restrict__ rd, int rw,
                                                          uint32_t* __restrict__ multi, unsigned long long* __restrict__ maxlen) {
  __shared__ unsigned long long s_m[4];
  unsigned long long l = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t r = a[i].x;
    const bool mu = (i > 0 && a[i - 1].x == r) || (i + 1 < m && a[i + 1].x == r);
    multi[i] = mu;
    if (mu) {
      const unsigned long long len = rd[(uint64_t)r * (uint64_t)rw + (uint64_t)(rw - 1)] & 0xFFFFu;
      l = len > l ? len : l;
    }
  }
  for (int d = 32; d; d >>= 1) {
    const unsigned long long o = __shfl_xor(l, d);
    l = o > l ? o : l;
  }
  if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = l;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (unsigned w = 1; w < (blockDim.x + 63) / 64; w++) l = s_m[w] > l ? s_m[w] : l;
    if (l) atomicMax(maxlen, l);
  }
}

// idx[j] = position of the j-th tuple with multi set (incl = inclusive scan of multi)
MUSC_KERNEL __launch_bounds__(256) void k_results_idx(const uint32_t* __restrict__ multi, const uint32_t* __restrict__ incl, uint64_t m,
                                                     uint32_t* __restrict__ idx) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x)
    if (multi[i]) idx[incl[i] - 1u] = (uint32_t)i;
}

// 21 bases of a target span as 3-bit codes, first base most significant: bases [21 w, 21 w + 21) of the `S` bases that
// start at database base `gbase`, gathered at whatever 2-bit phase that is.  ext64 reads at most two words past the
// one that holds the first base: the planes are allocated with 64 words of slack.
DEV uint64_t res_span_word(const uint32_t* __restrict__ db2, const uint32_t* __restrict__ dbm2, uint64_t gbase, uint32_t S, uint32_t w) {
  const uint64_t first = (uint64_t)w * RES_BASES_PER_WORD;
  if (first >= S) return 0;
  const uint32_t nb = S - (uint32_t)first < RES_BASES_PER_WORD ? S - (uint32_t)first : RES_BASES_PER_WORD;
  const uint64_t bo = 2ull * (gbase + first);
  const uint64_t bits = ext64(db2, bo);
  const uint64_t mb = dbm2 ? ext64(dbm2, bo) : 0ull;
  uint64_t key = 0;
  for (uint32_t j = 0; j < nb; j++) {
    const uint64_t code = ((mb >> (2u * j)) & 1ull) ? 5ull : ((bits >> (2u * j)) & 3ull) + 1ull;
    key |= code << (60u - 3u * j);
  }
  return key;
}

// keys[j] = one key word of tuple a[idx[perm[j]]] -- `what`: RES_KEY_RANK, _NUMBER, _READ, or RES_KEY_SPAN + w
MUSC_KERNEL __launch_bounds__(256) void k_results_keys(const uint4* __restrict__ a, const uint32_t* __restrict__ idx,
                                                      const uint32_t* __restrict__ perm, uint64_t k, uint32_t what,
                                                      const uint32_t* __restrict__ rank, const uint32_t* __restrict__ rd, int rw,
                                                      const uint32_t* __restrict__ db2, const uint32_t* __restrict__ dbm2,
                                                      const uint64_t* __restrict__ seq_off, uint64_t* __restrict__ keys) {
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < k; j += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t p = perm[j];  // a permutation of 0..k-1
    const uint4 h = a[idx ? idx[p] : p];
    uint64_t key;
    if (what == RES_KEY_RANK) key = rank[h.y];
    else if (what == RES_KEY_NUMBER) key = res_number_key(h.z, h.w);
    else if (what == RES_KEY_READ) key = h.x;
    else {
      const uint32_t L = rd[(uint64_t)h.x * (uint64_t)rw + (uint64_t)(rw - 1)] & 0xFFFFu;
      const uint64_t t0 = seq_off[h.y], left = seq_off[h.y + 1] - t0 - (uint64_t)h.z;
      const uint32_t S = left < (uint64_t)L ? (uint32_t)left : L;
      key = res_span_word(db2, dbm2, t0 + h.z, S, what - RES_KEY_SPAN);
    }
    keys[j] = key;
  }
}

// the ordered list: a singleton stays where it is, the j-th tuple of the others is the one the sort put there
MUSC_KERNEL __launch_bounds__(256) void k_results_place(const uint4* __restrict__ a, const uint32_t* __restrict__ multi,
                                                       const uint32_t* __restrict__ incl, const uint32_t* __restrict__ idx,
                                                       const uint32_t* __restrict__ perm, uint64_t m, uint4* __restrict__ out) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x)
    out[i] = multi[i] ? a[idx[perm[incl[i] - 1u]]] : a[i];
}

// ---- the bytes -------------------------------------------------------------------------------------------------
// len[i] = bytes of line i; len[m] = 0, so that the exclusive scan over m + 1 elements ends with the total
MUSC_KERNEL __launch_bounds__(256) void k_results_len(const uint4* __restrict__ hits, uint64_t m, ResData D, uint64_t* __restrict__ len) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= m; i += (uint64_t)gridDim.x * blockDim.x)
    len[i] = i < m ? res_line(D, hits[i]).total() : 0ull;
}

// Where a thread of a render kernel sits: one wave per record, the waves of the whole grid striding over the records.
// The kernel hands in threadIdx.x, blockIdx.x, blockDim.x and gridDim.x: read in the kernel's own body blockDim.x is one
// scalar load of a kernel argument and nwaves stays in SGPRs; read in here it came through a vector load and took two
// VGPRs in every render kernel.
struct WaveId {
  uint32_t lane;
  uint64_t wave, nwaves;
};
DEV WaveId wave_id(uint32_t tid, uint32_t bid, uint32_t bdim, uint32_t gdim) {
  WaveId w;
  w.lane = tid & 63u;
  w.wave = (uint64_t)bid * (bdim >> 6) + (tid >> 6);
  w.nwaves = (uint64_t)gdim * (bdim >> 6);
  return w;
}

// `total` bytes at `p`, byte k = at(k), by one wave: each lane assembles whole dwords at the alignment the destination
// ADDRESS has and stores them with one 4-byte store; only the bytes before the first aligned dword (lanes 0..2) and
// after the last one (lanes 8..10) are byte stores
template <class F>
DEV void wave_store(unsigned char* p, uint64_t total, uint32_t lane, F at) {
  const uint64_t mis = (uint64_t)(4u - ((uint32_t)(uintptr_t)p & 3u)) & 3u;
  const uint64_t head = mis < total ? mis : total;
  const uint64_t nd = (total - head) >> 2;
  for (uint64_t d = lane; d < nd; d += 64) {
    const uint64_t k = head + 4 * d;
    *reinterpret_cast<uint32_t*>(p + k) = at(k) | (at(k + 1) << 8) | (at(k + 2) << 16) | (at(k + 3) << 24);
  }
  const uint64_t tail0 = head + 4 * nd;
  if (lane < head) p[lane] = (unsigned char)at(lane);
  else if (lane >= 8 && tail0 + (lane - 8) < total) p[tail0 + (lane - 8)] = (unsigned char)at(tail0 + (lane - 8));
}

// Lines [line0, line1) of the ordered list into `out`, line i at byte off[i] - off[line0].  One wave per line: the
// line's descriptor is wave-uniform (scalar loads) and wave_store writes its bytes.  No LDS, no atomics; offsets are
// 64-bit.  Targets are rendered from the 2-bit planes: a target byte that is none of A C G T comes out as X.
// An ordered list was checked before any load and its offsets were made from the same data, so neither test below
// fails unless the context's bookkeeping is wrong; a line that does fail is not rendered and fails the call through
// *flag (a plain store: every writer stores the same word).
MUSC_KERNEL __launch_bounds__(256) void k_results_render(const uint4* __restrict__ hits, const uint64_t* __restrict__ off, uint64_t line0,
                                                        uint64_t line1, ResData D, unsigned char* __restrict__ out,
                                                        uint32_t* __restrict__ flag) {
  const WaveId w = wave_id(threadIdx.x, blockIdx.x, blockDim.x, gridDim.x);
  const uint64_t base = off[line0];
  for (uint64_t i = line0 + w.wave; i < line1; i += w.nwaves) {
    uint4 h = hits[i];
    h.x = __builtin_amdgcn_readfirstlane(h.x);
    h.y = __builtin_amdgcn_readfirstlane(h.y);
    h.z = __builtin_amdgcn_readfirstlane(h.z);
    h.w = __builtin_amdgcn_readfirstlane(h.w);
    if ((uint64_t)h.x >= D.nreads || h.y >= D.nseq) {
      if (w.lane == 0) *flag = 1u;
      continue;
    }
    const ResLine l = res_line(D, h);
    const uint64_t total = off[i + 1] - off[i];
    if (total != l.total()) {
      if (w.lane == 0) *flag = 1u;
      continue;
    }
    wave_store(out + (off[i] - base), total, w.lane, [&](uint64_t k) { return res_line_byte(D, l, k); });
  }
}
