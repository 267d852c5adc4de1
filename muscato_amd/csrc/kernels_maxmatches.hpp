// kernels_maxmatches.hpp -- the reference's MaxMatches truncation replayed from the resident tuples.
// Part of libmuscato_hip.so: included by muscato_hip.hip (one translation unit).
//
// Reference: cmd/muscato_confirm/main.go:183-244, 424-448.  A (window, key) block with more than MaxMatches accepted
// pairs keeps an order-dependent subset: candidates in the bytewise order of their smatch line outside, reads in the
// bytewise order of their win_k_sorted line inside; "first" stops after MaxMatches + 1 pairs, "best" is a sift-up heap
// whose array tail is cut at MaxMatches.  The specification, line by line, is apply_maxmatches of host/muscato_host.hpp.
//
// Text order on the device is the order of 3-bit codes, 0 = past the end (the tab that ends a field sorts below every
// letter), 1..5 = A C G T X: the byte order of the letters.  An X equals an X, as memcmp on the prepared text has it.
#pragma once

#include <rocprim/device/device_merge_sort.hpp>

#include "maxmatches_plan.hpp"

// the word of a (tuple, window): what the read's window is to the suspect blocks, and what became of the pair
#define MM_NONE 0xFFFFFFFFu    // the read has no valid window here
#define MM_EMITS 0x80000000u   // this window's confirm emits the tuple
#define MM_KEPT 0x40000000u    // the pair survived its block's truncation
#define MM_BLOCK 0x3FFFFFFFu   // the block's number; all ones: the window's block is no suspect

struct MmData {
  const uint32_t* rd;
  const uint32_t* rdm;   // null: no read holds an X
  const uint32_t* db2;
  const uint32_t* dbm2;  // null: the database holds no X
  const uint64_t* seq_off;
  uint64_t nreads;
  uint32_t nseq;
  int32_t rw;
  int32_t W, ww, min_dinuc, max_read_length;
  int32_t win[MUSC_MAX_WINDOWS];
};

DEV uint32_t mm_read_len(const MmData& D, uint32_t r) { return D.rd[(uint64_t)r * (uint64_t)D.rw + (uint64_t)(D.rw - 1)] & 0xFFFFu; }

// code of base q of read r (q below the read's length)
DEV uint32_t mm_read_code(const MmData& D, uint32_t r, uint32_t q) {
  const uint64_t w = (uint64_t)r * (uint64_t)D.rw + (q >> 4);
  const uint32_t sh = 2u * (q & 15u);
  if (D.rdm && ((D.rdm[w] >> sh) & 1u)) return 5u;
  return ((D.rd[w] >> sh) & 3u) + 1u;
}

// code of database base b
DEV uint32_t mm_db_code(const MmData& D, uint64_t b) {
  const uint32_t sh = 2u * ((uint32_t)b & 15u);
  if (D.dbm2 && ((D.dbm2[b >> 4] >> sh) & 1u)) return 5u;
  return ((D.db2[b >> 4] >> sh) & 3u) + 1u;
}

// `valid` of the specification: the read reaches the window's end and the window passes utils/entropy.go:5-40
DEV bool mm_valid(const MmData& D, uint32_t r, int k) {
  const uint32_t q1 = (uint32_t)D.win[k], q2 = q1 + (uint32_t)D.ww;
  if (mm_read_len(D, r) < q2) return false;
  if (D.min_dinuc <= 0) return true;
  uint32_t seen = 0, last = 0;
  for (uint32_t i = 0; i < (uint32_t)D.ww; i++) {
    const uint32_t v = (0x412300u >>(4u * mm_read_code(D, r, q1 + i))) & 15u;  // A 0, T 1, G 2, C 3, X 4
    if (i) seen |= 1u << (5u * last + v);
    last = v;
  }
  return __popc(seen) >= D.min_dinuc;
}

// `emits` of the specification: would window k's confirm emit tuple h
DEV bool mm_emits(const MmData& D, uint4 h, int k) {
  if (!mm_valid(D, h.x, k)) return false;
  const int64_t q1 = D.win[k], ww = D.ww, jx = (int64_t)h.z + q1, L = mm_read_len(D, h.x);
  const uint64_t t0 = D.seq_off[h.y];
  const int64_t T = (int64_t)(D.seq_off[h.y + 1] - t0);
  if (jx + ww > T) return false;
  for (int64_t i = 0; i < ww; i++)
    if (mm_read_code(D, h.x, (uint32_t)(q1 + i)) != mm_db_code(D, t0 + (uint64_t)(jx + i))) return false;
  if (jx == 0) return L <= (100 - ww < T ? 100 - ww : T);
  return (int64_t)h.z + L <= T;
}

// (window, key) of probe a against probe b: the window number, then the key's codes
DEV int mm_block_cmp(const MmData& D, uint32_t ra, uint32_t ka, uint32_t rb, uint32_t kb) {
  if (ka != kb) return ka < kb ? -1 : 1;
  const uint32_t q1 = (uint32_t)D.win[ka];
  for (uint32_t i = 0; i < (uint32_t)D.ww; i++) {
    const uint32_t ca = mm_read_code(D, ra, q1 + i), cb = mm_read_code(D, rb, q1 + i);
    if (ca != cb) return ca < cb ? -1 : 1;
  }
  return 0;
}

struct MmProbeLess {
  MmData D;
  __device__ bool operator()(const uint2& a, const uint2& b) const {
    const int c = mm_block_cmp(D, a.x, a.y, b.x, b.y);
    return c ? c < 0 : a.x < b.x;
  }
};

// The candidate's line `left \t right \t %011d \t pos` (cmd/muscato_screen/main.go:303-316, 341-363) of (gene, pos) in
// a block of window start q1: where its flanks lie in the database.  jx = pos + q1 is the window's start in the target;
// the left flank is the q1 bases before it (jx == 0 has none, and happens at q1 == 0 only).
struct MmCand {
  uint64_t t0;       // the target's first base
  uint32_t jx;
  uint64_t right0;   // database position of the right flank
  int64_t nright;
};
DEV MmCand mm_cand(const MmData& D, uint32_t g, uint32_t pos, uint32_t q1) {
  MmCand c;
  c.t0 = D.seq_off[g];
  const int64_t T = (int64_t)(D.seq_off[g + 1] - c.t0), ww = D.ww, q2 = (int64_t)q1 + ww;
  c.jx = pos + q1;
  if (c.jx == 0) {
    c.right0 = c.t0 + (uint64_t)ww;
    c.nright = (100 - q2 < T ? 100 - q2 : T) - ww;
  } else {
    const int64_t jy = (int64_t)c.jx + ww, lim = jy + (int64_t)D.max_read_length - q2;
    c.right0 = c.t0 + (uint64_t)jy;
    c.nright = (lim < T ? lim : T) - jy;
  }
  if (c.nright < 0) c.nright = 0;
  return c;
}

// Two base strings of one pair of planes (2-bit codes, X plane or null) as texts that end at their last base: string a
// = bases [a0, a0 + na), b likewise.  Equal stretches go 32 bases at a time (both planes word for word: equal codes);
// the first difference is found base by base.  A string that ends sorts below one that goes on (the tab).
// (ext64 reads up to two words past the one it starts in: the planes are allocated with that much to spare.)
DEV int mm_span_cmp(const uint32_t* __restrict__ p2, const uint32_t* __restrict__ pm, uint64_t a0, uint64_t na, uint64_t b0, uint64_t nb) {
  const uint64_t n = na < nb ? na : nb;
  uint64_t s = 0;
  while (s + 32 <= n && ext64(p2, 2 * (a0 + s)) == ext64(p2, 2 * (b0 + s)) && (!pm || ext64(pm, 2 * (a0 + s)) == ext64(pm, 2 * (b0 + s)))) s += 32;
  for (; s < n; s++) {
    const uint64_t a = a0 + s, b = b0 + s;
    const uint32_t sa = 2u * ((uint32_t)a & 15u), sb = 2u * ((uint32_t)b & 15u);
    const uint32_t ca = pm && ((pm[a >> 4] >> sa) & 1u) ? 5u : ((p2[a >> 4] >> sa) & 3u) + 1u;
    const uint32_t cb = pm && ((pm[b >> 4] >> sb) & 1u) ? 5u : ((p2[b >> 4] >> sb) & 3u) + 1u;
    if (ca != cb) return ca < cb ? -1 : 1;
  }
  return na == nb ? 0 : na < nb ? -1 : 1;
}

DEV int mm_cand_cmp(const MmData& D, uint32_t ga, uint32_t pa, uint32_t gb, uint32_t pb, uint32_t q1) {
  if (ga == gb && pa == pb) return 0;
  const MmCand a = mm_cand(D, ga, pa, q1), b = mm_cand(D, gb, pb, q1);
  // left: q1 bases before the window (q1 > 0: jx = pos + q1 > 0, both candidates have them; q1 == 0: none)
  int c = q1 ? mm_span_cmp(D.db2, D.dbm2, a.t0 + pa, q1, b.t0 + pb, q1) : 0;
  if (c) return c;
  c = mm_span_cmp(D.db2, D.dbm2, a.right0, (uint64_t)a.nright, b.right0, (uint64_t)b.nright);
  if (c) return c;
  if (ga != gb) return ga < gb ? -1 : 1;  // %011d: text order = numeric order
  const uint64_t na = res_number_key(a.jx, 0), nb = res_number_key(b.jx, 0);  // pos as decimal text
  return na < nb ? -1 : na > nb ? 1 : 0;
}

// the read's line `key \t left \t right` (cmd/muscato/main.go:261-270) within one block: left, then right
DEV int mm_read_cmp(const MmData& D, uint32_t ra, uint32_t rb, uint32_t q1) {
  if (ra == rb) return 0;
  const uint64_t a0 = (uint64_t)ra * (uint64_t)D.rw * 16ull, b0 = (uint64_t)rb * (uint64_t)D.rw * 16ull;
  const uint32_t q2 = q1 + (uint32_t)D.ww;
  int c = q1 ? mm_span_cmp(D.rd, D.rdm, a0, q1, b0, q1) : 0;
  if (c) return c;
  c = mm_span_cmp(D.rd, D.rdm, a0 + q2, mm_read_len(D, ra) - q2, b0 + q2, mm_read_len(D, rb) - q2);
  if (c) return c;
  return ra < rb ? -1 : 1;  // (equal lines: two loaded reads with one sequence; the reference's input has none)
}

// a pair = (tuple, block): block-major, then the candidate's line, then the read's line
struct MmPairLess {
  MmData D;
  const uint4* hits;
  const uint2* blocks;
  __device__ bool operator()(const uint2& a, const uint2& b) const {
    if (a.y != b.y) return a.y < b.y;
    const uint32_t q1 = (uint32_t)D.win[blocks[a.y].y];
    const uint4 ha = hits[a.x], hb = hits[b.x];
    int c = mm_cand_cmp(D, ha.y, ha.z, hb.y, hb.z, q1);
    if (c) return c < 0;
    c = mm_read_cmp(D, ha.x, hb.x, q1);
    return c ? c < 0 : a.x < b.x;
  }
};

// ---- 1. the suspect blocks: heads of the sorted probes, compacted to one representative (read, window) per block
MUSC_KERNEL __launch_bounds__(256) void k_mm_heads(MmData D, const uint2* __restrict__ probes, uint64_t np, uint32_t* __restrict__ heads) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < np; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint2 p = probes[i];
    heads[i] = i == 0 || mm_block_cmp(D, probes[i - 1].x, probes[i - 1].y, p.x, p.y) != 0;
  }
}
MUSC_KERNEL __launch_bounds__(256) void k_mm_blocks(const uint2* __restrict__ probes, const uint32_t* __restrict__ heads,
                                                   const uint32_t* __restrict__ excl, uint64_t np, uint2* __restrict__ blocks) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < np; i += (uint64_t)gridDim.x * blockDim.x)
    if (heads[i]) blocks[excl[i]] = probes[i];
}

// ---- 2. pairs: one lane per (tuple, window).  The window's block by binary search among the suspects; a pair that
// the window emits counts for its block.
MUSC_KERNEL __launch_bounds__(256) void k_mm_pairs(MmData D, const uint4* __restrict__ hits, uint64_t n, const uint2* __restrict__ blocks,
                                                  uint32_t nb, uint32_t* __restrict__ words, uint32_t* __restrict__ cnt) {
  const uint64_t total = n * (uint64_t)D.W;
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t i = t / (uint64_t)D.W;
    const int k = (int)(t % (uint64_t)D.W);
    const uint4 h = hits[i];
    uint32_t w = MM_NONE;
    if (h.x < D.nreads && h.y < D.nseq && mm_valid(D, h.x, k)) {
      uint32_t lo = 0, hi = nb;
      while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        const uint2 b = blocks[mid];
        if (mm_block_cmp(D, b.x, b.y, h.x, (uint32_t)k) < 0) lo = mid + 1; else hi = mid;
      }
      const bool found = lo < nb && mm_block_cmp(D, blocks[lo].x, blocks[lo].y, h.x, (uint32_t)k) == 0;
      const bool em = mm_emits(D, h, k);
      w = (found ? lo : MM_BLOCK) | (em ? MM_EMITS : 0u);
      if (found && em) atomicAdd(&cnt[lo], 1u);
    }
    words[t] = w;
  }
}

// a block with at most MaxMatches pairs is a false alarm of the hashed counters: size 0 from here on.  sizes has nb + 1
// entries (the last one 0: the scan's total)
MUSC_KERNEL __launch_bounds__(256) void k_mm_sizes(const uint32_t* __restrict__ cnt, uint32_t nb, uint32_t max_matches,
                                                  uint64_t* __restrict__ sizes, unsigned long long* __restrict__ ntrunc) {
  unsigned long long c = 0;
  for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b <= nb; b += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t v = b < nb ? cnt[b] : 0u;
    const bool tr = b < nb && v > max_matches;
    sizes[b] = tr ? v : 0ull;
    c += tr;
  }
  block_add_u64(c, ntrunc);
}

// the pairs of the truncated blocks, each block's in its own range [off[b], off[b] + sizes[b]) (in any order: the sort follows)
MUSC_KERNEL __launch_bounds__(256) void k_mm_fill(const uint32_t* __restrict__ words, uint64_t n, int W, const uint64_t* __restrict__ sizes,
                                                 const uint64_t* __restrict__ off, uint32_t* __restrict__ fill, uint2* __restrict__ pairs) {
  const uint64_t total = n * (uint64_t)W;
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t w = words[t];
    if (w == MM_NONE || !(w & MM_EMITS)) continue;
    const uint32_t b = w & MM_BLOCK;
    if (b == MM_BLOCK || !sizes[b]) continue;
    const uint64_t slot = off[b] + atomicAdd(&fill[b], 1u);
    if (slot < off[b] + sizes[b]) pairs[slot] = make_uint2((uint32_t)(t / (uint64_t)W), b);
  }
}

// ---- 4. the replay: one wave per truncated block over its pairs in line order.
// "first" (cmd/muscato_confirm/main.go:233-238) appends and stops once len > MaxMatches: the first MaxMatches + 1 pairs.
// "best" is qinsert (:424-448) on (mm, pair): append, sift up while the parent has MORE mismatches, cut the array at
// MaxMatches.  The wave stages 64 mismatch counts at a time (one coalesced gather); lane 0 inserts them in order.  The
// heap holds at most MaxMatches + 1 entries: in LDS when they fit `lds_cap`, else in the block's range of `gheap` (a
// truncated block has more than MaxMatches pairs, so its range of the pair array's size is large enough).
// No lane waits for anything but its own wave's barrier.
template <class Heap>
DEV uint32_t mm_qinsert(Heap heap, uint32_t size, uint32_t max_matches, uint32_t mm, uint32_t idx) {
  uint32_t ii = size;
  while (ii > 0) {
    const uint32_t jj = (ii - 1) >> 1;
    const uint2 p = heap[jj];
    if (p.x <= mm) break;
    heap[ii] = p;
    ii = jj;
  }
  heap[ii] = make_uint2(mm, idx);
  return size + 1 > max_matches ? max_matches : size + 1;
}

MUSC_KERNEL __launch_bounds__(64) void k_mm_replay(const uint4* __restrict__ hits, const uint2* __restrict__ pairs, const uint2* __restrict__ blocks,
                                                  const uint64_t* __restrict__ sizes, const uint64_t* __restrict__ off, uint32_t nb,
                                                  int W, uint32_t max_matches, int mode_first, uint32_t lds_cap,
                                                  uint2* __restrict__ gheap, uint32_t* __restrict__ words) {
  __shared__ uint2 s_heap[musc_mm::HEAP_LDS_ENTRIES];
  __shared__ uint32_t s_mm[64];
  __shared__ uint32_t s_size;
  const uint32_t lane = threadIdx.x;
  const bool in_lds = (uint64_t)max_matches + 1 <= (uint64_t)lds_cap;
  for (uint32_t b = blockIdx.x; b < nb; b += gridDim.x) {
    const uint64_t n = sizes[b];
    if (!n) continue;
    const uint64_t o = off[b];
    const uint64_t k = blocks[b].y;
    if (mode_first) {
      const uint64_t keep = n < (uint64_t)max_matches + 1 ? n : (uint64_t)max_matches + 1;
      for (uint64_t j = lane; j < keep; j += 64) words[(uint64_t)pairs[o + j].x * (uint64_t)W + k] |= MM_KEPT;
      continue;
    }
    uint32_t size = 0;  // lane 0's
    for (uint64_t base = 0; base < n; base += 64) {
      const uint32_t m = n - base < 64 ? (uint32_t)(n - base) : 64u;
      if (lane < m) s_mm[lane] = hits[pairs[o + base + lane].x].w;
      __syncthreads();
      if (lane == 0) {
        if (in_lds) for (uint32_t j = 0; j < m; j++) size = mm_qinsert(s_heap, size, max_matches, s_mm[j], (uint32_t)base + j);
        else for (uint32_t j = 0; j < m; j++) size = mm_qinsert(gheap + o, size, max_matches, s_mm[j], (uint32_t)base + j);
      }
      __syncthreads();
    }
    if (lane == 0) s_size = size;
    __syncthreads();
    const uint32_t kept = s_size;
    for (uint32_t j = lane; j < kept; j += 64) {
      const uint32_t idx = in_lds ? s_heap[j].y : gheap[o + j].y;
      words[(uint64_t)pairs[o + idx].x * (uint64_t)W + k] |= MM_KEPT;
    }
    __syncthreads();
  }
}

// ---- 5. survivors.  A read is affected when one of its valid windows lies in a truncated block; a tuple of an affected
// read survives if some window emits it and that window's block is not truncated or kept the pair.  words == null:
// every tuple survives (no suspect block: only the per-read selection below is applied).
MUSC_KERNEL __launch_bounds__(256) void k_mm_survive(const uint4* __restrict__ hits, uint64_t n, const uint32_t* __restrict__ words, int W,
                                                    const uint64_t* __restrict__ sizes, int apply_mmtol, uint32_t* __restrict__ flags,
                                                    uint32_t* __restrict__ best) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    bool affected = false, survive = false;
    for (int k = 0; words && k < W; k++) {
      const uint32_t w = words[i * (uint64_t)W + k];
      if (w == MM_NONE) continue;
      const uint32_t b = w & MM_BLOCK;
      const bool trunc = b != MM_BLOCK && sizes[b] != 0;
      affected |= trunc;
      if (w & MM_EMITS) survive |= !trunc || (w & MM_KEPT);
    }
    const uint32_t keep = !affected || survive;
    flags[i] = keep;
    if (keep && apply_mmtol) {
      const uint4 h = hits[i];
      atomicMin(&best[h.x], h.w);
    }
  }
}

// per read keep nmiss <= best + MMTol (cmd/muscato_combine_windows/main.go:36-60)
MUSC_KERNEL __launch_bounds__(256) void k_mm_best(const uint4* __restrict__ hits, uint64_t n, const uint32_t* __restrict__ best, uint32_t mmtol,
                                                 uint32_t* __restrict__ flags) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint4 h = hits[i];
    if (flags[i] && (uint64_t)h.w > (uint64_t)best[h.x] + mmtol) flags[i] = 0;
  }
}

// the survivors in list order: the list stays read-major
MUSC_KERNEL __launch_bounds__(256) void k_mm_compact(const uint4* __restrict__ hits, uint64_t n, const uint32_t* __restrict__ flags,
                                                    const uint32_t* __restrict__ excl, uint4* __restrict__ out) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
    if (flags[i]) out[excl[i]] = hits[i];
}
