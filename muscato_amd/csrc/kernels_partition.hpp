// kernels_partition.hpp -- the merge of a partitioned pass (a database whose index is built and matched one range of
// targets at a time).  Part of libmuscato_hip.so: included by muscato_hip.hip (one translation unit).
//
// Each partition's pass leaves a read-major tuple list (a read's tuples are one contiguous run, reads increasing); the
// lists are appended to one accumulation buffer, segment after segment.  The merge then keeps, per read, the tuples
// within the GLOBAL best + MMTol (apply_mmtol; exact: a partition's own selection kept every tuple within its local
// best + MMTol, and the local best is never below the global one) and writes the survivors read-major: reads
// increasing, within a read the segments in partition order and each segment's tuples in the order its pass emitted
// them.  Every kernel streams the tuples once; the per-read words are touched once per run (the head or tail lane of
// the run), atomics only where a run meets a wave boundary.
#pragma once

#define PART_NO_READ 0xFFFFFFFFu  // lanes past the end of a list (no read index reaches it: read_idx < 2^32 - 16)

// acc[i] += src[i]: the exact MaxMatches block counters of one partition's pass added to the whole database's
MUSC_KERNEL __launch_bounds__(256) void k_add_u32(uint32_t* __restrict__ acc, const uint32_t* __restrict__ src, uint64_t n) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
    acc[i] += src[i];
}

// Segmented reduction over the RUNS of a wave: consecutive lanes that hold the same read.  Afterwards a lane holds
// op(v) over itself and the later lanes of its run within the wave; the first lane of each run (within the wave)
// returns true.  A run is named by its number within the wave, not by its read: the accumulation buffer is read-major
// per segment only, so where segments are shorter than a wave one read turns up in several runs of the same wave, with
// other reads in between, and lanes d apart that hold the same read need not belong together (counted as one run they
// added a later run's sum to an earlier one: one slot too many for the read, left unwritten in the merged list).
template <class Op>
DEV bool wave_run_reduce(uint32_t r, uint32_t& v, Op op) {
  const int lane = threadIdx.x & 63;
  const uint32_t prev = __shfl_up(r, 1);
  const bool head = lane == 0 || prev != r;
  const unsigned long long heads = __ballot(head);
  const uint32_t run = (uint32_t)__popcll(heads & ((2ull << lane) - 1ull));  // (lane 63: 2 << 63 wraps to 0, the mask to all ones)
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t ov = __shfl_down(v, d), orun = __shfl_down(run, d);
    if (lane + d < 64 && orun == run) v = op(v, ov);
  }
  return r != PART_NO_READ && head;
}

DEV bool part_keep(uint32_t nmiss, uint32_t best, uint32_t mmtol, int apply_mmtol) {
  return !apply_mmtol || nmiss <= best + mmtol;
}

// best[r] = min(best[r], fewest mismatches of read r in this segment).  (best starts at 0xFFFFFFFF)
MUSC_KERNEL __launch_bounds__(256) void k_part_best(const uint4* __restrict__ hits, uint64_t n, uint32_t* __restrict__ best) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x; b < n; b += stride) {  // (uniform per wave: every lane shuffles)
    const uint64_t i = b + threadIdx.x;
    uint32_t r = PART_NO_READ, v = 0xFFFFFFFFu;
    if (i < n) {
      const uint4 h = hits[i];
      r = h.x;
      v = h.w;
    }
    if (wave_run_reduce(r, v, [](uint32_t a, uint32_t c) { return a < c ? a : c; })) atomicMin(&best[r], v);
  }
}

// cnt[r] += tuples of read r that survive the global selection (the whole accumulation buffer in one launch)
MUSC_KERNEL __launch_bounds__(256) void k_part_count(const uint4* __restrict__ hits, uint64_t n, const uint32_t* __restrict__ best,
                                                    uint32_t mmtol, int apply_mmtol, unsigned long long* __restrict__ cnt) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x; b < n; b += stride) {
    const uint64_t i = b + threadIdx.x;
    uint32_t r = PART_NO_READ, v = 0;
    if (i < n) {
      const uint4 h = hits[i];
      r = h.x;
      v = part_keep(h.w, best[r], mmtol, apply_mmtol) ? 1u : 0u;
    }
    if (wave_run_reduce(r, v, [](uint32_t a, uint32_t c) { return a + c; }) && v) atomicAdd(&cnt[r], (unsigned long long)v);
  }
}

// flags[i] = tuple i of one segment survives; flags[n] = 0 (the exclusive scan of n + 1 flags then ends in the total)
MUSC_KERNEL __launch_bounds__(256) void k_part_flags(const uint4* __restrict__ hits, uint64_t n, const uint32_t* __restrict__ best,
                                                    uint32_t mmtol, int apply_mmtol, uint32_t* __restrict__ flags) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += (uint64_t)gridDim.x * blockDim.x) {
    uint32_t f = 0;
    if (i < n) {
      const uint4 h = hits[i];
      f = part_keep(h.w, best[h.x], mmtol, apply_mmtol) ? 1u : 0u;
    }
    flags[i] = f;
  }
}

// The first tuple of each run of one segment: adj[r] = cursor[r] - S[i], so that survivor j of the run goes to
// adj[r] + S[j] (S: the exclusive scan of the segment's flags; u64 arithmetic wraps)
MUSC_KERNEL __launch_bounds__(256) void k_part_head(const uint4* __restrict__ hits, uint64_t n, const uint32_t* __restrict__ S,
                                                   const uint64_t* __restrict__ cursor, uint64_t* __restrict__ adj) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t r = hits[i].x;
    if (i == 0 || hits[i - 1].x != r) adj[r] = cursor[r] - (uint64_t)S[i];
  }
}

// The survivors of one segment to their places; the last tuple of each run moves the read's cursor past them
MUSC_KERNEL __launch_bounds__(256) void k_part_scatter(const uint4* __restrict__ hits, uint64_t n, const uint32_t* __restrict__ S,
                                                      const uint64_t* __restrict__ adj, uint64_t* __restrict__ cursor,
                                                      uint4* __restrict__ out, uint64_t out_cap, uint32_t* __restrict__ bad) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint4 h = hits[i];
    const uint64_t a = adj[h.x];
    const uint32_t s0 = S[i], s1 = S[i + 1];
    if (s1 != s0) {
      const uint64_t pos = a + (uint64_t)s0;
      if (pos < out_cap) out[pos] = h;
      else atomicOr(bad, 1u);
    }
    if (i + 1 == n || hits[i + 1].x != h.x) cursor[h.x] = a + (uint64_t)s1;
  }
}
