// kernels_read_names.hpp -- the kernels of the read-name stage, gfx950.  Each is a grid-stride loop that
// hands a lane its item and calls one function of read_names_lanes.hpp or read_names_keys.hpp, where everything a lane
// computes is written in plain C++ and held to the reference on the CPU item by item (host/read_names_plan_check.cpp).
// The render kernels run one wave per record in the shape of k_results_render (kernels_results.hpp): each lane stores
// its own dwords and bytes (lane_store).  No kernel uses shared memory, a barrier or a cross-lane operation, and none
// has a loop whose trip count is device data without a constant of the plan above it; k_rn_pairs alone has an atomic,
// one atomicMax of a clipped length per member of a larger group.
//
// The members of the groups above WAVE_GROUP_MAX are ordered by key_passes() stable passes of KeyPasses (the sort of
// the reads, muscato_prep.hpp); k_rn_keys makes the keys of a pass.  The driver is muscato_read_names.hpp.
#pragma once

#include "read_names_keys.hpp"

#define RN_GRID_STRIDE(i, n) \
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (uint64_t)gridDim.x * blockDim.x)

// gid[i] = the group of place i
MUSC_KERNEL __launch_bounds__(256) void k_rn_gid(const uint32_t* __restrict__ ustart, uint32_t nu, uint64_t n, uint32_t* __restrict__ gid) {
  RN_GRID_STRIDE(i, n) gid[i] = musc_rn::place_group(ustart, nu, i);
}

// meta[i] = the clipped length and the token length of kept read i
MUSC_KERNEL __launch_bounds__(256) void k_rn_measure(musc_rn::TextBytes rd, musc_rn::Names N, uint32_t* __restrict__ meta) {
  RN_GRID_STRIDE(i, N.n) meta[i] = musc_rn::measure_item(rd, N, i);
}

// the groups of up to WAVE_GROUP_MAX members ranked by counting; flag[i] = 1: place i is left for the key passes
MUSC_KERNEL __launch_bounds__(256) void k_rn_rank(musc_rn::TextBytes rd, musc_rn::Names N, const uint32_t* __restrict__ order,
                                                 const uint32_t* __restrict__ ustart, const uint32_t* __restrict__ gid,
                                                 uint32_t* __restrict__ ranked, uint32_t* __restrict__ flag) {
  RN_GRID_STRIDE(i, N.n) flag[i] = musc_rn::rank_item(rd, N, order, ustart, gid[i], i, ranked);
}

// the (group, kept read) pairs of the flagged places, and the longest clipped name among them
MUSC_KERNEL __launch_bounds__(256) void k_rn_pairs(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ excl,
                                                  const uint32_t* __restrict__ order, const uint32_t* __restrict__ gid, musc_rn::Names N,
                                                  uint2* __restrict__ pairs, uint32_t* __restrict__ place, uint32_t* __restrict__ max_clip) {
  RN_GRID_STRIDE(i, N.n) {
    musc_rn::pairs_item(flag, excl, order, gid[i], i, pairs, place);
    if (flag[i]) atomicMax(max_clip, musc_rn::clipped_len(N.name_len[order[i]]));
  }
}

// keys[k] = the key of pair perm[k] for pass `pass` of W + 2
MUSC_KERNEL __launch_bounds__(256) void k_rn_keys(musc_rn::TextBytes rd, musc_rn::Names N, const uint2* __restrict__ pairs,
                                                 const uint32_t* __restrict__ perm, uint64_t np, uint32_t pass, uint32_t W,
                                                 uint64_t* __restrict__ keys) {
  RN_GRID_STRIDE(k, np) keys[k] = musc_rn::sortkey(rd, N, pairs, perm, k, pass, W);
}

// the ordered pairs back into their groups' places
MUSC_KERNEL __launch_bounds__(256) void k_rn_unpairs(const uint2* __restrict__ pairs, const uint32_t* __restrict__ perm,
                                                    const uint32_t* __restrict__ place, uint64_t np, uint32_t* __restrict__ ranked) {
  RN_GRID_STRIDE(k, np) musc_rn::unpairs_by_perm(pairs, perm, place, k, ranked);
}

// per group: the token starts, the join's length, and the bytes of its record and of its line
MUSC_KERNEL __launch_bounds__(256) void k_rn_sizes(const uint32_t* __restrict__ ranked, const uint32_t* __restrict__ ustart,
                                                  const uint32_t* __restrict__ meta, const uint32_t* __restrict__ seq_len, uint64_t nu,
                                                  uint32_t* __restrict__ tstart, uint32_t* __restrict__ gsum, uint64_t* __restrict__ rec_bytes,
                                                  uint64_t* __restrict__ line_bytes) {
  RN_GRID_STRIDE(g, nu) {
    const musc_rn::GroupSizes z = musc_rn::sizes_item(ranked, ustart, meta, seq_len, g, tstart, gsum);
    rec_bytes[g] = z.record;
    line_bytes[g] = z.line;
  }
}

// ---- the renders: one wave per record, records [r0, r1) at out
MUSC_KERNEL __launch_bounds__(256) void k_rn_records(musc_rn::TextBytes rd, musc_rn::Names N, musc_rn::Groups G, const uint64_t* __restrict__ off,
                                                    uint64_t r0, uint64_t r1, unsigned char* __restrict__ out) {
  const WaveId w = wave_id(threadIdx.x, blockIdx.x, blockDim.x, gridDim.x);
  for (uint64_t g = r0 + w.wave; g < r1; g += w.nwaves) musc_rn::record_item(rd, N, G, off, r0, g, w.lane, out);
}
MUSC_KERNEL __launch_bounds__(256) void k_rn_copy(const char* __restrict__ ttext, const uint64_t* __restrict__ toff, uint64_t r0, uint64_t r1,
                                                 unsigned char* __restrict__ out) {
  const WaveId w = wave_id(threadIdx.x, blockIdx.x, blockDim.x, gridDim.x);
  for (uint64_t g = r0 + w.wave; g < r1; g += w.nwaves) musc_rn::copy_item(ttext, toff, r0, g, w.lane, out);
}
MUSC_KERNEL __launch_bounds__(256) void k_rn_lines(musc_rn::Reads S, const char* __restrict__ ttext, const uint64_t* __restrict__ toff,
                                                  const uint64_t* __restrict__ off, uint64_t r0, uint64_t r1, unsigned char* __restrict__ out) {
  const WaveId w = wave_id(threadIdx.x, blockIdx.x, blockDim.x, gridDim.x);
  for (uint64_t g = r0 + w.wave; g < r1; g += w.nwaves) musc_rn::line_item(S, ttext, toff, off, r0, g, w.lane, out);
}
