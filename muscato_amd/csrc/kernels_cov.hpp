// kernels_cov.hpp -- coverage from the resident tuples: bedGraph depth runs and a per-target summary.
// Part of libmuscato_hip.so: included by muscato_hip.hip (one translation unit), after kernels_sam.hpp, whose name
// kernels (k_sam_gnames, k_sam_runs) and byte picker (SamPick, SAM_LIT) it uses.
//
// A per-base difference array would cost four bytes per database base; the stage sorts events instead, so its memory
// is proportional to the lines.  Every line emits two events, (slot(f, a), +w) and (slot(f, a + S), -w); the events
// are sorted by slot (KeyPasses), the deltas summed in sorted order (scan_u32, modulo 2^32), and the partial sum at
// the last event of every group of equal slots is the depth from that slot on -- exact, because the total weight is
// below 2^32.  Group ends, then the group ends at which the depth changes (breakpoints), then the breakpoints of
// non-zero depth (runs) are compacted by scans; the run's end is the next breakpoint's slot.  The summary is prefix
// sums over the runs taken at the target boundaries, and integer atomics per target (order-independent).  The size
// rules are cov_plan.hpp's.  Grid-stride kernels are a lane per item; the two render kernels are a wave per record
// (wave_id, wave_store: kernels_results.hpp).  No LDS, nothing waits on another workgroup.
#pragma once

#include "cov_plan.hpp"

struct CovData {
  ResData R;
  const uint2* gname;    // per gene: x = first byte of the RNAME token within its text, y = its bytes
  const uint32_t* rank;  // per gene: RES_ABSENT without an id line
  uint32_t flags;        // MUSC_COV_*
};

// ---- events -------------------------------------------------------------------------------------------------------------
// Line i -> events 2 i (+w at the interval's first slot) and 2 i + 1 (-w at the slot behind its last base).  A line
// that does not contribute (MUSC_COV_UNIQUE, and its read has more lines than one) emits zero deltas.  nreads_t[f] +=
// w, *total += w (64 bits: the refusal is decided from it); *bad is raised by a tuple that does not fit the reads and
// the database in hand, whose events are (0, 0).
MUSC_KERNEL __launch_bounds__(256) void k_cov_events(const uint4* __restrict__ hits, uint64_t m, CovData D, const uint32_t* __restrict__ first,
                                                    const uint32_t* __restrict__ last, uint64_t* __restrict__ evkey,
                                                    uint32_t* __restrict__ evdelta, uint32_t* __restrict__ nreads_t,
                                                    unsigned long long* __restrict__ total, uint32_t* __restrict__ bad) {
  unsigned long long mine = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint4 h = hits[i];
    uint64_t k0 = 0, k1 = 0, w = 0;
    const bool fits = (uint64_t)h.x < D.R.nreads && h.y < D.R.nseq;
    const uint64_t t0 = fits ? D.R.seq_off[h.y] : 0, len = fits ? D.R.seq_off[h.y + 1] - t0 : 0;
    if (!fits || (uint64_t)h.z > len) {
      *bad = 1u;
    } else {
      const uint64_t L = D.R.rd[(uint64_t)h.x * (uint64_t)D.R.rw + (uint64_t)(D.R.rw - 1)] & 0xFFFFu;
      const musc_cov::Interval v = musc_cov::interval((D.flags & MUSC_COV_REV_PAIRS) != 0u, h.y, h.z, len, L);
      const uint64_t base = D.R.seq_off[v.f];
      k0 = musc_cov::slot(base, v.f, v.a);
      k1 = musc_cov::slot(base, v.f, v.a + v.S);
      w = 1;
      if ((D.flags & MUSC_COV_WEIGHTED) && D.R.ttext) {
        const uint64_t a = D.R.toff[h.x];
        w = musc_cov::weight(reinterpret_cast<const unsigned char*>(D.R.ttext) + a, D.R.toff[h.x + 1] - a);
      }
      if ((D.flags & MUSC_COV_UNIQUE) && first[h.x] != last[h.x]) w = 0;
      if (w) atomicAdd(nreads_t + v.f, (uint32_t)w);  // (modulo 2^32: read only when the total is below it)
      mine += w;
    }
    evkey[2 * i] = k0;
    evkey[2 * i + 1] = k1;
    evdelta[2 * i] = (uint32_t)w;
    evdelta[2 * i + 1] = 0u - (uint32_t)w;
  }
  for (int d = 32; d; d >>= 1) mine += __shfl_xor(mine, d);
  if ((threadIdx.x & 63u) == 0u && mine) atomicAdd(total, mine);
}

// keys[i] = the slot of event order[i]: what KeyPasses sorts
MUSC_KERNEL __launch_bounds__(256) void k_cov_keys(const uint32_t* __restrict__ order, const uint64_t* __restrict__ evkey, uint64_t n,
                                                  uint64_t* __restrict__ keys) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) keys[i] = evkey[order[i]];
}

// In sorted order: delta[i] = the delta of the i-th event, isend[i] = it is the last event of its slot; isend[n] = 0
MUSC_KERNEL __launch_bounds__(256) void k_cov_gather(const uint32_t* __restrict__ order, const uint64_t* __restrict__ evkey,
                                                    const uint32_t* __restrict__ evdelta, uint64_t n, uint32_t* __restrict__ delta,
                                                    uint32_t* __restrict__ isend) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += (uint64_t)gridDim.x * blockDim.x) {
    if (i == n) {
      isend[i] = 0u;
      continue;
    }
    const uint32_t e = order[i];
    delta[i] = evdelta[e];
    isend[i] = i + 1 == n || evkey[order[i + 1]] != evkey[e] ? 1u : 0u;
  }
}

// Group j = the j-th slot that has events: its depth (the inclusive sum at its last event), its slot and a line of it
MUSC_KERNEL __launch_bounds__(256) void k_cov_groups(const uint32_t* __restrict__ order, const uint64_t* __restrict__ evkey,
                                                    const uint32_t* __restrict__ isend, const uint32_t* __restrict__ gidx,
                                                    const uint32_t* __restrict__ incl, uint64_t n, uint32_t* __restrict__ gdepth,
                                                    uint64_t* __restrict__ gkey, uint32_t* __restrict__ gline) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    if (!isend[i]) continue;
    const uint32_t j = gidx[i], e = order[i];
    gdepth[j] = incl[i];
    gkey[j] = evkey[e];
    gline[j] = e >> 1;
  }
}

// isbreak[j] = the depth from group j on differs from the depth before it; isbreak[ng] = 0
MUSC_KERNEL __launch_bounds__(256) void k_cov_breaks(const uint32_t* __restrict__ gdepth, uint64_t ng, uint32_t* __restrict__ isbreak) {
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j <= ng; j += (uint64_t)gridDim.x * blockDim.x)
    isbreak[j] = j < ng && gdepth[j] != (j ? gdepth[j - 1] : 0u) ? 1u : 0u;
}

// Breakpoint b = the b-th group at which the depth changes; isrun[b] = its depth is not zero; isrun[nb] = 0 (the caller
// has cleared it)
MUSC_KERNEL __launch_bounds__(256) void k_cov_break_list(const uint32_t* __restrict__ isbreak, const uint32_t* __restrict__ bidx,
                                                        const uint32_t* __restrict__ gdepth, const uint64_t* __restrict__ gkey,
                                                        const uint32_t* __restrict__ gline, uint64_t ng, uint32_t* __restrict__ bdepth,
                                                        uint64_t* __restrict__ bkey, uint32_t* __restrict__ bline, uint32_t* __restrict__ isrun) {
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < ng; j += (uint64_t)gridDim.x * blockDim.x) {
    if (!isbreak[j]) continue;
    const uint32_t b = bidx[j];
    bdepth[b] = gdepth[j];
    bkey[b] = gkey[j];
    bline[b] = gline[j];
    isrun[b] = gdepth[j] != 0u ? 1u : 0u;
  }
}

// Run j = the j-th breakpoint of non-zero depth, up to the next breakpoint (which is in the same target: the depth is
// zero behind a target's last event).  The target comes from the breakpoint's line.  rlen / rarea / rbytes [j] = the
// run's bases, bases x depth and record bytes, [nruns] = 0; maxdepth[f] by atomicMax.
MUSC_KERNEL __launch_bounds__(256) void k_cov_runs(const uint4* __restrict__ hits, CovData D, const uint32_t* __restrict__ isrun,
                                                  const uint32_t* __restrict__ ridx, const uint32_t* __restrict__ bdepth,
                                                  const uint64_t* __restrict__ bkey, const uint32_t* __restrict__ bline, uint64_t nb, uint64_t nruns,
                                                  uint32_t* __restrict__ run_f, uint32_t* __restrict__ run_d, uint64_t* __restrict__ run_s,
                                                  uint64_t* __restrict__ run_e, uint64_t* __restrict__ rlen, uint64_t* __restrict__ rarea,
                                                  uint64_t* __restrict__ rbytes, uint32_t* __restrict__ maxdepth, uint32_t* __restrict__ bad) {
  for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b <= nb; b += (uint64_t)gridDim.x * blockDim.x) {
    if (b == nb) {
      rlen[nruns] = rarea[nruns] = rbytes[nruns] = 0;
      continue;
    }
    if (!isrun[b]) continue;
    const uint32_t j = ridx[b], g = hits[bline[b]].y;  // (the tuple passed k_cov_events' test)
    const uint32_t f = (D.flags & MUSC_COV_REV_PAIRS) && (g & 1u) ? g - 1u : g;
    const uint64_t base = D.R.seq_off[f] + f, len = D.R.seq_off[f + 1] - D.R.seq_off[f];
    const uint64_t s = bkey[b] - base, e = b + 1 < nb ? bkey[b + 1] - base : 0;
    const uint32_t d = bdepth[b];
    const bool ok = j < nruns && bkey[b] >= base && s < e && e <= len;
    if (!ok) *bad = 1u;
    if (j >= nruns) continue;
    run_f[j] = f;
    run_d[j] = d;
    run_s[j] = ok ? s : 0;
    run_e[j] = ok ? e : 0;
    rlen[j] = ok ? e - s : 0;
    rarea[j] = ok ? (e - s) * d : 0;
    rbytes[j] = ok ? musc_cov::run_bytes(D.gname[f].y, s, e, d) : 0;
    atomicMax(maxdepth + f, d);
  }
}

// The runs are sorted by target: b0[f] / b1[f] = the first run of target f and the one behind its last (both 0, as the
// caller has cleared them, for a target without a run)
MUSC_KERNEL __launch_bounds__(256) void k_cov_bounds(const uint32_t* __restrict__ run_f, uint64_t nruns, uint32_t* __restrict__ b0,
                                                    uint32_t* __restrict__ b1) {
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < nruns; j += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t f = run_f[j];
    if (j == 0 || run_f[j - 1] != f) b0[f] = (uint32_t)j;
    if (j + 1 == nruns || run_f[j + 1] != f) b1[f] = (uint32_t)j + 1u;
  }
}

DEV bool cov_has_line(const CovData& D, uint32_t t) { return D.rank[t] != RES_ABSENT && !((D.flags & MUSC_COV_REV_PAIRS) && (t & 1u)); }

// Per target: covbases and sumdepth as differences of the prefix sums over the runs, and whether the summary has a
// record for it; has[nseq] = 0
MUSC_KERNEL __launch_bounds__(256) void k_cov_targets(CovData D, const uint32_t* __restrict__ b0, const uint32_t* __restrict__ b1,
                                                     const uint64_t* __restrict__ plen, const uint64_t* __restrict__ parea,
                                                     uint64_t* __restrict__ covbases, uint64_t* __restrict__ sumdepth, uint32_t* __restrict__ has) {
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t <= D.R.nseq; t += (uint64_t)gridDim.x * blockDim.x) {
    if (t == D.R.nseq) {
      has[t] = 0u;
      continue;
    }
    covbases[t] = plen[b1[t]] - plen[b0[t]];
    sumdepth[t] = parea[b1[t]] - parea[b0[t]];
    has[t] = cov_has_line(D, (uint32_t)t) ? 1u : 0u;
  }
}

struct CovSummary {
  const uint32_t* target;  // per record: its target
  const uint32_t *numreads, *maxdepth;  // per target
  const uint64_t *covbases, *sumdepth;
};

DEV uint64_t cov_summary_bytes(const CovData& D, const CovSummary& S, uint32_t t) {
  return musc_cov::summary_bytes(D.gname[t].y, D.R.seq_off[t + 1] - D.R.seq_off[t], S.numreads[t], S.covbases[t], S.sumdepth[t], S.maxdepth[t]);
}

// Summary record k = the k-th target with a line: target[k] and its bytes; sbytes[nt] = 0
MUSC_KERNEL __launch_bounds__(256) void k_cov_target_list(CovData D, CovSummary S, const uint32_t* __restrict__ has, const uint32_t* __restrict__ tidx,
                                                         uint64_t nt, uint32_t* __restrict__ target, uint64_t* __restrict__ sbytes) {
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t <= D.R.nseq; t += (uint64_t)gridDim.x * blockDim.x) {
    if (t == D.R.nseq) {
      sbytes[nt] = 0;
      continue;
    }
    if (!has[t]) continue;
    const uint32_t k = tidx[t];
    if (k >= nt) continue;
    target[k] = (uint32_t)t;
    sbytes[k] = cov_summary_bytes(D, S, (uint32_t)t);
  }
}

// ---- the render kernels -----------------------------------------------------------------------------------------------
// Records [r0, r1) of the bedGraph into `out`, record j at byte off[j] - off[r0]; one wave per record.  A record whose
// length disagrees with its offsets, or whose name does not lie in its gene's text, is not rendered and fails the call
// through *flag.
MUSC_KERNEL __launch_bounds__(256) void k_cov_render(const uint32_t* __restrict__ run_f, const uint32_t* __restrict__ run_d,
                                                    const uint64_t* __restrict__ run_s, const uint64_t* __restrict__ run_e,
                                                    const uint64_t* __restrict__ off, uint64_t r0, uint64_t r1, CovData D,
                                                    unsigned char* __restrict__ out, uint32_t* __restrict__ flag) {
  const WaveId w = wave_id(threadIdx.x, blockIdx.x, blockDim.x, gridDim.x);
  const uint64_t base = off[r0];
  for (uint64_t j = r0 + w.wave; j < r1; j += w.nwaves) {
    const uint32_t f = __builtin_amdgcn_readfirstlane(run_f[j]), d = __builtin_amdgcn_readfirstlane(run_d[j]);
    const uint64_t s = run_s[j], e = run_e[j], total = off[j + 1] - off[j];
    if (f >= D.R.nseq) {
      if (w.lane == 0) *flag = 1u;
      continue;
    }
    const uint2 nm = D.gname[f];
    const uint64_t g0 = D.R.goff[f], G = D.R.goff[f + 1] - g0;
    if (total != musc_cov::run_bytes(nm.y, s, e, d) || (uint64_t)nm.x + nm.y > G) {
      if (w.lane == 0) *flag = 1u;
      continue;
    }
    const char* const name = D.R.gtext + g0 + nm.x;
    wave_store(out + (off[j] - base), total, w.lane, [&](uint64_t k) -> uint32_t {
      SamPick q(k);
      q.text(name, nm.y);
      q.lit(SAM_LIT("\t"));
      q.num64(s);
      q.lit(SAM_LIT("\t"));
      q.num64(e);
      q.lit(SAM_LIT("\t"));
      q.num(d);
      return q.out;  // (the newline is what is left)
    });
  }
}

// Records [r0, r1) of the summary, likewise
MUSC_KERNEL __launch_bounds__(256) void k_cov_sum_render(CovSummary S, const uint64_t* __restrict__ off, uint64_t r0, uint64_t r1, CovData D,
                                                        unsigned char* __restrict__ out, uint32_t* __restrict__ flag) {
  const WaveId w = wave_id(threadIdx.x, blockIdx.x, blockDim.x, gridDim.x);
  const uint64_t base = off[r0];
  for (uint64_t k = r0 + w.wave; k < r1; k += w.nwaves) {
    const uint32_t t = __builtin_amdgcn_readfirstlane(S.target[k]);
    const uint64_t total = off[k + 1] - off[k];
    if (t >= D.R.nseq) {
      if (w.lane == 0) *flag = 1u;
      continue;
    }
    const uint2 nm = D.gname[t];
    const uint64_t g0 = D.R.goff[t], G = D.R.goff[t + 1] - g0;
    if (total != cov_summary_bytes(D, S, t) || (uint64_t)nm.x + nm.y > G) {
      if (w.lane == 0) *flag = 1u;
      continue;
    }
    const char* const name = D.R.gtext + g0 + nm.x;
    const uint64_t len = D.R.seq_off[t + 1] - D.R.seq_off[t], cb = S.covbases[t], sd = S.sumdepth[t];
    const uint32_t nr = S.numreads[t], md = S.maxdepth[t];
    wave_store(out + (off[k] - base), total, w.lane, [&](uint64_t i) -> uint32_t {
      SamPick q(i);
      q.text(name, nm.y);
      q.lit(SAM_LIT("\t"));
      q.num64(len);
      q.lit(SAM_LIT("\t"));
      q.num(nr);
      q.lit(SAM_LIT("\t"));
      q.num64(cb);
      q.lit(SAM_LIT("\t"));
      q.num64(sd);
      q.lit(SAM_LIT("\t"));
      q.num(md);
      return q.out;  // (the newline is what is left)
    });
  }
}
