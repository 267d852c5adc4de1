// index_plan.hpp -- the decisions of the index layer: the shape of each bucket table, what each layout
// takes in device memory, the cascade context -> line -> 64-byte buckets, and the partition cuts.  Plain C++, no HIP:
// included by muscato_hip.hip (muscato_index.hpp acts on what is decided here, for the builds and the planner alike)
// and by host/index_plan_check.cpp, the stand-alone program that runs it under the sanitizers.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace musc_index {

// The bucket layout of an index, with the values of musc_stats.index_kind
enum Kind : uint32_t { K_CLASSIC64 = 0, K_CTX = 1, K_CTXW = 2, K_LINES = 3 };
inline bool is_ctx(Kind k) { return k == K_CTX || k == K_CTXW; }

// MUSC_INDEX: the two-kernel path, on the usual / the line / the 64-byte layout
enum { IDX_AUTO = 0, IDX_CLASSIC, IDX_LINES, IDX_CLASSIC64 };
// The knobs the decisions read (EnvKnobs fills them in)
struct Knobs {
  int index = IDX_AUTO;      // MUSC_INDEX
  int index_bits = 0;        // MUSC_DEBUG_INDEX_BITS (0: not set)
  bool ctx_direct = false;   // MUSC_DEBUG_CTX_DIRECT
  long index_budget_mb = 0;  // MUSC_DEBUG_INDEX_BUDGET_MB
};

// bytes of a bucket and of an overflow entry per layout (muscato_index.hpp holds them against the structs)
constexpr uint64_t BUCKET_BYTES = 64, LINE_BUCKET_BYTES = 128, ENTRY_BYTES = 16;
constexpr uint64_t CTX_BUCKET_BYTES = 128, CTX_ENTRY_BYTES = 40, CTX_ENTRYW_BYTES = 60;
inline uint64_t bucket_bytes(Kind k) { return k == K_CLASSIC64 ? BUCKET_BYTES : k == K_LINES ? LINE_BUCKET_BYTES : CTX_BUCKET_BYTES; }

// The index a pass asks for, and the one in hand: compared as one value.  ww == 0: none.
struct Resident {
  Kind kind = K_CLASSIC64;
  int ww = 0, CL = 0, bits = 0, direct = 0;  // CL: bases of left context (context buckets), else 0
  uint32_t g0 = 0, g1 = 0;                   // the targets covered: the whole database or one partition
  bool operator==(const Resident& o) const {
    return kind == o.kind && ww == o.ww && CL == o.CL && bits == o.bits && direct == o.direct && g0 == o.g0 && g1 == o.g1;
  }
};

struct Table {
  int bits, direct;
};
// The window-start table for width ww over `bases` bases: direct addressing (bucket = the 2*ww-bit key itself: exact,
// and bytewise-sorted reads walk the table front to back) when that table is at most 32x the database and at most
// 2^30 buckets (64 GiB; line buckets: 128 GiB); otherwise a hashed table with about one bucket per base, at most 2^31
// buckets (128 GiB; longer lists go to the overflow array).
// The context-bucket table: 4^ww buckets with the key as the bucket (exact) when that is at most twice the database's
// window count; else about one bucket per base under a 64-bit mix, at most 2^30 (a colliding key fails the window
// comparison in k_match: the context includes the window bases).
inline Table table_for(const Knobs& k, bool ctx, int32_t ww, uint64_t bases) {
  const int cap = ctx ? 30 : 31;
  const bool small = ctx ? (1ull << std::min(2 * ww, 30)) <= 2 * std::max<uint64_t>(bases, 1ull << 9) || k.ctx_direct  // (tests)
                         : (1ull << std::min(2 * ww, 30)) <= 32 * std::max<uint64_t>(bases, 1ull << 19);
  Table t{2 * ww, 1};
  if (2 * ww > 30 || !small) {
    t = Table{10, 0};
    while (t.bits < cap && (1ull << t.bits) < bases) t.bits++;
  }
  if (k.index_bits >= 8 && k.index_bits <= cap) t = Table{k.index_bits, 0};  // experiments only: force a hashed table size
  return t;
}

// What a table of 2^bits buckets over `bases` bases takes (the fit checks and the planner), and what is left to the
// pass's buffers beside it.  Line buckets: the table, the entries beyond the seventh in runs of eight (assume every
// bucket wastes half a run), 8 B per bucket of build temporaries; 12 GiB reserve.  64-byte buckets: the table, its
// build temporaries and at most one overflow entry per base; 4 GiB.  Context buckets: the table, 8 B + 4 B per bucket
// of build temporaries, and the overflow entries (their number is known only after the counting pass: assume a third
// of the windows, half on wide buckets); 4 GiB.
inline uint64_t index_need(Kind k, int bits, uint64_t bases) {
  const uint64_t nb = 1ull << bits;
  if (k == K_LINES) return (nb + 1) * (LINE_BUCKET_BYTES + 8) + (bases > 7 * nb ? (bases - 7 * nb) * ENTRY_BYTES : 0) + nb * 64;
  if (k == K_CLASSIC64) return (nb + 1) * (BUCKET_BYTES + 16) + bases * ENTRY_BYTES;
  return (nb + 1) * (CTX_BUCKET_BYTES + 12) + (k == K_CTXW ? bases / 2 * CTX_ENTRYW_BYTES : bases / 3 * CTX_ENTRY_BYTES);
}
inline uint64_t index_reserve(Kind k) { return k == K_LINES ? 12ull << 30 : 4ull << 30; }
// `avail`: the free device memory plus what the resident tables hold; MUSC_DEBUG_INDEX_BUDGET_MB caps what is left of
// it after the reserves (tests of the planner on small databases)
inline bool index_fits(const Knobs& k, Kind kind, int bits, uint64_t bases, uint64_t avail, uint64_t extra) {
  const uint64_t reserve = index_reserve(kind) + extra;
  uint64_t room = avail > reserve ? avail - reserve : 0;
  if (k.index_budget_mb > 0) room = std::min<uint64_t>(room, (uint64_t)k.index_budget_mb << 20);
  return index_need(kind, bits, bases) <= room;
}

// The cascade: the index a run builds over `bases` bases.  Context buckets (wide or not) when the run is eligible
// (ctx_ok) and they fit `avail` less their reserve and `extra`; else line buckets (LineBucket: a 128-byte line of seven
// entries + aligned overflow runs) when the direct table has four or more window starts per key on average, has at
// most 2^30 lines and fits, or MUSC_INDEX=lines asks for them; else 64-byte buckets (also: MUSC_INDEX=classic64).
// `fits`: the kind named fits; with need_fit = false the window-start kinds are not held to it.
struct Plan {
  Kind kind;
  int bits, direct;
  bool fits;
};
inline Plan cascade(const Knobs& k, int32_t ww, bool ctx_ok, bool wide, uint64_t bases, uint64_t avail, uint64_t extra, bool need_fit) {
  if (ctx_ok) {
    const Kind kind = wide ? K_CTXW : K_CTX;
    const Table t = table_for(k, true, ww, bases);
    if (index_fits(k, kind, t.bits, bases, avail, extra)) return Plan{kind, t.bits, t.direct, true};
  }
  const Table t = table_for(k, false, ww, bases);
  const bool lines = t.bits <= 30 && (k.index == IDX_LINES || (k.index != IDX_CLASSIC64 && t.direct && bases >= 4 * (1ull << t.bits) &&
                                                               index_fits(k, K_LINES, t.bits, bases, avail, extra)));
  const Kind kind = lines ? K_LINES : K_CLASSIC64;
  return Plan{kind, t.bits, t.direct, !need_fit || index_fits(k, kind, t.bits, bases, avail, extra)};
}

// ---- partitions
constexpr uint32_t MAX_PARTITIONS = 4096;

// Cut the targets (off: nseq + 1 ascending base offsets) into ranges of at most `limit` bases, greedily from the front
// (a target longer than that is a range of its own); returns false beyond MAX_PARTITIONS ranges
inline bool cut_targets(const std::vector<uint64_t>& off, uint64_t limit, std::vector<uint32_t>* first, uint64_t* largest) {
  const uint32_t nseq = (uint32_t)off.size() - 1;
  limit = std::min(limit, off[nseq]);
  first->assign(1, 0u);
  *largest = 0;
  uint32_t g = 0;
  while (g < nseq) {
    // the last boundary within `limit` bases of target g's start
    uint32_t g1 = (uint32_t)(std::upper_bound(off.begin() + g + 1, off.end(), off[g] + limit) - off.begin()) - 1;
    if (g1 <= g) g1 = g + 1;
    *largest = std::max<uint64_t>(*largest, off[g1] - off[g]);
    first->push_back(g1);
    if (first->size() > MAX_PARTITIONS + 1) return false;
    g = g1;
  }
  return true;
}

// The fewest shares n in 2 .. MAX_PARTITIONS of about equal bases whose cut is accepted -- fits(largest range) -- by a
// binary search over n.  Returns n and leaves its cut in first / largest; 0 when no n is accepted.
template <class Fits>
uint32_t fewest_partitions(const std::vector<uint64_t>& off, Fits fits, std::vector<uint32_t>* first, uint64_t* largest) {
  uint32_t lo = 2, hi = MAX_PARTITIONS, found = 0;
  while (lo <= hi) {
    const uint32_t n = lo + (hi - lo) / 2;
    std::vector<uint32_t> f;
    uint64_t lg = 0;
    if (cut_targets(off, (off.back() + n - 1) / n, &f, &lg) && fits(lg)) {
      first->swap(f);
      *largest = lg;
      found = n;
      hi = n - 1;
    } else {
      lo = n + 1;
    }
  }
  return found;
}

}  // namespace musc_index
