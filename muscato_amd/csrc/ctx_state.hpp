// ctx_state.hpp -- what in a context is still valid.  Every cause that can outdate something bumps one
// generation counter, at one place; everything derived carries a stamp of the generations it was made from and is
// valid exactly while the stamp equals the current ones.  The questions the entry points ask are the predicates at the
// end.  Plain C++, no HIP: included by muscato_hip.hip and by host/ctx_state_check.cpp, the stand-alone program that
// holds it against the six booleans it replaced.
#pragma once

#include <cstdint>

#include "../../include/muscato_hip.h"

namespace musc_state {

// (all start at 1: a stamp of zeros was never made)
struct Gens {
  uint64_t reads = 1;        // drop_reads
  uint64_t db = 1;           // free_db
  uint64_t gtext = 1;        // drop_gene_text: a musc_results_set_gene_text whose arguments passed, and free_db
  uint64_t ttext = 1;        // drop_read_text: musc_results_set_read_text likewise, and drop_reads
  uint64_t list = 1;         // the resident tuple list changes: every musc_match_device, the replay's first write
  uint64_t order = 1;        // every musc_results_order
  uint64_t pass_inputs = 1;  // reads, database or index changed: what the caches of a pass were made from
};

enum Origin { LIST_NONE = 0, LIST_PASS, LIST_REPLAYED };  // who left the resident list: nobody (or half of it), a pass, the replay

enum SideRefusal { SIDE_OK = 0, SIDE_NO_ORDER, SIDE_PASS_AFTER, SIDE_NO_READ_TEXT, SIDE_FORM, SIDE_TOO_MANY_READS };

struct State {
  Gens g;
  struct { uint64_t reads = 0, db = 0; Origin origin = LIST_NONE; } list;                              // `hits`
  struct Ordered { uint64_t reads = 0, db = 0, gtext = 0, ttext = 0, list = 0, order = 0; } ordered;  // res_hits / res_off
  uint64_t tokens = 0;  // side_tok: the ttext it was cut from
  uint64_t side = 0;    // the side tables: the order they describe
  uint64_t sam = 0;     // the SAM tables: the order they describe
  uint64_t cov = 0;     // the coverage tables: the order they describe

  // ---- the causes
  void reads_dropped() { g.reads++, g.pass_inputs++; }
  void db_freed() { g.db++, g.pass_inputs++; }
  void index_freed() { g.pass_inputs++; }
  void gene_text_dropped() { g.gtext++; }
  void read_text_dropped() { g.ttext++; }
  void list_changes() { g.list++, list.origin = LIST_NONE; }
  void list_forgotten() { list.origin = LIST_NONE; }  // (a gene text that could not be put in place: as before this header)
  // ---- what was made
  void list_made(Origin o) { list.reads = g.reads, list.db = g.db, list.origin = o; }
  void order_begins() { g.order++, ordered = Ordered(); }
  void order_made() { ordered = Ordered{g.reads, g.db, g.gtext, g.ttext, g.list, g.order}; }
  void tokens_made() { tokens = g.ttext; }
  void side_begins() { side = 0; }
  void side_made() { side = g.order; }
  void sam_begins() { sam = 0; }
  void sam_made() { sam = g.order; }
  void cov_begins() { cov = 0; }
  void cov_made() { cov = g.order; }

  // ---- the questions
  bool may_order_resident() const { return list.origin != LIST_NONE && list.reads == g.reads && list.db == g.db; }
  bool may_replay() const { return may_order_resident() && list.origin == LIST_PASS; }  // musc_maxmatches_apply
  bool ordered_current() const {  // musc_results_text / musc_results_hits
    return ordered.reads == g.reads && ordered.db == g.db && ordered.gtext == g.gtext && ordered.ttext == g.ttext;
  }
  bool list_changed_since_order() const { return ordered.list != g.list; }
  bool tokens_current() const { return tokens == g.ttext; }
  SideRefusal side_prepare_refusal(bool have_read_text, bool form_ok, uint64_t nreads) const {
    return !ordered_current() ? SIDE_NO_ORDER : list_changed_since_order() ? SIDE_PASS_AFTER : !have_read_text ? SIDE_NO_READ_TEXT
           : !form_ok ? SIDE_FORM : nreads >= 0xFFFFFFF0ull ? SIDE_TOO_MANY_READS : SIDE_OK;
  }
  bool may_side_text() const { return side == g.order && ordered_current() && !list_changed_since_order(); }
  bool may_sam_text() const { return sam == g.order && ordered_current(); }  // (as results.txt: a later pass does not outdate the ordered list)
  bool may_cov_text() const { return cov == g.order && ordered_current(); }  // (likewise)
};

// What a cache of the pass driver was made for: compared field by field (musc_params may carry padding, and a caller
// need not zero the window starts it does not use)
struct PassKey {
  uint64_t pass_inputs = 0;  // 0: made for nothing
  musc_params P{};
  int block_mode = -1;
  bool operator==(const PassKey& o) const {
    const musc_params &a = P, &b = o.P;
    if (pass_inputs != o.pass_inputs || block_mode != o.block_mode || a.n_windows != b.n_windows) return false;
    for (int k = 0; k < a.n_windows && k < MUSC_MAX_WINDOWS; k++)
      if (a.windows[k] != b.windows[k]) return false;
    return a.window_width == b.window_width && a.pmatch == b.pmatch && a.min_dinuc == b.min_dinuc &&
           a.max_read_length == b.max_read_length && a.max_matches == b.max_matches && a.match_mode == b.match_mode &&
           a.mmtol == b.mmtol && a.apply_mmtol == b.apply_mmtol && a.max_mismatch_p1 == b.max_mismatch_p1 &&
           a.skip_block_check == b.skip_block_check && a.n_shards == b.n_shards;
  }
};

}  // namespace musc_state
