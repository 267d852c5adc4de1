// ctx_state_check.cpp -- the stamps of csrc/ctx_state.hpp against the six booleans they replaced (hits_current, mm_list,
// res_valid, side_after_match, side_tok_valid, side_valid), as a program of its own so that it runs under the sanitizers.
// Old is the library before the header, transcribed event by event: each method sets and clears what the entry point of
// that name set and cleared, in its order.  New makes the calls the library makes now.  Both are driven with the event
// sequence of tests/test_gpu_side.py::test_refusals and with random sequences, and after every event every question of
// ctx_state.hpp has the same answer in both -- with one exception, which is the point of the change: a
// musc_maxmatches_apply that fails after its first write into the list.  Old went on calling the half-written list
// that of a pass; New must say LIST_NONE, and from there on Old is told so.
// The stamp of the coverage tables (cov_begins, cov_made, may_cov_text) came after the booleans; it is held
// to one kept here the old way -- set by a prepare that succeeds over a current order, cleared by every order and by
// whatever replaces the reads, the database or either text -- and by hand to be independent of the SAM stamp.
// It needs no GPU and is not part of the library; muscato_amd/build.py (CHECKS) builds it, plain and sanitized.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../ctx_state.hpp"
#include "check.hpp"

namespace {

using namespace musc_state;

// how a call ends, as the driver decides it
enum How {
  OK, FAIL,
  BAD_NSEQ,                            // set gene text: refused before anything changes
  RESIDENT_OK, RESIDENT_FAIL,          // order with the resident list (OK / FAIL: with supplied tuples)
  FAIL_AFTER_TOKENS,                   // side prepare: fails once the tokens are made (FAIL: before)
  REFUSED, FAIL_AFTER, OK_UNCHANGED,   // maxmatches apply: refused by the pass's parameters; fails after the first write;
                                       // nothing to truncate (FAIL: before the list changes)
};

// what both versions keep as data, not as validity: which texts exist and what form the gene text has
struct Facts {
  bool db = false, gtext = false, ttext = false, form_ok = false;
  uint64_t nreads = 0;
};

struct Old {
  bool hits_current = false, mm_list = false, res_valid = false, side_after_match = false, side_tok_valid = false, side_valid = false;
  void drop_gene_text() { side_valid = false, res_valid = false, hits_current = false; }
  void drop_read_text() { res_valid = false, side_tok_valid = false, side_valid = false; }
  void forget_read_text() { drop_read_text(), hits_current = false; }
  void free_index() {}
  void free_db() { free_index(), drop_gene_text(); }
  void drop_reads() { forget_read_text(); }

  void load_reads(How) { drop_reads(); }
  void load_db(How) { free_db(); }
  void set_gene_text(How how) {
    if (how == BAD_NSEQ) return;
    const bool list_ok = hits_current;
    drop_gene_text();
    hits_current = list_ok;
    if (how == FAIL) drop_gene_text();
  }
  void set_read_text(How how) {
    drop_read_text();
    if (how == FAIL) drop_read_text();
  }
  void pass(How how) {
    hits_current = false;
    side_after_match = true;
    hits_current = how == OK;
    mm_list = how == OK;
  }
  bool order(How how, const Facts& f) {
    res_valid = false;
    side_valid = false;
    if (!f.db || !f.gtext) return false;
    if ((how == RESIDENT_OK || how == RESIDENT_FAIL) && !hits_current) return false;
    if (how == FAIL || how == RESIDENT_FAIL) return false;
    res_valid = true;
    side_after_match = false;
    return true;
  }
  SideRefusal side_refusal(const Facts& f) const {
    if (!res_valid) return SIDE_NO_ORDER;
    if (side_after_match) return SIDE_PASS_AFTER;
    if (!f.ttext) return SIDE_NO_READ_TEXT;
    if (!f.form_ok) return SIDE_FORM;
    if (f.nreads >= 0xFFFFFFF0ull) return SIDE_TOO_MANY_READS;
    return SIDE_OK;
  }
  bool side_prepare(How how, const Facts& f) {
    side_valid = false;
    if (side_refusal(f) != SIDE_OK || how == FAIL) return false;
    side_tok_valid = true;
    if (how == FAIL_AFTER_TOKENS) return false;
    side_valid = true;
    return true;
  }
  bool may_order_resident() const { return hits_current; }
  bool may_results() const { return res_valid; }
  bool may_side_text() const { return !(!side_valid || !res_valid || side_after_match); }
  bool may_apply() const { return !(!hits_current || !mm_list); }
  bool apply(How how) {
    if (!may_apply() || how == REFUSED) return false;
    if (how == FAIL || how == FAIL_AFTER) return false;  // (FAIL_AFTER: c->hits is half written and nothing here says so)
    if (how == OK_UNCHANGED) return true;
    mm_list = false;
    side_after_match = true;
    return true;
  }
};

struct New {
  State st;
  void drop_gene_text() { st.gene_text_dropped(); }
  void drop_read_text() { st.read_text_dropped(); }
  void free_index() { st.index_freed(); }
  void free_db() { free_index(), drop_gene_text(), st.db_freed(); }
  void drop_reads() { drop_read_text(), st.reads_dropped(); }

  void load_reads(How how) {
    drop_reads();
    if (how == FAIL) drop_reads();  // reads_load_done
  }
  void load_db(How) { free_db(); }
  void set_gene_text(How how) {
    if (how == BAD_NSEQ) return;
    drop_gene_text();
    if (how == FAIL) drop_gene_text(), st.list_forgotten();
  }
  void set_read_text(How how) {
    drop_read_text();
    if (how == FAIL) drop_read_text();
  }
  void pass(How how) {
    st.list_changes();
    if (how == OK) st.list_made(LIST_PASS);
  }
  bool order(How how, const Facts& f) {
    st.order_begins();
    if (!f.db || !f.gtext) return false;
    if ((how == RESIDENT_OK || how == RESIDENT_FAIL) && !st.may_order_resident()) return false;
    if (how == FAIL || how == RESIDENT_FAIL) return false;
    st.order_made();
    return true;
  }
  SideRefusal side_refusal(const Facts& f) const { return st.side_prepare_refusal(f.ttext, f.form_ok, f.nreads); }
  bool side_prepare(How how, const Facts& f) {
    st.side_begins();
    if (side_refusal(f) != SIDE_OK || how == FAIL) return false;
    st.tokens_made();
    if (how == FAIL_AFTER_TOKENS) return false;
    st.side_made();
    return true;
  }
  bool apply(How how) {
    if (!st.may_replay() || how == REFUSED) return false;
    if (how == FAIL) return false;
    if (how == OK_UNCHANGED) return true;
    st.list_changes();
    if (how == FAIL_AFTER) return false;
    st.list_made(LIST_REPLAYED);
    return true;
  }
};

enum Event { LOAD_READS, LOAD_DB, FREE_INDEX, SET_GENE_TEXT, SET_READ_TEXT, PASS, ORDER, SIDE_PREPARE, SIDE_TEXT, APPLY, RELOAD_ENV, COV_PREPARE, N_EVENTS };

struct World {
  Old o;
  New n;
  Facts f;
  uint64_t pass_inputs_seen = 1;
  bool cov_valid = false;  // the coverage tables, kept as a boolean

  void agree() {
    EXPECT(cov_valid == n.st.may_cov_text());
    EXPECT(o.may_order_resident() == n.st.may_order_resident());
    EXPECT(o.may_results() == n.st.ordered_current());
    EXPECT(o.side_refusal(f) == n.side_refusal(f));
    EXPECT(o.may_side_text() == n.st.may_side_text());
    EXPECT(o.may_apply() == n.st.may_replay());
    EXPECT(o.side_tok_valid == n.st.tokens_current());  // (asked inside musc_side_prepare only)
    EXPECT(n.st.g.pass_inputs >= pass_inputs_seen);
    pass_inputs_seen = n.st.g.pass_inputs;
  }

  // one call on both versions; the same answer from both, which is returned
  bool step(Event e, How how, bool form_ok = true) {
    bool ro = true, rn = true;
    const uint64_t inputs = n.st.g.pass_inputs;
    if (e == LOAD_READS || e == LOAD_DB || e == SET_READ_TEXT || e == ORDER || (e == SET_GENE_TEXT && f.db && how != BAD_NSEQ)) cov_valid = false;
    switch (e) {
      case LOAD_READS:
        o.load_reads(how), n.load_reads(how);
        f.ttext = false;
        f.nreads = how == OK ? 60 : 0;
        EXPECT(n.st.g.pass_inputs > inputs);
        break;
      case LOAD_DB:
        o.load_db(how), n.load_db(how);
        f.db = how == OK;
        f.gtext = f.form_ok = false;
        EXPECT(n.st.g.pass_inputs > inputs);
        break;
      case FREE_INDEX:
        o.free_index(), n.free_index();
        EXPECT(n.st.g.pass_inputs > inputs);
        break;
      case SET_GENE_TEXT:
        if (!f.db) how = BAD_NSEQ;
        o.set_gene_text(how), n.set_gene_text(how);
        if (how != BAD_NSEQ) f.gtext = how == OK, f.form_ok = how == OK && form_ok;
        ro = rn = how == OK;
        break;
      case SET_READ_TEXT:
        o.set_read_text(how), n.set_read_text(how);
        f.ttext = how == OK;
        ro = rn = how == OK;
        break;
      case PASS:
        if (!f.db) how = FAIL;  // "no database loaded"
        o.pass(how), n.pass(how);
        ro = rn = how == OK;
        break;
      case ORDER: ro = o.order(how, f), rn = n.order(how, f); break;
      case SIDE_PREPARE: ro = o.side_prepare(how, f), rn = n.side_prepare(how, f); break;
      case SIDE_TEXT: ro = o.may_side_text(), rn = n.st.may_side_text(); break;
      case APPLY: {
        const bool may = o.may_apply();
        ro = o.apply(how), rn = n.apply(how);
        if (may && how == FAIL_AFTER) {  // the exception: exactly this, then Old follows
          EXPECT(n.st.list.origin == LIST_NONE);
          EXPECT(!n.st.may_order_resident() && !n.st.may_replay() && n.st.list_changed_since_order());
          EXPECT(o.hits_current && o.mm_list);
          o.hits_current = o.mm_list = false;
          o.side_after_match = true;
        }
        break;
      }
      case RELOAD_ENV: break;  // (the sized key and graph.failed: no standing of any list)
      case COV_PREPARE:  // musc_cov_prepare: needs a current order; a refusal or a failure leaves nothing prepared
        n.st.cov_begins();
        ro = rn = cov_valid = n.st.ordered_current() && how == OK;
        if (rn) n.st.cov_made();
        break;
      default: break;
    }
    EXPECT(ro == rn);
    agree();
    return rn;
  }

  void refused(SideRefusal why) {  // test_refusals: musc_side_prepare says so, and no side text is to be had
    EXPECT(n.side_refusal(f) == why);
    EXPECT(!step(SIDE_PREPARE, OK));
    EXPECT(!step(SIDE_TEXT, OK));
  }
  void good() {
    EXPECT(step(ORDER, OK));
    EXPECT(step(SIDE_PREPARE, OK));
    EXPECT(step(SIDE_TEXT, OK));
  }
};

void test_refusals_sequence() {
  {
    World fresh;
    fresh.agree();
    fresh.refused(SIDE_NO_ORDER);
  }
  World w;
  w.step(LOAD_DB, OK), w.step(LOAD_READS, OK), w.step(SET_GENE_TEXT, OK);  // load(): no read text
  w.refused(SIDE_NO_ORDER);
  EXPECT(w.step(ORDER, OK));
  w.refused(SIDE_NO_READ_TEXT);
  w.step(SET_READ_TEXT, OK);
  w.refused(SIDE_NO_ORDER);  // a new text invalidates the order
  w.good();
  w.step(LOAD_READS, OK);
  w.refused(SIDE_NO_ORDER);
  w.step(LOAD_READS, OK), w.step(SET_READ_TEXT, OK);
  w.good();
  w.step(LOAD_DB, OK);
  w.refused(SIDE_NO_ORDER);
  w.step(SET_GENE_TEXT, OK);
  w.refused(SIDE_NO_ORDER);
  w.good();
  w.step(SET_GENE_TEXT, OK);
  w.refused(SIDE_NO_ORDER);
  w.good();
  EXPECT(w.step(PASS, OK));
  w.refused(SIDE_PASS_AFTER);
  w.good();
  for (int bad = 0; bad < 6; bad++) {  // a gene text outside the simple form
    w.step(SET_GENE_TEXT, OK, false);
    EXPECT(w.step(ORDER, OK));
    EXPECT(w.n.st.ordered_current());
    w.refused(SIDE_FORM);
    EXPECT(w.n.st.ordered_current());  // results.txt does not need the form
  }
  w.step(SET_GENE_TEXT, OK);  // (the gene in the bad form is absent)
  EXPECT(w.step(ORDER, OK));
  EXPECT(w.step(SIDE_PREPARE, OK));
  w.step(SET_GENE_TEXT, OK);
  w.good();
  EXPECT(w.step(SIDE_TEXT, OK));
}

void by_hand() {
  World w;
  w.step(LOAD_DB, OK), w.step(LOAD_READS, OK), w.step(SET_GENE_TEXT, OK), w.step(SET_READ_TEXT, OK);
  EXPECT(!w.step(ORDER, RESIDENT_OK));  // nothing matched yet
  EXPECT(w.step(PASS, OK));
  w.step(SET_GENE_TEXT, OK);  // a new text leaves the list as good as it was
  EXPECT(w.step(ORDER, RESIDENT_OK));
  EXPECT(w.step(APPLY, OK_UNCHANGED) && w.step(APPLY, OK));
  EXPECT(!w.step(APPLY, OK));  // the list is the replay's now
  EXPECT(w.n.side_refusal(w.f) == SIDE_PASS_AFTER);
  EXPECT(w.step(ORDER, RESIDENT_OK));  // ... and may be ordered
  EXPECT(w.step(SIDE_PREPARE, OK));
  EXPECT(w.step(PASS, OK));
  EXPECT(!w.step(APPLY, FAIL_AFTER));  // the exception
  EXPECT(!w.step(ORDER, RESIDENT_OK) && !w.step(APPLY, OK));
  EXPECT(w.step(PASS, OK) && w.step(APPLY, OK));
  w.step(FREE_INDEX, OK);  // an index build outdates the pass caches, not the list
  EXPECT(w.step(ORDER, RESIDENT_OK));
  EXPECT(!w.step(PASS, FAIL));  // a failed pass leaves no list
  EXPECT(!w.step(ORDER, RESIDENT_OK));
}

// the coverage stamp beside SAM's: each is made and lost on its own, both go with the order
void cov_stamp() {
  World w;
  w.step(LOAD_DB, OK), w.step(LOAD_READS, OK), w.step(SET_GENE_TEXT, OK), w.step(SET_READ_TEXT, OK);
  EXPECT(!w.step(COV_PREPARE, OK));  // no ordered list
  EXPECT(w.step(ORDER, OK) && !w.n.st.may_cov_text());
  EXPECT(w.step(COV_PREPARE, OK) && w.n.st.may_cov_text() && !w.n.st.may_sam_text());
  w.n.st.sam_begins(), w.n.st.sam_made();
  EXPECT(w.n.st.may_cov_text() && w.n.st.may_sam_text());
  w.n.st.sam_begins();
  EXPECT(w.n.st.may_cov_text() && !w.n.st.may_sam_text());
  w.n.st.sam_made();
  EXPECT(!w.step(COV_PREPARE, FAIL) && !w.n.st.may_cov_text() && w.n.st.may_sam_text());  // a refusal: SAM's tables stay
  EXPECT(w.step(COV_PREPARE, OK));
  EXPECT(w.step(PASS, OK) && w.n.st.may_cov_text());  // as results.txt: a later pass does not outdate the ordered list
  EXPECT(w.step(SIDE_PREPARE, OK) == false && w.n.st.may_cov_text());
  for (Event e : {ORDER, LOAD_READS, LOAD_DB, SET_GENE_TEXT, SET_READ_TEXT}) {
    w.step(LOAD_DB, OK), w.step(LOAD_READS, OK), w.step(SET_GENE_TEXT, OK), w.step(SET_READ_TEXT, OK);
    EXPECT(w.step(ORDER, OK) && w.step(COV_PREPARE, OK) && w.n.st.may_cov_text());
    w.step(e, OK);
    EXPECT(!w.n.st.may_cov_text());
  }
}

}  // namespace

int main() {
  test_refusals_sequence();
  by_hand();
  cov_stamp();
  std::mt19937_64 rng(19);
  const int rounds = 120000;
  for (int round = 0; round < rounds && !failures; round++) {
    World w;
    const int len = 40 + (int)(rng() % 40);
    // (some rounds keep the loads rare, so that long chains of pass / order / prepare / apply build up)
    const unsigned calm = round % 3;
    for (int i = 0; i < len; i++) {
      Event e = (Event)(rng() % N_EVENTS);
      if (calm && (e == LOAD_READS || e == LOAD_DB) && rng() % (calm == 1 ? 4 : 16)) e = (Event)(PASS + rng() % (N_EVENTS - PASS));
      const unsigned r = (unsigned)(rng() % 16);
      How how = OK;
      switch (e) {
        case LOAD_READS: case LOAD_DB: case SET_READ_TEXT: case PASS: case COV_PREPARE: how = r < 3 ? FAIL : OK; break;
        case SET_GENE_TEXT: how = r < 2 ? FAIL : r < 4 ? BAD_NSEQ : OK; break;
        case ORDER: how = r < 2 ? FAIL : r < 4 ? RESIDENT_FAIL : r < 10 ? RESIDENT_OK : OK; break;
        case SIDE_PREPARE: how = r < 2 ? FAIL : r < 4 ? FAIL_AFTER_TOKENS : OK; break;
        case APPLY: how = r < 2 ? REFUSED : r < 4 ? FAIL : r < 7 ? FAIL_AFTER : r < 10 ? OK_UNCHANGED : OK; break;
        default: break;
      }
      w.step(e, how, rng() % 4 != 0);
    }
  }
  // PassKey: field by field; the window starts a run does not use and the reserved words do not count
  musc_params P{};
  P.n_windows = 2, P.windows[0] = 0, P.windows[1] = 10, P.window_width = 12, P.pmatch = 0.95;
  const PassKey k{7, P, 1};
  musc_params Q = P;
  Q.windows[5] = 99, Q.reserved[1] = -1;
  EXPECT((k == PassKey{7, Q, 1}));
  EXPECT(!(k == PassKey{8, P, 1}) && !(k == PassKey{7, P, 2}) && !(k == PassKey()));
  Q = P, Q.windows[1] = 11;
  EXPECT(!(k == PassKey{7, Q, 1}));
  Q = P, Q.max_matches = 5;
  EXPECT(!(k == PassKey{7, Q, 1}));
  Q = P, Q.pmatch = 0.9;
  EXPECT(!(k == PassKey{7, Q, 1}));
  return check_done("ctx_state_check");
}
