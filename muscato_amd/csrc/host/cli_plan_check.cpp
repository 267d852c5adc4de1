// cli_plan_check.cpp -- the placement plan of the `muscato` driver (cli_plan.hpp) against the boolean expressions it
// replaced, and the one name path of read preparation (cli_names.hpp) against the two loops it replaced, as a program of
// its own so that it runs under the sanitizers: muscato_amd/build.py (CHECKS) builds it, plain and sanitized.
// Old is the driver before the plan, transcribed expression by expression from run_muscato and run_hot_path as they
// were (prep_device, res_device, side_device, mm_device, want_rccl, list_on_device, and the conditions of the log
// lines); New makes the calls the driver makes now, in its order.  Both see the whole product of: each of the five
// variables over {unset, "", host, device, rccl, junk}, GPUs over {1, 2, 3}, odd target bytes or none, an overflow or
// none, each run-time demotion fired or not, and both values of each *_DEFAULT_DEVICE macro.  MUSC_PREP_NAMES, which came
// after the plan, is held to its boolean expression in that product too -- its value, its default and its demotion
// change with the combination, so that every pair of it with another input occurs -- and over the whole product of
// what the expression reads (check_names_plan).
// MUSC_COVERAGE (the coverage files) likewise (check_cov_plan).
// MUSC_SAM (the SAM file) is held to its boolean expression in the same way (check_sam_plan), and the size
// rules of a SAM record (sam_plan.hpp) to text that is built byte by byte (check_sam_sizes).
// The size rules of the coverage stage (cov_plan.hpp) are held to text built byte by byte, to a brute-force
// per-base count on small inputs, and their key arithmetic up to 2^36 bases and 2^24 targets (check_cov_sizes).
// The name rules run on fixed cases and on seeded random groups whose names sit in heap blocks of their exact size.
// It needs no GPU and is not part of the library.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "check.hpp"
#include "cli_names.hpp"
#include "cli_plan.hpp"
#include "../cov_plan.hpp"
#include "../sam_plan.hpp"

namespace {

using namespace musc;

// ---- the plan -------------------------------------------------------------------------------------------------

// what a stage finds when it runs
struct Events {
  bool overflow, prep_no_memory, rccl_failed, replay_pass_failed, replay_refused, side_refused;
  bool names_no_memory = false;
};

// everything of a run that depends on the placement
struct Outcome {
  bool prep_on_device = false;     // the read file was parsed on the device
  bool rccl = false;               // the tuples were gathered over RCCL
  bool note_odd = false;           // "results on the host: the targets hold bytes ..." was logged
  bool note_gpus = false;          // "MaxMatches replay on the host: the post-chain of %d GPUs ..." was logged
  bool died = false;               // the hot path threw
  bool replayed_on_device = false, replayed_on_host = false;
  bool results_on_device = false;  // context 0 outlives the hot path and orders results.txt
  bool list_on_device = false;     // ... from the resident list
  bool ctx_to_side = false;        // context 0 outlives results.txt
  bool side_from_device = false;   // the three side outputs are the device's
  bool names_on_device = false;    // the names of the reads were ordered, cut and joined on the device
  bool prep_ran_twice = false;     // ... or the device parse ran again without them
  bool operator==(const Outcome& o) const {
    return prep_on_device == o.prep_on_device && rccl == o.rccl && note_odd == o.note_odd && note_gpus == o.note_gpus &&
           died == o.died && replayed_on_device == o.replayed_on_device && replayed_on_host == o.replayed_on_host &&
           results_on_device == o.results_on_device && list_on_device == o.list_on_device && ctx_to_side == o.ctx_to_side &&
           side_from_device == o.side_from_device && names_on_device == o.names_on_device && prep_ran_twice == o.prep_ran_twice;
  }
};

Outcome old_run(const PlanEnv& env, int GPUs, size_t nodd, const Events& ev, const PlanDefaults& D) {
  const int MUSC_PREP_DEFAULT = D.prep, MUSC_RESULTS_DEFAULT = D.results, MUSC_SIDE_DEFAULT = D.side, MUSC_MAXMATCHES_DEFAULT = D.maxmatches;
  Outcome o;
  // run_muscato, read prep
  const char* prep_env = env.prep;
  const bool prep_device = prep_env ? !strcmp(prep_env, "device") : MUSC_PREP_DEFAULT != 0;
  o.prep_on_device = prep_device && !ev.prep_no_memory;  // (prep_reads_device ran prep_reads in its place)
  // (the names: the expression the plan's field stands for)
  const char* names_env = env.prep_names;
  const bool names_env_device = names_env && !strcmp(names_env, "device"), names_env_host = names_env && !strcmp(names_env, "host");
  const bool names_device = prep_device && (names_env_device || (!names_env_host && D.prep_names));
  o.prep_ran_twice = names_device && ev.names_no_memory && !ev.prep_no_memory;
  o.names_on_device = names_device && !ev.names_no_memory && !ev.prep_no_memory;
  // run_muscato, in front of the hot path
  const char* res_env = env.results;
  const bool env_device = res_env && !strcmp(res_env, "device"), env_host = res_env && !strcmp(res_env, "host");
  const bool res_device = GPUs == 1 && nodd == 0 && (env_device || (!env_host && MUSC_RESULTS_DEFAULT));
  if (nodd && GPUs == 1 && !env_host) o.note_odd = true;
  // run_hot_path(keep0 = res_device ? &ctx0 : nullptr)
  const int G = GPUs;
  bool err = false;
  const char* genv = env.gather;
  const bool want_rccl = G > 1 && genv && !strcmp(genv, "rccl");
  o.rccl = want_rccl && !ev.rccl_failed;
  const bool overflow = ev.overflow;
  bool replayed_on_device = false;
  if (overflow) {
    const char* mm_env = env.maxmatches;
    const bool mm_env_device = mm_env && !strcmp(mm_env, "device"), mm_env_host = mm_env && !strcmp(mm_env, "host");
    bool mm_device = mm_env_device || (!mm_env_host && MUSC_MAXMATCHES_DEFAULT);
    if (mm_device && G > 1) {
      o.note_gpus = true;
      mm_device = false;
    }
    if (ev.replay_pass_failed) {
      err = true;
      mm_device = false;
    }
    if (!err && mm_device) {
      if (!ev.replay_refused) replayed_on_device = true;
      else mm_device = false;
    }
    if (!err && !mm_device) o.replayed_on_host = true;
  }
  o.replayed_on_device = replayed_on_device;
  bool ctx0 = false, list_on_device = false;
  if (res_device && G == 1 && !err) {
    ctx0 = true;
    list_on_device = !overflow || replayed_on_device;
  }
  if (err) {
    o.died = true;
    return o;
  }
  // run_muscato, results.txt and the side outputs
  const char* side_env = env.side;
  const bool side_env_device = side_env && !strcmp(side_env, "device"), side_env_host = side_env && !strcmp(side_env, "host");
  const bool side_device = ctx0 && (side_env_device || (!side_env_host && MUSC_SIDE_DEFAULT));
  o.results_on_device = ctx0;
  o.list_on_device = list_on_device;
  if (ctx0 && !side_device) ctx0 = false;
  o.ctx_to_side = ctx0;
  bool from_device = false;
  if (ctx0) from_device = !ev.side_refused;
  o.side_from_device = from_device;
  return o;
}

Outcome new_run(const PlanEnv& env, int GPUs, size_t nodd, const Events& ev, const PlanDefaults& D) {
  Outcome o;
  Placement plan = make_placement(env, GPUs, D);
  // stage_read_prep: prep_reads_device with the names, without them when they found no memory, prep_reads when the
  // parse found none (a device without memory for the parse has none for the parse and the names)
  EXPECT(plan.prep_names == Where::Host || plan.prep == Where::Device);
  if (plan.prep == Where::Device && ev.prep_no_memory) plan.demote(Demotion::PrepNoMemory);
  if (plan.prep_names == Where::Device && ev.names_no_memory) {
    plan.demote(Demotion::PrepNamesNoMemory);
    o.prep_ran_twice = true;
  }
  o.prep_on_device = plan.prep == Where::Device;
  o.names_on_device = plan.prep_names == Where::Device;
  EXPECT(!o.names_on_device || o.prep_on_device);
  // stage_target_files, stage_hot_path
  if (nodd) plan.demote(Demotion::OddTargetBytes);
  o.note_odd = plan.note_odd_targets;
  // run_hot_path
  if (plan.gather_rccl && ev.rccl_failed) plan.demote(Demotion::GatherFailed);
  o.rccl = plan.gather_rccl;
  if (ev.overflow) {
    o.note_gpus = plan.note_replay_gpus;
    if (ev.replay_pass_failed) {
      plan.demote(Demotion::ReplayPassFailed);
      o.died = true;
      return o;
    }
    if (plan.maxmatches == Where::Device && ev.replay_refused) plan.demote(Demotion::ReplayRefused);
    o.replayed_on_device = plan.maxmatches == Where::Device;
    o.replayed_on_host = plan.maxmatches == Where::Host;
  }
  o.list_on_device = plan.list_on_device(ev.overflow);
  // stage_results
  o.results_on_device = plan.results == Where::Device;
  o.ctx_to_side = plan.side == Where::Device;
  EXPECT(!o.ctx_to_side || o.results_on_device);  // the side outputs need the list results.txt was ordered from
  // stage_side_outputs
  if (plan.side == Where::Device && ev.side_refused) plan.demote(Demotion::SideRefused);
  o.side_from_device = plan.side == Where::Device;
  return o;
}

unsigned long long check_plan() {  // -> the combinations seen
  static const char* const V[6] = {nullptr, "", "host", "device", "rccl", "junk"};
  unsigned long long n = 0;
  for (int d = 0; d < 16; d++) {
    PlanDefaults D;
    D.prep = d & 1, D.maxmatches = d & 2, D.results = d & 4, D.side = d & 8;
    for (int e = 0; e < 6 * 6 * 6 * 6 * 6; e++) {
      PlanEnv env;
      env.prep = V[e % 6], env.maxmatches = V[e / 6 % 6], env.results = V[e / 36 % 6], env.side = V[e / 216 % 6], env.gather = V[e / 1296];
      env.prep_names = V[(e / 6 + e / 7776 + d) % 6];  // (every value beside every value of each other variable)
      D.prep_names = ((e / 36) + d) & 1;
      for (int gpus = 1; gpus <= 3; gpus++)
        for (size_t nodd = 0; nodd <= 1; nodd++)
          for (int x = 0; x < 64; x++) {
            const Events ev = {(x & 1) != 0, (x & 2) != 0, (x & 4) != 0, (x & 8) != 0, (x & 16) != 0, (x & 32) != 0, ((x >> 1) + gpus + e) % 2 != 0};
            const Outcome a = old_run(env, gpus, nodd, ev, D), b = new_run(env, gpus, nodd, ev, D);
            n++;
            EXPECT_MSG(a == b, "plan differs: defaults %d env %s|%s|%s|%s|%s|%s GPUs %d nodd %zu events %d", d, env.prep ? env.prep : "(unset)",
                       env.maxmatches ? env.maxmatches : "(unset)", env.results ? env.results : "(unset)", env.side ? env.side : "(unset)",
                       env.gather ? env.gather : "(unset)", env.prep_names ? env.prep_names : "(unset)", gpus, nodd, x);
          }
    }
  }
  // the compiled defaults are what the measurements behind them decided
  const PlanDefaults compiled;
  EXPECT(!compiled.prep && compiled.maxmatches && compiled.results && compiled.side && !compiled.prep_names);
  // and the two parse rules differ where the comment of cli_plan.hpp says they do
  EXPECT(place_prep_by_env("junk", true) == Where::Host && place_by_env("junk", true) == Where::Device);
  EXPECT(place_prep_by_env("", true) == Where::Host && place_by_env("", true) == Where::Device);
  EXPECT(place_prep_by_env(nullptr, true) == Where::Device && place_by_env(nullptr, true) == Where::Device);
  return n;
}

// MUSC_PREP_NAMES over the whole product of what its expression reads -- itself and MUSC_PREP over the six values, both
// defaults, both no-memory events -- with every other variable over {unset, host, device}, GPUs over {1, 2, 3}, odd
// target bytes or none and an overflow or none: the rest of the outcome is what it is for MUSC_PREP_NAMES unset.
unsigned long long check_names_plan() {
  static const char* const V[6] = {nullptr, "", "host", "device", "rccl", "junk"};
  static const char* const O[3] = {nullptr, "host", "device"};
  unsigned long long n = 0;
  for (int d = 0; d < 4; d++)
    for (int e = 0; e < 36; e++)
      for (int o = 0; o < 81; o++)
        for (int gpus = 1; gpus <= 3; gpus++)
          for (int x = 0; x < 16; x++) {
            PlanDefaults D;
            D.prep = d & 1, D.prep_names = d & 2;
            PlanEnv env;
            env.prep = V[e % 6], env.prep_names = V[e / 6];
            env.maxmatches = O[o % 3], env.results = O[o / 3 % 3], env.side = O[o / 9 % 3], env.targets = O[o / 27];
            Events ev = {(x & 1) != 0, (x & 2) != 0, false, false, false, false, (x & 4) != 0};
            const size_t nodd = (x & 8) != 0;
            const Outcome a = old_run(env, gpus, nodd, ev, D), b = new_run(env, gpus, nodd, ev, D);
            EXPECT_MSG(a == b, "names plan differs: defaults %d env %d others %d GPUs %d events %d", d, e, o, gpus, x);
            PlanEnv unset = env;
            unset.prep_names = nullptr;
            D.prep_names = false;
            ev.names_no_memory = false;
            Outcome c = new_run(unset, gpus, nodd, ev, D);
            EXPECT(!c.names_on_device && !c.prep_ran_twice);
            c.names_on_device = b.names_on_device, c.prep_ran_twice = b.prep_ran_twice;
            EXPECT_MSG(b == c, "MUSC_PREP_NAMES moved another stage: defaults %d env %d others %d GPUs %d events %d", d, e, o, gpus, x);
            n++;
          }
  return n;
}

// MUSC_SAM over its six values, both defaults and the refusal of the device stage, with every other variable over
// {unset, host, device}, GPUs over {1, 2, 3}, odd target bytes or none, an overflow or none and a refused replay or none:
// the SAM file is the device's exactly when results.txt was ordered there from the resident list, the variable or the
// default says device, and musc_sam_prepare did not refuse; and no other stage moves with it.
unsigned long long check_sam_plan() {
  static const char* const V[6] = {nullptr, "", "host", "device", "rccl", "junk"};
  static const char* const O[3] = {nullptr, "host", "device"};
  unsigned long long n = 0;
  for (int d = 0; d < 2; d++)
    for (int e = 0; e < 6; e++)
      for (int o = 0; o < 81; o++)
        for (int gpus = 1; gpus <= 3; gpus++)
          for (int x = 0; x < 16; x++) {
            PlanDefaults D;
            D.sam = d != 0;
            PlanEnv env;
            env.sam = V[e];
            env.maxmatches = O[o % 3], env.results = O[o / 3 % 3], env.side = O[o / 9 % 3], env.targets = O[o / 27];
            const bool overflow = (x & 1) != 0, replay_refused = (x & 2) != 0, sam_refused = (x & 4) != 0;
            const size_t nodd = (x & 8) != 0;
            const Events ev = {overflow, false, false, false, replay_refused, false, false};
            // the expression
            const Outcome old = old_run(env, gpus, nodd, ev, D);
            const bool env_device = env.sam && !strcmp(env.sam, "device"), env_host = env.sam && !strcmp(env.sam, "host");
            const bool want = env_device || (!env_host && D.sam);
            const bool tried = old.results_on_device && old.list_on_device && want;
            // the plan, as stage_results and stage_sam use it
            Placement plan = make_placement(env, gpus, D);
            if (nodd) plan.demote(Demotion::OddTargetBytes);
            if (overflow && plan.maxmatches == Where::Device && replay_refused) plan.demote(Demotion::ReplayRefused);
            const bool resident = plan.list_on_device(overflow);
            EXPECT(resident == old.list_on_device);
            EXPECT_MSG(plan.sam_on_device(resident) == tried, "sam plan differs: default %d env %d others %d GPUs %d events %d", d, e, o, gpus, x);
            if (plan.sam_on_device(resident) && sam_refused) plan.demote(Demotion::SamRefused);
            EXPECT(plan.sam_on_device(resident) == (tried && !sam_refused));
            EXPECT(plan.sam == Where::Host || plan.results == Where::Device);
            // nothing else moves
            PlanEnv unset = env;
            unset.sam = nullptr;
            EXPECT(new_run(env, gpus, nodd, ev, D) == new_run(unset, gpus, nodd, ev, PlanDefaults()));
            n++;
          }
  EXPECT(!PlanDefaults().sam);  // unmeasured: the host writes the SAM file unless MUSC_SAM=device
  return n;
}

// MUSC_COVERAGE over its six values, both defaults and the refusal of the device stage, with every other variable over
// {unset, host, device}, GPUs over {1, 2, 3}, odd target bytes or none, an overflow or none and a refused replay or none:
// the coverage files are the device's exactly when results.txt was ordered there from the resident list, the variable or the
// default says device, and musc_cov_prepare did not refuse; and no other stage moves with it.
unsigned long long check_cov_plan() {
  static const char* const V[6] = {nullptr, "", "host", "device", "rccl", "junk"};
  static const char* const O[3] = {nullptr, "host", "device"};
  unsigned long long n = 0;
  for (int d = 0; d < 2; d++)
    for (int e = 0; e < 6; e++)
      for (int o = 0; o < 81; o++)
        for (int gpus = 1; gpus <= 3; gpus++)
          for (int x = 0; x < 16; x++) {
            PlanDefaults D;
            D.coverage = d != 0;
            PlanEnv env;
            env.coverage = V[e];
            env.maxmatches = O[o % 3], env.results = O[o / 3 % 3], env.side = O[o / 9 % 3], env.targets = O[o / 27];
            const bool overflow = (x & 1) != 0, replay_refused = (x & 2) != 0, cov_refused = (x & 4) != 0;
            const size_t nodd = (x & 8) != 0;
            const Events ev = {overflow, false, false, false, replay_refused, false, false};
            // the expression
            const Outcome old = old_run(env, gpus, nodd, ev, D);
            const bool env_device = env.coverage && !strcmp(env.coverage, "device"), env_host = env.coverage && !strcmp(env.coverage, "host");
            const bool want = env_device || (!env_host && D.coverage);
            const bool tried = old.results_on_device && old.list_on_device && want;
            // the plan, as stage_results and stage_coverage use it
            Placement plan = make_placement(env, gpus, D);
            if (nodd) plan.demote(Demotion::OddTargetBytes);
            if (overflow && plan.maxmatches == Where::Device && replay_refused) plan.demote(Demotion::ReplayRefused);
            const bool resident = plan.list_on_device(overflow);
            EXPECT(resident == old.list_on_device);
            EXPECT_MSG(plan.coverage_on_device(resident) == tried, "coverage plan differs: default %d env %d others %d GPUs %d events %d", d, e, o, gpus, x);
            if (plan.coverage_on_device(resident) && cov_refused) plan.demote(Demotion::CoverageRefused);
            EXPECT(plan.coverage_on_device(resident) == (tried && !cov_refused));
            EXPECT(plan.coverage == Where::Host || plan.results == Where::Device);
            // nothing else moves
            PlanEnv unset = env;
            unset.coverage = nullptr;
            EXPECT(new_run(env, gpus, nodd, ev, D) == new_run(unset, gpus, nodd, ev, PlanDefaults()));
            // ... the SAM file included: each of the two moves on its own
            Placement both = make_placement(env, gpus, D), none = make_placement(unset, gpus, PlanDefaults());
            EXPECT(both.sam == none.sam);
            both.demote(Demotion::SamRefused);
            EXPECT(both.coverage == make_placement(env, gpus, D).coverage);
            n++;
          }
  EXPECT(!PlanDefaults().coverage);  // unmeasured: the host makes the coverage files unless MUSC_COVERAGE=device
  return n;
}

// The size rules of sam_plan.hpp against text built byte by byte: decimal widths, the CIGAR, MD over random mismatch
// places (forward and reverse: the same length), a whole record, and the name rules on blocks of their exact size.
unsigned long long check_sam_sizes() {
  using namespace musc_sam;
  unsigned long long n = 0;
  for (uint64_t v : {0ull, 9ull, 10ull, 99ull, 100ull, 65535ull, 4294967295ull, 4294967296ull, 9999999999ull, 10000000000ull})
    EXPECT(ndigits(v) == std::to_string(v).size());
  EXPECT(flag(false, true) == 0 && flag(true, true) == 16 && flag(false, false) == 256 && flag(true, false) == 272);
  EXPECT(pos1(false, 100, 7, 20) == 8 && pos1(true, 100, 7, 20) == 74 && pos1(true, 100, 100, 0) == 1 && pos1(false, 100, 100, 0) == 101);
  std::mt19937 rng(28);
  for (int it = 0; it < 20000; it++) {
    const uint32_t L = 1 + rng() % (it % 50 == 0 ? 5000 : 300), S = it % 7 == 0 ? rng() % (L + 1) : L;
    std::string cigar = S == 0 ? "*" : std::to_string(S) + "M" + (L > S ? std::to_string(L - S) + "S" : "");
    EXPECT(cigar_bytes(L, S) == cigar.size());
    // mismatch places: none, all, or each with a probability that leaves runs of every width
    const unsigned mode = rng() % 8;
    std::vector<bool> mis(S);
    for (uint32_t j = 0; j < S; j++) mis[j] = mode == 0 ? false : mode == 1 ? true : rng() % (mode == 2 ? 2 : 120) == 0;
    MdSize z;
    std::string fwd, rev;
    size_t run = 0;
    for (uint32_t j = 0; j < S; j++) {
      if (!mis[j]) { run++; continue; }
      z.mismatch(j);
      fwd += std::to_string(run) + "A";
      run = 0;
    }
    fwd += std::to_string(run);
    run = 0;
    for (uint32_t j = S; j-- > 0;) {
      if (!mis[j]) { run++; continue; }
      rev += std::to_string(run) + "A";
      run = 0;
    }
    rev += std::to_string(run);
    EXPECT(z.finish(S) == fwd.size() && fwd.size() == rev.size());
    const RecordSizes r = {1 + (uint32_t)(rng() % 254), flag(rng() & 1, rng() & 1), 1 + (uint32_t)(rng() % 40), 1 + rng() % 5000000000ull, L, S, z.nmis,
                           z.finish(S), 1 + (uint32_t)(rng() % 3000), 1 + (uint32_t)(rng() % 3000), (uint32_t)(rng() % 70000), (uint32_t)(rng() % 9)};
    const std::string text = std::string(r.qname, 'q') + "\t" + std::to_string(r.flag) + "\t" + std::string(r.rname, 'r') + "\t" + std::to_string(r.pos1) +
                             "\t255\t" + cigar + "\t*\t0\t0\t" + std::string(L, 'A') + "\t*\tNM:i:" + std::to_string(r.d) + "\tMD:Z:" + fwd + "\tNH:i:" +
                             std::to_string(r.nh) + "\tHI:i:" + std::to_string(r.hi) + "\tXM:i:" + std::to_string(r.nmiss) +
                             (r.count_len ? "\tXC:i:" + std::string(r.count_len, '7') : std::string()) + "\n";
    EXPECT(record_bytes(r) == text.size());
    n++;
  }
  EXPECT(sq_bytes(4, 12345) == std::string("@SQ\tSN:chr1\tLN:12345\n").size());
  EXPECT(std::string(HD_LINE).size() == HD_BYTES && std::string(PG_LINE).size() == PG_BYTES && HD_LINE[HD_BYTES - 1] == '\n');
  // the name rules, each text in a heap block of its exact size
  struct T { const char* tail; size_t n; uint32_t count_len, q0, qlen; };
  const std::string long_name = "5\t" + std::string(300, 'n');
  const T tails[] = {{"12\tname;x", 9, 2, 3, 4}, {"1\t@name rest", 12, 1, 3, 4}, {"1\t>n", 4, 1, 3, 1}, {"1\t@@n", 5, 1, 3, 2}, {"7", 1, 1, 1, 0},
                     {"", 0, 0, 0, 0}, {"\tn", 2, 0, 1, 1}, {"x1\tn", 4, 0, 3, 1}, {"3\t", 2, 1, 2, 0}, {"3\t;n", 4, 1, 2, 0}, {"3\t n", 4, 1, 2, 0},
                     {"3\t@", 3, 1, 3, 0}, {"3\tn\x0bm", 5, 1, 2, 1}, {long_name.c_str(), long_name.size(), 1, 2, QNAME_MAX}};
  for (const T& t : tails) {
    std::unique_ptr<unsigned char[]> b(new unsigned char[t.n ? t.n : 1]);
    memcpy(b.get(), t.tail, t.n);
    const TailSpans s = tail_spans(b.get(), t.n);
    EXPECT_MSG(s.count_len == t.count_len && s.qlen == t.qlen && (s.qlen == 0 || s.q0 == t.q0), "tail_spans(%s)", t.tail);
    n++;
  }
  struct G { const char* text; size_t n; uint32_t n0, len; };
  const G genes[] = {{"chr1\t300", 8, 0, 4}, {">chr1 x\t300", 11, 1, 4}, {"  chr2", 6, 2, 4}, {">>a", 3, 1, 2}, {">", 1, 1, 0}, {"> a", 3, 1, 0},
                     {"", 0, 0, 0}, {" \t ", 3, 3, 0}, {"\t30", 3, 1, 2}};
  for (const G& g : genes) {
    std::unique_ptr<unsigned char[]> b(new unsigned char[g.n ? g.n : 1]);
    memcpy(b.get(), g.text, g.n);
    const NameSpan s = rname_span(b.get(), g.n);
    EXPECT_MSG(s.len == g.len && (s.len == 0 || s.n0 == g.n0), "rname_span(%s)", g.text);
    n++;
  }
  return n;
}

// The rules of cov_plan.hpp: the weight parse with its saturation against strtoull on blocks of their exact size, the
// record byte counts against text built byte by byte, the refusal bounds, the key arithmetic at the largest database
// the library loads (2^36 bases, 2^24 targets), and the whole event scheme -- interval, slot, sort, running sum, runs --
// against a per-base count on small random databases, pairs folded or not.
unsigned long long check_cov_sizes() {
  using namespace musc_cov;
  unsigned long long n = 0;
  // ---- the weight
  struct W { const char* tail; size_t len; uint64_t w; };
  const W tails[] = {{"0\tn", 3, 0}, {"1\tn", 3, 1}, {"12345\tn", 7, 12345}, {"007\tn", 5, 7}, {"x9\tn", 4, 1}, {"9x\tn", 4, 1}, {"\tn", 2, 1},
                     {"42", 2, 42}, {"nocount", 7, 1}, {"", 0, 1}, {"5 \tn", 4, 1}, {"-3\tn", 4, 1}, {"4294967295\tn", 12, 4294967295ull},
                     {"4294967296\tn", 12, WEIGHT_LIMIT}, {"4294967297", 10, WEIGHT_LIMIT}, {"10000000000\tn", 13, WEIGHT_LIMIT},
                     {"99999999999999999999999999\tn", 28, WEIGHT_LIMIT}, {"000000000000000000000000012\tn", 29, 12}};
  for (const W& t : tails) {
    std::unique_ptr<unsigned char[]> b(new unsigned char[t.len ? t.len : 1]);
    memcpy(b.get(), t.tail, t.len);
    EXPECT_MSG(weight(b.get(), t.len) == t.w, "weight(%s)", t.tail);
    n++;
  }
  std::mt19937_64 rng(29);
  for (int it = 0; it < 20000; it++) {
    const uint64_t v = it % 3 == 0 ? rng() : it % 3 == 1 ? rng() >> 31 : rng() % 100000;
    const std::string text = std::to_string(v) + (it & 1 ? "\tname" : "");
    std::unique_ptr<unsigned char[]> b(new unsigned char[text.size()]);
    memcpy(b.get(), text.data(), text.size());
    EXPECT(weight(b.get(), text.size()) == (v < WEIGHT_LIMIT ? v : WEIGHT_LIMIT));
    n++;
  }
  // ---- the refusal bounds
  EXPECT(!total_refused(0) && !total_refused(WEIGHT_LIMIT - 1) && total_refused(WEIGHT_LIMIT) && total_refused(~0ull));
  EXPECT(!lines_refused(0) && !lines_refused(LINES_LIMIT - 1) && lines_refused(LINES_LIMIT));
  EXPECT(ALL_FLAGS == 7u);
  // ---- the records
  for (int it = 0; it < 20000; it++) {
    const uint32_t name = 1 + (uint32_t)(rng() % 40), depth = (uint32_t)(rng() >> (32 + rng() % 32)), nr = (uint32_t)(rng() >> (32 + rng() % 32));
    const uint64_t start = rng() >> (28 + rng() % 36), end = start + 1 + (rng() >> (30 + rng() % 34)), cov = rng() >> (28 + rng() % 36), sum = rng() >> (16 + rng() % 48);
    const std::string run = std::string(name, 'r') + "\t" + std::to_string(start) + "\t" + std::to_string(end) + "\t" + std::to_string(depth) + "\n";
    EXPECT(run_bytes(name, start, end, depth) == run.size());
    const std::string rec = std::string(name, 'r') + "\t" + std::to_string(end) + "\t" + std::to_string(nr) + "\t" + std::to_string(cov) + "\t" +
                            std::to_string(sum) + "\t" + std::to_string(depth) + "\n";
    EXPECT(summary_bytes(name, end, nr, cov, sum, depth) == rec.size());
    n++;
  }
  // ---- the keys at the library's bounds: every slot of a database of nbases bases in nseq targets is below
  // nbases + nseq, which the end bit covers; the slots of consecutive targets do not meet
  for (unsigned bb = 0; bb <= 36; bb++)
    for (unsigned sb = 0; sb <= 24; sb++)
      for (int d = -1; d <= 1; d++) {
        const uint64_t nbases = (1ull << bb) + (uint64_t)d, nseq = 1ull << sb;
        if (nbases > (1ull << 36)) continue;
        const unsigned end = sort_end_bit(nbases, nseq);
        const uint64_t top = slot(nbases - (nbases ? 1 : 0), (uint32_t)(nseq - 1), nbases ? 1 : 0);  // the last slot of a last target of one base
        EXPECT(end >= 1 && end <= 37 && top == nbases + nseq - 1);
        EXPECT(end == 64 || top < (1ull << end));
        EXPECT(end == 1 || ((nbases + nseq) >> (end - 1)) == 1);  // the width, and not a bit more
        n++;
      }
  EXPECT(sort_end_bit(1ull << 36, 1ull << 24) == 37 && sort_end_bit(0, 0) == 1 && sort_end_bit(3, 1) == 3);
  // ---- the scheme against a per-base count
  for (int it = 0; it < 3000; it++) {
    const bool rev_pairs = it & 1;
    const uint32_t nt = 2 * (1 + (uint32_t)(rng() % 4));
    std::vector<uint64_t> len(nt), off(nt + 1, 0);
    for (uint32_t g = 0; g < nt; g++) len[g] = rev_pairs && (g & 1) ? len[g - 1] : rng() % 40;
    for (uint32_t g = 0; g < nt; g++) off[g + 1] = off[g] + len[g];
    std::vector<std::vector<uint64_t>> depth(nt);
    for (uint32_t g = 0; g < nt; g++) depth[g].assign(len[g], 0);
    std::vector<std::pair<uint64_t, uint32_t>> ev;
    const int lines = (int)(rng() % 30);
    for (int i = 0; i < lines; i++) {
      const uint32_t g = (uint32_t)(rng() % nt);
      const uint64_t pos = rng() % (len[g] + 1), L = rng() % 25, w = rng() % 4;
      const Interval v = interval(rev_pairs, g, pos, len[g], L);
      EXPECT(v.S == std::min(L, len[g] - pos) && v.a + v.S <= len[v.f] && (!rev_pairs || !(v.f & 1)));
      // by hand: base pos + j of an odd target is base len - 1 - pos - j of the even one
      for (uint64_t j = 0; j < v.S; j++) depth[v.f][rev_pairs && (g & 1) ? len[g] - 1 - pos - j : pos + j] += w;
      ev.push_back({slot(off[v.f], v.f, v.a), (uint32_t)w});
      ev.push_back({slot(off[v.f], v.f, v.a + v.S), 0u - (uint32_t)w});
    }
    std::stable_sort(ev.begin(), ev.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
    for (const auto& e : ev) EXPECT(e.first < (1ull << sort_end_bit(off[nt], nt)));
    // the depth from every slot on is the running sum at the last event of the slot; between targets it is zero
    std::vector<std::vector<uint64_t>> swept(nt);
    size_t e = 0;
    uint32_t sum = 0;
    for (uint32_t g = 0; g < nt; g++) {
      EXPECT(sum == 0);
      for (uint64_t x = 0; x <= len[g]; x++) {
        for (; e < ev.size() && ev[e].first == slot(off[g], g, x); e++) sum += ev[e].second;
        if (x < len[g]) swept[g].push_back(sum);
      }
    }
    EXPECT(e == ev.size() && sum == 0 && swept == depth);
    n++;
  }
  return n;
}

// ---- the names ------------------------------------------------------------------------------------------------

// a name in a heap block of its exact size (no terminator, no slack): a read past it is the sanitizer's to see
struct Block {
  std::unique_ptr<char[]> p;
  size_t n;
  explicit Block(const std::string& s) : p(new char[s.size()]), n(s.size()) { s.copy(p.get(), n); }
  std::string str() const { return std::string(p.get(), n); }
};

// prep_reads as it was: names clipped when parsed, a group sorted as pointers to the whole names
std::string old_host_names(const std::vector<Block>& raw) {
  std::vector<std::string> names;
  for (auto& b : raw) {
    std::string rn = b.str();
    if (rn.size() > 1000) rn = rn.substr(0, 995) + "...";
    names.push_back(std::move(rn));
  }
  std::vector<const std::string*> grp;
  for (auto& s : names) grp.push_back(&s);
  std::sort(grp.begin(), grp.end(), [](const std::string* a, const std::string* b) { return *a < *b; });
  std::string na;
  for (size_t i = 0; i < grp.size(); i++) {
    if (i) na += ';';
    na += grp[i]->substr(0, grp[i]->find('\t'));
  }
  if (na.size() > 1000) na = na.substr(0, 996) + "...";
  return na;
}

// prep_reads_device as it was: the clipped names of a group sorted as strings
std::string old_device_names(const std::vector<Block>& raw) {
  std::vector<std::string> grp;
  for (auto& b : raw) {
    std::string rn = b.str();
    if (rn.size() > 1000) rn = rn.substr(0, 995) + "...";
    grp.push_back(std::move(rn));
  }
  std::sort(grp.begin(), grp.end());
  std::string na;
  for (size_t i = 0; i < grp.size(); i++) {
    if (i) na += ';';
    na += grp[i].substr(0, grp[i].find('\t'));
  }
  if (na.size() > 1000) na = na.substr(0, 996) + "...";
  return na;
}

std::string new_names(const std::vector<Block>& raw) {
  std::vector<std::string> grp;
  for (auto& b : raw) grp.push_back(clip_name(b.str()));
  return join_group_names(grp.data(), grp.data() + grp.size());
}

// all three agree (so the two old loops agree with each other: one comparison serves both callers); returns the join
std::string check_group(const std::vector<std::string>& group) {
  std::vector<Block> raw;
  for (auto& s : group) raw.emplace_back(s);
  const std::string a = old_host_names(raw), b = old_device_names(raw), c = new_names(raw);
  EXPECT(a == b);
  EXPECT(a == c);
  return c;
}

unsigned long long check_names() {  // -> the random groups seen
  const std::string x999(999, 'x'), x1000(1000, 'y'), x1001(1001, 'z');
  EXPECT(clip_name(x999) == x999 && clip_name(x1000) == x1000);
  EXPECT(clip_name(x1001) == std::string(995, 'z') + "...");
  EXPECT(check_group({x999}) == x999);
  EXPECT(check_group({x1000}) == x1000);
  EXPECT(check_group({x1001}).size() == 998);
  EXPECT(check_group({x1001, x999, x1000}) == x999.substr(0, 996) + "...");
  // a join of exactly 1000 bytes stays, one of 1001 is clipped
  EXPECT(check_group({std::string(500, 'b'), std::string(499, 'a')}) == std::string(499, 'a') + ";" + std::string(500, 'b'));
  EXPECT(check_group({std::string(500, 'b'), std::string(500, 'a')}) == std::string(500, 'a') + ";" + std::string(495, 'b') + "...");
  // a clipped name cut at a tab beyond byte 995 keeps its "..."; one cut before it does not
  EXPECT(check_group({std::string(10, 'q') + "\t" + std::string(1200, 'r')}) == std::string(10, 'q'));
  EXPECT(check_group({"\tabc"}) == "");                    // a tab at byte 0
  EXPECT(check_group({"\tabc", "d"}) == ";d");
  EXPECT(check_group({"a\tb\tc"}) == "a");                 // two tabs
  EXPECT(check_group({"n\tz", "n\ta", "m"}) == "m;n;n");   // equal up to the tab, different after it
  EXPECT(check_group({"n\tz", "n", "n\t"}) == "n;n;n");
  EXPECT(check_group({"only"}) == "only");                 // a single name
  EXPECT(check_group({""}) == "");                         // an empty name
  EXPECT(check_group({"", "a", ""}) == ";;a");
  EXPECT(check_group({"b;a", "a"}) == "a;b;a");
  EXPECT(check_group({"B", "a", "\x80", "A"}) == std::string("A;B;a;\x80"));  // bytewise: unsigned

  std::mt19937 rng(20);
  static const char alphabet[] = {'a', 'b', '\t', ';', ' ', '\xff'};
  unsigned long long n = 0;
  for (int it = 0; it < 4000; it++) {
    std::vector<std::string> group(1 + rng() % 8);
    for (auto& s : group) {
      const unsigned kind = rng() % 16;
      const size_t len = kind == 0 ? 990 + rng() % 20 : kind == 1 ? 120 + rng() % 140 : rng() % 12;
      for (size_t i = 0; i < len; i++) s += alphabet[rng() % (kind ? 6 : 3)];
    }
    check_group(group);
    n++;
  }
  return n;
}

}  // namespace

int main() {
  char census[160];
  const unsigned long long n_plans = check_plan() + check_names_plan() + check_sam_plan() + check_cov_plan(), n_groups = check_names();
  const unsigned long long n_sam = check_sam_sizes(), n_cov = check_cov_sizes();
  snprintf(census, sizeof census, "%llu plan combinations, %llu random name groups, %llu SAM size cases, %llu coverage cases", n_plans, n_groups, n_sam, n_cov);
  return check_done("cli_plan_check", census);
}
