// cli_plan.hpp -- where each stage of a `muscato` run takes place, decided once.  Plain C++17: no
// library call and no getenv here; the driver reads the seven environment values in one place and passes them in.
// Included by muscato_host.hpp and by cli_plan_check.cpp, the stand-alone program that holds it to the boolean
// expressions it replaced, under the sanitizers.
#pragma once

#include <cstddef>
#include <cstring>

namespace musc {

// 1: with one GPU the CLI orders and renders results.txt on the device unless MUSC_RESULTS=host; 0: only with
// MUSC_RESULTS=device.  Measured (profiles/results_render.py): the results.txt lap of a 2 M-read run is
// 0.24 s on the device against 1.1 s on the host, the runs of either side within 0.25 s of each other.
#ifndef MUSC_RESULTS_DEFAULT_DEVICE
#define MUSC_RESULTS_DEFAULT_DEVICE 1
#endif

// 1: when results.txt came from the device the CLI also takes the three side outputs from it unless MUSC_SIDE=host;
// 0: only with MUSC_SIDE=device.  Measured (profiles/side_outputs.py): the `nonmatch + stats files` lap
// of a 2 M-read run is 0.10 s on the device against 1.41 s on the host, the runs of either side within 0.23 s of each other.
#ifndef MUSC_SIDE_DEFAULT_DEVICE
#define MUSC_SIDE_DEFAULT_DEVICE 1
#endif

// 1: the CLI replays the MaxMatches truncation on the device unless MUSC_MAXMATCHES=host; 0: only with
// MUSC_MAXMATCHES=device.  Measured (profiles/maxmatches.py): on a 2 M-read run with 150 truncated blocks
// the replay, results.txt and side-output laps add up to 0.39 s with the replay on the device against 1.52 s with it on
// the host, the runs of either side within 0.08 s of each other.
#ifndef MUSC_MAXMATCHES_DEFAULT_DEVICE
#define MUSC_MAXMATCHES_DEFAULT_DEVICE 1
#endif

// 1: the CLI parses the read file on the device unless MUSC_PREP=host; 0: only with MUSC_PREP=device.
#ifndef MUSC_PREP_DEFAULT_DEVICE
#define MUSC_PREP_DEFAULT_DEVICE 0
#endif

// 1: when the read file is parsed on the device the CLI also takes the names of the reads from it (their order within a
// group, the cut at the first tab, the join: DESIGN.md 23) unless MUSC_PREP_NAMES=host; 0: only with
// MUSC_PREP_NAMES=device.  0 until profiles/read_names.py has been run on more than one box.
#ifndef MUSC_PREP_NAMES_DEFAULT_DEVICE
#define MUSC_PREP_NAMES_DEFAULT_DEVICE 0
#endif

// 1: the CLI decodes, splits and packs the gene file on the device unless MUSC_TARGETS=host; 0: only with
// MUSC_TARGETS=device.  Measured (profiles/targets_load.py): the laps `windows check, target files` and
// `hot path (init, load, match)` of a 2 M-read run over a 100 MB gene file add up to 0.229 s with the gene file on the
// device against 0.503 s on the host, the runs of either side within 0.021 s of each other.
#ifndef MUSC_TARGETS_DEFAULT_DEVICE
#define MUSC_TARGETS_DEFAULT_DEVICE 1
#endif

// 1: when the ordered list is resident the CLI renders the SAM file (-SamFileName) on the device unless
// MUSC_SAM=host; 0: only with MUSC_SAM=device.  Unmeasured: 0 until profiles/sam.py has been run.
#ifndef MUSC_SAM_DEFAULT_DEVICE
#define MUSC_SAM_DEFAULT_DEVICE 0
#endif

// 1: when the ordered list is resident the CLI makes the coverage files (-CoverageFileName) on the device
// unless MUSC_COVERAGE=host; 0: only with MUSC_COVERAGE=device.  Unmeasured: 0 until profiles/coverage.py has been run.
#ifndef MUSC_COVERAGE_DEFAULT_DEVICE
#define MUSC_COVERAGE_DEFAULT_DEVICE 0
#endif

enum class Where { Host, Device };

// the nine environment values as the process has them, each possibly null
struct PlanEnv {
  const char *prep = nullptr, *maxmatches = nullptr, *results = nullptr, *side = nullptr, *gather = nullptr;
  const char* targets = nullptr;
  const char* prep_names = nullptr;
  const char* sam = nullptr;
  const char* coverage = nullptr;
};

// what a stage does when its variable does not say: the *_DEFAULT_DEVICE macros (arguments, so that the check program
// holds the plan to both values of each in one compile)
struct PlanDefaults {
  bool prep = MUSC_PREP_DEFAULT_DEVICE != 0, maxmatches = MUSC_MAXMATCHES_DEFAULT_DEVICE != 0,
       results = MUSC_RESULTS_DEFAULT_DEVICE != 0, side = MUSC_SIDE_DEFAULT_DEVICE != 0;
  bool targets = MUSC_TARGETS_DEFAULT_DEVICE != 0;
  bool prep_names = MUSC_PREP_NAMES_DEFAULT_DEVICE != 0;
  bool sam = MUSC_SAM_DEFAULT_DEVICE != 0;
  bool coverage = MUSC_COVERAGE_DEFAULT_DEVICE != 0;
};

// The parse rules, which are not the same for every variable (and stay so here):
//   MUSC_RESULTS, MUSC_SIDE, MUSC_MAXMATCHES,
//   MUSC_TARGETS, MUSC_PREP_NAMES, MUSC_SAM,
//   MUSC_COVERAGE                              "device" and "host" say so; unset, empty and every other value mean the
//                                              compiled default
//   MUSC_PREP                                  unset means the compiled default; once set, only "device" means the
//                                              device: empty and every other value mean the host
//   MUSC_GATHER                                counts only as exactly "rccl", and only with more than one GPU
inline Where place_by_env(const char* v, bool default_device) {
  if (v && !strcmp(v, "device")) return Where::Device;
  if (v && !strcmp(v, "host")) return Where::Host;
  return default_device ? Where::Device : Where::Host;
}
inline Where place_prep_by_env(const char* v, bool default_device) {
  if (v) return !strcmp(v, "device") ? Where::Device : Where::Host;
  return default_device ? Where::Device : Where::Host;
}

// Why a stage leaves the device.  The first two are known before the hot path has a context (static); the others are
// what a stage finds when it runs, and the driver logs each with the line DESIGN.md 20 lists.
enum class Demotion {
  SeveralGpus,       // the post-chain of several GPUs runs on the host: results, side outputs and the replay
  OddTargetBytes,    // targets with bytes that are none of ACGTX, which the device would render as X: results, hence side
  PrepNoMemory,      // musc_reads_prep_fastq found no device memory: the parse, and the names with it
  PrepNamesNoMemory, // musc_reads_prep_fastq_names found no device memory: the parse runs again without the names
  GatherFailed,      // musc_gather_rccl failed: the host gather takes over
  ReplayPassFailed,  // the reload or the pass in front of the replay failed (the run ends with that error)
  ReplayRefused,     // musc_maxmatches_apply returned 12 (refusal) or 10 (no memory)
  SideRefused,       // musc_side_prepare returned 12: a gene text that is not name\tlen without blanks
  TargetsNoMemory,   // musc_db_load_text found no device memory (10, "out of memory")
  TargetsRefused,    // ... returned 12: a chunk that declares more than 65 536 bytes, which sz_decode takes
  TargetsBadStream,  // ... returned 13: the host decoder then ends the run with its own message
  SamRefused,        // musc_sam_prepare returned 12 (refusal) or 10 (no memory): the host function writes the SAM file
  CoverageRefused,   // musc_cov_prepare returned 12 or 10: the host function makes the coverage files
};

struct Placement {
  Where prep = Where::Host, maxmatches = Where::Host, results = Where::Host, side = Where::Host;
  bool gather_rccl = false;
  // lines the driver owes the log for the static demotions (each as the expressions before the plan logged it)
  bool note_replay_gpus = false;  // "MaxMatches replay on the host: the post-chain of %d GPUs ...", when a replay is due
  bool note_odd_targets = false;  // "results on the host: the targets hold bytes that are none of ACGTX ..."
  int gpus = 1;
  bool results_env_host = false;
  Where targets = Where::Host;  // the gene file: snappy frames, lines, 2-bit pack
  // the names of the reads: on the device only when the parse is, since the stage reads them in the text
  // the parse keeps resident
  Where prep_names = Where::Host;
  // the SAM file: on the device only from an ordered list that is there, so whatever takes the results
  // to the host takes it along
  Where sam = Where::Host;
  // the coverage files: likewise
  Where coverage = Where::Host;

  // The one place a stage is moved to the host.  The side outputs are made from the ordered list behind results.txt,
  // which exists on the device only when results.txt was ordered there: whatever takes the results to the host takes
  // the side outputs along.
  void demote(Demotion why) {
    switch (why) {
      case Demotion::SeveralGpus:
        note_replay_gpus = maxmatches == Where::Device;
        maxmatches = results = side = sam = coverage = Where::Host;
        break;
      case Demotion::OddTargetBytes:
        note_odd_targets = gpus == 1 && !results_env_host;
        results = side = sam = coverage = Where::Host;
        break;
      case Demotion::PrepNoMemory: prep = prep_names = Where::Host; break;
      case Demotion::PrepNamesNoMemory: prep_names = Where::Host; break;
      case Demotion::GatherFailed: gather_rccl = false; break;
      case Demotion::ReplayPassFailed:
      case Demotion::ReplayRefused: maxmatches = Where::Host; break;
      case Demotion::SideRefused: side = Where::Host; break;
      case Demotion::TargetsNoMemory:
      case Demotion::TargetsRefused:
      case Demotion::TargetsBadStream: targets = Where::Host; break;
      case Demotion::SamRefused: sam = Where::Host; break;
      case Demotion::CoverageRefused: coverage = Where::Host; break;
    }
  }

  // Is the list results.txt is ordered from the one the last pass left on the device?  Without an overflow it is the
  // list of the only pass; after one it is the replay's selection, resident only when the replay ran on the device
  // (call this after the hot path, when every demotion of the replay has been applied).
  bool list_on_device(bool overflow) const { return results == Where::Device && (!overflow || maxmatches == Where::Device); }
  // Is the SAM file the device's?  Only when its variable or the default says so and the list is resident.
  bool sam_on_device(bool list_resident) const { return sam == Where::Device && list_resident; }
  // ... the coverage files?  By the same rule.
  bool coverage_on_device(bool list_resident) const { return coverage == Where::Device && list_resident; }
};

// The plan of a run, from what is known before any stage: the environment and the number of GPUs.  The target files
// are read after the read prep, so the one fact they add (a count of odd target bytes that is not zero) reaches the
// plan as demote(OddTargetBytes), before the hot path has a context.
inline Placement make_placement(const PlanEnv& env, int gpus, const PlanDefaults& def = PlanDefaults()) {
  Placement p;
  p.gpus = gpus;
  p.results_env_host = env.results && !strcmp(env.results, "host");
  p.prep = place_prep_by_env(env.prep, def.prep);
  p.prep_names = p.prep == Where::Device ? place_by_env(env.prep_names, def.prep_names) : Where::Host;
  p.maxmatches = place_by_env(env.maxmatches, def.maxmatches);
  p.results = place_by_env(env.results, def.results);
  p.side = p.results == Where::Device ? place_by_env(env.side, def.side) : Where::Host;
  p.gather_rccl = gpus > 1 && env.gather && !strcmp(env.gather, "rccl");
  p.targets = place_by_env(env.targets, def.targets);
  p.sam = p.results == Where::Device ? place_by_env(env.sam, def.sam) : Where::Host;
  p.coverage = p.results == Where::Device ? place_by_env(env.coverage, def.coverage) : Where::Host;
  if (gpus > 1) p.demote(Demotion::SeveralGpus);
  return p;
}

}  // namespace musc
