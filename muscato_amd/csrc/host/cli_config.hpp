// cli_config.hpp -- the reference's utils.Config and flag surface for the host tools: the configuration record, the
// reader and writer of its flat JSON object, the Go `flag` syntax, handleArgs and checkArgs.  Every function cites the
// reference code whose behaviour it reproduces (paths relative to kshedden/muscato).
#pragma once

#include <algorithm>
#include <cctype>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/muscato_hip.h"
#include "sz.hpp"

namespace musc {

// utils.Config (utils/config.go:10-101) + the additions of this build
struct Config {
  std::string ReadFileName, GeneFileName, GeneIdFileName, ResultsFileName;
  std::vector<int> Windows;
  int WindowWidth = 0;
  uint64_t BloomSize = 0;
  int NumHash = 0;
  double PMatch = 0;
  int MinDinuc = 0;
  std::string TempDir, LogDir;
  int MinReadLength = 0, MaxReadLength = 0, MaxMatches = 0, MaxConfirmProcs = 0, MMTol = 0;
  std::string MatchMode;
  int SortPar = 0;
  std::string SortTemp, SortMem;
  bool NoCleanTemp = false, CPUProfile = false;
  // additions (not in the reference): absolute mismatch budget and GPU selection
  int MaxMismatch = -1;  // --MaxMismatch: nmiss budget for every read instead of PMatch
  int GPUs = 1;          // --GPUs: shard the unique reads over this many devices
  int Device = 0;        // --Device: first device ordinal
  long long DbPartitionBases = 0;  // --DbPartitionBases: most target bases indexed at once, 0 = automatic
  std::string SamFileName;         // --SamFileName: also write the results as SAM; empty = no SAM file
  bool SamRev = false;             // --SamRev: the gene file was prepared with -rev, odd targets are reverse strands
  std::string CoverageFileName;    // --CoverageFileName: also write a bedGraph here and a summary to <name>_targets
  bool CoverageRev = false;        // --CoverageRev: the same fact as SamRev, for the coverage files
  bool CoverageWeighted = false;   // --CoverageWeighted: a line counts by its read's count
  bool CoverageUnique = false;     // --CoverageUnique: only the lines of reads with one line count
};

struct Die : std::runtime_error {
  int code;
  Die(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

// ---- minimal JSON reader for the flat config object (encoding/json semantics that matter:
// case-insensitive keys, unknown keys ignored, null leaves the field untouched)
struct JsonCursor {
  const std::string& s;
  size_t p = 0;
  explicit JsonCursor(const std::string& t) : s(t) {}
  void ws() { while (p < s.size() && isspace((unsigned char)s[p])) p++; }
  bool eat(char c) { ws(); if (p < s.size() && s[p] == c) { p++; return true; } return false; }
  void need(char c) { if (!eat(c)) throw Die(1, std::string("config: expected '") + c + "' at offset " + std::to_string(p)); }
  std::string str() {
    need('"');
    std::string o;
    while (p < s.size() && s[p] != '"') {
      char c = s[p++];
      if (c == '\\' && p < s.size()) {
        char e = s[p++];
        switch (e) {
          case 'n': o += '\n'; break; case 't': o += '\t'; break; case 'r': o += '\r'; break;
          case 'b': o += '\b'; break; case 'f': o += '\f'; break;
          case 'u': { unsigned v = 0; for (int i = 0; i < 4 && p < s.size(); i++) v = v * 16 + (unsigned)strtol(std::string(1, s[p++]).c_str(), nullptr, 16);
                      if (v < 0x80) o += (char)v; else if (v < 0x800) { o += (char)(0xC0 | (v >> 6)); o += (char)(0x80 | (v & 0x3F)); }
                      else { o += (char)(0xE0 | (v >> 12)); o += (char)(0x80 | ((v >> 6) & 0x3F)); o += (char)(0x80 | (v & 0x3F)); } break; }
          default: o += e;
        }
      } else {
        o += c;
      }
    }
    need('"');
    return o;
  }
  std::string scalar() {  // number / true / false / null as text
    ws();
    size_t b = p;
    while (p < s.size() && (isalnum((unsigned char)s[p]) || s[p] == '-' || s[p] == '+' || s[p] == '.')) p++;
    return s.substr(b, p - b);
  }
};

inline void config_from_json(const std::string& text, Config& c) {
  JsonCursor j(text);
  j.need('{');
  if (j.eat('}')) return;
  do {
    const std::string key = to_lower(j.str());
    j.need(':');
    j.ws();
    if (j.p < text.size() && text[j.p] == '"') {
      const std::string v = j.str();
      if (key == "readfilename") c.ReadFileName = v; else if (key == "genefilename") c.GeneFileName = v;
      else if (key == "geneidfilename") c.GeneIdFileName = v; else if (key == "resultsfilename") c.ResultsFileName = v;
      else if (key == "tempdir") c.TempDir = v; else if (key == "logdir") c.LogDir = v;
      else if (key == "matchmode") c.MatchMode = v; else if (key == "sorttemp") c.SortTemp = v;
      else if (key == "sortmem") c.SortMem = v; else if (key == "samfilename") c.SamFileName = v;
      else if (key == "coveragefilename") c.CoverageFileName = v;
    } else if (j.p < text.size() && text[j.p] == '[') {
      j.need('[');
      std::vector<int> v;
      if (!j.eat(']')) {
        do { v.push_back(atoi(j.scalar().c_str())); } while (j.eat(','));
        j.need(']');
      }
      if (key == "windows") c.Windows = v;
    } else {
      const std::string v = j.scalar();
      if (v == "null" || v.empty()) continue;
      const bool b = v == "true";
      const double d = (v == "true" || v == "false") ? (double)b : atof(v.c_str());
      if (key == "windowwidth") c.WindowWidth = (int)d; else if (key == "bloomsize") c.BloomSize = (uint64_t)d;
      else if (key == "numhash") c.NumHash = (int)d; else if (key == "pmatch") c.PMatch = d;
      else if (key == "mindinuc") c.MinDinuc = (int)d; else if (key == "minreadlength") c.MinReadLength = (int)d;
      else if (key == "maxreadlength") c.MaxReadLength = (int)d; else if (key == "maxmatches") c.MaxMatches = (int)d;
      else if (key == "maxconfirmprocs") c.MaxConfirmProcs = (int)d; else if (key == "mmtol") c.MMTol = (int)d;
      else if (key == "sortpar") c.SortPar = (int)d; else if (key == "nocleantemp") c.NoCleanTemp = b;
      else if (key == "cpuprofile") c.CPUProfile = b; else if (key == "maxmismatch") c.MaxMismatch = (int)d;
      else if (key == "gpus") c.GPUs = (int)d; else if (key == "device") c.Device = (int)d;
      else if (key == "dbpartitionbases") c.DbPartitionBases = (long long)d; else if (key == "samrev") c.SamRev = b;
      else if (key == "coveragerev") c.CoverageRev = b; else if (key == "coverageweighted") c.CoverageWeighted = b;
      else if (key == "coverageunique") c.CoverageUnique = b;
    }
  } while (j.eat(','));
  j.need('}');
}

inline std::string json_escape(const std::string& s) {
  std::string o;
  for (char c : s) {
    if (c == '"' || c == '\\') { o += '\\'; o += c; }
    else if (c == '\n') o += "\\n"; else if (c == '\t') o += "\\t";
    else o += c;
  }
  return o;
}

// saveConfig (cmd/muscato/main.go:680-697): the resolved configuration, one JSON object
inline std::string config_to_json(const Config& c) {
  std::string w = "[";
  for (size_t i = 0; i < c.Windows.size(); i++) w += (i ? "," : "") + std::to_string(c.Windows[i]);
  w += "]";
  char buf[64];
  snprintf(buf, sizeof buf, "%.17g", c.PMatch);
  auto S = [](const std::string& k, const std::string& v) { return "\"" + k + "\":\"" + json_escape(v) + "\""; };
  auto N = [](const std::string& k, long long v) { return "\"" + k + "\":" + std::to_string(v); };
  auto B = [](const std::string& k, bool v) { return "\"" + k + "\":" + (v ? "true" : "false"); };
  return "{" + S("ReadFileName", c.ReadFileName) + "," + S("GeneFileName", c.GeneFileName) + "," +
         S("GeneIdFileName", c.GeneIdFileName) + "," + S("ResultsFileName", c.ResultsFileName) + ",\"Windows\":" + w +
         "," + N("WindowWidth", c.WindowWidth) + "," + N("BloomSize", (long long)c.BloomSize) + "," +
         N("NumHash", c.NumHash) + ",\"PMatch\":" + buf + "," + N("MinDinuc", c.MinDinuc) + "," +
         S("TempDir", c.TempDir) + "," + S("LogDir", c.LogDir) + "," + N("MinReadLength", c.MinReadLength) + "," +
         N("MaxReadLength", c.MaxReadLength) + "," + N("MaxMatches", c.MaxMatches) + "," +
         N("MaxConfirmProcs", c.MaxConfirmProcs) + "," + N("MMTol", c.MMTol) + "," + S("MatchMode", c.MatchMode) +
         "," + N("SortPar", c.SortPar) + "," + S("SortTemp", c.SortTemp) + "," + S("SortMem", c.SortMem) + "," +
         B("NoCleanTemp", c.NoCleanTemp) + "," + B("CPUProfile", c.CPUProfile) + "," +
         N("MaxMismatch", c.MaxMismatch) + "," + N("GPUs", c.GPUs) + "," + N("Device", c.Device) + "," +
         N("DbPartitionBases", c.DbPartitionBases) +
         // (the SAM keys only when a SAM file is asked for: without the flag the saved configuration is what it always was)
         (c.SamFileName.empty() ? std::string() : "," + S("SamFileName", c.SamFileName) + "," + B("SamRev", c.SamRev)) +
         // (the coverage keys likewise, only when a coverage file is asked for)
         (c.CoverageFileName.empty() ? std::string()
                                     : "," + S("CoverageFileName", c.CoverageFileName) + "," + B("CoverageRev", c.CoverageRev) + "," +
                                           B("CoverageWeighted", c.CoverageWeighted) + "," + B("CoverageUnique", c.CoverageUnique)) +
         "}\n";
}

// ---- Go `flag` syntax: -name, --name, -name=value, -name value; bools take no value unless
// written -name=value; parsing stops at the first non-flag or at "--".
struct FlagSpec { const char* name; char kind; const char* help; };  // kind: s i f b

inline const std::vector<FlagSpec>& muscato_flags() {
  // cmd/muscato/main.go:708-732 (same names, kinds and help strings) + the additions
  static const std::vector<FlagSpec> f = {
      {"ConfigFileName", 's', "JSON file containing configuration parameters"},
      {"ReadFileName", 's', "Sequencing read file (fastq format)"},
      {"GeneFileName", 's', "Gene file name (processed form)"},
      {"GeneIdFileName", 's', "Gene ID file name (processed form)"},
      {"ResultsFileName", 's', "File name for results"},
      {"Windows", 's', "Starting position of each window"},
      {"WindowWidth", 'i', "Width of each window"},
      {"BloomSize", 'i', "Size of Bloom filter, in bits"},
      {"NumHash", 'i', "Number of hashses"},
      {"PMatch", 'f', "Required proportion of matching positions"},
      {"MinDinuc", 'i', "Minimum number of dinucleotides to check for match"},
      {"TempDir", 's', "Workspace for temporary files"},
      {"MinReadLength", 'i', "Reads shorter than this length are skipped"},
      {"MaxReadLength", 'i', "Reads longer than this length are truncated"},
      {"MaxMatches", 'i', "Return no more than this number of matches per window"},
      {"MaxConfirmProcs", 'i', "Run this number of match confirmation processes concurrently"},
      {"MMTol", 'i', "Number of mismatches allowed above best fit"},
      {"MatchMode", 's', "'first' or 'best' (retain first/best 'MaxMatches' matches meeting criteria)"},
      {"NoCleanTemp", 'b', "Do not delete temporary files from TempDir"},
      {"SortPar", 'i', "Number of parallel sort processes"},
      {"SortTemp", 's', "Directory to use for sort temp files"},
      {"SortMem", 's', "Gnu sort -S parameter"},
      {"CPUProfile", 'b', "Capture CPU profile data"},
      {"MaxMismatch", 'i', "(addition) absolute mismatch budget per read; overrides PMatch when >= 0"},
      {"GPUs", 'i', "(addition) number of GPUs to shard the reads over"},
      {"Device", 'i', "(addition) first GPU ordinal"},
      {"DbPartitionBases", 'i', "(addition) most target bases indexed at once; 0 = automatic"},
      {"SamFileName", 's', "(addition) also write the results as a SAM file of this name"},
      {"SamRev", 'b', "(addition) the gene file was prepared with -rev: odd targets are reverse strands in the SAM file"},
      {"CoverageFileName", 's', "(addition) also write a bedGraph of the depth runs to this file and a per-target summary to <name>_targets"},
      {"CoverageRev", 'b', "(addition) the gene file was prepared with -rev: odd targets fold onto the even ones in the coverage files"},
      {"CoverageWeighted", 'b', "(addition) a line counts by its read's count in the coverage files"},
      {"CoverageUnique", 'b', "(addition) only reads with one line count in the coverage files"},
  };
  return f;
}

inline std::string usage(const char* prog, const std::vector<FlagSpec>& flags) {
  std::vector<FlagSpec> v = flags;
  std::sort(v.begin(), v.end(), [](const FlagSpec& a, const FlagSpec& b) { return strcmp(a.name, b.name) < 0; });
  std::string o = std::string("Usage of ") + prog + ":\n";
  for (auto& f : v) {
    const char* ty = f.kind == 's' ? " string" : f.kind == 'i' ? " int" : f.kind == 'f' ? " float" : "";
    o += std::string("  -") + f.name + ty + "\n    \t" + f.help + "\n";
  }
  return o;
}

// returns name -> value for the flags present; bools map to "true"/"false"
inline std::map<std::string, std::string> parse_flags(int argc, char** argv, const std::vector<FlagSpec>& flags,
                                                      std::vector<std::string>* rest) {
  std::map<std::string, std::string> out;
  int i = 1;
  for (; i < argc; i++) {
    std::string a = argv[i];
    if (a.size() < 2 || a[0] != '-') break;
    if (a == "--") { i++; break; }
    size_t b = a[1] == '-' ? 2 : 1;
    std::string name = a.substr(b), val;
    bool hasval = false;
    size_t eq = name.find('=');
    if (eq != std::string::npos) { val = name.substr(eq + 1); name = name.substr(0, eq); hasval = true; }
    if (name == "help" || name == "h") throw Die(0, usage(argv[0], flags));
    const FlagSpec* spec = nullptr;
    for (auto& f : flags) if (name == f.name) spec = &f;
    if (!spec) throw Die(2, "flag provided but not defined: -" + name + "\n" + usage(argv[0], flags));
    if (spec->kind == 'b') {
      if (!hasval) val = "true";
      if (val != "true" && val != "false" && val != "1" && val != "0" && val != "t" && val != "f" && val != "T" &&
          val != "F" && val != "TRUE" && val != "FALSE" && val != "True" && val != "False")
        throw Die(2, "invalid boolean value \"" + val + "\" for -" + name);
      val = (val[0] == 't' || val[0] == 'T' || val[0] == '1') ? "true" : "false";
    } else {
      if (!hasval) {
        if (i + 1 >= argc) throw Die(2, "flag needs an argument: -" + name);
        val = argv[++i];
      }
      if (spec->kind == 'i') {
        char* e = nullptr;
        strtoll(val.c_str(), &e, 0);
        if (val.empty() || *e) throw Die(2, "invalid value \"" + val + "\" for flag -" + name + ": parse error");
      } else if (spec->kind == 'f') {
        char* e = nullptr;
        strtod(val.c_str(), &e);
        if (val.empty() || *e) throw Die(2, "invalid value \"" + val + "\" for flag -" + name + ": parse error");
      }
    }
    out[name] = val;
  }
  if (rest) for (; i < argc; i++) rest->push_back(argv[i]);
  return out;
}

// handleArgs (cmd/muscato/main.go:708-831): JSON first, then every non-zero flag overrides
inline Config handle_args(int argc, char** argv) {
  auto fl = parse_flags(argc, argv, muscato_flags(), nullptr);
  Config c;
  auto has = [&](const char* k) { return fl.count(k) > 0; };
  auto I = [&](const char* k) { return (int)strtoll(fl[k].c_str(), nullptr, 0); };
  if (has("ConfigFileName") && !fl["ConfigFileName"].empty()) config_from_json(slurp(fl["ConfigFileName"]), c);
  if (has("ReadFileName") && !fl["ReadFileName"].empty()) c.ReadFileName = fl["ReadFileName"];
  if (has("GeneFileName") && !fl["GeneFileName"].empty()) c.GeneFileName = fl["GeneFileName"];
  if (has("GeneIdFileName") && !fl["GeneIdFileName"].empty()) c.GeneIdFileName = fl["GeneIdFileName"];
  if (has("WindowWidth") && I("WindowWidth")) c.WindowWidth = I("WindowWidth");
  if (has("BloomSize") && I("BloomSize")) c.BloomSize = (uint64_t)strtoll(fl["BloomSize"].c_str(), nullptr, 0);
  if (has("NumHash") && I("NumHash")) c.NumHash = I("NumHash");
  if (has("PMatch") && atof(fl["PMatch"].c_str()) != 0) c.PMatch = atof(fl["PMatch"].c_str());
  if (has("MinDinuc") && I("MinDinuc")) c.MinDinuc = I("MinDinuc");
  if (has("TempDir") && !fl["TempDir"].empty()) c.TempDir = fl["TempDir"];
  if (has("MinReadLength") && I("MinReadLength")) c.MinReadLength = I("MinReadLength");
  if (has("MaxReadLength") && I("MaxReadLength")) c.MaxReadLength = I("MaxReadLength");
  if (has("MaxMatches") && I("MaxMatches")) c.MaxMatches = I("MaxMatches");
  if (has("MaxConfirmProcs") && I("MaxConfirmProcs")) c.MaxConfirmProcs = I("MaxConfirmProcs");
  if (has("MatchMode") && !fl["MatchMode"].empty()) c.MatchMode = fl["MatchMode"];
  if (has("MMTol") && I("MMTol")) c.MMTol = I("MMTol");
  if (has("ResultsFileName") && !fl["ResultsFileName"].empty()) c.ResultsFileName = fl["ResultsFileName"];
  if (has("NoCleanTemp") && fl["NoCleanTemp"] == "true") c.NoCleanTemp = true;
  if (has("CPUProfile") && fl["CPUProfile"] == "true") c.CPUProfile = true;
  if (has("SortPar") && I("SortPar")) c.SortPar = I("SortPar");
  if (has("SortMem") && !fl["SortMem"].empty()) c.SortMem = fl["SortMem"];
  if (has("SortTemp") && !fl["SortTemp"].empty()) c.SortTemp = fl["SortTemp"];
  if (has("MaxMismatch")) c.MaxMismatch = I("MaxMismatch");
  if (has("GPUs") && I("GPUs")) c.GPUs = I("GPUs");
  if (has("Device")) c.Device = I("Device");
  if (has("DbPartitionBases")) c.DbPartitionBases = strtoll(fl["DbPartitionBases"].c_str(), nullptr, 0);
  if (has("SamFileName") && !fl["SamFileName"].empty()) c.SamFileName = fl["SamFileName"];
  if (has("SamRev")) c.SamRev = fl["SamRev"] == "true";
  if (has("CoverageFileName") && !fl["CoverageFileName"].empty()) c.CoverageFileName = fl["CoverageFileName"];
  if (has("CoverageRev")) c.CoverageRev = fl["CoverageRev"] == "true";
  if (has("CoverageWeighted")) c.CoverageWeighted = fl["CoverageWeighted"] == "true";
  if (has("CoverageUnique")) c.CoverageUnique = fl["CoverageUnique"] == "true";
  if (c.ResultsFileName.empty()) {
    c.ResultsFileName = "results.txt";
    fputs("ResultsFileName not specified, defaulting to 'results.txt'\n", stderr);
  }
  if (has("Windows") && !fl["Windows"].empty()) {
    c.Windows.clear();
    std::string w = fl["Windows"];
    size_t p = 0;
    while (p <= w.size()) {
      size_t e = w.find(',', p);
      std::string tok = w.substr(p, e == std::string::npos ? std::string::npos : e - p);
      char* end = nullptr;
      long v = strtol(tok.c_str(), &end, 10);
      if (tok.empty() || *end) throw Die(1, "Error in handleArgs: bad Windows value \"" + tok + "\"");
      c.Windows.push_back((int)v);
      if (e == std::string::npos) break;
      p = e + 1;
    }
  }
  return c;
}

// checkArgs (cmd/muscato/main.go:833-904): required fields and defaults, same messages
inline void check_args(Config& c) {
  auto need = [](bool ok, const char* what) {
    if (!ok) throw Die(1, std::string("\n") + what + " not provided, run 'muscato --help for more information.\n\n");
  };
  need(!c.ReadFileName.empty(), "ReadFileName");
  need(!c.GeneFileName.empty(), "GeneFileName");
  need(!c.GeneIdFileName.empty(), "GeneIdFileName");
  need(!c.Windows.empty(), "Windows");
  need(c.WindowWidth != 0, "WindowWidth");
  if (c.BloomSize == 0) { fputs("BloomSize not provided, defaulting to 4 billion\n", stderr); c.BloomSize = 4000000000ull; }
  if (c.NumHash == 0) { fputs("NumHash not provided, defaulting to 20\n", stderr); c.NumHash = 20; }
  if (c.PMatch == 0) { fputs("PMatch not provided, defaulting to 1\n", stderr); c.PMatch = 1; }
  if (c.MaxReadLength == 0) throw Die(1, "MaxReadLength not provided, run 'muscato --help for more information.\n\n");
  if (c.MaxMatches == 0) { fputs("MaxMatches not provided, defaulting to 1 million\n", stderr); c.MaxMatches = 1000000; }
  if (c.MaxConfirmProcs == 0) { fputs("MaxConfirmProcs not provided, defaulting to 3\n", stderr); c.MaxConfirmProcs = 3; }
  if (!ends_with(c.ReadFileName, ".fastq"))
    fprintf(stderr, "Warning: %s may not be a fastq file, continuing anyway\n", c.ReadFileName.c_str());
  if (c.MatchMode.empty()) { fputs("MatchMode not provided, defaulting to 'best'\n", stderr); c.MatchMode = "best"; }
  if (c.MatchMode != "best" && c.MatchMode != "first") throw Die(1, "MatchMode must be 'first' or 'best'\n");
  if (c.SortPar == 0) c.SortPar = 8;
  if (c.SortMem.empty()) { fputs("SortMem not provided, defaulting to 50%\n", stderr); c.SortMem = "50%"; }
  if ((int)c.Windows.size() > MUSC_MAX_WINDOWS)
    throw Die(1, "at most " + std::to_string(MUSC_MAX_WINDOWS) + " windows are supported by this build\n");
  if (c.GPUs < 1) c.GPUs = 1;
  if (c.DbPartitionBases < 0) throw Die(1, "DbPartitionBases must be >= 0 (0 = automatic)\n");
}

}  // namespace musc
