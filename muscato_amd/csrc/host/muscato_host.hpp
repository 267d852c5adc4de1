// Host side of the `muscato` drop-in: the reference's utils.Config / flag surface, read and
// target preparation, and the text post-chain to results.txt -- everything around the GPU hot
// path, which is reached only through the C ABI of include/muscato_hip.h.
//
// The reference host is compiled Go; no Go toolchain exists in this image, so the host is C++
// (see INTEGRATION.md for the cgo binding a Go host would use instead).  Every function cites
// the reference code whose behaviour it reproduces (paths relative to kshedden/muscato).
// This header: target and read preparation, the texts rendered on the device and the driver; Config and
// the flags, the host post-chain, the host replay, the name rules and the placement plan are the cli_*.hpp it includes.
#pragma once

#include <sys/stat.h>
#include <sys/types.h>
#include <unistd.h>

#include <cstdarg>
#include <memory>
#include <random>
#include <thread>

#include "../../../include/muscato_cov.h"
#include "../../../include/muscato_sam.h"
#include "cli_config.hpp"
#include "cli_maxmatches_host.hpp"
#include "cli_names.hpp"
#include "cli_plan.hpp"
#include "cli_text.hpp"

namespace musc {

// owners of what the library hands out
struct CtxDestroy { void operator()(musc_ctx* c) const { musc_destroy(c); } };
struct Ctx : std::unique_ptr<musc_ctx, CtxDestroy> {  // a context: musc_init .. musc_destroy
  using std::unique_ptr<musc_ctx, CtxDestroy>::unique_ptr;
  static Ctx init(int device) {  // empty when musc_init fails (its text is musc_last_error(nullptr))
    musc_ctx* c = nullptr;
    return Ctx(musc_init(device, &c) ? nullptr : c);
  }
};
struct HitsFree { void operator()(musc_hit* p) const { musc_free_hits(p); } };
typedef std::unique_ptr<musc_hit[], HitsFree> LibHits;  // a musc_hit** output
struct U32Free { void operator()(uint32_t* p) const { musc_free_u32(p); } };
typedef std::unique_ptr<uint32_t[], U32Free> LibU32;  // a uint32_t** output
struct FastqPrep {  // the arrays of musc_reads_prep_fastq (a zeroed struct is fine to free)
  musc_fastq_prep fp{};
  FastqPrep() = default;
  FastqPrep(const FastqPrep&) = delete;
  FastqPrep& operator=(const FastqPrep&) = delete;
  ~FastqPrep() { musc_fastq_prep_free(&fp); }
};

// ------------------------------------------------------------------------------------
// target preparation (cmd/muscato_prep_targets/main.go)
// ------------------------------------------------------------------------------------
inline void subx(std::string& s) {  // :68-80 and cmd/muscato_prep_reads/main.go:33-44
  for (auto& c : s) if (c != 'A' && c != 'T' && c != 'C' && c != 'G') c = 'X';
}

inline std::string revcomp(const std::string& s) {  // :48-66 (bytes outside ATGCX become 0)
  std::string b(s.size(), '\0');
  const size_t m = s.size();
  for (size_t i = 0; i < m; i++) {
    char o = 0;
    switch (s[i]) { case 'A': o = 'T'; break; case 'T': o = 'A'; break; case 'G': o = 'C'; break;
                    case 'C': o = 'G'; break; case 'X': o = 'X'; break; }
    b[m - 1 - i] = o;
  }
  return b;
}

struct PreparedTargets {
  std::vector<std::string> seqs;  // one line each of musc_<file>.sz
  std::vector<std::string> ids;   // "%011d\tname\tlen" lines of musc_ids_<file>.sz
};

inline std::string id_line(size_t num, const std::string& name, size_t len) {
  char b[32];
  snprintf(b, sizeof b, "%011zu", num);
  return std::string(b) + "\t" + name + "\t" + std::to_string(len);
}

inline PreparedTargets prep_targets_text(const std::string& raw, bool rev) {  // processText :82-141
  PreparedTargets out;
  size_t lnum = 0;
  for (auto& line : split_lines(raw)) {
    if (line.empty()) break;
    size_t t = line.find('\t');
    if (t == std::string::npos || line.find('\t', t + 1) != std::string::npos) break;  // reference logs + exit(0)
    std::string nam = line.substr(0, t), seq = line.substr(t + 1);
    subx(seq);
    out.seqs.push_back(seq);
    if (rev) out.seqs.push_back(revcomp(seq));
    out.ids.push_back(id_line(lnum++, nam, seq.size()));
    if (rev) out.ids.push_back(id_line(lnum++, nam + "_r", seq.size()));
  }
  return out;
}

inline PreparedTargets prep_targets_fasta(const std::string& raw, bool rev) {  // processFasta :143-213
  PreparedTargets out;
  std::string name, seq;
  auto flush = [&](const std::string& s, bool r) {
    out.seqs.push_back(s);
    out.ids.push_back(id_line(out.ids.size(), name + (r ? "_r" : ""), s.size()));
  };
  for (auto& line : split_lines(raw)) {
    if (line.empty()) throw Die(1, "muscato_prep_targets: empty line in FASTA input (the reference panics here)");
    if (line[0] == '>') {
      if (!seq.empty()) {
        subx(seq);
        flush(seq, false);
        if (rev) flush(revcomp(seq), true);
      }
      name = line;  // the leading '>' is kept (:199)
      seq.clear();
      continue;
    }
    seq += line;
  }
  if (!seq.empty()) {  // the last record is NOT subx-ed (:204-212)
    flush(seq, false);
    if (rev) flush(revcomp(seq), true);
  }
  return out;
}

// targets() + main (:215-333): .gz/.sz inputs, "fasta" decided on the original file name,
// outputs musc_<file>.sz and musc_ids_<file>.sz next to the input
// 1: muscato_prep_targets prepares on the device unless MUSC_PREP_TARGETS=host; 0: only with MUSC_PREP_TARGETS=device
// (read as MUSC_RESULTS is: place_by_env).  The tool has always run without a GPU, and the host chain stays its default
// (DESIGN.md 22).
#ifndef MUSC_PREP_TARGETS_DEFAULT_DEVICE
#define MUSC_PREP_TARGETS_DEFAULT_DEVICE 0
#endif

// what both sides of prep_targets_file share: the input's kind, decided on the original file name, and the outputs' names
struct PrepTargetsNames {
  bool gz = false, sz = false, fasta = false;
  std::string seq_out, id_out;
};
inline PrepTargetsNames prep_targets_names(const std::string& path) {
  PrepTargetsNames n;
  const std::string low = to_lower(path);
  n.gz = ends_with(low, ".gz");
  n.sz = !n.gz && ends_with(low, ".sz");
  n.fasta = ends_with(low, "fasta");
  size_t slash = path.rfind('/');
  std::string dir = slash == std::string::npos ? "" : path.substr(0, slash + 1);
  std::string file = slash == std::string::npos ? path : path.substr(slash + 1);
  std::string lowf = to_lower(file);
  if (ends_with(lowf, ".gz") || ends_with(lowf, ".sz")) file = file.substr(0, file.size() - 3);
  n.seq_out = dir + "musc_" + file + ".sz";
  n.id_out = dir + "musc_ids_" + file + ".sz";
  return n;
}

// The device side (musc_targets_prep, musc_targets_prep_sz).  false, after one line on stderr: the host chain
// runs instead -- no device, no device memory (10, "out of memory"), a refusal (12), or a bad .sz stream (13), which
// the host decoder then ends with its own message.  An empty FASTA line (14) ends the run as the host's Die does.
inline bool prep_targets_device(const std::string& path, const PrepTargetsNames& n, bool rev) {
  Ctx ctx = Ctx::init(0);
  if (!ctx) {
    fprintf(stderr, "targets prep on the host: no device (%s)\n", musc_last_error(nullptr));
    return false;
  }
  musc_ctx* c = ctx.get();
  auto demoted = [&](int rc, const std::string& e) {
    if (!(rc == 12 || rc == 13 || (rc == 10 && e.find("out of memory") != std::string::npos))) throw Die(1, "targets prep: " + e + "\n");
    fprintf(stderr, "targets prep on the host: the device stage returned %d (%s)\n", rc, e.c_str());
    return false;
  };
  auto u8 = [](const std::string& s) { return reinterpret_cast<const uint8_t*>(s.data()); };
  auto m8 = [](std::string& s) { return reinterpret_cast<uint8_t*>(&s[0]); };
  std::string raw = n.gz ? gz_decode_file(path) : slurp(path);
  if (n.sz) {
    uint64_t nout = 0;
    int rc = musc_sz_decode(c, u8(raw), raw.size(), nullptr, 0, 0, &nout);
    if (rc) return demoted(rc, musc_last_error(c));
    std::string text(nout, '\0');
    if ((rc = musc_sz_decode(c, u8(raw), raw.size(), m8(text), nout, 0, &nout))) return demoted(rc, musc_last_error(c));
    raw.swap(text);
  }
  musc_targets_prep_info info;
  int rc = musc_targets_prep(c, u8(raw), raw.size(), 0, n.fasta ? 1 : 0, rev ? 1 : 0, &info);
  if (rc == 14) throw Die(1, "muscato_prep_targets: empty line in FASTA input (the reference panics here)");
  if (rc) return demoted(rc, musc_last_error(c));
  // both texts are framed where they lie (musc_targets_prep_sz): one crossing each, of the stream's bytes
  std::string framed[2];
  const uint64_t nb[2] = {info.n_seq_bytes, info.n_id_bytes};
  const int compressed = sz_write_compressed() ? 1 : 0;
  for (int w = 0; w < 2; w++) {
    uint64_t nout = 0;
    if ((rc = musc_targets_prep_sz(c, w, compressed, nullptr, 0, 0, &nout))) return demoted(rc, musc_last_error(c));
    framed[w].resize(nout);
    if ((rc = musc_targets_prep_sz(c, w, compressed, m8(framed[w]), nout, 0, &nout))) return demoted(rc, musc_last_error(c));
    framed[w].resize(nout);
  }
  spit(n.seq_out, framed[0]);
  spit(n.id_out, framed[1]);
  fprintf(stderr, "targets prep on the device: %llu lines, %llu targets, %llu + %llu bytes of text, %.3f ms\n", (unsigned long long)info.n_lines,
          (unsigned long long)info.n_targets, (unsigned long long)nb[0], (unsigned long long)nb[1], info.ms);
  return true;
}

inline void prep_targets_file(const std::string& path, bool rev, std::string* seq_out, std::string* id_out,
                              Where where = Where::Host) {
  const PrepTargetsNames n = prep_targets_names(path);
  *seq_out = n.seq_out;
  *id_out = n.id_out;
  if (where == Where::Device && prep_targets_device(path, n, rev)) return;
  std::string raw;
  if (n.gz) raw = gz_decode_file(path);
  else if (n.sz) raw = sz_decode(slurp(path));
  else raw = slurp(path);
  PreparedTargets pt = n.fasta ? prep_targets_fasta(raw, rev) : prep_targets_text(raw, rev);
  std::string a, b;
  for (auto& s : pt.seqs) { a += s; a += '\n'; }
  for (auto& s : pt.ids) { b += s; b += '\n'; }
  spit(*seq_out, sz_write(a));
  spit(*id_out, sz_write(b));
}

// A whole text of `nrec` records and `nbytes` bytes from the device, in ranges of 2^20 records: `fetch(rec0, n, dst,
// capacity, &nb)` renders records [rec0, rec0 + n), clipped at the end, into dst and reports their bytes (it throws on
// a library error).
template <class Fetch>
inline std::string device_text(const char* what, uint64_t nrec, uint64_t nbytes, Fetch fetch) {
  std::string out(nbytes, '\0');
  uint64_t done = 0;
  for (uint64_t r0 = 0; r0 < nrec; r0 += 1u << 20) {
    uint64_t nb = 0;
    fetch(r0, (uint64_t)1 << 20, &out[done], nbytes - done, &nb);
    done += nb;
  }
  if (done != nbytes) throw Die(1, std::string(what) + ": the rendered ranges do not add up to the whole");
  return out;
}

// The same bytes from the device (musc_results_*): `c` holds the database and every read; device_list =
// the tuples are the list the last pass left on the device, else `hits`.  Throws Die on a library error.
inline std::string results_text_device(musc_ctx* c, bool device_list, const std::vector<musc_hit>& hits, const std::vector<UniqueRead>& reads,
                                       size_t n_targets, const std::map<uint64_t, std::string>& id_rest,
                                       float* ms_order, float* ms_text, uint64_t* nlines_out = nullptr) {
  auto check = [&](int rc) { if (rc) throw Die(1, std::string("results on the device failed: ") + musc_last_error(c)); };
  {
    std::string text;
    std::vector<uint64_t> off(n_targets + 1, 0);
    std::vector<uint8_t> absent(n_targets, 1);
    for (auto& kv : id_rest) {
      if (kv.first >= n_targets) continue;  // (no tuple names such a gene)
      absent[kv.first] = 0;
      off[kv.first + 1] = kv.second.size();
    }
    for (size_t g = 0; g < n_targets; g++) off[g + 1] += off[g];
    text.resize(off.back());
    for (auto& kv : id_rest)
      if (kv.first < n_targets) memcpy(&text[off[kv.first]], kv.second.data(), kv.second.size());
    check(musc_results_set_gene_text(c, text.data(), off.data(), absent.data(), (uint32_t)n_targets));
  }
  {
    std::string text;
    std::vector<uint64_t> off;
    off.reserve(reads.size() + 1);
    off.push_back(0);
    for (auto& u : reads) {
      text += std::to_string(u.count);
      text += '\t';
      text += u.names;
      off.push_back(text.size());
    }
    check(musc_results_set_read_text(c, text.data(), off.data(), reads.size()));
  }
  uint64_t nlines = 0, nbytes = 0;
  static const musc_hit none = {0, 0, 0, 0};
  check(musc_results_order(c, device_list ? nullptr : hits.empty() ? &none : hits.data(), hits.size(), 0, &nlines, &nbytes));
  std::string out = device_text("results on the device", nlines, nbytes, [&](uint64_t l0, uint64_t n, char* dst, uint64_t cap, uint64_t* nb) {
    check(musc_results_text(c, l0, n, dst, cap, 0, nb));
  });
  musc_results_last_ms(c, ms_order, ms_text);
  if (nlines_out) *nlines_out = nlines;
  return out;
}

// The nonmatch FASTQ, genestats and readstats (out[MUSC_SIDE_*]) from the device (musc_side_*): `c` has
// just ordered and rendered results.txt.  false: the library refuses the gene text (code 12: a name with a blank, as
// a hand-made id file can hold) and the host functions of cli_text.hpp are to run.  Throws Die on a library error.
inline bool side_texts_device(musc_ctx* c, std::string out[3], float* ms_prepare, float* ms_text) {
  uint64_t nrec[3], nbytes[3];
  const int rc = musc_side_prepare(c, nrec, nbytes);
  if (rc == 12) return false;
  auto check = [&](int r) { if (r) throw Die(1, std::string("side outputs on the device failed: ") + musc_last_error(c)); };
  check(rc);
  for (int w = 0; w < 3; w++)
    out[w] = device_text("side outputs on the device", nrec[w], nbytes[w], [&](uint64_t r0, uint64_t n, char* dst, uint64_t cap, uint64_t* nb) {
      check(musc_side_text(c, w, r0, n, dst, cap, 0, nb));
    });
  musc_side_last_ms(c, ms_prepare, ms_text);
  return true;
}

// The SAM file (header, then one record per line of results.txt) from the device (musc_sam_*): `c` has just
// ordered and rendered results.txt from the list the pass left there.  false: the library refuses (12: rev_pairs on a
// database that is not in pairs, a gene text without a name) or found no memory (10), *why says which, and the host
// function of cli_text.hpp is to run.  Throws Die on any other library error.
inline bool sam_text_device(musc_ctx* c, bool rev_pairs, size_t n_targets, std::string* out, std::string* why, float* ms_prepare, float* ms_text) {
  uint64_t nrec = 0, hbytes = 0, rbytes = 0;
  const int rc = musc_sam_prepare(c, rev_pairs ? 1 : 0, &nrec, &hbytes, &rbytes);
  if (rc == 12 || rc == 10) return *why = "the device stage returned " + std::to_string(rc) + " (" + musc_last_error(c) + ")", false;
  auto check = [&](int r) { if (r) throw Die(1, std::string("sam file on the device failed: ") + musc_last_error(c)); };
  check(rc);
  *out = device_text("sam file on the device", n_targets + 2, hbytes, [&](uint64_t r0, uint64_t n, char* dst, uint64_t cap, uint64_t* nb) {
    check(musc_sam_text(c, 0, r0, n, dst, cap, 0, nb));
  });
  *out += device_text("sam file on the device", nrec, rbytes, [&](uint64_t r0, uint64_t n, char* dst, uint64_t cap, uint64_t* nb) {
    check(musc_sam_text(c, 1, r0, n, dst, cap, 0, nb));
  });
  musc_sam_last_ms(c, ms_prepare, ms_text);
  return true;
}

// The two coverage files (the bedGraph and the per-target summary) from the device (musc_cov_*), under the
// same conditions and with the same answers as sam_text_device.
inline bool coverage_text_device(musc_ctx* c, uint32_t flags, std::string* bed, std::string* summary, std::string* why, float* ms_prepare,
                                 float* ms_text) {
  uint64_t nruns = 0, rbytes = 0, nt = 0, sbytes = 0;
  const int rc = musc_cov_prepare(c, flags, &nruns, &rbytes, &nt, &sbytes);
  if (rc == 12 || rc == 10) return *why = "the device stage returned " + std::to_string(rc) + " (" + musc_last_error(c) + ")", false;
  auto check = [&](int r) { if (r) throw Die(1, std::string("coverage files on the device failed: ") + musc_last_error(c)); };
  check(rc);
  *bed = device_text("coverage files on the device", nruns, rbytes, [&](uint64_t r0, uint64_t n, char* dst, uint64_t cap, uint64_t* nb) {
    check(musc_cov_text(c, 0, r0, n, dst, cap, 0, nb));
  });
  *summary = device_text("coverage files on the device", nt, sbytes, [&](uint64_t r0, uint64_t n, char* dst, uint64_t cap, uint64_t* nb) {
    check(musc_cov_text(c, 1, r0, n, dst, cap, 0, nb));
  });
  musc_cov_last_ms(c, ms_prepare, ms_text);
  return true;
}

// ------------------------------------------------------------------------------------
// the pipeline (cmd/muscato/main.go:1005-1058), hot path through the C ABI
// ------------------------------------------------------------------------------------
inline void mkdir_p(const std::string& path) {
  std::string cur;
  for (size_t i = 0; i <= path.size(); i++) {
    if (i == path.size() || path[i] == '/') {
      if (!cur.empty() && mkdir(cur.c_str(), 0777) != 0 && errno != EEXIST)
        throw Die(1, "Directory " + cur + " does not exist and cannot be created.");
    }
    if (i < path.size()) cur += path[i];
  }
}

inline std::string join_path(const std::string& a, const std::string& b) {
  if (a.empty()) return b;
  return a.back() == '/' ? a + b : a + "/" + b;
}

inline std::string make_uid() {  // stands in for uuid.NewUUID (cmd/muscato/main.go:933)
  std::random_device rd;
  char b[40];
  snprintf(b, sizeof b, "%08x-%04x-%04x-%04x-%08x%04x", (unsigned)rd(), (unsigned)rd() & 0xFFFF, (unsigned)rd() & 0xFFFF,
           (unsigned)rd() & 0xFFFF, (unsigned)rd(), (unsigned)rd() & 0xFFFF);
  return b;
}

struct Logger {
  FILE* f = nullptr;
  void open(const std::string& path) { f = fopen(path.c_str(), "w"); }
  void printf(const char* fmt, ...) {
    if (!f) return;
    time_t t = time(nullptr);
    struct tm tmv;
    localtime_r(&t, &tmv);
    fprintf(f, "%02d:%02d:%02d ", tmv.tm_hour, tmv.tm_min, tmv.tm_sec);
    va_list ap;
    va_start(ap, fmt);
    vfprintf(f, fmt, ap);
    va_end(ap);
    fputc('\n', f);
    fflush(f);
  }
  ~Logger() { if (f) fclose(f); }
};

// wall time of the stages of a run, written to muscato.log (where the time goes end to end)
struct StageClock {
  Logger& log;
  double t0, last;
  static double now() {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec + 1e-9 * ts.tv_nsec;
  }
  explicit StageClock(Logger& l) : log(l), t0(now()), last(t0) {}
  void skip() { last = now(); }  // the time since the last lap belongs to no lap
  void lap(const char* what) {
    const double t = now();
    log.printf("stage %-28s %8.3f s (total %.3f s)", what, t - last, t - t0);
    last = t;
  }
};

inline musc_params to_params(const Config& c) {
  musc_params p;
  memset(&p, 0, sizeof p);
  p.n_windows = (int)c.Windows.size();
  for (int i = 0; i < p.n_windows; i++) p.windows[i] = c.Windows[i];
  p.window_width = c.WindowWidth;
  p.pmatch = c.PMatch;
  p.min_dinuc = c.MinDinuc;
  p.max_read_length = c.MaxReadLength;
  p.max_matches = c.MaxMatches;
  p.match_mode = c.MatchMode == "first" ? 1 : 0;
  p.mmtol = c.MMTol;
  p.apply_mmtol = 1;
  p.max_mismatch_p1 = c.MaxMismatch >= 0 ? c.MaxMismatch + 1 : 0;
  p.n_shards = c.GPUs > 1 ? c.GPUs : 0;
  return p;
}

struct Concat {
  std::string buf;
  std::vector<uint64_t> off;
};

template <class It, class F>
inline Concat concat(It b, It e, F seq_of) {
  Concat c;
  c.off.push_back(0);
  for (It i = b; i != e; ++i) {
    c.buf += seq_of(*i);
    c.off.push_back(c.buf.size());
  }
  c.buf.append(16, '\0');
  return c;
}

// ------------------------------------------------------------------------------------
// read preparation: utils/fastq.go, cmd/muscato_prep_reads, `sort`, cmd/muscato_uniqify
// ------------------------------------------------------------------------------------

// utils/fastq.go + cmd/muscato_prep_reads on the host (parse, MinReadLength on the raw length,
// subx, MaxReadLength, the 1000-character name rule); the `sort` of the `seq\tname` lines and
// cmd/muscato_uniqify/main.go:83-135 through musc_reads_sort_unique: the device orders the
// sequences bytewise and groups the identical ones, the host orders each group's names
// (= comparing the whole `seq\tname` line) and joins them (cli_names.hpp).
inline std::vector<UniqueRead> prep_reads(const std::string& fastq, const Config& c, size_t* n_total) {
  std::vector<std::string> seqs, names;
  {  // utils/fastq.go:35-61: records of four lines, name = whole first line, an incomplete last one is dropped
    std::string_view rec[4];
    int k = 0;
    for_each_line(fastq, [&](std::string_view line) {
      rec[k++] = line;
      if (k < 4) return;
      k = 0;
      if ((int)rec[1].size() < c.MinReadLength) return;
      std::string seq(rec[1]);
      subx(seq);
      if ((int)seq.size() > c.MaxReadLength) seq.resize(c.MaxReadLength);
      seqs.push_back(std::move(seq));
      names.push_back(clip_name(std::string(rec[0])));
    });
  }
  if (n_total) *n_total = seqs.size();
  std::vector<UniqueRead> out;
  if (seqs.empty()) return out;
  const Concat rd = concat(seqs.begin(), seqs.end(), [](const std::string& s) -> const std::string& { return s; });
  LibU32 order, ustart;
  uint64_t nu = 0;
  {  // (the context goes before the host makes its strings)
    Ctx ctx = Ctx::init(c.Device);
    if (!ctx) throw Die(1, std::string("read prep: ") + musc_last_error(nullptr));
    uint32_t *o = nullptr, *u = nullptr;
    const int rc = musc_reads_sort_unique(ctx.get(), rd.buf.data(), rd.off.data(), seqs.size(), 0, &o, &u, &nu);
    order.reset(o);
    ustart.reset(u);
    if (rc) throw Die(1, std::string("read prep: ") + musc_last_error(ctx.get()));
  }
  out.reserve(nu);
  std::vector<std::string> grp;
  for (uint64_t g = 0; g < nu; g++) {
    grp.clear();
    for (uint32_t k = ustart[g]; k < ustart[g + 1]; k++) grp.push_back(std::move(names[order[k]]));  // (a read is in one group)
    std::string na = join_group_names(grp.data(), grp.data() + grp.size());
    out.push_back(UniqueRead{seqs[order[ustart[g]]], grp.size(), std::move(na)});
  }
  return out;
}

// The names of the reads from the device too (MUSC_PREP_NAMES): musc_reads_prep_fastq_names has ordered,
// cut and joined them and rendered the lines seq\tcount\tnames\n, which are reads_sorted.txt byte for byte.  They come
// down in chunks of records and each line is cut into the three fields of a UniqueRead: no string is made per read of
// the file.  *line_text keeps the bytes for reads_sorted.txt.sz.
inline void reads_from_lines(musc_ctx* c, const musc_fastq_prep& fp, const musc_read_names& info, std::vector<UniqueRead>* out,
                             std::string* line_text) {
  const uint64_t chunk_records = 1ull << 20;
  line_text->resize(info.line_bytes);
  uint64_t pos = 0;
  for (uint64_t r0 = 0; r0 < fp.n_unique; r0 += chunk_records) {
    uint64_t nb = 0;
    if (musc_reads_names_text(c, 1, r0, chunk_records, &(*line_text)[0] + pos, info.line_bytes - pos, 0, &nb))
      throw Die(1, std::string("read prep: ") + musc_last_error(c));
    pos += nb;
  }
  if (pos != info.line_bytes) throw Die(1, "read prep: the line text of the device has " + std::to_string(pos) + " bytes, " + std::to_string(info.line_bytes) + " were announced");
  out->clear();
  out->reserve(fp.n_unique);
  const char* p = line_text->data();
  const char* const end = p + line_text->size();
  for (uint64_t g = 0; g < fp.n_unique; g++) {  // seq \t count \t names \n: the join holds no tab and no line end
    const char* t1 = (const char*)memchr(p, '\t', (size_t)(end - p));
    const char* t2 = t1 ? (const char*)memchr(t1 + 1, '\t', (size_t)(end - t1 - 1)) : nullptr;
    const char* nl = t2 ? (const char*)memchr(t2 + 1, '\n', (size_t)(end - t2 - 1)) : nullptr;
    if (!nl) throw Die(1, "read prep: line " + std::to_string(g) + " of the device's line text is incomplete");
    size_t count = 0;
    for (const char* q = t1 + 1; q < t2; q++) count = count * 10 + (size_t)(*q - '0');
    out->push_back(UniqueRead{std::string(p, t1), count, std::string(t2 + 1, nl)});
    p = nl + 1;
  }
  if (p != end) throw Die(1, "read prep: the device's line text holds more than its " + std::to_string(fp.n_unique) + " lines");
}

// The same with the parse on the device (musc_reads_prep_fastq: records, the \r rule, MinReadLength, subx,
// MaxReadLength, sort and collapse); the host makes strings of the group heads' sequences and of the names only, and
// keeps the name rules (cli_names.hpp) -- unless the plan puts the names on the device as well (reads_from_lines).
// false: the device had no memory for the stage, the log says so and the host path is to run.
inline bool prep_reads_device(const std::string& fastq, const Config& c, Placement& plan, size_t* n_total, Logger& log,
                              std::vector<UniqueRead>* out, std::string* line_text) {
  FastqPrep prep;
  musc_fastq_prep& fp = prep.fp;
  musc_stats st;
  bool names_done = false;
  {  // (the context goes before the host makes its strings, and before the host path runs in its place)
    Ctx ctx = Ctx::init(c.Device);
    if (!ctx) throw Die(1, std::string("read prep: ") + musc_last_error(nullptr));
    auto no_memory = [&](int rc, const std::string& e) {  // any other failure ends the run
      if (rc != 10 || e.find("out of memory") == std::string::npos) throw Die(1, "read prep: " + e);
    };
    if (plan.prep_names == Where::Device) {
      musc_read_names info{};
      const int rc = musc_reads_prep_fastq_names(ctx.get(), fastq.data(), fastq.size(), 0, c.MinReadLength, c.MaxReadLength, &fp, &info);
      if (rc) {
        const std::string e = musc_last_error(ctx.get());
        no_memory(rc, e);
        log.printf("read names on the host: the device stage found no memory (%s)", e.c_str());
        plan.demote(Demotion::PrepNamesNoMemory);
      } else {
        const LibU32 ranked(info.ranked);
        musc_get_stats(ctx.get(), &st);
        log.printf("read prep on the device: %llu records, %llu kept, %llu distinct, %.3f ms", (unsigned long long)fp.n_records,
                   (unsigned long long)fp.n_reads, (unsigned long long)fp.n_unique, st.ms_read_prep);
        log.printf("read names on the device: %llu groups of one, %llu counted, %llu sorted (%llu pairs, %u key passes), %llu bytes of lines, %.3f ms",
                   (unsigned long long)info.n_single, (unsigned long long)info.n_counted, (unsigned long long)info.n_sorted,
                   (unsigned long long)info.n_pairs, info.key_passes, (unsigned long long)info.line_bytes, info.ms_names);
        reads_from_lines(ctx.get(), fp, info, out, line_text);
        names_done = true;
      }
    }
    if (!names_done) {
      const int rc = musc_reads_prep_fastq(ctx.get(), fastq.data(), fastq.size(), 0, c.MinReadLength, c.MaxReadLength, &fp);
      if (rc) {
        const std::string e = musc_last_error(ctx.get());
        no_memory(rc, e);
        ctx.reset();
        log.printf("read prep on the host: the device stage found no memory (%s)", e.c_str());
        return false;
      }
      musc_get_stats(ctx.get(), &st);
    }
  }
  if (n_total) *n_total = fp.n_reads;
  if (names_done) return true;
  log.printf("read prep on the device: %llu records, %llu kept, %llu distinct, %.3f ms", (unsigned long long)fp.n_records,
             (unsigned long long)fp.n_reads, (unsigned long long)fp.n_unique, st.ms_read_prep);
  out->clear();
  out->reserve(fp.n_unique);
  std::vector<std::string> grp;
  for (uint64_t g = 0; g < fp.n_unique; g++) {
    grp.clear();
    for (uint32_t k = fp.ustart[g]; k < fp.ustart[g + 1]; k++) {
      const uint32_t r = fp.order[k];
      grp.push_back(clip_name(fastq.substr(fp.name_off[r], fp.name_len[r])));
    }
    std::string na = join_group_names(grp.data(), grp.data() + grp.size());
    const uint32_t h = fp.order[fp.ustart[g]];
    std::string seq = fastq.substr(fp.seq_off[h], fp.seq_len[h]);
    subx(seq);
    out->push_back(UniqueRead{std::move(seq), grp.size(), std::move(na)});
  }
  return true;
}

// ------------------------------------------------------------------------------------
// the hot path: load the targets, shard the unique reads over cfg.GPUs devices (one host thread + one
// musc_ctx per device, as the ABI's threading rule asks), match, gather, and replay MaxMatches where it was reached
// ------------------------------------------------------------------------------------
struct HotResult {
  std::vector<musc_hit> hits;   // matches.txt: the per-read best + MMTol selection
  Ctx ctx;                      // context 0, with the database and every read, when results.txt is ordered on the device
  bool list_on_device = false;  // `hits` is the list the last pass left in ctx (Placement::list_on_device)
  uint64_t res_lines = 0;       // lines of results.txt, when it was ordered on the device
  musc_stats st{};              // of the first GPU
};

inline Die hot_path_failed(const std::string& err) { return Die(1, "muscato hot path failed:\n" + err); }

struct Shards {
  std::vector<Ctx> ctx;        // one per GPU
  std::vector<uint64_t> base;  // the first read of each
};

// The gene file and the id file.  The targets as strings are host data that only host stages need (results_text and
// the MaxMatches replay on the host): targets() makes them on first use, with the host chain (decode_maybe_sz,
// split_lines, the cut at the first tab).  When the gene file went through the device (MUSC_TARGETS), ctx0
// is GPU 0's context with the database loaded and gene_raw the file's bytes, which the other GPUs load themselves.
struct TargetFiles {
  size_t n_targets = 0;                     // gene number = line index
  std::map<uint64_t, std::string> id_rest;  // gene number -> "name\tlen"
  std::string gene_path;
  mutable std::string gene_raw;  // (given up to the host chain unless the GPUs still load it)
  bool on_device = false;        // the database comes from musc_db_load_text of gene_raw
  Ctx ctx0;
  const std::vector<std::string>& targets() const {
    if (!have_strings) {
      const std::string text = on_device ? decode_maybe_sz(gene_raw, gene_path) : decode_maybe_sz(std::move(gene_raw), gene_path);
      for (auto& l : split_lines(text)) strings.push_back(l.substr(0, l.find('\t')));
      have_strings = true;
    }
    return strings;
  }
  int gene_framed() const { return ends_with(to_lower(gene_path), ".sz") ? 1 : -1; }  // as decode_maybe_sz decides

 private:
  mutable std::vector<std::string> strings;
  mutable bool have_strings = false;
};

inline Shards match_shards(const Config& cfg, const musc_params& P, const std::vector<UniqueRead>& reads, TargetFiles& tf) {
  const int G = cfg.GPUs;
  Concat db;
  if (!tf.on_device) {
    const std::vector<std::string>& targets = tf.targets();
    db = concat(targets.begin(), targets.end(), [](const std::string& s) -> const std::string& { return s; });
    if (targets.size() >= 0xFFFFFFFFull) throw Die(1, "too many targets");
  }
  Shards sh;
  sh.ctx.resize(G);
  if (tf.on_device) sh.ctx[0] = std::move(tf.ctx0);
  sh.base.assign(G, 0);
  std::vector<std::string> errs(G);
  std::vector<std::thread> th;
  for (int g = 0; g < G; g++) {
    const size_t lo = reads.size() * (size_t)g / G, hi = reads.size() * (size_t)(g + 1) / G;
    sh.base[g] = lo;
    th.emplace_back([&, g, lo, hi] {
      const bool loaded = sh.ctx[g] != nullptr;  // GPU 0's context came with the database (stage_target_files)
      if (!loaded) sh.ctx[g] = Ctx::init(cfg.Device + g);
      musc_ctx* c = sh.ctx[g].get();
      if (!c) { errs[g] = musc_last_error(nullptr); return; }
      if (!loaded) musc_db_set_partition_bases(c, (uint64_t)cfg.DbPartitionBases);  // (the MaxMatches replay reuses the first context)
      const Concat rd = concat(reads.begin() + lo, reads.begin() + hi, [](const UniqueRead& u) -> const std::string& { return u.seq; });
      uint64_t n = 0;
      const int db_rc = loaded ? 0
                        : tf.on_device ? musc_db_load_text(c, (const uint8_t*)tf.gene_raw.data(), tf.gene_raw.size(), 0, tf.gene_framed(), nullptr)
                                       : musc_db_load_ascii(c, db.buf.data(), db.off.data(), (uint32_t)tf.n_targets, 0);
      if (db_rc || musc_reads_load_ascii(c, rd.buf.data(), rd.off.data(), hi - lo, 0) || musc_match_device(c, &P, &n))
        errs[g] = musc_last_error(c);
    });
  }
  for (auto& t : th) t.join();
  std::string err;
  for (int g = 0; g < G; g++) if (!errs[g].empty()) err += "GPU " + std::to_string(cfg.Device + g) + ": " + errs[g] + "\n";
  if (!err.empty()) throw hot_path_failed(err);
  return sh;
}

// Every GPU copies its tuples to the host (musc_gather).  MUSC_GATHER=rccl (opt-in until it has run
// on a multi-GPU node) makes the shards' tuples meet on the first GPU over RCCL/xGMI and leave it
// in one copy; whatever goes wrong there, the host path takes over.  Returns the error text, empty when all is well
// (the per-GPU report is still due after a failure).
inline std::string gather_hits(const Config& cfg, const Shards& sh, Placement& plan, Logger& log, std::vector<musc_hit>* out) {
  std::vector<musc_ctx*> ctxs;
  for (auto& c : sh.ctx) ctxs.push_back(c.get());
  const int G = (int)ctxs.size();
  musc_hit* h = nullptr;
  uint64_t n = 0;
  int grc = 0;
  if (plan.gather_rccl) {
    grc = musc_gather_rccl(ctxs.data(), G, sh.base.data(), &h, &n);
    if (grc) {
      log.printf("RCCL gather failed (%d: %s): gathering through the host", grc, musc_last_error(ctxs[0]));
      plan.demote(Demotion::GatherFailed);
    } else {
      log.printf("tuples of %d GPUs gathered on GPU %d over RCCL", G, cfg.Device);
    }
  }
  if (!plan.gather_rccl) grc = musc_gather(ctxs.data(), G, sh.base.data(), &h, &n);
  const LibHits own(h);
  if (grc) return musc_last_error(ctxs[0]);
  out->assign(h, h + n);
  return std::string();
}

// the partition plan of one context (several partitions: a database whose index does not fit, or -DbPartitionBases)
inline uint32_t log_partition_plan(musc_ctx* c, int gpu, Logger& log) {
  uint32_t nparts = 0;
  musc_db_partitions(c, nullptr, 0, &nparts);
  if (nparts > 1) {
    std::vector<uint32_t> first(nparts + 1);
    musc_db_partitions(c, first.data(), nparts + 1, &nparts);
    std::string plan;
    for (uint32_t p = 0; p < nparts; p++)
      plan += (p ? " " : "") + std::to_string(first[p]) + "-" + std::to_string(first[p + 1] - 1);
    log.printf("gpu %d: database in %u partitions (targets %s)", gpu, nparts, plan.c_str());
  }
  return nparts;
}

// per GPU: the partition plan, one object of muscato_gpu_profile.json and one log line
inline void report_gpus(const Config& cfg, const Shards& sh, Logger& log) {
  std::string prof = "[";
  for (int g = 0; g < (int)sh.ctx.size(); g++) {
    musc_stats s;
    musc_get_stats(sh.ctx[g].get(), &s);
    const uint32_t nparts = log_partition_plan(sh.ctx[g].get(), cfg.Device + g, log);
    char pb[1024];
    snprintf(pb, sizeof pb,
             "%s{\"gpu\":%d,\"partitions\":%u,\"index_kind\":%u,\"index_bytes\":%llu,\"reads\":%llu,\"read_windows\":%llu,\"index_entries_walked\":%llu,"
             "\"pairs_compared\":%llu,\"accepted\":%llu,\"tuples\":%llu,\"batches\":%u,\"ms_total\":%.4f,\"ms_screen_or_match\":%.4f,"
             "\"ms_confirm\":%.4f,\"ms_scan\":%.4f,\"ms_compact\":%.4f,\"ms_index_build\":%.3f,\"confirm_bytes\":%llu,\"match_bytes\":%llu}",
             g ? "," : "", cfg.Device + g, nparts, s.index_kind, (unsigned long long)s.index_bytes, (unsigned long long)s.n_reads,
             (unsigned long long)s.n_read_windows, (unsigned long long)s.n_candidates, (unsigned long long)s.n_pairs,
             (unsigned long long)s.n_accepted, (unsigned long long)s.n_hits, s.n_batches, s.ms_total, s.ms_screen, s.ms_confirm,
             s.ms_scan, s.ms_select, s.ms_index_build, (unsigned long long)s.confirm_bytes, (unsigned long long)s.match_bytes);
    prof += pb;
    log.printf("gpu %d: reads %llu windows %llu candidates %llu pairs %llu accepted %llu hits %llu; device %.3f ms "
               "(screen %.3f scan %.3f confirm %.3f select %.3f), index build %.1f ms, confirm %.1f GB/s",
               cfg.Device + g, (unsigned long long)s.n_reads, (unsigned long long)s.n_read_windows,
               (unsigned long long)s.n_candidates, (unsigned long long)s.n_pairs, (unsigned long long)s.n_accepted,
               (unsigned long long)s.n_hits, s.ms_total, s.ms_screen, s.ms_scan, s.ms_confirm, s.ms_select,
               s.ms_index_build, s.ms_confirm > 0 ? s.confirm_bytes / 1e6 / s.ms_confirm : 0.0);
  }
  // --CPUProfile (cmd/muscato_screen/main.go:530-538 writes a pprof CPU profile of the screen to
  // LogDir): here the hot path runs on the GPU, so the profile is the per-kernel device timing
  if (cfg.CPUProfile) spit(join_path(cfg.LogDir, "muscato_gpu_profile.json"), prof + "]\n");
}

// may some (window, key) block of some shard exceed MaxMatches
inline bool any_overflow(const Shards& sh) {
  bool overflow = false;
  for (auto& c : sh.ctx) {
    musc_stats s;
    musc_get_stats(c.get(), &s);
    overflow = overflow || (s.n_overflow_blocks != 0 && s.n_overflow_blocks != ~0ull);
  }
  return overflow;
}

// What both replays start from: the pass redone on one GPU with every read and every accepted tuple kept (with one GPU
// the reload repeats a load the context already has).
struct ReplayPass {
  uint64_t n;              // accepted tuples, resident
  double t_load, t_replay; // before the reload, after the pass
};

inline ReplayPass replay_pass(musc_ctx* c, const musc_params& P, const std::vector<UniqueRead>& reads, Placement& plan) {
  musc_params P1 = P;
  P1.apply_mmtol = 0;
  P1.n_shards = 0;
  const Concat rd = concat(reads.begin(), reads.end(), [](const UniqueRead& u) -> const std::string& { return u.seq; });
  ReplayPass rp = {0, StageClock::now(), 0};
  if (musc_reads_load_ascii(c, rd.buf.data(), rd.off.data(), reads.size(), 0) || musc_match_device(c, &P1, &rp.n)) {
    plan.demote(Demotion::ReplayPassFailed);  // (no replay ran anywhere: the run ends here)
    throw hot_path_failed(musc_last_error(c));
  }
  rp.t_replay = StageClock::now();
  return rp;
}

// The truncation on the device (musc_maxmatches_apply), which leaves the selection resident, so that
// results.txt and the side outputs still come from the device.  A refusal (12) and a failed allocation (10) hand the
// replay to the host through the plan.
inline void replay_on_device(musc_ctx* c, const ReplayPass& rp, Placement& plan, Logger& log, std::vector<musc_hit>* out) {
  uint64_t nh = 0, np = 0, ntrunc = 0;
  const int rc = musc_maxmatches_apply(c, 1, &nh, &np, &ntrunc);
  if (rc == 12 || rc == 10) {
    log.printf("MaxMatches replay on the host: the device stage returned %d (%s)", rc, musc_last_error(c));
    plan.demote(Demotion::ReplayRefused);
    return;
  }
  if (rc) throw hot_path_failed(musc_last_error(c));
  out->resize(nh);
  std::string err;
  if (musc_hits_copy(c, out->data(), nh, 0)) err = musc_last_error(c);
  float ms = 0, ms_replay = 0;
  uint64_t npairs = 0;
  musc_maxmatches_last_ms(c, &ms);
  musc_maxmatches_last_detail(c, &npairs, &ms_replay);
  log.printf("MaxMatches: %llu suspect probes, %llu blocks truncated as the reference does", (unsigned long long)np,
             (unsigned long long)ntrunc);
  log.printf("MaxMatches replay on the device: %.3f s (device %.3f ms, k_mm_replay %.3f ms, %llu pairs in the truncated blocks), "
             "%llu tuples; the pass before it %.3f s",
             StageClock::now() - rp.t_replay, ms, ms_replay, (unsigned long long)npairs, (unsigned long long)nh, rp.t_replay - rp.t_load);
  if (!err.empty()) throw hot_path_failed(err);
}

// The truncation on the host (apply_maxmatches) from every accepted tuple and the suspect probes; its selection
// exists on the host only.
inline void replay_on_host(musc_ctx* c, const ReplayPass& rp, const Config& cfg, const std::vector<UniqueRead>& reads,
                           const std::vector<std::string>& targets, Logger& log, std::vector<musc_hit>* out) {
  std::vector<musc_hit> all(rp.n);
  uint64_t np = 0;
  uint32_t *pr = nullptr, *pw = nullptr;
  const bool failed = musc_hits_copy(c, all.data(), rp.n, 0) || musc_overflow_probes(c, &pr, &pw, &np);
  const LibU32 own_r(pr), own_w(pw);
  if (failed) throw hot_path_failed(musc_last_error(c));
  size_t ntrunc = 0;
  all = apply_maxmatches(cfg, reads, targets, std::move(all), pr, pw, np, &ntrunc);
  *out = best_filter(all, reads.size(), cfg.MMTol);
  log.printf("MaxMatches: %llu suspect probes, %zu blocks truncated as the reference does", (unsigned long long)np, ntrunc);
  log.printf("MaxMatches replay on the host: %.3f s, %zu tuples; the pass before it %.3f s", StageClock::now() - rp.t_replay,
             out->size(), rp.t_replay - rp.t_load);
}

inline HotResult run_hot_path(const Config& cfg, const std::vector<UniqueRead>& reads, TargetFiles& tf, Placement& plan, Logger& log) {
  const musc_params P = to_params(cfg);
  Shards sh = match_shards(cfg, P, reads, tf);
  HotResult r;
  const std::string gather_err = gather_hits(cfg, sh, plan, log, &r.hits);
  musc_get_stats(sh.ctx[0].get(), &r.st);
  report_gpus(cfg, sh, log);
  if (!gather_err.empty()) throw hot_path_failed(gather_err);
  const bool overflow = any_overflow(sh);
  sh.ctx.resize(1);  // the other GPUs' contexts go before the replay
  if (overflow) {
    // Some (window,key) block may exceed MaxMatches: redo the pass on one GPU with every read,
    // take all accepted tuples and replay the reference's truncation.
    fputs("MaxMatches reached in at least one window-key block: replaying the reference's truncation...\n", stderr);
    if (plan.note_replay_gpus) log.printf("MaxMatches replay on the host: the post-chain of %d GPUs runs on the host", cfg.GPUs);
    musc_ctx* c = sh.ctx[0].get();
    const ReplayPass rp = replay_pass(c, P, reads, plan);
    if (plan.maxmatches == Where::Device) replay_on_device(c, rp, plan, log, &r.hits);
    if (plan.maxmatches == Where::Host) replay_on_host(c, rp, cfg, reads, tf.targets(), log, &r.hits);
    r.st.n_overflow_blocks = 0;  // handled exactly
  }
  r.list_on_device = plan.list_on_device(overflow);
  if (plan.results == Where::Device) r.ctx = std::move(sh.ctx[0]);
  return r;
}

// ------------------------------------------------------------------------------------
// the pipeline (cmd/muscato/main.go:1005-1058) as its stages, in the order run_muscato calls them
// ------------------------------------------------------------------------------------

// the nine values the plan is made from: the only place the host tools read the environment
inline PlanEnv plan_env_of_process() {
  return PlanEnv{getenv("MUSC_PREP"), getenv("MUSC_MAXMATCHES"), getenv("MUSC_RESULTS"), getenv("MUSC_SIDE"), getenv("MUSC_GATHER"),
                 getenv("MUSC_TARGETS"), getenv("MUSC_PREP_NAMES"), getenv("MUSC_SAM"), getenv("MUSC_COVERAGE")};
}

// setupEnvs/makeTemp/setupLog/saveConfig (cmd/muscato/main.go:906-967, 680-706)
inline void setup_run(Config& cfg, Logger& log) {
  const std::string uid = make_uid();
  cfg.TempDir = join_path(cfg.TempDir.empty() ? "muscato_tmp" : cfg.TempDir, uid);
  mkdir_p(cfg.TempDir);
  cfg.LogDir = join_path(cfg.LogDir.empty() ? "muscato_logs" : cfg.LogDir, uid);
  mkdir_p(cfg.LogDir);
  log.open(join_path(cfg.LogDir, "muscato.log"));
  spit(join_path(cfg.LogDir, "config.json"), config_to_json(cfg));
}

// cleanTmp is deferred in the reference (cmd/muscato/main.go:969-979, 1019): the temporary
// directory goes away on every exit path, also when a stage fails, unless NoCleanTemp is set
struct TmpGuard {
  const Config& c;
  ~TmpGuard() {
    if (c.NoCleanTemp) return;
    unlink(join_path(c.TempDir, "reads_sorted.txt.sz").c_str());
    rmdir(c.TempDir.c_str());
  }
};

inline std::vector<UniqueRead> stage_read_prep(const Config& cfg, Placement& plan, Logger& log) {
  fputs("Preparing reads...\n", stderr);
  size_t n_total = 0;
  std::vector<UniqueRead> reads;
  std::string line_text;  // reads_sorted.txt as the device rendered it, when the names were made there
  {
    const std::string fastq = slurp(cfg.ReadFileName);
    if (plan.prep == Where::Device && !prep_reads_device(fastq, cfg, plan, &n_total, log, &reads, &line_text)) plan.demote(Demotion::PrepNoMemory);
    if (plan.prep == Where::Host) reads = prep_reads(fastq, cfg, &n_total);
  }
  if (reads.empty()) throw Die(1, "muscato_uniqify: no input from -");
  fprintf(stderr, "Found %zu total sequences\nFound %zu unique sequences\n", n_total, reads.size());
  spit(join_path(cfg.LogDir, "seqinfo.json"),
       "{\"NumUnique\":" + std::to_string(reads.size()) + ",\"NumTotal\":" + std::to_string(n_total) + "}\n");
  if (cfg.NoCleanTemp) {  // keep the one intermediate other tools consume
    std::string t;
    if (plan.prep_names == Where::Device) t.swap(line_text);  // (the same bytes, framed as they came)
    else
      for (auto& u : reads) t += u.seq + "\t" + std::to_string(u.count) + "\t" + u.names + "\n";
    spit(join_path(cfg.TempDir, "reads_sorted.txt.sz"), sz_write(t));
  }
  return reads;
}

inline void stage_window_check(const Config& cfg, const std::vector<UniqueRead>& reads, Logger& log) {
  fputs("Windowing reads...\n", stderr);
  for (size_t k = 0; k < cfg.Windows.size(); k++) {  // cmd/muscato_window_reads/main.go:143-151
    size_t nvalid = 0;
    for (auto& u : reads) nvalid += (int)u.seq.size() >= cfg.Windows[k] + cfg.WindowWidth;
    log.printf("Window %zu produced %zu valid reads", k, nvalid);
    if (nvalid == 0) throw Die(1, "Window " + std::to_string(k) + " produced no valid reads, exiting");
  }
}

// The gene file on the device (MUSC_TARGETS): GPU 0's context is made here and musc_db_load_text takes the
// file's bytes to the resident database; the census of odd bytes comes back with it.  False when the stage left the
// device -- no memory (10), a chunk beyond the format's 65 536 bytes (12), a bad stream (13) -- and the host chain is
// to run in its place: a corrupt file then ends the run with the host decoder's own message.
inline bool load_targets_device(const Config& cfg, TargetFiles& tf, Placement& plan, Logger& log, size_t* nodd, size_t* first_t) {
  Ctx ctx = Ctx::init(cfg.Device);
  if (!ctx) throw hot_path_failed("GPU " + std::to_string(cfg.Device) + ": " + musc_last_error(nullptr) + "\n");
  musc_db_set_partition_bases(ctx.get(), (uint64_t)cfg.DbPartitionBases);
  musc_db_text_info info;
  const int rc = musc_db_load_text(ctx.get(), (const uint8_t*)tf.gene_raw.data(), tf.gene_raw.size(), 0, tf.gene_framed(), &info);
  if (rc) {
    const std::string e = musc_last_error(ctx.get());
    if (rc == 12) plan.demote(Demotion::TargetsRefused);
    else if (rc == 13) plan.demote(Demotion::TargetsBadStream);
    else if (rc == 10 && e.find("out of memory") != std::string::npos) plan.demote(Demotion::TargetsNoMemory);
    else throw hot_path_failed("GPU " + std::to_string(cfg.Device) + ": " + e + "\n");
    log.printf("targets on the host: the device stage returned %d (%s)", rc, e.c_str());
    return false;
  }
  log.printf("targets on the device: %llu targets, %llu bases, %llu bytes of text in %llu chunks, decode %.3f ms, parse %.3f ms",
             (unsigned long long)info.n_targets, (unsigned long long)info.n_bases, (unsigned long long)info.n_text_bytes,
             (unsigned long long)info.n_chunks, info.ms_decode, info.ms_parse);
  tf.n_targets = info.n_targets;
  tf.on_device = true;
  tf.ctx0 = std::move(ctx);
  *nodd = info.n_odd;
  *first_t = info.first_odd_target;
  return true;
}

// gene file: sequence = text before the first tab, gene number = line index
// (cmd/muscato_screen/main.go:439-452); id file: "%011d\tname\tlen" (join field 1)
inline TargetFiles stage_target_files(const Config& cfg, Placement& plan, Logger& log) {
  TargetFiles tf;
  tf.gene_path = cfg.GeneFileName;
  tf.gene_raw = slurp(cfg.GeneFileName);
  size_t nodd = 0, first_t = 0;  // target bytes that are none of ACGTX
  if (plan.targets == Where::Device) load_targets_device(cfg, tf, plan, log, &nodd, &first_t);
  if (plan.targets == Where::Host) {
    const std::vector<std::string>& targets = tf.targets();
    tf.n_targets = targets.size();
    for (size_t t = 0; t < targets.size(); t++)
      for (unsigned char ch : targets[t])
        if (ch != 'A' && ch != 'C' && ch != 'G' && ch != 'T' && ch != 'X' && nodd++ == 0) first_t = t;
  }
  // Targets are compared as 2-bit bases + an "X" plane: every byte that is not A, C, G or T is an
  // X here.  muscato_prep_targets writes nothing else (it leaves the LAST FASTA record un-substituted,
  // cmd/muscato_prep_targets/main.go:204-212), but a hand-made gene file may: the reference then
  // compares the raw byte, so an 'N' in a target would mismatch an 'X' in a read where this tool
  // counts a match.  Say so instead of differing silently.
  if (nodd) {
    fprintf(stderr, "Warning: %zu target bytes are none of ACGTX (first in target %zu); they are treated as X\n", nodd, first_t);
    log.printf("%zu target bytes are none of ACGTX (first in target %zu): treated as X; the reference compares them "
               "literally, so they would mismatch an X of a read there", nodd, first_t);
    // The device renders and orders targetsub from the 2-bit planes, where every byte that is none of ACGT is an X;
    // results.txt quotes the target's own bytes.  Such a gene file keeps the host path, whatever MUSC_RESULTS says:
    // the bytes are the same on every path.
    plan.demote(Demotion::OddTargetBytes);
  }
  for (auto& l : split_lines(read_maybe_sz(cfg.GeneIdFileName))) {
    size_t t = l.find('\t');
    if (t == std::string::npos) continue;
    tf.id_rest.emplace(strtoull(l.substr(0, t).c_str(), nullptr, 10), l.substr(t + 1));
  }
  return tf;
}

inline HotResult stage_hot_path(const Config& cfg, const std::vector<UniqueRead>& reads, TargetFiles& tf, Placement& plan,
                                Logger& log) {
  fputs("Screening...\nConfirming...\n", stderr);
  if (plan.note_odd_targets)
    log.printf("results on the host: the targets hold bytes that are none of ACGTX, which the device would render as X");
  HotResult hot = run_hot_path(cfg, reads, tf, plan, log);
  if (hot.st.n_overflow_blocks)
    fprintf(stderr, "Warning: %llu window-key blocks may exceed MaxMatches; results keep all their matches\n",
            (unsigned long long)hot.st.n_overflow_blocks);
  return hot;
}

// results.txt, ordered and rendered where the plan says (MUSC_RESULTS).  Context 0 goes here unless the
// side outputs, the SAM file or the coverage files are to come from it.  With a SAM file or coverage files for the host
// to write, *ordered gets the tuples of the lines in line order -- from the host's own sort, or from the device's
// ordered list.
inline std::string stage_results(const Config& cfg, const Placement& plan, HotResult& hot, const std::vector<UniqueRead>& reads,
                                 const TargetFiles& tf, Logger& log, std::vector<musc_hit>* ordered) {
  fputs("Combining windows...\nJoining gene names...\nJoining read names...\n", stderr);
  const bool sam = !cfg.SamFileName.empty(), cov = !cfg.CoverageFileName.empty();
  std::string res;
  if (plan.results == Where::Device) {
    float ms_order = 0, ms_text = 0;
    uint64_t nlines = 0;
    res = results_text_device(hot.ctx.get(), hot.list_on_device, hot.hits, reads, tf.n_targets, tf.id_rest, &ms_order, &ms_text, &nlines);
    log.printf("results on the device: %zu bytes, order %.3f ms, text %.3f ms", res.size(), ms_order, ms_text);
    hot.res_lines = nlines;
    const bool ctx_for_sam = sam && plan.sam_on_device(hot.list_on_device), ctx_for_cov = cov && plan.coverage_on_device(hot.list_on_device);
    if ((sam && !ctx_for_sam) || (cov && !ctx_for_cov)) {
      ordered->resize(nlines);
      if (musc_results_hits(hot.ctx.get(), ordered->data(), nlines, 0))
        throw Die(1, std::string("results on the device failed: ") + musc_last_error(hot.ctx.get()));
    }
    if (plan.side == Where::Host && !ctx_for_sam && !ctx_for_cov) hot.ctx.reset();
  } else if (sam || cov) {
    const std::vector<ResultsLine> lines = results_lines(hot.hits.data(), hot.hits.size(), reads, tf.targets(), tf.id_rest);
    res = results_text(lines, reads);
    ordered->reserve(lines.size());
    for (auto& l : lines) ordered->push_back(l.hit);
    log.printf("results on the host: %zu bytes", res.size());
  } else {
    res = results_text(hot.hits.data(), hot.hits.size(), reads, tf.targets(), tf.id_rest);
    log.printf("results on the host: %zu bytes", res.size());
  }
  spit(cfg.ResultsFileName, res);
  return res;
}

// The SAM file (-SamFileName, MUSC_SAM), written where results.txt was made: on the device when the plan
// says so and the list results.txt was ordered from is the one the pass left there, else by the host function over
// `ordered`.  A refusal of the device stage (12) or no memory (10) logs one line and the host function runs.
inline void stage_sam(const Config& cfg, Placement& plan, HotResult& hot, const std::vector<UniqueRead>& reads, const TargetFiles& tf,
                      std::vector<musc_hit>& ordered, Logger& log) {
  fputs("Writing SAM file...\n", stderr);
  const double t0 = StageClock::now();
  std::string sam, why;
  if (plan.sam_on_device(hot.list_on_device)) {
    float ms_prepare = 0, ms_text = 0;
    musc_ctx* c = hot.ctx.get();
    if (sam_text_device(c, cfg.SamRev, tf.n_targets, &sam, &why, &ms_prepare, &ms_text)) {
      log.printf("sam on the device: %zu bytes, prepare %.3f ms, text %.3f ms", sam.size(), ms_prepare, ms_text);
    } else {
      log.printf("sam on the host: %s", why.c_str());
      plan.demote(Demotion::SamRefused);
      ordered.resize(hot.res_lines);  // (a refused call leaves the ordered list as it was)
      if (musc_results_hits(c, ordered.data(), ordered.size(), 0)) throw Die(1, std::string("sam file: ") + musc_last_error(c));
    }
    if (plan.side == Where::Host && !(!cfg.CoverageFileName.empty() && plan.coverage_on_device(hot.list_on_device))) hot.ctx.reset();
  }
  const bool from_device = plan.sam_on_device(hot.list_on_device);
  if (!from_device && !sam_text(ordered.data(), ordered.size(), reads, tf.targets(), tf.id_rest, cfg.SamRev, &sam, &why))
    throw Die(1, "SamFileName: " + why + "\n");
  spit(cfg.SamFileName, sam);
  log.printf("sam file on the %s: %.3f s", from_device ? "device" : "host", StageClock::now() - t0);
}

inline std::string coverage_targets_name(const std::string& coverage) { return coverage + "_targets"; }

inline uint32_t coverage_flags(const Config& cfg) {
  return (cfg.CoverageRev ? MUSC_COV_REV_PAIRS : 0u) | (cfg.CoverageWeighted ? MUSC_COV_WEIGHTED : 0u) | (cfg.CoverageUnique ? MUSC_COV_UNIQUE : 0u);
}

// The coverage files (-CoverageFileName, MUSC_COVERAGE): the bedGraph to the name given and the summary to
// <name>_targets, made where results.txt was made, by the rule of stage_sam: on the device when the plan says so and
// the list is the one the pass left there, else by coverage_text over `ordered`.  A refusal of the device stage (12) or
// no memory (10) logs one line and the host function runs; it holds the same refusals and ends the run with the reason.
inline void stage_coverage(const Config& cfg, Placement& plan, HotResult& hot, const std::vector<UniqueRead>& reads, const TargetFiles& tf,
                           std::vector<musc_hit>& ordered, Logger& log) {
  fputs("Writing coverage files...\n", stderr);
  const double t0 = StageClock::now();
  const uint32_t flags = coverage_flags(cfg);
  std::string bed, summary, why;
  if (plan.coverage_on_device(hot.list_on_device)) {
    float ms_prepare = 0, ms_text = 0;
    musc_ctx* c = hot.ctx.get();
    if (coverage_text_device(c, flags, &bed, &summary, &why, &ms_prepare, &ms_text)) {
      log.printf("coverage on the device: %zu + %zu bytes, %llu events, prepare %.3f ms, text %.3f ms", bed.size(), summary.size(),
                 2ull * hot.res_lines, ms_prepare, ms_text);
    } else {
      log.printf("coverage on the host: %s", why.c_str());
      plan.demote(Demotion::CoverageRefused);
      ordered.resize(hot.res_lines);  // (a refused call leaves the ordered list as it was)
      if (musc_results_hits(c, ordered.data(), ordered.size(), 0)) throw Die(1, std::string("coverage files: ") + musc_last_error(c));
    }
    if (plan.side == Where::Host) hot.ctx.reset();
  }
  const bool from_device = plan.coverage_on_device(hot.list_on_device);
  if (!from_device && !coverage_text(ordered.data(), ordered.size(), reads, tf.targets(), tf.id_rest, flags, &bed, &summary, &why))
    throw Die(1, "CoverageFileName: " + why + "\n");
  spit(cfg.CoverageFileName, bed);
  spit(coverage_targets_name(cfg.CoverageFileName), summary);
  log.printf("coverage files on the %s: %.3f s", from_device ? "device" : "host", StageClock::now() - t0);
}

// The nonmatch FASTQ and the two stats files (MUSC_SIDE): from the device, which takes them from the
// ordered list behind results.txt and whose context goes once they are rendered, or from `res` on the host, one thread
// each.
inline void stage_side_outputs(const Config& cfg, Placement& plan, Ctx ctx, const std::string& res,
                               const std::vector<UniqueRead>& reads, Logger& log) {
  fputs("Writing non-matching sequences...\nGenerating read statistics...\nGenerating gene statistics...\n", stderr);
  std::string side[3];
  if (plan.side == Where::Device) {
    float ms_prepare = 0, ms_text = 0;
    if (side_texts_device(ctx.get(), side, &ms_prepare, &ms_text)) {
      log.printf("side outputs on the device: prepare %.3f ms, text %.3f ms", ms_prepare, ms_text);
    } else {
      log.printf("side outputs on the host: the gene text is not name\\tlen without blanks, which the device needs");
      plan.demote(Demotion::SideRefused);
    }
    ctx.reset();
  }
  const bool from_device = plan.side == Where::Device;
  std::string err_side[3];
  auto guarded = [&](int i, auto fn) {
    return std::thread([&, i, fn] {
      try { fn(); } catch (const std::exception& e) { err_side[i] = e.what(); } catch (...) { err_side[i] = "failed"; }
    });
  };
  std::thread t0 = guarded(0, [&] {
    spit(nonmatch_name(cfg.ResultsFileName), from_device ? side[MUSC_SIDE_NONMATCH] : nonmatch_text(res, reads));
  });
  std::thread t1 = guarded(1, [&] {
    spit(stats_name(cfg.ResultsFileName, "_readstats"), from_device ? side[MUSC_SIDE_READSTATS] : readstats_text(res));
  });
  std::thread t2 = guarded(2, [&] {
    spit(stats_name(cfg.ResultsFileName, "_genestats"), from_device ? side[MUSC_SIDE_GENESTATS] : genestats_text(res));
  });
  t0.join(); t1.join(); t2.join();
  for (auto& e : err_side) if (!e.empty()) throw Die(1, "side output: " + e);
}

inline int run_muscato(Config cfg) {
  Logger log;
  setup_run(cfg, log);
  TmpGuard tmp_guard{cfg};
  Placement plan = make_placement(plan_env_of_process(), cfg.GPUs);

  StageClock clk(log);
  const std::vector<UniqueRead> reads = stage_read_prep(cfg, plan, log);
  clk.lap("read prep");
  stage_window_check(cfg, reads, log);
  TargetFiles tf = stage_target_files(cfg, plan, log);
  clk.lap("windows check, target files");
  HotResult hot = stage_hot_path(cfg, reads, tf, plan, log);
  clk.lap("hot path (init, load, match)");
  std::vector<musc_hit> ordered;  // the tuples of results.txt in line order, kept only for a SAM file or coverage files the host writes
  const std::string res = stage_results(cfg, plan, hot, reads, tf, log, &ordered);
  clk.lap("results.txt");
  if (!cfg.SamFileName.empty()) {
    stage_sam(cfg, plan, hot, reads, tf, ordered, log);
    clk.skip();  // (the stage logs its own line)
  }
  if (!cfg.CoverageFileName.empty()) {
    stage_coverage(cfg, plan, hot, reads, tf, ordered, log);
    clk.skip();
  }
  stage_side_outputs(cfg, plan, std::move(hot.ctx), res, reads, log);
  clk.lap("nonmatch + stats files");
  return 0;
}

}  // namespace musc
