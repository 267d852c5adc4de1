// targets_prep_plan_check.cpp -- the arithmetic of target preparation on the device (csrc/targets_prep_plan.hpp) and the
// passes of kernels_targets_prep.hpp restated in plain C++, against prep_targets_text / prep_targets_fasta / sz_encode
// of the host chain (muscato_host.hpp, sz.hpp), as a program of its own so that it runs under the sanitizers.
// It needs no GPU and is not part of the library; muscato_amd/build.py (CHECKS) builds it, plain and sanitized.
//
// Over seeded texts (short ones over the bytes that matter, longer ones with records, CRLF, headers and stop lines),
// each copied to a heap block of exactly its size so that a read past either end is an error under the address
// sanitizer, in both formats and with both values of rev:
//   - the passes as the kernels make them -- the line tables (begin, end, first and last tab), the stop line as a
//     minimum, the header scan, the prefix sum S of the bases, the header lines, the groups, the kept records, and every
//     byte of both texts found from its place in the output by binary search (the record in the offsets, the line in
//     S) -- give the bytes the host chain gives, and refuse exactly when prep_targets_fasta throws, with the first
//     empty line's number;
//   - id_line_len / id_rec_len are the lengths of the host's id lines, seq_fwd_off / seq_rev_off the places of the
//     host's sequence lines, n_targets their count;
//   - sz_frame_size, sz_chunk_pos and sz_chunk_len describe sz_encode's output of both texts, byte for byte.
// The CRC: crc32c_combine over the slices of k_sz_frame (crc_slice_dwords: an odd number of dwords per lane) against
// crc32c of the whole chunk, for every chunk size around the sizes at which the slice grows, and the refusal bound.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "../sz_plan.hpp"
#include "../targets_prep_plan.hpp"
#include "check.hpp"
#include "muscato_host.hpp"

namespace {

namespace tp = musc_tp;

const musc_sz::X2n x2n;
const uint64_t NONE = ~0ull;

// the largest i in [0, n) with a[i] * mult <= v (tp_find)
uint64_t find(const std::vector<uint64_t>& a, uint64_t n, uint64_t mult, uint64_t v) {
  uint64_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (a[mid] * mult <= v) lo = mid; else hi = mid;
  }
  return lo;
}

std::vector<uint64_t> exclusive_scan(std::vector<uint64_t> v) {
  uint64_t s = 0;
  for (auto& x : v) {
    const uint64_t t = x;
    x = s;
    s += t;
  }
  return v;
}

struct Passes {
  bool refused = false;
  uint64_t empty_line = NONE, stop_line = NONE, n_lines = 0, n_records = 0, n_dropped = 0;
  std::string seqs, ids;
};

// the passes of musc_targets_prep on text[0, n), one statement per lane
Passes passes(const unsigned char* text, uint64_t n, bool fasta, bool rev) {
  Passes P;
  if (n == 0) return P;
  // k_fq_count / k_tp_lines
  uint64_t newlines = 0;
  for (uint64_t p = 0; p < n; p++) newlines += text[p] == '\n';
  const uint64_t nlines = newlines + (text[n - 1] != '\n');
  P.n_lines = nlines;
  std::vector<uint64_t> begin(nlines), eol(nlines), ftab(nlines, NONE), ltab(nlines, 0);
  begin[0] = 0;
  if (text[n - 1] != '\n') eol[nlines - 1] = n;
  for (uint64_t p = 0, k = 0; p < n; p++) {
    if (text[p] == '\t') ftab[k] = std::min(ftab[k], p), ltab[k] = std::max(ltab[k], p + 1);
    if (text[p] == '\n') {
      eol[k] = p;
      if (k + 1 < nlines) begin[k + 1] = p + 1;
      k++;
    }
  }
  // k_tp_classify
  std::vector<uint64_t> hdr(nlines + 1, 0), bases(nlines + 1, 0);
  for (uint64_t k = 0; k < nlines; k++) {
    if (eol[k] > begin[k] && text[eol[k] - 1] == '\r') eol[k]--;
    const uint64_t len = eol[k] - begin[k];
    if (fasta) {
      if (len == 0) P.empty_line = std::min(P.empty_line, k);
      const bool h = len && text[begin[k]] == '>';
      hdr[k] = h;
      bases[k] = h ? 0 : len;
    } else if (len == 0 || ftab[k] == NONE || ftab[k] + 1 != ltab[k]) {
      P.stop_line = std::min(P.stop_line, k);
    }
  }
  uint64_t nrec = 0, exempt = NONE;
  std::vector<uint64_t> fo, src0, name_b, name_len, S;
  if (!fasta) {  // k_tp_text_recs
    nrec = std::min(P.stop_line, nlines);
    std::vector<uint64_t> a(nrec + 1, 0);
    src0.resize(nrec), name_b.resize(nrec), name_len.resize(nrec);
    for (uint64_t k = 0; k < nrec; k++) {
      a[k] = eol[k] - ftab[k];
      src0[k] = ftab[k] + 1;
      name_b[k] = begin[k];
      name_len[k] = ftab[k] - begin[k];
    }
    fo = exclusive_scan(a);
  } else {
    if (P.empty_line != NONE) {
      P.refused = true;
      return P;
    }
    const std::vector<uint64_t> hs = exclusive_scan(hdr);
    S = exclusive_scan(bases);
    const uint64_t nhdr = hs[nlines], ngroups = nhdr + 1;
    std::vector<uint64_t> hl(ngroups + 1, NONE);  // k_tp_hl
    hl[0] = 0, hl[ngroups] = nlines;
    for (uint64_t k = 0; k < nlines; k++)
      if (hs[k + 1] != hs[k]) hl[hs[k] + 1] = k;
    std::vector<uint64_t> kept(ngroups + 1, 0), a(ngroups + 1, 0);  // k_tp_groups
    for (uint64_t g = 0; g < ngroups; g++) {
      const uint64_t len = S[hl[g + 1]] - S[hl[g]];
      kept[g] = len != 0;
      a[g] = len ? len + 1 : 0;
    }
    const std::vector<uint64_t> kidx = exclusive_scan(kept), fg = exclusive_scan(a);
    nrec = kidx[ngroups];
    fo.assign(nrec + 1, 0), src0.resize(nrec), name_b.resize(nrec), name_len.resize(nrec);
    uint64_t kept0 = 0;
    for (uint64_t g = 0; g <= ngroups; g++) {  // k_tp_compact
      const uint64_t t = kidx[g];
      if (g == ngroups) {
        fo[t] = fg[g];
        break;
      }
      if (kidx[g + 1] == t) continue;
      const uint64_t h = hl[g];
      fo[t] = fg[g];
      src0[t] = S[h];
      name_b[t] = g ? begin[h] : 0;
      name_len[t] = g ? eol[h] - begin[h] : 0;
      if (g == 0) kept0 = 1;
      if (g + 1 == ngroups) exempt = t;
    }
    P.n_dropped = nhdr - (nrec - kept0);
  }
  P.n_records = nrec;
  // k_tp_seq and k_tp_rev, byte by byte
  const uint64_t mult = rev ? 2 : 1, total = tp::seq_fwd_off(fo[nrec], rev);
  P.seqs.assign(total, '?');
  auto src = [&](uint64_t t, uint64_t j) {
    if (!fasta) return src0[t] + j;
    const uint64_t x = src0[t] + j, L = find(S, nlines, 1, x);
    EXPECT(S[L + 1] > x);
    return begin[L] + (x - S[L]);
  };
  for (uint64_t p = 0; p < total; p++) {
    const uint64_t t = find(fo, nrec, mult, p), r = p - mult * fo[t], len = fo[t + 1] - fo[t] - 1;
    EXPECT(tp::seq_fwd_off(fo[t], rev) == mult * fo[t]);
    if (r < len) {
      const unsigned char ch = text[src(t, r)];
      P.seqs[p] = (char)(t == exempt || ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T' ? ch : 'X');
    } else if (r == len || r == 2 * len + 1) {
      P.seqs[p] = '\n';
    }
  }
  if (rev)
    for (uint64_t p = 0; p < total; p++) {
      const uint64_t t = find(fo, nrec, 2, p), base = 2 * fo[t], len = fo[t + 1] - fo[t] - 1, r = p - base;
      if (r > len && r - len - 1 < len) {
        EXPECT(p >= tp::seq_rev_off(fo[t], len) && p < tp::seq_rev_off(fo[t], len) + len);
        const char f = P.seqs[base + (len - 1 - (r - len - 1))];
        P.seqs[p] = f == 'A' ? 'T' : f == 'T' ? 'A' : f == 'C' ? 'G' : f == 'G' ? 'C' : f == 'X' ? 'X' : '\0';
      }
    }
  // k_tp_idlen, k_tp_ids
  std::vector<uint64_t> idb(nrec + 1, 0);
  for (uint64_t t = 0; t < nrec; t++) idb[t] = tp::id_rec_len(name_len[t], fo[t + 1] - fo[t] - 1, rev);
  const std::vector<uint64_t> ioff = exclusive_scan(idb);
  P.ids.assign(ioff[nrec], '?');
  auto digit = [](uint64_t v, uint32_t d) {
    for (; d; d--) v /= 10;
    return (char)('0' + v % 10);
  };
  for (uint64_t p = 0; p < ioff[nrec]; p++) {
    const uint64_t t = find(ioff, nrec, 1, p);
    const uint64_t nlen = name_len[t], len = fo[t + 1] - fo[t] - 1, line0 = tp::id_line_len(nlen, len, 0);
    uint64_t r = p - ioff[t];
    const uint32_t strand = rev && r >= line0;
    if (strand) r -= line0;
    const uint64_t name_end = tp::ID_NUM_DIGITS + 1 + nlen, tab2 = name_end + 2 * strand;
    const uint32_t nd = tp::dec_digits(len);
    char ch;
    if (r < tp::ID_NUM_DIGITS) ch = digit((rev ? 2 * t : t) + strand, tp::ID_NUM_DIGITS - 1 - (uint32_t)r);
    else if (r == tp::ID_NUM_DIGITS) ch = '\t';
    else if (r < name_end) ch = (char)text[name_b[t] + (r - (tp::ID_NUM_DIGITS + 1))];
    else if (r < tab2) ch = r == name_end ? '_' : 'r';
    else if (r == tab2) ch = '\t';
    else if (r <= tab2 + nd) ch = digit(len, nd - (uint32_t)(r - tab2));
    else ch = '\n';
    P.ids[p] = ch;
  }
  return P;
}

uint32_t crc_by_slices(const uint8_t* p, uint32_t ulen, uint32_t lanes) {  // as k_sz_frame slices a chunk
  const uint32_t sd = tp::crc_slice_dwords(ulen, lanes);
  EXPECT(sd & 1u);
  EXPECT((uint64_t)sd * 4 * lanes >= ulen);
  uint32_t total = 0;
  for (uint32_t t = 0; t < lanes; t++) {
    const uint32_t b0 = t * sd * 4, b1 = b0 + sd * 4 < ulen ? b0 + sd * 4 : ulen;
    if (b0 >= ulen) continue;
    total = musc_sz::crc32c_combine(x2n.t, total, musc::crc32c(p + b0, b1 - b0), b1 - b0);
  }
  return total;
}

// sz_encode's output of `data`, described by the plan
void check_frame(const std::string& data) {
  const std::string s = musc::sz_encode(data);
  EXPECT(s.size() == tp::sz_frame_size(data.size()));
  EXPECT(memcmp(s.data(), "\xff\x06\x00\x00sNaPpY", 10) == 0);
  for (uint64_t i = 0; i < tp::sz_chunks(data.size()); i++) {
    const uint64_t at = tp::sz_chunk_pos(i);
    const uint32_t ulen = tp::sz_chunk_len(data.size(), i);
    EXPECT(at + tp::SZ_HEAD + ulen <= s.size());
    const uint8_t* h = (const uint8_t*)s.data() + at;
    EXPECT(h[0] == 0x01 && (h[1] | (uint32_t)h[2] << 8 | (uint32_t)h[3] << 16) == ulen + 4);
    const uint32_t stored = h[4] | (uint32_t)h[5] << 8 | (uint32_t)h[6] << 16 | (uint32_t)h[7] << 24;
    EXPECT(stored == musc::mask_crc(crc_by_slices((const uint8_t*)data.data() + i * tp::SZ_CHUNK, ulen, 256)));
    EXPECT(memcmp(h + tp::SZ_HEAD, data.data() + i * tp::SZ_CHUNK, ulen) == 0);
  }
  if (!data.empty()) EXPECT(tp::sz_chunk_pos(tp::sz_chunks(data.size()) - 1) + tp::SZ_HEAD + tp::sz_chunk_len(data.size(), tp::sz_chunks(data.size()) - 1) == s.size());
}

unsigned long long n_texts = 0, n_refused = 0, n_stopped = 0, n_exempt = 0;

void check_text(const std::string& raw, bool frames) {
  n_texts++;
  std::unique_ptr<unsigned char[]> exact(new unsigned char[raw.size() ? raw.size() : 1]);  // exactly its size
  memcpy(exact.get(), raw.data(), raw.size());
  for (int fasta = 0; fasta < 2; fasta++)
    for (int rev = 0; rev < 2; rev++) {
      const Passes P = passes(exact.get(), raw.size(), fasta, rev);
      musc::PreparedTargets pt;
      bool threw = false;
      try {
        pt = fasta ? musc::prep_targets_fasta(raw, rev) : musc::prep_targets_text(raw, rev);
      } catch (const musc::Die&) {
        threw = true;
      }
      EXPECT(threw == P.refused);
      if (threw) {
        n_refused++;
        const auto lines = musc::split_lines(raw);
        EXPECT(P.empty_line < lines.size() && lines[P.empty_line].empty());
        for (uint64_t k = 0; k < P.empty_line && k < lines.size(); k++) EXPECT(!lines[k].empty());
        continue;
      }
      std::string a, b;
      uint64_t F = 0;
      EXPECT(pt.seqs.size() == pt.ids.size() && pt.seqs.size() == tp::n_targets(P.n_records, rev));
      for (size_t k = 0; k < pt.seqs.size(); k++) {
        const uint64_t len = pt.seqs[k].size();
        const int strand = rev ? (int)(k & 1) : 0;
        if (!strand) EXPECT(a.size() == tp::seq_fwd_off(F, rev));
        else EXPECT(a.size() == tp::seq_rev_off(F - (len + 1), len));
        if (!strand) F += len + 1;
        // the name is what stands between the first tab of the id line and its last one
        const size_t t1 = pt.ids[k].find('\t'), t2 = pt.ids[k].rfind('\t');
        EXPECT(t1 == tp::ID_NUM_DIGITS && t2 > t1);
        EXPECT(pt.ids[k].size() + 1 == tp::id_line_len(t2 - t1 - 1 - (strand ? 2 : 0), len, strand));
        a += pt.seqs[k], a += '\n';
        b += pt.ids[k], b += '\n';
      }
      EXPECT(a == P.seqs);
      EXPECT(b == P.ids);
      if (!fasta && P.stop_line != NONE) n_stopped++;
      if (fasta && a != [&] { std::string s = a; for (auto& c : s) if (c != '\n' && c != 'A' && c != 'C' && c != 'G' && c != 'T' && c != '\0') c = 'X'; return s; }()) n_exempt++;
      if (frames) check_frame(a), check_frame(b);
    }
}

std::string random_short(std::mt19937& rng) {
  static const char alphabet[] = {'A', 'C', 'G', 'T', 'N', 'a', 'X', '\t', '\n', '>', '\r', ' ', '\0', (char)0xFF};
  std::string s(rng() % 41, '\0');
  for (auto& c : s) c = alphabet[rng() % sizeof alphabet];
  return s;
}

std::string random_records(std::mt19937& rng, bool fasta) {
  std::string s;
  const bool crlf = rng() % 4 == 0;
  const int nrec = (int)(rng() % 40);
  for (int i = 0; i < nrec; i++) {
    std::string name = "g" + std::to_string(i) + std::string(rng() % 6, ' ');
    std::string seq(rng() % 3 ? rng() % 90 : rng() % 700, 'A');
    for (auto& c : seq) c = rng() % 20 ? "ACGT"[rng() % 4] : "Nn-X>"[rng() % 5];
    const char* nl = crlf ? "\r\n" : "\n";
    if (fasta) {
      if (i || rng() % 3) s += ">" + name + nl;
      const size_t w = 1 + rng() % 70;
      for (size_t p = 0; p < seq.size(); p += w) s += seq.substr(p, w) + nl;
    } else {
      s += name + "\t" + seq + nl;
      if (rng() % 60 == 0) s += rng() % 2 ? std::string(nl) : std::string("no tab") + nl;
    }
  }
  if (!s.empty() && rng() % 3 == 0) s.pop_back();  // no final newline (or a lone \r)
  return s;
}

void check_crc() {
  std::mt19937 rng(7);
  // the slice is ceil(ulen / 1024) | 1 dwords: it grows at every multiple of 2048 bytes plus one
  std::vector<uint32_t> sizes = {0, 1, 2, 3, 4, 5, 7, 8, 1019, 1020, 1021, 1023, 1024, 1025, 65531, 65532, 65533, 65535, 65536};
  for (uint32_t k = 1; k * 2048 <= 65536; k++)
    for (int d = -5; d <= 5; d++)
      if ((int64_t)k * 2048 + d <= 65536) sizes.push_back(k * 2048 + d);
  for (uint32_t n : sizes) {
    std::unique_ptr<uint8_t[]> buf(new uint8_t[n ? n : 1]);
    for (uint32_t i = 0; i < n; i++) buf[i] = (uint8_t)rng();
    EXPECT(crc_by_slices(buf.get(), n, 256) == musc::crc32c(buf.get(), n));
  }
  EXPECT(tp::crc_slice_dwords(65536, 256) * 4 * 256 >= 65536);
}

}  // namespace

int main() {
  check_crc();
  EXPECT(tp::dec_digits(0) == 1 && tp::dec_digits(9) == 1 && tp::dec_digits(10) == 2 && tp::dec_digits(99999) == 5 && tp::dec_digits(100000) == 6);
  EXPECT(tp::dec_digits(~0ull) == 20);
  EXPECT(!tp::refused(0xFFFFFFEFull, 0) && tp::refused(0xFFFFFFF0ull, 0) && !tp::refused(0x7FFFFFF7ull, 1) && tp::refused(0x7FFFFFF8ull, 1));
  EXPECT(tp::sz_frame_size(0) == 10 && tp::sz_frame_size(1) == 19 && tp::sz_frame_size(65536) == 10 + 8 + 65536 && tp::sz_frame_size(65537) == 10 + 16 + 65537);
  std::mt19937 rng(20260222);
  for (int i = 0; i < 40000; i++) check_text(random_short(rng), i % 50 == 0);
  for (int i = 0; i < 300; i++) check_text(random_records(rng, i & 1), i % 10 == 0);
  {  // a text of more than two chunks, and chunk-sized ones
    std::string big;
    for (int i = 0; big.size() < 150000; i++) big += "t" + std::to_string(i) + "\t" + std::string(997, "ACGTN"[i % 5]) + "\n";
    check_text(big, true);
    for (size_t n : {65535u, 65536u, 65537u, 131072u, 131073u}) check_frame(big.substr(0, n));
  }
  for (const char* t : {"", "\r", "\n", ">", ">\n", "A", "\t", "a\t", "\tA", ">a\nA\n>b\n", "A\n>b\nC"}) check_text(t, true);
  EXPECT(n_refused > 1000 && n_stopped > 1000 && n_exempt > 100);
  char census[128];
  snprintf(census, sizeof census, "%llu texts, %llu refused, %llu stopped, %llu with an unsubstituted last record", n_texts, n_refused, n_stopped, n_exempt);
  return check_done("targets_prep_plan_check", census);
}
