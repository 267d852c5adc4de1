// read_names_plan_check.cpp -- read_names_plan.hpp against a literal restatement of the reference's string code
// (cmd/muscato_prep_reads/main.go:76-79, cmd/muscato_uniqify/main.go:83-135), byte loop by byte loop: every name length
// 0..1100 with a tab at every place that matters and without one, joins of every length around the bounds, the decimal
// widths, the lengths of a record and a line, and the path of a group; and read_names_lanes.hpp, what a lane of the
// stage computes, in lock step against the same string code (below); and read_names_keys.hpp, the order of the larger
// groups as integer keys, whose W + 2 stable passes are held to std::sort under PairLess pair for pair, whatever the order
// in which the pairs enter.  Stand-alone, no GPU: muscato_amd/build.py (CHECKS) builds it, plain and under the sanitizers.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../read_names_keys.hpp"
#include "../read_names_lanes.hpp"
#include "../read_names_plan.hpp"
#include "check.hpp"

using namespace musc_rn;

// ---- the reference, as strings
static std::string ref_clip(const std::string& name) { return name.size() > 1000 ? name.substr(0, 995) + "..." : name; }
static std::string ref_token(const std::string& clipped) {
  std::string t;
  for (char ch : clipped) {
    if (ch == '\t') break;
    t.push_back(ch);
  }
  return t;
}
static std::string ref_join(const std::vector<std::string>& tokens) {
  std::string j;
  for (size_t i = 0; i < tokens.size(); i++) {
    if (i) j.push_back(';');
    j += tokens[i];
  }
  return j.size() > 1000 ? j.substr(0, 996) + "..." : j;
}

// a name of n bytes without a tab; every byte differs from its neighbours so that a shifted copy would show
static std::string make_name(uint32_t n) {
  std::string s(n, 'a');
  for (uint32_t i = 0; i < n; i++) s[i] = (char)('a' + i % 23);
  return s;
}

static void check_name(const std::string& name) {
  const uint32_t n = (uint32_t)name.size();
  const std::string c = ref_clip(name), t = ref_token(c);
  EXPECT_MSG(clipped_len(n) == c.size(), "name of %u bytes", n);
  EXPECT_MSG(text_len(n) <= n && text_len(n) <= clipped_len(n), "name of %u bytes", n);
  if (clipped_len(n) != c.size() || text_len(n) > n) return;  // (a failed check goes on: the loops below index by these)
  for (uint32_t i = 0; i < clipped_len(n); i++) {  // the clipped name by position
    const char b = virtual_byte(n, i) ? '.' : name[i];
    EXPECT_MSG(b == c[i], "name of %u bytes, byte %u", n, i);
    EXPECT_MSG(virtual_byte(n, i) == (i >= text_len(n)), "name of %u bytes, byte %u", n, i);
  }
  uint32_t tab = text_len(n);  // the search the kernel makes: over the bytes that come from the text only
  for (uint32_t i = 0; i < text_len(n); i++)
    if (name[i] == '\t') {
      tab = i;
      break;
    }
  EXPECT_MSG(token_len(n, tab) == t.size(), "name of %u bytes, first tab %u", n, tab);
  EXPECT_MSG(token_len(n, tab == text_len(n) ? 0xFFFFFFFFu : tab) == t.size(), "name of %u bytes: any value past the text says no tab", n);
  const uint32_t m = meta_pack(clipped_len(n), token_len(n, tab));
  EXPECT_MSG(meta_clip(m) == c.size() && meta_tok(m) == t.size(), "meta of a name of %u bytes", n);
}

// ---------------------------------------------------------------- the stage in lock step (read_names_lanes.hpp)
// A kernel of the stage is a loop over items that calls one *_item function (measure, rank, pairs, unpairs, sizes,
// record, copy, line); here those functions run over every item in grid order, on seeded FASTQ texts built below,
// through a reader that counts every load outside the text, and what they leave is compared with the string code
// above: the ranked members, every record and every line, byte for byte.  The comparison sort between pairs_item and
// unpairs_item is std::sort under the same PairLess.

static long long loads_outside = 0;
struct CheckedText {  // the emulation's reader: the text is a heap block of exactly nbytes (the sanitizer sees a miss too)
  const unsigned char* text;
  uint64_t nbytes;
  uint32_t byte(uint64_t p) const {
    if (p >= nbytes) {
      loads_outside++;
      return 0xEEu;
    }
    return text[p];
  }
};
struct Pair {
  uint32_t x, y;
};

struct Rng {
  uint64_t s;
  uint32_t next() { return (uint32_t)((s = s * 6364136223846793005ull + 1442695040888963407ull) >> 33); }
};
static std::string rand_name(Rng& r, uint32_t n, const std::string& head = "@L") {
  static const char A[] = "abcdefghijklmnopqrstuvwxyz0123456789_/:";
  std::string s = head.substr(0, n);
  while (s.size() < n) s.push_back(A[r.next() % (sizeof A - 1)]);
  return s;
}

// ---- the larger groups by keys (read_names_keys.hpp): what rocprim::radix_sort_pairs does on the device, here a stable
// counting sort of the (key, pair number) list by the eight bytes of the key, the least significant first
static void stable_by_key(std::vector<uint64_t>& key, std::vector<uint32_t>& perm) {
  const size_t n = perm.size();
  std::vector<uint64_t> k2(n);
  std::vector<uint32_t> p2(n);
  for (int b = 0; b < 8; b++) {
    size_t count[257] = {};
    for (size_t i = 0; i < n; i++) count[((key[i] >> (8 * b)) & 255u) + 1]++;
    for (int v = 0; v < 256; v++) count[v + 1] += count[v];
    for (size_t i = 0; i < n; i++) {
      const size_t at = count[(key[i] >> (8 * b)) & 255u]++;
      k2[at] = key[i], p2[at] = perm[i];
    }
    key.swap(k2), perm.swap(p2);
  }
}
// the key passes over the pairs, which enter in the order `perm`; returns W
template <class R, class P>
static uint32_t radix_rank(const R& rd, const Names& N, const std::vector<P>& pairs, std::vector<uint32_t>& perm) {
  uint32_t maxclip = 0;  // (k_rn_pairs: one atomicMax)
  for (const P& p : pairs) maxclip = std::max(maxclip, clipped_len(N.name_len[p.y]));
  const uint32_t W = key_words(maxclip);
  std::vector<uint64_t> key(pairs.size());
  for (uint32_t pass = 0; pass < key_passes(maxclip); pass++) {
    for (uint64_t k = 0; k < pairs.size(); k++) key[k] = sortkey(rd, N, pairs.data(), perm.data(), k, pass, W);
    if (pass == 0)
      for (uint64_t v : key) EXPECT(v >> TAIL_BITS == 0);
    if (pass == W + 1)
      for (uint64_t v : key) EXPECT(v >> GROUP_BITS == 0);
    stable_by_key(key, perm);
  }
  return W;
}

// a FASTQ text of groups of reads with one sequence each, and what the parse and the sort in front of the stage leave
struct Fastq {
  std::string raw;
  std::vector<uint64_t> name_off;
  std::vector<uint32_t> name_len, seq_len;
  std::vector<std::string> names, seqs;  // by kept read
  uint32_t k = 0;
  std::string seq() {
    k++;
    std::string s;
    for (int j = 0; j < 12; j++) s.push_back("ACGT"[(k >> (2 * j)) & 3]);
    return s + (k % 5 == 0 ? "GATXACA" : "GATTACA") + std::string(k % 7, 'C');  // (an X now and then, lengths that cross a word)
  }
  void rec(const std::string& name, const std::string& s) {
    name_off.push_back(raw.size());
    name_len.push_back((uint32_t)name.size());
    seq_len.push_back((uint32_t)s.size());
    names.push_back(name);
    seqs.push_back(s);
    raw += name + "\n" + s + "\n+\n" + std::string(s.size(), 'I') + "\n";
  }
  void group(const std::vector<std::string>& ns, int align = -1) {
    if (align >= 0) {  // a filler record in front puts the first name at `align` modulo 16
      const std::string fill = seq();
      const uint64_t fixed = 1 + fill.size() + 3 + fill.size() + 1;
      rec(std::string((size_t)(((uint64_t)align + 16 * 1024 - (raw.size() + fixed) % 16) % 16), 'f'), fill);
    }
    const std::string s = seq();
    for (const std::string& n : ns) rec(n, s);
  }
};

static void lockstep(const char* what, const Fastq& F, int want_words = -1) {
  const uint64_t n = F.names.size(), nbytes = F.raw.size();
  unsigned char* const text = new unsigned char[nbytes ? nbytes : 1];  // exactly the text, nothing behind it
  for (uint64_t i = 0; i < nbytes; i++) text[i] = (unsigned char)F.raw[i];
  const CheckedText rd{text, nbytes};
  const Names N{F.name_off.data(), F.name_len.data(), n};

  // ---- what the sort + collapse in front of the stage leaves: the order by sequence (ties in file order), the groups
  std::vector<uint32_t> order(n);
  for (uint64_t i = 0; i < n; i++) order[i] = (uint32_t)i;
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return F.seqs[a] < F.seqs[b]; });
  std::vector<uint32_t> ustart, gid(n);
  for (uint64_t i = 0; i < n; i++) {
    if (i == 0 || F.seqs[order[i]] != F.seqs[order[i - 1]]) ustart.push_back((uint32_t)i);
    gid[i] = (uint32_t)ustart.size() - 1;
  }
  const uint64_t nu = ustart.size();
  ustart.push_back((uint32_t)n);
  // ... and the records of the loaded reads
  uint32_t maxlen = 0;
  for (uint64_t i = 0; i < n; i++) maxlen = std::max(maxlen, F.seq_len[i]);
  const int rw = (int)((maxlen + 15) / 16 + 1);
  std::vector<uint32_t> rdw(nu * rw + 1, 0), rdmw(nu * rw + 1, 0);
  for (uint64_t g = 0; g < nu; g++) {
    const std::string& s = F.seqs[order[ustart[g]]];
    for (size_t q = 0; q < s.size(); q++) {
      const size_t code = std::string("ACGT").find(s[q]);
      if (code == std::string::npos) rdmw[g * rw + q / 16] |= 1u << (2 * (q % 16));
      else rdw[g * rw + q / 16] |= (uint32_t)code << (2 * (q % 16));
    }
    rdw[g * rw + rw - 1] = (uint32_t)s.size();
  }

  // ---- measure: one item per kept read
  std::vector<uint32_t> meta(n);
  for (uint64_t i = 0; i < n; i++) meta[i] = measure_item(rd, N, i);
  // ---- rank: one item per place
  std::vector<uint32_t> ranked(n, 0xFFFFFFFFu), flag(n + 1, 0), excl(n + 1, 0);
  for (uint64_t i = 0; i < n; i++) flag[i] = rank_item(rd, N, order.data(), ustart.data(), gid[i], i, ranked.data());
  for (uint64_t i = 0; i < n; i++) excl[i + 1] = excl[i] + flag[i];  // (scan_u32)
  const uint64_t np = excl[n];
  // ---- pairs, the sort under PairLess, unpairs
  if (np) {
    std::vector<Pair> pairs(np), sorted;
    std::vector<uint32_t> place(np);
    for (uint64_t i = 0; i < n; i++) pairs_item(flag.data(), excl.data(), order.data(), gid[i], i, pairs.data(), place.data());
    const PairLess<CheckedText, Pair> less{rd, N};
    sorted = pairs;
    std::sort(sorted.begin(), sorted.end(), less);
    for (uint64_t k = 0; k + 1 < np; k++)  // a strict total order: neighbours differ one way only
      EXPECT_MSG(less(sorted[k], sorted[k + 1]) && !less(sorted[k + 1], sorted[k]) && !less(sorted[k], sorted[k]), "%s: pair %llu", what, (unsigned long long)k);
    for (uint64_t k = 0; k < np; k++) unpairs_item(sorted.data(), place.data(), k, ranked.data());
    // ---- the same order from the W + 2 key passes: the pairs entering as made, reversed, and in a seeded shuffle
    Rng shuffle{np * 2654435761ull + 23};
    for (int entry = 0; entry < 3; entry++) {
      std::vector<uint32_t> perm(np);
      for (uint64_t k = 0; k < np; k++) perm[k] = (uint32_t)(entry == 1 ? np - 1 - k : k);
      if (entry == 2)
        for (uint64_t k = np; k-- > 1;) std::swap(perm[k], perm[shuffle.next() % (k + 1)]);
      const uint32_t W = radix_rank(rd, N, pairs, perm);
      EXPECT_MSG(W <= CMP_WORDS && (want_words < 0 || W == (uint32_t)want_words), "%s: %u key words", what, W);
      for (uint64_t k = 0; k < np; k++)
        EXPECT_MSG(pairs[perm[k]].x == sorted[k].x && pairs[perm[k]].y == sorted[k].y, "%s: entry order %d, pair %llu by keys", what, entry, (unsigned long long)k);
      std::vector<uint32_t> again(n, 0xFFFFFFFFu);
      for (uint64_t k = 0; k < np; k++) unpairs_by_perm(pairs.data(), perm.data(), place.data(), k, again.data());
      for (uint64_t k = 0; k < np; k++) EXPECT_MSG(again[place[k]] == ranked[place[k]], "%s: entry order %d, place %u", what, entry, place[k]);
    }
  }
  EXPECT_MSG(want_words < 0 || np, "%s: no pairs", what);
  for (uint64_t i = 0; i < n; i++) EXPECT_MSG(place_group(ustart.data(), (uint32_t)nu, i) == gid[i], "%s: the group of place %llu", what, (unsigned long long)i);
  // ---- sizes: one item per group; the offsets by scan
  std::vector<uint32_t> tstart(n, 0xFFFFFFFFu), gsum(nu);
  std::vector<uint64_t> roff(nu + 1, 0), loff(nu + 1, 0);
  for (uint64_t g = 0; g < nu; g++) {
    const GroupSizes z = sizes_item(ranked.data(), ustart.data(), meta.data(), F.seq_len.data(), g, tstart.data(), gsum.data());
    roff[g + 1] = roff[g] + z.record;
    loff[g + 1] = loff[g] + z.line;
  }

  // ---- the reference: strings
  std::string ref_text, ref_lines;
  std::vector<uint64_t> ref_roff(1, 0), ref_loff(1, 0);
  for (uint64_t g = 0; g < nu; g++) {
    std::vector<uint32_t> mem(order.begin() + ustart[g], order.begin() + ustart[g + 1]);  // file order
    std::stable_sort(mem.begin(), mem.end(), [&](uint32_t a, uint32_t b) { return ref_clip(F.names[a]) < ref_clip(F.names[b]); });
    std::vector<std::string> tokens;
    for (uint32_t m : mem) tokens.push_back(ref_token(ref_clip(F.names[m])));
    for (size_t j = 0; j < mem.size(); j++)
      EXPECT_MSG(ranked[ustart[g] + j] == mem[j], "%s: group %llu of %zu, member %zu", what, (unsigned long long)g, mem.size(), j);
    const std::string rec = std::to_string(mem.size()) + "\t" + ref_join(tokens);
    ref_text += rec;
    ref_lines += F.seqs[mem[0]] + "\t" + rec + "\n";
    ref_roff.push_back(ref_text.size());
    ref_loff.push_back(ref_lines.size());
    EXPECT_MSG(roff[g + 1] == ref_roff[g + 1] && loff[g + 1] == ref_loff[g + 1], "%s: offsets behind group %llu", what, (unsigned long long)g);
  }
  if (roff != ref_roff || loff != ref_loff) {  // (the renders below index by these)
    delete[] text;
    return;
  }

  // ---- records, lines, copy: one item per (record, lane), whole and in ranges, at every alignment of the
  // destination, between guard bytes
  const Groups G{ranked.data(), ustart.data(), meta.data(), tstart.data(), gsum.data()};
  const Reads S{rdw.data(), rdmw.data(), rw};
  std::vector<unsigned char> ttext(ref_text.size() + 16, 0xA5);
  for (uint64_t g = 0; g < nu; g++)
    for (uint32_t lane = 0; lane < 64; lane++) record_item(rd, N, G, roff.data(), 0, g, lane, ttext.data());
  EXPECT_MSG(std::string((const char*)ttext.data(), ref_text.size()) == ref_text, "%s: the records", what);
  for (int k = 0; k < 16; k++) EXPECT_MSG(ttext[ref_text.size() + k] == 0xA5, "%s: a byte behind the records", what);
  const uint64_t ranges[][2] = {{0, nu}, {0, 1}, {nu / 2, nu / 2 + 3 < nu ? nu / 2 + 3 : nu}, {nu - 1, nu}};
  for (int which = 0; which < 3; which++) {  // record_item, line_item, copy_item
    const std::string& ref = which == 1 ? ref_lines : ref_text;
    const std::vector<uint64_t>& off = which == 1 ? loff : roff;
    for (const auto& r : ranges)
      for (uint32_t a = 0; a < (r[1] - r[0] > 8 ? 4u : 16u); a++) {  // (a whole text at the four dword phases, a few records at all sixteen)
        const uint64_t bytes = off[r[1]] - off[r[0]];
        std::vector<unsigned char> buf(16 + a + bytes + 16, 0x5A);
        unsigned char* const out = buf.data() + ((16 - (uintptr_t)buf.data() % 16) % 16) + a;
        for (uint64_t g = r[0]; g < r[1]; g++)
          for (uint32_t lane = 0; lane < 64; lane++) {
            if (which == 1) line_item(S, (const char*)ttext.data(), roff.data(), loff.data(), r[0], g, lane, out);
            else if (which == 2) copy_item((const char*)ttext.data(), roff.data(), r[0], g, lane, out);
            else record_item(rd, N, G, roff.data(), r[0], g, lane, out);
          }
        EXPECT_MSG(std::string((const char*)out, bytes) == ref.substr(off[r[0]], bytes), "%s: text %d, records %llu..%llu at %u", what, which,
                   (unsigned long long)r[0], (unsigned long long)r[1], a);
        bool guards = true;
        for (unsigned char* p = buf.data(); p < buf.data() + buf.size(); p++)
          if ((p < out || p >= out + bytes) && *p != 0x5A) guards = false;
        EXPECT_MSG(guards, "%s: text %d, a byte outside the destination", what, which);
      }
  }
  delete[] text;
}

static void lockstep_all() {
  Rng r{2300};
  const uint32_t lens[] = {0, 1, 7, 8, 9, 994, 995, 996, 997, 998, 999, 1000, 1001, 1100};
  {  // name lengths alone and together, at different alignments
    Fastq F;
    int i = 0;
    for (uint32_t n : lens) F.group({rand_name(r, n)}, (3 * i++) % 16);
    std::vector<std::string> all;
    for (uint32_t n : lens) all.insert(all.begin(), rand_name(r, n));
    F.group(all, 5);
    lockstep("lengths", F);
  }
  {  // pairs that first differ at byte d, the greater first in the file, the group at every alignment (both names at
     // every phase of a compare word); a name that is a prefix of the other at every length up to 17
    Fastq F;
    for (uint32_t d = 0; d < 17; d++)
      for (int a = 0; a < 16; a++) {
        const std::string stem = rand_name(r, d + 6);
        std::string lo = stem, hi = stem;
        lo[d] = 'A', hi[d] = 'b';
        F.group({hi, lo}, a);
        F.group({stem, stem.substr(0, d)}, (a + 7) % 16);
      }
    lockstep("pairs", F);
  }
  {  // long names: a difference up to byte 994 orders them, one beyond is a tie in file order; dots beside the virtual ones
    Fastq F;
    int i = 0;
    for (uint32_t d : {993u, 994u, 995u, 996u, 997u, 1005u}) {
      const std::string stem = rand_name(r, 1010);
      std::string a = stem, b = stem, c = stem;
      a[d] = 'z', b[d] = 'B', c[d] = 'k';
      F.group({a, b, c}, (5 * i++ + 1) % 16);
    }
    const std::string stem = rand_name(r, 1005);
    F.group({stem, stem.substr(0, 995) + "...", stem.substr(0, 995) + "..", stem.substr(0, 995) + "....", stem.substr(0, 1001)}, 7);
    F.group({"@prefix_and_more", "@prefix", "@prefix_and", "@prefix_", "@prefix_a"}, 2);
    lockstep("long", F);
  }
  {  // unsigned bytes at the deciding place
    Fastq F;
    const int bytes[][2] = {{0x00, 0x7F}, {0x7F, 0x80}, {0x80, 0xFF}, {0x00, 0xFF}, {0x01, 0x80}, {0x7F, 0xFF}};
    int i = 0;
    for (const auto& xy : bytes)
      for (uint32_t d : {0u, 3u, 7u, 8u, 13u}) {
        const std::string stem = rand_name(r, 15);
        std::string a = stem, b = stem;
        a[d] = (char)xy[1], b[d] = (char)xy[0];
        F.group({a, b}, (i++ + (int)d) % 16);
      }
    F.group({std::string("@p\0\0", 4), std::string("@p\0", 3), "@p"}, 3);  // zero bytes behind a prefix: the longer name is behind
    lockstep("high bytes", F);
  }
  {  // tabs at 0, at the end, at 994 and 995 of a long name, two of them, none; empty names and empty tokens
    Fastq F;
    const std::string ln = rand_name(r, 1100);
    F.group({"\tlead", "@z\tlate", "@last\t"}, 9);
    for (uint32_t p : {0u, 993u, 994u, 995u, 996u, 1099u}) {
      std::string s = ln;
      s[p] = '\t';
      F.group({s}, (int)(p % 16));
      F.group({s, "@b\tx", s}, (int)((p + 5) % 16));
    }
    F.group({"@two\ttabs\there", "@none"}, 4);
    F.group({"", "\tq", ""}, 15);
    F.group({"@m", "", "@a"}, 6);
    lockstep("tabs", F);
  }
  {  // groups of every size around the two bounds, names in reverse file order; counts of one to four digits
    Fastq F;
    int i = 0;
    for (uint32_t k : {1u, 2u, 3u, 9u, 10u, 63u, 64u, 65u, 99u, 100u, 256u, 257u, 999u, 1000u, 1001u, 1002u, 1003u}) {
      std::vector<std::string> ns;
      for (uint32_t j = k; j-- > 0;) ns.push_back("@g" + std::to_string(k) + "_" + std::to_string(10000 + j));
      F.group(ns, (7 * i++) % 16);
    }
    F.group(std::vector<std::string>(1000, ""), 0);  // 999 separators and nothing else: the longest join that is not clipped
    F.group(std::vector<std::string>(1001, ""), 1);
    F.group(std::vector<std::string>(1002, ""), 2);
    F.group(std::vector<std::string>(1500, ""), 3);
    lockstep("group sizes", F);
  }
  {
    Fastq F;
    std::vector<std::string> ns;
    for (uint32_t j = 5000; j-- > 0;) ns.push_back("@r" + std::to_string(10000 + j) + (j % 3 ? "" : "\tcomment"));
    F.group(ns, 3);
    ns.pop_back();
    ns.push_back(rand_name(r, 998, "@!"));  // the first name of the join has 998 bytes
    F.group(ns, 10);
    lockstep("5000", F);
  }
  {  // joins of 999 to 1002 bytes by four tokens; a ';' at byte 996, at byte 995; the cut inside a token, by count and by sort
    Fastq F;
    int i = 0;
    for (uint32_t total : {998u, 999u, 1000u, 1001u, 1002u, 1003u}) {
      const uint32_t last = total - 3 - 3 * 249;
      F.group({rand_name(r, 249, "@j0"), rand_name(r, last, "@j1"), rand_name(r, 249, "@j2"), rand_name(r, 249, "@j3")}, (5 * i++) % 16);
    }
    F.group({rand_name(r, 498, "@1"), rand_name(r, 497, "@0"), rand_name(r, 30, "@2")}, 11);
    F.group({rand_name(r, 497, "@1"), rand_name(r, 497, "@0"), rand_name(r, 30, "@2")}, 14);
    F.group({rand_name(r, 496, "@1"), rand_name(r, 497, "@0"), rand_name(r, 30, "@2")}, 1);
    std::vector<std::string> w, s;
    for (uint32_t j = 40; j-- > 0;) w.push_back(rand_name(r, 60, "@w" + std::to_string(100 + j)));
    for (uint32_t j = 100; j-- > 0;) s.push_back(rand_name(r, 30, "@s" + std::to_string(1000 + j)));
    F.group(w, 8);
    F.group(s, 13);
    F.group({rand_name(r, 1100), rand_name(r, 1100)}, 6);  // two clipped names: 998 + 1 + 998
    lockstep("joins", F);
  }
  {  // a seeded mixture: random sizes, lengths, tabs and shared prefixes
    Fastq F;
    for (int g = 0; g < 300; g++) {
      const uint32_t k = 1 + r.next() % (g % 50 == 0 ? 200 : 6);
      std::vector<std::string> ns;
      const std::string stem = rand_name(r, r.next() % 40);
      for (uint32_t j = 0; j < k; j++) {
        std::string s = stem + rand_name(r, r.next() % 12, "");
        if (r.next() % 4 == 0 && !s.empty()) s[r.next() % s.size()] = '\t';
        if (r.next() % 16 == 0) s += rand_name(r, 980 + r.next() % 40, "");
        ns.push_back(s);
      }
      F.group(ns, (int)(r.next() % 16));
    }
    lockstep("mixture", F);
  }
  {  // a text that ends with its last name's last byte: no record is complete behind it, nothing is read behind it
    Fastq F;
    F.group({"@a", "@b"});
    F.name_off.push_back(F.raw.size()), F.name_len.push_back(3), F.seq_len.push_back((uint32_t)F.seqs[0].size());
    F.names.push_back("@a\t"), F.seqs.push_back(F.seqs[0]);
    F.raw += "@a\t";
    lockstep("name at the end", F);
  }
  // ---- the order of the larger groups by keys: cases of their own (every lock-step text above runs the passes too)
  const auto filled = [&](std::vector<std::string> ns, size_t k, const std::string& head, uint32_t len) {  // ... up to k members
    while (ns.size() < k) ns.insert(ns.begin() + (ns.size() * 7) % (ns.size() + 1), rand_name(r, len, head));
    return ns;
  };
  {  // a prefix with one, two and eight 0x00 bytes behind it; a prefix that ends on a word boundary and one inside a word
    Fastq F;
    const std::string z8(8, '\0');
    F.group(filled({std::string("@p\0", 3), "@p", std::string("@p\0\0", 4), "@p" + z8, std::string("@p\0\0\0", 5) + "a"}, 65, "@p", 12), 1);
    F.group(filled({"@prefix8" + z8, "@prefix8", "@prefix8" + std::string(1, '\0'), "@prefix8" + z8 + z8, "@prefix8" + z8 + "b"}, 70, "@prefix", 20), 6);
    F.group(filled({"@prefix8_and_more", "@prefix8", "@prefix8_", "@prefix8_and_more_behind_it"}, 66, "@prefix8", 9), 11);
    F.group(filled({"@prefix_in_a_word_and_more", "@prefix_in_a", "@prefix_in_a_", "@prefix_in_"}, 67, "@prefix_in_a_word", 30), 4);
    lockstep("prefixes by keys", F);
  }
  {  // W = 0, 1, 2, 124 and 125: each in a text of its own, W being the longest name of all the pairs
    const uint32_t longest[][2] = {{0, 0}, {1, 1}, {8, 1}, {9, 2}, {16, 2}, {985, 124}, {992, 124}, {993, 125}, {1000, 125}, {1001, 125}, {1100, 125}};
    int i = 0;
    for (const auto& lw : longest) {
      Fastq F;
      std::vector<std::string> ns;
      for (uint32_t j = 0; j < 65; j++) ns.push_back(rand_name(r, j % 3 == 0 ? lw[0] : lw[0] - lw[0] * (j % 5) / 7));
      if (lw[0] > 1000) ns.push_back(ns[0].substr(0, 996) + "!" + ns[0].substr(997)), ns.push_back(ns[0].substr(0, 994) + "!" + ns[0].substr(995));
      F.group({"@a_small_group", "@"}, 3);
      F.group(ns, (3 * i++) % 16);
      lockstep("key words", F, (int)lw[1]);
    }
  }
  {  // a larger group in which all names are equal (file order), beside one of distinct names; a group of exactly 65
    Fastq F;
    F.group(std::vector<std::string>(70, "@same_name_every_time"), 9);
    F.group(filled({}, 65, "@sixty-five", 16), 2);
    F.group(std::vector<std::string>(65, std::string(1100, 'q')), 13);
    lockstep("equal names", F);
  }
  EXPECT_MSG(loads_outside == 0, "%lld loads outside the text", loads_outside);
}

int main() {
  lockstep_all();
  // ---- names
  for (uint32_t n = 0; n <= 1100; n++) {
    const std::string base = make_name(n);
    check_name(base);
    std::vector<uint32_t> at = {0, 1, 7, 8, 9, n / 2, 993, 994, 995, 996, 997, 998, 999, 1000, n - 2, n - 1};
    for (uint32_t p : at) {
      if (p >= n) continue;
      std::string s = base;
      s[p] = '\t';
      check_name(s);
      if (p + 3 < n) {  // a second tab behind the first
        s[p + 3] = '\t';
        check_name(s);
      }
    }
  }
  // ---- decimal widths
  for (uint64_t v : {0ull, 1ull, 9ull, 10ull, 99ull, 100ull, 999ull, 1000ull, 9999ull, 10000ull, 99999ull, 100000ull, 4294967279ull,
                     4294967295ull, 9999999999ull, 10000000000ull})
    EXPECT_MSG(dec_width(v) == std::to_string(v).size(), "width of %llu", (unsigned long long)v);
  for (uint64_t v = 0; v < 200000; v++) EXPECT_MSG(dec_width(v) == std::to_string(v).size(), "width of %llu", (unsigned long long)v);

  // ---- joins: k tokens of equal length and one that sets the total, for every total around the bounds
  for (uint32_t k : {1u, 2u, 3u, 64u, 65u, 500u}) {
    for (uint32_t total = (k > 990 ? k : 990); total <= 1012; total++) {
      if (total < k - 1) continue;  // (the separators alone are longer)
      const uint32_t body = total - (k - 1), each = body / k;
      std::vector<std::string> tokens(k, make_name(each));
      tokens[k - 1] = make_name(body - each * (k - 1));
      uint64_t sum = 0;
      for (const std::string& t : tokens) sum += t.size() + 1;
      sum -= 1;
      EXPECT_MSG(sum == total, "a join of %u tokens", k);
      const std::string j = ref_join(tokens);
      for (uint64_t s : {sum, sum > JOIN_LIMIT ? (uint64_t)JOIN_LIMIT + 1 : sum, sum > JOIN_LIMIT ? sum + 100000 : sum}) {  // saturated sums say the same
        EXPECT_MSG(join_len(s) == j.size(), "join of %u bytes", total);
        EXPECT_MSG(join_clipped(s) == (total > 1000), "join of %u bytes", total);
        EXPECT_MSG(join_text_len(s) + (join_clipped(s) ? DOTS : 0) == j.size(), "join of %u bytes", total);
        for (uint64_t count : {1ull, 9ull, 10ull, 5000ull, 4294967279ull}) {
          const std::string rec = std::to_string(count) + "\t" + j;
          EXPECT_MSG(record_len(count, s) == rec.size(), "record of %llu reads, join of %u bytes", (unsigned long long)count, total);
          for (uint64_t L : {0ull, 1ull, 100ull, 65535ull}) {
            const std::string line = std::string(L, 'A') + "\t" + rec + "\n";
            EXPECT_MSG(line_len(L, count, s) == line.size(), "line of a read of %llu bases", (unsigned long long)L);
          }
        }
      }
      // the bytes of the join by position: token m starts at the scan of token + 1, nothing is written at or past the cut
      std::string byp(join_len(sum), '?');
      uint64_t start = 0;
      const uint32_t limit = join_text_len(sum);
      for (uint32_t m = 0; m < k && start < limit; m++) {
        for (uint64_t p = 0; p < tokens[m].size() && start + p < limit; p++) byp[start + p] = tokens[m][p];
        if (m + 1 < k && start + tokens[m].size() < limit) byp[start + tokens[m].size()] = ';';
        start += tokens[m].size() + 1;
      }
      if (join_clipped(sum))
        for (uint32_t d = 0; d < DOTS; d++) byp[limit + d] = '.';
      EXPECT_MSG(byp == j, "join of %u tokens, %u bytes, by position", k, total);
    }
  }
  // ---- paths and the refusal bound
  for (uint64_t c = 0; c < 10000; c++) {
    const Path p = group_path(c);
    EXPECT_MSG(p == (c < 2 ? PATH_SINGLE : c <= 64 ? PATH_WAVE : PATH_SORTED), "group of %llu", (unsigned long long)c);
  }
  EXPECT_MSG(group_path(0xFFFFFFFFull) == PATH_SORTED, "the largest group");
  EXPECT_MSG(!refused(0) && !refused(0xFFFFFFEFull) && refused(0xFFFFFFF0ull) && refused(0xFFFFFFFFull) && refused(1ull << 40), "refusal bound");
  return check_done("read_names_plan_check");
}
