// sz_plan_check.cpp -- the chunk table, the element walk and CRC-32C by parts (csrc/sz_plan.hpp: what the device decoder
// of framed snappy streams is planned and checked with) against sz.hpp's sz_decode, snappy_block_decode and crc32c, as
// a program of its own so that it runs under the sanitizers: muscato_amd/build.py (CHECKS) builds it, plain and sanitized.
// It needs no GPU and is not part of the library.
//
// Over seeded small streams, every single-byte change (each byte to each other value) and every truncation:
//   sz_decode throws  <=>  the plan rejects, or snappy_block_decode on a planned chunk throws, or a CRC differs
//     (but for the plan's refusal of a chunk that declares more than 65 536 bytes, a rule sz_decode does not have)
//   snappy_block_decode throws  <=>  block_walk (the kernel's element walk) fails, and their bytes agree when neither does
//   nothing throws  =>  the plan's sizes and offsets are those of what sz_decode produced
// Every mutated stream is copied into a buffer of exactly its size, so that a read past its end is an error under the
// address sanitizer.  The CRC: crc32c_combine against crc32c for every split of short buffers, and the slices of
// k_sz_decode (an odd number of dwords per lane, each CRC times x^(8 * bytes behind it), all XORed).
//
// The compressing writer (csrc/sz_compress_plan.hpp; sz.hpp's sz_encode_compressed is built on it):
//   - chunk_block, the rule in its tile form, read through a reader that counts every dword index outside the chunk's
//     own dwords (an array of exactly that size: a read past it is an error under the address sanitizer), against
//     restate_block, the rule said position by position with no table at all: the far candidate is the highest
//     position in front of the tile with the same hash, the near one the lowest position of the tile in front of i
//     with the same 12-bit key, both compared byte by byte.  Seeded texts of two, four and 253 letters, periods 1 to 3;
//   - sz_encode_compressed to sz_decode round trips: every text of two letters up to 13 bytes, seeded texts around the
//     tile and chunk sizes, several chunks;
//   - every literal head and every copy element to the encoders' limits, decoded bit by bit; the varint;
//   - the bound for every stream made here, and the stored rule on both sides of n - n / 8.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "../sz_compress_plan.hpp"
#include "../sz_plan.hpp"
#include "check.hpp"
#include "sz.hpp"

namespace {

namespace ms = musc_sz;

const ms::X2n x2n;

// ---- a small stream writer with copies in it (sz_encode writes uncompressed chunks only)

void put_varint(std::string& s, uint64_t n) {
  for (; n >= 0x80; n >>= 7) s.push_back((char)((n & 0x7F) | 0x80));
  s.push_back((char)n);
}

// a block of literals and copies that decodes to `plain` (built along): elements drawn by rng
std::string random_block(std::mt19937& rng, std::string& plain, size_t target) {
  std::string el;
  plain.clear();
  while (plain.size() < target) {
    const int kind = plain.empty() ? 0 : (int)(rng() % 4);
    if (kind == 0) {
      const size_t n = 1 + rng() % 70;
      if (n <= 60 && rng() % 3) {
        el.push_back((char)((n - 1) << 2));
      } else {
        const int nb = 1 + (int)(rng() % 4);
        el.push_back((char)((59 + nb) << 2));
        for (int i = 0; i < nb; i++) el.push_back((char)(((n - 1) >> (8 * i)) & 0xFF));
      }
      for (size_t i = 0; i < n; i++) {
        const char ch = "ACGT"[rng() % 4];
        el.push_back(ch);
        plain.push_back(ch);
      }
      continue;
    }
    const size_t off = 1 + rng() % plain.size();
    size_t len;
    if (kind == 1 && off < 2048) {
      len = 4 + rng() % 8;
      el.push_back((char)(1 | ((len - 4) << 2) | ((off >> 8) << 5)));
      el.push_back((char)(off & 0xFF));
    } else {
      len = 1 + rng() % 64;
      const int nb = kind == 3 ? 4 : 2;
      el.push_back((char)((nb == 2 ? 2 : 3) | ((len - 1) << 2)));
      for (int i = 0; i < nb; i++) el.push_back((char)((off >> (8 * i)) & 0xFF));
    }
    for (size_t i = 0; i < len; i++) plain.push_back(plain[plain.size() - off]);
  }
  std::string block;
  put_varint(block, plain.size());
  return block + el;
}

void put_chunk(std::string& s, uint8_t type, const std::string& body) {
  s.push_back((char)type);
  for (int i = 0; i < 3; i++) s.push_back((char)((body.size() >> (8 * i)) & 0xFF));
  s += body;
}

std::string crc_word(const std::string& plain) {
  const uint32_t c = musc::mask_crc(musc::crc32c((const uint8_t*)plain.data(), plain.size()));
  std::string w;
  for (int i = 0; i < 4; i++) w.push_back((char)((c >> (8 * i)) & 0xFF));
  return w;
}

std::string random_stream(std::mt19937& rng, std::string& plain) {
  std::string s;
  plain.clear();
  if (rng() % 4) put_chunk(s, 0xFF, "sNaPpY");
  const int nchunks = 1 + (int)(rng() % 3);
  for (int k = 0; k < nchunks; k++) {
    if (rng() % 5 == 0) put_chunk(s, rng() % 2 ? 0x80 : 0xFE, std::string(rng() % 5, 'z'));
    std::string piece;
    if (rng() % 3) {
      const std::string block = random_block(rng, piece, rng() % 90);
      put_chunk(s, 0x00, crc_word(piece) + block);
    } else {
      for (size_t i = 0, n = rng() % 40; i < n; i++) piece.push_back("ACGT"[rng() % 4]);
      put_chunk(s, 0x01, crc_word(piece) + piece);
    }
    plain += piece;
  }
  return s;
}

// ---- one stream, both ways

unsigned long long n_streams = 0, n_thrown = 0, n_refused = 0;

void check_stream(const std::string& stream) {
  n_streams++;
  std::unique_ptr<uint8_t[]> exact(new uint8_t[stream.size() ? stream.size() : 1]);  // exactly its size
  memcpy(exact.get(), stream.data(), stream.size());
  const uint8_t* p = exact.get();

  ms::Plan plan;
  const int rc = ms::sz_plan(p, stream.size(), plan);
  bool rejects = rc != 0;
  EXPECT(rc == 0 || rc == ms::SZ_BAD || rc == ms::SZ_REFUSED);
  if (rc == ms::SZ_REFUSED) {  // sz_decode has no such rule (and reserves what the varint says): nothing to compare
    n_refused++;
    EXPECT(!plan.msg.empty());
    return;
  }

  bool threw = false;
  std::string decoded;
  try {
    decoded = musc::sz_decode(stream);
  } catch (const std::exception&) {
    threw = true;
  }
  EXPECT((rc != 0) == !plan.msg.empty());
  std::string joined;
  if (!rejects) {
    uint64_t sum = 0;
    for (const ms::Chunk& c : plan.chunks) {
      EXPECT(c.out_off == sum);
      EXPECT(c.body + c.body_len <= stream.size() && c.block + c.block_len <= stream.size());
      EXPECT(c.ulen <= ms::SZ_MAX_CHUNK);
      sum += c.ulen;
      std::string piece;
      bool bad_block = false;
      if (c.type == 0) {
        try {
          musc::snappy_block_decode(p + c.block, c.block_len, piece);
        } catch (const std::exception&) {
          bad_block = true;
        }
        std::vector<uint8_t> walked;
        const uint32_t st = ms::block_walk(p + c.body, c.body_len, c.ulen, walked);
        EXPECT((st != ms::ST_OK) == bad_block);
        EXPECT(st < ms::ST_CHECKSUM);
        if (!bad_block && st == ms::ST_OK) EXPECT(piece == std::string(walked.begin(), walked.end()));
      } else {
        EXPECT(c.body == c.block && c.body_len == c.block_len && c.ulen == c.body_len);
        piece.assign((const char*)p + c.body, c.body_len);
      }
      if (bad_block) {
        rejects = true;
        break;
      }
      EXPECT(piece.size() == c.ulen);
      if (musc::mask_crc(musc::crc32c((const uint8_t*)piece.data(), piece.size())) != c.crc) {
        rejects = true;
        break;
      }
      joined += piece;
    }
    if (!rejects) EXPECT(sum == plan.n_out);
  }
  EXPECT(threw == rejects);
  if (threw) n_thrown++;
  if (!threw && !rejects) {
    EXPECT(joined == decoded);
    EXPECT(plan.n_out == decoded.size());
  }
}

void check_mutations(const std::string& stream) {
  check_stream(stream);
  for (size_t cut = 0; cut < stream.size(); cut++) check_stream(stream.substr(0, cut));
  std::string m = stream;
  for (size_t i = 0; i < m.size(); i++) {
    const char keep = m[i];
    for (int v = 0; v < 256; v++) {
      if ((char)v == keep) continue;
      m[i] = (char)v;
      check_stream(m);
    }
    m[i] = keep;
  }
}

// ---- CRC-32C by parts

uint32_t crc_by_slices(const uint8_t* p, uint32_t ulen, uint32_t lanes) {  // as k_sz_decode slices a chunk
  const uint32_t sd = ((ulen + 4 * lanes - 1) / (4 * lanes)) | 1u;
  uint32_t total = 0;
  for (uint32_t t = 0; t < lanes; t++) {
    const uint32_t b0 = t * sd * 4, b1 = b0 + sd * 4 < ulen ? b0 + sd * 4 : ulen;
    if (b0 >= ulen) continue;
    total ^= ms::gf2_mul(ms::x8n(x2n.t, ulen - b1), musc::crc32c(p + b0, b1 - b0));
  }
  return total;
}

void check_crc() {
  std::mt19937 rng(99);
  EXPECT(musc::crc32c((const uint8_t*)"123456789", 9) == 0xE3069283u);
  EXPECT(ms::x8n(x2n.t, 0) == 0x80000000u);
  for (size_t n = 0; n <= 40; n++) {
    std::vector<uint8_t> buf(n);
    for (auto& b : buf) b = (uint8_t)rng();
    const uint32_t whole = musc::crc32c(buf.data(), n);
    for (size_t k = 0; k <= n; k++)
      EXPECT(ms::crc32c_combine(x2n.t, musc::crc32c(buf.data(), k), musc::crc32c(buf.data() + k, n - k), n - k) == whole);
  }
  for (uint32_t n : {0u, 1u, 3u, 4u, 5u, 255u, 256u, 1023u, 1024u, 1025u, 3071u, 3072u, 3073u, 40000u, 65535u, 65536u}) {
    std::vector<uint8_t> buf(n);
    for (auto& b : buf) b = (uint8_t)rng();
    EXPECT(crc_by_slices(buf.data(), n, 256) == musc::crc32c(buf.data(), n));
    EXPECT(crc_by_slices(buf.data(), n, 7) == musc::crc32c(buf.data(), n));
  }
  // 256 slices of an odd number of dwords cover a whole chunk
  EXPECT((((ms::SZ_MAX_CHUNK + 1023) / 1024) | 1u) * 4 * 256 >= ms::SZ_MAX_CHUNK);
}

// ---- the compressing writer

namespace zc = musc_szc;

unsigned long long n_blocks = 0, n_roundtrips = 0, n_bad_reads = 0;

// the chunk's own dwords and nothing else: ((n - 1) >> 2) + 2 of them (load32 reads dword (i >> 2) + 1 for i < n)
struct ExactReader {
  std::unique_ptr<uint32_t[]> dw;
  uint32_t ndw;
  explicit ExactReader(const std::string& data) : ndw((((uint32_t)data.size() - 1) >> 2) + 2) {
    dw.reset(new uint32_t[ndw]);
    // (what lies beyond byte n must not decide anything: filled with a pattern that differs from dword to dword)
    for (uint32_t k = 0; k < ndw; k++) dw[k] = 0xA5C3E100u + k;
    memcpy(dw.get(), data.data(), data.size());
  }
  uint32_t operator()(uint32_t k) const {
    if (k >= ndw) {
      n_bad_reads++;
      return 0;
    }
    return dw[k];
  }
};

struct StringWriter {
  std::string out;
  void operator()(uint32_t at, uint8_t b) {
    if (at >= out.size()) out.resize(at + 1, '\0');
    out[at] = (char)b;
  }
};

void plain_literal(std::string& el, const std::string& data, size_t from, size_t to) {
  const size_t v = to - from - 1;
  if (v < 60) {
    el.push_back((char)(v << 2));
  } else if (v < 256) {
    el.push_back((char)(60 << 2));
    el.push_back((char)v);
  } else {
    el.push_back((char)(61 << 2));
    el.push_back((char)(v & 0xFF));
    el.push_back((char)(v >> 8));
  }
  el.append(data, from, to - from);
}

size_t common(const std::string& d, size_t j, size_t i) {  // byte by byte, to the end, at most 64
  size_t m = 0;
  while (m < 64 && i + m < d.size() && d[j + m] == d[i + m]) m++;
  return m;
}

// the rule with no table: every position finds its two candidates by looking through the text
std::string restate_block(const std::string& d) {
  const size_t n = d.size();
  auto key = [&](size_t i) {
    return zc::hash4((uint32_t)(uint8_t)d[i] | ((uint32_t)(uint8_t)d[i + 1] << 8) | ((uint32_t)(uint8_t)d[i + 2] << 16) | ((uint32_t)(uint8_t)d[i + 3] << 24));
  };
  std::string el;
  put_varint(el, n);
  size_t p = 0, ls = 0;
  while (p < n) {
    size_t len = 0, off = 0;
    if (p + 4 <= n) {
      const size_t T = p / 256 * 256;
      const uint32_t h = key(p);
      size_t mf = 0, mn = 0, jf = 0, jn = 0;
      for (size_t j = T; j-- > 0;)
        if (key(j) == h) {  // the highest position in front of the tile with the hash: the only far candidate
          jf = j;
          if (memcmp(&d[j], &d[p], 4) == 0) mf = common(d, j, p);
          break;
        }
      for (size_t j = T; j < p; j++)
        if ((key(j) >> 2) == (h >> 2)) {  // the lowest position of the tile with the 12-bit key: the only near one
          jn = j;
          if (memcmp(&d[j], &d[p], 4) == 0) mn = common(d, j, p);
          break;
        }
      if (mn >= 4 && mn >= mf) len = mn, off = p - jn;
      else if (mf >= 4) len = mf, off = p - jf;
    }
    if (len < 4) {
      p++;
      continue;
    }
    if (ls < p) plain_literal(el, d, ls, p);
    if (len <= 11 && off < 2048) {
      el.push_back((char)(1 | ((len - 4) << 2) | ((off >> 8) << 5)));
      el.push_back((char)(off & 0xFF));
    } else {
      el.push_back((char)(2 | ((len - 1) << 2)));
      el.push_back((char)(off & 0xFF));
      el.push_back((char)(off >> 8));
    }
    ls = p += len;
  }
  if (ls < n) plain_literal(el, d, ls, n);
  return el;
}

void check_block(const std::string& d) {  // 1 <= size <= a chunk
  n_blocks++;
  const ExactReader rd(d);
  StringWriter w;
  const uint32_t bsz = zc::chunk_block(rd, (uint32_t)d.size(), w);
  EXPECT(bsz == w.out.size());
  EXPECT(w.out == restate_block(d));
  std::string back;
  bool threw = false;
  try {
    musc::snappy_block_decode((const uint8_t*)w.out.data(), w.out.size(), back);
  } catch (const std::exception&) {
    threw = true;
  }
  EXPECT(!threw && back == d);
}

void check_roundtrip(const std::string& d) {
  n_roundtrips++;
  const std::string s = musc::sz_encode_compressed(d);
  EXPECT(s.size() <= zc::sz_compress_bound(d.size()) && s.size() <= musc::sz_encode(d).size());
  bool threw = false;
  std::string back;
  try {
    back = musc::sz_decode(s);
  } catch (const std::exception&) {
    threw = true;
  }
  EXPECT(!threw && back == d);
  // chunk by chunk: the type says which side of n - n / 8 the block fell on, and a kept block is chunk_block's
  size_t pos = 10, at = 0;
  EXPECT(s.compare(0, 10, std::string("\xff\x06\x00\x00sNaPpY", 10)) == 0);
  for (uint64_t k = 0; k < zc::chunks(d.size()); k++) {
    const uint32_t n = zc::chunk_len(d.size(), k);
    const size_t len = (uint8_t)s[pos + 1] | ((size_t)(uint8_t)s[pos + 2] << 8) | ((size_t)(uint8_t)s[pos + 3] << 16);
    const ExactReader rd(d.substr(at, n));
    StringWriter w;
    const uint32_t bsz = zc::chunk_block(rd, n, w);
    if (zc::stored(bsz, n)) EXPECT(s[pos] == 0x01 && len == n + 4u && s.compare(pos + 8, n, d, at, n) == 0);
    else EXPECT(s[pos] == 0x00 && len == bsz + 4u && s.compare(pos + 8, bsz, w.out) == 0);
    pos += 4 + len;
    at += n;
  }
  EXPECT(pos == s.size());
}

std::string letters(std::mt19937& rng, size_t n, unsigned nletters) {
  std::string d(n, '\0');
  for (auto& ch : d) ch = nletters <= 4 ? "ACGT"[rng() % nletters] : (char)(rng() % nletters);
  return d;
}

void check_compress() {
  std::mt19937 rng(27);
  // ---- the arithmetic
  EXPECT(zc::sz_compress_bound(0) == 10 && zc::sz_compress_bound(1) == 19 && zc::sz_compress_bound(65536) == 10 + 8 + 65536 &&
         zc::sz_compress_bound(65537) == 10 + 16 + 65537);
  for (uint32_t n = 1; n <= zc::CHUNK; n++) {
    EXPECT(!zc::stored(n - n / 8 - 1, n) && zc::stored(n - n / 8, n));
    std::string v;
    put_varint(v, n);
    StringWriter w;
    EXPECT(zc::put_varint(w, 0, n) == v.size() && w.out == v && zc::varint_size(n) == v.size());
  }
  for (uint32_t tile = 0; tile < zc::CHUNK / zc::TILE_POS; tile++)
    for (uint32_t t = 0; t < zc::TILE_POS; t++) {
      const uint32_t e = zc::near_entry(tile, t);
      EXPECT(e != 0 && zc::near_pos(e, tile) == tile * zc::TILE_POS + t && zc::near_pos(e, tile + 1) == zc::CHUNK && zc::near_pos(0, tile) == zc::CHUNK);
      EXPECT(t + 1 == zc::TILE_POS || zc::near_entry(tile, t + 1) < e);  // the earliest position of a tile wins a max
      EXPECT(zc::near_entry(tile + 1, zc::TILE_POS - 1) > zc::near_entry(tile, 0));  // and a later tile beats an earlier one
    }
  // ---- every literal head (decoded as snappy_block_decode reads it) and every copy element
  for (uint32_t L = 1; L <= zc::CHUNK; L++) {
    StringWriter w;
    const uint32_t s = zc::put_lit_head(w, 0, L);
    EXPECT(s == zc::lit_head_size(L) && s == w.out.size());
    const uint8_t tag = (uint8_t)w.out[0];
    size_t len = tag >> 2;
    EXPECT((tag & 3) == 0);
    if (len >= 60) {
      EXPECT(s == 1 + (len - 59));
      size_t v = 0;
      for (size_t i = 0; i + 1 < s; i++) v |= (size_t)(uint8_t)w.out[1 + i] << (8 * i);
      len = v;
    } else {
      EXPECT(s == 1);
    }
    EXPECT(len + 1 == L);
  }
  for (uint32_t off = 1; off < zc::CHUNK; off++)
    for (uint32_t len = zc::MIN_MATCH; len <= zc::MAX_MATCH; len++) {
      StringWriter w;
      const uint32_t s = zc::put_copy(w, 0, off, len);
      const uint8_t tag = (uint8_t)w.out[0];
      uint32_t dl, doff;
      if ((tag & 3) == 1) dl = ((tag >> 2) & 7) + 4, doff = ((uint32_t)(tag >> 5) << 8) | (uint8_t)w.out[1];
      else dl = (tag >> 2) + 1, doff = (uint8_t)w.out[1] | ((uint32_t)(uint8_t)w.out[2] << 8);
      EXPECT(s == w.out.size() && s == zc::copy_size(off, len) && s == ((tag & 3) == 1 ? 2u : 3u) && (tag & 3) != 0 && (tag & 3) != 3 && dl == len && doff == off);
      EXPECT(((tag & 3) == 1) == (len <= 11 && off < 2048));
    }
  // ---- the tile rule against its restatement, through the exact reader
  for (unsigned nletters : {1u, 2u, 4u, 253u})
    for (size_t n : {1u, 2u, 3u, 4u, 5u, 7u, 8u, 63u, 64u, 65u, 255u, 256u, 257u, 259u, 260u, 511u, 512u, 513u, 700u, 1027u, 2500u})
      for (int rep = 0; rep < 3; rep++) check_block(letters(rng, n, nletters));
  for (size_t period : {1u, 2u, 3u, 5u, 64u, 65u, 255u, 256u, 257u}) {
    const std::string unit = letters(rng, period, 253);
    std::string d;
    while (d.size() < 1500) d += unit;
    check_block(d);
    d[777] ^= 1;
    check_block(d.substr(0, 1203));
  }
  {  // lines of text: the near candidate at work
    std::string d;
    for (int i = 0; d.size() < 4000; i++) d += "0000000" + std::to_string(1000 + 7 * i) + "\tgene" + std::to_string(i) + (i % 2 ? "_r\t" : "\t") + std::to_string(rng() % 9000) + "\n";
    check_block(d);
  }
  EXPECT(n_bad_reads == 0);
  // ---- round trips: every text of two letters up to 13 bytes, then sizes around the tiles and the chunks
  for (size_t n = 0; n <= 13; n++)
    for (uint32_t bits = 0; bits < (1u << n); bits++) {
      std::string d(n, 'A');
      for (size_t i = 0; i < n; i++)
        if (bits >> i & 1) d[i] = 'C';
      check_roundtrip(d);
    }
  for (unsigned nletters : {2u, 4u, 253u})
    for (size_t n : {255u, 256u, 257u, 1000u, 65535u, 65536u, 65537u, 140000u}) check_roundtrip(letters(rng, n, nletters));
  EXPECT(n_bad_reads == 0);
  // ---- the stored rule: a random part and a run behind it, on both sides of the threshold
  {
    const std::string head = letters(rng, 4000, 253);
    int first_kept = -1;
    bool monotone = true;
    for (int r = 0; r <= 1200; r++) {
      const std::string s = musc::sz_encode_compressed(head + std::string(r, 'Z'));
      const bool kept = s[10] == 0x00;
      if (kept && first_kept < 0) first_kept = r;
      if (!kept && first_kept >= 0) monotone = false;
    }
    EXPECT(first_kept > 0 && first_kept < 1200 && monotone);
    check_roundtrip(head + std::string(first_kept - 1, 'Z'));
    check_roundtrip(head + std::string(first_kept, 'Z'));
  }
}

}  // namespace

int main() {
  check_crc();
  check_compress();
  std::mt19937 rng(20240229);
  for (int s = 0; s < 12; s++) {
    std::string plain;
    const std::string stream = random_stream(rng, plain);
    EXPECT(musc::sz_decode(stream) == plain);
    check_mutations(stream);
  }
  // a declared length above a chunk's room: the plan refuses
  {
    std::string s, block;
    put_varint(block, 65537);
    put_chunk(s, 0x00, std::string(4, '\0') + block + std::string("\x00" "A", 2));
    ms::Plan plan;
    EXPECT(ms::sz_plan((const uint8_t*)s.data(), s.size(), plan) == ms::SZ_REFUSED && plan.bad_index == 0);
    check_stream(s);
  }
  EXPECT(n_refused > 0);
  EXPECT(n_thrown > n_streams / 2 && n_thrown < n_streams);
  char census[160];
  snprintf(census, sizeof census, "%llu streams, %llu rejected, %llu refused; %llu blocks restated, %llu round trips", n_streams, n_thrown, n_refused,
           n_blocks, n_roundtrips);
  return check_done("sz_plan_check", census);
}
