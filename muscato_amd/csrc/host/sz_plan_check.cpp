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
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <string>
#include <vector>

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

}  // namespace

int main() {
  check_crc();
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
  char census[96];
  snprintf(census, sizeof census, "%llu streams, %llu rejected, %llu refused", n_streams, n_thrown, n_refused);
  return check_done("sz_plan_check", census);
}
