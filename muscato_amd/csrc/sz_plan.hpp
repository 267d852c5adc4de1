// sz_plan.hpp -- the chunk table of a framed snappy stream, and CRC-32C by parts.  Plain C++, no HIP:
// included by muscato_hip.hip (musc_sz_decode, musc_db_load_text) and by host/sz_plan_check.cpp, the stand-alone
// program that holds both to host/sz.hpp's sz_decode and crc32c.
//
// sz_plan walks the 4-byte chunk headers once and takes every framing rule of sz_decode, with its messages: truncated
// header or chunk, the stream identifier (anywhere in the stream), a data chunk shorter than its checksum, chunk types
// 0x80-0xfe skipped, 0x02-0x7f an error, and the varint preamble of a compressed chunk (truncated length / bad length).
// What it adds is the refusal: a chunk that declares more than 65 536 uncompressed bytes, which the framing format
// forbids and k_sz_decode has no room for.
#pragma once

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace musc_sz {

constexpr uint32_t SZ_MAX_CHUNK = 65536;  // uncompressed bytes of one chunk (framing_format.txt, 4.2 and 4.3)
constexpr int SZ_OK = 0, SZ_REFUSED = 12, SZ_BAD = 13;  // the library's codes

// one data chunk (type 0x00 or 0x01); what k_sz_decode reads of the stream is [body, body + body_len) and nothing else
struct Chunk {
  uint64_t body;      // stream offset of the chunk's data: behind the checksum and, type 0x00, behind the varint
  uint64_t out_off;   // where its bytes go in the output: the running sum of ulen
  uint32_t body_len;  // bytes of data
  uint32_t ulen;      // uncompressed length: the varint (0x00) or body_len (0x01)
  uint32_t crc;       // the stored word: mask_crc(crc32c(uncompressed bytes))
  uint32_t type;      // 0 compressed, 1 uncompressed
  uint64_t index;     // number of the chunk in the stream, counting every chunk from 0
  uint64_t block;     // stream offset of what follows the checksum (type 0x00: the varint first), block_len bytes
  uint32_t block_len;
};

struct Plan {
  std::vector<Chunk> chunks;
  uint64_t n_out = 0;
  uint64_t bad_index = 0;  // the chunk a non-zero result speaks of
  std::string msg;         // sz.hpp's message, or the refusal's
};

inline int sz_plan(const uint8_t* p, uint64_t n, Plan& plan) {
  plan = Plan();
  uint64_t pos = 0, index = 0;
  auto bad = [&](int code, const char* msg) {
    plan.bad_index = index;
    plan.msg = msg;
    return code;
  };
  for (; pos < n; index++) {
    if (pos + 4 > n) return bad(SZ_BAD, "sz: truncated chunk header");
    const uint8_t type = p[pos];
    const uint64_t len = p[pos + 1] | ((uint64_t)p[pos + 2] << 8) | ((uint64_t)p[pos + 3] << 16);
    pos += 4;
    if (pos + len > n) return bad(SZ_BAD, "sz: truncated chunk");
    const uint8_t* body = p + pos;
    const uint64_t at = pos;
    pos += len;
    if (type == 0xFF) {
      if (len != 6 || memcmp(body, "sNaPpY", 6) != 0) return bad(SZ_BAD, "sz: bad stream identifier");
    } else if (type == 0x00 || type == 0x01) {
      if (len < 4) return bad(SZ_BAD, "sz: chunk too short");
      Chunk c;
      c.crc = body[0] | ((uint32_t)body[1] << 8) | ((uint32_t)body[2] << 16) | ((uint32_t)body[3] << 24);
      c.type = type;
      c.index = index;
      c.out_off = plan.n_out;
      uint64_t q = 4, ulen = len - 4;
      if (type == 0x00) {
        ulen = 0;
        for (int shift = 0;;) {
          if (q >= len) return bad(SZ_BAD, "snappy: truncated length");
          const uint8_t b = body[q++];
          ulen |= (uint64_t)(b & 0x7F) << shift;
          if (b < 0x80) break;
          shift += 7;
          if (shift > 35) return bad(SZ_BAD, "snappy: bad length");
        }
      }
      if (ulen > SZ_MAX_CHUNK) return bad(SZ_REFUSED, "sz: a chunk declares more than 65536 uncompressed bytes");
      c.block = at + 4;
      c.block_len = (uint32_t)(len - 4);
      c.body = at + q;
      c.body_len = (uint32_t)(len - q);
      c.ulen = (uint32_t)ulen;
      plan.n_out += ulen;
      plan.chunks.push_back(c);
    } else if (type >= 0x80) {
      continue;  // skippable / padding
    } else {
      return bad(SZ_BAD, "sz: reserved unskippable chunk");
    }
  }
  return SZ_OK;
}

// ---- what a chunk's status word says (k_sz_decode writes it, plain C++ reads it)
enum Status : uint32_t {
  ST_OK = 0,
  ST_TRUNC_LITLEN,
  ST_TRUNC_LITERAL,
  ST_TRUNC_COPY,
  ST_BAD_OFFSET,
  ST_LENGTH,
  ST_CHECKSUM,
  ST_COUNT
};
inline const char* status_text(uint32_t s) {
  static const char* const T[ST_COUNT] = {"ok",
                                          "snappy: truncated literal length",
                                          "snappy: truncated literal",
                                          "snappy: truncated copy",
                                          "snappy: bad copy offset",
                                          "snappy: length mismatch",
                                          "sz: checksum mismatch"};
  return s < ST_COUNT ? T[s] : "sz: unknown status";
}

// The element walk of k_sz_decode in plain C++, statement for statement but for the lanes: every element is checked
// before a byte of it is written, and the first check that fails is the answer.  out gets the ulen bytes of a good
// block.  (host/sz_plan_check.cpp holds this to snappy_block_decode: one fails exactly when the other throws.)
inline uint32_t block_walk(const uint8_t* body, uint32_t n, uint32_t ulen, std::vector<uint8_t>& out) {
  out.assign(ulen, 0);
  uint32_t p = 0, pos = 0;
  while (p < n) {
    const uint32_t tag = body[p], t = tag & 3u;
    uint32_t len, off = 0;
    p++;
    if (t == 0) {
      uint64_t l = tag >> 2;
      if (l >= 60) {
        const uint32_t nb = (uint32_t)l - 59;
        if (nb > n - p) return ST_TRUNC_LITLEN;
        l = 0;
        for (uint32_t i = 0; i < nb; i++) l |= (uint64_t)body[p + i] << (8 * i);
        p += nb;
      }
      l += 1;
      if (l > n - p) return ST_TRUNC_LITERAL;
      if (l > ulen - pos) return ST_LENGTH;
      len = (uint32_t)l;
      for (uint32_t i = 0; i < len; i++) out[pos + i] = body[p + i];
      p += len;
    } else {
      const uint32_t nb = t == 1 ? 1u : t == 2 ? 2u : 4u;
      if (nb > n - p) return ST_TRUNC_COPY;
      if (t == 1) {
        len = ((tag >> 2) & 7u) + 4;
        off = ((tag >> 5) << 8) | body[p];
      } else {
        len = (tag >> 2) + 1;
        off = body[p] | ((uint32_t)body[p + 1] << 8);
        if (t == 3) off |= ((uint32_t)body[p + 2] << 16) | ((uint32_t)body[p + 3] << 24);
      }
      p += nb;
      if (off == 0 || off > pos) return ST_BAD_OFFSET;
      if (len > ulen - pos) return ST_LENGTH;
      for (uint32_t i = 0; i < len; i++) out[pos + i] = out[pos - off + i % off];
    }
    pos += len;
  }
  return pos == ulen ? ST_OK : ST_LENGTH;
}

// ---- CRC-32C by parts.  Polynomials over GF(2) in the reflected form a CRC register holds: bit 31 is x^0.
// crc(A || B) = crc(A) * x^(8 len(B)) + crc(B) (mod P), for the conditioned CRCs as they stand (zlib's crc32_combine).
constexpr uint32_t CRC32C_POLY = 0x82F63B78u;

inline uint32_t gf2_mul(uint32_t a, uint32_t b) {  // a * b mod P
  uint32_t p = 0;
  for (uint32_t m = 1u << 31; m; m >>= 1) {
    if (a & m) p ^= b;
    b = (b >> 1) ^ ((b & 1) ? CRC32C_POLY : 0);
  }
  return p;
}

// x2n[k] = x^(2^k) mod P
struct X2n {
  uint32_t t[32];
  X2n() {
    uint32_t p = 1u << 30;  // x^1
    t[0] = p;
    for (int k = 1; k < 32; k++) t[k] = p = gf2_mul(p, p);
  }
};

// x^(8 nbytes) mod P
inline uint32_t x8n(const uint32_t* x2n, uint64_t nbytes) {
  uint32_t p = 1u << 31;  // x^0
  for (int k = 3; nbytes; nbytes >>= 1, k = (k + 1) & 31)
    if (nbytes & 1) p = gf2_mul(x2n[k], p);
  return p;
}

inline uint32_t crc32c_combine(const uint32_t* x2n, uint32_t crc_a, uint32_t crc_b, uint64_t len_b) {
  return gf2_mul(x8n(x2n, len_b), crc_a) ^ crc_b;
}

}  // namespace musc_sz
