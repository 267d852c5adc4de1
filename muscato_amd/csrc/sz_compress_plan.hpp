// sz_compress_plan.hpp -- which bytes a chunk of a framed snappy stream compresses to.  Plain C++ that
// hipcc also compiles for the device: included by muscato_hip.hip (k_sz_compress in kernels_sz.hpp, musc_sz_compress),
// by host/sz.hpp (sz_encode_compressed, the host writer) and by host/sz_plan_check.cpp, the stand-alone program that
// holds the rule to a sequential restatement and to sz_decode.  tests/sz_compress_cases.py states the same rule in
// Python.  The output is a pure function of the input, so host and device agree byte for byte.
//
// The rule, for one chunk of n <= 65 536 bytes (the stream is chunks of 65 536 bytes, the last one shorter; an empty
// input is the ten identifier bytes alone):
//   Candidates.  The chunk is walked in tiles of TILE_POS = 256 positions.  A position i with i + 4 <= n hashes its four
//     bytes, hash4(le32) = (le32 * 0x1e35a7bd) >> 18, and reads the table entry as it stood after all EARLIER tiles.
//     After a tile's reads all its positions are inserted, the highest position winning (a max: the order inside a
//     tile does not matter).  An entry holds i + 1, 0 = empty.  A candidate j counts only if its four bytes equal
//     those at i (hashes collide).
//   The near candidate.  The table shows a position nothing of its own tile, and the best match of a line of text is
//     often the line before.  So every tile also notes, per 12-bit key (hash4 >> 2), the EARLIEST of its positions with
//     that key -- a min, again free of the order inside the tile -- and a position takes that one, if it lies in front
//     of it and its four bytes are equal, as a second candidate.  Of two matches the longer one is taken, the near one
//     when they are equal.  Both look-ups of a tile's 256 positions are independent of each other.
//   Match length.  The common extension of (j, i), which may overlap (j + m > i), ends at the chunk's end and is capped
//     at MAX_MATCH = 64: a match is exactly one copy element, and the work of a position is bounded (a run of one byte
//     over a whole chunk costs 16 dword comparisons per position, not 65 536).
//   Parse.  Greedy from the left: at p a match (>= 4 by construction) becomes a copy and p += len; otherwise p joins the
//     literal run and p += 1.  The last up to three positions have no four bytes and are literals.
//   Elements.  A literal of L bytes: L - 1 in the tag up to 59, beyond that one (L <= 256) or two length bytes.  A copy:
//     the 1-byte-offset form when len <= 11 and off < 2048, else the 2-byte form.
//   Chunk.  The block is varint(n) and the elements.  A block of >= n - n / 8 bytes is dropped and the chunk stored
//     (type 0x01): the rule of golang/snappy's writer (encode.go).  Either way the chunk carries the masked CRC-32C of
//     the plain bytes.  No chunk grows: sz_compress_bound(n) is the stored stream's size.
//
// The chunk is read as aligned dwords through a reader `rd(k)` = dword k of the chunk (the kernel: LDS; the host: a
// padded copy; the check program: a bounds-checked array).  No function here reads a dword beyond IN_DWORDS, and what
// a dword holds beyond byte n never decides anything.  Elements go out through a writer `w(at, byte)`.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define SZC_HD __host__ __device__ inline
#else
#define SZC_HD inline
#endif

namespace musc_szc {

constexpr uint32_t CHUNK = 65536;
constexpr uint32_t TILE_POS = 256;
constexpr uint32_t HASH_BITS = 14, TABLE = 1u << HASH_BITS;
constexpr uint32_t HASH_MUL = 0x1e35a7bdu;
constexpr uint32_t NEAR_BITS = 12, NEAR_TABLE = 1u << NEAR_BITS;  // the tile's own table
constexpr uint32_t MIN_MATCH = 4, MAX_MATCH = 64;
constexpr uint32_t IN_DWORDS = CHUNK / 4 + 2;  // the chunk and the dwords an unaligned read near its end may touch
constexpr uint64_t MAGIC = 10, HEAD = 8;       // the stream identifier; type, 3 length bytes, the masked CRC
constexpr uint64_t SLOT = HEAD + CHUNK;        // a chunk's room in the kernel's scratch buffer

SZC_HD uint64_t chunks(uint64_t nbytes) { return (nbytes + CHUNK - 1) / CHUNK; }
SZC_HD uint32_t chunk_len(uint64_t nbytes, uint64_t i) { return (uint32_t)(nbytes - i * CHUNK < CHUNK ? nbytes - i * CHUNK : CHUNK); }
// the most a stream of nbytes takes: every chunk stored (== musc_tp::sz_frame_size)
SZC_HD uint64_t sz_compress_bound(uint64_t nbytes) { return MAGIC + HEAD * chunks(nbytes) + nbytes; }

SZC_HD uint32_t hash4(uint32_t le32) { return (le32 * HASH_MUL) >> (32 - HASH_BITS); }

// The tile's own table needs no clearing between tiles: an entry is (tile + 1) << 8 | (255 - t) for position t of the
// tile, entries are joined by max, so a later tile's entry beats an earlier one's and within a tile the earliest position
// wins; 0 = empty.  near_pos: the position an entry names if it is of tile `tile`, else (and when empty) CHUNK.
SZC_HD uint32_t near_key(uint32_t hash) { return hash >> (HASH_BITS - NEAR_BITS); }
SZC_HD uint32_t near_entry(uint32_t tile, uint32_t t) { return ((tile + 1) << 8) | (TILE_POS - 1 - t); }
SZC_HD uint32_t near_pos(uint32_t entry, uint32_t tile) { return (entry >> 8) == tile + 1 ? tile * TILE_POS + (TILE_POS - 1 - (entry & 0xFFu)) : CHUNK; }

// the four bytes at byte position i, little endian (two aligned dwords: (i >> 2) + 1 < IN_DWORDS for every i < CHUNK + 4)
template <class R>
SZC_HD uint32_t load32(const R& rd, uint32_t i) {
  const uint64_t both = ((uint64_t)rd((i >> 2) + 1) << 32) | rd(i >> 2);
  return (uint32_t)(both >> (8 * (i & 3u)));
}
template <class R>
SZC_HD uint32_t load8(const R& rd, uint32_t i) { return (rd(i >> 2) >> (8 * (i & 3u))) & 0xFFu; }

// the common extension of (j, i), j < i, i < n: at most MAX_MATCH and at most n - i, by dwords (sixteen at the most)
template <class R>
SZC_HD uint32_t match_len(const R& rd, uint32_t j, uint32_t i, uint32_t n) {
  const uint32_t room = n - i, maxm = room < MAX_MATCH ? room : MAX_MATCH;
  for (uint32_t k = 0; k < MAX_MATCH; k += 4) {
    if (k >= maxm) break;
    const uint32_t x = load32(rd, i + k) ^ load32(rd, j + k);
    if (x) {
      const uint32_t m = k + ((uint32_t)__builtin_ctz(x) >> 3);
      return m < maxm ? m : maxm;
    }
  }
  return maxm;
}

// the match of position i (i + 4 <= n) against the candidate at j (j >= i: none): its length (>= 4), or 0 without one
template <class R>
SZC_HD uint32_t candidate_len(const R& rd, uint32_t j, uint32_t i, uint32_t n) {
  if (j >= i || load32(rd, j) != load32(rd, i)) return 0;
  return match_len(rd, j, i, n);
}

// What position i (i + 4 <= n) of tile `tile` makes of its two table entries: far = the hash table's (i' + 1 of an
// earlier tile, 0 = empty), near = the tile's own.  -> len << 16 | offset, 0 without a match (offset <= 65 532).
template <class R>
SZC_HD uint32_t position_match(const R& rd, uint32_t far, uint32_t near, uint32_t tile, uint32_t i, uint32_t n) {
  const uint32_t jf = far ? far - 1 : CHUNK, jn = near_pos(near, tile);
  const uint32_t mf = candidate_len(rd, jf, i, n), mn = candidate_len(rd, jn, i, n);
  if (mn >= MIN_MATCH && mn >= mf) return (mn << 16) | (i - jn);
  if (mf >= MIN_MATCH) return (mf << 16) | (i - jf);
  return 0;
}

// ---- element sizes and encoders
SZC_HD uint32_t varint_size(uint32_t n) { return n < 0x80u ? 1u : n < 0x4000u ? 2u : 3u; }  // n <= CHUNK
SZC_HD uint32_t lit_head_size(uint32_t L) { return L == 0 ? 0u : L <= 60 ? 1u : L <= 256 ? 2u : 3u; }  // L <= CHUNK
SZC_HD uint32_t copy_size(uint32_t off, uint32_t len) { return len <= 11 && off < 2048 ? 2u : 3u; }
SZC_HD bool stored(uint32_t block_bytes, uint32_t n) { return block_bytes >= n - n / 8; }

template <class W>
SZC_HD uint32_t put_varint(W& w, uint32_t at, uint32_t n) {
  const uint32_t s = varint_size(n);
  for (uint32_t k = 0; k < s; k++) w(at + k, (uint8_t)(((n >> (7 * k)) & 0x7Fu) | (k + 1 < s ? 0x80u : 0u)));
  return s;
}
template <class W>
SZC_HD uint32_t put_lit_head(W& w, uint32_t at, uint32_t L) {  // L >= 1; the L bytes follow
  const uint32_t s = lit_head_size(L), v = L - 1;
  if (s == 1) {
    w(at, (uint8_t)(v << 2));
  } else {
    w(at, (uint8_t)((59 + (s - 1)) << 2));
    w(at + 1, (uint8_t)(v & 0xFFu));
    if (s == 3) w(at + 2, (uint8_t)(v >> 8));
  }
  return s;
}
template <class W>
SZC_HD uint32_t put_copy(W& w, uint32_t at, uint32_t off, uint32_t len) {  // 4 <= len <= 64, 1 <= off < 65536
  if (copy_size(off, len) == 2) {
    w(at, (uint8_t)(1u | ((len - 4) << 2) | ((off >> 8) << 5)));
    w(at + 1, (uint8_t)(off & 0xFFu));
    return 2;
  }
  w(at, (uint8_t)(2u | ((len - 1) << 2)));
  w(at + 1, (uint8_t)(off & 0xFFu));
  w(at + 2, (uint8_t)(off >> 8));
  return 3;
}

// The rule in its tile form, in plain C++ (host only): the block of a chunk of n bytes (1 <= n <= CHUNK) read through
// rd goes out through w; the block's size comes back.  The caller decides by stored() what the chunk becomes; w may
// drop what lies at or beyond n - n / 8, which no kept block reaches.
template <class R, class W>
inline uint32_t chunk_block(const R& rd, uint32_t n, W& w) {
  static_assert(CHUNK - 4 + 1 <= 0xFFFFu, "an entry i + 1 fits 16 bits");
  uint16_t table[TABLE];
  for (uint32_t h = 0; h < TABLE; h++) table[h] = 0;
  uint32_t near[NEAR_TABLE];
  for (uint32_t k = 0; k < NEAR_TABLE; k++) near[k] = 0;
  uint32_t match[TILE_POS];  // position_match of the tile's positions
  uint32_t o = put_varint(w, 0, n), p = 0, ls = 0;  // p: the parse's position; ls: where the literal run in hand began
  for (uint32_t T = 0; T < n; T += TILE_POS) {
    const uint32_t tile = T / TILE_POS;
    for (uint32_t t = 0; t < TILE_POS && T + t + 4 <= n; t++) {
      uint32_t& e = near[near_key(hash4(load32(rd, T + t)))];
      if (e < near_entry(tile, t)) e = near_entry(tile, t);
    }
    for (uint32_t t = 0; t < TILE_POS; t++) {
      const uint32_t i = T + t;
      match[t] = 0;
      if (i + 4 > n) continue;
      const uint32_t h = hash4(load32(rd, i));
      match[t] = position_match(rd, table[h], near[near_key(h)], tile, i, n);
    }
    for (uint32_t t = 0; t < TILE_POS && T + t + 4 <= n; t++) {
      const uint32_t h = hash4(load32(rd, T + t));
      if (table[h] < T + t + 1) table[h] = (uint16_t)(T + t + 1);
    }
    while (p < T + TILE_POS && p < n) {
      const uint32_t len = match[p - T] >> 16;
      if (len < MIN_MATCH) {
        p++;
        continue;
      }
      if (ls < p) {
        o += put_lit_head(w, o, p - ls);
        for (; ls < p; ls++) w(o++, (uint8_t)load8(rd, ls));
      }
      o += put_copy(w, o, match[p - T] & 0xFFFFu, len);
      ls = p += len;
    }
  }
  if (ls < n) {
    o += put_lit_head(w, o, n - ls);
    for (; ls < n; ls++) w(o++, (uint8_t)load8(rd, ls));
  }
  return o;
}

}  // namespace musc_szc
