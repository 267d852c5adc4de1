// kernels_sz.hpp -- framed snappy on the GPU.  Included by muscato_hip.hip behind kernels_fastq.hpp, whose
// aligned 16-byte loads it reuses.  The chunk table comes from sz_plan (sz_plan.hpp), on the host.
//
// k_sz_decode: one workgroup per data chunk.  The chunk's output, at most 65 536 bytes, is built in LDS: a copy element
// reads bytes that an earlier element of the same chunk wrote, and LDS orders those accesses inside a workgroup with a
// barrier and no cache argument.  With the 4 KiB window of the body and the CRC table a workgroup holds 70 KiB, so a CU
// (160 KiB) takes two chunks.
//   - The tag walk is uniform over the workgroup: every lane reads the same tag and operand bytes from the window.
//   - A literal is a cooperative copy from the body; a copy element is out[pos + i] = out[pos - off + i mod off], i < len,
//     whose sources all lie before pos -- the overlapping (run-length) form is as parallel as the plain one.  A barrier
//     is needed only where a copy reads what was written since the last one (dirty_lo).
//   - Every element is checked before a byte of it is written: operand bytes inside the body, the literal inside the body
//     and inside the declared length, 1 <= off <= pos, pos + len <= the declared length; a chunk ends with pos == the
//     declared length.  So a chunk reads nothing outside [body, body + body_len) and writes nothing outside
//     [out_off, out_off + ulen), whatever its bytes say.  The first check that fails is the chunk's status (sz.hpp's
//     decoder, which appends first and compares lengths last, may name a later one).
//   - CRC-32C from LDS: each lane takes a slice of an odd number of dwords (no two lanes of a wave on one bank), the
//     slices' CRCs are joined by multiplication by x^(8 bytes behind the slice) mod P (sz_plan.hpp), masked as mask_crc
//     does and compared with the stored word.
//   - Only then is the chunk written out: whole dwords where the output address allows, bytes at the edges.

#include "sz_compress_plan.hpp"

#define SZ_BLOCK 256u
#define SZ_WIN_UNITS 256u  // 16-byte units of the body window

struct SzChunkDev {
  uint64_t body;     // offset in the stream
  uint64_t out_off;  // offset in the output
  uint32_t body_len, ulen, crc, type;
};

DEV uint32_t sz_gf2_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
#pragma unroll 8
  for (uint32_t m = 0x80000000u; m; m >>= 1) {
    p ^= (a & m) ? b : 0u;
    b = (b >> 1) ^ ((b & 1u) ? 0x82F63B78u : 0u);
  }
  return p;
}

// ---- CRC-32C by parts, for the three chunk kernels (k_sz_decode and k_sz_compress from LDS, k_sz_frame from global
// memory): the byte table's set-up, a lane's slice and its place in the whole, and the join over a workgroup of 256

DEV void sz_crc_table(uint32_t* __restrict__ s_tab, uint32_t tid) {  // tid < 256; a barrier before the first use
  uint32_t c = tid;
#pragma unroll
  for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ 0x82F63B78u : c >> 1;
  s_tab[tid] = c;
}

// Lane tid's term of the CRC of `ulen` bytes cut into `lanes` slices of an odd number of dwords: the CRC of its slice
// times x^(8 * bytes behind the slice) mod P; the terms' XOR is the CRC of the whole.  dw(i) = the four bytes at offset
// i (a multiple of four, i + 4 <= ulen), by(i) = the byte at offset i.
template <class DW, class BY>
DEV uint32_t sz_crc_slice(uint32_t ulen, uint32_t tid, uint32_t lanes, const uint32_t* __restrict__ s_tab,
                          const uint32_t* __restrict__ x2n, DW dw, BY by) {
  const uint32_t sd = ((ulen + 4 * lanes - 1) / (4 * lanes)) | 1u;  // dwords per slice, odd
  const uint32_t b0 = tid * sd * 4;
  const uint32_t b1 = b0 + sd * 4 < ulen ? b0 + sd * 4 : ulen;
  if (b0 >= ulen) return 0;
  uint32_t c = 0xFFFFFFFFu;
  uint32_t i = b0;
  for (; i + 4 <= b1; i += 4) {
    uint32_t v = dw(i);
#pragma unroll
    for (int k = 0; k < 4; k++, v >>= 8) c = s_tab[(c ^ v) & 0xFFu] ^ (c >> 8);
  }
  for (; i < b1; i++) c = s_tab[(c ^ by(i)) & 0xFFu] ^ (c >> 8);
  c ^= 0xFFFFFFFFu;
  uint32_t m = 0x80000000u;
  uint32_t behind = ulen - b1;
  for (uint32_t k = 3; behind; behind >>= 1, k++)
    if (behind & 1u) m = sz_gf2_mul(x2n[k], m);
  return sz_gf2_mul(m, c);
}

// the XOR of the 256 lanes' terms, masked as mask_crc does (one barrier inside; s_red: a word per wave, free again
// once every lane is past the next barrier)
DEV uint32_t sz_crc_join(uint32_t c, uint32_t* __restrict__ s_red, uint32_t tid) {
#pragma unroll
  for (int d = 32; d; d >>= 1) c ^= __shfl_xor(c, d);
  if ((tid & 63u) == 0) s_red[tid >> 6] = c;
  __syncthreads();
  c = 0;
#pragma unroll
  for (uint32_t k = 0; k < 4; k++) c ^= s_red[k];
  return ((c >> 15) | (c << 17)) + 0xa282ead8u;
}

// stream16 = the stream's address rounded down to 16, slo = the stream's first byte in that space.  dst == nullptr: decode
// and check only.  status[chunk] = musc_sz::Status.
MUSC_KERNEL __launch_bounds__(SZ_BLOCK) void k_sz_decode(const unsigned char* __restrict__ stream16, uint64_t slo,
                                                        const SzChunkDev* __restrict__ chunks, uint32_t nchunks,
                                                        const uint32_t* __restrict__ x2n, unsigned char* __restrict__ dst,
                                                        uint32_t* __restrict__ status) {
  __shared__ uint32_t s_out[65536 / 4];
  __shared__ uint4 s_win[SZ_WIN_UNITS];
  __shared__ uint32_t s_tab[256];
  __shared__ uint32_t s_red[SZ_BLOCK / 64];
  unsigned char* const out = reinterpret_cast<unsigned char*>(s_out);
  const unsigned char* const win = reinterpret_cast<const unsigned char*>(s_win);
  const uint32_t tid = threadIdx.x;
  sz_crc_table(s_tab, tid);
  for (uint32_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    const SzChunkDev C = chunks[ch];
    const uint64_t lo = slo + C.body, hi = lo + C.body_len;  // the body in the aligned address space
    const uint32_t n = C.body_len, ulen = C.ulen;
    uint32_t st = 0;
    __syncthreads();  // (the previous chunk's output and window are done with)
    if (C.type == 1) {
      for (uint32_t i = tid; i < ulen; i += SZ_BLOCK) out[i] = stream16[lo + i];
    } else {
      uint32_t p = 0, pos = 0, dirty_lo = 0;
      uint64_t win_j = ~0ull;  // first unit in the window; none yet
      while (p < n) {
        // the tag and its operand bytes (at most five) in the window
        const uint64_t a = lo + p;
        if (win_j == ~0ull || a < win_j * 16 || a + 5 > (win_j + SZ_WIN_UNITS) * 16) {
          __syncthreads();
          win_j = a / 16;
          if ((win_j + tid) * 16 < hi) s_win[tid] = fq_load16(stream16, win_j + tid, lo, hi);
          __syncthreads();
          dirty_lo = pos;
        }
        const unsigned char* w = win + (a - win_j * 16);
        const uint32_t tag = w[0], t = tag & 3u;
        uint32_t len, off = 0;
        p++;
        if (t == 0) {
          uint64_t l = tag >> 2;
          if (l >= 60) {
            const uint32_t nb = (uint32_t)l - 59;
            if (nb > n - p) { st = musc_sz::ST_TRUNC_LITLEN; break; }
            l = 0;
            for (uint32_t i = 0; i < nb; i++) l |= (uint64_t)w[1 + i] << (8 * i);
            p += nb;
          }
          l += 1;
          if (l > n - p) { st = musc_sz::ST_TRUNC_LITERAL; break; }
          if (l > ulen - pos) { st = musc_sz::ST_LENGTH; break; }
          len = (uint32_t)l;
          for (uint32_t i = tid; i < len; i += SZ_BLOCK) out[pos + i] = stream16[lo + p + i];
          p += len;
        } else {
          const uint32_t nb = t == 1 ? 1u : t == 2 ? 2u : 4u;
          if (nb > n - p) { st = musc_sz::ST_TRUNC_COPY; break; }
          if (t == 1) {
            len = ((tag >> 2) & 7u) + 4;
            off = ((tag >> 5) << 8) | w[1];
          } else {
            len = (tag >> 2) + 1;
            off = w[1] | ((uint32_t)w[2] << 8);
            if (t == 3) off |= ((uint32_t)w[3] << 16) | ((uint32_t)w[4] << 24);
          }
          p += nb;
          if (off == 0 || off > pos) { st = musc_sz::ST_BAD_OFFSET; break; }
          if (len > ulen - pos) { st = musc_sz::ST_LENGTH; break; }
          const uint32_t src = pos - off, src_end = src + (off < len ? off : len);
          if (src_end > dirty_lo) {  // reads what was written since the last barrier
            __syncthreads();
            dirty_lo = pos;
          }
          if (tid < len) out[pos + tid] = out[src + tid % off];  // (len <= 64)
        }
        pos += len;
      }
      if (st == 0 && pos != ulen) st = musc_sz::ST_LENGTH;
    }
    __syncthreads();

    // ---- CRC-32C of out[0, ulen)
    if (st == 0) {
      const uint32_t c = sz_crc_slice(ulen, tid, SZ_BLOCK, s_tab, x2n, [&](uint32_t i) { return s_out[i >> 2]; },
                                      [&](uint32_t i) { return (uint32_t)out[i]; });
      const uint32_t masked = sz_crc_join(c, s_red, tid);
      if (masked != C.crc) st = musc_sz::ST_CHECKSUM;
    }
    if (tid == 0) status[ch] = st;

    // ---- the chunk's bytes to dst + out_off: whole dwords where the address allows, bytes at the edges
    if (st == 0 && dst) {
      unsigned char* const d = dst + C.out_off;
      const uint32_t mis = (4u - ((uint32_t)(uintptr_t)d & 3u)) & 3u;
      const uint32_t head = mis < ulen ? mis : ulen;
      const uint32_t nd = (ulen - head) >> 2;
      for (uint32_t k = tid; k < nd; k += SZ_BLOCK) {
        const uint32_t q = head + 4 * k;
        uint32_t v;
        if (head == 0) v = s_out[k];
        else v = __builtin_amdgcn_alignbyte(s_out[(q >> 2) + 1], s_out[q >> 2], head);
        *reinterpret_cast<uint32_t*>(d + q) = v;
      }
      const uint32_t tail0 = head + 4 * nd;
      if (tid < head) d[tid] = out[tid];
      else if (tid >= 4 && tail0 + (tid - 4) < ulen) d[tail0 + (tid - 4)] = out[tail0 + (tid - 4)];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// The compressing writer.  The rule is sz_compress_plan.hpp's, whose per-position functions run here as
// they run on the host; this file adds the lanes.
//
// k_sz_compress: one workgroup of 256 lanes per chunk of 65 536 bytes, on a persistent grid.  The chunk (64 KiB), the
// hash table (16 384 words, 64 KiB) and the tile's own table (4 096 words, 16 KiB) are in LDS: 148 KiB with the small
// arrays, one workgroup per CU (160 KiB).  The chunk comes in by the aligned 16-byte loads of kernels_fastq.hpp, two per
// lane joined by a funnel shift where the text's address is no multiple of 16, the edges byte by byte: nothing outside
// [src, src + nbytes) is read.  Per tile of 256 positions, a lane per position (five barriers):
//   1. the lane's four bytes, their hash; its entry goes to the tile's own table (LDS max)            -- barrier
//   2. both look-ups and the extension (position_match: dwords from LDS, count of trailing zeros)     -- barrier
//   3. the hash table takes the tile's positions (LDS max); wave 0 picks the greedy parse among the tile's matches:
//      four ballots, then one round per copy -- the next match at or behind the parse's position, found in the four
//      words, its length read from the wave's registers by lane number; at most 64 rounds, a copy being four bytes
//      or more, and no memory access in a round.  It carries the end of the last copy across tiles (a copy may end in
//      the next one).
//                                                                                                    -- barrier
//   4. a lane per chosen position: where the literal run in front of it began (the end of the chosen position before
//      it, or what was carried in), the bytes of its literal head, its literal and its copy; a workgroup scan makes
//      them offsets in the block; the head and the copy are written                        -- a barrier in the scan, one after
//   5. a lane per position: a literal byte finds the copy that ends its run (the next chosen position in the four
//      words) and goes to its place.  The part of a run that lies in earlier tiles is copied by all lanes when the
//      run ends; the last run when the chunk does.
// The block goes to the chunk's slot of a scratch buffer (stride 8 + 65 536) through a guard that drops what lies at
// or beyond n - n / 8, which no kept block reaches.  Then the CRC from LDS (the slices of k_sz_decode), the eight header
// bytes, the stored form over the block where the rule says so, and the chunk's length.
// Every loop has its bound in the code: tiles <= 256, rounds <= 64, extension <= 16 dwords, cooperative copies
// <= 65 536 / 256 steps.  No workgroup waits for another.
//
// k_sz_gather: after an exclusive scan of the lengths, chunk i moves from its slot to dst + 10 + off[i] (dst at any
// alignment: whole dwords where the address allows, bytes at the edges); the workgroup of chunk 0 writes the identifier.

#define SZC_BLOCK 256u

struct SzcLds {  // the reader of sz_compress_plan.hpp over the chunk in LDS
  const uint32_t* dw;
  DEV uint32_t operator()(uint32_t k) const { return dw[k]; }
};
struct SzcGuard {  // its writer: the block in the chunk's slot
  unsigned char* p;
  uint32_t cap;
  DEV void operator()(uint32_t at, uint8_t b) const {
    if (at < cap) p[at] = b;
  }
};

// bytes [s, s + 16) of the 32 bytes a | b, s < 16 (wave-uniform)
DEV uint4 sz_funnel16(uint4 a, uint4 b, uint32_t s) {
  const uint32_t q = s >> 2, r = s & 3u;
  uint32_t w0 = a.x, w1 = a.y, w2 = a.z, w3 = a.w, w4 = b.x;
  if (q == 1) w0 = a.y, w1 = a.z, w2 = a.w, w3 = b.x, w4 = b.y;
  else if (q == 2) w0 = a.z, w1 = a.w, w2 = b.x, w3 = b.y, w4 = b.z;
  else if (q == 3) w0 = a.w, w1 = b.x, w2 = b.y, w3 = b.z, w4 = b.w;
  uint4 v;
  v.x = __builtin_amdgcn_alignbyte(w1, w0, r);
  v.y = __builtin_amdgcn_alignbyte(w2, w1, r);
  v.z = __builtin_amdgcn_alignbyte(w3, w2, r);
  v.w = __builtin_amdgcn_alignbyte(w4, w3, r);
  return v;
}

// the first set bit at or behind `from` in the 256 bits a0 .. a3 (a0 the lowest), 256 without one
DEV uint32_t sz_next_bit(unsigned long long a0, unsigned long long a1, unsigned long long a2, unsigned long long a3, uint32_t from) {
  uint32_t r = 256;
#pragma unroll
  for (int k = 3; k >= 0; k--) {
    const uint32_t lo = 64u * (uint32_t)k;
    const unsigned long long w = k == 0 ? a0 : k == 1 ? a1 : k == 2 ? a2 : a3;
    if (from < lo + 64) {
      const unsigned long long m = from > lo ? w & (~0ull << (from - lo)) : w;
      if (m) r = lo + (uint32_t)__builtin_ctzll(m);
    }
  }
  return r;
}

// the last set bit in front of `below` (< 256) in the 256 bits a0 .. a3, 256 without one
DEV uint32_t sz_prev_bit(unsigned long long a0, unsigned long long a1, unsigned long long a2, unsigned long long a3, uint32_t below) {
  uint32_t r = 256;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uint32_t lo = 64u * (uint32_t)k;
    const unsigned long long w = k == 0 ? a0 : k == 1 ? a1 : k == 2 ? a2 : a3;
    if (below > lo) {
      const unsigned long long m = below >= lo + 64 ? w : w & ~(~0ull << (below - lo));
      if (m) r = lo + 63u - (uint32_t)__builtin_clzll(m);
    }
  }
  return r;
}

// src16 = the text's address rounded down to 16, lo = the text's first byte in that space.  slots: nchunks slots of
// musc_szc::SLOT bytes, 8-byte aligned; lens[chunk] = the bytes of the chunk in the stream, its header included.
MUSC_KERNEL __launch_bounds__(SZC_BLOCK) void k_sz_compress(const unsigned char* __restrict__ src16, uint64_t lo, uint64_t nbytes,
                                                           uint64_t nchunks, const uint32_t* __restrict__ x2n,
                                                           unsigned char* __restrict__ slots, uint64_t* __restrict__ lens) {
  namespace zc = musc_szc;
  __shared__ uint4 s_in4[zc::CHUNK / 16 + 1];  // (>= IN_DWORDS dwords)
  __shared__ uint32_t s_far[zc::TABLE];
  __shared__ uint32_t s_near[zc::NEAR_TABLE];
  __shared__ uint32_t s_match[zc::TILE_POS];  // position_match of the tile's positions
  __shared__ uint32_t s_ls[zc::TILE_POS];     // of a chosen position: where the literal run in front of it began
  __shared__ uint32_t s_data[zc::TILE_POS];   // of a chosen position: where that run's bytes go in the block
  __shared__ unsigned long long s_sel[4];  // the chosen positions of the tile
  __shared__ uint32_t s_carry;             // the end of the last copy, after the tile
  __shared__ uint32_t s_lsin;              // ... and before it
  __shared__ uint32_t s_wsum[SZC_BLOCK / 64];
  __shared__ uint32_t s_tab[256];
  __shared__ uint32_t s_red[SZC_BLOCK / 64];
  static_assert(sizeof(uint4) * (zc::CHUNK / 16 + 1) >= 4 * zc::IN_DWORDS, "the chunk and its two spare dwords");
  uint32_t* const s_in = reinterpret_cast<uint32_t*>(s_in4);
  const SzcLds rd{s_in};
  const uint32_t tid = threadIdx.x;
  sz_crc_table(s_tab, tid);
  const uint64_t hi = lo + nbytes;
  for (uint64_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    const uint32_t n = zc::chunk_len(nbytes, ch);
    unsigned char* const slot = slots + ch * zc::SLOT;
    const SzcGuard w{slot + zc::HEAD, n - n / 8};
    __syncthreads();  // (the previous chunk's LDS is done with; s_tab is set)
    {
      const uint64_t a0 = lo + ch * zc::CHUNK, u0 = a0 >> 4;
      const uint32_t s = (uint32_t)a0 & 15u;
      for (uint32_t k = tid; 16 * k < n; k += SZC_BLOCK) {  // (at most 16 steps)
        const uint4 a = fq_load16(src16, u0 + k, lo, hi);
        uint4 b = make_uint4(0, 0, 0, 0);
        if (s != 0 && (u0 + k + 1) * 16 < hi) b = fq_load16(src16, u0 + k + 1, lo, hi);
        s_in4[k] = sz_funnel16(a, b, s);
      }
      for (uint32_t h = tid; h < zc::TABLE; h += SZC_BLOCK) s_far[h] = 0;
      for (uint32_t h = tid; h < zc::NEAR_TABLE; h += SZC_BLOCK) s_near[h] = 0;
    }
    __syncthreads();

    uint32_t o = zc::varint_size(n);  // the block's bytes so far (every lane's copy)
    if (tid == 0) zc::put_varint(w, 0, n);
    uint32_t ls = 0;  // wave 0: the end of the last copy = where the literal run in hand began
    const uint32_t ntiles = (n + zc::TILE_POS - 1) / zc::TILE_POS;
    for (uint32_t tile = 0; tile < ntiles; tile++) {  // (at most 256)
      const uint32_t T = tile * zc::TILE_POS, i = T + tid;
      const bool has4 = i + 4 <= n;
      uint32_t h = 0;
      if (has4) {
        h = zc::hash4(zc::load32(rd, i));
        atomicMax(&s_near[zc::near_key(h)], zc::near_entry(tile, tid));
      }
      __syncthreads();
      const uint32_t mm = has4 ? zc::position_match(rd, s_far[h], s_near[zc::near_key(h)], tile, i, n) : 0u;
      s_match[tid] = mm;
      __syncthreads();
      if (has4) atomicMax(&s_far[h], i + 1);
      if (tid < 64) {  // ---- the parse
        const unsigned long long m0 = __ballot(s_match[tid] != 0), m1 = __ballot(s_match[tid + 64] != 0),
                                 m2 = __ballot(s_match[tid + 128] != 0), m3 = __ballot(s_match[tid + 192] != 0);
        unsigned long long e0 = 0, e1 = 0, e2 = 0, e3 = 0;
        // the tile's match lengths in this wave's registers (lane l: positions l, l + 64, l + 128, l + 192), so that a
        // round reads one by lane number and touches no memory: the whole loop is scalar
        const uint32_t len0 = s_match[tid] >> 16, len1 = s_match[tid + 64] >> 16, len2 = s_match[tid + 128] >> 16, len3 = s_match[tid + 192] >> 16;
        const uint32_t ls_in = __builtin_amdgcn_readfirstlane(ls);
        uint32_t q = ls_in > T ? ls_in - T : 0, end = ls_in;
        for (uint32_t round = 0; round < zc::TILE_POS / zc::MIN_MATCH; round++) {
          const uint32_t pos = sz_next_bit(m0, m1, m2, m3, q);
          if (pos >= zc::TILE_POS) break;
          const uint32_t lane = pos & 63u;
          const uint32_t r0 = __builtin_amdgcn_readlane(len0, lane), r1 = __builtin_amdgcn_readlane(len1, lane),
                         r2 = __builtin_amdgcn_readlane(len2, lane), r3 = __builtin_amdgcn_readlane(len3, lane);
          const uint32_t len = pos < 64 ? r0 : pos < 128 ? r1 : pos < 192 ? r2 : r3;
          const unsigned long long bit = 1ull << lane;
          if (pos < 64) e0 |= bit;
          else if (pos < 128) e1 |= bit;
          else if (pos < 192) e2 |= bit;
          else e3 |= bit;
          q = pos + len;
          end = T + q;
        }
        ls = end;
        if (tid == 0) {
          s_sel[0] = e0, s_sel[1] = e1, s_sel[2] = e2, s_sel[3] = e3;
          s_lsin = ls_in;
          s_carry = end;
        }
      }
      __syncthreads();
      // ---- the elements: sizes, places, heads and copies
      const unsigned long long e0 = s_sel[0], e1 = s_sel[1], e2 = s_sel[2], e3 = s_sel[3];
      const unsigned long long mine = tid < 64 ? e0 : tid < 128 ? e1 : tid < 192 ? e2 : e3;
      const bool chosen = (mine >> (tid & 63u)) & 1ull;
      uint32_t L = 0, sz = 0;
      if (chosen) {
        // the run in front of a copy began where the copy before it ended, the tile's first at what wave 0 carried in
        const uint32_t prev = sz_prev_bit(e0, e1, e2, e3, tid);
        const uint32_t l0 = prev < zc::TILE_POS ? T + prev + (s_match[prev] >> 16) : s_lsin;
        s_ls[tid] = l0;
        L = i - l0;
        sz = zc::lit_head_size(L) + L + zc::copy_size(mm & 0xFFFFu, mm >> 16);
      }
      uint32_t incl = sz;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d);
        if ((tid & 63u) >= (uint32_t)d) incl += up;
      }
      if ((tid & 63u) == 63u) s_wsum[tid >> 6] = incl;
      __syncthreads();
      uint32_t before = 0, total = 0;
#pragma unroll
      for (uint32_t k = 0; k < SZC_BLOCK / 64; k++) {
        const uint32_t ws = s_wsum[k];
        if (k < (tid >> 6)) before += ws;
        total += ws;
      }
      if (chosen) {
        uint32_t at = o + before + incl - sz;
        if (L) at += zc::put_lit_head(w, at, L);
        s_data[tid] = at;
        zc::put_copy(w, at + L, mm & 0xFFFFu, mm >> 16);
      }
      o += total;
      __syncthreads();
      // ---- the literal bytes
      if (!chosen && i < n) {
        const uint32_t nq = sz_next_bit(e0, e1, e2, e3, tid + 1);
        if (nq < zc::TILE_POS) {
          const uint32_t l0 = s_ls[nq];
          if (i >= l0) w(s_data[nq] + (i - l0), (uint8_t)zc::load8(rd, i));
        }
      }
      const uint32_t fq = sz_next_bit(e0, e1, e2, e3, 0);
      if (fq < zc::TILE_POS) {
        const uint32_t l0 = s_ls[fq], d0 = s_data[fq];
        for (uint32_t b = l0 + tid; b < T; b += SZC_BLOCK) w(d0 + (b - l0), (uint8_t)zc::load8(rd, b));  // (at most 256 steps)
      }
      // (no barrier here: the next tile writes s_match, s_sel, s_lsin, s_ls, s_data and s_wsum behind its own first
      // barrier or a later one, which no lane passes before every lane has read them above)
    }
    {  // ---- the last literal run
      const uint32_t l0 = s_carry;
      if (l0 < n) {
        const uint32_t L = n - l0, hs = zc::lit_head_size(L);
        if (tid == 0) zc::put_lit_head(w, o, L);
        for (uint32_t b = l0 + tid; b < n; b += SZC_BLOCK) w(o + hs + (b - l0), (uint8_t)zc::load8(rd, b));  // (at most 256 steps)
        o += hs + L;
      }
    }
    // ---- the CRC of the plain bytes, the header, the stored form
    const uint32_t c = sz_crc_slice(n, tid, SZC_BLOCK, s_tab, x2n, [&](uint32_t i) { return s_in[i >> 2]; },
                                    [&](uint32_t i) { return zc::load8(rd, i); });
    const uint32_t masked = sz_crc_join(c, s_red, tid);  // (its barrier: the block's bytes are written before the stored form goes over them)
    const bool keep = !zc::stored(o, n);
    const uint32_t body = keep ? o : n;
    if (tid < 8) {
      const uint32_t len = body + 4;
      slot[tid] = tid == 0 ? (unsigned char)(keep ? 0x00 : 0x01) : tid < 4 ? (unsigned char)(len >> (8 * (tid - 1))) : (unsigned char)(masked >> (8 * (tid - 4)));
    }
    if (!keep) {
      uint32_t* const d32 = reinterpret_cast<uint32_t*>(slot + zc::HEAD);  // (slots are 8-byte aligned)
      for (uint32_t k = tid; 4 * k < n; k += SZC_BLOCK) {  // (at most 64 steps)
        if (4 * k + 4 <= n) d32[k] = s_in[k];
        else
          for (uint32_t b = 4 * k; b < n; b++) slot[zc::HEAD + b] = (unsigned char)zc::load8(rd, b);
      }
    }
    if (tid == 0) lens[ch] = zc::HEAD + body;
  }
}

// off = the exclusive scan of k_sz_compress's lens (nchunks + 1 elements); dst at any alignment
MUSC_KERNEL __launch_bounds__(SZC_BLOCK) void k_sz_gather(const unsigned char* __restrict__ slots, const uint64_t* __restrict__ off,
                                                         uint64_t nchunks, unsigned char* __restrict__ dst) {
  namespace zc = musc_szc;
  const uint32_t tid = threadIdx.x;
  if (blockIdx.x == 0 && tid < 10)  // ff 06 00 00 "sNaPpY", as k_sz_frame writes it
    dst[tid] = tid < 8 ? (unsigned char)(0x50614e73000006ffull >> (8 * tid)) : (unsigned char)(0x5970u >> (8 * (tid - 8)));
  for (uint64_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    const unsigned char* const s = slots + ch * zc::SLOT;
    const uint32_t* const s32 = reinterpret_cast<const uint32_t*>(s);
    const uint32_t len = (uint32_t)(off[ch + 1] - off[ch]);  // <= SLOT
    unsigned char* const d = dst + zc::MAGIC + off[ch];
    const uint32_t mis = (4u - ((uint32_t)(uintptr_t)d & 3u)) & 3u;
    const uint32_t head = mis < len ? mis : len;
    const uint32_t nd = (len - head) >> 2;
    for (uint32_t k = tid; k < nd; k += SZC_BLOCK) {  // (at most 65 steps)
      const uint32_t q = head + 4 * k;
      uint32_t v;
      if (head == 0) v = s32[k];
      else v = __builtin_amdgcn_alignbyte(s32[(q >> 2) + 1], s32[q >> 2], head);  // (the dword behind a slot's last: inside the buffer's spare bytes)
      *reinterpret_cast<uint32_t*>(d + q) = v;
    }
    const uint32_t tail0 = head + 4 * nd;
    if (tid < head) d[tid] = s[tid];
    else if (tid >= 4 && tid < 8 && tail0 + (tid - 4) < len) d[tail0 + (tid - 4)] = s[tail0 + (tid - 4)];
  }
}
