// load_plan.hpp -- the size rules of the loaders: the shape of the read records and its refusals, the
// words of the database planes and of the X-block bitmap, the schedule of a streamed load and the byte ranges of its
// pieces.  Plain C++, no HIP: included by muscato_hip.hip (muscato_load.hpp allocates and copies by what is decided
// here) and by host/load_plan_check.cpp, the stand-alone program that runs it under the sanitizers.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace musc_load {

// ---- read records: rw words each -- the 2-bit bases of the longest read, then the length word, rounded up to four
// words.  The refusals, in the order they are made (the caller words the message):
enum Refusal { SHAPE_OK = 0, TOO_MANY_READS, READ_TOO_LONG, TOO_MANY_WORDS };
struct RecShape { int rw = 4; uint64_t words = 0; };
inline Refusal rec_shape(uint64_t nreads, uint64_t maxlen, RecShape* s) {
  if (nreads >= 0xFFFFFFF0ull) return TOO_MANY_READS;  // (32-bit read_idx)
  if (maxlen > 65535) return READ_TOO_LONG;            // (16 bits of the length word)
  s->rw = std::max(((int)((2 * maxlen + 31) / 32) + 1 + 3) & ~3, 4);
  s->words = nreads * (uint64_t)s->rw;
  if (s->words >= (1ull << 32)) return TOO_MANY_WORDS;  // (one dispatch, a thread per word)
  return SHAPE_OK;
}

// ---- the database: 16 bases a word, DB_SLACK_WORDS zeroed words behind both planes (who reads into them: db_alloc),
// one bit of dbx per 64-base block of plane and slack
constexpr uint64_t DB_SLACK_WORDS = 64;
inline uint64_t db_words(uint64_t nbases) { return (nbases + 15) / 16; }
inline uint64_t db_plane_words(uint64_t words) { return words + DB_SLACK_WORDS; }
inline uint64_t dbx_blocks(uint64_t words) { return (db_plane_words(words) + 3) / 4; }
inline uint64_t dbx_words(uint64_t words) { return dbx_blocks(words) / 32 + 4; }

// ---- The read ranges of a streamed load (musc_reads_load_packed32 with async = 1) and of the pass that consumes it: the
// pieces the upload is queued in, and the batches the pass launches, every batch a whole number of pieces.  The upload
// is several times slower per read than the match, so the GPU idles through most of a streamed pass and what shows in
// its wall time is the work left after the last byte has landed: the pack and the match of the LAST batch.  Hence full
// batches (batch_reads, rounded up to whole wave-tiles) while at least two of them remain, then batches that take half
// of what is left each, down to a last batch of at most batch_reads / 16.  No batch holds more than twice the reads of
// the batch after it (give or take the rounding to 64), so the match of one batch ends well before the upload of the
// next one does, whatever the two rates are as long as the match is the faster one per read.  Every end but the last is
// a multiple of 64 reads: whole wave-tiles, and whole bytes of the 2-bit stream for any read length.
struct StreamPlan {
  std::vector<uint64_t> piece_end, batch_end;  // ascending; the last of each is the read count
};
inline void stream_plan(uint64_t nreads, uint64_t batch_reads, StreamPlan* sp) {
  auto up64 = [](uint64_t x) { return (x + 63) & ~63ull; };
  sp->piece_end.clear();
  sp->batch_end.clear();
  const uint64_t full = std::max<uint64_t>(up64(batch_reads), 64);
  const uint64_t last_max = std::max<uint64_t>(up64(batch_reads / 16), 64);
  const uint64_t piece = up64(std::max<uint64_t>(batch_reads / 4, 64));  // a quarter of a full batch
  for (uint64_t r0 = 0; r0 < nreads;) {
    const uint64_t left = nreads - r0;
    const uint64_t n = left >= 2 * full ? full : left <= last_max ? left : up64((left + 1) / 2);
    for (uint64_t p = r0 + piece; p < r0 + n; p += piece) sp->piece_end.push_back(p);
    r0 += n;
    sp->piece_end.push_back(r0);
    sp->batch_end.push_back(r0);
  }
}
// reads of the batch that starts at r0 on that schedule
inline uint64_t stream_plan_batch(const StreamPlan& sp, uint64_t r0) {
  const auto it = std::upper_bound(sp.batch_end.begin(), sp.batch_end.end(), r0);
  return it == sp.batch_end.end() ? 0 : *it - r0;
}

// ---- the 2-bit stream of nreads reads of L bases (reads_load_fixed): its bytes, the words of its staging buffer
// (k_pack_reads_fixed reads up to two words past a read's last; the last four are zeroed), and the bytes [b0, b1) of
// the piece of reads [r0, r1) -- 64 | r0, so b0 is a whole number of bytes
struct ByteRange { uint64_t b0, b1; };
inline uint64_t fixed_total_bytes(uint64_t nreads, uint32_t L) { return (nreads * (uint64_t)L + 3) / 4; }
inline uint64_t fixed_need_words(uint64_t total_bytes) { return (total_bytes + 3) / 4 + 4; }
inline ByteRange fixed_piece_bytes(uint64_t r0, uint64_t r1, uint32_t L, uint64_t total_bytes) {
  return ByteRange{r0 * (uint64_t)L / 4, std::min<uint64_t>((r1 * (uint64_t)L + 3) / 4, total_bytes)};
}

}  // namespace musc_load
