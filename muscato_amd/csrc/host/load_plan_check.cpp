// load_plan_check.cpp -- the size rules of the loaders (csrc/load_plan.hpp: the record shape and its refusals, the
// database's words, the schedule of a streamed load and the byte ranges of its pieces) against their properties, as a
// program of its own so that it runs under the sanitizers.
// It needs no GPU and is not part of the library; muscato_amd/build.py (CHECKS) builds it, plain and sanitized.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../load_plan.hpp"
#include "check.hpp"

namespace {

namespace ml = musc_load;

// ---- the record shape

void check_shape(uint64_t maxlen) {
  ml::RecShape s;
  EXPECT(ml::rec_shape(1000, maxlen, &s) == ml::SHAPE_OK);
  EXPECT(s.rw % 4 == 0 && s.rw >= 4);
  EXPECT((uint64_t)(s.rw - 1) * 32 >= 2 * maxlen);          // the bases, and the length word behind them
  EXPECT(s.rw == 4 || (uint64_t)(s.rw - 4 - 1) * 32 < 2 * maxlen);  // and no four words more than that takes
  EXPECT(s.words == 1000ull * (uint64_t)s.rw);
}

void check_refusals() {
  ml::RecShape s;
  // the read count: refused from 0xFFFFFFF0 on, whatever else holds (below it the word count refuses, not this)
  EXPECT(ml::rec_shape(0xFFFFFFF0ull, 0, &s) == ml::TOO_MANY_READS);
  EXPECT(ml::rec_shape(0xFFFFFFF0ull, 70000, &s) == ml::TOO_MANY_READS);
  EXPECT(ml::rec_shape(0xFFFFFFEFull, 0, &s) == ml::TOO_MANY_WORDS);
  // the length: 65 535 is a record, 65 536 is not
  EXPECT(ml::rec_shape(1, 65535, &s) == ml::SHAPE_OK && s.rw == 4100);
  EXPECT(ml::rec_shape(1, 65536, &s) == ml::READ_TOO_LONG);
  EXPECT(ml::rec_shape(0, 65536, &s) == ml::READ_TOO_LONG);  // (the length alone: what the sort asks before it sorts)
  // the words: 2^32 - 4 are a dispatch, 2^32 are not -- at the smallest stride and at a larger one
  EXPECT(ml::rec_shape((1ull << 30) - 1, 10, &s) == ml::SHAPE_OK && s.words == (1ull << 32) - 4);
  EXPECT(ml::rec_shape(1ull << 30, 10, &s) == ml::TOO_MANY_WORDS);
  EXPECT(ml::rec_shape((1ull << 29) - 1, 100, &s) == ml::SHAPE_OK && s.rw == 8);
  EXPECT(ml::rec_shape(1ull << 29, 100, &s) == ml::TOO_MANY_WORDS);
  EXPECT(ml::rec_shape(0, 0, &s) == ml::SHAPE_OK && s.rw == 4 && s.words == 0);
}

// ---- the database's words

void check_db(uint64_t nbases) {
  const uint64_t w = ml::db_words(nbases);
  EXPECT(w * 16 >= nbases && (w == 0 || (w - 1) * 16 < nbases));
  EXPECT(ml::db_plane_words(w) == w + 64);
  const uint64_t blocks = ml::dbx_blocks(w);
  EXPECT(blocks * 4 >= ml::db_plane_words(w) && (blocks - 1) * 4 < ml::db_plane_words(w));  // a bit for every word of plane and slack
  // db_span_has_x reads the bitmap word of a span's first block and the one behind it
  EXPECT(ml::dbx_words(w) > (blocks - 1) / 32 + 1);
}

// ---- the schedule of a streamed load and its pieces

void check_stream(uint64_t nreads, uint32_t L, uint64_t batch_reads) {
  ml::StreamPlan sp;
  ml::stream_plan(nreads, batch_reads, &sp);
  const std::vector<uint64_t>& pe = sp.piece_end;
  const std::vector<uint64_t>& be = sp.batch_end;
  if (nreads == 0) {
    EXPECT(pe.empty() && be.empty());
    return;
  }
  EXPECT(!pe.empty() && pe.back() == nreads && !be.empty() && be.back() == nreads);
  if (pe.empty() || be.empty()) return;
  // ascending, every end but the last on a whole wave-tile, every batch end a piece end
  size_t b = 0;
  for (size_t i = 0; i < pe.size(); i++) {
    EXPECT(pe[i] > (i ? pe[i - 1] : 0));
    if (i + 1 < pe.size()) EXPECT(pe[i] % 64 == 0);
    if (b < be.size() && be[b] == pe[i]) b++;
  }
  EXPECT(b == be.size());
  uint64_t r0 = 0;
  for (size_t k = 0; k < be.size(); k++) {  // the pass walks the batches by stream_plan_batch
    EXPECT(ml::stream_plan_batch(sp, r0) == be[k] - r0);
    r0 = be[k];
  }
  EXPECT(ml::stream_plan_batch(sp, nreads) == 0);
  // the pieces tile [0, total_bytes): no gap, no overlap, every piece but the last ends on a whole byte
  const uint64_t total = ml::fixed_total_bytes(nreads, L);
  EXPECT(total * 4 >= nreads * (uint64_t)L && (total == 0 || (total - 1) * 4 < nreads * (uint64_t)L));
  uint64_t at = 0;
  for (size_t i = 0; i < pe.size(); i++) {
    const ml::ByteRange r = ml::fixed_piece_bytes(i ? pe[i - 1] : 0, pe[i], L, total);
    EXPECT(r.b0 == at && r.b1 >= r.b0);
    if (i + 1 < pe.size()) EXPECT(pe[i] * (uint64_t)L % 4 == 0 && r.b1 == pe[i] * (uint64_t)L / 4);
    at = r.b1;
  }
  EXPECT(at == total);
  // the staging buffer: the last piece, and the two words k_pack_reads_fixed (ext64) reads past the word of the first
  // bit of a read's last record word
  const uint64_t need = ml::fixed_need_words(total);
  EXPECT(need * 4 >= total + 16);  // (the last four words are zeroed behind the stream)
  const uint64_t b0 = 16ull * ((L - 1) / 16);  // first base of the last record word that holds bases
  const uint64_t w = 2 * ((nreads - 1) * (uint64_t)L + b0) / 32;
  EXPECT(w + 2 < need);
}

}  // namespace

int main() {
  check_refusals();
  std::vector<uint32_t> lens;
  for (uint32_t L = 1; L <= 300; L++) lens.push_back(L);
  lens.push_back(65535);
  std::vector<uint64_t> counts = {0, 1, 2, 63};
  for (uint64_t m = 64; m <= 4096; m += 64)
    for (uint64_t d : {m - 1, m, m + 1}) counts.push_back(d);
  for (uint32_t L : lens) {
    check_shape(L);
    for (uint64_t n : counts)
      for (uint64_t batch : {1ull, 64ull, 100ull, 1000ull, 4096ull, 16ull << 20}) check_stream(n, L, batch);
    // the 32-bit limits: the most reads a read index takes, and the most whose record words fit one dispatch
    ml::RecShape s;
    EXPECT(ml::rec_shape(1, L, &s) == ml::SHAPE_OK);
    const uint64_t most = ((1ull << 32) - 1) / (uint64_t)s.rw;
    EXPECT(ml::rec_shape(most, L, &s) == ml::SHAPE_OK && ml::rec_shape(most + 1, L, &s) != ml::SHAPE_OK);
    for (uint64_t n : {most - 1, most, (uint64_t)0xFFFFFFEFull}) check_stream(n, L, 16ull << 20);
  }
  check_shape(0);
  for (uint64_t nb = 0; nb <= 5000; nb++) check_db(nb);
  for (uint64_t nb : {(1ull << 32) - 1, 1ull << 32, (1ull << 36) - 1}) check_db(nb);
  return check_done("load_plan_check");
}
