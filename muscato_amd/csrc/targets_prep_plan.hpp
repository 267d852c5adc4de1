// targets_prep_plan.hpp -- the arithmetic of target preparation that needs no device: the length of an
// id line, where a record's lines go in the sequence text with and without reverse complements, the size of a framed
// stream of uncompressed chunks and a chunk's place in it, and the refusal bound.  Plain C++ that hipcc also compiles
// for the device: included by muscato_hip.hip (kernels_targets_prep.hpp, muscato_targets_prep.hpp) and by
// host/targets_prep_plan_check.cpp, the stand-alone program that holds it to prep_targets_text / prep_targets_fasta /
// sz_encode of the host chain.
//
// Reference: cmd/muscato_prep_targets/main.go:82-141 (processText), :143-213 (processFasta), :246-258 (the framed
// writers); the id line is fmt.Sprintf("%011d\t%s\t%d\n", number, name, len(seq)).
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define TP_HD __host__ __device__ inline
#else
#define TP_HD inline
#endif

namespace musc_tp {

constexpr uint64_t TP_MAX_TARGETS = 0xFFFFFFF0ull;  // this many targets or more, both strands counted: refused (12)
constexpr uint64_t SZ_CHUNK = 65536;                // data bytes of one chunk of the framed writer
constexpr uint64_t SZ_MAGIC = 10, SZ_HEAD = 8;      // the stream identifier; type, 3 length bytes, the masked CRC
constexpr uint32_t ID_NUM_DIGITS = 11;              // %011d

TP_HD uint32_t dec_digits(uint64_t v) {
  uint32_t d = 1;
  while (v >= 10) v /= 10, d++;
  return d;
}

// bytes of one id line, its newline included: %011d \t name [_r] \t len \n (a number of more than eleven digits would
// be longer: TP_MAX_TARGETS keeps every number below 2^32)
TP_HD uint64_t id_line_len(uint64_t name_len, uint64_t seq_len, int strand) {
  return ID_NUM_DIGITS + 1 + name_len + (strand ? 2u : 0u) + 1 + dec_digits(seq_len) + 1;
}
// bytes of a record's id lines: one, or with rev the forward line and the complement's
TP_HD uint64_t id_rec_len(uint64_t name_len, uint64_t seq_len, int rev) {
  return id_line_len(name_len, seq_len, 0) + (rev ? id_line_len(name_len, seq_len, 1) : 0);
}

// F = the sum of len + 1 over the records in front.  The forward line of the record stands at seq_fwd_off, its
// complement (rev only) behind it; the record's lines end at seq_fwd_off(F + len + 1).
TP_HD uint64_t seq_fwd_off(uint64_t F, int rev) { return rev ? 2 * F : F; }
TP_HD uint64_t seq_rev_off(uint64_t F, uint64_t len) { return 2 * F + len + 1; }
TP_HD uint64_t n_targets(uint64_t n_records, int rev) { return rev ? 2 * n_records : n_records; }
TP_HD bool refused(uint64_t n_records, int rev) { return n_targets(n_records, rev) >= TP_MAX_TARGETS; }

// sz_encode's output for n bytes of data: the identifier, then chunks of SZ_CHUNK bytes, the last one shorter
TP_HD uint64_t sz_chunks(uint64_t n) { return (n + SZ_CHUNK - 1) / SZ_CHUNK; }
TP_HD uint64_t sz_frame_size(uint64_t n) { return SZ_MAGIC + SZ_HEAD * sz_chunks(n) + n; }
TP_HD uint64_t sz_chunk_pos(uint64_t i) { return SZ_MAGIC + i * (SZ_HEAD + SZ_CHUNK); }  // of chunk i's header
TP_HD uint32_t sz_chunk_len(uint64_t n, uint64_t i) { return (uint32_t)(n - i * SZ_CHUNK < SZ_CHUNK ? n - i * SZ_CHUNK : SZ_CHUNK); }

// the slices of k_sz_frame's CRC: `lanes` lanes, each an odd number of dwords; lane l takes bytes [b0, b1) of the chunk
TP_HD uint32_t crc_slice_dwords(uint32_t ulen, uint32_t lanes) { return ((ulen + 4 * lanes - 1) / (4 * lanes)) | 1u; }

}  // namespace musc_tp
