// read_names_plan.hpp -- the arithmetic of the read-name stage that needs no device: the 1000-byte rule of
// a name, the bytes of a clipped name that are not in the text, where a token ends, the width of a count, the lengths of
// a record of the read text and of a line of reads_sorted.txt, the path that ranks a group, and the refusal bound.  Plain
// C++ that hipcc also compiles for the device (RN_HD): included by read_names_lanes.hpp and read_names_keys.hpp -- what
// a lane of the stage's kernels (kernels_read_names.hpp) computes, in the same plain C++ -- and by
// host/read_names_plan_check.cpp, the stand-alone program that holds all three to a byte-loop restatement of the
// reference's string code.
//
// Reference: cmd/muscato_prep_reads/main.go:76-79 (a name of more than 1000 bytes becomes its first 995 and "..."),
// cmd/muscato_uniqify/main.go:83-135 (a name ends at its first tab; the names of a group are joined with ';' and a join
// of more than 1000 bytes becomes its first 996 and "...").
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define RN_HD __host__ __device__ inline
#else
#define RN_HD inline
#endif

namespace musc_rn {

constexpr uint32_t NAME_LIMIT = 1000, NAME_KEEP = 995;  // a longer name keeps NAME_KEEP bytes of its own
constexpr uint32_t JOIN_LIMIT = 1000, JOIN_KEEP = 996;  // a longer join keeps JOIN_KEEP bytes of its own
constexpr uint32_t DOTS = 3;                          // "..." behind what a clipped name or join keeps
constexpr uint32_t WAVE_GROUP_MAX = 64;               // the largest group one wave ranks
constexpr uint64_t RN_MAX_READS = 0xFFFFFFF0ull;      // this many kept reads or more: refused (2), as every read load does

// bytes of the name that come from the text / bytes of the clipped name
RN_HD uint32_t text_len(uint32_t name_len) { return name_len > NAME_LIMIT ? NAME_KEEP : name_len; }
RN_HD uint32_t clipped_len(uint32_t name_len) { return name_len > NAME_LIMIT ? NAME_KEEP + DOTS : name_len; }
// byte i of the clipped name, i < clipped_len: true = it is the '.' that stands for what was cut, false = byte i of the text
RN_HD bool virtual_byte(uint32_t name_len, uint32_t i) { return name_len > NAME_LIMIT && i >= NAME_KEEP; }

// The token: the clipped name up to its first tab.  first_tab = the place of the first tab among the first
// text_len(name_len) bytes of the name, or any value >= text_len when there is none (the dots hold no tab).
RN_HD uint32_t token_len(uint32_t name_len, uint32_t first_tab) { return first_tab < text_len(name_len) ? first_tab : clipped_len(name_len); }

RN_HD uint32_t dec_width(uint64_t v) {
  uint32_t d = 1;
  while (v >= 10) v /= 10, d++;
  return d;
}

// sum = the tokens of a group and the ';' between them (any value above JOIN_LIMIT stands for every such value)
RN_HD bool join_clipped(uint64_t sum) { return sum > JOIN_LIMIT; }
RN_HD uint32_t join_len(uint64_t sum) { return join_clipped(sum) ? JOIN_KEEP + DOTS : (uint32_t)sum; }
RN_HD uint32_t join_text_len(uint64_t sum) { return join_clipped(sum) ? JOIN_KEEP : (uint32_t)sum; }  // bytes of the tokens' own
// count \t J  /  seq \t count \t J \n
RN_HD uint64_t record_len(uint64_t count, uint64_t sum) { return (uint64_t)dec_width(count) + 1 + join_len(sum); }
RN_HD uint64_t line_len(uint64_t seq_len, uint64_t count, uint64_t sum) { return seq_len + 1 + record_len(count, sum) + 1; }

enum Path { PATH_SINGLE = 0, PATH_WAVE = 1, PATH_SORTED = 2 };
RN_HD Path group_path(uint64_t count) { return count <= 1 ? PATH_SINGLE : count <= WAVE_GROUP_MAX ? PATH_WAVE : PATH_SORTED; }

RN_HD bool refused(uint64_t n_reads) { return n_reads >= RN_MAX_READS; }

// the meta word of a read: its clipped length and its token length, both at most 1000
RN_HD uint32_t meta_pack(uint32_t clip, uint32_t tok) { return clip | (tok << 16); }
RN_HD uint32_t meta_clip(uint32_t m) { return m & 0xFFFFu; }
RN_HD uint32_t meta_tok(uint32_t m) { return m >> 16; }

}  // namespace musc_rn
