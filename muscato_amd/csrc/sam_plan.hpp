// sam_plan.hpp -- the size rules of a SAM record: decimal widths, the CIGAR, the bytes of `MD` from the
// mismatch places of a span, the name rules of QNAME and RNAME, and the byte count of a whole record.  Plain C++, usable
// on the host and on the device: included by kernels_sam.hpp (the counting pass and the render kernel), by
// host/cli_text.hpp (sam_text, the host copy of the format) and by host/cli_plan_check.cpp.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SAM_HD __host__ __device__ inline
#else
#define SAM_HD inline
#endif

namespace musc_sam {

constexpr uint32_t QNAME_MAX = 254;  // the SAM specification's bound on QNAME

SAM_HD uint32_t ndigits(uint64_t v) {
  uint32_t n = 1;
  while (v >= 10u) {
    v /= 10u;
    n++;
  }
  return n;
}

SAM_HD bool is_space(uint32_t b) { return b == 0x20u || b - 9u <= 4u; }  // C isspace in the C locale

// FLAG: 16 on the reverse strand, 256 on every line of a read but its first
SAM_HD uint32_t flag(bool rev, bool first_line) { return (rev ? 16u : 0u) | (first_line ? 0u : 256u); }

// POS (1-based, on the forward target): a reverse span [pos, pos + S) of the odd target is [len - pos - S, len - pos)
// of the even one
SAM_HD uint64_t pos1(bool rev, uint64_t len, uint64_t pos, uint64_t S) { return rev ? len - pos - S + 1 : pos + 1; }

// CIGAR: <S>M and, when the span was clipped at the target's end, <L - S>S behind it (before it on the reverse
// strand); `*` when S == 0
SAM_HD uint32_t cigar_bytes(uint32_t L, uint32_t S) {
  if (S == 0) return 1;
  return ndigits(S) + 1 + (L > S ? ndigits(L - S) + 1 : 0);
}

// The bytes of MD as they grow while the mismatch places of a span are visited in increasing order: every mismatch adds
// the digits of the match run before it and one base letter, and the end adds the digits of the last run.  The sum does
// not depend on the strand: the reverse strand has the same runs in the opposite order.
struct MdSize {
  uint32_t bytes = 0, nmis = 0;
  int64_t last = -1;  // place of the last mismatch
  SAM_HD void mismatch(uint32_t j) {
    bytes += ndigits((uint32_t)((int64_t)j - last - 1)) + 1;
    last = j;
    nmis++;
  }
  SAM_HD uint32_t finish(uint32_t S) const { return bytes + ndigits((uint32_t)((int64_t)S - last - 1)); }
};

// What of a read's tail (count \t names) a record quotes: count = the bytes before the first tab (the whole tail when
// it has none), kept for XC only when they are all decimal digits and there is at least one; QNAME = the bytes after
// that tab, one leading '@' or '>' dropped, cut at the first ';' or whitespace byte and at QNAME_MAX bytes.
struct TailSpans {
  uint32_t count_len, count_ok, q0, qlen;
};
SAM_HD TailSpans tail_spans(const unsigned char* p, uint64_t T) {
  TailSpans t = {0u, 1u, 0u, 0u};
  uint64_t i = 0;
  while (i < T && p[i] != '\t') {
    if (p[i] - (uint32_t)'0' > 9u) t.count_ok = 0u;
    i++;
  }
  if (i == 0 || i > 0xFFFFFFFFull) t.count_ok = 0u;
  t.count_len = t.count_ok ? (uint32_t)i : 0u;
  if (i < T) i++;  // the tab
  if (i < T && (p[i] == '@' || p[i] == '>')) i++;
  if (i > 0xFFFFFFFFull) return t;  // (a count of 4 GiB: no name within 32-bit reach)
  t.q0 = (uint32_t)i;
  while (i < T && t.qlen < QNAME_MAX && p[i] != ';' && !is_space(p[i])) i++, t.qlen++;
  return t;
}

// RNAME: the first whitespace-delimited token of a gene's text, one leading '>' dropped (len 0: the token is empty)
struct NameSpan {
  uint32_t n0, len;
};
SAM_HD NameSpan rname_span(const unsigned char* p, uint64_t G) {
  uint64_t i = 0;
  while (i < G && is_space(p[i])) i++;
  if (i < G && p[i] == '>') i++;
  const uint64_t b = i;
  while (i < G && !is_space(p[i])) i++;
  NameSpan s = {(uint32_t)b, (uint32_t)(i - b)};
  if (i > 0xFFFFFFFFull) s.len = 0;
  return s;
}

// What a record's byte count is made of
struct RecordSizes {
  uint32_t qname;      // bytes of QNAME (1 for `*`)
  uint32_t flag;       // the FLAG value
  uint32_t rname;      // bytes of RNAME
  uint64_t pos1;       // POS
  uint32_t L, S;       // bases of the read, of the span
  uint32_t d, md;      // NM, bytes of MD
  uint32_t nh, hi;     // NH, HI
  uint32_t nmiss;      // XM
  uint32_t count_len;  // bytes of XC's value; 0: no XC tag
};

//  QNAME \t FLAG \t RNAME \t POS \t 255 \t CIGAR \t * \t 0 \t 0 \t SEQ \t * \t NM:i:d \t MD:Z:md \t NH:i:k \t HI:i:j \t XM:i:n [\t XC:i:c] \n
SAM_HD uint64_t record_bytes(const RecordSizes& r) {
  return (uint64_t)r.qname + 1 + ndigits(r.flag) + 1 + r.rname + 1 + ndigits(r.pos1) + 1 + 4 + cigar_bytes(r.L, r.S) + 1 + 6 +
         (r.L ? r.L : 1u) + 1 + 1 + 6 + ndigits(r.d) + 6 + r.md + 6 + ndigits(r.nh) + 6 + ndigits(r.hi) + 6 + ndigits(r.nmiss) +
         (r.count_len ? 6 + r.count_len : 0u) + 1;
}

// Header lines: @HD \t VN:1.6 \t SO:unsorted \t GO:query \n ; @SQ \t SN:name \t LN:len \n ; @PG \t ID:muscato_amd \t PN:muscato_amd \n
constexpr char HD_LINE[] = "@HD\tVN:1.6\tSO:unsorted\tGO:query\n";
constexpr char PG_LINE[] = "@PG\tID:muscato_amd\tPN:muscato_amd\n";
constexpr uint32_t HD_BYTES = sizeof(HD_LINE) - 1, PG_BYTES = sizeof(PG_LINE) - 1;
SAM_HD uint64_t sq_bytes(uint32_t name_len, uint64_t target_len) { return 7ull + name_len + 4 + ndigits(target_len) + 1; }

}  // namespace musc_sam
