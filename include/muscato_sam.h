/* muscato_sam.h -- SAM output from the resident tuples: additions to the C ABI of muscato_hip.h, in a
 * header of their own.  No new struct, scalar out-parameters, MUSC_ABI_VERSION unchanged.
 *
 * One record per line of results.txt, in the order of the last musc_results_order, rendered on the device from what
 * that call left there: the ordered tuples, the planes of the reads and of the database, the gene text and the read
 * text.  For the tuple (r, g, pos, nmiss), L bases of read r and S = min(L, len(g) - pos):
 *   QNAME  the read text of r after its first tab, one leading '@' or '>' dropped, cut at the first ';' or whitespace
 *          byte and at 254 bytes; `*` when that is empty or no read text is set
 *   FLAG   16 on the reverse strand (rev_pairs and g odd) | 256 on every line of r but its first
 *   RNAME  the first whitespace-delimited token of the gene text of f (g, or g - 1 on the reverse strand), one leading
 *          '>' dropped
 *   POS    pos + 1; on the reverse strand len(g) - pos - S + 1
 *   MAPQ 255, CIGAR <S>M[<L - S>S] (the clip first on the reverse strand; `*` when S == 0), RNEXT `*`, PNEXT 0, TLEN 0
 *   SEQ    the read, X as N; on the reverse strand its reverse complement; QUAL `*`
 *   tags   NM:i MD:Z NH:i HI:i XM:i (nmiss, copied) and XC:i (the count of the read text, when there is one)
 * The header is @HD, one @SQ per target with an id line (under rev_pairs: the even ones), @PG. */
#ifndef MUSCATO_SAM_H
#define MUSCATO_SAM_H

#include "muscato_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Compare every span of the ordered list with its read, count NH / HI, and compute the byte offsets of the records and
 * of the header lines.  rev_pairs != 0: the database was prepared with reverse complements, target 2k + 1 is the
 * reverse complement of target 2k.  *nrecords = records (the lines of the ordered list), *header_bytes and
 * *record_bytes = the bytes of the two texts; any of the three may be NULL.
 * Code 2: no ordered list of the reads, the database and the texts in hand (musc_results_order).
 * Code 12 is a refusal that leaves the context untouched (as musc_side_prepare's): rev_pairs with an odd number of
 * targets or a pair of unequal lengths, or a target with an id line whose RNAME token (under rev_pairs: its even
 * partner's) is empty.  Code 10: a device allocation failed. */
int musc_sam_prepare(musc_ctx* ctx, int rev_pairs, uint64_t* nrecords, uint64_t* header_bytes, uint64_t* record_bytes);

/* Records [rec0, rec0 + nrec) of text `which` (0 the header, 1 the records), clipped at the text's end, into dst (host
 * memory, or device memory with dst_on_device != 0): the protocol of musc_side_text.  The header's records are its
 * slots: 0 = @HD, 1 + t = the @SQ line of target t (empty when it has none), the last = @PG.
 * Code 2: nothing prepared, or the reads, the database, a text or the ordered list were replaced since. */
int musc_sam_text(musc_ctx* ctx, int which, uint64_t rec0, uint64_t nrec, char* dst, uint64_t capacity, int dst_on_device,
                  uint64_t* nbytes);

/* HIP-event time of the last musc_sam_prepare and of all musc_sam_text calls since. */
int musc_sam_last_ms(musc_ctx* ctx, float* ms_prepare, float* ms_text);

#ifdef __cplusplus
}
#endif

#endif
