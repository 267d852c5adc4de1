/* muscato_cov.h -- coverage from the resident tuples: additions to the C ABI of muscato_hip.h, in a
 * header of their own.  No new struct, scalar out-parameters, MUSC_ABI_VERSION unchanged.
 *
 * Two texts from the ordered list of the last musc_results_order.  For the tuple (r, g, pos, nmiss) of a line, L bases
 * of read r, S = min(L, len(g) - pos); under MUSC_COV_REV_PAIRS an odd target is the reverse strand of the one before
 * it (f = g - 1), else f = g.  The line covers the forward-strand bases [a, a + S) of target f: a = pos, or
 * len(g) - pos - S on the reverse strand.  Its weight w is 1, or under MUSC_COV_WEIGHTED the count of the read (the
 * bytes of its text before the first tab when they are a non-empty string of decimal digits, saturated at 2^32; else
 * 1).  Under MUSC_COV_UNIQUE only the lines of reads with exactly one line contribute.  depth(f, x) = the sum of w
 * over the contributing lines whose interval holds x.
 *   text 0, bedGraph   rname \t start \t end \t depth \n   per maximal run of constant non-zero depth within a
 *                      target, start 0-based and end exclusive, in target order
 *   text 1, summary    rname \t len \t numreads \t covbases \t sumdepth \t maxdepth \n   per target with an id line
 *                      (under MUSC_COV_REV_PAIRS: the even ones), covered or not, in target order; numreads = the sum
 *                      of w over the contributing lines of the target
 * rname is the RNAME token of muscato_sam.h: the first whitespace-delimited token of the gene text, one `>` dropped. */
#ifndef MUSCATO_COV_H
#define MUSCATO_COV_H

#include "muscato_hip.h"

#define MUSC_COV_REV_PAIRS 1u /* fold the odd targets of a -rev database onto the even ones */
#define MUSC_COV_WEIGHTED 2u  /* each line counts by its read's multiplicity */
#define MUSC_COV_UNIQUE 4u    /* only lines of reads with one line count */

#ifdef __cplusplus
extern "C" {
#endif

/* Sort the interval ends of the ordered list, sum them to depths and lay out both texts.  *nruns and *run_bytes = the
 * records and the bytes of text 0, *ntargets and *summary_bytes = those of text 1; any of the four may be NULL.
 * Code 2: no ordered list of the reads, the database and the texts in hand (musc_results_order), or an unknown flag.
 * Code 12 is a refusal: the ordered list, the other texts and SAM's tables are left as they were, and what an earlier
 * musc_cov_prepare made is dropped (musc_cov_text then answers 2).  The reasons: the weights of the contributing lines
 * add up to 2^32 or more; the list has 2^31 lines or more; MUSC_COV_REV_PAIRS with an odd number of targets or a pair of unequal lengths; a
 * target with an id line whose RNAME token (under MUSC_COV_REV_PAIRS: its even partner's) is empty.
 * Code 10: a device allocation failed. */
int musc_cov_prepare(musc_ctx* ctx, uint32_t flags, uint64_t* nruns, uint64_t* run_bytes, uint64_t* ntargets, uint64_t* summary_bytes);

/* Records [rec0, rec0 + nrec) of text `which` (0 the bedGraph, 1 the summary), clipped at the text's end, into dst
 * (host memory, or device memory with dst_on_device != 0): the protocol of musc_side_text.
 * Code 2: nothing prepared, or the reads, the database, a text or the ordered list were replaced since. */
int musc_cov_text(musc_ctx* ctx, int which, uint64_t rec0, uint64_t nrec, char* dst, uint64_t capacity, int dst_on_device,
                  uint64_t* nbytes);

/* HIP-event time of the last musc_cov_prepare and of all musc_cov_text calls since. */
int musc_cov_last_ms(musc_ctx* ctx, float* ms_prepare, float* ms_text);

#ifdef __cplusplus
}
#endif

#endif
