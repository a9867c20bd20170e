/* Two inputs joined, for libsaihip: the rows two ascending position lists have in common -- what the host readers
 * run between reading a panel and a source file of its own (DESIGN_INGEST.md, "Sources from a file of their
 * own").  An extension with its own version number: the entry points and the version numbers of
 * saihip.h and of the other extension headers are not touched.  Host code only: this version has no GPU form.
 */
#ifndef SAIHIP_JOIN_H
#define SAIHIP_JOIN_H

#include <stdint.h>

#include "saihip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SAI_JOIN_ABI_VERSION 1
#define SAI_JOIN_INFO_WORDS 4 /* int64 words of info */

int sai_join_abi_version(void);

/* pos_a[n_a], pos_b[n_b]: int32 positions in host memory, strictly ascending, n = 0 .. 2^31 - 2.
 * rows_a[k] / rows_b[k] (room for min(n_a, n_b) entries each) = the rows of the k-th common position, ascending.
 * info[0] = n_common
 * info[1] = the first index of a whose position is not above its predecessor's, or -1
 * info[2] = the same for b
 * info[3] = 1 when rows_a is the identity (n_common == n_a), else 0
 * If info[1] or info[2] is not -1, info[0] and info[3] are 0 and rows_a / rows_b are not written.
 * n_a == 0 or n_b == 0 is SAI_OK with info = {0, -1, -1, n_a == 0}: nothing is read, neither list is checked. */
int sai_site_join_host(const int32_t* pos_a, int64_t n_a, const int32_t* pos_b, int64_t n_b, int32_t* rows_a,
                       int32_t* rows_b, int64_t* info);

#ifdef __cplusplus
}
#endif

#endif /* SAIHIP_JOIN_H */
