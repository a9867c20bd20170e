/* Per-site allele frequencies straight from packed2 blocks (the 2-bit layout of saihip.h), for
 * libsaihip: the site half of fd / df / Danc / Dplus in that layout (DESIGN_INGEST.md, "ABBA-BABA
 * statistics in the 2-bit layout").  sai_window_fourpop of saihip.h takes the frequencies as they
 * are.  An extension with its own version number: the entry points and the version numbers of
 * saihip.h and of the other extension headers are not touched.
 *
 * The existing way to these doubles is sai_site_pass_packed2(counts) + sai_site_freqs: it stops at
 * 2 + SAI_FUSED_SRC populations and moves 8 bytes of counts per population and site out and in again.
 * In the packed layout a lane owns a site, so one pass counts the three codes and divides.
 */
#ifndef SAIHIP_PACKED_STATS_H
#define SAIHIP_PACKED_STATS_H

#include <stdint.h>

#include "saihip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SAI_PACKED_STATS_ABI_VERSION 1
#define SAI_PACKED_FREQ_POPS 9 /* ref, tgt, SAI_FUSED_SRC sources, outgroup: what sai_site_freqs takes */

int sai_packed_stats_abi_version(void);

/* pops[p].tiles = a packed2 block (device, 16-byte aligned) of sai_packed2_bytes(n_sites, n_ind) bytes, ploidy > 0.
 * freqs[p * n_sites + site] = (ones + 2 * twos) / ((n_ind - missing) * ploidy) as f64, quiet NaN where the
 * denominator is 0: the doubles sai_site_pass_packed2(counts) + sai_site_freqs give, bit for bit.  Only
 * sites < n_sites are written.  n_sites == 0 is SAI_OK and touches nothing.
 * n_pops = 1..SAI_PACKED_FREQ_POPS, n_ind = 1..2^24 (SAI_ERR_UNSUPPORTED beyond), n_sites < 2^31 - 1. */
int sai_packed2_site_freqs(sai_ctx* ctx, int64_t n_sites, int32_t n_pops, const sai_pop* pops, double* freqs, void* stream);

/* the plain C++ twin: host pointers (of any alignment), same outputs bit for bit */
int sai_packed2_site_freqs_host(int64_t n_sites, int32_t n_pops, const sai_pop* pops, double* freqs, int32_t n_threads);

#ifdef __cplusplus
}
#endif

#endif /* SAIHIP_PACKED_STATS_H */
