/* PLINK 1 .bed rows decoded straight into the packed2 layout of saihip.h (2 bits per call), for
 * libsaihip: the rows never pass through the int8 [record][sample] block of saihip_plink.h
 * (DESIGN_INGEST.md, "PLINK 1 filesets in the 2-bit layout").  An extension with its own version
 * number: the entry points and the version numbers of saihip.h and saihip_plink.h are not touched.
 *
 * One call serves one population: individual i (of n_ind) takes .fam column col_of_ind[i] at the
 * population's ploidy.  The packed code is the int8 dosage of saihip_plink.h where it fits two bits
 * (0, 1, 2; a negative dosage = missing = 3):
 *
 *   code  meaning   ploidy 2   ploidy 2, flipped   ploidy 1   ploidy 1, flipped
 *   00    A1 A1         2              0               1              0
 *   10    A1 A2         1              1            refused        refused
 *   11    A2 A2         0              2               0              1
 *   01    missing       3            unfit             3              2
 *
 * status[row]: as sai_plink_decode -- 0 = fine; n_ind - i = individual i is the lowest of the row
 * with a heterozygous code at ploidy 1; SAI_PLINK_STATUS_BAD_INDEX = a row index or column outside
 * its range.  unfit[row]: 0, or n_ind - i for the lowest individual i whose dosage does not fit two
 * bits (a missing call in a flipped row at ploidy 2: dosage 4).  The field of a refused, unfit or
 * out-of-range call is 0; nothing is read outside the buffers.
 *
 * `packed` is the population's WHOLE block of sai_packed2_bytes(n_sites, n_ind) bytes.  A call writes
 * the 32-bit words of the sites [out_row0, out_row0 + n_out_rows) and nothing else (a word belongs to
 * one site, so batches may be cut anywhere, inside a tile too); the call that holds site n_sites - 1
 * also writes the padding sites of the last tile (all ones).  Fields of padding individuals are 0.
 */
#ifndef SAIHIP_PACKED_INGEST_H
#define SAIHIP_PACKED_INGEST_H

#include <stdint.h>

#include "saihip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SAI_PACKED_INGEST_ABI_VERSION 1

int sai_packed_ingest_abi_version(void);

/* rows = n_batch_rows rows of row_bytes bytes (host memory).  Output row r (of n_out_rows) is site
 * out_row0 + r of the block, decoded from batch row row_in_batch[r], flipped when row_flip[r] != 0.
 * first_col >= 0 promises col_of_ind[i] == first_col + i (col_of_ind may then be NULL); otherwise
 * col_of_ind may permute and repeat columns (< n_cols <= 4 * row_bytes).  ploidy = 1 or 2.
 * status, unfit = int32 [n_out_rows], zeroed by the call. */
int sai_bed_pack2_host(const uint8_t* rows, int64_t n_batch_rows, int64_t row_bytes, int64_t n_out_rows,
                       const int32_t* row_in_batch, const uint8_t* row_flip, int32_t n_cols, int32_t n_ind,
                       const int32_t* col_of_ind, int32_t first_col, int32_t ploidy, uint8_t* packed, int64_t n_sites,
                       int64_t out_row0, int32_t* status, int32_t* unfit, int32_t n_threads);

/* The same on the GPU: every pointer is device memory, `packed` is 16-byte aligned. */
int sai_bed_pack2(sai_ctx* ctx, const uint8_t* rows, int64_t n_batch_rows, int64_t row_bytes, int64_t n_out_rows,
                  const int32_t* row_in_batch, const uint8_t* row_flip, int32_t n_cols, int32_t n_ind,
                  const int32_t* col_of_ind, int32_t first_col, int32_t ploidy, uint8_t* packed, int64_t n_sites,
                  int64_t out_row0, int32_t* status, int32_t* unfit, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SAIHIP_PACKED_INGEST_H */
