/* PLINK 2 .pgen records decoded straight into the packed2 layout of saihip.h (2 bits per call), for
 * libsaihip: the rows never pass through the int8 [record][sample] block of saihip_pgen.h
 * (DESIGN_INGEST.md, "PLINK 2 filesets in the 2-bit layout").  An extension with its own version
 * number: the entry points and the version numbers of saihip.h, saihip_pgen.h and
 * saihip_packed_ingest.h are not touched.
 *
 * The input of a call is that of sai_pgen_decode (saihip_pgen.h): the raw bytes of a batch and, per
 * output row, the span and vrtype of its record and of its base.  The output is that of sai_bed_pack2
 * (saihip_packed_ingest.h): one call serves one population, individual i (of n_ind) takes sample column
 * col_of_ind[i] at the population's ploidy.  The packed field is the int8 dosage of saihip_pgen.h where
 * it fits two bits (0, 1, 2; a negative dosage = missing = 3):
 *
 *   code  meaning   ploidy 2   ploidy 2, flipped   ploidy 1   ploidy 1, flipped
 *   0     REF REF       0              2               0              1
 *   1     REF ALT       1              1            refused        refused
 *   2     ALT ALT       2              0               1              0
 *   3     missing       3            unfit             3              2
 *
 * status[row]: 0 = fine; n_ind - i = individual i is the lowest of the row with a heterozygous code at
 * ploidy 1; SAI_PGEN_STATUS_BAD_INDEX = a column outside its range; SAI_PGEN_STATUS_BAD_RECORD = the
 * record or its base does not lie inside the batch or does not parse (every field of the row is then 0
 * and unfit[row] is 0).  unfit[row]: 0, or n_ind - i for the lowest individual i whose dosage does not
 * fit two bits (a missing call in a flipped row at ploidy 2: dosage 4).  The field of a refused, unfit
 * or out-of-range call is 0; nothing is read outside the buffers.
 *
 * `packed` is the population's WHOLE block of sai_packed2_bytes(n_sites, n_ind) bytes.  A call writes
 * the 32-bit words of the sites [out_row0, out_row0 + n_out_rows) and nothing else (a word belongs to
 * one site, so batches may be cut anywhere, inside a tile too); the call that holds site n_sites - 1
 * also writes the padding sites of the last tile (all ones).  Fields of padding individuals are 0.
 */
#ifndef SAIHIP_PGEN_PACKED_H
#define SAIHIP_PGEN_PACKED_H

#include <stdint.h>

#include "saihip.h"
#include "saihip_pgen.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SAI_PGEN_PACKED_ABI_VERSION 1

int sai_pgen_packed_abi_version(void);

/* bytes = n_bytes raw bytes of the .pgen (host memory).  Output row r (of n_out_rows) is site
 * out_row0 + r of the block, expanded from the record rec[r] (and its base base[r]; both [n][3] =
 * offset counted from `bytes`, length, vrtype), flipped when row_flip[r] != 0.  first_col >= 0
 * promises col_of_ind[i] == first_col + i (col_of_ind may then be NULL); otherwise col_of_ind may
 * permute and repeat columns (< sample_ct).  ploidy = 1 or 2.  status, unfit = int32 [n_out_rows],
 * zeroed by the call. */
int sai_pgen_pack2_host(const uint8_t* bytes, int64_t n_bytes, int64_t n_out_rows, const int64_t* rec, const int64_t* base,
                        const uint8_t* row_flip, int32_t sample_ct, int32_t n_ind, const int32_t* col_of_ind,
                        int32_t first_col, int32_t ploidy, uint8_t* packed, int64_t n_sites, int64_t out_row0,
                        int32_t* status, int32_t* unfit, int32_t n_threads);

/* The same on the GPU: every pointer is device memory, `packed` is 16-byte aligned. */
int sai_pgen_pack2(sai_ctx* ctx, const uint8_t* bytes, int64_t n_bytes, int64_t n_out_rows, const int64_t* rec,
                   const int64_t* base, const uint8_t* row_flip, int32_t sample_ct, int32_t n_ind,
                   const int32_t* col_of_ind, int32_t first_col, int32_t ploidy, uint8_t* packed, int64_t n_sites,
                   int64_t out_row0, int32_t* status, int32_t* unfit, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SAIHIP_PGEN_PACKED_H */
