/* PLINK 1 binary filesets (.bed / .bim / .fam) for libsaihip: the host index of a fileset and the
 * decoders that turn variant-major .bed rows into the int8 [record][sample] dosage block which
 * sai_tokenize_gt writes for VCF text (DESIGN_INGEST.md, "PLINK 1 filesets").  An extension of
 * saihip.h with its own version number: the entry points of saihip.h and SAI_ABI_VERSION are not
 * touched by it.
 *
 * A .bed row holds sample i in bits [2 * (i % 4), +2) of byte i / 4.  A2 plays REF and A1 plays ALT,
 * so the dosage is the number of A1 copies, and a row flipped by the ancestral-allele rule counts
 * |a - 1| per allele exactly as the VCF tokenizer does (a missing allele counts 2):
 *
 *   code  meaning   ploidy 2   ploidy 2, flipped   ploidy 1   ploidy 1, flipped
 *   00    A1 A1         2              0               1              0
 *   10    A1 A2         1              1            refused        refused
 *   11    A2 A2         0              2               0              1
 *   01    missing      -2              4              -1              2
 *
 * status[row] of the decoders: 0 = fine; n_slots - s = slot s is the lowest slot of the row that is
 * configured with ploidy 1 and holds a heterozygous code (its output byte is 0);
 * SAI_PLINK_STATUS_BAD_INDEX = a row index, column or ploidy outside its range (the output bytes it
 * concerns are 0; nothing is read outside the buffers).
 */
#ifndef SAIHIP_PLINK_H
#define SAIHIP_PLINK_H

#include <stdint.h>

#include "saihip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SAI_PLINK_ABI_VERSION 1
#define SAI_PLINK_STATUS_BAD_INDEX 0x7FFFFFFF

typedef struct sai_plink_index sai_plink_index;

int sai_plink_abi_version(void);

/* First and last position of the first contiguous run of `chrom` in PREFIX.bim (-1, -1 if absent):
 * what sai_vcf_scan answers for a VCF. */
int sai_plink_scan(const char* prefix, const char* chrom, int64_t* first_pos, int64_t* last_pos);

/* Index of one region of a fileset.  Checks the .bed (magic, variant-major, size), resolves
 * `sample_names` (IID, column 2 of the .fam; a name may be asked for more than once, each time with
 * its own ploidy of 1 or 2) to .fam columns, selects the .bim rows of `chrom` inside [start, end]
 * (-1 = open) in file order and applies the ancestral-allele rule with REF = A2, ALT = A1.
 * n_samples == 0 selects rows only. */
int sai_plink_open(const char* prefix, const char* chrom, int64_t start, int64_t end, int32_t n_samples,
                   const char* const* sample_names, const int32_t* ploidy, const char* anc_bed_path, int32_t n_threads,
                   sai_plink_index** index_out);
/* Any pointer may be NULL.  n_matched = rows of the chromosome inside the region before
 * polarisation; first / last = as sai_plink_scan. */
int sai_plink_index_info(const sai_plink_index* index, int64_t* n_rows, int64_t* n_matched, int64_t* n_anc_entries,
                         int64_t* row_bytes, int64_t* n_fam, int64_t* n_bim, int64_t* first_pos, int64_t* last_pos);
/* pos[n_rows], file_row[n_rows] (0-based row of the .bed), flip[n_rows], col_of_slot[n_samples]; any may be NULL. */
int sai_plink_index_copy(const sai_plink_index* index, int32_t* pos, int64_t* file_row, uint8_t* flip, int32_t* col_of_slot);
int sai_plink_index_close(sai_plink_index* index);

/* rows = n_batch_rows rows of row_bytes bytes (host memory).  Output row r (of n_out_rows) is decoded
 * from batch row row_in_batch[r], flipped when row_flip[r] != 0; slot s (of n_slots) takes .fam column
 * col_of_slot[s] (< n_cols <= 4 * row_bytes) at ploidy_of_slot[s].  out = int8 [n_out_rows][n_slots],
 * status = int32 [n_out_rows]. */
int sai_plink_decode_host(const uint8_t* rows, int64_t n_batch_rows, int64_t row_bytes, int64_t n_out_rows,
                          const int32_t* row_in_batch, const uint8_t* row_flip, int32_t n_cols, int32_t n_slots,
                          const int32_t* col_of_slot, const int32_t* ploidy_of_slot, int8_t* out, int32_t* status,
                          int32_t n_threads);

/* The same on the GPU: every pointer is device memory.  `out` is the 16-byte aligned start of a
 * [*][n_slots] block of which this call writes the rows [out_row0, out_row0 + n_out_rows) (and nothing
 * else): the other arrays are indexed by the row of the call, 0 .. n_out_rows - 1.  Two promises of the
 * caller select the fast path and stand in for the arrays, which may then be NULL:
 * first_col >= 0: col_of_slot[s] == first_col + s for every slot; uniform_ploidy in {1, 2}:
 * ploidy_of_slot[s] == uniform_ploidy for every slot (0 = read the array). */
int sai_plink_decode(sai_ctx* ctx, const uint8_t* rows, int64_t n_batch_rows, int64_t row_bytes, int64_t n_out_rows,
                     const int32_t* row_in_batch, const uint8_t* row_flip, int32_t n_cols, int32_t n_slots,
                     const int32_t* col_of_slot, int32_t first_col, const int32_t* ploidy_of_slot, int32_t uniform_ploidy,
                     int8_t* out, int64_t out_row0, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SAIHIP_PLINK_H */
