/* EIGENSOFT filesets (PREFIX.geno + PREFIX.snp + PREFIX.ind) for libsaihip: the host index of a fileset and
 * the decoders that turn .geno records into the int8 [record][sample] dosage block which sai_tokenize_gt
 * writes for VCF text (DESIGN_INGEST.md, "EIGENSTRAT filesets").  An extension of saihip.h with its own
 * version number, as saihip_plink.h is: neither of the two is touched by it.
 *
 * A genotype value g counts the copies of the FIRST allele of the .snp line (column 5), which plays REF;
 * column 6 plays ALT.  The dosage is the number of ALT copies, and a row flipped by the ancestral-allele
 * rule counts |a - 1| per allele exactly as the VCF tokenizer does (a missing allele counts 2):
 *
 *   g         ploidy 2   ploidy 2, flipped   ploidy 1   ploidy 1, flipped
 *   0             2              0               1              0
 *   1             1              1            refused        refused
 *   2             0              2               0              1
 *   missing      -2              4              -1              2
 *
 * The three encodings of a .geno, told apart by content:
 *   text        one line per variant, one character per individual ('0' '1' '2', '9' = missing)
 *   packed      "GENO n_ind n_snp ..." in a first record of rlen = max(48, ceil(n_ind / 4)) bytes, then one
 *               record per variant: individual i in bits [6 - 2 * (i % 4), +2) of byte i / 4 (the FIRST
 *               individual in the two most significant bits), 3 = missing
 *   transposed  "TGENO n_ind n_snp ..." in a first record of rlen = max(48, ceil(n_snp / 4)) bytes, then
 *               one record per individual: variant k in bits [6 - 2 * (k % 4), +2) of byte k / 4
 *
 * status[row] of the decoders: 0 = fine; n_slots - s = slot s is the lowest slot of the row that is
 * configured with ploidy 1 and holds g = 1 (its output byte is 0); SAI_EIGENSTRAT_STATUS_BAD_CHAR = a
 * character other than 0 1 2 9 in a text record (output byte 0); SAI_EIGENSTRAT_STATUS_BAD_INDEX = a row
 * index, column or ploidy outside its range (the output bytes it concerns are 0; nothing is read outside
 * the buffers).  The largest applies.
 */
#ifndef SAIHIP_EIGENSTRAT_H
#define SAIHIP_EIGENSTRAT_H

#include <stdint.h>

#include "saihip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SAI_EIGENSTRAT_ABI_VERSION 1
#define SAI_EIGENSTRAT_STATUS_BAD_INDEX 0x7FFFFFFF
#define SAI_EIGENSTRAT_STATUS_BAD_CHAR 0x7FFFFFFE

#define SAI_EIGENSTRAT_TEXT 1
#define SAI_EIGENSTRAT_PACKED 2
#define SAI_EIGENSTRAT_TRANSPOSED 3

typedef struct sai_eigenstrat_index sai_eigenstrat_index;

int sai_eigenstrat_abi_version(void);

/* First and last position of the first contiguous run of `chrom` in PREFIX.snp (-1, -1 if absent):
 * what sai_vcf_scan answers for a VCF. */
int sai_eigenstrat_scan(const char* prefix, const char* chrom, int64_t* first_pos, int64_t* last_pos);

/* Index of one region of a fileset.  Detects the encoding of the .geno and checks its header and size
 * (the two hashes of a packed header are parsed and not verified), resolves `sample_names` (column 1 of
 * the .ind; a name may be asked for more than once, each time with its own ploidy of 1 or 2) to .ind
 * lines, selects the .snp rows of `chrom` inside [start, end] (-1 = open) in file order and applies the
 * ancestral-allele rule with REF = column 5, ALT = column 6.  n_samples == 0 selects rows only. */
int sai_eigenstrat_open(const char* prefix, const char* chrom, int64_t start, int64_t end, int32_t n_samples,
                        const char* const* sample_names, const int32_t* ploidy, const char* anc_bed_path, int32_t n_threads,
                        sai_eigenstrat_index** index_out);
/* Any pointer may be NULL.  n_matched = rows of the chromosome inside the region before polarisation;
 * first / last = as sai_eigenstrat_scan; encoding = SAI_EIGENSTRAT_TEXT / _PACKED / _TRANSPOSED;
 * record_bytes = the line length of a text .geno (newline included), else rlen; data_offset = where the
 * first record starts in the file (0 for text, else rlen). */
int sai_eigenstrat_index_info(const sai_eigenstrat_index* index, int64_t* n_rows, int64_t* n_matched, int64_t* n_anc_entries,
                              int64_t* n_ind, int64_t* n_snp, int64_t* first_pos, int64_t* last_pos, int64_t* encoding,
                              int64_t* record_bytes, int64_t* data_offset);
/* pos[n_rows], file_row[n_rows] (0-based record line of the .snp), flip[n_rows], col_of_slot[n_samples]
 * (0-based record line of the .ind); any may be NULL. */
int sai_eigenstrat_index_copy(const sai_eigenstrat_index* index, int32_t* pos, int64_t* file_row, uint8_t* flip, int32_t* col_of_slot);
int sai_eigenstrat_index_close(sai_eigenstrat_index* index);

/* Host decoder of all three encodings.  Output row r (of n_out_rows) is flipped when row_flip[r] != 0; slot
 * s (of n_slots) takes column col_of_slot[s] (< n_cols) at ploidy_of_slot[s].  out = int8
 * [n_out_rows][n_slots], status = int32 [n_out_rows].
 *   text, packed: records = n_batch_records records of record_bytes bytes, one per variant; row r is decoded
 *     from record row_in_batch[r]; a column is an individual; first_code must be 0.
 *   transposed: records = n_cols records of record_bytes bytes, one per staged individual, each holding the
 *     same range of the individual's record in the file: n_batch_records variants that start at code
 *     first_code (0 .. 3) of its first byte; row r is variant row_in_batch[r] of that range; a column is a
 *     staged individual. */
int sai_eigenstrat_decode_host(int32_t encoding, const uint8_t* records, int64_t n_batch_records, int64_t record_bytes,
                               int32_t first_code, int64_t n_out_rows, const int32_t* row_in_batch, const uint8_t* row_flip,
                               int32_t n_cols, int32_t n_slots, const int32_t* col_of_slot, const int32_t* ploidy_of_slot,
                               int8_t* out, int32_t* status, int32_t n_threads);

/* The variant-major encodings (SAI_EIGENSTRAT_TEXT, SAI_EIGENSTRAT_PACKED) on the GPU: every pointer is
 * device memory.  `out` is the 16-byte aligned start of a [*][n_slots] block of which this call writes the
 * rows [out_row0, out_row0 + n_out_rows) (and nothing else): the other arrays are indexed by the row of the
 * call, 0 .. n_out_rows - 1.  Two promises of the caller select the fast path and stand in for the arrays,
 * which may then be NULL: first_col >= 0: col_of_slot[s] == first_col + s for every slot; uniform_ploidy in
 * {1, 2}: ploidy_of_slot[s] == uniform_ploidy for every slot (0 = read the array). */
int sai_eigenstrat_decode(sai_ctx* ctx, int32_t encoding, const uint8_t* records, int64_t n_batch_records, int64_t record_bytes,
                          int64_t n_out_rows, const int32_t* row_in_batch, const uint8_t* row_flip, int32_t n_cols,
                          int32_t n_slots, const int32_t* col_of_slot, int32_t first_col, const int32_t* ploidy_of_slot,
                          int32_t uniform_ploidy, int8_t* out, int64_t out_row0, int32_t* status, void* stream);

/* The transposed encoding on the GPU: `staged` holds n_staged individuals, record_stride bytes apart (a
 * multiple of 16; `staged` itself 16-byte aligned), each the same byte range of the individual's record:
 * n_batch_variants variants that start at code first_code (0 .. 3) of the first byte, so
 * first_code + n_batch_variants <= 4 * record_stride.  Output row r is variant row_in_batch[r] of the batch
 * (any order; ascending rows are read once), slot s takes staged individual col_of_slot[s] at
 * ploidy_of_slot[s]; `out`, `out_row0` and `status` as in sai_eigenstrat_decode.  The kernel turns tiles
 * of 256 variants x 64 slots in LDS. */
int sai_eigenstrat_decode_transposed(sai_ctx* ctx, const uint8_t* staged, int32_t n_staged, int64_t record_stride,
                                     int32_t first_code, int64_t n_batch_variants, int64_t n_out_rows,
                                     const int32_t* row_in_batch, const uint8_t* row_flip, int32_t n_slots,
                                     const int32_t* col_of_slot, const int32_t* ploidy_of_slot, int8_t* out, int64_t out_row0,
                                     int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SAIHIP_EIGENSTRAT_H */
