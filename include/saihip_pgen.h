/* PLINK 2 binary filesets (.pgen / .pvar / .psam) for libsaihip: the host index of a fileset and the
 * decoders that expand the compressed hard-call records of a .pgen into the int8 [record][sample]
 * dosage block which sai_tokenize_gt writes for VCF text (DESIGN_INGEST.md, "PLINK 2 filesets").  An
 * extension of saihip.h with its own version number, as saihip_plink.h and saihip_eigenstrat.h are:
 * none of the three is touched by it.
 *
 * A hard call is a 2-bit code: 0 hom REF, 1 het, 2 hom ALT, 3 missing (REF and ALT as the .pvar names
 * them).  The dosage is the number of ALT copies, and a row flipped by the ancestral-allele rule counts
 * |a - 1| per allele exactly as the VCF tokenizer does (a missing allele counts 2):
 *
 *   code  meaning   ploidy 2   ploidy 2, flipped   ploidy 1   ploidy 1, flipped
 *   0     REF REF       0              2               0              1
 *   1     REF ALT       1              1            refused        refused
 *   2     ALT ALT       2              0               1              0
 *   3     missing      -2              4              -1              2
 *
 * A record is named by three 64-bit numbers, (offset in the batch, length in bytes, vrtype); the base of
 * a record of type 2 or 3 by three more, and a record without a base has -1 in their place.
 *
 * status[row] of the decoders: 0 = fine; n_slots - s = slot s is the lowest slot of the row that is
 * configured with ploidy 1 and holds a heterozygous code (its output byte is 0);
 * SAI_PGEN_STATUS_BAD_INDEX = a column or ploidy outside its range (the output bytes it concerns are 0);
 * SAI_PGEN_STATUS_BAD_RECORD = the record or its base does not lie inside the batch or does not parse
 * (every output byte of the row is 0).  Nothing is read or written outside the buffers.
 */
#ifndef SAIHIP_PGEN_H
#define SAIHIP_PGEN_H

#include <stdint.h>

#include "saihip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SAI_PGEN_ABI_VERSION 1
#define SAI_PGEN_STATUS_BAD_INDEX 0x7FFFFFFF
#define SAI_PGEN_STATUS_BAD_RECORD 0x7FFFFFFE

typedef struct sai_pgen_index sai_pgen_index;

int sai_pgen_abi_version(void);

/* First and last position of the first contiguous run of `chrom` in PREFIX.pvar (-1, -1 if absent):
 * what sai_vcf_scan answers for a VCF. */
int sai_pgen_scan(const char* prefix, const char* chrom, int64_t* first_pos, int64_t* last_pos);

/* Index of one region of a fileset.  Reads the .pgen header (magic, storage mode 0x02 or 0x10, counts,
 * block offsets, vrtypes and record lengths), resolves `sample_names` (IID of the .psam; a name may be
 * asked for more than once, each time with its own ploidy of 1 or 2) to sample columns, selects the
 * .pvar rows of `chrom` inside [start, end] (-1 = open) in file order and applies the ancestral-allele
 * rule.  n_samples == 0 selects rows only. */
int sai_pgen_open(const char* prefix, const char* chrom, int64_t start, int64_t end, int32_t n_samples,
                  const char* const* sample_names, const int32_t* ploidy, const char* anc_bed_path, int32_t n_threads,
                  sai_pgen_index** index_out);
/* Any pointer may be NULL.  n_matched = rows of the chromosome inside the region before
 * polarisation; first / last = as sai_pgen_scan; mode = the storage mode byte. */
int sai_pgen_index_info(const sai_pgen_index* index, int64_t* n_rows, int64_t* n_matched, int64_t* n_anc_entries,
                        int64_t* sample_ct, int64_t* variant_ct, int64_t* mode, int64_t* first_pos, int64_t* last_pos);
/* pos[n_rows], file_row[n_rows] (0-based variant of the .pgen), flip[n_rows], col_of_slot[n_samples],
 * rec[n_rows][3] = (file offset, length, vrtype) of the row's record, base[n_rows][3] = the same of its base
 * record or (-1, -1, -1); any may be NULL. */
int sai_pgen_index_copy(const sai_pgen_index* index, int32_t* pos, int64_t* file_row, uint8_t* flip, int32_t* col_of_slot,
                        int64_t* rec, int64_t* base);
int sai_pgen_index_close(sai_pgen_index* index);

/* bytes = n_bytes raw bytes of the .pgen (host memory).  Output row r (of n_out_rows) is expanded from
 * the record rec[r] (and its base base[r]), offsets counted from `bytes`, flipped when row_flip[r] != 0;
 * slot s (of n_slots) takes sample column col_of_slot[s] (< sample_ct) at ploidy_of_slot[s].
 * out = int8 [n_out_rows][n_slots], status = int32 [n_out_rows]. */
int sai_pgen_decode_host(const uint8_t* bytes, int64_t n_bytes, int64_t n_out_rows, const int64_t* rec, const int64_t* base,
                         const uint8_t* row_flip, int32_t sample_ct, int32_t n_slots, const int32_t* col_of_slot,
                         const int32_t* ploidy_of_slot, int8_t* out, int32_t* status, int32_t n_threads);

/* The same on the GPU: every pointer is device memory.  `out` is the 16-byte aligned start of a
 * [*][n_slots] block of which this call writes the rows [out_row0, out_row0 + n_out_rows) (and nothing
 * else): the other arrays are indexed by the row of the call, 0 .. n_out_rows - 1.  Two promises of the
 * caller select the fast path and stand in for the arrays, which may then be NULL:
 * first_col >= 0: col_of_slot[s] == first_col + s for every slot; uniform_ploidy in {1, 2}:
 * ploidy_of_slot[s] == uniform_ploidy for every slot (0 = read the array). */
int sai_pgen_decode(sai_ctx* ctx, const uint8_t* bytes, int64_t n_bytes, int64_t n_out_rows, const int64_t* rec,
                    const int64_t* base, const uint8_t* row_flip, int32_t sample_ct, int32_t n_slots,
                    const int32_t* col_of_slot, int32_t first_col, const int32_t* ploidy_of_slot, int32_t uniform_ploidy,
                    int8_t* out, int64_t out_row0, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SAIHIP_PGEN_H */
