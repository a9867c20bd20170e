// Writing an EIGENSOFT fileset from a VCF's calls (DESIGN_INGEST.md, "EIGENSOFT filesets written from a VCF"): the
// inverses of sai_eigenstrat_decode (PACKEDANCESTRYMAP, "GENO") and sai_eigenstrat_decode_transposed ("TGENO"), the
// hash of the header record and the .snp lines.  These entry points are internal to the package -- bound by
// sai_amd/utils/geno_writer.py, which is their only caller -- and no part of the drop-in C ABI under include/: they
// have a version number of their own and may change with the converter.
//
// The encoders read the int8 [row][slot] block every reader returns.  A genotype code is the number of copies of the
// first allele of the .snp line, and the first allele is REF: the unflipped column of include/saihip_eigenstrat.h,
// read backwards.
//
//   dosage in the block          ploidy 2    ploidy 1
//   0                            2           2
//   1                            1           0
//   2                            0           does not fit
//   wholly missing (-2 / -1)     3           3
//
// Any other value does not fit: its field is written 3 and status[row] = n_slots - s for the lowest such slot s (the
// convention of plink/bed_export.hpp); a ploidy outside 1 .. 2 writes 3 as well and gives SAI_PLINK_STATUS_BAD_INDEX
// for the row.
//
// Packed form: one record of rlen = max(48, ceil(n_slots / 4)) bytes per row; slot i sits in bits [6 - 2 * (i % 4), +2)
// of byte i / 4 -- the first slot in the two most significant bits, the opposite of a .bed.  Transposed form: one record
// of rlen = max(48, ceil(n_rows / 4)) bytes per slot; row k sits in bits [6 - 2 * (k % 4), +2) of byte k / 4.  Unused
// bits and padding bytes are 0 in both.  The header record is the caller's.
#pragma once

#include <stdint.h>

#include "saihip.h"
#include "saihip_plink.h"

#define SAI_GENO_EXPORT_ABI_VERSION 1

#ifdef __cplusplus
extern "C" {
#endif

int sai_geno_export_abi_version(void);

/* dosage = int8 [n_rows][n_slots], host memory.  uniform_ploidy in {1, 2} stands in for ploidy_of_slot, which may then
 * be NULL; 0 reads the array.
 * transposed == 0: out = uint8 [n_rows][max(48, (n_slots + 3) / 4)], status = int32 [n_rows] is written for every
 *   row; slot0 must be 0 and n_out n_slots.
 * transposed != 0: the records of the slots [slot0, slot0 + n_out) over all rows: out = uint8 [n_out][max(48,
 *   (n_rows + 3) / 4)].  status = int32 [n_rows] is shared by the calls that cover the slots of a block: it is NOT
 *   zeroed here, a row's value is only ever raised (the caller zeroes it once, before the first call). */
int sai_geno_encode_host(const int8_t* dosage, int64_t n_rows, int32_t n_slots, const int32_t* ploidy_of_slot, int32_t uniform_ploidy,
                         int32_t transposed, int32_t slot0, int32_t n_out, uint8_t* out, int32_t* status, int32_t n_threads);

/* The packed form on the GPU: every pointer is device memory, dosage and out are 16-byte aligned.  One call writes
 * less than 4 GiB of records.  Nothing is read outside [dosage, dosage + n_rows * n_slots), nothing written outside
 * out's n_rows * max(48, (n_slots + 3) / 4) bytes and status's n_rows words; status is zeroed by the call. */
int sai_geno_encode(sai_ctx* ctx, const int8_t* dosage, int64_t n_rows, int32_t n_slots, const int32_t* ploidy_of_slot,
                    int32_t uniform_ploidy, uint8_t* out, int32_t* status, void* stream);

/* The transposed form on the GPU, for the slots [slot0, slot0 + n_out) over all rows of the block: n_out whole records,
 * contiguous in out.  The same pointer rules and the same 4 GiB; status is not zeroed but raised (atomicMax), as
 * sai_geno_encode_host says: calls on one stream, or on several, combine to the maximum. */
int sai_geno_encode_transposed(sai_ctx* ctx, const int8_t* dosage, int64_t n_rows, int32_t n_slots, const int32_t* ploidy_of_slot,
                               int32_t uniform_ploidy, int32_t slot0, int32_t n_out, uint8_t* out, int32_t* status, void* stream);

/* EIGENSOFT's hasharr over the first word of every line of text[n_bytes] (a .ind or a .snp file as it is written: the
 * word ends at a blank or a tab), in file order, in 32-bit unsigned arithmetic:
 *   hashit(s):  h = h * 23 + byte   over the bytes of s, from 0
 *   hasharr:    h = (h * 17) ^ hashit(word)   over the words, from 0
 * Written from memory of admutils.c and not checked against an EIGENSOFT program. */
int sai_geno_hash_lines(const char* text, int64_t n_bytes, uint32_t* hash);

/* The .snp lines "ID CHROM 0.0 POS REF ALT" of the .bim lines "CHROM ID 0 POS ALT REF" that sai_vcf_sites_bim gives,
 * tab-separated; an ID of "." is written CHROM:POS.  *n_out = their length; they are written when out is not NULL and
 * cap >= that length. */
int sai_geno_snp_lines(const char* bim, int64_t n_bytes, char* out, int64_t cap, int64_t* n_out);

#ifdef __cplusplus
}

// One cell of the table, as the host encoder states it: the 2-bit code of dosage `v` at `ploidy`; *fits = false where
// the table has no entry (the code is then 3).
#if defined(__HIPCC__)
__host__ __device__
#endif
inline uint32_t geno_code_of(int32_t v, int32_t ploidy, bool* fits) {
  *fits = true;
  if (v == 0) return 2u;
  if (v == -ploidy) return 3u;
  if (ploidy == 2) {
    if (v == 1) return 1u;
    if (v == 2) return 0u;
  } else if (v == 1) {
    return 0u;
  }
  *fits = false;
  return 3u;
}

// bytes of a record that holds `n` 2-bit fields
inline int64_t geno_record_bytes(int64_t n) { return (n + 3) / 4 < 48 ? 48 : (n + 3) / 4; }
#endif
