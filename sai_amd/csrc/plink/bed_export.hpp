// Writing a PLINK 1 fileset from a VCF's calls (DESIGN_INGEST.md, "PLINK 1 filesets written from a VCF"): the
// inverse of sai_plink_decode and the host pass over a VCF's site columns.  These entry points are internal to
// the package -- bound by sai_amd/utils/bed_writer.py, which is their only caller -- and no part of the drop-in
// C ABI under include/: they have a version number of their own and may change with the converter.
//
// The encoder reads the int8 [row][slot] block every reader returns and writes variant-major .bed rows: slot i
// goes to bits [2 * (i % 4), +2) of byte i / 4 of its row, the unused bits of a row's last byte are 0.  The codes
// are the unflipped column of include/saihip_plink.h, read backwards:
//
//   ploidy 2:   2 -> 00    1 -> 10    0 -> 11    -2 -> 01
//   ploidy 1:   1 -> 00               0 -> 11    -1 -> 01
//
// Any other value does not fit: its field is written 01 and status[row] = n_slots - s for the lowest such slot s
// (the decoders' convention); a ploidy outside 1 .. 2 writes 01 as well and gives SAI_PLINK_STATUS_BAD_INDEX for
// the row; status[row] = 0 otherwise.
#pragma once

#include <stdint.h>

#include "saihip.h"
#include "saihip_plink.h"

#define SAI_BED_EXPORT_ABI_VERSION 1

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sai_vcf_sites sai_vcf_sites;

int sai_bed_export_abi_version(void);

/* dosage = int8 [n_rows][n_slots], out = uint8 [n_rows][(n_slots + 3) / 4], status = int32 [n_rows]: host memory.
 * uniform_ploidy in {1, 2} stands in for ploidy_of_slot, which may then be NULL; 0 reads the array. */
int sai_bed_encode_host(const int8_t* dosage, int64_t n_rows, int32_t n_slots, const int32_t* ploidy_of_slot,
                        int32_t uniform_ploidy, uint8_t* out, int32_t* status, int32_t n_threads);

/* The same on the GPU: every pointer is device memory, dosage and out are 16-byte aligned.  One call writes less
 * than 4 GiB of rows.  Nothing is read outside [dosage, dosage + n_rows * n_slots), nothing written outside out's
 * n_rows * ((n_slots + 3) / 4) bytes and status's n_rows words. */
int sai_bed_encode(sai_ctx* ctx, const int8_t* dosage, int64_t n_rows, int32_t n_slots, const int32_t* ploidy_of_slot,
                   int32_t uniform_ploidy, uint8_t* out, int32_t* status, void* stream);

/* One pass over a VCF's text (plain: mapped, on n_threads threads that split at line starts; gzip / bgzip: through
 * zlib on one thread) for the records of `chrom` with start <= POS <= end (-1 = open), in file order: POS, ID, REF,
 * the first ALT, whether ALT holds a comma, and the sample names of the #CHROM line.  CHROM is compared as a string;
 * no sample column is looked at. */
int sai_vcf_sites_open(const char* path, const char* chrom, int64_t start, int64_t end, int32_t n_threads, sai_vcf_sites** sites_out);
/* Any pointer may be NULL.  text_bytes = the bytes of all ID, REF and ALT strings; names_bytes = those of the sample names. */
int sai_vcf_sites_info(const sai_vcf_sites* sites, int64_t* n_rows, int64_t* n_samples, int64_t* text_bytes, int64_t* names_bytes);
/* pos[n_rows], multi[n_rows] (ALT holds a comma), text_off[3 * n_rows + 1] (row k: ID, REF, ALT = strings 3k, 3k + 1, 3k + 2
 * of text[text_bytes]), name_off[n_samples + 1] into names[names_bytes]; any may be NULL. */
int sai_vcf_sites_copy(const sai_vcf_sites* sites, int32_t* pos, uint8_t* multi, int64_t* text_off, char* text, int64_t* name_off, char* names);
/* The .bim lines "CHROM ID 0 POS ALT REF", tab-separated, of the rows whose skip[row] is 0 (skip == NULL: all).
 * *n_bytes = their length; they are written when out is not NULL and cap >= that length. */
int sai_vcf_sites_bim(const sai_vcf_sites* sites, const uint8_t* skip, char* out, int64_t cap, int64_t* n_bytes);
int sai_vcf_sites_close(sai_vcf_sites* sites);

#ifdef __cplusplus
}

// One cell of the table, as the host encoder and the kernel's slot-by-slot path state it: the 2-bit code of dosage
// `v` at `ploidy`; *fits = false where the table has no entry (the code is then 01).
#if defined(__HIPCC__)
__host__ __device__
#endif
inline uint32_t bed_code_of(int32_t v, int32_t ploidy, bool* fits) {
  *fits = true;
  if (v == 0) return 3u;
  if (v == ploidy) return 0u;
  if (v == -ploidy) return 1u;
  if (ploidy == 2 && v == 1) return 2u;
  *fits = false;
  return 1u;
}
#endif
