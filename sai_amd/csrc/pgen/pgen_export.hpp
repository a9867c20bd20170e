// Writing a PLINK 2 fileset from a VCF's calls (DESIGN_INGEST.md, "PLINK 2 filesets written from a VCF"): the
// inverse of sai_pgen_decode.  These entry points are internal to the package -- bound by
// sai_amd/utils/pgen_writer.py, which is their only caller -- and no part of the drop-in C ABI under include/:
// they have a version number of their own and may change with the converter.
//
// The encoder reads the int8 [row][slot] block every reader returns and writes, per row, the hard-call track of one
// .pgen record; the records of a call stand back to back in row order.  The codes are the unflipped columns of
// include/saihip_pgen.h, read backwards:
//
//   ploidy 2:   0 -> 0    1 -> 1    2 -> 2    -2 -> 3
//   ploidy 1:   0 -> 0              1 -> 2    -1 -> 3
//
// Any other value does not fit: its code is written 3 and status[row] = n_slots - s for the lowest such slot s (the
// decoders' convention); a ploidy outside 1 .. 2 writes 3 as well and gives SAI_PGEN_STATUS_BAD_INDEX for the row;
// status[row] = 0 otherwise.
//
// Every row takes the smallest of the record types 0, 1, 4, 6 and 7 by exact byte size, a tie going to the lower
// type (types 2 and 3, differences from an earlier record, are never written):
//
//   type 0          ceil(n / 4): the dense 2-bit codes
//   type 4 / 6 / 7  D({i : code_i != c}) for c = 0 / 2 / 3: a difflist against a constant row
//   type 1          1 + ceil(n / 8) + D({i : code_i not in {lo, hi}}): the byte 4 lo + (hi - lo), one bit per sample
//                   (set: hi), a difflist; (lo, hi) = the two most common codes of the row, a tie going to the
//                   higher code
//
// A difflist of L sorted entries is varint(L); when L > 0, per group of 64 entries the sample index of its first
// entry in w bytes (w = the bytes of the number n_slots), per group but the last the byte size of its deltas - 63,
// the entries' codes in 2 bits each, and per group the varints of the differences between consecutive entries.
#pragma once

#include <stdint.h>

#include "saihip.h"
#include "saihip_pgen.h"

#define SAI_PGEN_EXPORT_ABI_VERSION 1
#define SAI_PGEN_ENCODE_PLAN 1  /* vrtype, length, status */
#define SAI_PGEN_ENCODE_SCAN 2  /* offsets */
#define SAI_PGEN_ENCODE_WRITE 4 /* out */
#define SAI_PGEN_ENCODE_ALL 7

#ifdef __cplusplus
extern "C" {
#endif

int sai_pgen_export_abi_version(void);

/* dosage = int8 [n_rows][n_slots], out = uint8 [out_cap], vrtype = uint8 [n_rows], length = uint32 [n_rows],
 * status = int32 [n_rows], *total = the bytes of all records: host memory.  uniform_ploidy in {1, 2} stands in for
 * ploidy_of_slot, which may then be NULL; 0 reads the array.  No record is longer than (n_slots + 3) / 4 bytes, so
 * out_cap = n_rows * ((n_slots + 3) / 4) always suffices; a smaller out_cap that the records do not fit in is refused
 * after vrtype, length and *total are written and before a byte of out is. */
int sai_pgen_encode_host(const int8_t* dosage, int64_t n_rows, int32_t n_slots, const int32_t* ploidy_of_slot,
                         int32_t uniform_ploidy, uint8_t* out, int64_t out_cap, uint8_t* vrtype, uint32_t* length,
                         int32_t* status, int64_t* total, int32_t n_threads);

/* The same on the GPU: every pointer is device memory and dosage is 16-byte aligned.  offsets = uint32 [n_rows + 1]:
 * offsets[r] = the byte of out at which record r starts, offsets[n_rows] = the bytes of all records.  out holds
 * n_rows * ((n_slots + 3) / 4) bytes, which is less than 4 GiB.  Nothing is read outside
 * [dosage, dosage + n_rows * n_slots), nothing written outside the first offsets[n_rows] bytes of out and the
 * n_rows (n_rows + 1) elements of the four tables.  stages = SAI_PGEN_ENCODE_ALL; tools/pgen_export_rate.py times the
 * three kernels one by one with a single bit each (a later stage reads what the earlier ones wrote). */
int sai_pgen_encode(sai_ctx* ctx, const int8_t* dosage, int64_t n_rows, int32_t n_slots, const int32_t* ploidy_of_slot,
                    int32_t uniform_ploidy, uint8_t* out, uint8_t* vrtype, uint32_t* length, uint32_t* offsets,
                    int32_t* status, int32_t stages, void* stream);

/* The .pvar lines "CHROM POS ID REF ALT" of the .bim lines "CHROM ID 0 POS ALT REF" that sai_vcf_sites_bim writes
 * (tab-separated, every line ended by a newline): the same bytes in another order, two fewer per line.  out holds at
 * least n_bytes bytes; *n_out = the bytes written.  A line without six columns is refused. */
int sai_pgen_pvar_lines(const char* bim, int64_t n_bytes, char* out, int64_t* n_out);

/* Rows a plan / write grid of sai_pgen_encode takes at most before it strides: 16 wavefronts per compute unit. */
int64_t sai_pgen_encode_grid_cap(sai_ctx* ctx);

#ifdef __cplusplus
}

// One cell of the table, as the host encoder states it: the 2-bit code of dosage `v` at `ploidy`; *fits = false
// where the table has no entry (the code is then 3).
#if defined(__HIPCC__)
__host__ __device__
#endif
inline uint32_t pgen_code_of(int32_t v, int32_t ploidy, bool* fits) {
  *fits = true;
  if (v == 0) return 0u;
  if (v == ploidy) return 2u;
  if (v == -ploidy) return 3u;
  if (ploidy == 2 && v == 1) return 1u;
  *fits = false;
  return 3u;
}

// bytes of the base-128 varint of `v`
#if defined(__HIPCC__)
__host__ __device__
#endif
inline uint32_t pgen_varint_len(uint32_t v) { return v < (1u << 7) ? 1u : v < (1u << 14) ? 2u : v < (1u << 21) ? 3u : v < (1u << 28) ? 4u : 5u; }

// The two codes a type 1 record stores as bits: the two most common of the row, a tie going to the higher code.
#if defined(__HIPCC__)
__host__ __device__
#endif
inline void pgen_onebit_pair(const uint32_t count[4], uint32_t* lo, uint32_t* hi) {
  uint32_t first = 3;
  for (int c = 2; c >= 0; --c)
    if (count[c] > count[first]) first = static_cast<uint32_t>(c);
  uint32_t second = first == 3 ? 2 : 3;
  for (int c = static_cast<int>(second) - 1; c >= 0; --c)
    if (static_cast<uint32_t>(c) != first && count[c] > count[second]) second = static_cast<uint32_t>(c);
  *lo = first < second ? first : second;
  *hi = first < second ? second : first;
}
#endif
