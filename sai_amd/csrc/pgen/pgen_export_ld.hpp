// LD compression for the .pgen records `sai convert --out-pfile --ld-compress` writes (DESIGN_INGEST.md, "LD-compressed
// records"): pgen_export.hpp's encoder with the record types 2 and 3 added.  Internal to the package as that header is:
// bound by sai_amd/utils/pgen_writer.py alone, with a version number of its own, and no part of pgen_export.hpp's ABI,
// which stays as it is.
//
// The rows of a call are taken in segments of SAI_PGEN_LD_SEGMENT consecutive rows, the first at row 0 of the call.
//
//   * The first row of a segment is an anchor: it takes the smallest of the types 0, 1, 4, 6 and 7, as
//     sai_pgen_encode gives it.
//   * Every other row takes the smallest of the types 0, 1, 2, 3, 4, 6 and 7 by exact byte size, a tie going to the
//     lower type.  Its base is the nearest earlier row of the same segment whose type is neither 2 nor 3:
//
//       type 2   D({i : code_i != base_i}): a difflist against the base row
//       type 3   D({i : code_i != swap02(base)_i}): against the base row with the codes 0 and 2 exchanged
//
//     the entries being the row's own codes, and D the difflist of pgen_export.hpp.
//
// A reader finds the base of a type 2 / 3 record as the last record before it of another type: the same row, since
// an anchor is never of type 2 or 3.  16 divides the 65 536 variants of a header block, so as long as the rows of
// a file are encoded in calls of a multiple of 16 rows, a block's first record is an anchor, as the format demands,
// and the file does not depend on how its rows were split into calls.
#pragma once

#include "pgen_export.hpp"

#define SAI_PGEN_EXPORT_LD_VERSION 1
#define SAI_PGEN_LD_SEGMENT 16

#ifdef __cplusplus
extern "C" {
#endif

int sai_pgen_export_ld_version(void);

/* SAI_PGEN_LD_SEGMENT, as the library was built with it */
int sai_pgen_ld_segment(void);

/* sai_pgen_encode_host with the rule above: the same arguments, the same refusals, the same bound on a record. */
int sai_pgen_encode_ld_host(const int8_t* dosage, int64_t n_rows, int32_t n_slots, const int32_t* ploidy_of_slot,
                            int32_t uniform_ploidy, uint8_t* out, int64_t out_cap, uint8_t* vrtype, uint32_t* length,
                            int32_t* status, int64_t* total, int32_t n_threads);

/* sai_pgen_encode with the rule above: the same arguments, refusals and promises about what is read and written.  The
 * plan kernel takes a wavefront per segment, the write kernel one per row; the scan is sai_pgen_encode's. */
int sai_pgen_encode_ld(sai_ctx* ctx, const int8_t* dosage, int64_t n_rows, int32_t n_slots, const int32_t* ploidy_of_slot,
                       int32_t uniform_ploidy, uint8_t* out, uint8_t* vrtype, uint32_t* length, uint32_t* offsets,
                       int32_t* status, int32_t stages, void* stream);

#ifdef __cplusplus
}

// the code a type 3 record's base row holds where the row it stands for holds `code`: 0 and 2 exchanged
#if defined(__HIPCC__)
__host__ __device__
#endif
inline uint32_t pgen_swap02(uint32_t code) { return code ^ ((~code & 1u) << 1); }
#endif
