// The recode table of an EIGENSTRAT genotype value, shared by the host decoder (eigenstrat_index.cpp) and the
// kernels (geno_decode.hip, geno_transpose.hip): one 32-bit word per (ploidy, flipped), its byte c the int8
// dosage of code c (0, 1, 2 = copies of the first allele, which plays REF; 3 = missing).  The g = 1 entry of
// ploidy 1 is 0: such a call is flagged through status[row], never used.
#pragma once

#include <cstdint>

constexpr uint32_t kGenoLutP2 = 0xFE000102u;      //  2, 1, 0, -2
constexpr uint32_t kGenoLutP2Flip = 0x04020100u;  //  0, 1, 2,  4
constexpr uint32_t kGenoLutP1 = 0xFF000001u;      //  1, -, 0, -1
constexpr uint32_t kGenoLutP1Flip = 0x02010000u;  //  0, -, 1,  2
constexpr uint32_t kGenoHet = 1u;
constexpr uint32_t kGenoBadCode = 4u;             // of a text character outside 0 1 2 9
constexpr int32_t kGenoBadIndex = 0x7FFFFFFF;     // SAI_EIGENSTRAT_STATUS_BAD_INDEX
constexpr int32_t kGenoBadChar = 0x7FFFFFFE;      // SAI_EIGENSTRAT_STATUS_BAD_CHAR

// the code of a text character: '0' '1' '2' -> 0 1 2, '9' -> 3, anything else -> kGenoBadCode
#if defined(__HIPCC__)
__host__ __device__
#endif
inline uint32_t geno_code_of_char(uint32_t c) {
  const uint32_t d = c - 48u;
  return d <= 2u ? d : (d == 9u ? 3u : kGenoBadCode);
}
