// The recode table of a PLINK 1 genotype code, shared by the host decoder (plink_index.cpp) and the
// kernel (bed_decode.hip): one 32-bit word per (ploidy, flipped), its byte c the int8 dosage of code c
// (00 = A1 A1, 01 = missing, 10 = heterozygous, 11 = A2 A2; A1 plays ALT).  The heterozygous entry of
// ploidy 1 is 0: such a call is flagged through status[row], never used.
#pragma once

#include <cstdint>

constexpr uint32_t kPlinkLutP2 = 0x0001FE02u;      //  2, -2, 1, 0
constexpr uint32_t kPlinkLutP2Flip = 0x02010400u;  //  0,  4, 1, 2
constexpr uint32_t kPlinkLutP1 = 0x0000FF01u;      //  1, -1, -, 0
constexpr uint32_t kPlinkLutP1Flip = 0x01000200u;  //  0,  2, -, 1
constexpr uint32_t kPlinkHet = 2u;
constexpr int32_t kPlinkBadIndex = 0x7FFFFFFF;  // SAI_PLINK_STATUS_BAD_INDEX
