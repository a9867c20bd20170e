// What the host decoder (pgen_index.cpp) and the kernel (pgen_decode.hip) of PLINK 2 .pgen records share: the
// recode table of a hard-call code -- one 32-bit word per (ploidy, flipped), its byte c the int8 dosage of code c
// (0 = REF REF, 1 = heterozygous, 2 = ALT ALT, 3 = missing) -- and the constants of the record format.  The
// heterozygous entry of ploidy 1 is 0: such a call is flagged through status[row], never used.
#pragma once

#include <cstdint>

constexpr uint32_t kPgenLutP2 = 0xFE020100u;      //  0, 1, 2, -2
constexpr uint32_t kPgenLutP2Flip = 0x04000102u;  //  2, 1, 0,  4
constexpr uint32_t kPgenLutP1 = 0xFF010000u;      //  0, -, 1, -1
constexpr uint32_t kPgenLutP1Flip = 0x02000001u;  //  1, -, 0,  2
constexpr uint32_t kPgenHet = 1u;
constexpr int32_t kPgenBadIndex = 0x7FFFFFFF;   // SAI_PGEN_STATUS_BAD_INDEX
constexpr int32_t kPgenBadRecord = 0x7FFFFFFE;  // SAI_PGEN_STATUS_BAD_RECORD

constexpr int kPgenGroup = 64;       // entries of a difflist group
constexpr int kPgenMaxVarint = 5;    // bytes of the longest varint that is read: 35 bits, more than any 32-bit count
constexpr int64_t kPgenBlock = 65536;  // variants of a header block

// bytes of a difflist sample index: what the number sample_ct itself takes
#if defined(__HIP_DEVICE_COMPILE__) || defined(__HIPCC__)
__host__ __device__
#endif
inline int pgen_index_width(uint32_t sample_ct) {
  return sample_ct < (1u << 8) ? 1 : sample_ct < (1u << 16) ? 2 : sample_ct < (1u << 24) ? 3 : 4;
}

// the byte after a type 1 record's first one: lo = b / 4, hi = lo + (b & 3), both codes, hi > lo
#if defined(__HIP_DEVICE_COMPILE__) || defined(__HIPCC__)
__host__ __device__
#endif
inline bool pgen_onebit_legal(uint32_t b) { return b == 1 || b == 2 || b == 3 || b == 5 || b == 6 || b == 9; }
