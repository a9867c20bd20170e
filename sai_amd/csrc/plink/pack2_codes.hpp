// The packed2 field of a PLINK 1 genotype code, shared by the host decoder (bed_pack2_host.cpp) and the kernel
// (bed_pack2.hip): the table of include/saihip_packed_ingest.h.  It restates the int8 table of plink_codes.hpp
// (dosage 0, 1, 2 stays; a negative dosage is 3) with two entries that are no field: a heterozygous call at ploidy 1
// (flagged through status[row], as there) and a missing call in a flipped row at ploidy 2 (dosage 4: flagged
// through unfit[row]).  The host decoder reads the table entry by entry; the kernel applies it to the 16 fields
// of a word at once (pack2_recode).
#pragma once

#include <cstdint>

#include "plink_codes.hpp"

constexpr uint8_t kPack2Het = 0x10;    // no field: refused (ploidy 1)
constexpr uint8_t kPack2Unfit = 0x20;  // no field: dosage 4
// [ploidy - 1][flipped][code 00, 01, 10, 11]
constexpr uint8_t kPack2Table[2][2][4] = {
    {{1, 3, kPack2Het, 0}, {0, 2, kPack2Het, 1}},
    {{2, 3, 1, 0}, {0, kPack2Unfit, 1, 2}},
};

#if defined(__HIPCC__)
// 16 codes of one word -> 16 fields.  `valid` has bit 2k set for every field k that is an individual's (the
// others come out 0 and raise nothing); het / unfit have bit 2k set where field k is refused / does not fit.
// Bit operations on the two planes of the word (bit 0 and bit 1 of every code): no loop over the fields and
// no branch on a code.  PLOIDY is the call's; `flip` is the row's, applied as a mask.
template <int PLOIDY>
__device__ __forceinline__ uint32_t pack2_recode(uint32_t codes, uint32_t valid, bool flip, uint32_t& het, uint32_t& unfit) {
  const uint32_t lo = codes & valid, hi = (codes >> 1) & valid;
  const uint32_t a1a1 = ~(codes | (codes >> 1)) & valid;  // 00
  const uint32_t miss = lo & ~hi;                         // 01
  const uint32_t a1a2 = hi & ~lo;                         // 10
  const uint32_t a2a2 = hi & lo;                          // 11
  const uint32_t f = flip ? 0xFFFFFFFFu : 0u;
  uint32_t out_lo, out_hi;
  if (PLOIDY == 2) {
    // kept: 00 -> 2, 10 -> 1, 11 -> 0, 01 -> 3;  flipped: 00 -> 0, 10 -> 1, 11 -> 2, 01 -> unfit
    out_lo = a1a2 | (miss & ~f);
    out_hi = ((a1a1 | miss) & ~f) | (a2a2 & f);
    het = 0u;
    unfit = miss & f;
  } else {
    // kept: 00 -> 1, 11 -> 0, 01 -> 3;  flipped: 00 -> 0, 11 -> 1, 01 -> 2;  10 -> refused
    out_lo = ((a1a1 | miss) & ~f) | (a2a2 & f);
    out_hi = miss;
    het = a1a2;
    unfit = 0u;
  }
  return out_lo | (out_hi << 1);
}
#endif
