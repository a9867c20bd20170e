// The packed2 field of a PLINK 2 hard-call code, shared by the host decoder (pgen_pack2_host.cpp) and the kernel
// (pgen_pack2.hip): the table of include/saihip_pgen_packed.h.  It restates the int8 table of pgen_codes.hpp where
// that fits two bits (dosage 0, 1, 2 stays; a negative dosage is 3) with two entries that are no field: a
// heterozygous call at ploidy 1 (flagged through status[row], as there) and a missing call in a flipped row at
// ploidy 2 (dosage 4: flagged through unfit[row]).  The host decoder reads the table entry by entry; the kernel
// applies it to the 16 fields of a word at once (pgen_pack2_recode).
#pragma once

#include <cstdint>

#include "pgen_codes.hpp"

constexpr uint8_t kPgenPack2Het = 0x10;    // no field: refused (ploidy 1)
constexpr uint8_t kPgenPack2Unfit = 0x20;  // no field: dosage 4
// [ploidy - 1][flipped][code 0, 1, 2, 3]
constexpr uint8_t kPgenPack2Table[2][2][4] = {
    {{0, kPgenPack2Het, 1, 3}, {1, kPgenPack2Het, 0, 2}},
    {{0, 1, 2, 3}, {2, 1, 0, kPgenPack2Unfit}},
};

#if defined(__HIPCC__)
// 16 codes of one word -> 16 fields.  `valid` has bit 2k set for every field k that is an individual's (the
// others come out 0 and raise nothing); het / unfit have bit 2k set where field k is refused / does not fit.
// Bit operations on the two planes of the word (bit 0 and bit 1 of every code): no loop over the fields and no
// branch on a code.  PLOIDY is the call's; `flip` is the row's (wave-uniform).
template <int PLOIDY>
__device__ __forceinline__ uint32_t pgen_pack2_recode(uint32_t codes, uint32_t valid, bool flip, uint32_t& het, uint32_t& unfit) {
  const uint32_t both = valid | (valid << 1);
  const uint32_t lo = codes & valid, hi = (codes >> 1) & valid;
  het = 0u;
  unfit = 0u;
  if (PLOIDY == 2) {
    if (!flip) return codes & both;  // the field is the code
    unfit = hi & lo;                 // missing: dosage 4
    // 0 <-> 2: the high bit of a field whose low bit is clear; 1 stays, the code-3 fields are zeroed
    return (codes ^ ((~codes & 0x55555555u) << 1)) & both & ~(unfit | (unfit << 1));
  }
  het = lo & ~hi;
  // kept: 0 -> 0, 2 -> 1, 3 -> 3;  flipped: 0 -> 1, 2 -> 0, 3 -> 2;  1 -> refused, 0
  const uint32_t out_lo = flip ? ~(hi | lo) & valid : hi;
  return out_lo | ((hi & lo) << 1);
}
#endif
