// The recode step the 2-bit decoders share (bed_decode.hip here, ../pgen/pgen_decode.hip): a lane's 16 two-bit
// codes -- code k in bits [2k, 2k + 2) of one 32-bit word -- go through the table of a (ploidy, flipped) pair, four
// packed bytes selected by shifts, and come out as the 16 output bytes of one 128-bit store.  Only the tables differ
// between the formats (plink_codes.hpp, ../pgen/pgen_codes.hpp).
#pragma once

#include "../common.hpp"

//
// A macro, not a function: bed_decode_kernel was tuned with this loop nest written out in its body, and both an
// inlined helper per 32-bit word and one per 128-bit word changed the instructions the compiler emits for it (other
// v_perm selectors, another schedule).  Expanded as text the kernel's code is, instruction for instruction, what it was.
// word (u32x4) = the 16 output bytes of `codes`, or zeros when `ok` is false.
#define SAI_RECODE16(codes, lut, ok, word)                              \
  _Pragma("unroll") for (int j = 0; j < 4; ++j) {                       \
    uint32_t w = 0;                                                     \
    _Pragma("unroll") for (int k = 0; k < 4; ++k) {                     \
      const uint32_t code = ((codes) >> (2 * (4 * j + k))) & 3u;        \
      w |= (((lut) >> (8 * code)) & 0xFFu) << (8 * k);                  \
    }                                                                   \
    (word)[j] = (ok) ? w : 0u;                                          \
  }
