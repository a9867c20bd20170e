// The argument checks of sai_packed2_site_freqs and its host twin (include/saihip_packed_stats.h), in the words and
// with the codes of sai_site_pass_packed2 (../packed2.hip).  The layout's geometry comes from
// ../plink/packed2_layout.hpp.
#pragma once

#include <cstdint>

#include "../plink/packed2_layout.hpp"
#include "saihip_packed_stats.h"

extern "C" int sai_set_error(int code, const char* fmt, ...);

// What is checked before n_sites == 0 returns SAI_OK ...
inline int packed2_freqs_check_sizes(int64_t n_sites, int32_t n_pops, const sai_pop* pops) {
  if (n_sites < 0 || n_sites >= 0x7FFFFFFFll) return sai_set_error(SAI_ERR_ARG, "n_sites out of range");
  if (n_pops < 1 || n_pops > SAI_PACKED_FREQ_POPS) return sai_set_error(SAI_ERR_ARG, "n_pops must be 1..%d", SAI_PACKED_FREQ_POPS);
  if (!pops) return sai_set_error(SAI_ERR_ARG, "pops is NULL");
  return SAI_OK;
}

// ... and behind it.  `device`: the blocks are read with 16-byte loads and must be aligned for them.
inline int packed2_freqs_check_pops(int32_t n_pops, const sai_pop* pops, const double* freqs, bool device) {
  if (!freqs) return sai_set_error(SAI_ERR_ARG, "NULL buffer");
  for (int p = 0; p < n_pops; ++p) {
    if (pops[p].n_ind < 1 || pops[p].n_ind > kPackedMaxInd)
      return sai_set_error(SAI_ERR_UNSUPPORTED, "population %d: packed2 supports 1..%d individuals", p, kPackedMaxInd);
    if (device && (!pops[p].tiles || (reinterpret_cast<uintptr_t>(pops[p].tiles) & 15u)))
      return sai_set_error(SAI_ERR_ARG, "population %d: packed block must be a 16-byte aligned device pointer", p);
    if (!pops[p].tiles) return sai_set_error(SAI_ERR_ARG, "population %d: packed block is NULL", p);
    if (pops[p].ploidy <= 0) return sai_set_error(SAI_ERR_ARG, "ploidy[%d] must be positive", p);
  }
  return SAI_OK;
}
