// The geometry of the packed2 layout of saihip.h, as ../packed2.hip defines it next to the kernels that read it,
// restated for the kernel that decodes .bed rows into the layout (bed_pack2.hip) and for the host statement of that
// decoder (bed_pack2_host.cpp): plain functions, usable with and without a device compiler.  (packed2.hip keeps its
// own copy: the stored figures of profiles/ name the digest of the sources they were measured on, that file among
// them.  tests/test_bed_pack2_device.py holds the two together: the kernel's blocks equal sai_pack2_from_tiles'.)
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SAI_PACKED2_HD __host__ __device__ __forceinline__
#else
#define SAI_PACKED2_HD inline
#endif

constexpr int kPackedMaxInd = 1 << 24;  // as for the int8 layout: per-site totals are 32-bit

SAI_PACKED2_HD int packed2_full_groups(int n_ind) { return n_ind / 64; }
SAI_PACKED2_HD int packed2_tail_words(int n_ind) { return ((n_ind % 64) + 15) / 16; }
SAI_PACKED2_HD int64_t packed2_tile_words(int n_ind) {
  return static_cast<int64_t>(packed2_full_groups(n_ind)) * 256 + packed2_tail_words(n_ind) * 64;
}
