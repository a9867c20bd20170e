// The geometry of the packed2 layout of saihip.h, as ../packed2.hip defines it next to the kernels that read it,
// restated for the decoders that write it -- .bed rows (bed_pack2.hip, bed_pack2_host.cpp) and .pgen records
// (../pgen/pgen_pack2.hip, ../pgen/pgen_pack2_host.cpp) -- with what those four say alike: the argument checks, where
// a site's words go, the padding of the last tile, the launch.  Plain functions, usable with and without a device
// compiler; the device half expects ../common.hpp before it.  (packed2.hip keeps its own copy: the stored figures of
// profiles/ name the digest of the sources they were measured on, that file among them.
// tests/test_bed_pack2_device.py holds the two together: the kernel's blocks equal sai_pack2_from_tiles'.)
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SAI_PACKED2_HD __host__ __device__ __forceinline__
#else
#include "../host_threads.hpp"
#define SAI_PACKED2_HD inline
#endif

constexpr int kPackedMaxInd = 1 << 24;  // as for the int8 layout: per-site totals are 32-bit

SAI_PACKED2_HD int packed2_full_groups(int n_ind) { return n_ind / 64; }
SAI_PACKED2_HD int packed2_tail_words(int n_ind) { return ((n_ind % 64) + 15) / 16; }
SAI_PACKED2_HD int64_t packed2_tile_words(int n_ind) {
  return static_cast<int64_t>(packed2_full_groups(n_ind)) * 256 + packed2_tail_words(n_ind) * 64;
}

// The checks of the arguments every entry point takes, in two steps (a format's own checks go between them).
inline bool packed2_sizes_ok(int64_t n_out_rows, int32_t n_ind, int64_t n_sites, int64_t out_row0) {
  return n_out_rows >= 0 && n_ind >= 1 && n_ind <= kPackedMaxInd && out_row0 >= 0 && n_sites >= 0 && n_sites < 0x7FFFFFFFll &&
         out_row0 <= n_sites && n_out_rows <= n_sites - out_row0;
}
// nullptr, or what is wrong; `run_too_long` = the format's words for a run of columns that ends behind the n_cols there are
inline const char* packed2_bad_selection(int32_t ploidy, int32_t first_col, int32_t n_ind, int64_t n_cols, const char* run_too_long) {
  if (ploidy != 1 && ploidy != 2) return "ploidy must be 1 or 2";
  return first_col >= 0 && static_cast<int64_t>(first_col) + n_ind > n_cols ? run_too_long : nullptr;
}

#if defined(__HIPCC__)

// bit 2k set for every field k < n (any n: none below 1, all from 16 on)
__device__ __forceinline__ uint32_t valid_fields(int n) {
  return n >= 16 ? 0x55555555u : (n <= 0 ? 0u : (0x55555555u & ((1u << (2 * n)) - 1u)));
}

// The four words of group g of one site of the tile at `out`: a full group's are one 16-byte store (64 sites x 16 B =
// the group's 1 KiB block), the tail group's w_tail words lie back to back behind the full groups.
__device__ __forceinline__ void packed2_store_group(uint32_t* out, int n_full, int w_tail, int site_in_tile, int g, const u32x4& word) {
  if (g < n_full) {
    reinterpret_cast<u32x4*>(out)[g * kTile + site_in_tile] = word;
  } else {
    uint32_t* tw = out + static_cast<int64_t>(n_full) * 256 + site_in_tile * w_tail;
    tw[0] = word[0];
    if (w_tail > 1) tw[1] = word[1];
    if (w_tail > 2) tw[2] = word[2];
    if (w_tail > 3) tw[3] = word[3];
  }
}

// n_full, w_tail and n_groups (= n_full + (w_tail != 0)) of a kernel's arguments: the layout of n_ind
template <typename Args>
void packed2_set_groups(Args& a, int32_t n_ind) {
  a.n_full = packed2_full_groups(n_ind);
  a.w_tail = packed2_tail_words(n_ind);
  a.n_groups = a.n_full + (a.w_tail ? 1 : 0);
}

// The end of an entry point: the call's status and unfit cleared, then the <PLOIDY, FAST> instance of `kernel` that
// `ploidy` and a.first_col pick, all on `stream`.
#define SAI_PACKED2_LAUNCH(kernel, a, ploidy, n_out_rows, grid, block, stream)                               \
  do {                                                                                                      \
    hipStream_t st_ = static_cast<hipStream_t>(stream);                                                     \
    SAI_HIP(hipMemsetAsync((a).status, 0, static_cast<size_t>(n_out_rows) * sizeof(int32_t), st_));         \
    SAI_HIP(hipMemsetAsync((a).unfit, 0, static_cast<size_t>(n_out_rows) * sizeof(int32_t), st_));          \
    if ((ploidy) == 2 && (a).first_col >= 0) hipLaunchKernelGGL((kernel<2, true>), grid, block, 0, st_, a); \
    else if ((ploidy) == 2) hipLaunchKernelGGL((kernel<2, false>), grid, block, 0, st_, a);                 \
    else if ((a).first_col >= 0) hipLaunchKernelGGL((kernel<1, true>), grid, block, 0, st_, a);             \
    else hipLaunchKernelGGL((kernel<1, false>), grid, block, 0, st_, a);                                    \
  } while (0)

#else

// Where the host decoders write: word j of a site (16 individuals from 16 * j on) inside its tile -- full groups
// site-major, then the tail block.
struct Packed2Block {
  uint8_t* packed;
  int n_full, w_tail, words_per_site;
  int64_t tile_words;
  Packed2Block(uint8_t* p, int n_ind)
      : packed(p), n_full(packed2_full_groups(n_ind)), w_tail(packed2_tail_words(n_ind)), words_per_site(n_full * 4 + w_tail),
        tile_words(packed2_tile_words(n_ind)) {}
  void put(int64_t site, int j, uint32_t word) const {
    const int64_t tile = site / 64, s = site % 64;
    const int64_t in_tile = j < n_full * 4 ? static_cast<int64_t>(j / 4) * 256 + s * 4 + j % 4
                                           : static_cast<int64_t>(n_full) * 256 + s * w_tail + (j - n_full * 4);
    std::memcpy(packed + (tile * tile_words + in_tile) * 4, &word, 4);
  }
  // the padding sites of the last tile, by the call that holds the last site: all missing
  void pad(int64_t row_end, int64_t n_sites) const {
    for (int64_t site = n_sites; row_end == n_sites && site % 64 != 0; ++site)
      for (int j = 0; j < words_per_site; ++j) put(site, j, 0xFFFFFFFFu);
  }
};

// decode(lo, hi) over the rows [0, n_rows) on up to n_threads threads, one for every 2^18 `cells` of work
template <typename F>
void packed2_for_rows(int32_t n_threads, int64_t n_rows, int64_t cells, F&& decode) {
  const int nt = static_cast<int>(std::max<int64_t>(1, std::min<int64_t>({static_cast<int64_t>(std::max(n_threads, 1)), n_rows, cells / (int64_t(1) << 18) + 1})));
  ThreadGroup tg;
  for (int t = 1; t < nt; ++t) tg.spawn([&decode, t, nt, n_rows] { decode(n_rows * t / nt, n_rows * (t + 1) / nt); });
  decode(0, n_rows / nt);
  tg.join();
}

#endif
