// sai_packed2_site_freqs_host: the plain statement of include/saihip_packed_stats.h -- per-site allele frequencies of
// packed2 blocks, field by field from the layout formula of saihip.h.  The yardstick of the kernel
// (packed2_freqs.hip), which gives the same doubles bit for bit: both divide two exact integers.

#include <exception>
#include <limits>
#include <new>

#include "packed2_freqs_args.hpp"

namespace {

int packed2_site_freqs_host_impl(int64_t n_sites, int32_t n_pops, const sai_pop* pops, double* freqs, int32_t n_threads) {
  if (int rc = packed2_freqs_check_sizes(n_sites, n_pops, pops)) return rc;
  if (n_sites == 0) return SAI_OK;
  if (int rc = packed2_freqs_check_pops(n_pops, pops, freqs, false)) return rc;
  for (int p = 0; p < n_pops; ++p) {
    const uint8_t* block = reinterpret_cast<const uint8_t*>(pops[p].tiles);
    const int32_t n_ind = pops[p].n_ind, ploidy = pops[p].ploidy;
    const int n_full = packed2_full_groups(n_ind), w_tail = packed2_tail_words(n_ind);
    const int64_t tile_words = packed2_tile_words(n_ind);
    double* out = freqs + static_cast<int64_t>(p) * n_sites;
    auto count = [=](int64_t lo, int64_t hi) {
      for (int64_t site = lo; site < hi; ++site) {
        const int64_t tile = site / 64, s = site % 64;
        uint32_t ones = 0, twos = 0, miss = 0;
        for (int32_t i = 0; i < n_ind; ++i) {
          const int g = i / 64, j = (i % 64) / 16;
          const int64_t in_tile = g < n_full ? static_cast<int64_t>(g) * 256 + s * 4 + j : static_cast<int64_t>(n_full) * 256 + s * w_tail + j;
          uint32_t word;
          std::memcpy(&word, block + (tile * tile_words + in_tile) * 4, 4);
          const uint32_t field = (word >> (2 * (i % 16))) & 3u;
          ones += field == 1;
          twos += field == 2;
          miss += field == 3;
        }
        const uint32_t alt = ones + 2u * twos, called = static_cast<uint32_t>(n_ind) - miss;
        const int64_t den = static_cast<int64_t>(called) * ploidy;
        out[site] = den > 0 ? static_cast<double>(alt) / static_cast<double>(den) : std::numeric_limits<double>::quiet_NaN();
      }
    };
    packed2_for_rows(n_threads, n_sites, n_sites * static_cast<int64_t>(n_ind), count);
  }
  return SAI_OK;
}

}  // namespace

extern "C" {

int sai_packed_stats_abi_version(void) { return SAI_PACKED_STATS_ABI_VERSION; }

int sai_packed2_site_freqs_host(int64_t n_sites, int32_t n_pops, const sai_pop* pops, double* freqs, int32_t n_threads) {
  try {
    return packed2_site_freqs_host_impl(n_sites, n_pops, pops, freqs, n_threads);
  } catch (const std::bad_alloc&) {
    return sai_set_error(SAI_ERR_HIP, "sai_packed2_site_freqs_host: out of host memory");
  } catch (const std::exception& e) {
    return sai_set_error(SAI_ERR_HIP, "sai_packed2_site_freqs_host: %s", e.what());
  }
}

}  // extern "C"
