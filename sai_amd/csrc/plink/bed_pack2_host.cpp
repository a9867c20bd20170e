// sai_bed_pack2_host: the plain statement of include/saihip_packed_ingest.h -- variant-major PLINK 1 .bed rows ->
// one population's block in the packed2 layout of saihip.h, field by field from the table of pack2_codes.hpp.  The
// yardstick of the kernel (bed_pack2.hip), which makes the same decisions with the same status / unfit values.

#include <algorithm>
#include <cstring>
#include <exception>
#include <new>

#include "../host_threads.hpp"
#include "packed2_layout.hpp"
#include "pack2_codes.hpp"
#include "saihip_packed_ingest.h"

extern "C" int sai_set_error(int code, const char* fmt, ...);

namespace {

int bed_pack2_host_impl(const uint8_t* rows, int64_t n_batch_rows, int64_t row_bytes, int64_t n_out_rows,
                        const int32_t* row_in_batch, const uint8_t* row_flip, int32_t n_cols, int32_t n_ind,
                        const int32_t* col_of_ind, int32_t first_col, int32_t ploidy, uint8_t* packed, int64_t n_sites,
                        int64_t out_row0, int32_t* status, int32_t* unfit, int32_t n_threads) {
  if (n_batch_rows < 0 || row_bytes < 0 || n_cols < 0 || !packed2_sizes_ok(n_out_rows, n_ind, n_sites, out_row0))
    return sai_set_error(SAI_ERR_ARG, "size out of range");
  if (static_cast<int64_t>(n_cols) > 4 * row_bytes) return sai_set_error(SAI_ERR_ARG, "n_cols exceeds the 4 * row_bytes genotypes of a row");
  if (const char* why = packed2_bad_selection(ploidy, first_col, n_ind, n_cols, "first_col + n_slots exceeds n_cols")) return sai_set_error(SAI_ERR_ARG, "%s", why);
  if (n_out_rows == 0) return SAI_OK;
  if (!row_in_batch || !row_flip || !packed || !status || !unfit || (first_col < 0 && !col_of_ind) ||
      (n_batch_rows > 0 && row_bytes > 0 && !rows))
    return sai_set_error(SAI_ERR_ARG, "NULL buffer");
  const Packed2Block block(packed, n_ind);
  auto decode = [&](int64_t lo, int64_t hi) {
    for (int64_t r = lo; r < hi; ++r) {
      int32_t st = 0, uf = 0;
      const int64_t rib = row_in_batch[r];
      const bool row_ok = rib >= 0 && rib < n_batch_rows;
      const uint8_t* src = row_ok ? rows + rib * row_bytes : nullptr;
      const uint8_t* table = kPack2Table[ploidy - 1][row_flip[r] != 0];
      for (int j = 0; j < block.words_per_site; ++j) {
        uint32_t word = 0;
        for (int k = 0; k < 16; ++k) {
          const int32_t i = j * 16 + k;
          if (i >= n_ind) break;  // padding individuals: 0
          const int32_t col = first_col >= 0 ? first_col + i : col_of_ind[i];
          if (!row_ok || col < 0 || col >= n_cols) {
            st = kPlinkBadIndex;
            continue;
          }
          const uint8_t field = table[(src[col >> 2] >> (2 * (col & 3))) & 3u];
          if (field == kPack2Het) st = std::max(st, n_ind - i);
          else if (field == kPack2Unfit) uf = std::max(uf, n_ind - i);
          else word |= static_cast<uint32_t>(field) << (2 * k);
        }
        block.put(out_row0 + r, j, word);
      }
      status[r] = st;
      unfit[r] = uf;
    }
  };
  const int64_t cells = n_out_rows * static_cast<int64_t>(n_ind);
  packed2_for_rows(n_threads, n_out_rows, cells, decode);
  block.pad(out_row0 + n_out_rows, n_sites);
  return SAI_OK;
}

}  // namespace

extern "C" {

int sai_packed_ingest_abi_version(void) { return SAI_PACKED_INGEST_ABI_VERSION; }

int sai_bed_pack2_host(const uint8_t* rows, int64_t n_batch_rows, int64_t row_bytes, int64_t n_out_rows,
                       const int32_t* row_in_batch, const uint8_t* row_flip, int32_t n_cols, int32_t n_ind,
                       const int32_t* col_of_ind, int32_t first_col, int32_t ploidy, uint8_t* packed, int64_t n_sites,
                       int64_t out_row0, int32_t* status, int32_t* unfit, int32_t n_threads) {
  try {
    return bed_pack2_host_impl(rows, n_batch_rows, row_bytes, n_out_rows, row_in_batch, row_flip, n_cols, n_ind, col_of_ind,
                               first_col, ploidy, packed, n_sites, out_row0, status, unfit, n_threads);
  } catch (const std::bad_alloc&) {
    return sai_set_error(SAI_ERR_HIP, "sai_bed_pack2_host: out of host memory");
  } catch (const std::exception& e) {
    return sai_set_error(SAI_ERR_HIP, "sai_bed_pack2_host: %s", e.what());
  }
}

}  // extern "C"
