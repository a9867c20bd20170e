// sai_pgen_pack2_host: the plain statement of include/saihip_pgen_packed.h -- the records of a PLINK 2 .pgen -> one
// population's block in the packed2 layout of saihip.h.  A record is expanded to one code per sample by the rules
// sai_pgen_decode_host reads it by (pgen_expand_host.hpp: stated once), then every field comes from the table of
// pgen_pack2_codes.hpp, one by one.  The yardstick of the kernel (pgen_pack2.hip), which makes the same decisions
// with the same status / unfit values.

#include <atomic>
#include <exception>
#include <new>
#include <vector>

#include "../host_threads.hpp"
#include "../plink/packed2_layout.hpp"
#include "pgen_expand_host.hpp"
#include "pgen_pack2_codes.hpp"
#include "saihip_pgen_packed.h"

extern "C" int sai_set_error(int code, const char* fmt, ...);

namespace {

int pgen_pack2_host_impl(const uint8_t* bytes, int64_t n_bytes, int64_t n_out_rows, const int64_t* rec, const int64_t* base,
                         const uint8_t* row_flip, int32_t sample_ct, int32_t n_ind, const int32_t* col_of_ind, int32_t first_col,
                         int32_t ploidy, uint8_t* packed, int64_t n_sites, int64_t out_row0, int32_t* status, int32_t* unfit,
                         int32_t n_threads) {
  if (n_bytes < 0 || sample_ct < 1 || !packed2_sizes_ok(n_out_rows, n_ind, n_sites, out_row0)) return sai_set_error(SAI_ERR_ARG, "size out of range");
  if (const char* why = packed2_bad_selection(ploidy, first_col, n_ind, sample_ct, "first_col + n_slots exceeds sample_ct")) return sai_set_error(SAI_ERR_ARG, "%s", why);
  if (n_out_rows == 0) return SAI_OK;
  if (!rec || !base || !row_flip || !packed || !status || !unfit || (first_col < 0 && !col_of_ind) || (n_bytes > 0 && !bytes))
    return sai_set_error(SAI_ERR_ARG, "NULL buffer");
  const uint32_t n = static_cast<uint32_t>(sample_ct);
  const Packed2Block block(packed, n_ind);
  std::atomic<bool> failed{false};
  auto decode = [&](int64_t lo, int64_t hi) {
    std::vector<uint8_t> codes;
    try {
      codes.resize(n);
    } catch (...) {
      failed = true;
      return;
    }
    for (int64_t r = lo; r < hi; ++r) {
      const RecordRef own = {rec[3 * r], rec[3 * r + 1], rec[3 * r + 2]};
      const RecordRef from = {base[3 * r], base[3 * r + 1], base[3 * r + 2]};
      const bool sound = expand_record(bytes, n_bytes, own, from, n, codes.data());
      int32_t st = sound ? 0 : kPgenBadRecord, uf = 0;
      const uint8_t* table = kPgenPack2Table[ploidy - 1][row_flip[r] != 0];
      for (int j = 0; j < block.words_per_site; ++j) {
        uint32_t word = 0;
        for (int k = 0; sound && k < 16; ++k) {  // a bad row: every field 0
          const int32_t i = j * 16 + k;
          if (i >= n_ind) break;  // padding individuals: 0
          const int32_t col = first_col >= 0 ? first_col + i : col_of_ind[i];
          if (col < 0 || col >= sample_ct) {
            st = kPgenBadIndex;
            continue;
          }
          const uint8_t field = table[codes[col]];
          if (field == kPgenPack2Het) st = std::max(st, n_ind - i);
          else if (field == kPgenPack2Unfit) uf = std::max(uf, n_ind - i);
          else word |= static_cast<uint32_t>(field) << (2 * k);
        }
        block.put(out_row0 + r, j, word);
      }
      status[r] = st;
      unfit[r] = uf;
    }
  };
  const int64_t cells = n_out_rows * (static_cast<int64_t>(n_ind) + sample_ct);
  packed2_for_rows(n_threads, n_out_rows, cells, decode);
  if (failed) return sai_set_error(SAI_ERR_HIP, "out of host memory");
  block.pad(out_row0 + n_out_rows, n_sites);
  return SAI_OK;
}

}  // namespace

extern "C" {

int sai_pgen_packed_abi_version(void) { return SAI_PGEN_PACKED_ABI_VERSION; }

int sai_pgen_pack2_host(const uint8_t* bytes, int64_t n_bytes, int64_t n_out_rows, const int64_t* rec, const int64_t* base,
                        const uint8_t* row_flip, int32_t sample_ct, int32_t n_ind, const int32_t* col_of_ind,
                        int32_t first_col, int32_t ploidy, uint8_t* packed, int64_t n_sites, int64_t out_row0,
                        int32_t* status, int32_t* unfit, int32_t n_threads) {
  try {
    return pgen_pack2_host_impl(bytes, n_bytes, n_out_rows, rec, base, row_flip, sample_ct, n_ind, col_of_ind, first_col, ploidy,
                                packed, n_sites, out_row0, status, unfit, n_threads);
  } catch (const std::bad_alloc&) {
    return sai_set_error(SAI_ERR_HIP, "sai_pgen_pack2_host: out of host memory");
  } catch (const std::exception& e) {
    return sai_set_error(SAI_ERR_HIP, "sai_pgen_pack2_host: %s", e.what());
  }
}

}  // extern "C"
