// sai_pgen_encode_host: the plain statement of pgen_export.hpp -- the int8 [row][slot] block of the readers -> the
// hard-call records of a PLINK 2 .pgen, cell by cell from pgen_code_of, every candidate type sized in full (no
// candidate is skipped here) and the smallest written; the steps are in pgen_encode_host.hpp.  The yardstick of the
// kernels (pgen_encode.hip), which write the same bytes, types, lengths and status values, and the encoder of the
// SAI_AMD_INGEST=host route.

#include <atomic>
#include <exception>
#include <new>
#include <vector>

#include "pgen_encode_host.hpp"

extern "C" int sai_set_error(int code, const char* fmt, ...);

namespace {

int pgen_encode_host_impl(const int8_t* dosage, int64_t n_rows, int32_t n_slots, const int32_t* ploidy_of_slot, int32_t uniform_ploidy,
                          uint8_t* out, int64_t out_cap, uint8_t* vrtype, uint32_t* length, int32_t* status, int64_t* total, int32_t n_threads) {
  if (n_rows < 0 || n_slots < 1 || out_cap < 0) return sai_set_error(SAI_ERR_ARG, "size out of range");
  if (uniform_ploidy < 0 || uniform_ploidy > 2) return sai_set_error(SAI_ERR_ARG, "uniform_ploidy must be 0, 1 or 2");
  if (n_rows > (INT64_MAX - 16) / n_slots) return sai_set_error(SAI_ERR_ARG, "size out of range");
  if (!total) return sai_set_error(SAI_ERR_ARG, "NULL buffer");
  if (n_rows == 0) {
    *total = 0;
    return SAI_OK;
  }
  if (!dosage || !vrtype || !length || !status || (out_cap > 0 && !out) || (uniform_ploidy == 0 && !ploidy_of_slot))
    return sai_set_error(SAI_ERR_ARG, "NULL buffer");
  const Call c{dosage, n_rows, n_slots, ploidy_of_slot, uniform_ploidy};
  const uint32_t n = static_cast<uint32_t>(n_slots);
  over_rows(c, n_threads, [&](int64_t lo_row, int64_t hi_row) {
    std::vector<uint8_t> codes(n);
    for (int64_t r = lo_row; r < hi_row; ++r) {
      status[r] = codes_of_row(c, r, codes.data());
      uint32_t kind, lo, hi;
      uint64_t len;
      plan_row(codes.data(), n, &kind, &len, &lo, &hi);
      vrtype[r] = static_cast<uint8_t>(kind);
      length[r] = static_cast<uint32_t>(len);  // at most ceil(n / 4)
    }
  });
  std::vector<int64_t> offset(static_cast<size_t>(n_rows) + 1);
  offset[0] = 0;
  for (int64_t r = 0; r < n_rows; ++r) offset[r + 1] = offset[r] + length[r];
  *total = offset[n_rows];
  if (*total > out_cap) return sai_set_error(SAI_ERR_ARG, "out_cap: the records take %lld bytes and out holds %lld", static_cast<long long>(*total), static_cast<long long>(out_cap));
  std::atomic<bool> sound{true};
  over_rows(c, n_threads, [&](int64_t lo_row, int64_t hi_row) {
    std::vector<uint8_t> codes(n);
    for (int64_t r = lo_row; r < hi_row; ++r) {
      codes_of_row(c, r, codes.data());
      uint32_t kind, lo, hi;
      uint64_t len;
      plan_row(codes.data(), n, &kind, &len, &lo, &hi);
      const uint8_t* end = put_row(out + offset[r], codes.data(), n, kind, lo, hi);
      if (end != out + offset[r + 1]) sound = false;  // the size rule and the writer disagree: never
    }
  });
  if (!sound) return sai_set_error(SAI_ERR_HIP, "sai_pgen_encode_host: a record was not of the size planned for it");
  return SAI_OK;
}

}  // namespace

extern "C" {

int sai_pgen_export_abi_version(void) { return SAI_PGEN_EXPORT_ABI_VERSION; }

int sai_pgen_pvar_lines(const char* bim, int64_t n_bytes, char* out, int64_t* n_out) {
  if (n_bytes < 0 || !n_out || (n_bytes > 0 && (!bim || !out))) return sai_set_error(SAI_ERR_ARG, "NULL buffer or size out of range");
  char* at = out;
  for (int64_t line = 0, k = 0; k < n_bytes; ++line) {
    int64_t tab[5], n_tabs = 0, e = k;
    for (; e < n_bytes && bim[e] != '\n'; ++e)
      if (bim[e] == '\t') {
        if (n_tabs < 5) tab[n_tabs] = e;
        ++n_tabs;
      }
    if (e == n_bytes || n_tabs != 5) return sai_set_error(SAI_ERR_ARG, ".bim line %lld: not six tab-separated columns ended by a newline", static_cast<long long>(line + 1));
    auto copy = [&](int64_t from, int64_t to, char then) {  // [from, to) and one separator
      at = std::copy(bim + from, bim + to, at);
      *at++ = then;
    };
    copy(k, tab[0], '\t');           // CHROM
    copy(tab[2] + 1, tab[3], '\t');  // POS
    copy(tab[0] + 1, tab[1], '\t');  // ID
    copy(tab[4] + 1, e, '\t');       // REF, the last column of a .bim
    copy(tab[3] + 1, tab[4], '\n');  // ALT
    k = e + 1;
  }
  *n_out = at - out;
  return SAI_OK;
}

int sai_pgen_encode_host(const int8_t* dosage, int64_t n_rows, int32_t n_slots, const int32_t* ploidy_of_slot, int32_t uniform_ploidy,
                         uint8_t* out, int64_t out_cap, uint8_t* vrtype, uint32_t* length, int32_t* status, int64_t* total, int32_t n_threads) {
  try {
    return pgen_encode_host_impl(dosage, n_rows, n_slots, ploidy_of_slot, uniform_ploidy, out, out_cap, vrtype, length, status, total, n_threads);
  } catch (const std::bad_alloc&) {
    return sai_set_error(SAI_ERR_HIP, "sai_pgen_encode_host: out of host memory");
  } catch (const std::exception& e) {
    return sai_set_error(SAI_ERR_HIP, "sai_pgen_encode_host: %s", e.what());
  }
}

}  // extern "C"
