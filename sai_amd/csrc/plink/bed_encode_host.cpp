// sai_bed_encode_host: the plain statement of bed_export.hpp -- the int8 [row][slot] block of the readers -> variant-major
// PLINK 1 .bed rows, cell by cell from bed_code_of.  The yardstick of the kernel (bed_encode.hip), which writes the
// same bytes and the same status values, and the encoder of the SAI_AMD_INGEST=host route.

#include <algorithm>
#include <exception>
#include <new>

#include "../host_threads.hpp"
#include "bed_export.hpp"
#include "plink_codes.hpp"

extern "C" int sai_set_error(int code, const char* fmt, ...);

namespace {

int bed_encode_host_impl(const int8_t* dosage, int64_t n_rows, int32_t n_slots, const int32_t* ploidy_of_slot, int32_t uniform_ploidy,
                         uint8_t* out, int32_t* status, int32_t n_threads) {
  if (n_rows < 0 || n_slots < 1) return sai_set_error(SAI_ERR_ARG, "size out of range");
  if (uniform_ploidy < 0 || uniform_ploidy > 2) return sai_set_error(SAI_ERR_ARG, "uniform_ploidy must be 0, 1 or 2");
  if (n_rows > (INT64_MAX - 16) / n_slots) return sai_set_error(SAI_ERR_ARG, "size out of range");
  if (n_rows == 0) return SAI_OK;
  if (!dosage || !out || !status || (uniform_ploidy == 0 && !ploidy_of_slot)) return sai_set_error(SAI_ERR_ARG, "NULL buffer");
  const int64_t row_bytes = (static_cast<int64_t>(n_slots) + 3) / 4;
  auto encode = [&](int64_t lo, int64_t hi) {
    for (int64_t r = lo; r < hi; ++r) {
      const int8_t* src = dosage + r * n_slots;
      uint8_t* dst = out + r * row_bytes;
      int32_t st = 0;
      for (int64_t b = 0; b < row_bytes; ++b) {
        uint32_t byte = 0;
        for (int k = 0; k < 4; ++k) {
          const int64_t s = 4 * b + k;
          if (s >= n_slots) break;  // padding bits: 0
          const int32_t pl = uniform_ploidy ? uniform_ploidy : ploidy_of_slot[s];
          bool fits = false;
          uint32_t code = 1u;
          if (pl == 1 || pl == 2) code = bed_code_of(src[s], pl, &fits);
          else st = kPlinkBadIndex;
          if (!fits) st = std::max(st, static_cast<int32_t>(n_slots - s));
          byte |= code << (2 * k);
        }
        dst[b] = static_cast<uint8_t>(byte);
      }
      status[r] = st;
    }
  };
  // one thread for every 2^18 cells of work, as the host decoders
  const int64_t cells = n_rows * n_slots;
  const int nt = static_cast<int>(std::max<int64_t>(1, std::min<int64_t>({static_cast<int64_t>(std::max(n_threads, 1)), n_rows, cells / (int64_t(1) << 18) + 1})));
  ThreadGroup tg;
  for (int t = 1; t < nt; ++t) tg.spawn([&encode, t, nt, n_rows] { encode(n_rows * t / nt, n_rows * (t + 1) / nt); });
  encode(0, n_rows / nt);
  tg.join();
  return SAI_OK;
}

}  // namespace

extern "C" {

int sai_bed_export_abi_version(void) { return SAI_BED_EXPORT_ABI_VERSION; }

int sai_bed_encode_host(const int8_t* dosage, int64_t n_rows, int32_t n_slots, const int32_t* ploidy_of_slot, int32_t uniform_ploidy,
                        uint8_t* out, int32_t* status, int32_t n_threads) {
  try {
    return bed_encode_host_impl(dosage, n_rows, n_slots, ploidy_of_slot, uniform_ploidy, out, status, n_threads);
  } catch (const std::bad_alloc&) {
    return sai_set_error(SAI_ERR_HIP, "sai_bed_encode_host: out of host memory");
  } catch (const std::exception& e) {
    return sai_set_error(SAI_ERR_HIP, "sai_bed_encode_host: %s", e.what());
  }
}

}  // extern "C"
