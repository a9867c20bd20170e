// sai_pgen_encode_ld_host: the plain statement of pgen_export_ld.hpp -- sai_pgen_encode_host with the record types 2
// and 3.  A segment of 16 rows is walked in order with the codes of its current base row beside the row's; every
// candidate type is sized in full (no candidate is skipped here) and the smallest written, a tie going to the lower
// type.  The yardstick of the kernels (pgen_encode_ld.hip), which write the same bytes, types, lengths and status
// values, and the encoder of `sai convert --out-pfile --ld-compress` on the SAI_AMD_INGEST=host route.

#include <atomic>
#include <exception>
#include <new>
#include <vector>

#include "pgen_encode_host.hpp"
#include "pgen_export_ld.hpp"

extern "C" int sai_set_error(int code, const char* fmt, ...);

namespace {

constexpr int64_t kSegment = SAI_PGEN_LD_SEGMENT;

// One segment, row by row: visit(row, status, codes, start, kind, length, lo, hi) with `start` the row a type 2 / 3
// record lists against (the base, for type 3 with 0 and 2 exchanged), NULL for every other type.
template <class F>
void walk_segment(const Call& c, int64_t first, F&& visit) {
  const uint32_t n = static_cast<uint32_t>(c.n_slots);
  const int64_t end = std::min(first + kSegment, c.n_rows);
  std::vector<uint8_t> codes(n), base(n), swapped(n);
  for (int64_t r = first; r < end; ++r) {
    const int32_t st = codes_of_row(c, r, codes.data());
    uint32_t kind, lo, hi;
    uint64_t len;
    plan_row(codes.data(), n, &kind, &len, &lo, &hi);  // the smallest of 0, 1, 4, 6 and 7
    const uint8_t* start = nullptr;
    if (r != first) {  // no anchor: types 2 and 3 against the base, which win a tie against a higher type only
      for (uint32_t s = 0; s < n; ++s) swapped[s] = static_cast<uint8_t>(pgen_swap02(base[s]));
      const uint64_t size2 = difflist_size(codes.data(), base.data(), n, 2, 0, 0);
      const uint64_t size3 = difflist_size(codes.data(), swapped.data(), n, 3, 0, 0);
      if (size2 < len || (size2 == len && kind > 2)) {
        kind = 2;
        len = size2;
        start = base.data();
      }
      if (size3 < len || (size3 == len && kind > 3)) {
        kind = 3;
        len = size3;
        start = swapped.data();
      }
    }
    visit(r, st, codes.data(), start, kind, len, lo, hi);
    if (kind != 2 && kind != 3) base.swap(codes);  // the base of the rows behind it
  }
}

int pgen_encode_ld_host_impl(const int8_t* dosage, int64_t n_rows, int32_t n_slots, const int32_t* ploidy_of_slot, int32_t uniform_ploidy,
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
  const int64_t n_segments = (n_rows + kSegment - 1) / kSegment;
  over_items(n_segments, n_rows * n_slots, n_threads, [&](int64_t lo_seg, int64_t hi_seg) {
    for (int64_t seg = lo_seg; seg < hi_seg; ++seg)
      walk_segment(c, seg * kSegment, [&](int64_t r, int32_t st, const uint8_t*, const uint8_t*, uint32_t kind, uint64_t len, uint32_t, uint32_t) {
        status[r] = st;
        vrtype[r] = static_cast<uint8_t>(kind);
        length[r] = static_cast<uint32_t>(len);  // at most ceil(n / 4)
      });
  });
  std::vector<int64_t> offset(static_cast<size_t>(n_rows) + 1);
  offset[0] = 0;
  for (int64_t r = 0; r < n_rows; ++r) offset[r + 1] = offset[r] + length[r];
  *total = offset[n_rows];
  if (*total > out_cap) return sai_set_error(SAI_ERR_ARG, "out_cap: the records take %lld bytes and out holds %lld", static_cast<long long>(*total), static_cast<long long>(out_cap));
  std::atomic<bool> sound{true};
  over_items(n_segments, n_rows * n_slots, n_threads, [&](int64_t lo_seg, int64_t hi_seg) {
    for (int64_t seg = lo_seg; seg < hi_seg; ++seg)
      walk_segment(c, seg * kSegment, [&](int64_t r, int32_t, const uint8_t* codes, const uint8_t* start, uint32_t kind, uint64_t, uint32_t lo, uint32_t hi) {
        uint8_t* at = out + offset[r];
        const uint8_t* end = start ? put_difflist(at, codes, start, n, kind, 0, 0) : put_row(at, codes, n, kind, lo, hi);
        if (end != out + offset[r + 1]) sound = false;  // the size rule and the writer disagree: never
      });
  });
  if (!sound) return sai_set_error(SAI_ERR_HIP, "sai_pgen_encode_ld_host: a record was not of the size planned for it");
  return SAI_OK;
}

}  // namespace

extern "C" {

int sai_pgen_export_ld_version(void) { return SAI_PGEN_EXPORT_LD_VERSION; }

int sai_pgen_ld_segment(void) { return SAI_PGEN_LD_SEGMENT; }

int sai_pgen_encode_ld_host(const int8_t* dosage, int64_t n_rows, int32_t n_slots, const int32_t* ploidy_of_slot, int32_t uniform_ploidy,
                            uint8_t* out, int64_t out_cap, uint8_t* vrtype, uint32_t* length, int32_t* status, int64_t* total, int32_t n_threads) {
  try {
    return pgen_encode_ld_host_impl(dosage, n_rows, n_slots, ploidy_of_slot, uniform_ploidy, out, out_cap, vrtype, length, status, total, n_threads);
  } catch (const std::bad_alloc&) {
    return sai_set_error(SAI_ERR_HIP, "sai_pgen_encode_ld_host: out of host memory");
  } catch (const std::exception& e) {
    return sai_set_error(SAI_ERR_HIP, "sai_pgen_encode_ld_host: %s", e.what());
  }
}

}  // extern "C"
