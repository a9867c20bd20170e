// DD for source populations of any size, the host half: the entry points' statement, their plain C++ twins and the
// argument checks both halves share.  The group is internal to the package: it is declared HERE and in dd_table.hip
// (no header under include/), bound by sai_amd/dd_table.py alone, and carries a version number of its own.
//
//   int sai_dd_table_abi_version(void);                          -- SAI_DD_TABLE_ABI_VERSION
//
//   table[k * n_sites + site] = sum over pop's individuals g of |values[k] - g[site]|, raw int8 values, ANY int8 g (missing
//   calls enter as their negative numbers, as sai_site_absdiff takes them).  pop->tiles: the int8 tiled layout of saihip.h,
//   16-byte aligned, n_ind = 0..2^24; n_values = 1..SAI_DD_TABLE_VALUES, values distinct (host array); only sites < n_sites
//   are written; n_sites == 0 is SAI_OK and touches nothing.
//   int sai_site_absdiff_table(sai_ctx*, int64_t n_sites, const sai_pop* pop, int32_t n_values, const int8_t* values,
//                              uint32_t* table, void* stream);
//
//   Per window w (lo/hi clamped into the block exactly as sai_window_dd clamps them) and source individual s:
//     tr = sum_{i in [lo,hi)} table_ref[k(s,i)][i],  tt likewise,  k(s,i) = index in values of src's byte (s, i);
//     d[s] = double(tr) / double(n_ref_ind) - double(tt) / double(n_tgt_ind);   dd[w] = numpy_sum(d) / double(n_src_ind)
//   -- sai_window_dd's arithmetic operation for operation.  A source byte that is not in values adds nothing and is counted
//   in *n_unlisted (device int32, zeroed by the call, saturating at 2^31 - 1); the caller must then discard dd.
//   scratch: f64 [n_windows][n_src_ind].  src->tiles: any alignment, n_ind >= 1.  n_windows == 0 only zeroes the counter.
//   int sai_window_dd_table(sai_ctx*, int64_t n_sites, const sai_pop* src, int32_t n_values, const int8_t* values,
//                           const uint32_t* table_ref, int32_t n_ref_ind, const uint32_t* table_tgt, int32_t n_tgt_ind,
//                           int32_t n_windows, const int32_t* lo, const int32_t* hi, double* scratch, double* dd,
//                           int32_t* n_unlisted, void* stream);
//
//   sai_site_absdiff_table_host / sai_window_dd_table_host (below): the same without ctx and stream, host pointers of any
//   alignment, field by field from the layout formula of saihip.h (byte(tile, individual, site-in-tile) =
//   tiles[(tile * n_ind + individual) * 64 + site-in-tile]), the same outputs bit for bit: the table's entries and the window
//   totals are exact integers, the doubles are formed by the same operations in the same order.

#include <cstdint>
#include <cstring>
#include <exception>
#include <new>

#include "saihip.h"

#define SAI_DD_TABLE_ABI_VERSION 1
#define SAI_DD_TABLE_VALUES 8  // values of one table at most; dd_table.hip says the same (tests/test_dd_table_cpu.py)

extern "C" int sai_set_error(int code, const char* fmt, ...);

// ---- the argument checks of both halves (declared again in dd_table.hip), in the words of sai_site_absdiff and
// sai_window_dd (../dd.hip) where the check is the same ----

int sai_dd_table_check_values(int32_t n_values, const int8_t* values) {
  if (n_values < 1 || n_values > SAI_DD_TABLE_VALUES) return sai_set_error(SAI_ERR_ARG, "n_values must be 1..%d", SAI_DD_TABLE_VALUES);
  if (!values) return sai_set_error(SAI_ERR_ARG, "values is NULL");
  for (int a = 0; a < n_values; ++a)
    for (int b = 0; b < a; ++b)
      if (values[a] == values[b]) return sai_set_error(SAI_ERR_ARG, "values must be distinct");
  return SAI_OK;
}

// sai_site_absdiff_table: what is checked before n_sites == 0 returns SAI_OK ...
int sai_dd_table_check_sizes(int64_t n_sites, const sai_pop* pop, int32_t n_values, const int8_t* values) {
  if (n_sites < 0 || n_sites >= 0x7FFFFFFFll) return sai_set_error(SAI_ERR_ARG, "n_sites out of range");
  if (!pop) return sai_set_error(SAI_ERR_ARG, "NULL population");
  if (pop->n_ind < 0 || pop->n_ind > (1 << 24)) return sai_set_error(SAI_ERR_ARG, "bad n_ind");
  return sai_dd_table_check_values(n_values, values);
}

// ... and behind it.  `device`: the tiles are read with 16-byte loads and must be aligned for them.
int sai_dd_table_check_buffers(const sai_pop* pop, const uint32_t* table, bool device) {
  if (!table || (pop->n_ind > 0 && !pop->tiles)) return sai_set_error(SAI_ERR_ARG, "NULL buffer");
  if (device && (reinterpret_cast<uintptr_t>(pop->tiles) & 15u)) return sai_set_error(SAI_ERR_ARG, "tiles must be 16-byte aligned");
  return SAI_OK;
}

// sai_window_dd_table: everything; the counter is looked at before n_windows == 0 returns (it is zeroed even then)
int sai_dd_window_check(int64_t n_sites, const sai_pop* src, int32_t n_values, const int8_t* values, const uint32_t* table_ref,
                        int32_t n_ref_ind, const uint32_t* table_tgt, int32_t n_tgt_ind, int32_t n_windows, const int32_t* lo,
                        const int32_t* hi, const double* scratch, const double* dd, const int32_t* n_unlisted) {
  if (n_sites < 0 || n_sites >= 0x7FFFFFFFll || n_windows < 0) return sai_set_error(SAI_ERR_ARG, "size out of range");
  if (!src) return sai_set_error(SAI_ERR_ARG, "NULL population");
  if (src->n_ind < 1 || n_ref_ind < 1 || n_tgt_ind < 1) return sai_set_error(SAI_ERR_ARG, "every population needs an individual");
  if (src->n_ind > (1 << 24)) return sai_set_error(SAI_ERR_ARG, "bad n_ind");
  if (int rc = sai_dd_table_check_values(n_values, values)) return rc;
  if (!n_unlisted) return sai_set_error(SAI_ERR_ARG, "NULL buffer");
  if (n_windows == 0) return SAI_OK;
  if ((n_sites > 0 && (!table_ref || !table_tgt || !src->tiles)) || !lo || !hi || !scratch || !dd) return sai_set_error(SAI_ERR_ARG, "NULL buffer");
  return SAI_OK;
}

namespace {

// numpy's pairwise sum (../numpy_sum.hpp, restated for the host): a plain loop below 8 elements, else eight running
// sums and the tail; nodes of more than 128 elements are halved (the left half rounded down to a multiple of 8)
double pairwise(const double* a, int64_t n) {
  if (n < 8) {
    double res = 0.0;
    for (int64_t i = 0; i < n; ++i) res += a[i];
    return res;
  }
  if (n <= 128) {
    double r[8];
    for (int j = 0; j < 8; ++j) r[j] = a[j];
    int64_t i = 8;
    for (; i < n - (n % 8); i += 8)
      for (int j = 0; j < 8; ++j) r[j] += a[i + j];
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += a[i];
    return res;
  }
  int64_t n2 = n / 2;
  n2 -= n2 % 8;
  return pairwise(a, n2) + pairwise(a + n2, n - n2);
}

// np.sum: 8192-element pieces (the ufunc buffer), added in order
double numpy_sum_host(const double* a, int64_t n) {
  double res = 0.0;
  for (int64_t o = 0; o < n; o += 8192) res += pairwise(a + o, n - o < 8192 ? n - o : 8192);
  return res;
}

int site_absdiff_table_host_impl(int64_t n_sites, const sai_pop* pop, int32_t n_values, const int8_t* values, uint32_t* table) {
  if (int rc = sai_dd_table_check_sizes(n_sites, pop, n_values, values)) return rc;
  if (n_sites == 0) return SAI_OK;
  if (int rc = sai_dd_table_check_buffers(pop, table, false)) return rc;
  const int64_t n_ind = pop->n_ind;
  for (int k = 0; k < n_values; ++k) {
    const int v = values[k];
    for (int64_t site = 0; site < n_sites; ++site) {
      const int64_t tile = site / 64, s = site % 64;
      uint32_t sum = 0;
      for (int64_t i = 0; i < n_ind; ++i) {
        const int g = pop->tiles[(tile * n_ind + i) * 64 + s];
        sum += static_cast<uint32_t>(v > g ? v - g : g - v);
      }
      table[static_cast<int64_t>(k) * n_sites + site] = sum;
    }
  }
  return SAI_OK;
}

int window_dd_table_host_impl(int64_t n_sites, const sai_pop* src, int32_t n_values, const int8_t* values, const uint32_t* table_ref,
                              int32_t n_ref_ind, const uint32_t* table_tgt, int32_t n_tgt_ind, int32_t n_windows, const int32_t* lo,
                              const int32_t* hi, double* scratch, double* dd, int32_t* n_unlisted) {
  if (int rc = sai_dd_window_check(n_sites, src, n_values, values, table_ref, n_ref_ind, table_tgt, n_tgt_ind, n_windows, lo, hi, scratch, dd,
                               n_unlisted))
    return rc;
  *n_unlisted = 0;
  int index_of[256];
  for (int b = 0; b < 256; ++b) index_of[b] = -1;
  for (int k = 0; k < n_values; ++k) index_of[static_cast<uint8_t>(values[k])] = k;
  const int64_t n_src = src->n_ind;
  int64_t unlisted = 0;
  for (int32_t w = 0; w < n_windows; ++w) {
    const int64_t a = lo[w] < 0 ? 0 : (lo[w] > n_sites ? n_sites : lo[w]);
    const int64_t b = hi[w] < 0 ? 0 : (hi[w] > n_sites ? n_sites : hi[w]);
    double* d = scratch + static_cast<int64_t>(w) * n_src;
    for (int64_t s = 0; s < n_src; ++s) {
      long long tr = 0, tt = 0;
      for (int64_t i = a; i < b; ++i) {
        const int k = index_of[static_cast<uint8_t>(src->tiles[(i / 64 * n_src + s) * 64 + i % 64])];
        if (k < 0) {
          ++unlisted;
          continue;
        }
        tr += table_ref[static_cast<int64_t>(k) * n_sites + i];
        tt += table_tgt[static_cast<int64_t>(k) * n_sites + i];
      }
      d[s] = static_cast<double>(tr) / static_cast<double>(n_ref_ind) - static_cast<double>(tt) / static_cast<double>(n_tgt_ind);
    }
    dd[w] = numpy_sum_host(d, n_src) / static_cast<double>(n_src);
  }
  *n_unlisted = unlisted > 0x7FFFFFFFll ? 0x7FFFFFFF : static_cast<int32_t>(unlisted);
  return SAI_OK;
}

}  // namespace

extern "C" {

int sai_dd_table_abi_version(void) { return SAI_DD_TABLE_ABI_VERSION; }

int sai_site_absdiff_table_host(int64_t n_sites, const sai_pop* pop, int32_t n_values, const int8_t* values, uint32_t* table) {
  try {
    return site_absdiff_table_host_impl(n_sites, pop, n_values, values, table);
  } catch (const std::bad_alloc&) {
    return sai_set_error(SAI_ERR_HIP, "sai_site_absdiff_table_host: out of host memory");
  } catch (const std::exception& e) {
    return sai_set_error(SAI_ERR_HIP, "sai_site_absdiff_table_host: %s", e.what());
  }
}

int sai_window_dd_table_host(int64_t n_sites, const sai_pop* src, int32_t n_values, const int8_t* values, const uint32_t* table_ref,
                             int32_t n_ref_ind, const uint32_t* table_tgt, int32_t n_tgt_ind, int32_t n_windows, const int32_t* lo,
                             const int32_t* hi, double* scratch, double* dd, int32_t* n_unlisted) {
  try {
    return window_dd_table_host_impl(n_sites, src, n_values, values, table_ref, n_ref_ind, table_tgt, n_tgt_ind, n_windows, lo, hi, scratch,
                                     dd, n_unlisted);
  } catch (const std::bad_alloc&) {
    return sai_set_error(SAI_ERR_HIP, "sai_window_dd_table_host: out of host memory");
  } catch (const std::exception& e) {
    return sai_set_error(SAI_ERR_HIP, "sai_window_dd_table_host: %s", e.what());
  }
}

}  // extern "C"
