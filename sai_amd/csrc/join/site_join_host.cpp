// sai_site_join_host (include/saihip_join.h): a two-pointer merge of two strictly ascending position lists, after one
// look at each list for a position that is not above its predecessor.

#include "saihip_join.h"

extern "C" int sai_set_error(int code, const char* fmt, ...);

namespace {
constexpr int64_t kJoinMaxRows = 0x7FFFFFFFll - 1;  // row indices are int32
}

extern "C" {

int sai_join_abi_version(void) { return SAI_JOIN_ABI_VERSION; }

int sai_site_join_host(const int32_t* pos_a, int64_t n_a, const int32_t* pos_b, int64_t n_b, int32_t* rows_a, int32_t* rows_b,
                       int64_t* info) {
  if (n_a < 0 || n_b < 0 || n_a > kJoinMaxRows || n_b > kJoinMaxRows) return sai_set_error(SAI_ERR_ARG, "n_a and n_b must be 0..2^31 - 2");
  if (!info) return sai_set_error(SAI_ERR_ARG, "info is NULL");
  info[0] = 0, info[1] = info[2] = -1, info[3] = n_a == 0;
  if (n_a == 0 || n_b == 0) return SAI_OK;
  if (!pos_a || !pos_b || !rows_a || !rows_b) return sai_set_error(SAI_ERR_ARG, "NULL buffer");
  for (int64_t i = n_a - 1; i >= 1; --i)
    if (pos_a[i] <= pos_a[i - 1]) info[1] = i;
  for (int64_t j = n_b - 1; j >= 1; --j)
    if (pos_b[j] <= pos_b[j - 1]) info[2] = j;
  if (info[1] != -1 || info[2] != -1) return SAI_OK;
  int64_t i = 0, j = 0, k = 0;
  while (i < n_a && j < n_b) {
    if (pos_a[i] < pos_b[j]) {
      ++i;
    } else if (pos_b[j] < pos_a[i]) {
      ++j;
    } else {
      rows_a[k] = static_cast<int32_t>(i++);
      rows_b[k++] = static_cast<int32_t>(j++);
    }
  }
  info[0] = k;
  info[3] = k == n_a;
  return SAI_OK;
}

}  // extern "C"
