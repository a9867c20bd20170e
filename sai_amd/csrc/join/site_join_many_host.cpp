// sai_site_join_many_host: the rows of the positions that 2 to 17 strictly ascending int32 lists have in common -- a
// panel and up to sixteen source files of their own (DESIGN_INGEST.md, "Several source files").  One pass, a k-pointer
// merge: the largest head among the lists is the candidate, every other list is advanced to it, and a position is
// common when no list had to pass it.  Internal to the package: sai_amd/site_join.py, its only caller, binds it, and
// this unit declares it itself, as tile_rows.hip declares its entry points.
//
//   info[0]                       n_common
//   info[1]                       the number of the first list that is out of order, or -1
//   info[2 + j]                   the first index of list j whose position is not above its predecessor's, or -1
//   info[2 + n_lists + j]         1 when rows[j] is the identity (n_common == n[j]), else 0
// If a list is out of order, info[0] and the identity words are 0 and no row list is written.  An empty list is SAI_OK
// with n_common = 0: nothing is read and no list is checked.  For two lists the rows are sai_site_join_host's.

#include <cstdint>

#include "saihip.h"

extern "C" {
int sai_set_error(int code, const char* fmt, ...);
int sai_join_many_abi_version(void);
int sai_site_join_many_host(int32_t n_lists, const int32_t* const* pos, const int64_t* n, int32_t* const* rows, int64_t* info);
}

namespace {
constexpr int kJoinManyAbiVersion = 1;
constexpr int kMinLists = 2, kMaxLists = 17;        // a panel and 1 .. 16 source files
constexpr int64_t kJoinMaxRows = 0x7FFFFFFFll - 1;  // row indices are int32
}  // namespace

extern "C" {

int sai_join_many_abi_version(void) { return kJoinManyAbiVersion; }

int sai_site_join_many_host(int32_t n_lists, const int32_t* const* pos, const int64_t* n, int32_t* const* rows, int64_t* info) {
  if (n_lists < kMinLists || n_lists > kMaxLists) return sai_set_error(SAI_ERR_ARG, "n_lists must be 2..17");
  if (!info) return sai_set_error(SAI_ERR_ARG, "info is NULL");
  if (!n) return sai_set_error(SAI_ERR_ARG, "NULL buffer");
  bool empty = false;
  for (int j = 0; j < n_lists; ++j) {
    if (n[j] < 0 || n[j] > kJoinMaxRows) return sai_set_error(SAI_ERR_ARG, "the length of a list must be 0..2^31 - 2");
    empty |= n[j] == 0;
  }
  info[0] = 0, info[1] = -1;
  for (int j = 0; j < n_lists; ++j) info[2 + j] = -1, info[2 + n_lists + j] = n[j] == 0;
  if (empty) return SAI_OK;
  if (!pos || !rows) return sai_set_error(SAI_ERR_ARG, "NULL buffer");
  for (int j = 0; j < n_lists; ++j)
    if (!pos[j] || !rows[j]) return sai_set_error(SAI_ERR_ARG, "NULL buffer");
  for (int j = n_lists - 1; j >= 0; --j) {
    const int32_t* p = pos[j];
    for (int64_t i = n[j] - 1; i >= 1; --i)
      if (p[i] <= p[i - 1]) info[2 + j] = i;
    if (info[2 + j] != -1) info[1] = j;
  }
  if (info[1] != -1) {
    for (int j = 0; j < n_lists; ++j) info[2 + n_lists + j] = 0;
    return SAI_OK;
  }
  int64_t at[kMaxLists] = {};
  int64_t k = 0;
  int32_t want = pos[0][0];
  for (bool more = true; more;) {
    // every list up to the candidate; a list that passes it names the next candidate and the round starts again
    bool all = true;
    for (int j = 0; j < n_lists && more; ++j) {
      const int32_t* p = pos[j];
      int64_t i = at[j];
      while (i < n[j] && p[i] < want) ++i;
      at[j] = i;
      if (i == n[j]) {
        more = false;
      } else if (p[i] > want) {
        want = p[i];
        all = false;
      }
    }
    if (!more) break;
    if (!all) continue;
    for (int j = 0; j < n_lists; ++j) rows[j][k] = static_cast<int32_t>(at[j]++);
    ++k;
    if (at[0] == n[0]) break;
    want = pos[0][at[0]];
  }
  info[0] = k;
  for (int j = 0; j < n_lists; ++j) info[2 + n_lists + j] = k == n[j];
  return SAI_OK;
}

}  // extern "C"
