// sai_site_join_many_host (sai_amd/csrc/join/site_join_many_host.cpp) on buffers of exactly the promised sizes, for a
// run under ASan + UBSan: 2 to 17 lists against repeated std::set_intersection, lists out of order, empty lists, and
// the refusals.  Every buffer comes from malloc with not a byte to spare, so a read or a write past a promise is a
// finding.  Prints "ok <checks>" and exits 0, or says what differed and exits 1.

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iterator>
#include <vector>

#include "saihip.h"

extern "C" {
int sai_join_many_abi_version(void);
int sai_site_join_many_host(int32_t n_lists, const int32_t* const* pos, const int64_t* n, int32_t* const* rows, int64_t* info);
}

namespace {

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint32_t next() {
  g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
  return static_cast<uint32_t>(g_state >> 33);
}

template <typename T>
T* exact(size_t n) {  // malloc(0) may be NULL: one byte then, which nobody is to touch
  T* p = static_cast<T*>(std::malloc(n ? n * sizeof(T) : 1));
  if (!p) std::abort();
  return p;
}

int fail(const char* what, long long a = 0, long long b = 0) {
  std::printf("FAILED: %s (%lld, %lld)\n", what, a, b);
  return 1;
}

std::vector<int32_t> ascending(size_t n, bool high) {
  std::vector<int32_t> v(n);
  int64_t at = high ? 0x7FFFFFFFll - static_cast<int64_t>(4 * n) - 1 : 0;
  for (size_t i = 0; i < n; ++i) v[i] = static_cast<int32_t>(at += 1 + next() % 4);
  return v;
}

int check_join(const std::vector<std::vector<int32_t>>& lists) {
  const int k = static_cast<int>(lists.size());
  size_t room = lists[0].size();
  for (const auto& l : lists) room = std::min(room, l.size());
  std::vector<int32_t*> pos(k), rows(k);
  int64_t* n = exact<int64_t>(k);
  for (int j = 0; j < k; ++j) {
    pos[j] = exact<int32_t>(lists[j].size());
    rows[j] = exact<int32_t>(room);
    if (!lists[j].empty()) std::memcpy(pos[j], lists[j].data(), lists[j].size() * 4);
    n[j] = static_cast<int64_t>(lists[j].size());
  }
  int32_t** pos_table = exact<int32_t*>(k);
  int32_t** rows_table = exact<int32_t*>(k);
  std::copy(pos.begin(), pos.end(), pos_table);
  std::copy(rows.begin(), rows.end(), rows_table);
  int64_t* info = exact<int64_t>(2 + 2 * k);
  int bad = 0;
  if (sai_site_join_many_host(k, pos_table, n, rows_table, info) != SAI_OK) bad = fail("status", k, room);
  std::vector<int32_t> common = lists[0];
  for (int j = 1; j < k; ++j) {
    std::vector<int32_t> both;
    std::set_intersection(common.begin(), common.end(), lists[j].begin(), lists[j].end(), std::back_inserter(both));
    common.swap(both);
  }
  bool empty = false;
  for (const auto& l : lists) empty |= l.empty();
  if (!bad && (info[0] != static_cast<int64_t>(common.size()) || info[1] != -1)) bad = fail("info", info[0], common.size());
  for (int j = 0; !bad && j < k; ++j) {
    if (info[2 + j] != -1) bad = fail("order word", j, info[2 + j]);
    const bool identity = empty ? lists[j].empty() : common.size() == lists[j].size();
    if (!bad && info[2 + k + j] != identity) bad = fail("identity word", j, info[2 + k + j]);
    for (size_t i = 0; !bad && i < common.size(); ++i)
      if (rows[j][i] < 0 || lists[j][rows[j][i]] != common[i]) bad = fail("rows", j, i);
  }
  for (int j = 0; j < k; ++j) std::free(pos[j]), std::free(rows[j]);
  std::free(n), std::free(pos_table), std::free(rows_table), std::free(info);
  return bad;
}

}  // namespace

int main() {
  long long checks = 0;
  if (sai_join_many_abi_version() != 1) return fail("version");
  const size_t B = 256;
  for (int k : {2, 3, 4, 5, 17})
    for (size_t n : {size_t(0), size_t(1), size_t(2), B - 1, B, B + 1, 2 * B + 3, 7 * B})
      for (int high = 0; high < 2; ++high) {
        std::vector<int32_t> pool = ascending(2 * n + 5, high != 0);
        std::vector<std::vector<int32_t>> lists(k);
        for (int32_t p : pool)
          for (int j = 0; j < k; ++j)
            if ((j == 0 ? lists[0].size() < n : true) && next() % 8 != 0) lists[j].push_back(p);
        if (check_join(lists)) return 1;
        std::vector<std::vector<int32_t>> same(k, lists[k - 1]);  // identical lists: every side the identity
        if (check_join(same)) return 1;
        for (int at = 0; at < k; at += k - 1) {  // an empty list at the first and at the last place
          std::vector<std::vector<int32_t>> with_empty = lists;
          with_empty[at].clear();
          if (check_join(with_empty)) return 1;
        }
        lists[k / 2] = pool;  // one list holds all
        if (check_join(lists)) return 1;
        checks += 5;
      }
  {  // out of order: the number of the first list and, per list, the first index that tells; nothing written
    std::vector<int32_t> a = ascending(3 * B + 5, false), b = a, c = a;
    b[2 * B] = b[2 * B - 1];
    b[B] = b[B - 1] - 1;
    c[5] = c[4];
    const int32_t* pos[3] = {a.data(), b.data(), c.data()};
    const int64_t n[3] = {static_cast<int64_t>(a.size()), static_cast<int64_t>(b.size()), static_cast<int64_t>(c.size())};
    int32_t one[3] = {77, 77, 77};
    int32_t* rows[3] = {&one[0], &one[1], &one[2]};
    int64_t info[8];
    if (sai_site_join_many_host(3, pos, n, rows, info) != SAI_OK || info[0] != 0 || info[1] != 1 || info[2] != -1 ||
        info[3] != static_cast<int64_t>(B) || info[4] != 5 || info[5] || info[6] || info[7] || one[0] != 77 || one[1] != 77 || one[2] != 77)
      return fail("lists out of order", info[1], info[3]);
    if (sai_site_join_many_host(3, pos, n, rows, nullptr) != SAI_ERR_ARG) return fail("NULL info");
    if (sai_site_join_many_host(1, pos, n, rows, info) != SAI_ERR_ARG) return fail("one list");
    if (sai_site_join_many_host(18, pos, n, rows, info) != SAI_ERR_ARG) return fail("eighteen lists");
    if (sai_site_join_many_host(3, nullptr, n, rows, info) != SAI_ERR_ARG) return fail("NULL positions");
    const int32_t* hole[3] = {a.data(), nullptr, c.data()};
    if (sai_site_join_many_host(3, hole, n, rows, info) != SAI_ERR_ARG) return fail("a NULL list");
    const int64_t negative[3] = {n[0], -1, n[2]};
    if (sai_site_join_many_host(3, pos, negative, rows, info) != SAI_ERR_ARG) return fail("negative size");
    checks += 7;
  }
  std::printf("ok %lld\n", checks);
  return 0;
}
