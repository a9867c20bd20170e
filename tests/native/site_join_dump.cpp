// sai_site_join_host of include/saihip_join.h on buffers of exactly the promised sizes, for a run under ASan + UBSan:
// against std::set_intersection, with lists out of order, and the refusals.
// Every buffer comes from malloc with not a byte to spare, so a read or a write past a promise is a finding.
// Prints "ok <checks>" and exits 0, or says what differed and exits 1.

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "saihip_join.h"

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

int check_join(const std::vector<int32_t>& a, const std::vector<int32_t>& b) {
  const size_t room = std::min(a.size(), b.size());
  int32_t* pa = exact<int32_t>(a.size());
  int32_t* pb = exact<int32_t>(b.size());
  int32_t* rows_a = exact<int32_t>(room);
  int32_t* rows_b = exact<int32_t>(room);
  int64_t* info = exact<int64_t>(SAI_JOIN_INFO_WORDS);
  if (!a.empty()) std::memcpy(pa, a.data(), a.size() * 4);
  if (!b.empty()) std::memcpy(pb, b.data(), b.size() * 4);
  int bad = 0;
  if (sai_site_join_host(pa, a.size(), pb, b.size(), rows_a, rows_b, info) != SAI_OK) bad = fail("status", a.size(), b.size());
  std::vector<int32_t> common;
  std::set_intersection(a.begin(), a.end(), b.begin(), b.end(), std::back_inserter(common));
  if (!bad && (info[0] != static_cast<int64_t>(common.size()) || info[1] != -1 || info[2] != -1 || info[3] != (common.size() == a.size())))
    bad = fail("info", info[0], common.size());
  for (size_t k = 0; !bad && k < common.size(); ++k)
    if (rows_a[k] < 0 || rows_b[k] < 0 || a[rows_a[k]] != common[k] || b[rows_b[k]] != common[k]) bad = fail("rows", k, common[k]);
  std::free(pa), std::free(pb), std::free(rows_a), std::free(rows_b), std::free(info);
  return bad;
}

}  // namespace

int main() {
  long long checks = 0;
  if (sai_join_abi_version() != SAI_JOIN_ABI_VERSION) return fail("version");
  const size_t B = 256;
  for (size_t n : {size_t(0), size_t(1), size_t(2), B - 1, B, B + 1, 2 * B + 3, 7 * B})
    for (int high = 0; high < 2; ++high) {
      std::vector<int32_t> pool = ascending(2 * n + 5, high != 0), a, b;
      for (int32_t p : pool) {
        if (a.size() < n && next() % 3) a.push_back(p);
        if (next() % 2) b.push_back(p);
      }
      if (check_join(a, b) || check_join(b, a) || check_join(a, a) || check_join(a, pool) || check_join(pool, a) || check_join(a, {})) return 1;
      checks += 6;
    }
  {  // out of order: the first index that tells, on either side, and nothing written
    std::vector<int32_t> a = ascending(3 * B + 5, false), b = a;
    b[2 * B] = b[2 * B - 1];
    b[B] = b[B - 1] - 1;
    int32_t one = 0;
    int64_t info[SAI_JOIN_INFO_WORDS];
    if (sai_site_join_host(a.data(), a.size(), b.data(), b.size(), &one, &one, info) != SAI_OK || info[0] != 0 || info[1] != -1 ||
        info[2] != static_cast<int64_t>(B) || info[3] != 0)
      return fail("b out of order", info[2]);
    if (sai_site_join_host(b.data(), b.size(), a.data(), a.size(), &one, &one, info) != SAI_OK || info[1] != static_cast<int64_t>(B) || info[2] != -1)
      return fail("a out of order", info[1]);
    if (sai_site_join_host(a.data(), a.size(), b.data(), b.size(), &one, &one, nullptr) != SAI_ERR_ARG) return fail("NULL info");
    if (sai_site_join_host(nullptr, 3, b.data(), b.size(), &one, &one, info) != SAI_ERR_ARG) return fail("NULL positions");
    if (sai_site_join_host(a.data(), -1, b.data(), b.size(), &one, &one, info) != SAI_ERR_ARG) return fail("negative size");
    checks += 5;
  }
  std::printf("ok %lld\n", checks);
  return 0;
}
