// sai_pgen_encode_host: the plain statement of pgen_export.hpp -- the int8 [row][slot] block of the readers -> the
// hard-call records of a PLINK 2 .pgen, cell by cell from pgen_code_of, every candidate type sized in full (no
// candidate is skipped here) and the smallest written.  The yardstick of the kernels (pgen_encode.hip), which write
// the same bytes, types, lengths and status values, and the encoder of the SAI_AMD_INGEST=host route.

#include <algorithm>
#include <atomic>
#include <exception>
#include <new>
#include <vector>

#include "../host_threads.hpp"
#include "pgen_codes.hpp"
#include "pgen_export.hpp"

extern "C" int sai_set_error(int code, const char* fmt, ...);

namespace {

struct Call {
  const int8_t* dosage;
  int64_t n_rows;
  int32_t n_slots;
  const int32_t* ploidy_of_slot;
  int32_t uniform_ploidy;
};

// the codes of one row and its status
int32_t codes_of_row(const Call& c, int64_t row, uint8_t* codes) {
  const int8_t* src = c.dosage + row * c.n_slots;
  int32_t st = 0;
  for (int32_t s = 0; s < c.n_slots; ++s) {
    const int32_t pl = c.uniform_ploidy ? c.uniform_ploidy : c.ploidy_of_slot[s];
    bool fits = false;
    uint32_t code = 3u;
    if (pl == 1 || pl == 2) code = pgen_code_of(src[s], pl, &fits);
    else st = kPgenBadIndex;
    if (!fits) st = std::max(st, c.n_slots - s);
    codes[s] = static_cast<uint8_t>(code);
  }
  return st;
}

// which samples a record of `kind` lists: those that differ from what the record's other part says of them
inline bool listed(uint32_t code, uint32_t kind, uint32_t lo, uint32_t hi) {
  if (kind == 1) return code != lo && code != hi;
  return code != (kind == 4 ? 0u : kind == 6 ? 2u : 3u);
}

void put_varint(uint8_t*& at, uint32_t v) {
  while (v >= 128u) {
    *at++ = static_cast<uint8_t>(128u | (v & 127u));
    v >>= 7;
  }
  *at++ = static_cast<uint8_t>(v);
}

// bytes of the difflist of a record of `kind`
uint64_t difflist_size(const uint8_t* codes, uint32_t n, uint32_t kind, uint32_t lo, uint32_t hi) {
  uint64_t L = 0, deltas = 0;
  uint32_t prev = 0;
  for (uint32_t s = 0; s < n; ++s) {
    if (!listed(codes[s], kind, lo, hi)) continue;
    if (L % kPgenGroup != 0) deltas += pgen_varint_len(s - prev);
    prev = s;
    ++L;
  }
  if (L == 0) return 1;
  const uint64_t G = (L + kPgenGroup - 1) / kPgenGroup;
  return pgen_varint_len(static_cast<uint32_t>(L)) + G * static_cast<uint64_t>(pgen_index_width(n)) + (G - 1) + (L + 3) / 4 + deltas;
}

uint8_t* put_difflist(uint8_t* at, const uint8_t* codes, uint32_t n, uint32_t kind, uint32_t lo, uint32_t hi) {
  uint32_t L = 0;
  for (uint32_t s = 0; s < n; ++s) L += listed(codes[s], kind, lo, hi);
  put_varint(at, L);
  if (L == 0) return at;
  const uint32_t G = (L + kPgenGroup - 1) / kPgenGroup;
  const int w = pgen_index_width(n);
  uint8_t* firsts = at;
  uint8_t* sizes = firsts + static_cast<size_t>(G) * w;
  uint8_t* code_at = sizes + (G - 1);
  uint8_t* delta_at = code_at + (L + 3) / 4;
  std::fill(code_at, delta_at, uint8_t(0));
  uint32_t k = 0, prev = 0;
  uint8_t* group_start = delta_at;
  for (uint32_t s = 0; s < n; ++s) {
    if (!listed(codes[s], kind, lo, hi)) continue;
    if (k % kPgenGroup == 0) {
      const uint32_t g = k / kPgenGroup;
      for (int b = 0; b < w; ++b) firsts[static_cast<size_t>(g) * w + b] = static_cast<uint8_t>(s >> (8 * b));
      if (g > 0) sizes[g - 1] = static_cast<uint8_t>((delta_at - group_start) - (kPgenGroup - 1));
      group_start = delta_at;
    } else {
      put_varint(delta_at, s - prev);
    }
    code_at[k >> 2] |= static_cast<uint8_t>(codes[s] << (2 * (k & 3u)));
    prev = s;
    ++k;
  }
  return delta_at;
}

// type and length of the row whose codes are given
void plan_row(const uint8_t* codes, uint32_t n, uint32_t* kind_out, uint64_t* len_out, uint32_t* lo_out, uint32_t* hi_out) {
  uint32_t count[4] = {0, 0, 0, 0};
  for (uint32_t s = 0; s < n; ++s) ++count[codes[s]];
  uint32_t lo, hi;
  pgen_onebit_pair(count, &lo, &hi);
  uint32_t best_kind = 0;
  uint64_t best = (static_cast<uint64_t>(n) + 3) / 4;
  const uint32_t kinds[4] = {1, 4, 6, 7};  // ascending: a tie stays with the lower type
  for (uint32_t kind : kinds) {
    uint64_t size = difflist_size(codes, n, kind, lo, hi);
    if (kind == 1) size += 1 + (static_cast<uint64_t>(n) + 7) / 8;
    if (size < best) {
      best = size;
      best_kind = kind;
    }
  }
  *kind_out = best_kind;
  *len_out = best;
  *lo_out = lo;
  *hi_out = hi;
}

uint8_t* put_row(uint8_t* at, const uint8_t* codes, uint32_t n, uint32_t kind, uint32_t lo, uint32_t hi) {
  if (kind == 0) {
    for (uint64_t b = 0; b < (static_cast<uint64_t>(n) + 3) / 4; ++b) {
      uint32_t byte = 0;
      for (uint32_t k = 0; k < 4 && 4 * b + k < n; ++k) byte |= static_cast<uint32_t>(codes[4 * b + k]) << (2 * k);  // padding bits: 0
      *at++ = static_cast<uint8_t>(byte);
    }
    return at;
  }
  if (kind == 1) {
    *at++ = static_cast<uint8_t>(4 * lo + (hi - lo));
    for (uint64_t b = 0; b < (static_cast<uint64_t>(n) + 7) / 8; ++b) {
      uint32_t byte = 0;
      for (uint32_t k = 0; k < 8 && 8 * b + k < n; ++k) byte |= static_cast<uint32_t>(codes[8 * b + k] == hi) << k;
      *at++ = static_cast<uint8_t>(byte);
    }
  }
  return put_difflist(at, codes, n, kind, lo, hi);
}

template <class F>
void over_rows(const Call& c, int32_t n_threads, F&& body) {
  // one thread for every 2^18 cells of work, as the host decoders
  const int64_t cells = c.n_rows * c.n_slots;
  const int nt = static_cast<int>(std::max<int64_t>(1, std::min<int64_t>({static_cast<int64_t>(std::max(n_threads, 1)), c.n_rows, cells / (int64_t(1) << 18) + 1})));
  ThreadGroup tg;
  const int64_t n_rows = c.n_rows;
  for (int t = 1; t < nt; ++t) tg.spawn([&body, t, nt, n_rows] { body(n_rows * t / nt, n_rows * (t + 1) / nt); });
  body(0, n_rows / nt);
  tg.join();
}

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
