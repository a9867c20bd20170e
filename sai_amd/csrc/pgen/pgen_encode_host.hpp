// What the two host encoders of .pgen records share (pgen_encode_host.cpp, pgen_encode_ld_host.cpp): the codes of a
// row of the int8 block, the difflist sized and written sample by sample, a record of the types that need no other
// row, and the split of a call over threads.  The plain statement of pgen_export.hpp; host code only, local to the
// unit that includes it.
#pragma once

#include <algorithm>
#include <vector>

#include "../host_threads.hpp"
#include "pgen_codes.hpp"
#include "pgen_export.hpp"

namespace {

struct Call {
  const int8_t* dosage;
  int64_t n_rows;
  int32_t n_slots;
  const int32_t* ploidy_of_slot;
  int32_t uniform_ploidy;
};

// the codes of one row and its status
inline int32_t codes_of_row(const Call& c, int64_t row, uint8_t* codes) {
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

// Which samples a record lists: those that differ from what the record's other part says of them.  With `start` that
// part is a row of codes (the base row of a type 2 or 3 record, as that type reads it); without, it follows from
// `kind`: the pair of a type 1 record, the constant of a type 4, 6 or 7 one.
inline bool listed(const uint8_t* codes, const uint8_t* start, uint32_t s, uint32_t kind, uint32_t lo, uint32_t hi) {
  if (start) return codes[s] != start[s];
  if (kind == 1) return codes[s] != lo && codes[s] != hi;
  return codes[s] != (kind == 4 ? 0u : kind == 6 ? 2u : 3u);
}

inline void put_varint(uint8_t*& at, uint32_t v) {
  while (v >= 128u) {
    *at++ = static_cast<uint8_t>(128u | (v & 127u));
    v >>= 7;
  }
  *at++ = static_cast<uint8_t>(v);
}

// bytes of the difflist of a record of `kind`
inline uint64_t difflist_size(const uint8_t* codes, const uint8_t* start, uint32_t n, uint32_t kind, uint32_t lo, uint32_t hi) {
  uint64_t L = 0, deltas = 0;
  uint32_t prev = 0;
  for (uint32_t s = 0; s < n; ++s) {
    if (!listed(codes, start, s, kind, lo, hi)) continue;
    if (L % kPgenGroup != 0) deltas += pgen_varint_len(s - prev);
    prev = s;
    ++L;
  }
  if (L == 0) return 1;
  const uint64_t G = (L + kPgenGroup - 1) / kPgenGroup;
  return pgen_varint_len(static_cast<uint32_t>(L)) + G * static_cast<uint64_t>(pgen_index_width(n)) + (G - 1) + (L + 3) / 4 + deltas;
}

inline uint8_t* put_difflist(uint8_t* at, const uint8_t* codes, const uint8_t* start, uint32_t n, uint32_t kind, uint32_t lo, uint32_t hi) {
  uint32_t L = 0;
  for (uint32_t s = 0; s < n; ++s) L += listed(codes, start, s, kind, lo, hi);
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
    if (!listed(codes, start, s, kind, lo, hi)) continue;
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

// type and length of the row whose codes are given, among the types 0, 1, 4, 6 and 7
inline void plan_row(const uint8_t* codes, uint32_t n, uint32_t* kind_out, uint64_t* len_out, uint32_t* lo_out, uint32_t* hi_out) {
  uint32_t count[4] = {0, 0, 0, 0};
  for (uint32_t s = 0; s < n; ++s) ++count[codes[s]];
  uint32_t lo, hi;
  pgen_onebit_pair(count, &lo, &hi);
  uint32_t best_kind = 0;
  uint64_t best = (static_cast<uint64_t>(n) + 3) / 4;
  const uint32_t kinds[4] = {1, 4, 6, 7};  // ascending: a tie stays with the lower type
  for (uint32_t kind : kinds) {
    uint64_t size = difflist_size(codes, nullptr, n, kind, lo, hi);
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

// the record of a row of type 0, 1, 4, 6 or 7
inline uint8_t* put_row(uint8_t* at, const uint8_t* codes, uint32_t n, uint32_t kind, uint32_t lo, uint32_t hi) {
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
  return put_difflist(at, codes, nullptr, n, kind, lo, hi);
}

// body(first, last) over [0, n_items) in contiguous parts, one per thread: one thread for every 2^18 cells of work,
// as the host decoders
template <class F>
void over_items(int64_t n_items, int64_t cells, int32_t n_threads, F&& body) {
  const int nt = static_cast<int>(std::max<int64_t>(1, std::min<int64_t>({static_cast<int64_t>(std::max(n_threads, 1)), n_items, cells / (int64_t(1) << 18) + 1})));
  ThreadGroup tg;
  for (int t = 1; t < nt; ++t) tg.spawn([&body, t, nt, n_items] { body(n_items * t / nt, n_items * (t + 1) / nt); });
  body(0, n_items / nt);
  tg.join();
}

template <class F>
void over_rows(const Call& c, int32_t n_threads, F&& body) {
  over_items(c.n_rows, c.n_rows * c.n_slots, n_threads, body);
}

}  // namespace
