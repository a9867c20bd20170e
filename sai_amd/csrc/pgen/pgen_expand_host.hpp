// The record expansion of the host decoders, shared by sai_pgen_decode_host (pgen_index.cpp: int8 rows) and
// sai_pgen_pack2_host (pgen_pack2_host.cpp: packed2 blocks): one record of a .pgen -> the hard-call code of every
// sample, one byte each.  The plain statement of the format rules of DESIGN_INGEST.md ("PLINK 2 filesets"), moved
// here from pgen_index.cpp as it stood so that the rules are stated once.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>

#include "pgen_codes.hpp"

namespace {

inline uint64_t load_le(const uint8_t* p, int n) {
  uint64_t v = 0;
  for (int k = 0; k < n; ++k) v |= static_cast<uint64_t>(p[k]) << (8 * k);
  return v;
}

inline bool get_varint(const uint8_t*& p, const uint8_t* e, uint64_t& v) {
  v = 0;
  for (int k = 0; k < kPgenMaxVarint; ++k) {
    if (p >= e) return false;
    const uint8_t b = *p++;
    v |= static_cast<uint64_t>(b & 0x7Fu) << (7 * k);
    if (!(b & 0x80u)) return true;
  }
  return false;
}

// the difflist at [p, e) of a record: its entries overwrite codes[0 .. n)
bool apply_difflist(const uint8_t* p, const uint8_t* e, uint32_t n, uint8_t* codes) {
  uint64_t L;
  if (!get_varint(p, e, L)) return false;
  if (L == 0) return true;
  if (L > n) return false;
  const uint64_t G = (L + kPgenGroup - 1) / kPgenGroup;
  const int w = pgen_index_width(n);
  const uint64_t fixed = G * w + (G - 1) + (L + 3) / 4;
  if (static_cast<uint64_t>(e - p) < fixed) return false;
  const uint8_t* firsts = p;
  const uint8_t* sizes = firsts + G * w;
  const uint8_t* code_bytes = sizes + (G - 1);
  const uint8_t* d = code_bytes + (L + 3) / 4;
  int64_t prev = -1;
  for (uint64_t g = 0; g < G; ++g) {
    uint64_t at = load_le(firsts + g * w, w);
    if (at >= n || static_cast<int64_t>(at) <= prev) return false;
    const uint64_t k0 = g * kPgenGroup, cnt = std::min<uint64_t>(kPgenGroup, L - k0);
    const uint8_t* group_end = e;
    if (g + 1 < G) {
      const uint64_t bytes = static_cast<uint64_t>(sizes[g]) + (kPgenGroup - 1);
      if (static_cast<uint64_t>(e - d) < bytes) return false;
      group_end = d + bytes;
    }
    codes[at] = (code_bytes[k0 >> 2] >> (2 * (k0 & 3))) & 3u;
    for (uint64_t j = 1; j < cnt; ++j) {
      uint64_t delta;
      if (!get_varint(d, group_end, delta) || delta == 0) return false;
      at += delta;
      if (at >= n) return false;
      const uint64_t k = k0 + j;
      codes[at] = (code_bytes[k >> 2] >> (2 * (k & 3))) & 3u;
    }
    if (g + 1 < G && d != group_end) return false;
    prev = static_cast<int64_t>(at);
  }
  return true;
}

struct RecordRef {
  int64_t off, len, vrtype;
};

// a record that stands alone (type 0, 1, 4, 6, 7) into codes[0 .. n)
bool expand_alone(const uint8_t* bytes, int64_t n_bytes, const RecordRef& r, uint32_t n, uint8_t* codes) {
  if (r.off < 0 || r.len < 0 || r.off > n_bytes || r.len > n_bytes - r.off) return false;
  const uint8_t* p = bytes + r.off;
  const uint8_t* e = p + r.len;
  const unsigned kind = static_cast<unsigned>(r.vrtype) & 7u;
  switch (kind) {
    case 0: {
      if (static_cast<uint64_t>(r.len) < (static_cast<uint64_t>(n) + 3) / 4) return false;
      for (uint32_t i = 0; i < n; ++i) codes[i] = (p[i >> 2] >> (2 * (i & 3))) & 3u;
      return true;
    }
    case 1: {
      const uint64_t bit_bytes = (static_cast<uint64_t>(n) + 7) / 8;
      if (static_cast<uint64_t>(r.len) < 1 + bit_bytes) return false;
      const uint32_t b = p[0];
      if (!pgen_onebit_legal(b)) return false;
      const uint8_t lo = static_cast<uint8_t>(b >> 2), hi = static_cast<uint8_t>(lo + (b & 3u));
      for (uint32_t i = 0; i < n; ++i) codes[i] = (p[1 + (i >> 3)] >> (i & 7)) & 1u ? hi : lo;
      return apply_difflist(p + 1 + bit_bytes, e, n, codes);
    }
    case 4:
    case 6:
    case 7:
      memset(codes, kind == 4 ? 0 : kind == 6 ? 2 : 3, n);
      return apply_difflist(p, e, n, codes);
    default:  // 5 is reserved; 2 and 3 are no base
      return false;
  }
}

bool expand_record(const uint8_t* bytes, int64_t n_bytes, const RecordRef& r, const RecordRef& base, uint32_t n, uint8_t* codes) {
  const unsigned kind = static_cast<unsigned>(r.vrtype) & 7u;
  if (kind != 2 && kind != 3) return expand_alone(bytes, n_bytes, r, n, codes);
  if (r.off < 0 || r.len < 0 || r.off > n_bytes || r.len > n_bytes - r.off) return false;
  if (base.off < 0 || !expand_alone(bytes, n_bytes, base, n, codes)) return false;
  if (kind == 3)
    for (uint32_t i = 0; i < n; ++i) codes[i] ^= static_cast<uint8_t>((~codes[i] & 1u) << 1);  // 0 <-> 2; 1 and 3 stay
  return apply_difflist(bytes + r.off, bytes + r.off + r.len, n, codes);
}

}  // namespace
