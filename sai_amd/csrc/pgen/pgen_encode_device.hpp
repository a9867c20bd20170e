// What the kernels of sai_pgen_encode (pgen_encode.hip) and of sai_pgen_encode_ld (pgen_encode_ld.hip) share: the
// recoding of a row of the int8 block into words of 2-bit codes, the counts of a row, and the difflist, sized or
// written by one routine so that a plan and a write kernel cannot disagree.  Device code only: a .hip unit includes
// this file once, and everything here is local to that unit.  The rules are stated in pgen_export.hpp and
// pgen_export_ld.hpp, the kernels that use these pieces in the two units.
//
// The difflist (size_or_write_difflist): a step takes 1 024 samples; the lanes' entries are ranked by a wave prefix
// sum of their popcounts and compacted, index and code, into an LDS buffer behind what the step before left.  Every
// full 64 entries of the buffer are one group of the list: lane j holds entry j, the delta to entry j - 1 is a varint
// of 1 .. 5 bytes, a wave prefix sum of those lengths gives every delta's byte and the group's size, the first
// entry's index goes to the group's slot of the index array, the size to the byte array behind it (positions known
// from L alone, the values only now), and the 64 codes to 16 bytes, put together from two ballots.  What is left
// (fewer than 64 entries) moves to the buffer's front; the last group is flushed after the last step.
//
// With LD set, the kinds 2 and 3 list the samples whose code differs from a base row's (kind 3: from the base row
// with the codes 0 and 2 exchanged); the base is a second RowView.  Without it that view is never read, and the
// routine is what it was before the kinds 2 and 3 existed.
#pragma once

#include "../common.hpp"
#include "pgen_codes.hpp"
#include "pgen_export.hpp"

namespace {

constexpr int kWave = 64;
constexpr int kTileWords = 1024;               // 32-bit words of codes kept in LDS per row: 16 384 samples
constexpr int kStepEntries = kWave * 16;       // entries a step can add
constexpr int kEntCap = kStepEntries + kWave;  // ... behind fewer than 64 left over
constexpr uint32_t kOnes = 0x01010101u;
constexpr uint32_t kLow = 0x55555555u;  // the low bit of each 2-bit field
constexpr int kWavesPerCu = 16;

struct EncodeArgs {
  const uint8_t* in;  // the dosages as bytes
  int64_t in_bytes;   // n_rows * n_slots
  int64_t n_rows;
  uint32_t n;          // n_slots
  uint32_t n_words;    // ceil(n / 16)
  uint32_t row_bytes;  // ceil(n / 4)
  const int32_t* ploidy_of_slot;
  int32_t uniform_ploidy;  // 1 or 2: every slot; 0: ploidy_of_slot
  uint8_t* out;
  uint8_t* vrtype;
  uint32_t* length;
  uint32_t* offsets;  // [n_rows + 1]
  int32_t* status;
};

// the aligned 16-byte word at byte `at` of the input (at % 16 == 0); bytes behind the input are 0
__device__ __forceinline__ u32x4 load_word(const EncodeArgs& a, int64_t at) {
  if (at + 16 <= a.in_bytes) return *reinterpret_cast<const u32x4*>(a.in + at);
  u32x4 w = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (at + 4 * j + k < a.in_bytes) w[j] |= static_cast<uint32_t>(a.in[at + 4 * j + k]) << (8 * k);
  return w;
}

// bits 8k, 8k + 1 of t (k = 0 .. 3) -> bits 2k, 2k + 1
__device__ __forceinline__ uint32_t gather4(uint32_t t) {
  t |= t >> 6;
  return (t | (t >> 12)) & 0xFFu;
}

// Four dosages (the bytes of w) -> their four codes in bits 0 .. 7; `bad` gets bit 8k set where byte k is outside
// the table.  b0 / b1 are the two low bits of every byte; `small` marks the bytes 0 .. 3 and `neg` the bytes
// -4 .. -1 (the six high bits all 0 / all 1, found without a carry between bytes: they are shifted down first).
template <int PLOIDY>
__device__ __forceinline__ uint32_t encode4(uint32_t w, uint32_t& bad) {
  const uint32_t b0 = w & kOnes, b1 = (w >> 1) & kOnes;
  const uint32_t high = (w >> 2) & 0x3F3F3F3Fu;
  const uint32_t small = ~((high + 0x3F3F3F3Fu) >> 6) & kOnes;
  const uint32_t neg = ~(((high ^ 0x3F3F3F3Fu) + 0x3F3F3F3Fu) >> 6) & kOnes;
  uint32_t lo, hi;
  if (PLOIDY == 2) {
    // 0 -> 00, 1 -> 01, 2 -> 10, -2 (..10) -> 11; anything else 11
    const uint32_t other = ~(small & ~(b0 & b1)) & kOnes;  // not 0, 1 or 2
    lo = b0 | other;
    hi = b1 | other;
    bad = other & ~(neg & b1 & ~b0);
  } else {
    // 0 -> 00, 1 -> 10, -1 (..11) -> 11; anything else 11
    const uint32_t other = ~(small & ~b1) & kOnes;  // not 0 or 1
    lo = other;
    hi = b0 | other;
    bad = other & ~(neg & b1 & b0);
  }
  // Masked once more although lo and hi hold nothing outside bit 0 of a byte: gather4 ORs shifted copies, so it needs
  // clean fields, and a first form of these lines -- (b & plain) | (~plain & kOnes) -- came out of the compiler
  // (ROCm's clang for gfx950, which folds such terms into v_bitop3_b32) with the mask on b & plain gone and wrong
  // codes behind every byte with bit 2 set and bit 1 clear.  tests/test_pgen_export_device.py runs all 256 values.
  return gather4((lo | (hi << 1)) & 0x03030303u);
}

// Word i of the dense form of the row whose first dosage is byte `row_at` of the input: the codes of samples
// 16 i .. 16 i + 15, those behind the row 0.  *bad: bit 2k set where sample 16 i + k holds a value outside the table;
// *ploidy_bad: one of its ploidies is outside 1 .. 2 (its code is 3).
__device__ __forceinline__ uint32_t row_word(const EncodeArgs& a, int64_t row_at, uint32_t i, uint32_t* bad, bool* ploidy_bad) {
  const int64_t at = row_at + 16 * static_cast<int64_t>(i);  // < in_bytes
  const int64_t base = at & ~int64_t(15);
  const uint32_t shift = static_cast<uint32_t>(at & 15);
  const u32x4 v0 = load_word(a, base);
  u32x4 v1 = {0u, 0u, 0u, 0u};
  if (shift) v1 = load_word(a, base + 16);
  const uint32_t w[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
  const uint32_t q = shift >> 2, bits = (shift & 3u) * 8u;
  const uint32_t s0 = 16u * i;
  const uint32_t nv = a.n - s0 < 16u ? a.n - s0 : 16u;  // the samples of this word: 1 .. 16
  uint32_t codes = 0, bad_all = 0;
  bool pl_bad = false;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    // words j + q and j + q + 1, picked with selects: q is the lane's own, the indices stay static
    const uint32_t lo = q == 0 ? w[j] : q == 1 ? w[j + 1] : q == 2 ? w[j + 2] : w[j + 3];
    const uint32_t hi = q == 0 ? w[j + 1] : q == 1 ? w[j + 2] : q == 2 ? w[j + 3] : w[j + 4];
    const uint32_t src = __funnelshift_r(lo, hi, bits);
    uint32_t c, b;
    if (a.uniform_ploidy == 2) {
      c = encode4<2>(src, b);
    } else if (a.uniform_ploidy == 1) {
      c = encode4<1>(src, b);
    } else {
      // per-slot ploidies: both recodings, and per field the one its slot's ploidy asks for; neither: 11
      uint32_t m1 = 0, m2 = 0;  // bit 8k: sample k of these four has ploidy 1 / 2
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (static_cast<uint32_t>(4 * j + k) < nv) {
          const int32_t pl = a.ploidy_of_slot[s0 + 4 * j + k];
          m1 |= static_cast<uint32_t>(pl == 1) << (8 * k);
          m2 |= static_cast<uint32_t>(pl == 2) << (8 * k);
          pl_bad |= pl != 1 && pl != 2;
        }
      uint32_t b1, b2;
      const uint32_t c1 = encode4<1>(src, b1), c2 = encode4<2>(src, b2);
      const uint32_t f1 = gather4(m1 | (m1 << 1)), f2 = gather4(m2 | (m2 << 1));
      c = (c1 & f1) | (c2 & f2) | (0xFFu & ~(f1 | f2));
      b = (b1 & m1) | (b2 & m2);
    }
    codes |= c << (8 * j);
    bad_all |= gather4(b) << (8 * j);
  }
  if (nv < 16u) {
    const uint32_t keep = (1u << (2u * nv)) - 1u;
    codes &= keep;
    bad_all &= keep;
  }
  *bad = bad_all;
  *ploidy_bad = pl_bad;
  return codes;
}

// bit 2k set where field k of `codes` is `x`
__device__ __forceinline__ uint32_t fields_equal(uint32_t codes, uint32_t x) {
  const uint32_t t = codes ^ (x * kLow);
  return ~(t | (t >> 1)) & kLow;
}

// bit 2k set for every sample of word i, none behind the row
__device__ __forceinline__ uint32_t valid_fields(uint32_t n, uint32_t i) {
  const uint32_t left = n - 16u * i;
  return left >= 16u ? kLow : kLow & ((1u << (2u * left)) - 1u);
}

// bit 2k set where sample k of the word is listed by a record of `kind`
__device__ __forceinline__ uint32_t listed_fields(uint32_t codes, uint32_t valid, uint32_t kind, uint32_t lo, uint32_t hi) {
  if (kind == 1) return valid & ~fields_equal(codes, lo) & ~fields_equal(codes, hi);
  return valid & ~fields_equal(codes, kind == 4 ? 0u : kind == 6 ? 2u : 3u);
}

// every field of `codes` with the codes 0 and 2 exchanged: bit 1 of a field flips where its bit 0 is clear
__device__ __forceinline__ uint32_t swap02_fields(uint32_t codes) { return codes ^ ((~codes & kLow) << 1); }

// bit 2k set where sample k of the word differs from the base row's (kind 2) or from the base row's with 0 and 2
// exchanged (kind 3)
__device__ __forceinline__ uint32_t differing_fields(uint32_t codes, uint32_t base, uint32_t valid, uint32_t kind) {
  const uint32_t t = codes ^ (kind == 3 ? swap02_fields(base) : base);
  return valid & (t | (t >> 1)) & kLow;
}

__device__ __forceinline__ uint32_t wave_inclusive_sum(uint32_t v, int lane) {
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const uint32_t t = __shfl_up(v, off);
    if (lane >= off) v += t;
  }
  return v;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// bits 0 .. 3 of x -> bits 0, 2, 4, 6
__device__ __forceinline__ uint32_t spread4(uint32_t x) {
  x = (x | (x << 2)) & 0x33u;
  return (x | (x << 1)) & 0x55u;
}

// one byte of a record: `pos` counted from the record's first byte, of which it has `room`
template <bool WRITE>
__device__ __forceinline__ void put(uint8_t* rec, uint32_t room, uint32_t pos, uint32_t byte) {
  if (WRITE && pos < room) rec[pos] = static_cast<uint8_t>(byte);
}

// What the kernels keep of a row between passes: where it starts, and its first kTileWords words when `tile` is set.
struct RowView {
  int64_t row_at;
  const uint32_t* tile;  // NULL: every word comes from the block
};

__device__ __forceinline__ uint32_t view_word(const EncodeArgs& a, const RowView& v, uint32_t i) {
  if (v.tile && i < static_cast<uint32_t>(kTileWords)) return v.tile[i];
  uint32_t bad;
  bool pl_bad;
  return row_word(a, v.row_at, i, &bad, &pl_bad);
}

// The difflist of a record of `kind` with L entries, written from byte `at` of the record (WRITE) or only sized.
// Returns the list's bytes, to every lane.  Called by all 64 lanes of a single-wave workgroup: the __syncthreads()
// are barriers of that one wavefront.  LD: the kinds 2 and 3 are known, and `bv` is the base row they list against.
// Always inlined: as a function of its own it would take the arguments' structures through scratch memory.
template <bool WRITE, bool LD>
__device__ __forceinline__ uint32_t size_or_write_difflist_of(const EncodeArgs& a, const RowView& v, const RowView& bv, uint32_t kind, uint32_t lo, uint32_t hi,
                                              uint32_t L, uint8_t* rec, uint32_t room, uint32_t at, uint32_t* ent_idx, uint8_t* ent_code) {
  const int lane = threadIdx.x;
  const uint32_t len_l = pgen_varint_len(L);
  if (lane == 0) {
    uint32_t value = L, pos = at;
    while (value >= 128u) {
      put<WRITE>(rec, room, pos++, 128u | (value & 127u));
      value >>= 7;
    }
    put<WRITE>(rec, room, pos, value);
  }
  if (L == 0) return len_l;
  const uint32_t G = (L + kPgenGroup - 1) / kPgenGroup;
  const uint32_t w = static_cast<uint32_t>(pgen_index_width(a.n));
  const uint32_t firsts_at = at + len_l, sizes_at = firsts_at + G * w, codes_at = sizes_at + (G - 1);
  const uint32_t deltas_at = codes_at + (L + 3) / 4;
  uint32_t fill = 0;         // entries in the buffer
  uint32_t g = 0;            // groups flushed
  uint32_t delta_bytes = 0;  // of the groups flushed

  auto flush = [&](uint32_t b, uint32_t cnt) {  // the entries [b, b + cnt) of the buffer are group g
    const bool mine = static_cast<uint32_t>(lane) < cnt;
    const uint32_t idx = mine ? ent_idx[b + lane] : 0u;
    const uint32_t before = mine && lane > 0 ? ent_idx[b + lane - 1] : 0u;
    const uint32_t code = mine ? ent_code[b + lane] : 0u;
    const uint32_t dl = mine && lane > 0 ? pgen_varint_len(idx - before) : 0u;
    const uint32_t incl = wave_inclusive_sum(dl, lane);
    const uint32_t group_bytes = __shfl(incl, kWave - 1);
    if (WRITE) {
      if (lane == 0) {
        for (uint32_t k = 0; k < w; ++k) put<WRITE>(rec, room, firsts_at + g * w + k, (idx >> (8 * k)) & 0xFFu);
        if (g + 1 < G) put<WRITE>(rec, room, sizes_at + g, group_bytes - (kPgenGroup - 1));
      } else if (mine) {
        uint32_t pos = deltas_at + delta_bytes + (incl - dl), value = idx - before;
        while (value >= 128u) {
          put<WRITE>(rec, room, pos++, 128u | (value & 127u));
          value >>= 7;
        }
        put<WRITE>(rec, room, pos, value);
      }
      const unsigned long long low = __ballot(code & 1u), high = __ballot(code & 2u);
      if (4u * lane < cnt) {
        const uint32_t byte = spread4(static_cast<uint32_t>(low >> (4 * lane)) & 15u) | (spread4(static_cast<uint32_t>(high >> (4 * lane)) & 15u) << 1);
        put<WRITE>(rec, room, codes_at + 16u * g + lane, byte);
      }
    }
    delta_bytes += group_bytes;
    ++g;
  };

  for (uint32_t i0 = 0; i0 < a.n_words; i0 += kWave) {
    const uint32_t i = i0 + lane;
    uint32_t codes = 0, listed = 0;
    if (i < a.n_words) {
      codes = view_word(a, v, i);
      if (LD && (kind == 2 || kind == 3))
        listed = differing_fields(codes, view_word(a, bv, i), valid_fields(a.n, i), kind);
      else
        listed = listed_fields(codes, valid_fields(a.n, i), kind, lo, hi);
    }
    const uint32_t here = __popc(listed);
    const uint32_t incl = wave_inclusive_sum(here, lane);
    uint32_t slot = fill + (incl - here);
    for (uint32_t m = listed; m; m &= m - 1) {
      const uint32_t bit = __builtin_ctz(m);
      ent_idx[slot] = 16u * i + (bit >> 1);
      ent_code[slot] = static_cast<uint8_t>((codes >> bit) & 3u);
      ++slot;
    }
    fill += __shfl(incl, kWave - 1);
    __syncthreads();
    const uint32_t whole = fill / kPgenGroup;
    for (uint32_t t = 0; t < whole; ++t) flush(t * kPgenGroup, kPgenGroup);
    const uint32_t left = fill - whole * kPgenGroup;
    if (whole > 0) {  // what is left moves to the front
      uint32_t idx = 0, code = 0;
      if (static_cast<uint32_t>(lane) < left) {
        idx = ent_idx[whole * kPgenGroup + lane];
        code = ent_code[whole * kPgenGroup + lane];
      }
      __syncthreads();
      if (static_cast<uint32_t>(lane) < left) {
        ent_idx[lane] = idx;
        ent_code[lane] = static_cast<uint8_t>(code);
      }
    }
    fill = left;
    __syncthreads();
  }
  if (fill > 0) flush(0, fill);
  __syncthreads();  // the next caller overwrites the buffer
  return deltas_at + delta_bytes - at;
}

// the same for the kinds 1, 4, 6 and 7 alone, which have no base row
template <bool WRITE>
__device__ __forceinline__ uint32_t size_or_write_difflist(const EncodeArgs& a, const RowView& v, uint32_t kind, uint32_t lo, uint32_t hi, uint32_t L,
                                                           uint8_t* rec, uint32_t room, uint32_t at, uint32_t* ent_idx, uint8_t* ent_code) {
  return size_or_write_difflist_of<WRITE, false>(a, v, v, kind, lo, hi, L, rec, room, at, ent_idx, ent_code);
}

// the four code counts of the row (to every lane); with `tile` the first kTileWords words are kept in it
__device__ __forceinline__ void count_row(const EncodeArgs& a, int64_t row_at, uint32_t* tile, uint32_t count[4], int32_t* status) {
  const int lane = threadIdx.x;
  uint32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0;
  int32_t st = 0;
  for (uint32_t i = lane; i < a.n_words; i += kWave) {
    uint32_t bad;
    bool pl_bad;
    const uint32_t codes = row_word(a, row_at, i, &bad, &pl_bad);
    if (tile && i < static_cast<uint32_t>(kTileWords)) tile[i] = codes;
    const uint32_t valid = valid_fields(a.n, i);
    c0 += __popc(fields_equal(codes, 0u) & valid);
    c1 += __popc(fields_equal(codes, 1u) & valid);
    c2 += __popc(fields_equal(codes, 2u) & valid);
    c3 += __popc(fields_equal(codes, 3u) & valid);
    if (bad) {  // the lowest slot of the lane's first such word is the lane's lowest
      const int32_t here = static_cast<int32_t>(a.n - (16u * i + (static_cast<uint32_t>(__builtin_ctz(bad)) >> 1)));
      st = st > here ? st : here;
    }
    if (pl_bad) st = kPgenBadIndex;
  }
  count[0] = wave_sum(c0);
  count[1] = wave_sum(c1);
  count[2] = wave_sum(c2);
  count[3] = wave_sum(c3);
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    const int32_t t = __shfl_xor(st, off);
    st = st > t ? st : t;
  }
  *status = st;
}

__device__ __forceinline__ uint32_t entries_of(uint32_t n, const uint32_t count[4], uint32_t kind, uint32_t lo, uint32_t hi) {
  if (kind == 1) return n - count[lo] - count[hi];
  return n - count[kind == 4 ? 0 : kind == 6 ? 2 : 3];
}

// What a record of `row`, of a kind that needs no other row (0, 1, 4, 6 or 7), holds before its difflist, written at
// `rec`, of which it has `room` bytes: the row is recoded from the block and stored byte by byte but for the whole
// words of a 4-byte aligned dense record.  false: the record is complete (type 0).  true: a difflist of *L entries
// follows at byte *at, with the pair (*lo, *hi) of a type 1 record; the row was counted again for them.  Called by all
// 64 lanes of a single-wave workgroup.
__device__ __forceinline__ bool write_record_head(const EncodeArgs& a, int64_t row_at, uint32_t kind, uint8_t* rec, uint32_t room, uint32_t* lo_out,
                                                  uint32_t* hi_out, uint32_t* L, uint32_t* at_out) {
  const int lane = threadIdx.x;
  if (kind == 0) {
    const bool aligned = (reinterpret_cast<uintptr_t>(rec) & 3u) == 0;
    for (uint32_t i = lane; i < a.n_words; i += kWave) {
      uint32_t bad;
      bool pl_bad;
      const uint32_t codes = row_word(a, row_at, i, &bad, &pl_bad);
      if (aligned && 4u * i + 4u <= room) {
        *reinterpret_cast<uint32_t*>(rec + 4u * i) = codes;
      } else {
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k)
          if (4u * i + k < a.row_bytes) put<true>(rec, room, 4u * i + k, (codes >> (8 * k)) & 0xFFu);
      }
    }
    return false;
  }
  uint32_t count[4];
  int32_t st;
  count_row(a, row_at, nullptr, count, &st);
  uint32_t lo, hi;
  pgen_onebit_pair(count, &lo, &hi);
  uint32_t at = 0;
  if (kind == 1) {
    if (lane == 0) put<true>(rec, room, 0u, 4u * lo + (hi - lo));
    const uint32_t bit_bytes = (a.n + 7u) / 8u;
    for (uint32_t i = lane; i < a.n_words; i += kWave) {
      uint32_t bad;
      bool pl_bad;
      const uint32_t is_hi = fields_equal(row_word(a, row_at, i, &bad, &pl_bad), hi) & valid_fields(a.n, i);
      // bit 2k -> bit k: the low bits of the fields, packed
      uint32_t x = is_hi;
      x = (x | (x >> 1)) & 0x33333333u;
      x = (x | (x >> 2)) & 0x0F0F0F0Fu;
      x = (x | (x >> 4)) & 0x00FF00FFu;
      x = (x | (x >> 8)) & 0x0000FFFFu;
      if (2u * i < bit_bytes) put<true>(rec, room, 1u + 2u * i, x & 0xFFu);
      if (2u * i + 1u < bit_bytes) put<true>(rec, room, 2u + 2u * i, x >> 8);
    }
    at = 1u + bit_bytes;
  }
  *lo_out = lo;
  *hi_out = hi;
  *L = entries_of(a.n, count, kind, lo, hi);
  *at_out = at;
  return true;
}

// The fields of the call's arguments that follow from the sizes.
inline EncodeArgs encode_args(const int8_t* dosage, int64_t n_rows, int32_t n_slots, const int32_t* ploidy_of_slot, int32_t uniform_ploidy, uint8_t* out,
                              uint8_t* vrtype, uint32_t* length, uint32_t* offsets, int32_t* status) {
  EncodeArgs a;
  a.in = reinterpret_cast<const uint8_t*>(dosage);
  a.in_bytes = n_rows * n_slots;
  a.n_rows = n_rows;
  a.n = static_cast<uint32_t>(n_slots);
  a.n_words = (a.n + 15u) / 16u;
  a.row_bytes = (a.n + 3u) / 4u;
  a.ploidy_of_slot = ploidy_of_slot;
  a.uniform_ploidy = uniform_ploidy;
  a.out = out;
  a.vrtype = vrtype;
  a.length = length;
  a.offsets = offsets;
  a.status = status;
  return a;
}

}  // namespace
