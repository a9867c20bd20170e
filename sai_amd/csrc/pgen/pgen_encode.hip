// sai_pgen_encode: int8 dosages [row][slot] in HBM -> the hard-call records of a PLINK 2 .pgen, back to back in row
// order: the inverse of sai_pgen_decode (pgen_export.hpp has the table and the size rules; the plain statement of
// them is pgen_encode_host.cpp, and these kernels make the same decisions).  Three kernels:
//
//  * plan -- one wavefront (one 64-lane workgroup, as pgen_decode.hip) per row.  A lane takes 16 samples at a time:
//    the row starts at any byte of the block, so it loads the two aligned 128-bit words that hold its 16 dosages and
//    funnel-shifts them into place (as plink/bed_encode.hip does), then recodes four dosages at a time by bit
//    operations into one 32-bit word of 2-bit codes -- word i of the row's dense form.  The words stay in LDS (4 KiB,
//    16 384 samples: the decoder's tile), the four code counts come from popcounts, the status from the mask of the
//    values outside the table.  With the counts every candidate's entry count L is known, and a candidate is sized
//    only when 5 L < 4 * (best size so far): a difflist of L entries takes more than 5 L / 4 bytes (a code quarter
//    and at least one delta or index byte per entry), so a skipped candidate is strictly larger than the best and can
//    neither win nor tie.  The dense size ceil(n / 4) is the first best, so L < n / 5 for every candidate that is
//    sized: at most one of types 4 / 6 / 7, and type 1.  Sizing walks the words again, from LDS.
//  * scan -- one workgroup: the exclusive prefix sum of the lengths, the record offsets of the call and their total.
//  * write -- one wavefront per row again: it recodes the row as the plan kernel does, counts it again for L and the
//    pair of a type 1 record, and writes the record at its offset.  Records start at any byte, so everything but the
//    whole words of a 4-byte aligned dense record is stored byte by byte, and every store is checked against the
//    record's planned length: a disagreement between the two kernels could shorten a record, never leave it.
//
// The difflist (size_or_write_difflist, shared by both kernels, so that they cannot disagree): a step takes 1 024
// samples; the lanes' entries are ranked by a wave prefix sum of their popcounts and compacted, index and code, into
// an LDS buffer behind what the step before left.  Every full 64 entries of the buffer are one group of the list:
// lane j holds entry j, the delta to entry j - 1 is a varint of 1 .. 5 bytes, a wave prefix sum of those lengths
// gives every delta's byte and the group's size, the first entry's index goes to the group's slot of the index
// array, the size to the byte array behind it (positions known from L alone, the values only now), and the 64 codes
// to 16 bytes, put together from two ballots.  What is left (fewer than 64 entries) moves to the buffer's front; the
// last group is flushed after the last step.
//
// Rows wider than the tile (more than 16 384 samples): the words behind the tile are not kept -- every later pass
// loads and recodes them again from the block, which the first pass left in L2.  Slower per sample, same bytes.
// LDS: 9.5 KiB per plan wavefront, 5.5 KiB per write wavefront.  Grids are capped at 16 wavefronts per CU; beyond,
// rows are taken in a grid stride.  Registers, LDS, occupancy and scratch (0 bytes): DESIGN_INGEST.md.

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
constexpr int kScanBlock = 1024;

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
// are barriers of that one wavefront.
template <bool WRITE>
__device__ uint32_t size_or_write_difflist(const EncodeArgs& a, const RowView& v, uint32_t kind, uint32_t lo, uint32_t hi, uint32_t L,
                                           uint8_t* rec, uint32_t room, uint32_t at, uint32_t* ent_idx, uint8_t* ent_code) {
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

__global__ __launch_bounds__(kWave) void pgen_plan_kernel(EncodeArgs a) {
  __shared__ uint32_t tile[kTileWords];
  __shared__ uint32_t ent_idx[kEntCap];
  __shared__ uint8_t ent_code[kEntCap];
  const int lane = threadIdx.x;
  for (int64_t row = blockIdx.x; row < a.n_rows; row += gridDim.x) {
    const int64_t row_at = row * a.n;
    uint32_t count[4];
    int32_t st;
    count_row(a, row_at, tile, count, &st);
    __syncthreads();
    uint32_t lo, hi;
    pgen_onebit_pair(count, &lo, &hi);
    const RowView view{row_at, tile};
    uint32_t best = a.row_bytes, best_kind = 0;
#pragma unroll 1
    for (int c = 0; c < 4; ++c) {  // ascending types: a tie stays with the lower
      const uint32_t kind = c == 0 ? 1u : c == 1 ? 4u : c == 2 ? 6u : 7u;
      const uint32_t L = entries_of(a.n, count, kind, lo, hi);
      if (5ull * L >= 4ull * best) continue;  // more than 5 L / 4 bytes: larger than the best
      uint32_t size = size_or_write_difflist<false>(a, view, kind, lo, hi, L, nullptr, 0u, 0u, ent_idx, ent_code);
      if (kind == 1) size += 1u + (a.n + 7u) / 8u;  // n < 5 * 2^29 / 4 here: no overflow
      if (size < best) {
        best = size;
        best_kind = kind;
      }
    }
    if (lane == 0) {
      a.vrtype[row] = static_cast<uint8_t>(best_kind);
      a.length[row] = best;
      a.status[row] = st;
    }
    __syncthreads();  // the next row overwrites the tile
  }
}

// offsets[r] = length[0] + .. + length[r - 1], offsets[n_rows] = their total (less than 2^32: the entry point checked
// the dense bound): one workgroup, a chunk of its size at a time.
__global__ __launch_bounds__(kScanBlock) void pgen_scan_kernel(const uint32_t* length, int64_t n_rows, uint32_t* offsets) {
  __shared__ uint32_t wave_total[kScanBlock / kWave];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  uint32_t carry = 0;
  for (int64_t r0 = 0; r0 < n_rows; r0 += kScanBlock) {
    const int64_t r = r0 + tid;
    const uint32_t v = r < n_rows ? length[r] : 0u;
    const uint32_t incl = wave_inclusive_sum(v, lane);
    if (lane == kWave - 1) wave_total[wave] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (int k = 0; k < kScanBlock / kWave; ++k) {
      const uint32_t t = wave_total[k];
      if (k < wave) before += t;
      all += t;
    }
    if (r < n_rows) offsets[r] = carry + before + (incl - v);
    carry += all;
    __syncthreads();
  }
  if (tid == 0) offsets[n_rows] = carry;
}

__global__ __launch_bounds__(kWave) void pgen_write_kernel(EncodeArgs a) {
  __shared__ uint32_t ent_idx[kEntCap];
  __shared__ uint8_t ent_code[kEntCap];
  const int lane = threadIdx.x;
  for (int64_t row = blockIdx.x; row < a.n_rows; row += gridDim.x) {
    const int64_t row_at = row * a.n;
    const uint32_t kind = a.vrtype[row], room = a.length[row];
    uint8_t* rec = a.out + a.offsets[row];
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
      continue;
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
    const RowView view{row_at, nullptr};
    size_or_write_difflist<true>(a, view, kind, lo, hi, entries_of(a.n, count, kind, lo, hi), rec, room, at, ent_idx, ent_code);
  }
}

}  // namespace

extern "C" int64_t sai_pgen_encode_grid_cap(sai_ctx* ctx) { return ctx ? static_cast<int64_t>(ctx->n_cu) * kWavesPerCu : -1; }

extern "C" int sai_pgen_encode(sai_ctx* ctx, const int8_t* dosage, int64_t n_rows, int32_t n_slots, const int32_t* ploidy_of_slot,
                               int32_t uniform_ploidy, uint8_t* out, uint8_t* vrtype, uint32_t* length, uint32_t* offsets, int32_t* status,
                               int32_t stages, void* stream) {
  if (int rc = enter(ctx)) return rc;
  if (n_rows < 0 || n_slots < 1) return fail(SAI_ERR_ARG, "size out of range: a .pgen record holds 1 to 2^31 - 1 samples");
  if (uniform_ploidy < 0 || uniform_ploidy > 2) return fail(SAI_ERR_ARG, "uniform_ploidy must be 0, 1 or 2");
  if (stages < 1 || stages > SAI_PGEN_ENCODE_ALL) return fail(SAI_ERR_ARG, "stages must be 1 .. 7");
  const int64_t row_bytes = (static_cast<int64_t>(n_slots) + 3) / 4;
  if (n_rows > (int64_t(0xFFFFFFFFll) - 16) / row_bytes) return fail(SAI_ERR_ARG, "size out of range: a call writes less than 4 GiB of records");
  if (!offsets) return fail(SAI_ERR_ARG, "NULL buffer");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (n_rows == 0) {
    SAI_HIP(hipMemsetAsync(offsets, 0, sizeof(uint32_t), st));
    return SAI_OK;
  }
  if (!dosage || !out || !vrtype || !length || !status || (uniform_ploidy == 0 && !ploidy_of_slot)) return fail(SAI_ERR_ARG, "NULL buffer");
  if (reinterpret_cast<uintptr_t>(dosage) & 15u) return fail(SAI_ERR_ARG, "dosage must be 16-byte aligned");
  EncodeArgs a;
  a.in = reinterpret_cast<const uint8_t*>(dosage);
  a.in_bytes = n_rows * n_slots;
  a.n_rows = n_rows;
  a.n = static_cast<uint32_t>(n_slots);
  a.n_words = (a.n + 15u) / 16u;
  a.row_bytes = static_cast<uint32_t>(row_bytes);
  a.ploidy_of_slot = ploidy_of_slot;
  a.uniform_ploidy = uniform_ploidy;
  a.out = out;
  a.vrtype = vrtype;
  a.length = length;
  a.offsets = offsets;
  a.status = status;
  // a wavefront per row; beyond the 16 per CU rows are taken in a grid stride
  const int64_t cap = sai_pgen_encode_grid_cap(ctx);
  const dim3 grid(static_cast<unsigned>(n_rows < cap ? n_rows : cap));
  if (stages & SAI_PGEN_ENCODE_PLAN) {
    hipLaunchKernelGGL(pgen_plan_kernel, grid, dim3(kWave), 0, st, a);
    if (int rc = check_launch("pgen_plan")) return rc;
  }
  if (stages & SAI_PGEN_ENCODE_SCAN) {
    hipLaunchKernelGGL(pgen_scan_kernel, dim3(1), dim3(kScanBlock), 0, st, static_cast<const uint32_t*>(length), n_rows, offsets);
    if (int rc = check_launch("pgen_scan")) return rc;
  }
  if (stages & SAI_PGEN_ENCODE_WRITE) {
    hipLaunchKernelGGL(pgen_write_kernel, grid, dim3(kWave), 0, st, a);
    if (int rc = check_launch("pgen_write")) return rc;
  }
  return SAI_OK;
}
