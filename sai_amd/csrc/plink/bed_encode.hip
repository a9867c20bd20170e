// sai_bed_encode: int8 dosages [row][slot] in HBM -> variant-major PLINK 1 .bed rows, the inverse of sai_plink_decode
// (bed_export.hpp has the table).
//
// An element-wise, memory-bound pass: 16 input bytes become 4 output bytes.  The output rows, taken as one flat
// byte array, are cut into aligned 32-bit words and every lane owns one: it loads the 16 dosages of its word and
// stores the word, so a wave stores 256 contiguous bytes.  A row of 2 002 samples is 501 bytes and starts at byte
// 2 002 * r of the input, so neither the word nor its 16 dosages are aligned to the rows:
//  * word path -- rows of at least four bytes: the word's
//    dosages are consecutive bytes of the input that start at any byte of it, so the lane loads the two aligned
//    128-bit words that hold them and funnel-shifts them into place (as bcf/bcf_decode.hip does).  Four dosages are
//    recoded at a time by bit operations on a 32-bit word: no branch depends on a sample, no LDS.  A word that
//    crosses into the next row (two words of 126 at 2 002 samples) stays on this path: its bytes of the next row
//    find their dosages a few bytes earlier, by as many as the row's last byte has unused fields, which is one more
//    funnel shift; the unused fields are masked.  With per-slot ploidies the lane also loads the ploidies of its 16
//    slots (an array every row shares: L2) and takes, field by field, the recoding its slot asks for.  One trip to memory for every lane of a wave: the pass is bound
//    by the latency of that trip (profiles/bed_export.txt), and a second path for the crossing words, taken by one
//    lane of every other wave, cost a second trip;
//  * slot-by-slot path -- rows of fewer than four bytes (at most 12 samples): one dosage at a time, bed_code_of.
// An aligned 128-bit load never leaves [dosage, dosage + n_rows * n_slots): a word that would is assembled from its
// bytes inside.  Only the last word of the call can hold bytes behind the rows; it is stored byte by byte.
// status[row] is zeroed by the entry point and raised with atomicMax by the rare lane that meets a value outside
// the table.  The grid is not capped: a lane takes one word, and a call of 4 GiB of rows or more is refused.

#include "../common.hpp"
#include "bed_export.hpp"
#include "plink_codes.hpp"

namespace {

struct EncodeArgs {
  const uint8_t* in;  // the dosages as bytes
  int64_t in_bytes;   // n_rows * n_slots
  int32_t n_slots;
  uint32_t row_bytes;
  const int32_t* ploidy_of_slot;
  int32_t uniform_ploidy;  // 1 or 2: every slot; 0: ploidy_of_slot
  uint8_t* out;
  uint32_t out_bytes;  // n_rows * row_bytes
  uint32_t n_words;    // aligned 32-bit words that hold a byte of the rows
  int32_t* status;
};

constexpr int kEncodeBlock = 256;
constexpr uint32_t kOnes = 0x01010101u;

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
    // 0 -> 11, 1 -> 10, 2 -> 00, -2 (..10) -> 01; anything else 01
    hi = small & ~b1;
    lo = ~(small & (b0 ^ b1)) & kOnes;
    bad = ~((small & ~(b0 & b1)) | (neg & b1 & ~b0)) & kOnes;
  } else {
    // 0 -> 11, 1 -> 00, -1 (..11) -> 01; anything else 01
    hi = small & ~b1 & ~b0;
    lo = ~(small & ~b1 & b0) & kOnes;
    bad = ~((small & ~b1) | (neg & b1 & b0)) & kOnes;
  }
  return gather4(lo | (hi << 1));
}

// one output byte, slot by slot: byte b of `row`
__device__ __forceinline__ uint32_t encode_byte(const EncodeArgs& a, uint32_t row, uint32_t b) {
  const int64_t base = static_cast<int64_t>(row) * a.n_slots;
  uint32_t byte = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int32_t s = static_cast<int32_t>(4 * b) + k;
    if (s < a.n_slots) {
      const int32_t pl = a.uniform_ploidy ? a.uniform_ploidy : a.ploidy_of_slot[s];
      bool fits = false;
      uint32_t code = 1u;
      if (pl == 1 || pl == 2) {
        code = bed_code_of(static_cast<int8_t>(a.in[base + s]), pl, &fits);
        if (!fits) atomicMax(a.status + row, a.n_slots - s);
      } else {
        atomicMax(a.status + row, kPlinkBadIndex);
      }
      byte |= code << (2 * k);
    }
  }
  return byte;
}

__global__ __launch_bounds__(kEncodeBlock) void bed_encode_kernel(EncodeArgs a) {
  const uint32_t word = blockIdx.x * kEncodeBlock + threadIdx.x;
  if (word >= a.n_words) return;
  const uint32_t o0 = 4u * word;  // the word's first byte of the flat output
  const uint32_t row = o0 / a.row_bytes;
  const uint32_t b = o0 - row * a.row_bytes;
  if (a.row_bytes >= 4u) {
    // The word's bytes lie in `row` and, behind its last byte, in row + 1 (a row holds at least four bytes, so no
    // further).  Their dosages are consecutive bytes of the input from `at` on -- row + 1 follows `row` there -- but
    // the last byte of a row has `pad` fields without a dosage, so a byte of row + 1 finds its four dosages `pad`
    // bytes earlier than a byte of `row` would.
    const uint32_t pad = 4u * a.row_bytes - static_cast<uint32_t>(a.n_slots);  // 0 .. 3
    const int64_t at = static_cast<int64_t>(row) * a.n_slots + 4 * b;          // < in_bytes
    const int64_t base = at & ~int64_t(15);
    const uint32_t shift = static_cast<uint32_t>(at & 15);
    const u32x4 v0 = load_word(a, base);
    u32x4 v1 = {0u, 0u, 0u, 0u};
    if (shift) v1 = load_word(a, base + 16);
    const uint32_t w[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
    const uint32_t q = shift >> 2, bits = (shift & 3u) * 8u;
    uint32_t in[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      // words i + q and i + q + 1, picked with selects: q is the lane's own, the indices stay static
      const uint32_t lo = q == 0 ? w[i] : q == 1 ? w[i + 1] : q == 2 ? w[i + 2] : w[i + 3];
      const uint32_t hi = q == 0 ? w[i + 1] : q == 1 ? w[i + 2] : q == 2 ? w[i + 3] : w[i + 4];
      in[i] = __funnelshift_r(lo, hi, bits);
    }
    constexpr uint32_t kNone = 0xFFFFFFFFu;
    uint32_t result = 0, bad_here = kNone, bad_next = kNone;  // the lowest slot outside the table, in row and in row + 1
    bool ploidy_here = true, ploidy_next = true;               // every ploidy read for that row was 1 or 2
#pragma unroll
    for (int j = 3; j >= 0; --j) {
      const bool next = b + j >= a.row_bytes;
      const uint32_t bj = next ? b + j - a.row_bytes : b + j;  // the byte of its row
      uint32_t src = in[j];
      if (j > 0 && pad != 0 && next) src = __funnelshift_r(in[j > 0 ? j - 1 : 0], in[j], 32u - 8u * pad);
      // the slots of this byte: four, fewer in a row's last byte, none behind the call's last row
      const uint32_t left = static_cast<uint32_t>(a.n_slots) - 4u * bj;
      const uint32_t nv = o0 + j < a.out_bytes ? (left < 4u ? left : 4u) : 0u;
      uint32_t bad, codes;
      if (a.uniform_ploidy == 2) {
        codes = encode4<2>(src, bad);
      } else if (a.uniform_ploidy == 1) {
        codes = encode4<1>(src, bad);
      } else {
        // per-slot ploidies: both recodings, and per field the one its slot's ploidy asks for; neither: 01
        uint32_t m1 = 0, m2 = 0;  // bit 8k: slot k of the byte has ploidy 1 / 2
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (static_cast<uint32_t>(k) < nv) {  // 4 * bj + k < n_slots
            const int32_t pl = a.ploidy_of_slot[4u * bj + k];
            m1 |= static_cast<uint32_t>(pl == 1) << (8 * k);
            m2 |= static_cast<uint32_t>(pl == 2) << (8 * k);
          }
        uint32_t bad1, bad2;
        const uint32_t c1 = encode4<1>(src, bad1), c2 = encode4<2>(src, bad2);
        const uint32_t f1 = gather4(m1 | (m1 << 1)), f2 = gather4(m2 | (m2 << 1));
        codes = (c1 & f1) | (c2 & f2) | (0x55u & ~(f1 | f2));
        bad = (bad1 & m1) | (bad2 & m2);
        const uint32_t asked = nv < 4u ? (1u << (8u * nv)) - 1u : 0xFFFFFFFFu;
        if (~(m1 | m2) & kOnes & asked) {
          if (next) ploidy_next = false;
          else ploidy_here = false;
        }
      }
      if (nv < 4u) {
        codes &= (1u << (2u * nv)) - 1u;
        bad &= (1u << (8u * nv)) - 1u;
      }
      result |= codes << (8 * j);
      if (bad) {  // descending j: the lowest stays
        const uint32_t slot = 4u * bj + (static_cast<uint32_t>(__builtin_ctz(bad)) >> 3);
        if (next) bad_next = slot;
        else bad_here = slot;
      }
    }
    if (bad_here != kNone) atomicMax(a.status + row, a.n_slots - static_cast<int32_t>(bad_here));
    if (bad_next != kNone) atomicMax(a.status + row + 1, a.n_slots - static_cast<int32_t>(bad_next));
    if (!ploidy_here) atomicMax(a.status + row, kPlinkBadIndex);
    if (!ploidy_next) atomicMax(a.status + row + 1, kPlinkBadIndex);
    if (o0 + 4u <= a.out_bytes) {
      *reinterpret_cast<uint32_t*>(a.out + o0) = result;
    } else {  // the last word of the call: the bytes behind the rows are not its own
      for (uint32_t j = 0; o0 + j < a.out_bytes; ++j) a.out[o0 + j] = static_cast<uint8_t>(result >> (8 * j));
    }
    return;
  }
  uint32_t result = 0, r = row, at_b = b;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (o0 + j < a.out_bytes) {
      result |= encode_byte(a, r, at_b) << (8 * j);
      if (++at_b == a.row_bytes) {
        at_b = 0;
        ++r;
      }
    }
  }
  if (o0 + 4u <= a.out_bytes) {
    *reinterpret_cast<uint32_t*>(a.out + o0) = result;
  } else {  // the last word of the call: the bytes behind the rows are not its own
    for (uint32_t j = 0; o0 + j < a.out_bytes; ++j) a.out[o0 + j] = static_cast<uint8_t>(result >> (8 * j));
  }
}

}  // namespace

extern "C" int sai_bed_encode(sai_ctx* ctx, const int8_t* dosage, int64_t n_rows, int32_t n_slots, const int32_t* ploidy_of_slot,
                              int32_t uniform_ploidy, uint8_t* out, int32_t* status, void* stream) {
  if (int rc = enter(ctx)) return rc;
  if (n_rows < 0 || n_slots < 1) return fail(SAI_ERR_ARG, "size out of range");
  if (uniform_ploidy < 0 || uniform_ploidy > 2) return fail(SAI_ERR_ARG, "uniform_ploidy must be 0, 1 or 2");
  const int64_t row_bytes = (static_cast<int64_t>(n_slots) + 3) / 4;
  if (n_rows > (int64_t(0xFFFFFFFFll) - 16) / row_bytes) return fail(SAI_ERR_ARG, "size out of range: a call writes less than 4 GiB of rows");
  if (n_rows == 0) return SAI_OK;
  if (!dosage || !out || !status || (uniform_ploidy == 0 && !ploidy_of_slot)) return fail(SAI_ERR_ARG, "NULL buffer");
  if (reinterpret_cast<uintptr_t>(dosage) & 15u) return fail(SAI_ERR_ARG, "dosage must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(out) & 15u) return fail(SAI_ERR_ARG, "out must be 16-byte aligned");
  EncodeArgs a;
  a.in = reinterpret_cast<const uint8_t*>(dosage);
  a.in_bytes = n_rows * n_slots;
  a.n_slots = n_slots;
  a.row_bytes = static_cast<uint32_t>(row_bytes);
  a.ploidy_of_slot = ploidy_of_slot;
  a.uniform_ploidy = uniform_ploidy;
  a.out = out;
  a.out_bytes = static_cast<uint32_t>(n_rows * row_bytes);
  a.n_words = (a.out_bytes + 3u) / 4u;
  a.status = status;
  hipStream_t st = static_cast<hipStream_t>(stream);
  SAI_HIP(hipMemsetAsync(status, 0, static_cast<size_t>(n_rows) * sizeof(int32_t), st));
  const unsigned blocks = (a.n_words + kEncodeBlock - 1) / kEncodeBlock;  // at most 2^22
  hipLaunchKernelGGL(bed_encode_kernel, dim3(blocks), dim3(kEncodeBlock), 0, st, a);
  return check_launch("bed_encode");
}
