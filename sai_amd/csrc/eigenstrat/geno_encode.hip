// sai_geno_encode and sai_geno_encode_transposed: int8 dosages [row][slot] in HBM -> the records of a packed ("GENO")
// or a transposed ("TGENO") .geno, the inverses of sai_eigenstrat_decode and sai_eigenstrat_decode_transposed
// (geno_export.hpp has the table and the two layouts).
//
// Packed -- plink/bed_encode.hip with another table, another field order and records of rlen = max(48, ceil(n / 4))
// bytes.  The records, taken as one flat byte array, are cut into aligned 32-bit words and every lane owns one: it
// loads the two aligned 128-bit words that hold the 16 dosages of its word, funnel-shifts them into place, recodes
// four dosages at a time by bit operations on a 32-bit word and stores the word; no branch depends on a sample, no LDS.
//  * wide rows (n > 192): rlen = ceil(n / 4), the geometry of a .bed row.  A word that crosses into the next record
//    finds that record's dosages `pad` bytes earlier, by as many as the last byte has unused fields: one more funnel
//    shift, as in bed_encode.hip.
//  * narrow rows (n <= 192): rlen = 48, a multiple of four, and out is aligned: no word crosses a record.  A byte
//    behind ceil(n / 4) holds no field (its `left` is not positive), so the padding comes out as zeros from the same
//    code, and a word that is all padding loads nothing.
//  A record never has fewer than 48 bytes, so bed_encode's slot-by-slot path for rows of fewer than four bytes has no
//  counterpart here.  Within a byte the first field is the most significant: the four codes, one per byte of a 32-bit
//  word, are gathered by one multiplication (gather4).
//
// Transposed -- a 2-bit transpose.  A workgroup of 256 lanes takes a tile of 256 rows x 64 slots:
//  * load -- a lane owns four neighbouring slots and, in each of four passes, four consecutive rows: per row the 16
//    lanes of a row group load 64 contiguous bytes (a row starts at any byte of the block, so the four dosages are
//    loaded as one dword of alignment 1 where they lie inside the block's bytes, byte by byte at its very end).  The four
//    dwords are recoded (one code per byte) and merged into one dword whose byte k is the OUTPUT byte of slot k for
//    the four rows: c(row 0) << 6 | c(row 1) << 4 | c(row 2) << 2 | c(row 3).  All 16 loads of a lane are issued before the
//    first is used;
//  * the turn -- that dword goes to LDS at [row quad][slot], 64 row quads of 17 dwords (the 17th is padding).  A
//    half-wave writes 2 row quads x 16 consecutive dwords: 32 different banks of the 64;
//  * store -- a lane owns (slot, word w of the 16 output words of the tile): it reads the bytes [4 w + j][slot],
//    j = 0 .. 3; the 16 lanes of a slot read quads 4 w + j, at dword 17 * (4 w + j) + slot / 4 = bank 4 w + 17 j +
//    slot / 4 (mod 64): 16 different banks, and the four slots of a wave share a dword (a broadcast).  The 16 lanes
//    store 64 contiguous bytes of the slot's record; a record starts at any byte (rlen need not be a multiple of
//    four), so the word is stored with alignment 1, and byte by byte where the record ends inside it.
//  Rows behind n_rows give code 0, so the unused bits of a record's last byte and the padding of a narrow record
//  (n_rows <= 192) are written as zeros by the tiles that cover byte 0 .. rlen - 1.  The grid is rows x slots of
//  tiles and is not capped.
// status[row] is raised with atomicMax by the rare lane that meets a value outside the table; the packed entry point
// zeroes it, the transposed one does not (the calls over the slot groups of a block share it; geno_export.hpp).
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): geno_encode_kernel 31 VGPRs,
// geno_encode_transposed_kernel 40 VGPRs and 4 352 bytes of LDS; scratch 0 for both.  Measured: profiles/geno_export.txt.

#include "../common.hpp"
#include "../plink/plink_codes.hpp"
#include "geno_export.hpp"

namespace {

struct EncodeArgs {
  const uint8_t* in;  // the dosages as bytes
  int64_t in_bytes;   // n_rows * n_slots
  int32_t n_slots;
  uint32_t row_bytes;   // rlen
  uint32_t data_bytes;  // ceil(n_slots / 4) <= rlen
  const int32_t* ploidy_of_slot;
  int32_t uniform_ploidy;  // 1 or 2: every slot; 0: ploidy_of_slot
  uint8_t* out;
  uint32_t out_bytes;  // n_rows * rlen
  uint32_t n_words;    // aligned 32-bit words that hold a byte of the records
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

// bits 8k, 8k + 1 of t (k = 0 .. 3) -> bits 6 - 2k, 7 - 2k: the first field in the two most significant bits.  The
// product puts field k at bits 8k + {0, 10, 20, 30}; those forty positions are all different, so nothing carries, and
// bits 24 .. 31 hold fields 3, 2, 1, 0 from the bottom.
__device__ __forceinline__ uint32_t gather4(uint32_t t) { return ((t & 0x03030303u) * 0x40100401u) >> 24; }

// Four dosages (the bytes of w) -> their four codes, code k in bits 8k, 8k + 1; `bad` gets bit 8k set where byte k is
// outside the table.  b0 / b1 are the two low bits of every byte; `small` marks the bytes 0 .. 3 and `neg` the bytes
// -4 .. -1 (the six high bits all 0 / all 1, found without a carry between bytes: they are shifted down first).
template <int PLOIDY>
__device__ __forceinline__ uint32_t codes4(uint32_t w, uint32_t& bad) {
  const uint32_t b0 = w & kOnes, b1 = (w >> 1) & kOnes;
  const uint32_t high = (w >> 2) & 0x3F3F3F3Fu;
  const uint32_t small = ~((high + 0x3F3F3F3Fu) >> 6) & kOnes;
  const uint32_t neg = ~(((high ^ 0x3F3F3F3Fu) + 0x3F3F3F3Fu) >> 6) & kOnes;
  uint32_t lo, hi;
  if (PLOIDY == 2) {
    // 0 -> 10, 1 -> 01, 2 -> 00, -2 (..10) -> 11; anything else 11
    const uint32_t in_table = small & ~(b0 & b1);
    hi = (~in_table | (small & ~b1 & ~b0)) & kOnes;
    lo = (~in_table | (small & ~b1 & b0)) & kOnes;
    bad = ~(in_table | (neg & b1 & ~b0)) & kOnes;
  } else {
    // 0 -> 10, 1 -> 00, -1 (..11) -> 11; anything else 11
    const uint32_t in_table = small & ~b1;
    hi = (~in_table | (in_table & ~b0)) & kOnes;
    lo = ~in_table & kOnes;
    bad = ~(in_table | (neg & b1 & b0)) & kOnes;
  }
  return lo | (hi << 1);
}

// the same for fields of either ploidy: m1 / m2 have bit 8k set where field k is read at ploidy 1 / 2; a field of
// neither is 11 and is not `bad` (its row's status says BAD_INDEX, the caller's business)
__device__ __forceinline__ uint32_t codes4_mixed(uint32_t w, uint32_t m1, uint32_t m2, uint32_t& bad) {
  uint32_t bad1, bad2;
  const uint32_t c1 = codes4<1>(w, bad1), c2 = codes4<2>(w, bad2);
  const uint32_t f1 = m1 | (m1 << 1), f2 = m2 | (m2 << 1);
  bad = (bad1 & m1) | (bad2 & m2);
  return (c1 & f1) | (c2 & f2) | (0x03030303u & ~(f1 | f2));
}

__global__ __launch_bounds__(kEncodeBlock) void geno_encode_kernel(EncodeArgs a) {
  const uint32_t word = blockIdx.x * kEncodeBlock + threadIdx.x;
  if (word >= a.n_words) return;
  const uint32_t o0 = 4u * word;  // the word's first byte of the flat output
  const uint32_t row = o0 / a.row_bytes;
  const uint32_t b = o0 - row * a.row_bytes;
  uint32_t result = 0;
  // A word whose first byte is padding is padding throughout: a narrow record is 48 bytes, a multiple of the word, and
  // a wide one has no padding byte.
  if (b < a.data_bytes) {
    // The word's bytes lie in `row` and, behind its last byte, in row + 1 (a record holds at least 48 bytes, so no
    // further).  Their dosages are consecutive bytes of the input from `at` on -- row + 1 follows `row` there -- but
    // the last byte of a row has `pad` fields without a dosage, so a byte of row + 1 finds its four dosages `pad`
    // bytes earlier than a byte of `row` would.  (Only a wide record is crossed: there data_bytes = row_bytes.)
    const uint32_t pad = 4u * a.data_bytes - static_cast<uint32_t>(a.n_slots);  // 0 .. 3
    const int64_t at = static_cast<int64_t>(row) * a.n_slots + 4 * b;           // < in_bytes
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
    uint32_t bad_here = kNone, bad_next = kNone;  // the lowest slot outside the table, in row and in row + 1
    bool ploidy_here = true, ploidy_next = true;  // every ploidy read for that row was 1 or 2
#pragma unroll
    for (int j = 3; j >= 0; --j) {
      const bool next = b + j >= a.row_bytes;
      const uint32_t bj = next ? b + j - a.row_bytes : b + j;  // the byte of its record
      uint32_t src = in[j];
      if (j > 0 && pad != 0 && next) src = __funnelshift_r(in[j > 0 ? j - 1 : 0], in[j], 32u - 8u * pad);
      // the slots of this byte: four, fewer in a row's last data byte, none in padding or behind the call's last record
      const int32_t left = a.n_slots - static_cast<int32_t>(4u * bj);
      const uint32_t nv = (o0 + j < a.out_bytes && left > 0) ? (left < 4 ? static_cast<uint32_t>(left) : 4u) : 0u;
      uint32_t bad, codes;
      if (a.uniform_ploidy == 2) {
        codes = codes4<2>(src, bad);
      } else if (a.uniform_ploidy == 1) {
        codes = codes4<1>(src, bad);
      } else {
        uint32_t m1 = 0, m2 = 0;  // bit 8k: slot k of the byte has ploidy 1 / 2
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (static_cast<uint32_t>(k) < nv) {  // 4 * bj + k < n_slots
            const int32_t pl = a.ploidy_of_slot[4u * bj + k];
            m1 |= static_cast<uint32_t>(pl == 1) << (8 * k);
            m2 |= static_cast<uint32_t>(pl == 2) << (8 * k);
          }
        codes = codes4_mixed(src, m1, m2, bad);
        const uint32_t asked = nv < 4u ? (1u << (8u * nv)) - 1u : 0xFFFFFFFFu;
        if (~(m1 | m2) & kOnes & asked) {
          if (next) ploidy_next = false;
          else ploidy_here = false;
        }
      }
      if (nv < 4u) {  // the fields without a slot: 0, and no finding
        const uint32_t have = (1u << (8u * nv)) - 1u;
        codes &= have;
        bad &= have;
      }
      result |= gather4(codes) << (8 * j);
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
  }
  if (o0 + 4u <= a.out_bytes) {
    *reinterpret_cast<uint32_t*>(a.out + o0) = result;
  } else {  // the last word of the call: the bytes behind the records are not its own
    for (uint32_t j = 0; o0 + j < a.out_bytes; ++j) a.out[o0 + j] = static_cast<uint8_t>(result >> (8 * j));
  }
}

// ---- transposed ----

struct TransposedArgs {
  const uint8_t* in;
  int64_t in_bytes;  // n_rows * n_slots
  int64_t n_rows;
  int32_t n_slots;
  const int32_t* ploidy_of_slot;
  int32_t uniform_ploidy;
  int32_t slot0, n_out;
  int64_t rlen;  // max(48, ceil(n_rows / 4))
  uint8_t* out;
  int32_t* status;
};

constexpr int kTileRows = 256, kTileSlots = 64, kTileQuads = kTileRows / 4;
constexpr int kQuadPitch = kTileSlots / 4 + 1;  // dwords of an LDS row: 16 of codes and one of padding
constexpr int kTransposedBlock = 256;

__global__ __launch_bounds__(kTransposedBlock) void geno_encode_transposed_kernel(TransposedArgs a) {
  __shared__ uint32_t turned[kTileQuads * kQuadPitch];
  const int tid = threadIdx.x;
  const int64_t row0 = static_cast<int64_t>(blockIdx.x) * kTileRows;
  const int32_t out0 = static_cast<int32_t>(blockIdx.y) * kTileSlots;  // the tile's first record of the call
  {
    const int l = tid & 15, g = tid >> 4;             // the lane's four slots; its row quad of every pass
    const int32_t rec = out0 + 4 * l;                 // record of the call
    const int32_t left = a.n_out - rec;
    const uint32_t nv = left > 0 ? (left < 4 ? static_cast<uint32_t>(left) : 4u) : 0u;
    const uint32_t have = nv < 4u ? (1u << (8u * nv)) - 1u : 0xFFFFFFFFu;
    const int32_t slot = a.slot0 + rec;               // slot + nv <= slot0 + n_out <= n_slots
    uint32_t m1 = 0, m2 = 0;
    if (a.uniform_ploidy == 0) {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (static_cast<uint32_t>(k) < nv) {
          const int32_t pl = a.ploidy_of_slot[slot + k];
          m1 |= static_cast<uint32_t>(pl == 1) << (8 * k);
          m2 |= static_cast<uint32_t>(pl == 2) << (8 * k);
        }
    }
    const bool ploidy_ok = a.uniform_ploidy != 0 || ((~(m1 | m2) & kOnes & have) == 0u);
    uint32_t v[16];
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t row = row0 + 4 * (16 * p + g) + i;
        const int64_t at = row * a.n_slots + slot;
        uint32_t w = 0;
        if (nv != 0u && row < a.n_rows) {
          if (at + 4 <= a.in_bytes) {
            __builtin_memcpy(&w, a.in + at, 4);  // alignment 1: one dword load on gfx950
          } else {
            for (int k = 0; k < 4; ++k)
              if (at + k < a.in_bytes) w |= static_cast<uint32_t>(a.in[at + k]) << (8 * k);
          }
        }
        v[4 * p + i] = w;
      }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int quad = 16 * p + g;
      uint32_t merged = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t row = row0 + 4 * quad + i;
        uint32_t bad, codes;
        if (a.uniform_ploidy == 2) codes = codes4<2>(v[4 * p + i], bad);
        else if (a.uniform_ploidy == 1) codes = codes4<1>(v[4 * p + i], bad);
        else codes = codes4_mixed(v[4 * p + i], m1, m2, bad);
        if (nv == 0u || row >= a.n_rows) {  // no such cell: 0, and no finding
          codes = 0;
          bad = 0;
        } else {
          codes &= have;
          bad &= have;
          if (bad) atomicMax(a.status + row, a.n_slots - (slot + static_cast<int32_t>(__builtin_ctz(bad) >> 3)));
          if (!ploidy_ok) atomicMax(a.status + row, kPlinkBadIndex);
        }
        merged |= codes << (6 - 2 * i);
      }
      turned[quad * kQuadPitch + l] = merged;
    }
  }
  __syncthreads();
  const uint8_t* bytes = reinterpret_cast<const uint8_t*>(turned);
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int w = tid & 15, s = 16 * p + (tid >> 4);  // word of the tile's 64 record bytes; slot of the tile
    const int32_t rec = out0 + s;
    const int64_t at = row0 / 4 + 4 * w;  // byte of the record
    if (rec >= a.n_out || at >= a.rlen) continue;
    uint32_t word = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) word |= static_cast<uint32_t>(bytes[(4 * w + j) * (4 * kQuadPitch) + s]) << (8 * j);
    uint8_t* dst = a.out + rec * a.rlen + at;
    if (at + 4 <= a.rlen) {
      __builtin_memcpy(dst, &word, 4);  // alignment 1: a record starts at any byte
    } else {
      for (int j = 0; at + j < a.rlen; ++j) dst[j] = static_cast<uint8_t>(word >> (8 * j));
    }
  }
}

}  // namespace

extern "C" int sai_geno_encode(sai_ctx* ctx, const int8_t* dosage, int64_t n_rows, int32_t n_slots, const int32_t* ploidy_of_slot,
                               int32_t uniform_ploidy, uint8_t* out, int32_t* status, void* stream) {
  if (int rc = enter(ctx)) return rc;
  if (n_rows < 0 || n_slots < 1) return fail(SAI_ERR_ARG, "size out of range");
  if (uniform_ploidy < 0 || uniform_ploidy > 2) return fail(SAI_ERR_ARG, "uniform_ploidy must be 0, 1 or 2");
  const int64_t data_bytes = (static_cast<int64_t>(n_slots) + 3) / 4;
  const int64_t row_bytes = geno_record_bytes(n_slots);
  if (n_rows > (int64_t(0xFFFFFFFFll) - 16) / row_bytes) return fail(SAI_ERR_ARG, "size out of range: a call writes less than 4 GiB of records");
  if (n_rows == 0) return SAI_OK;
  if (!dosage || !out || !status || (uniform_ploidy == 0 && !ploidy_of_slot)) return fail(SAI_ERR_ARG, "NULL buffer");
  if (reinterpret_cast<uintptr_t>(dosage) & 15u) return fail(SAI_ERR_ARG, "dosage must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(out) & 15u) return fail(SAI_ERR_ARG, "out must be 16-byte aligned");
  EncodeArgs a;
  a.in = reinterpret_cast<const uint8_t*>(dosage);
  a.in_bytes = n_rows * n_slots;
  a.n_slots = n_slots;
  a.row_bytes = static_cast<uint32_t>(row_bytes);
  a.data_bytes = static_cast<uint32_t>(data_bytes);
  a.ploidy_of_slot = ploidy_of_slot;
  a.uniform_ploidy = uniform_ploidy;
  a.out = out;
  a.out_bytes = static_cast<uint32_t>(n_rows * row_bytes);
  a.n_words = (a.out_bytes + 3u) / 4u;
  a.status = status;
  hipStream_t st = static_cast<hipStream_t>(stream);
  SAI_HIP(hipMemsetAsync(status, 0, static_cast<size_t>(n_rows) * sizeof(int32_t), st));
  const unsigned blocks = (a.n_words + kEncodeBlock - 1) / kEncodeBlock;  // at most 2^22
  hipLaunchKernelGGL(geno_encode_kernel, dim3(blocks), dim3(kEncodeBlock), 0, st, a);
  return check_launch("geno_encode");
}

extern "C" int sai_geno_encode_transposed(sai_ctx* ctx, const int8_t* dosage, int64_t n_rows, int32_t n_slots, const int32_t* ploidy_of_slot,
                                          int32_t uniform_ploidy, int32_t slot0, int32_t n_out, uint8_t* out, int32_t* status, void* stream) {
  if (int rc = enter(ctx)) return rc;
  if (n_rows < 0 || n_slots < 1) return fail(SAI_ERR_ARG, "size out of range");
  if (uniform_ploidy < 0 || uniform_ploidy > 2) return fail(SAI_ERR_ARG, "uniform_ploidy must be 0, 1 or 2");
  if (n_rows > (std::numeric_limits<int64_t>::max() - 16) / n_slots) return fail(SAI_ERR_ARG, "size out of range");
  if (slot0 < 0 || n_out < 0 || static_cast<int64_t>(slot0) + n_out > n_slots) return fail(SAI_ERR_ARG, "slot0 + n_out exceeds n_slots");
  const int64_t rlen = geno_record_bytes(n_rows);
  if (n_out > (int64_t(0xFFFFFFFFll) - 16) / rlen) return fail(SAI_ERR_ARG, "size out of range: a call writes less than 4 GiB of records");
  if (n_out == 0) return SAI_OK;
  if ((n_rows > 0 && (!dosage || !status)) || !out || (uniform_ploidy == 0 && !ploidy_of_slot)) return fail(SAI_ERR_ARG, "NULL buffer");
  if (reinterpret_cast<uintptr_t>(dosage) & 15u) return fail(SAI_ERR_ARG, "dosage must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(out) & 15u) return fail(SAI_ERR_ARG, "out must be 16-byte aligned");
  const int64_t row_tiles = (rlen + kTileQuads - 1) / kTileQuads;  // rlen >= ceil(n_rows / 4): every row and every padding byte
  const int64_t slot_tiles = (static_cast<int64_t>(n_out) + kTileSlots - 1) / kTileSlots;
  if (row_tiles > 0x7FFFFFFFll || slot_tiles > 65535) return fail(SAI_ERR_UNSUPPORTED, "too many rows or slots for one call");
  TransposedArgs a;
  a.in = reinterpret_cast<const uint8_t*>(dosage);
  a.in_bytes = n_rows * n_slots;
  a.n_rows = n_rows;
  a.n_slots = n_slots;
  a.ploidy_of_slot = ploidy_of_slot;
  a.uniform_ploidy = uniform_ploidy;
  a.slot0 = slot0;
  a.n_out = n_out;
  a.rlen = rlen;
  a.out = out;
  a.status = status;
  hipLaunchKernelGGL(geno_encode_transposed_kernel, dim3(static_cast<unsigned>(row_tiles), static_cast<unsigned>(slot_tiles)), dim3(kTransposedBlock), 0,
                     static_cast<hipStream_t>(stream), a);
  return check_launch("geno_encode_transposed");
}
