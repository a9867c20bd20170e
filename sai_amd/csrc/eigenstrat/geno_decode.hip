// sai_eigenstrat_decode: variant-major .geno records in HBM (PACKEDANCESTRYMAP records, or the lines of a text
// EIGENSTRAT file) -> int8 dosages [row][slot], the block sai_tokenize_gt writes for VCF text.
//
// The contract and the shape are those of sai_plink_decode (plink/bed_decode.hip): the [row][slot] block is
// one flat byte array, every lane owns 16 consecutive, 16-byte aligned bytes of it and stores them as one
// 128-bit word; a call writes the rows [out_row0, out_row0 + n_out_rows) only, so its first and its last
// chunk, which may hold bytes of other rows, are stored byte by byte.
//  * fast path -- the slots are a run of consecutive .ind lines at one ploidy and the lane's 16 slots lie in
//    one row: the lane fetches its 16 codes as one word, code k in bits [2k, 2k + 2), and recodes it;
//  * general path -- any col_of_slot, per-slot ploidies, and the lanes whose 16 bytes cross a row boundary.
// One kernel template serves both encodings; its parameter says how a code is fetched:
//  * PackedFetch -- four individuals per byte, THE FIRST IN THE TWO MOST SIGNIFICANT BITS.  The 16 codes of a
//    lane are 32 consecutive bits of the record in that order: the five bytes that hold them are assembled
//    big-endian, shifted to the lane's first code, and one bit reversal plus one swap of neighbouring bits
//    turns the word into the least-significant-first form the recode reads (not 16 separate extracts);
//  * TextFetch -- one character per individual; a character outside 0 1 2 9 has the code kGenoBadCode, is
//    written as 0 and raises SAI_EIGENSTRAT_STATUS_BAD_CHAR.
// The recode table of a (ploidy, flipped) pair is one register of four packed bytes selected by shifts
// (eigenstrat_codes.hpp), so no branch depends on a genotype code.  status[row] is zeroed by the entry point
// and raised with atomicMax only by the rare lane that has something to report; every index is checked
// before it is used, nothing is read out of bounds.

#include "../common.hpp"
#include "eigenstrat_codes.hpp"
#include "saihip_eigenstrat.h"

namespace {

struct GenoArgs {
  const uint8_t* records;
  int64_t n_batch_records;
  int64_t record_bytes;
  const int32_t* row_in_batch;
  const uint8_t* row_flip;
  int32_t n_cols;
  int32_t n_slots;
  const int32_t* col_of_slot;
  int32_t first_col;  // >= 0: col_of_slot[s] == first_col + s
  const int32_t* ploidy_of_slot;
  int32_t uniform_ploidy;  // 1 or 2: every slot; 0: ploidy_of_slot
  int8_t* out;
  int32_t* status;
  int64_t e_begin, e_end;  // the call's bytes of the flat block: [out_row0 * n_slots, (out_row0 + n_out_rows) * n_slots)
  int64_t chunk0;          // e_begin / 16
  int64_t n_chunks;        // aligned 16-byte chunks that hold a byte of the call
};

constexpr int kGenoBlock = 256;

__device__ __forceinline__ uint32_t lut_for(int32_t ploidy, bool flip) {
  const uint32_t two = flip ? kGenoLutP2Flip : kGenoLutP2;
  const uint32_t one = flip ? kGenoLutP1Flip : kGenoLutP1;
  return ploidy == 2 ? two : one;
}

struct PackedFetch {
  // the code of column `col` of the record at `src`
  static __device__ __forceinline__ uint32_t one(const uint8_t* src, int32_t col) {
    return (static_cast<uint32_t>(src[col >> 2]) >> (6 - 2 * (col & 3))) & 3u;
  }
  // the codes of columns col .. col + 15, code k in bits [2k, 2k + 2); *bad = bit 2k set where code k is no code
  static __device__ __forceinline__ uint32_t sixteen(const uint8_t* src, int64_t record_bytes, int32_t col, uint32_t* bad) {
    const int64_t b0 = col >> 2;
    uint64_t bits = 0;  // big-endian: the first code of byte b0 in bits 39:38
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const uint64_t byte = b0 + k < record_bytes ? src[b0 + k] : 0;
      bits |= byte << (8 * (4 - k));
    }
    const uint32_t msb_first = static_cast<uint32_t>((bits << (2 * (col & 3))) >> 8);  // code k in bits [30 - 2k, 32 - 2k)
    const uint32_t rev = __brev(msb_first);  // code k in bits [2k, 2k + 2), its two bits swapped
    *bad = 0u;
    return ((rev >> 1) & 0x55555555u) | ((rev & 0x55555555u) << 1);
  }
};

struct TextFetch {
  static __device__ __forceinline__ uint32_t one(const uint8_t* src, int32_t col) { return geno_code_of_char(src[col]); }
  static __device__ __forceinline__ uint32_t sixteen(const uint8_t* src, int64_t record_bytes, int32_t col, uint32_t* bad) {
    uint32_t codes = 0, flagged = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const uint32_t c = col + k < record_bytes ? geno_code_of_char(src[col + k]) : kGenoBadCode;
      flagged |= (c >> 2) << (2 * k);
      codes |= (c & 3u) << (2 * k);
    }
    *bad = flagged;
    return codes;
  }
};

struct RowState {
  const uint8_t* src;
  bool ok;
  bool flip;
};

__device__ __forceinline__ RowState load_row(const GenoArgs& a, int64_t row) {
  RowState r;
  const int64_t rib = a.row_in_batch[row];
  r.ok = rib >= 0 && rib < a.n_batch_records;
  r.src = a.records + (r.ok ? rib : 0) * a.record_bytes;
  r.flip = a.row_flip[row] != 0;
  return r;
}

// the output byte of (row, slot) on the general path
template <typename Fetch>
__device__ __forceinline__ uint32_t decode_cell(const GenoArgs& a, const RowState& r, int64_t row, int32_t slot) {
  const int32_t col = a.first_col >= 0 ? a.first_col + slot : a.col_of_slot[slot];
  const int32_t pl = a.uniform_ploidy ? a.uniform_ploidy : a.ploidy_of_slot[slot];
  const bool valid = r.ok && col >= 0 && col < a.n_cols && (pl == 1 || pl == 2);
  if (!valid) {
    atomicMax(a.status + row, kGenoBadIndex);
    return 0u;
  }
  const uint32_t code = Fetch::one(r.src, col);
  if (code == kGenoBadCode) {
    atomicMax(a.status + row, kGenoBadChar);
    return 0u;
  }
  if (pl == 1 && code == kGenoHet) atomicMax(a.status + row, a.n_slots - slot);
  return (lut_for(pl, r.flip) >> (8 * code)) & 0xFFu;
}

template <typename Fetch>
__global__ __launch_bounds__(kGenoBlock) void geno_decode_kernel(GenoArgs a) {
  const bool fast = a.first_col >= 0 && a.uniform_ploidy != 0;
  const bool narrow = a.e_end - a.e_begin <= 0xFFFFFFFFll;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kGenoBlock;
  for (int64_t chunk = static_cast<int64_t>(blockIdx.x) * kGenoBlock + threadIdx.x; chunk < a.n_chunks; chunk += stride) {
    const int64_t e0 = (a.chunk0 + chunk) * 16;
    const int64_t rel = (e0 > a.e_begin ? e0 : a.e_begin) - a.e_begin;  // the lane's first byte, counted from the call's first
    int64_t row;  // of the call: indexes row_in_batch, row_flip and status
    int32_t slot;
    if (narrow) {  // one division per 16 output bytes; 32-bit whenever the call allows it
      const uint32_t q = static_cast<uint32_t>(rel) / static_cast<uint32_t>(a.n_slots);
      row = q;
      slot = static_cast<int32_t>(static_cast<uint32_t>(rel) - q * static_cast<uint32_t>(a.n_slots));
    } else {
      row = rel / a.n_slots;
      slot = static_cast<int32_t>(rel - row * a.n_slots);
    }
    RowState r = load_row(a, row);
    u32x4 word = {0u, 0u, 0u, 0u};
    if (fast && e0 >= a.e_begin && slot + 16 <= a.n_slots) {
      uint32_t codes = 0, bad = 0;
      if (r.ok) codes = Fetch::sixteen(r.src, a.record_bytes, a.first_col + slot, &bad);
      else atomicMax(a.status + row, kGenoBadIndex);
      if (bad) atomicMax(a.status + row, kGenoBadChar);
      const uint32_t lut = lut_for(a.uniform_ploidy, r.flip);
      if (a.uniform_ploidy == 1) {
        const uint32_t het = codes & ~(codes >> 1) & ~bad & 0x55555555u;  // bit 2k set: code k is 01
        if (het && r.ok) atomicMax(a.status + row, a.n_slots - (slot + (__builtin_ctz(het) >> 1)));
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        uint32_t w = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const uint32_t code = (codes >> (2 * (4 * j + k))) & 3u;
          const uint32_t byte = (lut >> (8 * code)) & 0xFFu;
          const uint32_t is_bad = (bad >> (2 * (4 * j + k))) & 1u;
          w |= (byte & (is_bad - 1u)) << (8 * k);
        }
        word[j] = r.ok ? w : 0u;
      }
      *reinterpret_cast<u32x4*>(a.out + e0) = word;
      continue;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      uint32_t w = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int64_t e = e0 + 4 * j + k;
        if (e >= a.e_begin && e < a.e_end) {
          w |= decode_cell<Fetch>(a, r, row, slot) << (8 * k);
          if (++slot == a.n_slots) {
            slot = 0;
            ++row;
            if (e + 1 < a.e_end) r = load_row(a, row);
          }
        }
      }
      word[j] = w;
    }
    if (e0 >= a.e_begin && e0 + 16 <= a.e_end) {
      *reinterpret_cast<u32x4*>(a.out + e0) = word;
    } else {  // the first or the last chunk of the call, shared with bytes that are not its own
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int64_t e = e0 + 4 * j + k;
          if (e >= a.e_begin && e < a.e_end) a.out[e] = static_cast<int8_t>((word[j] >> (8 * k)) & 0xFFu);
        }
    }
  }
}

}  // namespace

extern "C" int sai_eigenstrat_decode(sai_ctx* ctx, int32_t encoding, const uint8_t* records, int64_t n_batch_records, int64_t record_bytes,
                                     int64_t n_out_rows, const int32_t* row_in_batch, const uint8_t* row_flip, int32_t n_cols,
                                     int32_t n_slots, const int32_t* col_of_slot, int32_t first_col, const int32_t* ploidy_of_slot,
                                     int32_t uniform_ploidy, int8_t* out, int64_t out_row0, int32_t* status, void* stream) {
  if (int rc = enter(ctx)) return rc;
  if (encoding != SAI_EIGENSTRAT_TEXT && encoding != SAI_EIGENSTRAT_PACKED) return fail(SAI_ERR_ARG, "encoding must be text or packed: the transposed one has a kernel of its own");
  const bool text = encoding == SAI_EIGENSTRAT_TEXT;
  if (n_batch_records < 0 || record_bytes < 0 || n_out_rows < 0 || n_cols < 0 || n_slots < 1 || out_row0 < 0) return fail(SAI_ERR_ARG, "size out of range");
  if (record_bytes > (int64_t(1) << 60) || static_cast<int64_t>(n_cols) > (text ? record_bytes : 4 * record_bytes)) return fail(SAI_ERR_ARG, "n_cols exceeds the genotypes of a record");
  if (uniform_ploidy < 0 || uniform_ploidy > 2) return fail(SAI_ERR_ARG, "uniform_ploidy must be 0, 1 or 2");
  if (first_col >= 0 && static_cast<int64_t>(first_col) + n_slots > n_cols) return fail(SAI_ERR_ARG, "first_col + n_slots exceeds n_cols");
  if (n_out_rows == 0) return SAI_OK;
  if (!row_in_batch || !row_flip || !out || !status || (first_col < 0 && !col_of_slot) || (uniform_ploidy == 0 && !ploidy_of_slot) ||
      (n_batch_records > 0 && record_bytes > 0 && !records))
    return fail(SAI_ERR_ARG, "NULL buffer");
  if (reinterpret_cast<uintptr_t>(out) & 15u) return fail(SAI_ERR_ARG, "out must be 16-byte aligned");
  if (out_row0 + n_out_rows > (std::numeric_limits<int64_t>::max() - 16) / n_slots) return fail(SAI_ERR_ARG, "size out of range");
  GenoArgs a;
  a.records = records;
  a.n_batch_records = n_batch_records;
  a.record_bytes = record_bytes;
  a.row_in_batch = row_in_batch;
  a.row_flip = row_flip;
  a.n_cols = n_cols;
  a.n_slots = n_slots;
  a.col_of_slot = col_of_slot;
  a.first_col = first_col < 0 ? -1 : first_col;
  a.ploidy_of_slot = ploidy_of_slot;
  a.uniform_ploidy = uniform_ploidy;
  a.out = out;
  a.status = status;
  a.e_begin = out_row0 * n_slots;
  a.e_end = (out_row0 + n_out_rows) * n_slots;
  a.chunk0 = a.e_begin / 16;
  a.n_chunks = (a.e_end + 15) / 16 - a.chunk0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  SAI_HIP(hipMemsetAsync(status, 0, static_cast<size_t>(n_out_rows) * sizeof(int32_t), st));
  // a memory-bound pass: enough workgroups to fill the chip, grid-stride beyond that
  const int64_t want = (a.n_chunks + kGenoBlock - 1) / kGenoBlock;
  const int64_t cap = static_cast<int64_t>(ctx->n_cu) * 16;  // past this cap: tests/test_grid_stride_device.py
  const dim3 grid(static_cast<unsigned>(want < cap ? want : cap));
  if (text) hipLaunchKernelGGL(geno_decode_kernel<TextFetch>, grid, dim3(kGenoBlock), 0, st, a);
  else hipLaunchKernelGGL(geno_decode_kernel<PackedFetch>, grid, dim3(kGenoBlock), 0, st, a);
  return check_launch("geno_decode");
}
