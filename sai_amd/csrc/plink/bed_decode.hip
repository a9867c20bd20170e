// sai_plink_decode: variant-major PLINK 1 .bed rows in HBM -> int8 dosages [row][slot], the block
// sai_tokenize_gt writes for VCF text.
//
// The output is four times the input, so the stores are the traffic that counts: the [row][slot] block
// is taken as one flat byte array and every lane owns 16 consecutive, 16-byte aligned bytes of it, stored
// as one 128-bit word (a wave stores 1 KiB contiguously).  A call decodes the rows [out_row0, out_row0 +
// n_out_rows) of the block, so a reader fills one allocation batch by batch; only the call's first and
// last chunk can hold bytes of other rows, and those two are stored byte by byte.  Taking the block flat
// also packs narrow outputs: with two slots a lane covers eight rows, so a two-sample pass over 10^7
// rows is 5 000 workgroups, not 10^7.
//  * fast path -- the slots are a run of consecutive .fam columns at one ploidy (the usual population
//    list; the caller says so) and the lane's 16 slots lie in one row: the lane takes the five input
//    bytes that hold its 16 codes, shifts them into one 32-bit word and recodes it;
//  * general path -- any col_of_slot (permutation, repeats), per-slot ploidies, and the lanes whose 16
//    bytes cross a row boundary: one input byte per output byte.
// A row is 501 bytes at 2 002 samples and each of its bytes is wanted by one lane (fast path) or by a
// few neighbouring lanes, so the re-reads are served by L1 / L2 and the row leaves HBM once; no LDS.
// The recode table of a (ploidy, flipped) pair is one register of four packed bytes selected by shifts
// (plink_codes.hpp), so no branch depends on a genotype code.  status[row] is zeroed by the entry point
// and raised with atomicMax only by the rare lane that meets a heterozygous code at ploidy 1 or an
// index outside its range; every index is checked before it is used, nothing is read out of bounds.

#include "../common.hpp"
#include "plink_codes.hpp"
#include "recode16.hpp"
#include "saihip_plink.h"

namespace {

struct DecodeArgs {
  const uint8_t* rows;
  int64_t n_batch_rows;
  int64_t row_bytes;
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

constexpr int kDecodeBlock = 256;

__device__ __forceinline__ uint32_t lut_for(int32_t ploidy, bool flip) {
  const uint32_t two = flip ? kPlinkLutP2Flip : kPlinkLutP2;
  const uint32_t one = flip ? kPlinkLutP1Flip : kPlinkLutP1;
  return ploidy == 2 ? two : one;
}

struct RowState {
  const uint8_t* src;
  bool ok;
  bool flip;
};

__device__ __forceinline__ RowState load_row(const DecodeArgs& a, int64_t row) {
  RowState r;
  const int64_t rib = a.row_in_batch[row];
  r.ok = rib >= 0 && rib < a.n_batch_rows;
  r.src = a.rows + (r.ok ? rib : 0) * a.row_bytes;
  r.flip = a.row_flip[row] != 0;
  return r;
}

// the output byte of (row, slot) on the general path
__device__ __forceinline__ uint32_t decode_cell(const DecodeArgs& a, const RowState& r, int64_t row, int32_t slot) {
  const int32_t col = a.first_col >= 0 ? a.first_col + slot : a.col_of_slot[slot];
  const int32_t pl = a.uniform_ploidy ? a.uniform_ploidy : a.ploidy_of_slot[slot];
  const bool valid = r.ok && col >= 0 && col < a.n_cols && (pl == 1 || pl == 2);
  if (!valid) {
    atomicMax(a.status + row, kPlinkBadIndex);
    return 0u;
  }
  const uint32_t code = (static_cast<uint32_t>(r.src[col >> 2]) >> (2 * (col & 3))) & 3u;
  if (pl == 1 && code == kPlinkHet) atomicMax(a.status + row, a.n_slots - slot);
  return (lut_for(pl, r.flip) >> (8 * code)) & 0xFFu;
}

__global__ __launch_bounds__(kDecodeBlock) void bed_decode_kernel(DecodeArgs a) {
  const bool fast = a.first_col >= 0 && a.uniform_ploidy != 0;
  const bool narrow = a.e_end - a.e_begin <= 0xFFFFFFFFll;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kDecodeBlock;
  for (int64_t chunk = static_cast<int64_t>(blockIdx.x) * kDecodeBlock + threadIdx.x; chunk < a.n_chunks; chunk += stride) {
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
      // the lane's 16 codes are 32 consecutive bits of the row, starting at bit 2 * col of it
      const int32_t col = a.first_col + slot;
      const int64_t b0 = col >> 2;
      uint64_t bits = 0;
      if (r.ok) {
#pragma unroll
        for (int k = 0; k < 5; ++k) {
          const uint64_t byte = b0 + k < a.row_bytes ? r.src[b0 + k] : 0;
          bits |= byte << (8 * k);
        }
      } else {
        atomicMax(a.status + row, kPlinkBadIndex);
      }
      const uint32_t codes = static_cast<uint32_t>(bits >> (2 * (col & 3)));
      const uint32_t lut = lut_for(a.uniform_ploidy, r.flip);
      if (a.uniform_ploidy == 1) {
        const uint32_t het = (codes >> 1) & ~codes & 0x55555555u;  // bit 2k set: code k is 10
        if (het && r.ok) atomicMax(a.status + row, a.n_slots - (slot + (__builtin_ctz(het) >> 1)));
      }
      SAI_RECODE16(codes, lut, r.ok, word)
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
          w |= decode_cell(a, r, row, slot) << (8 * k);
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

extern "C" int sai_plink_decode(sai_ctx* ctx, const uint8_t* rows, int64_t n_batch_rows, int64_t row_bytes, int64_t n_out_rows,
                                const int32_t* row_in_batch, const uint8_t* row_flip, int32_t n_cols, int32_t n_slots,
                                const int32_t* col_of_slot, int32_t first_col, const int32_t* ploidy_of_slot,
                                int32_t uniform_ploidy, int8_t* out, int64_t out_row0, int32_t* status, void* stream) {
  if (int rc = enter(ctx)) return rc;
  if (n_batch_rows < 0 || row_bytes < 0 || n_out_rows < 0 || n_cols < 0 || n_slots < 1 || out_row0 < 0) return fail(SAI_ERR_ARG, "size out of range");
  if (static_cast<int64_t>(n_cols) > 4 * row_bytes) return fail(SAI_ERR_ARG, "n_cols exceeds the 4 * row_bytes genotypes of a row");
  if (uniform_ploidy < 0 || uniform_ploidy > 2) return fail(SAI_ERR_ARG, "uniform_ploidy must be 0, 1 or 2");
  if (first_col >= 0 && static_cast<int64_t>(first_col) + n_slots > n_cols) return fail(SAI_ERR_ARG, "first_col + n_slots exceeds n_cols");
  if (n_out_rows == 0) return SAI_OK;
  if (!row_in_batch || !row_flip || !out || !status || (first_col < 0 && !col_of_slot) || (uniform_ploidy == 0 && !ploidy_of_slot) ||
      (n_batch_rows > 0 && row_bytes > 0 && !rows))
    return fail(SAI_ERR_ARG, "NULL buffer");
  if (reinterpret_cast<uintptr_t>(out) & 15u) return fail(SAI_ERR_ARG, "out must be 16-byte aligned");
  if (out_row0 + n_out_rows > (std::numeric_limits<int64_t>::max() - 16) / n_slots) return fail(SAI_ERR_ARG, "size out of range");
  DecodeArgs a;
  a.rows = rows;
  a.n_batch_rows = n_batch_rows;
  a.row_bytes = row_bytes;
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
  const int64_t want = (a.n_chunks + kDecodeBlock - 1) / kDecodeBlock;
  const int64_t cap = static_cast<int64_t>(ctx->n_cu) * 16;  // past this cap: tests/test_grid_stride_device.py
  hipLaunchKernelGGL(bed_decode_kernel, dim3(static_cast<unsigned>(want < cap ? want : cap)), dim3(kDecodeBlock), 0, st, a);
  return check_launch("bed_decode");
}
