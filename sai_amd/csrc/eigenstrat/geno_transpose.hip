// sai_eigenstrat_decode_transposed: a batch of a transposed packed .geno ("TGENO": one record per individual,
// four variants per byte, the first in the two most significant bits) -> int8 dosages [variant][slot].
//
// The input is contiguous along the variant axis and the output along the slot axis, so the 2-bit matrix has
// to be turned.  A workgroup of 256 lanes takes a tile of 256 output rows x 64 slots and turns it in LDS:
//  * load -- the variants of 256 consecutive rows lie in one or a few 64-byte segments of an individual's
//    staged record (one when every variant of the batch is selected).  Per segment, four lanes read the 64
//    bytes of one individual as 4 x 128 bits, a wave reads 16 such segments, and the words go to LDS as they
//    are: one LDS row of 16 dwords per slot;
//  * store -- as in the variant-major kernels the [row][slot] block is taken flat and a lane owns 16
//    consecutive, 16-byte ALIGNED bytes of it, so four neighbouring lanes store one aligned 64-byte segment
//    of an output row and a wave 16 of them.  A row starts at any byte of the flat block (n_slots need not be
//    a multiple of 16), so the tile's slot window is shifted per row by the row's phase (rowbase mod 16):
//    slot tile j of a row with phase A holds the slots [64 j - A, 64 j + 64 - A), and LDS holds the 80 slots
//    [64 j - 16, 64 j + 64) that the 16 phases need.  Only the chunks at the two ends of a row are partial;
//    they are stored byte by byte, and nothing outside the call's rows is written;
//  * the turn -- for each of its 16 slots a lane reads the dword of that slot's LDS row which holds its
//    variant, shifts the code out and recodes it through the packed-byte register of (ploidy of the slot,
//    flip of the row): no branch depends on a code.
// LDS banks (32 banks of 4 bytes for 32-bit accesses, served per half-wave): dword w of LDS row l is kept at
// position w ^ 4 * ((l >> 4) & 3) ^ ((l >> 1) & 3) of the row.  On the store side the 8 rows x 4 lanes of a
// half-wave read rows l, l + 16, l + 32, l + 48 at one or two neighbouring w (rows of one phase: n_slots a
// multiple of 16, or 16 rows apart otherwise): the first term sends the four to four different quarters of
// the banks, and lanes of the same row group read the same address (a broadcast).  On the load side a
// half-wave writes dword i of 8 consecutive rows x 4 sixteen-byte pieces: the row parity picks the half of the
// banks, the piece the quarter of it and the second term the bank, 32 different ones.  Rows of different
// phase (n_slots not a multiple of 16) can meet on a bank two at a time.
// The selected variants of a batch may be sparse (the ancestral-allele filter) and in any order: the
// workgroup walks the 64-byte segments from the lowest to the highest one its rows need and a row is
// produced in the pass that holds its byte.  Every index is checked before it is used.

#include <climits>

#include "../common.hpp"
#include "eigenstrat_codes.hpp"
#include "saihip_eigenstrat.h"

namespace {

struct TransposeArgs {
  const uint8_t* staged;
  int32_t n_staged;
  int64_t record_stride;
  int32_t first_code;
  int64_t n_batch_variants;
  int64_t n_out_rows;
  const int32_t* row_in_batch;
  const uint8_t* row_flip;
  int32_t n_slots;
  const int32_t* col_of_slot;
  const int32_t* ploidy_of_slot;
  int8_t* out;
  int64_t out_row0;
  int32_t* status;
};

constexpr int kTileRows = 256;
constexpr int kTileSlots = 64;
constexpr int kLdsSlots = kTileSlots + 16;  // the slot windows of all 16 row phases
constexpr int kSegment = 64;                // bytes of a staged record per pass
constexpr int kTransposeBlock = 256;
constexpr int kNoRow = -2, kBadRow = -1;

__device__ __forceinline__ int lds_word(int l, int w) { return l * 16 + (w ^ (4 * ((l >> 4) & 3)) ^ ((l >> 1) & 3)); }

struct Tile {
  uint32_t in[kLdsSlots * 16];
  int32_t col[kLdsSlots];    // the staged individual of an LDS row; -1: no such slot, or an index out of range
  uint8_t ploidy[kLdsSlots];  // 1 or 2; 0: out of range
  int32_t byte_of_row[kTileRows];  // the byte of a staged record that holds the row's variant; kBadRow; kNoRow
  uint8_t shift_of_row[kTileRows];
  uint8_t flip_of_row[kTileRows];
  int32_t lowest, highest;  // over byte_of_row
};

// the 16 output bytes of (row `rl` of the tile, chunk q of the row's slot window); `seg` = the staged bytes LDS holds
__device__ __forceinline__ void emit(const TransposeArgs& a, const Tile& t, int rl, int q, int seg) {
  const int64_t row = static_cast<int64_t>(blockIdx.x) * kTileRows + rl;
  const int64_t rowbase = (a.out_row0 + row) * a.n_slots;
  const int phase = static_cast<int>(rowbase & 15);
  const int64_t slot_lo = static_cast<int64_t>(blockIdx.y) * kTileSlots + 16 * q - phase;
  if (slot_lo >= a.n_slots || slot_lo + 16 <= 0) return;
  const int l0 = 16 * q + 16 - phase;  // the LDS row of slot_lo: 1 .. 64
  const int byte = t.byte_of_row[rl];
  const bool row_ok = byte >= 0;
  const int w = row_ok ? (byte - seg) >> 2 : 0;
  const int shift = row_ok ? 8 * ((byte - seg) & 3) + t.shift_of_row[rl] : 0;
  const bool flip = t.flip_of_row[rl] != 0;
  const uint32_t two = flip ? kGenoLutP2Flip : kGenoLutP2;
  const uint32_t one = flip ? kGenoLutP1Flip : kGenoLutP1;
  u32x4 word = {0u, 0u, 0u, 0u};
  bool bad = false;
  int het_slot = INT_MAX;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    uint32_t packed = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = 4 * j + k;
      const int64_t slot = slot_lo + i;
      const bool inside = slot >= 0 && slot < a.n_slots;
      const uint32_t pl = t.ploidy[l0 + i];
      const bool valid = inside && row_ok && (pl == 1u || pl == 2u) && t.col[l0 + i] >= 0;
      const uint32_t code = (t.in[lds_word(l0 + i, w)] >> shift) & 3u;
      const uint32_t lut = pl == 2u ? two : one;
      packed |= (valid ? (lut >> (8 * code)) & 0xFFu : 0u) << (8 * k);
      bad |= inside && !valid;
      if (valid && pl == 1u && code == kGenoHet && static_cast<int>(slot) < het_slot) het_slot = static_cast<int>(slot);
    }
    word[j] = packed;
  }
  if (bad) atomicMax(a.status + row, kGenoBadIndex);
  else if (het_slot != INT_MAX) atomicMax(a.status + row, a.n_slots - het_slot);
  const int64_t e0 = rowbase + slot_lo;  // a multiple of 16
  if (slot_lo >= 0 && slot_lo + 16 <= a.n_slots) {
    *reinterpret_cast<u32x4*>(a.out + e0) = word;
  } else {  // the first or the last chunk of the row, shared with bytes of its neighbours
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int64_t slot = slot_lo + 4 * j + k;
        if (slot >= 0 && slot < a.n_slots) a.out[e0 + 4 * j + k] = static_cast<int8_t>((word[j] >> (8 * k)) & 0xFFu);
      }
  }
}

__global__ __launch_bounds__(kTransposeBlock) void geno_transpose_kernel(TransposeArgs a) {
  __shared__ Tile t;
  const int tid = threadIdx.x;
  const int64_t slot_base = static_cast<int64_t>(blockIdx.y) * kTileSlots - 16;  // the slot of LDS row 0
  if (tid == 0) {
    t.lowest = INT_MAX;
    t.highest = -1;
  }
  if (tid < kLdsSlots) {
    const int64_t slot = slot_base + tid;
    int32_t col = -1;
    uint32_t pl = 0;
    if (slot >= 0 && slot < a.n_slots) {
      col = a.col_of_slot[slot];
      pl = static_cast<uint32_t>(a.ploidy_of_slot[slot]);
      if (col < 0 || col >= a.n_staged) col = -1;
      if (pl != 1u && pl != 2u) pl = 0;
    }
    t.col[tid] = col;
    t.ploidy[tid] = static_cast<uint8_t>(pl);
  }
  __syncthreads();
  {
    const int64_t row = static_cast<int64_t>(blockIdx.x) * kTileRows + tid;
    int32_t byte = kNoRow;
    if (row < a.n_out_rows) {
      const int64_t rib = a.row_in_batch[row];
      byte = kBadRow;
      if (rib >= 0 && rib < a.n_batch_variants) {
        const int64_t code_at = a.first_code + rib;  // < 2^31 + 3
        byte = static_cast<int32_t>(code_at >> 2);
        t.shift_of_row[tid] = static_cast<uint8_t>(6 - 2 * (code_at & 3));
        atomicMin(&t.lowest, byte);
        atomicMax(&t.highest, byte);
      }
      t.flip_of_row[tid] = a.row_flip[row];
    }
    t.byte_of_row[tid] = byte;
  }
  __syncthreads();
#pragma unroll 1
  for (int k = 0; k < 4; ++k) {  // rows whose index is out of range: zeros and a flag, no pass needed
    const int item = tid + kTransposeBlock * k;
    if (t.byte_of_row[item >> 2] == kBadRow) emit(a, t, item >> 2, item & 3, 0);
  }
  const int highest = t.highest;
  for (int seg = t.lowest & ~(kSegment - 1); seg <= highest; seg += kSegment) {
    for (int piece = tid; piece < kLdsSlots * 4; piece += kTransposeBlock) {
      const int l = piece >> 2, c = piece & 3;
      const int32_t col = t.col[l];
      const int64_t at = static_cast<int64_t>(seg) + 16 * c;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (col >= 0 && at + 16 <= a.record_stride) v = *reinterpret_cast<const u32x4*>(a.staged + col * a.record_stride + at);
#pragma unroll
      for (int i = 0; i < 4; ++i) t.in[lds_word(l, 4 * c + i)] = v[i];
    }
    __syncthreads();
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {
      const int item = tid + kTransposeBlock * k;
      const int byte = t.byte_of_row[item >> 2];
      if (byte >= seg && byte < seg + kSegment) emit(a, t, item >> 2, item & 3, seg);
    }
    __syncthreads();
  }
}

}  // namespace

extern "C" int sai_eigenstrat_decode_transposed(sai_ctx* ctx, const uint8_t* staged, int32_t n_staged, int64_t record_stride,
                                                int32_t first_code, int64_t n_batch_variants, int64_t n_out_rows,
                                                const int32_t* row_in_batch, const uint8_t* row_flip, int32_t n_slots,
                                                const int32_t* col_of_slot, const int32_t* ploidy_of_slot, int8_t* out,
                                                int64_t out_row0, int32_t* status, void* stream) {
  if (int rc = enter(ctx)) return rc;
  if (n_staged < 0 || record_stride < 0 || n_batch_variants < 0 || n_batch_variants > 0x7FFFFFFFll || n_out_rows < 0 || n_slots < 1 || out_row0 < 0)
    return fail(SAI_ERR_ARG, "size out of range");
  if (first_code < 0 || first_code > 3) return fail(SAI_ERR_ARG, "first_code must be 0 .. 3");
  if (record_stride & 15) return fail(SAI_ERR_ARG, "record_stride must be a multiple of 16");
  if (record_stride > (int64_t(1) << 40) || first_code + n_batch_variants > 4 * record_stride)
    return fail(SAI_ERR_ARG, "first_code + n_batch_variants exceeds the 4 * record_stride genotypes of a staged record");
  if (n_out_rows == 0) return SAI_OK;
  if (!row_in_batch || !row_flip || !col_of_slot || !ploidy_of_slot || !out || !status || (n_staged > 0 && record_stride > 0 && !staged))
    return fail(SAI_ERR_ARG, "NULL buffer");
  if ((reinterpret_cast<uintptr_t>(out) & 15u) || (reinterpret_cast<uintptr_t>(staged) & 15u)) return fail(SAI_ERR_ARG, "out and staged must be 16-byte aligned");
  if (out_row0 + n_out_rows > (std::numeric_limits<int64_t>::max() - 16) / n_slots) return fail(SAI_ERR_ARG, "size out of range");
  const int64_t row_tiles = (n_out_rows + kTileRows - 1) / kTileRows;
  const int64_t slot_tiles = (static_cast<int64_t>(n_slots) + 15 + kTileSlots - 1) / kTileSlots;  // a row's window starts up to 15 slots early
  if (row_tiles > 0x7FFFFFFFll || slot_tiles > 65535) return fail(SAI_ERR_UNSUPPORTED, "too many rows or slots for one call");
  TransposeArgs a;
  a.staged = staged;
  a.n_staged = n_staged;
  a.record_stride = record_stride;
  a.first_code = first_code;
  a.n_batch_variants = n_batch_variants;
  a.n_out_rows = n_out_rows;
  a.row_in_batch = row_in_batch;
  a.row_flip = row_flip;
  a.n_slots = n_slots;
  a.col_of_slot = col_of_slot;
  a.ploidy_of_slot = ploidy_of_slot;
  a.out = out;
  a.out_row0 = out_row0;
  a.status = status;
  hipStream_t st = static_cast<hipStream_t>(stream);
  SAI_HIP(hipMemsetAsync(status, 0, static_cast<size_t>(n_out_rows) * sizeof(int32_t), st));
  hipLaunchKernelGGL(geno_transpose_kernel, dim3(static_cast<unsigned>(row_tiles), static_cast<unsigned>(slot_tiles)), dim3(kTransposeBlock), 0, st, a);
  return check_launch("geno_transpose");
}
