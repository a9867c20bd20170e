// sai_pgen_decode: the compressed hard-call records of a PLINK 2 .pgen in HBM -> int8 dosages [row][slot], the
// block sai_tokenize_gt writes for VCF text.  The rules of the format are in DESIGN_INGEST.md ("PLINK 2 filesets");
// the plain statement of them is the host decoder (pgen_index.cpp), and this kernel makes the same decisions.
//
// One wavefront (one 64-lane workgroup, as inflate.hip) per output row.  The row is expanded to dense 2-bit codes in
// LDS, a tile of kTileSamples samples at a time, and recoded from there (the expand and difflist steps are shared
// with pgen_pack2.hip and live in pgen_expand.hpp):
//  * expand -- a dense record (type 0) is copied, a one-bit record (type 1) has every lane spread 16 bits to 16 codes,
//    types 4 / 6 / 7 are a constant fill.  A record of type 2 or 3 expands its base first by the same code (a base is
//    never of type 2 or 3: no recursion), type 3 then exchanges the codes 0 and 2 word by word;
//  * difflist -- groups of 64 entries can be entered anywhere: a lane takes a group, finds its delta bytes at the wave
//    prefix sum of the group sizes and walks its own varints.  An entry of the tile lands in the packed row with two LDS
//    atomics on its 32-bit word (clear the field, set it); indices are unique, so entries do not order.  Every lane
//    checks what it reads before it uses it: the span of the record against the batch, L, the group sizes and the
//    varints against the record's end, sample indices against sample_ct and against strict increase (across groups
//    through the neighbour lane), the byte of type 1, type 5.  The first tile walks every group, so whether a row is
//    bad is known before a byte of it is written: a bad row is zeros and SAI_PGEN_STATUS_BAD_RECORD.  Later tiles walk
//    only the groups that can reach into them;
//  * recode -- as bed_decode.hip: the [row][slot] block is one flat byte array, a lane owns 16 consecutive, 16-byte
//    aligned bytes of the row and stores them as one 128-bit word; the fast path (a run of consecutive columns at one
//    ploidy) takes its 16 codes as 32 bits of two LDS words, the general path one code per byte.  The loop nest of the
//    table look-up is shared with that kernel (../plink/recode16.hpp), only the table differs.  Chunks that a row
//    shares with its neighbours (first, last) and, in rows wider than a tile, chunks whose columns lie in several
//    tiles are stored byte by byte, each byte by the tile that holds its column.
// LDS: 4 KiB per wavefront (16 384 samples per tile).  The kernel's 97 VGPRs allow four wavefronts per SIMD, 16
// per CU, which take 64 KiB of the CU's 160 KiB: the registers limit occupancy, LDS does not, and rows up to 16 384
// samples -- every panel this project has been run on -- take one tile.  No scratch.

#include "../common.hpp"
#include "../plink/recode16.hpp"
#include "pgen_codes.hpp"
#include "pgen_expand.hpp"
#include "saihip_pgen.h"

namespace {

struct PgenArgs {
  const uint8_t* bytes;
  int64_t n_bytes;
  int64_t n_out_rows;
  const int64_t* rec;   // [n_out_rows][3]
  const int64_t* base;  // [n_out_rows][3]
  const uint8_t* row_flip;
  uint32_t sample_ct;
  int32_t n_slots;
  const int32_t* col_of_slot;
  int32_t first_col;  // >= 0: col_of_slot[s] == first_col + s
  const int32_t* ploidy_of_slot;
  int32_t uniform_ploidy;  // 1 or 2: every slot; 0: ploidy_of_slot
  int8_t* out;
  int64_t out_row0;
  int32_t* status;
};

__device__ __forceinline__ uint32_t lut_for(int32_t ploidy, bool flip) {
  const uint32_t two = flip ? kPgenLutP2Flip : kPgenLutP2;
  const uint32_t one = flip ? kPgenLutP1Flip : kPgenLutP1;
  return ploidy == 2 ? two : one;
}

__global__ __launch_bounds__(kWave) void pgen_decode_kernel(PgenArgs a) {
  __shared__ uint32_t tile[kTileWords];
  const int lane = threadIdx.x;
  const uint32_t n = a.sample_ct;
  const bool fast = a.first_col >= 0 && a.uniform_ploidy != 0;
  const u32x4 zero = {0u, 0u, 0u, 0u};
  for (int64_t row = blockIdx.x; row < a.n_out_rows; row += gridDim.x) {
    const Record own = load_record(a, a.rec + 3 * row);
    const bool derived = own.kind == 2 || own.kind == 3;
    Record from = own;
    if (derived) from = load_record(a, a.base + 3 * row);
    const bool flip = a.row_flip[row] != 0;
    const int64_t e_begin = (a.out_row0 + row) * a.n_slots, e_end = e_begin + a.n_slots;  // the row's bytes of the flat block
    const int64_t chunk0 = e_begin >> 4, chunk1 = (e_end - 1) >> 4;
    bool bad = false;
    for (uint32_t s0 = 0; s0 < n; s0 += kTileSamples) {
      const uint32_t s1 = n - s0 < kTileSamples ? n : s0 + kTileSamples;
      const bool validate = s0 == 0;
      SAI_PGEN_EXPAND_ROW(ok, own, from, derived, a.base[3 * row], n, s0, s1, validate, tile, lane)
      if (validate && !ok) {
        bad = true;
        break;
      }
      for (int64_t chunk = chunk0 + lane; chunk <= chunk1; chunk += kWave) {
        const int64_t e0 = chunk * 16;
        const bool whole = e0 >= e_begin && e0 + 16 <= e_end;
        u32x4 word = zero;
        if (fast && whole) {
          const uint32_t col = static_cast<uint32_t>(a.first_col) + static_cast<uint32_t>(e0 - e_begin);  // col + 16 <= sample_ct: the entry point checked it
          if (col + 16 <= s0 || col >= s1) continue;  // another tile's
          if (col >= s0 && col + 16 <= s1) {
            const uint32_t rel = col - s0, wd = rel >> 4, sh = 2 * (rel & 15u);
            uint32_t codes = tile[wd] >> sh;
            if (sh) codes |= tile[wd + 1 < kTileWords ? wd + 1 : wd] << (32 - sh);
            const uint32_t lut = lut_for(a.uniform_ploidy, flip);
            if (a.uniform_ploidy == 1) {
              const uint32_t het = codes & ~(codes >> 1) & 0x55555555u;  // bit 2k set: code k is 01
              if (het) atomicMax(a.status + row, a.n_slots - (static_cast<int32_t>(e0 - e_begin) + (__builtin_ctz(het) >> 1)));
            }
            SAI_RECODE16(codes, lut, true, word)
            *reinterpret_cast<u32x4*>(a.out + e0) = word;
            continue;
          }
        }
        uint32_t mine = 0;  // bit k: byte k of the chunk belongs to this row and this tile
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          uint32_t wv = 0;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const int64_t e = e0 + 4 * j + k;
            if (e < e_begin || e >= e_end) continue;
            const int32_t slot = static_cast<int32_t>(e - e_begin);
            const int32_t col = a.first_col >= 0 ? a.first_col + slot : a.col_of_slot[slot];
            const int32_t pl = a.uniform_ploidy ? a.uniform_ploidy : a.ploidy_of_slot[slot];
            const bool valid = col >= 0 && static_cast<uint32_t>(col) < n && (pl == 1 || pl == 2);
            if (!valid) {  // the first tile's byte: 0
              if (validate) {
                atomicMax(a.status + row, kPgenBadIndex);
                mine |= 1u << (4 * j + k);
              }
              continue;
            }
            if (static_cast<uint32_t>(col) < s0 || static_cast<uint32_t>(col) >= s1) continue;
            const uint32_t rel = static_cast<uint32_t>(col) - s0;
            const uint32_t code = (tile[rel >> 4] >> (2 * (rel & 15u))) & 3u;
            if (pl == 1 && code == kPgenHet) atomicMax(a.status + row, a.n_slots - slot);
            wv |= ((lut_for(pl, flip) >> (8 * code)) & 0xFFu) << (8 * k);
            mine |= 1u << (4 * j + k);
          }
          word[j] = wv;
        }
        if (mine == 0xFFFFu) {
          *reinterpret_cast<u32x4*>(a.out + e0) = word;
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k)
              if ((mine >> (4 * j + k)) & 1u) a.out[e0 + 4 * j + k] = static_cast<int8_t>((word[j] >> (8 * k)) & 0xFFu);
        }
      }
      __syncthreads();  // the next tile, or the next row, overwrites the codes
    }
    if (bad) {
      for (int64_t chunk = chunk0 + lane; chunk <= chunk1; chunk += kWave) {
        const int64_t e0 = chunk * 16;
        if (e0 >= e_begin && e0 + 16 <= e_end) {
          *reinterpret_cast<u32x4*>(a.out + e0) = zero;
        } else {
          for (int k = 0; k < 16; ++k)
            if (e0 + k >= e_begin && e0 + k < e_end) a.out[e0 + k] = 0;
        }
      }
      if (lane == 0) a.status[row] = kPgenBadRecord;
      __syncthreads();
    }
  }
}

}  // namespace

extern "C" int sai_pgen_decode(sai_ctx* ctx, const uint8_t* bytes, int64_t n_bytes, int64_t n_out_rows, const int64_t* rec,
                               const int64_t* base, const uint8_t* row_flip, int32_t sample_ct, int32_t n_slots,
                               const int32_t* col_of_slot, int32_t first_col, const int32_t* ploidy_of_slot, int32_t uniform_ploidy,
                               int8_t* out, int64_t out_row0, int32_t* status, void* stream) {
  if (int rc = enter(ctx)) return rc;
  if (n_bytes < 0 || n_out_rows < 0 || sample_ct < 1 || n_slots < 1 || out_row0 < 0) return fail(SAI_ERR_ARG, "size out of range");
  if (uniform_ploidy < 0 || uniform_ploidy > 2) return fail(SAI_ERR_ARG, "uniform_ploidy must be 0, 1 or 2");
  if (first_col >= 0 && static_cast<int64_t>(first_col) + n_slots > sample_ct) return fail(SAI_ERR_ARG, "first_col + n_slots exceeds sample_ct");
  if (n_out_rows == 0) return SAI_OK;
  if (!rec || !base || !row_flip || !out || !status || (first_col < 0 && !col_of_slot) || (uniform_ploidy == 0 && !ploidy_of_slot) ||
      (n_bytes > 0 && !bytes))
    return fail(SAI_ERR_ARG, "NULL buffer");
  if (reinterpret_cast<uintptr_t>(out) & 15u) return fail(SAI_ERR_ARG, "out must be 16-byte aligned");
  if (out_row0 + n_out_rows > (std::numeric_limits<int64_t>::max() - 16) / n_slots) return fail(SAI_ERR_ARG, "size out of range");
  PgenArgs a;
  a.bytes = bytes;
  a.n_bytes = n_bytes;
  a.n_out_rows = n_out_rows;
  a.rec = rec;
  a.base = base;
  a.row_flip = row_flip;
  a.sample_ct = static_cast<uint32_t>(sample_ct);
  a.n_slots = n_slots;
  a.col_of_slot = col_of_slot;
  a.first_col = first_col < 0 ? -1 : first_col;
  a.ploidy_of_slot = ploidy_of_slot;
  a.uniform_ploidy = uniform_ploidy;
  a.out = out;
  a.out_row0 = out_row0;
  a.status = status;
  hipStream_t st = static_cast<hipStream_t>(stream);
  SAI_HIP(hipMemsetAsync(status, 0, static_cast<size_t>(n_out_rows) * sizeof(int32_t), st));
  // a wavefront per row; beyond the 16 per CU that are resident at once rows are taken in a grid stride
  const int64_t cap = static_cast<int64_t>(ctx->n_cu) * 16;  // past this cap: tests/test_grid_stride_device.py
  hipLaunchKernelGGL(pgen_decode_kernel, dim3(static_cast<unsigned>(n_out_rows < cap ? n_out_rows : cap)), dim3(kWave), 0, st, a);
  return check_launch("pgen_decode");
}
