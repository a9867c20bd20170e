// sai_pgen_pack2: the compressed hard-call records of a PLINK 2 .pgen in HBM -> one population's block in the
// packed2 layout of saihip.h (include/saihip_pgen_packed.h), without the int8 [record][sample] block in between.
//
// The shape is that of pgen_decode.hip: one wavefront (one 64-lane workgroup) per output row, the row expanded to
// dense 2-bit codes in 4 KiB of LDS by the shared expand half (pgen_expand.hpp), rows beyond 16 per CU in a grid
// stride.  Only what happens to the codes differs.  They sit in LDS in the .bed bit order and a packed2 tile wants
// 64 consecutive codes of one row per site and group, so nothing is widened and nothing is transposed: the wave of
// row r owns site r % 64 of tile r / 64 and
//  * fast path -- the individuals are a run of consecutive sample columns (the caller says so): lane l takes the
//    groups l, l + 64, ...; a group's 64 codes are 128 bits of LDS from code first_col + 64 g on, read as one aligned
//    16-byte word and the word behind it, funnel-shifted by 2 * (first_col & 15) and recoded 16 fields at a time on
//    the two bit planes (pgen_pack2_recode): no loop over the fields, no branch on a code.  One 16-byte store per
//    group at tile + g * 1 KiB + site * 16 B; the tail group's w_tail words at n_full * 1 KiB + site * 4 * w_tail;
//  * general path -- any col_of_ind (permutation, repeats): one 2-bit gather per field from LDS into the same
//    words, recoded and stored the same way.
// Rows wider than one LDS window (16 384 samples) never assemble a group from two windows through global memory.
// On the fast path the windows are placed by the population, not by the row: window k starts at the 16-aligned
// sample that holds the first code of group 255 k and serves the groups [255 k, 255 k + 255), whose 4 x 255 + 1
// words fit the 1 024 of a window.  On the general path a lane keeps the four words of its group in
// registers while the windows pass, 64 groups at a time.  As in pgen_decode.hip the first window validates the whole
// record before a word of the row is written (a bad row is zeros and SAI_PGEN_STATUS_BAD_RECORD); later windows
// validate nothing and walk only the difflist groups that reach into them.
// status / unfit: every lane keeps the lowest individual it met and raises it with one atomicMax at the end of the
// row.  The call that holds the last site fills the padding sites of the last tile with ones: extra grid entries
// behind the rows.  Every index is checked before it is used.

#include "../common.hpp"
#include "../plink/packed2_layout.hpp"
#include "pgen_codes.hpp"
#include "pgen_expand.hpp"
#include "pgen_pack2_codes.hpp"
#include "saihip_pgen_packed.h"

namespace {

constexpr int kWindowGroups = (kTileWords - 4) / 4;        // 255: groups of the fast path per LDS window
static_assert(4 * kWindowGroups + 1 <= kTileWords, "the last group of a window reads five words");

struct PackArgs {
  const uint8_t* bytes;
  int64_t n_bytes;
  int64_t n_out_rows;
  const int64_t* rec;   // [n_out_rows][3]
  const int64_t* base;  // [n_out_rows][3]
  const uint8_t* row_flip;
  uint32_t sample_ct;
  int32_t n_ind;
  const int32_t* col_of_ind;
  int32_t first_col;  // >= 0: col_of_ind[i] == first_col + i
  uint32_t* packed;
  int64_t row_begin;  // the call's sites [row_begin, row_begin + n_out_rows)
  int64_t n_pad;      // padding sites behind them that this call fills (it holds the last site), else 0
  int32_t* status;
  int32_t* unfit;
  int32_t n_full, w_tail;  // the layout of n_ind
  int32_t n_groups;        // n_full + (w_tail != 0)
};

// every word of one site the same (a bad row: 0; a padding site: ones)
__device__ __forceinline__ void fill_site(const PackArgs& a, uint32_t* out, int site_in_tile, uint32_t value) {
  const u32x4 word = {value, value, value, value};
  for (int g = threadIdx.x; g < a.n_groups; g += kWave) packed2_store_group(out, a.n_full, a.w_tail, site_in_tile, g, word);
}

template <int PLOIDY, bool FAST>
__global__ __launch_bounds__(kWave) void pgen_pack2_kernel(PackArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t tile[kTileWords];
  const int lane = threadIdx.x;
  const uint32_t n = a.sample_ct;
  const int64_t tile_words = static_cast<int64_t>(a.n_full) * 256 + a.w_tail * 64;
  for (int64_t row = blockIdx.x; row < a.n_out_rows + a.n_pad; row += gridDim.x) {
    const int64_t site = a.row_begin + row;
    uint32_t* out = a.packed + (site / kTile) * tile_words;
    const int sit = static_cast<int>(site % kTile);
    if (row >= a.n_out_rows) {  // a padding site of the last tile: all missing
      fill_site(a, out, sit, 0xFFFFFFFFu);
      continue;
    }
    const Record own = load_record(a, a.rec + 3 * row);
    const bool derived = own.kind == 2 || own.kind == 3;
    Record from = own;
    if (derived) from = load_record(a, a.base + 3 * row);
    const bool flip = a.row_flip[row] != 0;
    int32_t first_het = -1, first_unfit = -1;  // the lowest individual of this lane that is refused / does not fit
    bool bad = false, bad_index = false;
    if (FAST) {
      const uint32_t aligned = static_cast<uint32_t>(a.first_col) & ~15u;
      const uint32_t shift = 2u * (static_cast<uint32_t>(a.first_col) & 15u);
      for (int g_lo = 0; g_lo < a.n_groups; g_lo += kWindowGroups) {
        const uint32_t s0 = aligned + 64u * static_cast<uint32_t>(g_lo);  // < first_col + n_ind <= sample_ct: the entry point checked it
        const uint32_t s1 = n - s0 < kTileSamples ? n : s0 + kTileSamples;
        const bool validate = g_lo == 0;
        SAI_PGEN_EXPAND_ROW(ok, own, from, derived, a.base[3 * row], n, s0, s1, validate, tile, lane)
        if (validate && !ok) {
          bad = true;
          break;
        }
        const int g_hi = min(g_lo + kWindowGroups, a.n_groups);
        for (int g = g_lo + lane; g < g_hi; g += kWave) {
          const int wd = 4 * (g - g_lo);  // + 4 < kTileWords
          const u32x4 d = *reinterpret_cast<const u32x4*>(tile + wd);
          const uint32_t d4 = tile[wd + 4];
          const int n_here = min(64, a.n_ind - 64 * g);  // individuals of this group (the tail group: fewer than 64)
          const uint32_t codes[4] = {__funnelshift_r(d[0], d[1], shift), __funnelshift_r(d[1], d[2], shift),
                                     __funnelshift_r(d[2], d[3], shift), __funnelshift_r(d[3], d4, shift)};
          u32x4 word;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            uint32_t het, unfit;
            word[j] = pgen_pack2_recode<PLOIDY>(codes[j], valid_fields(n_here - 16 * j), flip, het, unfit);
            if (PLOIDY == 1 && het && first_het < 0) first_het = 64 * g + 16 * j + (__builtin_ctz(het) >> 1);
            if (PLOIDY == 2 && unfit && first_unfit < 0) first_unfit = 64 * g + 16 * j + (__builtin_ctz(unfit) >> 1);
          }
          packed2_store_group(out, a.n_full, a.w_tail, sit, g, word);
        }
        __syncthreads();  // the next window, or the next row, overwrites the codes
      }
    } else {
      const bool one_window = n <= kTileSamples;
      for (int g_lo = 0; g_lo < a.n_groups && !bad; g_lo += kWave) {
        const int g = g_lo + lane;
        const int n_here = g < a.n_groups ? min(64, a.n_ind - 64 * g) : 0;
        uint32_t codes[4] = {0u, 0u, 0u, 0u}, valid[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) valid[j] = valid_fields(n_here - 16 * j);
        for (uint32_t s0 = 0; s0 < n; s0 += kTileSamples) {
          const uint32_t s1 = n - s0 < kTileSamples ? n : s0 + kTileSamples;
          const bool validate = s0 == 0 && g_lo == 0;
          if (!one_window || g_lo == 0) {  // one window: its codes stay in LDS for every round of groups
            SAI_PGEN_EXPAND_ROW(ok, own, from, derived, a.base[3 * row], n, s0, s1, validate, tile, lane)
            if (validate && !ok) {
              bad = true;
              break;
            }
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int n_word = min(16, n_here - 16 * j);
            for (int k = 0; k < n_word; ++k) {
              const int32_t col = a.col_of_ind[64 * g + 16 * j + k];
              if (col < 0 || static_cast<uint32_t>(col) >= n) {
                valid[j] &= ~(1u << (2 * k));
                bad_index = true;
              } else if (static_cast<uint32_t>(col) >= s0 && static_cast<uint32_t>(col) < s1) {
                const uint32_t rel = static_cast<uint32_t>(col) - s0;
                codes[j] |= ((tile[rel >> 4] >> (2 * (rel & 15u))) & 3u) << (2 * k);
              }
            }
          }
          if (!one_window) __syncthreads();  // the next window overwrites the codes
        }
        if (bad || g >= a.n_groups) continue;
        u32x4 word;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          uint32_t het, unfit;
          word[j] = pgen_pack2_recode<PLOIDY>(codes[j], valid[j], flip, het, unfit);
          if (PLOIDY == 1 && het && first_het < 0) first_het = 64 * g + 16 * j + (__builtin_ctz(het) >> 1);
          if (PLOIDY == 2 && unfit && first_unfit < 0) first_unfit = 64 * g + 16 * j + (__builtin_ctz(unfit) >> 1);
        }
        packed2_store_group(out, a.n_full, a.w_tail, sit, g, word);
      }
      __syncthreads();  // the next row overwrites the codes
    }
    if (bad) {
      fill_site(a, out, sit, 0u);
      if (lane == 0) a.status[row] = kPgenBadRecord;
      __syncthreads();
      continue;
    }
    if (bad_index) atomicMax(a.status + row, kPgenBadIndex);
    if (first_het >= 0) atomicMax(a.status + row, a.n_ind - first_het);
    if (first_unfit >= 0) atomicMax(a.unfit + row, a.n_ind - first_unfit);
  }
}

}  // namespace

extern "C" int sai_pgen_pack2(sai_ctx* ctx, const uint8_t* bytes, int64_t n_bytes, int64_t n_out_rows, const int64_t* rec,
                              const int64_t* base, const uint8_t* row_flip, int32_t sample_ct, int32_t n_ind,
                              const int32_t* col_of_ind, int32_t first_col, int32_t ploidy, uint8_t* packed, int64_t n_sites,
                              int64_t out_row0, int32_t* status, int32_t* unfit, void* stream) {
  if (int rc = enter(ctx)) return rc;
  if (n_bytes < 0 || sample_ct < 1 || !packed2_sizes_ok(n_out_rows, n_ind, n_sites, out_row0)) return fail(SAI_ERR_ARG, "size out of range");
  if (const char* why = packed2_bad_selection(ploidy, first_col, n_ind, sample_ct, "first_col + n_slots exceeds sample_ct")) return fail(SAI_ERR_ARG, "%s", why);
  if (n_out_rows == 0) return SAI_OK;
  if (!rec || !base || !row_flip || !packed || !status || !unfit || (first_col < 0 && !col_of_ind) || (n_bytes > 0 && !bytes))
    return fail(SAI_ERR_ARG, "NULL buffer");
  if (reinterpret_cast<uintptr_t>(packed) & 15u) return fail(SAI_ERR_ARG, "packed must be 16-byte aligned");
  PackArgs a;
  a.bytes = bytes;
  a.n_bytes = n_bytes;
  a.n_out_rows = n_out_rows;
  a.rec = rec;
  a.base = base;
  a.row_flip = row_flip;
  a.sample_ct = static_cast<uint32_t>(sample_ct);
  a.n_ind = n_ind;
  a.col_of_ind = col_of_ind;
  a.first_col = first_col < 0 ? -1 : first_col;
  a.packed = reinterpret_cast<uint32_t*>(packed);
  a.row_begin = out_row0;
  const int64_t row_end = out_row0 + n_out_rows;
  a.n_pad = row_end == n_sites ? (kTile - row_end % kTile) % kTile : 0;
  a.status = status;
  a.unfit = unfit;
  packed2_set_groups(a, n_ind);
  // a wavefront per row (and per padding site); beyond the 16 per CU that are resident at once rows are taken in a grid stride
  const int64_t want = n_out_rows + a.n_pad;
  const int64_t cap = static_cast<int64_t>(ctx->n_cu) * 16;  // past this cap: tests/test_grid_stride_device.py
  const dim3 grid(static_cast<unsigned>(want < cap ? want : cap)), block(kWave);
  SAI_PACKED2_LAUNCH(pgen_pack2_kernel, a, ploidy, n_out_rows, grid, block, stream);
  return check_launch("pgen_pack2");
}
