// sai_bed_pack2: variant-major PLINK 1 .bed rows in HBM -> one population's block in the packed2 layout of saihip.h
// (include/saihip_packed_ingest.h), without the int8 [record][sample] block in between.
//
// Nothing is transposed: a .bed is variant-major and a packed2 tile is site-major inside a 64-individual group, so
// the 16 bytes a site holds of a full group are 64 consecutive codes of one .bed row, shifted to a word boundary
// and recoded.  One wavefront owns a tile of 64 sites and a run of its groups (the tail group is the last of them);
// lane l is site l of the tile and walks ITS row:
//  * fast path -- the individuals are a run of consecutive .fam columns (the caller says so): per group the lane
//    reads the aligned 32-bit words that hold its 64 codes (four new ones per group: the fifth is the first of the
//    next group), funnel-shifts them by the row's byte offset and the 2 * (column & 3) bits, and recodes each word
//    with bit operations on its two planes (pack2_recode): no loop over the fields, no branch on a code;
//  * general path -- any col_of_ind (permutation, repeats): one 2-bit gather per field into the same 16-code
//    words, recoded the same way.
// Stores: a lane's four words of a full group are one 16-byte store, 64 lanes x 16 B = the group's 1 KiB block in
// one instruction; the tail group's w_tail words per lane lie back to back across the wave as well.  A lane whose
// site is outside the call's range stores nothing (a word belongs to one site, so calls never share one), except
// that the call which holds the last site fills the padding sites of the last tile with ones.
// Reads: a row is 501 bytes at 2 002 samples, a lane takes 16 bytes of it per group and the next group's lie in
// the line it has just touched, so the lines are reused from L1 / L2 and the rows leave HBM once.  No LDS; the only
// atomics are the rare atomicMax on status / unfit.  Every index is checked before it is used and an aligned word
// is read only where all four of its bytes lie inside the rows buffer (its edges are read byte by byte).

#include "../common.hpp"
#include "packed2_layout.hpp"
#include "pack2_codes.hpp"
#include "saihip_packed_ingest.h"

namespace {

struct PackArgs {
  const uint8_t* rows;
  const uint8_t* rows_end;  // rows + n_batch_rows * row_bytes
  int64_t n_batch_rows;
  int64_t row_bytes;
  const int32_t* row_in_batch;
  const uint8_t* row_flip;
  int32_t n_cols;
  int32_t n_ind;
  const int32_t* col_of_ind;
  int32_t first_col;  // >= 0: col_of_ind[i] == first_col + i
  uint32_t* packed;
  int64_t n_sites;
  int64_t row_begin, row_end;  // the call's sites [out_row0, out_row0 + n_out_rows)
  int32_t* status;
  int32_t* unfit;
  int64_t tile0;            // the first tile that holds a site of the call
  int64_t n_units;          // (tiles of the call) x (runs per tile)
  int32_t n_full, w_tail;   // the layout of n_ind
  int32_t n_groups;         // n_full + (w_tail != 0)
  int32_t runs_per_tile;    // ceil(n_groups / groups_per_run)
  int32_t groups_per_run;
};

constexpr int kPackBlock = 256;  // four wavefronts, each with a unit of its own
constexpr int kGroupsPerRun = 8;

// the aligned 32-bit word at p, read only where it lies inside the rows buffer
__device__ __forceinline__ uint32_t load_word(const PackArgs& a, const uint8_t* p) {
  if (p >= a.rows && p + 4 <= a.rows_end) return *reinterpret_cast<const uint32_t*>(p);
  uint32_t w = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (p + k >= a.rows && p + k < a.rows_end) w |= static_cast<uint32_t>(p[k]) << (8 * k);
  return w;
}

template <int PLOIDY, bool FAST>
__global__ __launch_bounds__(kPackBlock) void bed_pack2_kernel(PackArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = static_cast<int64_t>(blockIdx.x) * (kPackBlock / 64) + (threadIdx.x >> 6);
  const int64_t n_waves = static_cast<int64_t>(gridDim.x) * (kPackBlock / 64);
  const int64_t tile_words = static_cast<int64_t>(a.n_full) * 256 + a.w_tail * 64;
  for (int64_t unit = wave; unit < a.n_units; unit += n_waves) {
    const int64_t tile = a.tile0 + unit / a.runs_per_tile;
    const int g0 = static_cast<int>(unit % a.runs_per_tile) * a.groups_per_run;
    const int g1 = min(g0 + a.groups_per_run, a.n_groups);
    const int64_t site = tile * kTile + lane;
    const bool mine = site >= a.row_begin && site < a.row_end;
    const bool padding = site >= a.n_sites && a.row_end == a.n_sites;  // of the last tile, by the call that holds the last site
    if (!mine && !padding) continue;
    uint32_t* out = a.packed + tile * tile_words;
    const int64_t r = site - a.row_begin;  // the row of the call: indexes row_in_batch, row_flip, status, unfit
    bool ok = false, flip = false;
    const uint8_t* src = a.rows;
    if (mine) {
      const int64_t rib = a.row_in_batch[r];
      ok = rib >= 0 && rib < a.n_batch_rows;
      if (ok) src = a.rows + rib * a.row_bytes;
      else atomicMax(a.status + r, kPlinkBadIndex);
      flip = a.row_flip[r] != 0;
    }
    // fast path: the aligned word that holds the first code of group g0, and what to shift by
    const uint8_t* p = nullptr;
    uint32_t shift = 0, carry = 0;
    if (FAST && ok) {
      const int64_t col0 = static_cast<int64_t>(a.first_col) + 64ll * g0;
      const uint8_t* first = src + (col0 >> 2);
      const uintptr_t mis = reinterpret_cast<uintptr_t>(first) & 3u;
      p = first - mis;
      shift = static_cast<uint32_t>(8 * mis + 2 * (col0 & 3));  // 0 .. 30
      carry = load_word(a, p);
    }
    int32_t first_het = -1, first_unfit = -1;  // the lowest individual of this run that is refused / does not fit
    for (int g = g0; g < g1; ++g) {
      const int n_here = min(64, a.n_ind - 64 * g);  // individuals of this group (the tail group: fewer than 64)
      u32x4 word = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
      if (mine) {
        uint32_t codes[4] = {0u, 0u, 0u, 0u}, valid[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) valid[j] = ok ? valid_fields(n_here - 16 * j) : 0u;
        if (FAST) {
          if (ok) {
            uint32_t d[5];
            d[0] = carry;
#pragma unroll
            for (int j = 1; j < 5; ++j) d[j] = load_word(a, p + 4 * j);
#pragma unroll
            for (int j = 0; j < 4; ++j) codes[j] = __funnelshift_r(d[j], d[j + 1], shift);
            carry = d[4];
            p += 16;
          }
        } else if (ok) {
          for (int j = 0; j < 4; ++j) {
            const int n_word = min(16, n_here - 16 * j);
            for (int k = 0; k < n_word; ++k) {
              const int32_t col = a.col_of_ind[64 * g + 16 * j + k];
              if (col >= 0 && col < a.n_cols) {
                codes[j] |= ((static_cast<uint32_t>(src[col >> 2]) >> (2 * (col & 3))) & 3u) << (2 * k);
              } else {
                valid[j] &= ~(1u << (2 * k));
                atomicMax(a.status + r, kPlinkBadIndex);
              }
            }
          }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          uint32_t het, unfit;
          word[j] = pack2_recode<PLOIDY>(codes[j], valid[j], flip, het, unfit);
          if (PLOIDY == 1 && het && first_het < 0) first_het = 64 * g + 16 * j + (__builtin_ctz(het) >> 1);
          if (PLOIDY == 2 && unfit && first_unfit < 0) first_unfit = 64 * g + 16 * j + (__builtin_ctz(unfit) >> 1);
        }
      }
      packed2_store_group(out, a.n_full, a.w_tail, lane, g, word);  // a full group: its 1 KiB block, one store per wave
    }
    if (first_het >= 0) atomicMax(a.status + r, a.n_ind - first_het);
    if (first_unfit >= 0) atomicMax(a.unfit + r, a.n_ind - first_unfit);
  }
}

int groups_per_run() {
  static const int n = [] {  // SAI_BED_PACK2_GROUPS: tuning knob for sweeps (tools/plink_packed_rate.py)
    const char* e = std::getenv("SAI_BED_PACK2_GROUPS");
    const int v = e ? std::atoi(e) : 0;
    return v > 0 ? v : kGroupsPerRun;
  }();
  return n;
}

}  // namespace

extern "C" int sai_bed_pack2(sai_ctx* ctx, const uint8_t* rows, int64_t n_batch_rows, int64_t row_bytes, int64_t n_out_rows,
                             const int32_t* row_in_batch, const uint8_t* row_flip, int32_t n_cols, int32_t n_ind,
                             const int32_t* col_of_ind, int32_t first_col, int32_t ploidy, uint8_t* packed, int64_t n_sites,
                             int64_t out_row0, int32_t* status, int32_t* unfit, void* stream) {
  if (int rc = enter(ctx)) return rc;
  if (n_batch_rows < 0 || row_bytes < 0 || n_cols < 0 || !packed2_sizes_ok(n_out_rows, n_ind, n_sites, out_row0))
    return fail(SAI_ERR_ARG, "size out of range");
  if (static_cast<int64_t>(n_cols) > 4 * row_bytes) return fail(SAI_ERR_ARG, "n_cols exceeds the 4 * row_bytes genotypes of a row");
  if (const char* why = packed2_bad_selection(ploidy, first_col, n_ind, n_cols, "first_col + n_slots exceeds n_cols")) return fail(SAI_ERR_ARG, "%s", why);
  if (n_out_rows == 0) return SAI_OK;
  if (!row_in_batch || !row_flip || !packed || !status || !unfit || (first_col < 0 && !col_of_ind) ||
      (n_batch_rows > 0 && row_bytes > 0 && !rows))
    return fail(SAI_ERR_ARG, "NULL buffer");
  if (reinterpret_cast<uintptr_t>(packed) & 15u) return fail(SAI_ERR_ARG, "packed must be 16-byte aligned");
  if (n_batch_rows > 0 && row_bytes > std::numeric_limits<int64_t>::max() / n_batch_rows) return fail(SAI_ERR_ARG, "size out of range");
  PackArgs a;
  a.rows = rows;
  a.rows_end = rows + n_batch_rows * row_bytes;
  a.n_batch_rows = n_batch_rows;
  a.row_bytes = row_bytes;
  a.row_in_batch = row_in_batch;
  a.row_flip = row_flip;
  a.n_cols = n_cols;
  a.n_ind = n_ind;
  a.col_of_ind = col_of_ind;
  a.first_col = first_col < 0 ? -1 : first_col;
  a.packed = reinterpret_cast<uint32_t*>(packed);
  a.n_sites = n_sites;
  a.row_begin = out_row0;
  a.row_end = out_row0 + n_out_rows;
  a.status = status;
  a.unfit = unfit;
  packed2_set_groups(a, n_ind);
  a.groups_per_run = groups_per_run();
  a.runs_per_tile = (a.n_groups + a.groups_per_run - 1) / a.groups_per_run;
  a.tile0 = out_row0 / kTile;
  const int64_t n_tiles = (a.row_end + kTile - 1) / kTile - a.tile0;
  a.n_units = n_tiles * a.runs_per_tile;
  // a memory-bound pass: enough workgroups to fill the chip, grid-stride beyond that
  const int64_t want = (a.n_units + kPackBlock / 64 - 1) / (kPackBlock / 64);
  const int64_t cap = static_cast<int64_t>(ctx->n_cu) * 16;  // past this cap: tests/test_grid_stride_device.py
  const dim3 grid(static_cast<unsigned>(want < cap ? want : cap)), block(kPackBlock);
  SAI_PACKED2_LAUNCH(bed_pack2_kernel, a, ploidy, n_out_rows, grid, block, stream);
  return check_launch("bed_pack2");
}
