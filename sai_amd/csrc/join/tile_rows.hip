// sai_tile_rows_from_site_major: selected rows of an int8 [record][sample] block in HBM -> the tiled SoA layout of
// saihip.h, in one pass.  After two inputs were joined (site_join_host.cpp) every population keeps the rows of the
// common sites only; gathering them (index_select) and re-tiling the copy (core.hip) would read and write every
// genotype twice and hold a third copy of the block.  Here the row list is an argument of the re-tiling itself:
//   byte(tile t, individual i, site s) = src[rows[t * 64 + s] * row_stride + i],  rows == NULL: the identity.
// The two entry points are internal to the package: sai_amd/site_join_device.py, their only caller, binds them, and
// this unit declares them itself (DESIGN_INGEST.md, "Sources from a file of their own").
//
// A 256-thread workgroup moves an image of 16 KiB through LDS: 64 * TPW selected rows by W individuals, W = 16 .. 256
// a power of two and TPW = 256 / W site tiles, so that a narrow population (two source individuals) fills its
// workgroups with sites where a wide one fills them with individuals.
//  * Load.  W / 4 neighbouring lanes take one row's run of W bytes, four bytes a lane: at W = 256 a wave instruction
//    reads 256 contiguous bytes of one row, and every thread has its 16 loads in flight before the first is used.  A
//    population is a run of columns inside a wider block, so a row starts at any byte: the four bytes are loaded as
//    one dword whatever their address (gfx950 serves a dword at any byte address; the compiler emits
//    global_load_dword).  Where fewer than four bytes of the run are left -- the ragged tail of the last column
//    block -- the lane loads the dword that ends with the run and shifts; a population of one to three individuals
//    is read byte by byte.  No byte outside [row, row + n_ind) of a row of the block is ever read.
//  * Image.  Row r lies at r * W + 12 * (r >> 4) bytes: every sixteen-row part of the image begins three banks
//    behind where it would, which makes the transposed byte reads below free of bank conflicts (32 lanes = the 4 parts
//    of a tile x 8 individuals, two dwords per part: banks 3 q + {0, 1}); the dword writes of the load are
//    consecutive banks.
//  * Store.  A lane gathers the 16 bytes (one individual, sixteen sites of a tile) from sixteen rows of the image and
//    stores them as one 16-byte word; neighbouring lanes hold neighbouring words, so a wave writes 1 KiB runs of dst.
// A row index outside [0, n_src_rows) is not followed: the lanes read the block's first row in its place (no branch
// around the loads), the site's bytes are written as 0 and *n_bad counts it (once, by the first column block).  The grid is not capped: gridDim.x = groups of TPW tiles, gridDim.y = column blocks of W.

#include "../common.hpp"

extern "C" {
int sai_join_device_abi_version(void);
int sai_tile_rows_from_site_major(sai_ctx* ctx, const int8_t* src, int64_t n_src_rows, int32_t n_ind, int64_t row_stride,
                                  const int32_t* rows, int64_t n_rows, int8_t* dst, int32_t* n_bad, void* stream);
}

namespace {

constexpr int kJoinDeviceAbiVersion = 1;
constexpr int kRowsBlock = 256;
constexpr int kImageBytes = 16384;  // 64 * TPW rows of W bytes
constexpr int kPartSkew = 12;       // bytes between two sixteen-row parts of the image, on top of their rows
constexpr int kMinLogWidth = 4, kMaxLogWidth = 8;
static_assert(kTile == 64, "a tile is four parts of sixteen sites");

template <int LW, bool NARROW>  // NARROW: a population of one to three individuals
__global__ __launch_bounds__(kRowsBlock) void tile_rows_kernel(const int8_t* __restrict__ src, int64_t n_src_rows, int32_t n_ind,
                                                               int64_t row_stride, const int32_t* __restrict__ rows, int64_t n_rows,
                                                               int64_t n_tiles, int8_t* __restrict__ dst, int32_t* __restrict__ n_bad) {
  constexpr int W = 1 << LW;                    // individuals of a workgroup
  constexpr int kLanesPerRow = W / 4;
  constexpr int kTilesPerGroup = kRowsBlock / W;
  constexpr int kRowsPerTrip = kRowsBlock / kLanesPerRow;  // rows the 256 threads load at a time
  constexpr int kTrips = kTile * kTilesPerGroup / kRowsPerTrip;
  static_assert(kTrips == 16 && kTile * kTilesPerGroup * W == kImageBytes, "16 KiB a workgroup, 16 loads a thread");
  __shared__ __attribute__((aligned(16))) uint8_t image[kImageBytes + (kTile * kTilesPerGroup / 16) * kPartSkew];

  const int tid = threadIdx.x;
  const int64_t tile0 = static_cast<int64_t>(blockIdx.x) * kTilesPerGroup;
  const int ind0 = static_cast<int>(blockIdx.y) * W;
  const int width = min(W, n_ind - ind0);  // individuals of this column block
  {
    const int c = (tid & (kLanesPerRow - 1)) * 4;  // the lane's first byte of the run
    const int r0 = tid >> (LW - 2);
    const int have = width - c;                    // bytes of the run from c on
    const bool counts = c == 0 && blockIdx.y == 0;
    // the row indices first, all of them in flight together: a site behind the list takes the list's last entry
    int32_t listed[kTrips];
    if (rows) {
#pragma unroll
      for (int t = 0; t < kTrips; ++t) {
        const int64_t k = tile0 * kTile + r0 + t * kRowsPerTrip;
        listed[t] = rows[k < n_rows ? k : n_rows - 1];
      }
    }
    // where each row starts, and which rows are read at all: a site behind the list or with an index outside the block
    // takes the block's first row -- an address that can be read -- and its bytes are zeroed afterwards
    int64_t start[kTrips];
    uint32_t read_mask = 0;
    int bad = 0;
#pragma unroll
    for (int t = 0; t < kTrips; ++t) {
      const int64_t k = tile0 * kTile + r0 + t * kRowsPerTrip;
      const int64_t row = rows ? static_cast<int64_t>(listed[t]) : k;
      const bool inside = row >= 0 && row < n_src_rows;
      bad += k < n_rows && !inside;
      if (k < n_rows && inside) read_mask |= 1u << t;
      start[t] = (k < n_rows && inside ? row : 0) * row_stride;
    }
    if (bad && counts) atomicAdd(n_bad, bad);
    uint32_t v[kTrips];
#pragma unroll
    for (int t = 0; t < kTrips; ++t) v[t] = 0;
    const int8_t* run = src + ind0 + c;
    if (n_src_rows > 0 && have > 0) {
      if constexpr (!NARROW) {
        // sixteen dwords in flight.  The lane at the ragged tail of the run (fewer than four bytes left) loads the four
        // bytes that END with the run -- n_ind >= 4: they are bytes of the same row -- and shifts its own down
        const int back = have >= 4 ? 0 : 4 - have;
#pragma unroll
        for (int t = 0; t < kTrips; ++t) __builtin_memcpy(&v[t], run + start[t] - back, 4);
#pragma unroll
        for (int t = 0; t < kTrips; ++t) v[t] >>= 8 * back;
      } else {  // a population of one to three individuals: its bytes one by one, in the first lane of every row
#pragma unroll
        for (int b = 0; b < 3; ++b) {
          if (b >= n_ind) break;
#pragma unroll
          for (int t = 0; t < kTrips; ++t) v[t] |= static_cast<uint32_t>(static_cast<uint8_t>(run[start[t] + b])) << (8 * b);
        }
      }
    }
#pragma unroll
    for (int t = 0; t < kTrips; ++t) v[t] = (read_mask >> t) & 1u ? v[t] : 0u;
#pragma unroll
    for (int t = 0; t < kTrips; ++t) {
      const int r = r0 + t * kRowsPerTrip;
      *reinterpret_cast<uint32_t*>(image + r * W + (r >> 4) * kPartSkew + c) = v[t];
    }
  }
  __syncthreads();
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int u = t * kRowsBlock + tid;  // a 16-byte word of dst: (tile, individual, part)
    const int q = u & 3;
    const int i = (u >> 2) & (W - 1);
    const int tt = u >> (LW + 2);
    if (i >= width || tile0 + tt >= n_tiles) continue;
    const uint8_t* col = image + (tt * kTile + q * 16) * W + (tt * 4 + q) * kPartSkew + i;
    u32x4 out;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      uint32_t word = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b) word |= static_cast<uint32_t>(col[(4 * j + b) * W]) << (8 * b);
      out[j] = word;
    }
    *reinterpret_cast<u32x4*>(dst + ((tile0 + tt) * n_ind + ind0 + i) * kTile + q * 16) = out;
  }
}

template <int LW>
void launch_tile_rows(bool narrow, int log_width, dim3 grid, hipStream_t st, const int8_t* src, int64_t n_src_rows, int32_t n_ind, int64_t row_stride,
                      const int32_t* rows, int64_t n_rows, int64_t n_tiles, int8_t* dst, int32_t* n_bad) {
  if constexpr (LW < kMaxLogWidth) {
    if (log_width != LW) return launch_tile_rows<LW + 1>(narrow, log_width, grid, st, src, n_src_rows, n_ind, row_stride, rows, n_rows, n_tiles, dst, n_bad);
  }
  if constexpr (LW == kMinLogWidth) {
    if (narrow) {
      hipLaunchKernelGGL((tile_rows_kernel<LW, true>), grid, dim3(kRowsBlock), 0, st, src, n_src_rows, n_ind, row_stride, rows, n_rows, n_tiles, dst, n_bad);
      return;
    }
  }
  hipLaunchKernelGGL((tile_rows_kernel<LW, false>), grid, dim3(kRowsBlock), 0, st, src, n_src_rows, n_ind, row_stride, rows, n_rows, n_tiles, dst, n_bad);
}

}  // namespace

extern "C" {

int sai_join_device_abi_version(void) { return kJoinDeviceAbiVersion; }

int sai_tile_rows_from_site_major(sai_ctx* ctx, const int8_t* src, int64_t n_src_rows, int32_t n_ind, int64_t row_stride,
                                  const int32_t* rows, int64_t n_rows, int8_t* dst, int32_t* n_bad, void* stream) {
  if (int rc = enter(ctx)) return rc;
  if (n_src_rows < 0 || n_ind < 0 || n_rows < 0) return fail(SAI_ERR_ARG, "negative size");
  if (!n_bad) return fail(SAI_ERR_ARG, "NULL buffer");
  hipStream_t st = static_cast<hipStream_t>(stream);
  SAI_HIP(hipMemsetAsync(n_bad, 0, sizeof(int32_t), st));
  if (n_rows == 0 || n_ind == 0) return SAI_OK;
  if (!src || !dst) return fail(SAI_ERR_ARG, "NULL buffer");
  if (reinterpret_cast<uintptr_t>(dst) & 15) return fail(SAI_ERR_ARG, "dst is not 16-byte aligned");
  if (row_stride < n_ind) return fail(SAI_ERR_ARG, "row_stride %lld < n_ind %d", (long long)row_stride, n_ind);
  if (!rows && n_rows != n_src_rows)
    return fail(SAI_ERR_ARG, "rows is NULL (the identity) but n_rows %lld != n_src_rows %lld", (long long)n_rows, (long long)n_src_rows);
  int log_width = kMinLogWidth;  // the narrowest workgroup that takes the population in one column block, else the widest
  while (log_width < kMaxLogWidth && (1 << log_width) < n_ind) ++log_width;
  const int64_t n_tiles = (n_rows + kTile - 1) / kTile;
  const int64_t tiles_per_group = kRowsBlock >> log_width;
  const int64_t n_groups = (n_tiles + tiles_per_group - 1) / tiles_per_group;
  const int64_t n_blk = (static_cast<int64_t>(n_ind) + (1 << log_width) - 1) >> log_width;
  if (n_groups > 0x7FFFFFFFll || n_blk > 65535) return fail(SAI_ERR_UNSUPPORTED, "block too large for one launch");
  dim3 grid(static_cast<unsigned>(n_groups), static_cast<unsigned>(n_blk));
  launch_tile_rows<kMinLogWidth>(n_ind < 4, log_width, grid, st, src, n_src_rows, n_ind, row_stride, rows, n_rows, n_tiles, dst, n_bad);
  return check_launch("tile_rows_from_site_major");
}

}  // extern "C"
