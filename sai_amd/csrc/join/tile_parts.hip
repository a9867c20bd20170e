// sai_tile_rows_from_parts: ONE tiled population whose individuals come from several int8 [record][sample] blocks in HBM,
// each with its own row list -- a source population such as NEA = {Altai, Vindija} whose genomes arrived in a file each
// (DESIGN_INGEST.md, "Several source files").  Part p owns the individuals [ind0_p, ind0_p + n_ind_p) of the population:
//   byte(tile t, individual ind0_p + i, site s) = src_p[rows_p[t * 64 + s] * row_stride_p + i],  rows_p == NULL: the identity.
// Stacking the columns, making the stack contiguous and tiling it would move every genotype three times and needs an
// index_select per block in front of it; P launches of tile_rows.hip cannot write one population.  Here one launch
// fills every row of the image from all parts.  The entry points are internal to the package:
// sai_amd/site_join_parts.py, their only caller, binds them, and this unit declares them itself.
//
// The scheme is tile_rows.hip's: a 256-thread workgroup moves an image of 16 KiB through LDS, 64 * TPW sites by W
// individuals of the POPULATION (W = 16 .. 256, TPW = 256 / W), row r at r * W + 12 * (r >> 4) bytes, and stores whole
// 1 KiB runs of dst as 16-byte words.  What differs is the load: the workgroup walks the parts (they are kernel
// arguments, so the walk is scalar) and fills, for each part that has columns in its column block, that run of columns
// -- a "segment" -- of every image row:
//  * a segment of four columns or more as tile_rows.hip loads a population: W / 4 lanes a row, four bytes a lane as one
//    dword at any byte address, the lane at the ragged tail loading the dword that ENDS with the segment; sixteen row
//    indices, then sixteen dwords in flight per thread.  A segment starts at any byte of the image row, so a full dword
//    goes to LDS as a dword only where the segment starts on one, else as four bytes; the tail lane writes its bytes
//    one by one -- the next byte of the image row belongs to another part;
//  * a segment of one to three columns -- one archaic genome per file, the shape this kernel is for -- a thread per
//    image row: its row indices first, then its bytes one by one, written to the image as bytes.
// No byte outside [row, row + n_ind_p) of a row of a part's block is read.  A row index outside [0, n_src_rows_p) is not
// followed: the lanes read the block's first row in its place, the part's bytes of the site are 0 and *n_bad counts the
// (site, part) pair once, in the column block that holds the part's first individual.  The parts cover [0, n_ind)
// exactly once (the host checks it), so every byte of the image that is stored was written by exactly one part.

#include "../common.hpp"

#define SAI_TILE_MAX_PARTS 16

extern "C" {
struct sai_tile_part {
  const int8_t* src;     // the part's block, at its first column
  int64_t n_src_rows;    // rows of the block
  int64_t row_stride;    // bytes between two rows, >= n_ind
  const int32_t* rows;   // n_rows device indices into the block, or NULL: the identity (n_rows == n_src_rows)
  int32_t ind0, n_ind;   // the individuals [ind0, ind0 + n_ind) of the population
};
int sai_tile_parts_abi_version(void);
int sai_tile_rows_from_parts(sai_ctx* ctx, int32_t n_parts, const sai_tile_part* parts_host, int64_t n_rows, int32_t n_ind, int8_t* dst,
                             int32_t* n_bad, void* stream);
}

namespace {

constexpr int kTilePartsAbiVersion = 1;
constexpr int kPartsBlock = 256;
constexpr int kImageBytes = 16384;  // 64 * TPW rows of W bytes
constexpr int kPartSkew = 12;       // bytes between two sixteen-row parts of the image, on top of their rows
constexpr int kMinLogWidth = 4, kMaxLogWidth = 8;
static_assert(kTile == 64, "a tile is four parts of sixteen sites");
static_assert(sizeof(sai_tile_part) == 40, "sixteen parts are 640 bytes of kernel arguments");

struct PartList {
  sai_tile_part p[SAI_TILE_MAX_PARTS];
};

template <int LW>
__global__ __launch_bounds__(kPartsBlock) void tile_parts_kernel(const PartList parts, int32_t n_parts, int32_t n_ind, int64_t n_rows,
                                                                 int64_t n_tiles, int8_t* __restrict__ dst, int32_t* __restrict__ n_bad) {
  constexpr int W = 1 << LW;  // individuals of a workgroup
  constexpr int kLanesPerRow = W / 4;
  constexpr int kTilesPerGroup = kPartsBlock / W;
  constexpr int kImageRows = kTile * kTilesPerGroup;
  constexpr int kRowsPerTrip = kPartsBlock / kLanesPerRow;  // rows the 256 threads load at a time, four bytes a lane
  constexpr int kTrips = kImageRows / kRowsPerTrip;
  constexpr int kNarrowTrips = kImageRows > kPartsBlock ? kImageRows / kPartsBlock : 1;  // rows a thread fills of a narrow segment
  static_assert(kTrips == 16 && kImageRows * W == kImageBytes, "16 KiB a workgroup, 16 loads a thread");
  __shared__ __attribute__((aligned(16))) uint8_t image[kImageBytes + (kImageRows / 16) * kPartSkew];

  const int thread = threadIdx.x;
  const int64_t tile0 = static_cast<int64_t>(blockIdx.x) * kTilesPerGroup;
  const int ind0 = static_cast<int>(blockIdx.y) * W;
  const int width = min(W, n_ind - ind0);  // individuals of this column block
  // what is left of the row lists from this workgroup's first site on, at most an image: 1 .. kImageRows (the grid has
  // no workgroup behind the last site)
  const int64_t site0 = tile0 * kTile;
  const int left = static_cast<int>(min(n_rows - site0, static_cast<int64_t>(kImageRows)));
#pragma nounroll
  for (int p = 0; p < n_parts; ++p) {
    const sai_tile_part part = parts.p[p];
    // The thread's number as the loop body sees it.  Everything a thread computes from it below (its rows, its image
    // addresses, the masks of its sixteen trips) is the same for every part, and the compiler would compute all of it
    // once in front of the loop and keep it in registers across it: 187 VGPRs, two waves a SIMD.  Recomputing it per
    // part costs a few dozen VALU instructions next to thirty-two loads from HBM.
    int tid = thread;
    asm volatile("" : "+v"(tid));
    const int first = part.ind0, count = part.n_ind;
    const int a = max(first, ind0), b = min(first + count, ind0 + width);  // the part's columns in this column block
    if (a >= b) continue;
    const int8_t* __restrict__ src = part.src + (a - first);
    const int32_t* __restrict__ rows = part.rows ? part.rows + site0 : nullptr;  // the list from this workgroup's first site on
    const int64_t n_src_rows = part.n_src_rows, row_stride = part.row_stride;
    const int seg = b - a;       // columns of the segment
    const int o = a - ind0;      // its first byte in an image row
    const bool counts = a == first;  // the column block that holds the part's first individual counts its bad rows
    if (seg >= 4) {
      const int c = (tid & (kLanesPerRow - 1)) * 4;  // the lane's first byte of the segment
      const int r0 = tid >> (LW - 2);
      const int have = seg - c;                      // bytes of the segment from c on
      // the row indices first, all of them in flight together: a site behind the list takes the list's last entry
      int32_t listed[kTrips];
      if (rows) {
#pragma unroll
        for (int t = 0; t < kTrips; ++t) {
          const int k = r0 + t * kRowsPerTrip;
          listed[t] = rows[k < left ? k : left - 1];
        }
      }
      // where each row starts, and which rows are read at all: a site behind the list or with an index outside the block
      // takes the block's first row -- an address that can be read -- and its bytes are zeroed afterwards
      int64_t start[kTrips];
      uint32_t read_mask = 0;
      int bad = 0;
#pragma unroll
      for (int t = 0; t < kTrips; ++t) {
        const int k = r0 + t * kRowsPerTrip;
        const int64_t row = rows ? static_cast<int64_t>(listed[t]) : site0 + k;
        const bool inside = row >= 0 && row < n_src_rows;
        bad += k < left && !inside;
        if (k < left && inside) read_mask |= 1u << t;
        start[t] = (k < left && inside ? row : 0) * row_stride;
      }
      if (bad && counts && c == 0) atomicAdd(n_bad, bad);
      uint32_t v[kTrips];
#pragma unroll
      for (int t = 0; t < kTrips; ++t) v[t] = 0;
      if (n_src_rows > 0 && have > 0) {
        // sixteen dwords in flight.  The lane at the ragged tail of the segment (fewer than four bytes left) loads the
        // four bytes that END with the segment -- seg >= 4: they are bytes of the same row of the part -- and shifts
        const int back = have >= 4 ? 0 : 4 - have;
        const int8_t* run = src + c - back;
#pragma unroll
        for (int t = 0; t < kTrips; ++t) __builtin_memcpy(&v[t], run + start[t], 4);
#pragma unroll
        for (int t = 0; t < kTrips; ++t) v[t] >>= 8 * back;
      }
#pragma unroll
      for (int t = 0; t < kTrips; ++t) v[t] = (read_mask >> t) & 1u ? v[t] : 0u;
      if (have >= 4) {
        if ((o & 3) == 0) {  // the segment starts on a dword of the image row
#pragma unroll
          for (int t = 0; t < kTrips; ++t) {
            const int r = r0 + t * kRowsPerTrip;
            *reinterpret_cast<uint32_t*>(image + r * W + (r >> 4) * kPartSkew + o + c) = v[t];
          }
        } else {
#pragma unroll
          for (int t = 0; t < kTrips; ++t) {
            const int r = r0 + t * kRowsPerTrip;
            uint8_t* at = image + r * W + (r >> 4) * kPartSkew + o + c;
#pragma unroll
            for (int j = 0; j < 4; ++j) at[j] = static_cast<uint8_t>(v[t] >> (8 * j));
          }
        }
      } else if (have > 0) {  // the ragged tail: one to three bytes, and the byte behind them is another part's
#pragma unroll
        for (int t = 0; t < kTrips; ++t) {
          const int r = r0 + t * kRowsPerTrip;
          uint8_t* at = image + r * W + (r >> 4) * kPartSkew + o + c;
#pragma unroll
          for (int j = 0; j < 3; ++j)
            if (j < have) at[j] = static_cast<uint8_t>(v[t] >> (8 * j));
        }
      }
    } else if (kImageRows >= kPartsBlock || tid < kImageRows) {  // one to three columns: a thread per image row
      int32_t listed[kNarrowTrips];
      if (rows) {
#pragma unroll
        for (int t = 0; t < kNarrowTrips; ++t) {
          const int k = tid + t * kPartsBlock;
          listed[t] = rows[k < left ? k : left - 1];
        }
      }
      int64_t start[kNarrowTrips];
      uint32_t read_mask = 0;
      int bad = 0;
#pragma unroll
      for (int t = 0; t < kNarrowTrips; ++t) {
        const int k = tid + t * kPartsBlock;
        const int64_t row = rows ? static_cast<int64_t>(listed[t]) : site0 + k;
        const bool inside = row >= 0 && row < n_src_rows;
        bad += k < left && !inside;
        if (k < left && inside) read_mask |= 1u << t;
        start[t] = (k < left && inside ? row : 0) * row_stride;
      }
      if (bad && counts) atomicAdd(n_bad, bad);
      uint32_t v[kNarrowTrips];
#pragma unroll
      for (int t = 0; t < kNarrowTrips; ++t) v[t] = 0;
      if (n_src_rows > 0) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          if (j >= seg) break;
#pragma unroll
          for (int t = 0; t < kNarrowTrips; ++t) v[t] |= static_cast<uint32_t>(static_cast<uint8_t>(src[start[t] + j])) << (8 * j);
        }
      }
#pragma unroll
      for (int t = 0; t < kNarrowTrips; ++t) {
        const int r = tid + t * kPartsBlock;
        const uint32_t value = (read_mask >> t) & 1u ? v[t] : 0u;
        uint8_t* at = image + r * W + (r >> 4) * kPartSkew + o;
#pragma unroll
        for (int j = 0; j < 3; ++j)
          if (j < seg) at[j] = static_cast<uint8_t>(value >> (8 * j));
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int u = t * kPartsBlock + thread;  // a 16-byte word of dst: (tile, individual, part of the tile)
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
void launch_tile_parts(int log_width, dim3 grid, hipStream_t st, const PartList& parts, int32_t n_parts, int32_t n_ind, int64_t n_rows,
                       int64_t n_tiles, int8_t* dst, int32_t* n_bad) {
  if constexpr (LW < kMaxLogWidth) {
    if (log_width != LW) return launch_tile_parts<LW + 1>(log_width, grid, st, parts, n_parts, n_ind, n_rows, n_tiles, dst, n_bad);
  }
  hipLaunchKernelGGL((tile_parts_kernel<LW>), grid, dim3(kPartsBlock), 0, st, parts, n_parts, n_ind, n_rows, n_tiles, dst, n_bad);
}

}  // namespace

extern "C" {

int sai_tile_parts_abi_version(void) { return kTilePartsAbiVersion; }

int sai_tile_rows_from_parts(sai_ctx* ctx, int32_t n_parts, const sai_tile_part* parts_host, int64_t n_rows, int32_t n_ind, int8_t* dst,
                             int32_t* n_bad, void* stream) {
  if (int rc = enter(ctx)) return rc;
  if (n_parts < 1 || n_parts > SAI_TILE_MAX_PARTS) return fail(SAI_ERR_ARG, "n_parts %d is outside 1..%d", n_parts, SAI_TILE_MAX_PARTS);
  if (n_ind < 0 || n_rows < 0) return fail(SAI_ERR_ARG, "negative size");
  if (!parts_host || !n_bad) return fail(SAI_ERR_ARG, "NULL buffer");
  PartList parts = {};
#pragma nounroll
  for (int p = 0; p < n_parts; ++p) {
    const sai_tile_part& part = parts_host[p];
    if (part.n_src_rows < 0 || part.n_ind < 0 || part.ind0 < 0) return fail(SAI_ERR_ARG, "negative size");
    if (part.row_stride < part.n_ind) return fail(SAI_ERR_ARG, "row_stride %lld < n_ind %d", (long long)part.row_stride, part.n_ind);
    if (!part.rows && part.n_ind > 0 && n_rows != part.n_src_rows)
      return fail(SAI_ERR_ARG, "rows is NULL (the identity) but n_rows %lld != n_src_rows %lld", (long long)n_rows, (long long)part.n_src_rows);
    parts.p[p] = part;
  }
  // the parts cover [0, n_ind) exactly once: walked in the order of their first individual (a part of no individual owns nothing)
  int64_t covered = 0;
  for (int done = 0; done < n_parts; ++done) {
    int next = -1;
    for (int p = 0; p < n_parts; ++p)
      if (parts.p[p].ind0 >= covered && parts.p[p].n_ind > 0 && (next < 0 || parts.p[p].ind0 < parts.p[next].ind0)) next = p;
    if (next < 0) break;
    if (parts.p[next].ind0 != covered) break;
    covered += parts.p[next].n_ind;
  }
  int64_t total = 0;
  for (int p = 0; p < n_parts; ++p) total += parts.p[p].n_ind;
  if (covered != n_ind || total != n_ind)
    return fail(SAI_ERR_ARG, "the parts overlap or leave a gap: they hold %lld individuals and cover 0 .. %lld of %d", (long long)total,
                (long long)covered, n_ind);
  hipStream_t st = static_cast<hipStream_t>(stream);
  SAI_HIP(hipMemsetAsync(n_bad, 0, sizeof(int32_t), st));
  if (n_rows == 0 || n_ind == 0) return SAI_OK;
  if (!dst) return fail(SAI_ERR_ARG, "NULL buffer");
  for (int p = 0; p < n_parts; ++p)
    if (!parts.p[p].src && parts.p[p].n_ind > 0 && parts.p[p].n_src_rows > 0) return fail(SAI_ERR_ARG, "NULL buffer");
  if (reinterpret_cast<uintptr_t>(dst) & 15) return fail(SAI_ERR_ARG, "dst is not 16-byte aligned");
  int log_width = kMinLogWidth;  // the narrowest workgroup that takes the population in one column block, else the widest
  while (log_width < kMaxLogWidth && (1 << log_width) < n_ind) ++log_width;
  const int64_t n_tiles = (n_rows + kTile - 1) / kTile;
  const int64_t tiles_per_group = kPartsBlock >> log_width;
  const int64_t n_groups = (n_tiles + tiles_per_group - 1) / tiles_per_group;
  const int64_t n_blk = (static_cast<int64_t>(n_ind) + (1 << log_width) - 1) >> log_width;
  if (n_groups > 0x7FFFFFFFll || n_blk > 65535) return fail(SAI_ERR_UNSUPPORTED, "block too large for one launch");
  dim3 grid(static_cast<unsigned>(n_groups), static_cast<unsigned>(n_blk));
  launch_tile_parts<kMinLogWidth>(log_width, grid, st, parts, n_parts, n_ind, n_rows, n_tiles, dst, n_bad);
  return check_launch("tile_rows_from_parts");
}

}  // extern "C"
