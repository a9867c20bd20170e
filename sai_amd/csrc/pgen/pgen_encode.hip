// sai_pgen_encode: int8 dosages [row][slot] in HBM -> the hard-call records of a PLINK 2 .pgen, back to back in row
// order: the inverse of sai_pgen_decode (pgen_export.hpp has the table and the size rules; the plain statement of
// them is pgen_encode_host.cpp, and these kernels make the same decisions).  Three kernels:
//
//  * plan -- one wavefront (one 64-lane workgroup, as pgen_decode.hip) per row.  A lane takes 16 samples at a time:
//    the row starts at any byte of the block, so it loads the two aligned 128-bit words that hold its 16 dosages and
//    funnel-shifts them into place (as plink/bed_encode.hip does), then recodes four dosages at a time by bit
//    operations into one 32-bit word of 2-bit codes -- word i of the row's dense form.  The words stay in LDS (4 KiB,
//    16 384 samples: the decoder's tile), the four code counts come from popcounts, the status from the mask of the
//    values outside the table.  With the counts every candidate's entry count L is known, and a candidate is sized
//    only when 5 L < 4 * (best size so far): a difflist of L entries takes more than 5 L / 4 bytes (a code quarter
//    and at least one delta or index byte per entry), so a skipped candidate is strictly larger than the best and can
//    neither win nor tie.  The dense size ceil(n / 4) is the first best, so L < n / 5 for every candidate that is
//    sized: at most one of types 4 / 6 / 7, and type 1.  Sizing walks the words again, from LDS.
//  * scan -- one workgroup: the exclusive prefix sum of the lengths, the record offsets of the call and their total.
//  * write -- one wavefront per row again: it recodes the row as the plan kernel does, counts it again for L and the
//    pair of a type 1 record, and writes the record at its offset.  Records start at any byte, so everything but the
//    whole words of a 4-byte aligned dense record is stored byte by byte, and every store is checked against the
//    record's planned length: a disagreement between the two kernels could shorten a record, never leave it.
//
// The recoding, the counts and the difflist (size_or_write_difflist, shared by both kernels, so that they cannot
// disagree) are in pgen_encode_device.hpp, which sai_pgen_encode_ld's kernels (pgen_encode_ld.hip) use as well.
//
// Rows wider than the tile (more than 16 384 samples): the words behind the tile are not kept -- every later pass
// loads and recodes them again from the block, which the first pass left in L2.  Slower per sample, same bytes.
// LDS: 9.5 KiB per plan wavefront, 5.5 KiB per write wavefront.  Grids are capped at 16 wavefronts per CU; beyond,
// rows are taken in a grid stride.  Registers, LDS, occupancy and scratch (0 bytes): DESIGN_INGEST.md.

#include "pgen_encode_device.hpp"

namespace {

constexpr int kScanBlock = 1024;

__global__ __launch_bounds__(kWave) void pgen_plan_kernel(EncodeArgs a) {
  __shared__ uint32_t tile[kTileWords];
  __shared__ uint32_t ent_idx[kEntCap];
  __shared__ uint8_t ent_code[kEntCap];
  const int lane = threadIdx.x;
  for (int64_t row = blockIdx.x; row < a.n_rows; row += gridDim.x) {
    const int64_t row_at = row * a.n;
    uint32_t count[4];
    int32_t st;
    count_row(a, row_at, tile, count, &st);
    __syncthreads();
    uint32_t lo, hi;
    pgen_onebit_pair(count, &lo, &hi);
    const RowView view{row_at, tile};
    uint32_t best = a.row_bytes, best_kind = 0;
#pragma unroll 1
    for (int c = 0; c < 4; ++c) {  // ascending types: a tie stays with the lower
      const uint32_t kind = c == 0 ? 1u : c == 1 ? 4u : c == 2 ? 6u : 7u;
      const uint32_t L = entries_of(a.n, count, kind, lo, hi);
      if (5ull * L >= 4ull * best) continue;  // more than 5 L / 4 bytes: larger than the best
      uint32_t size = size_or_write_difflist<false>(a, view, kind, lo, hi, L, nullptr, 0u, 0u, ent_idx, ent_code);
      if (kind == 1) size += 1u + (a.n + 7u) / 8u;  // n < 5 * 2^29 / 4 here: no overflow
      if (size < best) {
        best = size;
        best_kind = kind;
      }
    }
    if (lane == 0) {
      a.vrtype[row] = static_cast<uint8_t>(best_kind);
      a.length[row] = best;
      a.status[row] = st;
    }
    __syncthreads();  // the next row overwrites the tile
  }
}

// offsets[r] = length[0] + .. + length[r - 1], offsets[n_rows] = their total (less than 2^32: the entry point checked
// the dense bound): one workgroup, a chunk of its size at a time.
__global__ __launch_bounds__(kScanBlock) void pgen_scan_kernel(const uint32_t* length, int64_t n_rows, uint32_t* offsets) {
  __shared__ uint32_t wave_total[kScanBlock / kWave];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  uint32_t carry = 0;
  for (int64_t r0 = 0; r0 < n_rows; r0 += kScanBlock) {
    const int64_t r = r0 + tid;
    const uint32_t v = r < n_rows ? length[r] : 0u;
    const uint32_t incl = wave_inclusive_sum(v, lane);
    if (lane == kWave - 1) wave_total[wave] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (int k = 0; k < kScanBlock / kWave; ++k) {
      const uint32_t t = wave_total[k];
      if (k < wave) before += t;
      all += t;
    }
    if (r < n_rows) offsets[r] = carry + before + (incl - v);
    carry += all;
    __syncthreads();
  }
  if (tid == 0) offsets[n_rows] = carry;
}

__global__ __launch_bounds__(kWave) void pgen_write_kernel(EncodeArgs a) {
  __shared__ uint32_t ent_idx[kEntCap];
  __shared__ uint8_t ent_code[kEntCap];
  for (int64_t row = blockIdx.x; row < a.n_rows; row += gridDim.x) {
    const int64_t row_at = row * a.n;
    const uint32_t kind = a.vrtype[row], room = a.length[row];
    uint8_t* rec = a.out + a.offsets[row];
    uint32_t lo, hi, L, at;
    if (!write_record_head(a, row_at, kind, rec, room, &lo, &hi, &L, &at)) continue;
    const RowView view{row_at, nullptr};
    size_or_write_difflist<true>(a, view, kind, lo, hi, L, rec, room, at, ent_idx, ent_code);
  }
}

}  // namespace

extern "C" int64_t sai_pgen_encode_grid_cap(sai_ctx* ctx) { return ctx ? static_cast<int64_t>(ctx->n_cu) * kWavesPerCu : -1; }

extern "C" int sai_pgen_encode(sai_ctx* ctx, const int8_t* dosage, int64_t n_rows, int32_t n_slots, const int32_t* ploidy_of_slot,
                               int32_t uniform_ploidy, uint8_t* out, uint8_t* vrtype, uint32_t* length, uint32_t* offsets, int32_t* status,
                               int32_t stages, void* stream) {
  if (int rc = enter(ctx)) return rc;
  if (n_rows < 0 || n_slots < 1) return fail(SAI_ERR_ARG, "size out of range: a .pgen record holds 1 to 2^31 - 1 samples");
  if (uniform_ploidy < 0 || uniform_ploidy > 2) return fail(SAI_ERR_ARG, "uniform_ploidy must be 0, 1 or 2");
  if (stages < 1 || stages > SAI_PGEN_ENCODE_ALL) return fail(SAI_ERR_ARG, "stages must be 1 .. 7");
  const int64_t row_bytes = (static_cast<int64_t>(n_slots) + 3) / 4;
  if (n_rows > (int64_t(0xFFFFFFFFll) - 16) / row_bytes) return fail(SAI_ERR_ARG, "size out of range: a call writes less than 4 GiB of records");
  if (!offsets) return fail(SAI_ERR_ARG, "NULL buffer");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (n_rows == 0) {
    SAI_HIP(hipMemsetAsync(offsets, 0, sizeof(uint32_t), st));
    return SAI_OK;
  }
  if (!dosage || !out || !vrtype || !length || !status || (uniform_ploidy == 0 && !ploidy_of_slot)) return fail(SAI_ERR_ARG, "NULL buffer");
  if (reinterpret_cast<uintptr_t>(dosage) & 15u) return fail(SAI_ERR_ARG, "dosage must be 16-byte aligned");
  const EncodeArgs a = encode_args(dosage, n_rows, n_slots, ploidy_of_slot, uniform_ploidy, out, vrtype, length, offsets, status);
  // a wavefront per row; beyond the 16 per CU rows are taken in a grid stride
  const int64_t cap = sai_pgen_encode_grid_cap(ctx);
  const dim3 grid(static_cast<unsigned>(n_rows < cap ? n_rows : cap));
  if (stages & SAI_PGEN_ENCODE_PLAN) {
    hipLaunchKernelGGL(pgen_plan_kernel, grid, dim3(kWave), 0, st, a);
    if (int rc = check_launch("pgen_plan")) return rc;
  }
  if (stages & SAI_PGEN_ENCODE_SCAN) {
    hipLaunchKernelGGL(pgen_scan_kernel, dim3(1), dim3(kScanBlock), 0, st, static_cast<const uint32_t*>(length), n_rows, offsets);
    if (int rc = check_launch("pgen_scan")) return rc;
  }
  if (stages & SAI_PGEN_ENCODE_WRITE) {
    hipLaunchKernelGGL(pgen_write_kernel, grid, dim3(kWave), 0, st, a);
    if (int rc = check_launch("pgen_write")) return rc;
  }
  return SAI_OK;
}
