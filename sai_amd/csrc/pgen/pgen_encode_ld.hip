// sai_pgen_encode_ld: sai_pgen_encode with the record types 2 and 3 -- a row as its differences from an earlier row
// (pgen_export_ld.hpp has the rule; its plain statement is pgen_encode_ld_host.cpp, and these kernels make the same
// decisions).  What a row may use depends on the types of the rows before it; the rule cuts that chain every 16 rows,
// so the chain is walked by one wavefront and the launch is parallel over segments.
//
//  * plan -- one wavefront (one 64-lane workgroup) per segment of 16 rows, which it walks in order.  A row is recoded
//    into an LDS tile as pgen_encode.hip's plan does (pgen_encode_device.hpp); a second tile holds the dense words of
//    the current base row.  For a row that is no anchor one more pass over the two tiles gives the entry counts of
//    the types 2 and 3 -- popcounts over the XOR of the row's word and the base's (for type 3 the base's with 0 and 2
//    exchanged) -- and the candidates are sized in ascending type order under the short cut of pgen_encode.hip: one
//    whose L has 5 L >= 4 * (best so far) is more than the best and is skipped.  A row whose type is neither 2 nor 3
//    becomes the base of the rows behind it: the two tiles change roles, nothing is copied.
//  * scan -- sai_pgen_encode's own, through that entry point.
//  * write -- one wavefront per row.  A row of type 2 or 3 finds its base by looking back through vrtype, at most to
//    the first row of its segment (15 entries), recodes both rows from the block, counts the entries and writes the
//    difflist through the routine the plan sized it with; every other row is written as pgen_encode.hip writes it.
//    Every store is checked against the record's planned length.
//
// Rows wider than the tile (more than 16 384 samples): the words behind the tile are recoded again from the block in
// every pass, for the base row too.  LDS: 13.5 KiB per plan wavefront (two tiles of 4 KiB and the entry buffer), 5.5 KiB
// per write wavefront.  The plan grid is capped at 16 wavefronts per CU over segments, the write grid over rows.
// Registers, LDS, occupancy and scratch (0 bytes): DESIGN_INGEST.md.

#include "pgen_encode_device.hpp"
#include "pgen_export_ld.hpp"

namespace {

constexpr int kSegment = SAI_PGEN_LD_SEGMENT;

// the entries a type 2 and a type 3 record of the row would list against the base (to every lane)
__device__ __forceinline__ void count_differing(const EncodeArgs& a, const RowView& v, const RowView& bv, uint32_t* l2, uint32_t* l3) {
  uint32_t d2 = 0, d3 = 0;
  for (uint32_t i = threadIdx.x; i < a.n_words; i += kWave) {
    const uint32_t codes = view_word(a, v, i), base = view_word(a, bv, i), valid = valid_fields(a.n, i);
    d2 += __popc(differing_fields(codes, base, valid, 2u));
    d3 += __popc(differing_fields(codes, base, valid, 3u));
  }
  *l2 = wave_sum(d2);
  *l3 = wave_sum(d3);
}

__global__ __launch_bounds__(kWave) void pgen_ld_plan_kernel(EncodeArgs a, int64_t n_segments) {
  __shared__ uint32_t tiles[2][kTileWords];
  __shared__ uint32_t ent_idx[kEntCap];
  __shared__ uint8_t ent_code[kEntCap];
  const int lane = threadIdx.x;
  for (int64_t seg = blockIdx.x; seg < n_segments; seg += gridDim.x) {
    const int64_t first = seg * kSegment;
    const int64_t end = first + kSegment < a.n_rows ? first + kSegment : a.n_rows;
    uint32_t cur = 0;     // the tile the row is recoded into; the other holds the base
    int64_t base_at = 0;  // where the base row starts in the block
#pragma unroll 1
    for (int64_t row = first; row < end; ++row) {
      const int64_t row_at = row * a.n;
      uint32_t count[4];
      int32_t st;
      count_row(a, row_at, tiles[cur], count, &st);
      __syncthreads();
      uint32_t lo, hi;
      pgen_onebit_pair(count, &lo, &hi);
      const RowView view{row_at, tiles[cur]}, base{base_at, tiles[cur ^ 1u]};
      const bool anchor = row == first;
      uint32_t l2 = 0, l3 = 0;
      if (!anchor) count_differing(a, view, base, &l2, &l3);
      uint32_t best = a.row_bytes, best_kind = 0;
#pragma unroll 1
      for (uint32_t kind = 1; kind <= 7; ++kind) {  // ascending types: a tie stays with the lower
        if (kind == 5 || (anchor && (kind == 2 || kind == 3))) continue;
        const uint32_t L = kind == 2 ? l2 : kind == 3 ? l3 : entries_of(a.n, count, kind, lo, hi);
        if (5ull * L >= 4ull * best) continue;  // more than 5 L / 4 bytes: larger than the best
        uint32_t size = size_or_write_difflist_of<false, true>(a, view, base, kind, lo, hi, L, nullptr, 0u, 0u, ent_idx, ent_code);
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
      if (best_kind != 2 && best_kind != 3) {  // the base of the rows behind it: the tiles change roles
        cur ^= 1u;
        base_at = row_at;
      }
      __syncthreads();  // the next row overwrites a tile
    }
  }
}

__global__ __launch_bounds__(kWave) void pgen_ld_write_kernel(EncodeArgs a) {
  __shared__ uint32_t ent_idx[kEntCap];
  __shared__ uint8_t ent_code[kEntCap];
  for (int64_t row = blockIdx.x; row < a.n_rows; row += gridDim.x) {
    const int64_t row_at = row * a.n;
    const uint32_t kind = a.vrtype[row], room = a.length[row];
    uint8_t* rec = a.out + a.offsets[row];
    const RowView view{row_at, nullptr};
    RowView base = view;
    uint32_t lo = 0, hi = 0, L, at = 0;
    if (kind == 2 || kind == 3) {
      // the base: the nearest earlier row of the segment of another type; never before the segment's first row
      const int64_t first = row - row % kSegment;
      int64_t b = row;
      while (b > first) {
        --b;
        const uint32_t t = a.vrtype[b];
        if (t != 2 && t != 3) break;
      }
      base.row_at = b * a.n;
      uint32_t l2, l3;
      count_differing(a, view, base, &l2, &l3);
      L = kind == 2 ? l2 : l3;
    } else if (!write_record_head(a, row_at, kind, rec, room, &lo, &hi, &L, &at)) {
      continue;
    }
    size_or_write_difflist_of<true, true>(a, view, base, kind, lo, hi, L, rec, room, at, ent_idx, ent_code);
  }
}

}  // namespace

extern "C" int sai_pgen_encode_ld(sai_ctx* ctx, const int8_t* dosage, int64_t n_rows, int32_t n_slots, const int32_t* ploidy_of_slot,
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
  const int64_t cap = sai_pgen_encode_grid_cap(ctx);
  if (stages & SAI_PGEN_ENCODE_PLAN) {  // a wavefront per segment; beyond the 16 per CU segments are taken in a grid stride
    const int64_t n_segments = (n_rows + kSegment - 1) / kSegment;
    hipLaunchKernelGGL(pgen_ld_plan_kernel, dim3(static_cast<unsigned>(n_segments < cap ? n_segments : cap)), dim3(kWave), 0, st, a, n_segments);
    if (int rc = check_launch("pgen_ld_plan")) return rc;
  }
  if (stages & SAI_PGEN_ENCODE_SCAN) {
    if (int rc = sai_pgen_encode(ctx, dosage, n_rows, n_slots, ploidy_of_slot, uniform_ploidy, out, vrtype, length, offsets, status, SAI_PGEN_ENCODE_SCAN, stream))
      return rc;
  }
  if (stages & SAI_PGEN_ENCODE_WRITE) {  // a wavefront per row
    hipLaunchKernelGGL(pgen_ld_write_kernel, dim3(static_cast<unsigned>(n_rows < cap ? n_rows : cap)), dim3(kWave), 0, st, a);
    if (int rc = check_launch("pgen_ld_write")) return rc;
  }
  return SAI_OK;
}
