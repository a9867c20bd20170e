// DD for source populations of any size, the device half (the entry points are stated in dd_table_host.cpp, which also
// holds their host twins and the argument checks).
//
// sai_site_absdiff_table: site_absdiff_kernel's loop (../dd.hip) -- single-wave workgroups, stream_grid() of them and
// grid-strided beyond, 16-byte non-temporal loads with kUnroll in flight, clamped tail loads, the butterfly
// reduce-scatter over the 16 row lanes, non-temporal stores -- with the sums formed as ../site_pass_dd.hip forms
// them: the four words that the four loads in flight hold for the same four sites are transposed in registers (eight
// v_perm_b32) into one word per site with four individuals in it, every byte biased to unsigned (x ^ 0x80), and
// v_sad_u8 against the biased value replicated four times adds the four |v - g| of a site at once.  The source
// is a constant here, so the replicated words are kernel arguments (scalar registers), and up to eight values go in
// one pass.  Two neighbouring sites share an accumulator register as 16-bit fields (the odd site's SAD is shifted
// in): 8 registers per value instead of 16.  A group of four rows adds at most 1020 to a field, so after
// kTableChunkGroups = 64 groups (4 096 individuals) the chunk is closed -- per value the fields are widened, the
// butterfly leaves this lane's ONE site, added to a 32-bit total -- and the fields start empty again.  Rows that do
// not exist (the last group is padded) are loaded as zero words, i.e. as dosages of 0; the |v| each of them adds is
// taken off at the end.  All integers are exact (every result is at most 255 * 2^24 < 2^32).
//
// sai_window_dd_table: window_dd_kernel (../dd.hip) with the term looked up instead of read: one wave per window; per
// source individual the lanes walk the window's sites, read the source's byte (a row of a tile is 64 contiguous
// bytes), find its index among the values and add the two table entries; then window_dd_kernel's reduction, divisions
// and numpy_sum, statement for statement.  A window of up to dd_stage_sites(n_values) sites has its share of both
// tables copied to LDS first, so that the n_src_ind trips over it do not go to memory; a longer one reads the tables
// in place.  The totals are exact integers either way, so both forms give the same doubles.

#include "../numpy_sum.hpp"
#include "../stream_loops.hpp"

#define SAI_DD_TABLE_VALUES 8  // values of one table at most, as dd_table_host.cpp says

// dd_table_host.cpp: the argument checks, shared with the host twins
int sai_dd_table_check_sizes(int64_t n_sites, const sai_pop* pop, int32_t n_values, const int8_t* values);
int sai_dd_table_check_buffers(const sai_pop* pop, const uint32_t* table, bool device);
int sai_dd_window_check(int64_t n_sites, const sai_pop* src, int32_t n_values, const int8_t* values, const uint32_t* table_ref,
                        int32_t n_ref_ind, const uint32_t* table_tgt, int32_t n_tgt_ind, int32_t n_windows, const int32_t* lo,
                        const int32_t* hi, const double* scratch, const double* dd, const int32_t* n_unlisted);

namespace {

// Groups of four rows per lane that the packed 16-bit fields of the streaming kernel absorb: a group adds at most
// 4 * 255 = 1020 to a field, 64 * 1020 = 65 280 < 2^16.  A group is four iterations of 16 rows: a population of more
// than 64 * 4 * 16 = 4 096 individuals closes a chunk (a butterfly per value) and starts the next with empty fields.
constexpr int kTableChunkGroups = 64;
constexpr int kTableGroupIters = 4;
static_assert(kTableChunkGroups * kTableGroupIters * 255 < (1 << 16), "the packed 16-bit fields overflow");
static_assert(kUnroll == kTableGroupIters, "a group is the four loads in flight");

// 32-bit words of LDS in which sai_window_dd_table stages a window's share of both tables: a window of up to
// dd_stage_sites(n_values) sites is staged, a longer one reads the tables in place.
constexpr int kDdStageWords = 8192;
inline int dd_stage_sites(int n_values) { return (kDdStageWords / (2 * n_values)) & ~63; }
constexpr int kTableChunkIters = kTableChunkGroups * kTableGroupIters;

struct TableArgs {
  int64_t n_sites;
  int64_t n_tiles;
  const int8_t* pop_tiles;
  int32_t n_ind;
  int32_t pad;
  uint32_t rep[SAI_DD_TABLE_VALUES];    // the biased value in all four bytes
  uint32_t abs_v[SAI_DD_TABLE_VALUES];  // |value|: what a padding row (dosage 0) adds
  uint32_t* table;                      // [K][n_sites]
};

// bytes b of four words -> four words of one byte position each: t[b] = {w0.b, w1.b, w2.b, w3.b} (../site_pass_dd.hip)
__device__ __forceinline__ void transpose4(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t (&t)[4]) {
  const uint32_t a_lo = __builtin_amdgcn_perm(w1, w0, 0x05010400u);  // w0.b0 w1.b0 w0.b1 w1.b1
  const uint32_t a_hi = __builtin_amdgcn_perm(w1, w0, 0x07030602u);  // w0.b2 w1.b2 w0.b3 w1.b3
  const uint32_t b_lo = __builtin_amdgcn_perm(w3, w2, 0x05010400u);
  const uint32_t b_hi = __builtin_amdgcn_perm(w3, w2, 0x07030602u);
  t[0] = __builtin_amdgcn_perm(b_lo, a_lo, 0x05040100u);
  t[1] = __builtin_amdgcn_perm(b_lo, a_lo, 0x07060302u);
  t[2] = __builtin_amdgcn_perm(b_hi, a_hi, 0x05040100u);
  t[3] = __builtin_amdgcn_perm(b_hi, a_hi, 0x07060302u);
}

// one group: four rows of this lane's 16 sites.  acc[k][i] holds sites 2 i (low field) and 2 i + 1 (high field).
template <int K>
__device__ __forceinline__ void table_group(const u32x4 (&v)[kUnroll], uint32_t (&acc)[K][8], const TableArgs& a) {
  const uint32_t w[4][4] = {{v[0].x, v[0].y, v[0].z, v[0].w}, {v[1].x, v[1].y, v[1].z, v[1].w},
                            {v[2].x, v[2].y, v[2].z, v[2].w}, {v[3].x, v[3].y, v[3].z, v[3].w}};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    uint32_t t[4];
    transpose4(w[0][j] ^ 0x80808080u, w[1][j] ^ 0x80808080u, w[2][j] ^ 0x80808080u, w[3][j] ^ 0x80808080u, t);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      acc[k][2 * j] = __builtin_amdgcn_sad_u8(t[0], a.rep[k], acc[k][2 * j]);
      acc[k][2 * j] += __builtin_amdgcn_sad_u8(t[1], a.rep[k], 0u) << 16;
      acc[k][2 * j + 1] = __builtin_amdgcn_sad_u8(t[2], a.rep[k], acc[k][2 * j + 1]);
      acc[k][2 * j + 1] += __builtin_amdgcn_sad_u8(t[3], a.rep[k], 0u) << 16;
    }
  }
}

template <int K>
__global__ __launch_bounds__(64) void site_absdiff_table_kernel(TableArgs a) {
  const int lane = threadIdx.x;
  const int r = lane >> 2;
  const int n_full = a.n_ind >> 4;         // iterations in which all 16 rows exist
  const int n_iter = (a.n_ind + 15) >> 4;  // plus at most one partial iteration
  for (int64_t tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
    const u32x4* base = reinterpret_cast<const u32x4*>(a.pop_tiles + tile * static_cast<int64_t>(a.n_ind) * kTile) + lane;
    uint32_t total[K];
#pragma unroll
    for (int k = 0; k < K; ++k) total[k] = 0;
    int it = 0, slots = 0;
    while (it < n_iter) {  // chunks the 16-bit fields can absorb
      uint32_t acc[K][8];
#pragma unroll
      for (int k = 0; k < K; ++k)
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[k][i] = 0;
      const int chunk_end = min(n_iter, it + kTableChunkIters);
      const int full_end = min(n_full, chunk_end);
      for (; it + kUnroll <= full_end; it += kUnroll) {
        u32x4 v[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) v[u] = __builtin_nontemporal_load(base + (it + u) * 64);
        table_group<K>(v, acc, a);
      }
      slots = it;
      if (chunk_end == n_iter && it < n_iter) {  // the last one to four iterations as ONE batch of clamped loads; rows that do not exist become zero words
        u32x4 v[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          const int row = min(it + u, n_iter - 1) * 16 + r;
          v[u] = __builtin_nontemporal_load(base + (min(row, a.n_ind - 1) - r) * 4);
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u)
          if (!((it + u < n_iter) && ((it + u) * 16 + r < a.n_ind))) v[u] = u32x4{0u, 0u, 0u, 0u};
        table_group<K>(v, acc, a);
        slots = it + kUnroll;
        it = n_iter;
      }
#pragma unroll
      for (int k = 0; k < K; ++k) {  // close the chunk: this lane's site of every value
        uint32_t wide[16];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          wide[2 * i] = acc[k][i] & 0xFFFFu;
          wide[2 * i + 1] = acc[k][i] >> 16;
        }
        reduce_scatter_step<16, 32>(wide, lane);
        reduce_scatter_step<8, 16>(wide, lane);
        reduce_scatter_step<4, 8>(wide, lane);
        reduce_scatter_step<2, 4>(wide, lane);
        total[k] += wide[0];
      }
    }
    const uint32_t pad_rows = 16u * static_cast<uint32_t>(slots) - static_cast<uint32_t>(a.n_ind);
    const int64_t site = tile * kTile + (lane & 3) * 16 + r;
    if (site < a.n_sites) {
#pragma unroll
      for (int k = 0; k < K; ++k)
        __builtin_nontemporal_store(total[k] - pad_rows * a.abs_v[k], a.table + static_cast<int64_t>(k) * a.n_sites + site);
    }
  }
}

template <int K>
int launch_table(sai_ctx* ctx, const TableArgs& a, hipStream_t st) {
  hipLaunchKernelGGL((site_absdiff_table_kernel<K>), dim3(stream_grid(ctx, a.n_tiles)), dim3(64), 0, st, a);
  return check_launch("site_absdiff_table");
}

struct WindowTableArgs {
  int64_t n_sites;
  const int8_t* src_tiles;
  int32_t n_src_ind;
  int32_t n_values;
  int32_t value[SAI_DD_TABLE_VALUES];  // unused slots hold a number no byte has
  const uint32_t* table_ref;           // [n_values][n_sites]
  const uint32_t* table_tgt;
  int32_t n_ref_ind;
  int32_t n_tgt_ind;
  int32_t n_windows;
  int32_t stage_sites;  // dd_stage_sites(n_values)
  const int32_t* lo;
  const int32_t* hi;
  double* scratch;  // [n_windows][n_src_ind]
  double* dd;       // [n_windows]
  int32_t* n_unlisted;
};

struct ScratchElemT {
  const double* p;
  __device__ __forceinline__ double operator()(int i) const { return p[i]; }
};

__device__ __forceinline__ int value_index(int g, const WindowTableArgs& a) {
  int k = -1;
#pragma unroll
  for (int q = 0; q < SAI_DD_TABLE_VALUES; ++q) k = (g == a.value[q]) ? q : k;
  return k;
}

template <bool STAGED>
__device__ __forceinline__ void window_rows(const WindowTableArgs& a, int lo, int hi, int lane, const uint32_t* ref, const uint32_t* tgt,
                                            int64_t stride, double* d, long long& unlisted) {
  // ref / tgt: entry of value k at site i is ref[k * stride + i - (STAGED ? lo : 0)]
  const int shift = STAGED ? lo : 0;
  for (int s = 0; s < a.n_src_ind; ++s) {
    long long tr = 0, tt = 0;
    for (int i = lo + lane; i < hi; i += 64) {
      const int g = a.src_tiles[(static_cast<int64_t>(i >> 6) * a.n_src_ind + s) * kTile + (i & 63)];
      const int k = value_index(g, a);
      if (k >= 0) {
        tr += ref[k * stride + (i - shift)];
        tt += tgt[k * stride + (i - shift)];
      } else {
        ++unlisted;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      tr += __shfl_xor(tr, o, 64);
      tt += __shfl_xor(tt, o, 64);
    }
    if (lane == 0)  // np.mean(cdist(...), axis=1): exact integer sums, one division each
      d[s] = static_cast<double>(tr) / static_cast<double>(a.n_ref_ind) - static_cast<double>(tt) / static_cast<double>(a.n_tgt_ind);
  }
}

__global__ __launch_bounds__(64) void window_dd_table_kernel(WindowTableArgs a) {
  __shared__ uint32_t stage[kDdStageWords];
  const int lane = threadIdx.x;
  const int w = blockIdx.x;
  // the caller's ranges, clamped into the block
  const int lo = static_cast<int>(min(max(static_cast<int64_t>(a.lo[w]), int64_t{0}), a.n_sites));
  const int hi = static_cast<int>(min(max(static_cast<int64_t>(a.hi[w]), int64_t{0}), a.n_sites));
  double* d = a.scratch + static_cast<int64_t>(w) * a.n_src_ind;
  long long unlisted = 0;
  if (hi - lo <= a.stage_sites) {  // wave-uniform; an empty or reversed window stages nothing
    const int cap = a.stage_sites;
    uint32_t* stage_tgt = stage + a.n_values * cap;
    for (int k = 0; k < a.n_values; ++k)
      for (int i = lo + lane; i < hi; i += 64) {
        stage[k * cap + (i - lo)] = a.table_ref[static_cast<int64_t>(k) * a.n_sites + i];
        stage_tgt[k * cap + (i - lo)] = a.table_tgt[static_cast<int64_t>(k) * a.n_sites + i];
      }
    __syncthreads();
    window_rows<true>(a, lo, hi, lane, stage, stage_tgt, cap, d, unlisted);
  } else {
    window_rows<false>(a, lo, hi, lane, a.table_ref, a.table_tgt, a.n_sites, d, unlisted);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) unlisted += __shfl_xor(unlisted, o, 64);
  if (lane == 0) {
    __threadfence_block();
    ScratchElemT e{d};
    a.dd[w] = numpy_sum(e, 0, a.n_src_ind) / static_cast<double>(a.n_src_ind);  // np.mean over the individuals
    if (unlisted > 0) {  // rare: a saturating add, so that no number of them wraps the counter to zero
      const int add = static_cast<int>(min(unlisted, static_cast<long long>(0x7FFFFFFF)));
      int seen = *a.n_unlisted;
      for (;;) {
        const int want = seen > 0x7FFFFFFF - add ? 0x7FFFFFFF : seen + add;
        const int prev = atomicCAS(a.n_unlisted, seen, want);
        if (prev == seen) break;
        seen = prev;
      }
    }
  }
}

}  // namespace

// ------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------

extern "C" {

int sai_site_absdiff_table(sai_ctx* ctx, int64_t n_sites, const sai_pop* pop, int32_t n_values, const int8_t* values, uint32_t* table,
                           void* stream) {
  if (int rc = enter(ctx)) return rc;
  if (int rc = sai_dd_table_check_sizes(n_sites, pop, n_values, values)) return rc;
  if (n_sites == 0) return SAI_OK;
  if (int rc = sai_dd_table_check_buffers(pop, table, true)) return rc;
  TableArgs a;
  std::memset(&a, 0, sizeof(a));
  a.n_sites = n_sites;
  a.n_tiles = (n_sites + kTile - 1) / kTile;
  a.pop_tiles = pop->tiles;
  a.n_ind = pop->n_ind;
  for (int k = 0; k < n_values; ++k) {
    a.rep[k] = 0x01010101u * (static_cast<uint32_t>(static_cast<uint8_t>(values[k])) ^ 0x80u);
    a.abs_v[k] = static_cast<uint32_t>(values[k] < 0 ? -static_cast<int>(values[k]) : static_cast<int>(values[k]));
  }
  a.table = table;
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (n_values) {
    case 1: return launch_table<1>(ctx, a, st);
    case 2: return launch_table<2>(ctx, a, st);
    case 3: return launch_table<3>(ctx, a, st);
    case 4: return launch_table<4>(ctx, a, st);
    case 5: return launch_table<5>(ctx, a, st);
    case 6: return launch_table<6>(ctx, a, st);
    case 7: return launch_table<7>(ctx, a, st);
    default: return launch_table<8>(ctx, a, st);
  }
}

int sai_window_dd_table(sai_ctx* ctx, int64_t n_sites, const sai_pop* src, int32_t n_values, const int8_t* values,
                        const uint32_t* table_ref, int32_t n_ref_ind, const uint32_t* table_tgt, int32_t n_tgt_ind, int32_t n_windows,
                        const int32_t* lo, const int32_t* hi, double* scratch, double* dd, int32_t* n_unlisted, void* stream) {
  if (int rc = enter(ctx)) return rc;
  if (int rc = sai_dd_window_check(n_sites, src, n_values, values, table_ref, n_ref_ind, table_tgt, n_tgt_ind, n_windows, lo, hi, scratch, dd,
                               n_unlisted))
    return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  SAI_HIP(hipMemsetAsync(n_unlisted, 0, sizeof(int32_t), st));
  if (n_windows == 0) return SAI_OK;
  WindowTableArgs a;
  std::memset(&a, 0, sizeof(a));
  a.n_sites = n_sites;
  a.src_tiles = src->tiles;
  a.n_src_ind = src->n_ind;
  a.n_values = n_values;
  for (int k = 0; k < SAI_DD_TABLE_VALUES; ++k) a.value[k] = k < n_values ? static_cast<int32_t>(values[k]) : 1000;
  a.table_ref = table_ref;
  a.table_tgt = table_tgt;
  a.n_ref_ind = n_ref_ind;
  a.n_tgt_ind = n_tgt_ind;
  a.n_windows = n_windows;
  a.stage_sites = dd_stage_sites(n_values);
  a.lo = lo;
  a.hi = hi;
  a.scratch = scratch;
  a.dd = dd;
  a.n_unlisted = n_unlisted;
  hipLaunchKernelGGL(window_dd_table_kernel, dim3(static_cast<unsigned>(n_windows)), dim3(64), 0, st, a);
  return check_launch("window_dd_table");
}

}  // extern "C"
