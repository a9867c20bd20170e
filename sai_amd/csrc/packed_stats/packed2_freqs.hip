// sai_packed2_site_freqs: per-site allele frequencies (f64) of up to nine populations straight from their packed2
// blocks (include/saihip_packed_stats.h) -- the site half of fd / df / Danc / Dplus in the 2-bit layout;
// sai_window_fourpop (../fourpop.hip) takes the frequencies as they are.
//
// The loop is site_counts_packed2_kernel's (../packed2.hip): one single-wave workgroup per tile of 64 sites, lane =
// site, per population 16-byte non-temporal loads of the full groups (kUnroll in flight; a remainder of 2 .. kUnroll - 1
// groups as one batch), the tail group's 1..4 words, the three codes counted with popcounts into registers of the
// lane.  What follows is site_freqs_kernel's divide (../fourpop.hip) on values the lane already holds:
// double(ones + 2 * twos) / double(int64(n_ind - missing) * ploidy), both operands exact integers, so the quotient is
// the one the two existing launches give -- without the 8 bytes of counts per population and site that they write and
// read back, and for nine populations (ref, tgt, SAI_FUSED_SRC sources, outgroup) where the site pass takes eight.
// Each population ends in one 8-byte store per lane: 512 contiguous bytes per wave.  No LDS, no cross-lane step.
// A wave reads whole tiles (the padding sites of the last tile belong to the block) and stores only sites < n_sites.

#include "../common.hpp"
#include "packed2_freqs_args.hpp"

namespace {

constexpr int kUnroll = 8;  // wave loads in flight per batch, as in ../packed2.hip

struct FreqPop {
  const uint32_t* data;
  int32_t n_ind;
  int32_t n_full;  // full groups of 64 individuals
  int32_t w_tail;  // words per site of the tail group (0..4)
  int32_t ploidy;
};

struct PackedFreqArgs {
  int64_t n_sites;
  int64_t n_tiles;
  int32_t n_pops;
  FreqPop pop[SAI_PACKED_FREQ_POPS];
  double* freqs;
};

__device__ __forceinline__ void count_codes(const u32x4& v, uint32_t& ones, uint32_t& twos, uint32_t& miss) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t lo = w[j] & 0x55555555u, hi = (w[j] >> 1) & 0x55555555u;
    ones += __popc(lo & ~hi);
    twos += __popc(hi & ~lo);
    miss += __popc(lo & hi);
  }
}

__global__ __launch_bounds__(64) void packed2_site_freqs_kernel(PackedFreqArgs a) {
  const int lane = threadIdx.x;
  for (int64_t tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
    const int64_t site = tile * kTile + lane;
    for (int p = 0; p < a.n_pops; ++p) {
      const int n_groups = a.pop[p].n_full, w_tail = a.pop[p].w_tail;
      const uint32_t* tile_words = a.pop[p].data + tile * (static_cast<int64_t>(n_groups) * 256 + w_tail * 64);
      const u32x4* base = reinterpret_cast<const u32x4*>(tile_words) + lane;
      uint32_t ones = 0, twos = 0, miss = 0;
      int g = 0;
      for (; g + kUnroll <= n_groups; g += kUnroll) {
        u32x4 v[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) v[u] = __builtin_nontemporal_load(base + (g + u) * kTile);
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) count_codes(v[u], ones, twos, miss);
      }
      if (g + 1 == n_groups) {  // one full group left: a single load
        count_codes(__builtin_nontemporal_load(base + g * kTile), ones, twos, miss);
      } else if (g < n_groups) {  // 2 .. kUnroll - 1 groups as one batch: clamped addresses, zeroed extras
        u32x4 v[kUnroll - 1];
#pragma unroll
        for (int u = 0; u < kUnroll - 1; ++u) v[u] = __builtin_nontemporal_load(base + min(g + u, n_groups - 1) * kTile);
#pragma unroll
        for (int u = 0; u < kUnroll - 1; ++u) {
          if (g + u >= n_groups) v[u] = u32x4{0u, 0u, 0u, 0u};
          count_codes(v[u], ones, twos, miss);
        }
      }
      if (w_tail) {  // the tail group's words of this lane's site; padding individuals carry code 0
        const uint32_t* tw = tile_words + n_groups * 256 + lane * w_tail;
        u32x4 tail = {0u, 0u, 0u, 0u};
        tail.x = __builtin_nontemporal_load(tw);
        if (w_tail > 1) tail.y = __builtin_nontemporal_load(tw + 1);
        if (w_tail > 2) tail.z = __builtin_nontemporal_load(tw + 2);
        if (w_tail > 3) tail.w = __builtin_nontemporal_load(tw + 3);  // 49..63 individuals
        count_codes(tail, ones, twos, miss);
      }
      const uint32_t alt = ones + 2u * twos, called = static_cast<uint32_t>(a.pop[p].n_ind) - miss;
      const int64_t den = static_cast<int64_t>(called) * a.pop[p].ploidy;
      if (site < a.n_sites)
        a.freqs[static_cast<int64_t>(p) * a.n_sites + site] =
            den > 0 ? static_cast<double>(alt) / static_cast<double>(den) : std::numeric_limits<double>::quiet_NaN();
    }
  }
}

}  // namespace

extern "C" int sai_packed2_site_freqs(sai_ctx* ctx, int64_t n_sites, int32_t n_pops, const sai_pop* pops, double* freqs,
                                      void* stream) {
  if (int rc = enter(ctx)) return rc;
  if (int rc = packed2_freqs_check_sizes(n_sites, n_pops, pops)) return rc;
  if (n_sites == 0) return SAI_OK;
  if (int rc = packed2_freqs_check_pops(n_pops, pops, freqs, true)) return rc;
  PackedFreqArgs a;
  std::memset(&a, 0, sizeof(a));
  a.n_sites = n_sites;
  a.n_tiles = (n_sites + kTile - 1) / kTile;
  a.n_pops = n_pops;
  for (int p = 0; p < n_pops; ++p) {
    a.pop[p].data = reinterpret_cast<const uint32_t*>(pops[p].tiles);
    a.pop[p].n_ind = pops[p].n_ind;
    a.pop[p].n_full = packed2_full_groups(pops[p].n_ind);
    a.pop[p].w_tail = packed2_tail_words(pops[p].n_ind);
    a.pop[p].ploidy = pops[p].ploidy;
  }
  a.freqs = freqs;
  // a memory-bound pass: enough single-wave workgroups to fill the chip, grid-stride beyond that
  const dim3 grid(stream_grid(ctx, a.n_tiles));
  hipLaunchKernelGGL(packed2_site_freqs_kernel, grid, dim3(64), 0, static_cast<hipStream_t>(stream), a);
  return check_launch("packed2_site_freqs");
}
