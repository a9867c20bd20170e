// site_counts / site_flags / the fused site pass: the hot kernel of the U / Q path.

#include "site_eval.hpp"
#include "stream_loops.hpp"

namespace {

struct FlagArgs {
  int64_t n_sites;
  int32_t n_pops;
  int16_t n_sets;      // sets of THIS launch
  int16_t with_inv;
  int16_t set0;        // ... which are sets set0 .. set0 + n_sets - 1 of a row of n_row_sets sets
  int16_t n_row_sets;
  int32_t pad;
  int32_t ploidy[kBigPops];
  const uint2* counts;
  double* tgt_freq;
  uint64_t* planes;
  int64_t plane_stride;
  double* adj_freq;
  EvalSets es;
};
static_assert(sizeof(FlagArgs) <= 4096, "kernel arguments exceed the kernarg segment");

// one wavefront per tile (four per workgroup): lane = site inside the tile.  MAXP = kMaxPops: the usual build;
// kBigPops: up to SAI_MAX_SRC sources (table form only; its launcher takes as many sets per launch as the
// table holds).
template <int MAXP>
__global__ __launch_bounds__(256) void site_flags_kernel(FlagArgs a) {
  __shared__ PredTable table;
  stage_pred_table(a.es, &table);
  __syncthreads();
  const int64_t site = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if ((site & ~int64_t{63}) >= a.n_sites) return;  // whole wavefronts beyond the last tile: there is no row for them
  const bool live = site < a.n_sites;              // the last tile's spare lanes vote 0
  eval_site<MAXP>(
      a.n_pops, a.ploidy,
      [&](int p) { return live ? a.counts[static_cast<int64_t>(p) * a.n_sites + site] : make_uint2(0u, 0u); }, a.n_sets,
      a.es, &table, site >> 6, static_cast<int>(threadIdx.x & 63), live, a.n_sites, a.tgt_freq, a.planes, a.plane_stride,
      a.adj_freq, false, a.with_inv != 0, a.set0, a.n_row_sets);
}

// ------------------------------------------------------------------------------------------
// site_counts: the HBM-bound kernel.
//
// One wavefront owns one 64-site tile and streams every population's rows of that tile.  A wave
// instruction loads 16 rows x 64 B = 1 KiB contiguous: lane l holds individual (16*q + l/4),
// sites (l%4)*16 .. +15 as four 32-bit words.  Bytes are accumulated SWAR-style into 16-bit
// (dosage) and 8-bit (missing) fields, widened to 32 bit every <= 248 rows per lane, and the 16
// row-groups are combined with a 4-step butterfly reduce-scatter so that lane l ends with the
// totals of site (l%4)*16 + l/4.  No barriers, no LDS staging of the genotypes (the fused form
// parks each lane's per-population counts in LDS as an indexed register file); 4 KiB of loads in
// flight per wave and 4 waves per SIMD hide HBM latency.
// ------------------------------------------------------------------------------------------

static_assert(sizeof(CountsArgs) + sizeof(FusedArgs) <= 4096, "kernel arguments exceed the kernarg segment");

// The vote of the skipping form: can a condition bit of this lane's site still be up, whatever the target holds?
// eval_site's set-by-set decision for sets polarised by ancestral alleles -- the same f64 quotients and compares --
// without the target's term of `valid`: exactly the sites whose bit is up once the target proves valid, and no others.
template <typename GetCounts>
__device__ __forceinline__ bool target_may_matter(int n_pops, const FusedArgs& fa, GetCounts get, bool live) {
  double f[kMaxPops];
  bool valid = live;
#pragma unroll
  for (int p = 0; p < kMaxPops; ++p) {
    if (p != 1 && p < n_pops) {
      const uint2 c = get(p);
      const int64_t den = static_cast<int64_t>(c.y) * fa.ploidy[p];
      const double v = den > 0 ? static_cast<double>(c.x) / static_cast<double>(den)
                               : std::numeric_limits<double>::quiet_NaN();
      f[p] = v;
      valid = valid && (v >= 0.0) && (v <= 1.0);
    } else {
      f[p] = 0.0;
    }
  }
  const int n_src = n_pops - 2;
  bool may = false;
  for (int s = 0; s < fa.n_sets; ++s) {
    const DevSet& ps = fa.es.sets[s];
    bool hit = true;
#pragma unroll
    for (int k = 0; k < SAI_FUSED_SRC; ++k)
      if (k < n_src) hit = hit && cmp_op(ps.op[k], f[2 + k], ps.y[k]);
    may = may || (hit && (f[0] < ps.w));
  }
  return valid && may;
}

// The first vote of the probing form, taken once a tile's sources are counted: bit s is up iff the sources are valid at
// this lane's site and set s's source comparisons hold -- target_may_matter's quotients and compares without ref's terms.
template <typename GetCounts>
__device__ __forceinline__ uint32_t source_hits(int n_pops, const FusedArgs& fa, GetCounts get, bool live) {
  double f[kMaxPops];
  bool valid = live;
#pragma unroll
  for (int p = 2; p < kMaxPops; ++p) {
    if (p < n_pops) {
      const uint2 c = get(p);
      const int64_t den = static_cast<int64_t>(c.y) * fa.ploidy[p];
      const double v = den > 0 ? static_cast<double>(c.x) / static_cast<double>(den)
                               : std::numeric_limits<double>::quiet_NaN();
      f[p] = v;
      valid = valid && (v >= 0.0) && (v <= 1.0);
    } else {
      f[p] = 0.0;
    }
  }
  const int n_src = n_pops - 2;
  uint32_t hits = 0;
  for (int s = 0; s < fa.n_sets; ++s) {
    const DevSet& ps = fa.es.sets[s];
    bool hit = valid;
#pragma unroll
    for (int k = 0; k < SAI_FUSED_SRC; ++k)
      if (k < n_src) hit = hit && cmp_op(ps.op[k], f[2 + k], ps.y[k]);
    hits |= hit ? 1u << s : 0u;
  }
  return hits;
}

// The second vote: ref's alt sum only grows as rows are added (a missing call adds nothing) and its divisor
// n_called * ploidy is at most n_ref * ploidy, so the final quotient is at least partial_alt / (n_ref * ploidy) -- as
// doubles too: both terms are exact and the division rounds monotonically.  A set whose w that bound has reached is
// out; a site with no set left cannot have a bit up.
__device__ __forceinline__ bool ref_may_pass(const FusedArgs& fa, uint32_t hits, uint32_t partial_alt, int n_ref) {
  const double bound =
      static_cast<double>(partial_alt) / static_cast<double>(static_cast<int64_t>(n_ref) * fa.ploidy[0]);
  bool may = false;
  for (int s = 0; s < fa.n_sets; ++s) may = may || (((hits >> s) & 1u) != 0u && bound < fa.es.sets[s].w);
  return may;
}

// {alt_sum, missing calls} of rows 0 .. n_ind - 1 behind `base`, for site (lane % 4) * 16 + lane / 4.  At most
// 16 * (kChunkIters + 1) rows: one pass, widened once -- and ONE butterfly for both sums.  A whole population of the
// forms that are not MULTI, or a piece of ref in the probing form.
__device__ __forceinline__ uint2 count_piece(const u32x4* base, int n_ind, int r, int lane) {
  const int n_full = n_ind >> 4;
  const int n_iter = (n_ind + 15) >> 4;
  int it = 0;
  uint32_t lo[4] = {0, 0, 0, 0}, hi[4] = {0, 0, 0, 0}, ms[4] = {0, 0, 0, 0};
  accumulate_rows(base, it, n_full, n_full, n_iter, n_ind, r, lo, hi, ms);
  // a site's alt sum stays below 2^20 and its missing count below 2^12 for the at most 3 984 individuals of this
  // form, so the two travel through the butterfly in one word: half of the cross-lane work per population, which
  // is what a tile of NARROW populations is made of (a lone C2: 0.689 against 0.677 of peak; wide populations: the same)
  static_assert(16 * (kChunkIters + 1) * 255 < (1 << 20) && 16 * (kChunkIters + 1) < (1 << 12), "packed butterfly fields overflow");
  uint32_t both[16];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    both[4 * j + 0] = lo[j] & 0xFFFFu;
    both[4 * j + 1] = hi[j] & 0xFFFFu;
    both[4 * j + 2] = lo[j] >> 16;
    both[4 * j + 3] = hi[j] >> 16;
  }
  if (__ballot((ms[0] | ms[1] | ms[2] | ms[3]) != 0u) != 0ull) {  // wave-uniform: some lane met a missing call
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      both[4 * j + 0] |= (ms[j] & 0xFFu) << 20;
      both[4 * j + 1] |= ((ms[j] >> 8) & 0xFFu) << 20;
      both[4 * j + 2] |= ((ms[j] >> 16) & 0xFFu) << 20;
      both[4 * j + 3] |= (ms[j] >> 24) << 20;
    }
  }
  reduce_scatter_step<16, 32>(both, lane);
  reduce_scatter_step<8, 16>(both, lane);
  reduce_scatter_step<4, 8>(both, lane);
  reduce_scatter_step<2, 4>(both, lane);
  return make_uint2(both[0] & 0xFFFFFu, both[0] >> 20);
}

// MULTI: some population has more than 16 * kChunkIters individuals, so the packed fields are
// widened several times per population (keeps 32 more registers live across the load loop).
// FUSED: evaluate the parameter sets at the end of each tile (site_flags folded in).
// The second launch bound keeps the usual form at 5 waves per SIMD (<= 96 VGPRs): four resident waves of
// more than that leave the windows stage's waves no room next to the pass, and the pipelined step loses
// what the overlap gives (measured at 99 VGPRs: C5 3.63 -> 3.79 ms per step).
// (Round 4 also had a 64-register form for passes with many parameter sets, at 16 waves per CU.  With the
// predicate table of site_eval.hpp the per-site decision no longer decides the grid: the usual form at 12
// waves per CU gives C5's pipelined step 3.09 ms where that form gave 3.15 with the set-by-set decision and
// 3.41 with the table -- profiles/r05_c5_grid.txt -- and the form is gone.)
// SKIP (fused, not MULTI, candidates' frequencies only, every set polarised by ancestral alleles, set-by-set form):
// a condition bit can only be up where ref_freq < w and the sources' comparisons hold -- the target enters
// tgt_freq at such sites and the validity test, which can only CLEAR a bit.  The tile's sources and ref are
// streamed first, lane = site votes whether some set can still pass, and the target's rows -- half of C3's
// bytes -- are read only in tiles where a lane said yes (one site in 1 000 passes: 6 % of C3's tiles); the
// other tiles' rows are stored as zeros.  The outputs are the other form's bit for bit.
// PROBE (SKIP, a ref of at least kRefProbeMinInd individuals): what the result uses of ref is one bit per site,
// ref_freq < w, and only at sites where the sources' comparisons hold.  The sources are streamed first and the
// lanes vote (source_hits): a tile without such a site reads neither ref nor target.  Then ref's first PROBE rows are
// counted as a population of their own and the lanes vote again (ref_may_pass): the rows beyond are read only where
// some site's partial sum has not reached w yet, and their counts added -- from there on the tile is the SKIP form's,
// on the counts a full read gives.  C3: 6.6 % of the tiles go on beyond 64 rows, 6.2 % hold a candidate.
template <bool MULTI, bool FUSED, bool SKIP = false, int PROBE = 0>
__global__ __launch_bounds__(64, MULTI ? 4 : 5) void site_counts_kernel(CountsArgs a, FusedArgs fa) {
  static_assert(!SKIP || (FUSED && !MULTI), "the skipping form is the usual fused form's");
  static_assert(PROBE == 0 || SKIP, "the probing form is the skipping form's");
  // FUSED: the butterfly leaves lane l with site (l%4)*16 + l/4 of the tile; each lane parks those
  // {alt_sum, n_called} per population in LDS AT ITS SITE'S INDEX, and once all populations of the
  // tile are done lane l takes site l back and evaluates the parameter sets for it -- lanes in site
  // order, so the ballots per set are the tile's flag planes and the candidates' tgt_freq leave packed
  __shared__ uint2 stash[FUSED ? kMaxPops : 1][FUSED ? 64 : 1];
  __shared__ uint32_t table_words[FUSED ? sizeof(PredTable) / 4 : 1];
  PredTable* table = reinterpret_cast<PredTable*>(table_words);
  if (FUSED) {
    stage_pred_table(fa.es, table);
    wave_lds_fence();
  }
  for (int64_t tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
    const int lane = threadIdx.x;
    const int r = lane >> 2;
    if constexpr (PROBE > 0) {  // sources, vote, ref's first rows, vote, ref's other rows, vote, target -- or nothing from a vote on
      const int mine = (lane & 3) * 16 + r;  // the site whose counts the butterfly leaves in this lane
      const bool live = tile * kTile + lane < a.n_sites;
      auto rows_of = [&](int p) {
        return reinterpret_cast<const u32x4*>(a.pop[p].tiles + tile * static_cast<int64_t>(a.pop[p].n_ind) * kTile) + lane;
      };
      auto count_pop = [&](int p) {
        const uint2 c = count_piece(rows_of(p), a.pop[p].n_ind, r, lane);
        return make_uint2(c.x, static_cast<uint32_t>(a.pop[p].n_ind) - c.y);
      };
      for (int p = 2; p < a.n_pops; ++p) stash[p][mine] = count_pop(p);
      wave_lds_fence();
      const uint32_t hits = source_hits(a.n_pops, fa, [&](int q) { return stash[q][lane]; }, live);
      bool go = __ballot(hits != 0u) != 0ull;
      if (go) {
        const int n_ref = a.pop[0].n_ind;
        uint2 ref = count_piece(rows_of(0), PROBE, r, lane);
        stash[0][mine] = ref;
        wave_lds_fence();
        go = __ballot(ref_may_pass(fa, hits, stash[0][lane].x, n_ref)) != 0ull;
        if (go) {
          wave_lds_fence();  // the vote's reads are over before the whole population's counts replace the probe's
          const uint2 rest = count_piece(rows_of(0) + PROBE * 4, n_ref - PROBE, r, lane);
          stash[0][mine] = make_uint2(ref.x + rest.x, static_cast<uint32_t>(n_ref) - (ref.y + rest.y));
          wave_lds_fence();
          go = __ballot(target_may_matter(a.n_pops, fa, [&](int q) { return stash[q][lane]; }, live)) != 0ull;
        }
      }
      if (!go) {
        // the row eval_site would have stored: "any" and the sets' conditions all down, no frequency
        if (lane <= fa.n_sets) __builtin_nontemporal_store(uint64_t{0}, fa.planes + tile * fa.plane_stride + lane);
        wave_lds_fence();  // the next tile's counts must not overtake the votes' reads
        continue;
      }
      stash[1][mine] = count_pop(1);
    }
    // SKIP: sources, ref, the vote, then the target (p = 1) -- or nothing
    int k = 0;
    for (; PROBE == 0 && k < a.n_pops; ++k) {
      const int p = !SKIP ? k : k + 2 < a.n_pops ? k + 2 : k + 2 == a.n_pops ? 0 : 1;
      if (SKIP && p == 1) {
        wave_lds_fence();
        if (__ballot(target_may_matter(a.n_pops, fa, [&](int q) { return stash[q][lane]; },
                                       tile * kTile + lane < a.n_sites)) == 0ull) {
          // the row eval_site would have stored: "any" and the sets' conditions all down, no frequency
          if (lane <= fa.n_sets) __builtin_nontemporal_store(uint64_t{0}, fa.planes + tile * fa.plane_stride + lane);
          break;
        }
      }
      const int n_ind = a.pop[p].n_ind;
      const u32x4* base =
          reinterpret_cast<const u32x4*>(a.pop[p].tiles + tile * static_cast<int64_t>(n_ind) * kTile) + lane;
      const int n_full = n_ind >> 4;         // iterations in which all 16 rows exist
      const int n_iter = (n_ind + 15) >> 4;  // plus at most one partial iteration
      int it = 0;
      uint2 cnt;
      if (MULTI) {
        uint32_t sum32[16], miss32[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) sum32[j] = miss32[j] = 0;
        while (it < n_iter) {
          uint32_t lo[4] = {0, 0, 0, 0}, hi[4] = {0, 0, 0, 0}, ms[4] = {0, 0, 0, 0};
          accumulate_rows(base, it, min(n_full, it + kChunkIters), n_full, n_iter, n_ind, r, lo, hi, ms);
          widen_fields(lo, hi, ms, sum32, miss32);
        }
        reduce_scatter_step<16, 32>(sum32, lane);
        reduce_scatter_step<8, 16>(sum32, lane);
        reduce_scatter_step<4, 8>(sum32, lane);
        reduce_scatter_step<2, 4>(sum32, lane);
        reduce_scatter_step<16, 32>(miss32, lane);
        reduce_scatter_step<8, 16>(miss32, lane);
        reduce_scatter_step<4, 8>(miss32, lane);
        reduce_scatter_step<2, 4>(miss32, lane);
        cnt = make_uint2(sum32[0], static_cast<uint32_t>(n_ind) - miss32[0]);
      } else {  // n_iter <= kChunkIters + 1: one pass, widened once -- and ONE butterfly for both sums (count_piece)
        cnt = count_piece(base, n_ind, r, lane);
        cnt.y = static_cast<uint32_t>(n_ind) - cnt.y;
      }
      const int64_t site = tile * kTile + (lane & 3) * 16 + r;
      if (!SKIP && a.counts && site < a.n_sites) store_counts_nt(a.counts + static_cast<int64_t>(p) * a.n_sites + site, cnt);
      if (FUSED) stash[p][(lane & 3) * 16 + r] = cnt;
    }
    if (SKIP && PROBE == 0 && k < a.n_pops) {  // the target was left unread
      wave_lds_fence();  // the next tile's counts must not overtake the vote's reads
      continue;
    }
    if (FUSED) {
      wave_lds_fence();
      eval_site<kMaxPops>(
          a.n_pops, fa.ploidy, [&](int p) { return stash[p][lane]; }, fa.n_sets, fa.es, table, tile, lane,
          tile * kTile + lane < a.n_sites, a.n_sites, fa.tgt_freq, fa.planes, fa.plane_stride, nullptr,
          fa.sparse_freq != 0, fa.with_inv != 0);
      wave_lds_fence();  // the next tile's counts must not overtake these reads
    }
  }
}

}  // namespace

int check_plane_stride(int64_t plane_stride, int32_t n_sets) {
  if (plane_stride < static_cast<int64_t>(kPlanesPerSet) * n_sets || plane_stride > (int64_t{1} << 20))
    return fail(SAI_ERR_ARG, "plane_stride %lld does not hold %d sets", static_cast<long long>(plane_stride), n_sets);
  return SAI_OK;
}

extern "C" int32_t sai_skip_min_tgt_ind(void) { return kSkipMinTgtInd; }
extern "C" int32_t sai_ref_probe_rows(void) { return kRefProbeRows; }
extern "C" int32_t sai_ref_probe_min_ind(void) { return kRefProbeMinInd; }

extern "C" int64_t sai_plane_words(int64_t n_sites, int32_t n_sets) {
  if (n_sites < 0 || n_sets < 0 || n_sites >= 0x7FFFFFFFll) return -1;
  return (n_sites + kTile - 1) / kTile * kPlanesPerSet * n_sets;
}

int check_sets(int32_t n_sets, const sai_params* sets, int32_t n_src, int32_t max_sets) {
  if (n_sets < 1 || n_sets > max_sets) return fail(SAI_ERR_ARG, "n_sets must be 1..%d", max_sets);
  if (!sets) return fail(SAI_ERR_ARG, "sets_host is NULL");
  for (int s = 0; s < n_sets; ++s) {
    if (n_src >= 0 && sets[s].n_src != n_src)
      return fail(SAI_ERR_ARG, "set %d: n_src %d != source populations %d", s, sets[s].n_src, n_src);
    for (int k = 0; k < sets[s].n_src && k < SAI_MAX_SRC; ++k)
      if (sets[s].op[k] < SAI_OP_EQ || sets[s].op[k] > SAI_OP_GE)
        return fail(SAI_ERR_ARG, "set %d: bad operator %d", s, sets[s].op[k]);
  }
  return SAI_OK;
}

// shared by sai_site_counts (n_sets == 0) and sai_site_pass
static int launch_site_counts(sai_ctx* ctx, int64_t n_sites, int32_t n_pops, const sai_pop* pops, uint32_t* counts,
                              int32_t n_sets, const sai_params* sets_host, int32_t freq_mode, double* tgt_freq,
                              uint64_t* planes, int64_t plane_stride, void* stream) {
  if (n_sites < 0 || n_sites >= 0x7FFFFFFFll) return fail(SAI_ERR_ARG, "n_sites out of range");
  if (n_pops < 1 || n_pops > kMaxPops) return fail(SAI_ERR_ARG, "n_pops must be 1..%d", kMaxPops);
  if (!pops) return fail(SAI_ERR_ARG, "pops is NULL");
  if (n_sites == 0) return SAI_OK;
  CountsArgs a;
  FusedArgs fa;
  std::memset(&fa, 0, sizeof(fa));
  a.n_sites = n_sites;
  a.n_tiles = (n_sites + kTile - 1) / kTile;
  a.n_pops = n_pops;
  bool multi = false;
  for (int p = 0; p < n_pops; ++p) {
    if (pops[p].n_ind < 0) return fail(SAI_ERR_ARG, "population %d: negative n_ind", p);
    if (pops[p].n_ind > 0 && !pops[p].tiles) return fail(SAI_ERR_ARG, "population %d: NULL tiles", p);
    if (pops[p].n_ind > (1 << 24)) return fail(SAI_ERR_UNSUPPORTED, "population %d: n_ind > 2^24", p);
    if (reinterpret_cast<uintptr_t>(pops[p].tiles) & 15u)
      return fail(SAI_ERR_ARG, "population %d: tiles must be 16-byte aligned", p);
    a.pop[p].tiles = pops[p].tiles;
    a.pop[p].n_ind = pops[p].n_ind;
    a.pop[p].pad = 0;
    multi = multi || pops[p].n_ind > 16 * kChunkIters;
    fa.ploidy[p] = pops[p].ploidy;
  }
  a.counts = reinterpret_cast<uint2*>(counts);
  fa.n_sets = n_sets;
  fa.sparse_freq = freq_mode != SAI_FREQ_DENSE;
  fa.with_inv = n_sets > 0 && sets_with_inverted(n_sets, sets_host);
  fa.tgt_freq = tgt_freq;
  fa.planes = planes;
  fa.plane_stride = plane_stride;
  if (n_sets > 0) fill_eval_sets(fa.es, n_sets, sets_host, n_pops - 2);
  int64_t individuals = 0;
  for (int p = 0; p < n_pops; ++p) individuals += pops[p].n_ind;
  hipStream_t st = static_cast<hipStream_t>(stream);
  // the form that leaves the target unread where no site can pass: only where its outputs are the other form's bit
  // for bit (the candidates' frequencies alone, no counts, no inverted words -- an inverted bit depends on the
  // target's validity where the condition is false) and the decision is taken set by set (a call of C5's many
  // sets has a candidate in every tile); SAI_TGT_SKIP=0: A/B knob, read at every launch
  const char* skip_env = std::getenv("SAI_TGT_SKIP");
  const bool skip = n_sets > 0 && !multi && freq_mode == SAI_FREQ_CANDIDATES && !counts && !fa.with_inv &&
                    !fa.es.use_table && pops[1].n_ind >= kSkipMinTgtInd && !(skip_env && skip_env[0] == '0');
  // ... and ref beyond its first rows: a ref wide enough for that to pay, and fewer sets than the grid rule calls many
  // (a set-by-set call of many sets has a candidate in nearly every tile: the votes' loops over the sets would be work
  // for nothing -- 18 of C5's sets: 3.86 against 3.01 ms); SAI_REF_PROBE=0: A/B knob, likewise
  const char* probe_env = std::getenv("SAI_REF_PROBE");
  const bool probe = skip && n_sets < many_sets() && pops[0].n_ind >= kRefProbeMinInd && !(probe_env && probe_env[0] == '0');
  // most tiles of the probing form are 4 KiB behind two trips to memory, not 128 KB of streaming: where the rule
  // gives wide populations 8 waves per CU -- and only there: the one case the sweep covers -- it takes 24 (C3: 0.541 ms
  // at 8, 0.413 at 16, 0.396 at 24, 0.403 at 20 and at 32 -- profiles/ref_probe_ab.txt)
  int waves_per_cu = site_pass_waves_per_cu(ctx, a.n_tiles, n_sets, n_pops, individuals);
  if (probe && waves_per_cu == 8) waves_per_cu = kRefProbeWavesPerCu;
  const dim3 grid(stream_grid(ctx, a.n_tiles, waves_per_cu));
  if (n_sets > 0) {
    if (multi) launch_pass(ctx, site_counts_kernel<true, true>, grid, dim3(64), st, a, fa);
    else if (probe) launch_pass(ctx, site_counts_kernel<false, true, true, kRefProbeRows>, grid, dim3(64), st, a, fa);
    else if (skip) launch_pass(ctx, site_counts_kernel<false, true, true>, grid, dim3(64), st, a, fa);
    else launch_pass(ctx, site_counts_kernel<false, true>, grid, dim3(64), st, a, fa);
  } else {
    if (multi) launch_pass(ctx, site_counts_kernel<true, false>, grid, dim3(64), st, a, fa);
    else launch_pass(ctx, site_counts_kernel<false, false>, grid, dim3(64), st, a, fa);
  }
  return check_launch("site_counts");
}

// ------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------

extern "C" {

int sai_site_counts(sai_ctx* ctx, int64_t n_sites, int32_t n_pops, const sai_pop* pops, uint32_t* counts,
                    void* stream) {
  if (int rc = enter(ctx)) return rc;
  if (!counts && n_sites > 0) return fail(SAI_ERR_ARG, "counts is NULL");
  return launch_site_counts(ctx, n_sites, n_pops, pops, counts, 0, nullptr, SAI_FREQ_DENSE, nullptr, nullptr, 0, stream);
}

int sai_site_pass(sai_ctx* ctx, int64_t n_sites, int32_t n_pops, const sai_pop* pops, uint32_t* counts,
                  int32_t n_sets, const sai_params* sets_host, int32_t freq_mode, double* tgt_freq, uint64_t* planes,
                  int64_t plane_stride, void* stream) {
  if (int rc = enter(ctx)) return rc;
  if (freq_mode != SAI_FREQ_DENSE && freq_mode != SAI_FREQ_CANDIDATES && freq_mode != SAI_FREQ_CANDIDATES_READ_ALL)
    return fail(SAI_ERR_ARG, "bad freq_mode %d", freq_mode);
  if (n_pops < 2) return fail(SAI_ERR_ARG, "n_pops must be >= 2 (ref, tgt, sources)");
  if (n_sets > kFusedSets)
    return fail(SAI_ERR_UNSUPPORTED, "sai_site_pass carries at most %d parameter sets; use sai_site_counts + sai_site_flags",
                kFusedSets);
  if (int rc = check_sets(n_sets, sets_host, n_pops - 2, kFusedSets)) return rc;
  if (pops)
    for (int p = 0; p < n_pops && p < kMaxPops; ++p)
      if (pops[p].ploidy <= 0) return fail(SAI_ERR_ARG, "ploidy[%d] must be positive", p);
  if (n_sites > 0 && (!tgt_freq || !planes)) return fail(SAI_ERR_ARG, "NULL buffer");
  if (int rc = check_plane_stride(plane_stride, n_sets)) return rc;
  return launch_site_counts(ctx, n_sites, n_pops, pops, counts, n_sets, sets_host, freq_mode, tgt_freq, planes,
                            plane_stride, stream);
}

int sai_site_flags(sai_ctx* ctx, int64_t n_sites, int32_t n_pops, const int32_t* ploidy_host,
                   const uint32_t* counts, int32_t n_sets, const sai_params* sets_host, double* tgt_freq,
                   uint64_t* planes, int64_t plane_stride, double* adj_freq, void* stream) {
  if (int rc = enter(ctx)) return rc;
  if (n_sites < 0 || n_sites >= 0x7FFFFFFFll) return fail(SAI_ERR_ARG, "n_sites out of range");
  if (n_pops < 2 || n_pops > kBigPops) return fail(SAI_ERR_ARG, "n_pops must be 2..%d (ref, tgt, sources)", kBigPops);
  if (!ploidy_host) return fail(SAI_ERR_ARG, "ploidy_host is NULL");
  if (int rc = check_sets(n_sets, sets_host, n_pops - 2)) return rc;
  if (n_sites == 0) return SAI_OK;
  if (!counts || !tgt_freq || !planes) return fail(SAI_ERR_ARG, "NULL buffer");
  if (int rc = check_plane_stride(plane_stride, n_sets)) return rc;
  FlagArgs a;
  std::memset(&a, 0, sizeof(a));
  a.n_sites = n_sites;
  a.n_pops = n_pops;
  a.with_inv = sets_with_inverted(n_sets, sets_host);
  a.n_row_sets = static_cast<int16_t>(n_sets);
  for (int p = 0; p < n_pops; ++p) {
    if (ploidy_host[p] <= 0) return fail(SAI_ERR_ARG, "ploidy[%d] must be positive", p);
    a.ploidy[p] = ploidy_host[p];
  }
  a.counts = reinterpret_cast<const uint2*>(counts);
  a.tgt_freq = tgt_freq;
  a.planes = planes;
  a.plane_stride = plane_stride;
  a.adj_freq = adj_freq;
  const unsigned grid = static_cast<unsigned>((n_sites + 255) / 256);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (n_pops <= kMaxPops) {
    a.n_sets = static_cast<int16_t>(n_sets);
    fill_eval_sets(a.es, n_sets, sets_host, n_pops - 2);
    hipLaunchKernelGGL(site_flags_kernel<kMaxPops>, dim3(grid), dim3(256), 0, st, a);
    return check_launch("site_flags");
  }
  // more than SAI_FUSED_SRC sources (stat_utils.py:114-119 loops over any number): the table form only, as many
  // sets of the row per launch as the table's 32 comparisons hold (one set of 14 sources needs at most 30)
  for (int s0 = 0; s0 < n_sets;) {
    int k = n_sets - s0;
    while (k > 1 && !fill_eval_sets(a.es, k, sets_host + s0, n_pops - 2, true)) --k;
    if (k == 1 && !fill_eval_sets(a.es, 1, sets_host + s0, n_pops - 2, true))
      return fail(SAI_ERR_UNSUPPORTED, "set %d: more distinct comparisons than one launch evaluates", s0);
    a.set0 = static_cast<int16_t>(s0);
    a.n_sets = static_cast<int16_t>(k);
    hipLaunchKernelGGL(site_flags_kernel<kBigPops>, dim3(grid), dim3(256), 0, st, a);
    if (int rc = check_launch("site_flags")) return rc;
    s0 += k;
  }
  return SAI_OK;
}

}  // extern "C"
