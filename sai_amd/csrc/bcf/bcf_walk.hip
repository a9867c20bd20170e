// sai_bcf_chain_segments / sai_bcf_record_heads: the records of an inflated BCF stream in HBM, found without a serial
// walk from its first byte (include/saihip_bcf_device.h; DESIGN_INGEST.md, "BCF files: members inflated and records
// found on the GPU").  The plain C++ twins are in bcf_feed.cpp; the test of one position and the head of one record
// are shared text (bcf_record.hpp).
//
// Kernel A, one wavefront per segment of seg_bytes:
//  1. the segment is staged into LDS a tile of 16 KiB (and 32 bytes of overhang) at a time, with aligned 16-byte
//     loads; a word that would leave n_bytes is assembled from the bytes inside.  Every lane takes four consecutive
//     offsets at a time: the two LDS words that hold the word at o + 28 are funnel-shifted into the four alignments
//     and compared with the sample count -- the test that nearly every byte fails -- and only an offset that passes
//     reads its l_shared and CHROM (from LDS, byte by byte: it may lie anywhere).  A candidate sets its bit in one
//     LDS bitmap and the bit of its successor, when that lies inside the segment, in another;
//  2. heads = candidates that are nobody's successor, listed in ascending order by a prefix sum over the lanes'
//     popcounts, max_heads at most;
//  3. lane k follows the chain of head k.  A successor is strictly more than 31 bytes further, so a chain makes at
//     most seg_bytes / 32 + 1 hops before it leaves the segment: that is the loop bound.  The lengths of a chain
//     position are read from global memory byte by byte (the position is a candidate, so its 32 bytes lie inside
//     n_bytes); whether a successor is a candidate is one bit of the LDS bitmap.
// Kernel B, one wavefront per segment the true chain enters: lane 0 follows the chain through the segment and leaves
// the offsets in LDS, then every lane fills the 64-byte heads of its records.
// Neither grid is capped: a batch of 2^31 bytes is at most 2^23 segments.

#include "../common.hpp"
#include "bcf_record.hpp"

namespace {

constexpr int kWave = 64;
constexpr int kTileBytes = 16384;
constexpr int kMaxSegWords = SAI_BCF_SEG_MAX / 32;      // bitmap words of a segment
constexpr int kMaxSegRecords = SAI_BCF_SEG_MAX / 32 + 1;  // records that start inside a segment

struct ChainArgs {
  const uint8_t* text;
  int64_t n_bytes;
  int32_t seg_bytes, max_heads;
  const uint8_t* contig_defined;
  int32_t n_contigs, n_sample;
  sai_bcf_chain* chains;
  int32_t* seg_info;
};

// the aligned 16-byte word at byte `at` (at % 16 == 0); bytes at or behind n_bytes are 0
__device__ __forceinline__ u32x4 load_word16(const uint8_t* text, int64_t n_bytes, int64_t at) {
  if (at + 16 <= n_bytes) return *reinterpret_cast<const u32x4*>(text + at);
  u32x4 w = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (at + 4 * j + k < n_bytes) w[j] |= static_cast<uint32_t>(text[at + 4 * j + k]) << (8 * k);
  return w;
}

__device__ __forceinline__ uint32_t lds_le32(const uint8_t* b, int i) {
  return static_cast<uint32_t>(b[i]) | static_cast<uint32_t>(b[i + 1]) << 8 | static_cast<uint32_t>(b[i + 2]) << 16 |
         static_cast<uint32_t>(b[i + 3]) << 24;
}

__global__ __launch_bounds__(kWave) void bcf_chain_segments_kernel(ChainArgs a) {
  __shared__ u32x4 tile16[(kTileBytes + 32) / 16];
  __shared__ uint32_t cand[kMaxSegWords], issucc[kMaxSegWords];
  __shared__ uint32_t head_rel[SAI_BCF_MAX_HEADS_LIMIT];
  const int lane = threadIdx.x;
  const int64_t seg = blockIdx.x;
  const int64_t seg_begin = seg * a.seg_bytes, seg_end = seg_begin + a.seg_bytes;
  const int n_words = a.seg_bytes / 32;
  for (int w = lane; w < n_words; w += kWave) cand[w] = issucc[w] = 0u;
  const uint32_t* tile = reinterpret_cast<const uint32_t*>(tile16);
  const uint8_t* tile8 = reinterpret_cast<const uint8_t*>(tile16);
  const int tile_len = a.seg_bytes < kTileBytes ? a.seg_bytes : kTileBytes;
  for (int tile_off = 0; tile_off < a.seg_bytes && seg_begin + tile_off < a.n_bytes; tile_off += tile_len) {
    __syncthreads();  // the tile before has been tested (and the bitmaps are zero)
    const int64_t tb = seg_begin + tile_off;
    for (int w = lane; w < (tile_len + 32) / 16; w += kWave) tile16[w] = load_word16(a.text, a.n_bytes, tb + 16 * static_cast<int64_t>(w));
    __syncthreads();
    for (int j = lane; j < tile_len / 4; j += kWave) {
      const uint32_t lo = tile[j + 7], hi = tile[j + 8];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint32_t w28 = k ? __funnelshift_r(lo, hi, 8 * k) : lo;
        if ((w28 & 0xFFFFFFu) != static_cast<uint32_t>(a.n_sample)) continue;
        const int in_tile = 4 * j + k;
        const int64_t o = tb + in_tile;
        if (o + 32 > a.n_bytes) continue;
        const uint32_t l_shared = lds_le32(tile8, in_tile), l_indiv = lds_le32(tile8, in_tile + 4);
        if (!bcfrec::fixed_fields_pass(l_shared, lds_le32(tile8, in_tile + 8), w28, a.contig_defined, a.n_contigs, a.n_sample)) continue;
        const int rel = tile_off + in_tile;
        atomicOr(&cand[rel >> 5], 1u << (rel & 31));
        const int64_t succ = o + 8 + static_cast<int64_t>(l_shared) + static_cast<int64_t>(l_indiv);
        if (succ < seg_end) {
          const int srel = static_cast<int>(succ - seg_begin);
          atomicOr(&issucc[srel >> 5], 1u << (srel & 31));
        }
      }
    }
  }
  __syncthreads();
  // the heads in ascending order: a prefix sum of the lanes' popcounts, 64 bitmap words at a time
  int total = 0;
  for (int base = 0; base < n_words && total <= a.max_heads; base += kWave) {
    const int w = base + lane;
    uint32_t hw = w < n_words ? cand[w] & ~issucc[w] : 0u;
    const int c = __popc(hw);
    int incl = c;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
      const int up = __shfl_up(incl, d);
      if (lane >= d) incl += up;
    }
    int at = total + incl - c;
    while (hw && at < a.max_heads) {
      const int bit = __ffs(hw) - 1;
      hw &= hw - 1;
      head_rel[at++] = static_cast<uint32_t>(w * 32 + bit);
    }
    total += __shfl(incl, kWave - 1);
  }
  __syncthreads();
  const int n_heads = total < a.max_heads ? total : a.max_heads;
  if (lane == 0) a.seg_info[seg] = n_heads | (total > a.max_heads ? 1 << 30 : 0);
  if (lane >= a.max_heads) return;
  sai_bcf_chain out = {0u, 0u, 0u, 0u};
  if (lane < n_heads) {
    int64_t p = seg_begin + head_rel[lane];
    out.head = static_cast<uint32_t>(p);
    out.flags = SAI_BCF_CHAIN_BROKEN;  // what a chain that outlasts the bound would be: it cannot
    const int max_hops = a.seg_bytes / 32 + 1;  // a hop is at least 32 bytes
    for (int hop = 0; hop < max_hops; ++hop) {
      const int64_t next = bcfrec::successor(a.text, p);  // p is a candidate: its 32 bytes lie inside n_bytes
      if (next > a.n_bytes) { out.flags = SAI_BCF_CHAIN_INCOMPLETE; break; }
      ++out.n_records;
      p = next;
      if (p >= seg_end) { out.flags = 0; break; }
      if (p + 32 > a.n_bytes) { out.flags = SAI_BCF_CHAIN_INCOMPLETE; break; }
      const int rel = static_cast<int>(p - seg_begin);
      if (!(cand[rel >> 5] >> (rel & 31) & 1u)) break;  // broken
    }
    out.chain_exit = static_cast<uint32_t>(p);
  }
  a.chains[seg * a.max_heads + lane] = out;
}

struct HeadArgs {
  const uint8_t* text;
  int64_t n_bytes;
  int32_t seg_bytes;
  const int64_t* seg_entry;
  const int64_t* seg_first_record;
  int64_t carry_from, n_records, gt_key;
  int32_t want_gt;
  sai_bcf_record_head* heads;
};

__global__ __launch_bounds__(kWave) void bcf_record_heads_kernel(HeadArgs a) {
  __shared__ uint32_t offs[kMaxSegRecords];
  __shared__ int n_found;
  const int lane = threadIdx.x;
  const int64_t seg = blockIdx.x;
  const int64_t seg_begin = seg * a.seg_bytes, seg_end = seg_begin + a.seg_bytes;
  const int64_t entry = a.seg_entry[seg];
  if (entry < seg_begin || entry >= seg_end) return;  // -1: the chain does not enter this segment
  if (lane == 0) {
    int n = 0;
    int64_t p = entry;
    const int max_records = a.seg_bytes / 32 + 1;  // a record is at least 32 bytes
    while (n < max_records && p < seg_end && p < a.carry_from && p + 32 <= a.n_bytes) {
      const int64_t next = bcfrec::successor(a.text, p);
      if (next > a.n_bytes || bcfrec::le32_at(a.text, p) < 24u) break;
      offs[n++] = static_cast<uint32_t>(p);
      p = next;
    }
    n_found = n;
  }
  __syncthreads();
  const int64_t first = a.seg_first_record[seg];
  for (int i = lane; i < n_found; i += kWave) {
    const int64_t r = first + i;
    if (r >= 0 && r < a.n_records) bcfrec::fill_head(a.text, offs[i], a.gt_key, a.want_gt != 0, a.heads + r);
  }
}

}  // namespace

extern "C" int sai_bcf_chain_segments(sai_ctx* ctx, const uint8_t* text, int64_t n_bytes, int32_t seg_bytes, int32_t max_heads,
                                      const uint8_t* contig_defined, int32_t n_contigs, int32_t n_sample, sai_bcf_chain* chains,
                                      int32_t* seg_info, void* stream) {
  if (int rc = enter(ctx)) return rc;
  if (int rc = bcfrec::check_stream_args(text, n_bytes, seg_bytes, true)) return rc;
  if (max_heads < 1 || max_heads > SAI_BCF_MAX_HEADS_LIMIT) return fail(SAI_ERR_ARG, "max_heads must be in 1 .. %d", SAI_BCF_MAX_HEADS_LIMIT);
  if (n_contigs < 0 || n_sample < 0 || n_sample > 0xFFFFFF) return fail(SAI_ERR_ARG, "size out of range");
  if (n_bytes == 0) return SAI_OK;
  if (!chains || !seg_info || (n_contigs > 0 && !contig_defined)) return fail(SAI_ERR_ARG, "NULL buffer");
  const int64_t n_segments = (n_bytes + seg_bytes - 1) / seg_bytes;
  ChainArgs a{text, n_bytes, seg_bytes, max_heads, contig_defined, n_contigs, n_sample, chains, seg_info};
  hipLaunchKernelGGL(bcf_chain_segments_kernel, dim3(static_cast<unsigned>(n_segments)), dim3(kWave), 0, static_cast<hipStream_t>(stream), a);
  return check_launch("bcf_chain_segments");
}

extern "C" int sai_bcf_record_heads(sai_ctx* ctx, const uint8_t* text, int64_t n_bytes, int32_t seg_bytes, const int64_t* seg_entry,
                                    const int64_t* seg_first_record, int64_t carry_from, int64_t n_records, int64_t gt_key,
                                    int32_t want_gt, sai_bcf_record_head* heads, void* stream) {
  if (int rc = enter(ctx)) return rc;
  if (int rc = bcfrec::check_stream_args(text, n_bytes, seg_bytes, true)) return rc;
  if (carry_from < 0 || carry_from > n_bytes || n_records < 0) return fail(SAI_ERR_ARG, "size out of range");
  if (n_bytes == 0 || n_records == 0) return SAI_OK;
  if (!seg_entry || !seg_first_record || !heads) return fail(SAI_ERR_ARG, "NULL buffer");
  const int64_t n_segments = (n_bytes + seg_bytes - 1) / seg_bytes;
  HeadArgs a{text, n_bytes, seg_bytes, seg_entry, seg_first_record, carry_from, n_records, gt_key, want_gt, heads};
  hipLaunchKernelGGL(bcf_record_heads_kernel, dim3(static_cast<unsigned>(n_segments)), dim3(kWave), 0, static_cast<hipStream_t>(stream), a);
  return check_launch("bcf_record_heads");
}
