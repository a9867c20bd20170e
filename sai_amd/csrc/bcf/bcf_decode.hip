// sai_bcf_decode: the GT arrays of BCF records in HBM -> int8 dosages [row][slot], the block sai_tokenize_gt
// writes for the same calls as VCF text (include/saihip_bcf.h).
//
// The contract and the shape are those of sai_plink_decode (plink/bed_decode.hip): the [row][slot] block is one
// flat byte array, every lane owns 16 consecutive, 16-byte aligned bytes of it and stores them as one 128-bit
// word; a call writes the rows [out_row0, out_row0 + n_out_rows) only, so its first and its last chunk, which may
// hold bytes of other rows, are stored byte by byte.  A row names the bytes of its own values (1, 2 or 4), so one
// kernel serves every width and reads it per row; the template over the width is the value loader of the general path.
//  * fast path (width 1) -- the slots are a run of consecutive sample columns at one ploidy p, the row holds L = 1
//    or L = 2 values per sample with p <= L, and the lane's 16 slots lie in one row: its 16 * L input bytes start
//    at any byte, so the lane loads the L + 1 aligned 128-bit words that hold them and funnel-shifts them into
//    place.  Four values are recoded at a time in a 32-bit word: the phase bit is shifted out, a byte with the
//    sign bit set (end-of-vector, missing) becomes allele + 1 = 0 like a missing allele, the positions from p on
//    are masked away and the values of a pair are summed.  No branch depends on a sample.  With at most two
//    alleles of at most 62 the int8 range cannot be left.
//  * general path -- any col_of_slot, per-slot ploidies, p > L, L > 2, widths 2 and 4, and the lanes whose 16
//    bytes cross a row boundary: one value at a time.
// status[row] is zeroed by the entry point and raised with atomicMax only by the rare lane that has something to
// report; every offset, column and ploidy is checked before it is used, and a load never leaves [batch, batch +
// batch_bytes): an aligned word that would is assembled from its bytes inside.
// The grid is not capped: a lane takes one chunk of 16 output bytes, a batch is at most a staging buffer, and a call
// of more than 2^24 blocks (2^32 threads, 64 GiB of output) is refused by the entry point.

#include "../common.hpp"
#include "saihip_bcf.h"

namespace {

struct BcfArgs {
  const uint8_t* batch;
  int64_t batch_bytes;
  const int64_t* gt_off;
  const uint8_t* gt_width;
  const int32_t* gt_len;
  const uint8_t* row_flip;
  int32_t n_cols;
  int32_t n_slots;
  const int32_t* col_of_slot;
  int32_t first_col;  // >= 0: col_of_slot[s] == first_col + s
  const int32_t* ploidy_of_slot;
  int32_t uniform_ploidy;  // 1 .. 64: every slot; 0: ploidy_of_slot
  int8_t* out;
  int32_t* status;
  int64_t e_begin, e_end;  // the call's bytes of the flat block: [out_row0 * n_slots, (out_row0 + n_out_rows) * n_slots)
  int64_t chunk0;          // e_begin / 16
  int64_t n_chunks;        // aligned 16-byte chunks that hold a byte of the call
};

constexpr int kBcfBlock = 256;

struct RowState {
  const uint8_t* src;  // the row's GT array
  int64_t off;
  int32_t L;
  int32_t width;
  bool ok;
  bool flip;
};

__device__ __forceinline__ RowState load_row(const BcfArgs& a, int64_t row) {
  RowState r;
  r.off = a.gt_off[row];
  r.L = a.gt_len[row];
  r.width = a.gt_width[row];
  r.flip = a.row_flip[row] != 0;
  r.ok = (r.width == 1 || r.width == 2 || r.width == 4) && r.L >= 0 && r.off >= 0 && r.off <= a.batch_bytes;
  if (r.ok && a.n_cols > 0) r.ok = r.L <= (a.batch_bytes - r.off) / r.width / a.n_cols;
  r.src = a.batch + (r.ok ? r.off : 0);
  return r;
}

template <int W>
__device__ __forceinline__ int32_t load_value(const uint8_t* p) {
  if (W == 1) return static_cast<int8_t>(p[0]);
  if (W == 2) return static_cast<int16_t>(static_cast<uint16_t>(p[0] | p[1] << 8));  // a GT array may start at any byte
  return static_cast<int32_t>(static_cast<uint32_t>(p[0]) | static_cast<uint32_t>(p[1]) << 8 | static_cast<uint32_t>(p[2]) << 16 |
                              static_cast<uint32_t>(p[3]) << 24);
}

// the output byte of (row, slot) on the general path
template <int W>
__device__ __forceinline__ uint32_t decode_cell(const BcfArgs& a, const RowState& r, int64_t row, int32_t slot) {
  const int32_t col = a.first_col >= 0 ? a.first_col + slot : a.col_of_slot[slot];
  const int32_t pl = a.uniform_ploidy ? a.uniform_ploidy : a.ploidy_of_slot[slot];
  if (!r.ok || col < 0 || col >= a.n_cols || pl < 1 || pl > 64) {
    atomicMax(a.status + row, SAI_BCF_STATUS_BAD_INDEX);
    return 0u;
  }
  constexpr int32_t type_min = W == 1 ? -128 : W == 2 ? -32768 : INT32_MIN;
  const uint8_t* sample = r.src + static_cast<int64_t>(col) * r.L * W;
  int32_t d = 0, fd = 0;
  bool bad = false;
  for (int32_t k = 0; k < pl; ++k) {
    int32_t al = -1;
    if (k < r.L) {
      const int32_t v = load_value<W>(sample + static_cast<int64_t>(k) * W);
      if (v >= 0) al = (v >> 1) - 1;
      else bad = bad || (v != type_min && v != type_min + 1);
    }
    d += al;
    fd += al >= 1 ? al - 1 : 1 - al;
    // 64 alleles of less than 2^30 each: the sums of a slot that will be refused may wrap, so they are clamped
    d = d > 1 << 20 ? 1 << 20 : d;
    fd = fd > 1 << 20 ? 1 << 20 : fd;
  }
  if (bad) {
    atomicMax(a.status + row, SAI_BCF_STATUS_BAD_VALUE);
    return 0u;
  }
  if (d > 127 || fd > 127 || d < -128) {
    atomicMax(a.status + row, SAI_BCF_STATUS_RANGE);
    return 0u;
  }
  return static_cast<uint32_t>(r.flip ? fd : d) & 0xFFu;
}

// the aligned 16-byte word at byte `at` of the batch (at % 16 == 0, at < batch_bytes); bytes behind the batch are 0
__device__ __forceinline__ u32x4 load_word(const BcfArgs& a, int64_t at) {
  if (at + 16 <= a.batch_bytes) return *reinterpret_cast<const u32x4*>(a.batch + at);
  u32x4 w = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (at + 4 * j + k < a.batch_bytes) w[j] |= static_cast<uint32_t>(a.batch[at + 4 * j + k]) << (8 * k);
  return w;
}

// Four width-1 values in one word -> per byte allele + 1 (0 for a missing allele, end-of-vector and the type's
// missing value); *bad = bit 7 of every byte that holds another value with the sign bit set.
__device__ __forceinline__ uint32_t alleles_plus_one(uint32_t x, uint32_t* bad) {
  const uint32_t neg = x & 0x80808080u;
  const uint32_t full = (neg >> 7) * 0xFFu;                                // 0xFF in the bytes with the sign bit
  *bad = neg & ((x & 0x7E7E7E7Eu) + 0x7E7E7E7Eu);                           // 0x82 .. 0xFF: bits 1 .. 6 not all clear
  return ((x >> 1) & 0x7F7F7F7Fu) & ~full;
}

// per byte |t - 2| of t = allele + 1 in 0 .. 63: what a flipped row counts for an allele (a - 1 from 1 on, 1 - a below)
__device__ __forceinline__ uint32_t flipped_count(uint32_t t) {
  const uint32_t s = (t | 0x80808080u) - 0x02020202u;  // per byte 0x80 + t - 2: no borrow leaves a byte
  const uint32_t ge2 = ((s & 0x80808080u) >> 7) * 0xFFu;
  return (s & 0x7F7F7F7Fu & ge2) | ((0x02020202u - (t & ~ge2)) & ~ge2);
}

// The 16 outputs of a fast lane.  L = values per sample (1 or 2); in = its 16 * L input bytes.
template <int L>
__device__ __forceinline__ u32x4 recode_fast(const uint32_t (&in)[4 * L], int32_t ploidy, bool flip, uint32_t* any_bad) {
  u32x4 word;
  uint32_t bad_all = 0;
  if (L == 1) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      uint32_t bad;
      const uint32_t t = alleles_plus_one(in[j], &bad);
      bad_all |= bad;
      // d = t - 1 per byte, in -1 .. 62
      const uint32_t d = ((t | 0x80808080u) - 0x01010101u) ^ 0x80808080u;
      word[j] = flip ? flipped_count(t) : d;
    }
  } else {
    const uint32_t keep = ploidy == 2 ? 0xFFFFFFFFu : 0x00FF00FFu;  // the positions below the ploidy
    const uint32_t minus = static_cast<uint32_t>(ploidy) * 0x00010001u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      uint32_t pair[2];  // two samples each, the result of a sample in the low byte of its 16 bits
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        uint32_t bad;
        const uint32_t t = alleles_plus_one(in[2 * j + h], &bad);
        bad_all |= bad & keep;
        const uint32_t c = (flip ? flipped_count(t) : t) & keep;
        const uint32_t sum = (c + (c >> 8)) & 0x00FF00FFu;  // at most 126
        pair[h] = flip ? sum : ((sum | 0x01000100u) - minus) & 0x00FF00FFu;  // d = sum of (allele + 1) - ploidy
      }
      word[j] = (pair[0] & 0xFFu) | ((pair[0] >> 8) & 0xFF00u) | ((pair[1] & 0xFFu) << 16) | ((pair[1] << 8) & 0xFF000000u);
    }
  }
  *any_bad = bad_all;
  return word;
}

// the 16 * L bytes from byte `at` of the batch on (all inside it), funnel-shifted out of L + 1 aligned words
template <int L>
__device__ __forceinline__ void load_unaligned(const BcfArgs& a, int64_t at, uint32_t (&in)[4 * L]) {
  const int64_t base = at & ~int64_t(15);
  const uint32_t shift = static_cast<uint32_t>(at & 15);
  uint32_t w[4 * L + 4];
#pragma unroll
  for (int k = 0; k <= L; ++k) {
    u32x4 v = {0u, 0u, 0u, 0u};
    if (k < L || shift) v = load_word(a, base + 16 * k);  // the last word only when the bytes reach into it
#pragma unroll
    for (int j = 0; j < 4; ++j) w[4 * k + j] = v[j];
  }
  const uint32_t q = shift >> 2, bits = (shift & 3u) * 8u;
#pragma unroll
  for (int i = 0; i < 4 * L; ++i) {
    // words i + q and i + q + 1, picked with selects: q is the lane's own, the indices stay static
    const uint32_t lo = q == 0 ? w[i] : q == 1 ? w[i + 1] : q == 2 ? w[i + 2] : w[i + 3];
    const uint32_t hi = q == 0 ? w[i + 1] : q == 1 ? w[i + 2] : q == 2 ? w[i + 3] : w[i + 4];
    in[i] = __funnelshift_r(lo, hi, bits);
  }
}

__device__ __forceinline__ uint32_t decode_any(const BcfArgs& a, const RowState& r, int64_t row, int32_t slot) {
  if (r.width == 2) return decode_cell<2>(a, r, row, slot);
  if (r.width == 4) return decode_cell<4>(a, r, row, slot);
  return decode_cell<1>(a, r, row, slot);  // also a row that is not ok: it is flagged before anything is read
}

__global__ __launch_bounds__(kBcfBlock) void bcf_decode_kernel(BcfArgs a) {
  const int64_t chunk = static_cast<int64_t>(blockIdx.x) * kBcfBlock + threadIdx.x;
  if (chunk >= a.n_chunks) return;
  const bool fast = a.first_col >= 0 && a.uniform_ploidy >= 1 && a.uniform_ploidy <= 2;
  const bool narrow = a.e_end - a.e_begin <= 0xFFFFFFFFll;
  const int64_t e0 = (a.chunk0 + chunk) * 16;
  const int64_t rel = (e0 > a.e_begin ? e0 : a.e_begin) - a.e_begin;  // the lane's first byte, counted from the call's first
  int64_t row;  // of the call: indexes the row tables and status
  int32_t slot;
  if (narrow) {  // one division per 16 output bytes; 32-bit whenever the call allows it
    const uint32_t q = static_cast<uint32_t>(rel) / static_cast<uint32_t>(a.n_slots);
    row = q;
    slot = static_cast<int32_t>(static_cast<uint32_t>(rel) - q * static_cast<uint32_t>(a.n_slots));
  } else {
    row = rel / a.n_slots;
    slot = static_cast<int32_t>(rel - row * a.n_slots);
  }
  RowState r = load_row(a, row);
  if (fast && e0 >= a.e_begin && slot + 16 <= a.n_slots && r.ok && r.width == 1 && a.uniform_ploidy <= r.L && r.L <= 2) {
    // first_col + n_slots <= n_cols (the entry point's check) and the row lies inside the batch: so do these bytes
    const int64_t at = r.off + static_cast<int64_t>(a.first_col + slot) * r.L;
    uint32_t bad;
    u32x4 word;
    if (r.L == 1) {
      uint32_t in[4];
      load_unaligned<1>(a, at, in);
      word = recode_fast<1>(in, a.uniform_ploidy, r.flip, &bad);
    } else {
      uint32_t in[8];
      load_unaligned<2>(a, at, in);
      word = recode_fast<2>(in, a.uniform_ploidy, r.flip, &bad);
    }
    if (!bad) {
      *reinterpret_cast<u32x4*>(a.out + e0) = word;
      return;
    }
    // a damaged value among the 16 samples: the general path says which bytes are 0
  }
  u32x4 word = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    uint32_t w = 0;
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {
      const int64_t e = e0 + 4 * j + k;
      if (e >= a.e_begin && e < a.e_end) {
        w |= decode_any(a, r, row, slot) << (8 * k);
        if (++slot == a.n_slots) {
          slot = 0;
          ++row;
          if (e + 1 < a.e_end) r = load_row(a, row);
        }
      }
    }
    word[j] = w;
  }
  if (e0 >= a.e_begin && e0 + 16 <= a.e_end) {
    *reinterpret_cast<u32x4*>(a.out + e0) = word;
  } else {  // the first or the last chunk of the call, shared with bytes that are not its own
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int64_t e = e0 + 4 * j + k;
        if (e >= a.e_begin && e < a.e_end) a.out[e] = static_cast<int8_t>((word[j] >> (8 * k)) & 0xFFu);
      }
  }
}

}  // namespace

extern "C" int sai_bcf_decode(sai_ctx* ctx, const uint8_t* batch, int64_t batch_bytes, int64_t n_out_rows, const int64_t* gt_off,
                              const uint8_t* gt_width, const int32_t* gt_len, const uint8_t* row_flip, int32_t n_cols, int32_t n_slots,
                              const int32_t* col_of_slot, int32_t first_col, const int32_t* ploidy_of_slot, int32_t uniform_ploidy,
                              int8_t* out, int64_t out_row0, int32_t* status, void* stream) {
  if (int rc = enter(ctx)) return rc;
  if (batch_bytes < 0 || n_out_rows < 0 || n_cols < 0 || n_slots < 1 || out_row0 < 0) return fail(SAI_ERR_ARG, "size out of range");
  if (uniform_ploidy < 0 || uniform_ploidy > 64) return fail(SAI_ERR_ARG, "uniform_ploidy must be 0 or 1 .. 64");
  if (first_col >= 0 && static_cast<int64_t>(first_col) + n_slots > n_cols) return fail(SAI_ERR_ARG, "first_col + n_slots exceeds n_cols");
  if (n_out_rows == 0) return SAI_OK;
  if (!gt_off || !gt_width || !gt_len || !row_flip || !out || !status || (first_col < 0 && !col_of_slot) || (uniform_ploidy == 0 && !ploidy_of_slot) ||
      (batch_bytes > 0 && !batch))
    return fail(SAI_ERR_ARG, "NULL buffer");
  if (reinterpret_cast<uintptr_t>(out) & 15u) return fail(SAI_ERR_ARG, "out must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(batch) & 15u) return fail(SAI_ERR_ARG, "batch must be 16-byte aligned");
  if (out_row0 + n_out_rows > (std::numeric_limits<int64_t>::max() - 16) / n_slots) return fail(SAI_ERR_ARG, "size out of range");
  BcfArgs a;
  a.batch = batch;
  a.batch_bytes = batch_bytes;
  a.gt_off = gt_off;
  a.gt_width = gt_width;
  a.gt_len = gt_len;
  a.row_flip = row_flip;
  a.n_cols = n_cols;
  a.n_slots = n_slots;
  a.col_of_slot = col_of_slot;
  a.first_col = first_col < 0 ? -1 : first_col;
  a.ploidy_of_slot = ploidy_of_slot;
  a.uniform_ploidy = uniform_ploidy;
  a.out = out;
  a.status = status;
  a.e_begin = out_row0 * n_slots;
  a.e_end = (out_row0 + n_out_rows) * n_slots;
  a.chunk0 = a.e_begin / 16;
  a.n_chunks = (a.e_end + 15) / 16 - a.chunk0;
  const int64_t blocks = (a.n_chunks + kBcfBlock - 1) / kBcfBlock;
  // 2^24 blocks of 256 lanes are 2^32 threads, the most one launch takes: 64 GiB of output
  if (blocks > (1ll << 24)) return fail(SAI_ERR_UNSUPPORTED, "more than 2^24 blocks (64 GiB) of output in one call: decode the rows in several calls");
  hipStream_t st = static_cast<hipStream_t>(stream);
  SAI_HIP(hipMemsetAsync(status, 0, static_cast<size_t>(n_out_rows) * sizeof(int32_t), st));
  hipLaunchKernelGGL(bcf_decode_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kBcfBlock), 0, st, a);
  return check_launch("bcf_decode");
}
