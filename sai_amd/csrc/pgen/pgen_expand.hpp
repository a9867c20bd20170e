// The expand half of the .pgen kernels, shared by pgen_decode.hip (int8 rows) and pgen_pack2.hip (packed2 blocks):
// one record -> the dense 2-bit codes of a window [s0, s1) of its samples in LDS, in the .bed bit order (sample
// s0 + 16 w + k in bits [2k, 2k + 2) of word w).  Moved here from pgen_decode.hip as it stood; what each step does
// and checks is described at the top of that file.
//
// Every function is called by ALL 64 lanes of a single-wave workgroup: the __syncthreads() inside are barriers of
// that one wavefront.  A kernel that puts several rows' waves into one workgroup must replace every one of them
// (rows diverge: a bad record returns early, record types differ), or the workgroup hangs.
// s0 must be a multiple of 16 (a type 0 / type 1 record is copied from the byte that holds sample s0).
#pragma once

#include "../common.hpp"
#include "pgen_codes.hpp"

namespace {

constexpr int kWave = 64;
constexpr int kTileWords = 1024;                // 32-bit words of LDS per wavefront
constexpr uint32_t kTileSamples = kTileWords * 16;

// a record inside the batch (wave-uniform)
struct Record {
  const uint8_t* p;
  int64_t len;
  uint32_t kind;
  bool ok;  // the span lies inside the batch
};

// Args: the kernel's argument block, of which `bytes` and `n_bytes` are the batch
template <class Args>
__device__ __forceinline__ Record load_record(const Args& a, const int64_t* t) {
  Record r;
  const int64_t off = t[0];
  r.len = t[1];
  r.kind = static_cast<uint32_t>(t[2]) & 7u;
  r.ok = off >= 0 && r.len >= 0 && off <= a.n_bytes && r.len <= a.n_bytes - off;
  r.p = a.bytes + (r.ok ? off : 0);
  return r;
}

__device__ __forceinline__ void put_code(uint32_t* tile, uint32_t s0, uint32_t s1, uint32_t sample, uint32_t code) {
  if (sample < s0 || sample >= s1) return;
  const uint32_t rel = sample - s0;  // < kTileSamples
  const uint32_t sh = 2 * (rel & 15u);
  atomicAnd(tile + (rel >> 4), ~(3u << sh));
  atomicOr(tile + (rel >> 4), code << sh);
}

// The difflist that starts at byte `at` of the record: its entries of [s0, s1) overwrite the tile.  With `validate`
// every group is walked and checked; without, only the groups that can hold an entry of the tile (the list was
// validated by the row's first tile).  Returns, to every lane, whether the list is sound.
__device__ bool walk_difflist(const Record& r, int64_t at, uint32_t n, uint32_t s0, uint32_t s1, bool validate, uint32_t* tile) {
  const int lane = threadIdx.x;
  const uint8_t* p = r.p;
  const int64_t len = r.len;
  uint64_t L = 0;
  bool ended = false;
  for (int k = 0; k < kPgenMaxVarint && at < len; ++k) {
    const uint32_t b = p[at++];
    L |= static_cast<uint64_t>(b & 0x7Fu) << (7 * k);
    if (!(b & 0x80u)) {
      ended = true;
      break;
    }
  }
  if (!ended) return false;
  if (L == 0) return true;
  if (L > n) return false;
  const int64_t G = static_cast<int64_t>((L + kPgenGroup - 1) / kPgenGroup);
  const int w = pgen_index_width(n);
  const int64_t code_len = static_cast<int64_t>((L + 3) / 4);
  if (len - at < G * w + (G - 1) + code_len) return false;
  const int64_t firsts = at, sizes = firsts + G * w, code_at = sizes + (G - 1);
  int64_t carry = code_at + code_len;  // where the delta bytes of the round's first group start
  int32_t prev_last = -1;              // the last sample of the group before the round's first
  bool ok = true;
  for (int64_t g0 = 0; g0 < G; g0 += kWave) {
    const int64_t g = g0 + lane;
    const bool active = g < G;
    const bool inner = g + 1 < G;  // every group but the last has a stored byte size
    const int32_t size = inner ? static_cast<int32_t>(p[sizes + g]) + (kPgenGroup - 1) : 0;
    int32_t incl = size;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
      const int32_t t = __shfl_up(incl, off);
      if (lane >= off) incl += t;
    }
    const int64_t d0 = carry + (incl - size);
    const int64_t group_end = inner ? d0 + size : len;
    carry += __shfl(incl, kWave - 1);
    int32_t first = -1, last = -1;
    if (active) {
      uint32_t at_sample = 0;
      for (int k = 0; k < w; ++k) at_sample |= static_cast<uint32_t>(p[firsts + g * w + k]) << (8 * k);
      bool walk = group_end <= len && at_sample < n;
      if (!walk) ok = false;
      first = last = static_cast<int32_t>(at_sample & 0x7FFFFFFFu);
      if (walk && !validate) {  // can the group hold an entry of the tile?
        uint32_t next_first = n;
        if (inner) {
          next_first = 0;
          for (int k = 0; k < w; ++k) next_first |= static_cast<uint32_t>(p[firsts + (g + 1) * w + k]) << (8 * k);
        }
        walk = at_sample < s1 && next_first > s0;
      }
      if (walk) {
        const int64_t k0 = g * kPgenGroup;
        const int cnt = static_cast<int>(L - static_cast<uint64_t>(k0) < static_cast<uint64_t>(kPgenGroup) ? L - static_cast<uint64_t>(k0) : kPgenGroup);
        uint32_t code_byte = p[code_at + (k0 >> 2)];
        put_code(tile, s0, s1, at_sample, code_byte & 3u);
        int64_t d = d0;
        for (int j = 1; j < cnt; ++j) {
          uint64_t delta = 0;
          bool whole = false;
          for (int k = 0; k < kPgenMaxVarint && d < group_end; ++k) {
            const uint32_t b = p[d++];
            delta |= static_cast<uint64_t>(b & 0x7Fu) << (7 * k);
            if (!(b & 0x80u)) {
              whole = true;
              break;
            }
          }
          const uint64_t next = at_sample + delta;
          if (!whole || delta == 0 || next >= n) {
            ok = false;
            break;
          }
          at_sample = static_cast<uint32_t>(next);
          if ((j & 3) == 0) code_byte = p[code_at + ((k0 + j) >> 2)];
          put_code(tile, s0, s1, at_sample, (code_byte >> (2 * (j & 3))) & 3u);
        }
        if (ok && inner && d != group_end) ok = false;
        last = static_cast<int32_t>(at_sample);
      }
    }
    // strict increase from group to group: the neighbour lane's last sample
    int32_t before = __shfl_up(last, 1);
    if (lane == 0) before = prev_last;
    if (active && validate && first <= before) ok = false;
    prev_last = __shfl(last, kWave - 1);
  }
  return __all(ok);
}

// 16 bits -> 16 two-bit fields, bit k to bit 2k
__device__ __forceinline__ uint32_t spread16(uint32_t x) {
  x = (x | (x << 8)) & 0x00FF00FFu;
  x = (x | (x << 4)) & 0x0F0F0F0Fu;
  x = (x | (x << 2)) & 0x33333333u;
  x = (x | (x << 1)) & 0x55555555u;
  return x;
}

// A record that stands alone (type 0, 1, 4, 6, 7): the codes of [s0, s1) into the tile, its difflist applied.
// Returns, to every lane, whether the record is sound; the tile is then complete and visible to the wavefront.
__device__ bool expand_alone(const Record& r, uint32_t n, uint32_t s0, uint32_t s1, bool validate, uint32_t* tile) {
  const int lane = threadIdx.x;
  if (!r.ok) return false;
  const int n_words = static_cast<int>((s1 - s0 + 15u) >> 4);
  int64_t list_at = 0;
  if (r.kind == 0) {
    const int64_t row_bytes = (static_cast<int64_t>(n) + 3) >> 2;
    if (r.len < row_bytes) return false;
    for (int wd = lane; wd < n_words; wd += kWave) {
      const int64_t b0 = (static_cast<int64_t>(s0) >> 2) + 4 * wd;
      uint32_t word = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (b0 + k < row_bytes) word |= static_cast<uint32_t>(r.p[b0 + k]) << (8 * k);
      tile[wd] = word;
    }
    __syncthreads();
    return true;
  }
  if (r.kind == 1) {
    const int64_t bit_bytes = (static_cast<int64_t>(n) + 7) >> 3;
    if (r.len < 1 + bit_bytes) return false;
    const uint32_t b = r.p[0];
    if (!pgen_onebit_legal(b)) return false;
    const uint32_t lo = b >> 2, step = b & 3u;  // hi = lo + step <= 3: no field carries into the next
    for (int wd = lane; wd < n_words; wd += kWave) {
      const int64_t b0 = (static_cast<int64_t>(s0) >> 3) + 2 * wd;
      uint32_t bits = 0;
      if (b0 < bit_bytes) bits = r.p[1 + b0];
      if (b0 + 1 < bit_bytes) bits |= static_cast<uint32_t>(r.p[2 + b0]) << 8;
      tile[wd] = lo * 0x55555555u + spread16(bits) * step;
    }
    list_at = 1 + bit_bytes;
  } else if (r.kind == 4 || r.kind == 6 || r.kind == 7) {
    const uint32_t fill = r.kind == 4 ? 0u : r.kind == 6 ? 0xAAAAAAAAu : 0xFFFFFFFFu;
    for (int wd = lane; wd < n_words; wd += kWave) tile[wd] = fill;
  } else {
    return false;  // 5 is reserved; 2 and 3 are no base
  }
  __syncthreads();
  const bool ok = walk_difflist(r, list_at, n, s0, s1, validate, tile);
  __syncthreads();
  return ok;
}

// The row's record into the tile, as a macro and no function: the statements stand in pgen_decode_kernel exactly as
// they did before they were shared (as a function the kernel's code came out differently; see DESIGN_INGEST.md).
// OWN / FROM = the row's record and, when it is of type 2 or 3 (DERIVED), its base; BASE_OFF = the base's offset as
// the caller names it (-1: none).  The base is expanded by expand_alone, type 3 then exchanges the codes 0 and 2
// word by word, then the row's own difflist is applied.  Declares `bool OK`: to every lane, whether the row is sound.
#define SAI_PGEN_EXPAND_ROW(OK, OWN, FROM, DERIVED, BASE_OFF, N, S0, S1, VALIDATE, TILE, LANE)                           \
  bool OK;                                                                                                             \
  if (DERIVED) {                                                                                                       \
    OK = (OWN).ok && (BASE_OFF) >= 0 && expand_alone(FROM, N, S0, S1, VALIDATE, TILE);                                 \
    if (OK) {                                                                                                          \
      if ((OWN).kind == 3) { /* 0 <-> 2: the high bit of a field whose low bit is clear; 1 and 3 stay */               \
        const int n_words = static_cast<int>(((S1) - (S0) + 15u) >> 4);                                                \
        for (int wd = LANE; wd < n_words; wd += kWave) (TILE)[wd] ^= (~(TILE)[wd] & 0x55555555u) << 1;                 \
        __syncthreads();                                                                                               \
      }                                                                                                                \
      OK = walk_difflist(OWN, 0, N, S0, S1, VALIDATE, TILE);                                                           \
      __syncthreads();                                                                                                 \
    }                                                                                                                  \
  } else {                                                                                                             \
    OK = expand_alone(OWN, N, S0, S1, VALIDATE, TILE);                                                                 \
  }

}  // namespace
