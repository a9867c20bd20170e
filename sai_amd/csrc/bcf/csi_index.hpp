// The parsed form of a .csi index (CSI v1) and its one query (include/saihip_bcf_index.h; DESIGN_INGEST.md, "BCF
// files: a region is a seek").  Defined in csi_index.cpp; bcf_index.cpp and bcf_feed.cpp ask it where to begin.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "saihip_bcf_index.h"

namespace csi {

struct Chunk {
  uint64_t beg, end;  // virtual offsets, beg < end
};

struct Bin {
  uint32_t bin;
  uint64_t loffset;
  uint32_t first_chunk, n_chunk;  // in Index::chunks
};

struct Ref {
  std::vector<Bin> bins;            // by bin number, the pseudo-bin left out
  uint64_t lo = ~0ull, hi = 0;      // smallest chunk_beg and largest chunk_end of the reference
};

struct Index {
  int32_t min_shift = 0, depth = 0;
  int64_t n_no_coor = -1;  // -1: the stream ends without it
  std::vector<Ref> refs;
  std::vector<Chunk> chunks;

  // first bin number of level l
  static uint64_t level_start(int l) { return ((uint64_t(1) << (3 * l)) - 1) / 7; }
  // one of SAI_BCF_INDEX_NONE / _SEEK / _WALK for the 1-based inclusive [start, end] (-1 = open) of reference tid
  int query(int32_t tid, int64_t start, int64_t end, uint64_t* v) const;
};

// The inflated bytes of an index -> its parsed form, every field checked before use.  false: `why` says what is wrong.
bool parse(const unsigned char* d, size_t n, int64_t data_file_bytes, Index& out, std::string& why);
// The BGZF file at `path`, inflated and parsed.
bool load(const char* path, int64_t data_file_bytes, Index& out, std::string& why);

}  // namespace csi

struct sai_bcf_index {
  csi::Index ix;
};
