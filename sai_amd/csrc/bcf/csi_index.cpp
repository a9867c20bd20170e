// The .csi index of a BCF file: loaded, parsed, validated and asked where a region's walk may begin
// (include/saihip_bcf_index.h; DESIGN_INGEST.md, "BCF files: a region is a seek").  Plain C++: part of libsaihip and
// of the sanitizer build of the host units.

#include "csi_index.hpp"

#include "../ingest_base.hpp"

namespace csi {

namespace {

struct Reader {
  const unsigned char* d;
  size_t n, o = 0;
  size_t left() const { return n - o; }
  uint32_t u32() { const uint32_t v = le32(d + o); o += 4; return v; }
  int32_t i32() { return static_cast<int32_t>(u32()); }
  uint64_t u64() { const uint64_t lo = u32(); return lo | static_cast<uint64_t>(u32()) << 32; }
};

}  // namespace

bool parse(const unsigned char* d, size_t n, int64_t data_file_bytes, Index& out, std::string& why) {
  auto fail = [&](const char* what) { why = what; return false; };
  Reader r{d, n};
  if (r.left() < 16) return fail("the stream ends inside the magic, min_shift, depth and l_aux");
  if (memcmp(d, "CSI\1", 4) != 0) return fail("the magic is not CSI\\1");
  r.o = 4;
  out = Index();
  out.min_shift = r.i32();
  out.depth = r.i32();
  const int32_t l_aux = r.i32();
  if (out.min_shift < 0 || out.depth < 0 || out.depth > 10 || out.min_shift + 3 * out.depth > 62) return fail("min_shift or depth is out of range");
  if (l_aux < 0 || static_cast<size_t>(l_aux) > r.left()) return fail("l_aux leaves the stream");
  r.o += static_cast<size_t>(l_aux);
  if (r.left() < 4) return fail("the stream ends before n_ref");
  const int32_t n_ref = r.i32();
  if (n_ref < 0 || static_cast<size_t>(n_ref) > r.left() / 4) return fail("n_ref leaves the stream");
  const uint64_t pseudo = Index::level_start(out.depth + 1) + 1;
  const uint64_t size = data_file_bytes < 0 ? 0 : static_cast<uint64_t>(data_file_bytes);
  auto inside = [&](uint64_t v) { return (v >> 16) < size; };
  out.refs.resize(static_cast<size_t>(n_ref));
  for (Ref& ref : out.refs) {
    if (r.left() < 4) return fail("the stream ends before n_bin");
    const int32_t n_bin = r.i32();
    if (n_bin < 0 || static_cast<size_t>(n_bin) > r.left() / 16) return fail("n_bin leaves the stream");
    for (int32_t b = 0; b < n_bin; ++b) {
      if (r.left() < 16) return fail("the stream ends inside a bin");
      Bin bin;
      bin.bin = r.u32();
      bin.loffset = r.u64();
      const int32_t n_chunk = r.i32();
      if (n_chunk < 0 || static_cast<size_t>(n_chunk) > r.left() / 16) return fail("n_chunk leaves the stream");
      if (bin.bin == pseudo) {  // counts, not chunks of records
        r.o += static_cast<size_t>(n_chunk) * 16;
        continue;
      }
      if (bin.bin > pseudo - 2) return fail("a bin number beyond the last level");
      if (!inside(bin.loffset)) return fail("a loffset beyond the data file");
      bin.first_chunk = static_cast<uint32_t>(out.chunks.size());
      bin.n_chunk = static_cast<uint32_t>(n_chunk);
      if (out.chunks.size() + static_cast<size_t>(n_chunk) > 0xFFFFFFFFull) return fail("too many chunks");
      for (int32_t c = 0; c < n_chunk; ++c) {
        Chunk ch;
        ch.beg = r.u64();
        ch.end = r.u64();
        if (ch.beg >= ch.end) return fail("chunk_beg >= chunk_end");
        if (!inside(ch.beg) || !inside(ch.end)) return fail("a chunk beyond the data file");
        ref.lo = std::min(ref.lo, ch.beg);
        ref.hi = std::max(ref.hi, ch.end);
        out.chunks.push_back(ch);
      }
      ref.bins.push_back(bin);
    }
    std::sort(ref.bins.begin(), ref.bins.end(), [](const Bin& a, const Bin& b) { return a.bin < b.bin; });
    for (size_t k = 1; k < ref.bins.size(); ++k)
      if (ref.bins[k].bin == ref.bins[k - 1].bin) return fail("a bin is listed twice");
  }
  if (r.left() == 8) out.n_no_coor = static_cast<int64_t>(r.u64());
  else if (r.left() != 0) return fail("bytes are left behind the last reference that are not n_no_coor");
  return true;
}

bool load(const char* path, int64_t data_file_bytes, Index& out, std::string& why) {
  auto fail = [&](const char* what) { why = what; return false; };
  FILE* f = fopen(path, "rb");
  if (!f) return fail("cannot be opened");
  std::vector<unsigned char> comp;
  unsigned char block[1 << 16];
  size_t got;
  while ((got = fread(block, 1, sizeof(block), f)) > 0) {
    comp.insert(comp.end(), block, block + got);
    if (comp.size() > (size_t(1) << 30)) break;
  }
  const bool read_error = ferror(f) != 0;
  fclose(f);
  if (read_error) return fail("read error");
  if (comp.size() > (size_t(1) << 30)) return fail("larger than 1 GiB");
  std::vector<char> text;
  Inflater inf;
  for (size_t off = 0; off < comp.size();) {
    size_t hlen = 0;
    const long bsize = bgzf_member_size(comp.data() + off, comp.size() - off, &hlen);
    if (bsize <= 0 || off + static_cast<size_t>(bsize) > comp.size() || static_cast<size_t>(bsize) < hlen + 8) return fail("not a BGZF file, or a truncated one");
    const unsigned char* tail = comp.data() + off + bsize - 8;
    const uint32_t isize = le32(tail + 4);
    if (isize > 65536u) return fail("a BGZF block with ISIZE > 64 KiB");
    const BgzfMember mem{off + hlen, static_cast<uint32_t>(static_cast<size_t>(bsize) - hlen - 8), isize, le32(tail), text.size()};
    text.resize(text.size() + isize);
    if (!inflate_member(comp.data(), mem, text.data(), inf)) return fail("a BGZF block fails to inflate or its CRC");
    off += static_cast<size_t>(bsize);
  }
  return parse(reinterpret_cast<const unsigned char*>(text.data()), text.size(), data_file_bytes, out, why);
}

int Index::query(int32_t tid, int64_t start, int64_t end, uint64_t* v) const {
  if (tid < 0 || static_cast<size_t>(tid) >= refs.size()) return SAI_BCF_INDEX_WALK;
  const uint64_t range = uint64_t(1) << (min_shift + 3 * depth);
  const uint64_t beg = start <= 0 ? 0 : static_cast<uint64_t>(start) - 1;
  const uint64_t fin = end < 0 ? range : std::min(static_cast<uint64_t>(end), range);
  if (beg >= range || fin <= beg) return SAI_BCF_INDEX_WALK;
  const Ref& ref = refs[static_cast<size_t>(tid)];
  if (ref.bins.empty()) return SAI_BCF_INDEX_NONE;
  // the walk takes the first contiguous run of a chromosome: where the index shows the contig's records mixed with
  // another one's, only a walk from the start knows which run that is
  for (size_t k = 0; k < refs.size(); ++k)
    if (k != static_cast<size_t>(tid) && refs[k].lo < ref.hi && ref.lo < refs[k].hi) return SAI_BCF_INDEX_WALK;
  // floor: the loffset of the leaf bin that holds beg, or of the nearest leaf bin before it
  const uint64_t leaf0 = level_start(depth), want_leaf = leaf0 + (beg >> min_shift);
  uint64_t floor = 0;
  for (const Bin& b : ref.bins)
    if (b.bin >= leaf0 && b.bin <= want_leaf) floor = b.loffset;  // sorted: the last one wins
  uint64_t best = ~0ull;
  int level = 0;
  for (const Bin& b : ref.bins) {
    while (level < depth && b.bin >= level_start(level + 1)) ++level;
    const int s = min_shift + 3 * (depth - level);
    // the bins that overlap [beg, range), not only those of [beg, fin): the index is not used for the end, and a
    // region that holds no record then still begins at or before the first record behind it, never behind that
    if (b.bin - level_start(level) < (beg >> s)) continue;
    for (uint32_t c = 0; c < b.n_chunk; ++c) {
      const Chunk& ch = chunks[b.first_chunk + c];
      if (ch.end > floor) best = std::min(best, ch.beg);
    }
  }
  if (best == ~0ull) return SAI_BCF_INDEX_NONE;
  *v = best;
  return SAI_BCF_INDEX_SEEK;
}

}  // namespace csi

extern "C" {

int sai_bcf_index_abi_version(void) { return SAI_BCF_INDEX_ABI_VERSION; }

int sai_bcf_index_open(const char* index_path, int64_t data_file_bytes, sai_bcf_index** index_out) {
  return guarded("sai_bcf_index_open", [&]() -> int {
    if (!index_path || !index_out) return sai_set_error(SAI_ERR_ARG, "NULL argument");
    *index_out = nullptr;
    if (data_file_bytes < 0) return sai_set_error(SAI_ERR_ARG, "data_file_bytes must not be negative");
    std::unique_ptr<sai_bcf_index> idx(new sai_bcf_index);
    std::string why;
    if (!csi::load(index_path, data_file_bytes, idx->ix, why)) return sai_set_error(SAI_ERR_ARG, "%s: the index is not used: %s", index_path, why.c_str());
    *index_out = idx.release();
    return SAI_OK;
  });
}

int sai_bcf_index_info(const sai_bcf_index* index, int32_t* min_shift, int32_t* depth, int32_t* n_ref, int64_t* n_no_coor) {
  if (!index) return sai_set_error(SAI_ERR_ARG, "NULL argument");
  if (min_shift) *min_shift = index->ix.min_shift;
  if (depth) *depth = index->ix.depth;
  if (n_ref) *n_ref = static_cast<int32_t>(index->ix.refs.size());
  if (n_no_coor) *n_no_coor = index->ix.n_no_coor;
  return SAI_OK;
}

int sai_bcf_index_query(const sai_bcf_index* index, int32_t contig, int64_t start, int64_t end, int32_t* answer, uint64_t* voffset) {
  if (!index || !answer || !voffset) return sai_set_error(SAI_ERR_ARG, "NULL argument");
  *voffset = 0;
  *answer = index->ix.query(contig, start, end, voffset);
  return SAI_OK;
}

int sai_bcf_index_close(sai_bcf_index* index) {
  delete index;
  return SAI_OK;
}

}  // extern "C"
