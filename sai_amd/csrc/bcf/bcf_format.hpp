// What the two host units of the BCF reader share (bcf_index.cpp: the host walk and its stream; bcf_feed.cpp: the
// feed of the GPU route): the inflated stream of a BGZF file, the typed values, the header with its dictionaries,
// the resolution of the sample names and the row selection of a record's fixed fields.  Header-only with internal
// linkage, as ingest_base.hpp is: every unit compiles its own copy.
#pragma once

#include "../ingest_base.hpp"
#include "saihip_bcf.h"

#include <chrono>
namespace {

constexpr size_t kInflateStep = size_t(4) << 20;  // inflated bytes asked of the source at a time

inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// ---- the inflated stream -----------------------------------------------------------------------------------

// The members of a BGZF file, inflated by `n_threads` threads and appended to the caller's buffer.
struct BgzfSource {
  std::string path;
  FILE* f = nullptr;
  WorkerPool pool;
  std::vector<unsigned char> cbuf;
  size_t chave = 0;
  bool ceof = false;
  double read_s = 0.0, inflate_s = 0.0;  // seconds in fread / in inflate_member (the threads' wall time)
  int64_t inflated_bytes = 0;
  int64_t file_bytes = 0, n_members = 0;  // the members inflated so far: their bytes in the file, their number
  std::vector<BgzfMember> members;
  BgzfSource(const char* p, int n_threads) : path(p), pool(n_threads), cbuf(size_t(1) << 20) {}
  ~BgzfSource() { if (f) fclose(f); }
  BgzfSource(const BgzfSource&) = delete;
  BgzfSource& operator=(const BgzfSource&) = delete;

  int open() {
    if (f) fclose(f);  // once more from the start
    chave = 0;
    ceof = false;
    f = fopen(path.c_str(), "rb");
    if (!f) return sai_set_error(SAI_ERR_ARG, "cannot open BCF %s", path.c_str());
    unsigned char head[64];
    const size_t n = fread(head, 1, sizeof(head), f);
    size_t hlen = 0;
    if (n >= 3 && memcmp(head, "BCF", 3) == 0)
      return sai_set_error(SAI_ERR_UNSUPPORTED, "%s: a raw (uncompressed) BCF is not read: compress it with bgzip (bcftools view -Ob)", path.c_str());
    if (bgzf_member_size(head, n, &hlen) <= 0) return sai_set_error(SAI_ERR_ARG, "%s: not a BGZF file", path.c_str());
    if (fseeko(f, 0, SEEK_SET) != 0) return sai_set_error(SAI_ERR_ARG, "seek failed in %s", path.c_str());
    return SAI_OK;
  }

  // the file offset of the next member fill() will inflate
  int64_t next_member_off() const { return static_cast<int64_t>(ftello(f)) - static_cast<int64_t>(chave); }

  // fill() goes on with the member at file offset `coffset`
  bool seek(int64_t coffset) {
    chave = 0;
    ceof = false;
    return fseeko(f, static_cast<off_t>(coffset), SEEK_SET) == 0;
  }

  // Appends the inflated bytes of the next members to out[have ..): at least one byte unless the file has ended
  // (*eof), about `want` where the file has them.
  int fill(std::vector<char>& out, size_t& have, size_t want, bool* eof) {
    *eof = false;
    for (;;) {
      if (!ceof && chave < cbuf.size()) {
        const double t0 = now_s();
        const size_t got = fread(cbuf.data() + chave, 1, cbuf.size() - chave, f);
        read_s += now_s() - t0;
        if (got == 0) {
          if (ferror(f)) return sai_set_error(SAI_ERR_ARG, "read error in %s", path.c_str());
          ceof = true;
        }
        chave += got;
      }
      members.clear();
      size_t off = 0, out_total = 0;
      while (off < chave && out_total < want) {
        size_t hlen = 0;
        const long bsize = bgzf_member_size(cbuf.data() + off, chave - off, &hlen);
        if (bsize < 0) return sai_set_error(SAI_ERR_ARG, "%s: corrupt BGZF block", path.c_str());
        if (bsize == 0 || off + static_cast<size_t>(bsize) > chave) break;  // incomplete member
        if (static_cast<size_t>(bsize) < hlen + 8) return sai_set_error(SAI_ERR_ARG, "%s: corrupt BGZF block", path.c_str());
        const unsigned char* tail = cbuf.data() + off + bsize - 8;
        if (le32(tail + 4) > 65536u) return sai_set_error(SAI_ERR_ARG, "%s: corrupt BGZF block (ISIZE > 64 KiB)", path.c_str());
        members.push_back({off + hlen, static_cast<uint32_t>(static_cast<size_t>(bsize) - hlen - 8), le32(tail + 4), le32(tail), out_total});
        out_total += le32(tail + 4);
        off += static_cast<size_t>(bsize);
      }
      if (members.empty()) {
        if (ceof) {
          if (chave) return sai_set_error(SAI_ERR_ARG, "%s: truncated BGZF file", path.c_str());
          *eof = true;
          return SAI_OK;
        }
        if (chave == cbuf.size()) cbuf.resize(cbuf.size() * 2);
        continue;
      }
      if (out.size() < have + out_total) out.resize(have + out_total);
      const int nt = std::max(1, std::min<int>(pool.size(), static_cast<int>(members.size())));
      std::vector<char> bad(static_cast<size_t>(nt), 0);
      char* dst = out.data() + have;
      auto work = [&](int t) {  // inflate_member allocates nothing but the decompressor's own state: no throw
        const size_t lo = members.size() * static_cast<size_t>(t) / static_cast<size_t>(nt);
        const size_t hi = members.size() * static_cast<size_t>(t + 1) / static_cast<size_t>(nt);
        Inflater inf;
        for (size_t i = lo; i < hi; ++i)
          if (!inflate_member(cbuf.data(), members[i], dst, inf)) bad[static_cast<size_t>(t)] = 1;
      };
      const double t0 = now_s();
      pool.run(nt, work);
      inflate_s += now_s() - t0;
      inflated_bytes += static_cast<int64_t>(out_total);
      file_bytes += static_cast<int64_t>(off);
      n_members += static_cast<int64_t>(members.size());
      for (char b : bad)
        if (b) return sai_set_error(SAI_ERR_ARG, "%s: BGZF block fails to inflate or its CRC", path.c_str());
      memmove(cbuf.data(), cbuf.data() + off, chave - off);
      chave -= off;
      have += out_total;
      if (out_total) return SAI_OK;  // only empty members (the EOF marker): read on
    }
  }
};

// ---- typed values ----------------------------------------------------------------------------------------

struct Cursor {
  const unsigned char* p;
  const unsigned char* end;
};

inline int type_width(int type) { return type == 1 || type == 7 ? 1 : type == 2 ? 2 : type == 3 || type == 5 ? 4 : type == 0 ? 0 : -1; }

inline int64_t read_int(const unsigned char* p, int width) {
  if (width == 1) return static_cast<int8_t>(p[0]);
  if (width == 2) return static_cast<int16_t>(static_cast<uint16_t>(p[0] | p[1] << 8));
  return static_cast<int32_t>(le32(p));
}

// one typed integer scalar
bool typed_int(Cursor& c, int64_t* v) {
  if (c.p >= c.end) return false;
  const int desc = *c.p++;
  const int type = desc & 15, width = type_width(type);
  if ((desc >> 4) != 1 || type < 1 || type > 3 || c.end - c.p < width) return false;
  *v = read_int(c.p, width);
  c.p += width;
  return true;
}

// descriptor of a typed value: its type and count (a count of 15 is followed by the real one)
bool typed_desc(Cursor& c, int* type, int64_t* count) {
  if (c.p >= c.end) return false;
  const int desc = *c.p++;
  *type = desc & 15;
  *count = desc >> 4;
  if (*count == 15 && (!typed_int(c, count) || *count < 0)) return false;
  return type_width(*type) >= 0;
}

// a typed string: where it lies
bool typed_string(Cursor& c, const char** s, size_t* n) {
  int type;
  int64_t count;
  if (!typed_desc(c, &type, &count)) return false;
  if (type == 0) count = 0;
  else if (type != 7) return false;
  if (c.end - c.p < count) return false;
  *s = reinterpret_cast<const char*>(c.p);
  *n = static_cast<size_t>(count);
  c.p += count;
  return true;
}

// ---- header --------------------------------------------------------------------------------------------

struct BcfHeader {
  std::vector<std::string> contig;      // by dictionary index
  std::vector<char> contig_defined;
  int64_t gt_key = -1;                  // index of "GT" in the string dictionary, -1 if it is not there
  std::vector<std::string> samples;
  size_t data_off = 0;                  // where the records start in the inflated stream
};

// ID=... and IDX=... of a structured header line "##KEY=<...>" (values may be quoted)
void line_id_idx(const char* p, const char* end, std::string* id, int64_t* idx) {
  *idx = -1;
  id->clear();
  while (p < end && *p != '>') {
    const char* key = p;
    while (p < end && *p != '=' && *p != ',' && *p != '>') ++p;
    const size_t key_len = static_cast<size_t>(p - key);
    const char* val = p;
    size_t val_len = 0;
    if (p < end && *p == '=') {
      ++p;
      if (p < end && *p == '"') {
        val = ++p;
        while (p < end && *p != '"') { if (*p == '\\' && p + 1 < end) ++p; ++p; }
        val_len = static_cast<size_t>(p - val);
        if (p < end) ++p;
      } else {
        val = p;
        while (p < end && *p != ',' && *p != '>') ++p;
        val_len = static_cast<size_t>(p - val);
      }
    }
    if (key_len == 2 && memcmp(key, "ID", 2) == 0 && id->empty()) id->assign(val, val_len);
    if (key_len == 3 && memcmp(key, "IDX", 3) == 0) {
      int64_t v = 0;
      bool digits = val_len > 0;
      for (size_t i = 0; i < val_len; ++i) {
        if (val[i] < '0' || val[i] > '9' || v > (int64_t(1) << 40)) { digits = false; break; }
        v = v * 10 + (val[i] - '0');
      }
      if (digits) *idx = v;
    }
    if (p < end && *p == ',') ++p;
  }
}

// The header text -> dictionaries and sample names.  0, or a negative status.
int parse_bcf_header(const char* text, size_t n, const char* path, BcfHeader& h) {
  std::unordered_map<std::string, int64_t> strings, contigs;
  strings.emplace("PASS", 0);
  int64_t next_string = 1, next_contig = 0;
  bool have_chrom_line = false;
  const char* p = text;
  const char* end = text + n;
  while (p < end && *p) {
    const char* eol = static_cast<const char*>(memchr(p, '\n', static_cast<size_t>(end - p)));
    if (!eol) eol = end;
    const char* le = eol;
    while (le > p && (le[-1] == '\r' || le[-1] == '\0')) --le;
    const size_t len = static_cast<size_t>(le - p);
    auto starts = [&](const char* s) { const size_t k = strlen(s); return len >= k && memcmp(p, s, k) == 0; };
    std::string id;
    int64_t idx;
    if (starts("##contig=<")) {
      line_id_idx(p + 10, le, &id, &idx);
      if (!id.empty() && !contigs.count(id)) {
        if (idx < 0) idx = next_contig;
        if (idx > (int64_t(1) << 24)) return sai_set_error(SAI_ERR_ARG, "%s: contig %s has IDX=%lld", path, id.c_str(), static_cast<long long>(idx));
        contigs.emplace(id, idx);
        next_contig = std::max(next_contig, idx + 1);
        if (h.contig.size() <= static_cast<size_t>(idx)) { h.contig.resize(static_cast<size_t>(idx) + 1); h.contig_defined.resize(static_cast<size_t>(idx) + 1, 0); }
        h.contig[static_cast<size_t>(idx)] = id;
        h.contig_defined[static_cast<size_t>(idx)] = 1;
      }
    } else if (starts("##FILTER=<") || starts("##INFO=<") || starts("##FORMAT=<")) {
      const char* lt = static_cast<const char*>(memchr(p, '<', len));
      line_id_idx(lt + 1, le, &id, &idx);
      if (!id.empty() && !strings.count(id)) {
        if (idx < 0) idx = next_string;
        strings.emplace(id, idx);
        next_string = std::max(next_string, idx + 1);
      }
    } else if (starts("#CHROM")) {
      have_chrom_line = true;
      const char* q = p;
      int c = 0;
      while (q <= le) {
        const char* t = find_tab(q, le);
        if (c >= 9) h.samples.emplace_back(q, static_cast<size_t>(t - q));
        q = t + 1;
        ++c;
      }
    }
    p = eol < end ? eol + 1 : end;
  }
  if (!have_chrom_line) return sai_set_error(SAI_ERR_ARG, "%s: the BCF header has no #CHROM line", path);
  const auto gt = strings.find("GT");
  h.gt_key = gt == strings.end() ? -1 : gt->second;
  return SAI_OK;
}

// ---- the row selection ------------------------------------------------------------------------------------

// The rows of one chromosome inside [start, stop] (-1 = open; 1-based), first contiguous run only, as parse_lines()
// selects them: step() takes the fixed fields of every record in file order.
struct RowSelect {
  enum { kSkip = 0, kStop = 1, kRow = 2 };
  int target = -1;        // dictionary index of the chromosome, -1 when the header does not define it
  int64_t start = -1, stop = -1;
  bool whole_file = false;  // go on counting records behind the run (the scan)
  bool seen = false, run_over = false;
  int64_t first = -1, last = -1, n_matched = 0;

  void aim(const BcfHeader& h, const std::string& chrom) {
    target = -1;
    for (size_t i = 0; i < h.contig.size(); ++i)
      if (h.contig_defined[i] && h.contig[i] == chrom) target = static_cast<int>(i);
  }

  int step(int32_t chrom_idx, int64_t pos) {
    if (chrom_idx != target) {
      if (seen) run_over = true;
      return run_over && !whole_file ? kStop : kSkip;
    }
    if (run_over) return kSkip;
    seen = true;
    if (first < 0) first = pos;
    last = pos;
    if (stop >= 0 && pos > stop) return whole_file ? kSkip : kStop;  // the run has passed the region
    if (start >= 0 && pos < start) return kSkip;
    ++n_matched;
    return kRow;
  }
};

// the ancestral-allele rule on REF and the first ALT: 1 = flip, 0 = keep, -1 = drop
inline int anc_decision(const AncAllele& a, const char* ref, size_t ref_len, const char* alt, size_t alt_len) {
  if (a.size() == alt_len && memcmp(a.data(), alt, alt_len) == 0) return 1;
  if (a.size() == ref_len && memcmp(a.data(), ref, ref_len) == 0) return 0;
  return -1;
}

int resolve_samples(const BcfHeader& h, const char* path, const std::vector<std::string>& names, std::vector<int32_t>& col_of_slot) {
  std::unordered_map<std::string, int32_t> index;
  for (size_t i = 0; i < h.samples.size(); ++i) index.emplace(h.samples[i], static_cast<int32_t>(i));
  col_of_slot.clear();
  for (const std::string& nme : names) {
    const auto it = index.find(nme);
    if (it == index.end()) return sai_set_error(SAI_ERR_ARG, "samples not found in %s: %s", path, nme.c_str());
    col_of_slot.push_back(it->second);
  }
  return SAI_OK;
}

}  // namespace
