// What the host indexes of the genotype filesets share (plink_index.cpp here, ../eigenstrat/eigenstrat_index.cpp):
// a read-only mapping of a text file, the blank-separated token split, the ancestral-allele decision of
// parse_lines() (ingest_base.hpp) and the two passes every fileset has -- one over its sample file, which
// resolves the requested names to columns, and one over its variant file, which selects the rows of a
// chromosome inside a region in file order.  The formats differ only in which column holds what.
#pragma once

#include <sys/mman.h>

#include "../ingest_base.hpp"

namespace {

struct MappedFile {
  const char* data = nullptr;
  size_t size = 0;
  bool ok = false;
  explicit MappedFile(const std::string& path) {
    const int fd = open(path.c_str(), O_RDONLY);
    if (fd < 0) return;
    struct stat sb;
    if (fstat(fd, &sb) == 0 && S_ISREG(sb.st_mode)) {
      size = static_cast<size_t>(sb.st_size);
      ok = true;
      if (size) {
        void* p = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
        if (p == MAP_FAILED) ok = false;
        else data = static_cast<const char*>(p);
      }
    }
    close(fd);
  }
  ~MappedFile() {
    if (data) munmap(const_cast<char*>(data), size);
  }
  MappedFile(const MappedFile&) = delete;
  MappedFile& operator=(const MappedFile&) = delete;
};

inline bool is_blank(char c) { return c == ' ' || c == '\t' || c == '\r'; }

// up to `want` blank-separated tokens of [p, eol); returns how many were found
inline int split_tokens(const char* p, const char* eol, int want, const char** tok, size_t* len) {
  int found = 0;
  while (found < want) {
    while (p < eol && is_blank(*p)) ++p;
    if (p >= eol) break;
    const char* s = p;
    while (p < eol && !is_blank(*p)) ++p;
    tok[found] = s;
    len[found] = static_cast<size_t>(p - s);
    ++found;
  }
  return found;
}

enum AncDecision { kDrop = 0, kKeep = 1, kFlip = 2 };

// ingest_base.hpp, parse_lines(): not listed -> drop; the ancestral allele equals ALT -> flip;
// else equals REF -> keep; else drop
inline AncDecision anc_decision(const AncMap& anc, int64_t pos, const char* alt, size_t n_alt, const char* ref, size_t n_ref) {
  if (!anc.active) return kKeep;
  const auto it = anc.allele.find(pos);
  if (it == anc.allele.end()) return kDrop;
  const AncAllele& a = it->second;
  if (a.size() == n_alt && memcmp(a.data(), alt, n_alt) == 0) return kFlip;
  if (a.size() == n_ref && memcmp(a.data(), ref, n_ref) == 0) return kKeep;
  return kDrop;
}

// Which column of a variant line (.bim, .snp) holds what, and how strict the format is.
struct VariantLayout {
  int chrom_col, pos_col, ref_col, alt_col;
  int min_cols;         // a record line with fewer columns is refused; the allele columns may lie beyond it (then optional)
  bool hash_comments;   // lines whose first non-blank character is '#' are skipped
  bool strict_pos;      // a position that is not a plain non-negative integer is refused
  bool mark_multi = false;  // the first selected row whose ALT column holds a comma is reported (VariantRows::first_multi)
};

// The rows a variant pass selects, and what it learns on the way.
struct VariantRows {
  std::vector<int32_t> pos;
  std::vector<int64_t> file_row;  // 0-based record line of the variant file
  std::vector<uint8_t> flip;
  int64_t n_matched = 0;
  int64_t n_lines = 0;            // record lines of the whole file
  int64_t first = -1, last = -1;  // the first contiguous run of the chromosome, whole file
  int64_t first_multi = -1;       // file_row of the first selected row with several ALT alleles (VariantLayout::mark_multi)
};

enum VariantLineError { kLineFine = 0, kLineShort = 1, kLineBadPos = 2, kLineNoAlleles = 3 };

struct VariantPiece {
  int64_t n_lines = 0;  // record lines (blank lines are not rows)
  int64_t matched = 0;
  std::vector<int32_t> pos;
  std::vector<int64_t> row;  // counted from the piece's first record line
  std::vector<uint8_t> flip;
  int64_t first = -1, last = -1;  // the first run of the chromosome inside the piece
  bool other_before = false, ended = false;
  int64_t bad_line = -1;  // the first refused line (piece-relative) ...
  VariantLineError bad_why = kLineFine;  // ... and why
  bool failed = false;    // out of memory
  int64_t multi_line = -1;  // the first selected line (piece-relative) with a comma in ALT
};

constexpr int kMaxVariantCols = 6;

inline void variant_piece(const char* p, const char* end, const VariantLayout& lay, const std::string& chrom, int64_t start,
                          int64_t stop, const AncMap& anc, bool want_rows, VariantPiece& out) {
  const int want = std::max(std::max(lay.ref_col, lay.alt_col) + 1, lay.min_cols);
  while (p < end) {
    const char* eol = static_cast<const char*>(memchr(p, '\n', static_cast<size_t>(end - p)));
    if (!eol) eol = end;
    const char* tok[kMaxVariantCols];
    size_t len[kMaxVariantCols];
    const int found = split_tokens(p, eol, want, tok, len);
    p = eol + 1;
    if (found == 0) continue;
    if (lay.hash_comments && tok[0][0] == '#') continue;
    const int64_t line = out.n_lines++;
    if (found < lay.min_cols) {
      out.bad_line = line;
      out.bad_why = kLineShort;
      return;
    }
    int64_t pos = 0;
    const char* f = tok[lay.pos_col];
    const char* fe = f + len[lay.pos_col];
    for (; f < fe && *f >= '0' && *f <= '9' && pos < (int64_t(1) << 40); ++f) pos = pos * 10 + (*f - '0');
    if (lay.strict_pos && (f != fe || pos > 0x7FFFFFFF)) {
      out.bad_line = line;
      out.bad_why = kLineBadPos;
      return;
    }
    const bool has_alleles = found > std::max(lay.ref_col, lay.alt_col);
    if (anc.active && !has_alleles) {
      out.bad_line = line;
      out.bad_why = kLineNoAlleles;
      return;
    }
    if (len[lay.chrom_col] != chrom.size() || memcmp(tok[lay.chrom_col], chrom.data(), chrom.size()) != 0) {
      if (out.first >= 0) out.ended = true;
      else out.other_before = true;
      continue;
    }
    if (!out.ended) {
      if (out.first < 0) out.first = pos;
      out.last = pos;
    }
    if ((start >= 0 && pos < start) || (stop >= 0 && pos > stop)) continue;
    ++out.matched;
    if (!want_rows) continue;
    const AncDecision d = anc.active ? anc_decision(anc, pos, tok[lay.alt_col], len[lay.alt_col], tok[lay.ref_col], len[lay.ref_col]) : kKeep;
    if (d == kDrop) continue;
    out.pos.push_back(static_cast<int32_t>(pos));
    out.row.push_back(line);
    out.flip.push_back(d == kFlip ? 1 : 0);
    if (lay.mark_multi && out.multi_line < 0 && found > lay.alt_col && memchr(tok[lay.alt_col], ',', len[lay.alt_col])) out.multi_line = line;
  }
}

// One pass over a variant file, split over n_threads at line boundaries.
inline int variant_pass(const std::string& path, const VariantLayout& lay, const std::string& chrom, int64_t start, int64_t stop,
                        const AncMap& anc, bool want_rows, int n_threads, VariantRows& idx) {
  MappedFile file(path);
  if (!file.ok) return sai_set_error(SAI_ERR_ARG, "cannot open %s", path.c_str());
  const char* base = file.data;
  const size_t total = file.size;
  const int nt = static_cast<int>(std::max<size_t>(1, std::min<size_t>(static_cast<size_t>(std::max(n_threads, 1)), total / (size_t(1) << 20) + 1)));
  std::vector<size_t> edge(static_cast<size_t>(nt) + 1, total);
  edge[0] = 0;
  for (int t = 1; t < nt; ++t) {
    const size_t guess = std::max(edge[static_cast<size_t>(t) - 1], total * static_cast<size_t>(t) / static_cast<size_t>(nt));
    const void* nl = guess < total ? memchr(base + guess, '\n', total - guess) : nullptr;
    edge[static_cast<size_t>(t)] = nl ? static_cast<size_t>(static_cast<const char*>(nl) - base) + 1 : total;
  }
  std::vector<VariantPiece> pieces(static_cast<size_t>(nt));
  auto work = [&](int t) {  // an exception must not leave a worker thread
    VariantPiece& pc = pieces[static_cast<size_t>(t)];
    try {
      if (total) variant_piece(base + edge[static_cast<size_t>(t)], base + edge[static_cast<size_t>(t) + 1], lay, chrom, start, stop, anc, want_rows, pc);
    } catch (...) {
      pc.failed = true;
    }
  };
  {
    ThreadGroup tg;
    for (int t = 1; t < nt; ++t) tg.spawn([&work, t] { work(t); });
    work(0);
    tg.join();
  }
  int64_t line0 = 0;
  size_t n_rows = 0;
  for (const VariantPiece& pc : pieces) {
    if (pc.failed) return sai_set_error(SAI_ERR_HIP, "%s: out of host memory", path.c_str());
    const long long at = static_cast<long long>(line0 + pc.bad_line + 1);
    if (pc.bad_why == kLineShort)
      return sai_set_error(SAI_ERR_ARG, "%s: variant line %lld has fewer than %d columns", path.c_str(), at, lay.min_cols);
    if (pc.bad_why == kLineBadPos)
      return sai_set_error(SAI_ERR_ARG, "%s: variant line %lld: the position is not an integer", path.c_str(), at);
    if (pc.bad_why == kLineNoAlleles)
      return sai_set_error(SAI_ERR_ARG, "%s: variant line %lld has no allele columns: an ancestral-allele file cannot be applied to it",
                           path.c_str(), at);
    line0 += pc.n_lines;
    n_rows += pc.pos.size();
  }
  idx.n_lines = line0;
  idx.pos.reserve(n_rows);
  idx.file_row.reserve(n_rows);
  idx.flip.reserve(n_rows);
  line0 = 0;
  bool run_over = false;
  for (const VariantPiece& pc : pieces) {  // in file order
    idx.n_matched += pc.matched;
    idx.pos.insert(idx.pos.end(), pc.pos.begin(), pc.pos.end());
    for (int64_t r : pc.row) idx.file_row.push_back(line0 + r);
    idx.flip.insert(idx.flip.end(), pc.flip.begin(), pc.flip.end());
    if (idx.first_multi < 0 && pc.multi_line >= 0) idx.first_multi = line0 + pc.multi_line;
    line0 += pc.n_lines;
    if (run_over) continue;
    if (idx.first < 0) {
      if (pc.first >= 0) {
        idx.first = pc.first;
        idx.last = pc.last;
        run_over = pc.ended;
      }
    } else if (pc.other_before) {
      run_over = true;  // the run ended where the previous piece ended
    } else if (pc.first >= 0) {
      idx.last = pc.last;
      run_over = pc.ended;
    } else if (pc.ended) {
      run_over = true;
    }
  }
  return SAI_OK;
}

// One pass over a sample file (.fam, .ind): counts its record lines and resolves the requested names, found in
// column `name_col`, to 0-based record lines.  A name that is asked for must occur exactly once.
inline int resolve_samples(const std::string& path, int name_col, bool hash_comments, int32_t n_samples,
                           const char* const* sample_names, std::vector<int32_t>& col_of_slot, int64_t* n_lines) {
  MappedFile file(path);
  if (!file.ok) return sai_set_error(SAI_ERR_ARG, "cannot open %s", path.c_str());
  std::unordered_map<std::string, std::pair<int32_t, bool>> col_of;  // name -> (first column, seen again)
  const char* p = file.data;
  const char* endp = file.data + file.size;
  int64_t n = 0;
  while (p < endp) {
    const char* eol = static_cast<const char*>(memchr(p, '\n', static_cast<size_t>(endp - p)));
    if (!eol) eol = endp;
    const char* tok[2];
    size_t len[2];
    const int found = split_tokens(p, eol, name_col + 1, tok, len);
    p = eol + 1;
    if (found == 0) continue;
    if (hash_comments && tok[0][0] == '#') continue;
    if (found < name_col + 1)
      return sai_set_error(SAI_ERR_ARG, "%s: sample line %lld has fewer than %d columns", path.c_str(), static_cast<long long>(n + 1), name_col + 1);
    if (n >= 0x7FFFFFFF) return sai_set_error(SAI_ERR_UNSUPPORTED, "%s: too many samples", path.c_str());
    if (n_samples > 0) {
      auto ins = col_of.emplace(std::string(tok[name_col], len[name_col]), std::make_pair(static_cast<int32_t>(n), false));
      if (!ins.second) ins.first->second.second = true;
    }
    ++n;
  }
  *n_lines = n;
  col_of_slot.resize(static_cast<size_t>(n_samples));
  for (int32_t s = 0; s < n_samples; ++s) {
    const auto it = col_of.find(sample_names[s]);
    if (it == col_of.end()) return sai_set_error(SAI_ERR_ARG, "samples not found in %s: %s", path.c_str(), sample_names[s]);
    if (it->second.second) return sai_set_error(SAI_ERR_ARG, "sample %s occurs twice in %s", sample_names[s], path.c_str());
    col_of_slot[static_cast<size_t>(s)] = it->second.first;
  }
  return SAI_OK;
}

}  // namespace
