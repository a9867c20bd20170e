// sai_vcf_sites_*: the site columns of a VCF the readers do not keep -- ID, REF and the first ALT beside POS -- and
// the sample names of its #CHROM line, for the .bim and .fam of a fileset written from it (bed_export.hpp).  One
// pass over the text that looks at no sample column: a line is cut at its first five tabs, CHROM is compared as a
// string, POS is filtered by the region.  The rules are those of sai_amd/utils/vcf.py::read_site_columns.
//  * plain text is mapped and cut into one piece per thread at line starts; the pieces' rows are joined in file order;
//  * gzip and bgzip text is read through zlib on one thread, line by line out of a buffer that carries the cut line.

#include <zlib.h>

#include <algorithm>
#include <cstring>
#include <exception>
#include <new>
#include <string>
#include <vector>

#include "../host_threads.hpp"
#include "bed_export.hpp"
#include "fileset_index.hpp"

struct sai_vcf_sites {
  std::string chrom;
  std::vector<int32_t> pos;
  std::vector<uint8_t> multi;
  std::vector<int64_t> text_off{0};  // 3 * rows + 1
  std::string text;
  std::vector<int64_t> name_off{0};  // samples + 1
  std::string names;
  bool header = false;
};

namespace {

struct Piece {
  std::vector<int32_t> pos;
  std::vector<uint8_t> multi;
  std::vector<int64_t> len;  // 3 per row
  std::string text;
  const char* header = nullptr;  // the #CHROM line, without its newline
  size_t header_len = 0;
  std::string error;
};

struct Filter {
  const char* chrom;
  size_t chrom_len;
  int64_t start, end;
};

// one line [p, e), without its newline
void take_line(const char* p, const char* e, const Filter& f, Piece& out) {
  if (p == e) return;
  if (*p == '#') {
    if (!out.header && e - p >= 6 && memcmp(p, "#CHROM", 6) == 0) out.header = p, out.header_len = static_cast<size_t>(e - p);
    return;
  }
  const char* tab = static_cast<const char*>(memchr(p, '\t', static_cast<size_t>(e - p)));
  if (!tab || static_cast<size_t>(tab - p) != f.chrom_len || memcmp(p, f.chrom, f.chrom_len) != 0) return;
  const char* field[5];  // the ends of POS, ID, REF, ALT
  const char* at = tab + 1;
  for (int k = 0; k < 4; ++k) {
    const char* t = at <= e ? static_cast<const char*>(memchr(at, '\t', static_cast<size_t>(e - at))) : nullptr;
    if (!t) {
      if (k < 3 || at > e) {
        if (out.error.empty()) out.error = "a record of chromosome " + std::string(f.chrom, f.chrom_len) + " has fewer than 5 columns";
        return;
      }
      t = e;  // ALT is the line's last column
    }
    field[k] = t;
    at = t + 1;
  }
  int64_t pos = 0;
  const char* d = tab + 1;
  if (d == field[0]) pos = -1;
  for (; d < field[0] && pos >= 0; ++d) pos = (*d >= '0' && *d <= '9' && pos < (int64_t(1) << 40)) ? pos * 10 + (*d - '0') : -1;
  if (pos < 0 || pos > INT32_MAX) {
    if (out.error.empty()) out.error = "a record of chromosome " + std::string(f.chrom, f.chrom_len) + " has the position '" + std::string(tab + 1, field[0]) + "'";
    return;
  }
  if ((f.start >= 0 && pos < f.start) || (f.end >= 0 && pos > f.end)) return;
  const char* alt = field[2] + 1;
  const char* alt_end = field[3];
  if (alt_end > alt && alt_end[-1] == '\r') --alt_end;  // only where ALT ends the line
  const char* comma = static_cast<const char*>(memchr(alt, ',', static_cast<size_t>(alt_end - alt)));
  out.pos.push_back(static_cast<int32_t>(pos));
  out.multi.push_back(comma ? 1 : 0);
  const char* from[3] = {field[0] + 1, field[1] + 1, alt};
  const char* to[3] = {field[1], field[2], comma ? comma : alt_end};
  for (int k = 0; k < 3; ++k) {
    out.len.push_back(to[k] - from[k]);
    out.text.append(from[k], to[k]);
  }
}

// the whole lines of [p, e): a last line without a newline counts
void take_lines(const char* p, const char* e, const Filter& f, Piece& out) {
  while (p < e) {
    const char* nl = static_cast<const char*>(memchr(p, '\n', static_cast<size_t>(e - p)));
    const char* eol = nl ? nl : e;
    take_line(p, eol, f, out);
    p = eol + 1;
  }
}

void set_header(sai_vcf_sites& s, const char* line, size_t len) {
  if (s.header) return;
  s.header = true;
  const char* e = line + len;
  if (e > line && e[-1] == '\r') --e;
  const char* p = line;
  for (int col = 0; p <= e; ++col) {
    const char* t = static_cast<const char*>(memchr(p, '\t', static_cast<size_t>(e - p)));
    const char* end = t ? t : e;
    if (col >= 9) {
      s.names.append(p, end);
      s.name_off.push_back(static_cast<int64_t>(s.names.size()));
    }
    if (!t) break;
    p = t + 1;
  }
}

void join(sai_vcf_sites& s, Piece& piece) {
  if (piece.header) set_header(s, piece.header, piece.header_len);
  s.pos.insert(s.pos.end(), piece.pos.begin(), piece.pos.end());
  s.multi.insert(s.multi.end(), piece.multi.begin(), piece.multi.end());
  int64_t at = s.text_off.back();
  for (int64_t n : piece.len) s.text_off.push_back(at += n);
  s.text += piece.text;
}

int scan_plain(const char* path, const Filter& f, int32_t n_threads, sai_vcf_sites& s) {
  MappedFile file(path);
  if (!file.ok) return sai_set_error(SAI_ERR_ARG, "cannot open %s", path);
  const char* data = file.data;
  const size_t size = file.size;
  const int nt = static_cast<int>(std::max<size_t>(1, std::min<size_t>(static_cast<size_t>(std::max(n_threads, 1)), size / (size_t(1) << 20) + 1)));
  // piece t = the lines that start in [cut[t], cut[t + 1])
  std::vector<size_t> cut(static_cast<size_t>(nt) + 1, size);
  cut[0] = 0;
  for (int t = 1; t < nt; ++t) {
    const size_t guess = size / static_cast<size_t>(nt) * static_cast<size_t>(t);
    const char* nl = guess > 0 ? static_cast<const char*>(memchr(data + guess - 1, '\n', size - guess + 1)) : data - 1;
    cut[static_cast<size_t>(t)] = nl ? static_cast<size_t>(nl + 1 - data) : size;
  }
  std::vector<Piece> pieces(static_cast<size_t>(nt));
  auto work = [&](int t) {
    try {
      const size_t lo = cut[static_cast<size_t>(t)], hi = cut[static_cast<size_t>(t) + 1];
      if (lo < hi) take_lines(data + lo, data + hi, f, pieces[static_cast<size_t>(t)]);
    } catch (const std::exception& e) {
      pieces[static_cast<size_t>(t)].error = e.what();
    }
  };
  {
    ThreadGroup tg;
    for (int t = 1; t < nt; ++t) tg.spawn([&work, t] { work(t); });
    work(0);
    tg.join();
  }
  for (Piece& piece : pieces) {
    if (!piece.error.empty()) return sai_set_error(SAI_ERR_ARG, "%s: %s", path, piece.error.c_str());
    join(s, piece);
  }
  return SAI_OK;
}

int scan_gz(const char* path, const Filter& f, sai_vcf_sites& s) {
  gzFile gz = gzopen(path, "rb");
  if (!gz) return sai_set_error(SAI_ERR_ARG, "cannot open %s", path);
  gzbuffer(gz, 1 << 20);
  std::vector<char> buf(size_t(4) << 20);
  size_t have = 0;
  int rc = SAI_OK;
  for (bool last = false; !last && rc == SAI_OK;) {
    if (have == buf.size()) buf.resize(buf.size() * 2);  // one line longer than the buffer
    const int got = gzread(gz, buf.data() + have, static_cast<unsigned>(std::min<size_t>(buf.size() - have, size_t(1) << 30)));
    if (got < 0) {
      rc = sai_set_error(SAI_ERR_ARG, "%s: cannot be inflated", path);
      break;
    }
    last = got == 0;
    if (last) {  // a stream that was cut off gives the bytes it has and then nothing: only gzerror tells it from an end
      int zerr = Z_OK;
      gzerror(gz, &zerr);
      if (zerr != Z_OK && zerr != Z_STREAM_END) {
        rc = sai_set_error(SAI_ERR_ARG, "%s: the gzip stream ends before its end mark (a truncated file?)", path);
        break;
      }
    }
    have += static_cast<size_t>(got);
    // the whole lines of the buffer; at the end of the file also a last line without a newline
    size_t whole = have;
    if (!last) {
      while (whole > 0 && buf[whole - 1] != '\n') --whole;
      if (whole == 0) continue;
    }
    Piece piece;
    take_lines(buf.data(), buf.data() + whole, f, piece);
    if (!piece.error.empty()) rc = sai_set_error(SAI_ERR_ARG, "%s: %s", path, piece.error.c_str());
    else join(s, piece);  // the header line is copied out of the buffer here
    memmove(buf.data(), buf.data() + whole, have - whole);
    have -= whole;
  }
  const int closed = gzclose(gz);
  if (rc == SAI_OK && closed != Z_OK) rc = sai_set_error(SAI_ERR_ARG, "%s: the gzip stream ends before its end mark (a truncated file?)", path);
  return rc;
}

int sites_open_impl(const char* path, const char* chrom, int64_t start, int64_t end, int32_t n_threads, sai_vcf_sites** sites_out) {
  if (!path || !chrom || !sites_out) return sai_set_error(SAI_ERR_ARG, "NULL argument");
  *sites_out = nullptr;
  unsigned char magic[2] = {0, 0};
  FILE* fp = fopen(path, "rb");
  if (!fp) return sai_set_error(SAI_ERR_ARG, "cannot open %s", path);
  const size_t n_magic = fread(magic, 1, 2, fp);
  fclose(fp);
  sai_vcf_sites* s = new sai_vcf_sites;
  s->chrom = chrom;
  const Filter f{s->chrom.data(), s->chrom.size(), start, end};
  const bool gz = n_magic == 2 && magic[0] == 0x1f && magic[1] == 0x8b;
  int rc = gz ? scan_gz(path, f, *s) : scan_plain(path, f, n_threads, *s);
  if (rc == SAI_OK && !s->header) rc = sai_set_error(SAI_ERR_ARG, "%s: not a VCF (no #CHROM header)", path);
  if (rc != SAI_OK) {
    delete s;
    return rc;
  }
  *sites_out = s;
  return SAI_OK;
}

}  // namespace

extern "C" {

int sai_vcf_sites_open(const char* path, const char* chrom, int64_t start, int64_t end, int32_t n_threads, sai_vcf_sites** sites_out) {
  return guarded("sai_vcf_sites_open", [&] { return sites_open_impl(path, chrom, start, end, n_threads, sites_out); });
}

int sai_vcf_sites_info(const sai_vcf_sites* s, int64_t* n_rows, int64_t* n_samples, int64_t* text_bytes, int64_t* names_bytes) {
  if (!s) return sai_set_error(SAI_ERR_ARG, "sites is NULL");
  if (n_rows) *n_rows = static_cast<int64_t>(s->pos.size());
  if (n_samples) *n_samples = static_cast<int64_t>(s->name_off.size()) - 1;
  if (text_bytes) *text_bytes = static_cast<int64_t>(s->text.size());
  if (names_bytes) *names_bytes = static_cast<int64_t>(s->names.size());
  return SAI_OK;
}

int sai_vcf_sites_copy(const sai_vcf_sites* s, int32_t* pos, uint8_t* multi, int64_t* text_off, char* text, int64_t* name_off, char* names) {
  if (!s) return sai_set_error(SAI_ERR_ARG, "sites is NULL");
  if (pos && !s->pos.empty()) memcpy(pos, s->pos.data(), s->pos.size() * sizeof(int32_t));
  if (multi && !s->multi.empty()) memcpy(multi, s->multi.data(), s->multi.size());
  if (text_off) memcpy(text_off, s->text_off.data(), s->text_off.size() * sizeof(int64_t));
  if (text && !s->text.empty()) memcpy(text, s->text.data(), s->text.size());
  if (name_off) memcpy(name_off, s->name_off.data(), s->name_off.size() * sizeof(int64_t));
  if (names && !s->names.empty()) memcpy(names, s->names.data(), s->names.size());
  return SAI_OK;
}

int sai_vcf_sites_bim(const sai_vcf_sites* s, const uint8_t* skip, char* out, int64_t cap, int64_t* n_bytes) {
  return guarded("sai_vcf_sites_bim", [&] {
    if (!s || !n_bytes) return sai_set_error(SAI_ERR_ARG, "NULL argument");
    std::string lines;
    lines.reserve(s->text.size() + s->pos.size() * (s->chrom.size() + 20));
    for (size_t k = 0; k < s->pos.size(); ++k) {
      if (skip && skip[k]) continue;
      const int64_t* off = s->text_off.data() + 3 * k;
      lines += s->chrom;
      lines += '\t';
      lines.append(s->text, static_cast<size_t>(off[0]), static_cast<size_t>(off[1] - off[0]));  // ID
      lines += "\t0\t";
      lines += std::to_string(s->pos[k]);
      lines += '\t';
      lines.append(s->text, static_cast<size_t>(off[2]), static_cast<size_t>(off[3] - off[2]));  // ALT
      lines += '\t';
      lines.append(s->text, static_cast<size_t>(off[1]), static_cast<size_t>(off[2] - off[1]));  // REF
      lines += '\n';
    }
    *n_bytes = static_cast<int64_t>(lines.size());
    if (out && cap >= *n_bytes && !lines.empty()) memcpy(out, lines.data(), lines.size());
    return static_cast<int>(SAI_OK);
  });
}

int sai_vcf_sites_close(sai_vcf_sites* s) {
  delete s;
  return SAI_OK;
}

}  // extern "C"
