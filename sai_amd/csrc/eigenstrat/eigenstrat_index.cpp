// Host side of the EIGENSOFT fileset reader: the index of PREFIX.ind / PREFIX.snp (which .ind line is which
// requested sample, which .snp rows lie in the region, which of them the ancestral-allele rule keeps or
// flips), the detection and the checks of the three .geno encodings, and the host decoder of their records.
// The genotypes themselves are never read here (apart from the line ends of a text .geno): records are
// fixed-length, so the selected ones are byte ranges the streaming reader (sai_amd/utils/eigenstrat.py)
// preads straight into pinned memory.
//
// The rules are those of the VCF readers with column 5 of the .snp in the place of REF and column 6 in the
// place of ALT; the passes over the two text files are those of the PLINK reader (plink/fileset_index.hpp).
// The formats are built to their published description (DESIGN_INGEST.md, "EIGENSTRAT filesets"); the two
// hashes of a packed header are parsed and not verified.

#include "../plink/fileset_index.hpp"
#include "eigenstrat_codes.hpp"
#include "saihip_eigenstrat.h"

struct sai_eigenstrat_index {
  VariantRows rows;  // file_row = 0-based record line of the .snp
  std::vector<int32_t> col_of_slot;
  int64_t n_anc_entries = 0;
  int64_t n_ind = 0;
  int64_t encoding = 0;
  int64_t record_bytes = 0;
  int64_t data_offset = 0;
  uint64_t hash_ind = 0, hash_snp = 0;  // as the header gives them; not verified
};

namespace {

// .snp: id, chromosome, genetic position, position, first allele (plays REF), second allele (plays ALT);
// the two allele columns are optional
constexpr VariantLayout kSnpLayout = {1, 3, 4, 5, 4, true, true};
constexpr int64_t kMinRecord = 48;

int eigenstrat_scan_impl(const char* prefix, const char* chrom, int64_t* first_pos, int64_t* last_pos) {
  if (!prefix || !chrom || !first_pos || !last_pos) return sai_set_error(SAI_ERR_ARG, "NULL argument");
  VariantRows rows;
  AncMap none;
  if (int rc = variant_pass(std::string(prefix) + ".snp", kSnpLayout, chrom, -1, -1, none, false, kScanThreads, rows)) return rc;
  *first_pos = rows.first;
  *last_pos = rows.last;
  return SAI_OK;
}

inline bool all_digits(const char* p, size_t n) {
  if (n == 0 || n > 18) return false;
  for (size_t i = 0; i < n; ++i)
    if (p[i] < '0' || p[i] > '9') return false;
  return true;
}

// The header record of a packed .geno: "GENO" or "TGENO", n_ind, n_snp and optionally two hexadecimal hashes.
int check_packed(const std::string& path, const char* head, size_t n_head, long long size, bool transposed, sai_eigenstrat_index& idx) {
  const char* tok[5];
  size_t len[5];
  const int found = split_tokens(head, head + strnlen(head, n_head), 5, tok, len);
  if (found < 3 || !all_digits(tok[1], len[1]) || !all_digits(tok[2], len[2]))
    return sai_set_error(SAI_ERR_ARG, "%s: malformed %s header: the counts of individuals and variants are expected after the tag", path.c_str(),
                         transposed ? "TGENO" : "GENO");
  const long long n_ind = atoll(std::string(tok[1], len[1]).c_str()), n_snp = atoll(std::string(tok[2], len[2]).c_str());
  if (found > 3) idx.hash_ind = strtoull(std::string(tok[3], len[3]).c_str(), nullptr, 16);
  if (found > 4) idx.hash_snp = strtoull(std::string(tok[4], len[4]).c_str(), nullptr, 16);
  if (n_ind != idx.n_ind || n_snp != idx.rows.n_lines)
    return sai_set_error(SAI_ERR_ARG, "%s: the header counts %lld individuals and %lld variants, but the .ind has %lld lines and the .snp has %lld",
                         path.c_str(), n_ind, n_snp, static_cast<long long>(idx.n_ind), static_cast<long long>(idx.rows.n_lines));
  const long long per_record = transposed ? n_snp : n_ind, records = transposed ? n_ind : n_snp;
  const long long rlen = std::max<long long>(kMinRecord, (per_record + 3) / 4);
  const long long want = rlen * (1 + records);
  if (size != want)
    return sai_set_error(SAI_ERR_ARG, "%s: %lld bytes, expected %lld (a header and %lld records of %lld bytes): truncated, or not the .geno of this fileset",
                         path.c_str(), size, want, records, rlen);
  idx.encoding = transposed ? SAI_EIGENSTRAT_TRANSPOSED : SAI_EIGENSTRAT_PACKED;
  idx.record_bytes = rlen;
  idx.data_offset = rlen;
  return SAI_OK;
}

// A text .geno: every line holds one character per individual and ends in "\n" or "\r\n"; the last newline may be missing.
int check_text(const std::string& path, sai_eigenstrat_index& idx) {
  MappedFile geno(path);
  if (!geno.ok) return sai_set_error(SAI_ERR_ARG, "cannot open %s", path.c_str());
  const long long size = static_cast<long long>(geno.size), n_ind = idx.n_ind, n_snp = idx.rows.n_lines;
  const char* nl = static_cast<const char*>(memchr(geno.data, '\n', static_cast<size_t>(std::min(size, n_ind + 2))));
  long long line_len, held;
  bool crlf = false;
  if (nl) {
    line_len = nl - geno.data + 1;
    crlf = line_len >= 2 && nl[-1] == '\r';
    held = line_len - 1 - (crlf ? 1 : 0);
  } else {
    held = size;  // one line without its newline, or a line that is too long
    line_len = held + 1;
  }
  if (held != n_ind)
    return sai_set_error(SAI_ERR_ARG, "%s: the first line holds %s%lld characters, but the .ind has %lld lines", path.c_str(),
                         nl ? "" : "more than ", nl ? held : n_ind + 1, n_ind);
  const long long whole = std::min(n_snp, size / line_len);
  for (long long k = 0; k < whole; ++k) {
    const char* last = geno.data + (k + 1) * line_len - 1;
    if (*last != '\n' || (crlf && last[-1] != '\r'))
      return sai_set_error(SAI_ERR_ARG, "%s: lines of unequal length: line %lld does not end after %lld characters as the first line does",
                           path.c_str(), k + 1, held);
  }
  const long long want = n_snp * line_len;
  if (size != want && size != want - 1 && !(crlf && size == want - 2))
    return sai_set_error(SAI_ERR_ARG, "%s: %lld bytes, expected %lld (%lld variants of the .snp x lines of %lld bytes): truncated, or not the .geno of this fileset",
                         path.c_str(), size, want, n_snp, line_len);
  idx.encoding = SAI_EIGENSTRAT_TEXT;
  idx.record_bytes = line_len;
  idx.data_offset = 0;
  return SAI_OK;
}

int check_geno(const std::string& path, sai_eigenstrat_index& idx) {
  const int fd = open(path.c_str(), O_RDONLY);
  if (fd < 0) return sai_set_error(SAI_ERR_ARG, "cannot open %s", path.c_str());
  struct stat sb;
  char head[kMinRecord + 1];
  memset(head, 0, sizeof head);
  const bool stat_ok = fstat(fd, &sb) == 0;
  const ssize_t got = stat_ok ? pread(fd, head, kMinRecord, 0) : -1;
  close(fd);
  if (!stat_ok || got < 0) return sai_set_error(SAI_ERR_ARG, "cannot read %s", path.c_str());
  const size_t n_head = static_cast<size_t>(got);
  if (n_head >= 6 && memcmp(head, "TGENO", 5) == 0 && is_blank(head[5])) return check_packed(path, head, n_head, sb.st_size, true, idx);
  if (n_head >= 5 && memcmp(head, "GENO", 4) == 0 && is_blank(head[4])) return check_packed(path, head, n_head, sb.st_size, false, idx);
  if (n_head >= 1 && geno_code_of_char(static_cast<unsigned char>(head[0])) != kGenoBadCode) return check_text(path, idx);
  char shown[3 * 8 + 1] = "";
  for (size_t i = 0; i < std::min<size_t>(n_head, 8); ++i) snprintf(shown + 3 * i, 4, "%02X ", static_cast<unsigned char>(head[i]));
  return sai_set_error(SAI_ERR_ARG, "%s: not a .geno file: it starts with the bytes %s(expected GENO, TGENO or one of the characters 0 1 2 9)",
                       path.c_str(), n_head ? shown : "<none> ");
}

int eigenstrat_open_impl(const char* prefix, const char* chrom, int64_t start, int64_t end, int32_t n_samples,
                         const char* const* sample_names, const int32_t* ploidy, const char* anc_bed_path, int32_t n_threads,
                         sai_eigenstrat_index** index_out) {
  if (!prefix || !chrom || !index_out) return sai_set_error(SAI_ERR_ARG, "NULL argument");
  *index_out = nullptr;
  if (n_samples < 0 || (n_samples > 0 && (!sample_names || !ploidy))) return sai_set_error(SAI_ERR_ARG, "bad sample selection");
  for (int32_t s = 0; s < n_samples; ++s)  // before anything is read
    if (ploidy[s] < 1 || ploidy[s] > 2)
      return sai_set_error(SAI_ERR_ARG, "sample %s is configured with ploidy %d: an EIGENSTRAT fileset holds haploid and diploid calls only",
                           sample_names[s], ploidy[s]);
  if (n_threads < 1) n_threads = 1;
  const std::string pre(prefix), c(chrom);
  std::unique_ptr<sai_eigenstrat_index> holder(new sai_eigenstrat_index);
  sai_eigenstrat_index& idx = *holder;
  // .ind: one individual per record line, the name is column 1
  if (int rc = resolve_samples(pre + ".ind", 0, true, n_samples, sample_names, idx.col_of_slot, &idx.n_ind)) return rc;
  AncMap anc;
  if (anc_bed_path) {
    if (int rc = load_anc(anc_bed_path, c, start, end, anc, &idx.n_anc_entries)) return rc;
  }
  if (int rc = variant_pass(pre + ".snp", kSnpLayout, c, start, end, anc, true, n_threads, idx.rows)) return rc;
  if (int rc = check_geno(pre + ".geno", idx)) return rc;
  *index_out = holder.release();
  return SAI_OK;
}

inline uint32_t lut_for(int32_t ploidy, bool flip) {
  return ploidy == 2 ? (flip ? kGenoLutP2Flip : kGenoLutP2) : (flip ? kGenoLutP1Flip : kGenoLutP1);
}

int eigenstrat_decode_host_impl(int32_t encoding, const uint8_t* records, int64_t n_batch_records, int64_t record_bytes,
                                int32_t first_code, int64_t n_out_rows, const int32_t* row_in_batch, const uint8_t* row_flip,
                                int32_t n_cols, int32_t n_slots, const int32_t* col_of_slot, const int32_t* ploidy_of_slot,
                                int8_t* out, int32_t* status, int32_t n_threads) {
  if (encoding < SAI_EIGENSTRAT_TEXT || encoding > SAI_EIGENSTRAT_TRANSPOSED) return sai_set_error(SAI_ERR_ARG, "unknown encoding");
  if (n_batch_records < 0 || record_bytes < 0 || n_out_rows < 0 || n_cols < 0 || n_slots < 1) return sai_set_error(SAI_ERR_ARG, "size out of range");
  const bool transposed = encoding == SAI_EIGENSTRAT_TRANSPOSED, text = encoding == SAI_EIGENSTRAT_TEXT;
  if (transposed) {
    if (first_code < 0 || first_code > 3) return sai_set_error(SAI_ERR_ARG, "first_code must be 0 .. 3");
    if (record_bytes > (int64_t(1) << 60) || first_code + n_batch_records > 4 * record_bytes)
      return sai_set_error(SAI_ERR_ARG, "first_code + n_batch_records exceeds the 4 * record_bytes genotypes of a record");
  } else {
    if (first_code != 0) return sai_set_error(SAI_ERR_ARG, "first_code must be 0 for a variant-major encoding");
    if (static_cast<int64_t>(n_cols) > (text ? record_bytes : 4 * record_bytes)) return sai_set_error(SAI_ERR_ARG, "n_cols exceeds the genotypes of a record");
  }
  if (n_out_rows == 0) return SAI_OK;
  const int64_t n_records = transposed ? n_cols : n_batch_records;
  if (!row_in_batch || !row_flip || !col_of_slot || !ploidy_of_slot || !out || !status || (n_records > 0 && record_bytes > 0 && !records))
    return sai_set_error(SAI_ERR_ARG, "NULL buffer");
  auto decode = [&](int64_t lo, int64_t hi) {
    for (int64_t r = lo; r < hi; ++r) {
      int8_t* o = out + r * n_slots;
      int32_t st = 0;
      const int64_t rib = row_in_batch[r];
      const bool row_ok = rib >= 0 && rib < n_batch_records;
      const bool flip = row_flip[r] != 0;
      for (int32_t s = 0; s < n_slots; ++s) {
        const int32_t col = col_of_slot[s], pl = ploidy_of_slot[s];
        if (!row_ok || col < 0 || col >= n_cols || pl < 1 || pl > 2) {
          o[s] = 0;
          st = kGenoBadIndex;
          continue;
        }
        uint32_t code;
        if (transposed) {
          const int64_t k = first_code + rib;
          code = (records[col * record_bytes + (k >> 2)] >> (6 - 2 * (k & 3))) & 3u;
        } else if (text) {
          code = geno_code_of_char(records[rib * record_bytes + col]);
        } else {
          code = (records[rib * record_bytes + (col >> 2)] >> (6 - 2 * (col & 3))) & 3u;
        }
        if (code == kGenoBadCode) {
          o[s] = 0;
          st = std::max(st, kGenoBadChar);
          continue;
        }
        if (pl == 1 && code == kGenoHet) st = std::max(st, n_slots - s);
        o[s] = static_cast<int8_t>((lut_for(pl, flip) >> (8 * code)) & 0xFFu);
      }
      status[r] = st;
    }
  };
  const int64_t cells = n_out_rows * static_cast<int64_t>(n_slots);
  const int nt = static_cast<int>(std::max<int64_t>(1, std::min<int64_t>({static_cast<int64_t>(std::max(n_threads, 1)), n_out_rows, cells / (int64_t(1) << 18) + 1})));
  ThreadGroup tg;
  for (int t = 1; t < nt; ++t) tg.spawn([&decode, t, nt, n_out_rows] { decode(n_out_rows * t / nt, n_out_rows * (t + 1) / nt); });
  decode(0, n_out_rows / nt);
  tg.join();
  return SAI_OK;
}

}  // namespace

extern "C" {

int sai_eigenstrat_abi_version(void) { return SAI_EIGENSTRAT_ABI_VERSION; }

int sai_eigenstrat_scan(const char* prefix, const char* chrom, int64_t* first_pos, int64_t* last_pos) {
  return guarded("sai_eigenstrat_scan", [&] { return eigenstrat_scan_impl(prefix, chrom, first_pos, last_pos); });
}

int sai_eigenstrat_open(const char* prefix, const char* chrom, int64_t start, int64_t end, int32_t n_samples,
                        const char* const* sample_names, const int32_t* ploidy, const char* anc_bed_path, int32_t n_threads,
                        sai_eigenstrat_index** index_out) {
  return guarded("sai_eigenstrat_open", [&] {
    return eigenstrat_open_impl(prefix, chrom, start, end, n_samples, sample_names, ploidy, anc_bed_path, n_threads, index_out);
  });
}

int sai_eigenstrat_index_info(const sai_eigenstrat_index* index, int64_t* n_rows, int64_t* n_matched, int64_t* n_anc_entries,
                              int64_t* n_ind, int64_t* n_snp, int64_t* first_pos, int64_t* last_pos, int64_t* encoding,
                              int64_t* record_bytes, int64_t* data_offset) {
  if (!index) return sai_set_error(SAI_ERR_ARG, "index is NULL");
  if (n_rows) *n_rows = static_cast<int64_t>(index->rows.pos.size());
  if (n_matched) *n_matched = index->rows.n_matched;
  if (n_anc_entries) *n_anc_entries = index->n_anc_entries;
  if (n_ind) *n_ind = index->n_ind;
  if (n_snp) *n_snp = index->rows.n_lines;
  if (first_pos) *first_pos = index->rows.first;
  if (last_pos) *last_pos = index->rows.last;
  if (encoding) *encoding = index->encoding;
  if (record_bytes) *record_bytes = index->record_bytes;
  if (data_offset) *data_offset = index->data_offset;
  return SAI_OK;
}

int sai_eigenstrat_index_copy(const sai_eigenstrat_index* index, int32_t* pos, int64_t* file_row, uint8_t* flip, int32_t* col_of_slot) {
  if (!index) return sai_set_error(SAI_ERR_ARG, "index is NULL");
  const size_t n = index->rows.pos.size();
  if (pos && n) memcpy(pos, index->rows.pos.data(), n * sizeof(int32_t));
  if (file_row && n) memcpy(file_row, index->rows.file_row.data(), n * sizeof(int64_t));
  if (flip && n) memcpy(flip, index->rows.flip.data(), n);
  if (col_of_slot && !index->col_of_slot.empty()) memcpy(col_of_slot, index->col_of_slot.data(), index->col_of_slot.size() * sizeof(int32_t));
  return SAI_OK;
}

int sai_eigenstrat_index_close(sai_eigenstrat_index* index) {
  delete index;
  return SAI_OK;
}

int sai_eigenstrat_decode_host(int32_t encoding, const uint8_t* records, int64_t n_batch_records, int64_t record_bytes,
                               int32_t first_code, int64_t n_out_rows, const int32_t* row_in_batch, const uint8_t* row_flip,
                               int32_t n_cols, int32_t n_slots, const int32_t* col_of_slot, const int32_t* ploidy_of_slot,
                               int8_t* out, int32_t* status, int32_t n_threads) {
  return guarded("sai_eigenstrat_decode_host", [&] {
    return eigenstrat_decode_host_impl(encoding, records, n_batch_records, record_bytes, first_code, n_out_rows, row_in_batch, row_flip,
                                       n_cols, n_slots, col_of_slot, ploidy_of_slot, out, status, n_threads);
  });
}

}  // extern "C"
