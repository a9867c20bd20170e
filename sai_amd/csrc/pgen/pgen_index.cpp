// Host side of the PLINK 2 fileset reader: the index of PREFIX.psam / PREFIX.pvar (which sample column is which
// requested sample, which variants lie in the region, which of them the ancestral-allele rule keeps or flips), the
// header of PREFIX.pgen (storage mode, counts, block offsets, the vrtype and the length of every record) and the
// host decoder of its records.  The passes over the two text files are those of the PLINK 1 reader
// (../plink/fileset_index.hpp) with the columns of a .pvar / .psam; a file of either kind without a header line is
// read as a .bim / .fam.
//
// The record format is restated in DESIGN_INGEST.md ("PLINK 2 filesets").  Records are independent except for one
// back-reference: a record of type 2 or 3 holds its genotypes as differences from its base, the nearest earlier
// record of another type.  The index finds the base of every selected row by one pass over the vrtypes and hands
// out its span next to the row's own, so the streaming reader (sai_amd/utils/pgen.py) fetches both and the decoders
// never look at a third record.  sai_pgen_decode_host is the plain statement of the rules: the SAI_AMD_INGEST=host
// route and the yardstick of the kernel (pgen_decode.hip), which makes the same decisions with the same status values.

#include <atomic>

#include "../plink/fileset_index.hpp"
#include "pgen_codes.hpp"
#include "pgen_expand_host.hpp"
#include "saihip_pgen.h"

struct sai_pgen_index {
  VariantRows rows;  // file_row = 0-based variant of the .pgen (= record line of the .pvar)
  std::vector<int32_t> col_of_slot;
  std::vector<int64_t> rec, base;  // [n_rows][3]: file offset, length, vrtype; the base or -1, -1, -1
  int64_t n_anc_entries = 0;
  int64_t sample_ct = 0;
  int64_t variant_ct = 0;
  int64_t mode = 0;
};

namespace {

// .pvar with a header line: #CHROM POS ID REF ALT ...; without one it is a .bim
constexpr VariantLayout kPvarLayout = {0, 1, 3, 4, 5, true, false, true};
constexpr VariantLayout kBimLayout = {0, 3, 5, 4, 6, true, false, true};

inline bool token_is(const char* tok, size_t len, const char* want) { return len == strlen(want) && memcmp(tok, want, len) == 0; }

// the first line of a text file that is neither blank nor a "##" line: [*line, *eol), or false when there is none
bool first_line(const MappedFile& file, const char** line, const char** eol_out) {
  const char* p = file.data;
  const char* endp = file.data + file.size;
  while (p < endp) {
    const char* eol = static_cast<const char*>(memchr(p, '\n', static_cast<size_t>(endp - p)));
    if (!eol) eol = endp;
    const char* q = p;
    while (q < eol && is_blank(*q)) ++q;
    if (q < eol && !(eol - q >= 2 && q[0] == '#' && q[1] == '#')) {
      *line = q;
      *eol_out = eol;
      return true;
    }
    p = eol + 1;
  }
  return false;
}

int missing_file(const std::string& path) {
  struct stat sb;
  if (stat(path.c_str(), &sb) == 0 && S_ISREG(sb.st_mode)) return SAI_OK;
  const std::string zst = path + ".zst";
  if (stat(zst.c_str(), &sb) == 0)
    return sai_set_error(SAI_ERR_UNSUPPORTED, "%s is not found, but %s is: decompress it first (zstd -d), no zstd decoder is built into this library",
                         path.c_str(), zst.c_str());
  return sai_set_error(SAI_ERR_ARG, "%s is not found", path.c_str());
}

int pvar_layout(const std::string& path, VariantLayout* lay) {
  if (int rc = missing_file(path)) return rc;
  MappedFile file(path);
  if (!file.ok) return sai_set_error(SAI_ERR_ARG, "cannot open %s", path.c_str());
  *lay = kBimLayout;
  const char *line, *eol;
  if (!first_line(file, &line, &eol) || line[0] != '#') return SAI_OK;
  const char* tok[5];
  size_t len[5];
  static const char* const want[5] = {"#CHROM", "POS", "ID", "REF", "ALT"};
  const int found = split_tokens(line, eol, 5, tok, len);
  for (int k = 0; k < 5; ++k)
    if (k >= found || !token_is(tok[k], len[k], want[k]))
      return sai_set_error(SAI_ERR_UNSUPPORTED, "%s: the header line does not begin with #CHROM POS ID REF ALT", path.c_str());
  *lay = kPvarLayout;
  return SAI_OK;
}

// the IID column of a .psam and whether it has a header line
int psam_layout(const std::string& path, int* name_col, bool* header) {
  if (int rc = missing_file(path)) return rc;
  MappedFile file(path);
  if (!file.ok) return sai_set_error(SAI_ERR_ARG, "cannot open %s", path.c_str());
  *name_col = 1;  // a .fam
  *header = false;
  const char *line, *eol;
  if (!first_line(file, &line, &eol) || line[0] != '#') return SAI_OK;
  const char* tok[2];
  size_t len[2];
  const int found = split_tokens(line, eol, 2, tok, len);
  *header = true;
  if (found >= 1 && token_is(tok[0], len[0], "#IID")) {
    *name_col = 0;
    return SAI_OK;
  }
  if (found >= 2 && token_is(tok[0], len[0], "#FID") && token_is(tok[1], len[1], "IID")) return SAI_OK;
  return sai_set_error(SAI_ERR_UNSUPPORTED, "%s: the header line does not begin with #FID IID or #IID", path.c_str());
}

int pgen_scan_impl(const char* prefix, const char* chrom, int64_t* first_pos, int64_t* last_pos) {
  if (!prefix || !chrom || !first_pos || !last_pos) return sai_set_error(SAI_ERR_ARG, "NULL argument");
  VariantRows rows;
  AncMap none;
  VariantLayout lay;
  const std::string path = std::string(prefix) + ".pvar";
  if (int rc = pvar_layout(path, &lay)) return rc;
  lay.mark_multi = false;
  if (int rc = variant_pass(path, lay, chrom, -1, -1, none, false, kScanThreads, rows)) return rc;
  *first_pos = rows.first;
  *last_pos = rows.last;
  return SAI_OK;
}

// The .pgen header: fills idx.rec / idx.base for the selected rows.
int read_pgen_header(const std::string& path, sai_pgen_index& idx) {
  MappedFile file(path);
  if (!file.ok) return sai_set_error(SAI_ERR_ARG, "cannot open %s", path.c_str());
  const uint8_t* d = reinterpret_cast<const uint8_t*>(file.data);
  const uint64_t size = file.size;
  if (size < 3 || d[0] != 0x6C || d[1] != 0x1B)
    return sai_set_error(SAI_ERR_ARG, "%s: not a PLINK 2 .pgen file (it does not start with the bytes 6C 1B)", path.c_str());
  const unsigned mode = d[2];
  if (mode == 0x01)
    return sai_set_error(SAI_ERR_UNSUPPORTED, "%s: storage mode 0x01: this is a PLINK 1 .bed file, give its fileset with --bfile", path.c_str());
  if (mode != 0x02 && mode != 0x10)
    return sai_set_error(SAI_ERR_UNSUPPORTED, "%s: storage mode 0x%02X is not supported (0x02 and 0x10 are)", path.c_str(), mode);
  if (size < 12) return sai_set_error(SAI_ERR_ARG, "%s: %llu bytes, shorter than the 12-byte header", path.c_str(), static_cast<unsigned long long>(size));
  idx.mode = mode;
  const uint64_t variant_ct = load_le(d + 3, 4), sample_ct = load_le(d + 7, 4);
  if (static_cast<int64_t>(variant_ct) != idx.rows.n_lines)
    return sai_set_error(SAI_ERR_ARG, "%s: the header counts %llu variants, the .pvar has %lld", path.c_str(),
                         static_cast<unsigned long long>(variant_ct), static_cast<long long>(idx.rows.n_lines));
  if (static_cast<int64_t>(sample_ct) != idx.sample_ct)
    return sai_set_error(SAI_ERR_ARG, "%s: the header counts %llu samples, the .psam has %lld", path.c_str(),
                         static_cast<unsigned long long>(sample_ct), static_cast<long long>(idx.sample_ct));
  if (sample_ct == 0 || sample_ct > 0x7FFFFFFFull) return sai_set_error(SAI_ERR_UNSUPPORTED, "%s: %llu samples", path.c_str(), static_cast<unsigned long long>(sample_ct));
  idx.variant_ct = static_cast<int64_t>(variant_ct);
  const uint64_t row_bytes = (sample_ct + 3) / 4;
  const size_t n_rows = idx.rows.pos.size();
  idx.rec.assign(3 * n_rows, -1);
  idx.base.assign(3 * n_rows, -1);
  if (mode == 0x02) {
    const uint64_t want = 12 + variant_ct * row_bytes;
    if (size != want)
      return sai_set_error(SAI_ERR_ARG, "%s: %llu bytes, expected %llu (12 + %llu variants x %llu bytes for %llu samples): truncated, or not the .pgen of this fileset",
                           path.c_str(), static_cast<unsigned long long>(size), static_cast<unsigned long long>(want),
                           static_cast<unsigned long long>(variant_ct), static_cast<unsigned long long>(row_bytes),
                           static_cast<unsigned long long>(sample_ct));
    for (size_t k = 0; k < n_rows; ++k) {
      idx.rec[3 * k] = static_cast<int64_t>(12 + static_cast<uint64_t>(idx.rows.file_row[k]) * row_bytes);
      idx.rec[3 * k + 1] = static_cast<int64_t>(row_bytes);
      idx.rec[3 * k + 2] = 0;
    }
    return SAI_OK;
  }
  const unsigned control = d[11];
  const unsigned c = control & 15u;
  if (c >= 8) return sai_set_error(SAI_ERR_UNSUPPORTED, "%s: the header control byte %02X has a vrtype and record-length code of %u (0 to 7 are defined)", path.c_str(), control, c);
  const bool wide_types = c >= 4;
  const unsigned len_bytes = (c & 3u) + 1, allele_bytes = (control >> 4) & 3u;
  const bool flags = (control >> 6) == 3u;
  const uint64_t n_blocks = (variant_ct + kPgenBlock - 1) / kPgenBlock;
  uint64_t cursor = 12 + 8 * n_blocks;
  if (cursor > size) return sai_set_error(SAI_ERR_ARG, "%s: truncated inside the block offsets", path.c_str());
  std::vector<int64_t> off(variant_ct);
  std::vector<uint32_t> len(variant_ct);
  std::vector<uint8_t> vrtype(variant_ct);
  std::vector<int64_t> base_of(variant_ct);
  uint64_t records_end = 0;  // end of the records seen so far
  int64_t last_base = -1;
  for (uint64_t b = 0; b < n_blocks; ++b) {
    const uint64_t v0 = b * kPgenBlock, n = std::min<uint64_t>(kPgenBlock, variant_ct - v0);
    const uint64_t type_bytes = wide_types ? n : (n + 1) / 2;
    const uint64_t need = type_bytes + n * len_bytes + n * allele_bytes + (flags ? (n + 7) / 8 : 0);
    if (need > size - cursor) return sai_set_error(SAI_ERR_ARG, "%s: truncated inside the header of block %llu", path.c_str(), static_cast<unsigned long long>(b));
    const uint8_t* types = d + cursor;
    const uint8_t* lens = types + type_bytes;
    cursor += need;
    uint64_t at = load_le(d + 12 + 8 * b, 8);
    if (at > size || at < records_end)
      return sai_set_error(SAI_ERR_ARG, "%s: block %llu starts at byte %llu, which %s", path.c_str(), static_cast<unsigned long long>(b),
                           static_cast<unsigned long long>(at), at > size ? "is outside the file" : "overlaps the records of the block before");
    for (uint64_t j = 0; j < n; ++j) {
      const uint64_t v = v0 + j;
      const uint8_t t = wide_types ? types[j] : static_cast<uint8_t>((types[j >> 1] >> (4 * (j & 1))) & 15u);
      const uint64_t l = load_le(lens + j * len_bytes, static_cast<int>(len_bytes));
      if (l > size - at)
        return sai_set_error(SAI_ERR_ARG, "%s: the record of variant %llu (%llu bytes from byte %llu) leaves the file", path.c_str(),
                             static_cast<unsigned long long>(v + 1), static_cast<unsigned long long>(l), static_cast<unsigned long long>(at));
      vrtype[v] = t;
      off[v] = static_cast<int64_t>(at);
      len[v] = static_cast<uint32_t>(l);
      at += l;
      const unsigned kind = t & 7u;
      if (kind == 2 || kind == 3) {
        if (j == 0)
          return sai_set_error(SAI_ERR_ARG, "%s: variant %llu, the first of block %llu, is of type %u: it has no record to differ from", path.c_str(),
                               static_cast<unsigned long long>(v + 1), static_cast<unsigned long long>(b), kind);
      } else {
        last_base = static_cast<int64_t>(v);
      }
      base_of[v] = (kind == 2 || kind == 3) ? last_base : -1;
    }
    records_end = at;
  }
  for (uint64_t b = 0; b < n_blocks; ++b)
    if (load_le(d + 12 + 8 * b, 8) < cursor)
      return sai_set_error(SAI_ERR_ARG, "%s: block %llu starts at byte %llu, inside the header (%llu bytes)", path.c_str(),
                           static_cast<unsigned long long>(b), static_cast<unsigned long long>(load_le(d + 12 + 8 * b, 8)),
                           static_cast<unsigned long long>(cursor));
  for (size_t k = 0; k < n_rows; ++k) {
    const int64_t v = idx.rows.file_row[k];
    if (vrtype[v] & 8u)
      return sai_set_error(SAI_ERR_UNSUPPORTED, "%s: variant %lld (position %d) is multiallelic: split it into biallelic records first", path.c_str(),
                           static_cast<long long>(v + 1), idx.rows.pos[k]);
    if (len[v] == 0)
      return sai_set_error(SAI_ERR_ARG, "%s: the record of variant %lld is empty", path.c_str(), static_cast<long long>(v + 1));
    idx.rec[3 * k] = off[v];
    idx.rec[3 * k + 1] = len[v];
    idx.rec[3 * k + 2] = vrtype[v];
    const int64_t bv = base_of[v];
    if (bv >= 0) {
      if (len[bv] == 0)
        return sai_set_error(SAI_ERR_ARG, "%s: the record of variant %lld is empty", path.c_str(), static_cast<long long>(bv + 1));
      idx.base[3 * k] = off[bv];
      idx.base[3 * k + 1] = len[bv];
      idx.base[3 * k + 2] = vrtype[bv];
    }
  }
  return SAI_OK;
}

int pgen_open_impl(const char* prefix, const char* chrom, int64_t start, int64_t end, int32_t n_samples,
                   const char* const* sample_names, const int32_t* ploidy, const char* anc_bed_path, int32_t n_threads,
                   sai_pgen_index** index_out) {
  if (!prefix || !chrom || !index_out) return sai_set_error(SAI_ERR_ARG, "NULL argument");
  *index_out = nullptr;
  if (n_samples < 0 || (n_samples > 0 && (!sample_names || !ploidy))) return sai_set_error(SAI_ERR_ARG, "bad sample selection");
  for (int32_t s = 0; s < n_samples; ++s)  // before anything is read
    if (ploidy[s] < 1 || ploidy[s] > 2)
      return sai_set_error(SAI_ERR_ARG, "sample %s is configured with ploidy %d: a PLINK 2 fileset is read as haploid and diploid hard calls only",
                           sample_names[s], ploidy[s]);
  if (n_threads < 1) n_threads = 1;
  const std::string pre(prefix), c(chrom);
  std::unique_ptr<sai_pgen_index> holder(new sai_pgen_index);
  sai_pgen_index& idx = *holder;
  int name_col = 1;
  bool psam_header = false;
  if (int rc = psam_layout(pre + ".psam", &name_col, &psam_header)) return rc;
  if (int rc = resolve_samples(pre + ".psam", name_col, psam_header, n_samples, sample_names, idx.col_of_slot, &idx.sample_ct)) return rc;
  VariantLayout lay;
  if (int rc = pvar_layout(pre + ".pvar", &lay)) return rc;
  AncMap anc;
  if (anc_bed_path) {
    if (int rc = load_anc(anc_bed_path, c, start, end, anc, &idx.n_anc_entries)) return rc;
  }
  if (int rc = variant_pass(pre + ".pvar", lay, c, start, end, anc, true, n_threads, idx.rows)) return rc;
  if (idx.rows.first_multi >= 0)
    return sai_set_error(SAI_ERR_UNSUPPORTED, "%s.pvar: variant %lld is multiallelic (a comma in ALT): split it into biallelic records first", pre.c_str(),
                         static_cast<long long>(idx.rows.first_multi + 1));
  if (int rc = read_pgen_header(pre + ".pgen", idx)) return rc;
  *index_out = holder.release();
  return SAI_OK;
}

// ---- the host decoder ----

inline uint32_t lut_for(int32_t ploidy, bool flip) {
  return ploidy == 2 ? (flip ? kPgenLutP2Flip : kPgenLutP2) : (flip ? kPgenLutP1Flip : kPgenLutP1);
}

int pgen_decode_host_impl(const uint8_t* bytes, int64_t n_bytes, int64_t n_out_rows, const int64_t* rec, const int64_t* base,
                          const uint8_t* row_flip, int32_t sample_ct, int32_t n_slots, const int32_t* col_of_slot,
                          const int32_t* ploidy_of_slot, int8_t* out, int32_t* status, int32_t n_threads) {
  if (n_bytes < 0 || n_out_rows < 0 || sample_ct < 1 || n_slots < 1) return sai_set_error(SAI_ERR_ARG, "size out of range");
  if (n_out_rows == 0) return SAI_OK;
  if (!rec || !base || !row_flip || !col_of_slot || !ploidy_of_slot || !out || !status || (n_bytes > 0 && !bytes))
    return sai_set_error(SAI_ERR_ARG, "NULL buffer");
  const uint32_t n = static_cast<uint32_t>(sample_ct);
  std::atomic<bool> failed{false};
  auto decode = [&](int64_t lo, int64_t hi) {
    std::vector<uint8_t> codes;
    try {
      codes.resize(n);
    } catch (...) {
      failed = true;
      return;
    }
    for (int64_t r = lo; r < hi; ++r) {
      int8_t* o = out + r * n_slots;
      const RecordRef own = {rec[3 * r], rec[3 * r + 1], rec[3 * r + 2]};
      const RecordRef from = {base[3 * r], base[3 * r + 1], base[3 * r + 2]};
      if (!expand_record(bytes, n_bytes, own, from, n, codes.data())) {
        memset(o, 0, static_cast<size_t>(n_slots));
        status[r] = kPgenBadRecord;
        continue;
      }
      int32_t st = 0;
      const bool flip = row_flip[r] != 0;
      for (int32_t s = 0; s < n_slots; ++s) {
        const int32_t col = col_of_slot[s], pl = ploidy_of_slot[s];
        if (col < 0 || col >= sample_ct || pl < 1 || pl > 2) {
          o[s] = 0;
          st = kPgenBadIndex;
          continue;
        }
        const uint32_t code = codes[col];
        if (pl == 1 && code == kPgenHet) st = std::max(st, n_slots - s);
        o[s] = static_cast<int8_t>((lut_for(pl, flip) >> (8 * code)) & 0xFFu);
      }
      status[r] = st;
    }
  };
  const int64_t cells = n_out_rows * (static_cast<int64_t>(n_slots) + sample_ct);
  const int nt = static_cast<int>(std::max<int64_t>(1, std::min<int64_t>({static_cast<int64_t>(std::max(n_threads, 1)), n_out_rows, cells / (int64_t(1) << 18) + 1})));
  ThreadGroup tg;
  for (int t = 1; t < nt; ++t) tg.spawn([&decode, t, nt, n_out_rows] { decode(n_out_rows * t / nt, n_out_rows * (t + 1) / nt); });
  decode(0, n_out_rows / nt);
  tg.join();
  if (failed) return sai_set_error(SAI_ERR_HIP, "out of host memory");
  return SAI_OK;
}

}  // namespace

extern "C" {

int sai_pgen_abi_version(void) { return SAI_PGEN_ABI_VERSION; }

int sai_pgen_scan(const char* prefix, const char* chrom, int64_t* first_pos, int64_t* last_pos) {
  return guarded("sai_pgen_scan", [&] { return pgen_scan_impl(prefix, chrom, first_pos, last_pos); });
}

int sai_pgen_open(const char* prefix, const char* chrom, int64_t start, int64_t end, int32_t n_samples,
                  const char* const* sample_names, const int32_t* ploidy, const char* anc_bed_path, int32_t n_threads,
                  sai_pgen_index** index_out) {
  return guarded("sai_pgen_open", [&] {
    return pgen_open_impl(prefix, chrom, start, end, n_samples, sample_names, ploidy, anc_bed_path, n_threads, index_out);
  });
}

int sai_pgen_index_info(const sai_pgen_index* index, int64_t* n_rows, int64_t* n_matched, int64_t* n_anc_entries,
                        int64_t* sample_ct, int64_t* variant_ct, int64_t* mode, int64_t* first_pos, int64_t* last_pos) {
  if (!index) return sai_set_error(SAI_ERR_ARG, "index is NULL");
  if (n_rows) *n_rows = static_cast<int64_t>(index->rows.pos.size());
  if (n_matched) *n_matched = index->rows.n_matched;
  if (n_anc_entries) *n_anc_entries = index->n_anc_entries;
  if (sample_ct) *sample_ct = index->sample_ct;
  if (variant_ct) *variant_ct = index->variant_ct;
  if (mode) *mode = index->mode;
  if (first_pos) *first_pos = index->rows.first;
  if (last_pos) *last_pos = index->rows.last;
  return SAI_OK;
}

int sai_pgen_index_copy(const sai_pgen_index* index, int32_t* pos, int64_t* file_row, uint8_t* flip, int32_t* col_of_slot,
                        int64_t* rec, int64_t* base) {
  if (!index) return sai_set_error(SAI_ERR_ARG, "index is NULL");
  const size_t n = index->rows.pos.size();
  if (pos && n) memcpy(pos, index->rows.pos.data(), n * sizeof(int32_t));
  if (file_row && n) memcpy(file_row, index->rows.file_row.data(), n * sizeof(int64_t));
  if (flip && n) memcpy(flip, index->rows.flip.data(), n);
  if (col_of_slot && !index->col_of_slot.empty()) memcpy(col_of_slot, index->col_of_slot.data(), index->col_of_slot.size() * sizeof(int32_t));
  if (rec && n) memcpy(rec, index->rec.data(), 3 * n * sizeof(int64_t));
  if (base && n) memcpy(base, index->base.data(), 3 * n * sizeof(int64_t));
  return SAI_OK;
}

int sai_pgen_index_close(sai_pgen_index* index) {
  delete index;
  return SAI_OK;
}

int sai_pgen_decode_host(const uint8_t* bytes, int64_t n_bytes, int64_t n_out_rows, const int64_t* rec, const int64_t* base,
                         const uint8_t* row_flip, int32_t sample_ct, int32_t n_slots, const int32_t* col_of_slot,
                         const int32_t* ploidy_of_slot, int8_t* out, int32_t* status, int32_t n_threads) {
  return guarded("sai_pgen_decode_host", [&] {
    return pgen_decode_host_impl(bytes, n_bytes, n_out_rows, rec, base, row_flip, sample_ct, n_slots, col_of_slot, ploidy_of_slot,
                                 out, status, n_threads);
  });
}

}  // extern "C"
