// Host side of the PLINK 1 fileset reader: the index of PREFIX.fam / PREFIX.bim (which .fam column is
// which requested sample, which .bim rows lie in the region, which of them the ancestral-allele rule
// keeps or flips) and the host decoder of .bed rows.  The .bed itself is never parsed here beyond its
// three magic bytes and its size: rows are fixed-length, so the selected rows are byte ranges the
// streaming reader (sai_amd/utils/plink.py) preads straight into pinned memory.
//
// The rules are those of the VCF readers with A2 in the place of REF and A1 in the place of ALT
// (what `plink2 --make-bed` and `plink --keep-allele-order` write from a VCF): rows of the chromosome
// inside [start, end] in file order; with an ancestral-allele file only listed sites are kept, a site
// whose ancestral allele is A1 is flipped, one whose ancestral allele is neither is dropped -- the
// decision of parse_lines() in ingest_base.hpp, restated in anc_decision() of fileset_index.hpp, which also holds the
// passes over the .fam and the .bim (shared with the EIGENSTRAT reader).

#include "fileset_index.hpp"
#include "plink_codes.hpp"
#include "saihip_plink.h"

struct sai_plink_index {
  VariantRows rows;  // file_row = 0-based row of the .bed (= record line of the .bim)
  std::vector<int32_t> col_of_slot;
  int64_t n_anc_entries = 0;
  int64_t row_bytes = 0;
  int64_t n_fam = 0;
};

namespace {

// .bim: chromosome, id, genetic position, position, A1 (plays ALT), A2 (plays REF)
constexpr VariantLayout kBimLayout = {0, 3, 5, 4, 6, false, false};

int plink_scan_impl(const char* prefix, const char* chrom, int64_t* first_pos, int64_t* last_pos) {
  if (!prefix || !chrom || !first_pos || !last_pos) return sai_set_error(SAI_ERR_ARG, "NULL argument");
  VariantRows rows;
  AncMap none;
  if (int rc = variant_pass(std::string(prefix) + ".bim", kBimLayout, chrom, -1, -1, none, false, kScanThreads, rows)) return rc;
  *first_pos = rows.first;
  *last_pos = rows.last;
  return SAI_OK;
}

int plink_open_impl(const char* prefix, const char* chrom, int64_t start, int64_t end, int32_t n_samples,
                    const char* const* sample_names, const int32_t* ploidy, const char* anc_bed_path, int32_t n_threads,
                    sai_plink_index** index_out) {
  if (!prefix || !chrom || !index_out) return sai_set_error(SAI_ERR_ARG, "NULL argument");
  *index_out = nullptr;
  if (n_samples < 0 || (n_samples > 0 && (!sample_names || !ploidy))) return sai_set_error(SAI_ERR_ARG, "bad sample selection");
  for (int32_t s = 0; s < n_samples; ++s)  // before anything is read
    if (ploidy[s] < 1 || ploidy[s] > 2)
      return sai_set_error(SAI_ERR_ARG, "sample %s is configured with ploidy %d: a PLINK 1 fileset holds haploid and diploid calls only",
                           sample_names[s], ploidy[s]);
  if (n_threads < 1) n_threads = 1;
  const std::string pre(prefix), c(chrom);
  std::unique_ptr<sai_plink_index> holder(new sai_plink_index);
  sai_plink_index& idx = *holder;
  // .fam: one sample per record line, the name is column 2 (IID)
  if (int rc = resolve_samples(pre + ".fam", 1, false, n_samples, sample_names, idx.col_of_slot, &idx.n_fam)) return rc;
  idx.row_bytes = (idx.n_fam + 3) / 4;
  AncMap anc;
  if (anc_bed_path) {
    if (int rc = load_anc(anc_bed_path, c, start, end, anc, &idx.n_anc_entries)) return rc;
  }
  if (int rc = variant_pass(pre + ".bim", kBimLayout, c, start, end, anc, true, n_threads, idx.rows)) return rc;
  {  // .bed: magic, variant-major, exactly one row per .bim line
    const std::string path = pre + ".bed";
    const int fd = open(path.c_str(), O_RDONLY);
    if (fd < 0) return sai_set_error(SAI_ERR_ARG, "cannot open %s", path.c_str());
    struct FdGuard { int fd; ~FdGuard() { close(fd); } } guard{fd};
    struct stat sb;
    if (fstat(fd, &sb) != 0) return sai_set_error(SAI_ERR_ARG, "cannot stat %s", path.c_str());
    unsigned char magic[3] = {0, 0, 0};
    const ssize_t got = pread(fd, magic, 3, 0);
    if (got != 3 || magic[0] != 0x6C || magic[1] != 0x1B)
      return sai_set_error(SAI_ERR_ARG, "%s: not a PLINK 1 .bed file (it does not start with the bytes 6C 1B)", path.c_str());
    if (magic[2] == 0x00)
      return sai_set_error(SAI_ERR_UNSUPPORTED, "%s: sample-major .bed files are not supported (third byte 00); rewrite the fileset variant-major", path.c_str());
    if (magic[2] != 0x01)
      return sai_set_error(SAI_ERR_ARG, "%s: not a PLINK 1 .bed file (third byte %02X, expected 01)", path.c_str(), magic[2]);
    const long long want = 3 + static_cast<long long>(idx.rows.n_lines) * static_cast<long long>(idx.row_bytes);
    if (static_cast<long long>(sb.st_size) != want)
      return sai_set_error(SAI_ERR_ARG, "%s: %lld bytes, expected %lld (3 + %lld variants of the .bim x %lld bytes for the %lld samples of the .fam): truncated, or not the .bed of this fileset",
                           path.c_str(), static_cast<long long>(sb.st_size), want, static_cast<long long>(idx.rows.n_lines),
                           static_cast<long long>(idx.row_bytes), static_cast<long long>(idx.n_fam));
  }
  *index_out = holder.release();
  return SAI_OK;
}

inline uint32_t lut_for(int32_t ploidy, bool flip) {
  return ploidy == 2 ? (flip ? kPlinkLutP2Flip : kPlinkLutP2) : (flip ? kPlinkLutP1Flip : kPlinkLutP1);
}

int plink_decode_host_impl(const uint8_t* rows, int64_t n_batch_rows, int64_t row_bytes, int64_t n_out_rows,
                           const int32_t* row_in_batch, const uint8_t* row_flip, int32_t n_cols, int32_t n_slots,
                           const int32_t* col_of_slot, const int32_t* ploidy_of_slot, int8_t* out, int32_t* status,
                           int32_t n_threads) {
  if (n_batch_rows < 0 || row_bytes < 0 || n_out_rows < 0 || n_cols < 0 || n_slots < 1) return sai_set_error(SAI_ERR_ARG, "size out of range");
  if (static_cast<int64_t>(n_cols) > 4 * row_bytes) return sai_set_error(SAI_ERR_ARG, "n_cols exceeds the 4 * row_bytes genotypes of a row");
  if (n_out_rows == 0) return SAI_OK;
  if (!row_in_batch || !row_flip || !col_of_slot || !ploidy_of_slot || !out || !status || (n_batch_rows > 0 && row_bytes > 0 && !rows))
    return sai_set_error(SAI_ERR_ARG, "NULL buffer");
  auto decode = [&](int64_t lo, int64_t hi) {
    for (int64_t r = lo; r < hi; ++r) {
      int8_t* o = out + r * n_slots;
      int32_t st = 0;
      const int64_t rib = row_in_batch[r];
      const bool row_ok = rib >= 0 && rib < n_batch_rows;
      const uint8_t* src = row_ok ? rows + rib * row_bytes : nullptr;
      const bool flip = row_flip[r] != 0;
      for (int32_t s = 0; s < n_slots; ++s) {
        const int32_t col = col_of_slot[s], pl = ploidy_of_slot[s];
        if (!row_ok || col < 0 || col >= n_cols || pl < 1 || pl > 2) {
          o[s] = 0;
          st = kPlinkBadIndex;
          continue;
        }
        const uint32_t code = (src[col >> 2] >> (2 * (col & 3))) & 3u;
        if (pl == 1 && code == kPlinkHet) st = std::max(st, n_slots - s);
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

int sai_plink_abi_version(void) { return SAI_PLINK_ABI_VERSION; }

int sai_plink_scan(const char* prefix, const char* chrom, int64_t* first_pos, int64_t* last_pos) {
  return guarded("sai_plink_scan", [&] { return plink_scan_impl(prefix, chrom, first_pos, last_pos); });
}

int sai_plink_open(const char* prefix, const char* chrom, int64_t start, int64_t end, int32_t n_samples,
                   const char* const* sample_names, const int32_t* ploidy, const char* anc_bed_path, int32_t n_threads,
                   sai_plink_index** index_out) {
  return guarded("sai_plink_open", [&] {
    return plink_open_impl(prefix, chrom, start, end, n_samples, sample_names, ploidy, anc_bed_path, n_threads, index_out);
  });
}

int sai_plink_index_info(const sai_plink_index* index, int64_t* n_rows, int64_t* n_matched, int64_t* n_anc_entries,
                         int64_t* row_bytes, int64_t* n_fam, int64_t* n_bim, int64_t* first_pos, int64_t* last_pos) {
  if (!index) return sai_set_error(SAI_ERR_ARG, "index is NULL");
  if (n_rows) *n_rows = static_cast<int64_t>(index->rows.pos.size());
  if (n_matched) *n_matched = index->rows.n_matched;
  if (n_anc_entries) *n_anc_entries = index->n_anc_entries;
  if (row_bytes) *row_bytes = index->row_bytes;
  if (n_fam) *n_fam = index->n_fam;
  if (n_bim) *n_bim = index->rows.n_lines;
  if (first_pos) *first_pos = index->rows.first;
  if (last_pos) *last_pos = index->rows.last;
  return SAI_OK;
}

int sai_plink_index_copy(const sai_plink_index* index, int32_t* pos, int64_t* file_row, uint8_t* flip, int32_t* col_of_slot) {
  if (!index) return sai_set_error(SAI_ERR_ARG, "index is NULL");
  const size_t n = index->rows.pos.size();
  if (pos && n) memcpy(pos, index->rows.pos.data(), n * sizeof(int32_t));
  if (file_row && n) memcpy(file_row, index->rows.file_row.data(), n * sizeof(int64_t));
  if (flip && n) memcpy(flip, index->rows.flip.data(), n);
  if (col_of_slot && !index->col_of_slot.empty()) memcpy(col_of_slot, index->col_of_slot.data(), index->col_of_slot.size() * sizeof(int32_t));
  return SAI_OK;
}

int sai_plink_index_close(sai_plink_index* index) {
  delete index;
  return SAI_OK;
}

int sai_plink_decode_host(const uint8_t* rows, int64_t n_batch_rows, int64_t row_bytes, int64_t n_out_rows,
                          const int32_t* row_in_batch, const uint8_t* row_flip, int32_t n_cols, int32_t n_slots,
                          const int32_t* col_of_slot, const int32_t* ploidy_of_slot, int8_t* out, int32_t* status,
                          int32_t n_threads) {
  return guarded("sai_plink_decode_host", [&] {
    return plink_decode_host_impl(rows, n_batch_rows, row_bytes, n_out_rows, row_in_batch, row_flip, n_cols, n_slots,
                                  col_of_slot, ploidy_of_slot, out, status, n_threads);
  });
}

}  // extern "C"
