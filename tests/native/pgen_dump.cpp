// The host part of the PLINK 2 fileset reader as a stand-alone program, for tests/test_pgen_cpu.py: the test
// compiles it with -fsanitize=address,undefined over the host units of libsaihip, hands it the filesets and the
// damaged records it wrote and compares what it prints with what the library answers.
//
//   pgen_dump PREFIX CHROM START END ANC_FILE|- N_THREADS NAME:PLOIDY ...
//
// prints "info n_rows n_matched n_anc_entries first last sample_ct variant_ct mode", then one line per selected row:
// "POS FILE_ROW FLIP STATUS d0 d1 ...".  Exit status 3 with the library's message on stderr when the index is
// refused.
//
//   pgen_dump --records BYTES_FILE TABLE_FILE SAMPLE_CT
//
// decodes the records of TABLE_FILE (one per line: offset length vrtype base_offset base_length base_vrtype flip)
// from the bytes of BYTES_FILE, held in a heap block of exactly their size, into every sample at ploidy 2, and
// prints "STATUS d0 d1 ..." per record.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "saihip_pgen.h"

static bool read_file(const std::string& path, std::vector<uint8_t>& out) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return false;
  fseek(f, 0, SEEK_END);
  const long size = ftell(f);
  fseek(f, 0, SEEK_SET);
  out.resize(static_cast<size_t>(size));
  const bool ok = size == 0 || fread(out.data(), 1, out.size(), f) == out.size();
  fclose(f);
  return ok;
}

static int dump_records(const char* bytes_file, const char* table_file, int32_t sample_ct) {
  std::vector<uint8_t> bytes;
  if (!read_file(bytes_file, bytes)) return 4;
  std::vector<int64_t> rec, base;
  std::vector<uint8_t> flip;
  FILE* f = fopen(table_file, "r");
  if (!f) return 4;
  long long v[7];
  while (fscanf(f, "%lld %lld %lld %lld %lld %lld %lld", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6]) == 7) {
    rec.insert(rec.end(), {v[0], v[1], v[2]});
    base.insert(base.end(), {v[3], v[4], v[5]});
    flip.push_back(static_cast<uint8_t>(v[6]));
  }
  fclose(f);
  const int64_t n_rows = static_cast<int64_t>(flip.size());
  std::vector<int32_t> col(sample_ct), ploidy(sample_ct, 2), status(n_rows);
  for (int32_t s = 0; s < sample_ct; ++s) col[s] = s;
  std::vector<int8_t> out(static_cast<size_t>(n_rows) * sample_ct);
  if (sai_pgen_decode_host(bytes.data(), static_cast<int64_t>(bytes.size()), n_rows, rec.data(), base.data(), flip.data(), sample_ct, sample_ct,
                           col.data(), ploidy.data(), out.data(), status.data(), 2)) {
    fprintf(stderr, "%s\n", sai_last_error());
    return 3;
  }
  for (int64_t k = 0; k < n_rows; ++k) {
    printf("%d", status[k]);
    for (int32_t s = 0; s < sample_ct; ++s) printf(" %d", out[static_cast<size_t>(k) * sample_ct + s]);
    printf("\n");
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 5 && strcmp(argv[1], "--records") == 0) return dump_records(argv[2], argv[3], atoi(argv[4]));
  if (argc < 7) {
    fprintf(stderr, "usage: pgen_dump PREFIX CHROM START END ANC|- N_THREADS NAME:PLOIDY ...\n");
    return 2;
  }
  const std::string prefix = argv[1];
  const long long start = atoll(argv[3]), end = atoll(argv[4]);
  const char* anc = strcmp(argv[5], "-") == 0 ? nullptr : argv[5];
  const int n_threads = atoi(argv[6]);
  std::vector<std::string> names;
  std::vector<int32_t> ploidy;
  for (int i = 7; i < argc; ++i) {
    const std::string a = argv[i];
    const size_t colon = a.rfind(':');
    if (colon == std::string::npos) return 2;
    names.push_back(a.substr(0, colon));
    ploidy.push_back(atoi(a.c_str() + colon + 1));
  }
  std::vector<const char*> name_ptr;
  for (const std::string& s : names) name_ptr.push_back(s.c_str());
  const int32_t n = static_cast<int32_t>(names.size());
  sai_pgen_index* idx = nullptr;
  if (sai_pgen_open(prefix.c_str(), argv[2], start, end, n, name_ptr.data(), ploidy.data(), anc, n_threads, &idx)) {
    fprintf(stderr, "%s\n", sai_last_error());
    return 3;
  }
  int64_t n_rows, n_matched, n_anc, sample_ct, variant_ct, mode, first, last;
  sai_pgen_index_info(idx, &n_rows, &n_matched, &n_anc, &sample_ct, &variant_ct, &mode, &first, &last);
  std::vector<int32_t> pos(n_rows), col(n);
  std::vector<int64_t> file_row(n_rows), rec(3 * n_rows), base(3 * n_rows);
  std::vector<uint8_t> flip(n_rows);
  sai_pgen_index_copy(idx, pos.data(), file_row.data(), flip.data(), col.data(), rec.data(), base.data());
  sai_pgen_index_close(idx);
  printf("info %lld %lld %lld %lld %lld %lld %lld %lld\n", (long long)n_rows, (long long)n_matched, (long long)n_anc, (long long)first,
         (long long)last, (long long)sample_ct, (long long)variant_ct, (long long)mode);
  std::vector<uint8_t> bytes;
  if (!read_file(prefix + ".pgen", bytes)) return 4;
  std::vector<int32_t> status(n_rows);
  std::vector<int8_t> out(static_cast<size_t>(n_rows) * n);
  if (n > 0 && sai_pgen_decode_host(bytes.data(), static_cast<int64_t>(bytes.size()), n_rows, rec.data(), base.data(), flip.data(),
                                    static_cast<int32_t>(sample_ct), n, col.data(), ploidy.data(), out.data(), status.data(), n_threads)) {
    fprintf(stderr, "%s\n", sai_last_error());
    return 3;
  }
  for (int64_t k = 0; k < n_rows; ++k) {
    printf("%d %lld %d %d", pos[k], (long long)file_row[k], flip[k], n > 0 ? status[k] : 0);
    for (int32_t s = 0; s < n; ++s) printf(" %d", out[static_cast<size_t>(k) * n + s]);
    printf("\n");
  }
  return 0;
}
