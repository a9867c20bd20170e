// The host part of the EIGENSOFT fileset reader as a stand-alone program, for tests/test_eigenstrat_cpu.py: the
// test compiles it with -fsanitize=address,undefined over the host units of libsaihip, hands it the filesets
// it wrote and compares what it prints with what the library answers.
//
//   eigenstrat_dump PREFIX CHROM START END ANC_FILE|- N_THREADS NAME:PLOIDY ...
//
// prints "info n_rows n_matched n_anc_entries first last encoding record_bytes data_offset", then one line per
// selected row: "POS FILE_ROW FLIP STATUS d0 d1 ...".  Exit status 3 with the library's message on stderr when
// the index or the decoder refuses.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "saihip_eigenstrat.h"

int main(int argc, char** argv) {
  if (argc < 7) {
    fprintf(stderr, "usage: eigenstrat_dump PREFIX CHROM START END ANC|- N_THREADS NAME:PLOIDY ...\n");
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
  sai_eigenstrat_index* idx = nullptr;
  if (sai_eigenstrat_open(prefix.c_str(), argv[2], start, end, n, name_ptr.data(), ploidy.data(), anc, n_threads, &idx)) {
    fprintf(stderr, "%s\n", sai_last_error());
    return 3;
  }
  int64_t n_rows, n_matched, n_anc, n_ind, n_snp, first, last, encoding, record_bytes, data_offset;
  sai_eigenstrat_index_info(idx, &n_rows, &n_matched, &n_anc, &n_ind, &n_snp, &first, &last, &encoding, &record_bytes, &data_offset);
  std::vector<int32_t> pos(n_rows), col(n);
  std::vector<int64_t> file_row(n_rows);
  std::vector<uint8_t> flip(n_rows);
  sai_eigenstrat_index_copy(idx, pos.data(), file_row.data(), flip.data(), col.data());
  sai_eigenstrat_index_close(idx);
  printf("info %lld %lld %lld %lld %lld %lld %lld %lld\n", (long long)n_rows, (long long)n_matched, (long long)n_anc, (long long)first,
         (long long)last, (long long)encoding, (long long)record_bytes, (long long)data_offset);
  // the records of the whole file; the last line of a text file may lack its newline
  const bool transposed = encoding == SAI_EIGENSTRAT_TRANSPOSED;
  const int64_t n_records = transposed ? n_ind : n_snp;
  std::vector<uint8_t> geno(static_cast<size_t>(n_records * record_bytes), 0);
  FILE* f = fopen((prefix + ".geno").c_str(), "rb");
  if (!f || fseek(f, static_cast<long>(data_offset), SEEK_SET) != 0) return 4;
  const size_t got = fread(geno.data(), 1, geno.size(), f);
  fclose(f);
  if (got + 2 < geno.size()) return 4;
  std::vector<int32_t> rib(n_rows), status(n_rows);
  for (int64_t k = 0; k < n_rows; ++k) rib[k] = static_cast<int32_t>(file_row[k]);
  std::vector<int8_t> out(static_cast<size_t>(n_rows) * n);
  if (n > 0 && sai_eigenstrat_decode_host(static_cast<int32_t>(encoding), geno.data(), n_snp, record_bytes, 0, n_rows, rib.data(), flip.data(),
                                          static_cast<int32_t>(n_ind), n, col.data(), ploidy.data(), out.data(), status.data(), n_threads)) {
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
