// The host part of the BCF reader as a stand-alone program, for tests/test_bcf_cpu.py: the test compiles it with
// -fsanitize=address,undefined over the host units of libsaihip, hands it the files it wrote and compares what it
// prints with what the library answers.
//
//   bcf_dump FILE CHROM START END ANC_FILE|- N_THREADS BUFFER_BYTES NAME:PLOIDY ...
//
// prints "probe P", "scan first last n_records_total n_samples", one line per selected row "POS FLIP WIDTH L STATUS
// d0 d1 ..." and at last "counts n_matched n_anc_entries" ("scan refused" where the scan refuses).  Exit status 3 with
// the library's message on stderr when the stream or the decoder refuses.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "saihip_bcf.h"

static int refused() {
  fprintf(stderr, "%s\n", sai_last_error());
  return 3;
}

int main(int argc, char** argv) {
  if (argc < 8) {
    fprintf(stderr, "usage: bcf_dump FILE CHROM START END ANC|- N_THREADS BUFFER_BYTES NAME:PLOIDY ...\n");
    return 2;
  }
  const char* path = argv[1];
  const long long start = atoll(argv[3]), end = atoll(argv[4]);
  const char* anc = strcmp(argv[5], "-") == 0 ? nullptr : argv[5];
  const int n_threads = atoi(argv[6]);
  const long long cap = atoll(argv[7]);
  std::vector<std::string> names;
  std::vector<int32_t> ploidy;
  for (int i = 8; i < argc; ++i) {
    const std::string a = argv[i];
    const size_t colon = a.rfind(':');
    if (colon == std::string::npos) return 2;
    names.push_back(a.substr(0, colon));
    ploidy.push_back(atoi(a.c_str() + colon + 1));
  }
  std::vector<const char*> name_ptr;
  for (const std::string& s : names) name_ptr.push_back(s.c_str());
  const int32_t n = static_cast<int32_t>(names.size());
  printf("probe %d\n", sai_bcf_probe(path));
  int64_t first, last, n_records, n_samples;
  // the scan follows the record chain of the whole file and may refuse where the stream, which stops behind the
  // chromosome's run and looks into the selected records, says something else: the stream's word is the exit status
  if (sai_bcf_scan(path, argv[2], &first, &last, &n_records, &n_samples)) printf("scan refused\n");
  else printf("scan %lld %lld %lld %lld\n", (long long)first, (long long)last, (long long)n_records, (long long)n_samples);
  std::vector<uint8_t> buf0(static_cast<size_t>(cap)), buf1(static_cast<size_t>(cap));
  sai_bcf_stream* st = nullptr;
  if (sai_bcf_stream_open(path, argv[2], start, end, n, name_ptr.data(), ploidy.data(), anc, n_threads, buf0.data(), buf1.data(), cap, &st))
    return refused();
  std::vector<int32_t> col(static_cast<size_t>(n) + 1);
  int32_t n_cols = 0;
  int rc = 0;
  for (;;) {
    int32_t b, done;
    int64_t n_bytes, n_rows;
    const int32_t *pos, *len;
    const uint8_t *flip, *width;
    const int64_t* off;
    if (sai_bcf_stream_next(st, &b, &n_bytes, &n_rows, &pos, &flip, &off, &width, &len, &done)) { rc = refused(); break; }
    if (done) break;
    if (sai_bcf_stream_selection(st, col.data(), n, &n_cols, nullptr, nullptr)) { rc = refused(); break; }
    std::vector<int8_t> out(static_cast<size_t>(n_rows) * n + 1);
    std::vector<int32_t> status(static_cast<size_t>(n_rows) + 1, 0);
    if (n > 0 && sai_bcf_decode_host(b ? buf1.data() : buf0.data(), n_bytes, n_rows, off, width, len, flip, n_cols, n, col.data(), ploidy.data(),
                                     out.data(), status.data(), n_threads)) { rc = refused(); break; }
    for (int64_t k = 0; k < n_rows; ++k) {
      if (off[k] % SAI_BCF_GT_ALIGN) { fprintf(stderr, "row %lld starts at %lld\n", (long long)k, (long long)off[k]); rc = 4; }
      printf("%d %d %d %d %d", pos[k], flip[k], width[k], len[k], status[k]);
      for (int32_t s = 0; s < n; ++s) printf(" %d", out[static_cast<size_t>(k) * n + s]);
      printf("\n");
    }
  }
  if (!rc) {
    int64_t n_matched = 0, n_anc = 0;
    if (sai_bcf_stream_selection(st, nullptr, 0, nullptr, &n_matched, &n_anc) == 0) printf("counts %lld %lld\n", (long long)n_matched, (long long)n_anc);
  }
  sai_bcf_stream_close(st);
  return rc;
}
