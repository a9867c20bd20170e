// The .csi index of a BCF file and the host route that begins where it says, as a stand-alone program for
// tests/test_bcf_index_cpu.py: the test compiles it with -fsanitize=address,undefined over the host units of libsaihip,
// hands it the files it wrote and compares what it prints with what the library answers.
//
//   csi_dump FILE INDEX CHROM CONTIG N_THREADS BUFFER_BYTES N_REGIONS START END ... NAME:PLOIDY ...
//
// prints "index MIN_SHIFT DEPTH N_REF N_NO_COOR" ("index refused" where the index fails a check: the regions are then
// streamed without it), and per region "query ANSWER VOFFSET", one line per selected row "POS FLIP d0 d1 ...",
// "counts n_matched n_anc_entries" and "seek MADE VOFFSET FILE_BYTES MEMBERS".  Exit status 3 with the library's message
// on stderr when the stream or the decoder refuses.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "saihip_bcf_index.h"

static int refused() {
  fprintf(stderr, "%s\n", sai_last_error());
  return 3;
}

int main(int argc, char** argv) {
  if (argc < 8) {
    fprintf(stderr, "usage: csi_dump FILE INDEX CHROM CONTIG N_THREADS BUFFER_BYTES N_REGIONS START END ... NAME:PLOIDY ...\n");
    return 2;
  }
  const char* path = argv[1];
  const int contig = atoi(argv[4]), n_threads = atoi(argv[5]);
  const long long cap = atoll(argv[6]);
  const int n_regions = atoi(argv[7]);
  if (n_regions < 0 || argc < 8 + 2 * n_regions) return 2;
  std::vector<std::string> names;
  std::vector<int32_t> ploidy;
  for (int i = 8 + 2 * n_regions; i < argc; ++i) {
    const std::string a = argv[i];
    const size_t colon = a.rfind(':');
    if (colon == std::string::npos) return 2;
    names.push_back(a.substr(0, colon));
    ploidy.push_back(atoi(a.c_str() + colon + 1));
  }
  std::vector<const char*> name_ptr;
  for (const std::string& s : names) name_ptr.push_back(s.c_str());
  const int32_t n = static_cast<int32_t>(names.size());
  FILE* f = fopen(path, "rb");
  if (!f) return 2;
  fseek(f, 0, SEEK_END);
  const long long size = ftell(f);
  fclose(f);
  sai_bcf_index* index = nullptr;
  if (sai_bcf_index_open(argv[2], size, &index)) {
    printf("index refused\n");
  } else {
    int32_t min_shift, depth, n_ref;
    int64_t n_no_coor;
    if (sai_bcf_index_info(index, &min_shift, &depth, &n_ref, &n_no_coor)) return refused();
    printf("index %d %d %d %lld\n", min_shift, depth, n_ref, (long long)n_no_coor);
  }
  std::vector<uint8_t> buf0(static_cast<size_t>(cap)), buf1(static_cast<size_t>(cap));
  int rc = 0;
  for (int k = 0; k < n_regions && !rc; ++k) {
    const long long start = atoll(argv[8 + 2 * k]), end = atoll(argv[9 + 2 * k]);
    if (index) {
      int32_t answer;
      uint64_t v;
      if (sai_bcf_index_query(index, contig, start, end, &answer, &v)) { rc = refused(); break; }
      printf("query %d %llu\n", answer, (unsigned long long)v);
    }
    sai_bcf_stream* st = nullptr;
    if (sai_bcf_stream_open_at(path, argv[3], start, end, n, name_ptr.data(), ploidy.data(), nullptr, n_threads, buf0.data(), buf1.data(), cap, index, &st)) {
      rc = refused();
      break;
    }
    std::vector<int32_t> col(static_cast<size_t>(n) + 1);
    int32_t n_cols = 0;
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
      for (int64_t r = 0; r < n_rows; ++r) {
        printf("%d %d", pos[r], flip[r]);
        for (int32_t s = 0; s < n; ++s) printf(" %d", out[static_cast<size_t>(r) * n + s]);
        printf("\n");
      }
    }
    if (!rc) {
      int64_t n_matched = 0, n_anc = 0, file_bytes = 0, members = 0;
      int32_t made = 0;
      uint64_t v = 0;
      if (sai_bcf_stream_selection(st, nullptr, 0, nullptr, &n_matched, &n_anc) == 0) printf("counts %lld %lld\n", (long long)n_matched, (long long)n_anc);
      if (sai_bcf_stream_seek_stats(st, &made, &v, &file_bytes, &members)) rc = refused();
      else printf("seek %d %llu %lld %lld\n", made, (unsigned long long)v, (long long)file_bytes, (long long)members);
    }
    sai_bcf_stream_close(st);
  }
  sai_bcf_index_close(index);
  return rc;
}
