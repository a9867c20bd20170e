// The host decoder of .bed rows into the packed2 layout as a stand-alone program, for tests/test_bed_pack2_cpu.py:
// the test compiles it with -fsanitize=address,undefined over the host units of libsaihip, hands it rows in a
// file and compares what it prints with the numpy statement of the layout and with the library.
//
//   bed_pack2_dump ROWS_FILE ROW_BYTES N_COLS PLOIDY FIRST_COL CUT N_THREADS ROW_IN_BATCH,... FLIP,... COL,...
//
// decodes the rows in two calls cut at CUT (one call when CUT is 0) and prints the status values, the unfit
// values and the block as hexadecimal digits, one line each.  Every buffer has exactly the size the header
// asks for, so a byte read or written outside one is the sanitizer's to report.  Exit status 3 with the
// library's message on stderr when a call is refused.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "saihip_packed_ingest.h"

template <typename T>
static std::vector<T> list_of(const char* text) {
  std::vector<T> out;
  for (const char* p = text; *p;) {
    char* end = nullptr;
    out.push_back(static_cast<T>(strtol(p, &end, 10)));
    p = *end == ',' ? end + 1 : end;
    if (end == p && *p) break;
  }
  return out;
}

int main(int argc, char** argv) {
  if (argc != 11) {
    fprintf(stderr, "usage: bed_pack2_dump ROWS_FILE ROW_BYTES N_COLS PLOIDY FIRST_COL CUT N_THREADS RIB,... FLIP,... COL,...\n");
    return 2;
  }
  const int64_t row_bytes = atoll(argv[2]);
  const int32_t n_cols = atoi(argv[3]), ploidy = atoi(argv[4]), first_col = atoi(argv[5]), n_threads = atoi(argv[7]);
  const int64_t cut = atoll(argv[6]);
  const std::vector<int32_t> rib = list_of<int32_t>(argv[8]), cols = list_of<int32_t>(argv[10]);
  const std::vector<uint8_t> flip = list_of<uint8_t>(argv[9]);
  if (rib.size() != flip.size() || row_bytes < 1) return 2;
  std::vector<uint8_t> rows;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 4;
  for (int c; (c = fgetc(f)) != EOF;) rows.push_back(static_cast<uint8_t>(c));
  fclose(f);
  const int64_t n_sites = static_cast<int64_t>(rib.size()), n_batch = static_cast<int64_t>(rows.size()) / row_bytes;
  const int32_t n_ind = static_cast<int32_t>(cols.size());
  const int64_t words = (n_sites + 63) / 64 * ((n_ind / 64) * 256 + ((n_ind % 64 + 15) / 16) * 64);
  std::vector<uint8_t> packed(static_cast<size_t>(words) * 4, 0xA5);
  std::vector<int32_t> status(rib.size(), -7), unfit(rib.size(), -7);
  const int64_t bounds[3] = {0, cut > 0 && cut < n_sites ? cut : n_sites, n_sites};
  for (int part = 0; part < 2; ++part) {
    const int64_t lo = bounds[part], hi = bounds[part + 1];
    if (hi == lo && part == 1) continue;
    if (sai_bed_pack2_host(rows.data(), n_batch, row_bytes, hi - lo, rib.data() + lo, flip.data() + lo, n_cols, n_ind,
                           first_col >= 0 ? nullptr : cols.data(), first_col, ploidy, packed.data(), n_sites, lo, status.data() + lo,
                           unfit.data() + lo, n_threads)) {
      fprintf(stderr, "%s\n", sai_last_error());
      return 3;
    }
  }
  for (size_t k = 0; k < status.size(); ++k) printf("%d ", status[k]);
  printf("\n");
  for (size_t k = 0; k < unfit.size(); ++k) printf("%d ", unfit[k]);
  printf("\n");
  for (uint8_t b : packed) printf("%02x", b);
  printf("\n");
  return 0;
}
