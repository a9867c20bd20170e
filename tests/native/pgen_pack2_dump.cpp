// The host decoder of .pgen records into the packed2 layout as a stand-alone program, for
// tests/test_pgen_pack2_cpu.py: the test compiles it with -fsanitize=address,undefined over the host units of
// libsaihip, hands it the bytes of a batch and a table of records in two files and compares what it prints with the
// numpy statement of the layout and with the library.
//
//   pgen_pack2_dump BYTES_FILE RECORDS_FILE SAMPLE_CT PLOIDY FIRST_COL CUT N_THREADS COL,...
//
// RECORDS_FILE holds one line per output row: the offset, length and vrtype of its record, the same of its base
// (or -1 -1 -1) and its flip flag.  The rows are decoded in two calls cut at CUT (one call when CUT is 0) and the
// status values, the unfit values and the block are printed as one line each, the block as hexadecimal digits.
// Every buffer has exactly the size the header asks for, so a byte read or written outside one is the sanitizer's
// to report.  Exit status 3 with the library's message on stderr when a call is refused.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "saihip_pgen_packed.h"

static std::vector<int32_t> list_of(const char* text) {
  std::vector<int32_t> out;
  for (const char* p = text; *p;) {
    char* end = nullptr;
    out.push_back(static_cast<int32_t>(strtol(p, &end, 10)));
    if (end == p) break;
    p = *end == ',' ? end + 1 : end;
  }
  return out;
}

int main(int argc, char** argv) {
  if (argc != 9) {
    fprintf(stderr, "usage: pgen_pack2_dump BYTES_FILE RECORDS_FILE SAMPLE_CT PLOIDY FIRST_COL CUT N_THREADS COL,...\n");
    return 2;
  }
  const int32_t sample_ct = atoi(argv[3]), ploidy = atoi(argv[4]), first_col = atoi(argv[5]), n_threads = atoi(argv[7]);
  const int64_t cut = atoll(argv[6]);
  const std::vector<int32_t> cols = list_of(argv[8]);
  std::vector<uint8_t> bytes;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 4;
  for (int c; (c = fgetc(f)) != EOF;) bytes.push_back(static_cast<uint8_t>(c));
  fclose(f);
  std::vector<int64_t> rec, base;
  std::vector<uint8_t> flip;
  f = fopen(argv[2], "r");
  if (!f) return 4;
  long long v[7];
  while (fscanf(f, "%lld %lld %lld %lld %lld %lld %lld", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6) == 7) {
    rec.insert(rec.end(), v, v + 3);
    base.insert(base.end(), v + 3, v + 6);
    flip.push_back(static_cast<uint8_t>(v[6]));
  }
  fclose(f);
  const int64_t n_sites = static_cast<int64_t>(flip.size());
  const int32_t n_ind = static_cast<int32_t>(cols.size());
  const int64_t words = (n_sites + 63) / 64 * ((n_ind / 64) * 256 + ((n_ind % 64 + 15) / 16) * 64);
  std::vector<uint8_t> packed(static_cast<size_t>(words) * 4, 0xA5);
  std::vector<int32_t> status(flip.size(), -7), unfit(flip.size(), -7);
  const int64_t bounds[3] = {0, cut > 0 && cut < n_sites ? cut : n_sites, n_sites};
  for (int part = 0; part < 2; ++part) {
    const int64_t lo = bounds[part], hi = bounds[part + 1];
    if (hi == lo && part == 1) continue;
    if (sai_pgen_pack2_host(bytes.data(), static_cast<int64_t>(bytes.size()), hi - lo, rec.data() + 3 * lo, base.data() + 3 * lo,
                            flip.data() + lo, sample_ct, n_ind, first_col >= 0 ? nullptr : cols.data(), first_col, ploidy, packed.data(),
                            n_sites, lo, status.data() + lo, unfit.data() + lo, n_threads)) {
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
