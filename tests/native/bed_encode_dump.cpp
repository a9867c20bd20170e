// The host encoder of .bed rows as a stand-alone program, for tests/test_bed_export_cpu.py: the test compiles it with
// -fsanitize=address,undefined over the host units of libsaihip, hands it an int8 block in a file and compares what
// it prints with the numpy statement of the table and with the library.
//
//   bed_encode_dump DOSAGE_FILE N_ROWS N_SLOTS UNIFORM_PLOIDY N_THREADS [PLOIDY,...]
//
// prints the status values and the rows as hexadecimal digits, one line each.  Every buffer has exactly the size
// bed_export.hpp asks for, so a byte read or written outside one is the sanitizer's to report.  Exit status 3
// with the library's message on stderr when the call is refused.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../sai_amd/csrc/plink/bed_export.hpp"

int main(int argc, char** argv) {
  if (argc != 6 && argc != 7) {
    fprintf(stderr, "usage: bed_encode_dump DOSAGE_FILE N_ROWS N_SLOTS UNIFORM_PLOIDY N_THREADS [PLOIDY,...]\n");
    return 2;
  }
  const int64_t n_rows = atoll(argv[2]);
  const int32_t n_slots = atoi(argv[3]), uniform = atoi(argv[4]), n_threads = atoi(argv[5]);
  std::vector<int32_t> ploidy;
  if (argc == 7)
    for (const char* p = argv[6]; *p;) {
      char* end = nullptr;
      ploidy.push_back(static_cast<int32_t>(strtol(p, &end, 10)));
      if (end == p) break;
      p = *end == ',' ? end + 1 : end;
    }
  std::vector<int8_t> dosage;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 4;
  for (int c; (c = fgetc(f)) != EOF;) dosage.push_back(static_cast<int8_t>(static_cast<unsigned char>(c)));
  fclose(f);
  if (n_rows < 0 || n_slots < 1 || static_cast<int64_t>(dosage.size()) != n_rows * n_slots) return 2;
  if (uniform == 0 && static_cast<int64_t>(ploidy.size()) != n_slots) return 2;
  std::vector<uint8_t> rows(static_cast<size_t>(n_rows) * static_cast<size_t>((n_slots + 3) / 4), 0xA5);
  std::vector<int32_t> status(static_cast<size_t>(n_rows), -7);
  if (sai_bed_encode_host(dosage.data(), n_rows, n_slots, uniform ? nullptr : ploidy.data(), uniform, rows.data(), status.data(), n_threads)) {
    fprintf(stderr, "%s\n", sai_last_error());
    return 3;
  }
  for (int32_t s : status) printf("%d ", s);
  printf("\n");
  for (uint8_t b : rows) printf("%02x", b);
  printf("\n");
  return 0;
}
