// The LD-compressing host encoder of .pgen records as a stand-alone program, for tests/test_pgen_ld_cpu.py: the test
// compiles it with -fsanitize=address,undefined over the host units of libsaihip, hands it an int8 block in a file and
// compares what it prints with the library and the test writer.
//
//   pgen_ld_dump DOSAGE_FILE N_ROWS N_SLOTS UNIFORM_PLOIDY N_THREADS [PLOIDY,...]
//
// prints the status values, the record types and the record lengths, one line each, then the byte count and the
// FNV-1a digest (64 bits) of the records.  The first call has no room for records and learns their total; the second
// gets exactly that many bytes, and the block and the tables are exactly as long as the call says, so a byte read or
// written outside them -- a base row looked for before its segment, say -- is the sanitizer's to report.  Exit status 3
// with the library's message on stderr when the call is refused.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../sai_amd/csrc/pgen/pgen_export_ld.hpp"

int main(int argc, char** argv) {
  if (argc != 6 && argc != 7) {
    fprintf(stderr, "usage: pgen_ld_dump DOSAGE_FILE N_ROWS N_SLOTS UNIFORM_PLOIDY N_THREADS [PLOIDY,...]\n");
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
  dosage.shrink_to_fit();
  if (n_rows < 0 || n_slots < 1 || static_cast<int64_t>(dosage.size()) != n_rows * n_slots) return 2;
  if (uniform == 0 && static_cast<int64_t>(ploidy.size()) != n_slots) return 2;
  if (sai_pgen_export_ld_version() != SAI_PGEN_EXPORT_LD_VERSION || sai_pgen_ld_segment() != SAI_PGEN_LD_SEGMENT) return 5;
  std::vector<uint8_t> vrtype(static_cast<size_t>(n_rows), 0xA5);
  std::vector<uint32_t> length(static_cast<size_t>(n_rows), 0xA5A5A5A5u);
  std::vector<int32_t> status(static_cast<size_t>(n_rows), -7);
  const int32_t* pl = uniform ? nullptr : ploidy.data();
  int64_t total = -1;
  int rc = sai_pgen_encode_ld_host(dosage.data(), n_rows, n_slots, pl, uniform, nullptr, 0, vrtype.data(), length.data(), status.data(), &total, n_threads);
  if (rc && total < 0) {
    fprintf(stderr, "%s\n", sai_last_error());
    return 3;
  }
  std::vector<uint8_t> records(static_cast<size_t>(total));
  rc = sai_pgen_encode_ld_host(dosage.data(), n_rows, n_slots, pl, uniform, records.data(), total, vrtype.data(), length.data(), status.data(), &total, n_threads);
  if (rc) {
    fprintf(stderr, "%s\n", sai_last_error());
    return 3;
  }
  for (int32_t s : status) printf("%d ", s);
  printf("\n");
  for (uint8_t t : vrtype) printf("%u ", t);
  printf("\n");
  for (uint32_t l : length) printf("%u ", l);
  printf("\n");
  uint64_t digest = 0xcbf29ce484222325ull;
  for (uint8_t b : records) digest = (digest ^ b) * 0x100000001b3ull;
  printf("%lld %016llx\n", static_cast<long long>(total), static_cast<unsigned long long>(digest));
  return 0;
}
