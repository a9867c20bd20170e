// The host encoder of .geno records, the header hash and the .snp pass as a stand-alone program, for
// tests/test_geno_export_cpu.py: the test compiles it with -fsanitize=address,undefined over the host units of
// libsaihip and compares what it prints with the library.
//
//   geno_export_dump encode DOSAGE_FILE N_ROWS N_SLOTS UNIFORM_PLOIDY N_THREADS TRANSPOSED SLOT0 N_OUT [PLOIDY,...]
//     prints the status values on one line, then the byte count and the FNV-1a digest (64 bits) of the records.  The
//     records get exactly the bytes the form asks for, so a byte written outside them is the sanitizer's to report.
//     The transposed form is encoded in two calls (the first half of the slots, then the rest) that share the status.
//   geno_export_dump text BIM_FILE
//     prints the hash of the file's first words, then the byte count, the digest and the hash of its .snp lines.
//
// Exit status 3 with the library's message on stderr when a call is refused.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../sai_amd/csrc/eigenstrat/geno_export.hpp"

static std::vector<char> read_file(const char* path, bool* ok) {
  std::vector<char> data;
  FILE* f = fopen(path, "rb");
  *ok = f != nullptr;
  if (!f) return data;
  for (int c; (c = fgetc(f)) != EOF;) data.push_back(static_cast<char>(c));
  fclose(f);
  return data;
}

static unsigned long long fnv1a(const uint8_t* p, size_t n) {
  uint64_t digest = 0xcbf29ce484222325ull;
  for (size_t i = 0; i < n; ++i) digest = (digest ^ p[i]) * 0x100000001b3ull;
  return digest;
}

static int refused() {
  fprintf(stderr, "%s\n", sai_last_error());
  return 3;
}

int main(int argc, char** argv) {
  bool ok = false;
  if (argc == 3 && !strcmp(argv[1], "text")) {
    const std::vector<char> bim = read_file(argv[2], &ok);
    if (!ok) return 4;
    uint32_t h_bim = 0, h_snp = 0;
    int64_t n = -1;
    if (sai_geno_hash_lines(bim.data(), static_cast<int64_t>(bim.size()), &h_bim)) return refused();
    if (sai_geno_snp_lines(bim.data(), static_cast<int64_t>(bim.size()), nullptr, 0, &n)) return refused();
    std::vector<char> snp(static_cast<size_t>(n));
    if (sai_geno_snp_lines(bim.data(), static_cast<int64_t>(bim.size()), snp.data(), n, &n)) return refused();
    if (sai_geno_hash_lines(snp.data(), n, &h_snp)) return refused();
    printf("%x %lld %016llx %x\n", h_bim, static_cast<long long>(n), fnv1a(reinterpret_cast<const uint8_t*>(snp.data()), snp.size()), h_snp);
    return 0;
  }
  if ((argc != 10 && argc != 11) || strcmp(argv[1], "encode")) {
    fprintf(stderr, "usage: geno_export_dump encode DOSAGE_FILE N_ROWS N_SLOTS UNIFORM_PLOIDY N_THREADS TRANSPOSED SLOT0 N_OUT [PLOIDY,...]\n"
                    "       geno_export_dump text BIM_FILE\n");
    return 2;
  }
  const int64_t n_rows = atoll(argv[3]);
  const int32_t n_slots = atoi(argv[4]), uniform = atoi(argv[5]), n_threads = atoi(argv[6]), transposed = atoi(argv[7]), slot0 = atoi(argv[8]),
                n_out = atoi(argv[9]);
  std::vector<int32_t> ploidy;
  if (argc == 11)
    for (const char* p = argv[10]; *p;) {
      char* end = nullptr;
      ploidy.push_back(static_cast<int32_t>(strtol(p, &end, 10)));
      if (end == p) break;
      p = *end == ',' ? end + 1 : end;
    }
  const std::vector<char> raw = read_file(argv[2], &ok);
  if (!ok) return 4;
  if (n_rows < 0 || n_slots < 1 || static_cast<int64_t>(raw.size()) != n_rows * n_slots) return 2;
  if (uniform == 0 && static_cast<int64_t>(ploidy.size()) != n_slots) return 2;
  const int8_t* dosage = reinterpret_cast<const int8_t*>(raw.data());
  const int32_t* pl = uniform ? nullptr : ploidy.data();
  std::vector<int32_t> status(static_cast<size_t>(n_rows), transposed ? 0 : -7);
  std::vector<uint8_t> records;
  if (!transposed) {
    records.assign(static_cast<size_t>(n_rows * geno_record_bytes(n_slots)), 0xA5);
    if (sai_geno_encode_host(dosage, n_rows, n_slots, pl, uniform, 0, slot0, n_out, records.data(), status.data(), n_threads)) return refused();
  } else {
    if (n_out < 0) return 2;
    const int64_t rlen = geno_record_bytes(n_rows);
    records.assign(static_cast<size_t>(n_out * rlen), 0xA5);
    const int32_t half = n_out / 2;
    if (sai_geno_encode_host(dosage, n_rows, n_slots, pl, uniform, 1, slot0, half, records.data(), status.data(), n_threads)) return refused();
    std::vector<uint8_t> rest(static_cast<size_t>((n_out - half) * rlen), 0xA5);  // a buffer of its own: its ends are the sanitizer's
    if (sai_geno_encode_host(dosage, n_rows, n_slots, pl, uniform, 1, slot0 + half, n_out - half, rest.data(), status.data(), n_threads)) return refused();
    memcpy(records.data() + half * rlen, rest.data(), rest.size());
  }
  for (int32_t s : status) printf("%d ", s);
  printf("\n%lld %016llx\n", static_cast<long long>(records.size()), fnv1a(records.data(), records.size()));
  return 0;
}
