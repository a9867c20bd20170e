// The host twin of the packed2 frequency kernel as a stand-alone program, for tests/test_packed_stats_cpu.py: the test
// compiles it with -fsanitize=address,undefined together with packed_stats/packed2_freqs_host.cpp, hands it packed2
// blocks in files and compares what it prints with the numpy statement and with the library.
//
//   packed_freqs_dump N_SITES N_THREADS N_IND:PLOIDY:BLOCK_FILE ...
//
// prints one line per population: the N_SITES doubles as 16 hexadecimal digits each.  Every buffer has exactly the
// size the header asks for (a block file must hold sai_packed2_bytes(N_SITES, N_IND) bytes: exit status 5 otherwise),
// so a byte read or written outside one is the sanitizer's to report.  Exit status 3 with the library's message on
// stderr when the call is refused.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "saihip_packed_stats.h"

int main(int argc, char** argv) {
  if (argc < 4) {
    fprintf(stderr, "usage: packed_freqs_dump N_SITES N_THREADS N_IND:PLOIDY:BLOCK_FILE ...\n");
    return 2;
  }
  const int64_t n_sites = atoll(argv[1]);
  const int32_t n_threads = atoi(argv[2]), n_pops = argc - 3;
  std::vector<std::vector<uint8_t>> blocks(n_pops);
  std::vector<sai_pop> pops(n_pops);
  for (int p = 0; p < n_pops; ++p) {
    char* rest = nullptr;
    pops[p].n_ind = static_cast<int32_t>(strtol(argv[3 + p], &rest, 10));
    if (*rest != ':') return 2;
    pops[p].ploidy = static_cast<int32_t>(strtol(rest + 1, &rest, 10));
    if (*rest != ':') return 2;
    FILE* f = fopen(rest + 1, "rb");
    if (!f) return 4;
    for (int c; (c = fgetc(f)) != EOF;) blocks[p].push_back(static_cast<uint8_t>(c));
    fclose(f);
    const int32_t n_ind = pops[p].n_ind;
    const int64_t words = (n_sites + 63) / 64 * (static_cast<int64_t>(n_ind / 64) * 256 + ((n_ind % 64 + 15) / 16) * 64);
    if (n_ind >= 1 && static_cast<int64_t>(blocks[p].size()) != words * 4) return 5;
    pops[p].tiles = reinterpret_cast<const int8_t*>(blocks[p].data());
  }
  std::vector<double> freqs(static_cast<size_t>(n_pops) * static_cast<size_t>(n_sites > 0 ? n_sites : 0), -1.0);
  if (sai_packed2_site_freqs_host(n_sites, n_pops, pops.data(), freqs.data(), n_threads)) {
    fprintf(stderr, "%s\n", sai_last_error());
    return 3;
  }
  for (int p = 0; p < n_pops; ++p) {
    for (int64_t s = 0; s < n_sites; ++s) {
      uint64_t bits;
      memcpy(&bits, &freqs[static_cast<size_t>(p) * n_sites + s], 8);
      printf("%016" PRIx64, bits);
    }
    printf("\n");
  }
  return 0;
}
