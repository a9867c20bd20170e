// The host twins of the DD table kernels as a stand-alone program, for tests/test_dd_table_cpu.py: the test compiles it
// with -fsanitize=address,undefined together with the host units of libsaihip (dd_table/dd_table_host.cpp among
// them), hands it blocks in files and compares what it prints with the numpy statement and with the library.
//
//   dd_table_dump table  N_SITES N_IND TILES_FILE VALUES
//   dd_table_dump window N_SITES N_SRC SRC_TILES_FILE VALUES REF_TABLE_FILE N_REF TGT_TABLE_FILE N_TGT WINDOWS_FILE
//
// VALUES = comma-separated int8 values.  `table` prints one line per value: the N_SITES entries as 8 hexadecimal
// digits each.  `window` (tables: uint32 [n_values][N_SITES]; windows: int32 pairs lo hi) prints the counter of
// unlisted bytes, then dd, then one line of d per window, doubles as 16 hexadecimal digits each.  Every buffer has
// exactly the size the entry points ask for (exit status 5 for a file of another size), so a byte read or written outside
// one is the sanitizer's to report.  Exit status 3 with the library's message on stderr when the call is refused.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "saihip.h"

// the two host twins, as sai_amd/csrc/dd_table/dd_table_host.cpp states them
extern "C" {
int sai_site_absdiff_table_host(int64_t n_sites, const sai_pop* pop, int32_t n_values, const int8_t* values, uint32_t* table);
int sai_window_dd_table_host(int64_t n_sites, const sai_pop* src, int32_t n_values, const int8_t* values, const uint32_t* table_ref,
                             int32_t n_ref_ind, const uint32_t* table_tgt, int32_t n_tgt_ind, int32_t n_windows, const int32_t* lo,
                             const int32_t* hi, double* scratch, double* dd, int32_t* n_unlisted);
}

static bool slurp(const char* path, std::vector<uint8_t>& out) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  for (int c; (c = fgetc(f)) != EOF;) out.push_back(static_cast<uint8_t>(c));
  fclose(f);
  return true;
}

static std::vector<int8_t> parse_values(const char* text) {
  std::vector<int8_t> out;
  for (const char* p = text; *p;) {
    char* rest = nullptr;
    out.push_back(static_cast<int8_t>(strtol(p, &rest, 10)));
    if (rest == p) break;
    p = *rest == ',' ? rest + 1 : rest;
  }
  return out;
}

static void print_doubles(const double* p, size_t n) {
  for (size_t i = 0; i < n; ++i) {
    uint64_t bits;
    memcpy(&bits, p + i, 8);
    printf("%016" PRIx64, bits);
  }
  printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 6) {
    fprintf(stderr, "usage: dd_table_dump table|window N_SITES N_IND TILES_FILE VALUES ...\n");
    return 2;
  }
  const std::string mode = argv[1];
  const int64_t n_sites = atoll(argv[2]);
  const int32_t n_ind = atoi(argv[3]);
  std::vector<uint8_t> tiles;
  if (!slurp(argv[4], tiles)) return 4;
  const int64_t want = n_sites > 0 && n_ind > 0 ? (n_sites + 63) / 64 * static_cast<int64_t>(n_ind) * 64 : 0;
  if (static_cast<int64_t>(tiles.size()) != want) return 5;
  const std::vector<int8_t> values = parse_values(argv[5]);
  const int32_t n_values = static_cast<int32_t>(values.size());
  sai_pop pop;
  memset(&pop, 0, sizeof(pop));
  pop.tiles = tiles.empty() ? nullptr : reinterpret_cast<const int8_t*>(tiles.data());
  pop.n_ind = n_ind;
  pop.ploidy = 1;
  const size_t sites = static_cast<size_t>(n_sites > 0 ? n_sites : 0);
  if (mode == "table") {
    std::vector<uint32_t> table(static_cast<size_t>(n_values) * sites, 0xDEADBEEFu);
    if (sai_site_absdiff_table_host(n_sites, &pop, n_values, values.data(), table.data())) {
      fprintf(stderr, "%s\n", sai_last_error());
      return 3;
    }
    for (int k = 0; k < n_values; ++k) {
      for (size_t s = 0; s < sites; ++s) printf("%08" PRIx32, table[static_cast<size_t>(k) * sites + s]);
      printf("\n");
    }
    return 0;
  }
  if (mode != "window" || argc != 11) return 2;
  std::vector<uint8_t> ref_bytes, tgt_bytes, win_bytes;
  if (!slurp(argv[6], ref_bytes) || !slurp(argv[8], tgt_bytes) || !slurp(argv[10], win_bytes)) return 4;
  if (ref_bytes.size() != static_cast<size_t>(n_values) * sites * 4 || tgt_bytes.size() != ref_bytes.size() || win_bytes.size() % 8) return 5;
  std::vector<uint32_t> table_ref(ref_bytes.size() / 4), table_tgt(tgt_bytes.size() / 4);
  memcpy(table_ref.data(), ref_bytes.data(), ref_bytes.size());
  memcpy(table_tgt.data(), tgt_bytes.data(), tgt_bytes.size());
  const int32_t n_windows = static_cast<int32_t>(win_bytes.size() / 8);
  std::vector<int32_t> lo(n_windows), hi(n_windows);
  for (int32_t w = 0; w < n_windows; ++w) {
    memcpy(&lo[w], win_bytes.data() + 8 * w, 4);
    memcpy(&hi[w], win_bytes.data() + 8 * w + 4, 4);
  }
  std::vector<double> scratch(static_cast<size_t>(n_windows) * static_cast<size_t>(n_ind > 0 ? n_ind : 0), -1.0), dd(n_windows, -1.0);
  int32_t n_unlisted = -1;
  if (sai_window_dd_table_host(n_sites, &pop, n_values, values.data(), table_ref.data(), atoi(argv[7]), table_tgt.data(), atoi(argv[9]), n_windows,
                               lo.data(), hi.data(), scratch.data(), dd.data(), &n_unlisted)) {
    fprintf(stderr, "%s\n", sai_last_error());
    return 3;
  }
  printf("%" PRId32 "\n", n_unlisted);
  print_doubles(dd.data(), dd.size());
  for (int32_t w = 0; w < n_windows; ++w) print_doubles(scratch.data() + static_cast<size_t>(w) * n_ind, n_ind);
  return 0;
}
