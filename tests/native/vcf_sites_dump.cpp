// The site scanner of a VCF as a stand-alone program, for tests/test_bed_export_cpu.py: the test compiles it with
// -fsanitize=address,undefined over the host units of libsaihip and compares what it prints with
// sai_amd/utils/vcf.py::read_site_columns and with the library.
//
//   vcf_sites_dump VCF CHROM START END N_THREADS        (START / END: -1 = open)
//
// prints "sites N_ROWS N_SAMPLES", the sample names on one line, one line "POS MULTI ID REF ALT" per row and the
// .bim text of the rows without a comma in ALT.  Every buffer has exactly the size sai_vcf_sites_info reports.
// Exit status 3 with the library's message on stderr when a call is refused.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../sai_amd/csrc/plink/bed_export.hpp"

static int refused() {
  fprintf(stderr, "%s\n", sai_last_error());
  return 3;
}

int main(int argc, char** argv) {
  if (argc != 6) {
    fprintf(stderr, "usage: vcf_sites_dump VCF CHROM START END N_THREADS\n");
    return 2;
  }
  sai_vcf_sites* sites = nullptr;
  if (sai_vcf_sites_open(argv[1], argv[2], atoll(argv[3]), atoll(argv[4]), atoi(argv[5]), &sites)) return refused();
  int64_t n_rows = 0, n_samples = 0, text_bytes = 0, names_bytes = 0;
  if (sai_vcf_sites_info(sites, &n_rows, &n_samples, &text_bytes, &names_bytes)) return refused();
  std::vector<int32_t> pos(static_cast<size_t>(n_rows));
  std::vector<uint8_t> multi(static_cast<size_t>(n_rows));
  std::vector<int64_t> text_off(static_cast<size_t>(3 * n_rows + 1)), name_off(static_cast<size_t>(n_samples + 1));
  std::vector<char> text(static_cast<size_t>(text_bytes)), names(static_cast<size_t>(names_bytes));
  if (sai_vcf_sites_copy(sites, pos.data(), multi.data(), text_off.data(), text.data(), name_off.data(), names.data())) return refused();
  printf("sites %lld %lld\n", static_cast<long long>(n_rows), static_cast<long long>(n_samples));
  for (int64_t i = 0; i < n_samples; ++i)
    printf("%s%.*s", i ? "\t" : "", static_cast<int>(name_off[i + 1] - name_off[i]), names.data() + name_off[i]);
  printf("\n");
  for (int64_t k = 0; k < n_rows; ++k) {
    printf("%d %d", pos[k], multi[k]);
    for (int c = 0; c < 3; ++c) printf(" %.*s", static_cast<int>(text_off[3 * k + c + 1] - text_off[3 * k + c]), text.data() + text_off[3 * k + c]);
    printf("\n");
  }
  int64_t n_bytes = 0;
  if (sai_vcf_sites_bim(sites, multi.data(), nullptr, 0, &n_bytes)) return refused();
  std::vector<char> bim(static_cast<size_t>(n_bytes));
  if (sai_vcf_sites_bim(sites, multi.data(), bim.data(), n_bytes, &n_bytes)) return refused();
  fwrite(bim.data(), 1, bim.size(), stdout);
  sai_vcf_sites_close(sites);
  return 0;
}
