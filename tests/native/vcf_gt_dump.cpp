// The host VCF reader as a stand-alone program, for tests/test_tokenize_cases_cpu.py: the test compiles it with
// -fsanitize=address,undefined over the host units of libsaihip and runs it on the files of the genotype rules
// table (tests/tokenize_cases.py), the lines with allele indices that would overflow an int among them.
//
//   vcf_gt_dump VCF CHROM N_THREADS ANC_BED|- NAME:PLOIDY [NAME:PLOIDY ...]
//
// prints "rows N_ROWS N_SAMPLES" and one line "POS d d d ..." per row.  Exit status 3 with the library's message on
// stderr when the load is refused.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "saihip.h"

static int refused() {
  fprintf(stderr, "%s\n", sai_last_error());
  return 3;
}

int main(int argc, char** argv) {
  if (argc < 6) {
    fprintf(stderr, "usage: vcf_gt_dump VCF CHROM N_THREADS ANC_BED|- NAME:PLOIDY [NAME:PLOIDY ...]\n");
    return 2;
  }
  std::vector<std::string> names;
  std::vector<int32_t> ploidy;
  for (int i = 5; i < argc; ++i) {
    const char* colon = strrchr(argv[i], ':');
    if (!colon) {
      fprintf(stderr, "sample without a ploidy: %s\n", argv[i]);
      return 2;
    }
    names.emplace_back(argv[i], static_cast<size_t>(colon - argv[i]));
    ploidy.push_back(atoi(colon + 1));
  }
  std::vector<const char*> name_ptrs;
  for (const std::string& n : names) name_ptrs.push_back(n.c_str());
  const char* anc = strcmp(argv[4], "-") == 0 ? nullptr : argv[4];
  const int32_t n_samples = static_cast<int32_t>(names.size());
  sai_vcf_block* blk = nullptr;
  if (sai_vcf_load(argv[1], argv[2], -1, -1, n_samples, name_ptrs.data(), ploidy.data(), anc, atoi(argv[3]), &blk)) return refused();
  int64_t n_rows = 0, n_matched = 0, n_anc = 0;
  if (sai_vcf_block_info(blk, &n_rows, &n_matched, &n_anc)) return refused();
  std::vector<int32_t> pos(static_cast<size_t>(n_rows));
  std::vector<int8_t> dos(static_cast<size_t>(n_rows) * static_cast<size_t>(n_samples));
  if (sai_vcf_block_copy(blk, pos.data(), dos.data())) return refused();
  printf("rows %lld %d\n", static_cast<long long>(n_rows), n_samples);
  for (int64_t r = 0; r < n_rows; ++r) {
    printf("%d", pos[static_cast<size_t>(r)]);
    for (int32_t s = 0; s < n_samples; ++s) printf(" %d", dos[static_cast<size_t>(r * n_samples + s)]);
    printf("\n");
  }
  sai_vcf_block_free(blk);
  return 0;
}
