// The host side of the BCF route that finds the records on the GPU, run end to end without a GPU: the feed hands
// the members over, zlib stands in for sai_inflate_bgzf, and the host twins of the two kernels, the stitch and the
// selection do the rest, batch by batch with the carry in front -- the loop of sai_amd/utils/bcf.py.  Built with
// the host units of libsaihip, once plain and once under ASan + UBSan (tests/test_bcf_walk_cpu.py).
//
//   bcf_walk_dump FILE CHROM START END ANC|- SEG_BYTES MAX_HEADS TEXT_BATCH WHOLE_FILE [SAMPLE ...]
//
// Prints a line per batch (segments, heads, records, carry), a line per selected row (pos flip width L and the
// FNV-1a hash of its GT array) and the counts; "host-route WHY" and exit status 4 where the route hands the read
// over.  Exit status 3: an error of the library, its sentence on stderr; 6: the feed wrote behind the buffer it was given.

#include <zlib.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "saihip_bcf_device.h"

static int fail_with_error() {
  fprintf(stderr, "%s\n", sai_last_error());
  return 3;
}

// The two buffers the feed fills, with guard bytes behind the comp_cap bytes it is told of: the sanitizers do not see
// what fread writes, so the program looks itself.
static const int64_t comp_cap = 65536 * 2 + 64;
static const size_t guard_bytes = 64;
static std::vector<unsigned char> comp[2] = {std::vector<unsigned char>(comp_cap + guard_bytes, 0xA5), std::vector<unsigned char>(comp_cap + guard_bytes, 0xA5)};

static bool guards_intact() {
  for (const auto& buf : comp)
    for (size_t i = 0; i < guard_bytes; ++i)
      if (buf[static_cast<size_t>(comp_cap) + i] != 0xA5) return false;
  return true;
}

static int host_route(const char* why, sai_bcf_feed* feed) {
  printf("host-route %s\n", why);
  sai_bcf_feed_close(feed);
  return guards_intact() ? 4 : 6;
}

int main(int argc, char** argv) {
  if (argc < 10) return 2;
  const char* path = argv[1];
  const char* chrom = argv[2];
  const int64_t start = atoll(argv[3]), end = atoll(argv[4]);
  const char* anc = strcmp(argv[5], "-") ? argv[5] : nullptr;
  const int32_t seg_bytes = atoi(argv[6]), max_heads = atoi(argv[7]);
  const int64_t text_batch = atoll(argv[8]);
  const int32_t whole_file = atoi(argv[9]);
  std::vector<const char*> names(argv + 10, argv + argc);
  sai_bcf_feed* feed = nullptr;
  int rc = sai_bcf_feed_open(path, chrom, start, end, static_cast<int32_t>(names.size()), names.data(), anc, comp[0].data(), comp[1].data(), comp_cap,
                             text_batch, whole_file, &feed);
  if (rc == SAI_BCF_HOST_ROUTE) { printf("host-route open\n"); return 4; }
  if (rc) return fail_with_error();
  int32_t n_contigs = 0, n_file_samples = 0;
  int64_t gt_key = 0;
  if (sai_bcf_feed_selection(feed, nullptr, 0, nullptr, 0, &n_contigs, &n_file_samples, &gt_key, nullptr, nullptr, nullptr, nullptr, nullptr)) return fail_with_error();
  std::vector<uint8_t> contig_defined(static_cast<size_t>(n_contigs) + 1);
  std::vector<int32_t> cols(names.size() + 1);
  if (sai_bcf_feed_selection(feed, cols.data(), static_cast<int32_t>(names.size()), contig_defined.data(), n_contigs, nullptr, nullptr, nullptr, nullptr, nullptr,
                             nullptr, nullptr, nullptr))
    return fail_with_error();
  printf("header contigs %d samples %d gt_key %lld cols", n_contigs, n_file_samples, static_cast<long long>(gt_key));
  for (size_t s = 0; s < names.size(); ++s) printf(" %d", cols[s]);
  printf("\n");
  std::vector<uint8_t> text, carry;
  bool stopped = false;
  for (int batch = 0; !stopped; ++batch) {
    int32_t b = 0, n_members = 0, done = 0;
    int64_t n_comp = 0, n_text = 0, e0 = 0;
    const sai_bgzf_member* members = nullptr;
    if (sai_bcf_feed_next(feed, &b, &n_comp, &n_members, &members, &n_text, &e0, &done)) return host_route("reader", feed);
    if (done) break;
    text = carry;
    text.resize(carry.size() + static_cast<size_t>(n_text) + 1);  // + 1: never an empty vector
    for (int32_t m = 0; m < n_members; ++m) {
      if (members[m].isize == 0) continue;
      z_stream zs;
      memset(&zs, 0, sizeof(zs));
      if (inflateInit2(&zs, -15) != Z_OK) return 2;
      zs.next_in = comp[b].data() + members[m].data_off;
      zs.avail_in = members[m].data_len;
      zs.next_out = text.data() + carry.size() + members[m].out_off;
      zs.avail_out = members[m].isize;
      const int zrc = inflate(&zs, Z_FINISH);
      const bool ok = zrc == Z_STREAM_END && zs.total_out == members[m].isize &&
                      crc32(crc32(0L, Z_NULL, 0), text.data() + carry.size() + members[m].out_off, members[m].isize) == members[m].crc;
      inflateEnd(&zs);
      if (!ok) return host_route("member", feed);
    }
    sai_bcf_feed_release(feed);
    const int64_t n_bytes = static_cast<int64_t>(carry.size()) + n_text;
    const int64_t entry = carry.empty() ? e0 : 0;
    const int64_t n_seg = (n_bytes + seg_bytes - 1) / seg_bytes;
    std::vector<sai_bcf_chain> chains(static_cast<size_t>(n_seg * max_heads) + 1);
    std::vector<int32_t> seg_info(static_cast<size_t>(n_seg) + 1);
    std::vector<int64_t> seg_entry(static_cast<size_t>(n_seg) + 1), seg_first(static_cast<size_t>(n_seg) + 1);
    if (sai_bcf_chain_segments_host(text.data(), n_bytes, seg_bytes, max_heads, contig_defined.data(), n_contigs, n_file_samples, chains.data(), seg_info.data()))
      return fail_with_error();
    int64_t n_records = 0, carry_from = 0, total_heads = 0;
    int32_t verdict = 0;
    if (sai_bcf_stitch(chains.data(), seg_info.data(), n_bytes, seg_bytes, max_heads, entry, seg_entry.data(), seg_first.data(), &n_records, &carry_from, &verdict))
      return fail_with_error();
    for (int64_t s = 0; s < n_seg; ++s) total_heads += seg_info[static_cast<size_t>(s)] & 0xFFFF;
    printf("batch %d bytes %lld segments %lld heads %lld records %lld carry_from %lld verdict %d\n", batch, static_cast<long long>(n_bytes),
           static_cast<long long>(n_seg), static_cast<long long>(total_heads), static_cast<long long>(n_records), static_cast<long long>(carry_from), verdict);
    if (verdict) return host_route("stitch", feed);
    std::vector<sai_bcf_record_head> heads(static_cast<size_t>(n_records) + 1);
    if (sai_bcf_record_heads_host(text.data(), n_bytes, seg_bytes, seg_entry.data(), seg_first.data(), carry_from, n_records, gt_key, !names.empty(), heads.data()))
      return fail_with_error();
    int64_t n_rows = 0;
    const int32_t* pos;
    const uint8_t* flip;
    const int64_t* off;
    const uint8_t* width;
    const int32_t* len;
    int32_t sel_done = 0;
    if (sai_bcf_feed_select(feed, heads.data(), n_records, &n_rows, &pos, &flip, &off, &width, &len, &sel_done, &verdict)) return fail_with_error();
    if (verdict) return host_route("select", feed);
    for (int64_t r = 0; r < n_rows; ++r) {
      uint64_t h = 1469598103934665603ull;
      const int64_t bytes = static_cast<int64_t>(n_file_samples) * len[r] * width[r];
      if (off[r] < 0 || off[r] + bytes > n_bytes) return 5;  // the selection names bytes outside the batch
      for (int64_t i = 0; i < bytes; ++i) h = (h ^ text[static_cast<size_t>(off[r] + i)]) * 1099511628211ull;
      printf("%d %d %d %d %016llx\n", pos[r], flip[r], width[r], len[r], static_cast<unsigned long long>(h));
    }
    stopped = sel_done != 0;
    carry.assign(text.begin() + carry_from, text.begin() + n_bytes);
  }
  if (!stopped && !carry.empty()) return host_route("trailing-bytes", feed);
  int64_t n_matched = 0, n_anc = 0, n_total = 0, first = 0, last = 0;
  if (sai_bcf_feed_selection(feed, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, &n_matched, &n_anc, &n_total, &first, &last)) return fail_with_error();
  printf("counts %lld %lld records %lld first %lld last %lld\n", static_cast<long long>(n_matched), static_cast<long long>(n_anc),
         static_cast<long long>(n_total), static_cast<long long>(first), static_cast<long long>(last));
  sai_bcf_feed_close(feed);
  return guards_intact() ? 0 : 6;
}
