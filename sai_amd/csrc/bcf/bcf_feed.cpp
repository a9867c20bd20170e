// The host side of the BCF route that inflates the members and finds the records on the GPU
// (include/saihip_bcf_device.h; DESIGN_INGEST.md, "BCF files: members inflated and records found on the GPU"): the
// plain C++ twins of the two kernels of bcf_walk.hip, the stitch over their summaries, and the feed -- the header read
// on the host, the file's members handed over as they are, and the row selection of the host walk (bcf_format.hpp)
// applied to the record heads the GPU sends back.  Plain C++: part of libsaihip and of the sanitizer build of the
// host units.

#include "bcf_format.hpp"
#include "bcf_record.hpp"
#include "csi_index.hpp"
#include "saihip_bcf_device.h"

static_assert(sizeof(sai_bcf_record_head) == 64, "a record head is 64 bytes");
static_assert(sizeof(sai_bcf_chain) == 16, "a chain summary is 16 bytes");

struct sai_bcf_feed {
  std::string path, chrom;
  bool want_gt = false;
  AncMap anc;
  int64_t n_anc = 0;
  BcfHeader header;
  std::vector<int32_t> cols;
  RowSelect sel;
  int64_t n_records_total = 0;
  // the tables of the last sai_bcf_feed_select
  std::vector<int32_t> pos, len;
  std::vector<uint8_t> flip, width;
  std::vector<int64_t> off;
  // the reader thread: batch k lives in buffer k % 2
  FILE* f = nullptr;
  unsigned char* bufs[2] = {nullptr, nullptr};
  size_t cap = 0, text_batch = 0;
  int64_t first_member_off = 0, first_e0 = 0;
  struct Batch {
    std::vector<sai_bgzf_member> members;
    size_t comp_bytes = 0, text_bytes = 0;
  };
  std::mutex m;
  std::condition_variable cv;
  Batch batch[2];
  int state[2] = {0, 0};  // 0 free, 1 full, 2 held by the consumer
  int64_t produced = 0, consumed = 0;
  int held = -1;
  bool finished = false, cancel = false;
  int rc = 0;
  std::string err;
  std::thread reader;
  double read_s = 0.0, header_s = 0.0, select_s = 0.0, wait_s = 0.0;
  int64_t comp_total = 0;
  // the seek (sai_bcf_feed_open_at, sai_bcf_feed_seek_stats)
  int64_t header_end_off = 0;  // the file offset behind the last member that holds a byte of the header
  bool seeked = false;
  uint64_t seek_v = 0;
  int64_t file_bytes = 0, n_members = 0;  // members read so far (the header's, inflated on the host, included)
  ~sai_bcf_feed() { if (f) fclose(f); }
};

namespace {

// Reads the members of the file from first_member_off on into the two buffers in turn.
int feed_read(sai_bcf_feed* fd) {
  const char* path = fd->path.c_str();
  if (fseeko(fd->f, static_cast<off_t>(fd->first_member_off), SEEK_SET) != 0) return sai_set_error(SAI_ERR_ARG, "seek failed in %s", path);
  bool eof = false;
  while (!eof) {
    int b;
    {
      const double t0 = now_s();
      std::unique_lock<std::mutex> lk(fd->m);
      b = static_cast<int>(fd->produced % 2);
      fd->cv.wait(lk, [&] { return fd->state[b] == 0 || fd->cancel; });
      fd->wait_s += now_s() - t0;
      if (fd->cancel) return SAI_OK;
    }
    sai_bcf_feed::Batch& bt = fd->batch[b];
    bt.members.clear();
    unsigned char* buf = fd->bufs[b];
    size_t at = 0, text = 0, raw = 0;  // raw: the members' bytes in the file, without the padding between them
    const double t0 = now_s();
    // a member is at most 64 KiB: one is started only where a whole one fits
    while (at + 65536 + 4 <= fd->cap) {
      const off_t member_at = ftello(fd->f);
      unsigned char* p = buf + at;
      size_t got = fread(p, 1, 12, fd->f);
      if (got == 0 && feof(fd->f)) { eof = true; break; }
      if (got < 12) return sai_set_error(SAI_ERR_ARG, "%s: truncated BGZF file", path);
      if (p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || !(p[3] & 4)) return sai_set_error(SAI_ERR_ARG, "%s: corrupt BGZF block", path);
      const size_t xlen = static_cast<size_t>(p[10]) | static_cast<size_t>(p[11]) << 8;
      // XLEN is file content: a whole member is at most 64 KiB, which is all the room the loop condition promises
      if (12 + xlen + 8 > 65536) return sai_set_error(SAI_ERR_ARG, "%s: corrupt BGZF block", path);
      if (fread(p + 12, 1, xlen, fd->f) != xlen) return sai_set_error(SAI_ERR_ARG, "%s: truncated BGZF file", path);
      size_t hlen = 0;
      const long bsize = bgzf_member_size(p, 12 + xlen, &hlen);
      if (bsize <= 0 || static_cast<size_t>(bsize) < hlen + 8) return sai_set_error(SAI_ERR_ARG, "%s: corrupt BGZF block", path);
      const size_t rest = static_cast<size_t>(bsize) - hlen;
      if (fread(p + hlen, 1, rest, fd->f) != rest) return sai_set_error(SAI_ERR_ARG, "%s: truncated BGZF file", path);
      const unsigned char* tail = p + bsize - 8;
      const uint32_t isize = le32(tail + 4);
      if (isize > 65536u) return sai_set_error(SAI_ERR_ARG, "%s: corrupt BGZF block (ISIZE > 64 KiB)", path);
      if (!bt.members.empty() && text + isize > fd->text_batch) {  // this one opens the next batch
        if (fseeko(fd->f, member_at, SEEK_SET) != 0) return sai_set_error(SAI_ERR_ARG, "seek failed in %s", path);
        break;
      }
      sai_bgzf_member mem;
      mem.data_off = static_cast<int64_t>(at + hlen);
      mem.out_off = static_cast<int64_t>(text);
      mem.data_len = static_cast<uint32_t>(rest - 8);
      mem.isize = isize;
      mem.crc = le32(tail);
      mem.reserved = 0;
      bt.members.push_back(mem);
      text += isize;
      at += static_cast<size_t>(bsize);
      raw += static_cast<size_t>(bsize);
      while (at & 3u) buf[at++] = 0;
    }
    bt.comp_bytes = at;
    bt.text_bytes = text;
    {
      std::lock_guard<std::mutex> lk(fd->m);
      fd->read_s += now_s() - t0;
      fd->comp_total += static_cast<int64_t>(at);
      fd->file_bytes += static_cast<int64_t>(raw);
      fd->n_members += static_cast<int64_t>(bt.members.size());
      if (!bt.members.empty()) {
        fd->state[b] = 1;
        ++fd->produced;
      }
    }
    fd->cv.notify_all();
  }
  return SAI_OK;
}

void feed_reader(sai_bcf_feed* fd) {
  int rc;
  std::string err;
  try {
    rc = feed_read(fd);
    if (rc) err = sai_last_error();
  } catch (const std::exception& e) {
    rc = SAI_ERR_HIP;
    err = std::string("sai_bcf_feed: ") + e.what();
  } catch (...) {
    rc = SAI_ERR_HIP;
    err = "sai_bcf_feed: unknown failure";
  }
  {
    std::lock_guard<std::mutex> lk(fd->m);
    fd->rc = rc;
    fd->err = err;
    fd->finished = true;
  }
  fd->cv.notify_all();
}

// The header, inflated on the host member by member; where the records start in the file and in that member's text.
// false: whatever is wrong with the file, the host route says it.
bool feed_header(sai_bcf_feed* fd) {
  BgzfSource src(fd->path.c_str(), 1);
  if (src.open()) return false;
  std::vector<char> buf;
  size_t have = 0;
  bool eof = false;
  int64_t last_off = 0, last_text = 0;  // of the last call of fill: its first member in the file, its first byte in the stream
  auto need = [&](size_t n) {
    while (have < n && !eof) {
      last_off = static_cast<int64_t>(ftello(src.f)) - static_cast<int64_t>(src.chave);
      last_text = static_cast<int64_t>(have);
      if (src.fill(buf, have, 1, &eof)) return false;
    }
    return have >= n;
  };
  if (!need(9) || memcmp(buf.data(), "BCF\2\2", 5) != 0) return false;
  const size_t l_text = le32(reinterpret_cast<const unsigned char*>(buf.data()) + 5);
  if (!need(9 + l_text)) return false;
  if (parse_bcf_header(buf.data() + 9, l_text, fd->path.c_str(), fd->header)) return false;
  const int64_t data_off = static_cast<int64_t>(9 + l_text);
  if (data_off == static_cast<int64_t>(have)) {  // the records start with the next member
    fd->first_member_off = static_cast<int64_t>(ftello(src.f)) - static_cast<int64_t>(src.chave);
    fd->first_e0 = 0;
  } else {
    fd->first_member_off = last_off;
    fd->first_e0 = data_off - last_text;
  }
  fd->header_end_off = src.next_member_off();
  fd->file_bytes = src.file_bytes;
  fd->n_members = src.n_members;
  return true;
}

}  // namespace

extern "C" {

int sai_bcf_device_abi_version(void) { return SAI_BCF_DEVICE_ABI_VERSION; }

int sai_bcf_chain_segments_host(const uint8_t* text, int64_t n_bytes, int32_t seg_bytes, int32_t max_heads, const uint8_t* contig_defined,
                                int32_t n_contigs, int32_t n_sample, sai_bcf_chain* chains, int32_t* seg_info) {
  return guarded("sai_bcf_chain_segments_host", [&]() -> int {
    if (int rc = bcfrec::check_stream_args(text, n_bytes, seg_bytes, false)) return rc;
    if (max_heads < 1 || max_heads > SAI_BCF_MAX_HEADS_LIMIT) return sai_set_error(SAI_ERR_ARG, "max_heads must be in 1 .. %d", SAI_BCF_MAX_HEADS_LIMIT);
    if (n_contigs < 0 || n_sample < 0 || n_sample > 0xFFFFFF) return sai_set_error(SAI_ERR_ARG, "size out of range");
    if (n_bytes == 0) return SAI_OK;
    if (!chains || !seg_info || (n_contigs > 0 && !contig_defined)) return sai_set_error(SAI_ERR_ARG, "NULL buffer");
    const int64_t n_segments = (n_bytes + seg_bytes - 1) / seg_bytes;
    std::vector<char> cand(static_cast<size_t>(seg_bytes)), is_succ(static_cast<size_t>(seg_bytes));
    for (int64_t seg = 0; seg < n_segments; ++seg) {
      const int64_t seg_begin = seg * seg_bytes, seg_end = seg_begin + seg_bytes;
      std::fill(cand.begin(), cand.end(), 0);
      std::fill(is_succ.begin(), is_succ.end(), 0);
      for (int64_t o = seg_begin; o < seg_end && o + 32 <= n_bytes; ++o) {
        if (!bcfrec::is_candidate(text, n_bytes, o, contig_defined, n_contigs, n_sample)) continue;
        cand[static_cast<size_t>(o - seg_begin)] = 1;
        const int64_t succ = bcfrec::successor(text, o);
        if (succ < seg_end) is_succ[static_cast<size_t>(succ - seg_begin)] = 1;
      }
      sai_bcf_chain* row = chains + seg * max_heads;
      memset(row, 0, sizeof(sai_bcf_chain) * static_cast<size_t>(max_heads));
      int32_t n_heads = 0;
      bool dense = false;
      for (int32_t rel = 0; rel < seg_bytes; ++rel) {
        if (!cand[static_cast<size_t>(rel)] || is_succ[static_cast<size_t>(rel)]) continue;
        if (n_heads == max_heads) { dense = true; break; }
        sai_bcf_chain& c = row[n_heads++];
        int64_t p = seg_begin + rel;
        c.head = static_cast<uint32_t>(p);
        c.flags = SAI_BCF_CHAIN_BROKEN;
        const int max_hops = seg_bytes / 32 + 1;  // a hop is at least 32 bytes
        for (int hop = 0; hop < max_hops; ++hop) {
          const int64_t next = bcfrec::successor(text, p);
          if (next > n_bytes) { c.flags = SAI_BCF_CHAIN_INCOMPLETE; break; }
          ++c.n_records;
          p = next;
          if (p >= seg_end) { c.flags = 0; break; }
          if (p + 32 > n_bytes) { c.flags = SAI_BCF_CHAIN_INCOMPLETE; break; }
          if (!cand[static_cast<size_t>(p - seg_begin)]) break;  // broken
        }
        c.chain_exit = static_cast<uint32_t>(p);
      }
      seg_info[seg] = n_heads | (dense ? 1 << 30 : 0);
    }
    return SAI_OK;
  });
}

int sai_bcf_stitch(const sai_bcf_chain* chains, const int32_t* seg_info, int64_t n_bytes, int32_t seg_bytes, int32_t max_heads, int64_t e0,
                   int64_t* seg_entry, int64_t* seg_first_record, int64_t* n_records, int64_t* carry_from, int32_t* verdict) {
  return guarded("sai_bcf_stitch", [&]() -> int {
    if (int rc = bcfrec::check_stream_args(reinterpret_cast<const uint8_t*>(chains), n_bytes, seg_bytes, false)) return rc;
    if (max_heads < 1 || max_heads > SAI_BCF_MAX_HEADS_LIMIT || e0 < 0 || e0 > n_bytes) return sai_set_error(SAI_ERR_ARG, "size out of range");
    if (!n_records || !carry_from || !verdict || (n_bytes > 0 && (!seg_info || !seg_entry || !seg_first_record))) return sai_set_error(SAI_ERR_ARG, "NULL argument");
    const int64_t n_segments = (n_bytes + seg_bytes - 1) / seg_bytes;
    for (int64_t s = 0; s < n_segments; ++s) { seg_entry[s] = -1; seg_first_record[s] = 0; }
    *n_records = 0;
    *verdict = 0;
    int64_t e = e0;
    for (;;) {
      *carry_from = e;
      if (e + 32 > n_bytes) break;  // nothing, or the start of a record whose rest comes with the next batch
      const int64_t seg = e / seg_bytes;
      const sai_bcf_chain* row = chains + seg * max_heads;
      const int32_t n_heads = seg_info[seg] & 0xFFFF;
      const bool dense = (seg_info[seg] >> 30 & 1) != 0;  // heads are missing from the row: what it holds proves nothing
      const sai_bcf_chain* c = nullptr;
      for (int32_t k = 0; k < n_heads && k < max_heads && !c && !dense; ++k)
        if (row[k].head == static_cast<uint32_t>(e)) c = row + k;
      // not a head (or one of those a dense segment has no room for), a broken chain; a summary the kernel never writes
      if (!c || (c->flags & SAI_BCF_CHAIN_BROKEN) || static_cast<int64_t>(c->chain_exit) > n_bytes || (c->flags == 0 && static_cast<int64_t>(c->chain_exit) <= e)) {
        *verdict = SAI_BCF_HOST_ROUTE;
        break;
      }
      seg_entry[seg] = e;
      seg_first_record[seg] = *n_records;
      *n_records += c->n_records;
      e = c->chain_exit;
      if (c->flags & SAI_BCF_CHAIN_INCOMPLETE) {
        *carry_from = e;
        break;
      }
    }
    return SAI_OK;
  });
}

int sai_bcf_record_heads_host(const uint8_t* text, int64_t n_bytes, int32_t seg_bytes, const int64_t* seg_entry, const int64_t* seg_first_record,
                              int64_t carry_from, int64_t n_records, int64_t gt_key, int32_t want_gt, sai_bcf_record_head* heads) {
  return guarded("sai_bcf_record_heads_host", [&]() -> int {
    if (int rc = bcfrec::check_stream_args(text, n_bytes, seg_bytes, false)) return rc;
    if (carry_from < 0 || carry_from > n_bytes || n_records < 0) return sai_set_error(SAI_ERR_ARG, "size out of range");
    if (n_bytes == 0 || n_records == 0) return SAI_OK;
    if (!seg_entry || !seg_first_record || !heads) return sai_set_error(SAI_ERR_ARG, "NULL buffer");
    const int64_t n_segments = (n_bytes + seg_bytes - 1) / seg_bytes;
    for (int64_t seg = 0; seg < n_segments; ++seg) {
      const int64_t seg_begin = seg * seg_bytes, seg_end = seg_begin + seg_bytes;
      int64_t p = seg_entry[seg];
      if (p < seg_begin || p >= seg_end) continue;
      const int max_records = seg_bytes / 32 + 1;  // a record is at least 32 bytes
      for (int n = 0; n < max_records && p < seg_end && p < carry_from && p + 32 <= n_bytes; ++n) {
        const int64_t next = bcfrec::successor(text, p);
        if (next > n_bytes || bcfrec::le32_at(text, p) < 24u) break;
        const int64_t r = seg_first_record[seg] + n;
        if (r >= 0 && r < n_records) bcfrec::fill_head(text, p, gt_key, want_gt != 0, heads + r);
        p = next;
      }
    }
    return SAI_OK;
  });
}

int sai_bcf_feed_open(const char* path, const char* chrom, int64_t start, int64_t end, int32_t n_samples, const char* const* sample_names,
                      const char* anc_bed_path, void* comp0_host, void* comp1_host, int64_t comp_buffer_bytes, int64_t text_batch_bytes,
                      int32_t whole_file, sai_bcf_feed** feed_out) {
  return sai_bcf_feed_open_at(path, chrom, start, end, n_samples, sample_names, anc_bed_path, comp0_host, comp1_host, comp_buffer_bytes, text_batch_bytes,
                              whole_file, nullptr, feed_out);
}

int sai_bcf_feed_open_at(const char* path, const char* chrom, int64_t start, int64_t end, int32_t n_samples, const char* const* sample_names,
                         const char* anc_bed_path, void* comp0_host, void* comp1_host, int64_t comp_buffer_bytes, int64_t text_batch_bytes,
                         int32_t whole_file, const sai_bcf_index* index, sai_bcf_feed** feed_out) {
  return guarded("sai_bcf_feed_open", [&]() -> int {
    if (!path || !chrom || !feed_out) return sai_set_error(SAI_ERR_ARG, "NULL argument");
    *feed_out = nullptr;
    if (n_samples < 0 || (n_samples > 0 && !sample_names)) return sai_set_error(SAI_ERR_ARG, "bad sample selection");
    if (!comp0_host || !comp1_host || comp_buffer_bytes < 65536 + 4) return sai_set_error(SAI_ERR_ARG, "two buffers of at least one member (65 540 bytes) are needed");
    if (text_batch_bytes < 1) return sai_set_error(SAI_ERR_ARG, "text_batch_bytes must be positive");
    std::unique_ptr<sai_bcf_feed> fd(new sai_bcf_feed);
    fd->path = path;
    fd->chrom = chrom;
    fd->want_gt = n_samples > 0;
    if (anc_bed_path) {
      if (load_anc(anc_bed_path, fd->chrom, start, end, fd->anc, &fd->n_anc)) return SAI_BCF_HOST_ROUTE;
      for (uint32_t n : fd->anc.allele.len)
        if (n > SAI_BCF_ALLELE_BYTES) return SAI_BCF_HOST_ROUTE;  // a head carries no more of REF and ALT
    }
    const double t0 = now_s();
    if (!feed_header(fd.get())) return SAI_BCF_HOST_ROUTE;
    fd->header_s = now_s() - t0;
    std::vector<std::string> names;
    for (int32_t s = 0; s < n_samples; ++s) names.emplace_back(sample_names[s]);
    if (resolve_samples(fd->header, path, names, fd->cols)) return SAI_BCF_HOST_ROUTE;
    fd->sel.aim(fd->header, fd->chrom);
    fd->sel.start = start;
    fd->sel.stop = end;
    fd->sel.whole_file = whole_file != 0;
    uint64_t v = 0;
    if (index && !whole_file && (start >= 0 || end >= 0) && fd->sel.target >= 0 && index->ix.refs.size() <= fd->header.contig.size() &&
        index->ix.query(fd->sel.target, start, end, &v) == SAI_BCF_INDEX_SEEK && static_cast<int64_t>(v >> 16) >= fd->header_end_off) {
      fd->first_member_off = static_cast<int64_t>(v >> 16);
      fd->first_e0 = static_cast<int64_t>(v & 0xFFFFu);
      fd->seeked = true;
      fd->seek_v = v;
    }
    fd->f = fopen(path, "rb");
    if (!fd->f) return SAI_BCF_HOST_ROUTE;
    fd->bufs[0] = static_cast<unsigned char*>(comp0_host);
    fd->bufs[1] = static_cast<unsigned char*>(comp1_host);
    fd->cap = static_cast<size_t>(comp_buffer_bytes);
    fd->text_batch = static_cast<size_t>(text_batch_bytes);
    fd->reader = std::thread(feed_reader, fd.get());
    *feed_out = fd.release();
    return SAI_OK;
  });
}

int sai_bcf_feed_release(sai_bcf_feed* fd) {
  if (!fd) return sai_set_error(SAI_ERR_ARG, "NULL argument");
  {
    std::lock_guard<std::mutex> lk(fd->m);
    if (fd->held >= 0) {
      fd->state[fd->held] = 0;
      fd->held = -1;
    }
  }
  fd->cv.notify_all();
  return SAI_OK;
}

int sai_bcf_feed_next(sai_bcf_feed* fd, int32_t* buffer_index, int64_t* n_comp_bytes, int32_t* n_members, const sai_bgzf_member** members_host,
                      int64_t* n_text_bytes, int64_t* e0, int32_t* done) {
  if (!fd || !buffer_index || !n_comp_bytes || !n_members || !members_host || !n_text_bytes || !e0 || !done) return sai_set_error(SAI_ERR_ARG, "NULL argument");
  sai_bcf_feed_release(fd);
  std::unique_lock<std::mutex> lk(fd->m);
  const int b = static_cast<int>(fd->consumed % 2);
  fd->cv.wait(lk, [&] { return fd->state[b] == 1 || fd->finished; });
  if (fd->state[b] != 1) {  // nothing more will come
    *done = 1;
    *buffer_index = -1;
    *n_comp_bytes = *n_text_bytes = *e0 = 0;
    *n_members = 0;
    *members_host = nullptr;
    if (fd->rc) return sai_set_error(fd->rc, "%s", fd->err.c_str());
    return SAI_OK;
  }
  const sai_bcf_feed::Batch& bt = fd->batch[b];
  fd->state[b] = 2;
  fd->held = b;
  *e0 = fd->consumed == 0 ? fd->first_e0 : 0;
  ++fd->consumed;
  *done = 0;
  *buffer_index = b;
  *n_comp_bytes = static_cast<int64_t>(bt.comp_bytes);
  *n_members = static_cast<int32_t>(bt.members.size());
  *members_host = bt.members.data();
  *n_text_bytes = static_cast<int64_t>(bt.text_bytes);
  return SAI_OK;
}

int sai_bcf_feed_select(sai_bcf_feed* fd, const sai_bcf_record_head* heads, int64_t n_heads, int64_t* n_rows, const int32_t** row_pos_host,
                        const uint8_t** row_flip_host, const int64_t** gt_off_host, const uint8_t** gt_width_host, const int32_t** gt_len_host,
                        int32_t* done, int32_t* verdict) {
  return guarded("sai_bcf_feed_select", [&]() -> int {
    if (!fd || !n_rows || !row_pos_host || !row_flip_host || !gt_off_host || !gt_width_host || !gt_len_host || !done || !verdict || n_heads < 0 ||
        (n_heads > 0 && !heads))
      return sai_set_error(SAI_ERR_ARG, "NULL argument");
    const double t0 = now_s();
    fd->pos.clear();
    fd->len.clear();
    fd->flip.clear();
    fd->width.clear();
    fd->off.clear();
    *done = 0;
    *verdict = 0;
    const int error_flags = SAI_BCF_HEAD_NO_GT | SAI_BCF_HEAD_GT_NOT_INT | SAI_BCF_HEAD_LEAVES;
    for (int64_t i = 0; i < n_heads && !*done && !*verdict; ++i) {
      const sai_bcf_record_head& h = heads[i];
      const int64_t pos = static_cast<int64_t>(h.pos0) + 1;  // 0-based in the file
      ++fd->n_records_total;
      const int what = fd->sel.step(h.chrom, pos);
      if (what == RowSelect::kStop) *done = 1;
      if (what != RowSelect::kRow) continue;
      uint8_t flip = 0;
      if (fd->anc.active) {
        const auto it = fd->anc.allele.find(pos);
        if (it == fd->anc.allele.end()) continue;
        if (h.flags & SAI_BCF_HEAD_SHARED_LEAVES) { *verdict = SAI_BCF_HOST_ROUTE; break; }
        // the table's alleles are at most SAI_BCF_ALLELE_BYTES long (sai_bcf_feed_open), so a longer REF or ALT,
        // whose length a head gives saturated, equals none of them -- as on the host
        const int decision = anc_decision(it->second, reinterpret_cast<const char*>(h.ref), h.ref_len, reinterpret_cast<const char*>(h.alt), h.alt_len);
        if (decision < 0) continue;
        flip = static_cast<uint8_t>(decision);
      }
      if (fd->want_gt && (h.flags & error_flags)) { *verdict = SAI_BCF_HOST_ROUTE; break; }
      fd->pos.push_back(static_cast<int32_t>(pos));
      fd->flip.push_back(flip);
      fd->off.push_back(fd->want_gt ? static_cast<int64_t>(h.gt_off) : 0);
      fd->width.push_back(fd->want_gt ? h.gt_width : 1);
      fd->len.push_back(fd->want_gt ? h.gt_len : 0);
    }
    *n_rows = static_cast<int64_t>(fd->pos.size());
    *row_pos_host = fd->pos.data();
    *row_flip_host = fd->flip.data();
    *gt_off_host = fd->off.data();
    *gt_width_host = fd->width.data();
    *gt_len_host = fd->len.data();
    fd->select_s += now_s() - t0;
    return SAI_OK;
  });
}

int sai_bcf_feed_selection(sai_bcf_feed* fd, int32_t* col_of_slot_host, int32_t capacity, uint8_t* contig_defined_host, int32_t capacity_contigs,
                           int32_t* n_contigs, int32_t* n_file_samples, int64_t* gt_key, int64_t* n_matched, int64_t* n_anc_entries,
                           int64_t* n_records_total, int64_t* first_pos, int64_t* last_pos) {
  if (!fd) return sai_set_error(SAI_ERR_ARG, "NULL argument");
  if (col_of_slot_host) {
    if (static_cast<size_t>(capacity) < fd->cols.size()) return sai_set_error(SAI_ERR_ARG, "col_of_slot capacity %d < %zu", capacity, fd->cols.size());
    for (size_t s = 0; s < fd->cols.size(); ++s) col_of_slot_host[s] = fd->cols[s];
  }
  if (contig_defined_host) {
    if (static_cast<size_t>(capacity_contigs) < fd->header.contig_defined.size()) return sai_set_error(SAI_ERR_ARG, "contig capacity %d < %zu", capacity_contigs, fd->header.contig_defined.size());
    for (size_t i = 0; i < fd->header.contig_defined.size(); ++i) contig_defined_host[i] = fd->header.contig_defined[i] ? 1 : 0;
  }
  if (n_contigs) *n_contigs = static_cast<int32_t>(fd->header.contig_defined.size());
  if (n_file_samples) *n_file_samples = static_cast<int32_t>(fd->header.samples.size());
  if (gt_key) *gt_key = fd->header.gt_key;
  if (n_matched) *n_matched = fd->sel.n_matched;
  if (n_anc_entries) *n_anc_entries = fd->n_anc;
  if (n_records_total) *n_records_total = fd->n_records_total;
  if (first_pos) *first_pos = fd->sel.first;
  if (last_pos) *last_pos = fd->sel.last;
  return SAI_OK;
}

int sai_bcf_feed_stats(sai_bcf_feed* fd, double* file_read_s, double* header_inflate_s, double* select_s, double* wait_s, int64_t* comp_bytes) {
  if (!fd) return sai_set_error(SAI_ERR_ARG, "NULL argument");
  std::lock_guard<std::mutex> lk(fd->m);
  if (file_read_s) *file_read_s = fd->read_s;
  if (header_inflate_s) *header_inflate_s = fd->header_s;
  if (select_s) *select_s = fd->select_s;
  if (wait_s) *wait_s = fd->wait_s;
  if (comp_bytes) *comp_bytes = fd->comp_total;
  return SAI_OK;
}

int sai_bcf_feed_seek_stats(sai_bcf_feed* fd, int32_t* seeked, uint64_t* voffset, int32_t* contig, int64_t* file_bytes_read, int64_t* members_read) {
  if (!fd) return sai_set_error(SAI_ERR_ARG, "NULL argument");
  std::lock_guard<std::mutex> lk(fd->m);
  if (seeked) *seeked = fd->seeked ? 1 : 0;
  if (voffset) *voffset = fd->seek_v;
  if (contig) *contig = fd->sel.target;
  if (file_bytes_read) *file_bytes_read = fd->file_bytes;
  if (members_read) *members_read = fd->n_members;
  return SAI_OK;
}

int sai_bcf_feed_close(sai_bcf_feed* fd) {
  if (!fd) return SAI_OK;
  {
    std::lock_guard<std::mutex> lk(fd->m);
    fd->cancel = true;
  }
  fd->cv.notify_all();
  if (fd->reader.joinable()) fd->reader.join();
  delete fd;
  return SAI_OK;
}

}  // extern "C"
