// BCF 2.x files (BGZF) on the host: the record walk with the row selection of parse_lines(), the chromosome scan,
// the stream that hands the selected rows' GT arrays to the caller's staging buffers, and the host statement of the
// dosage table (include/saihip_bcf.h; DESIGN_INGEST.md, "BCF files").  The inflated source, the typed values, the
// header with its dictionaries and the row selection are in bcf_format.hpp, shared with bcf_feed.cpp.
// Plain C++: part of libsaihip and of the sanitizer build of the host units.

#include "bcf_format.hpp"
#include "bcf_record.hpp"
#include "csi_index.hpp"

namespace {

// ---- the record walk --------------------------------------------------------------------------------------

struct WalkRow {
  int32_t pos;
  uint8_t flip;
  const unsigned char* gt;  // the GT array (n_sample * L values), nullptr when no sample is asked for
  int64_t gt_bytes;
  uint8_t width;
  int32_t L;
};

struct WalkResult {
  int64_t first = -1, last = -1, n_records_total = 0, n_matched = 0;
};

struct Walk {
  BgzfSource src;
  std::string path, chrom;
  int64_t start, stop;
  bool whole_file;  // go on counting records behind the run (the scan)
  bool want_gt;
  const AncMap* anc;
  BcfHeader header;
  std::vector<char> buf;
  size_t lo = 0, have = 0;
  size_t step = kInflateStep;  // inflated bytes asked of the source at a time
  bool eof = false;
  Walk(const char* p, const char* c, int64_t s, int64_t e, int n_threads, bool whole, bool gt, const AncMap* a)
      : src(p, n_threads), path(p), chrom(c), start(s), stop(e), whole_file(whole), want_gt(gt), anc(a) {}

  // at least `n` bytes from `lo` on; false at the end of the stream (rc says whether that was an error)
  bool need(size_t n, int* rc) {
    *rc = SAI_OK;
    while (have - lo < n && !eof) {
      if (lo) {
        memmove(buf.data(), buf.data() + lo, have - lo);
        have -= lo;
        lo = 0;
      }
      *rc = src.fill(buf, have, std::max(step, n - have), &eof);
      if (*rc) return false;
    }
    return have - lo >= n;
  }

  int read_header() {
    if (int rc = src.open()) return rc;
    lo = have = 0;
    eof = false;
    header = BcfHeader();
    int rc;
    if (!need(5, &rc)) return rc ? rc : sai_set_error(SAI_ERR_ARG, "%s: the stream ends inside the BCF magic", path.c_str());
    const unsigned char* m = reinterpret_cast<const unsigned char*>(buf.data());
    if (memcmp(m, "BCF", 3) != 0) return sai_set_error(SAI_ERR_ARG, "%s: not a BCF (the inflated stream does not start with BCF\\2\\2)", path.c_str());
    if (m[3] != 2 || m[4] != 2)
      return sai_set_error(SAI_ERR_UNSUPPORTED, "%s: BCF version %d.%d is not read: only BCF 2.2 (magic BCF\\2\\2) is", path.c_str(), m[3], m[4]);
    if (!need(9, &rc)) return rc ? rc : sai_set_error(SAI_ERR_ARG, "%s: the stream ends before the length of the header text", path.c_str());
    const size_t l_text = le32(reinterpret_cast<const unsigned char*>(buf.data()) + 5);
    if (!need(9 + l_text, &rc))
      return rc ? rc : sai_set_error(SAI_ERR_ARG, "%s: l_text of %zu bytes lies beyond the end of the stream", path.c_str(), l_text);
    if (int hrc = parse_bcf_header(buf.data() + 9, l_text, path.c_str(), header)) return hrc;
    lo = 9 + l_text;
    return SAI_OK;
  }

  // Behind read_header(): go on at the virtual offset `v` instead of at the first record, if a record of contig `tid`
  // can start there (include/saihip_bcf_index.h).  false: nothing of the stream is valid any more -- read_header() again.
  bool seek(uint64_t v, int32_t tid) {
    if (!src.seek(static_cast<int64_t>(v >> 16))) return false;
    lo = have = 0;
    eof = false;
    const size_t u = static_cast<size_t>(v & 0xFFFFu);
    int rc;
    if (!need(u + 32, &rc)) return false;
    const uint8_t* t = reinterpret_cast<const uint8_t*>(buf.data());
    const uint8_t* defined = reinterpret_cast<const uint8_t*>(header.contig_defined.data());
    if (!bcfrec::is_candidate(t, static_cast<int64_t>(have), static_cast<int64_t>(u), defined, static_cast<int32_t>(header.contig_defined.size()),
                              static_cast<int32_t>(header.samples.size())))
      return false;
    if (static_cast<int32_t>(bcfrec::le32_at(t, static_cast<int64_t>(u) + 8)) != tid) return false;
    lo = u;
    return true;
  }

  // on_row(row) -> 0 go on, > 0 enough, < 0 a status
  template <typename F>
  int run(WalkResult& res, F&& on_row) {
    RowSelect sel;
    sel.aim(header, chrom);
    sel.start = start;
    sel.stop = stop;
    sel.whole_file = whole_file;
    const int64_t n_hdr_samples = static_cast<int64_t>(header.samples.size());
    const char* pth = path.c_str();
    for (;;) {
      int rc;
      if (!need(8, &rc)) {
        if (rc) return rc;
        if (have - lo) return sai_set_error(SAI_ERR_ARG, "%s: the stream ends inside the lengths of record %lld", pth, static_cast<long long>(res.n_records_total + 1));
        return SAI_OK;
      }
      const unsigned char* r = reinterpret_cast<const unsigned char*>(buf.data() + lo);
      const uint64_t l_shared = le32(r), l_indiv = le32(r + 4);
      const long long recno = static_cast<long long>(res.n_records_total + 1);
      if (l_shared < 24) return sai_set_error(SAI_ERR_ARG, "%s: record %lld has l_shared = %llu, fewer than the 24 bytes of its fixed fields", pth, recno, static_cast<unsigned long long>(l_shared));
      const size_t total = static_cast<size_t>(8 + l_shared + l_indiv);
      if (!need(total, &rc)) return rc ? rc : sai_set_error(SAI_ERR_ARG, "%s: record %lld (%zu bytes) leaves the stream", pth, recno, total);
      r = reinterpret_cast<const unsigned char*>(buf.data() + lo);
      lo += total;
      ++res.n_records_total;
      const int32_t chrom_idx = static_cast<int32_t>(le32(r + 8));
      const int64_t pos = static_cast<int64_t>(static_cast<int32_t>(le32(r + 12))) + 1;  // 0-based in the file
      const uint32_t n_allele = le32(r + 24) >> 16;
      const uint32_t n_fmt = le32(r + 28) >> 24, n_sample = le32(r + 28) & 0xFFFFFFu;
      if (chrom_idx < 0 || static_cast<size_t>(chrom_idx) >= header.contig.size() || !header.contig_defined[static_cast<size_t>(chrom_idx)])
        return sai_set_error(SAI_ERR_ARG, "%s: record %lld has CHROM index %d, which no ##contig line of the header defines", pth, recno, chrom_idx);
      if (n_sample != n_hdr_samples)
        return sai_set_error(SAI_ERR_ARG, "%s: record %lld holds %u samples but the header names %lld", pth, recno, n_sample, static_cast<long long>(n_hdr_samples));
      const int what = sel.step(chrom_idx, pos);
      res.first = sel.first;
      res.last = sel.last;
      res.n_matched = sel.n_matched;
      if (what == RowSelect::kStop) return SAI_OK;
      if (what == RowSelect::kSkip) continue;
      WalkRow row{static_cast<int32_t>(pos), 0, nullptr, 0, 1, 0};
      if (anc && anc->active) {
        auto it = anc->allele.find(pos);
        if (it == anc->allele.end()) continue;
        Cursor c{r + 32, r + 8 + l_shared};
        const char* s;
        size_t n;
        bool ok = typed_string(c, &s, &n);  // ID
        const char* ref = "";
        const char* alt = ".";  // a record without an ALT is "." in VCF text
        size_t ref_len = 0, alt_len = 1;
        if (ok && n_allele >= 1) ok = typed_string(c, &ref, &ref_len);
        if (ok && n_allele >= 2) ok = typed_string(c, &alt, &alt_len);
        if (!ok) return sai_set_error(SAI_ERR_ARG, "%s: record %s:%lld: a typed value of the shared part leaves the record", pth, chrom.c_str(), static_cast<long long>(pos));
        const int decision = anc_decision(it->second, ref, ref_len, alt, alt_len);
        if (decision < 0) continue;
        row.flip = static_cast<uint8_t>(decision);
      }
      if (want_gt) {
        Cursor c{r + 8 + l_shared, r + total};
        bool found = false;
        for (uint32_t k = 0; k < n_fmt && !found; ++k) {
          int64_t key, count;
          int type;
          if (!typed_int(c, &key) || !typed_desc(c, &type, &count))
            return sai_set_error(SAI_ERR_ARG, "%s: record %s:%lld: a typed value of the individual part leaves the record", pth, chrom.c_str(), static_cast<long long>(pos));
          const int width = type_width(type);
          if (count > (int64_t(1) << 31) / std::max<int64_t>(1, static_cast<int64_t>(n_sample) * std::max(width, 1)))
            return sai_set_error(SAI_ERR_ARG, "%s: record %s:%lld: a FORMAT vector of %lld values per sample leaves the record", pth, chrom.c_str(), static_cast<long long>(pos), static_cast<long long>(count));
          const int64_t bytes = static_cast<int64_t>(n_sample) * count * width;
          if (key == header.gt_key) {
            if (type < 1 || type > 3)
              return sai_set_error(SAI_ERR_ARG, "%s: record %s:%lld: the GT vector has type %d, not an integer type", pth, chrom.c_str(), static_cast<long long>(pos), type);
            if (c.end - c.p < bytes)
              return sai_set_error(SAI_ERR_ARG, "%s: record %s:%lld: the GT array (%lld bytes) leaves the record", pth, chrom.c_str(), static_cast<long long>(pos), static_cast<long long>(bytes));
            row.gt = c.p;
            row.gt_bytes = bytes;
            row.width = static_cast<uint8_t>(width);
            row.L = static_cast<int32_t>(count);
            found = true;
          } else {
            if (c.end - c.p < bytes)
              return sai_set_error(SAI_ERR_ARG, "%s: record %s:%lld: a FORMAT vector leaves the record", pth, chrom.c_str(), static_cast<long long>(pos));
            c.p += bytes;
          }
        }
        if (!found) {
          if (header.gt_key < 0)
            return sai_set_error(SAI_ERR_ARG, "%s: the header declares no FORMAT field GT, but the genotypes of record %s:%lld are asked for", pth, chrom.c_str(), static_cast<long long>(pos));
          return sai_set_error(SAI_ERR_ARG, "%s: record %s:%lld has no GT field", pth, chrom.c_str(), static_cast<long long>(pos));
        }
      }
      const int orc = on_row(row);
      if (orc < 0) return orc;
      if (orc > 0) return SAI_OK;
    }
  }
};

// ---- the dosage table ------------------------------------------------------------------------------------

// the output byte of one slot; *st is raised
inline int8_t decode_slot(const unsigned char* sample, int width, int32_t L, int32_t ploidy, bool flip, int32_t* st) {
  int64_t d = 0, fd = 0;
  for (int32_t k = 0; k < ploidy; ++k) {
    int64_t a = -1;
    if (k < L) {
      const int64_t v = read_int(sample + static_cast<size_t>(k) * static_cast<size_t>(width), width);
      const int64_t type_min = width == 1 ? -128 : width == 2 ? -32768 : INT32_MIN;
      if (v >= 0) a = (v >> 1) - 1;
      else if (v != type_min && v != type_min + 1) { *st = std::max(*st, SAI_BCF_STATUS_BAD_VALUE); return 0; }
    }
    d += a;
    fd += a >= 1 ? a - 1 : 1 - a;
  }
  if (d > 127 || fd > 127 || d < -128) { *st = std::max(*st, SAI_BCF_STATUS_RANGE); return 0; }
  return static_cast<int8_t>(flip ? fd : d);
}

}  // namespace

struct sai_bcf_stream {
  std::string path, chrom, anc_path;
  int64_t start = -1, end = -1;
  int n_threads = 1;
  std::vector<std::string> names;
  std::vector<int32_t> ploidy;
  unsigned char* bufs[2] = {nullptr, nullptr};
  size_t cap = 0;
  // producer state
  AncMap anc;
  std::vector<int32_t> col_of_slot;
  int32_t n_file_samples = 0;
  bool header_seen = false;
  int64_t n_matched = 0, n_anc = 0;
  // the producer's phases, seconds: complete once the producer has finished (sai_bcf_stream_stats)
  double read_s = 0.0, inflate_s = 0.0, walk_s = 0.0, copy_s = 0.0, wait_s = 0.0;
  int64_t inflated_bytes = 0, staged_bytes = 0;
  // the seek (sai_bcf_stream_open_at, sai_bcf_stream_seek_stats)
  const csi::Index* index = nullptr;
  bool seeked = false;
  uint64_t seek_v = 0;
  int64_t file_bytes = 0, n_members = 0;
  struct Batch {
    std::vector<int32_t> pos, len;
    std::vector<uint8_t> flip, width;
    std::vector<int64_t> off;
    size_t bytes = 0;
    void clear() { pos.clear(); len.clear(); flip.clear(); width.clear(); off.clear(); bytes = 0; }
  };
  // hand-over: batch k lives in buffer k % 2
  std::mutex m;
  std::condition_variable cv;
  Batch batch[2];
  int state[2] = {0, 0};  // 0 free, 1 full, 2 held by the consumer
  int64_t produced = 0, consumed = 0;
  int held = -1;
  bool finished = false, cancel = false;
  int rc = 0;
  std::string err;
  std::thread producer;
};

namespace {

int bcf_stream_run(sai_bcf_stream* st) {
  const char* path = st->path.c_str();
  if (!st->anc_path.empty()) {
    if (int rc = load_anc(st->anc_path.c_str(), st->chrom, st->start, st->end, st->anc, &st->n_anc)) return rc;
  }
  const double t_begin = now_s();
  double copy_s = 0.0, wait_s = 0.0;
  int64_t staged = 0;
  const bool want_gt = !st->names.empty();
  Walk walk(path, st->chrom.c_str(), st->start, st->end, st->n_threads, false, want_gt, &st->anc);
  if (st->index) walk.step = 1;  // member by member: what lies behind the header may not be wanted
  if (int rc = walk.read_header()) return rc;
  walk.step = kInflateStep;
  if (st->index) {
    RowSelect aim;
    aim.aim(walk.header, st->chrom);
    uint64_t v = 0;
    if (aim.target >= 0 && st->index->refs.size() <= walk.header.contig.size() &&
        st->index->query(aim.target, st->start, st->end, &v) == SAI_BCF_INDEX_SEEK && static_cast<int64_t>(v >> 16) >= walk.src.next_member_off()) {
      if (walk.seek(v, aim.target)) {
        std::lock_guard<std::mutex> lk(st->m);
        st->seeked = true;
        st->seek_v = v;
      } else if (int rc = walk.read_header()) {  // from the start, as without an index
        return rc;
      }
    }
  }
  std::vector<int32_t> cols;
  if (int rc = resolve_samples(walk.header, path, st->names, cols)) return rc;
  {
    std::lock_guard<std::mutex> lk(st->m);
    st->col_of_slot = cols;
    st->n_file_samples = static_cast<int32_t>(walk.header.samples.size());
    st->header_seen = true;
  }
  int b = -1;  // the buffer being filled
  auto acquire = [&]() -> bool {
    const double t0 = now_s();
    std::unique_lock<std::mutex> lk(st->m);
    b = static_cast<int>(st->produced % 2);
    st->cv.wait(lk, [&] { return st->state[b] == 0 || st->cancel; });
    wait_s += now_s() - t0;
    if (st->cancel) return false;
    st->batch[b].clear();
    return true;
  };
  // the phases so far: inflate and file read from the source, copy and wait from here, the walk is the rest
  auto account = [&]() {
    std::lock_guard<std::mutex> lk(st->m);
    st->read_s = walk.src.read_s;
    st->inflate_s = walk.src.inflate_s;
    st->copy_s = copy_s;
    st->wait_s = wait_s;
    st->walk_s = std::max(0.0, now_s() - t_begin - walk.src.read_s - walk.src.inflate_s - copy_s - wait_s);
    st->inflated_bytes = walk.src.inflated_bytes;
    st->staged_bytes = staged;
    st->file_bytes = walk.src.file_bytes;
    st->n_members = walk.src.n_members;
  };
  auto publish = [&](int64_t matched) {
    {
      std::lock_guard<std::mutex> lk(st->m);
      st->n_matched = matched;
      st->state[b] = 1;
      ++st->produced;
    }
    st->cv.notify_all();
    b = -1;
  };
  WalkResult res;
  const int rc = walk.run(res, [&](const WalkRow& row) -> int {
    const size_t bytes = static_cast<size_t>(row.gt_bytes);
    if (bytes > st->cap)
      return sai_set_error(SAI_ERR_UNSUPPORTED, "%s: the staging buffer of %zu bytes is smaller than the GT array of record %s:%d (%zu bytes): raise SAI_AMD_INGEST_BUFFER",
                           path, st->cap, st->chrom.c_str(), row.pos, bytes);
    if (b >= 0) {
      const size_t at = (st->batch[b].bytes + SAI_BCF_GT_ALIGN - 1) / SAI_BCF_GT_ALIGN * SAI_BCF_GT_ALIGN;
      if (at + bytes > st->cap) publish(res.n_matched - 1);
    }
    if (b < 0 && !acquire()) return 1;
    sai_bcf_stream::Batch& bt = st->batch[b];
    const size_t at = (bt.bytes + SAI_BCF_GT_ALIGN - 1) / SAI_BCF_GT_ALIGN * SAI_BCF_GT_ALIGN;
    if (bytes) {
      const double t0 = now_s();
      memset(st->bufs[b] + bt.bytes, 0, at - bt.bytes);
      memcpy(st->bufs[b] + at, row.gt, bytes);
      copy_s += now_s() - t0;
      staged += static_cast<int64_t>(bytes);
    }
    bt.pos.push_back(row.pos);
    bt.flip.push_back(row.flip);
    bt.off.push_back(static_cast<int64_t>(bytes ? at : bt.bytes));
    bt.width.push_back(row.width);
    bt.len.push_back(row.L);
    if (bytes) bt.bytes = at + bytes;
    return 0;
  });
  account();
  if (rc) return rc;
  if (b >= 0) publish(res.n_matched);
  std::lock_guard<std::mutex> lk(st->m);
  st->n_matched = res.n_matched;
  return SAI_OK;
}

void bcf_stream_producer(sai_bcf_stream* st) {
  int rc;
  std::string err;
  try {
    rc = bcf_stream_run(st);
    if (rc) err = sai_last_error();  // the producer thread's own message
  } catch (const std::bad_alloc&) {
    rc = SAI_ERR_HIP;
    err = "sai_bcf_stream: out of host memory";
  } catch (const std::exception& e) {
    rc = SAI_ERR_HIP;
    err = std::string("sai_bcf_stream: ") + e.what();
  } catch (...) {
    rc = SAI_ERR_HIP;
    err = "sai_bcf_stream: unknown failure";
  }
  {
    std::lock_guard<std::mutex> lk(st->m);
    st->rc = rc;
    st->err = err;
    st->finished = true;
  }
  st->cv.notify_all();
}

}  // namespace

extern "C" {

int sai_bcf_abi_version(void) { return SAI_BCF_ABI_VERSION; }

int sai_bcf_probe(const char* path) {
  if (!path) return 0;
  const int yes = guarded("sai_bcf_probe", [&]() -> int {
    FILE* f = fopen(path, "rb");
    if (!f) return 0;
    std::vector<unsigned char> head(size_t(1) << 16);
    const size_t n = fread(head.data(), 1, head.size(), f);
    fclose(f);
    size_t hlen = 0;
    const long bsize = bgzf_member_size(head.data(), n, &hlen);
    if (bsize <= 0 || static_cast<size_t>(bsize) > n || static_cast<size_t>(bsize) < hlen + 8) return 0;
    const unsigned char* tail = head.data() + bsize - 8;
    const uint32_t isize = le32(tail + 4);
    if (isize < 3 || isize > 65536u) return 0;
    std::vector<char> text(isize);
    const BgzfMember mem{hlen, static_cast<uint32_t>(static_cast<size_t>(bsize) - hlen - 8), isize, le32(tail), 0};
    Inflater inf;
    if (!inflate_member(head.data(), mem, text.data(), inf)) return 0;
    return memcmp(text.data(), "BCF", 3) == 0 ? 1 : 0;
  });
  return yes == 1 ? 1 : 0;
}

int sai_bcf_scan(const char* path, const char* chrom, int64_t* first_pos, int64_t* last_pos, int64_t* n_records_total, int64_t* n_samples) {
  return guarded("sai_bcf_scan", [&]() -> int {
    if (!path || !chrom) return sai_set_error(SAI_ERR_ARG, "NULL argument");
    Walk walk(path, chrom, -1, -1, kScanThreads, true, false, nullptr);
    if (int rc = walk.read_header()) return rc;
    WalkResult res;
    if (int rc = walk.run(res, [](const WalkRow&) { return 0; })) return rc;
    if (first_pos) *first_pos = res.first;
    if (last_pos) *last_pos = res.last;
    if (n_records_total) *n_records_total = res.n_records_total;
    if (n_samples) *n_samples = static_cast<int64_t>(walk.header.samples.size());
    return SAI_OK;
  });
}

int sai_bcf_stream_open(const char* path, const char* chrom, int64_t start, int64_t end, int32_t n_samples,
                        const char* const* sample_names, const int32_t* ploidy, const char* anc_bed_path, int32_t n_threads,
                        void* buffer0_host, void* buffer1_host, int64_t buffer_bytes, sai_bcf_stream** stream_out) {
  return sai_bcf_stream_open_at(path, chrom, start, end, n_samples, sample_names, ploidy, anc_bed_path, n_threads, buffer0_host, buffer1_host,
                                buffer_bytes, nullptr, stream_out);
}

int sai_bcf_stream_open_at(const char* path, const char* chrom, int64_t start, int64_t end, int32_t n_samples,
                           const char* const* sample_names, const int32_t* ploidy, const char* anc_bed_path, int32_t n_threads,
                           void* buffer0_host, void* buffer1_host, int64_t buffer_bytes, const sai_bcf_index* index,
                           sai_bcf_stream** stream_out) {
  return guarded("sai_bcf_stream_open", [&]() -> int {
    if (!path || !chrom || !stream_out) return sai_set_error(SAI_ERR_ARG, "NULL argument");
    *stream_out = nullptr;
    if (n_samples < 0 || (n_samples > 0 && (!sample_names || !ploidy))) return sai_set_error(SAI_ERR_ARG, "bad sample selection");
    if (!buffer0_host || !buffer1_host || buffer_bytes < 1) return sai_set_error(SAI_ERR_ARG, "two staging buffers are needed");
    for (int32_t s = 0; s < n_samples; ++s)
      if (ploidy[s] < 1 || ploidy[s] > 64)
        return sai_set_error(SAI_ERR_ARG, "%s: ploidy %d of sample %s is outside 1 .. 64", path, ploidy[s], sample_names[s]);
    std::unique_ptr<sai_bcf_stream> st(new sai_bcf_stream);
    st->path = path;
    st->chrom = chrom;
    st->start = start;
    st->end = end;
    st->n_threads = n_threads < 1 ? 1 : n_threads;
    if (anc_bed_path) st->anc_path = anc_bed_path;
    if (index && (start >= 0 || end >= 0)) st->index = &index->ix;
    for (int32_t s = 0; s < n_samples; ++s) {
      st->names.emplace_back(sample_names[s]);
      st->ploidy.push_back(ploidy[s]);
    }
    st->bufs[0] = static_cast<unsigned char*>(buffer0_host);
    st->bufs[1] = static_cast<unsigned char*>(buffer1_host);
    st->cap = static_cast<size_t>(buffer_bytes);
    st->producer = std::thread(bcf_stream_producer, st.get());
    *stream_out = st.release();
    return SAI_OK;
  });
}

int sai_bcf_stream_next(sai_bcf_stream* st, int32_t* buffer_index, int64_t* n_bytes, int64_t* n_rows, const int32_t** row_pos_host,
                        const uint8_t** row_flip_host, const int64_t** gt_off_host, const uint8_t** gt_width_host,
                        const int32_t** gt_len_host, int32_t* done) {
  if (!st || !buffer_index || !n_bytes || !n_rows || !row_pos_host || !row_flip_host || !gt_off_host || !gt_width_host || !gt_len_host || !done)
    return sai_set_error(SAI_ERR_ARG, "NULL argument");
  std::unique_lock<std::mutex> lk(st->m);
  if (st->held >= 0) {  // the caller is done with the batch it got last time
    st->state[st->held] = 0;
    st->held = -1;
    st->cv.notify_all();
  }
  const int b = static_cast<int>(st->consumed % 2);
  st->cv.wait(lk, [&] { return st->state[b] == 1 || st->finished; });
  if (st->state[b] != 1) {  // nothing more will come
    *done = 1;
    *n_rows = *n_bytes = 0;
    *buffer_index = -1;
    if (st->rc) return sai_set_error(st->rc, "%s", st->err.c_str());
    return SAI_OK;
  }
  const sai_bcf_stream::Batch& bt = st->batch[b];
  st->state[b] = 2;
  st->held = b;
  ++st->consumed;
  *done = 0;
  *buffer_index = b;
  *n_bytes = static_cast<int64_t>(bt.bytes);
  *n_rows = static_cast<int64_t>(bt.pos.size());
  *row_pos_host = bt.pos.data();
  *row_flip_host = bt.flip.data();
  *gt_off_host = bt.off.data();
  *gt_width_host = bt.width.data();
  *gt_len_host = bt.len.data();
  return SAI_OK;
}

int sai_bcf_stream_selection(sai_bcf_stream* st, int32_t* col_of_slot_host, int32_t capacity, int32_t* n_file_samples,
                             int64_t* n_matched, int64_t* n_anc_entries) {
  if (!st) return sai_set_error(SAI_ERR_ARG, "NULL argument");
  std::lock_guard<std::mutex> lk(st->m);
  if (!st->header_seen) return sai_set_error(SAI_ERR_ARG, "the header has not been read yet");
  if (col_of_slot_host) {
    if (static_cast<size_t>(capacity) < st->col_of_slot.size()) return sai_set_error(SAI_ERR_ARG, "col_of_slot capacity %d < %zu", capacity, st->col_of_slot.size());
    for (size_t s = 0; s < st->col_of_slot.size(); ++s) col_of_slot_host[s] = st->col_of_slot[s];
  }
  if (n_file_samples) *n_file_samples = st->n_file_samples;
  if (n_matched) *n_matched = st->n_matched;
  if (n_anc_entries) *n_anc_entries = st->n_anc;
  return SAI_OK;
}

int sai_bcf_stream_stats(sai_bcf_stream* st, double* file_read_s, double* inflate_s, double* walk_s, double* copy_s, double* wait_s,
                         int64_t* inflated_bytes, int64_t* staged_bytes) {
  if (!st) return sai_set_error(SAI_ERR_ARG, "NULL argument");
  std::lock_guard<std::mutex> lk(st->m);
  if (!st->finished) return sai_set_error(SAI_ERR_ARG, "the producer has not finished yet: read the stream to its end first");
  if (file_read_s) *file_read_s = st->read_s;
  if (inflate_s) *inflate_s = st->inflate_s;
  if (walk_s) *walk_s = st->walk_s;
  if (copy_s) *copy_s = st->copy_s;
  if (wait_s) *wait_s = st->wait_s;
  if (inflated_bytes) *inflated_bytes = st->inflated_bytes;
  if (staged_bytes) *staged_bytes = st->staged_bytes;
  return SAI_OK;
}

int sai_bcf_stream_seek_stats(sai_bcf_stream* st, int32_t* seeked, uint64_t* voffset, int64_t* file_bytes_read, int64_t* members_inflated) {
  if (!st) return sai_set_error(SAI_ERR_ARG, "NULL argument");
  std::lock_guard<std::mutex> lk(st->m);
  if (!st->finished) return sai_set_error(SAI_ERR_ARG, "the producer has not finished yet: read the stream to its end first");
  if (seeked) *seeked = st->seeked ? 1 : 0;
  if (voffset) *voffset = st->seek_v;
  if (file_bytes_read) *file_bytes_read = st->file_bytes;
  if (members_inflated) *members_inflated = st->n_members;
  return SAI_OK;
}

int sai_bcf_stream_close(sai_bcf_stream* st) {
  if (!st) return SAI_OK;
  {
    std::lock_guard<std::mutex> lk(st->m);
    st->cancel = true;
  }
  st->cv.notify_all();
  if (st->producer.joinable()) st->producer.join();
  delete st;
  return SAI_OK;
}

int sai_bcf_decode_host(const uint8_t* batch, int64_t batch_bytes, int64_t n_rows, const int64_t* gt_off, const uint8_t* gt_width,
                        const int32_t* gt_len, const uint8_t* row_flip, int32_t n_cols, int32_t n_slots, const int32_t* col_of_slot,
                        const int32_t* ploidy_of_slot, int8_t* out, int32_t* status, int32_t n_threads) {
  return guarded("sai_bcf_decode_host", [&]() -> int {
    if (batch_bytes < 0 || n_rows < 0 || n_cols < 0 || n_slots < 0) return sai_set_error(SAI_ERR_ARG, "size out of range");
    if (n_rows == 0) return SAI_OK;
    if (!gt_off || !gt_width || !gt_len || !row_flip || !status || (n_slots && (!col_of_slot || !ploidy_of_slot || !out)) || (batch_bytes && !batch))
      return sai_set_error(SAI_ERR_ARG, "NULL buffer");
    const int nt = static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(n_threads, n_rows / 64 + 1)));
    auto work = [&](int t) {
      for (int64_t r = n_rows * t / nt; r < n_rows * (t + 1) / nt; ++r) {
        int8_t* o = out + r * n_slots;
        int32_t st = 0;
        const int width = gt_width[r];
        const int64_t L = gt_len[r], off = gt_off[r];
        const bool row_ok = (width == 1 || width == 2 || width == 4) && L >= 0 && off >= 0 && off <= batch_bytes &&
                            (n_cols == 0 || L <= (batch_bytes - off) / width / n_cols);
        for (int32_t s = 0; s < n_slots; ++s) {
          const int32_t col = col_of_slot[s], pl = ploidy_of_slot[s];
          if (!row_ok || col < 0 || col >= n_cols || pl < 1 || pl > 64) {
            st = std::max(st, SAI_BCF_STATUS_BAD_INDEX);
            o[s] = 0;
            continue;
          }
          o[s] = decode_slot(batch + off + static_cast<int64_t>(col) * L * width, width, static_cast<int32_t>(L), pl, row_flip[r] != 0, &st);
        }
        status[r] = st;
      }
    };
    ThreadGroup tg;
    for (int t = 1; t < nt; ++t) tg.spawn([&work, t] { work(t); });
    work(0);
    tg.join();
    return SAI_OK;
  });
}

}  // extern "C"
