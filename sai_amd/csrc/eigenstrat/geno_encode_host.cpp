// sai_geno_encode_host: the plain statement of geno_export.hpp -- the int8 [row][slot] block of the readers -> the
// records of a packed or a transposed .geno, cell by cell from geno_code_of.  The yardstick of the two kernels
// (geno_encode.hip), which write the same bytes and the same status values, and the encoder of the
// SAI_AMD_INGEST=host route.  Beside it the two passes over text the fileset needs: the hash of the header record and
// the .snp lines.

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <exception>
#include <new>

#include "../host_threads.hpp"
#include "../plink/plink_codes.hpp"
#include "geno_export.hpp"

extern "C" int sai_set_error(int code, const char* fmt, ...);

namespace {

struct Call {
  const int8_t* dosage;
  int64_t n_rows;
  int32_t n_slots;
  const int32_t* ploidy_of_slot;
  int32_t uniform_ploidy;
};

// the code of (row, slot); *st is raised where the cell does not fit
inline uint32_t code_at(const Call& c, int64_t r, int64_t s, int32_t* st) {
  const int32_t pl = c.uniform_ploidy ? c.uniform_ploidy : c.ploidy_of_slot[s];
  bool fits = false;
  uint32_t code = 3u;
  if (pl == 1 || pl == 2) code = geno_code_of(c.dosage[r * c.n_slots + s], pl, &fits);
  else *st = kPlinkBadIndex;
  if (!fits) *st = std::max(*st, static_cast<int32_t>(c.n_slots - s));
  return code;
}

template <class F>
void over(int64_t n_items, int64_t cells, int32_t n_threads, F&& body) {
  // one thread for every 2^18 cells of work, as the host decoders
  const int nt = static_cast<int>(std::max<int64_t>(1, std::min<int64_t>({static_cast<int64_t>(std::max(n_threads, 1)), n_items, cells / (int64_t(1) << 18) + 1})));
  ThreadGroup tg;
  for (int t = 1; t < nt; ++t) tg.spawn([&body, t, nt, n_items] { body(n_items * t / nt, n_items * (t + 1) / nt); });
  body(0, n_items / nt);
  tg.join();
}

int geno_encode_host_impl(const int8_t* dosage, int64_t n_rows, int32_t n_slots, const int32_t* ploidy_of_slot, int32_t uniform_ploidy,
                          int32_t transposed, int32_t slot0, int32_t n_out, uint8_t* out, int32_t* status, int32_t n_threads) {
  if (n_rows < 0 || n_slots < 1) return sai_set_error(SAI_ERR_ARG, "size out of range");
  if (uniform_ploidy < 0 || uniform_ploidy > 2) return sai_set_error(SAI_ERR_ARG, "uniform_ploidy must be 0, 1 or 2");
  if (n_rows > (INT64_MAX - 16) / n_slots) return sai_set_error(SAI_ERR_ARG, "size out of range");
  if (slot0 < 0 || n_out < 0 || static_cast<int64_t>(slot0) + n_out > n_slots) return sai_set_error(SAI_ERR_ARG, "slot0 + n_out exceeds n_slots");
  if (!transposed && (slot0 != 0 || n_out != n_slots)) return sai_set_error(SAI_ERR_ARG, "the packed form takes every slot: slot0 = 0 and n_out = n_slots");
  if (n_rows == 0 && !transposed) return SAI_OK;
  if (transposed && n_out == 0) return SAI_OK;
  if ((n_rows > 0 && (!dosage || !status)) || !out || (uniform_ploidy == 0 && !ploidy_of_slot)) return sai_set_error(SAI_ERR_ARG, "NULL buffer");
  const Call c{dosage, n_rows, n_slots, ploidy_of_slot, uniform_ploidy};
  if (!transposed) {
    const int64_t rlen = geno_record_bytes(n_slots);
    over(n_rows, n_rows * n_slots, n_threads, [&](int64_t lo, int64_t hi) {
      for (int64_t r = lo; r < hi; ++r) {
        uint8_t* dst = out + r * rlen;
        std::memset(dst, 0, static_cast<size_t>(rlen));
        int32_t st = 0;
        for (int64_t s = 0; s < n_slots; ++s) dst[s >> 2] |= static_cast<uint8_t>(code_at(c, r, s, &st) << (6 - 2 * (s & 3)));
        status[r] = st;
      }
    });
    return SAI_OK;
  }
  // Transposed: a thread owns a range of row QUADS (the rows of whole output bytes), so no two threads touch one
  // byte or one status word.
  const int64_t rlen = geno_record_bytes(n_rows);
  const int64_t quads = (n_rows + 3) / 4;
  if (n_rows == 0) {
    std::memset(out, 0, static_cast<size_t>(rlen * n_out));
    return SAI_OK;
  }
  over(quads, n_rows * n_out, n_threads, [&](int64_t lo, int64_t hi) {
    for (int64_t i = 0; i < n_out; ++i) {
      uint8_t* rec = out + i * rlen;
      std::memset(rec + lo, 0, static_cast<size_t>(hi - lo));
      if (hi == quads) std::memset(rec + quads, 0, static_cast<size_t>(rlen - quads));  // the padding of a narrow record
    }
    for (int64_t r = 4 * lo; r < std::min(4 * hi, n_rows); ++r) {
      int32_t st = status[r];
      for (int64_t i = 0; i < n_out; ++i) out[i * rlen + (r >> 2)] |= static_cast<uint8_t>(code_at(c, r, slot0 + i, &st) << (6 - 2 * (r & 3)));
      status[r] = st;
    }
  });
  return SAI_OK;
}

}  // namespace

extern "C" {

int sai_geno_export_abi_version(void) { return SAI_GENO_EXPORT_ABI_VERSION; }

int sai_geno_encode_host(const int8_t* dosage, int64_t n_rows, int32_t n_slots, const int32_t* ploidy_of_slot, int32_t uniform_ploidy,
                         int32_t transposed, int32_t slot0, int32_t n_out, uint8_t* out, int32_t* status, int32_t n_threads) {
  try {
    return geno_encode_host_impl(dosage, n_rows, n_slots, ploidy_of_slot, uniform_ploidy, transposed, slot0, n_out, out, status, n_threads);
  } catch (const std::bad_alloc&) {
    return sai_set_error(SAI_ERR_HIP, "sai_geno_encode_host: out of host memory");
  } catch (const std::exception& e) {
    return sai_set_error(SAI_ERR_HIP, "sai_geno_encode_host: %s", e.what());
  }
}

int sai_geno_hash_lines(const char* text, int64_t n_bytes, uint32_t* hash) {
  if (n_bytes < 0 || !hash || (n_bytes > 0 && !text)) return sai_set_error(SAI_ERR_ARG, "NULL buffer or size out of range");
  uint32_t all = 0;
  for (int64_t k = 0; k < n_bytes;) {
    uint32_t h = 0;  // hashit of the line's first word
    int64_t e = k;
    for (; e < n_bytes && text[e] != '\n' && text[e] != ' ' && text[e] != '\t'; ++e) h = h * 23u + static_cast<unsigned char>(text[e]);
    all = (all * 17u) ^ h;  // hasharr
    for (; e < n_bytes && text[e] != '\n'; ++e) {
    }
    k = e + 1;
  }
  *hash = all;
  return SAI_OK;
}

int sai_geno_snp_lines(const char* bim, int64_t n_bytes, char* out, int64_t cap, int64_t* n_out) {
  if (n_bytes < 0 || cap < 0 || !n_out || (n_bytes > 0 && !bim)) return sai_set_error(SAI_ERR_ARG, "NULL buffer or size out of range");
  // every line grows by the two bytes of "0.0" against "0", and by CHROM:POS less the dot where the ID is "."
  for (int pass = 0; pass < 2; ++pass) {
    char* at = out;
    int64_t need = 0;
    for (int64_t line = 0, k = 0; k < n_bytes; ++line) {
      int64_t tab[5], n_tabs = 0, e = k;
      for (; e < n_bytes && bim[e] != '\n'; ++e)
        if (bim[e] == '\t') {
          if (n_tabs < 5) tab[n_tabs] = e;
          ++n_tabs;
        }
      if (e == n_bytes || n_tabs != 5) return sai_set_error(SAI_ERR_ARG, ".bim line %lld: not six tab-separated columns ended by a newline", static_cast<long long>(line + 1));
      const bool no_id = tab[1] - tab[0] == 2 && bim[tab[0] + 1] == '.';
      if (pass == 0) {
        need += (e + 1 - k) + 2 + (no_id ? (tab[0] - k) + (tab[3] - tab[2] - 1) : 0);
      } else {
        auto copy = [&](int64_t from, int64_t to, char then) {  // [from, to) and one separator
          at = std::copy(bim + from, bim + to, at);
          *at++ = then;
        };
        if (no_id) {
          copy(k, tab[0], ':');                // CHROM:POS
          copy(tab[2] + 1, tab[3], '\t');
        } else {
          copy(tab[0] + 1, tab[1], '\t');      // ID
        }
        copy(k, tab[0], '\t');                 // CHROM
        at = std::copy_n("0.0\t", 4, at);      // genetic position: none
        copy(tab[2] + 1, tab[3], '\t');        // POS
        copy(tab[4] + 1, e, '\t');             // REF: the first allele
        copy(tab[3] + 1, tab[4], '\n');        // ALT
      }
      k = e + 1;
    }
    if (pass == 0) {
      *n_out = need;
      if (!out || cap < need) return SAI_OK;
    } else if (at - out != *n_out) {
      return sai_set_error(SAI_ERR_HIP, "sai_geno_snp_lines: the lines were not of the size counted for them");
    }
  }
  return SAI_OK;
}

}  // extern "C"
