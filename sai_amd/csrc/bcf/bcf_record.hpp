// One BCF record in a byte stream, for the kernels of bcf_walk.hip and their plain C++ twins in bcf_feed.cpp: the
// candidate test of include/saihip_bcf_device.h and the 64-byte head of a record.  The functions are the same text
// for both compilers, so a head is the same bytes on both sides by construction; how a segment is searched and
// its chains are followed is written twice.  The typed-value rules are those of bcf_format.hpp (typed_int,
// typed_desc, typed_string), restated on offsets so that every read is checked against the record's end first.
#pragma once

#include <stdint.h>

#include "saihip_bcf_device.h"

#if defined(__HIPCC__)
#define SAI_BCF_HD __host__ __device__ inline
#else
#define SAI_BCF_HD inline
#endif

extern "C" int sai_set_error(int code, const char* fmt, ...);  // host_core.cpp

namespace bcfrec {

// the arguments the kernels' entry points and their host twins share; only a device buffer has to be aligned
inline int check_stream_args(const uint8_t* text, int64_t n_bytes, int32_t seg_bytes, bool aligned) {
  if (n_bytes < 0 || n_bytes >= (int64_t(1) << 31)) return sai_set_error(SAI_ERR_ARG, "n_bytes must be in [0, 2^31)");
  if (seg_bytes < SAI_BCF_SEG_MIN || seg_bytes > SAI_BCF_SEG_MAX || (seg_bytes & (seg_bytes - 1)))
    return sai_set_error(SAI_ERR_ARG, "seg_bytes must be a power of two in [%d, %d]", SAI_BCF_SEG_MIN, SAI_BCF_SEG_MAX);
  if (n_bytes > 0 && !text) return sai_set_error(SAI_ERR_ARG, "NULL buffer");
  if (aligned && (reinterpret_cast<uintptr_t>(text) & 15u)) return sai_set_error(SAI_ERR_ARG, "text must be 16-byte aligned");
  return 0;
}

SAI_BCF_HD uint32_t le32_at(const uint8_t* t, int64_t o) {
  return static_cast<uint32_t>(t[o]) | static_cast<uint32_t>(t[o + 1]) << 8 | static_cast<uint32_t>(t[o + 2]) << 16 |
         static_cast<uint32_t>(t[o + 3]) << 24;
}

// the three checks on the fixed fields, given the words (o + 32 <= n_bytes is the caller's)
SAI_BCF_HD bool fixed_fields_pass(uint32_t l_shared, uint32_t chrom, uint32_t word28, const uint8_t* contig_defined, int32_t n_contigs,
                                  int32_t n_sample) {
  return l_shared >= 24u && (word28 & 0xFFFFFFu) == static_cast<uint32_t>(n_sample) && chrom < static_cast<uint32_t>(n_contigs) &&
         contig_defined[chrom] != 0;
}

SAI_BCF_HD bool is_candidate(const uint8_t* t, int64_t n_bytes, int64_t o, const uint8_t* contig_defined, int32_t n_contigs, int32_t n_sample) {
  if (o < 0 || o + 32 > n_bytes) return false;
  return fixed_fields_pass(le32_at(t, o), le32_at(t, o + 8), le32_at(t, o + 28), contig_defined, n_contigs, n_sample);
}

SAI_BCF_HD int64_t successor(const uint8_t* t, int64_t o) { return o + 8 + static_cast<int64_t>(le32_at(t, o)) + static_cast<int64_t>(le32_at(t, o + 4)); }

SAI_BCF_HD int type_width(int type) { return type == 1 || type == 7 ? 1 : type == 2 ? 2 : type == 3 || type == 5 ? 4 : type == 0 ? 0 : -1; }

struct Cur {
  const uint8_t* t;
  int64_t p, end;  // end <= n_bytes
};

SAI_BCF_HD bool typed_int(Cur& c, int64_t* v) {
  if (c.p >= c.end) return false;
  const int desc = c.t[c.p++];
  const int type = desc & 15, width = type_width(type);
  if ((desc >> 4) != 1 || type < 1 || type > 3 || c.end - c.p < width) return false;
  if (width == 1) *v = static_cast<int8_t>(c.t[c.p]);
  else if (width == 2) *v = static_cast<int16_t>(static_cast<uint16_t>(c.t[c.p] | c.t[c.p + 1] << 8));
  else *v = static_cast<int32_t>(le32_at(c.t, c.p));
  c.p += width;
  return true;
}

SAI_BCF_HD bool typed_desc(Cur& c, int* type, int64_t* count) {
  if (c.p >= c.end) return false;
  const int desc = c.t[c.p++];
  *type = desc & 15;
  *count = desc >> 4;
  if (*count == 15 && (!typed_int(c, count) || *count < 0)) return false;
  return type_width(*type) >= 0;
}

// a typed string: where it lies (*at, *n)
SAI_BCF_HD bool typed_string(Cur& c, int64_t* at, int64_t* n) {
  int type;
  int64_t count;
  if (!typed_desc(c, &type, &count)) return false;
  if (type == 0) count = 0;
  else if (type != 7) return false;
  if (c.end - c.p < count) return false;
  *at = c.p;
  *n = count;
  c.p += count;
  return true;
}

// The head of the record at `off`: a complete record inside n_bytes with l_shared >= 24 (what the stitched chain
// guarantees; checked again by the caller).
SAI_BCF_HD void fill_head(const uint8_t* t, int64_t off, int64_t gt_key, bool want_gt, sai_bcf_record_head* out) {
  // the scalars are kept in registers and every field is stored once: a head built in a local struct would live in
  // scratch memory on the GPU (its allele bytes are indexed by a loop)
  const uint32_t l_shared = le32_at(t, off), l_indiv = le32_at(t, off + 4);
  const uint32_t n_allele = le32_at(t, off + 24) >> 16, w28 = le32_at(t, off + 28), n_fmt = w28 >> 24;
  const int64_t n_sample = w28 & 0xFFFFFFu;
  const int64_t shared_end = off + 8 + static_cast<int64_t>(l_shared), total_end = shared_end + static_cast<int64_t>(l_indiv);
  uint32_t flags = 0, gt_off = 0, gt_width = 0, ref_len = 0, alt_len = 1;
  int32_t gt_len = 0;
  for (int i = 0; i < SAI_BCF_ALLELE_BYTES; ++i) out->ref[i] = out->alt[i] = 0;
  out->alt[0] = '.';
  {
    Cur c{t, off + 32, shared_end};
    int64_t at = 0, n = 0;
    bool ok = typed_string(c, &at, &n);  // ID
    if (ok && n_allele >= 1) {
      ok = typed_string(c, &at, &n);
      if (ok) {
        ref_len = static_cast<uint32_t>(n > 255 ? 255 : n);
        for (int i = 0; i < SAI_BCF_ALLELE_BYTES && i < n; ++i) out->ref[i] = t[at + i];
      }
    }
    if (ok && n_allele >= 2) {
      ok = typed_string(c, &at, &n);
      if (ok) {
        alt_len = static_cast<uint32_t>(n > 255 ? 255 : n);
        out->alt[0] = 0;
        for (int i = 0; i < SAI_BCF_ALLELE_BYTES && i < n; ++i) out->alt[i] = t[at + i];
      }
    }
    if (!ok) flags |= SAI_BCF_HEAD_SHARED_LEAVES;
  }
  if (want_gt) {
    Cur c{t, shared_end, total_end};
    bool found = false, bad = false;
    for (uint32_t k = 0; k < n_fmt && !found && !bad; ++k) {
      int64_t key, count;
      int type;
      if (!typed_int(c, &key) || !typed_desc(c, &type, &count)) {
        flags |= SAI_BCF_HEAD_LEAVES;
        bad = true;
        break;
      }
      const int width = type_width(type);
      const int64_t per = n_sample * (width > 1 ? width : 1);
      if (count > (int64_t(1) << 31) / (per > 1 ? per : 1)) {
        flags |= SAI_BCF_HEAD_LEAVES;
        bad = true;
        break;
      }
      const int64_t bytes = n_sample * count * width;
      if (key == gt_key) {
        if (type < 1 || type > 3) {
          flags |= SAI_BCF_HEAD_GT_NOT_INT;
          gt_width = static_cast<uint32_t>(type);
          bad = true;
        } else if (c.end - c.p < bytes) {
          flags |= SAI_BCF_HEAD_LEAVES;
          bad = true;
        } else {
          gt_off = static_cast<uint32_t>(c.p);
          gt_width = static_cast<uint32_t>(width);
          gt_len = static_cast<int32_t>(count);
          found = true;
        }
      } else if (c.end - c.p < bytes) {
        flags |= SAI_BCF_HEAD_LEAVES;
        bad = true;
      } else {
        c.p += bytes;
      }
    }
    if (!found && !bad) flags |= SAI_BCF_HEAD_NO_GT;
  }
  out->off = static_cast<uint32_t>(off);
  out->gt_off = gt_off;
  out->l_shared = l_shared;
  out->l_indiv = l_indiv;
  out->chrom = static_cast<int32_t>(le32_at(t, off + 8));
  out->pos0 = static_cast<int32_t>(le32_at(t, off + 12));
  out->gt_len = gt_len;
  out->n_allele = static_cast<uint16_t>(n_allele);
  out->n_fmt = static_cast<uint8_t>(n_fmt);
  out->flags = static_cast<uint8_t>(flags);
  out->ref_len = static_cast<uint8_t>(ref_len);
  out->alt_len = static_cast<uint8_t>(alt_len);
  out->gt_width = static_cast<uint8_t>(gt_width);
  out->reserved0 = 0;
  out->reserved1 = 0;
}

}  // namespace bcfrec
