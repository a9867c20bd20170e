/* BCF 2.x files whose members are inflated and whose records are found on the GPU (DESIGN_INGEST.md, "BCF files:
 * members inflated and records found on the GPU").  An extension of saihip.h and saihip_bcf.h with its own version
 * number, as saihip_pgen_packed.h is: no other header is touched by it.
 *
 * The inflated stream of a batch -- the carry of the batch before, then the text sai_inflate_bgzf wrote behind it --
 * lies in HBM.  A record chain has to be followed from its start, so the stream is cut into segments of seg_bytes
 * and every segment is walked from every place where a record COULD start:
 *
 *   sai_bcf_chain_segments   one wavefront per segment: the candidates of the segment, the heads of their chains
 *                            and where every chain leaves the segment
 *   sai_bcf_stitch           on the host, over the summaries: from the one known entry, exit to exit
 *   sai_bcf_record_heads     one wavefront per segment with a true entry: a 64-byte head per record
 *
 * A byte offset o is a CANDIDATE when o + 32 <= n_bytes and the 32 bytes at o pass the checks the host walk makes
 * on the fixed fields of a record: l_shared >= 24, CHROM is an index a ##contig line defines, and the low 24 bits of
 * the word at o + 28 are the sample count of the header.  Its successor is o + 8 + l_shared + l_indiv > o + 31.
 * The *_host twins are plain C++ with the same arguments and the same outputs bit for bit.
 */
#ifndef SAIHIP_BCF_DEVICE_H
#define SAIHIP_BCF_DEVICE_H

#include <stdint.h>

#include "saihip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SAI_BCF_DEVICE_ABI_VERSION 1
#define SAI_BCF_MAX_HEADS 8       /* the default max_heads; at most SAI_BCF_MAX_HEADS_LIMIT */
#define SAI_BCF_MAX_HEADS_LIMIT 64
#define SAI_BCF_SEG_MIN 256       /* seg_bytes is a power of two in [SAI_BCF_SEG_MIN, SAI_BCF_SEG_MAX] */
#define SAI_BCF_SEG_MAX 65536
#define SAI_BCF_ALLELE_BYTES 12   /* bytes of REF and of the first ALT a record head carries */
#define SAI_BCF_HOST_ROUTE 1      /* a return value (> 0, no error is set): this read is for sai_bcf_stream_* */

/* the chain of one head inside its segment */
#define SAI_BCF_CHAIN_BROKEN 1     /* a successor inside n_bytes is not a candidate: chain_exit is that successor */
#define SAI_BCF_CHAIN_INCOMPLETE 2 /* chain_exit is a record that does not lie inside n_bytes (or its 32 bytes do not) */
typedef struct sai_bcf_chain {
  uint32_t head;       /* offset of the head */
  uint32_t chain_exit; /* first chain position at or behind the segment's end, or the incomplete / broken offset */
  uint32_t n_records;  /* complete records of the chain that start inside the segment */
  uint32_t flags;
} sai_bcf_chain;

/* what sai_bcf_record_heads writes per record */
#define SAI_BCF_HEAD_NO_GT 1        /* genotypes asked for, no FORMAT entry has the header's GT key */
#define SAI_BCF_HEAD_GT_NOT_INT 2   /* the GT entry's type is not an integer type (gt_width holds the type) */
#define SAI_BCF_HEAD_LEAVES 4       /* a typed value, a FORMAT vector or the GT array of the individual part leaves the record */
#define SAI_BCF_HEAD_SHARED_LEAVES 8 /* ID, REF or the first ALT leaves the shared part */
typedef struct sai_bcf_record_head {
  uint32_t off;      /* of the record inside the batch */
  uint32_t gt_off;   /* absolute offset of the GT array inside the batch */
  uint32_t l_shared, l_indiv;
  int32_t chrom;     /* the dictionary index */
  int32_t pos0;      /* 0-based, as the file has it */
  int32_t gt_len;    /* values per sample L */
  uint16_t n_allele;
  uint8_t n_fmt;
  uint8_t flags;
  uint8_t ref_len, alt_len; /* saturated at 255; an absent ALT is length 1 and "." */
  uint8_t gt_width;  /* 1, 2 or 4 */
  uint8_t reserved0;
  uint8_t ref[SAI_BCF_ALLELE_BYTES], alt[SAI_BCF_ALLELE_BYTES]; /* the first bytes, the rest 0 */
  uint32_t reserved1;
} sai_bcf_record_head; /* 64 bytes */

int sai_bcf_device_abi_version(void);

/* Kernel A.  text = n_bytes (< 2^31) of inflated stream in HBM, 16-byte aligned; contig_defined[n_contigs] (uint8,
 * device) and n_sample from the header.  n_segments = ceil(n_bytes / seg_bytes).  Outputs (device), all of them
 * written in full: chains[n_segments * max_heads] -- the first n_heads[seg] entries of a segment's row hold its heads
 * in ascending order, the others are zero -- and seg_info[n_segments] = number of heads written | 1 << 30 when the
 * segment has more than max_heads of them (it is DENSE).  The grid is one wavefront per segment, never capped. */
int sai_bcf_chain_segments(sai_ctx* ctx, const uint8_t* text, int64_t n_bytes, int32_t seg_bytes, int32_t max_heads,
                           const uint8_t* contig_defined, int32_t n_contigs, int32_t n_sample, sai_bcf_chain* chains,
                           int32_t* seg_info, void* stream);
int sai_bcf_chain_segments_host(const uint8_t* text, int64_t n_bytes, int32_t seg_bytes, int32_t max_heads,
                                const uint8_t* contig_defined, int32_t n_contigs, int32_t n_sample, sai_bcf_chain* chains,
                                int32_t* seg_info);

/* Host only, over the summaries copied back.  From the known entry e0 (<= n_bytes) exit to exit: seg_entry[seg] =
 * the offset at which the true chain enters the segment (-1: it does not), seg_first_record[seg] = the index of
 * the record there, *n_records = the complete records of the batch, *carry_from = the offset of the first
 * incomplete record, or n_bytes.  *verdict = 0, or SAI_BCF_HOST_ROUTE when the entry is not a head of its segment,
 * the chain is broken or a dense segment lies on it (the other outputs then say how far the chain was followed). */
int sai_bcf_stitch(const sai_bcf_chain* chains_host, const int32_t* seg_info_host, int64_t n_bytes, int32_t seg_bytes,
                   int32_t max_heads, int64_t e0, int64_t* seg_entry_host, int64_t* seg_first_record_host,
                   int64_t* n_records, int64_t* carry_from, int32_t* verdict);

/* Kernel B.  seg_entry / seg_first_record as sai_bcf_stitch left them (device copies); a segment's chain is
 * followed from its entry while it stays inside the segment and in front of carry_from, and record i of the batch
 * gets heads[i] (i < n_records; nothing else is written).  want_gt != 0: the GT entry is looked for by stepping
 * over the n_fmt typed entries as the host walk does (gt_key = the header's, -1 when it has none).  Nothing is read
 * outside a record or outside n_bytes. */
int sai_bcf_record_heads(sai_ctx* ctx, const uint8_t* text, int64_t n_bytes, int32_t seg_bytes, const int64_t* seg_entry,
                         const int64_t* seg_first_record, int64_t carry_from, int64_t n_records, int64_t gt_key,
                         int32_t want_gt, sai_bcf_record_head* heads, void* stream);
int sai_bcf_record_heads_host(const uint8_t* text, int64_t n_bytes, int32_t seg_bytes, const int64_t* seg_entry,
                              const int64_t* seg_first_record, int64_t carry_from, int64_t n_records, int64_t gt_key,
                              int32_t want_gt, sai_bcf_record_head* heads);

/* The feed, in the shape of sai_bgzf_stream_*.  open loads the ancestral table, inflates on the host the members that
 * hold the header, parses it and resolves the samples, and starts a reader thread that hands the file's members
 * over as they are, padded to 4 bytes, in the caller's two pinned buffers in turn, at most text_batch_bytes of
 * inflated bytes per batch.  The first batch starts at the member in which the header ends.  Returns
 * SAI_BCF_HOST_ROUTE where this route does not serve the read (an ancestral allele of the region longer than
 * SAI_BCF_ALLELE_BYTES).  whole_file != 0: the selection goes on behind the run and counts every record (the scan).
 * A batch never holds more members than fit comp_buffer_bytes, and always at least one. */
typedef struct sai_bcf_feed sai_bcf_feed;
int sai_bcf_feed_open(const char* path, const char* chrom, int64_t start, int64_t end, int32_t n_samples,
                      const char* const* sample_names, const char* anc_bed_path, void* comp0_host, void* comp1_host,
                      int64_t comp_buffer_bytes, int64_t text_batch_bytes, int32_t whole_file, sai_bcf_feed** feed_out);
/* Batch k (blocking; the buffer of batch k - 1 is given back): the table sai_inflate_bgzf takes, out_off counted
 * from the first byte behind the carry.  *e0 = where the records start inside the batch's own text: the first byte
 * behind the header for the first batch, else 0.  *done = 1: the file has ended (nothing was handed out). */
int sai_bcf_feed_next(sai_bcf_feed* feed, int32_t* buffer_index, int64_t* n_comp_bytes, int32_t* n_members,
                      const sai_bgzf_member** members_host, int64_t* n_text_bytes, int64_t* e0, int32_t* done);
/* Early form of the release sai_bcf_feed_next performs: the batch's compressed bytes and its table have been copied. */
int sai_bcf_feed_release(sai_bcf_feed* feed);
/* The row selection of the host walk over the heads of a batch (host memory), continued from the batch before:
 * chromosome, first contiguous run, start / end, the ancestral rule, the early stop.  Per selected row (the tables
 * stay valid until the next call) pos (1-based), flip, gt_off, gt_width, gt_len; *done = 1 once the run has passed
 * `end` or another chromosome follows (with whole_file the walk goes on and counts).  *verdict = SAI_BCF_HOST_ROUTE
 * when a selected row carries an error flag. */
int sai_bcf_feed_select(sai_bcf_feed* feed, const sai_bcf_record_head* heads_host, int64_t n_heads, int64_t* n_rows,
                        const int32_t** row_pos_host, const uint8_t** row_flip_host, const int64_t** gt_off_host,
                        const uint8_t** gt_width_host, const int32_t** gt_len_host, int32_t* done, int32_t* verdict);
/* col_of_slot[n_samples of the request] (NULL = not wanted), contig_defined[capacity_contigs] (NULL = not wanted;
 * *n_contigs says how many there are), the samples of the file, the header's GT key, and the counts of the
 * selection so far: rows matched before polarisation, entries of the ancestral table, records seen, first and last
 * position of the run (-1: none). */
int sai_bcf_feed_selection(sai_bcf_feed* feed, int32_t* col_of_slot_host, int32_t capacity, uint8_t* contig_defined_host,
                           int32_t capacity_contigs, int32_t* n_contigs, int32_t* n_file_samples, int64_t* gt_key,
                           int64_t* n_matched, int64_t* n_anc_entries, int64_t* n_records_total, int64_t* first_pos,
                           int64_t* last_pos);
/* Seconds of reading the file, inflating the header's members, selecting, and of the reader thread's waiting for a
 * free buffer; the compressed bytes handed over.  Any pointer may be NULL. */
int sai_bcf_feed_stats(sai_bcf_feed* feed, double* file_read_s, double* header_inflate_s, double* select_s, double* wait_s,
                       int64_t* comp_bytes);
int sai_bcf_feed_close(sai_bcf_feed* feed);

#ifdef __cplusplus
}
#endif

#endif /* SAIHIP_BCF_DEVICE_H */
