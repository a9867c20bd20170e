/* BCF 2.x files (BGZF-compressed) for libsaihip: the host record walk of a file and the decoders that turn the
 * GT vectors of its records into the int8 [record][slot] dosage block which sai_tokenize_gt writes for the same
 * calls as VCF text (DESIGN_INGEST.md, "BCF files").  An extension of saihip.h with its own version number, as
 * saihip_plink.h is: neither saihip.h nor another extension header is touched by it.
 *
 * A GT vector holds, sample-major, L values per sample of 1, 2 or 4 bytes: v = (allele + 1) << 1 | phased,
 * 0 = a missing allele; the end-of-vector value (0x81 / 0x8001 / 0x80000001) and the type's missing value
 * (0x80 / 0x8000 / 0x80000000) count as a missing allele.  A slot of ploidy p reads positions 0 .. p - 1 of its
 * sample's vector (positions at or beyond L are missing alleles, positions from p on are ignored), and with the
 * alleles a (a missing one is -1):
 *
 *   d  = sum a                      the byte of a row that is not flipped
 *   fd = sum (a >= 1 ? a - 1 : 1 - a)   the byte of a row flipped by the ancestral-allele rule
 *
 * status[row] of the decoders: 0 = fine, else the largest of
 *   SAI_BCF_STATUS_RANGE      d > 127, fd > 127 or d < -128 for a slot of the row
 *   SAI_BCF_STATUS_BAD_VALUE  a value with the sign bit set that is neither end-of-vector nor missing
 *   SAI_BCF_STATUS_BAD_INDEX  the row's offset, width or length, a column or a ploidy outside its range
 * and the output bytes the status concerns are 0.  Nothing is read outside the batch.
 */
#ifndef SAIHIP_BCF_H
#define SAIHIP_BCF_H

#include <stdint.h>

#include "saihip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SAI_BCF_ABI_VERSION 1
#define SAI_BCF_STATUS_RANGE 1
#define SAI_BCF_STATUS_BAD_VALUE 2
#define SAI_BCF_STATUS_BAD_INDEX 3
#define SAI_BCF_GT_ALIGN 16 /* every GT array of a stream batch starts at a multiple of this */

typedef struct sai_bcf_stream sai_bcf_stream;

int sai_bcf_abi_version(void);

/* 1 when `path` is a BGZF file whose inflated stream starts with "BCF", else 0 (also when it cannot be read):
 * never an error.  Which BCF version it is, is the business of the calls below. */
int sai_bcf_probe(const char* path);

/* First and last 1-based position of the first contiguous run of `chrom` (-1, -1 if absent), the number of
 * records of the file and the number of samples of its header.  Any pointer may be NULL.  Walks the whole file. */
int sai_bcf_scan(const char* path, const char* chrom, int64_t* first_pos, int64_t* last_pos, int64_t* n_records_total,
                 int64_t* n_samples);

/* One region of a file as a stream of batches, in the shape of sai_vcf_stream_*: a producer thread inflates the
 * members (n_threads at a time), walks the records, selects the rows of `chrom` inside [start, end] (-1 = open;
 * 1-based) under the ancestral-allele rule and copies the GT array of every selected row -- and nothing else --
 * into the two buffers in turn, each array at a multiple of SAI_BCF_GT_ALIGN.  The buffers are the caller's
 * (pinned for the device route), buffer_bytes each.  A sample may be asked for more than once, each time with its
 * own ploidy (1 .. 64): every request is a slot, and that is intended also for the same (sample, ploidy) pair given
 * twice, which simply fills two slots with the same bytes (read_data_device sends ONE pass in which a sample that
 * sits in populations of different ploidy appears once per ploidy; the VCF reader refuses a repeat and is given
 * several passes instead).  n_samples == 0 selects rows only. */
int sai_bcf_stream_open(const char* path, const char* chrom, int64_t start, int64_t end, int32_t n_samples,
                        const char* const* sample_names, const int32_t* ploidy, const char* anc_bed_path, int32_t n_threads,
                        void* buffer0_host, void* buffer1_host, int64_t buffer_bytes, sai_bcf_stream** stream_out);
/* The next batch (the one handed out before is given back to the producer): the buffer it lies in, the bytes
 * filled, the rows, and per row the 1-based position, the flip flag, the byte offset of the GT array inside the
 * batch, the bytes per value (1, 2 or 4) and the values per sample L.  The tables stay valid until the next call.
 * *done = 1: nothing more comes (and nothing was handed out). */
int sai_bcf_stream_next(sai_bcf_stream* stream, int32_t* buffer_index, int64_t* n_bytes, int64_t* n_rows, const int32_t** row_pos_host,
                        const uint8_t** row_flip_host, const int64_t** gt_off_host, const uint8_t** gt_width_host,
                        const int32_t** gt_len_host, int32_t* done);
/* Once the first sai_bcf_stream_next has returned: col_of_slot[n_samples of the request] (the 0-based sample
 * column of every slot; NULL = not wanted, else `capacity` entries are available), the samples of the file, and
 * the counts of the walk so far (complete once `done` was reported): rows of the chromosome inside the region
 * before polarisation, entries of the ancestral-allele table. */
int sai_bcf_stream_selection(sai_bcf_stream* stream, int32_t* col_of_slot_host, int32_t capacity, int32_t* n_file_samples,
                             int64_t* n_matched, int64_t* n_anc_entries);
/* Once `done` was reported: the producer thread's seconds by phase -- reading the file, inflating its members
 * (wall time of the n_threads workers), walking the records (header, dictionaries and selection included),
 * copying GT arrays into the staging buffers, waiting for a free buffer -- and the bytes inflated and staged.
 * Any pointer may be NULL.  What tools/bcf_rate.py reports. */
int sai_bcf_stream_stats(sai_bcf_stream* stream, double* file_read_s, double* inflate_s, double* walk_s, double* copy_s, double* wait_s,
                         int64_t* inflated_bytes, int64_t* staged_bytes);
int sai_bcf_stream_close(sai_bcf_stream* stream);

/* The plain statement of the dosage table, on the host.  `batch` = batch_bytes bytes; output row r (of n_rows) is
 * decoded from the n_cols * gt_len[r] values of gt_width[r] bytes at batch + gt_off[r] and is flipped when
 * row_flip[r] != 0; slot s (of n_slots) takes column col_of_slot[s] (< n_cols) at ploidy_of_slot[s].
 * out = int8 [n_rows][n_slots], status = int32 [n_rows]. */
int sai_bcf_decode_host(const uint8_t* batch, int64_t batch_bytes, int64_t n_rows, const int64_t* gt_off, const uint8_t* gt_width,
                        const int32_t* gt_len, const uint8_t* row_flip, int32_t n_cols, int32_t n_slots, const int32_t* col_of_slot,
                        const int32_t* ploidy_of_slot, int8_t* out, int32_t* status, int32_t n_threads);

/* The same on the GPU: every pointer is device memory, `batch` 16-byte aligned, gt_off[r] any byte.  `out` is the
 * 16-byte aligned start of a [*][n_slots] block of which this call writes the rows [out_row0, out_row0 +
 * n_out_rows) (and nothing else): the other arrays are indexed by the row of the call, 0 .. n_out_rows - 1.  Two
 * promises of the caller select the fast path and stand in for the arrays, which may then be NULL: first_col >= 0:
 * col_of_slot[s] == first_col + s for every slot; uniform_ploidy in 1 .. 64: ploidy_of_slot[s] == uniform_ploidy
 * for every slot (0 = read the array). */
int sai_bcf_decode(sai_ctx* ctx, const uint8_t* batch, int64_t batch_bytes, int64_t n_out_rows, const int64_t* gt_off,
                   const uint8_t* gt_width, const int32_t* gt_len, const uint8_t* row_flip, int32_t n_cols, int32_t n_slots,
                   const int32_t* col_of_slot, int32_t first_col, const int32_t* ploidy_of_slot, int32_t uniform_ploidy, int8_t* out,
                   int64_t out_row0, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SAIHIP_BCF_H */
