/* The .csi index of a BCF file: a region read begins at a virtual offset the index names instead of at the first
 * record of the file (DESIGN_INGEST.md, "BCF files: a region is a seek").  An extension of saihip_bcf.h and
 * saihip_bcf_device.h with its own version number: neither of them, nor any other header, is touched by it.
 *
 * A virtual offset is coffset << 16 | uoffset: the file offset of a BGZF member and the byte inside that member's
 * inflated text.  The index answers one question -- where may the walk for [start, end] of a contig begin -- and the
 * answer may lie earlier than necessary but never behind the first record of the contig whose POS is >= start.
 * Where to stop stays the walk's own rule.  The index is never an error of a read: sai_bcf_index_open is the only
 * call that words what is wrong with one, and the *_open_at calls below read from the start of the file, exactly as
 * sai_bcf_stream_open / sai_bcf_feed_open do, whenever the index does not serve the read.
 */
#ifndef SAIHIP_BCF_INDEX_H
#define SAIHIP_BCF_INDEX_H

#include <stdint.h>

#include "saihip.h"
#include "saihip_bcf.h"
#include "saihip_bcf_device.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SAI_BCF_INDEX_ABI_VERSION 1
/* the answers of sai_bcf_index_query */
#define SAI_BCF_INDEX_NONE 0 /* no record of the contig overlaps the region or lies behind it */
#define SAI_BCF_INDEX_SEEK 1 /* *voffset is where the walk may begin */
#define SAI_BCF_INDEX_WALK 2 /* the index does not serve the question: walk from the start */

typedef struct sai_bcf_index sai_bcf_index;

int sai_bcf_index_abi_version(void);

/* Loads, parses and validates `index_path` (a BGZF file, CSI v1) for a data file of data_file_bytes bytes: the magic,
 * min_shift + 3 * depth <= 62 and depth <= 10, every count against the bytes that are left, every coffset below
 * data_file_bytes, chunk_beg < chunk_end, no bin twice.  The handle is immutable: any number of reads may share it. */
int sai_bcf_index_open(const char* index_path, int64_t data_file_bytes, sai_bcf_index** index_out);
/* min_shift, depth, the references of the index and n_no_coor (-1 where the file ends without it).  Any pointer may
 * be NULL. */
int sai_bcf_index_info(const sai_bcf_index* index, int32_t* min_shift, int32_t* depth, int32_t* n_ref, int64_t* n_no_coor);
/* The question above for the reference `contig` (the BCF contig index) and the 1-based inclusive [start, end]
 * (-1 = open).  `end` only tells an empty region: the bins asked are those that overlap [start, the end of the index's
 * range), so that the answer holds also where the region itself has no record.  SAI_BCF_INDEX_WALK: the contig is not in the index, start lies beyond the index's range, the region
 * is empty, or the chunks of the contig and those of another one interleave (the walk takes the first contiguous
 * run of a chromosome, and only a walk from the start knows which one that is). */
int sai_bcf_index_query(const sai_bcf_index* index, int32_t contig, int64_t start, int64_t end, int32_t* answer, uint64_t* voffset);
int sai_bcf_index_close(sai_bcf_index* index);

/* sai_bcf_stream_open with an index (NULL: exactly sai_bcf_stream_open).  The header is read from the start of the
 * file; the producer then asks the index for the region and continues at the member `coffset` with its first record
 * at `uoffset`, provided that the index has no more references than the header has contigs, the answer is
 * SAI_BCF_INDEX_SEEK, coffset lies behind the members that hold the header, the member inflates, and the 32 bytes at
 * uoffset pass the three checks of a candidate (saihip_bcf_device.h) and name the contig asked for.  Otherwise it
 * reads on from the header as sai_bcf_stream_open does.  A stream that has seeked and then meets an error words it
 * with record numbers counted from the seek: read again without the index for the sentence of the unindexed read. */
int sai_bcf_stream_open_at(const char* path, const char* chrom, int64_t start, int64_t end, int32_t n_samples,
                           const char* const* sample_names, const int32_t* ploidy, const char* anc_bed_path, int32_t n_threads,
                           void* buffer0_host, void* buffer1_host, int64_t buffer_bytes, const sai_bcf_index* index,
                           sai_bcf_stream** stream_out);
/* Once `done` was reported: whether the producer seeked and to which virtual offset, the bytes of the data file whose
 * members it inflated (the header's members included; a failed attempt to seek too) and the number of those members.
 * Any pointer may be NULL. */
int sai_bcf_stream_seek_stats(sai_bcf_stream* stream, int32_t* seeked, uint64_t* voffset, int64_t* file_bytes_read, int64_t* members_inflated);

/* sai_bcf_feed_open with an index (NULL: exactly sai_bcf_feed_open), under the same conditions but the last two: the
 * first batch's members start at `coffset` and the e0 of the first sai_bcf_feed_next is `uoffset`; whether a record
 * starts there is for sai_bcf_stitch to say.  The member at coffset holds the end of earlier records in front of
 * uoffset, whose chains run into uoffset: the caller clears the bytes [0, e0) of the first batch's text before
 * sai_bcf_chain_segments, so that uoffset is the head of its chain. */
int sai_bcf_feed_open_at(const char* path, const char* chrom, int64_t start, int64_t end, int32_t n_samples, const char* const* sample_names,
                         const char* anc_bed_path, void* comp0_host, void* comp1_host, int64_t comp_buffer_bytes, int64_t text_batch_bytes,
                         int32_t whole_file, const sai_bcf_index* index, sai_bcf_feed** feed_out);
/* Whether the feed seeked, to which virtual offset, the contig index of the chromosome (-1: the header has none), and
 * so far: the bytes of the data file read as members (those the host inflated for the header included) and the
 * number of those members.  Any pointer may be NULL. */
int sai_bcf_feed_seek_stats(sai_bcf_feed* feed, int32_t* seeked, uint64_t* voffset, int32_t* contig, int64_t* file_bytes_read, int64_t* members_read);

#ifdef __cplusplus
}
#endif

#endif /* SAIHIP_BCF_INDEX_H */
