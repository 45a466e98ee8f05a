/*
 * fem_hip.h — C ABI of libfemhip.so: FEM's per-read mapping hot path on MI355X (gfx950).
 *
 * The reference (haowenz/FEM v0.2) has no plugin/FFI layer; the seam this
 * library replaces is the per-read call sequence inside
 * single_end_read_mapping_thread (src/map.c:27-55):
 *
 *     generate_group_seeding_candidates()   src/filter.h:9   (src/filter.c:146-223)
 *     verify_candidates()                   src/align.h:13   (src/align.c:4-51)
 *     MappingStats accumulation             src/map.c:25,32-33,37,43-44,48,51
 *
 * called once per read and strand.  Here the same work is done one BATCH at a
 * time: the index (src/index.h:7-14) and the reference text are uploaded once
 * and stay resident in HBM, reads are handed over as one contiguous byte
 * array + offsets, and the per-candidate verification outcome comes back as
 * flat arrays from which the host rebuilds the reference's Mapping lists
 * (src/utils.h:44-49) in the reference's order.
 *
 * Plain C types only; no exits or aborts: every call returns 0 (FEM_OK) or a
 * negative fem_status, and fem_dev_last_error() holds a message.
 * A handle is not thread-safe; distinct handles are independent.
 */
#ifndef FEM_HIP_H_
#define FEM_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum fem_status {
  FEM_OK = 0,
  FEM_ERR_INVALID = -1,     /* bad argument (NULL, out-of-range parameter, bad slot) */
  FEM_ERR_HIP = -2,         /* a HIP runtime call failed; see fem_dev_last_error() */
  FEM_ERR_NOMEM = -3,       /* host or device allocation failed */
  FEM_ERR_STATE = -4,       /* call order violated (e.g. map before index upload) */
  FEM_ERR_UNSUPPORTED = -5, /* input outside what the device path handles (see fem_dev_limits) */
  FEM_ERR_RCCL = -6         /* an RCCL call failed */
};

/* FEMArgs (src/utils.h:63-70) minus threads/seeding_method.  `FEM map` always
 * runs k=12, step=3 (src/FEM_map.c:67-68); 0<=e<=7, 0<=a<=2 (src/FEM_map.c:30,38).
 * 1<=k<=15, 1<=step<=16.  k = 16 is refused everywhere: the reference's hash mask is
 * ((uint32_t)1 << 32) - 1 there (src/utils.h:84,104), which is undefined.  k must be
 * the resident index's; step need not be its step (the seeds are then looked up in
 * an occurrence table sampled at another step). */
typedef struct {
  int32_t k;
  int32_t step;
  int32_t e; /* error_threshold */
  int32_t a; /* num_additional_qgrams */
} fem_params;

/* One batch of reads: what a SequenceBatch (src/sequence_batch.h:15-24) holds
 * for the hot path — the raw read characters, concatenated, and n_reads+1 offsets. */
typedef struct {
  const char *bases;
  const uint64_t *offsets;
  uint64_t n_reads;
} fem_read_batch;

/* Outcome of one batch.  Pointers refer to pinned host memory owned by the
 * handle and stay valid until the slot is staged or mapped again.
 * Slot 2*i+d describes strand d (0 = POSITIVE_DIRECTION, 1 = NEGATIVE_DIRECTION,
 * src/utils.h:21-22) of read i: its candidates (src/filter.c:221-222, ascending,
 * already shifted by -e) are cand[cand_begin[s] .. cand_begin[s]+cand_count[s]),
 * and ed[]/end[] hold banded_edit_distance's result for each (src/align.c:102-147;
 * ed == 0xFF when the candidate is rejected, i.e. the reference would not push
 * a Mapping, src/align.c:22,40). */
typedef struct {
  uint64_t n_reads;
  uint64_t n_candidates; /* slots in cand/ed/end; includes padding slots that no (read, strand) refers to */
  const uint32_t *cand_begin; /* 2*n_reads */
  const uint32_t *cand_count; /* 2*n_reads */
  const uint64_t *cand;       /* n_candidates: seq<<32 | (pos - e) */
  const uint8_t *ed;          /* n_candidates */
  const int16_t *end;         /* n_candidates: Mapping.end_position_offset */
  /* MappingStats (src/utils.h:55-61): reads, mapped reads, candidates before the
   * additional q-gram filter, candidates, mappings */
  uint64_t stats[5];
} fem_batch_result;

/* The same outcome in the form that crosses the link (round 5): 11.4 instead of 30.8 bytes per read at BASELINE config 2.
 * The candidate slots of fem_batch_result are handed out in chunks per wavefront (padding between them, 16 bytes of
 * cand_begin / cand_count per read); here the candidates of strands [256 b, 256 b + 256) (strand s = 2 * read + direction,
 * as above) lie in strand order from seg_begin[b] on, without padding, and a strand has count[s] of them — count[s] == 255
 * means "255 or more": its real count is listed in big[] (n_big pairs: strand, count).  A caller walking the batch in read
 * order — what process_mappings does, src/align.c:56-92 — keeps one running index per segment and never needs an offset
 * per read.  Same lifetime as fem_batch_result. */
typedef struct {
  uint64_t n_reads;
  uint64_t n_candidates;     /* entries of cand/ed/end: every one belongs to a strand */
  const uint8_t *count;      /* 2*n_reads */
  const uint32_t *seg_begin; /* ceil(2*n_reads / 256) */
  const uint64_t *cand;      /* seq<<32 | (pos - e) */
  const uint8_t *ed;         /* 0xFF = rejected */
  const int16_t *end;
  const uint32_t *big;       /* 2*n_big: (strand, count) */
  uint32_t n_big;
  uint64_t stats[5];
} fem_batch_packed;

/* The records of one batch as process_mappings would hand them to the writer
 * (src/align.c:56-92): each mapped read's Mappings ordered by radix_sort_mapping
 * (src/align.c:53,66; klib semantics, src/ksort.h:101-151), then per Mapping
 * generate_alignment + generate_MD_tag (src/align.c:279-544) and the record
 * fields of generate_bam1_t (src/align.c:546-632).  Pointers refer to pinned
 * host memory owned by the handle, valid until the slot's next fetch_records. */
typedef struct {
  uint64_t n_reads;
  uint64_t n_records;
  const uint32_t *rec_begin; /* n_reads+1: records of read i are [rec_begin[i], rec_begin[i+1]); the first is the primary */
  const uint16_t *flag;      /* 16 = BAM_FREVERSE, 256 = BAM_FSECONDARY; 0x8000 = the reference would have asserted (empty CIGAR/MD) */
  const uint32_t *tid;       /* reference sequence index */
  const uint32_t *pos0;      /* 0-based leftmost position (src/align.c:80) */
  const uint8_t *nm;         /* edit distance */
  const uint32_t *cigar_off; /* n_records+1 */
  const uint32_t *cigar;     /* BAM encoding: len<<4 | op, M=0 I=1 D=2 */
  const uint32_t *md_off;    /* n_records+1 */
  const char *md;            /* MD tag characters, not NUL-terminated */
  uint64_t stats[5];
} fem_batch_records;

/* The batch's output as SAM text, rendered on the device (replaces process_mappings + generate_bam1_t + the SAM writer,
 * src/align.c:56-92,546-632, src/output_queue.c:93-116, for the batch): the lines of every mapped read, reads in batch
 * order, a read's records in the reference's order.  Pinned host memory owned by the library, valid until the slot is
 * fetched this way again. */
typedef struct {
  const char *text;
  uint64_t len;
  uint64_t n_reads, n_records;
  uint64_t n_asserted; /* records on which the reference would have tripped an assertion: written with CIGAR * */
  uint64_t stats[5];
} fem_batch_sam;

typedef struct fem_dev fem_dev;

/* Process-wide, before fem_dev_open: handles opened afterwards make their threads SLEEP while they wait for the device
 * (hipDeviceScheduleBlockingSync) instead of spinning.  For callers that keep several threads waiting on one handle while
 * other threads need the cores (FEM map: a thread per batch in flight beside the FASTQ parser); a caller with one thread
 * that waits rarely (bench.py's pipeline) is better off with the default. */
int fem_set_blocking_waits(int on);

/* ---- lifetime ---- */
int fem_dev_open(int device, fem_dev **out);
int fem_dev_close(fem_dev *h);
const char *fem_strerror(int rc);
const char *fem_dev_last_error(const fem_dev *h);
/* Limits of the device path: max read length, number of batch slots. */
int fem_dev_limits(const fem_dev *h, uint32_t *max_read_len, int32_t *n_slots);

/* ---- resident data (replaces load_index / the reference SequenceBatch;
 *      src/index.c:100-131, src/FEM_map.c:135-143) ---- */
/* lookup: 4^k+1 prefix sums; occ: seq<<32|pos, ascending in each bucket — byte
 * for byte the arrays of the index file (src/index.c:133-168).  1<=k<=15, step>=1. */
int fem_dev_upload_index(fem_dev *h, int32_t k, int32_t step, const uint32_t *lookup, uint64_t n_lookup,
                         const uint64_t *occ, uint64_t n_occ);
/* seq[i] points at seq_len[i] raw FASTA characters (any case; non-ACGT = N). */
int fem_dev_upload_reference(fem_dev *h, uint32_t n_seq, const char *const *seq, const uint32_t *seq_len);
/* Build the index on the device from the uploaded reference (construct_index,
 * src/index.c:57-98) and keep it resident.  If lookup_out/occ_out are non-NULL
 * the arrays are also copied back (occ_cap entries available); *n_occ_out is
 * always set.  The result is byte-identical to the reference's index arrays.
 * 1<=k<=15, step>=1; a reference without a sequence of k bases gives an empty index. */
int fem_dev_build_index(fem_dev *h, int32_t k, int32_t step, uint32_t *lookup_out, uint64_t *occ_out,
                        uint64_t occ_cap, uint64_t *n_occ_out);
/* Copies the resident index arrays (uploaded or built) to the host: what save_index
 * writes (src/index.c:133-168).  lookup_out holds 4^k+1 entries, occ_out occ_cap >= n_occ;
 * either may be NULL.  `FEM index` builds once, sizes its buffers from *n_occ_out, then fetches. */
int fem_dev_fetch_index(fem_dev *h, uint32_t *lookup_out, uint64_t *occ_out, uint64_t occ_cap);

/* ---- mapping one batch (replaces the loop body src/map.c:27-49) ---- */
/* submit = stage + map + start of the copy back; wait = finish + result.
 * Two (or more) slots let the transfer of one batch overlap the kernels of another. */
int fem_dev_map_batch_submit(fem_dev *h, int slot, const fem_params *p, const fem_read_batch *reads);
int fem_dev_map_batch_wait(fem_dev *h, int slot, fem_batch_result *out);

/* The same in separate phases. */
/* Copies the caller's batch into the slot's pinned staging buffers (several host threads), checks it
 * (offsets ascending, reads within fem_dev_limits) and starts the asynchronous copy to HBM.  Returns without
 * waiting for the copy; the caller's buffers are free again on return. */
int fem_dev_stage_reads(fem_dev *h, int slot, const fem_read_batch *reads);
/* A batch of equal-length reads crosses the link as two bits per base for the characters A C G T plus, for every other
 * byte (lower case, N, anything), its position and the byte, and is rebuilt byte for byte on the device.  Batches of
 * mixed lengths, or with more than one such byte in sixteen, go as characters + offsets.  FEM_NO_PACK=1 turns the
 * packing off.  fem_dev_stage_info: bytes the slot's last staging (either form) sent to the device, and whether they
 * were packed. */
int fem_dev_stage_info(fem_dev *h, int slot, uint64_t *h2d_bytes, int32_t *packed);
/* A packed batch is seeded (dense indexes) and verified from its codes; its characters are made on the device when a
 * consumer asks for them: the sparse seed kernel, the mapping tail (records, SAM, BAM), never for fem_dev_fetch alone.
 * fem_dev_stage_front: whether the slot's last mapping selected its seeds from the codes, and whether the slot's batch
 * has its characters in device memory.  FEM_TESTING=1 FEM_SELECT_CHARS=1: characters at commit, selection from them. */
int fem_dev_stage_front(fem_dev *h, int slot, int32_t *select_packed, int32_t *chars_ready);
/* Zero-copy form (north_star: "reads streamed in pinned batches"; the reusable SequenceBatch ring of
 * src/input_queue.c:34-51): the library lends the slot's PINNED staging buffers, the FASTQ parser writes the
 * batch straight into them, commit starts the asynchronous H2D copy and returns at once.
 *   acquire: waits until the slot is idle, grows the buffers to n_reads_cap + 1 offsets and n_bases_cap
 *            characters (+ 64 bytes of slack the caller may overrun), returns them; valid until the next acquire.
 *            Once the slot's batch has been fetched (fem_dev_fetch*, fem_dev_sync) the same buffers may be
 *            refilled and committed again without another acquire.
 *   commit:  the batch is complete: n_reads reads, offsets[0] == 0, offsets ascending, offsets[n_reads]
 *            characters, longest read max_len (the parser knows it; no per-read host work happens here).
 *            A wrong max_len / offset table is the caller's bug: the kernels trust them. */
int fem_dev_acquire_stage(fem_dev *h, int slot, uint64_t n_reads_cap, uint64_t n_bases_cap, char **bases,
                          uint64_t **offsets);
int fem_dev_commit_stage(fem_dev *h, int slot, uint64_t n_reads, uint32_t max_len);
/* The same for a batch in which every read has exactly read_len characters (what a sequencer run usually is):
 * read i sits at bases + i * read_len, and the offset table is neither read from the staging buffer nor copied —
 * it is generated on the device (8 of the 108 bytes per 100 bp read that cross the host link otherwise). */
int fem_dev_commit_stage_uniform(fem_dev *h, int slot, uint64_t n_reads, uint32_t read_len);
/* The same for a batch the caller (a FASTQ parser, a sequencer's base caller) already holds at TWO BITS PER BASE — what the
 * device consumes; fem_dev_stage_reads produces this form from characters on the library's host threads, this entry point
 * takes it as it is: no host work per base, a quarter of the bytes over the link.  The reusable batch of
 * src/input_queue.c:34-79 in the form the GPU wants.  Layout inside the `bases` buffer lent by fem_dev_acquire_stage
 * (acquired for n_reads * read_len characters as before):
 *   codes    read i takes bytes [i * bpr, (i + 1) * bpr), bpr = ceil(read_len / 4); base j of a read sits in bits
 *            2 (j & 3) of its byte j / 4; A C G T = 0 1 2 3 (src/utils.h:72); unused bits zero;
 *   at byte exc_offset = n_reads * bpr rounded up to 8:  uint32 pos[n_exceptions], then uint8 chr[n_exceptions] —
 *            every character of the batch that is not one of the upper-case letters A C G T (N, lower case, anything):
 *            its index in the batch (i * read_len + j; its code bits are 0) and the byte itself.  The device rebuilds the
 *            batch byte for byte (the traceback compares characters, src/align.c:289-300).
 * fem_dev_packed_layout: bpr, exc_offset and the most exceptions such a batch may carry (one byte in sixteen, and what
 * the buffer has room for); a batch with more goes through fem_dev_commit_stage_uniform as characters.  Needs no handle.
 * commit_stage_packed checks the exception positions (a wrong one would write outside the batch) and nothing else. */
int fem_dev_packed_layout(uint64_t n_reads, uint32_t read_len, uint32_t *bytes_per_read, uint64_t *exc_offset, uint64_t *exc_cap);
int fem_dev_commit_stage_packed(fem_dev *h, int slot, uint64_t n_reads, uint32_t read_len, uint64_t n_exceptions);
int fem_dev_map_staged(fem_dev *h, int slot, const fem_params *p);          /* kernels only, asynchronous */
int fem_dev_sync(fem_dev *h, int slot);                                     /* wait; re-runs on scratch overflow */
int fem_dev_fetch_stats(fem_dev *h, int slot, uint64_t stats[5]);           /* sync + the five counters */
/* sync + full result to the host.  The arrays are the slot's pinned result buffers: valid until the slot is mapped
 * again (fem_dev_map_staged / fem_dev_map_batch_submit) — behind fem_dev_stage_reads the next batch's arrays are sent
 * home right behind its kernels, so that this call usually finds them there. */
int fem_dev_fetch(fem_dev *h, int slot, fem_batch_result *out);
/* The same outcome as fem_batch_packed (above): a third of the bytes over the link.  Once a slot has been fetched this way
 * its next batches are packed and sent home behind their kernels (as fem_dev_fetch's arrays are behind fem_dev_stage_reads);
 * fem_dev_fetch on the same batch still works (and switches the slot back).  FEM_ERR_UNSUPPORTED if more than 4 096 strands
 * of the batch have 255 candidates or more (-a 0 on a large reference): fem_dev_fetch takes any batch. */
int fem_dev_fetch_packed(fem_dev *h, int slot, fem_batch_packed *out);
/* sync + the mapping tail on the device (replaces process_mappings, src/map.c:50-54 -> src/align.c:56-92, up to
 * the point where the reference packs a bam1_t): sorted records with CIGAR and MD.  Independent of fem_dev_fetch. */
int fem_dev_fetch_records(fem_dev *h, int slot, fem_batch_records *out);

/* ---- SAM text on the device ----
 * upload_reference_names: the @SQ names (first token of every FASTA header), once, next to the reference.
 * acquire_text_stage / commit_text_stage: pinned staging for the batch's quality strings (same offsets as the bases)
 *   and read names (name i = names[name_off[i] .. name_off[i+1])), filled by the parser like the bases; commit after
 *   fem_dev_commit_stage* of the same batch (before or after its fem_dev_map_staged: the copies run on a stream of
 *   the slot's own, beside the batch's kernels, and only the SAM text waits for them), asynchronous.
 * fetch_sam: sync + mapping tail + text, all on the device; one D2H copy of the finished lines. */
int fem_dev_upload_reference_names(fem_dev *h, uint32_t n_seq, const char *names, const uint64_t *name_off);
int fem_dev_acquire_text_stage(fem_dev *h, int slot, uint64_t n_reads_cap, uint64_t n_bases_cap, uint64_t n_name_bytes_cap,
                               char **quals, char **names, uint64_t **name_off);
int fem_dev_commit_text_stage(fem_dev *h, int slot, uint64_t n_reads, uint64_t n_name_bytes);
/* The same without the qualities (the staging's `quals` need not be filled): they stay with the caller.  With the text from
 * the device 228 of the 473 bytes per 100-bp read on the link are the qualities going to the device and coming back unchanged;
 * this form sends none up and the SAM text comes back with the QUAL field of every read's first record sized but NOT WRITTEN.
 * fem_dev_sam_quals (once the text is home: after fem_dev_fetch_sam / fem_dev_sam_wait) gives qual_at[n_reads]: where in the
 * text read r's field starts, UINT64_MAX for a read without a record (fem_dev_set_unmapped: such a read has a line, and its
 * field's start stands here like any other's); the caller copies each read's quality string there
 * (libfemhost's fem_sam_fill_quals does it on several threads) before it uses the text.  Pinned memory of the slot, valid until
 * the slot's next SAM text. */
int fem_dev_commit_names_stage(fem_dev *h, int slot, uint64_t n_reads, uint64_t n_name_bytes);
int fem_dev_sam_quals(fem_dev *h, int slot, const uint64_t **qual_at, uint64_t *n_reads);
/* Optional: device and pinned buffers of the slot for batches of this shape and `text_bytes` of SAM text, allocated now
 * (pinning host memory costs ~0.25 ms per MB; otherwise the first batch of every slot pays for it).  With fem_dev_set_xa a primary
 * line grows by up to 6 + FEM_XA_MAX_BYTES bytes while the secondary lines it stands for go: the text as a whole gets no larger. */
int fem_dev_reserve_text(fem_dev *h, int slot, uint64_t n_reads, uint64_t n_bases, uint64_t n_name_bytes, uint64_t text_bytes);
/* Optional, after the index is resident: everything else a batch of up to n_reads reads of up to max_len characters with up
 * to n_records mappings allocates in this slot on its way through fem_dev_map_staged and fem_dev_fetch_records /
 * fem_dev_fetch_sam (per-read and per-candidate arrays, the selection's hand-over, the mapping tail's thirty arrays) —
 * otherwise the first batch of every slot makes these allocations between its kernels (FEM map, 16 M reads: 20 of the job's
 * 145 ms).  Larger batches still grow what they need. */
int fem_dev_reserve_batch(fem_dev *h, int slot, uint64_t n_reads, uint64_t n_records, uint32_t max_len, const fem_params *p);
int fem_dev_fetch_sam(fem_dev *h, int slot, fem_batch_sam *out);
/* The same, returning as soon as the copy of the text to the host is queued: out->text must not be read before
 * fem_dev_sam_wait(h, slot) has returned — the one call that may be made from another thread than the one driving
 * the handle (a writer thread waits there while the GPU's thread starts on the next batch). */
int fem_dev_fetch_sam_nowait(fem_dev *h, int slot, fem_batch_sam *out);
int fem_dev_sam_wait(fem_dev *h, int slot);

/* ---- BAM output (new: the reference writes SAM only) ----
 * fem_dev_fetch_bam: the lines fem_dev_fetch_sam would render, as BAM records (SAM/BAM specification 4.2), compressed on the
 *   device into BGZF members (4.1) of whole records, each cut greedily at 65280 input bytes.  data holds the members only: no
 *   BAM header (fem_bam_header of libfemhost, compressed with fem_dev_bgzf_compress), no EOF block.  raw_len = bytes of the
 *   uncompressed records, n_blocks = members.  level 1: deflate with dynamic Huffman codes, a member stored where that is not
 *   larger; level 0: stored members.  n_records, n_asserted and stats are fem_dev_fetch_sam's.  Lifetime, threads, pair mode
 *   and rescue as fem_dev_fetch_sam / _nowait / fem_dev_sam_wait (the data shares the text's pinned memory).
 *   Encoding: refID pos = the record's tid pos0; l_read_name = name + 1; MAPQ 255 (fem_dev_set_mapq: its rule); bin = reg2bin(pos0, end0) with end0 = pos0 +
 *   the M/D/N/=/X lengths (pos0 + 1 for none); CIGAR as the device's words; FLAG & 0x7FFF (0x8000 still counted in n_asserted);
 *   l_seq = L where the text prints SEQ, else 0; next_refID next_pos tlen = -1 -1 0, or the pair's mate columns; SEQ in 4-bit
 *   codes of the letters the text prints; QUAL - 33; aux NM:C then MD:Z.
 *   FEM_ERR_STATE after fem_dev_commit_names_stage (the qualities must be on the device); FEM_ERR_UNSUPPORTED for a read name
 *   over 254 characters; FEM_ERR_INVALID for a level other than 0 or 1.
 * fem_dev_bgzf_compress: any n bytes into BGZF members cut every 65280 bytes (n = 0: nothing, *out_len = 0); FEM_ERR_INVALID
 *   when they do not fit in out_cap (65536 bytes per started 65280 always do). */
typedef struct {
  const uint8_t *data;
  uint64_t len, raw_len, n_blocks, n_records, n_asserted;
  uint64_t stats[5];
} fem_batch_bam;
int fem_dev_fetch_bam(fem_dev *h, int slot, int level, fem_batch_bam *out);
int fem_dev_fetch_bam_nowait(fem_dev *h, int slot, int level, fem_batch_bam *out);
int fem_dev_bam_wait(fem_dev *h, int slot);
int fem_dev_bgzf_compress(fem_dev *h, const void *in, uint64_t n, int level, void *out, uint64_t out_cap, uint64_t *out_len);

/* ---- read pairs (new: the reference maps single-end reads only) ----
 * fem_dev_set_pairs: the slot's batches are read pairs from now on: read i and read n_reads/2 + i are the two mates of pair i
 *   (mate 1's reads first, then mate 2's, in the same order).  NULL: single-end again.  FEM_ERR_INVALID for min_insert < 0,
 *   max_insert < min_insert, max_insert > 2^30.
 * In pair mode fem_dev_fetch_sam / fem_dev_fetch_sam_nowait render the paired text: pairs in batch order, mate 1's lines then
 *   mate 2's, the chosen combination's records first (below), FLAG with 0x1 0x2 0x8 0x20 0x40 0x80, RNEXT PNEXT TLEN filled.
 *   The qualities may stay on the host as in single-end mode (fem_dev_commit_names_stage -> fem_dev_sam_quals: qual_at per read,
 *   numbered as staged).  fem_dev_fetch, fem_dev_fetch_packed, fem_dev_fetch_records and fem_dev_fetch_stats keep their
 *   single-end meaning over the n_reads reads.  An odd n_reads is FEM_ERR_INVALID at fetch time.
 * Pairing: the records of each mate as single-end mode makes them, lists A and B.  (a, b) is concordant when neither carries
 *   0x8000, both lie on one sequence on opposite strands, the forward one f starts at or before the reverse one r, and
 *   min_insert <= end0(r) - pos0(f) <= max_insert (end0 = pos0 + the M and D lengths of the CIGAR: the insert).  The chosen
 *   combination has the least nm(a) + nm(b), ties to the smaller index in A, then in B; a pair with one is a proper pair.
 * A paired batch's call order: fem_dev_acquire_stage + fem_dev_acquire_text_stage, the parser fills mate 1's reads then mate
 *   2's (offsets and name offsets running on), fem_dev_commit_stage*, fem_dev_map_staged, fem_dev_commit_text_stage (or
 *   _names_stage), fem_dev_fetch_sam[_nowait] (+ fem_dev_sam_wait), fem_dev_pair_count. */
typedef struct {
  int32_t min_insert, max_insert;
} fem_pair_params;
int fem_dev_set_pairs(fem_dev *h, int slot, const fem_pair_params *pp);
/* The records of the slot's batch in paired output order.  Same lifetime as fem_batch_records.  FEM_ERR_STATE without pair mode. */
typedef struct {
  uint64_t n_pairs, n_records;
  const uint32_t *rec_begin; /* 2*n_pairs+1: mate m (0, 1) of pair i has records [rec_begin[2i+m], rec_begin[2i+m+1]), primary first */
  const uint16_t *flag;      /* the full SAM flag as written (0x8000 kept as in fem_batch_records) */
  const uint32_t *tid, *pos0;
  const uint8_t *nm;
  const uint32_t *cigar_off, *cigar, *md_off;
  const char *md;
  const uint32_t *mate_tid, *mate_pos0; /* 0xFFFFFFFF: the other mate has no record */
  const int32_t *tlen;
  uint64_t n_proper;
  uint64_t stats[5];
} fem_batch_pairs;
int fem_dev_fetch_pairs(fem_dev *h, int slot, fem_batch_pairs *out);
/* Proper pairs of the slot's last paired SAM text (valid once fem_dev_fetch_sam[_nowait] has returned) or fem_dev_fetch_pairs. */
int fem_dev_pair_count(fem_dev *h, int slot, uint64_t *n_proper);

/* ---- the insert size range, learned from a batch (new; it changes nothing: a caller takes the range and sets it) ----
 * fem_dev_estimate_insert: what the slot's batch of read pairs says about the library's insert sizes, from the single-end
 *   records fem_dev_fetch_records makes (which it runs: sync + mapping tail), on the device.  FEM_ERR_STATE without pair mode,
 *   FEM_ERR_INVALID for a null out or, at fetch time, an odd n_reads.  It needs no text stage and no reference names, changes
 *   none of the slot's options and none of its counts: a fem_dev_fetch_sam, _bam or _pairs of the same batch afterwards gives
 *   what it gives without the call.  The slot's own min_insert / max_insert play no part.
 * Rule (integers throughout).  Over the pairs of the batch (read i and read n_reads/2 + i):
 *   1. A pair is unique when each mate has exactly one record and neither record carries 0x8000.
 *   2. A unique pair is informative when both records lie on one sequence on opposite strands, the forward one f starts at or
 *      before the reverse one r (pos0(f) <= pos0(r)) and ins = end0(r) - pos0(f) <= FEM_INSERT_MAX (end0 = pos0 + the M and D
 *      lengths of the CIGAR): the pairing rule above with the range 0 .. FEM_INSERT_MAX.
 *   3. v[0..n) the informative inserts in ascending order: q25 = v[(n - 1) / 4], q50 = v[2 (n - 1) / 4], q75 = v[3 (n - 1) / 4]
 *      (integer division); iqr = q75 - q25.  n == 0: the three are -1.
 *   4. estimated = n >= FEM_INSERT_MIN_PAIRS; then min_insert = max(0, q25 - 3 iqr), max_insert = q75 + 3 iqr (the quartile
 *      fence; max_insert - min_insert <= 65532, so fem_dev_set_rescue's window limit holds for a learned range).  Else both
 *      are 0 and mean nothing. */
#define FEM_INSERT_MAX 16383
#define FEM_INSERT_MIN_PAIRS 64
typedef struct {
  uint64_t n_pairs, n_unique, n_informative;
  int32_t q25, q50, q75;
  int32_t min_insert, max_insert;
  int32_t estimated;
} fem_insert_estimate;
int fem_dev_estimate_insert(fem_dev *h, int slot, fem_insert_estimate *out);

/* ---- the library's orientation (new; the default, FR, is every rule above as it stands) ----
 * fem_dev_set_orientation: a slot option of its own, FEM_ERR_INVALID for anything but the three values.  It takes effect in pair
 *   mode and stays through fem_dev_set_pairs calls, as the other fem_dev_set_* options do.
 * Rule.  An orientation is a pair of flip bits (flip1, flip2) for mate 1 and mate 2:
 *     FEM_ORIENT_FR  0 0  forward mate upstream, reverse mate downstream, facing each other
 *     FEM_ORIENT_RF  1 1  the reverse-strand mate starts at or before the forward-strand one (the mates point away from each other)
 *     FEM_ORIENT_FF  0 1  mate 1 forward upstream of mate 2 forward, or the whole fragment on the other strand: both reverse,
 *                         mate 2 upstream of mate 1
 *   The virtual strand of a record of mate m is its strand (FLAG & 16) XOR flip_m.  Every rule of pair mode is kept word for
 *   word with "strand" read as "virtual strand":
 *   Pairing.  (a, b) is concordant when neither carries 0x8000, both lie on one sequence, their virtual strands differ, the
 *     virtually forward one f has pos0(f) <= pos0(r), and min_insert <= end0(r) - pos0(f) <= max_insert.  The choice (least NM
 *     sum, ties to the smaller a, then b) is unchanged.  TLEN is +ins on f's primary line and -ins on r's: f is the leftmost
 *     starting mate in all three orientations, at equal pos0 the virtually forward one.  FLAG 0x10 and 0x20, RNEXT and PNEXT
 *     stay the real strands and places.  fem_dev_set_mapq's pair term counts the concordant combinations of this rule.
 *   Rescue (fem_dev_set_rescue, fem_dev_set_rescue_discordant).  For an anchor of mate m_a and the searched mate m_b:
 *     v = strand(anchor) XOR flip_{m_a}; the window is the rule's below with v for the anchor's strand; B is searched
 *     reverse-complemented iff (v is forward) XOR flip_{m_b}; the traced record carries FLAG 16 iff B was reverse-complemented;
 *     it is kept iff start >= 0 and it is concordant with its anchor by the rule above, on its real CIGAR span.  Tiles, the
 *     key, the anchor limit, the order of the directions and of the appended records are untouched.
 *   fem_dev_estimate_insert follows the slot's orientation: informative = concordant by the rule above within
 *     0 .. FEM_INSERT_MAX.  A unique pair at equal pos0 on opposite strands is informative under FR and under RF.
 * fem_dev_estimate_library: one pass over the batch, the three estimates side by side: by[O] is what fem_dev_estimate_insert
 *   gives with orientation O set (n_pairs and n_unique are the same in all three).  orientation = the O with the most
 *   informative pairs among those with estimated = 1, ties in the order FR, RF, FF; -1 when none reaches FEM_INSERT_MIN_PAIRS.
 *   Preconditions, errors and the promise that the slot's options and counts stay as they are: fem_dev_estimate_insert's. */
#define FEM_ORIENT_FR 0
#define FEM_ORIENT_RF 1
#define FEM_ORIENT_FF 2
int fem_dev_set_orientation(fem_dev *h, int slot, int orientation);
typedef struct {
  fem_insert_estimate by[3];
  int32_t orientation;
} fem_library_estimate;
int fem_dev_estimate_library(fem_dev *h, int slot, fem_library_estimate *out);

/* ---- mate rescue (new; opt-in: with it off every paired output stays byte for byte what it is without it) ----
 * fem_dev_set_rescue: the slot's read pairs are rescued at max_edits = E edits (0 <= E <= 15, else FEM_ERR_INVALID); NULL: off.
 *   It takes effect with pair mode (fem_dev_set_pairs); fetch time refuses max_insert - min_insert > 65536 (FEM_ERR_UNSUPPORTED).
 * Rule.  A pair is a candidate when exactly one mate, B (length L), has no record.  A mate of length 0 is never searched (every
 *   window would "hit" it at 0 edits with an empty CIGAR): such a pair stays as it is and B stays unmapped.  The anchors are those
 *   of the other mate's first FEM_RESCUE_ANCHORS records that do not carry 0x8000.  Per anchor a (sequence tid, pa = pos0, ea = end0, signed
 *   arithmetic), the window of B's pos0 is
 *     anchor forward: B reverse-complemented, lo = max(pa, pa + I - L), hi = pa + X - L;
 *     anchor reverse: B forward,             lo = max(0, ea - X),         hi = min(pa, ea - I);      none when lo > hi
 *   (I, X = min_insert, max_insert).  Tiles c_j = lo + j (2E + 1) <= hi, skipped where c_j + L + 2E exceeds the sequence; tile c
 *   runs the banded Myers of the mapping (fo_banded_ed32: one 32-bit word, first strict minimum) at E over ref[c, c + L + 2E)
 *   and hits when ed <= E and pos0 = c + end - L + 1 <= hi.  Each anchor keeps its least (ed, pos0); the pair takes the least
 *   (nm(a) + ed, a); that hit is traced at E (the traceback of the mapping) into a record: FLAG 16 if B was reverse-complemented
 *   else 0, the anchor's tid, pos0 = c + start, NM = ed, CIGAR and MD.  It is kept only if start >= 0 and it is concordant with
 *   its anchor (the pairing rule above, the real CIGAR span); a kept record is B's only record, otherwise the pair stays as it
 *   is (no fall-back to another anchor).
 * Pairing then runs unchanged on the extended lists (the rescued pair is a proper one, counted by fem_dev_pair_count), and
 *   fem_batch_pairs holds the rescued records like any other.  fem_dev_fetch_records and the stats keep their single-end meaning.
 * fem_dev_rescue_count: kept rescued records of the slot's last paired text or fem_dev_fetch_pairs (valid when
 *   fem_dev_pair_count is); 0 with rescue off. */
#define FEM_RESCUE_ANCHORS 8
typedef struct {
  int32_t max_edits;
} fem_rescue_params;
int fem_dev_set_rescue(fem_dev *h, int slot, const fem_rescue_params *rp);
int fem_dev_rescue_count(fem_dev *h, int slot, uint64_t *n_rescued);

/* ---- mate rescue for pairs whose records do not pair (new; opt-in: with it off, or with rescue off, every output stays byte
 *      for byte what it is without it) ----
 * fem_dev_set_rescue_discordant: on != 0: where pair mode and fem_dev_set_rescue are on, a pair is a candidate in two ways.
 *   Kind 1 (as above): exactly one mate has no record; nothing about it changes.
 *   Kind 2: both mates have at least one record and no combination (a, b) of their records is concordant (the pairing rule
 *   above; records with 0x8000 never pair).
 * Rule for kind 2.  Both directions are searched: d = 0, B is mate 2 and the anchors are mate 1's first FEM_RESCUE_ANCHORS
 *   records without 0x8000; d = 1, B is mate 1 and the anchors are mate 2's.  Per direction and anchor the rule above applies
 *   unchanged (window, strand, tiles, the banded Myers at E, the hit test, the least (ed, pos0) per anchor).  The pair takes the
 *   least (nm(anchor) + ed, d, anchor index); that one hit is traced at E and kept only if start >= 0 and the record is
 *   concordant with its anchor by its real CIGAR span; there is no fall-back to another anchor or to the other direction.
 *   A kept record is added to B's list behind B's own records, which all stay.  Pairing then runs by its unchanged rule on the
 *   lists: B's own records pair with nothing, so the chosen combination is (some a, the rescued record), the a of the least nm
 *   sum, ties to the smaller a (not necessarily the anchor), and the pair is a proper one.  B's lines are the rescued record
 *   first (0x2, TLEN, no 0x100), then its own records in their order with 0x100.  For MAPQ the rescued record is "rescued": q_x
 *   = 0, so B's primary line gets min(qp, 40).
 *   A rescued hit can lie at the place of one of B's own records whose own traceback span put it just outside [I, X]: no merge
 *   by locus is done.  No second pass starts from a rescued mate.
 * fem_dev_rescue_count counts every kept record, of either kind; fem_dev_rescue_discordant_count those of kind 2 (valid when
 *   fem_dev_rescue_count is; 0 with the switch or rescue off).  fem_dev_fetch_records and the stats keep their single-end meaning. */
int fem_dev_set_rescue_discordant(fem_dev *h, int slot, int on);
int fem_dev_rescue_discordant_count(fem_dev *h, int slot, uint64_t *n);

/* ---- mapping qualities (new; opt-in: the reference prints MAPQ 255, "not available", and so does every output without it) ----
 * fem_dev_set_mapq: on != 0: the slot's fem_dev_fetch_sam[_nowait] text and fem_dev_fetch_bam[_nowait] records carry MAPQ from
 *   the hit strata below; 0: 255 again.  fem_batch_records and fem_batch_pairs are unchanged (MAPQ is output text only).
 * Rule.  Q(g, c) = min(60, max(0, 20 g - 3 floor(log2 c))) for a gap of g >= 1 edits and c >= 1 alternatives (20 per edit of
 *   gap, 3 = 10 log10 2 per doubling of the alternatives, capped at 60), in integers: floor(log2 c) = 31 - clz(c).
 *   Single-end value of read r, mapped at -e e, from its records as single-end mapping makes them (NM non-decreasing; every
 *   record counts, 0x8000 included, none merged by locus): d1 = NM of the first record, c1 = records with NM = d1.  c1 >= 2:
 *   q_se(r) = 0.  Else d2 = the least NM above d1 and c2 = records with NM = d2, or d2 = e + 1 and c2 = 1 when there is none;
 *   q_se(r) = Q(d2 - d1, c2).
 *   Single-end lines: a read's primary line gets q_se(r), every other line 0.
 *   Pair mode (fem_dev_set_pairs, with or without rescue; a rescued record is its mate's only record).  Not a proper pair:
 *   each mate's primary line gets q_se(mate), every other line 0.  Proper pair with chosen combination (a, b): s1 = nm(a) +
 *   nm(b), cp1 = concordant combinations with sum s1, s2 = the least concordant sum above s1, cp2 = how many have it; qp = 0
 *   if cp1 >= 2, 60 if there is no s2, else Q(s2 - s1, cp2).  For the chosen record x of a mate, q_x = q_se(mate) if x is
 *   not rescued and nm(x) = d1(mate), else 0; the mate's primary line gets max(q_x, min(qp, q_x + 40)), every 0x100 line 0.
 *   "Concordant" is the pairing rule above. */
int fem_dev_set_mapq(fem_dev *h, int slot, int on);

/* ---- lines for unmapped reads (new; opt-in: the reference drops a read without a mapping, and so does every output without it) ----
 * fem_dev_set_unmapped: on != 0: the slot's fem_dev_fetch_sam[_nowait] text and fem_dev_fetch_bam[_nowait] records carry one
 *   line for every unmapped read; 0: none again.  fem_batch_sam / fem_batch_bam keep their layout and n_records keeps meaning
 *   mapping records: lines = n_records (+ the rescued mates in pair mode) + fem_dev_unmapped_count.  fem_batch_records and
 *   fem_batch_pairs are unchanged (as with MAPQ, this is output text only; mate_tid there stays 0xFFFFFFFF).
 * Rule.  A read is unmapped when, after single-end mapping and (pair mode with rescue) after mate rescue, it has no record.
 *   It gets exactly one line, where its records would have stood: single-end in batch read order between its neighbours'
 *   lines; in pair mode in the pair's slot (mate 1's lines, then mate 2's).  Mapped reads keep their lines.
 *   Single-end, and a pair with both mates unmapped, the unplaced line: QNAME as on a mapped line; FLAG 4 (pairs: 0x1 | 0x4 |
 *   0x8 | 0x40 = 77 for mate 1, 0x1 | 0x4 | 0x8 | 0x80 = 141 for mate 2); RNAME * POS 0; MAPQ 0, with and without
 *   fem_dev_set_mapq (never 255); CIGAR *; RNEXT * PNEXT 0 TLEN 0; SEQ and QUAL the read as given (forward) through the letter
 *   table and quality handling of a mapped read's primary line (* and * for a read of length 0; with
 *   fem_dev_commit_names_stage QUAL is sized, not written, and qual_at[r] says where); no tags: the line ends after QUAL.
 *   A pair with one mapped mate A and one unmapped mate B, the placed line (the SAM specification's recommended practice).
 *   a0 = A's first line (no combination was chosen for such a pair: A's first single-end record), on sequence t at pos0 p.
 *   B's line: FLAG 0x1 | 0x4 | 0x40 or 0x80, | 0x20 when a0 is reverse; RNAME t, POS p + 1; MAPQ 0; CIGAR *; RNEXT =, PNEXT
 *   p + 1; TLEN 0; SEQ and QUAL forward as given; no tags.  A's lines keep 0x8 and everything else they have without the
 *   switch, except RNEXT PNEXT (there * 0), which name where B was placed: RNEXT = where the line's own sequence is t, else
 *   t's name; PNEXT p + 1.  TLEN stays 0; the pair is not proper and not counted as one.  With fem_dev_set_mapq A's lines get
 *   what they get without the switch, B's line 0.
 *   BAM records are these lines field for field in the encoding above: refID pos -1 -1 and bin 4680 unplaced; t, p and
 *   reg2bin(p, p + 1) placed; n_cigar_op 0; l_seq L with the 4-bit SEQ and QUAL - 33; no aux.
 * fem_dev_unmapped_count: the lines for unmapped reads in the slot's last text or BAM (valid once the fetch has returned);
 *   0 with the switch off. */
int fem_dev_set_unmapped(fem_dev *h, int slot, int on);
int fem_dev_unmapped_count(fem_dev *h, int slot, uint64_t *n);

/* ---- the line filter: best strata and a hit limit per read (new; opt-in: the reference writes every mapping, and so does every
 *      output without it) ----
 * fem_dev_set_report: the slot's fem_dev_fetch_sam[_nowait] text and fem_dev_fetch_bam[_nowait] records leave out the lines the
 *   rule below drops.  strata S: 0 .. 15, or -1 for off; max_hits N: 1 .. 2^31 - 1, or -1 for off; rp == NULL: both off.  Anything
 *   else is FEM_ERR_INVALID.  With both off nothing changes.  fem_batch_records, fem_batch_pairs, the stats and
 *   fem_dev_pair_count / fem_dev_rescue_count / fem_dev_unmapped_count are unchanged (as MAPQ and the unmapped reads' lines, this
 *   is output text only).  n_records of fem_batch_sam / fem_batch_bam counts the mapping records whose lines are there: lines =
 *   n_records (+ the rescued mates in pair mode) + fem_dev_unmapped_count, as without the filter.  qual_at of
 *   fem_dev_sam_quals still points at each read's primary QUAL field (a primary line always stays).
 * Rule.  The filter acts on LINES, after everything else has been decided: the single-end order, rescue, pairing, MAPQ, the line
 *   of an unmapped read.  It only removes lines: a line that stays is byte for byte what it is without the filter (FLAG, MAPQ,
 *   RNEXT / PNEXT / TLEN, NM, MD), the primary line stays the primary line, and the proper-pair, rescued and unmapped counts
 *   are what they are without it.  The filtered output is the unfiltered output minus some lines, in the same order.
 *   A slot is a read single-end, or one mate of a pair.  Its lines in output order are l_0 .. l_{c-1}; l_0 is the primary line
 *   (in a proper pair the chosen record, which need not have the mate's least NM); d = the least NM over ALL of the slot's lines
 *   (records with 0x8000 count, as for MAPQ).  l_0 is always kept.  A later line l_t (t >= 1) is kept iff
 *     (S off or nm(l_t) <= d + S)  and  (N off or fewer than N lines of the slot have been kept before it, l_0 included).
 *   So N = 1 leaves one line per mapped read, and a slot of one line (a rescued mate's record; with fem_dev_set_unmapped an
 *   unmapped read's line) keeps it.  The placed line of an unmapped mate and its mate's RNEXT / PNEXT name the mapped mate's
 *   first line, which is l_0 and there.  NM is NOT assumed to be non-decreasing along a slot's lines (in pair mode it is not).
 * fem_dev_filtered_count: the lines left out of the slot's last text or BAM (valid once the fetch has returned); 0 with the
 *   filter off. */
typedef struct {
  int32_t strata;   /* 0 .. 15, -1: off */
  int32_t max_hits; /* >= 1, -1: off */
} fem_report_params;
int fem_dev_set_report(fem_dev *h, int slot, const fem_report_params *rp);
int fem_dev_filtered_count(fem_dev *h, int slot, uint64_t *n);

/* ---- read-group and hit-count tags: RG:Z, NH:i, HI:i (new; opt-in: the reference writes NM and MD alone, and so does every output
 *      without it) ----
 * fem_dev_set_tags: the lines of the slot's fem_dev_fetch_sam[_nowait] text and the records of its fem_dev_fetch_bam[_nowait]
 *   carry further optional fields behind the last one they have.  read_group: the ID, NUL-terminated, 1 .. 255 bytes of [ -~]
 *   (copied at the call: the caller's string need not live on), or NULL for no RG tag; hit_tags != 0: NH and HI; tp == NULL: all
 *   off.  An empty or over-long ID, or a byte outside [ -~], is FEM_ERR_INVALID and leaves the slot's setting as it was.  With
 *   all off nothing changes.  fem_batch_records, fem_batch_pairs, the stats, n_records and every count are unchanged (output
 *   text only).  The tags stand behind QUAL, so qual_at of fem_dev_sam_quals still points at each read's QUAL field.
 * Rule.  The tags are added to LINES, after everything else has been decided: the single-end order, rescue, pairing, MAPQ, the
 *   lines of unmapped reads, the line filter.  Every byte in front of them is what it is without them.
 *   Field order on a mapped line: NM:i MD:Z NH:i HI:i RG:Z.  The line of an unmapped read (fem_dev_set_unmapped) carries RG:Z
 *   alone, behind QUAL, and never NH / HI.
 *   RG:Z:<ID> stands on every line: primary, secondary, 0x8000 record, rescued mate, unmapped read.
 *   A slot is a read single-end, or one mate of a pair (the slot of fem_dev_set_report).  NH of a mapped line is the number of
 *   lines of its slot that ARE IN THE OUTPUT: after rescue, pairing and the line filter; lines whose record carries 0x8000
 *   count, as they do for MAPQ and the filter.  HI is the line's 1-based place among its slot's lines in output order, so the
 *   primary line has HI 1.  A rescued mate's record has NH 1 HI 1.  With max_hits 1 every mapped line has NH 1: NH states what is
 *   in the file, not what was found.
 *   BAM: NH and HI are type I (uint32, seven bytes each whatever the value), RG is type Z (the ID and a NUL); block_size
 *   includes them; an unmapped read's record has the RG aux alone. */
typedef struct {
  const char *read_group; /* the ID, NUL-terminated, 1..255 bytes of [ -~]; NULL: no RG tag */
  int32_t hit_tags;       /* != 0: NH:i and HI:i on every mapped line */
} fem_tag_params;
int fem_dev_set_tags(fem_dev *h, int slot, const fem_tag_params *tp);

/* ---- mate tags: MC:Z, MQ:i, ms:i (new; opt-in: what `samtools fixmate -m` would add in a pass of its own, here written with the
 *      line) ----
 * fem_dev_set_mate_tags: on != 0: every line of the slot's fem_dev_fetch_sam[_nowait] text and every record of its
 *   fem_dev_fetch_bam[_nowait] IN PAIR MODE (fem_dev_set_pairs) carries the three tags below behind every field it has without
 *   them; 0: none, every byte as before.  A single-end slot is unchanged by the setting.  fem_batch_records, fem_batch_pairs, the
 *   stats, n_records and every count are unchanged (output text only).
 *   ms is made from the qualities on the device: a fetch of a text or of BAM records with the setting on in pair mode and the
 *   slot's qualities kept on the host (fem_dev_commit_names_stage) is FEM_ERR_INVALID.  (Leaving ms out silently would be worse.)
 *   fem_dev_reserve_text: a line grows by up to 6 + the mate's CIGAR, 6 + 3 and 6 + 6 bytes.
 * Rule.  A slot is one mate of a pair (slot 2i + m, as for fem_dev_set_report); its other mate is slot s ^ 1.  The other mate's
 *   PRIMARY LINE is the first of its lines as the pairing made them: in a proper pair the chosen record, otherwise the first
 *   single-end record, or the rescued one (where a line of an unmapped mate is placed, fem_dev_set_unmapped).  The primary line
 *   is always in the output, whatever the line filter does.  Every line of a slot carries the same values, in this order:
 *   MC:Z:<cigar>  iff the other mate has a record and its primary line's CIGAR column is not "*" (a primary record with 0x8000
 *     prints "*": no MC then): that column, byte for byte.
 *   MQ:i:<n>      iff the other mate has a record: what its primary line prints in its MAPQ column (255 without fem_dev_set_mapq).
 *   ms:i:<n>      iff the batch has qualities on the device (where QUAL prints "*" for lack of them, there is no ms): the sum over
 *     the other mate's quality bytes b of b - 33 where b - 33 >= 15; bytes below 48 add nothing; a read of length 0 gives 0.  The
 *     other mate need not be mapped.  (As far as known what `samtools fixmate -m` computes; this rule is the specification.)
 *   Field order on a mapped line: NM:i MD:Z [NH:i HI:i] [RG:Z] [MC:Z] [MQ:i] [ms:i]; on the line of an unmapped read
 *   (fem_dev_set_unmapped): [RG:Z] [MC:Z MQ:i] [ms:i] behind QUAL, MC and MQ when its mate is mapped (the placed line), ms alone
 *   for a pair of which nothing maps.  Secondary lines are tagged like the primary one, as RNEXT and PNEXT are.  The tags stand
 *   behind QUAL, so qual_at of fem_dev_sam_quals is unchanged.
 *   BAM: MC is type Z (the characters and a NUL), MQ type C (four bytes), ms type I (uint32, seven bytes whatever the value, as NH
 *   and HI); block_size includes them. */
int fem_dev_set_mate_tags(fem_dev *h, int slot, int on);

/* ---- SEQ and QUAL as SAM orders them (new; opt-in: the reference prints every read as it came from the sequencer, src/align.c:79,
 *      also on lines with FLAG 0x10, and so does every output without it) ----
 * fem_dev_set_sam_seq: on != 0: the lines of the slot's fem_dev_fetch_sam[_nowait] text and the records of its
 *   fem_dev_fetch_bam[_nowait] that the rule below names print the read in the reference's direction, as POS, CIGAR, NM and MD of
 *   the same line already are; 0: every byte as before.  Per slot and sticky, as the other options.  fem_batch_records and
 *   fem_batch_pairs carry no SEQ and are unchanged, as are the stats, n_records and every count (output text only).
 *   QUAL is reversed where it is written, on the device: a fetch of a text with the setting on and the slot's qualities kept on the
 *   host (fem_dev_commit_names_stage, where the caller fills the QUAL holes forward) is FEM_ERR_INVALID.  Both ways of staging the
 *   bases serve it (characters, and the 2-bit packed transfer).
 * Rule.  A line or record changes only if its FLAG AS WRITTEN has 0x10 and it carries SEQ: a read's primary line in single-end
 *   output; a line without 0x100 in paired output, rescued mates' lines included.  A record with 0x8000 follows the same rule by
 *   its 0x10 bit.  On such a line, L being the read's length:
 *   SEQ   character i is the complement of character L - 1 - i of what is printed without the setting, that is, after the letter
 *     table of the 4-bit round trip (IUPAC letters upper-cased, anything else N).  The complement maps the sixteen letters
 *     =ACMGRSVTWYHKDBN to =TGKCYSBAWRDMHVN: the 4-bit BAM code with its bits reversed (htslib's table).  So a -> A -> T and
 *     . -> N -> N.
 *   QUAL  byte i is byte L - 1 - i.  A QUAL printed as * stays *.
 *   BAM   the same letters as 4-bit codes packed from the reversed order: byte k holds positions 2k and 2k + 1 of the reversed
 *     read, the low nibble of the last byte of an odd L is 0; qual - 33 is reversed (0xFF stays 0xFF); l_seq, block_size and bin
 *     are unchanged.
 *   Nothing else changes: no line or record changes its length, no offset, count or counter changes, no forward-strand line, no
 *   secondary line (* and *), no line of an unmapped read, placed or not (it has no 0x10, whatever 0x20 says, and stays as
 *   sequenced), no tag (ms:i is a sum).  FLAG 0x10 is the real strand under every fem_dev_set_orientation. */
int fem_dev_set_sam_seq(fem_dev *h, int slot, int on);

/* ---- secondary hits folded into XA:Z on the primary line (new; opt-in: the reference writes a line of its own for every mapping,
 *      and so does every output without it) ----
 * fem_dev_set_xa: max_entries N: 0 is off, every byte as before; 1 .. 2^31 - 1 is on with at most N entries per slot; a negative
 *   value is FEM_ERR_INVALID.  Per slot and sticky, as the other options.  It applies to the slot's fem_dev_fetch_sam[_nowait] text
 *   and fem_dev_fetch_bam[_nowait] records, single-end and in pair mode, with both ways of staging the bases and with the qualities
 *   on the device or kept on the host (fem_dev_commit_names_stage: XA stands behind QUAL and needs no quality).  It adds no refusal.
 *   fem_dev_reserve_text: a primary line grows by up to 6 + FEM_XA_MAX_BYTES bytes (and the secondary lines it stands for go).
 * Rule.  Folding acts on LINES, after everything else has been decided: the single-end order, rescue, pairing, MAPQ, the lines of
 *   unmapped reads, the line filter, and every other tag.  A slot is a read single-end, or one mate of a pair (the slot of
 *   fem_dev_set_report).  Its lines in output order are l_0 .. l_{c-1}; l_0 is the primary line, the only line of the slot without
 *   FLAG 0x100; an unmapped read's line is a slot with c = 1.
 *   Entry.  The entry of a secondary line l_t is <RNAME>,<s><POS>,<CIGAR>,<NM>; where RNAME, POS and CIGAR are the bytes of those
 *     columns as l_t prints them (a record with 0x8000 prints * for CIGAR), <s> is - if l_t's FLAG as written has 0x10, else +
 *     (the real strand under every fem_dev_set_orientation), and <NM> is the digits of its NM:i.  len_t is the entry's byte count.
 *   How many fold.  With B = FEM_XA_MAX_BYTES, f is the largest f <= min(c - 1, N) with len_1 + .. + len_f <= B.  The folded lines
 *     are always the prefix l_1 .. l_f of the secondary lines.
 *   f = 0: the slot's lines are byte for byte as without the option (so a slot of one line never carries XA).
 *   f >= 1: l_1 .. l_f are not written; l_0 is written byte for byte as without the option plus one last field, a tab, XA:Z: and the
 *     f entries in order; l_{f+1} .. l_{c-1} are written byte for byte as without the option.
 *   Field order on a mapped line: NM:i MD:Z [NH:i HI:i] [RG:Z] [MC:Z] [MQ:i] [ms:i] [XA:Z].  XA carries no MD: that is the format.
 *   Unchanged: every byte in front of XA; the values of NH / HI on every line that stays (a folded hit is still a reported hit, so
 *     a line keeps the numbers it has without the option); MAPQ, the mate columns, SEQ and QUAL, hence qual_at of
 *     fem_dev_sam_quals; the order of everything that stays; fem_batch_records, fem_batch_pairs and the five stats; the proper,
 *     rescued, unmapped and filtered counts; n_asserted (a folded 0x8000 record is still counted); n_records, which counts the
 *     mapping records that are in the output as a line OR AS AN ENTRY and so equals the value without the option.
 *   BAM: the primary record carries aux XA of type Z (the same characters and a NUL) as its last aux field; block_size includes it;
 *     bin, l_seq and the rest are unchanged; folded records are absent.  B keeps a record far below the 65 280 bytes at which
 *     fem_dev_fetch_bam cuts BGZF members of whole records.
 * fem_dev_xa_count: the entries (folded lines) of the slot's last text or BAM (valid once the fetch has returned); 0 with the
 *   option off. */
/* The byte budget of one XA value.  The worst-case BAM record with it, for the device's longest read (L = 1024, e = 7): fixed part
 * 36 + name <= 255 + CIGAR words (a few dozen bytes for an ordinary alignment; the traceback's bound of 2 L + 2 e + 8 operations
 * would be 8344) + SEQ 512 + QUAL 1024 + NM 4 + MD 3 + (<= a few hundred characters for <= 7 edits) + 1 + the existing tags (NH HI
 * 14, RG <= 259, MC a few dozen, MQ 4, ms 7) + XA 4 + FEM_XA_MAX_BYTES: on the order of 12 KB, and below 50 KB even with every term
 * at its formal bound, so always below the 65 280 bytes of a BGZF member's input. */
#define FEM_XA_MAX_BYTES 8192
int fem_dev_set_xa(fem_dev *h, int slot, int32_t max_entries);
int fem_dev_xa_count(fem_dev *h, int slot, uint64_t *n_entries);

/* ---- read trimming: soft clips made on the device (new; opt-in: the reference maps every read end to end as given, and so does
 *      every batch without it) ----
 * fem_dev_set_trim: trim5, trim3: 0 .. 1024 bases cut from the 5' and the 3' end of every read; qual: 0 is off, 1 .. 93 trims the 3'
 *   end by quality.  tp == NULL or all three 0: off, every byte of every output as before and no kernel more.  Out-of-range values
 *   are FEM_ERR_INVALID and leave the setting as it was.  Per slot and sticky, as the other options; in pair mode each mate is
 *   trimmed on its own by the same setting.  The setting is READ AT fem_dev_map_staged / fem_dev_map_batch_submit and holds for
 *   that batch through all of its fetches: a fem_dev_set_trim between map and fetch acts on the next batch.
 * Rule (integers throughout; it is the specification).  For a read of length L with quality bytes b[0 .. L):
 *   1. Fixed trims: c5 = min(trim5, L), c3f = min(trim3, L - c5).  The rest has L' = L - c5 - c3f bases, q[p] = (int)b[c5 + p] - 33.
 *   2. Quality trim, only with Q = qual >= 1 and L' > K = FEM_TRIM_MIN_KEEP; otherwise cut = L'.  s = 0, best = 0, cut = L'; for
 *      l = L' - 1 down to K: s += Q - q[l]; if s < 0 stop; if s > best (strictly) best = s, cut = l.  (The running-sum rule of
 *      `bwa aln -q`; it never keeps fewer than K bases, and among equal sums it takes the largest l: the least cut.)
 *      The same in parallel form: S[l] the suffix sum of Q - q over [l, L'); stop the largest l >= K with S[l] < 0, K - 1 if none;
 *      cut the largest l in (stop, L') with S[l] the maximum over that range if that maximum is > 0, else L'.
 *   3. c3 = c3f + (L' - cut).  The kept part is bases [c5, L - c3).
 * The as-if property.  Every result of the batch is what the library gives for the batch of the kept parts staged as characters:
 *   fem_dev_fetch, _fetch_packed, _fetch_stats, _fetch_records, _fetch_pairs, _estimate_insert, _estimate_library, every counter,
 *   MAPQ, NH / HI, pairing, TLEN, both rescues, the line filter.  fem_batch_records and fem_batch_pairs carry no S operations: the
 *   clips are output text only, as MAPQ and the tags are.  The text and the BAM records are that batch's with these differences:
 *   CIGAR  a line whose CIGAR column is not * gets <n>S in front of and behind its operations, for n > 0 only: c5 in front and c3
 *     behind without FLAG 0x10, c3 in front and c5 behind with it (the CIGAR runs in the reference's direction).  POS, NM, MD, TLEN
 *     and the BAM bin ignore the clips.
 *   MC:Z and XA:Z carry "the bytes the line would have printed", so the clips too; XA's byte budget counts them.
 *   SEQ and QUAL, where a line carries them, are the whole read as given: L letters (BAM l_seq = L); with fem_dev_set_sam_seq on a
 *     0x10 line the whole read turned.  A read whose kept part is empty is unmapped and prints its whole read, not *.
 *   ms:i sums the other mate's whole quality string, the QUAL that is printed.
 * Staging.  With qual > 0 the batch's qualities must have been committed with fem_dev_commit_text_stage BEFORE fem_dev_map_staged
 *   (the trim stage waits for their copy): otherwise, and after fem_dev_commit_names_stage, FEM_ERR_STATE; so fem_dev_map_batch_submit
 *   with qual > 0 is FEM_ERR_STATE.  With any trimming on, a text or BAM fetch of a batch whose qualities stayed on the host is
 *   FEM_ERR_INVALID.  fem_dev_stage_reads on a slot with trimming set stages equal-length reads as characters, not packed;
 *   fem_dev_commit_stage_packed followed by a map with trimming on is FEM_ERR_UNSUPPORTED.
 *   fem_dev_reserve_text: a line grows by up to 2 x 5 bytes of CIGAR (MC and XA entries likewise) and by the clipped letters twice.
 * fem_dev_fetch_trim: sync + the clip points c5 and c3 of the slot's batch, read for read (pinned memory of the slot, valid until
 *   the slot is mapped again); FEM_ERR_STATE for a batch mapped without trimming.
 * fem_dev_trim_count: sync + the reads with c5 + c3 > 0 and the sum of c5 + c3 over the batch; both 0 without trimming. */
#define FEM_TRIM_MIN_KEEP 35
typedef struct {
  int32_t trim5, trim3; /* 0 .. 1024 */
  int32_t qual;         /* 0: off, 1 .. 93 */
} fem_trim_params;
int fem_dev_set_trim(fem_dev *h, int slot, const fem_trim_params *tp);
int fem_dev_fetch_trim(fem_dev *h, int slot, const uint16_t **clip5, const uint16_t **clip3, uint64_t *n_reads);
int fem_dev_trim_count(fem_dev *h, int slot, uint64_t *n_reads_trimmed, uint64_t *n_bases_trimmed);

/* ---- 3' adapter read-through: matched and clipped on the device (new; opt-in, as trimming is) ----
 * When a fragment is shorter than the read the sequencer runs into the adapter, and the read as given maps nowhere at -e edits.
 * fem_dev_set_adapter: seq1 the adapter of the reads (of mate 1 in pair mode), seq2 that of mate 2 (NULL: seq1 for both): 4 .. 64
 *   letters of ACGT each, lower case accepted and upper-cased; min_overlap O: 1 .. the adapter's length (the shorter one's of two);
 *   err_pct E: 0 .. 30.  ap == NULL or seq1 == NULL: off, every byte of every output as before and no kernel more.  The strings are
 *   copied.  Out-of-range values are FEM_ERR_INVALID and leave the setting as it was.  Per slot and sticky; READ AT fem_dev_map_staged
 *   as fem_dev_set_trim is, with the slot's pair mode (fem_dev_set_pairs) as it is then: in pair mode reads i and n_reads / 2 + i are
 *   the mates, the reads of the second half are matched against seq2, the rest against seq1.
 * Rule (integers throughout; it is the specification).  For a read of length L, A its adapter of m letters:
 *   1. Fixed trims as above: c5, c3f, L' = L - c5 - c3f, x[p] = base[c5 + p].
 *   2. Adapter match.  For p = 0 .. L' - 1: o = min(m, L' - p); mm = the number of j < o with upper(x[p + j]) != A[j], where a read
 *      byte that is not one of ACGTacgt mismatches every letter.  p matches when o >= O and mm * 100 <= o * E.  a3 = L' - p for the
 *      LEAST matching p, 0 when none matches.  Hamming distance only; no floor: a read that is all adapter (p = 0) keeps nothing, as
 *      a read used up by the fixed trims does.
 *   3. The quality trim above runs on what is left: its L' is L' - a3 (so it acts only when that is above FEM_TRIM_MIN_KEEP), and
 *      c3 = c3f + a3 + (what the quality rule cuts).
 *   Everything else is trimming as above: the kept part [c5, L - c3) is the mapping view, the as-if property holds, the text and BAM
 *   carry S around every printed CIGAR and SEQ and QUAL of the whole read.  "Adapter set" counts as trimming on for the staging
 *   rules above: a packed batch is FEM_ERR_UNSUPPORTED, fem_dev_stage_reads stages as characters, a text or BAM fetch with the
 *   qualities on the host is FEM_ERR_INVALID.  The match itself reads no qualities: only qual > 0 needs them before the map.
 *   fem_dev_fetch_trim and fem_dev_trim_count keep their meaning: c3 and the sums include a3; with the adapter alone they work.
 * fem_dev_fetch_adapter: sync + a3 of the slot's batch, read for read (pinned memory of the slot, valid until the slot is mapped
 *   again); FEM_ERR_STATE for a batch mapped without an adapter.
 * fem_dev_adapter_count: sync + the reads with a3 > 0 and the sum of a3 over the batch; both 0 without an adapter. */
typedef struct {
  const char *seq1, *seq2;      /* 4 .. 64 letters of ACGT; seq2 NULL: seq1 */
  int32_t min_overlap, err_pct; /* 1 .. the adapter's length; 0 .. 30 */
} fem_adapter_params;
int fem_dev_set_adapter(fem_dev *h, int slot, const fem_adapter_params *ap);
int fem_dev_fetch_adapter(fem_dev *h, int slot, const uint16_t **adapt3, uint64_t *n_reads);
int fem_dev_adapter_count(fem_dev *h, int slot, uint64_t *n_reads, uint64_t *n_bases);

/* ---- read-through found from the mates' overlap: no adapter sequence needed (new; opt-in, pair mode only) ----
 * When a fragment is shorter than the reads BOTH mates read through it, and mate 1 is the reverse complement of mate 2 over the
 * whole fragment.  That overlap gives the fragment's length, and so the cut of both mates, from 1 read-through base on.
 * fem_dev_set_pair_overlap: min_overlap O: 8 .. 1024; err_pct E: 0 .. 30.  vp == NULL: off, every byte of every output as before and
 *   no kernel more.  Out-of-range values are FEM_ERR_INVALID and leave the setting as it was.  Per slot and sticky; READ AT
 *   fem_dev_map_staged as fem_dev_set_trim is; a set between map and fetch acts on the next batch.  A batch mapped with it on while
 *   the slot is not in pair mode (fem_dev_set_pairs) is FEM_ERR_STATE.
 * Rule (integers throughout; it is the specification).  Reads i and n_reads / 2 + i of a batch are the mates of pair i.
 *   1. Fixed trims as above on each mate: c5, c3f, L1', L2'; x[j] = the base of mate 1 at c5 + j, y[j] the same for mate 2.
 *   2. Base classes: up(b) is the upper-case letter for ACGTacgt and 0 for every other byte, comp the complement on letters.  A
 *      position whose up is 0 matches nothing, in either mate, also when both mates have such a byte at aligned places.
 *   3. The window of a candidate fragment length f, 1 <= f < max(L1', L2'): mate 1 covers the fragment's positions [0, min(f, L1')),
 *      mate 2 covers [max(0, f - L2'), f); their common part is lo = max(0, f - L2'), hi = min(f, L1'), o = hi - lo.
 *   4. The test: mm = the number of j in [lo, hi) for which up(x[j]) is 0, up(y[f - 1 - j]) is 0, or
 *      up(x[j]) != comp(up(y[f - 1 - j])).  f matches when o >= O and mm * 100 <= o * E.  Hamming distance only; the qualities are
 *      not looked at.
 *   5. The pair's fragment length F is the LARGEST matching f (the least cut: in a tandem repeat several f match), 0 when none does.
 *   6. The cuts: v3 of mate k = max(0, Lk' - F) when F > 0, else 0.  As f < max(L1', L2') a matching pair cuts at least one base of
 *      at least one mate; as F >= O every mate keeps min(Lk', O) bases at the least: the rule makes no empty read.
 *   7. Composition: the adapter's a3 (fem_dev_set_adapter, where set as well) and v3 are measured from the same end of the same L';
 *      the 3' cut behind the fixed trims is max(a3, v3).  The quality trim runs on what that leaves exactly as it runs behind a3
 *      alone, and everything after that is trimming as above: the mapping view and the as-if property, the soft clips in CIGAR,
 *      MC:Z and XA:Z, the insert estimate sampling the reads as the run trims them.
 *   8. The overlap is the sequencer's geometry, not the library's: the rule is the same under every fem_dev_set_orientation.
 *   "Overlap set" counts as trimming on for the staging rules above: a packed batch is FEM_ERR_UNSUPPORTED, fem_dev_stage_reads
 *   stages as characters.  It needs no qualities.  fem_dev_fetch_adapter and fem_dev_adapter_count keep their meaning, the
 *   adapter's own matches; c3 and the sums of fem_dev_fetch_trim / fem_dev_trim_count include the composed cut, every cut base once.
 * fem_dev_fetch_pair_overlap: sync + v3 of the slot's batch, read for read (pinned memory of the slot, valid until the slot is
 *   mapped again); FEM_ERR_STATE for a batch mapped without the setting.
 * fem_dev_pair_overlap_count: sync + the pairs with F > 0 and the sum of v3 over both mates; both 0 without the setting. */
typedef struct {
  int32_t min_overlap, err_pct; /* 8 .. 1024; 0 .. 30 */
} fem_pair_overlap_params;
int fem_dev_set_pair_overlap(fem_dev *h, int slot, const fem_pair_overlap_params *vp);
int fem_dev_fetch_pair_overlap(fem_dev *h, int slot, const uint16_t **over3, uint64_t *n_reads);
int fem_dev_pair_overlap_count(fem_dev *h, int slot, uint64_t *n_pairs, uint64_t *n_bases);

/* ---- the coverage track: windowed depth of the output lines, summed on the device over the whole run (new; opt-in: the reference
 *      knows no coverage, and every output without it is byte for byte as before with no kernel more) ----
 * The first output that is accumulated across batches and not rendered per batch: the array belongs to the HANDLE, not to a slot.
 * fem_dev_set_coverage: window W: 1 .. 1 000 000; all_hits: 0 or 1; min_mapq: 0 .. 60.  cp == NULL turns the track off and frees its
 *   array.  It needs the reference on the device (fem_dev_upload_reference), else FEM_ERR_STATE; out-of-range values, or a reference
 *   with more than 2^29 windows at W (the message names the least W that fits), are FEM_ERR_INVALID and leave the setting and the
 *   array as they were.  Setting it again, with the same values or others, zeroes the array.  A new fem_dev_upload_reference waits for the device
 *   and turns it off (as for the reference itself, the caller has no fetch in flight on another thread then).  It never touches a line: the texts and BAM records are byte for byte those without it.
 * Rule (integers throughout; it is the specification).  Coverage is a property of LINES.  It is taken after everything else about
 *   the batch's lines has been decided: the single-end order, rescue, pairing, MAPQ, the lines of unmapped reads, the line filter.
 *   1. Lines that count.  A line counts when its FLAG as written has neither 0x4 nor 0x100, its CIGAR column does not print * (so
 *      a record with 0x8000 never counts), and its MAPQ column as printed is >= min_mapq (without fem_dev_set_mapq the column is
 *      255: every line passes).  With all_hits lines with 0x100 count too, each judged by its own MAPQ column, and so do the lines
 *      that fem_dev_set_xa folds into entries: a folded hit is still a reported hit, as for NH / HI and n_records, and is judged
 *      as the line it would have been.  Folding therefore never changes the track.  Lines the filter (fem_dev_set_report) left
 *      out never count.
 *   2. Span.  A counting line covers [pos0, pos0 + s) of its sequence, s = the summed lengths of the M and D operations of the
 *      record's CIGAR words.  The soft clips of a trimmed batch are output text only and do not enter; an insertion covers
 *      nothing; a deletion counts as covered (the whole-span rule of `mosdepth -x`).  A span is cut at its sequence's end (no line
 *      the mapper makes reaches past it).
 *   3. Windows.  A sequence of n bases has ceil(n / W) windows, the last one ending at n.  bin_off[t] = the sum over the sequences
 *      before t of ceil(len / W); base p of sequence t falls in bin bin_off[t] + p / W.  Each counting line adds, to every bin its
 *      span meets, the number of bases they share.  The bins are 64-bit.
 *   4. Accumulation.  The first text or BAM fetch of a mapped batch (fem_dev_fetch_sam[_nowait], fem_dev_fetch_bam[_nowait]) adds
 *      that batch's lines, exactly once, with the slot's options as they are at that fetch.  Further fetches of the same batch add
 *      nothing; a batch that is mapped but never fetched as text or BAM (fem_dev_fetch_records, _fetch_pairs, the estimates) adds
 *      nothing.  Integer adds commute: the result does not depend on the number of slots, the batch size or the fetch order.
 * fem_dev_coverage_layout: the number of bins and bin_off (n_seq + 1 entries; either pointer may be NULL); FEM_ERR_STATE with the
 *   track off.  The arithmetic is fem_coverage_layout's (fem_host.h).
 * fem_dev_fetch_coverage: waits for every slot's streams (a text fetched with _nowait is complete once its wait has returned, and
 *   also here) and copies the bins to `bins`; cap < n_bins is FEM_ERR_INVALID, the track off FEM_ERR_STATE.  The caller has no
 *   fetch in flight on another thread while it, fem_dev_set_coverage or fem_dev_reset_coverage runs.
 * fem_dev_reset_coverage: zeroes the array; FEM_ERR_STATE with the track off. */
typedef struct {
  int32_t window;   /* 1 .. 1 000 000 */
  int32_t all_hits; /* 0: primary lines only; 1: every hit that is in the output */
  int32_t min_mapq; /* 0 .. 60 */
} fem_coverage_params;
int fem_dev_set_coverage(fem_dev *h, const fem_coverage_params *cp);
int fem_dev_coverage_layout(const fem_dev *h, uint64_t *n_bins, uint64_t *bin_off /* n_seq + 1, or NULL */);
int fem_dev_fetch_coverage(fem_dev *h, uint64_t *bins, uint64_t cap);
int fem_dev_reset_coverage(fem_dev *h);

/* Name of the seed + filter kernel fem_dev_map_staged would launch first for these parameters on the resident
 * index ("seed_join_kernel" — behind its "seed_select_kernel"; "seed_join_banked_kernel" where the reference's sequences
 * need more than one 32-bit coordinate space —, "seed_fast_kernel<hash>", "seed_fast_kernel<lean>" or
 * "seed_filter_kernel"); the generic seed_filter_kernel always follows for whatever those queue.  Static string. */
const char *fem_dev_seed_kernel(const fem_dev *h, const fem_params *p);
/* Which derived tables the resident index has (one line of text, NUL-terminated, cut at cap): "dense: 32-bit occurrence
 * table, strided with pads (8192 MiB), 1 bank, ..." / "... compact ..." / "sparse: bucket summaries" — so that a
 * measurement can say what it ran on (the strided table is taken from 16 entries per bucket on, and may be declined when
 * memory is short). */
int fem_dev_index_info(const fem_dev *h, char *buf, uint64_t cap);

/* ---- measurement ---- */
/* With timing on, every kernel launch is bracketed by HIP events on the stream
 * it is launched on; fem_dev_kernel_time reports their sum and count since
 * the last reset.  kernel: 0 = seed/filter kernel (fast form, k=12 step=3; on a dense
 * index the join kernel, whose selection kernel is 8),
 * 1 = verify kernel, 2 = seed/filter kernel (generic form: the reads the fast
 * form queued, or every read when the fast form does not apply); of
 * fem_dev_fetch_records: 3 = ordering of the mappings, 4 = traceback + MD,
 * 5 = compaction (one entry per call, several kernels each);
 * 6 = unused, always 0 (the count kernel of rounds 1-2; the counters come out of kernel 1 now); of fem_dev_fetch_sam:
 * 7 = the SAM text kernels;
 * 8 = seed selection kernel of the dense-index path (it runs beside the previous batch's kernel 0: its event time is
 * what it takes there, not what it would take alone);
 * 9 = the pairing kernel of a paired fem_dev_fetch_sam (fem_dev_set_pairs);
 * 10 = the mate rescue kernels in front of it (fem_dev_set_rescue; their host waits included; with
 *   fem_dev_set_rescue_discordant the probe of the pairs whose records do not pair runs at their head, inside this id);
 * of fem_dev_fetch_bam: 11 = the BAM record kernels, 12 = the BGZF kernels;
 * 13 = the MAPQ kernel of a fem_dev_fetch_sam / fem_dev_fetch_bam with fem_dev_set_mapq on (one entry per call; the
 * pairing kernel's MAPQ part stays in 9);
 * 14 = the line index kernels of a fem_dev_fetch_sam / fem_dev_fetch_bam with fem_dev_set_unmapped on (one entry per call;
 * the unmapped reads' lines themselves are written by the text and BAM record kernels: 7 and 11; none with a line filter set);
 * 15 = the line filter's line index kernels of a fem_dev_fetch_sam / fem_dev_fetch_bam with fem_dev_set_report on (one entry
 * per call; they make the unmapped reads' part of the index too, so 14 has no entry then);
 * 16 = the insert sampling and bounds kernels of fem_dev_estimate_insert or fem_dev_estimate_library (one entry per call, the zeroing of the histogram
 * included; its fem_dev_fetch_records counts 3, 4 and 5 as any other; no fetch of records, text or pairs counts here);
 * 17 = the score kernel (ms:i) of a paired fem_dev_fetch_sam / fem_dev_fetch_bam with fem_dev_set_mate_tags on (one entry per
 * call; MC, MQ and ms themselves are written by the text and BAM record kernels: 7 and 11; none with the setting off);
 * 18 = the fold index kernels (XA:Z) of a fem_dev_fetch_sam / fem_dev_fetch_bam with fem_dev_set_xa on (one entry per call; where no
 * line filter is set the line index they read is made inside this id, and 14 has no entry; the entries' bytes themselves are
 * written under 7 and 11; none with the option off);
 * of fem_dev_map_staged: 19 = the trim stage of a batch mapped with fem_dev_set_trim, fem_dev_set_adapter or fem_dev_set_pair_overlap on (one
 * entry per batch: adapter_match_kernel where an adapter is set, pair_overlap_kernel where the mates' overlap is, trim_clip_kernel, the
 * scan of the kept lengths, trim_gather_kernel; none with trimming off). */
int fem_dev_set_timing(fem_dev *h, int on);
int fem_dev_reset_timing(fem_dev *h);
int fem_dev_kernel_time(fem_dev *h, int kernel, double *ms_total, uint64_t *launches);
/* Achieved device-to-device copy bandwidth in GB/s over `bytes` (roofline cross-check). */
int fem_dev_copy_bandwidth(fem_dev *h, uint64_t bytes, int iters, double *gb_per_s);
/* Achieved pinned-host-to-device bandwidth in GB/s (what bounds the read stream). */
int fem_dev_h2d_bandwidth(fem_dev *h, uint64_t bytes, int iters, double *gb_per_s);
/* Debug: the bytes of device memory and of pinned host memory that the library's buffers hold at this moment, summed
 * over every handle of the process (either pointer may be null).  Needs no handle; back at its earlier value once a
 * handle is closed. */
int fem_dbg_live_bytes(uint64_t *device_bytes, uint64_t *pinned_bytes);
/* Debug: the device time in ms of one stage of the slot's LAST fetch of records, text or BAM, whether or not timing is on.
 * Negative: the stage was not part of that fetch, the slot has fetched none, or the stream has not yet passed the stage's end (a
 * text that was not waited for).  Stages: 0 order, 1 traceback, 2 compaction, 3 the text's or BAM records' kernels, 4 pairing,
 * 5 rescue, 6 MAPQ, 7 the unmapped reads' line index, 8 the line filter's, 9 the insert estimate, 10 the mate score, 11 the fold
 * index, 12 coverage_kernel (fem_dev_set_coverage). */
#define FEM_STAGE_TEXT 3
#define FEM_STAGE_COVERAGE 12
int fem_dbg_stage_ms(fem_dev *h, int slot, int stage, float *ms);

/* ---- host placement (new; the reference leaves its threads to the scheduler, src/FEM_map.c:172-198) ---- */
/* NUMA node of the host memory GPU `device` is attached to (-1 if the system does not say) and that node's CPUs
 * as a Linux cpulist ("64-127,192-255").  Needs no handle. */
int fem_device_numa(int device, int32_t *node, char *cpulist, uint64_t cap);
/* Restricts the CALLING thread (and the threads it creates afterwards) to those CPUs, so that the pinned staging
 * buffers and the threads that fill them sit next to the GPU.  0 = bound; 1 = nothing done (unknown topology, none of
 * the node's CPUs allowed to this process, or FEM_NUMA_BIND=0).  Call it before the first fem_dev_open on a thread. */
int fem_bind_thread_near_device(int device);

/* ---- multi-GPU (replaces the thread reduction src/FEM_map.c:200-212) ---- */
/* Sums the five MappingStats counters of n handles (one per GPU of this
 * process) with one RCCL all-reduce; stats is n x 5, reduced in place.  The
 * communicator is created on the first call and kept until one of its
 * handles is closed. */
int fem_dev_allreduce_stats(fem_dev *const *h, int n, uint64_t *stats);

#ifdef __cplusplus
}
#endif
#endif /* FEM_HIP_H_ */
