/* ref_fn.c — TEST INFRASTRUCTURE ONLY (see fem_oracle.h): a flat C interface over the reference's OWN functions, one
 * read at a time, so that the tests can compare the oracle, libfemhost and the kernels with the reference stage by stage.
 * Linked with the reference's sources from where they lie (never copied) and the htslib stand-in (ref_standin.c):
 *     make -C oracle ref   ->   oracle/_ref/libfemref_fn.so      (loader: oracle/ref_fem.py)
 *
 *   index       construct_index / save_index / load_index                      src/index.c:57-168
 *   candidates  generate_group_seeding_candidates                              src/filter.c:146-223
 *   verify      verify_candidates: vectorized_banded_edit_distance for full groups of 8, banded_edit_distance for the
 *               remainder                                                       src/align.c:4-51
 *   align       generate_alignment (+ generate_MD_tag)                          src/align.c:279-544
 *
 * Both SequenceBatches (reference, reads) are filled by the reference's own loader (src/sequence_batch.c) from files the
 * caller wrote; the reads are one batch, as one round of load_batch_of_sequences_into_sequence_batch gives it.
 * The reference's asserts stay live (no -DNDEBUG): a call that trips one aborts the process, as `FEM map` would.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "align.h"
#include "filter.h"
#include "index.h"
#include "sequence_batch.h"
#include "utils.h"

typedef struct {
  SequenceBatch ref;
  SequenceBatch reads;
  int has_reads;
  Index index;
  int has_index;
  kvec_t_uint64_t buffer1, buffer2, candidates;
  kvec_t_Mapping mappings;
  kvec_t_uint32_t cigar;
  kstring_t md;
} rf_handle;

static FEMArgs args_of(const rf_handle *h, int e, int a) {
  FEMArgs f;
  memset(&f, 0, sizeof f);
  f.kmer_size = h->index.kmer_size, f.step_size = h->index.step_size;
  f.error_threshold = e, f.num_additional_qgrams = a, f.num_threads = 1, f.seeding_method = 'g';
  return f;
}

/* The reference file, loaded as FEM_index.c:25-28 and FEM_map.c:138-141 load it. */
rf_handle *rf_open(const char *reference_path) {
  rf_handle *h = (rf_handle *)calloc(1, sizeof *h);
  initialize_sequence_batch(&h->ref);
  initialize_sequence_batch_loading(reference_path, &h->ref);
  load_all_sequences_into_sequence_batch(&h->ref);
  initialize_index(&h->index);
  kv_init(h->buffer1.v), kv_init(h->buffer2.v), kv_init(h->candidates.v), kv_init(h->mappings.v), kv_init(h->cigar.v);
  return h;
}

uint32_t rf_num_sequences(const rf_handle *h) { return h->ref.num_loaded_sequences; }
uint32_t rf_sequence_length(const rf_handle *h, uint32_t i) { return get_sequence_length_from_sequence_batch_at(&h->ref, i); }
const char *rf_sequence_name(const rf_handle *h, uint32_t i) { return get_sequence_name_from_sequence_batch_at(&h->ref, i); }

void rf_index_construct(rf_handle *h, int k, int step) {
  destroy_index(&h->index);
  h->index.kmer_size = k, h->index.step_size = step;
  construct_index(&h->ref, &h->index);
  h->has_index = 1;
}

void rf_index_save(rf_handle *h, const char *path) { save_index(path, &h->index); }

void rf_index_load(rf_handle *h, const char *path) {
  destroy_index(&h->index);
  load_index(path, &h->index);
  h->has_index = 1;
}

/* The resident index's arrays (owned by the handle): lookup has 4^k + 1 entries, occ has *n_occ. */
void rf_index_arrays(const rf_handle *h, int *k, int *step, const uint32_t **lookup, uint64_t *n_occ, const uint64_t **occ) {
  *k = h->index.kmer_size, *step = h->index.step_size;
  *lookup = h->index.lookup_table, *n_occ = h->index.occurrence_table_size, *occ = h->index.occurrence_table;
}

/* One batch of at most max_reads reads from a FASTA/FASTQ file; returns how many were loaded.  The negative strands are
 * prepared for all of them (src/map.c:40 does it per read, between the two strands). */
uint32_t rf_load_reads(rf_handle *h, const char *reads_path, uint32_t max_reads) {
  if (h->has_reads) return UINT32_MAX; /* one batch per handle */
  initialize_sequence_batch_with_max_size(max_reads, &h->reads);
  initialize_sequence_batch_loading(reads_path, &h->reads);
  load_batch_of_sequences_into_sequence_batch(&h->reads);
  for (uint32_t i = 0; i < h->reads.num_loaded_sequences; ++i) prepare_negative_sequence_at(i, &h->reads);
  h->has_reads = 1;
  return h->reads.num_loaded_sequences;
}

uint32_t rf_read_length(const rf_handle *h, uint32_t read) { return get_sequence_length_from_sequence_batch_at(&h->reads, read); }

/* generate_group_seeding_candidates for one strand of one read.  Returns the number of candidates and copies at most cap
 * of them; *pre_filter: the count before the additional q-gram filter (0 where the function returns before setting it,
 * as src/map.c:30,41 initialise it). */
uint32_t rf_candidates(rf_handle *h, int e, int a, uint32_t read, int direction, uint64_t *out, uint32_t cap, uint32_t *pre_filter) {
  FEMArgs f = args_of(h, e, a);
  uint32_t pre = 0;
  uint32_t n = generate_group_seeding_candidates(&f, &h->reads, read, (uint8_t)direction, &h->ref, &h->index, &h->buffer1,
                                                 &h->buffer2, &h->candidates, &pre);
  for (uint32_t i = 0; i < n && i < cap; ++i) out[i] = kv_A(h->candidates.v, i);
  *pre_filter = pre;
  return n;
}

/* verify_candidates on n candidates of one strand.  Returns the number of mappings, each as (edit distance, end offset,
 * direction, candidate) in the order the function appends them; the out arrays hold n entries. */
uint32_t rf_verify(rf_handle *h, int e, int a, uint32_t read, int direction, const uint64_t *candidates, uint32_t n, uint8_t *ed,
                   int16_t *end, uint8_t *dir, uint64_t *cand) {
  FEMArgs f = args_of(h, e, a);
  kv_clear(h->mappings.v);
  uint32_t m = n ? verify_candidates(&f, &h->reads, read, (uint8_t)direction, &h->ref, candidates, n, &h->mappings) : 0;
  for (uint32_t i = 0; i < m; ++i) {
    Mapping x = kv_A(h->mappings.v, i);
    ed[i] = x.edit_distance, end[i] = x.end_position_offset, dir[i] = x.direction, cand[i] = x.candidate_position;
  }
  return m;
}

/* generate_alignment for one mapping, called as process_mappings calls it (src/align.c:71-78).  Returns the start offset
 * inside the candidate's window; *n_cigar operations (BAM encoding) go to cigar (at most cigar_cap are copied), the MD
 * string with its NUL to md (at most md_cap bytes). */
int rf_align(rf_handle *h, int e, uint32_t read, int direction, uint64_t candidate, int ed, int end, uint32_t *cigar, int cigar_cap,
             int *n_cigar, char *md, int md_cap) {
  FEMArgs f = args_of(h, e, 0);
  const char *text = direction == POSITIVE_DIRECTION ? get_sequence_from_sequence_batch_at(&h->reads, read)
                                                     : get_negative_sequence_from_sequence_batch_at(&h->reads, read);
  const char *pattern = get_sequence_from_sequence_batch_at(&h->ref, candidate >> 32) + (uint32_t)candidate;
  kv_clear(h->cigar.v);
  h->md.l = 0;
  int start = generate_alignment(&f, pattern, text, (int)rf_read_length(h, read), ed, end, &h->cigar, &h->md);
  *n_cigar = (int)kv_size(h->cigar.v);
  for (int i = 0; i < *n_cigar && i < cigar_cap; ++i) cigar[i] = kv_A(h->cigar.v, i);
  if (md_cap > 0) {
    size_t n = h->md.l < (size_t)md_cap - 1 ? h->md.l : (size_t)md_cap - 1;
    if (n) memcpy(md, h->md.s, n);
    md[n] = '\0';
  }
  return start;
}

void rf_close(rf_handle *h) {
  if (!h) return;
  if (h->has_reads) {
    finalize_sequence_batch_loading(&h->reads);
    destory_sequence_batch(&h->reads);
  }
  destroy_index(&h->index);
  finalize_sequence_batch_loading(&h->ref);
  destory_sequence_batch(&h->ref);
  kv_destroy(h->buffer1.v), kv_destroy(h->buffer2.v), kv_destroy(h->candidates.v), kv_destroy(h->mappings.v);
  kv_destroy(h->cigar.v);
  free(h->md.s);
  free(h);
}
