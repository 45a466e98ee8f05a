// fem_tail.hip.h — the mapping tail on the device: what process_mappings does for every mapped read
// (reference src/align.c:53-92) — order the read's Mappings with radix_sort_mapping, then for each one
// generate_alignment (src/align.c:279-499: ungapped shortcut, or the Myers recurrence re-run with D0/HP kept per
// column and the traceback with its 'S' pseudo-run) and generate_MD_tag (src/align.c:501-544).
// Input: the per-candidate verification outcome the mapping kernels left in HBM.  Output: records in the reference's
// order (FLAG, reference id, POS, NM, BAM-encoded CIGAR, MD), compacted on the device, copied to pinned host memory.
#pragma once
#include <mutex>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <memory>
#include <string>

namespace femt {

struct TailInput {  // device pointers unless noted
  const uint8_t *bases;        // raw read characters, concatenated
  const uint64_t *read_off;    // n_reads + 1
  uint32_t n_reads;
  uint32_t max_len;            // host: longest read of the batch
  const uint8_t *ref_raw;      // raw reference characters (case kept: the traceback compares characters, src/align.c:355)
  uint64_t ref_bytes;          // host: bytes in ref_raw, its slack included
  // the batch as it arrived packed (fem_dev_stage_reads on equal-length reads): two bits per base, four bases per byte,
  // packed_bpr bytes per read; bit r of exc_bits: read r has a character that is not one of ACGT (kept in `bases` only).
  // nullptr: the batch came as characters.
  const uint8_t *packed;
  uint32_t packed_bpr;
  const uint32_t *exc_bits;
  const uint8_t *planes;       // bit planes over the reference (femk::plane_window): code bits 0..2, and "character is none of ACGTN"
  const uint64_t *seq_off;
  const uint64_t *cand;        // per candidate slot
  const uint8_t *ed;           // 0xFF = rejected
  const int16_t *end;
  const uint32_t *cand_begin;  // 2 * n_reads
  const uint32_t *cand_count;
  const uint32_t *n_map;       // n_reads: accepted candidates of each read
  int32_t e;
  uint64_t n_records;          // host: total accepted candidates (the "number of mapping" counter)
  // a trimmed batch (fem_dev_set_trim): bases / read_off above are the kept parts, the mapping view, and these the whole reads
  // and each read's clipped bases at its 5' and 3' end.  sam() and bam() print SEQ, QUAL and ms:i from the whole reads and the
  // CIGARs with the clips as S operations around them (clip_count_kernel, clip_write_kernel).  nullptr: not trimmed.
  const uint8_t *text_bases;
  const uint64_t *text_read_off;
  const uint16_t *clip5, *clip3;
};

struct TailOutput {  // pinned host memory owned by the Tail object, valid until its next run
  uint64_t n_reads, n_records;
  const uint32_t *rec_begin;  // n_reads + 1: records of read i are [rec_begin[i], rec_begin[i+1]), primary first
  const uint16_t *flag;       // 16 = reverse strand, 256 = secondary; 0x8000 = the reference would have asserted
  const uint32_t *tid;
  const uint32_t *pos0;       // 0-based leftmost reference position
  const uint8_t *nm;
  const uint32_t *cigar_off;  // n_records + 1
  const uint32_t *cigar;      // BAM encoding len << 4 | op (M 0, I 1, D 2)
  const uint32_t *md_off;     // n_records + 1
  const char *md;
};

// ---- SAM text on the device: the records of the last run() rendered as the reference's output lines
//      (generate_bam1_t + htslib's SAM writer, src/align.c:546-632, src/output_queue.c:93-116) ----
struct SamInput {  // device pointers (what the lines look like: LineOptions)
  const uint8_t *quals;          // quality characters, same offsets as the bases
  const uint8_t *names;          // read names, concatenated
  const uint64_t *name_off;      // n_reads + 1
  const uint8_t *ref_names;      // reference sequence names, concatenated
  const uint32_t *ref_name_off;  // n_seq + 1
  bool qual_hole;                // quals == nullptr and the QUAL field of a primary record is LEFT UNWRITTEN (the caller fills it: SamOutput::qual_at)
};
struct SamOutput {  // pinned host memory owned by the Tail object, valid until its next sam()
  const char *text;
  uint64_t len;
  uint64_t n_asserted;  // records on which the reference would have tripped an assertion (written with CIGAR *)
  const uint64_t *qual_at;  // qual_hole: per READ, where in `text` its QUAL field starts (~0: the read has no line, or a line without QUAL); else nullptr
};

// ---- BAM on the device: the same lines as BAM records, BGZF-compressed (fem_bgzf.hip) ----
struct BamOutput {  // pinned host memory owned by the Tail object (the SAM text's), valid until its next sam() / bam()
  const uint8_t *data;  // whole BGZF members: no header, no EOF block
  uint64_t len, raw_len, n_blocks;
  uint64_t n_asserted;
};

// ---- pair mode: the reads of the last run() are n / 2 read pairs, read i and read n / 2 + i the two mates of pair i ----
struct PairOutput {  // pinned host memory owned by the Tail object, valid until its next pair_fetch()
  uint64_t n_pairs, n_records, n_proper;
  const uint32_t *pair_begin;  // 2 * n_pairs + 1: mate m of pair i has output lines [pair_begin[2i+m], pair_begin[2i+m+1])
  const uint32_t *perm;        // n_records: line k renders record perm[k] (record numbers of run()'s output)
  const uint16_t *flag;        // per line: the SAM flag as written, 0x8000 kept
  const uint32_t *mate_tid, *mate_pos0;  // per line: the other mate's primary (0xFFFFFFFF: the other mate has no record)
  const int32_t *tlen;         // per line
  // mate rescue (RescueInput): records first_rescued .. first_rescued + n_rescued - 1 are not run()'s but the rescued mates'
  uint32_t first_rescued;
  uint64_t n_rescued;
  const uint16_t *r_flag;
  const uint32_t *r_tid, *r_pos0;
  const uint8_t *r_nm;
  const uint32_t *r_cigar_off, *r_cigar;  // r_cigar_off: n_rescued + 1, from r_cigar_off[0] (not 0) on
  const uint32_t *r_md_off;               // n_rescued + 1, from r_md_off[0] on
  const char *r_md;
};

// Mate rescue (LineOptions::rescue): what pair() needs besides the records to search the mapped mate's insert window.
struct RescueInput {  // device pointers unless noted
  const uint8_t *bases;        // the batch's read characters (both stagings leave them on the device)
  const uint64_t *read_off;
  uint32_t max_len;            // host: longest read of the batch
  const uint8_t *ref_raw;
  uint64_t ref_bytes;          // host: bytes in ref_raw, its slack included
  const uint64_t *seq_off;
  const uint32_t *seq_len;
};

// What the lines of a slot's texts and BAM records look like: host values, one field per option of the C API's fem_dev_set_*.
// pair() reads the pairing and rescue fields, sam() / bam() the others and `paired`.  A new output option is a field here.
struct LineOptions {
  bool paired = false;             // the lines in the order of the last pair() with its mate columns (the records of both stay on the device)
  int32_t min_insert = 0, max_insert = 0;
  int32_t orientation = 0;         // FEM_ORIENT_FR / _RF / _FF: which mates' strands the pairing rule reads flipped (in pair mode)
  bool rescue = false;             // mate rescue at rescue_edits edits (E, 0 .. 15), in pair mode
  int32_t rescue_edits = 0;
  // a pair with records on both sides and no concordant combination is a candidate too, searched from either mate's anchors
  // (pair_probe_kernel in front of the rescue kernels)
  bool rescue_discordant = false;
  bool mapq = false;               // MAPQ from the hit strata (mapq_kernel; pair() leaves pair_kernel's bytes for it); else 255
  bool unmapped = false;           // a line for every read without a record (the kernels' kUnm instances)
  int32_t strata = -1;             // the line filter (report_kernel): a slot's lines within this many edits of its best, -1: off
  int32_t max_hits = -1;           // ... and at most this many lines per slot (>= 1), -1: off
  std::string read_group;          // the ID every line's RG:Z tag carries; empty: no RG tag
  bool hit_tags = false;           // NH:i and HI:i on every mapped line
  bool mate_tags = false;          // MC:Z MQ:i ms:i on every line of a paired text (mate_score_kernel; the kernels' kMate instances)
  bool sam_seq = false;            // SEQ reverse-complemented and QUAL reversed on the lines with 0x10 that carry them (the write kernels)
  // the coverage track (fem_dev_set_coverage): this text's lines are added to the handle's bins (coverage_kernel).
  // Set by the caller for the first text of a batch alone; window 0: off
  struct Coverage {
    int32_t window = 0;            // W
    bool all_hits = false;         // lines with 0x100 count too (folded ones among them)
    int32_t min_mapq = 0;          // a line counts from this MAPQ column on
    uint32_t n_seq = 0;
    const uint64_t *bin_off = nullptr;   // device: n_seq + 1
    const uint32_t *seq_len = nullptr;   // device: n_seq
    unsigned long long *bins = nullptr;  // device: the handle's array
  } coverage;
  int32_t xa_entries = 0;          // secondary lines folded into XA:Z on the slot's first line, at most this many per slot; 0: off (xa_index_kernel, xa_write_kernel)
  bool filters() const { return strata >= 0 || max_hits >= 1; }  // the line filter is on
  bool folds() const { return xa_entries > 0; }
  bool covers() const { return coverage.window > 0; }
  bool rescues() const { return paired && rescue; }
  bool mates() const { return paired && mate_tags; }
  // the mates' flips as the kernels take them: 16 where the mate's strand is flipped (FR 0 0, RF 16 16, FF 0 16)
  uint32_t flip1() const { return orientation == 1 ? 16u : 0u; }
  uint32_t flip2() const { return orientation == 0 ? 0u : 16u; }
};
// What the last pair() and the last sam() / bam() counted (Tail::counts).
struct LineCounts {
  uint64_t n_proper = 0;              // proper pairs
  uint64_t n_rescued = 0;             // kept rescued records (0 without LineOptions::rescue)
  uint64_t n_rescued_discordant = 0;  // ... those of pairs with records on both sides (0 without LineOptions::rescue_discordant)
  uint64_t n_unmapped = 0;            // lines for unmapped reads (0 without LineOptions::unmapped)
  uint64_t n_filtered = 0;            // lines the filter left out (0 without LineOptions::strata / max_hits)
  uint64_t n_xa = 0;                  // lines folded into XA:Z entries (0 without LineOptions::xa_entries)
};

// What estimate_insert() learns from the unique pairs of the last run() (include/fem_hip.h, fem_dev_estimate_insert: the rule).
struct InsertEstimate {
  uint64_t n_pairs, n_unique, n_informative;
  int32_t q25, q50, q75;           // -1 without an informative pair
  int32_t min_insert, max_insert;  // 0 unless estimated
  bool estimated;
};
// What estimate_library() learns: the estimate under each orientation (FR, RF, FF) and the chosen one, -1 for none.
struct LibraryEstimate {
  InsertEstimate by[3];
  int32_t orientation;
};

// One text on its way home at a time (per GPU).  Two device-to-host copies queued in the copy engines take both of them, and
// the next batch's reads wait for their copy in until every queued text is home (scratch/sdma_probe.hip: a 30 MB copy in
// behind ONE 300 MB copy out is done after 0.6 ms, behind four after all four, 22 ms); FEM map's device then alternated
// between four batches' kernels and four batches' texts going home.  The thread that queues a text's copy waits here for
// the previous text to have arrived.
struct TextGate {
  std::mutex mu;
  hipEvent_t last = nullptr;  // the latest text's arrival (an event of some slot's Tail; never destroyed before the handle's tails are)
};

// The timed stages of a batch's way out of the device.  Each runs between two events on its stream, recorded whether or not
// anybody asks (Tail::stage_ms).  run(): kOrder, kTrace, kCompact.  pair(): kRescue when it rescues, kPairing.  sam() / bam():
// kMapq with LineOptions::mapq; kFilterIndex, the line index with the line filter, or else kUnmappedIndex, the one with
// LineOptions::unmapped alone; kMateScore, mate_score_kernel with LineOptions::mate_tags on a batch with device qualities;
// kText, the SAM text's or the BAM records' kernels (xa_write_kernel among them); kXaIndex with LineOptions::xa_entries, the fold index
// behind the line index (and the line index itself where the line filter is off: report_kernel with nothing to leave out).
// kCoverage with LineOptions::coverage, coverage_kernel behind the line index and the MAPQ kernel.
// estimate_insert() and estimate_library(): kInsert.  (The numbers are those of fem_dbg_stage_ms, include/fem_hip.h: new stages at the end.)
enum Stage { kOrder, kTrace, kCompact, kText, kPairing, kRescue, kMapq, kUnmappedIndex, kFilterIndex, kInsert, kMateScore, kXaIndex, kCoverage, kStages };

class Tail {
 public:
  Tail();
  ~Tail();
  Tail(const Tail &) = delete;
  Tail &operator=(const Tail &) = delete;
  // Runs on `stream` and waits for it.
  // tiny = test hook: per-record CIGAR/MD staging starts far too small so that the overflow pass runs.
  // copy_records = false: the records stay on the device (for sam()); *out then only carries the counts.
  int run(const TailInput &in, hipStream_t stream, int n_cu, bool tiny, TailOutput *out, std::string *err, bool copy_records = true);
  // Makes room for `bytes` of SAM text ahead of time (pinning host memory costs ~0.25 ms per MB: better spent before
  // the first batch than inside it).
  int reserve_text(uint64_t bytes, std::string *err);
  // ... and for everything else run() and sam() allocate for a batch of n_reads reads with n_records records.
  int reserve(uint32_t n_reads, uint32_t n_records, uint32_t max_len, int e, bool tiny, std::string *err);
  // ... and loads the kernels (a code object is loaded by its first launch otherwise) and wakes `stream`.
  int warm(hipStream_t stream, std::string *err);
  // The records of the last run() as SAM lines, in record order; opt.paired: in the order of the last pair().
  // wait = false: returns once the copy of the text to the host has been queued; wait_text() (which may be called from
  // another thread) returns when it has arrived.
  int sam(const TailInput &in, const SamInput &names, const LineOptions &opt, hipStream_t stream, int n_cu, SamOutput *out, std::string *err,
          bool wait = true, TextGate *gate = nullptr);
  // The same lines as BAM records (names.quals must be set: no qual_hole), compressed at `level` (0 or 1) into BGZF members.
  // bgzf_ms (optional) receives the BGZF kernels' device time (the record kernels' is stage kText's).  wait, gate: as sam().
  // FEM_ERR_UNSUPPORTED for a read name over 254 characters.
  int bam(const TailInput &in, const SamInput &names, const LineOptions &opt, int level, hipStream_t stream, int n_cu, BamOutput *out,
          std::string *err, float *bgzf_ms, bool wait = true, TextGate *gate = nullptr);
  // Pairs the records of the last run() (pair_kernel): output order, FLAG, mate columns and TLEN of every line, the proper-pair
  // count.  Asynchronous on `stream`; counts().n_proper is valid once the stream has been synchronised (sam() does).
  // opt.rescues(): mate rescue first (the rescue kernels, reading `rescue`), the kept rescued records appended behind run()'s;
  // pair() then waits for the stream twice (the candidate count, the kept count).  LineOptions::rescue_discordant:
  // pair_probe_kernel runs at their head, inside stage kRescue, and adds no wait.
  // opt.mapq: pair_kernel also writes each line's pairing byte (qp and whether the chosen record may keep its own MAPQ), which the
  // next sam() / bam() with LineOptions::mapq turns into the MAPQ of the mates' primary lines.
  int pair(const LineOptions &opt, const RescueInput &rescue, hipStream_t stream, std::string *err);
  // The insert size range the records of the last run() suggest (insert_sample_kernel, insert_bounds_kernel): the pairs whose
  // mates have one record each, their inserts' quartiles, the fence around them.  Runs on `stream` and waits for it.  Reads the
  // records only: what pair() made, the slot's options and the counts stay as they are.
  // "Informative" follows opt.orientation.
  int estimate_insert(const LineOptions &opt, hipStream_t stream, InsertEstimate *out, std::string *err);
  // The same under the three orientations in one pass (library_sample_kernel, insert_bounds_kernel with a block each), and the
  // choice: the orientation with the most informative pairs among the estimated ones, ties in the order FR RF FF, -1 for none.
  int estimate_library(hipStream_t stream, LibraryEstimate *out, std::string *err);
  // The counts of the last pair() (all 0 unless it ran since the last run()) and of the last sam() / bam().
  LineCounts counts() const;
  // The device time of a stage, in ms.  Negative: the stage was not part of the last run() and of what followed it (pair(),
  // sam() or bam()), or its stream has not yet passed its end (a text that was not waited for).
  float stage_ms(Stage stage) const;
  // coverage_kernel has been queued since the last run() (a sam() / bam() with LineOptions::coverage got that far, whether or not
  // it succeeded afterwards): the batch's lines are in the track, or on their way there.
  bool coverage_queued() const;
  // The arrays of the last pair() to the host (waits for `stream`).
  int pair_fetch(hipStream_t stream, PairOutput *out, std::string *err);
  int wait_text();

 private:
  struct Impl;
  std::unique_ptr<Impl> impl_;
  int impl(Impl **m);  // the state, made on first use; FEM_ERR_NOMEM
  int estimate(const LineOptions *opt, uint32_t n_hist, hipStream_t stream, InsertEstimate *out, std::string *err);
};

}  // namespace femt
