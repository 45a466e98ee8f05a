// fem_main.cc — the drop-in command line: `FEM index` and `FEM map` (reference src/FEM.c, src/FEM_index.c,
// src/FEM_map.c).  Same verbs, flags, index file format and SAM output; the per-read hot path runs on the GPU
// through libfemhip.so (include/fem_hip.h).  There is no CPU mapping path in this binary: without a GPU it fails.
//
// New, optional: `--gpus N` (map) spreads read batches over N GPUs of this node (whichever GPU has a free slot takes the
// next batch; record order in the SAM file follows completion, parity is modulo record order); `--batch N` sets reads
// per batch.  `--read2 STR` maps read pairs (record i of --read1 and of --read2 are the two mates of pair i), with -I / -X the
// accepted insert size: the pairing and the paired SAM text on the device (fem_dev_set_pairs); `--rescue INT` adds mate rescue
// at INT edits (fem_dev_set_rescue), `--rescue-discordant` also for pairs whose records do not pair (fem_dev_set_rescue_discordant).  `--mapq` writes mapping qualities made on the device (fem_dev_set_mapq) instead of 255.
// `--infer-insert[=N]` learns -I / -X from the input's first N pairs on the device, before the run (fem_dev_estimate_insert).
// `--unmapped` adds a line for every read without a mapping, made on the device (fem_dev_set_unmapped).
// `--strata INT` / `--max-hits INT` leave out the lines of a read beyond its best strata / its first INT (fem_dev_set_report).
// `--header` puts @HD in front of the @SQ lines and @PG behind them; `--rg LINE` adds the @RG line and RG:Z on every line, `--nh`
// NH:i and HI:i on every mapped line, both made on the device (fem_dev_set_tags).
// `--orientation fr|rf|ff|auto` sets the library's orientation (fem_dev_set_orientation); `auto` learns it with the insert size
// range, in --infer-insert's pre-pass (fem_dev_estimate_library).
// `--mate-tags` adds MC:Z, MQ:i and ms:i to every line of a paired output, made on the device (fem_dev_set_mate_tags).
// `--sam-seq` prints SEQ reverse-complemented and QUAL reversed on the reverse-strand lines that carry them, as the SAM
// specification orders them, made on the device (fem_dev_set_sam_seq).
// `--trim5 N`, `--trim3 N`, `--trim-qual Q` trim every read on the device before it is mapped (fixed counts off its ends, its
// 3' end by quality: the running-sum rule of include/fem_hip.h) and print what was cut as soft clips (fem_dev_set_trim).
// `--adapter SEQ` (`--adapter2 SEQ` for mate 2, `--adapter-overlap INT`, `--adapter-err INT`) has the 3' adapter of read-through
// reads matched and cut on the device in front of the quality trim, printed as soft clips as well (fem_dev_set_adapter).
// `--trim-overlap` (`--trim-overlap-min INT`, `--trim-overlap-err INT`) finds the read-through of a pair from the overlap of its
// mates, with no adapter given, and cuts both mates at the fragment's end on the device (fem_dev_set_pair_overlap).
// `--xa[=N]` folds the secondary lines of a read (of a mate) into an XA:Z field on its primary line, at most N of them and
// FEM_XA_MAX_BYTES bytes per line, made on the device (fem_dev_set_xa).
// `--coverage FILE` (`--coverage-window INT`, `--coverage-all`, `--coverage-mapq INT`) writes the windowed depth of the output's
// lines as BED text: summed on the device over the whole run, one array per GPU, added up and written here at the end
// (fem_dev_set_coverage, fem_coverage_write).
#include <errno.h>
#include <fcntl.h>
#include <getopt.h>
#include <unistd.h>
#include <malloc.h>
#include <sys/resource.h>
#include <sys/stat.h>
#include <sys/time.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/fem_hip.h"
#include "fem_host.h"

#define FEM_VERSION "0.2"

namespace {

double real_time() {
  struct timeval tp;
  gettimeofday(&tp, nullptr);
  return tp.tv_sec + tp.tv_usec * 1e-6;
}
double cpu_time() {
  struct rusage r;
  getrusage(RUSAGE_SELF, &r);
  return r.ru_utime.tv_sec + r.ru_stime.tv_sec + 1e-6 * (r.ru_utime.tv_usec + r.ru_stime.tv_usec);
}

// --adapter / --adapter2: 4 to 64 letters of ACGT, either case
bool adapter_ok(const char *a) {
  const size_t m = strlen(a);
  return m >= 4 && m <= 64 && strspn(a, "ACGTacgt") == m;
}

void usage_main() {
  fprintf(stderr, "\nProgram: FEM (Fast and Efficient short read Mapper), MI355X build\n");
  fprintf(stderr, "Version: %s\n\n", FEM_VERSION);
  fprintf(stderr, "Usage:   FEM <command> [options]\n\n");
  fprintf(stderr, "Command: index   build index for reference\n");
  fprintf(stderr, "         map     map reads\n\n");
  fprintf(stderr, "Note: To use FEM, you need to first index the genome with `FEM index'.\n\n");
}
void usage_index() { fprintf(stderr, "Usage: FEM index <window_size> <step_size> <reference> <output>\n"); }
void usage_map() {
  fprintf(stderr, "\nUsage:  FEM map [options] \n\nOptions:\n");
  fprintf(stderr, "        -e       INT  error threshold \n");
  fprintf(stderr, "        -t       INT  number of threads \n");
  fprintf(stderr, "        -f       STR  seeding algorithm: \"g\" for group seeding and \"v\" for variable-length seeding \n");
  fprintf(stderr, "        -a       INT  # additional q-grams (only for test)\n");
  fprintf(stderr, "        --gpus   INT  number of GPUs to shard read batches over [1]\n");
  fprintf(stderr, "        --batch  INT  reads per device batch [250000]\n\n");
  fprintf(stderr, "Input/output: \n");
  fprintf(stderr, "        --ref    STR  Input reference file\n");
  fprintf(stderr, "        --index  STR  Input index file\n");
  fprintf(stderr, "        --read1  STR  Input read1 file\n");
  fprintf(stderr, "        --read2  STR  Input read2 file: map read pairs (record i of both files is pair i)\n");
  fprintf(stderr, "        -I, --minins INT  minimum insert size of a proper pair [0]\n");
  fprintf(stderr, "        -X, --maxins INT  maximum insert size of a proper pair [500]\n");
  fprintf(stderr, "        --infer-insert[=INT]  with --read2: learn -I / -X from the first INT (64-262144) [65536] pairs, on the GPU, before the run\n");
  fprintf(stderr, "        --orientation STR  with --read2: the library's orientation, fr, rf or ff [fr]; auto: learned with --infer-insert, on the GPU, before the run\n");
  fprintf(stderr, "        --rescue INT  with --read2: search a mate without records in its mate's insert window at INT (0-15) edits\n");
  fprintf(stderr, "        --rescue-discordant  with --rescue: also search the mates of a pair whose records do not pair\n");
  fprintf(stderr, "        --bam[=INT]   write BAM instead of SAM: BGZF level 1 (default) or 0 (uncompressed)\n");
  fprintf(stderr, "        --mapq        write mapping qualities (0-60) from the hits' edit distances instead of 255\n");
  fprintf(stderr, "        --unmapped    write a line for every read without a mapping too (FLAG 0x4; a mate placed at its mapped mate)\n");
  fprintf(stderr, "        --strata INT  write only a read's (a mate's) lines within INT (0-15) edits of its best one; the primary line always\n");
  fprintf(stderr, "        --max-hits INT  write at most INT (>= 1) lines per read (per mate)\n");
  fprintf(stderr, "        --header      begin the output with @HD (VN:1.6 SO:unsorted GO:query) and end its header with @PG (the command line)\n");
  fprintf(stderr, "        --rg     STR  a whole @RG line, its fields separated by tabs or \\t ('@RG\\tID:x\\tSM:y'): written into the header\n");
  fprintf(stderr, "                      (implies --header), and every line gets RG:Z:<ID>\n");
  fprintf(stderr, "        --nh          write NH:i (the read's, or the mate's, lines in the output) and HI:i (which of them) on every mapped line\n");
  fprintf(stderr, "        --mate-tags   with --read2: write MC:Z, MQ:i and ms:i (the other mate's CIGAR, MAPQ and quality score, as samtools fixmate -m) on every line\n");
  fprintf(stderr, "        --xa[=N]      fold a read's secondary lines into XA:Z:(rname,+-pos,CIGAR,NM;)* on its primary line, at most N (1-1000000; default: all that fit %d bytes); the rest stay lines\n", FEM_XA_MAX_BYTES);
  fprintf(stderr, "        --trim5 INT   trim INT (0-1024) bases off the 5' end of every read before mapping, on the GPU; printed as soft clips\n");
  fprintf(stderr, "        --trim3 INT   trim INT (0-1024) bases off the 3' end of every read before mapping, on the GPU; printed as soft clips\n");
  fprintf(stderr, "        --trim-qual INT  trim the 3' end of every read by quality INT (1-93) before mapping, on the GPU, keeping %d bases at the least; printed as soft clips\n", FEM_TRIM_MIN_KEEP);
  fprintf(stderr, "        --adapter STR  cut the 3' adapter STR (4-64 letters of ACGT) and what follows it off every read before mapping, on the GPU, in front of --trim-qual; printed as soft clips\n");
  fprintf(stderr, "        --adapter2 STR  with --read2: the adapter of the second mates (default: that of --adapter)\n");
  fprintf(stderr, "        --adapter-overlap INT  the least number of adapter bases at a read's end that count as a match (1 to the adapter's length) [5]\n");
  fprintf(stderr, "        --adapter-err INT  mismatches allowed in an adapter match, per cent of the overlap (0-30) [10]\n");
  fprintf(stderr, "        --trim-overlap  with --read2: where the mates of a pair overlap as a fragment shorter than the reads does, cut both at the fragment's end before mapping, on the GPU; no adapter needed; printed as soft clips\n");
  fprintf(stderr, "        --trim-overlap-min INT  the least number of overlapping bases that count as a match (8-1024) [20]\n");
  fprintf(stderr, "        --trim-overlap-err INT  mismatches allowed in the overlap, per cent of it (0-30) [10]\n");
  fprintf(stderr, "        --coverage FILE  write the windowed depth of the output's lines to FILE as BED (name, start, end, covered bases, mean depth), summed on the GPU\n");
  fprintf(stderr, "        --coverage-window INT  the window (1-1000000) [1000]\n");
  fprintf(stderr, "        --coverage-all  count every hit that is in the output (secondary lines and XA entries too), not the primary lines alone\n");
  fprintf(stderr, "        --coverage-mapq INT  with --mapq: count the lines whose MAPQ is INT (1-60) at the least\n");
  fprintf(stderr, "        --sam-seq     write SEQ reverse-complemented and QUAL reversed on reverse-strand lines (FLAG 0x10), as the SAM specification orders them\n");
  fprintf(stderr, "        -o       STR  Output SAM file \n\n");
}

std::string g_pg_line;  // the @PG line of `--header`: main() makes it of its argv, before getopt reorders that

struct Reference {
  fem_seqset set{};
  std::vector<uint32_t> len;
  fem_tail_ref view{};
  bool load(const char *path) {
    double t0 = real_time();
    fem_seqfile *f = fem_seqfile_open(path);
    if (!f) {
      fprintf(stderr, "Cannot find sequence file!");
      return false;
    }
    int rc = fem_seqfile_read(f, 0, &set);
    fem_seqfile_close(f);
    if (rc != 0) {
      fprintf(stderr, "Didn't reach the end of sequence file, which might be corrupted!");
      return false;
    }
    len.resize(set.n);
    for (uint64_t i = 0; i < set.n; ++i) {
      uint64_t l = set.off[i + 1] - set.off[i];
      if (l > 0xFFFFFFFFull) {
        fprintf(stderr, "Reference sequence longer than 2^32 bases.\n");
        return false;
      }
      len[i] = (uint32_t)l;
    }
    view.text = set.bases, view.off = set.off, view.len = len.data(), view.n_seq = (uint32_t)set.n;
    view.names = set.names, view.name_off = set.name_off;
    fprintf(stderr, "Number of sequences: %lu\n", (unsigned long)set.n);
    fprintf(stderr, "Number of bases: %lu\n", (unsigned long)set.off[set.n]);
    fprintf(stderr, "Loaded all sequences successfully in %fs\n", real_time() - t0);
    return set.n > 0;
  }
  int upload(fem_dev *h) const {
    std::vector<const char *> ptr(set.n);
    for (uint64_t i = 0; i < set.n; ++i) ptr[i] = set.bases + set.off[i];
    return fem_dev_upload_reference(h, (uint32_t)set.n, ptr.data(), len.data());
  }
  ~Reference() { fem_seqset_free(&set); }
};

int dev_fail(fem_dev *h, const char *what, int rc) {
  fprintf(stderr, "[FEM] %s failed: %s (%s)\n", what, fem_strerror(rc), h ? fem_dev_last_error(h) : "");
  return EXIT_FAILURE;
}

// ---------------------------------------------------------------- FEM index (src/FEM_index.c:11-39)
int index_main(int argc, char **argv) {
  if (argc < 5) {
    fprintf(stderr, "%s\n", "Too few args!");
    usage_index();
    exit(EXIT_FAILURE);
  }
  int k = atoi(argv[1]), step = atoi(argv[2]);
  const char *ref_path = argv[3], *out_path = argv[4];
  fprintf(stderr, "k: %d, step size: %d, reference: %s, output: %s\n", k, step, ref_path, out_path);
  if (k < 1 || k > 15 || step < 1) {
    fprintf(stderr, "window_size must be 1..15 and step_size >= 1.\n");
    usage_index();
    exit(EXIT_FAILURE);
  }
  (void)fem_bind_thread_near_device(0);  // host threads and buffers next to the GPU (FEM_NUMA_BIND=0: leave them alone)
  Reference ref;
  if (!ref.load(ref_path)) exit(EXIT_FAILURE);
  fem_dev *h = nullptr;
  int rc = fem_dev_open(0, &h);
  if (rc) return dev_fail(nullptr, "fem_dev_open (the index is built on the GPU; no CPU path)", rc);
  double t0 = real_time();
  if ((rc = ref.upload(h))) return dev_fail(h, "reference upload", rc);
  uint64_t n_occ = 0;
  if ((rc = fem_dev_build_index(h, k, step, nullptr, nullptr, 0, &n_occ))) return dev_fail(h, "index build", rc);
  std::vector<uint32_t> lookup(((size_t)1 << (2 * k)) + 1);
  std::vector<uint64_t> occ(n_occ ? n_occ : 1);
  if ((rc = fem_dev_fetch_index(h, lookup.data(), occ.data(), occ.size()))) return dev_fail(h, "index fetch", rc);
  fprintf(stderr, "Collected %lu seeds.\n", (unsigned long)n_occ);
  fprintf(stderr, "Lookup table size: %lu, occurrence table size: %lu.\n", (unsigned long)lookup.size(), (unsigned long)n_occ);
  fprintf(stderr, "Built index in %fs.\n", real_time() - t0);
  fem_dev_close(h);
  if (fem_index_save(out_path, k, step, lookup.data(), n_occ, occ.data()) != 0) {
    fprintf(stderr, "Write error while initializing hash table.\n");
    exit(EXIT_FAILURE);
  }
  return 0;
}

// ---------------------------------------------------------------- FEM map (src/FEM_map.c:57-227)
//
// The reference runs 1 reader + T mapping threads + 1 writer over two queues (src/FEM_map.c:172-198,
// src/input_queue.c, src/output_queue.c).  Here the T mapping threads are the GPUs:
//
//   reader     parses the next FASTQ window (all -t threads; bases, qualities, names) STRAIGHT INTO the pinned staging buffers of a free
//              (GPU, slot) pair — whichever GPU has one free, so the GPUs balance by themselves
//   worker[g]  one thread per GPU, the only one that talks to that GPU's handle: starts H2D + kernels of a filled
//              slot (asynchronous), keeps two batches in flight, then fetches the finished batch's SAM text
//              (sort + traceback + CIGAR/MD + the text itself run on the device, fem_dev_fetch_sam)
//   writer     writes the text
//   formatter  only with FEM_HOST_FORMAT=1 / FEM_HOST_TAIL=1: renders records as SAM text on the host threads
// A slot goes  free -> filled -> in flight -> fetched -> written -> free  and there are four per GPU.
template <typename T>
class Channel {  // unbounded hand-off between pipeline stages (the number of slots bounds what is in flight)
 public:
  void push(T v) {
    {
      std::lock_guard<std::mutex> l(m_);
      q_.push_back(std::move(v));
    }
    cv_.notify_one();
  }
  T pop() {
    std::unique_lock<std::mutex> l(m_);
    cv_.wait(l, [&] { return !q_.empty(); });
    T v = std::move(q_.front());
    q_.pop_front();
    return v;
  }
  bool try_pop_for(T &v, double seconds) {  // waits up to `seconds` for an element
    std::unique_lock<std::mutex> l(m_);
    if (!cv_.wait_for(l, std::chrono::duration<double>(seconds), [&] { return !q_.empty(); })) return false;
    v = std::move(q_.front());
    q_.pop_front();
    return true;
  }
  bool try_pop(T &v) {
    std::lock_guard<std::mutex> l(m_);
    if (q_.empty()) return false;
    v = std::move(q_.front());
    q_.pop_front();
    return true;
  }

 private:
  std::mutex m_;
  std::condition_variable cv_;
  std::deque<T> q_;
};

struct Growable {  // a reusable host array: only ever grows
  char *p = nullptr;
  uint64_t cap = 0;
  bool reserve(uint64_t n) {
    if (n <= cap) return true;
    const uint64_t want = n + n / 8 + 4096;
    char *q = (char *)realloc(p, want);
    if (!q) return false;
    p = q, cap = want;
    return true;
  }
  ~Growable() { free(p); }
};

constexpr int kCutKinds = 3;  // what cuts reads on the device in front of the mapping: the trims, --adapter, --trim-overlap (cut_kinds in map_main)

struct BatchBuf {  // everything about the batch that sits in one (GPU, slot) pair
  uint64_t seq = 0;  // submission number on its GPU: results are handed on in this order
  int gpu = 0, slot = 0;
  char *bases = nullptr;      // pinned staging lent by the device library (fem_dev_acquire_stage)
  uint64_t *off = nullptr;
  uint64_t reads_cap = 0, bases_cap = 0;
  Growable quals, names, name_off;  // host formatting (FEM_HOST_FORMAT=1 / FEM_HOST_TAIL=1): names and qualities stay on the host
  bool packed = false;                          // the parser wrote this batch at two bits per base (fem_seqfile_fill_packed)
  uint64_t n_exc = 0;                           // ... and this many characters outside "ACGT" behind the codes
  bool spliced = false;                         // ... and copied nothing else: names, bases, qualities stay in the input's mapping
  Growable r_name, r_name_len, r_seq, r_qual;   //     (where each read's fields lie: fem_seqfile_fill_packed_refs)
  fem_read_refs refs{};
  char *q_stage = nullptr, *n_stage = nullptr;  // device SAM text: pinned staging lent by the library
  uint64_t *no_stage = nullptr;
  uint64_t names_cap = 0, want_names = 0;
  fem_batch_sam sam{};
  fem_batch_shape shape{};
  uint64_t want_reads = 0, want_bases = 0;  // set by the reader when the staging buffers are too small
  fem_batch_records rec{};                  // device tail's records (default path)
  uint64_t n_proper = 0;                    // paired: proper pairs of the batch
  uint64_t n_rescued = 0;                   // --rescue: rescued mates of the batch
  uint64_t n_rescued_discordant = 0;        // --rescue-discordant: those of pairs whose records did not pair
  uint64_t n_unmapped = 0;                  // --unmapped: lines for unmapped reads of the batch
  uint64_t n_filtered = 0;                  // --strata / --max-hits: lines left out of the batch's text
  uint64_t n_xa = 0;                        // --xa: lines folded into XA:Z entries in the batch's text
  uint64_t n_cut[kCutKinds][2] = {};            // per cut kind: reads (--trim-overlap: pairs) of the batch with a cut, and the bases cut
  fem_batch_result res{};                   // per-candidate outcome (FEM_HOST_TAIL=1)
  double t_submit = 0;
  double t_slot = 0, t_filled = 0, t_submitted = 0, t_retired = 0, t_text = 0;  // FEM_STAGE_TIMES=2: the batch's way through the stages
};

struct TextOut {  // one batch of SAM text: parts[i] of buf, in order
  char *buf = nullptr;
  uint64_t cap = 0;
  std::vector<fem_text_part> parts;
  bool owned_elsewhere = false;  // buf was malloc'd by fem_tail_sam: free it after writing
};

enum MsgKind { kFilled, kRecycle, kRegrow, kStop };
struct Msg {
  MsgKind kind = kStop;
  BatchBuf *b = nullptr;
};

int map_main(int argc, char **argv) {
  // Batches come and go as a few 100 MB allocations: keep them in the heap instead of mapping and unmapping them, so
  // that a recycled buffer's pages are already there (page faults were a visible share of the host time).
  mallopt(M_MMAP_MAX, 0);
  mallopt(M_TRIM_THRESHOLD, -1);
  char *ref_path = nullptr, *index_path = nullptr, *read_path = nullptr, *read2_path = nullptr, *out_path = nullptr;
  long long min_insert = 0, max_insert = 500;
  long long rescue_edits = 0;  // --rescue (mate rescue at this many edits, fem_dev_set_rescue)
  bool rescue_given = false;
  // --infer-insert[=N]: the insert size range from the input's first N pairs (fem_dev_estimate_insert), -I / -X the fallback
  bool infer_insert = false;
  long long infer_pairs = 65536;
  // --orientation: FEM_ORIENT_FR / _RF / _FF (fem_dev_set_orientation); kOrientAuto: learned in --infer-insert's pre-pass
  // (fem_dev_estimate_library); -1: another word, refused below
  constexpr int kOrientAuto = 3;
  int orientation = FEM_ORIENT_FR;
  bool orientation_given = false;
  bool rescue_discordant = false;  // --rescue-discordant (fem_dev_set_rescue_discordant)
  int bam_level = -1;  // --bam[=LEVEL]: BAM records and BGZF members made on the device (fem_dev_fetch_bam); -1: SAM
  bool unmapped = false;  // --unmapped: a line for every read without a mapping, made on the device (fem_dev_set_unmapped)
  long long strata = -1, max_hits = -1;  // --strata / --max-hits: the line filter, made on the device (fem_dev_set_report); -1: off
  bool strata_given = false, max_hits_given = false;
  bool mapq = false;   // --mapq: MAPQ from the hit strata, made on the device (fem_dev_set_mapq); else 255 as the reference
  bool header = false;  // --header: @HD in front of the @SQ lines, @PG behind them
  const char *rg_arg = nullptr;  // --rg: the @RG line (implies --header) and RG:Z on every line, made on the device (fem_dev_set_tags)
  bool hit_tags = false;         // --nh: NH:i and HI:i on every mapped line, made on the device (fem_dev_set_tags)
  bool mate_tags = false;        // --mate-tags: MC:Z, MQ:i and ms:i on every line of a paired output, made on the device (fem_dev_set_mate_tags)
  bool sam_seq = false;          // --sam-seq: SEQ and QUAL of the lines with 0x10 in the reference's direction, made on the device (fem_dev_set_sam_seq)
  long long xa_entries = 0;      // --xa[=N]: secondary lines folded into XA:Z on the primary line, made on the device (fem_dev_set_xa); 0: off
  bool xa_given = false;
  // --trim5 / --trim3 / --trim-qual: every read trimmed on the device before it is mapped, the cut bases soft clips (fem_dev_set_trim)
  long long trim5 = 0, trim3 = 0, trim_qual = 0;
  bool trim_given = false;
  // --adapter / --adapter2 / --adapter-overlap / --adapter-err: the 3' adapter matched and cut on the device (fem_dev_set_adapter)
  const char *adapter1 = nullptr, *adapter2 = nullptr;
  long long adapter_overlap = 5, adapter_err = 10;
  bool adapter_overlap_given = false, adapter_err_given = false;
  // --trim-overlap / --trim-overlap-min / --trim-overlap-err: read-through found from the mates' overlap (fem_dev_set_pair_overlap)
  bool trim_overlap = false, trim_overlap_min_given = false, trim_overlap_err_given = false;
  long long trim_overlap_min = 20, trim_overlap_err = 10;
  // --coverage FILE / --coverage-window / --coverage-all / --coverage-mapq: windowed depth of the output lines, summed on the device
  // over the whole run and written as BED text at its end (fem_dev_set_coverage, fem_coverage_write)
  const char *coverage_path = nullptr;
  long long coverage_window = 1000, coverage_mapq = 0;
  bool coverage_window_given = false, coverage_all = false, coverage_mapq_given = false;
  fem_params params{12, 3, 2, 1};  // src/FEM_map.c:67-70: k and step are fixed, whatever the index header says
  int n_threads = 1, n_gpus = 1;
  // reads per batch: 250 k fills the pipeline soonest on small inputs; a batch costs three host round trips on its way through
  // the tail, which 1 M-read batches amortise on large ones (16 M reads of C2 to /dev/null: 105 -> 116 Mreads/s, 8 M of C3:
  // 71 -> 81; round 4) — chosen by the size of the read file unless --batch says otherwise
  uint64_t batch_reads = 250000;
  bool batch_given = false;
  const char *short_opt = "ha:f:e:t:o:r:i:b:I:X:";
  static struct option long_opt[] = {{"help", no_argument, nullptr, 'h'},       {"ref", required_argument, nullptr, 'r'},
                                     {"index", required_argument, nullptr, 'i'}, {"read1", required_argument, nullptr, 'b'},
                                     {"gpus", required_argument, nullptr, 'G'},  {"batch", required_argument, nullptr, 'B'},
                                     {"read2", required_argument, nullptr, 'c'}, {"minins", required_argument, nullptr, 'I'},
                                     {"maxins", required_argument, nullptr, 'X'}, {"rescue", required_argument, nullptr, 'R'},
                                     {"rescue-discordant", no_argument, nullptr, 'D'},
                                     {"infer-insert", optional_argument, nullptr, 'F'},
                                     {"orientation", required_argument, nullptr, 'O'},
                                     {"bam", optional_argument, nullptr, 'Z'},  {"mapq", no_argument, nullptr, 'Q'},
                                     {"unmapped", no_argument, nullptr, 'U'},
                                     {"strata", required_argument, nullptr, 'S'}, {"max-hits", required_argument, nullptr, 'N'},
                                     {"header", no_argument, nullptr, 'H'},      {"rg", required_argument, nullptr, 'T'},
                                     {"nh", no_argument, nullptr, 'n'},          {"mate-tags", no_argument, nullptr, 'M'},
                                     {"sam-seq", no_argument, nullptr, 'q'},
                                     {"xa", optional_argument, nullptr, 'x'},
                                     {"trim5", required_argument, nullptr, '5'},
                                     {"trim3", required_argument, nullptr, '3'},
                                     {"trim-qual", required_argument, nullptr, 'm'},
                                     {"adapter", required_argument, nullptr, 1001},
                                     {"adapter2", required_argument, nullptr, 1002},
                                     {"adapter-overlap", required_argument, nullptr, 1003},
                                     {"adapter-err", required_argument, nullptr, 1004},
                                     {"trim-overlap", no_argument, nullptr, 1005},
                                     {"trim-overlap-min", required_argument, nullptr, 1006},
                                     {"trim-overlap-err", required_argument, nullptr, 1007},
                                     {"coverage", required_argument, nullptr, 1008},
                                     {"coverage-window", required_argument, nullptr, 1009},
                                     {"coverage-all", no_argument, nullptr, 1010},
                                     {"coverage-mapq", required_argument, nullptr, 1011},
                                     {nullptr, 0, nullptr, 0}};
  int c, oi = 0;
  while ((c = getopt_long(argc, argv, short_opt, long_opt, &oi)) >= 0) {
    switch (c) {
      case 'H': header = true; break;
      case 'T': rg_arg = optarg, header = true; break;
      case 'n': hit_tags = true; break;
      case 'M': mate_tags = true; break;
      case 'q': sam_seq = true; break;
      case 'x':
        xa_given = true, xa_entries = 0x7FFFFFFFll;  // (alone: the byte budget bounds the folding)
        if (optarg) {
          char *end = nullptr;
          xa_entries = strtoll(optarg, &end, 10);
          if (!end || end == optarg || *end) xa_entries = -1;  // (not a number: refused below)
        }
        break;
      case '5':
      case '3':
      case 'm': {
        char *end = nullptr;
        long long v = strtoll(optarg, &end, 10);
        if (!end || end == optarg || *end) v = -1;  // (not a number: refused below)
        (c == '5' ? trim5 : c == '3' ? trim3 : trim_qual) = v;
        if (c == 'm' && v == 0) trim_qual = -1;  // (--trim-qual 0 is no quality: refused)
        trim_given = true;
        break;
      }
      case 1001: adapter1 = optarg; break;
      case 1002: adapter2 = optarg; break;
      case 1003:
      case 1004: {
        char *end = nullptr;
        long long v = strtoll(optarg, &end, 10);
        if (!end || end == optarg || *end) v = -1;  // (not a number: refused below)
        (c == 1003 ? adapter_overlap : adapter_err) = v;
        (c == 1003 ? adapter_overlap_given : adapter_err_given) = true;
        break;
      }
      case 1005: trim_overlap = true; break;
      case 1006:
      case 1007: {
        char *end = nullptr;
        long long v = strtoll(optarg, &end, 10);
        if (!end || end == optarg || *end) v = -1;  // (not a number: refused below)
        (c == 1006 ? trim_overlap_min : trim_overlap_err) = v;
        (c == 1006 ? trim_overlap_min_given : trim_overlap_err_given) = true;
        break;
      }
      case 1008: coverage_path = optarg; break;
      case 1010: coverage_all = true; break;
      case 1009:
      case 1011: {
        char *end = nullptr;
        long long v = strtoll(optarg, &end, 10);
        if (!end || end == optarg || *end) v = -1;  // (not a number: refused below)
        (c == 1009 ? coverage_window : coverage_mapq) = v;
        (c == 1009 ? coverage_window_given : coverage_mapq_given) = true;
        break;
      }
      case 'r': ref_path = optarg; break;
      case 'i': index_path = optarg; break;
      case 'b': read_path = optarg; break;
      case 'c': read2_path = optarg; break;
      case 'I': min_insert = strtoll(optarg, nullptr, 10); break;
      case 'X': max_insert = strtoll(optarg, nullptr, 10); break;
      case 'R': {
        char *end = nullptr;
        rescue_edits = strtoll(optarg, &end, 10);
        if (!end || end == optarg || *end) rescue_edits = -1;  // (not a number: refused below)
        rescue_given = true;
        break;
      }
      case 'Z':
        bam_level = !optarg ? 1 : strcmp(optarg, "0") == 0 ? 0 : strcmp(optarg, "1") == 0 ? 1 : -2;  // (-2: refused below)
        break;
      case 'D': rescue_discordant = true; break;
      case 'F':
        infer_insert = true;
        if (optarg) {
          char *end = nullptr;
          infer_pairs = strtoll(optarg, &end, 10);
          if (!end || end == optarg || *end) infer_pairs = -1;  // (not a number: refused below)
        }
        break;
      case 'O':
        orientation = strcmp(optarg, "fr") == 0 ? FEM_ORIENT_FR : strcmp(optarg, "rf") == 0 ? FEM_ORIENT_RF : strcmp(optarg, "ff") == 0 ? FEM_ORIENT_FF
                      : strcmp(optarg, "auto") == 0 ? kOrientAuto : -1;
        orientation_given = true;
        break;
      case 'Q': mapq = true; break;
      case 'U': unmapped = true; break;
      case 'S': {
        char *end = nullptr;
        strata = strtoll(optarg, &end, 10);
        if (!end || end == optarg || *end) strata = -2;  // (not a number: refused below)
        strata_given = true;
        break;
      }
      case 'N': {
        char *end = nullptr;
        max_hits = strtoll(optarg, &end, 10);
        if (!end || end == optarg || *end) max_hits = -2;  // (not a number: refused below)
        max_hits_given = true;
        break;
      }
      case 'e': params.e = atoi(optarg); break;
      case 't': n_threads = atoi(optarg); break;
      case 'a': params.a = atoi(optarg); break;
      case 'G': n_gpus = atoi(optarg); break;
      case 'B': batch_reads = strtoull(optarg, nullptr, 10), batch_given = true; break;
      case 'f':
        if (strcmp(optarg, "v") != 0 && strcmp(optarg, "g") != 0) {  // parsed and ignored (src/FEM_map.c:108-118)
          fprintf(stderr, "%s\n", "Wrong name of seeding algorithm!");
          usage_map();
          exit(EXIT_FAILURE);
        }
        break;
      case 'o': out_path = optarg; break;
      default:
        usage_map();
        exit(EXIT_SUCCESS);
    }
  }
  char *rg_line = nullptr, rg_id[256] = "";
  if (rg_arg) {
    char why[512] = "";
    if (fem_parse_read_group(rg_arg, &rg_line, rg_id, why, sizeof why) != 0) {
      fprintf(stderr, "Wrong --rg line: %s.\n", why[0] ? why : "out of memory");
      exit(EXIT_FAILURE);
    }
  }
  // check_args (src/FEM_map.c:29-55)
  const char *bad = nullptr;
  if (params.e < 0 || params.e > 7) bad = "Wrong error threshold.";
  else if (n_threads <= 0) bad = "Wrong number of threads.";
  else if (params.a < 0 || params.a > 2) bad = "Wrong number of additional q-grams.";
  else if (min_insert < 0 || max_insert < min_insert || max_insert > (1ll << 30)) bad = "Wrong insert size range.";
  else if (infer_insert && !read2_path) bad = "--infer-insert needs read pairs (--read2).";
  else if (infer_insert && (infer_pairs < 64 || infer_pairs > 262144)) bad = "Wrong number of pairs to infer from (64-262144).";
  else if (orientation < 0) bad = "Wrong library orientation (fr, rf, ff or auto).";
  else if (orientation_given && !read2_path) bad = "--orientation needs read pairs (--read2).";
  else if (orientation == kOrientAuto && !infer_insert) bad = "--orientation auto needs --infer-insert.";
  else if (mate_tags && !read2_path) bad = "--mate-tags needs --read2.";
  else if (rescue_discordant && !rescue_given) bad = "--rescue-discordant needs --rescue.";
  else if (rescue_given && !read2_path) bad = "--rescue needs read pairs (--read2).";
  else if (rescue_given && (rescue_edits < 0 || rescue_edits > 15)) bad = "Wrong rescue error threshold (0-15).";
  else if (rescue_given && max_insert - min_insert > 65536) bad = "--rescue searches insert size ranges of at most 65536.";
  else if (bam_level == -2) bad = "Wrong BAM compression level (0-1).";
  else if (strata_given && (strata < 0 || strata > 15)) bad = "Wrong number of strata (0-15).";
  else if (max_hits_given && (max_hits < 1 || max_hits > 0x7FFFFFFFll)) bad = "Wrong hit limit (>= 1).";
  else if (xa_given && xa_entries != 0x7FFFFFFFll && (xa_entries < 1 || xa_entries > 1000000)) bad = "Wrong number of --xa entries (1-1000000).";
  else if (trim5 < 0 || trim5 > 1024 || trim3 < 0 || trim3 > 1024) bad = "Wrong number of bases to trim (0-1024).";
  else if (trim_qual < 0 || trim_qual > 93) bad = "Wrong trimming quality (1-93).";
  else if (!adapter1 && (adapter2 || adapter_overlap_given || adapter_err_given)) bad = "--adapter2, --adapter-overlap and --adapter-err need --adapter.";
  else if (adapter2 && !read2_path) bad = "--adapter2 needs --read2.";
  else if ((adapter1 && !adapter_ok(adapter1)) || (adapter2 && !adapter_ok(adapter2))) bad = "Wrong adapter sequence (4-64 letters of ACGT).";
  else if (adapter1 && (adapter_overlap < 1 || adapter_overlap > (long long)std::min(strlen(adapter1), strlen(adapter2 ? adapter2 : adapter1))))
    bad = "Wrong adapter overlap (1 to the adapter's length).";
  else if (adapter1 && (adapter_err < 0 || adapter_err > 30)) bad = "Wrong adapter error percentage (0-30).";
  else if (!trim_overlap && (trim_overlap_min_given || trim_overlap_err_given)) bad = "--trim-overlap-min and --trim-overlap-err need --trim-overlap.";
  else if (trim_overlap && !read2_path) bad = "--trim-overlap needs read pairs (--read2).";
  else if (trim_overlap && (trim_overlap_min < 8 || trim_overlap_min > 1024)) bad = "Wrong overlap of the mates (8-1024).";
  else if (trim_overlap && (trim_overlap_err < 0 || trim_overlap_err > 30)) bad = "Wrong overlap error percentage (0-30).";
  else if (!coverage_path && (coverage_window_given || coverage_all || coverage_mapq_given)) bad = "--coverage-window, --coverage-all and --coverage-mapq need --coverage.";
  else if (coverage_path && (coverage_window < 1 || coverage_window > 1000000)) bad = "Wrong coverage window (1-1000000).";
  else if (coverage_mapq_given && (coverage_mapq < 1 || coverage_mapq > 60)) bad = "Wrong coverage MAPQ threshold (1-60).";
  else if (coverage_mapq_given && !mapq) bad = "--coverage-mapq needs --mapq.";
  else if (!ref_path) bad = "Reference file path is required.";
  else if (!index_path) bad = "Index file path is required.";
  else if (!read_path) bad = "Read file path is required.";
  else if (!out_path) bad = "Output file path is required.";
  else if (n_gpus < 1 || n_gpus > 64) bad = "Wrong number of GPUs.";
  else if (batch_reads < 1) bad = "Wrong batch size.";
  if (bad) {
    fprintf(stderr, "%s\n", bad);
    usage_map();
    exit(EXIT_FAILURE);
  }
  const char *pg_line = g_pg_line.empty() ? nullptr : g_pg_line.c_str();  // (no @PG line rather than an empty one)
  const bool bam = bam_level >= 0;
  for (const char *v : {"FEM_HOST_TAIL", "FEM_HOST_FORMAT", "FEM_HOST_QUALS"}) {  // (BAM records are made on the device, from its qualities)
    const char *x = getenv(v);
    if (bam && x && x[0] == '1') {
      fprintf(stderr, "--bam is not supported with %s=1: BAM records are made on the device, with the qualities there.\n", v);
      exit(EXIT_FAILURE);
    }
  }
  for (const char *v : {"FEM_HOST_TAIL", "FEM_HOST_FORMAT", "FEM_HOST_QUALS"}) {  // (nor can ms:i be: it is a sum over the mate's qualities)
    const char *x = getenv(v);
    if (mate_tags && x && x[0] == '1') {
      fprintf(stderr, "--mate-tags is not supported with %s=1: the mate tags are made on the device, with the qualities there.\n", v);
      exit(EXIT_FAILURE);
    }
  }
  for (const char *v : {"FEM_HOST_TAIL", "FEM_HOST_FORMAT", "FEM_HOST_QUALS"}) {  // (nor QUAL reversed: the host would fill it in forward)
    const char *x = getenv(v);
    if (sam_seq && x && x[0] == '1') {
      fprintf(stderr, "--sam-seq is not supported with %s=1: SEQ and QUAL are turned on the device, with the qualities there.\n", v);
      exit(EXIT_FAILURE);
    }
  }
  // what --trim5 / --trim3 / --trim-qual steer, --adapter and --trim-overlap steer too: a batch with any is a trimmed batch on the device
  const bool clip_given = trim_given || adapter1 != nullptr || trim_overlap;
  // The cut kinds of the device's trim stage, a row each: whether its options were given, whether its counters
  // are read (the trimmed reads and bases are those of every kind), its count call, its refusal and its two lines on stderr.
  const struct {
    bool given, counted;
    int (*count)(fem_dev *, int, uint64_t *, uint64_t *);
    const char *refusal, *line[2];
  } cut_kinds[kCutKinds] = {
      {trim_given, clip_given, fem_dev_trim_count,
       "--trim5, --trim3 and --trim-qual are not supported with %s=1: the reads are trimmed and their soft clips written on the device, with the qualities there.\n",
       {"The number of trimmed reads", "The number of trimmed bases"}},
      {adapter1 != nullptr, adapter1 != nullptr, fem_dev_adapter_count,
       "--adapter is not supported with %s=1: the adapter is cut and the soft clips written on the device, with the qualities there.\n",
       {"The number of reads with adapter", "The number of adapter bases"}},
      {trim_overlap, trim_overlap, fem_dev_pair_overlap_count,
       "--trim-overlap is not supported with %s=1: the mates are cut and the soft clips written on the device, with the qualities there.\n",
       {"The number of pairs with overlap cut", "The number of overlap bases"}}};
  for (const auto &kind : cut_kinds) {  // (nor the whole read around its kept part: clips, SEQ and QUAL are the device's)
    for (const char *v : {"FEM_HOST_TAIL", "FEM_HOST_FORMAT", "FEM_HOST_QUALS"}) {
      const char *x = getenv(v);
      if (kind.given && x && x[0] == '1') {
        fprintf(stderr, kind.refusal, v);
        exit(EXIT_FAILURE);
      }
    }
  }
  for (const char *v : {"FEM_HOST_TAIL", "FEM_HOST_FORMAT"}) {  // (the host formatter has no MAPQ path)
    const char *x = getenv(v);
    if (mapq && x && x[0] == '1') {
      fprintf(stderr, "--mapq is not supported with %s=1: mapping qualities are made on the device, with its SAM text or BAM.\n", v);
      exit(EXIT_FAILURE);
    }
    if (unmapped && x && x[0] == '1') {  // (nor lines for unmapped reads)
      fprintf(stderr, "--unmapped is not supported with %s=1: the lines of unmapped reads are made on the device, with its SAM text or BAM.\n", v);
      exit(EXIT_FAILURE);
    }
    if ((rg_arg || hit_tags) && x && x[0] == '1') {  // (nor tags)
      fprintf(stderr, "--rg and --nh are not supported with %s=1: the tags are made on the device, with its SAM text or BAM.\n", v);
      exit(EXIT_FAILURE);
    }
    if (xa_given && x && x[0] == '1') {  // (nor XA:Z: the folding acts on the device's lines; FEM_HOST_QUALS=1 is served, XA stands behind QUAL)
      fprintf(stderr, "--xa is not supported with %s=1: the secondary lines are folded on the device, with its SAM text or BAM.\n", v);
      exit(EXIT_FAILURE);
    }
    if (coverage_path && x && x[0] == '1') {  // (nor a coverage track: it is summed from the device's lines)
      fprintf(stderr, "--coverage is not supported with %s=1: the coverage track is summed on the device, from the lines of its SAM text or BAM.\n", v);
      exit(EXIT_FAILURE);
    }
    if ((strata_given || max_hits_given) && x && x[0] == '1') {  // (nor a line filter)
      fprintf(stderr, "--strata and --max-hits are not supported with %s=1: the lines are filtered on the device, with its SAM text or BAM.\n", v);
      exit(EXIT_FAILURE);
    }
  }
  const bool report = strata_given || max_hits_given;

  // Host placement: with one GPU the whole process (parser, formatter, staging buffers) moves next to it, before any
  // thread pool exists; with several, each GPU's worker thread does so for itself and the buffers it acquires.
  const char *sg = getenv("FEM_TEST_SHARE_GPU"), *tg = getenv("FEM_TESTING");  // (test hook: honoured under FEM_TESTING=1 only)
  const bool share_gpu = sg && sg[0] == '1' && tg && tg[0] == '1';
  if (n_gpus == 1 || share_gpu) (void)fem_bind_thread_near_device(0);
  Reference ref;
  if (!ref.load(ref_path)) exit(EXIT_FAILURE);
  // --coverage: the track's windows, from the sequences' lengths alone, before the index is read and before any device is opened
  std::vector<uint64_t> coverage_off;
  uint64_t coverage_bins = 0;
  if (coverage_path) {
    coverage_off.resize((size_t)ref.view.n_seq + 1);
    if (fem_coverage_layout(ref.view.n_seq, ref.view.len, (int32_t)coverage_window, coverage_off.data(), &coverage_bins) != 0) {
      const int32_t least = fem_coverage_min_window(ref.view.n_seq, ref.view.len);
      if (least) fprintf(stderr, "--coverage-window %lld gives %lu windows on this reference, more than 2^29; the least window that fits is %d.\n",
                         coverage_window, (unsigned long)coverage_bins, least);
      else fprintf(stderr, "--coverage: this reference has more than 2^29 windows at every window up to 1000000.\n");
      exit(EXIT_FAILURE);
    }
  }
  double t_idx = real_time();
  int32_t ik = 0, istep = 0;
  uint32_t *lookup = nullptr;
  uint64_t *occ = nullptr, n_occ = 0;
  if (fem_index_load(index_path, &ik, &istep, &lookup, &n_occ, &occ) != 0) {
    fprintf(stderr, "Failed to open index file %s\n", index_path);
    exit(EXIT_FAILURE);
  }
  fprintf(stderr, "Loaded index in %fs!\n", real_time() - t_idx);
  if (ik != params.k) {  // the reference would silently index a 4^12 table with the wrong hashes; refuse instead
    fprintf(stderr, "Index was built with k=%d but map always uses k=%d.\n", ik, params.k);
    exit(EXIT_FAILURE);
  }

  const char *ht = getenv("FEM_HOST_TAIL");
  const bool host_tail = ht && ht[0] == '1';
  // Where the SAM text is made.  Default: on the device (fem_dev_fetch_sam: qualities and names go there with the bases, the
  // finished text comes back: ~365 bytes per read over the link).  FEM_HOST_FORMAT=1: the device maps, orders, traces back and
  // hands over RECORDS (FLAG, RNAME id, POS, CIGAR, NM, MD: ~30 bytes per read) and the host threads splice them between
  // QNAME, SEQ and QUAL, which never leave the host — for a plain FASTQ file they are not even copied: the formatter reads them
  // out of the input's mapping (fem_seqfile_fill_packed_refs; FEM_SPLICE=0: copied by the parser).  ~55 bytes per read cross
  // the link; the price is ~0.07 core-microseconds of formatting per read, which on a 16-core share of the host is more than
  // the link costs (measured, 16 M reads of C2 to /dev/null: 75-93 Mreads/s against 100-117), so it is the
  // option, not the default.  FEM_HOST_TAIL=1: ordering, traceback and text by the host threads from the per-candidate outcome.
  const char *hf = getenv("FEM_HOST_FORMAT"), *spl = getenv("FEM_SPLICE");
  const bool device_text = !host_tail && !(hf && hf[0] == '1');
  // Read pairs: paired and rendered on the device only (fem_dev_set_pairs), the reads staged as characters.
  const bool paired = read2_path != nullptr;
  if (paired && !device_text) {
    fprintf(stderr, "%s is not supported with --read2: the paired SAM text is made on the device only.\n",
            host_tail ? "FEM_HOST_TAIL=1" : "FEM_HOST_FORMAT=1");
    exit(EXIT_FAILURE);
  }
  // ... with the qualities kept on the host (fem_dev_commit_names_stage: the device leaves their field open and the batch's
  // retiring thread fills it in): they are 228 of the 473 bytes per read on the link otherwise — and 0.027 core-µs per read on
  // the host then, next to the parser's 0.078.  With 16 cores per GPU the two forms are within +7 / -16 % of each other from box
  // to box (the run is bound by the link in one and by the cores in the other); from 24 threads on the qualities stay on the
  // host.  FEM_HOST_QUALS=1 / FEM_DEVICE_QUALS=1 decide it by hand.
  const char *dq = getenv("FEM_DEVICE_QUALS"), *hq = getenv("FEM_HOST_QUALS");
  const bool host_quals = device_text && !bam && !mate_tags && !sam_seq && !clip_given && !(dq && dq[0] == '1') && ((hq && hq[0] == '1') || n_threads >= 24);
  const bool splice = !host_tail && !device_text && !(spl && spl[0] == '0');
  // With the text on the device the link is what bounds the run: batches of equal-length reads then cross it at two bits per
  // base — the parser writes that form straight into the pinned staging (fem_seqfile_fill_packed ->
  // fem_dev_commit_stage_packed: no host work per base beyond the parse itself) (FEM_PACK_BASES=0: always as characters).
  const char *pk = getenv("FEM_PACK_BASES");
  const bool pack_bases = !host_tail && !paired && !clip_given && !(pk && pk[0] == '0');  // (a trimmed batch goes as characters: the trim stage reads them)
  if (!batch_given) {
    struct stat st;
    if (stat(read_path, &st) == 0 && st.st_size >= (off_t)(1ll << 30)) batch_reads = 1000000;  // (plain FASTQ of >= ~4 M reads)
  }
  const uint64_t batch_bytes = batch_reads * 250ull;  // header + bases + '+' + qualities of a ~100 bp record
  // a FASTQ window of batch_bytes characters holds fewer than batch_bytes / 2 bases; records under 32 bytes are unusual
  // (the reader asks for larger buffers when a batch needs them)
  const uint64_t reads_cap0 = batch_bytes / 32 + 16, bases_cap0 = batch_bytes / 2 + 4096, names_cap0 = bases_cap0 / 2 + 4096;
  std::vector<fem_dev *> devs((size_t)n_gpus, nullptr);
  // FEM_TEST_SHARE_GPU=1 (test hook for one-GPU boxes): all `--gpus N` workers open GPU 0, each with its own handle, and
  // the counters are summed on the host (RCCL refuses two ranks on one device)
  // What a batch will look like, from the input's first records: the device library then makes a batch's allocations during
  // the setup (fem_dev_reserve_batch) instead of between the first batches' kernels.
  uint64_t res_reads = 0;
  uint32_t res_len = 0;
  if (device_text) {
    if (fem_seqfile *f0 = fem_seqfile_open(read_path)) {
      fem_batch_plan *pl = nullptr;
      fem_batch_shape sh{};
      if (fem_seqfile_plan(f0, 1u << 18, 1, &pl, &sh) == 0 && pl && sh.n_reads > 0) {
        const uint64_t per_record = (2 * sh.n_bases + sh.n_name_bytes) / sh.n_reads + 6;
        res_reads = batch_bytes / per_record + batch_bytes / per_record / 8 + 1024, res_len = sh.max_len;
      }
      fem_batch_plan_free(pl);
      fem_seqfile_close(f0);
    }
  }
  (void)fem_set_blocking_waits(1);  // (a thread per batch in flight waits for the device; the parser needs the cores)
  const double t_dev = real_time();
  {  // one thread per GPU uploads the replicated reference + index (src/FEM_map.c:135-143)
    std::vector<int> up_rc((size_t)n_gpus, 0);
    std::vector<std::thread> up;
    for (int g = 0; g < n_gpus; ++g)
      up.emplace_back([&, g] {
        if (n_gpus > 1 && !share_gpu) (void)fem_bind_thread_near_device(g);  // the handle's pinned result buffers
        int rc = fem_dev_open(share_gpu ? 0 : g, &devs[(size_t)g]);
        if (!rc) rc = ref.upload(devs[(size_t)g]);
        if (!rc) rc = fem_dev_upload_index(devs[(size_t)g], ik, istep, lookup, ((uint64_t)1 << (2 * ik)) + 1, occ, n_occ);
        // the slots' pinned staging (and, for the device's SAM text, its buffers): pinning host memory takes ~0.25 ms per
        // MB, 35 ms per slot here, and belongs to the setup rather than to the first batches
        int32_t ns = 4;
        uint32_t max_read_len = 0;
        if (!rc) (void)fem_dev_limits(devs[(size_t)g], &max_read_len, &ns);
        for (int sl = 0; !rc && sl < ns; ++sl) {
          char *pb = nullptr, *pq = nullptr, *pn = nullptr;
          uint64_t *po = nullptr, *pno = nullptr;
          rc = fem_dev_acquire_stage(devs[(size_t)g], sl, reads_cap0, bases_cap0, &pb, &po);
          if (!rc && device_text) rc = fem_dev_acquire_text_stage(devs[(size_t)g], sl, reads_cap0, bases_cap0, names_cap0, &pq, &pn, &pno);
          if (!rc && device_text) rc = fem_dev_reserve_text(devs[(size_t)g], sl, reads_cap0, bases_cap0, names_cap0,
                                                                  // (--unmapped: a read of which nothing maps still has a line of its name, bases and qualities)
                                                                  // (--rg / --nh: the tags of a line, one line per read at the least)
                                                                  batch_bytes + batch_bytes / (unmapped ? 2 : 4) +
                                                                      // (--mate-tags: MC of a few operations, MQ, ms)
                                                                      reads_cap0 * ((rg_arg ? 6 + strlen(rg_id) : 0) + (hit_tags ? 16 : 0) + (mate_tags ? 16 + 9 + 12 : 0) +
                                                                                    // (trimming: two S operations on a line's CIGAR and on its MC; the clipped letters are part of the read's already)
                                                                                    (clip_given ? 10 + (mate_tags ? 10 : 0) : 0)));
          // (a read over the device's limit among the first records: no reservation, the staging of its batch names the read)
          if (!rc && device_text && res_reads && res_len <= max_read_len) rc = fem_dev_reserve_batch(devs[(size_t)g], sl, res_reads, res_reads + res_reads / 8, res_len, &params);
          if (!rc && mapq) rc = fem_dev_set_mapq(devs[(size_t)g], sl, 1);
          if (!rc && unmapped) rc = fem_dev_set_unmapped(devs[(size_t)g], sl, 1);
          if (!rc && report) {
            const fem_report_params fp{(int32_t)strata, (int32_t)max_hits};
            rc = fem_dev_set_report(devs[(size_t)g], sl, &fp);
          }
          if (!rc && (rg_arg || hit_tags)) {
            const fem_tag_params tp{rg_arg ? rg_id : nullptr, hit_tags ? 1 : 0};
            rc = fem_dev_set_tags(devs[(size_t)g], sl, &tp);
          }
          if (!rc && sam_seq) rc = fem_dev_set_sam_seq(devs[(size_t)g], sl, 1);
          if (!rc && xa_given) rc = fem_dev_set_xa(devs[(size_t)g], sl, (int32_t)xa_entries);
          if (!rc && trim_given) {
            const fem_trim_params tp{(int32_t)trim5, (int32_t)trim3, (int32_t)trim_qual};
            rc = fem_dev_set_trim(devs[(size_t)g], sl, &tp);
          }
          if (!rc && adapter1) {
            const fem_adapter_params ap{adapter1, adapter2, (int32_t)adapter_overlap, (int32_t)adapter_err};
            rc = fem_dev_set_adapter(devs[(size_t)g], sl, &ap);
          }
          if (!rc && trim_overlap) {
            const fem_pair_overlap_params vp{(int32_t)trim_overlap_min, (int32_t)trim_overlap_err};
            rc = fem_dev_set_pair_overlap(devs[(size_t)g], sl, &vp);
          }
          if (!rc && paired) {
            const fem_pair_params pp{(int32_t)min_insert, (int32_t)max_insert};
            rc = fem_dev_set_pairs(devs[(size_t)g], sl, &pp);
            if (!rc && orientation_given && orientation != kOrientAuto) rc = fem_dev_set_orientation(devs[(size_t)g], sl, orientation);
            if (!rc && mate_tags) rc = fem_dev_set_mate_tags(devs[(size_t)g], sl, 1);
            if (!rc && rescue_given) {
              const fem_rescue_params rp{(int32_t)rescue_edits};
              rc = fem_dev_set_rescue(devs[(size_t)g], sl, &rp);
              if (!rc && rescue_discordant) rc = fem_dev_set_rescue_discordant(devs[(size_t)g], sl, 1);
            }
          }
        }
        up_rc[(size_t)g] = rc;
      });
    for (auto &t : up) t.join();
    for (int g = 0; g < n_gpus; ++g)
      if (up_rc[(size_t)g]) return dev_fail(devs[(size_t)g], "device setup (mapping runs on the GPU; no CPU path)", up_rc[(size_t)g]);
  }
  free(lookup), free(occ);
  fprintf(stderr, "Reference and index resident on %d GPU%s in %fs.\n", n_gpus, n_gpus > 1 ? "s" : "", real_time() - t_dev);

  // --infer-insert: the insert size range from the input's first pairs, before anything is written and before the first batch
  // is read: the sample is mapped single-end on the first device and its unique pairs say what the library's inserts are
  // (fem_dev_estimate_insert).  The range then holds for the whole run, whatever --batch, -t and --gpus are; the main pass reads
  // the input from its start and counts nothing of this.  Files that do not give as many records each, or a sample the reader
  // cannot parse: no estimate, and the main pass reports the input as it does without the switch.
  // --orientation auto: the same sample says which orientation the library has, too (fem_dev_estimate_library): the one under
  // which most of its unique pairs are informative; the range is then that orientation's.
  if (infer_insert) {
    const bool learn_orientation = orientation == kOrientAuto;
    fem_library_estimate lib{};
    lib.orientation = -1;
    const double t_pre = real_time();
    fem_seqset mate[2] = {};
    bool sampled = true;
    for (int m = 0; m < 2; ++m) {
      fem_seqfile *f = fem_seqfile_open(m ? read2_path : read_path);
      sampled = sampled && f && fem_seqfile_read(f, (uint64_t)infer_pairs, &mate[m]) == 0;
      if (f) fem_seqfile_close(f);
    }
    sampled = sampled && mate[0].n == mate[1].n;
    int rc = 0;
    fem_insert_estimate est{};
    est.q25 = est.q50 = est.q75 = -1;
    if (sampled && mate[0].n) {  // mate 1's reads, then mate 2's, as one batch
      const uint64_t np = mate[0].n, b1 = mate[0].off[np], b2 = mate[1].off[np];
      std::vector<char> bases((size_t)(b1 + b2));
      std::vector<uint64_t> off((size_t)(2 * np + 1));
      if (b1) memcpy(bases.data(), mate[0].bases, (size_t)b1);
      if (b2) memcpy(bases.data() + b1, mate[1].bases, (size_t)b2);
      for (uint64_t i = 0; i <= np; ++i) off[(size_t)i] = mate[0].off[i], off[(size_t)(np + i)] = b1 + mate[1].off[i];
      const fem_read_batch sample{bases.data(), off.data(), 2 * np};
      fem_dev *h = devs[0];
      rc = fem_dev_stage_reads(h, 0, &sample);  // (slot 0 carries the run's trimming: the sample is trimmed as the run's reads will be)
      if (!rc && trim_qual > 0) {  // ... by its qualities, which go to the device in front of the mapping then; the names are not needed: empty ones
        char *pq = nullptr, *pn = nullptr;
        uint64_t *pno = nullptr;
        sampled = mate[0].quals && mate[1].quals;
        rc = !sampled ? FEM_OK : fem_dev_acquire_text_stage(h, 0, 2 * np, b1 + b2, 0, &pq, &pn, &pno);
        if (!rc && sampled) {
          if (b1) memcpy(pq, mate[0].quals, (size_t)b1);
          if (b2) memcpy(pq + b1, mate[1].quals, (size_t)b2);
          memset(pno, 0, (size_t)(2 * np + 1) * sizeof(uint64_t));
          rc = fem_dev_commit_text_stage(h, 0, 2 * np, 0);
        }
      }
      if (!rc && sampled) rc = fem_dev_map_staged(h, 0, &params);
      if (!rc && sampled) rc = learn_orientation ? fem_dev_estimate_library(h, 0, &lib) : fem_dev_estimate_insert(h, 0, &est);
      if (rc) dev_fail(h, "insert size estimate", rc);
    }
    for (fem_seqset &s : mate) fem_seqset_free(&s);
    if (rc) return EXIT_FAILURE;
    if (learn_orientation) {
      static const char *const kOrientName[3] = {"FR", "RF", "FF"};
      const unsigned long a = (unsigned long)lib.by[0].n_informative, b = (unsigned long)lib.by[1].n_informative,
                          c3 = (unsigned long)lib.by[2].n_informative, S = (unsigned long)lib.by[0].n_pairs;
      if (sampled && lib.orientation >= 0) {
        orientation = lib.orientation, est = lib.by[lib.orientation];
        fprintf(stderr, "Inferred library orientation: %s (FR %lu, RF %lu, FF %lu informative of %lu pairs).\n", kOrientName[orientation], a, b, c3, S);
      } else {
        orientation = FEM_ORIENT_FR, est.estimated = 0;
        if (sampled)
          fprintf(stderr, "Library orientation not inferred (FR %lu, RF %lu, FF %lu informative of %lu pairs, %d needed): using FR, %lld-%lld.\n", a, b,
                  c3, S, FEM_INSERT_MIN_PAIRS, min_insert, max_insert);
      }
    }
    if (sampled && est.estimated) {
      const fem_pair_params pp{est.min_insert, est.max_insert};
      for (fem_dev *h : devs) {
        int32_t ns = 4;
        (void)fem_dev_limits(h, nullptr, &ns);
        for (int sl = 0; sl < ns; ++sl) {
          if ((rc = fem_dev_set_pairs(h, sl, &pp))) return dev_fail(h, "insert size range", rc);
          if (learn_orientation && (rc = fem_dev_set_orientation(h, sl, orientation))) return dev_fail(h, "library orientation", rc);
        }
      }
      fprintf(stderr, "Inferred insert size range: %d-%d (quartiles %d %d %d, %lu informative of %lu pairs).\n", est.min_insert, est.max_insert,
              est.q25, est.q50, est.q75, (unsigned long)est.n_informative, (unsigned long)est.n_pairs);
    } else if (sampled && !learn_orientation) {
      fprintf(stderr, "Insert size range not inferred (%lu informative of %lu pairs, %d needed): using %lld-%lld.\n",
              (unsigned long)est.n_informative, (unsigned long)est.n_pairs, FEM_INSERT_MIN_PAIRS, min_insert, max_insert);
    }
    const char *st = getenv("FEM_STAGE_TIMES");
    if (st && (st[0] == '1' || st[0] == '2')) fprintf(stderr, "[FEM] insert size pre-pass: %fs\n", real_time() - t_pre);
  }
  // --coverage: every device keeps a track of its own from here on (behind the sample pass, which adds nothing to it); the host
  // sums them at the end
  if (coverage_path) {
    const fem_coverage_params cp{(int32_t)coverage_window, coverage_all ? 1 : 0, (int32_t)coverage_mapq};
    for (fem_dev *h : devs)
      if (int rc = fem_dev_set_coverage(h, &cp)) return dev_fail(h, "coverage track", rc);
  }

  const int out_fd = open(out_path, O_WRONLY | O_CREAT | O_TRUNC, 0666);
  if (out_fd < 0) {
    fprintf(stderr, "Cannot open output file %s\n", out_path);
    exit(EXIT_FAILURE);
  }
  std::atomic<int> exit_code{0};
  // The SAM text of a batch is a handful of stretches (one per formatter thread), written one after the other.  (Side
  // by side with pwrite from four threads was tried twice: round 3 on tmpfs, 2.8 GB/s against 5.5 from one thread; round 5 on
  // the GPU box's /tmp, where four writers into four FILES take 56-61 GB/s against 16.5 from one: into ONE file 10.4 GB/s with
  // one, four or eight writers — buffered writes to a file take its inode's lock.)
  auto write_all = [&](const char *p, uint64_t n) -> bool {
    while (n) {
      ssize_t w = write(out_fd, p, n);
      if (w < 0 && errno == EINTR) continue;
      if (w <= 0) return false;
      p += w, n -= (uint64_t)w;
    }
    return true;
  };
  if (bam) {  // the BAM header, through the device's compressor
    uint8_t *raw = nullptr;
    uint64_t rl = 0, zl = 0;
    int rc = header ? fem_bam_header_full(&ref.view, rg_line, pg_line, &raw, &rl) : fem_bam_header(&ref.view, &raw, &rl);
    if (rc == -5) {
      fprintf(stderr, "A reference sequence of 2^31 bases or more cannot be written as BAM.\n");
      exit(EXIT_FAILURE);
    }
    if (rc) {
      fprintf(stderr, "BAM header failed (%d)\n", rc);
      exit(EXIT_FAILURE);
    }
    std::vector<uint8_t> z((size_t)(rl / 65280 + 1) * 65536);
    rc = fem_dev_bgzf_compress(devs[0], raw, rl, bam_level, z.data(), z.size(), &zl);
    free(raw);
    if (rc) return dev_fail(devs[0], "BAM header", rc);
    if (!write_all((const char *)z.data(), zl)) {
      fprintf(stderr, "[FEM] write error on %s\n", out_path);
      exit_code = EXIT_FAILURE;
    }
  } else {
    char *hdr = nullptr;
    uint64_t hl = 0;
    if (header) fem_sam_header_full(&ref.view, rg_line, pg_line, &hdr, &hl);
    else fem_sam_header(&ref.view, &hdr, &hl);
    if (!write_all(hdr, hl)) {
      fprintf(stderr, "[FEM] write error on %s\n", out_path);
      exit_code = EXIT_FAILURE;
    }
    free(hdr);
  }
  free(rg_line);

  if (device_text)
    for (fem_dev *h : devs) {
      int rc = fem_dev_upload_reference_names(h, (uint32_t)ref.set.n, ref.set.names, ref.set.name_off);
      if (rc) return dev_fail(h, "reference names", rc);
    }

  double t_start = real_time();
  auto cpu_seconds = [](double *user, double *sys) {
    struct rusage ru;
    getrusage(RUSAGE_SELF, &ru);
    *user = ru.ru_utime.tv_sec + 1e-6 * ru.ru_utime.tv_usec, *sys = ru.ru_stime.tv_sec + 1e-6 * ru.ru_stime.tv_usec;
  };
  double cpu_u0 = 0, cpu_s0 = 0;
  cpu_seconds(&cpu_u0, &cpu_s0);
  // -t threads are shared by the two host stages that run side by side (FEM_SPLIT_THREADS=0: each gets all of them)
  const char *sp_env = getenv("FEM_SPLIT_THREADS");
  const bool split = !(sp_env && sp_env[0] == '0') && n_threads >= 4;
  int rd_share = 50;  // per cent of the threads that parse (FEM_READER_SHARE)
  if (const char *rs = getenv("FEM_READER_SHARE")) rd_share = std::min(90, std::max(10, atoi(rs)));
  const int rd_threads = !device_text && split ? std::max(1, std::min(n_threads - 1, (n_threads * rd_share + 50) / 100)) : n_threads;
  const int fmt_threads = !device_text && split ? n_threads - rd_threads : n_threads;
  int32_t n_slots = 4;
  (void)fem_dev_limits(devs[0], nullptr, &n_slots);
  // FEM_STAGE_TIMES=1: busy seconds of each pipeline stage on stderr at the end
  const char *st_env = getenv("FEM_STAGE_TIMES");
  const bool stage_times = st_env && (st_env[0] == '1' || st_env[0] == '2');
  const bool batch_times = st_env && st_env[0] == '2';  // ... =2: and every batch's way through them, and the form its bases took
  double busy_read = 0, busy_text = 0, busy_write = 0, busy_plan = 0;
  std::mutex stat_mu;  // (busy_text: the batches' retiring threads add to it)
  double wait_slot = 0, wait_records = 0, wait_text_buf = 0;  // reader waiting for a free slot, formatter for records / a text buffer
  std::vector<double> busy_submit((size_t)n_gpus, 0.0), busy_recycle((size_t)n_gpus, 0.0);
  double t_first_slot = 0, t_first_filled = 0, t_reader_done = 0, t_workers_done = 0;
  std::vector<double> busy_wait((size_t)n_gpus, 0.0);
  std::atomic<uint64_t> n_asserted{0};

  std::vector<BatchBuf> bufs((size_t)n_gpus * (size_t)n_slots);
  Channel<BatchBuf *> free_q, text_q, regrown_q;
  std::vector<Channel<Msg>> work_q((size_t)n_gpus);
  struct WriteItem {
    TextOut *t = nullptr;   // host-rendered text, or
    BatchBuf *b = nullptr;  // a batch whose text the device rendered (b->sam)
  };
  Channel<TextOut *> text_free_q;
  Channel<WriteItem> write_q;
  std::vector<TextOut> texts(3);
  for (TextOut &t : texts) text_free_q.push(&t);
  std::vector<uint64_t> per_gpu((size_t)n_gpus * 5, 0), per_gpu_proper((size_t)n_gpus, 0),
      per_gpu_rescued((size_t)n_gpus, 0), per_gpu_rescued_disc((size_t)n_gpus, 0), per_gpu_unmapped((size_t)n_gpus, 0), per_gpu_filtered((size_t)n_gpus, 0), per_gpu_xa((size_t)n_gpus, 0),
      per_gpu_cut((size_t)n_gpus * kCutKinds * 2, 0);

  // ---- writer (src/output_queue.c:60-91) ----
  std::thread writer([&] {
    for (;;) {
      WriteItem it = write_q.pop();
      if (!it.t && !it.b) break;
      if (it.b) {  // text rendered on the device: one stretch of the library's pinned memory
        const int wrc = fem_dev_sam_wait(devs[(size_t)it.b->gpu], it.b->slot);  // the copy of the text to the host has arrived
        // (this thread must not read the handle's error string, which the GPU's worker thread may be writing: the code says enough)
        if (wrc && !exit_code.exchange(EXIT_FAILURE)) fprintf(stderr, "[FEM] SAM text failed: %s\n", fem_strerror(wrc));
        double t0 = real_time();
        it.b->t_text = t0;
        const double t_w = real_time();
        bool ok = wrc != 0 || it.b->sam.len == 0 || write_all(it.b->sam.text, it.b->sam.len);
        if (!ok && !exit_code.exchange(EXIT_FAILURE)) fprintf(stderr, "[FEM] write error on %s\n", out_path);
        busy_write += real_time() - t_w;
        fprintf(stderr, "Mapped read batch in %fs.\n", real_time() - it.b->t_submit);
        if (batch_times)
          fprintf(stderr, "[FEM] batch %lu gpu %d slot %d (ms): slot %.2f filled %.2f submit %.2f..%.2f retired %.2f text home %.2f written %.2f; "
                          "bases sent as %s\n",
                  (unsigned long)it.b->seq, it.b->gpu, it.b->slot, 1e3 * (it.b->t_slot - t_start), 1e3 * (it.b->t_filled - t_start),
                  1e3 * (it.b->t_submit - t_start), 1e3 * (it.b->t_submitted - t_start), 1e3 * (it.b->t_retired - t_start),
                  1e3 * (it.b->t_text - t_start), 1e3 * (real_time() - t_start), it.b->packed ? "2-bit codes" : "characters");
        free_q.push(it.b);  // written: the slot's buffers may be refilled
        continue;
      }
      TextOut *t = it.t;
      double t0 = real_time();
      bool ok = true;
      for (const fem_text_part &p : t->parts)
        if (ok && p.length) ok = write_all(t->buf + p.offset, p.length);
      if (!ok && !exit_code.exchange(EXIT_FAILURE)) fprintf(stderr, "[FEM] write error on %s\n", out_path);
      if (t->owned_elsewhere) {
        free(t->buf);
        t->buf = nullptr, t->cap = 0, t->owned_elsewhere = false;
      }
      busy_write += real_time() - t0;
      text_free_q.push(t);
    }
  });

  // ---- formatter: records -> SAM text (src/align.c:546-632, src/output_queue.c:93-116) ----
  std::thread formatter([&] {
    for (;;) {
      const double t_pop = real_time();
      BatchBuf *b = text_q.pop();
      if (!b) break;
      const double t_got = real_time();
      wait_records += t_got - t_pop;
      TextOut *t = text_free_q.pop();
      double t0 = real_time();
      wait_text_buf += t0 - t_got;
      fem_seqset reads{};
      reads.n = b->shape.n_reads, reads.bases = b->bases, reads.off = b->off, reads.quals = b->quals.p, reads.names = b->names.p;
      reads.name_off = (uint64_t *)b->name_off.p;
      int fmt;
      if (host_tail) {  // FEM_HOST_TAIL=1: ordering / traceback / MD by libfemhost from the per-candidate outcome
        fem_tail_input in{b->res.n_reads, b->res.cand_begin, b->res.cand_count, b->res.cand, b->res.ed, b->res.end};
        char *text = nullptr;
        uint64_t len = 0;
        fmt = fem_tail_sam(params.e, &ref.view, &reads, &in, fmt_threads, &text, &len);
        if (!fmt) {
          free(t->buf);
          t->buf = text, t->cap = len, t->owned_elsewhere = true;
          t->parts.assign(1, fem_text_part{0, len});
        }
      } else {  // default: the records come off the device, the host only renders text
        const fem_batch_records &rec = b->rec;
        fem_record_view rv{rec.n_reads, rec.n_records, rec.rec_begin, rec.flag, rec.tid, rec.pos0, rec.nm,
                           rec.cigar_off, rec.cigar, rec.md_off, rec.md};
        t->parts.assign((size_t)fmt_threads, fem_text_part{0, 0});
        uint64_t na = 0;
        fmt = b->spliced ? fem_records_sam_refs(&ref.view, &b->refs, &rv, fmt_threads, &t->buf, &t->cap, t->parts.data(), &na)
                         : fem_records_sam_parts(&ref.view, &reads, &rv, fmt_threads, &t->buf, &t->cap, t->parts.data(), &na);
        n_asserted += na;
      }
      busy_text += real_time() - t0;
      if (fmt != 0) {
        if (!exit_code.exchange(EXIT_FAILURE)) fprintf(stderr, "[FEM] out of memory while formatting SAM records\n");
        t->parts.clear();
      }
      write_q.push(WriteItem{t, nullptr});
      fprintf(stderr, "Mapped read batch in %fs.\n", real_time() - b->t_submit);
      free_q.push(b);  // fetched and rendered: the staging buffers may be refilled (they stay acquired, include/fem_hip.h)
    }
  });

  // ---- one worker per GPU (the mapping threads of src/FEM_map.c:182-185) ----
  std::vector<std::thread> workers;
  for (int g = 0; g < n_gpus; ++g)
    workers.emplace_back([&, g] {
      fem_dev *h = devs[(size_t)g];
      if (n_gpus > 1 && !share_gpu) (void)fem_bind_thread_near_device(g);
      auto acquire = [&](BatchBuf *b, uint64_t reads_cap, uint64_t bases_cap) -> bool {
        char *pb = nullptr;
        uint64_t *po = nullptr;
        int rc = 0;
        rc = fem_dev_acquire_stage(h, b->slot, reads_cap, bases_cap, &pb, &po);
        if (rc) {
          if (!exit_code.exchange(EXIT_FAILURE)) dev_fail(h, "staging buffers", rc);
          return false;
        }
        b->bases = pb, b->off = po, b->reads_cap = reads_cap, b->bases_cap = bases_cap;
        if (device_text) {  // qualities and names go to the GPU as well: pinned staging for them
          const uint64_t names_cap = std::max<uint64_t>(b->want_names, std::max<uint64_t>(b->names_cap, names_cap0));
          rc = fem_dev_acquire_text_stage(h, b->slot, reads_cap, bases_cap, names_cap, &b->q_stage, &b->n_stage, &b->no_stage);
          if (rc) {
            if (!exit_code.exchange(EXIT_FAILURE)) dev_fail(h, "text staging buffers", rc);
            return false;
          }
          b->names_cap = names_cap;
        }
        return true;
      };
      for (int s = 0; s < n_slots; ++s) {
        BatchBuf *b = &bufs[(size_t)g * (size_t)n_slots + (size_t)s];
        b->gpu = g, b->slot = s;
        if (!acquire(b, reads_cap0, bases_cap0)) b->bases = nullptr;  // (allocated during the setup: this only hands them out)
        free_q.push(b);  // (without buffers when the acquisition failed: the reader stops on it instead of waiting for ever)
      }
      // Round 5: the thread that submits does not retire.  A batch's way home has host round trips in it (the mapping's
      // counters, the records counted, the text sized: fem_dev_fetch_sam), each of which can wait behind another batch's
      // kernels on the device; with one thread per GPU doing both, those waits came one after the other and the GPU idled
      // (16 M reads of C3 to /dev/null: 91 Mreads/s with 9.4 ms of "device wait" per 1 M-read batch, of which 5 were
      // kernels).  Now every batch in flight is retired by a thread of its own (the library takes calls on different
      // slots of a handle from different threads), and a sequencer hands the results on in submission order.
      std::mutex seq_mu;
      uint64_t seq_next = 0, seq_submit = 0;
      std::map<uint64_t, std::function<void()>> seq_held;
      auto deliver = [&](uint64_t seq, std::function<void()> fn) {
        std::lock_guard<std::mutex> l(seq_mu);
        seq_held.emplace(seq, std::move(fn));
        for (auto it = seq_held.find(seq_next); it != seq_held.end(); it = seq_held.find(seq_next)) {
          it->second();
          seq_held.erase(it);
          ++seq_next;
        }
      };
      Channel<BatchBuf *> retire_q;
      // BAM: the batch's BGZF members take the text's place (the writer waits for them with fem_dev_sam_wait as for a text)
      auto fetch_bam = [&](fem_dev *hd, BatchBuf *b) -> int {
        fem_batch_bam z{};
        const int rc = fem_dev_fetch_bam_nowait(hd, b->slot, bam_level, &z);
        if (rc) return rc;
        b->sam.text = (const char *)z.data, b->sam.len = z.len, b->sam.n_records = z.n_records, b->sam.n_asserted = z.n_asserted;
        memcpy(b->sam.stats, z.stats, sizeof z.stats);
        return FEM_OK;
      };
      auto retire = [&](BatchBuf *b) {
        double t0 = real_time();
        int rc = host_tail     ? fem_dev_map_batch_wait(h, b->slot, &b->res)
                 : bam         ? fetch_bam(h, b)
                 : device_text ? fem_dev_fetch_sam_nowait(h, b->slot, &b->sam)  // (the writer waits for the text itself)
                               : fem_dev_fetch_records(h, b->slot, &b->rec);
        if (!rc && paired) rc = fem_dev_pair_count(h, b->slot, &b->n_proper);
        if (!rc && rescue_given) rc = fem_dev_rescue_count(h, b->slot, &b->n_rescued);
        if (!rc && rescue_discordant) rc = fem_dev_rescue_discordant_count(h, b->slot, &b->n_rescued_discordant);
        if (!rc && unmapped) rc = fem_dev_unmapped_count(h, b->slot, &b->n_unmapped);
        if (!rc && report) rc = fem_dev_filtered_count(h, b->slot, &b->n_filtered);
        if (!rc && xa_given) rc = fem_dev_xa_count(h, b->slot, &b->n_xa);
        for (int k = 0; k < kCutKinds; ++k)
          if (!rc && cut_kinds[k].counted) rc = cut_kinds[k].count(h, b->slot, &b->n_cut[k][0], &b->n_cut[k][1]);
        const double waited = real_time() - t0;
        b->t_retired = t0 + waited;
        double placing = 0;
        if (!rc && host_quals) {
          // the qualities never left the host: once the text is home, into the fields the device left open — on this thread
          // (a batch's own), so that the writer only writes
          rc = fem_dev_sam_wait(h, b->slot);
          if (!rc && b->sam.len) {
            const double t1 = real_time();
            const uint64_t *qual_at = nullptr;
            uint64_t n_q = 0;
            int qrc = fem_dev_sam_quals(h, b->slot, &qual_at, &n_q);
            if (!qrc)
              qrc = fem_sam_fill_quals(const_cast<char *>(b->sam.text), b->sam.len, qual_at, n_q, b->q_stage, b->packed ? nullptr : b->off, b->shape.max_len,
                                       std::max(1, n_threads / 2));
            if (qrc) {
              if (!exit_code.exchange(EXIT_FAILURE)) fprintf(stderr, "[FEM] qualities could not be placed in the SAM text (%d)\n", qrc);
              rc = FEM_ERR_STATE;
            }
            placing = real_time() - t1;
          }
        }
        deliver(b->seq, [&, b, rc, waited, placing] {
          busy_wait[(size_t)g] += waited;
          {
            std::lock_guard<std::mutex> l(stat_mu);
            busy_text += placing;
          }
          if (rc) {
            if (!exit_code.exchange(EXIT_FAILURE)) dev_fail(h, "mapping", rc);
            work_q[(size_t)g].push(Msg{kRecycle, b});
            return;
          }
          const uint64_t *st = host_tail ? b->res.stats : device_text ? b->sam.stats : b->rec.stats;
          for (int i = 0; i < 5; ++i) per_gpu[(size_t)g * 5 + (size_t)i] += st[i];
          if (paired) per_gpu_proper[(size_t)g] += b->n_proper, per_gpu_rescued[(size_t)g] += b->n_rescued;
          if (paired) per_gpu_rescued_disc[(size_t)g] += b->n_rescued_discordant;
          per_gpu_unmapped[(size_t)g] += b->n_unmapped;
          per_gpu_filtered[(size_t)g] += b->n_filtered;
          per_gpu_xa[(size_t)g] += b->n_xa;
          for (int i = 0; i < kCutKinds * 2; ++i) per_gpu_cut[(size_t)g * kCutKinds * 2 + (size_t)i] += b->n_cut[i / 2][i % 2];
          if (device_text) {
            n_asserted += b->sam.n_asserted;
            write_q.push(WriteItem{nullptr, b});
          } else {
            text_q.push(b);
          }
        });
      };
      int n_retire = std::max(1, n_slots);  // (one per slot: a batch's thread also waits for its text and places the qualities)
      if (const char *fl = getenv("FEM_FLIGHT")) n_retire = std::max(1, std::min(n_slots, atoi(fl)));
      std::vector<std::thread> retirers;
      for (int r = 0; r < n_retire; ++r)
        retirers.emplace_back([&] {
          if (n_gpus > 1 && !share_gpu) (void)fem_bind_thread_near_device(g);
          for (;;) {
            BatchBuf *b = retire_q.pop();
            if (!b) break;
            retire(b);
          }
        });
      for (;;) {
        Msg m = work_q[(size_t)g].pop();
        if (m.kind == kStop) break;
        if (m.kind == kRecycle) {
          const double t0 = real_time();
          if (!acquire(m.b, m.b->reads_cap, m.b->bases_cap)) m.b->bases = nullptr;
          busy_recycle[(size_t)g] += real_time() - t0;
          free_q.push(m.b);
          continue;
        }
        if (m.kind == kRegrow) {
          if (!acquire(m.b, m.b->want_reads, m.b->want_bases)) m.b->bases = nullptr;
          regrown_q.push(m.b);
          continue;
        }
        BatchBuf *b = m.b;  // kFilled
        b->t_submit = real_time();
        int rc = exit_code ? FEM_ERR_STATE
                 : b->packed ? fem_dev_commit_stage_packed(h, b->slot, b->shape.n_reads, b->shape.max_len, b->n_exc)
                 : b->shape.min_len == b->shape.max_len  // reads of one length: the offsets need not cross the link
                     ? fem_dev_commit_stage_uniform(h, b->slot, b->shape.n_reads, b->shape.max_len)
                     : fem_dev_commit_stage(h, b->slot, b->shape.n_reads, b->shape.max_len);
        const double t_c1 = real_time();
        // (--trim-qual reads the qualities in front of the mapping: on this path alone the text stage is committed first)
        if (!rc && trim_given) rc = fem_dev_commit_text_stage(h, b->slot, b->shape.n_reads, b->shape.n_name_bytes);
        if (!rc) rc = fem_dev_map_staged(h, b->slot, &params);
        const double t_c2 = real_time();
        // (qualities and names behind the mapping's launches: the call that hands the link 140 MB can wait for room in the copy
        //  engine's queue, 8-10 ms now and then, and the kernels need none of it)
        if (!rc && device_text && !trim_given)
          rc = host_quals ? fem_dev_commit_names_stage(h, b->slot, b->shape.n_reads, b->shape.n_name_bytes)
                          : fem_dev_commit_text_stage(h, b->slot, b->shape.n_reads, b->shape.n_name_bytes);
        if (batch_times && real_time() - b->t_submit > 1e-3)
          fprintf(stderr, "[FEM] slow submit (ms): reads committed %.2f, mapping queued %.2f, text committed %.2f\n", 1e3 * (t_c1 - b->t_submit),
                  1e3 * (t_c2 - t_c1), 1e3 * (real_time() - t_c2));
        if (rc) {
          if (!exit_code.exchange(EXIT_FAILURE)) dev_fail(h, "batch submit", rc);
          work_q[(size_t)g].push(Msg{kRecycle, b});
          continue;
        }
        b->t_submitted = real_time();
        busy_submit[(size_t)g] += b->t_submitted - b->t_submit;
        b->seq = seq_submit++;
        retire_q.push(b);
      }
      for (int r = 0; r < n_retire; ++r) retire_q.push(nullptr);
      for (auto &t : retirers) t.join();
    });

  // ---- reader (src/input_queue.c:53-79): this thread ----
  fem_seqfile *read_file = nullptr, *read2_file = nullptr;
  {
    fem_seqfile *f = read_file = fem_seqfile_open(read_path);
    fem_seqfile *f2 = read2_file = paired ? fem_seqfile_open(read2_path) : nullptr;
    if (!f || (paired && !f2)) {
      fprintf(stderr, "Cannot find sequence file!");  // the reference exits here (src/sequence_batch.c:33-35)
      exit_code = EXIT_FAILURE;
      f = nullptr;
    }
    // The planner: cuts the next batch out of the input (one pass over it: where the records end, how many, how long) on a
    // thread of its own, ahead of the batch being filled where the file allows it (plain FASTQ through a mapping: a plan's records
    // stay where they are) — a batch's plan needs no staging slot, so it is also made while the reader waits for one.  On boxes
    // whose cores are slow the reader's plan-then-fill in a row bounded the run (32 M reads of C3: 118-121 Mreads/s against
    // 130-140 elsewhere, the reader busy 0.19-0.24 of the run's 0.25-0.27 s).
    struct Planned {
      fem_batch_plan *plan = nullptr;
      fem_batch_shape shape{};
      int rc = 0;
      fem_batch_plan *plan2 = nullptr;  // paired: as many records of --read2 (one, to see that it ends, behind the end of --read1)
      fem_batch_shape shape2{};
      int rc2 = 0;
    };
    Channel<Planned> planned_q;
    Channel<int> plan_tokens;  // a plan is made per token: one while nothing may run ahead, two where it may
    std::atomic<bool> plan_stop{false};
    const bool ahead = f && fem_seqfile_plan_ahead_ok(f) && (!paired || fem_seqfile_plan_ahead_ok(f2)) &&
                       !(getenv("FEM_PLAN_AHEAD") && getenv("FEM_PLAN_AHEAD")[0] == '0');
    plan_tokens.push(1);
    if (ahead) plan_tokens.push(1);
    std::thread planner([&] {
      while (f) {
        (void)plan_tokens.pop();
        if (plan_stop) break;
        Planned pl;
        const double t_p = real_time();
        pl.rc = fem_seqfile_plan(f, paired ? batch_bytes / 2 : batch_bytes, rd_threads, &pl.plan, &pl.shape);
        if (paired && pl.plan && pl.rc == 0)  // the mates: cut by count where the first file was cut by bytes
          pl.rc2 = fem_seqfile_plan_count(f2, std::max<uint64_t>(pl.shape.n_reads, 1), rd_threads, &pl.plan2, &pl.shape2);
        busy_plan += real_time() - t_p;
        const bool last = !pl.plan || pl.rc != 0 || pl.shape.n_reads == 0;
        planned_q.push(pl);
        if (last) break;
      }
    });
    // A batch of read pairs in the slot's staging: mate 1's records, then mate 2's behind them (offsets and name offsets running
    // on), a trailing /1 or /2 taken off every name, the two names of each pair compared.  0 = filled, 2 = the names differ
    // (reported here), anything else = the reader failed.  Frees both plans.
    auto fill_pair = [&](fem_seqfile *fa, fem_batch_plan *pa, fem_seqfile *fb, fem_batch_plan *pb, const fem_batch_shape &sa,
                         BatchBuf *b) -> int {
      int frc = fem_seqfile_fill(fa, pa, rd_threads, b->bases, b->off, b->q_stage, b->n_stage, b->no_stage);
      const uint64_t n1 = sa.n_reads, nb1 = sa.n_bases, nn1 = sa.n_name_bytes;
      if (frc) {
        fem_batch_plan_free(pb);
        return frc;
      }
      frc = fem_seqfile_fill(fb, pb, rd_threads, b->bases + nb1, b->off + n1, b->q_stage + nb1, b->n_stage + nn1, b->no_stage + n1);
      if (frc) return frc;
      const uint64_t n = b->shape.n_reads;
      uint64_t *off = b->off, *no = b->no_stage;
      char *nm = b->n_stage;
      for (uint64_t r = n1; r <= n; ++r) off[r] += nb1, no[r] += nn1;
      uint64_t w = 0, from = no[0];
      for (uint64_t r = 0; r < n; ++r) {
        const uint64_t to = no[r + 1];
        uint64_t len = to - from;
        if (len >= 2 && nm[from + len - 2] == '/' && (nm[from + len - 1] == '1' || nm[from + len - 1] == '2')) len -= 2;
        if (w != from) memmove(nm + w, nm + from, len);
        no[r] = w, w += len, from = to;
      }
      no[n] = w;
      b->shape.n_name_bytes = w;
      for (uint64_t i = 0; i < n1; ++i) {
        const uint64_t l1 = no[i + 1] - no[i], l2 = no[n1 + i + 1] - no[n1 + i];
        if (l1 != l2 || memcmp(nm + no[i], nm + no[n1 + i], l1) != 0) {
          fprintf(stderr, "Read names differ in the two read files: %.*s %.*s\n", (int)l1, nm + no[i], (int)l2, nm + no[n1 + i]);
          return 2;
        }
      }
      return 0;
    };
    bool planner_done = false;  // the planner has handed over its last plan (end of input or failure)
    while (f && !exit_code) {
      const double t_pop = real_time();
      BatchBuf *b = free_q.pop();
      if (!b->bases) break;  // its GPU could not provide staging buffers (reported by the worker)
      double t0 = real_time();
      wait_slot += t0 - t_pop;
      b->t_slot = t0;
      if (t_first_slot == 0) t_first_slot = t0;
      Planned pd = planned_q.pop();
      t0 = real_time();  // (the reader is busy from here: the plan was made beside the previous batch)
      fem_batch_plan *plan = pd.plan;
      b->shape = pd.shape;
      int rc = pd.rc;
      if (!plan || rc != 0 || pd.shape.n_reads == 0) planner_done = true;
      bool ok = plan != nullptr;
      if (paired && ok && rc == 0) {
        if (!pd.plan2 || pd.rc2 != 0) {
          rc = pd.rc2 ? pd.rc2 : -1;
        } else if (pd.shape2.n_reads != pd.shape.n_reads) {
          fprintf(stderr, "The two read files hold different numbers of reads.\n");
          exit_code = EXIT_FAILURE;
          ok = false;
        } else if (pd.shape.n_reads > 0) {  // one batch of both mates: mate 1's reads, then mate 2's
          const fem_batch_shape &s2 = pd.shape2;
          b->shape.n_reads += s2.n_reads, b->shape.n_bases += s2.n_bases, b->shape.n_name_bytes += s2.n_name_bytes;
          b->shape.max_len = std::max(b->shape.max_len, s2.max_len), b->shape.min_len = std::min(b->shape.min_len, s2.min_len);
          b->shape.has_qual = b->shape.has_qual && s2.has_qual;
        }
      }
      if (rc != 0) {  // the reference exits on a truncated file (src/sequence_batch.c:63-66): nothing of this batch is mapped
        fprintf(stderr, "Didn't reach the end of sequence file, which might be corrupted!");
        exit_code = EXIT_FAILURE;
        ok = false;
      }
      if (ok && b->shape.n_reads > 0 && !b->shape.has_qual) {
        fprintf(stderr, "Reads without qualities (FASTA) are not supported: the SAM records need QUAL.\n");
        exit_code = EXIT_FAILURE;
        ok = false;
      }
      if (ok && b->shape.n_reads > 0 &&
          (b->shape.n_reads > b->reads_cap || b->shape.n_bases + 64 > b->bases_cap || (device_text && b->shape.n_name_bytes + 64 > b->names_cap))) {
        b->want_reads = std::max(b->reads_cap, b->shape.n_reads + b->shape.n_reads / 8);
        b->want_bases = std::max(b->bases_cap, b->shape.n_bases + b->shape.n_bases / 8 + 4096);
        b->want_names = b->shape.n_name_bytes + b->shape.n_name_bytes / 8 + 4096;
        work_q[(size_t)b->gpu].push(Msg{kRegrow, b});
        BatchBuf *back = regrown_q.pop();  // (one request at a time: it is ours)
        ok = back->bases != nullptr;
      }
      if (ok && b->shape.n_reads > 0 && !device_text) {
        ok = b->quals.reserve(b->shape.n_bases + 1) && b->names.reserve(b->shape.n_name_bytes + 1) &&
             b->name_off.reserve((b->shape.n_reads + 1) * sizeof(uint64_t));
        if (!ok) {
          fprintf(stderr, "[FEM] out of memory while reading\n");
          exit_code = EXIT_FAILURE;
        }
      }
      if (!ok || b->shape.n_reads == 0) {
        fem_batch_plan_free(plan);
        fem_batch_plan_free(pd.plan2);
        busy_read += real_time() - t0;
        break;  // end of input (or failure)
      }
      b->packed = false, b->spliced = false, b->n_exc = 0;
      rc = 1;
      if (pack_bases && b->shape.min_len == b->shape.max_len && b->shape.n_bases < 0xFFFFFFF0ull) {
        // reads of one length: two bits per base straight into the staging; 1 = too many characters outside "ACGT" for that form
        uint64_t exc_cap = 0;
        const bool lay = fem_dev_packed_layout(b->shape.n_reads, b->shape.max_len, nullptr, nullptr, &exc_cap) == FEM_OK;
        if (lay && splice) {
          // ... and nothing else copied: where each read's name, bases and qualities lie in the file's mapping (2 = the records
          // do not sit in a mapping that stays: gzip / BGZF windows, the sequential reader)
          const uint64_t n = b->shape.n_reads;
          if (b->r_name.reserve(n * sizeof(char *)) && b->r_seq.reserve(n * sizeof(char *)) && b->r_qual.reserve(n * sizeof(char *)) &&
              b->r_name_len.reserve(n * sizeof(uint32_t))) {
            b->refs.name = (const char **)b->r_name.p, b->refs.seq = (const char **)b->r_seq.p, b->refs.qual = (const char **)b->r_qual.p;
            b->refs.name_len = (uint32_t *)b->r_name_len.p;
            rc = fem_seqfile_fill_packed_refs(f, plan, rd_threads, b->shape.max_len, (uint8_t *)b->bases, exc_cap, &b->n_exc, &b->refs);
            b->packed = b->spliced = rc == 0;
            if (rc == 2) rc = 1;
          }
        } else if (lay && device_text) {
          rc = fem_seqfile_fill_packed(f, plan, rd_threads, b->shape.max_len, (uint8_t *)b->bases, exc_cap, &b->n_exc, b->q_stage, b->n_stage,
                                       b->no_stage);
          b->packed = rc == 0;
        }
      }
      if (rc == 1 && paired) {
        rc = fill_pair(f, plan, f2, pd.plan2, pd.shape, b);
        pd.plan2 = nullptr;
        if (rc == 2) {
          exit_code = EXIT_FAILURE;
          break;
        }
      } else if (rc == 1) {
        rc = device_text ? fem_seqfile_fill(f, plan, rd_threads, b->bases, b->off, b->q_stage, b->n_stage, b->no_stage)
                         : fem_seqfile_fill(f, plan, rd_threads, b->bases, b->off, b->quals.p, b->names.p, (uint64_t *)b->name_off.p);
      }
      busy_read += real_time() - t0;
      plan_tokens.push(1);  // (this batch's plan is consumed: the planner may cut the next but one)
      if (rc) {
        fprintf(stderr, "[FEM] reading failed\n");
        exit_code = EXIT_FAILURE;
        break;
      }
      b->t_filled = real_time();
      if (t_first_filled == 0) t_first_filled = b->t_filled;
      work_q[(size_t)b->gpu].push(Msg{kFilled, b});
    }
    // the planner: told to stop if it is still waiting for a token, its unread plans freed
    plan_stop = true;
    plan_tokens.push(1), plan_tokens.push(1);
    planner.join();
    {
      Planned pd;
      while (!planner_done && planned_q.try_pop_for(pd, 0.0)) fem_batch_plan_free(pd.plan), fem_batch_plan_free(pd.plan2);
    }
    // (the file stays open until the mapping phase is over: unmapping 4 GB of faulted-in pages takes 0.08 s, which the GPUs
    // would otherwise spend waiting for their stop message)
    t_reader_done = real_time();
  }
  for (int g = 0; g < n_gpus; ++g) work_q[(size_t)g].push(Msg{kStop, nullptr});
  for (auto &w : workers) w.join();
  t_workers_done = real_time();
  text_q.push(nullptr);
  formatter.join();
  write_q.push(WriteItem{});
  writer.join();
  if (stage_times) {
    double bw = 0;
    for (double x : busy_wait) bw += x;
    double bs = 0, br = 0;
    for (double x : busy_submit) bs += x;
    for (double x : busy_recycle) br += x;
    fprintf(stderr, "[FEM] stage busy seconds: reader %.3f (+ planner %.3f), device wait %.3f, SAM text %.3f, writer %.3f\n", busy_read, busy_plan, bw,
            busy_text, busy_write);
    fprintf(stderr, "[FEM] waiting seconds: reader for a free slot %.3f, formatter for records %.3f and for a text buffer %.3f; "
                    "GPU threads: submit %.3f, slot recycling %.3f\n", wait_slot, wait_records, wait_text_buf, bs, br);
    double cpu_u1 = 0, cpu_s1 = 0;
    cpu_seconds(&cpu_u1, &cpu_s1);
    fprintf(stderr, "[FEM] host CPU in the mapping phase: %.3f s user + %.3f s system = %.1f cores on average\n", cpu_u1 - cpu_u0, cpu_s1 - cpu_s0,
            (cpu_u1 - cpu_u0 + cpu_s1 - cpu_s0) / std::max(1e-9, real_time() - t_start));
    fprintf(stderr, "[FEM] timeline (s after the mapping phase began): first staging slot %.3f, first batch parsed %.3f, input read %.3f, "
                    "devices done %.3f, output written %.3f\n", t_first_slot - t_start, t_first_filled - t_start, t_reader_done - t_start,
            t_workers_done - t_start, real_time() - t_start);
  }
  if (bam) {  // the BGZF end-of-file marker (SAM/BAM specification 4.1.2)
    static const unsigned char eof[28] = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0, 27, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (!write_all((const char *)eof, sizeof eof) && !exit_code.exchange(EXIT_FAILURE)) fprintf(stderr, "[FEM] write error on %s\n", out_path);
  }
  if (close(out_fd) != 0 && !exit_code.exchange(EXIT_FAILURE)) fprintf(stderr, "[FEM] write error on %s\n", out_path);
  if (n_asserted)
    fprintf(stderr, "[FEM] %lu records on which the reference would have tripped an assertion (src/align.c:366-368) were "
                    "written with CIGAR *\n", (unsigned long)n_asserted.load());

  // MappingStats reduction (src/FEM_map.c:200-212): across GPUs it is one RCCL all-reduce of 5 counters
  if (n_gpus > 1 && !exit_code && !share_gpu) {
    int rc = fem_dev_allreduce_stats(devs.data(), n_gpus, per_gpu.data());
    if (rc) exit_code = dev_fail(devs[0], "stats all-reduce", rc);
  } else if (n_gpus > 1) {
    for (int g = 1; g < n_gpus; ++g)
      for (int i = 0; i < 5; ++i) per_gpu[(size_t)i] += per_gpu[(size_t)g * 5 + (size_t)i];
  }
  uint64_t totals[5];
  for (int i = 0; i < 5; ++i) totals[i] = per_gpu[(size_t)i];
  // --coverage: the devices' tracks home, summed, and the file (inside the timed phase: it is part of what the switch costs)
  uint64_t n_covered = 0;
  if (coverage_path && !exit_code) {
    std::vector<uint64_t> bins((size_t)coverage_bins, 0), part(n_gpus > 1 ? (size_t)coverage_bins : 0);
    for (int g = 0; g < n_gpus && !exit_code; ++g) {
      uint64_t *to = g ? part.data() : bins.data();
      if (int rc = fem_dev_fetch_coverage(devs[(size_t)g], to, coverage_bins)) exit_code = dev_fail(devs[(size_t)g], "coverage track", rc);
      if (g && !exit_code)
        for (size_t k = 0; k < bins.size(); ++k) bins[k] += part[k];
    }
    if (!exit_code) {
      FILE *cf = fopen(coverage_path, "w");
      const int wrc = cf ? fem_coverage_write(cf, ref.view.n_seq, ref.view.names, ref.view.name_off, ref.view.len, (int32_t)coverage_window, bins.data(), &n_covered) : -3;
      if ((!cf || wrc || fclose(cf) != 0) && !exit_code.exchange(EXIT_FAILURE)) fprintf(stderr, "[FEM] write error on %s\n", coverage_path);
    }
  }
  const double t_mapping = real_time() - t_start;  // (the reference's timer stops after the counter reduction, src/FEM_map.c:219)
  for (TextOut &t : texts) free(t.buf);
  if (read_file) fem_seqfile_close(read_file);
  if (read2_file) fem_seqfile_close(read2_file);
  for (fem_dev *h : devs) fem_dev_close(h);
  if (exit_code) return exit_code;
  fprintf(stderr, "The number of read: %lu\n", (unsigned long)totals[0]);
  fprintf(stderr, "The number of mapped read: %lu\n", (unsigned long)totals[1]);
  fprintf(stderr, "The number of candidate before additional q-gram filter: %lu\n", (unsigned long)totals[2]);
  fprintf(stderr, "The number of candidate: %lu\n", (unsigned long)totals[3]);
  fprintf(stderr, "The number of mapping: %lu\n", (unsigned long)totals[4]);
  if (paired) {  // (not part of the all-reduce of the five: summed here, per GPU)
    uint64_t n_proper = 0;
    for (uint64_t x : per_gpu_proper) n_proper += x;
    fprintf(stderr, "The number of proper pairs: %lu\n", (unsigned long)n_proper);
    if (rescue_given) {
      uint64_t n_rescued = 0;
      for (uint64_t x : per_gpu_rescued) n_rescued += x;
      fprintf(stderr, "The number of rescued mates: %lu\n", (unsigned long)n_rescued);
      if (rescue_discordant) {
        uint64_t n_disc = 0;
        for (uint64_t x : per_gpu_rescued_disc) n_disc += x;
        fprintf(stderr, "The number of rescued discordant pairs: %lu\n", (unsigned long)n_disc);
      }
    }
  }
  if (unmapped) {
    uint64_t n_unmapped = 0;
    for (uint64_t x : per_gpu_unmapped) n_unmapped += x;
    fprintf(stderr, "The number of unmapped reads: %lu\n", (unsigned long)n_unmapped);
  }
  if (report) {
    uint64_t n_filtered = 0;
    for (uint64_t x : per_gpu_filtered) n_filtered += x;
    fprintf(stderr, "The number of filtered lines: %lu\n", (unsigned long)n_filtered);
  }
  if (xa_given) {
    uint64_t n_xa = 0;
    for (uint64_t x : per_gpu_xa) n_xa += x;
    fprintf(stderr, "The number of XA entries: %lu\n", (unsigned long)n_xa);
  }
  for (int k = 0; k < kCutKinds; ++k) {
    for (int j = 0; j < 2 && cut_kinds[k].counted; ++j) {
      uint64_t sum = 0;
      for (int g = 0; g < n_gpus; ++g) sum += per_gpu_cut[((size_t)g * kCutKinds + (size_t)k) * 2 + (size_t)j];
      fprintf(stderr, "%s: %lu\n", cut_kinds[k].line[j], (unsigned long)sum);
    }
  }
  if (coverage_path) fprintf(stderr, "The number of covered bases: %lu\n", (unsigned long)n_covered);
  fprintf(stderr, "Time: %fs\n", t_mapping);
  return 0;
}

}  // namespace

int main(int argc, char *argv[]) {
  if (argc < 2) {
    fprintf(stderr, "%s\n", "Too few arguements.");
    usage_main();
    exit(EXIT_FAILURE);
  }
  int rv = 0;
  double t0 = real_time(), c0 = cpu_time();
  if (strcmp(argv[1], "index") == 0) {
    rv = index_main(argc - 1, argv + 1);
  } else if (strcmp(argv[1], "map") == 0) {
    char *pg = nullptr;
    if (fem_pg_line(argc, argv, FEM_VERSION, &pg) == 0) g_pg_line = pg;
    free(pg);
    rv = map_main(argc - 1, argv + 1);
  } else {
    fprintf(stderr, "[%s] unrecognized command '%s'\n", __func__, argv[1]);
    exit(EXIT_FAILURE);
  }
  if (rv == 0) {
    fprintf(stderr, "[%s] Version: %s\n", __func__, FEM_VERSION);
    fprintf(stderr, "[%s] CMD:", __func__);
    for (int i = 0; i < argc; ++i) fprintf(stderr, " %s", argv[i]);
    fprintf(stderr, "\n[%s] Real time: %.3f sec; CPU: %.3f sec\n", __func__, real_time() - t0, cpu_time() - c0);
  }
  return rv;
}
