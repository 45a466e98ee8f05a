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
void cpu_seconds(double *user, double *sys) {
  struct rusage ru;
  getrusage(RUSAGE_SELF, &ru);
  *user = ru.ru_utime.tv_sec + 1e-6 * ru.ru_utime.tv_usec, *sys = ru.ru_stime.tv_sec + 1e-6 * ru.ru_stime.tv_usec;
}
double cpu_time() {
  double user = 0, sys = 0;
  cpu_seconds(&user, &sys);
  return user + sys;
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

// ---- the options: everything the command line and the environment decide, made once (parse_map_options) and read-only after ----
constexpr int kOrientAuto = 3;  // --orientation auto: learned in --infer-insert's pre-pass (fem_dev_estimate_library)
const char *const kHostEnv[3] = {"FEM_HOST_TAIL", "FEM_HOST_FORMAT", "FEM_HOST_QUALS"};  // the host-side paths (host_refusals)

struct MapOptions {
  char *ref_path = nullptr, *index_path = nullptr, *read_path = nullptr, *read2_path = nullptr, *out_path = nullptr;
  fem_params params{12, 3, 2, 1};  // src/FEM_map.c:67-70: k and step are fixed, whatever the index header says
  int n_threads = 1, n_gpus = 1;
  // reads per batch: 250 k fills the pipeline soonest on small inputs; a batch costs three host round trips on its way through
  // the tail, which 1 M-read batches amortise on large ones (16 M reads of C2 to /dev/null: 105 -> 116 Mreads/s, 8 M of C3:
  // 71 -> 81; round 4) — chosen by the size of the read file unless --batch says otherwise (size_batches)
  uint64_t batch_reads = 250000;
  bool batch_given = false;
  long long min_insert = 0, max_insert = 500;
  long long rescue_edits = 0;  // --rescue (mate rescue at this many edits, fem_dev_set_rescue)
  bool rescue_given = false;
  bool rescue_discordant = false;  // --rescue-discordant (fem_dev_set_rescue_discordant)
  // --infer-insert[=N]: the insert size range from the input's first N pairs (fem_dev_estimate_insert), -I / -X the fallback
  bool infer_insert = false;
  long long infer_pairs = 65536;
  // --orientation: FEM_ORIENT_FR / _RF / _FF (fem_dev_set_orientation); kOrientAuto; -1: another word, refused by the checks
  int orientation = FEM_ORIENT_FR;
  bool orientation_given = false;
  int bam_level = -1;  // --bam[=LEVEL]: BAM records and BGZF members made on the device (fem_dev_fetch_bam); -1: SAM; -2: refused
  bool unmapped = false;  // --unmapped: a line for every read without a mapping, made on the device (fem_dev_set_unmapped)
  long long strata = -1, max_hits = -1;  // --strata / --max-hits: the line filter, made on the device (fem_dev_set_report); -1: off
  bool strata_given = false, max_hits_given = false;
  bool mapq = false;   // --mapq: MAPQ from the hit strata, made on the device (fem_dev_set_mapq); else 255 as the reference
  bool header = false;  // --header: @HD in front of the @SQ lines, @PG behind them
  const char *rg_arg = nullptr;  // --rg: the @RG line (implies --header) and RG:Z on every line, made on the device (fem_dev_set_tags)
  char *rg_line = nullptr, rg_id[256] = "";  // ... as fem_parse_read_group made them of it
  const char *pg_line = nullptr;  // g_pg_line (no @PG line rather than an empty one)
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

  // derived from the above
  bool bam = false, paired = false, report = false, tags = false, adapter_given = false, coverage = false;
  // what --trim5 / --trim3 / --trim-qual steer, --adapter and --trim-overlap steer too: a batch with any is a trimmed batch on the device
  bool clip_given = false;

  // the environment, and what it decides together with the above
  bool host_env[3] = {};  // kHostEnv[i] is 1
  bool host_tail = false;  // FEM_HOST_TAIL=1: ordering, traceback and text by the host threads from the per-candidate outcome
  // Where the SAM text is made.  Default: on the device (fem_dev_fetch_sam: qualities and names go there with the bases, the
  // finished text comes back: ~365 bytes per read over the link).  FEM_HOST_FORMAT=1: the device maps, orders, traces back and
  // hands over RECORDS (FLAG, RNAME id, POS, CIGAR, NM, MD: ~30 bytes per read) and the host threads splice them between
  // QNAME, SEQ and QUAL, which never leave the host — for a plain FASTQ file they are not even copied: the formatter reads them
  // out of the input's mapping (fem_seqfile_fill_packed_refs; FEM_SPLICE=0: copied by the parser).  ~55 bytes per read cross
  // the link; the price is ~0.07 core-microseconds of formatting per read, which on a 16-core share of the host is more than
  // the link costs (measured, 16 M reads of C2 to /dev/null: 75-93 Mreads/s against 100-117), so it is the
  // option, not the default.
  bool device_text = true, splice = false;
  // ... with the qualities kept on the host (fem_dev_commit_names_stage: the device leaves their field open and the batch's
  // retiring thread fills it in): they are 228 of the 473 bytes per read on the link otherwise — and 0.027 core-µs per read on
  // the host then, next to the parser's 0.078.  With 16 cores per GPU the two forms are within +7 / -16 % of each other from box
  // to box (the run is bound by the link in one and by the cores in the other); from 24 threads on the qualities stay on the
  // host.  FEM_HOST_QUALS=1 / FEM_DEVICE_QUALS=1 decide it by hand.
  bool host_quals = false;
  // With the text on the device the link is what bounds the run: batches of equal-length reads then cross it at two bits per
  // base — the parser writes that form straight into the pinned staging (fem_seqfile_fill_packed ->
  // fem_dev_commit_stage_packed: no host work per base beyond the parse itself) (FEM_PACK_BASES=0: always as characters).
  bool pack_bases = false;
  // FEM_TEST_SHARE_GPU=1 (test hook for one-GPU boxes, honoured under FEM_TESTING=1 only): all `--gpus N` workers open GPU 0,
  // each with its own handle, and the counters are summed on the host (RCCL refuses two ranks on one device)
  bool share_gpu = false;
  bool stage_times = false;  // FEM_STAGE_TIMES=1: busy seconds of each pipeline stage on stderr at the end
  bool batch_times = false;  // ... =2: and every batch's way through them, and the form its bases took
  bool split_threads = false;  // -t threads are shared by the two host stages that run side by side (FEM_SPLIT_THREADS=0: each gets all of them)
  int reader_share = 50;       // per cent of the threads that parse (FEM_READER_SHARE)
  int flight = 1 << 30;        // FEM_FLIGHT: retiring threads per GPU, at most one per slot (which is the default)
  bool plan_ahead = true;  // FEM_PLAN_AHEAD=0: the planner never cuts a batch ahead of the one being filled
};

struct EnvVar {  // an environment variable, read once: whether it is set, its first character, its value as a number
  bool set;
  char c;
  int n;
};
EnvVar env_var(const char *name) {
  const char *x = getenv(name);
  return EnvVar{x != nullptr, x ? x[0] : '\0', x ? atoi(x) : 0};
}

// an option's argument as a number; -1 where it is none, which every range check of check_map_options refuses
long long number(const char *s) {
  char *end = nullptr;
  const long long v = strtoll(s, &end, 10);
  return !end || end == s || *end ? -1 : v;
}

void parse_map_options(int argc, char **argv, MapOptions *o) {
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
      case 'H': o->header = true; break;
      case 'T': o->rg_arg = optarg, o->header = true; break;
      case 'n': o->hit_tags = true; break;
      case 'M': o->mate_tags = true; break;
      case 'q': o->sam_seq = true; break;
      case 'x': o->xa_given = true, o->xa_entries = optarg ? number(optarg) : 0x7FFFFFFFll; break;  // (alone: the byte budget bounds the folding)
      case '5': o->trim_given = true, o->trim5 = number(optarg); break;
      case '3': o->trim_given = true, o->trim3 = number(optarg); break;
      case 'm':
        o->trim_given = true, o->trim_qual = number(optarg);
        if (o->trim_qual == 0) o->trim_qual = -1;  // (--trim-qual 0 is no quality: refused)
        break;
      case 1001: o->adapter1 = optarg; break;
      case 1002: o->adapter2 = optarg; break;
      case 1003: o->adapter_overlap_given = true, o->adapter_overlap = number(optarg); break;
      case 1004: o->adapter_err_given = true, o->adapter_err = number(optarg); break;
      case 1005: o->trim_overlap = true; break;
      case 1006: o->trim_overlap_min_given = true, o->trim_overlap_min = number(optarg); break;
      case 1007: o->trim_overlap_err_given = true, o->trim_overlap_err = number(optarg); break;
      case 1008: o->coverage_path = optarg; break;
      case 1009: o->coverage_window_given = true, o->coverage_window = number(optarg); break;
      case 1010: o->coverage_all = true; break;
      case 1011: o->coverage_mapq_given = true, o->coverage_mapq = number(optarg); break;
      case 'r': o->ref_path = optarg; break;
      case 'i': o->index_path = optarg; break;
      case 'b': o->read_path = optarg; break;
      case 'c': o->read2_path = optarg; break;
      case 'I': o->min_insert = strtoll(optarg, nullptr, 10); break;
      case 'X': o->max_insert = strtoll(optarg, nullptr, 10); break;
      case 'R': o->rescue_given = true, o->rescue_edits = number(optarg); break;
      case 'Z':
        o->bam_level = !optarg ? 1 : strcmp(optarg, "0") == 0 ? 0 : strcmp(optarg, "1") == 0 ? 1 : -2;  // (-2: refused by the checks)
        break;
      case 'D': o->rescue_discordant = true; break;
      case 'F':
        o->infer_insert = true;
        if (optarg) o->infer_pairs = number(optarg);
        break;
      case 'O':
        o->orientation = strcmp(optarg, "fr") == 0 ? FEM_ORIENT_FR : strcmp(optarg, "rf") == 0 ? FEM_ORIENT_RF : strcmp(optarg, "ff") == 0 ? FEM_ORIENT_FF
                         : strcmp(optarg, "auto") == 0 ? kOrientAuto : -1;
        o->orientation_given = true;
        break;
      case 'Q': o->mapq = true; break;
      case 'U': o->unmapped = true; break;
      case 'S': o->strata_given = true, o->strata = number(optarg); break;
      case 'N': o->max_hits_given = true, o->max_hits = number(optarg); break;
      case 'e': o->params.e = atoi(optarg); break;
      case 't': o->n_threads = atoi(optarg); break;
      case 'a': o->params.a = atoi(optarg); break;
      case 'G': o->n_gpus = atoi(optarg); break;
      case 'B': o->batch_reads = strtoull(optarg, nullptr, 10), o->batch_given = true; break;
      case 'f':
        if (strcmp(optarg, "v") != 0 && strcmp(optarg, "g") != 0) {  // parsed and ignored (src/FEM_map.c:108-118)
          fprintf(stderr, "%s\n", "Wrong name of seeding algorithm!");
          usage_map();
          exit(EXIT_FAILURE);
        }
        break;
      case 'o': o->out_path = optarg; break;
      default:
        usage_map();
        exit(EXIT_SUCCESS);
    }
  }
  if (o->rg_arg) {
    char why[512] = "";
    if (fem_parse_read_group(o->rg_arg, &o->rg_line, o->rg_id, why, sizeof why) != 0) {
      fprintf(stderr, "Wrong --rg line: %s.\n", why[0] ? why : "out of memory");
      exit(EXIT_FAILURE);
    }
  }
  o->pg_line = g_pg_line.empty() ? nullptr : g_pg_line.c_str();
  o->bam = o->bam_level >= 0, o->paired = o->read2_path != nullptr, o->report = o->strata_given || o->max_hits_given;
  o->tags = o->rg_arg || o->hit_tags, o->adapter_given = o->adapter1 != nullptr, o->coverage = o->coverage_path != nullptr;
  o->clip_given = o->trim_given || o->adapter_given || o->trim_overlap;
  for (int v = 0; v < 3; ++v) o->host_env[v] = env_var(kHostEnv[v]).c == '1';
  o->host_tail = o->host_env[0];
  o->device_text = !o->host_tail && !o->host_env[1];
  o->host_quals = o->device_text && !o->bam && !o->mate_tags && !o->sam_seq && !o->clip_given && env_var("FEM_DEVICE_QUALS").c != '1' &&
                  (o->host_env[2] || o->n_threads >= 24);
  o->splice = !o->host_tail && !o->device_text && env_var("FEM_SPLICE").c != '0';
  o->pack_bases = !o->host_tail && !o->paired && !o->clip_given && env_var("FEM_PACK_BASES").c != '0';  // (a trimmed batch goes as characters: the trim stage reads them)
  o->share_gpu = env_var("FEM_TEST_SHARE_GPU").c == '1' && env_var("FEM_TESTING").c == '1';
  const char st = env_var("FEM_STAGE_TIMES").c;
  o->stage_times = st == '1' || st == '2', o->batch_times = st == '2';
  o->split_threads = env_var("FEM_SPLIT_THREADS").c != '0' && o->n_threads >= 4;
  if (const EnvVar rs = env_var("FEM_READER_SHARE"); rs.set) o->reader_share = std::min(90, std::max(10, rs.n));
  if (const EnvVar fl = env_var("FEM_FLIGHT"); fl.set) o->flight = fl.n;
  o->plan_ahead = env_var("FEM_PLAN_AHEAD").c != '0';
}

// check_args (src/FEM_map.c:29-55): the first thing wrong with the options, or null
const char *check_map_options(const MapOptions &o) {
  const bool paired = o.paired;
  if (o.params.e < 0 || o.params.e > 7) return "Wrong error threshold.";
  if (o.n_threads <= 0) return "Wrong number of threads.";
  if (o.params.a < 0 || o.params.a > 2) return "Wrong number of additional q-grams.";
  if (o.min_insert < 0 || o.max_insert < o.min_insert || o.max_insert > (1ll << 30)) return "Wrong insert size range.";
  if (o.infer_insert && !paired) return "--infer-insert needs read pairs (--read2).";
  if (o.infer_insert && (o.infer_pairs < 64 || o.infer_pairs > 262144)) return "Wrong number of pairs to infer from (64-262144).";
  if (o.orientation < 0) return "Wrong library orientation (fr, rf, ff or auto).";
  if (o.orientation_given && !paired) return "--orientation needs read pairs (--read2).";
  if (o.orientation == kOrientAuto && !o.infer_insert) return "--orientation auto needs --infer-insert.";
  if (o.mate_tags && !paired) return "--mate-tags needs --read2.";
  if (o.rescue_discordant && !o.rescue_given) return "--rescue-discordant needs --rescue.";
  if (o.rescue_given && !paired) return "--rescue needs read pairs (--read2).";
  if (o.rescue_given && (o.rescue_edits < 0 || o.rescue_edits > 15)) return "Wrong rescue error threshold (0-15).";
  if (o.rescue_given && o.max_insert - o.min_insert > 65536) return "--rescue searches insert size ranges of at most 65536.";
  if (o.bam_level == -2) return "Wrong BAM compression level (0-1).";
  if (o.strata_given && (o.strata < 0 || o.strata > 15)) return "Wrong number of strata (0-15).";
  if (o.max_hits_given && (o.max_hits < 1 || o.max_hits > 0x7FFFFFFFll)) return "Wrong hit limit (>= 1).";
  if (o.xa_given && o.xa_entries != 0x7FFFFFFFll && (o.xa_entries < 1 || o.xa_entries > 1000000)) return "Wrong number of --xa entries (1-1000000).";
  if (o.trim5 < 0 || o.trim5 > 1024 || o.trim3 < 0 || o.trim3 > 1024) return "Wrong number of bases to trim (0-1024).";
  if (o.trim_qual < 0 || o.trim_qual > 93) return "Wrong trimming quality (1-93).";
  if (!o.adapter1 && (o.adapter2 || o.adapter_overlap_given || o.adapter_err_given)) return "--adapter2, --adapter-overlap and --adapter-err need --adapter.";
  if (o.adapter2 && !paired) return "--adapter2 needs --read2.";
  if ((o.adapter1 && !adapter_ok(o.adapter1)) || (o.adapter2 && !adapter_ok(o.adapter2))) return "Wrong adapter sequence (4-64 letters of ACGT).";
  if (o.adapter1 && (o.adapter_overlap < 1 || o.adapter_overlap > (long long)std::min(strlen(o.adapter1), strlen(o.adapter2 ? o.adapter2 : o.adapter1))))
    return "Wrong adapter overlap (1 to the adapter's length).";
  if (o.adapter1 && (o.adapter_err < 0 || o.adapter_err > 30)) return "Wrong adapter error percentage (0-30).";
  if (!o.trim_overlap && (o.trim_overlap_min_given || o.trim_overlap_err_given)) return "--trim-overlap-min and --trim-overlap-err need --trim-overlap.";
  if (o.trim_overlap && !paired) return "--trim-overlap needs read pairs (--read2).";
  if (o.trim_overlap && (o.trim_overlap_min < 8 || o.trim_overlap_min > 1024)) return "Wrong overlap of the mates (8-1024).";
  if (o.trim_overlap && (o.trim_overlap_err < 0 || o.trim_overlap_err > 30)) return "Wrong overlap error percentage (0-30).";
  if (!o.coverage && (o.coverage_window_given || o.coverage_all || o.coverage_mapq_given)) return "--coverage-window, --coverage-all and --coverage-mapq need --coverage.";
  if (o.coverage && (o.coverage_window < 1 || o.coverage_window > 1000000)) return "Wrong coverage window (1-1000000).";
  if (o.coverage_mapq_given && (o.coverage_mapq < 1 || o.coverage_mapq > 60)) return "Wrong coverage MAPQ threshold (1-60).";
  if (o.coverage_mapq_given && !o.mapq) return "--coverage-mapq needs --mapq.";
  if (!o.ref_path) return "Reference file path is required.";
  if (!o.index_path) return "Index file path is required.";
  if (!o.read_path) return "Read file path is required.";
  if (!o.out_path) return "Output file path is required.";
  if (o.n_gpus < 1 || o.n_gpus > 64) return "Wrong number of GPUs.";
  if (o.batch_reads < 1) return "Wrong batch size.";
  return nullptr;
}

// What the host-side paths cannot serve, a row each in the order it is looked at: the option, whether FEM_HOST_QUALS=1 refuses it
// as FEM_HOST_TAIL=1 and FEM_HOST_FORMAT=1 do, and what is said (about the first of the variables that is set).
const struct {
  bool MapOptions::*given;
  bool quals_too;
  const char *refusal;
} host_refusals[] = {
    {&MapOptions::bam, true, "--bam is not supported with %s=1: BAM records are made on the device, with the qualities there.\n"},
    {&MapOptions::mate_tags, true, "--mate-tags is not supported with %s=1: the mate tags are made on the device, with the qualities there.\n"},  // (ms:i is a sum over the mate's qualities)
    {&MapOptions::sam_seq, true, "--sam-seq is not supported with %s=1: SEQ and QUAL are turned on the device, with the qualities there.\n"},  // (the host would fill QUAL in forward)
    // (the cut kinds of the device's trim stage, DESIGN.md §4.6p.1: the whole read around its kept part, clips, SEQ and QUAL are the device's)
    {&MapOptions::trim_given, true, "--trim5, --trim3 and --trim-qual are not supported with %s=1: the reads are trimmed and their soft clips written on the device, with the qualities there.\n"},
    {&MapOptions::adapter_given, true, "--adapter is not supported with %s=1: the adapter is cut and the soft clips written on the device, with the qualities there.\n"},
    {&MapOptions::trim_overlap, true, "--trim-overlap is not supported with %s=1: the mates are cut and the soft clips written on the device, with the qualities there.\n"},
    {&MapOptions::mapq, false, "--mapq is not supported with %s=1: mapping qualities are made on the device, with its SAM text or BAM.\n"},  // (the host formatter has no MAPQ path)
    {&MapOptions::unmapped, false, "--unmapped is not supported with %s=1: the lines of unmapped reads are made on the device, with its SAM text or BAM.\n"},
    {&MapOptions::tags, false, "--rg and --nh are not supported with %s=1: the tags are made on the device, with its SAM text or BAM.\n"},
    // (the folding acts on the device's lines; FEM_HOST_QUALS=1 is served, XA stands behind QUAL)
    {&MapOptions::xa_given, false, "--xa is not supported with %s=1: the secondary lines are folded on the device, with its SAM text or BAM.\n"},
    {&MapOptions::coverage, false, "--coverage is not supported with %s=1: the coverage track is summed on the device, from the lines of its SAM text or BAM.\n"},
    {&MapOptions::report, false, "--strata and --max-hits are not supported with %s=1: the lines are filtered on the device, with its SAM text or BAM.\n"}};

void refuse_host_paths(const MapOptions &o) {
  for (const auto &row : host_refusals)
    for (int v = 0; v < (row.quals_too ? 3 : 2); ++v)
      if (o.*row.given && o.host_env[v]) {
        fprintf(stderr, row.refusal, kHostEnv[v]);
        exit(EXIT_FAILURE);
      }
}

// The counters of a batch's output lines beside the five of MappingStats, a row each in the order they are read and printed:
// whether the run counts it, its count call (one or two values) and its line or two lines on stderr.  The last three are the cut
// kinds of the device's trim stage: the trimmed reads and bases are those of every kind, so any kind counts them.
// (None is part of the all-reduce of the five: they are summed on the host, per GPU.)
constexpr int kCounters = 9;
const struct {
  bool MapOptions::*enabled;
  int (*count)(fem_dev *, int slot, uint64_t *v);
  const char *line[2];
} counters[kCounters] = {
    {&MapOptions::paired, fem_dev_pair_count, {"The number of proper pairs", nullptr}},
    {&MapOptions::rescue_given, fem_dev_rescue_count, {"The number of rescued mates", nullptr}},
    {&MapOptions::rescue_discordant, fem_dev_rescue_discordant_count, {"The number of rescued discordant pairs", nullptr}},
    {&MapOptions::unmapped, fem_dev_unmapped_count, {"The number of unmapped reads", nullptr}},
    {&MapOptions::report, fem_dev_filtered_count, {"The number of filtered lines", nullptr}},
    {&MapOptions::xa_given, fem_dev_xa_count, {"The number of XA entries", nullptr}},
    {&MapOptions::clip_given, [](fem_dev *h, int s, uint64_t *v) { return fem_dev_trim_count(h, s, &v[0], &v[1]); }, {"The number of trimmed reads", "The number of trimmed bases"}},
    {&MapOptions::adapter_given, [](fem_dev *h, int s, uint64_t *v) { return fem_dev_adapter_count(h, s, &v[0], &v[1]); }, {"The number of reads with adapter", "The number of adapter bases"}},
    {&MapOptions::trim_overlap, [](fem_dev *h, int s, uint64_t *v) { return fem_dev_pair_overlap_count(h, s, &v[0], &v[1]); }, {"The number of pairs with overlap cut", "The number of overlap bases"}}};

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
  uint64_t n_line[kCounters][2] = {};       // the batch's values of `counters`
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
struct WriteItem {
  TextOut *t = nullptr;   // host-rendered text, or
  BatchBuf *b = nullptr;  // a batch whose text the device rendered (b->sam)
};
struct Planned {  // the planner's cut of the next batch out of the input
  fem_batch_plan *plan = nullptr;
  fem_batch_shape shape{};
  int rc = 0;
  fem_batch_plan *plan2 = nullptr;  // paired: as many records of --read2 (one, to see that it ends, behind the end of --read1)
  fem_batch_shape shape2{};
  int rc2 = 0;
};

// --coverage: the track's windows, from the sequences' lengths alone, before the index is read and before any device is opened
uint64_t coverage_layout(const MapOptions &o, const Reference &ref) {
  std::vector<uint64_t> coverage_off((size_t)ref.view.n_seq + 1);
  uint64_t coverage_bins = 0;
  if (fem_coverage_layout(ref.view.n_seq, ref.view.len, (int32_t)o.coverage_window, coverage_off.data(), &coverage_bins) != 0) {
    const int32_t least = fem_coverage_min_window(ref.view.n_seq, ref.view.len);
    if (least) fprintf(stderr, "--coverage-window %lld gives %lu windows on this reference, more than 2^29; the least window that fits is %d.\n",
                       o.coverage_window, (unsigned long)coverage_bins, least);
    else fprintf(stderr, "--coverage: this reference has more than 2^29 windows at every window up to 1000000.\n");
    exit(EXIT_FAILURE);
  }
  return coverage_bins;
}

struct Index {
  int32_t k = 0, step = 0;
  uint32_t *lookup = nullptr;
  uint64_t *occ = nullptr, n_occ = 0;
};
void load_index(const MapOptions &o, Index *ix) {
  double t_idx = real_time();
  if (fem_index_load(o.index_path, &ix->k, &ix->step, &ix->lookup, &ix->n_occ, &ix->occ) != 0) {
    fprintf(stderr, "Failed to open index file %s\n", o.index_path);
    exit(EXIT_FAILURE);
  }
  fprintf(stderr, "Loaded index in %fs!\n", real_time() - t_idx);
  if (ix->k != o.params.k) {  // the reference would silently index a 4^12 table with the wrong hashes; refuse instead
    fprintf(stderr, "Index was built with k=%d but map always uses k=%d.\n", ix->k, o.params.k);
    exit(EXIT_FAILURE);
  }
}

struct BatchSizes {  // what a batch's buffers are sized for
  uint64_t batch_bytes = 0;  // the FASTQ window a batch is cut from
  uint64_t reads_cap0 = 0, bases_cap0 = 0, names_cap0 = 0;  // the slots' staging at the start (the reader asks for larger buffers when a batch needs them)
  uint64_t res_reads = 0;  // what the device library reserves for a batch during the setup (0: nothing)
  uint32_t res_len = 0;
};
BatchSizes size_batches(const MapOptions &o) {
  BatchSizes z;
  uint64_t batch_reads = o.batch_reads;
  if (!o.batch_given) {
    struct stat st;
    if (stat(o.read_path, &st) == 0 && st.st_size >= (off_t)(1ll << 30)) batch_reads = 1000000;  // (plain FASTQ of >= ~4 M reads)
  }
  z.batch_bytes = batch_reads * 250ull;  // header + bases + '+' + qualities of a ~100 bp record
  // a FASTQ window of batch_bytes characters holds fewer than batch_bytes / 2 bases; records under 32 bytes are unusual
  z.reads_cap0 = z.batch_bytes / 32 + 16, z.bases_cap0 = z.batch_bytes / 2 + 4096, z.names_cap0 = z.bases_cap0 / 2 + 4096;
  // What a batch will look like, from the input's first records: the device library then makes a batch's allocations during
  // the setup (fem_dev_reserve_batch) instead of between the first batches' kernels.
  if (o.device_text) {
    if (fem_seqfile *f0 = fem_seqfile_open(o.read_path)) {
      fem_batch_plan *pl = nullptr;
      fem_batch_shape sh{};
      if (fem_seqfile_plan(f0, 1u << 18, 1, &pl, &sh) == 0 && pl && sh.n_reads > 0) {
        const uint64_t per_record = (2 * sh.n_bases + sh.n_name_bytes) / sh.n_reads + 6;
        z.res_reads = z.batch_bytes / per_record + z.batch_bytes / per_record / 8 + 1024, z.res_len = sh.max_len;
      }
      fem_batch_plan_free(pl);
      fem_seqfile_close(f0);
    }
  }
  return z;
}

// the SAM text (or BAM) a slot's batch may come to, for fem_dev_reserve_text
uint64_t text_estimate(const MapOptions &o, const BatchSizes &z) {
  // (--unmapped: a read of which nothing maps still has a line of its name, bases and qualities)
  const uint64_t lines = z.batch_bytes + z.batch_bytes / (o.unmapped ? 2 : 4);
  // (--rg / --nh: the tags of a line, one line per read at the least)
  uint64_t per_read = (o.rg_arg ? 6 + strlen(o.rg_id) : 0) + (o.hit_tags ? 16 : 0);
  // (--mate-tags: MC of a few operations, MQ, ms)
  per_read += o.mate_tags ? 16 + 9 + 12 : 0;
  // (trimming: two S operations on a line's CIGAR and on its MC; the clipped letters are part of the read's already)
  per_read += o.clip_given ? 10 + (o.mate_tags ? 10 : 0) : 0;
  return lines + z.reads_cap0 * per_read;
}

// the options of the output's lines and of the trim stage, on one slot of a handle
int configure_slot(fem_dev *h, int sl, const MapOptions &o) {
  int rc = 0;
  if (!rc && o.mapq) rc = fem_dev_set_mapq(h, sl, 1);
  if (!rc && o.unmapped) rc = fem_dev_set_unmapped(h, sl, 1);
  if (!rc && o.report) {
    const fem_report_params fp{(int32_t)o.strata, (int32_t)o.max_hits};
    rc = fem_dev_set_report(h, sl, &fp);
  }
  if (!rc && o.tags) {
    const fem_tag_params tp{o.rg_arg ? o.rg_id : nullptr, o.hit_tags ? 1 : 0};
    rc = fem_dev_set_tags(h, sl, &tp);
  }
  if (!rc && o.sam_seq) rc = fem_dev_set_sam_seq(h, sl, 1);
  if (!rc && o.xa_given) rc = fem_dev_set_xa(h, sl, (int32_t)o.xa_entries);
  if (!rc && o.trim_given) {
    const fem_trim_params tp{(int32_t)o.trim5, (int32_t)o.trim3, (int32_t)o.trim_qual};
    rc = fem_dev_set_trim(h, sl, &tp);
  }
  if (!rc && o.adapter_given) {
    const fem_adapter_params ap{o.adapter1, o.adapter2, (int32_t)o.adapter_overlap, (int32_t)o.adapter_err};
    rc = fem_dev_set_adapter(h, sl, &ap);
  }
  if (!rc && o.trim_overlap) {
    const fem_pair_overlap_params vp{(int32_t)o.trim_overlap_min, (int32_t)o.trim_overlap_err};
    rc = fem_dev_set_pair_overlap(h, sl, &vp);
  }
  if (!rc && o.paired) {  // read pairs: paired and rendered on the device only (fem_dev_set_pairs), the reads staged as characters
    const fem_pair_params pp{(int32_t)o.min_insert, (int32_t)o.max_insert};
    rc = fem_dev_set_pairs(h, sl, &pp);
    if (!rc && o.orientation_given && o.orientation != kOrientAuto) rc = fem_dev_set_orientation(h, sl, o.orientation);
    if (!rc && o.mate_tags) rc = fem_dev_set_mate_tags(h, sl, 1);
    if (!rc && o.rescue_given) {
      const fem_rescue_params rp{(int32_t)o.rescue_edits};
      rc = fem_dev_set_rescue(h, sl, &rp);
    }
    if (!rc && o.rescue_discordant) rc = fem_dev_set_rescue_discordant(h, sl, 1);
  }
  return rc;
}

// one thread per GPU uploads the replicated reference + index (src/FEM_map.c:135-143) and sets its slots up; frees the index
int open_devices(const MapOptions &o, const Reference &ref, const Index &ix, const BatchSizes &z, std::vector<fem_dev *> *devs) {
  (void)fem_set_blocking_waits(1);  // (a thread per batch in flight waits for the device; the parser needs the cores)
  const double t_dev = real_time();
  std::vector<int> up_rc((size_t)o.n_gpus, 0);
  std::vector<std::thread> up;
  for (int g = 0; g < o.n_gpus; ++g)
    up.emplace_back([&, g] {
      fem_dev *&h = (*devs)[(size_t)g];
      if (o.n_gpus > 1 && !o.share_gpu) (void)fem_bind_thread_near_device(g);  // the handle's pinned result buffers
      int rc = fem_dev_open(o.share_gpu ? 0 : g, &h);
      if (!rc) rc = ref.upload(h);
      if (!rc) rc = fem_dev_upload_index(h, ix.k, ix.step, ix.lookup, ((uint64_t)1 << (2 * ix.k)) + 1, ix.occ, ix.n_occ);
      // the slots' pinned staging (and, for the device's SAM text, its buffers): pinning host memory takes ~0.25 ms per
      // MB, 35 ms per slot here, and belongs to the setup rather than to the first batches
      int32_t ns = 4;
      uint32_t max_read_len = 0;
      if (!rc) (void)fem_dev_limits(h, &max_read_len, &ns);
      for (int sl = 0; !rc && sl < ns; ++sl) {
        char *pb = nullptr, *pq = nullptr, *pn = nullptr;
        uint64_t *po = nullptr, *pno = nullptr;
        rc = fem_dev_acquire_stage(h, sl, z.reads_cap0, z.bases_cap0, &pb, &po);
        if (!rc && o.device_text) rc = fem_dev_acquire_text_stage(h, sl, z.reads_cap0, z.bases_cap0, z.names_cap0, &pq, &pn, &pno);
        if (!rc && o.device_text) rc = fem_dev_reserve_text(h, sl, z.reads_cap0, z.bases_cap0, z.names_cap0, text_estimate(o, z));
        // (a read over the device's limit among the first records: no reservation, the staging of its batch names the read)
        if (!rc && o.device_text && z.res_reads && z.res_len <= max_read_len)
          rc = fem_dev_reserve_batch(h, sl, z.res_reads, z.res_reads + z.res_reads / 8, z.res_len, &o.params);
        if (!rc) rc = configure_slot(h, sl, o);
      }
      up_rc[(size_t)g] = rc;
    });
  for (auto &t : up) t.join();
  for (int g = 0; g < o.n_gpus; ++g)
    if (up_rc[(size_t)g]) return dev_fail((*devs)[(size_t)g], "device setup (mapping runs on the GPU; no CPU path)", up_rc[(size_t)g]);
  free(ix.lookup), free(ix.occ);
  fprintf(stderr, "Reference and index resident on %d GPU%s in %fs.\n", o.n_gpus, o.n_gpus > 1 ? "s" : "", real_time() - t_dev);
  if (env_var("FEM_TESTING").c == '1') {  // (a test that steers the kernel choice through the environment reads here what ran)
    char info[512] = "";
    (void)fem_dev_index_info((*devs)[0], info, sizeof info);
    fprintf(stderr, "Seed kernel: %s (index: %s).\n", fem_dev_seed_kernel((*devs)[0], &o.params), info);
  }
  return 0;
}

// --infer-insert: the insert size range from the input's first pairs, before anything is written and before the first batch
// is read: the sample is mapped single-end on the first device and its unique pairs say what the library's inserts are
// (fem_dev_estimate_insert).  The range then holds for the whole run, whatever --batch, -t and --gpus are; the main pass reads
// the input from its start and counts nothing of this.  Files that do not give as many records each, or a sample the reader
// cannot parse: no estimate, and the main pass reports the input as it does without the switch.
// --orientation auto: the same sample says which orientation the library has, too (fem_dev_estimate_library): the one under
// which most of its unique pairs are informative; the range is then that orientation's.
// What is learned is set on every slot of every handle; nothing else of the run reads it.
int infer_library(const MapOptions &o, const std::vector<fem_dev *> &devs) {
  const bool learn_orientation = o.orientation == kOrientAuto;
  int orientation = o.orientation;
  fem_library_estimate lib{};
  lib.orientation = -1;
  const double t_pre = real_time();
  fem_seqset mate[2] = {};
  bool sampled = true;
  for (int m = 0; m < 2; ++m) {
    fem_seqfile *f = fem_seqfile_open(m ? o.read2_path : o.read_path);
    sampled = sampled && f && fem_seqfile_read(f, (uint64_t)o.infer_pairs, &mate[m]) == 0;
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
    if (!rc && o.trim_qual > 0) {  // ... by its qualities, which go to the device in front of the mapping then; the names are not needed: empty ones
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
    if (!rc && sampled) rc = fem_dev_map_staged(h, 0, &o.params);
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
                c3, S, FEM_INSERT_MIN_PAIRS, o.min_insert, o.max_insert);
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
            (unsigned long)est.n_informative, (unsigned long)est.n_pairs, FEM_INSERT_MIN_PAIRS, o.min_insert, o.max_insert);
  }
  if (o.stage_times) fprintf(stderr, "[FEM] insert size pre-pass: %fs\n", real_time() - t_pre);
  return 0;
}

// ---- the pipeline: what its threads share, and a member function per thread ----
struct MapRun {
  const MapOptions &o;
  const BatchSizes &z;
  const std::vector<fem_dev *> &devs;
  const Reference &ref;
  const int out_fd;
  std::atomic<int> exit_code{0};
  double t_start = 0;  // the mapping phase begins (run)
  int rd_threads = 0, fmt_threads = 0;  // the -t threads of the parser and of the formatter
  int32_t n_slots = 4;
  fem_seqfile *read_file = nullptr, *read2_file = nullptr;  // opened by the reader, closed by map_main when the mapping phase is over
  fem_seqfile *f = nullptr, *f2 = nullptr;  // ... as the planner and the reader read them (f: null where one of them could not be opened)

  std::vector<BatchBuf> bufs;  // n_slots per GPU
  Channel<BatchBuf *> free_q, text_q, regrown_q;  // writer / formatter / workers -> reader; workers -> formatter; worker -> reader
  std::vector<Channel<Msg>> work_q = std::vector<Channel<Msg>>(devs.size());  // per GPU: reader (and its own retiring threads) -> worker
  Channel<TextOut *> text_free_q;  // writer -> formatter
  Channel<WriteItem> write_q;      // formatter / workers -> writer
  std::vector<TextOut> texts = std::vector<TextOut>(3);
  Channel<Planned> planned_q;  // planner -> reader
  Channel<int> plan_tokens;  // a plan is made per token: one while nothing may run ahead, two where it may
  std::atomic<bool> plan_stop{false};

  // busy and waiting seconds (FEM_STAGE_TIMES): each written by one thread (reader, formatter, writer, planner, worker g) and read
  // after its join, except
  double busy_read = 0, busy_text = 0, busy_write = 0, busy_plan = 0;
  std::mutex stat_mu;  // (busy_text: the batches' retiring threads add to it)
  double wait_slot = 0, wait_records = 0, wait_text_buf = 0;  // reader waiting for a free slot, formatter for records / a text buffer
  std::vector<double> busy_submit = std::vector<double>(devs.size(), 0.0), busy_recycle = busy_submit, busy_wait = busy_submit;  // per GPU
  double t_first_slot = 0, t_first_filled = 0, t_reader_done = 0, t_workers_done = 0;
  std::atomic<uint64_t> n_asserted{0};
  std::vector<uint64_t> per_gpu = std::vector<uint64_t>(devs.size() * 5, 0);                    // per GPU, by its worker's sequencer: the five counters of MappingStats
  std::vector<uint64_t> per_gpu_lines = std::vector<uint64_t>(devs.size() * kCounters * 2, 0);  // ... and the values of `counters`

  MapRun(const MapOptions &o_, const BatchSizes &z_, const std::vector<fem_dev *> &d, const Reference &r, int fd) : o(o_), z(z_), devs(d), ref(r), out_fd(fd) {}
  bool write_all(const char *p, uint64_t n);
  void write_error() {
    if (!exit_code.exchange(EXIT_FAILURE)) fprintf(stderr, "[FEM] write error on %s\n", o.out_path);
  }
  bool write_header();
  void run();
  void writer();
  void formatter();
  void worker(int g);
  void planner();
  int fill_pair(fem_batch_plan *pa, fem_batch_plan *pb, const fem_batch_shape &sa, BatchBuf *b);
  void reader();
  void finish_output();
  void reduce_stats();
  uint64_t write_coverage(uint64_t coverage_bins);
};

// The SAM text of a batch is a handful of stretches (one per formatter thread), written one after the other.  (Side
// by side with pwrite from four threads was tried twice: round 3 on tmpfs, 2.8 GB/s against 5.5 from one thread; round 5 on
// the GPU box's /tmp, where four writers into four FILES take 56-61 GB/s against 16.5 from one: into ONE file 10.4 GB/s with
// one, four or eight writers — buffered writes to a file take its inode's lock.)
bool MapRun::write_all(const char *p, uint64_t n) {
  while (n) {
    ssize_t w = write(out_fd, p, n);
    if (w < 0 && errno == EINTR) continue;
    if (w <= 0) return false;
    p += w, n -= (uint64_t)w;
  }
  return true;
}

// the SAM header, or the BAM header through the device's compressor; false: the run ends here (reported)
bool MapRun::write_header() {
  if (o.bam) {
    uint8_t *raw = nullptr;
    uint64_t rl = 0, zl = 0;
    int rc = o.header ? fem_bam_header_full(&ref.view, o.rg_line, o.pg_line, &raw, &rl) : fem_bam_header(&ref.view, &raw, &rl);
    if (rc == -5) {
      fprintf(stderr, "A reference sequence of 2^31 bases or more cannot be written as BAM.\n");
      exit(EXIT_FAILURE);
    }
    if (rc) {
      fprintf(stderr, "BAM header failed (%d)\n", rc);
      exit(EXIT_FAILURE);
    }
    std::vector<uint8_t> zb((size_t)(rl / 65280 + 1) * 65536);
    rc = fem_dev_bgzf_compress(devs[0], raw, rl, o.bam_level, zb.data(), zb.size(), &zl);
    free(raw);
    if (rc) {
      dev_fail(devs[0], "BAM header", rc);
      return false;
    }
    if (!write_all((const char *)zb.data(), zl)) write_error();
  } else {
    char *hdr = nullptr;
    uint64_t hl = 0;
    if (o.header) fem_sam_header_full(&ref.view, o.rg_line, o.pg_line, &hdr, &hl);
    else fem_sam_header(&ref.view, &hdr, &hl);
    if (!write_all(hdr, hl)) write_error();
    free(hdr);
  }
  return true;
}

// ---- writer (src/output_queue.c:60-91) ----
void MapRun::writer() {
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
      if (!ok) write_error();
      busy_write += real_time() - t_w;
      fprintf(stderr, "Mapped read batch in %fs.\n", real_time() - it.b->t_submit);
      if (o.batch_times)
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
    if (!ok) write_error();
    if (t->owned_elsewhere) {
      free(t->buf);
      t->buf = nullptr, t->cap = 0, t->owned_elsewhere = false;
    }
    busy_write += real_time() - t0;
    text_free_q.push(t);
  }
}

// ---- formatter: records -> SAM text (src/align.c:546-632, src/output_queue.c:93-116) ----
void MapRun::formatter() {
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
    if (o.host_tail) {  // FEM_HOST_TAIL=1: ordering / traceback / MD by libfemhost from the per-candidate outcome
      fem_tail_input in{b->res.n_reads, b->res.cand_begin, b->res.cand_count, b->res.cand, b->res.ed, b->res.end};
      char *text = nullptr;
      uint64_t len = 0;
      fmt = fem_tail_sam(o.params.e, &ref.view, &reads, &in, fmt_threads, &text, &len);
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
}

// ---- one worker per GPU (the mapping threads of src/FEM_map.c:182-185): the only thread that submits to that GPU's handle ----
void MapRun::worker(int g) {
  fem_dev *h = devs[(size_t)g];
  if (o.n_gpus > 1 && !o.share_gpu) (void)fem_bind_thread_near_device(g);
  auto acquire = [&](BatchBuf *b, uint64_t reads_cap, uint64_t bases_cap) -> bool {
    char *pb = nullptr;
    uint64_t *po = nullptr;
    int rc = fem_dev_acquire_stage(h, b->slot, reads_cap, bases_cap, &pb, &po);
    if (rc) {
      if (!exit_code.exchange(EXIT_FAILURE)) dev_fail(h, "staging buffers", rc);
      return false;
    }
    b->bases = pb, b->off = po, b->reads_cap = reads_cap, b->bases_cap = bases_cap;
    if (o.device_text) {  // qualities and names go to the GPU as well: pinned staging for them
      const uint64_t names_cap = std::max<uint64_t>(b->want_names, std::max<uint64_t>(b->names_cap, z.names_cap0));
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
    if (!acquire(b, z.reads_cap0, z.bases_cap0)) b->bases = nullptr;  // (allocated during the setup: this only hands them out)
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
    fem_batch_bam zb{};
    const int rc = fem_dev_fetch_bam_nowait(hd, b->slot, o.bam_level, &zb);
    if (rc) return rc;
    b->sam.text = (const char *)zb.data, b->sam.len = zb.len, b->sam.n_records = zb.n_records, b->sam.n_asserted = zb.n_asserted;
    memcpy(b->sam.stats, zb.stats, sizeof zb.stats);
    return FEM_OK;
  };
  auto retire = [&](BatchBuf *b) {
    double t0 = real_time();
    int rc = o.host_tail     ? fem_dev_map_batch_wait(h, b->slot, &b->res)
             : o.bam         ? fetch_bam(h, b)
             : o.device_text ? fem_dev_fetch_sam_nowait(h, b->slot, &b->sam)  // (the writer waits for the text itself)
                             : fem_dev_fetch_records(h, b->slot, &b->rec);
    for (int k = 0; k < kCounters; ++k)
      if (!rc && o.*counters[k].enabled) rc = counters[k].count(h, b->slot, b->n_line[k]);
    const double waited = real_time() - t0;
    b->t_retired = t0 + waited;
    double placing = 0;
    if (!rc && o.host_quals) {
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
                                   std::max(1, o.n_threads / 2));
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
      const uint64_t *st = o.host_tail ? b->res.stats : o.device_text ? b->sam.stats : b->rec.stats;
      for (int i = 0; i < 5; ++i) per_gpu[(size_t)g * 5 + (size_t)i] += st[i];
      for (int i = 0; i < kCounters * 2; ++i) per_gpu_lines[(size_t)g * kCounters * 2 + (size_t)i] += b->n_line[i / 2][i % 2];
      if (o.device_text) {
        n_asserted += b->sam.n_asserted;
        write_q.push(WriteItem{nullptr, b});
      } else {
        text_q.push(b);
      }
    });
  };
  const int n_retire = std::max(1, std::min(n_slots, o.flight));  // (one per slot: a batch's thread also waits for its text and places the qualities)
  std::vector<std::thread> retirers;
  for (int r = 0; r < n_retire; ++r)
    retirers.emplace_back([&] {
      if (o.n_gpus > 1 && !o.share_gpu) (void)fem_bind_thread_near_device(g);
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
    if (!rc && o.trim_given) rc = fem_dev_commit_text_stage(h, b->slot, b->shape.n_reads, b->shape.n_name_bytes);
    if (!rc) rc = fem_dev_map_staged(h, b->slot, &o.params);
    const double t_c2 = real_time();
    // (qualities and names behind the mapping's launches: the call that hands the link 140 MB can wait for room in the copy
    //  engine's queue, 8-10 ms now and then, and the kernels need none of it)
    if (!rc && o.device_text && !o.trim_given)
      rc = o.host_quals ? fem_dev_commit_names_stage(h, b->slot, b->shape.n_reads, b->shape.n_name_bytes)
                        : fem_dev_commit_text_stage(h, b->slot, b->shape.n_reads, b->shape.n_name_bytes);
    if (o.batch_times && real_time() - b->t_submit > 1e-3)
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
}

// The planner: cuts the next batch out of the input (one pass over it: where the records end, how many, how long) on a
// thread of its own, ahead of the batch being filled where the file allows it (plain FASTQ through a mapping: a plan's records
// stay where they are) — a batch's plan needs no staging slot, so it is also made while the reader waits for one.  On boxes
// whose cores are slow the reader's plan-then-fill in a row bounded the run (32 M reads of C3: 118-121 Mreads/s against
// 130-140 elsewhere, the reader busy 0.19-0.24 of the run's 0.25-0.27 s).
void MapRun::planner() {
  while (f) {
    (void)plan_tokens.pop();
    if (plan_stop) break;
    Planned pl;
    const double t_p = real_time();
    pl.rc = fem_seqfile_plan(f, o.paired ? z.batch_bytes / 2 : z.batch_bytes, rd_threads, &pl.plan, &pl.shape);
    if (o.paired && pl.plan && pl.rc == 0)  // the mates: cut by count where the first file was cut by bytes
      pl.rc2 = fem_seqfile_plan_count(f2, std::max<uint64_t>(pl.shape.n_reads, 1), rd_threads, &pl.plan2, &pl.shape2);
    busy_plan += real_time() - t_p;
    const bool last = !pl.plan || pl.rc != 0 || pl.shape.n_reads == 0;
    planned_q.push(pl);
    if (last) break;
  }
}

// A batch of read pairs in the slot's staging: mate 1's records, then mate 2's behind them (offsets and name offsets running
// on), a trailing /1 or /2 taken off every name, the two names of each pair compared.  0 = filled, 2 = the names differ
// (reported here), anything else = the reader failed.  Frees both plans.
int MapRun::fill_pair(fem_batch_plan *pa, fem_batch_plan *pb, const fem_batch_shape &sa, BatchBuf *b) {
  int frc = fem_seqfile_fill(f, pa, rd_threads, b->bases, b->off, b->q_stage, b->n_stage, b->no_stage);
  const uint64_t n1 = sa.n_reads, nb1 = sa.n_bases, nn1 = sa.n_name_bytes;
  if (frc) {
    fem_batch_plan_free(pb);
    return frc;
  }
  frc = fem_seqfile_fill(f2, pb, rd_threads, b->bases + nb1, b->off + n1, b->q_stage + nb1, b->n_stage + nn1, b->no_stage + n1);
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
}

// ---- reader (src/input_queue.c:53-79): parses the planner's batches into the staging of whichever (GPU, slot) is free ----
void MapRun::reader() {
  f = read_file = fem_seqfile_open(o.read_path);
  f2 = read2_file = o.paired ? fem_seqfile_open(o.read2_path) : nullptr;
  if (!f || (o.paired && !f2)) {
    fprintf(stderr, "Cannot find sequence file!");  // the reference exits here (src/sequence_batch.c:33-35)
    exit_code = EXIT_FAILURE;
    f = nullptr;
  }
  const bool ahead = f && fem_seqfile_plan_ahead_ok(f) && (!o.paired || fem_seqfile_plan_ahead_ok(f2)) && o.plan_ahead;
  plan_tokens.push(1);
  if (ahead) plan_tokens.push(1);
  std::thread planner_thread(&MapRun::planner, this);
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
    if (o.paired && ok && rc == 0) {
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
        (b->shape.n_reads > b->reads_cap || b->shape.n_bases + 64 > b->bases_cap || (o.device_text && b->shape.n_name_bytes + 64 > b->names_cap))) {
      b->want_reads = std::max(b->reads_cap, b->shape.n_reads + b->shape.n_reads / 8);
      b->want_bases = std::max(b->bases_cap, b->shape.n_bases + b->shape.n_bases / 8 + 4096);
      b->want_names = b->shape.n_name_bytes + b->shape.n_name_bytes / 8 + 4096;
      work_q[(size_t)b->gpu].push(Msg{kRegrow, b});
      BatchBuf *back = regrown_q.pop();  // (one request at a time: it is ours)
      ok = back->bases != nullptr;
    }
    if (ok && b->shape.n_reads > 0 && !o.device_text) {
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
    if (o.pack_bases && b->shape.min_len == b->shape.max_len && b->shape.n_bases < 0xFFFFFFF0ull) {
      // reads of one length: two bits per base straight into the staging; 1 = too many characters outside "ACGT" for that form
      uint64_t exc_cap = 0;
      const bool lay = fem_dev_packed_layout(b->shape.n_reads, b->shape.max_len, nullptr, nullptr, &exc_cap) == FEM_OK;
      if (lay && o.splice) {
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
      } else if (lay && o.device_text) {
        rc = fem_seqfile_fill_packed(f, plan, rd_threads, b->shape.max_len, (uint8_t *)b->bases, exc_cap, &b->n_exc, b->q_stage, b->n_stage,
                                     b->no_stage);
        b->packed = rc == 0;
      }
    }
    if (rc == 1 && o.paired) {
      rc = fill_pair(plan, pd.plan2, pd.shape, b);
      pd.plan2 = nullptr;
      if (rc == 2) {
        exit_code = EXIT_FAILURE;
        break;
      }
    } else if (rc == 1) {
      rc = o.device_text ? fem_seqfile_fill(f, plan, rd_threads, b->bases, b->off, b->q_stage, b->n_stage, b->no_stage)
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
  planner_thread.join();
  {
    Planned pd;
    while (!planner_done && planned_q.try_pop_for(pd, 0.0)) fem_batch_plan_free(pd.plan), fem_batch_plan_free(pd.plan2);
  }
  // (the file stays open until the mapping phase is over: unmapping 4 GB of faulted-in pages takes 0.08 s, which the GPUs
  // would otherwise spend waiting for their stop message)
  t_reader_done = real_time();
}

// The mapping phase: the stages started, the reader on this thread, and the stages stopped in the order of the batches' way.
void MapRun::run() {
  t_start = real_time();
  double cpu_u0 = 0, cpu_s0 = 0;
  cpu_seconds(&cpu_u0, &cpu_s0);
  const bool split = !o.device_text && o.split_threads;
  rd_threads = split ? std::max(1, std::min(o.n_threads - 1, (o.n_threads * o.reader_share + 50) / 100)) : o.n_threads;
  fmt_threads = split ? o.n_threads - rd_threads : o.n_threads;
  (void)fem_dev_limits(devs[0], nullptr, &n_slots);
  bufs = std::vector<BatchBuf>((size_t)o.n_gpus * (size_t)n_slots);
  for (TextOut &t : texts) text_free_q.push(&t);
  std::thread writer_thread(&MapRun::writer, this), formatter_thread(&MapRun::formatter, this);
  std::vector<std::thread> workers;
  for (int g = 0; g < o.n_gpus; ++g) workers.emplace_back(&MapRun::worker, this, g);
  reader();
  for (int g = 0; g < o.n_gpus; ++g) work_q[(size_t)g].push(Msg{kStop, nullptr});
  for (auto &w : workers) w.join();
  t_workers_done = real_time();
  text_q.push(nullptr);
  formatter_thread.join();
  write_q.push(WriteItem{});
  writer_thread.join();
  if (!o.stage_times) return;
  double bw = 0, bs = 0, br = 0;
  for (double x : busy_wait) bw += x;
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

// the end of the output file, and what is said about its records
void MapRun::finish_output() {
  if (o.bam) {  // the BGZF end-of-file marker (SAM/BAM specification 4.1.2)
    static const unsigned char eof[28] = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0, 27, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (!write_all((const char *)eof, sizeof eof)) write_error();
  }
  if (close(out_fd) != 0) write_error();
  if (n_asserted)
    fprintf(stderr, "[FEM] %lu records on which the reference would have tripped an assertion (src/align.c:366-368) were "
                    "written with CIGAR *\n", (unsigned long)n_asserted.load());
}

// MappingStats reduction (src/FEM_map.c:200-212): across GPUs it is one RCCL all-reduce of 5 counters -> per_gpu[0..5)
void MapRun::reduce_stats() {
  if (o.n_gpus > 1 && !exit_code && !o.share_gpu) {
    int rc = fem_dev_allreduce_stats(devs.data(), o.n_gpus, per_gpu.data());
    if (rc) exit_code = dev_fail(devs[0], "stats all-reduce", rc);
  } else if (o.n_gpus > 1) {
    for (int g = 1; g < o.n_gpus; ++g)
      for (int i = 0; i < 5; ++i) per_gpu[(size_t)i] += per_gpu[(size_t)g * 5 + (size_t)i];
  }
}

// --coverage: the devices' tracks home, summed, and the file (inside the timed phase: it is part of what the switch costs)
// -> the covered bases
uint64_t MapRun::write_coverage(uint64_t coverage_bins) {
  const fem_tail_ref &view = ref.view;
  uint64_t n_covered = 0;
  if (!o.coverage || exit_code) return 0;
  std::vector<uint64_t> bins((size_t)coverage_bins, 0), part(o.n_gpus > 1 ? (size_t)coverage_bins : 0);
  for (int g = 0; g < o.n_gpus && !exit_code; ++g) {
    uint64_t *to = g ? part.data() : bins.data();
    if (int rc = fem_dev_fetch_coverage(devs[(size_t)g], to, coverage_bins)) exit_code = dev_fail(devs[(size_t)g], "coverage track", rc);
    if (g && !exit_code)
      for (size_t k = 0; k < bins.size(); ++k) bins[k] += part[k];
  }
  if (!exit_code) {
    FILE *cf = fopen(o.coverage_path, "w");
    const int wrc = cf ? fem_coverage_write(cf, view.n_seq, view.names, view.name_off, view.len, (int32_t)o.coverage_window, bins.data(), &n_covered) : -3;
    if ((!cf || wrc || fclose(cf) != 0) && !exit_code.exchange(EXIT_FAILURE)) fprintf(stderr, "[FEM] write error on %s\n", o.coverage_path);
  }
  return n_covered;
}

void print_counters(const MapRun &run, uint64_t n_covered, double t_mapping) {
  static const char *const kStats[5] = {"read", "mapped read", "candidate before additional q-gram filter", "candidate", "mapping"};
  for (int i = 0; i < 5; ++i) fprintf(stderr, "The number of %s: %lu\n", kStats[i], (unsigned long)run.per_gpu[(size_t)i]);
  for (int k = 0; k < kCounters; ++k)
    for (int j = 0; j < 2 && run.o.*counters[k].enabled && counters[k].line[j]; ++j) {
      uint64_t sum = 0;
      for (int g = 0; g < run.o.n_gpus; ++g) sum += run.per_gpu_lines[((size_t)g * kCounters + (size_t)k) * 2 + (size_t)j];
      fprintf(stderr, "%s: %lu\n", counters[k].line[j], (unsigned long)sum);
    }
  if (run.o.coverage) fprintf(stderr, "The number of covered bases: %lu\n", (unsigned long)n_covered);
  fprintf(stderr, "Time: %fs\n", t_mapping);
}

int map_main(int argc, char **argv) {
  // Batches come and go as a few 100 MB allocations: keep them in the heap instead of mapping and unmapping them, so
  // that a recycled buffer's pages are already there (page faults were a visible share of the host time).
  mallopt(M_MMAP_MAX, 0);
  mallopt(M_TRIM_THRESHOLD, -1);
  MapOptions o;
  parse_map_options(argc, argv, &o);
  if (const char *bad = check_map_options(o)) {
    fprintf(stderr, "%s\n", bad);
    usage_map();
    exit(EXIT_FAILURE);
  }
  refuse_host_paths(o);
  // Host placement: with one GPU the whole process (parser, formatter, staging buffers) moves next to it, before any
  // thread pool exists; with several, each GPU's worker thread does so for itself and the buffers it acquires.
  if (o.n_gpus == 1 || o.share_gpu) (void)fem_bind_thread_near_device(0);
  Reference ref;
  if (!ref.load(o.ref_path)) exit(EXIT_FAILURE);
  const uint64_t coverage_bins = o.coverage ? coverage_layout(o, ref) : 0;
  Index ix;
  load_index(o, &ix);
  if (o.paired && !o.device_text) {
    fprintf(stderr, "%s is not supported with --read2: the paired SAM text is made on the device only.\n",
            o.host_tail ? "FEM_HOST_TAIL=1" : "FEM_HOST_FORMAT=1");
    exit(EXIT_FAILURE);
  }
  const BatchSizes z = size_batches(o);
  std::vector<fem_dev *> devs((size_t)o.n_gpus, nullptr);
  if (open_devices(o, ref, ix, z, &devs)) return EXIT_FAILURE;
  if (o.infer_insert && infer_library(o, devs)) return EXIT_FAILURE;
  // --coverage: every device keeps a track of its own from here on (behind the sample pass, which adds nothing to it); the host
  // sums them at the end
  if (o.coverage) {
    const fem_coverage_params cp{(int32_t)o.coverage_window, o.coverage_all ? 1 : 0, (int32_t)o.coverage_mapq};
    for (fem_dev *h : devs)
      if (int rc = fem_dev_set_coverage(h, &cp)) return dev_fail(h, "coverage track", rc);
  }
  const int out_fd = open(o.out_path, O_WRONLY | O_CREAT | O_TRUNC, 0666);
  if (out_fd < 0) {
    fprintf(stderr, "Cannot open output file %s\n", o.out_path);
    exit(EXIT_FAILURE);
  }
  MapRun run(o, z, devs, ref, out_fd);
  if (!run.write_header()) return EXIT_FAILURE;
  free(o.rg_line);
  if (o.device_text)
    for (fem_dev *h : devs) {
      int rc = fem_dev_upload_reference_names(h, (uint32_t)ref.set.n, ref.set.names, ref.set.name_off);
      if (rc) return dev_fail(h, "reference names", rc);
    }
  run.run();
  run.finish_output();
  run.reduce_stats();
  const uint64_t n_covered = run.write_coverage(coverage_bins);
  const double t_mapping = real_time() - run.t_start;  // (the reference's timer stops after the counter reduction, src/FEM_map.c:219)
  for (TextOut &t : run.texts) free(t.buf);
  if (run.read_file) fem_seqfile_close(run.read_file);
  if (run.read2_file) fem_seqfile_close(run.read2_file);
  for (fem_dev *h : devs) fem_dev_close(h);
  if (run.exit_code) return run.exit_code;
  print_counters(run, n_covered, t_mapping);
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
