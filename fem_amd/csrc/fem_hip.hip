// fem_hip.hip — host side of libfemhip.so: the C ABI declared in include/fem_hip.h.
// Owns device memory, streams, pinned result buffers and the launch logic of the
// kernels in fem_kernels.hip.h and fem_verify.hip.h.  No CPU fallback: every entry point needs a GPU.
#include "../../include/fem_hip.h"

#include <cstring>  // before rocprim: its headers use memcpy unqualified
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>
#include <rccl/rccl.h>
#include <sched.h>
#if defined(__x86_64__)
#include <immintrin.h>
#endif

#include <algorithm>
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <functional>
#include <memory>
#include <atomic>
#include <chrono>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "fem_buf.hip.h"
#include "fem_index_build.hip.h"
#include "fem_pack.h"
#include "fem_kernels.hip.h"
#include "fem_verify.hip.h"
#include "fem_seed_fast.hip.h"
#include "fem_seed_join.hip.h"
#include "fem_tail.hip.h"
#include "fem_bgzf.hip.h"
#include "fem_trim.hip.h"
#include "fem_adapter.hip.h"
#include "fem_overlap.hip.h"
#include "fem_coverage.h"

namespace {

using femb::Buf;
using femb::Event;
using femb::PinBuf;
using femb::Stream;
// A slot's staging buffers grow by half at least, so that batches of slowly rising size do not re-allocate each time
template <typename T>
using StageBuf = femb::Buf<T, femb::Mem::Device, femb::Grow::Half>;
template <typename T>
using PinStageBuf = femb::Buf<T, femb::Mem::Pinned, femb::Grow::Half>;

#ifndef FEM_SLOTS
#define FEM_SLOTS 4
#endif
constexpr int kSlots = FEM_SLOTS;
constexpr uint32_t kMaxReadLen = 1024;
constexpr size_t kFrontPad = 16;  // kernels fetch a reverse-strand chunk from up to 15 bytes in front of a read
constexpr size_t kPackedFrontPad = 256;  // ... and verify_kernel_packed up to 16 bytes in front of a read's codes (a multiple of hipMalloc's alignment)
constexpr uint64_t kExpandAllShare = 8;  // a packed batch with more exceptions than one per this many reads is expanded whole at commit
constexpr uint32_t kXcapSmall = 512, kFcap = 128, kCcap = 128;

constexpr int kTimedKernels = 20;  // fem_dev_kernel_time ids: 19 the trim stage (fem_dev_set_trim, fem_dev_set_adapter, fem_dev_set_pair_overlap: adapter_match_kernel, pair_overlap_kernel, clip points, scan, gather); else 0 seed (join), 1 verify, 2 generic seed, 3-5 tail, 6 pack_results_kernel (round 5; the count kernel of rounds 1-2 before), 7 SAM text, 8 seed selection, 9 pairing, 10 mate rescue, 11 BAM records, 12 BGZF, 13 MAPQ, 14 the line index with unmapped reads, 15 the line filter's line index, 16 the insert estimate, 17 the mate tags' score kernel, 18 the fold index (XA:Z); 3-5, 7, 9-11, 13-15, 17 and 18 are stages of the device tail (kTailStages), 16 is one too (fem_dev_estimate_insert counts it itself)
struct TimedLaunch {
  int kernel;
  hipEvent_t start, stop;
  bool counts = true;  // false: a further part of a launch that is already counted (a batch mapped in parts, launch_batch)
};
constexpr int kMaxParts = 4;

// The trim stage in front of the selection (enqueue_trim) has CUT PRODUCERS: a kernel each that writes a
// uint16 cut per read and two counters.  A kind is a row here (its setter and what a batch mapped without it lacks, as the
// refusals word them), a Cuts in the slot and a member of PrepSettings.  kTrim is the stage's last step, which takes the others'
// cuts in and makes the batch's clip points: it has two arrays (clip5, clip3) and runs for every trimmed batch.
enum CutKind { kTrim, kAdapter, kOverlap, kCutKinds };
constexpr struct {
  const char *setter, *what;
} kCutRows[kCutKinds] = {{"fem_dev_set_trim", "trimming"}, {"fem_dev_set_adapter", "an adapter"}, {"fem_dev_set_pair_overlap", "the mates' overlap"}};

// What the three setters made of a slot's trim stage
struct PrepSettings {
  fem_trim_params trim{0, 0, 0};
  struct Adapter {  // as the kernel takes it
    bool on = false;
    uint64_t occ[2][4] = {};
    int32_t len[2] = {0, 0}, min_overlap = 0, err_pct = 0;
  } adapter;
  struct PairOverlap {
    bool on = false;
    int32_t min_overlap = 0, err_pct = 0;
  } overlap;
  // a batch mapped under these settings is a TRIMMED batch: staged as characters, with clip points and a mapping view
  bool any() const { return trim.trim5 > 0 || trim.trim3 > 0 || trim.qual > 0 || adapter.on || overlap.on; }
  bool has(int kind) const { return kind == kAdapter ? adapter.on : kind == kOverlap ? overlap.on : any(); }
};

// A producer's cuts of the slot's mapped batch and its two counters: on the device, the counters pinned on the host behind the
// stage, the arrays from the batch's first fetch on.
struct Cuts {
  int n_arrays = 1;
  StageBuf<uint16_t> d[2];
  PinStageBuf<uint16_t> h[2];
  Buf<unsigned long long> d_ctr;
  PinBuf<unsigned long long> h_ctr;
  bool home = false;  // h holds the mapped batch's cuts
  hipError_t size(size_t n) {
    hipError_t e = hipSuccess;
    for (int k = 0; k < n_arrays && e == hipSuccess; ++k) e = d[k].ensure(std::max<size_t>(n, 1));
    if (e == hipSuccess) e = d_ctr.ensure(2);
    return e == hipSuccess ? h_ctr.ensure(2) : e;
  }
  hipError_t zero_counts(hipStream_t st) { return hipMemsetAsync(d_ctr, 0, 2 * sizeof(unsigned long long), st); }
  hipError_t counts_home(hipStream_t st) { return hipMemcpyAsync(h_ctr, d_ctr, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st); }
  // the arrays of n reads in h, copied once per batch (the host waits for the stream)
  hipError_t fetch(size_t n, hipStream_t st) {
    if (home) return hipSuccess;
    hipError_t e = hipSuccess;
    for (int k = 0; k < n_arrays && e == hipSuccess; ++k) e = h[k].ensure(std::max<size_t>(n, 1));
    for (int k = 0; k < n_arrays && n && e == hipSuccess; ++k) e = hipMemcpyAsync(h[k], d[k], n * sizeof(uint16_t), hipMemcpyDeviceToHost, st);
    if (n && e == hipSuccess) e = hipStreamSynchronize(st);
    home = e == hipSuccess;
    return e;
  }
};

struct Slot {
  Stream stream;
  // inputs
  StageBuf<uint8_t> d_bases_alloc;  // kFrontPad bytes of padding, then the batch's characters, then 64 bytes of slack
  uint8_t *bases() const { return d_bases_alloc + 16; }
  StageBuf<uint64_t> d_off;
  uint64_t n_reads = 0;
  uint64_t n_bases = 0;
  uint32_t max_len = 0;
  bool staged = false;
  // pinned host staging lent to the parser (fem_dev_acquire_stage)
  PinStageBuf<char> h_bases;
  PinStageBuf<uint64_t> h_off;
  uint64_t acq_reads = 0, acq_bases = 0;  // what the last fem_dev_acquire_stage asked for
  // qualities and names for the device SAM text (fem_dev_acquire_text_stage / fem_dev_fetch_sam): pinned staging + copies in HBM
  PinStageBuf<char> h_quals, h_names;
  PinStageBuf<uint64_t> h_name_off;
  StageBuf<uint8_t> d_quals, d_names;
  StageBuf<uint64_t> d_name_off;
  bool text_staged = false;
  bool host_quals = false;             // the batch's qualities stayed on the host (fem_dev_commit_names_stage): the text leaves their field open
  const uint64_t *qual_at = nullptr;   // ... and where each read's field starts in the slot's last text (pinned, the tail's)
  Stream text_stream;   // qualities and names go to the device beside the batch's kernels, not in front of them
  Stream out_stream;    // the batch's way out (mapping tail, SAM text, its copy home): HIGH priority, see out_stream_of
  Event ev_text_staged; // ... and have arrived (the SAM text's kernels wait for it)
  Event ev_text_order;  // the slot's last SAM text has been rendered (its kernels read the same arrays)
  bool have_text_order = false;
  StageBuf<uint8_t> d_packed_alloc;      // packed transfer (fem_dev_stage_reads): kPackedFrontPad bytes of padding, 2-bit codes + positions of other characters, 64 bytes of slack
  uint8_t *packed() const { return d_packed_alloc + kPackedFrontPad; }
  StageBuf<uint32_t> d_exc_bits;         // ... bit r: read r has such a character (the device tail reads the others' bases from d_packed)
  uint32_t packed_bpr = 0;
  // fem_dev_fetch callers get the result arrays sent home behind the kernels, without the host waiting for the batch first:
  // the per-read arrays whole, the per-candidate arrays up to what the slot's previous batch needed (the rest at fetch)
  bool prefetch_results = false, staged_by_copy = false;
  uint64_t prefetched_reads2 = 0, prefetched_cand = 0, last_n_cand = 0;
  uint64_t h2d_bytes = 0;                 // what the last staging sent over the link
  bool sent_packed = false;
  // A packed batch's characters (bases(), d_off) are made when something asks for them (ensure_chars); until then only the
  // reads marked in d_exc_bits have theirs.  select_packed: the slot's last dense mapping read the codes in seed_select_kernel.
  bool chars_ready = true, offs_ready = true, select_packed = false;  // (offs_ready: d_off alone is filled, see enqueue_packed)
  uint64_t n_exc = 0;   // exceptions of the packed batch (their positions and bytes lie behind its codes in packed())
  Event ev_chars;       // the expansion on the slot's stream is done (a tail on another stream waits for it)
  // A batch committed to an IDLE device is sent and mapped in `parts` pieces (reads [part_begin[q], part_begin[q + 1])), so that
  // the join of its first piece starts after a quarter of the copy and a quarter of the selection (launch_batch): the fill of
  // the pipeline.  ev_part[q]: piece q's characters are in HBM; ev_sel[q]: its selection is done.
  int parts = 1;
  uint32_t part_begin[kMaxParts + 1] = {0, 0, 0, 0, 0};
  Event ev_part[kMaxParts], ev_sel[kMaxParts];
  Event ev_zeroed;
  Event ev_results;  // the batch's results are final on the device
  // outputs on the device
  // (arrays that share a capacity are allocated together, femb::alloc_all: all of them hold it or none holds anything)
  Buf<uint64_t> d_cand;
  Buf<uint32_t> d_meta;
  Buf<uint8_t> d_ed;
  Buf<int16_t> d_end;
  uint32_t cand_cap = 0;  // published once all four exist
  Buf<uint32_t> d_begin, d_count, d_nmap;  // 2, 2 and 1 entries per read
  // counters, flags and work cursors (CtlBlock)
  Buf<uint8_t> d_ctl;
  PinBuf<uint8_t> h_ctl;  // pinned mirror of its head
  Buf<uint64_t> d_arena;
  uint64_t arena_cap = 0;
  Buf<uint32_t> d_slow;  // reads the fast seed kernel leaves to the generic one
  uint32_t slow_cap = 0;
  // dense indexes: what seed_select_kernel hands seed_join_kernel (6 R selected seeds + one header per read)
  StageBuf<uint2> d_sel, d_sel_hdr;
  // pinned host results
  PinBuf<uint32_t> h_begin, h_count;
  PinBuf<uint64_t> h_cand;
  PinBuf<uint8_t> h_ed;
  PinBuf<int16_t> h_end;
  // the outcome in the form that crosses the link (fem_dev_fetch_packed; pack_results_kernel): on the device, pinned on the host
  StageBuf<uint8_t> d_count8;
  StageBuf<uint32_t> d_seg;
  Buf<uint64_t> d_pcand;
  Buf<uint8_t> d_ped;
  Buf<int16_t> d_pend;
  Buf<uint2> d_big;
  PinBuf<uint8_t> h_count8, h_ped;
  PinBuf<uint32_t> h_seg;
  PinBuf<uint64_t> h_pcand;
  PinBuf<int16_t> h_pend;
  PinBuf<uint2> h_big;
  bool want_packed = false;    // the slot's last fetch was fem_dev_fetch_packed: launch_batch packs and sends home behind the kernels
  bool packed_enqueued = false;  // pack_results_kernel ran (or is queued) for the slot's current batch
  uint64_t packed_home = 0, last_n_packed = 0;  // packed candidates copied home behind the kernels / of the slot's previous batch
  bool packed_per_read_home = false;
  uint32_t n_packed = 0, n_big = 0;
  // state of the last launch
  fem_params params{};
  bool mapped = false, synced = false;
  bool covered = false;  // the slot's mapped batch has been added to the coverage track (its first text or BAM fetch does that)
  uint64_t stats[5] = {0, 0, 0, 0, 0};
  uint32_t n_cand = 0;
  std::vector<TimedLaunch> pending;
  std::unique_ptr<femt::Tail> tail;  // device mapping tail (fem_dev_fetch_records), created on first use
  // what the fem_dev_set_* functions made of the slot's SAM text and BAM records (opt.paired, fem_dev_set_pairs: the batches
  // are read pairs, read i and read n_reads / 2 + i), and what its last text, BAM or fetch_pairs counted (fem_dev_*_count)
  femt::LineOptions opt;
  femt::LineCounts counts;
  // fem_dev_fetch_pairs: the records in output order (host copies, valid until the slot's next fetch_pairs)
  std::vector<uint16_t> pr_flag;
  std::vector<uint32_t> pr_tid, pr_pos0, pr_cigar_off, pr_cigar, pr_md_off;
  std::vector<uint8_t> pr_nm;
  std::vector<char> pr_md;
  // The trim stage (enqueue_trim): what fem_dev_set_trim, fem_dev_set_adapter and fem_dev_set_pair_overlap wrote, what the slot's
  // mapped batch was made with (taken at fem_dev_map_staged), that batch's cuts and counters per producer (cuts[kTrim]: the clip
  // points clip5 and clip3), and its MAPPING VIEW: the kept parts' characters and offsets, which the mapping kernels, the
  // traceback and the rescue read in place of bases() / d_off (those stay the whole reads, for SEQ and QUAL of the text)
  PrepSettings prep, prep_batch;
  Cuts cuts[kCutKinds] = {{2}, {}, {}};
  struct MapView {
    bool trimmed = false;              // the mapped batch is a trimmed batch: it has this view and clip points
    StageBuf<uint8_t> d_bases_alloc;   // laid out as the slot's d_bases_alloc
    StageBuf<uint64_t> d_off, d_keep;  // the kept lengths and their scan
    Buf<uint8_t> d_scan_tmp;
  } view;
  const uint8_t *map_bases() const { return view.trimmed ? view.d_bases_alloc + 16 : bases(); }
  const uint64_t *map_off() const { return view.trimmed ? view.d_off.get() : d_off.get(); }
};

// A slot's control block as it lies in d_ctl (kCtlAlloc bytes, zeroed whole in front of every launch of a batch); its first
// kCtlBytes go home into h_ctl behind the batch's kernels.  The kernels get plain pointers to its members.
struct CtlBlock {
  uint32_t ctr[4];
  unsigned long long arena_ctr[2];
  unsigned long long stats[4];
  uint32_t pack_cursor[2];  // pack_results_kernel: packed candidates, big[] entries
  // ... and, in cache lines of their own behind them, the work cursors: a pair per part of a batch mapped in parts
  struct Work {
    alignas(64) uint32_t select;  // seed_select_kernel; part 0's is seed_fast_kernel's too
    alignas(64) uint32_t join;    // seed_join_kernel
  } work[kMaxParts];
};
constexpr size_t kCtlPackCursor = offsetof(CtlBlock, pack_cursor);
constexpr size_t kCtlBytes = kCtlPackCursor + sizeof(CtlBlock::pack_cursor);
constexpr uint32_t kBigCap = 4096;  // strands with 255 candidates and more that a packed result lists (beyond: fetch the plain form)
constexpr size_t kCtlWorkCursor = offsetof(CtlBlock, work), kCtlWorkCursor2 = kCtlWorkCursor + offsetof(CtlBlock::Work, join);
constexpr size_t kCtlPartStride = sizeof(CtlBlock::Work), kCtlAlloc = 1024;
static_assert(kCtlWorkCursor2 + (kMaxParts - 1) * kCtlPartStride + 64 <= kCtlAlloc, "control block layout");
static_assert(kCtlBytes <= kCtlWorkCursor, "control block layout");
static_assert(offsetof(CtlBlock, arena_ctr) == 16 && offsetof(CtlBlock, stats) == 32 && kCtlPackCursor == 64 && kCtlBytes == 72, "control block layout");
static_assert(kCtlWorkCursor == 128 && kCtlWorkCursor2 == 192 && kCtlPartStride == 128 && sizeof(CtlBlock) <= kCtlAlloc, "control block layout");
// (the device's block: for the addresses of its members only, the host never reads through it; the mirror: its first kCtlBytes)
CtlBlock *ctl_of(const Slot &s) { return (CtlBlock *)s.d_ctl.get(); }
const CtlBlock *ctl_home(const Slot &s) { return (const CtlBlock *)s.h_ctl.get(); }

}  // namespace

namespace {
// The host threads of fem_dev_stage_reads: created once per handle and parked between batches (a batch every few ms:
// starting and joining a dozen threads per batch cost more than the packing gained, and under a cgroup CPU quota the
// short-lived threads, scattered over the machine's CPUs, had the whole process throttled now and then).
class StagePool {
 public:
  ~StagePool() {
    {
      std::lock_guard<std::mutex> l(m_);
      stop_ = true;
    }
    cv_.notify_all();
    for (auto &t : threads_) t.join();
  }
  // work(t) for t in [0, n): t = 0 on the calling thread, the rest on the pool
  void run(unsigned n, const std::function<void(unsigned)> &work) {
    if (n <= 1) return work(0u);
    {
      std::lock_guard<std::mutex> l(m_);
      while (threads_.size() + 1 < n) {
        const unsigned id = (unsigned)threads_.size() + 1;
        threads_.emplace_back([this, id] { loop(id); });
      }
      work_ = &work, n_ = n, pending_ = n - 1, ++epoch_;
    }
    cv_.notify_all();
    work(0u);
    std::unique_lock<std::mutex> l(m_);
    done_.wait(l, [&] { return pending_ == 0; });
    work_ = nullptr;
  }

 private:
  void loop(unsigned id) {
    uint64_t seen = 0;
    for (;;) {
      const std::function<void(unsigned)> *w = nullptr;
      {
        std::unique_lock<std::mutex> l(m_);
        cv_.wait(l, [&] { return stop_ || (epoch_ != seen && id < n_); });
        if (stop_) return;
        seen = epoch_, w = work_;
      }
      (*w)(id);
      std::lock_guard<std::mutex> l(m_);
      if (--pending_ == 0) done_.notify_one();
    }
  }
  std::mutex m_;
  std::condition_variable cv_, done_;
  std::vector<std::thread> threads_;
  const std::function<void(unsigned)> *work_ = nullptr;
  unsigned n_ = 0, pending_ = 0;
  uint64_t epoch_ = 0;
  bool stop_ = false;
};
}  // namespace

struct fem_dev {
  // Calls on DIFFERENT slots of one handle may come from different threads (round 5: `FEM map` retires its batches in flight on
  // a thread each, so that one batch's host round trips — records counted, text sized — do not hold up the next one's): what
  // the slots share (the kernels' chaining events, the event pool, the timing sums, the error string) is touched under this
  // lock; a thread waiting for the device does not hold it.
  femt::TextGate text_gate;  // one SAM text on its way to the host at a time (fem_tail.hip.h)
  // fem_dev_bgzf_compress: its compressor, input buffer and stream
  std::unique_ptr<femz::Bgzf> bgzf;
  Buf<uint8_t> d_zin;
  Stream z_stream;
  std::recursive_mutex mu;
  int device = 0;
  std::unique_ptr<StagePool> stage_pool;  // host threads of fem_dev_stage_reads
  Buf<uint8_t> d_ref_names;   // reference sequence names for the device SAM text
  Buf<uint32_t> d_ref_name_off;
  int n_cu = 256;
  std::string err;
  // index
  Buf<uint32_t> d_lookup;
  uint64_t n_lookup = 0;
  Buf<uint64_t> d_occ;
  uint64_t n_occ = 0;
  int32_t k = 0, step = 0;
  Buf<uint32_t> d_summary;  // bucket summaries (femk::SeedParams::summary), built for sparse indexes only
  // dense indexes: occurrence table in 32-bit global coordinates + its sequence tables (fem_seed_dense.hip.h)
  Buf<uint32_t> d_occ32, d_goff, d_blkseq;
  uint32_t list_shift = 0;        // != 0: d_occ32 is the strided table (bucket h at h << list_shift, fem_seed_dense.hip.h); 0: compact
  bool no_strided = false;        // FEM_NO_STRIDED=1: keep the compact 32-bit table (test hook / A-B)
  bool select_chars = false;      // FEM_SELECT_CHARS=1: packed batches are expanded at commit and selected from characters (test hook / A-B)
  bool verify_chars = false;      // FEM_VERIFY_CHARS=1: verify_kernel (characters) on packed batches too (test hook / A-B)
  Buf<uint32_t> d_freq11;  // saturated byte frequencies per 11-mer (fem_seed_select.hip.h), 64 MiB
  // banks of sequences, each with 32-bit coordinates of its own (fem_seed_dense.hip.h); 1 = the whole reference in one
  uint32_t n_banks = 1, bank_first[5] = {0, 0, 0, 0, 0};
  Buf<uint32_t> d_bank_lo;  // [n_banks - 1][n_buckets]: where each further bank's part of a bucket's list starts
  uint64_t bank_limit = 0;        // FEM_TEST_BANK_BASES: coordinates per bank (tests: banks on small references); 0 = kDenseLimit
  uint32_t bank_seqs = 0;         // FEM_TEST_BANK_SEQS: sequences per bank (tests); 0 = kDenseMaxSeq
  // reference
  // bit q of the codes, one bit per base (verify_kernel's windows); [3]: the uploaded character is not one of "ACGTN"
  Buf<uint8_t> d_planes;  // femk::plane_window
  Buf<uint8_t> d_ref_raw;  // the characters as uploaded (the traceback and MD compare and print them)
  uint64_t ref_bytes = 0;
  Buf<uint64_t> d_seq_off;
  Buf<uint32_t> d_seq_len;
  uint32_t n_seq = 0;
  std::vector<uint64_t> seq_off;
  std::vector<uint32_t> seq_len;
  // the coverage track (fem_dev_set_coverage): the setting, the windows' layout (host and device) and the bins, which every slot's
  // first text of a batch adds to (Slot::covered) and which stay until the setting changes
  struct Coverage {
    bool on = false;
    fem_coverage_params set{0, 0, 0};
    uint64_t n_bins = 0;
    std::vector<uint64_t> bin_off;  // n_seq + 1
    Buf<uint64_t> d_bin_off;
    Buf<unsigned long long> d_bins;
  } coverage;
  Slot slot[kSlots];
  bool timing = false;
  // blocks of a kernel that a CU holds at a time, as the runtime answered once per (kernel, block threads, LDS bytes): resident_blocks
  struct Residency { const void *kernel; uint32_t threads, lds; int blocks; };
  std::vector<Residency> residency;
  double t_ms[kTimedKernels] = {};
  uint64_t t_n[kTimedKernels] = {};
  bool force_generic = false;  // FEM_FORCE_GENERIC=1: skip the fast seed kernel (test hook)
  bool force_hash = false;     // FEM_FORCE_HASH=1: always use the hash-join form of the fast kernel (test hook)
  bool force_dense = false;    // FEM_FORCE_DENSE=1: build the 32-bit tables and run seed_select_kernel + seed_join_kernel whatever the index density (test hook)
  bool no_dense = false;       // FEM_NO_DENSE=1: never take the dense-index path (measurement / A-B hook)
  bool tiny_buffers = false;   // FEM_TEST_TINY_BUFFERS=1: start every scratch buffer tiny so the grow + re-run paths run (test hook)
  femb::EventPool event_pool;
  // The slots' streams overlap copies with kernels, but the kernels of different batches run one after the other
  // (each batch's first kernel waits for the previous batch's last): two batches' seed kernels side by side only
  // evict each other's index lines, and per-kernel event times stay those of a kernel that has the chip to itself.
  Event ev_kernels_done;
  bool have_kernels_done = false;
  // Dense indexes: seed_select_kernel of batch i + 1 runs BESIDE batch i's seed_join_kernel (it is bound by the rate of
  // table sectors the fabric delivers and needs four waves per CU for that; the join is bound by instruction issue):
  // selections are chained among themselves, and a batch's join waits for its own selection and the previous batch's
  // kernels.  FEM_NO_OVERLAP=1: one after the other (measurement hook).
  Event ev_select_done;
  bool have_select_done = false;
  bool no_overlap = false;
  // The batches' H2D copies go one after the other (each waits for the previous one's): four batches committed at once —
  // the start of every job — used to share the link, and the first one's kernels started when all four had arrived.
  Event ev_h2d_done;
  bool have_h2d_done = false;
  Stream side_stream;  // the selections of a batch mapped in parts (beside the joins on the slot's stream)
  bool no_parts = false;              // FEM_NO_PARTS=1 (measurement hook)
  int max_parts = 2;                  // parts of a batch that meets an idle device (FEM_PARTS, measurement hook): two halves —
                                      // every further launch of the join costs ~0.35 ms of ramp and tail, what a finer first part saves
  // FEM_TIMELINE=1 (with FEM_TESTING=1 and timing on): every timed launch and copy is printed with its start and end in ms since
  // the last fem_dev_reset_timing — the pipeline's fill and drain made visible (ids >= kTimedKernels: 20 H2D + unpack, 21 D2H)
  bool timeline = false, have_epoch = false;
  Event ev_epoch;
};

namespace {

// Test / measurement switches of the library are read only when FEM_TESTING=1 (tests/conftest.py sets it): a production
// process does not steer kernels through its environment.
bool testing_switch(const char *name) {
  const char *t = getenv("FEM_TESTING");  // (read every time: a process may open a plain handle first and a test handle later)
  if (!(t && t[0] == '1')) return false;
  const char *v = getenv(name);
  return v && v[0] == '1';
}

int fail(fem_dev *h, int rc, const std::string &msg) {
  if (h) {
    std::lock_guard<std::recursive_mutex> lock(h->mu);
    h->err = msg;
  }
  return rc;
}
#define FEM_LOCK(h) std::lock_guard<std::recursive_mutex> fem_lock_(h->mu)

#define HIP_TRY(h, expr)                                                                          \
  do {                                                                                            \
    hipError_t e_ = (expr);                                                                       \
    if (e_ != hipSuccess)                                                                         \
      return fail(h, e_ == hipErrorOutOfMemory ? FEM_ERR_NOMEM : FEM_ERR_HIP,                     \
                  std::string(#expr) + ": " + hipGetErrorString(e_));                             \
  } while (0)

bool params_ok(const fem_params *p) {
  return p && p->k >= 1 && p->k <= 15 && p->step >= 1 && p->step <= 16 && p->e >= 0 && p->e <= 7 && p->a >= 0 &&
         p->a <= 2;
}

// LDS carve-up of one wave for reads up to max_len (see femk::SeedLayout)
femk::SeedLayout make_layout(const fem_params &p, uint32_t max_len) {
  femk::SeedLayout l{};
  const uint32_t R = (uint32_t)(p.e + 1 + p.a);
  const uint32_t lg = (uint32_t)(p.k / p.step + (p.k % p.step ? 1 : 0));
  const uint32_t n_groups = 2u * (uint32_t)p.step;
  uint32_t smax = max_len >= (uint32_t)p.k ? max_len - (uint32_t)p.k + 1u : 1u;
  int c = (int)(smax / (uint32_t)p.step) - (int)(R * lg) + 2;
  uint32_t cmax = (uint32_t)std::max(c, 2);
  l.smax = smax;
  l.cmax = cmax;
  l.cw = (cmax + 31u) / 32u;
  l.n_words = (max_len + 15u) / 16u + 2u;
  l.xcap = kXcapSmall, l.fcap = kFcap, l.ccap = kCcap;
  uint32_t o = 0;
  auto take = [&](uint32_t bytes) {
    uint32_t at = o;
    o += (bytes + 15u) & ~15u;
    return at;
  };
  l.pkw = take(l.n_words * 4u);
  l.nkw = take(l.n_words * 4u);
  l.sf = take(2u * smax * 8u);
  l.dp_rows = take(n_groups * 2u * cmax * 4u);
  l.dp_bits = take(std::max(n_groups * R * l.cw * 4u, n_groups * R * 8u));  // serial form: bit rows; DPP form: one ballot per row
  l.picked = take(n_groups * R * 16u);
  l.rb = take(2u * (R + 1u) * 4u);
  l.X = take(l.xcap * 8u);
  l.F = take(l.fcap * 8u);
  l.A = take(l.ccap * 8u);
  l.B = take(l.ccap * 8u);
  l.wave_bytes = o;
  return l;
}

// LDS of one wave of seed_fast_kernel: packed bases, (lookup, frequency) per seed, DP take bits, selected seeds, scatter
femk::SeedLayout make_layout_fast(const fem_params &p, uint32_t max_len, bool hash) {
  femk::SeedLayout l{};
  const uint32_t R = (uint32_t)(p.e + 1 + p.a);
  const uint32_t n_groups = 2u * (uint32_t)p.step;
  l.smax = max_len >= (uint32_t)p.k ? max_len - (uint32_t)p.k + 1u : 1u;
  l.n_words = (max_len + 15u) / 16u + 2u;
  l.xcap = 64;
  uint32_t o = 0;
  auto take = [&](uint32_t bytes) {
    uint32_t at = o;
    o += (bytes + 15u) & ~15u;
    return at;
  };
  if (hash) {  // (the lean form encodes a block of reads at once: strm)
    l.pkw = take(l.n_words * 4u);
    l.nkw = take(l.n_words * 4u);
  }
  // (hash, frequency) of every seed of both strands, reused for the strands' candidates once the seeds are selected
  // — hash-join form only: the lean form looks its seeds up straight into the group queue
  if (hash) l.sf = take(std::max(2u * l.smax * 8u, 2u * 64u * 8u));
  l.dp_bits = take(std::max(n_groups, femk::kGroupQueue) * R * 8u);  // one ballot per (pass, row); up to kGroupQueue passes
  if (hash) {
    l.X = take(64u * 8u);                 // scatter
    l.A = take(femk::kListScratchBytes);  // lists_in_lanes
  }  // (lean form: no per-read list phase; flush_small lays its scratch over the group queue, dead by then)
  l.B = take(2u * femk::kReadBlock * 8u);  // the block's begin/count entries
  if (!hash) {
    // One block of reads (kReadBlock consecutive ones, contiguous in the batch) is staged and encoded at once; blocks
    // longer than this many characters (reads over 256 bases among them) go to the generic kernel.
    const uint32_t blk_chars = femk::kReadBlock * std::min(max_len, 256u);
    l.strm_words = blk_chars / 16u + 3u;
    l.strm = take(3u * l.strm_words * 4u);
    const uint32_t q_at = o;
    l.F = take(femk::kQueueBytes);  // queue of small reads' seeds
    // queue of live phase groups: a read may add all six of its groups, each with G - Lg + 1 words
    const uint32_t g0 = l.smax / (uint32_t)femk::kStep;
    const uint32_t n_used = g0 > (uint32_t)femk::kLg ? g0 - (uint32_t)femk::kLg + 1u : 1u;
    l.gq_cap = std::max(384u, n_groups * n_used);
    l.gq = take(std::max(l.gq_cap * 4u + femk::kGroupQueue * 16u + 2u * 32u * 4u, femk::kFlushScratchBytes));
    // the block's raw characters (+ slack for the 16-byte copies) are dead once the streams exist, and both queues
    // are empty at that point: they share the space
    l.blk_bytes = blk_chars + 32u;
    l.blk = q_at;
    if (o < q_at + l.blk_bytes) take(q_at + l.blk_bytes - o);
  }
  if (hash) {              // hash-join form: open-addressing table; xcap = most occurrences one group may select
    l.xcap = (uint32_t)femk::bloom_chunks((int)R) * 64u;
    l.F = take(femk::bloom_slots((int)R) / 16u * 4u);  // bitmap: two bits per key slot
  }
  l.wave_bytes = o;
  return l;
}

// LDS of one wave of seed_select_kernel (fem_seed_select.hip.h): the block's read offsets, the sub-block's two 2-bit
// streams, one frequency byte per seed, strand and phase group, the per-read words.  The reads of a block are worked
// on `nb` at a time, as many as a budget of 3 KB of 16-bit frequencies holds (a block of four waves then stays within the
// 16 KB that six blocks of the join leave of a CU's LDS) (the kernel runs beside seed_join_kernel, whose
// bitmaps want the LDS).
femk::SeedLayout make_layout_select(const fem_params &p, uint32_t max_len, bool packed) {
  femk::SeedLayout l{};
  const uint32_t R = (uint32_t)(p.e + 1 + p.a);
  l.smax = max_len >= (uint32_t)p.k ? max_len - (uint32_t)p.k + 1u : 1u;
  // a phase group's DP takes at most kSelMaxCols columns: groups of more than kSelMaxCols - 1 + 4 R seeds go to the generic kernel
  const uint32_t g_max = std::min<uint32_t>((l.smax + 2u) / 3u, femk::kSelMaxCols - 1u + 4u * R);
  // one array of 16-bit frequencies per strand, in seed order (group g's seed c at 3 c + g): even, and an odd number of
  // 32-bit words, so that the rows of the DP's lanes spread over the LDS banks
  l.gstride = 3u * g_max + 2u;
  l.gstride += l.gstride & 1u;
  if (!((l.gstride >> 1) & 1u)) l.gstride += 2u;
  l.nb = std::max<uint32_t>(1u, std::min<uint32_t>(femk::kReadBlock, 3100u / (2u * 2u * l.gstride)));
  // (a packed batch's reads lie in the stream as they came, each padded to a whole byte = four bases: up to three words more
  //  per stream where the length is no multiple of four; a batch of characters keeps the layout it had)
  l.strm_words = (l.nb * (packed ? (max_len + 3u) & ~3u : max_len) + 15u) / 16u + 2u;
  uint32_t o = 0;
  auto take = [&](uint32_t bytes) {
    uint32_t at = o;
    o += (bytes + 15u) & ~15u;
    return at;
  };
  l.rb = take((femk::kReadBlock + 2u) * 8u);
  l.rinfo = take(4u * femk::kReadBlock * 4u);
  l.strm = take(2u * l.strm_words * 4u);
  l.fq = take(l.nb * 2u * l.gstride * 2u + 256u);  // (+ what an idle lane of the last strand reads past its array)
  l.wave_bytes = o;
  return l;
}

// LDS of one wave of seed_join_kernel: the strands' candidates, flagged values per phase group, scatter, the block's
// begin/count entries, the sequence table, the join's bitmap
femk::SeedLayout make_layout_join(const fem_params &p, bool banked, bool padded = false) {
  femk::SeedLayout l{};
  const uint32_t R = (uint32_t)(p.e + 1 + p.a);
  uint32_t o = 0;
  auto take = [&](uint32_t bytes) {
    uint32_t at = o;
    o += (bytes + 15u) & ~15u;
    return at;
  };
  l.sf = take(2u * 64u * 4u);
  l.X = take(64u * 4u);
  l.A = take(3u * (femk::dense_flag_cap((int)R) + 1u) * 4u);
  l.B = take(2u * femk::kReadBlock * 8u);
  l.F = take(femk::join_bitmap_words((int)R, padded) * 4u);
  if (banked) l.gq = take(2u * 64u * 8u);  // a strand's candidates of bank after bank (seed_join_body<R, true>)
  l.wave_bytes = o;
  l.picked = 0;  // the block's sequence table: set by the launcher (behind the waves' regions)
  return l;
}

// The handle has the 32-bit occurrence table and the 11-mer frequencies of a dense index (refresh_dense)
bool has_dense_tables(const fem_dev *h) { return h->d_occ32 && h->d_freq11; }

// Which seed kernels map a batch of given parameters on this handle: seed_filter_kernel over every read (generic), or, in
// front of it, seed_fast_kernel in one of its two forms, or seed_select_kernel and seed_join_kernel on one of the three forms
// of a dense index's table.  launch_batch, fem_dev_seed_kernel and fem_dev_reserve_batch all follow this one decision.
struct SeedPath {
  enum Kind { kGeneric, kFastLean, kFastHash, kDenseCompact, kDenseBanked, kDenseStrided } kind;
  int R;  // e + 1 + a, the seeds selected per phase group
  bool dense() const { return kind >= kDenseCompact; }
  bool fast() const { return kind == kFastLean || kind == kFastHash; }
  bool banked() const { return kind == kDenseBanked; }
};
SeedPath seed_path(const fem_dev *h, const fem_params &p) {
  const int R = p.e + 1 + p.a;
  // the fast and the dense kernels are compiled for one seed length and step and for R up to kMaxR
  if (!(p.k == femk::kK && p.step == femk::kStep && R >= 1 && R <= femk::kMaxR && !h->force_generic)) return {SeedPath::kGeneric, R};
  if (has_dense_tables(h)) return {h->n_banks > 1 ? SeedPath::kDenseBanked : h->list_shift ? SeedPath::kDenseStrided : SeedPath::kDenseCompact, R};
  // long occurrence lists: the hash-join form of the fast kernel; short ones: lists in lanes only
  return {h->force_hash || (double)h->n_occ > (double)h->n_lookup ? SeedPath::kFastHash : SeedPath::kFastLean, R};
}

typedef void (*SeedKernel)(femk::SeedParams);
template <size_t... I>
SeedKernel select_kernel_of(int R, bool banked, bool packed, std::index_sequence<I...>) {
  static const SeedKernel k[2][2][femk::kMaxR] = {
      {{femk::seed_select_kernel<(int)I + 1, false, false>...}, {femk::seed_select_kernel<(int)I + 1, true, false>...}},
      {{femk::seed_select_kernel<(int)I + 1, false, true>...}, {femk::seed_select_kernel<(int)I + 1, true, true>...}}};
  return k[packed][banked][std::min(std::max(R, 1), femk::kMaxR) - 1];
}
template <size_t... I>
SeedKernel fast_kernel_of(int R, bool hash, std::index_sequence<I...>) {
  static const SeedKernel k[2][femk::kMaxR] = {{femk::seed_fast_kernel<(int)I + 1, false>...}, {femk::seed_fast_kernel<(int)I + 1, true>...}};
  return k[hash][std::min(std::max(R, 1), femk::kMaxR) - 1];
}
// (`banked`: the reference's sequences lie in more than one coordinate space, fem_seed_dense.hip.h; `packed`: the batch's
//  2-bit codes are read, SeedParams::packed, not its characters)
SeedKernel select_kernel(int R, bool banked, bool packed) { return select_kernel_of(R, banked, packed, std::make_index_sequence<femk::kMaxR>{}); }
// (`hash`: the hash-join form for long occurrence lists; otherwise the lean one, lists in lanes only)
SeedKernel fast_kernel(int R, bool hash) { return fast_kernel_of(R, hash, std::make_index_sequence<femk::kMaxR>{}); }
// (the dense kinds in SeedPath's order: the compact table, references in banks (compact, cut at bank_lo), the strided table with its pads)
SeedKernel join_kernel(SeedPath path) {
  const int R = path.R, which = path.kind - SeedPath::kDenseCompact;
  static const SeedKernel k[3][femk::kMaxR] = {
      {femk::seed_join_kernel_r1, femk::seed_join_kernel_r2, femk::seed_join_kernel_r3, femk::seed_join_kernel_r4, femk::seed_join_kernel_r5,
       femk::seed_join_kernel_r6, femk::seed_join_kernel_r7, femk::seed_join_kernel_r8, femk::seed_join_kernel_r9, femk::seed_join_kernel_r10},
      {femk::seed_join_banked_kernel_r1, femk::seed_join_banked_kernel_r2, femk::seed_join_banked_kernel_r3, femk::seed_join_banked_kernel_r4,
       femk::seed_join_banked_kernel_r5, femk::seed_join_banked_kernel_r6, femk::seed_join_banked_kernel_r7, femk::seed_join_banked_kernel_r8,
       femk::seed_join_banked_kernel_r9, femk::seed_join_banked_kernel_r10},
      {femk::seed_join_kernel_padded_r1, femk::seed_join_kernel_padded_r2, femk::seed_join_kernel_padded_r3, femk::seed_join_kernel_padded_r4,
       femk::seed_join_kernel_padded_r5, femk::seed_join_kernel_padded_r6, femk::seed_join_kernel_padded_r7, femk::seed_join_kernel_padded_r8,
       femk::seed_join_kernel_padded_r9, femk::seed_join_kernel_padded_r10}};
  return k[which][std::min(std::max(R, 1), femk::kMaxR) - 1];
}

// Blocks of `kernel` one CU holds at a time, `threads` to a block with `lds` bytes (registers and LDS both count): the runtime
// is asked once per such triple and handle (under the handle's lock, as every launch).  Where it does not say: what the LDS
// alone allows, and four blocks of a kernel without LDS (the verification's 256-thread blocks).
uint64_t resident_blocks(fem_dev *h, const void *kernel, uint32_t threads, uint32_t lds) {
  auto at = std::find_if(h->residency.begin(), h->residency.end(), [&](const fem_dev::Residency &r) { return r.kernel == kernel && r.threads == threads && r.lds == lds; });
  if (at == h->residency.end()) {
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, (int)threads, lds) != hipSuccess) nb = 0;
    at = h->residency.insert(at, {kernel, threads, lds, nb});
  }
  return at->blocks > 0 ? (uint64_t)at->blocks : lds ? std::max<uint64_t>(1, 160u * 1024u / lds) : 4;
}
// vector registers per lane of the path's seed_join_kernel<R> / seed_select_kernel<R>
// (handles of several GPUs launch from their own threads: the cache is atomic; every thread would store the same value)
uint32_t kernel_regs(SeedPath path, bool join, bool packed = false) {
  static std::atomic<uint32_t> cache[3][3][femk::kMaxR + 1] = {};
  std::atomic<uint32_t> &slot = cache[join ? path.kind - SeedPath::kDenseCompact : path.banked()][join ? 1 : packed ? 2 : 0][std::min(std::max(path.R, 1), femk::kMaxR)];
  uint32_t c = slot.load(std::memory_order_relaxed);
  if (c) return c;
  hipFuncAttributes a{};
  const void *f = join ? (const void *)join_kernel(path) : (const void *)select_kernel(path.R, path.banked(), packed);
  c = hipFuncGetAttributes(&a, f) == hipSuccess && a.numRegs > 0 ? (uint32_t)a.numRegs : 128u;
  slot.store(c, std::memory_order_relaxed);
  return c;
}

// (timeline only) events around a copy on `st`
struct Span {
  fem_dev *h;
  Slot &s;
  hipStream_t st;
  TimedLaunch t;
  bool on;
  Span(fem_dev *h_, Slot &s_, int id, hipStream_t st_) : h(h_), s(s_), st(st_), t{id, nullptr, nullptr, false}, on(h_->timing && h_->timeline) {
    if (on) {
      t.start = h->event_pool.get(), t.stop = h->event_pool.get();
      (void)hipEventRecord(t.start, st);
    }
  }
  ~Span() {
    if (on) {
      (void)hipEventRecord(t.stop, st);
      s.pending.push_back(t);
    }
  }
};

void drain_timing(fem_dev *h, Slot &s) {
  for (auto &t : s.pending) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, t.start, t.stop) == hipSuccess && t.kernel < kTimedKernels) {
      h->t_ms[t.kernel] += ms;
      h->t_n[t.kernel] += t.counts ? 1 : 0;
    }
    if (h->timeline && h->have_epoch) {
      float a = 0.f, b = 0.f;
      if (hipEventElapsedTime(&a, h->ev_epoch, t.start) == hipSuccess && hipEventElapsedTime(&b, h->ev_epoch, t.stop) == hipSuccess)
        fprintf(stderr, "TL slot %d id %2d  %9.3f %9.3f  (%.3f)\n", (int)(&s - h->slot), t.kernel, a, b, b - a);
    }
    h->event_pool.put(t.start);
    h->event_pool.put(t.stop);
  }
  s.pending.clear();
}

int ensure_outputs(fem_dev *h, Slot &s) {
  if ((size_t)s.n_reads > s.d_nmap.size() || !s.d_nmap) {  // (d_nmap comes last: where it exists, so do the other two)
    const size_t cap = std::max<size_t>((size_t)s.n_reads, 1);
    s.d_nmap.release();
    HIP_TRY(h, femb::alloc_all(cap * 2, s.d_begin, s.d_count));
    HIP_TRY(h, s.d_nmap.ensure(cap));
  }
  if (!s.d_cand || s.cand_cap == 0) {
    uint64_t want = 2 * s.n_reads + (5u << 20);  // ~1 candidate per strand on typical data + chunk padding
    if (h->tiny_buffers) want = 512;
    want = std::min<uint64_t>(want, 0xFFFFFFF0ull);
    s.cand_cap = 0;
    HIP_TRY(h, femb::alloc_all(want, s.d_cand, s.d_meta, s.d_ed, s.d_end));
    s.cand_cap = (uint32_t)want;
  }
  HIP_TRY(h, s.d_ctl.ensure(kCtlAlloc));
  HIP_TRY(h, s.h_ctl.ensure(kCtlBytes));
  if (!s.d_arena) {
    s.arena_cap = h->tiny_buffers ? 256u : (4u << 20);  // entries (32 MiB); grown on demand
    HIP_TRY(h, s.d_arena.ensure(s.arena_cap));
  }
  {
    // With long occurrence lists (large references) nearly every read overflows the lanes of the fast kernel
    // and is queued; with short ones almost none is.  Size the queue for the likely case, grow + re-run otherwise.
    const double avg_bucket = (double)h->n_occ / (double)(h->n_lookup ? h->n_lookup : 1);
    uint64_t want = avg_bucket > 1.0 ? s.n_reads + (1u << 20) : (1u << 18);
    if (h->tiny_buffers) want = s.d_slow ? s.slow_cap : 32;
    if (want > s.slow_cap || !s.d_slow) {
      s.d_slow.release();
      HIP_TRY(h, s.d_slow.ensure(want));
      s.slow_cap = (uint32_t)want;
    }
  }
  return FEM_OK;
}

int grow_candidates(fem_dev *h, Slot &s, uint64_t want) {
  if (want > 0xFFFFFFF0ull) return fail(h, FEM_ERR_UNSUPPORTED, "more than 2^32 candidates in one batch; split the batch");
  s.cand_cap = 0;  // published again only once all four arrays exist (ensure_outputs re-allocates otherwise)
  HIP_TRY(h, femb::alloc_all(want, s.d_cand, s.d_meta, s.d_ed, s.d_end));
  s.cand_cap = (uint32_t)want;
  return FEM_OK;
}

// The link is handed from one batch's copy to the next: call before and after a slot's H2D copies.
int h2d_begin(fem_dev *h, Slot &s) {
  if (h->have_h2d_done) HIP_TRY(h, hipStreamWaitEvent(s.stream, h->ev_h2d_done, 0));
  return FEM_OK;
}
int h2d_end(fem_dev *h, Slot &s) {
  HIP_TRY(h, hipEventRecord(h->ev_h2d_done, s.stream));
  h->have_h2d_done = true;
  return FEM_OK;
}
// No batch's kernels are pending on the device: the batch being committed starts a pipeline (it is sent and mapped in parts)
bool device_idle(fem_dev *h) {
  return (!h->have_kernels_done || hipEventQuery(h->ev_kernels_done) == hipSuccess) &&
         (!h->have_select_done || hipEventQuery(h->ev_select_done) == hipSuccess);
}
// The parts of a batch of n reads, reads [part_begin[q], part_begin[q + 1]): more than one only where the batch meets an idle
// device (and `allowed`: what the caller knows does not speak against it) — a part is at least kPartMinReads reads and begins
// at a multiple of 64.  The copy (enqueue_packed) and the kernels (plan_batch) are split by this one rule.
constexpr uint64_t kPartMinReads = 1u << 16;
int plan_parts(fem_dev *h, uint64_t n, bool allowed, uint32_t part_begin[kMaxParts + 1]) {
  int parts = 1;
  if (allowed && !h->no_parts && !h->no_overlap && n >= 2 * kPartMinReads && device_idle(h)) parts = (int)std::min<uint64_t>((uint64_t)h->max_parts, n / kPartMinReads);
  for (int q = 0; q <= parts; ++q) part_begin[q] = q == parts ? (uint32_t)n : (uint32_t)((n * q / parts) & ~63ull);
  return parts;
}

// `launch` on `st`, between two events when the handle times its kernels (id: fem_dev_kernel_time; counts = false: a further
// part of a launch that is counted already)
template <typename Launch>
int timed_launch(fem_dev *h, Slot &s, int id, hipStream_t st, bool counts, Launch &&launch) {
  TimedLaunch t{id, nullptr, nullptr, counts};
  if (h->timing) {
    t.start = h->event_pool.get(), t.stop = h->event_pool.get();
    HIP_TRY(h, hipEventRecord(t.start, st));
  }
  launch();
  HIP_TRY(h, hipGetLastError());
  if (h->timing) {
    HIP_TRY(h, hipEventRecord(t.stop, st));
    s.pending.push_back(t);
  }
  return FEM_OK;
}

// pack_results_kernel behind the slot's verification, and (send_home) the packed arrays' copies behind it: the per-strand
// bytes and the segment table whole, the per-candidate arrays up to what the slot's previous batch needed (the rest at fetch).
int enqueue_pack(fem_dev *h, Slot &s, bool kernel, bool send_home) {
  const size_t n2 = (size_t)s.n_reads * 2, n_seg = (n2 + 255) / 256;
  int rc;
  HIP_TRY(h, s.d_count8.ensure(n2 + 16));
  HIP_TRY(h, s.d_seg.ensure(n_seg + 4));
  if (s.d_pcand.size() < s.cand_cap || !s.d_pcand) HIP_TRY(h, femb::alloc_all(s.cand_cap, s.d_pcand, s.d_ped, s.d_pend));
  HIP_TRY(h, s.d_big.ensure(kBigCap));
  HIP_TRY(h, s.h_count8.ensure(n2 + 16));
  HIP_TRY(h, s.h_seg.ensure(n_seg + 4));
  HIP_TRY(h, s.h_big.ensure(kBigCap));
  if (kernel) {
    femk::PackParams pp{};
    pp.cand_begin = s.d_begin, pp.cand_count = s.d_count, pp.cand = s.d_cand, pp.ed = s.d_ed, pp.end = s.d_end;
    pp.ctr = ctl_of(s)->ctr, pp.n_strands = (uint32_t)n2;
    pp.count8 = s.d_count8, pp.seg_begin = s.d_seg, pp.pcand = s.d_pcand, pp.ped = s.d_ped, pp.pend = s.d_pend, pp.pcap = (uint32_t)s.d_pcand.size();
    pp.cursor = ctl_of(s)->pack_cursor, pp.big = s.d_big, pp.big_cap = kBigCap;
    const uint32_t grid = (uint32_t)std::max<size_t>(1, (n_seg + femk::kPackSegs - 1) / femk::kPackSegs);  // (a block per sixteen segments)
    // (kernel id 6: pack_results_kernel)
    if ((rc = timed_launch(h, s, 6, s.stream, true, [&] { hipLaunchKernelGGL(femk::pack_results_kernel, dim3(grid), dim3(256), 0, s.stream, pp); }))) return rc;
    s.packed_enqueued = true;
  }
  if (send_home) {  // (on the slot's own stream: see enqueue_prefetch)
    Span span(h, s, 21, s.stream);
    HIP_TRY(h, hipMemcpyAsync(s.h_count8, s.d_count8, n2, hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(h, hipMemcpyAsync(s.h_seg, s.d_seg, n_seg * sizeof(uint32_t), hipMemcpyDeviceToHost, s.stream));
    s.packed_per_read_home = true;
    const size_t guess = std::min<size_t>({(size_t)(s.last_n_packed + s.last_n_packed / 32 + 1024), s.h_pcand.size(), s.d_pcand.size()});
    if (s.last_n_packed && s.h_pcand && guess) {
      HIP_TRY(h, hipMemcpyAsync(s.h_pcand, s.d_pcand, guess * sizeof(uint64_t), hipMemcpyDeviceToHost, s.stream));
      HIP_TRY(h, hipMemcpyAsync(s.h_ped, s.d_ped, guess * sizeof(uint8_t), hipMemcpyDeviceToHost, s.stream));
      HIP_TRY(h, hipMemcpyAsync(s.h_pend, s.d_pend, guess * sizeof(int16_t), hipMemcpyDeviceToHost, s.stream));
      s.packed_home = guess;
    }
  }
  return FEM_OK;
}

int ensure_chars(fem_dev *h, Slot &s);

// One kernel of a batch as it will be launched (plan_batch): a wave's LDS carve-up, the waves of a block — four at most, as many
// as `lds_budget` bytes hold of the layout —, the block's dynamic LDS (`extra`: what it has besides the waves' regions) and the
// grid: as many blocks as the reads want at `reads_per_wave` a wave, at most `max_grid`, what the device holds at a time (the
// planner's).  A grid-stride kernel (no layout, 256 threads) gets exactly max_grid.
struct KernelShape {
  femk::SeedLayout lay{};
  uint32_t wpb = 4, lds = 0, reads_per_block = 0;
  uint64_t max_grid = 1;
  KernelShape() = default;
  KernelShape(const femk::SeedLayout &l, uint32_t lds_budget, uint32_t reads_per_wave, uint32_t extra = 0)
      : lay(l), wpb(std::min<uint32_t>(4u, std::max<uint32_t>(1u, lds_budget / l.wave_bytes))), lds(wpb * l.wave_bytes + extra), reads_per_block(reads_per_wave * wpb) {}
  dim3 block() const { return dim3(64u * wpb); }
  dim3 grid(uint64_t n_reads) const {
    const uint64_t wanted = reads_per_block ? (n_reads + reads_per_block - 1) / reads_per_block : max_grid;
    return dim3((uint32_t)std::max<uint64_t>(1, std::min(wanted, max_grid)));
  }
};
typedef void (*VerifyKernel)(femk::VerifyParams);
VerifyKernel verify_kernel_of(bool packed) { return packed ? femk::verify_kernel_packed : femk::verify_kernel; }

struct BatchPlan {
  SeedPath path{};
  int parts = 1;                  // > 1: mapped in parts, reads [part_begin[q], part_begin[q + 1]) (Slot::parts)
  uint32_t part_begin[kMaxParts + 1] = {};
  bool copied_in_parts = false;   // ... the parts it was copied in (enqueue_packed): ev_part[q] says that part q has arrived
  bool overlap = false;           // dense path: the selection runs beside the previous batch's join (fem_dev::ev_select_done)
  bool need_chars = false;        // a kernel reads the whole batch's characters (ensure_chars)
  bool select_packed = false, verify_packed = false;  // the seed kernels / the verification read the batch's 2-bit codes
  KernelShape select, join, fast, generic, verify;    // (select and join or fast as the path has them; the other two always)
};

// What the slot's staged batch will launch under s.params: every decision, every query of the runtime and every refusal.
// Queues nothing and changes nothing in the slot.
int plan_batch(fem_dev *h, const Slot &s, BatchPlan &pl) {
  const fem_params &p = s.params;
  const SeedPath path = pl.path = seed_path(h, p);
  pl.overlap = path.dense() && !h->no_overlap;
  // A batch that meets an IDLE device (the start of a job) is mapped in parts on a dense index: those of its copy where it
  // was copied in parts (enqueue_packed), else (an exception kept the copy whole, or the batch is mapped again) cut here.
  pl.copied_in_parts = s.parts > 1 && path.dense();
  pl.parts = pl.copied_in_parts ? s.parts : plan_parts(h, s.n_reads, path.dense(), pl.part_begin);
  if (pl.copied_in_parts) std::copy(s.part_begin, s.part_begin + kMaxParts + 1, pl.part_begin);
  // Who reads a whole batch's characters gets them made first (ensure_chars): seed_fast_kernel, the generic kernel over all
  // reads, verify_kernel.  The dense kernels read a packed batch's codes, and characters of its marked reads only.
  pl.need_chars = s.n_reads && (!path.dense() || h->verify_chars);
  pl.select_packed = s.sent_packed && !h->select_chars && path.dense();
  // A batch that came packed (equal-length reads, codes in d_packed_alloc) is verified straight from its 2-bit codes; every
  // other one — mixed lengths, FEM_NO_PACK, the zero-copy character forms — from its characters.
  pl.verify_packed = s.sent_packed && !h->verify_chars;
  const uint32_t max_len = std::max<uint32_t>(s.max_len, (uint32_t)p.k);
  pl.generic = KernelShape(make_layout(p, max_len), 64u * 1024u, 1);
  if (pl.generic.lay.wave_bytes > 64u * 1024u) return fail(h, FEM_ERR_UNSUPPORTED, "read too long for the device path");
  const uint32_t generic_waves_per_cu = std::min<uint32_t>(32u, (160u * 1024u / pl.generic.lds) * pl.generic.wpb);
  pl.generic.max_grid = (uint64_t)h->n_cu * std::max<uint32_t>(1u, generic_waves_per_cu / pl.generic.wpb) * 4;
  if (s.n_reads == 0) return FEM_OK;
  // grid-stride kernel: exactly the blocks that are resident together, or the ones that start late set the makespan
  pl.verify.max_grid = (uint64_t)h->n_cu * resident_blocks(h, (const void *)verify_kernel_of(pl.verify_packed), 256, 0);
  if (path.dense()) {
    pl.select = KernelShape(make_layout_select(p, max_len, pl.select_packed), 64u * 1024u, femk::kReadBlock);
    if (pl.select.lay.wave_bytes > 64u * 1024u) return fail(h, FEM_ERR_UNSUPPORTED, "read too long for the device path");
    pl.join = KernelShape(make_layout_join(p, path.banked(), path.kind == SeedPath::kDenseStrided), 60u * 1024u, femk::kReadBlock, 64u * 8u);
    pl.join.lay.picked = pl.join.wpb * pl.join.lay.wave_bytes;  // the block's sequence table, behind the waves' regions
    const KernelShape &ks = pl.select, &kj = pl.join;
    // (3.3 ms per 2.5 M reads of C3 with one block per CU as with five: sectors per second, not waves)
    const uint64_t per_cu_s = pl.overlap ? 1 : resident_blocks(h, (const void *)select_kernel(path.R, path.banked(), pl.select_packed), 64u * ks.wpb, ks.lds);
    uint64_t per_cu_j = resident_blocks(h, (const void *)join_kernel(path), 64u * kj.wpb, kj.lds);
    if (pl.overlap) {
      // leave one block of the next batch's seed_select_kernel room on every CU: registers (512 per lane and SIMD,
      // handed out in eights), LDS (160 KB) and wave slots (8 per SIMD) of both kernels together
      const uint32_t vj = (kernel_regs(path, true) + 7u) & ~7u, vs = (kernel_regs(path, false, pl.select_packed) + 7u) & ~7u;
      const uint32_t wj = 64u * kj.wpb / 256u ? 64u * kj.wpb / 256u : 1u, ws = 64u * ks.wpb / 256u ? 64u * ks.wpb / 256u : 1u;  // waves per SIMD and block
      const uint32_t lj = (kj.lds + 511u) & ~511u, ls = (ks.lds + 511u) & ~511u;  // (LDS is handed out in pieces of 512 bytes)
      while (per_cu_j > 1 && (per_cu_j * wj * vj + ws * vs > 512u || per_cu_j * lj + ls > 160u * 1024u || per_cu_j * wj + ws > 8u)) --per_cu_j;
    }
    pl.select.max_grid = (uint64_t)h->n_cu * per_cu_s, pl.join.max_grid = (uint64_t)h->n_cu * per_cu_j;
  } else if (path.fast()) {
    const bool hash = path.kind == SeedPath::kFastHash;
    pl.fast = KernelShape(make_layout_fast(p, max_len, hash), 64u * 1024u, femk::kReadBlock);
    // The kernel's waves pull blocks of reads from a cursor: the grid is exactly what is resident at a time
    // (registers included).  (With a fixed stride per wave the same grid took 6.9 ms against 6.2 at six times as
    // many waves: the CUs do not all run at the same pace.  Every wave pads its last chunk of candidate slots, so
    // extra waves cost the verify kernel lanes.)  FEM_GRID_MULT overrides the multiple (measurement only).
    static const uint64_t mult = testing_switch("FEM_TESTING") && getenv("FEM_GRID_MULT") ? (uint64_t)std::max(1, atoi(getenv("FEM_GRID_MULT"))) : 1;
    pl.fast.max_grid = (uint64_t)h->n_cu * resident_blocks(h, (const void *)fast_kernel(path.R, hash), 64u * pl.fast.wpb, pl.fast.lds) * mult;
  }
  return FEM_OK;
}

// What every seed kernel of the batch takes, with the generic kernel's layout (the dense kernels' tables: enqueue_dense)
femk::SeedParams seed_params(const fem_dev *h, const Slot &s, const BatchPlan &pl) {
  const fem_params &p = s.params;
  CtlBlock *ctl = ctl_of(s);
  femk::SeedParams sp{};
  if (pl.select_packed) sp.packed = s.packed(), sp.exc_bits = s.d_exc_bits, sp.bpr = s.packed_bpr, sp.len = s.max_len;
  sp.bases = s.map_bases(), sp.read_off = s.map_off(), sp.n_reads = (uint32_t)s.n_reads;
  sp.lookup = h->d_lookup, sp.occ = h->d_occ, sp.inf32 = (uint32_t)h->n_occ, sp.summary = h->d_summary;
  sp.seq_len = h->d_seq_len, sp.n_seq = h->n_seq;
  sp.e = p.e, sp.a = p.a, sp.R = pl.path.R, sp.k = p.k, sp.step = p.step;
  sp.lg = p.k / p.step + (p.k % p.step ? 1 : 0);
  sp.cand = s.d_cand, sp.cand_meta = s.d_meta, sp.cand_cap = s.cand_cap;
  sp.cand_begin = s.d_begin, sp.cand_count = s.d_count;
  sp.ctr = ctl->ctr, sp.stats = ctl->stats, sp.work_cursor = &ctl->work[0].select;
  sp.arena = s.d_arena, sp.arena_cap = s.arena_cap, sp.arena_ctr = ctl->arena_ctr;
  sp.slow_queue = s.d_slow, sp.slow_cap = s.slow_cap;  // (work_queue: enqueue_generic)
  sp.lay = pl.generic.lay;
  return sp;
}

femk::VerifyParams verify_params(const fem_dev *h, const Slot &s, const BatchPlan &pl) {
  CtlBlock *ctl = ctl_of(s);
  femk::VerifyParams vp{};
  vp.bases = s.map_bases(), vp.read_off = s.map_off();
  vp.planes = h->d_planes, vp.seq_off = h->d_seq_off;
  vp.cand = s.d_cand, vp.cand_meta = s.d_meta;
  vp.ctr = ctl->ctr, vp.cand_cap = s.cand_cap, vp.e = s.params.e;
  vp.ed = s.d_ed, vp.end = s.d_end;
  vp.n_map = s.d_nmap, vp.stats = ctl->stats;
  if (pl.verify_packed) vp.packed = s.packed(), vp.exc_bits = s.d_exc_bits, vp.bpr = s.packed_bpr, vp.len = s.max_len;
  return vp;
}

// Dense index: seed selection for blocks of reads (fem_seed_select.hip.h), then the bitmap join on 32-bit coordinates, a wave
// per read (fem_seed_dense.hip.h).  A batch mapped in parts: part q's selection on the side stream as soon as its characters
// are in HBM, its join on the slot's stream behind its selection — beside the selection of part q + 1.  Any other batch is one
// part, selection and join on the slot's stream as before.
int enqueue_dense(fem_dev *h, Slot &s, const BatchPlan &pl, femk::SeedParams fp) {
  const SeedPath path = pl.path;
  const int parts = pl.parts;
  int rc;
  HIP_TRY(h, s.d_sel.ensure((size_t)s.n_reads * 6u * (size_t)path.R * h->n_banks));
  HIP_TRY(h, s.d_sel_hdr.ensure((size_t)s.n_reads));
  fp.occ32 = h->d_occ32, fp.list_shift = h->list_shift, fp.goff = h->d_goff, fp.blkseq = h->d_blkseq;
  fp.freq11 = h->d_freq11, fp.sel = s.d_sel, fp.sel_hdr = s.d_sel_hdr;
  fp.n_banks = h->n_banks, fp.bank_lo = h->d_bank_lo, fp.n_buckets = (uint32_t)(h->n_lookup - 1);
  fp.blk_stride = (femk::kDenseRemap >> femk::kDenseBlkShift) + 1u;
  for (uint32_t b = 0; b <= femk::kDenseMaxBanks; ++b) fp.bank_first[b] = h->bank_first[b];
  if (parts > 1 && !pl.copied_in_parts) {  // (the copy went whole, on the slot's stream: the side stream starts behind it)
    HIP_TRY(h, hipEventRecord(s.ev_zeroed, s.stream));
    HIP_TRY(h, hipStreamWaitEvent(h->side_stream, s.ev_zeroed, 0));
  }
  hipStream_t st_sel = parts > 1 ? h->side_stream : s.stream;
  for (int q = 0; q < parts; ++q) {
    const uint32_t n_part = pl.part_begin[q + 1] - pl.part_begin[q];
    fp.read_begin = pl.part_begin[q], fp.n_reads = pl.part_begin[q + 1];
    CtlBlock::Work *cursors = &ctl_of(s)->work[q];
    if (parts > 1) {
      if (pl.copied_in_parts) HIP_TRY(h, hipStreamWaitEvent(st_sel, s.ev_part[q], 0));
    } else if (pl.overlap && h->have_select_done) {
      HIP_TRY(h, hipStreamWaitEvent(s.stream, h->ev_select_done, 0));
    }
    fp.lay = pl.select.lay, fp.work_cursor = &cursors->select;
    const SeedKernel select = select_kernel(path.R, path.banked(), pl.select_packed);
    if ((rc = timed_launch(h, s, 8, st_sel, q == 0, [&] { hipLaunchKernelGGL(select, pl.select.grid(n_part), pl.select.block(), pl.select.lds, st_sel, fp); }))) return rc;
    if (parts > 1) {
      HIP_TRY(h, hipEventRecord(s.ev_sel[q], st_sel));
      HIP_TRY(h, hipStreamWaitEvent(s.stream, s.ev_sel[q], 0));
    }
    if (pl.overlap && q + 1 == parts) {
      HIP_TRY(h, hipEventRecord(h->ev_select_done, st_sel));
      h->have_select_done = true;
    }
    if (pl.overlap && q == 0 && h->have_kernels_done) HIP_TRY(h, hipStreamWaitEvent(s.stream, h->ev_kernels_done, 0));
    fp.lay = pl.join.lay, fp.work_cursor = &cursors->join;
    if ((rc = timed_launch(h, s, 0, s.stream, q == 0, [&] { hipLaunchKernelGGL(join_kernel(path), pl.join.grid(n_part), pl.join.block(), pl.join.lds, s.stream, fp); }))) return rc;
  }
  return FEM_OK;
}

// Sparse index: seed_fast_kernel over the whole batch, in the form the path names
int enqueue_fast(fem_dev *h, Slot &s, const BatchPlan &pl, femk::SeedParams fp) {
  const KernelShape &k = pl.fast;
  const SeedKernel fast = fast_kernel(pl.path.R, pl.path.kind == SeedPath::kFastHash);
  fp.lay = k.lay;
  return timed_launch(h, s, 0, s.stream, true, [&] { hipLaunchKernelGGL(fast, k.grid(s.n_reads), k.block(), k.lds, s.stream, fp); });
}
// seed_filter_kernel: over every read on the generic path; behind the fast or the dense kernels it finishes what they queued
int enqueue_generic(fem_dev *h, Slot &s, const BatchPlan &pl, femk::SeedParams sp) {
  const KernelShape &k = pl.generic;
  if (pl.path.kind != SeedPath::kGeneric) sp.work_queue = s.d_slow;
  return timed_launch(h, s, 2, s.stream, true, [&] { hipLaunchKernelGGL(femk::seed_filter_kernel, k.grid(s.n_reads), k.block(), k.lds, s.stream, sp); });
}
int enqueue_verify(fem_dev *h, Slot &s, const BatchPlan &pl) {
  const femk::VerifyParams vp = verify_params(h, s, pl);
  const VerifyKernel verify = verify_kernel_of(pl.verify_packed);
  return timed_launch(h, s, 1, s.stream, true, [&] { hipLaunchKernelGGL(verify, pl.verify.grid(s.n_reads), pl.verify.block(), 0, s.stream, vp); });
}

// fem_dev_fetch callers get the per-read arrays sent home behind the kernels, and the per-candidate arrays up to what the slot's
// previous batch needed (Slot::prefetch_results) — on the slot's own stream.  (Tried: one stream for every slot's results
// behind an event of the slot's stream — consistent 0.63 ms per 32 MB where a slot's own stream takes 0.6 to 1.5 beside the next
// batch's H2D copy, but the calls that enqueue the copies then kept the host until the batch's kernels were through: 326 -> 284
// Mreads/s.  Ten streams timed one by one all copy at 54 GB/s: the slow copies are the link shared with the other direction,
// not a slow engine.)
int enqueue_prefetch(fem_dev *h, Slot &s) {
  s.prefetched_reads2 = 0, s.prefetched_cand = 0;
  static const bool no_prefetch = testing_switch("FEM_NO_PREFETCH");
  // (only behind fem_dev_stage_reads, whose caller packs the next batch in the meantime; a caller of the zero-copy form is
  // idle until it fetches, and the extra traffic next to its four-times-larger H2D cost 5 % there)
  if (!s.prefetch_results || s.want_packed || !s.staged_by_copy || no_prefetch) return FEM_OK;
  Span span(h, s, 21, s.stream);
  const size_t n2 = (size_t)s.n_reads * 2;
  if (n2 && s.h_begin && n2 <= s.h_begin.size()) {
    HIP_TRY(h, hipMemcpyAsync(s.h_begin, s.d_begin, n2 * sizeof(uint32_t), hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(h, hipMemcpyAsync(s.h_count, s.d_count, n2 * sizeof(uint32_t), hipMemcpyDeviceToHost, s.stream));
    s.prefetched_reads2 = n2;
  }
  const size_t guess = std::min<size_t>({(size_t)(s.last_n_cand + s.last_n_cand / 32 + 1024), s.h_cand.size(), (size_t)s.cand_cap});
  if (s.last_n_cand && s.h_cand && guess) {
    HIP_TRY(h, hipMemcpyAsync(s.h_cand, s.d_cand, guess * sizeof(uint64_t), hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(h, hipMemcpyAsync(s.h_ed, s.d_ed, guess * sizeof(uint8_t), hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(h, hipMemcpyAsync(s.h_end, s.d_end, guess * sizeof(int16_t), hipMemcpyDeviceToHost, s.stream));
    s.prefetched_cand = guess;
  }
  return FEM_OK;
}

// Enqueue one batch (asynchronous): its kernels as plan_batch has them — the path's seed kernels, the generic kernel, the
// verification — on the slot's stream (a batch mapped in parts: its selections on the side stream), and behind them what
// goes home.  Different batches' kernels are chained by the handle's events (fem_dev::ev_kernels_done, ev_select_done).
int launch_batch(fem_dev *h, Slot &s) {
  int rc;
  BatchPlan pl;
  if ((rc = plan_batch(h, s, pl))) return rc;
  s.parts = 1;  // (consumed: the slot's batch mapped again starts from the device's state then)
  // (a batch mapped in parts: zeroed on the side stream, ahead of the slot's stream, which may still be busy with the rest of its copy)
  if (pl.parts > 1 && h->have_select_done) HIP_TRY(h, hipStreamWaitEvent(h->side_stream, h->ev_select_done, 0));
  HIP_TRY(h, hipMemsetAsync(s.d_ctl, 0, kCtlAlloc, pl.parts > 1 ? h->side_stream.s : s.stream.s));
  if (pl.need_chars && (rc = ensure_chars(h, s))) return rc;
  s.select_packed = pl.select_packed && s.n_reads != 0;
  s.packed_enqueued = false, s.packed_home = 0, s.packed_per_read_home = false;
  if (s.n_reads) {
    const bool dense = pl.path.dense();
    const femk::SeedParams sp = seed_params(h, s, pl);
    if (!pl.overlap && h->have_kernels_done) HIP_TRY(h, hipStreamWaitEvent(s.stream, h->ev_kernels_done, 0));
    HIP_TRY(h, hipMemsetAsync(s.d_nmap, 0, (size_t)s.n_reads * sizeof(uint32_t), s.stream));  // (the verification counts into it)
    if ((rc = dense ? enqueue_dense(h, s, pl, sp) : pl.path.fast() ? enqueue_fast(h, s, pl, sp) : FEM_OK)) return rc;
    if ((rc = enqueue_generic(h, s, pl, sp))) return rc;
    if ((rc = enqueue_verify(h, s, pl))) return rc;
    // (the packing inside the chain of the batches' kernels, 0.07 ms: beside the next batch's join — three kernels starting at
    //  once — it cost that join 0.6 ms; on a sparse index, where nothing runs beside the seed kernel, it goes behind the chain)
    if (s.want_packed && dense && (rc = enqueue_pack(h, s, true, false))) return rc;
    HIP_TRY(h, hipEventRecord(h->ev_kernels_done, s.stream));
    h->have_kernels_done = true;
    if (s.want_packed && (rc = enqueue_pack(h, s, !dense, true))) return rc;
  }
  HIP_TRY(h, hipMemcpyAsync(s.h_ctl, s.d_ctl, kCtlBytes, hipMemcpyDeviceToHost, s.stream));
  if ((rc = enqueue_prefetch(h, s))) return rc;
  s.mapped = true, s.synced = false, s.covered = false;
  return FEM_OK;
}

// After the index is resident: for sparse indexes build the bucket summaries the fast seed kernel tests first.
int refresh_summary(fem_dev *h) {
  h->d_summary.release();
  const uint64_t n_buckets = h->n_lookup - 1;
  // dense index: nearly every bucket is non-empty, the tests would not pay.  (Fewer than 2^31 entries also keeps bit
  // 31 of a lookup value free: the fast seed kernel tags deferred lookups with it.)
  if (h->n_occ >= n_buckets || h->n_occ >= 0x80000000ull || (n_buckets >> 3) >= (1ull << 22)) return FEM_OK;
  const uint64_t words = n_buckets / femk::kSummaryBuckets + 2;
  HIP_TRY(h, h->d_summary.ensure(words));
  HIP_TRY(h, hipMemset(h->d_summary, 0, words * sizeof(uint32_t)));
  hipLaunchKernelGGL(femk::bucket_summary_kernel, dim3((uint32_t)h->n_cu * 8u), dim3(256), 0, 0, h->d_lookup, n_buckets, h->d_summary);
  HIP_TRY(h, hipGetLastError());
  HIP_TRY(h, hipDeviceSynchronize());
  return FEM_OK;
}

// After index AND reference are resident: for dense indexes (long occurrence lists) derive the occurrence table in
// 32-bit global coordinates that seed_join_kernel joins on (fem_seed_dense.hip.h) and the byte frequencies seed_select_kernel reads.  Skipped (the 64-bit hash-join
// form of seed_fast_kernel runs instead) when the coordinates do not fit 32 bits.
constexpr double kDenseMinAvgBucket = 4.0;
int refresh_dense(fem_dev *h) {
  auto drop = [&]() {
    h->d_occ32.release(), h->d_goff.release(), h->d_blkseq.release(), h->d_freq11.release(), h->d_bank_lo.release();
    h->n_banks = 1, h->list_shift = 0;
  };
  drop();
  if (!h->d_occ || !h->d_ref_raw || h->no_dense || h->k != femk::kK || h->step != femk::kStep || h->n_occ == 0) return FEM_OK;
  const uint64_t n_buckets = h->n_lookup - 1;
  if (!h->force_dense && (double)h->n_occ < kDenseMinAvgBucket * (double)n_buckets) return FEM_OK;
  // Coordinates: goff[seq] + pos, a gap between sequences; where the next sequence would pass the 32-bit limit a new BANK
  // starts with coordinates of its own (fem_seed_dense.hip.h) — up to kDenseMaxBanks of them, else the 64-bit join
  const uint64_t limit = h->bank_limit ? std::min<uint64_t>(h->bank_limit, femk::kDenseLimit) : femk::kDenseLimit;
  const uint32_t seq_limit = h->bank_seqs ? std::min<uint32_t>(h->bank_seqs, femk::kDenseMaxSeq) : femk::kDenseMaxSeq;
  std::vector<uint32_t> goff(h->n_seq + 1);
  uint32_t n_banks = 1, bank_first[5] = {0, 0, 0, 0, 0};
  // Where more than one bank is needed they are cut about EQUAL, not the first ones filled to the brim: the join runs once
  // per bank on that bank's part of every list, and a pass over lists of up to 64 entries costs about half of one over
  // longer lists (their second chunks).  Filling each bank up to the mean + one sequence never needs more banks.
  uint64_t cap = limit;
  {
    uint64_t total_c = femk::kDenseGap, longest = 0;
    for (uint32_t i = 0; i < h->n_seq; ++i) total_c += (uint64_t)h->seq_len[i] + femk::kDenseGap, longest = std::max<uint64_t>(longest, h->seq_len[i]);
    const uint64_t want = (total_c + limit - 1) / limit;
    if (want > 1) cap = std::min<uint64_t>(limit, (total_c + want - 1) / want + longest + femk::kDenseGap);
  }
  uint64_t at = femk::kDenseGap;
  for (uint32_t i = 0; i < h->n_seq; ++i) {
    // (a bank also ends at kDenseMaxSeq sequences: the remapped near-start entries carry the index within the bank)
    if ((at + (uint64_t)h->seq_len[i] + femk::kDenseGap > cap && at != femk::kDenseGap) || i - bank_first[n_banks - 1] >= seq_limit) {
      if (n_banks == femk::kDenseMaxBanks) return FEM_OK;
      bank_first[n_banks++] = i;
      at = femk::kDenseGap;
    }
    goff[i] = (uint32_t)at;
    at += (uint64_t)h->seq_len[i] + femk::kDenseGap;
    if (at > femk::kDenseLimit) return FEM_OK;  // one sequence beyond 32 bits: 64-bit join
  }
  goff[h->n_seq] = (uint32_t)at;
  for (uint32_t b = n_banks; b <= femk::kDenseMaxBanks; ++b) bank_first[b] = h->n_seq;
  const uint32_t n_blk = (femk::kDenseRemap >> femk::kDenseBlkShift) + 1u;
  std::vector<uint32_t> blkseq((size_t)n_blk * n_banks, 0);  // per bank: the last of its sequences starting at or before each 2^20 block
  for (uint32_t bank = 0; bank < n_banks; ++bank)
    for (uint32_t b = 0, sq = bank_first[bank]; b < n_blk; ++b) {
      const uint64_t first = (uint64_t)b << femk::kDenseBlkShift;
      while (sq + 1u < bank_first[bank + 1] && goff[sq + 1u] <= first) ++sq;
      blkseq[(size_t)bank * n_blk + b] = sq;
    }
  // These tables are optional (4 bytes per occurrence: 4 GB at 3 Gbp): a failed allocation declines the dense form —
  // the 64-bit hash-join form of seed_fast_kernel runs without them — instead of failing the upload.
  Buf<uint32_t> d_bad;
  auto decline = [&]() {
    drop();
    (void)hipGetLastError();  // (clears the out-of-memory error)
    return FEM_OK;
  };
  // One coordinate space: the STRIDED 32-bit table (fem_seed_dense.hip.h: 512 bytes per bucket, lists on line boundaries, found
  // by the hash alone).  Where it does not fit, and for references in banks (whose lists are cut at bank_lo), the compact one.
  // It is 8.6 GB whatever the reference, so it is taken where the compact table is at least an eighth of that (16 entries per
  // bucket and more: references from ~0.8 Gbp; at 3 Gbp it is 2.1 x the compact table and bought 7 % of the step) — and
  // wherever FEM_FORCE_DENSE asks for the dense kernels on a small reference (the parity tests of the padded join).
  uint32_t list_shift = 0;
  const bool strided_pays = h->force_dense || h->n_occ >= (n_buckets << 4);
  if (n_banks == 1 && !h->no_strided && strided_pays) {
    const size_t words = ((size_t)n_buckets + femk::kDensePadBuckets) << femk::kDenseListShift;
    bool ok = h->d_occ32.ensure(words) == hipSuccess;
    if (ok) {  // every slot reads "pad" (fem_seed_dense.hip.h) until dense_occ32_strided_kernel writes a bucket's entries over its first ones
      hipLaunchKernelGGL(femk::dense_pad_kernel, dim3((uint32_t)h->n_cu * 16u), dim3(256), 0, 0, (uint4 *)h->d_occ32.get(), (uint64_t)(words / 4));
      ok = hipGetLastError() == hipSuccess;
    }
    if (ok) {
      list_shift = femk::kDenseListShift;
    } else {
      h->d_occ32.release();
      (void)hipGetLastError();
    }
  }
  if (h->d_goff.ensure(goff.size()) != hipSuccess || h->d_blkseq.ensure(blkseq.size()) != hipSuccess ||
      (!list_shift && h->d_occ32.ensure(h->n_occ + 256) != hipSuccess) || h->d_freq11.ensure((size_t)femk::kX11 * 4u) != hipSuccess ||
      (n_banks > 1 && h->d_bank_lo.ensure((size_t)(n_banks - 1) * n_buckets) != hipSuccess) || d_bad.ensure(1) != hipSuccess)
    return decline();
  if (hipMemset(d_bad, 0, sizeof(uint32_t)) != hipSuccess ||
      hipMemcpy(h->d_goff, goff.data(), goff.size() * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(h->d_blkseq, blkseq.data(), blkseq.size() * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess) {
    (void)decline();
    return fail(h, FEM_ERR_HIP, "dense tables: copy to the device failed");
  }
  femk::BankFirst bf{};
  bf.n = n_banks;
  for (uint32_t b = 0; b <= femk::kDenseMaxBanks; ++b) bf.first[b] = bank_first[b];
  if (list_shift)
    hipLaunchKernelGGL(femk::dense_occ32_strided_kernel, dim3((uint32_t)h->n_cu * 8u), dim3(256), 0, 0, h->d_occ, h->d_lookup, (uint32_t)n_buckets, h->d_goff,
                       h->n_seq, h->d_occ32, d_bad);
  else
    hipLaunchKernelGGL(femk::dense_occ32_kernel, dim3((uint32_t)h->n_cu * 8u), dim3(256), 0, 0, h->d_occ, h->n_occ, h->d_goff, h->n_seq, bf,
                       h->d_occ32, d_bad);
  uint32_t bad = 0;
  if (hipGetLastError() != hipSuccess || hipMemcpy(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost) != hipSuccess) {
    (void)decline();
    return fail(h, FEM_ERR_HIP, "dense tables: building the 32-bit occurrence table failed");
  }
  if (bad) return decline();  // the index names sequences the reference does not have: leave that to the 64-bit path's checks
  d_bad.release();
  for (uint32_t b = 1; b < n_banks; ++b)  // where bank b's part of every list starts
    hipLaunchKernelGGL(femk::bank_split_kernel, dim3((uint32_t)h->n_cu * 8u), dim3(256), 0, 0, h->d_occ, h->d_lookup, (uint32_t)n_buckets, bank_first[b],
                       h->d_bank_lo + (size_t)(b - 1) * n_buckets);
  h->n_banks = n_banks, h->list_shift = list_shift;
  for (uint32_t b = 0; b <= femk::kDenseMaxBanks; ++b) h->bank_first[b] = bank_first[b];
  // byte frequencies per 11-mer for seed_select_kernel (fem_seed_select.hip.h)
  hipLaunchKernelGGL(femk::freq11_kernel, dim3((uint32_t)h->n_cu * 8u), dim3(256), 0, 0, h->d_lookup, h->d_freq11);
  HIP_TRY(h, hipGetLastError());
  HIP_TRY(h, hipDeviceSynchronize());
  return FEM_OK;
}

// The RCCL communicator of fem_dev_allreduce_stats (one process, one handle per GPU): kept across calls.
struct CommSet {
  std::vector<int> devs;
  std::vector<ncclComm_t> comms;
  std::vector<Buf<uint64_t>> bufs;
};
std::mutex g_comm_mu;
CommSet *g_comm = nullptr;
void destroy_comm_set() {  // caller holds g_comm_mu
  if (!g_comm) return;
  for (size_t i = 0; i < g_comm->devs.size(); ++i) {
    (void)hipSetDevice(g_comm->devs[i]);
    g_comm->bufs[i].release();
    if (g_comm->comms[i]) ncclCommDestroy(g_comm->comms[i]);
  }
  delete g_comm;
  g_comm = nullptr;
}

int check_slot(fem_dev *h, int slot) {
  if (!h) return FEM_ERR_INVALID;
  if (slot < 0 || slot >= kSlots) return fail(h, FEM_ERR_INVALID, "slot out of range");
  return FEM_OK;
}
// A setter or getter of one slot's output options and counts: `body` gets the slot, under the handle's lock.
template <class Body>
int with_slot(fem_dev *h, int slot, Body body) {
  int rc = check_slot(h, slot);
  if (rc) return rc;
  FEM_LOCK(h);
  return body(h->slot[slot]);
}


// ---- packed read transfer: host side in fem_pack.h (the device side is unpack_reads_kernel) ----
using fempack::pack_bases;

// The whole batch's characters and offsets in HBM, for whoever reads s.bases() or s.d_off of more than the marked reads
// (DESIGN.md 5.1 lists them): enqueued on the slot's stream, once per batch.  A batch that came as characters has them.
int ensure_chars(fem_dev *h, Slot &s) {
  if (s.chars_ready) return FEM_OK;
  const uint64_t n = s.n_reads, n_exc = s.n_exc;
  const uint32_t len = s.max_len, bpr = s.packed_bpr;
  const uint64_t code_bytes = fempack::code_bytes(n, len);
  if (!s.offs_ready)
    hipLaunchKernelGGL(femk::uniform_offsets_kernel, dim3((uint32_t)std::min<uint64_t>((n + 256) / 256, (uint64_t)h->n_cu * 8u)), dim3(256), 0,
                       s.stream, s.d_off, n, len);
  if (n) {
    const uint32_t grid = (uint32_t)std::min<uint64_t>((n * bpr + 255) / 256, (uint64_t)h->n_cu * 16u);
    hipLaunchKernelGGL(femk::unpack_reads_kernel, dim3(grid), dim3(256), 0, s.stream, (const uint8_t *)s.packed(), n, len, bpr, s.bases());
  }
  if (n_exc) {
    const dim3 g((uint32_t)std::min<uint64_t>((n_exc + 255) / 256, (uint64_t)h->n_cu * 4u));
    hipLaunchKernelGGL(femk::scatter_chars_kernel, g, dim3(256), 0, s.stream, (const uint32_t *)(s.packed() + code_bytes),
                       (const uint8_t *)(s.packed() + code_bytes + 4u * n_exc), n_exc, s.bases());
  }
  HIP_TRY(h, hipGetLastError());
  HIP_TRY(h, hipEventRecord(s.ev_chars, s.stream));
  s.chars_ready = true, s.offs_ready = true;
  return FEM_OK;
}

// Device side of a packed batch that sits in the slot's pinned staging (codes | uint32 positions | bytes, fem_pack.h):
// one copy; the reads marked as holding a character other than "ACGT" get their characters and offsets at once, the
// rest of the batch when something asks (ensure_chars).
int enqueue_packed(fem_dev *h, Slot &s, uint64_t n, uint32_t len, uint64_t n_exc) {
  const uint32_t bpr = fempack::bytes_per_read(len);
  const uint64_t code_bytes = fempack::code_bytes(n, len), n_bases = n * (uint64_t)len;
  const uint64_t total = code_bytes + n_exc * 5u;
  int rc;
  HIP_TRY(h, s.d_packed_alloc.ensure(kPackedFrontPad + (size_t)total + 64));
  HIP_TRY(h, s.d_bases_alloc.ensure(kFrontPad + (size_t)n_bases + 64));
  HIP_TRY(h, s.d_off.ensure((size_t)n + 1));
  HIP_TRY(h, s.d_exc_bits.ensure((size_t)n / 32 + 2));
  // parts: only where nothing is pending on the device (the start of a job), for batches without exceptions (their scatter
  // follows the whole batch) and of some size
  s.parts = plan_parts(h, n, n_exc == 0, s.part_begin);
  HIP_TRY(h, hipMemsetAsync(s.d_exc_bits, 0, ((size_t)n / 32 + 1) * sizeof(uint32_t), s.stream));
  // The characters are made here only where the selection is to read them (FEM_SELECT_CHARS) or where more than one read in
  // kExpandAllShare may be marked: expanding read by read then moves about as much as expanding the batch, less well.
  const bool at_commit = h->select_chars || n_exc * kExpandAllShare > n;
  // (a handle without the dense tables will ask for the characters when the batch is mapped: its offset table, which depends on
  //  nothing the copy brings, is still written here, in front of the copy — behind it it cost C2 6 us per step)
  const bool offs_at_commit = at_commit || !has_dense_tables(h);
  if (offs_at_commit)
    hipLaunchKernelGGL(femk::uniform_offsets_kernel, dim3((uint32_t)std::min<uint64_t>((n + 256) / 256, (uint64_t)h->n_cu * 8u)), dim3(256), 0,
                       s.stream, s.d_off, n, len);
  if ((rc = h2d_begin(h, s))) return rc;
  for (int q = 0; q < s.parts; ++q) {
    const uint64_t r0 = s.part_begin[q], r1 = s.part_begin[q + 1];
    // (the last part takes the codes' padding and the exceptions along)
    const uint64_t b0 = r0 * bpr, b1 = q + 1 == s.parts ? total : r1 * bpr;
    Span span(h, s, 20, s.stream);
    if (b1 > b0) HIP_TRY(h, hipMemcpyAsync(s.packed() + b0, s.h_bases + b0, b1 - b0, hipMemcpyHostToDevice, s.stream));
    // (the link goes to the next batch's copy as soon as this batch's last byte is over — not behind the expansion kernel,
    //  which waits for a free wave slot beside the running kernels: that chained C2's batches at 2.0 ms apiece)
    if (q + 1 == s.parts && (rc = h2d_end(h, s))) return rc;
    if (at_commit && r1 > r0) {
      const uint32_t grid = (uint32_t)std::min<uint64_t>(((r1 - r0) * bpr + 255) / 256, (uint64_t)h->n_cu * 16u);
      hipLaunchKernelGGL(femk::unpack_reads_kernel, dim3(grid), dim3(256), 0, s.stream, (const uint8_t *)s.packed() + b0, r1 - r0, len, bpr,
                         s.bases() + r0 * len);
    }
    if (s.parts > 1) HIP_TRY(h, hipEventRecord(s.ev_part[q], s.stream));
  }
  if (n_exc) {
    const dim3 g((uint32_t)std::min<uint64_t>((n_exc + 255) / 256, (uint64_t)h->n_cu * 4u));
    if (!at_commit) {  // the marked reads alone: their characters and their d_off entries, then the bytes that belong there
      const dim3 gm((uint32_t)std::min<uint64_t>((n_exc * bpr + 255) / 256, (uint64_t)h->n_cu * 8u));
      hipLaunchKernelGGL(femk::unpack_marked_reads_kernel, gm, dim3(256), 0, s.stream, (const uint8_t *)s.packed(),
                         (const uint32_t *)(s.packed() + code_bytes), n_exc, len, bpr, s.bases(), s.d_off.get());
    }
    hipLaunchKernelGGL(femk::scatter_chars_kernel, g, dim3(256), 0, s.stream, (const uint32_t *)(s.packed() + code_bytes),
                       (const uint8_t *)(s.packed() + code_bytes + 4u * n_exc), n_exc, s.bases());
    hipLaunchKernelGGL(femk::mark_exception_reads_kernel, g, dim3(256), 0, s.stream, (const uint32_t *)(s.packed() + code_bytes), n_exc, len,
                       s.d_exc_bits);
  }
  s.packed_bpr = bpr;
  HIP_TRY(h, hipGetLastError());
  s.n_reads = n, s.n_bases = n_bases, s.max_len = len;
  s.staged = true, s.mapped = false, s.synced = false;
  s.h2d_bytes = total, s.sent_packed = true;
  s.chars_ready = at_commit, s.offs_ready = offs_at_commit, s.n_exc = n_exc;
  return FEM_OK;
}

// The trim stage of the batch fem_dev_map_staged is about to map, on the slot's stream in front of the selection: the slot's
// settings become the batch's; the cut producers that are on run first (adapter_match_kernel, pair_overlap_kernel) and hand
// trim_clip_kernel their cuts, of which it takes the larger; it makes the clip points and kept lengths, their scan the mapping
// view's offsets, trim_gather_kernel its characters; every producer's two counters go home behind them.  Any one setting makes
// the batch a trimmed one.  With nothing set it launches nothing.
int enqueue_trim(fem_dev *h, Slot &s) {
  const PrepSettings &b = s.prep_batch = s.prep;
  s.view.trimmed = false;
  for (Cuts &c : s.cuts) c.home = false;
  if (!b.any()) return FEM_OK;
  const bool adapter = b.adapter.on, overlap = b.overlap.on;
  if (overlap && !s.opt.paired) return fail(h, FEM_ERR_STATE, "the mates' overlap (fem_dev_set_pair_overlap) needs the slot in pair mode (fem_dev_set_pairs)");
  if (s.sent_packed) {
    // (the setters are named in the table's order up to the last one that is on)
    int last = kTrim;
    for (int k = 0; k < kCutKinds; ++k)
      if (b.has(k)) last = k;
    std::string setters;
    for (int k = 0; k <= last; ++k) setters += (k ? ", " : "") + std::string(kCutRows[k].setter);
    return fail(h, FEM_ERR_UNSUPPORTED, "trimming (" + setters + ") reads a batch staged as characters, not a packed one (fem_dev_commit_stage_packed)");
  }
  if (b.trim.qual > 0 && (!s.text_staged || s.host_quals))
    return fail(h, FEM_ERR_STATE, "quality trimming (fem_dev_set_trim) needs the batch's qualities on the device before it is mapped (fem_dev_commit_text_stage)");
  const size_t n = (size_t)s.n_reads;
  Cuts &clips = s.cuts[kTrim], &adapt3 = s.cuts[kAdapter], &over3 = s.cuts[kOverlap];
  HIP_TRY(h, s.view.d_bases_alloc.ensure(kFrontPad + (size_t)s.n_bases + 64));
  HIP_TRY(h, s.view.d_off.ensure(n + 1));
  HIP_TRY(h, s.view.d_keep.ensure(n + 1));
  for (int k = 0; k < kCutKinds; ++k)
    if (b.has(k)) HIP_TRY(h, s.cuts[k].size(n));
  size_t scan_bytes = 0;
  HIP_TRY(h, rocprim::exclusive_scan(nullptr, scan_bytes, s.view.d_keep.get(), s.view.d_off.get(), (uint64_t)0, n + 1, rocprim::plus<uint64_t>(), s.stream.s));
  HIP_TRY(h, s.view.d_scan_tmp.ensure(std::max<size_t>(scan_bytes, 16)));
  scan_bytes = s.view.d_scan_tmp.size();
  if (b.trim.qual > 0) HIP_TRY(h, hipStreamWaitEvent(s.stream, s.ev_text_staged, 0));  // (the qualities came on the slot's text stream)
  for (int k = 0; k < kCutKinds; ++k)
    if (b.has(k)) HIP_TRY(h, s.cuts[k].zero_counts(s.stream));
  femtr::TrimParams tp{};
  tp.quals = b.trim.qual > 0 ? s.d_quals.get() : nullptr, tp.read_off = s.d_off, tp.n_reads = (uint32_t)n;
  tp.trim5 = b.trim.trim5, tp.trim3 = b.trim.trim3, tp.qual = b.trim.qual;
  tp.clip5 = clips.d[0], tp.clip3 = clips.d[1], tp.keep = s.view.d_keep, tp.ctr = clips.d_ctr;
  tp.adapt3 = adapter ? adapt3.d[0].get() : nullptr, tp.over3 = overlap ? over3.d[0].get() : nullptr;
  femad::AdapterParams ap{};
  if (adapter) {
    ap.bases = s.bases(), ap.read_off = s.d_off, ap.n_reads = (uint32_t)n;
    ap.second_begin = s.opt.paired ? (uint32_t)(n / 2) : (uint32_t)n;  // (pair mode: the second half are the mates 2)
    ap.trim5 = b.trim.trim5, ap.trim3 = b.trim.trim3;
    ap.min_overlap = b.adapter.min_overlap, ap.err_pct = b.adapter.err_pct;
    memcpy(ap.occ, b.adapter.occ, sizeof ap.occ);
    ap.len[0] = b.adapter.len[0], ap.len[1] = b.adapter.len[1];
    ap.adapt3 = adapt3.d[0], ap.ctr = adapt3.d_ctr;
  }
  femov::OverlapParams vp{};
  if (overlap) {
    vp.bases = s.bases(), vp.read_off = s.d_off, vp.n_reads = (uint32_t)n;
    vp.trim5 = b.trim.trim5, vp.trim3 = b.trim.trim3;
    vp.min_overlap = b.overlap.min_overlap, vp.err_pct = b.overlap.err_pct;
    vp.over3 = over3.d[0], vp.ctr = over3.d_ctr;
  }
  const uint32_t grid_pairs = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n / 2 + femov::kWaves - 1) / femov::kWaves, (uint64_t)h->n_cu * 8u));  // (a pair per wave)
  const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + 3) / 4, (uint64_t)h->n_cu * 8u));  // (four reads per block)
  hipError_t scan_rc = hipSuccess;
  // (kernel id 19: the steps of the stage as one entry)
  const int rc = timed_launch(h, s, 19, s.stream, true, [&] {
    if (adapter) hipLaunchKernelGGL(femad::adapter_match_kernel, dim3(grid), dim3(256), 0, s.stream, ap);
    if (overlap) hipLaunchKernelGGL(femov::pair_overlap_kernel, dim3(grid_pairs), dim3(64 * femov::kWaves), 0, s.stream, vp);
    hipLaunchKernelGGL(femtr::trim_clip_kernel, dim3(grid), dim3(256), 0, s.stream, tp);
    scan_rc = rocprim::exclusive_scan(s.view.d_scan_tmp.get(), scan_bytes, s.view.d_keep.get(), s.view.d_off.get(), (uint64_t)0, n + 1, rocprim::plus<uint64_t>(), s.stream.s);
    if (n && scan_rc == hipSuccess)
      hipLaunchKernelGGL(femtr::trim_gather_kernel, dim3(grid), dim3(256), 0, s.stream, (const uint8_t *)s.bases(), (const uint64_t *)s.d_off.get(),
                         (const uint16_t *)clips.d[0].get(), (const uint64_t *)s.view.d_off.get(), (uint32_t)n, s.view.d_bases_alloc + kFrontPad);
  });
  HIP_TRY(h, scan_rc);
  if (rc) return rc;
  for (int k = 0; k < kCutKinds; ++k)
    if (b.has(k)) HIP_TRY(h, s.cuts[k].counts_home(s.stream));
  s.view.trimmed = true;
  return FEM_OK;
}

// fem_dev_fetch_trim, _adapter, _pair_overlap: a producer's cuts of the slot's mapped batch, copied home at the batch's first fetch
int fetch_cuts(fem_dev *h, int slot, int kind, const uint16_t **first, const uint16_t **second, uint64_t *n_reads) {
  int rc = fem_dev_sync(h, slot);
  if (rc) return rc;
  Slot &s = h->slot[slot];
  if (!s.view.trimmed || !s.prep_batch.has(kind))
    return fail(h, FEM_ERR_STATE, std::string("the slot's batch was mapped without ") + kCutRows[kind].what + " (" + kCutRows[kind].setter + ")");
  Cuts &c = s.cuts[kind];
  HIP_TRY(h, c.fetch((size_t)s.n_reads, s.stream));
  if (first) *first = c.h[0];
  if (second) *second = c.h[1];
  if (n_reads) *n_reads = s.n_reads;
  return FEM_OK;
}

// fem_dev_trim_count, _adapter_count, _pair_overlap_count: its two counters, 0 when the batch was mapped without it
int cut_counts(fem_dev *h, int slot, int kind, uint64_t *n_cut, uint64_t *n_bases) {
  int rc = fem_dev_sync(h, slot);
  if (rc) return rc;
  const Slot &s = h->slot[slot];
  const bool on = s.view.trimmed && s.prep_batch.has(kind);
  if (n_cut) *n_cut = on ? s.cuts[kind].h_ctr[0] : 0;
  if (n_bases) *n_bases = on ? s.cuts[kind].h_ctr[1] : 0;
  return FEM_OK;
}

unsigned stage_threads(uint64_t n_reads) {
  unsigned want = 12;  // (measured on the GPU box's 16-core share: 8 -> 12 threads still gains, 16 does not)
  if (const char *e = getenv("FEM_STAGE_THREADS")) want = (unsigned)std::max(1, atoi(e));
  const unsigned hw = std::thread::hardware_concurrency();
  return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>({(uint64_t)(hw ? hw : 1), (uint64_t)want, n_reads / 65536 + 1}));
}

}  // namespace

extern "C" {

const char *fem_strerror(int rc) {
  switch (rc) {
    case FEM_OK: return "ok";
    case FEM_ERR_INVALID: return "invalid argument";
    case FEM_ERR_HIP: return "HIP runtime error";
    case FEM_ERR_NOMEM: return "out of memory";
    case FEM_ERR_STATE: return "call order violated";
    case FEM_ERR_UNSUPPORTED: return "input not supported by the device path";
    case FEM_ERR_RCCL: return "RCCL error";
    default: return "unknown error";
  }
}

const char *fem_dev_last_error(const fem_dev *h) { return h ? h->err.c_str() : "null handle"; }

static std::atomic<int> g_blocking_waits{0};
int fem_set_blocking_waits(int on) {
  g_blocking_waits.store(on ? 1 : 0);
  return FEM_OK;
}

int fem_dev_open(int device, fem_dev **out) {
  if (!out) return FEM_ERR_INVALID;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return FEM_ERR_HIP;  // no GPU: fail loudly, no fallback
  if (device < 0 || device >= n) return FEM_ERR_INVALID;
  fem_dev *h = new (std::nothrow) fem_dev();
  if (!h) return FEM_ERR_NOMEM;
  h->device = device;
  if (hipSetDevice(device) != hipSuccess) {
    delete h;
    return FEM_ERR_HIP;
  }
  // Threads that wait for the device sleep instead of spinning (fem_set_blocking_waits): FEM map has a thread per batch in
  // flight waiting most of the time, on hosts where the parser wants every core (16 M reads: 15.6 -> 13.9 cores busy).
  if (g_blocking_waits.load() || testing_switch("FEM_BLOCKING_SYNC")) (void)hipSetDeviceFlags(hipDeviceScheduleBlockingSync);
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess) h->n_cu = prop.multiProcessorCount;
  for (int i = 0; i < kSlots; ++i) {
    if (h->slot[i].stream.create(hipStreamNonBlocking) != hipSuccess) {
      delete h;
      return FEM_ERR_HIP;
    }
  }
  bool ok_ev = h->ev_kernels_done.create(hipEventDisableTiming) == hipSuccess && h->ev_select_done.create(hipEventDisableTiming) == hipSuccess &&
               h->ev_h2d_done.create(hipEventDisableTiming) == hipSuccess && h->side_stream.create(hipStreamNonBlocking) == hipSuccess;
  for (int i = 0; ok_ev && i < kSlots; ++i) {
    Slot &sl = h->slot[i];
    ok_ev = sl.ev_zeroed.create(hipEventDisableTiming) == hipSuccess && sl.ev_results.create(hipEventDisableTiming) == hipSuccess &&
            sl.ev_chars.create(hipEventDisableTiming) == hipSuccess;
    for (int q = 0; ok_ev && q < kMaxParts; ++q)
      ok_ev = sl.ev_part[q].create(hipEventDisableTiming) == hipSuccess && sl.ev_sel[q].create(hipEventDisableTiming) == hipSuccess;
  }
  if (!ok_ev) {
    (void)fem_dev_close(h);
    return FEM_ERR_HIP;
  }
  // Kernel-choice and buffer-size overrides exist for the parity tests and for A/B measurements only: a production process
  // does not look at its environment for them unless FEM_TESTING=1 says so.
  if (testing_switch("FEM_TESTING")) {
    h->no_overlap = testing_switch("FEM_NO_OVERLAP");
    h->no_parts = testing_switch("FEM_NO_PARTS");
    if (const char *mp = getenv("FEM_PARTS")) h->max_parts = std::min(kMaxParts, std::max(1, atoi(mp)));
    h->timeline = testing_switch("FEM_TIMELINE");
    if (h->timeline && h->ev_epoch.create() == hipSuccess && hipEventRecord(h->ev_epoch, h->side_stream) == hipSuccess)
      h->timing = true, h->have_epoch = true;  // (a process that never asks for timing, FEM map, is timed from its handle's opening)
    h->force_generic = testing_switch("FEM_FORCE_GENERIC");
    h->force_hash = testing_switch("FEM_FORCE_HASH");
    h->force_dense = testing_switch("FEM_FORCE_DENSE");
    h->no_dense = testing_switch("FEM_NO_DENSE");
    h->no_strided = testing_switch("FEM_NO_STRIDED");
    h->verify_chars = testing_switch("FEM_VERIFY_CHARS");
    h->select_chars = testing_switch("FEM_SELECT_CHARS");
    h->tiny_buffers = testing_switch("FEM_TEST_TINY_BUFFERS");
    if (const char *bl = getenv("FEM_TEST_BANK_BASES")) h->bank_limit = strtoull(bl, nullptr, 10);
    if (const char *bs = getenv("FEM_TEST_BANK_SEQS")) h->bank_seqs = (uint32_t)strtoul(bs, nullptr, 10);
  }
  *out = h;
  return FEM_OK;
}

int fem_dev_close(fem_dev *h) {
  if (!h) return FEM_ERR_INVALID;
  {
    std::lock_guard<std::mutex> lock(g_comm_mu);
    if (g_comm && std::find(g_comm->devs.begin(), g_comm->devs.end(), h->device) != g_comm->devs.end()) destroy_comm_set();
  }
  (void)hipSetDevice(h->device);
  (void)hipDeviceSynchronize();
  for (auto &s : h->slot) drain_timing(h, s);  // (the timing events go back to the pool)
  delete h;  // every buffer, event and stream of the handle and its slots frees itself (fem_buf.hip.h)
  return FEM_OK;
}

int fem_dev_limits(const fem_dev *h, uint32_t *max_read_len, int32_t *n_slots) {
  if (!h) return FEM_ERR_INVALID;
  if (max_read_len) *max_read_len = kMaxReadLen;
  if (n_slots) *n_slots = kSlots;
  return FEM_OK;
}

int fem_dev_upload_index(fem_dev *h, int32_t k, int32_t step, const uint32_t *lookup, uint64_t n_lookup,
                         const uint64_t *occ, uint64_t n_occ) {
  if (!h || !lookup || (!occ && n_occ)) return FEM_ERR_INVALID;
  if (k < 1 || k > 15 || step < 1) return fail(h, FEM_ERR_INVALID, "k must be 1..15 and step >= 1");
  if (n_lookup != (1ull << (2 * k)) + 1) return fail(h, FEM_ERR_INVALID, "lookup table must have 4^k + 1 entries");
  if (n_occ > 0xFFFFFFFFull) return fail(h, FEM_ERR_INVALID, "occurrence table larger than its uint32 prefix sums");
  HIP_TRY(h, hipSetDevice(h->device));
  h->d_lookup.release(), h->d_occ.release();
  HIP_TRY(h, h->d_lookup.ensure(n_lookup));
  HIP_TRY(h, h->d_occ.ensure(std::max<uint64_t>(n_occ, 1)));
  HIP_TRY(h, hipMemcpy(h->d_lookup, lookup, n_lookup * sizeof(uint32_t), hipMemcpyHostToDevice));
  if (n_occ) HIP_TRY(h, hipMemcpy(h->d_occ, occ, n_occ * sizeof(uint64_t), hipMemcpyHostToDevice));
  h->n_lookup = n_lookup, h->n_occ = n_occ, h->k = k, h->step = step;
  int rc = refresh_summary(h);
  return rc ? rc : refresh_dense(h);
}

namespace {
// The reference as base codes 0..4 (what the bit planes and the index build are made from) in a buffer of its own, from the
// resident characters.  A temporary: nothing on the mapping path reads it, so it is not kept (3 GB at 3 Gbp).
int make_codes(fem_dev *h, Buf<uint8_t> *codes) {
  const uint64_t total = h->ref_bytes;
  HIP_TRY(h, codes->ensure(total + 128));
  HIP_TRY(h, hipMemcpy(*codes, h->d_ref_raw, total, hipMemcpyDeviceToDevice));
  HIP_TRY(h, hipMemset(*codes + total, 4, 128));
  if (total) {
    hipLaunchKernelGGL(femk::ref_encode_kernel, dim3((uint32_t)h->n_cu * 8u), dim3(256), 0, 0, codes->get(), total);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipDeviceSynchronize());
  }
  return FEM_OK;
}
}  // namespace

int fem_dev_upload_reference(fem_dev *h, uint32_t n_seq, const char *const *seq, const uint32_t *seq_len) {
  if (!h || !seq || !seq_len || n_seq == 0) return FEM_ERR_INVALID;
  HIP_TRY(h, hipSetDevice(h->device));
  h->seq_off.assign(n_seq, 0);
  h->seq_len.assign(seq_len, seq_len + n_seq);
  uint64_t total = 0;
  for (uint32_t i = 0; i < n_seq; ++i) {
    h->seq_off[i] = total;
    total += seq_len[i];
  }
  auto drop_reference = [&]() {
    h->d_ref_raw.release(), h->d_seq_off.release(), h->d_seq_len.release(), h->d_planes.release();
    h->ref_bytes = 0, h->n_seq = 0;
    h->coverage = fem_dev::Coverage{};  // (the track's windows were the old reference's: off)
  };
  if (h->coverage.on) HIP_TRY(h, hipDeviceSynchronize());  // (a text that was not waited for may still be adding to the bins that go)
  drop_reference();
  // 64 bytes of slack so that 4-byte window reads at the very end stay inside the allocation
  HIP_TRY(h, h->d_ref_raw.ensure(total + 128));
  HIP_TRY(h, h->d_seq_off.ensure(n_seq));
  HIP_TRY(h, h->d_seq_len.ensure(n_seq));
  for (uint32_t i = 0; i < n_seq; ++i)
    if (seq_len[i]) HIP_TRY(h, hipMemcpy(h->d_ref_raw + h->seq_off[i], seq[i], seq_len[i], hipMemcpyHostToDevice));
  // (the slack zeroed, as the oracle pads its concatenation: a traceback whose 'S' fold walks past the last sequence reads it)
  HIP_TRY(h, hipMemset(h->d_ref_raw + total, 0, 128));
  HIP_TRY(h, hipMemcpy(h->d_seq_off, h->seq_off.data(), n_seq * sizeof(uint64_t), hipMemcpyHostToDevice));
  HIP_TRY(h, hipMemcpy(h->d_seq_len, h->seq_len.data(), n_seq * sizeof(uint32_t), hipMemcpyHostToDevice));
  HIP_TRY(h, hipMemset(h->d_ref_raw + total, 'N', 128));
  h->ref_bytes = total, h->n_seq = n_seq;
  {  // bit planes of the codes, 64 bases of slack (code 4) included; the codes themselves are not kept
    // (a failure from here on must not leave a reference without its planes behind: fem_dev_map_staged and
    //  fem_dev_build_index test d_ref_raw)
    Buf<uint8_t> codes;
    int rc = make_codes(h, &codes);
    if (rc) {
      drop_reference();
      return rc;
    }
    const uint64_t n_pb = (total + 64 + 7) / 8;
    hipError_t e = h->d_planes.ensure(femk::plane_bytes(n_pb));
    if (e == hipSuccess) e = hipMemset(h->d_planes, 0, femk::plane_bytes(n_pb));
    if (e == hipSuccess) {
      hipLaunchKernelGGL(femk::ref_planes_kernel, dim3((uint32_t)h->n_cu * 8u), dim3(256), 0, 0, codes.get(), h->d_ref_raw.get(), n_pb, h->d_planes.get());
      e = hipGetLastError();
      if (e == hipSuccess) e = hipDeviceSynchronize();
    }
    if (e != hipSuccess) drop_reference();
    HIP_TRY(h, e);
  }
  return refresh_dense(h);
}

int fem_dev_build_index(fem_dev *h, int32_t k, int32_t step, uint32_t *lookup_out, uint64_t *occ_out, uint64_t occ_cap,
                        uint64_t *n_occ_out) {
  if (!h) return FEM_ERR_INVALID;
  if (!h->d_ref_raw) return fail(h, FEM_ERR_STATE, "upload the reference before building the index");
  if (k < 1 || k > 15 || step < 1) return fail(h, FEM_ERR_INVALID, "k must be 1..15 and step >= 1");
  HIP_TRY(h, hipSetDevice(h->device));
  h->d_lookup.release(), h->d_occ.release();
  uint64_t n_occ = 0;
  std::string err;
  Buf<uint8_t> codes;  // (base codes of the reference: made for the build, not kept)
  int rc = make_codes(h, &codes);
  if (rc) return rc;
  rc = femix::build_index(codes, h->seq_off, h->seq_len, k, step, h->n_cu, &h->d_lookup, &h->d_occ, &n_occ, &err);
  codes.release();
  if (rc != FEM_OK) return fail(h, rc, err);
  h->n_lookup = (1ull << (2 * k)) + 1, h->n_occ = n_occ, h->k = k, h->step = step;
  if ((rc = refresh_summary(h))) return rc;
  if ((rc = refresh_dense(h))) return rc;
  if (n_occ_out) *n_occ_out = n_occ;
  if (lookup_out)
    HIP_TRY(h, hipMemcpy(lookup_out, h->d_lookup, h->n_lookup * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (occ_out) {
    if (occ_cap < n_occ) return fail(h, FEM_ERR_INVALID, "occ_out too small");
    if (n_occ) HIP_TRY(h, hipMemcpy(occ_out, h->d_occ, n_occ * sizeof(uint64_t), hipMemcpyDeviceToHost));
  }
  return FEM_OK;
}

int fem_dev_fetch_index(fem_dev *h, uint32_t *lookup_out, uint64_t *occ_out, uint64_t occ_cap) {
  if (!h) return FEM_ERR_INVALID;
  if (!h->d_lookup) return fail(h, FEM_ERR_STATE, "no index is resident");
  HIP_TRY(h, hipSetDevice(h->device));
  if (lookup_out) HIP_TRY(h, hipMemcpy(lookup_out, h->d_lookup, h->n_lookup * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (occ_out) {
    if (occ_cap < h->n_occ) return fail(h, FEM_ERR_INVALID, "occ_out too small");
    if (h->n_occ) HIP_TRY(h, hipMemcpy(occ_out, h->d_occ, h->n_occ * sizeof(uint64_t), hipMemcpyDeviceToHost));
  }
  return FEM_OK;
}

int fem_dev_acquire_stage(fem_dev *h, int slot, uint64_t n_reads_cap, uint64_t n_bases_cap, char **bases, uint64_t **offsets) {
  int rc = check_slot(h, slot);
  if (rc) return rc;
  FEM_LOCK(h);
  if (!bases || !offsets) return fail(h, FEM_ERR_INVALID, "null output pointer");
  if (n_reads_cap > 0x3FFFFFF0ull) return fail(h, FEM_ERR_UNSUPPORTED, "more than 2^30 reads in one batch");
  Slot &s = h->slot[slot];
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipStreamSynchronize(s.stream));  // the previous batch's copy out of these buffers is done
  if (s.out_stream) HIP_TRY(h, hipStreamSynchronize(s.out_stream));  // ... and its records and text (they read the slot's device arrays)
  drain_timing(h, s);
  HIP_TRY(h, s.h_bases.ensure((size_t)n_bases_cap + 64));
  HIP_TRY(h, s.h_off.ensure((size_t)n_reads_cap + 1));
  s.staged = false, s.mapped = false, s.synced = false, s.text_staged = false;
  s.acq_reads = n_reads_cap, s.acq_bases = n_bases_cap;
  *bases = s.h_bases, *offsets = s.h_off;
  return FEM_OK;
}

int fem_dev_commit_stage(fem_dev *h, int slot, uint64_t n_reads, uint32_t max_len) {
  int rc = check_slot(h, slot);
  if (rc) return rc;
  FEM_LOCK(h);
  Slot &s = h->slot[slot];
  if (!s.h_bases || !s.h_off) return fail(h, FEM_ERR_STATE, "acquire the slot's staging buffers first");
  if (n_reads > s.acq_reads) return fail(h, FEM_ERR_INVALID, "more reads than the staging buffers were acquired for");
  if (max_len > kMaxReadLen)
    return fail(h, FEM_ERR_UNSUPPORTED, "read longer than the device path supports (" + std::to_string(kMaxReadLen) + ")");
  const uint64_t n_bases = n_reads ? s.h_off[n_reads] : 0;
  if (n_reads && (s.h_off[0] != 0 || n_bases > s.acq_bases)) return fail(h, FEM_ERR_INVALID, "staged offsets must start at 0 and end inside the buffer");
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, s.d_bases_alloc.ensure(kFrontPad + (size_t)n_bases + 64));
  HIP_TRY(h, s.d_off.ensure((size_t)n_reads + 1));
  if ((rc = h2d_begin(h, s))) return rc;
  if (n_bases) HIP_TRY(h, hipMemcpyAsync(s.bases(), s.h_bases, n_bases, hipMemcpyHostToDevice, s.stream));
  if (n_reads) HIP_TRY(h, hipMemcpyAsync(s.d_off, s.h_off, (n_reads + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s.stream));
  if ((rc = h2d_end(h, s))) return rc;
  s.parts = 1;
  s.n_reads = n_reads, s.n_bases = n_bases, s.max_len = max_len;
  s.staged = true, s.mapped = false, s.synced = false;
  s.h2d_bytes = n_bases + (n_reads ? (n_reads + 1) * sizeof(uint64_t) : 0), s.sent_packed = false, s.chars_ready = true, s.offs_ready = true, s.n_exc = 0, s.staged_by_copy = false;
  return FEM_OK;
}

int fem_dev_commit_stage_uniform(fem_dev *h, int slot, uint64_t n_reads, uint32_t read_len) {
  int rc = check_slot(h, slot);
  if (rc) return rc;
  FEM_LOCK(h);
  Slot &s = h->slot[slot];
  if (!s.h_bases) return fail(h, FEM_ERR_STATE, "acquire the slot's staging buffers first");
  if (read_len > kMaxReadLen)
    return fail(h, FEM_ERR_UNSUPPORTED, "read longer than the device path supports (" + std::to_string(kMaxReadLen) + ")");
  const uint64_t n_bases = n_reads * (uint64_t)read_len;
  if (n_reads > s.acq_reads || n_bases > s.acq_bases) return fail(h, FEM_ERR_INVALID, "more reads than the staging buffers were acquired for");
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, s.d_bases_alloc.ensure(kFrontPad + (size_t)n_bases + 64));
  HIP_TRY(h, s.d_off.ensure((size_t)n_reads + 1));
  if ((rc = h2d_begin(h, s))) return rc;
  if (n_bases) HIP_TRY(h, hipMemcpyAsync(s.bases(), s.h_bases, n_bases, hipMemcpyHostToDevice, s.stream));
  if ((rc = h2d_end(h, s))) return rc;
  s.parts = 1;
  hipLaunchKernelGGL(femk::uniform_offsets_kernel, dim3((uint32_t)std::min<uint64_t>((n_reads + 256) / 256, (uint64_t)h->n_cu * 8u)), dim3(256), 0,
                     s.stream, s.d_off, n_reads, read_len);
  HIP_TRY(h, hipGetLastError());
  s.n_reads = n_reads, s.n_bases = n_bases, s.max_len = read_len;
  s.staged = true, s.mapped = false, s.synced = false;
  s.h2d_bytes = n_bases, s.sent_packed = false, s.chars_ready = true, s.offs_ready = true, s.n_exc = 0, s.staged_by_copy = false;
  return FEM_OK;
}

int fem_dev_packed_layout(uint64_t n_reads, uint32_t read_len, uint32_t *bytes_per_read, uint64_t *exc_offset, uint64_t *exc_cap) {
  if (read_len == 0 || read_len > kMaxReadLen) return FEM_ERR_INVALID;
  const uint64_t n_bases = n_reads * (uint64_t)read_len, cb = fempack::code_bytes(n_reads, read_len);
  if (bytes_per_read) *bytes_per_read = fempack::bytes_per_read(read_len);
  if (exc_offset) *exc_offset = cb;
  // what a staging buffer acquired for n_reads * read_len characters has left behind the codes, and never more than one
  // byte in sixteen (beyond that the characters themselves are the smaller message: fem_dev_commit_stage_uniform)
  if (exc_cap) *exc_cap = std::min<uint64_t>((n_bases + 64 - std::min<uint64_t>(cb, n_bases + 64)) / 5u, n_bases / 16u);
  return FEM_OK;
}

int fem_dev_commit_stage_packed(fem_dev *h, int slot, uint64_t n_reads, uint32_t read_len, uint64_t n_exceptions) {
  int rc = check_slot(h, slot);
  if (rc) return rc;
  FEM_LOCK(h);
  Slot &s = h->slot[slot];
  if (!s.h_bases) return fail(h, FEM_ERR_STATE, "acquire the slot's staging buffers first");
  if (read_len == 0 && n_reads) return fail(h, FEM_ERR_INVALID, "packed batches hold reads of one non-zero length");
  if (read_len > kMaxReadLen)
    return fail(h, FEM_ERR_UNSUPPORTED, "read longer than the device path supports (" + std::to_string(kMaxReadLen) + ")");
  const uint64_t n_bases = n_reads * (uint64_t)read_len;
  if (n_reads > s.acq_reads || n_bases > s.acq_bases) return fail(h, FEM_ERR_INVALID, "more reads than the staging buffers were acquired for");
  if (n_bases >= 0xFFFFFFF0ull) return fail(h, FEM_ERR_UNSUPPORTED, "a packed batch holds fewer than 2^32 bases; split the batch");
  const uint64_t code_bytes = fempack::code_bytes(n_reads, read_len);
  if (code_bytes + n_exceptions * 5u > s.acq_bases + 64 || n_exceptions > n_bases / 16u)
    return fail(h, FEM_ERR_INVALID, "more exceptions than a packed batch may carry (fem_dev_packed_layout): commit the characters instead");
  // the positions are the one thing here a wrong value of which would make a kernel write outside its buffers
  const uint32_t *pos = (const uint32_t *)(s.h_bases + code_bytes);
  for (uint64_t i = 0; i < n_exceptions; ++i)
    if (pos[i] >= n_bases) return fail(h, FEM_ERR_INVALID, "exception position outside the batch");
  HIP_TRY(h, hipSetDevice(h->device));
  if ((rc = enqueue_packed(h, s, n_reads, read_len, n_exceptions))) return rc;
  s.staged_by_copy = true;  // (a quarter of the characters' bytes go out: the results may come home behind the kernels, launch_batch)
  return FEM_OK;
}

int fem_dev_stage_reads(fem_dev *h, int slot, const fem_read_batch *reads) {
  int rc = check_slot(h, slot);
  if (rc) return rc;
  if (!reads || (reads->n_reads && (!reads->bases || !reads->offsets))) return fail(h, FEM_ERR_INVALID, "null read batch");
  if (reads->n_reads > 0x3FFFFFF0ull) return fail(h, FEM_ERR_UNSUPPORTED, "more than 2^30 reads in one batch");
  const uint64_t n = reads->n_reads;
  const uint64_t base0 = n ? reads->offsets[0] : 0;
  if (n && reads->offsets[n] < base0) return fail(h, FEM_ERR_INVALID, "read offsets must be ascending");
  const uint64_t n_bases = n ? reads->offsets[n] - base0 : 0;
  char *hb = nullptr;
  uint64_t *ho = nullptr;
  if ((rc = fem_dev_acquire_stage(h, slot, n, n_bases, &hb, &ho))) return rc;
  Slot &s = h->slot[slot];
  const unsigned n_thr = stage_threads(n);
  if (!h->stage_pool) h->stage_pool.reset(new (std::nothrow) StagePool());
  if (!h->stage_pool) return fail(h, FEM_ERR_NOMEM, "out of host memory");
  auto run_threads = [&](unsigned nt, const std::function<void(unsigned)> &work) { h->stage_pool->run(nt, work); };
  // ---- pass 1 (a few host threads): order, longest and shortest read ----
  std::vector<uint32_t> t_max(n_thr, 0), t_min(n_thr, 0xFFFFFFFFu);
  std::atomic<int> bad{0};
  run_threads(n_thr, [&](unsigned t) {
    const uint64_t r_lo = n * t / n_thr, r_hi = n * (t + 1) / n_thr;
    uint32_t mx = 0, mn = 0xFFFFFFFFu;
    for (uint64_t i = r_lo; i < r_hi; ++i) {
      const uint64_t o0 = reads->offsets[i], o1 = reads->offsets[i + 1];
      if (o1 < o0) {
        bad.store(1);
        return;
      }
      const uint64_t len = o1 - o0;
      if (len > kMaxReadLen) {
        bad.store(2);
        return;
      }
      mx = std::max<uint32_t>(mx, (uint32_t)len), mn = std::min<uint32_t>(mn, (uint32_t)len);
    }
    t_max[t] = mx, t_min[t] = mn;
  });
  if (bad.load() == 1) return fail(h, FEM_ERR_INVALID, "read offsets must be ascending");
  if (bad.load() == 2)
    return fail(h, FEM_ERR_UNSUPPORTED, "read longer than the device path supports (" + std::to_string(kMaxReadLen) + ")");
  uint32_t max_len = 0, min_len = 0xFFFFFFFFu;
  for (unsigned t = 0; t < n_thr; ++t) max_len = std::max(max_len, t_max[t]), min_len = std::min(min_len, t_min[t]);
  // ---- reads of one length: two bits per base cross the link instead of eight ----
  // (test hook, read per batch on purpose: tests/test_gpu_packed.py switches it between two batches of one handle; one
  // getenv per batch of >= 10^4 reads is not measurable)
  // (a slot with trimming, an adapter or the mates' overlap set stages its batches as characters: the trim stage reads and gathers them)
  const bool no_pack = testing_switch("FEM_NO_PACK") || h->slot[slot].prep.any();
  if (n && min_len == max_len && max_len > 0 && n_bases < 0xFFFFFFF0ull && !no_pack) {
    const uint32_t len = max_len, bpr = (len + 3u) / 4u;
    const uint64_t code_bytes = (n * bpr + 7u) & ~7ull;
    const uint64_t exc_cap = (n_bases + 64 - std::min<uint64_t>(code_bytes, n_bases + 64)) / 5u;  // what is left of the staging buffer
    std::vector<std::vector<uint64_t>> exc(n_thr);
    const uint8_t *src = (const uint8_t *)reads->bases + base0;
    // (pieces of 32 Ki reads handed out as the threads ask for them: one thread held up by the host's other tenants
    // holds up its piece, not a twelfth of the batch)
    constexpr uint64_t kPiece = 32768;
    std::atomic<uint64_t> next_piece{0};
    run_threads(n_thr, [&](unsigned t) {
      for (;;) {
        const uint64_t r_lo = next_piece.fetch_add(1, std::memory_order_relaxed) * kPiece;
        if (r_lo >= n) break;
        const uint64_t r_hi = std::min(n, r_lo + kPiece);
        if ((len & 3u) == 0u) {  // no padding: the piece's reads are one stream
          pack_bases(src + r_lo * len, (r_hi - r_lo) * len, (uint8_t *)hb + r_lo * bpr, r_lo * len, exc[t]);
        } else {
          for (uint64_t i = r_lo; i < r_hi; ++i) pack_bases(src + i * len, len, (uint8_t *)hb + i * bpr, i * len, exc[t]);
        }
      }
    });
    uint64_t n_exc = 0;
    for (const auto &v : exc) n_exc += v.size();
    if (n_exc <= exc_cap && n_exc <= n_bases / 16u) {  // (more than that and the characters themselves are the smaller message)
      // codes | positions (uint32 each) | the bytes that belong there
      uint32_t *he = (uint32_t *)(hb + code_bytes);
      uint8_t *hc = (uint8_t *)(he + n_exc);
      for (const auto &v : exc)
        for (uint64_t x : v) *he++ = (uint32_t)(x >> 8), *hc++ = (uint8_t)x;
      {
        FEM_LOCK(h);
        if ((rc = enqueue_packed(h, s, n, len, n_exc))) return rc;
      }
      s.staged_by_copy = true;
      return FEM_OK;
    }
  }
  // ---- any other batch: the characters and the offsets as they are ----
  run_threads(n_thr, [&](unsigned t) {
    const uint64_t r_lo = n * t / n_thr, r_hi = n * (t + 1) / n_thr;
    for (uint64_t i = r_lo; i < r_hi; ++i) ho[i] = reads->offsets[i] - base0;
    if (r_hi == n) ho[n] = reads->offsets[n] - base0;
    if (r_hi > r_lo) memcpy(hb + (reads->offsets[r_lo] - base0), reads->bases + reads->offsets[r_lo], reads->offsets[r_hi] - reads->offsets[r_lo]);
  });
  if (n == 0) ho[0] = 0;
  rc = fem_dev_commit_stage(h, slot, n, max_len);
  s.staged_by_copy = true;
  return rc;
}

int fem_dev_stage_info(fem_dev *h, int slot, uint64_t *h2d_bytes, int32_t *packed) {
  int rc = check_slot(h, slot);
  if (rc) return rc;
  if (h2d_bytes) *h2d_bytes = h->slot[slot].h2d_bytes;
  if (packed) *packed = h->slot[slot].sent_packed ? 1 : 0;
  return FEM_OK;
}

int fem_dev_stage_front(fem_dev *h, int slot, int32_t *select_packed, int32_t *chars_ready) {
  int rc = check_slot(h, slot);
  if (rc) return rc;
  if (select_packed) *select_packed = h->slot[slot].select_packed ? 1 : 0;
  if (chars_ready) *chars_ready = h->slot[slot].chars_ready ? 1 : 0;
  return FEM_OK;
}

int fem_dev_map_staged(fem_dev *h, int slot, const fem_params *p) {
  int rc = check_slot(h, slot);
  if (rc) return rc;
  FEM_LOCK(h);
  if (!params_ok(p)) return fail(h, FEM_ERR_INVALID, "parameters out of range (k 1..15, step 1..16, e 0..7, a 0..2)");
  if (!h->d_lookup || !h->d_ref_raw || !h->d_planes) return fail(h, FEM_ERR_STATE, "index and reference must be uploaded first");
  if (p->k != h->k) return fail(h, FEM_ERR_INVALID, "k differs from the uploaded index");
  Slot &s = h->slot[slot];
  if (!s.staged) return fail(h, FEM_ERR_STATE, "no reads staged in this slot");
  HIP_TRY(h, hipSetDevice(h->device));
  s.params = *p;
  if ((rc = ensure_outputs(h, s))) return rc;
  if ((rc = enqueue_trim(h, s))) return rc;
  return launch_batch(h, s);
}

int fem_dev_sync(fem_dev *h, int slot) {
  int rc = check_slot(h, slot);
  if (rc) return rc;
  Slot &s = h->slot[slot];
  if (!s.mapped) return fail(h, FEM_ERR_STATE, "nothing was mapped in this slot");
  HIP_TRY(h, hipSetDevice(h->device));  // the callers (fetch, fetch_records) allocate and launch on this device
  if (s.synced) return FEM_OK;
  for (int attempt = 0; attempt < 8; ++attempt) {
    HIP_TRY(h, hipStreamSynchronize(s.stream));  // (without the handle's lock: other slots' calls go on meanwhile)
    FEM_LOCK(h);
    drain_timing(h, s);
    const CtlBlock *ctl = ctl_home(s);
    uint32_t flags = ctl->ctr[1];
    if (flags & femk::kFlagTooLarge)
      return fail(h, FEM_ERR_UNSUPPORTED, "a read selects more than 2^31 occurrence entries in one seed group");
    if (flags == 0) {
      s.n_cand = ctl->ctr[0];
      s.n_packed = ctl->pack_cursor[0], s.n_big = ctl->pack_cursor[1];
      s.stats[0] = s.n_reads;
      s.stats[1] = ctl->stats[3];
      s.stats[2] = ctl->stats[0];
      s.stats[3] = ctl->stats[1];
      s.stats[4] = ctl->stats[2];
      s.synced = true;
      return FEM_OK;
    }
    // scratch too small: grow exactly what was asked for and run the batch again
    if (flags & femk::kFlagCandOverflow) {
      uint64_t want = (uint64_t)ctl->ctr[0] + ctl->ctr[0] / 8 + 1024;
      if ((rc = grow_candidates(h, s, std::min<uint64_t>(want, 0xFFFFFFF0ull)))) return rc;
    }
    if (flags & femk::kFlagQueueOverflow) {
      uint64_t want = (uint64_t)ctl->ctr[2] + ctl->ctr[2] / 8 + 4096;
      s.d_slow.release();
      s.slow_cap = 0;
      if (s.d_slow.ensure(want) != hipSuccess) return fail(h, FEM_ERR_NOMEM, "slow-read queue does not fit in device memory");
      s.slow_cap = (uint32_t)std::min<uint64_t>(want, 0xFFFFFFF0ull);
    }
    if (flags & femk::kFlagArenaOverflow) {
      uint64_t want = ctl->arena_ctr[1] + ctl->arena_ctr[1] / 8 + 1024;
      s.d_arena.release();
      if (s.d_arena.ensure(want) != hipSuccess) {
        s.arena_cap = 0;
        return fail(h, FEM_ERR_NOMEM, "scratch arena for oversized seed lists does not fit in device memory; use smaller batches");
      }
      s.arena_cap = want;
    }
    if ((rc = launch_batch(h, s))) return rc;
  }
  return fail(h, FEM_ERR_HIP, "batch kept overflowing its scratch buffers");
}

int fem_dev_fetch_stats(fem_dev *h, int slot, uint64_t stats[5]) {
  int rc = fem_dev_sync(h, slot);
  if (rc) return rc;
  if (stats) memcpy(stats, h->slot[slot].stats, sizeof(uint64_t) * 5);
  h->slot[slot].prefetch_results = false;  // this caller takes the counters only
  return FEM_OK;
}

int fem_dev_fetch(fem_dev *h, int slot, fem_batch_result *out) {
  int rc = fem_dev_sync(h, slot);
  if (rc) return rc;
  if (!out) return fail(h, FEM_ERR_INVALID, "null result");
  Slot &s = h->slot[slot];
  const size_t n2 = (size_t)s.n_reads * 2, nc = s.n_cand;
  bool regrown = false;
  if (n2 > s.h_begin.size() || !s.h_begin) {
    regrown = true;
    HIP_TRY(h, femb::alloc_all(std::max<size_t>(n2, 2), s.h_begin, s.h_count));
  }
  if (nc > s.h_cand.size() || !s.h_cand) {
    regrown = true;
    HIP_TRY(h, femb::alloc_all(std::max<size_t>(nc + nc / 4, 1024), s.h_cand, s.h_ed, s.h_end));
  }
  // what did not come home behind the kernels already (launch_batch; nothing did if a buffer was regrown just now)
  const bool per_read_home = !regrown && s.prefetched_reads2 == n2;
  const size_t c_from = regrown ? 0 : std::min<size_t>(s.prefetched_cand, nc);
  if (n2 && !per_read_home) {
    HIP_TRY(h, hipMemcpyAsync(s.h_begin, s.d_begin, n2 * sizeof(uint32_t), hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(h, hipMemcpyAsync(s.h_count, s.d_count, n2 * sizeof(uint32_t), hipMemcpyDeviceToHost, s.stream));
  }
  if (nc > c_from) {
    HIP_TRY(h, hipMemcpyAsync(s.h_cand + c_from, s.d_cand + c_from, (nc - c_from) * sizeof(uint64_t), hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(h, hipMemcpyAsync(s.h_ed + c_from, s.d_ed + c_from, (nc - c_from) * sizeof(uint8_t), hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(h, hipMemcpyAsync(s.h_end + c_from, s.d_end + c_from, (nc - c_from) * sizeof(int16_t), hipMemcpyDeviceToHost, s.stream));
  }
  if ((n2 && !per_read_home) || nc > c_from) HIP_TRY(h, hipStreamSynchronize(s.stream));
  s.prefetch_results = true, s.last_n_cand = nc, s.want_packed = false;
  out->n_reads = s.n_reads;
  out->n_candidates = nc;
  out->cand_begin = s.h_begin, out->cand_count = s.h_count;
  out->cand = s.h_cand, out->ed = s.h_ed, out->end = s.h_end;
  memcpy(out->stats, s.stats, sizeof s.stats);
  return FEM_OK;
}

int fem_dev_fetch_packed(fem_dev *h, int slot, fem_batch_packed *out) {
  int rc = fem_dev_sync(h, slot);
  if (rc) return rc;
  if (!out) return fail(h, FEM_ERR_INVALID, "null result");
  Slot &s = h->slot[slot];
  const size_t n2 = (size_t)s.n_reads * 2, n_seg = (n2 + 255) / 256;
  if (!s.packed_enqueued && s.n_reads) {  // the slot's first packed fetch: pack now; from the next batch on it happens behind the kernels
    if ((rc = enqueue_pack(h, s, true, false))) return rc;
    HIP_TRY(h, hipMemcpyAsync(s.h_ctl, s.d_ctl, kCtlBytes, hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(h, hipStreamSynchronize(s.stream));
    s.n_packed = ctl_home(s)->pack_cursor[0], s.n_big = ctl_home(s)->pack_cursor[1];
  }
  if (s.n_big > kBigCap) return fail(h, FEM_ERR_UNSUPPORTED, "more strands with 255 candidates and more than a packed result lists: use fem_dev_fetch");
  const size_t np = s.n_reads ? s.n_packed : 0;
  bool regrown = false;
  if (np > s.h_pcand.size() || !s.h_pcand) {
    regrown = true;
    HIP_TRY(h, femb::alloc_all(std::max<size_t>(np + np / 4, 1024), s.h_pcand, s.h_ped, s.h_pend));
  }
  bool copied = false;
  if (n2 && !s.packed_per_read_home) {
    HIP_TRY(h, hipMemcpyAsync(s.h_count8, s.d_count8, n2, hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(h, hipMemcpyAsync(s.h_seg, s.d_seg, n_seg * sizeof(uint32_t), hipMemcpyDeviceToHost, s.stream));
    s.packed_per_read_home = true, copied = true;
  }
  const size_t c_from = regrown ? 0 : std::min<size_t>(s.packed_home, np);
  if (np > c_from) {
    HIP_TRY(h, hipMemcpyAsync(s.h_pcand + c_from, s.d_pcand + c_from, (np - c_from) * sizeof(uint64_t), hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(h, hipMemcpyAsync(s.h_ped + c_from, s.d_ped + c_from, (np - c_from) * sizeof(uint8_t), hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(h, hipMemcpyAsync(s.h_pend + c_from, s.d_pend + c_from, (np - c_from) * sizeof(int16_t), hipMemcpyDeviceToHost, s.stream));
    s.packed_home = np, copied = true;
  }
  if (s.n_big) {
    HIP_TRY(h, hipMemcpyAsync(s.h_big, s.d_big, (size_t)s.n_big * sizeof(uint2), hipMemcpyDeviceToHost, s.stream));
    copied = true;
  }
  if (copied) HIP_TRY(h, hipStreamSynchronize(s.stream));
  s.want_packed = true, s.last_n_packed = np;
  out->n_reads = s.n_reads;
  out->n_candidates = np;
  out->count = s.h_count8, out->seg_begin = s.h_seg;
  out->cand = s.h_pcand, out->ed = s.h_ped, out->end = s.h_pend;
  out->big = (const uint32_t *)s.h_big.get(), out->n_big = s.n_big;
  memcpy(out->stats, s.stats, sizeof s.stats);
  return FEM_OK;
}

int fem_dev_upload_reference_names(fem_dev *h, uint32_t n_seq, const char *names, const uint64_t *name_off) {
  if (!h || !names || !name_off || n_seq == 0) return FEM_ERR_INVALID;
  if (h->n_seq && n_seq != h->n_seq) return fail(h, FEM_ERR_INVALID, "as many names as reference sequences, please");
  if (name_off[n_seq] < name_off[0] || name_off[n_seq] - name_off[0] > 0xFFFFFFF0ull) return fail(h, FEM_ERR_INVALID, "name offsets out of range");
  HIP_TRY(h, hipSetDevice(h->device));
  std::vector<uint32_t> off(n_seq + 1);
  for (uint32_t i = 0; i <= n_seq; ++i) {
    if (name_off[i] < name_off[0] || (i && name_off[i] < name_off[i - 1])) return fail(h, FEM_ERR_INVALID, "name offsets must be ascending");
    off[i] = (uint32_t)(name_off[i] - name_off[0]);
  }
  h->d_ref_names.release(), h->d_ref_name_off.release();
  HIP_TRY(h, h->d_ref_names.ensure(std::max<size_t>(off[n_seq], 1)));
  HIP_TRY(h, h->d_ref_name_off.ensure(n_seq + 1));
  if (off[n_seq]) HIP_TRY(h, hipMemcpy(h->d_ref_names, names + name_off[0], off[n_seq], hipMemcpyHostToDevice));
  HIP_TRY(h, hipMemcpy(h->d_ref_name_off, off.data(), (n_seq + 1) * sizeof(uint32_t), hipMemcpyHostToDevice));
  return FEM_OK;
}

int fem_dev_acquire_text_stage(fem_dev *h, int slot, uint64_t n_reads_cap, uint64_t n_bases_cap, uint64_t n_name_bytes_cap, char **quals,
                               char **names, uint64_t **name_off) {
  int rc = check_slot(h, slot);
  if (rc) return rc;
  FEM_LOCK(h);
  if (!quals || !names || !name_off) return fail(h, FEM_ERR_INVALID, "null output pointer");
  Slot &s = h->slot[slot];
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipStreamSynchronize(s.stream));  // the previous batch's copies out of these buffers are done
  if (s.text_stream) HIP_TRY(h, hipStreamSynchronize(s.text_stream));
  if (s.out_stream) HIP_TRY(h, hipStreamSynchronize(s.out_stream));
  HIP_TRY(h, s.h_quals.ensure((size_t)n_bases_cap + 64));
  HIP_TRY(h, s.h_names.ensure((size_t)n_name_bytes_cap + 64));
  HIP_TRY(h, s.h_name_off.ensure((size_t)n_reads_cap + 1));
  s.text_staged = false;
  *quals = s.h_quals, *names = s.h_names, *name_off = s.h_name_off;
  return FEM_OK;
}

int fem_dev_reserve_text(fem_dev *h, int slot, uint64_t n_reads, uint64_t n_bases, uint64_t n_name_bytes, uint64_t text_bytes) {
  int rc = check_slot(h, slot);
  if (rc) return rc;
  FEM_LOCK(h);
  Slot &s = h->slot[slot];
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, s.d_bases_alloc.ensure(kFrontPad + (size_t)n_bases + 64));
  HIP_TRY(h, s.d_off.ensure((size_t)n_reads + 1));
  HIP_TRY(h, s.d_quals.ensure((size_t)n_bases + 64));
  HIP_TRY(h, s.d_names.ensure((size_t)n_name_bytes + 64));
  HIP_TRY(h, s.d_name_off.ensure((size_t)n_reads + 1));
  if (!s.tail) s.tail.reset(new (std::nothrow) femt::Tail());
  if (!s.tail) return fail(h, FEM_ERR_NOMEM, "out of host memory");
  std::string err;
  if ((rc = s.tail->reserve_text(text_bytes, &err))) return fail(h, rc, err);
  return FEM_OK;
}

// The stream a batch's records and text are made on.  The mapping has been waited for by then (fem_dev_sync), so nothing ties
// this work to the slot's own stream — and on that stream, at the same priority as every other slot's, the small kernels of a
// batch on its way OUT queue behind the joins of the batches coming IN (a join's persistent blocks fill the chip): with more
// batches in flight each took longer, finished out of order and kept its slot (FEM map, 8 slots: a batch's records 56 ms after
// its submission).  At high priority the oldest batch's kernels take the first resources that come free.
static hipStream_t out_stream_of(fem_dev *h, Slot &s) {
  static const bool plain = testing_switch("FEM_NO_OUT_PRIORITY");  // (A/B)
  if (plain) return s.stream;
  if (!s.out_stream) {
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess || s.out_stream.create(hipStreamNonBlocking, greatest) != hipSuccess)
      s.out_stream.s = nullptr;
  }
  (void)h;
  return s.out_stream ? s.out_stream : s.stream;
}

int fem_dev_reserve_batch(fem_dev *h, int slot, uint64_t n_reads, uint64_t n_records, uint32_t max_len, const fem_params *p) {
  int rc = check_slot(h, slot);
  if (rc) return rc;
  FEM_LOCK(h);
  if (!params_ok(p)) return fail(h, FEM_ERR_INVALID, "parameters out of range (k 1..15, step 1..16, e 0..7, a 0..2)");
  if (!h->d_lookup) return fail(h, FEM_ERR_STATE, "the index must be uploaded first (what a batch needs depends on it)");
  if (n_reads == 0 || n_reads > 0x7FFFFFF0ull || n_records > 0xFFFFFFF0ull || max_len == 0 || max_len > kMaxReadLen)
    return fail(h, FEM_ERR_INVALID, "batch shape out of range");
  Slot &s = h->slot[slot];
  if (s.mapped && !s.synced) return fail(h, FEM_ERR_STATE, "a batch is in flight in this slot");
  HIP_TRY(h, hipSetDevice(h->device));
  // the mapping's own arrays: per read, per candidate (ensure_outputs sizes them by the slot's read count), the packed form's
  const uint64_t n_was = s.n_reads;
  s.n_reads = n_reads;
  rc = ensure_outputs(h, s);
  s.n_reads = n_was;
  if (rc) return rc;
  const uint64_t n_bases = n_reads * (uint64_t)max_len;
  HIP_TRY(h, s.d_packed_alloc.ensure(kPackedFrontPad + (size_t)fempack::code_bytes(n_reads, max_len) + 64));
  HIP_TRY(h, s.d_bases_alloc.ensure(kFrontPad + (size_t)n_bases + 64));
  HIP_TRY(h, s.d_off.ensure((size_t)n_reads + 1));
  HIP_TRY(h, s.d_exc_bits.ensure((size_t)n_reads / 32 + 2));
  if (const SeedPath path = seed_path(h, *p); path.dense()) {  // the selection's hand-over to the join
    HIP_TRY(h, s.d_sel.ensure((size_t)n_reads * 6u * (size_t)path.R * h->n_banks));
    HIP_TRY(h, s.d_sel_hdr.ensure((size_t)n_reads));
  }
  // the mapping tail and the SAM text's bookkeeping
  if (!s.tail) s.tail.reset(new (std::nothrow) femt::Tail());
  if (!s.tail) return fail(h, FEM_ERR_NOMEM, "out of host memory");
  std::string err;
  if ((rc = s.tail->reserve((uint32_t)n_reads, (uint32_t)n_records, max_len, p->e, h->tiny_buffers, &err))) return fail(h, rc, err);
  // first uses: the slot's streams (a stream's queue is made by its first command) and the tail's code object
  if (!s.text_stream) HIP_TRY(h, s.text_stream.create(hipStreamNonBlocking));
  HIP_TRY(h, hipMemsetAsync(s.d_sel_hdr ? (void *)s.d_sel_hdr.get() : (void *)s.d_off.get(), 0, 8, s.text_stream));
  HIP_TRY(h, hipStreamSynchronize(s.text_stream));
  HIP_TRY(h, hipMemsetAsync(s.d_off, 0, 8, h->side_stream));
  HIP_TRY(h, hipStreamSynchronize(h->side_stream));
  // ... and the copy paths a batch takes, in both directions, from and to the buffers it will use
  const size_t probe = 1u << 20;
  if (s.h_bases && s.h_bases.size() >= probe && s.d_bases_alloc.size() >= kFrontPad + probe)
    HIP_TRY(h, hipMemcpyAsync(s.d_bases_alloc + kFrontPad, s.h_bases, probe, hipMemcpyHostToDevice, s.stream));
  if (s.h_quals && s.d_quals && s.h_quals.size() >= probe && s.d_quals.size() >= probe)
    HIP_TRY(h, hipMemcpyAsync(s.d_quals, s.h_quals, probe, hipMemcpyHostToDevice, s.text_stream));
  HIP_TRY(h, hipMemcpyAsync(s.h_ctl, s.d_ctl, kCtlBytes, hipMemcpyDeviceToHost, s.stream));
  HIP_TRY(h, hipStreamSynchronize(s.text_stream));
  HIP_TRY(h, hipStreamSynchronize(s.stream));
  if ((rc = s.tail->warm(out_stream_of(h, s), &err))) return fail(h, rc, err);
  return FEM_OK;
}

static int commit_text(fem_dev *h, int slot, uint64_t n_reads, uint64_t n_name_bytes, bool with_quals) {
  int rc = check_slot(h, slot);
  if (rc) return rc;
  FEM_LOCK(h);
  Slot &s = h->slot[slot];
  if (!s.staged) return fail(h, FEM_ERR_STATE, "commit the reads of the batch first");
  if ((with_quals && !s.h_quals) || !s.h_names || !s.h_name_off) return fail(h, FEM_ERR_STATE, "acquire the slot's text staging buffers first");
  if (n_reads != s.n_reads) return fail(h, FEM_ERR_INVALID, "as many names as reads, please");
  if ((with_quals && s.n_bases + 64 > s.h_quals.size()) || n_name_bytes + 64 > s.h_names.size() || n_reads + 1 > s.h_name_off.size())
    return fail(h, FEM_ERR_INVALID, "more qualities or names than the text staging buffers were acquired for");
  if (n_reads && (s.h_name_off[0] != 0 || s.h_name_off[n_reads] != n_name_bytes))
    return fail(h, FEM_ERR_INVALID, "name offsets must start at 0 and end at the number of name bytes");
  HIP_TRY(h, hipSetDevice(h->device));
  if (with_quals) HIP_TRY(h, s.d_quals.ensure((size_t)s.n_bases + 64));
  HIP_TRY(h, s.d_names.ensure((size_t)n_name_bytes + 64));
  HIP_TRY(h, s.d_name_off.ensure((size_t)n_reads + 1));
  // On a stream of their own: nothing before the SAM text reads them, and on the slot's stream these copies (1.25 times the
  // characters of the reads: 2.5 ms per million 100-bp reads) stood between the batch's reads and its first kernel.
  if (!s.text_stream) HIP_TRY(h, s.text_stream.create(hipStreamNonBlocking));
  HIP_TRY(h, s.ev_text_staged.create(hipEventDisableTiming));
  // (the slot's previous batch may still be rendering its text out of the same arrays)
  if (s.have_text_order) HIP_TRY(h, hipStreamWaitEvent(s.text_stream, s.ev_text_order, 0));
  if (with_quals && s.n_bases) HIP_TRY(h, hipMemcpyAsync(s.d_quals, s.h_quals, s.n_bases, hipMemcpyHostToDevice, s.text_stream));
  if (n_name_bytes) HIP_TRY(h, hipMemcpyAsync(s.d_names, s.h_names, n_name_bytes, hipMemcpyHostToDevice, s.text_stream));
  HIP_TRY(h, hipMemcpyAsync(s.d_name_off, s.h_name_off, (n_reads + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s.text_stream));
  HIP_TRY(h, hipEventRecord(s.ev_text_staged, s.text_stream));
  s.text_staged = true, s.host_quals = !with_quals, s.qual_at = nullptr;
  return FEM_OK;
}

int fem_dev_commit_text_stage(fem_dev *h, int slot, uint64_t n_reads, uint64_t n_name_bytes) { return commit_text(h, slot, n_reads, n_name_bytes, true); }
// Names only: the qualities stay where the caller has them (228 of the 473 bytes per read that cross the link with the device's
// SAM text are the qualities going up and coming back unchanged).  The text then leaves the QUAL field of every read's first
// record unwritten, and fem_dev_sam_quals says where each read's field is.
int fem_dev_commit_names_stage(fem_dev *h, int slot, uint64_t n_reads, uint64_t n_name_bytes) { return commit_text(h, slot, n_reads, n_name_bytes, false); }

int fem_dev_sam_quals(fem_dev *h, int slot, const uint64_t **qual_at, uint64_t *n_reads) {
  int rc = check_slot(h, slot);
  if (rc) return rc;
  FEM_LOCK(h);
  Slot &s = h->slot[slot];
  if (!qual_at) return fail(h, FEM_ERR_INVALID, "null output pointer");
  if (!s.host_quals || !s.qual_at) return fail(h, FEM_ERR_STATE, "the slot's last SAM text was rendered with its qualities (or there is none)");
  *qual_at = s.qual_at;
  if (n_reads) *n_reads = s.n_reads;
  return FEM_OK;
}

static int fetch_sam(fem_dev *h, int slot, fem_batch_sam *out, bool wait);
int fem_dev_fetch_sam(fem_dev *h, int slot, fem_batch_sam *out) { return fetch_sam(h, slot, out, true); }
int fem_dev_fetch_sam_nowait(fem_dev *h, int slot, fem_batch_sam *out) { return fetch_sam(h, slot, out, false); }
int fem_dev_sam_wait(fem_dev *h, int slot) {
  if (!h || slot < 0 || slot >= kSlots) return FEM_ERR_INVALID;
  Slot &s = h->slot[slot];
  if (!s.tail) return FEM_ERR_STATE;
  if (hipSetDevice(h->device) != hipSuccess) return FEM_ERR_HIP;
  return s.tail->wait_text();  // (touches nothing but the slot's event: safe next to the thread that drives the handle)
}

// Pairs the records the slot's tail has just made, on `stream`, as `opt` (the slot's options, or a copy) says; mate rescue
// reads the slot's batch and the reference (fetch time: the insert window's width is checked here).
static int pair_records(fem_dev *h, Slot &s, const femt::LineOptions &opt, hipStream_t stream) {
  if (s.n_reads & 1) return fail(h, FEM_ERR_INVALID, "a batch of read pairs holds an even number of reads");
  if (opt.rescues() && (int64_t)opt.max_insert - opt.min_insert > 65536)
    return fail(h, FEM_ERR_UNSUPPORTED, "mate rescue searches insert windows of at most 65536 (max_insert - min_insert)");
  const femt::RescueInput ri{s.map_bases(), s.map_off(), s.max_len, h->d_ref_raw, h->ref_bytes + 64, h->d_seq_off, h->d_seq_len};
  std::string err;
  const int rc = s.tail->pair(opt, ri, stream, &err);
  return rc ? fail(h, rc, err) : FEM_OK;
}

// What the device tail reads of the slot's batch and of the index.
static femt::TailInput tail_input(const fem_dev *h, const Slot &s) {
  femt::TailInput in{};
  in.bases = s.map_bases(), in.read_off = s.map_off(), in.n_reads = (uint32_t)s.n_reads, in.max_len = s.max_len;
  if (s.view.trimmed) in.text_bases = s.bases(), in.text_read_off = s.d_off, in.clip5 = s.cuts[kTrim].d[0], in.clip3 = s.cuts[kTrim].d[1];
  in.ref_raw = h->d_ref_raw, in.ref_bytes = h->ref_bytes + 64, in.seq_off = h->d_seq_off;
  in.planes = h->d_planes;
  if (s.sent_packed) in.packed = s.packed(), in.packed_bpr = s.packed_bpr, in.exc_bits = s.d_exc_bits;
  in.cand = s.d_cand, in.ed = s.d_ed, in.end = s.d_end, in.cand_begin = s.d_begin, in.cand_count = s.d_count;
  in.n_map = s.d_nmap, in.e = s.params.e, in.n_records = s.stats[4];
  return in;
}

// What the front of a fetch leaves for the rest of it: the records were made on `stream` (a text goes there); host time
// from t_in to the mapping synced and to the records made.
struct TailFront {
  femt::TailInput in;
  femt::TailOutput t;
  hipStream_t stream;
  double ms_sync, ms_run;
  std::chrono::steady_clock::time_point t_in;
};

// The fem_dev_kernel_time id of each stage of the device tail, and the slots that count it (nullptr: every fetch, a fetch of
// records too; the others: texts).  A text's own stage, femt::kText, goes under its fetch's id: 7 SAM, 11 BAM.
struct TailStage {
  femt::Stage stage;
  int id;
  bool (*counted)(const femt::LineOptions &);
};
static const TailStage kTailStages[] = {
    {femt::kOrder, 3, nullptr}, {femt::kTrace, 4, nullptr}, {femt::kCompact, 5, nullptr},
    {femt::kPairing, 9, [](const femt::LineOptions &o) { return o.paired; }},
    {femt::kRescue, 10, [](const femt::LineOptions &o) { return o.rescues(); }},
    {femt::kMapq, 13, [](const femt::LineOptions &o) { return o.mapq; }},  // (its events precede the text's sizing, which sam() and bam() wait for)
    {femt::kUnmappedIndex, 14, [](const femt::LineOptions &o) { return o.unmapped && !o.filters() && !o.folds(); }},  // (as do these)
    {femt::kFilterIndex, 15, [](const femt::LineOptions &o) { return o.filters(); }},  // (whose line index is the unmapped reads' too: no 14 then)
    {femt::kMateScore, 17, [](const femt::LineOptions &o) { return o.mates(); }},  // (a text with mate tags has its qualities on the device: tail_records)
    {femt::kXaIndex, 18, [](const femt::LineOptions &o) { return o.folds(); }},  // (the line index it reads is made inside it where no filter is set: no 14, no 15 then)
};

// Timing: counts the stages of the slot's last fetch once each, with their device time where the tail has one.  text_id: the
// id femt::kText goes under, < 0: none (records; a text that was not waited for: its time cannot be read yet).
static void count_tail_stages(fem_dev *h, const Slot &s, bool text, int text_id) {
  FEM_LOCK(h);  // (FEM map retires each slot's batches from a thread of its own)
  auto count = [&](femt::Stage stage, int id) { h->t_ms[id] += std::max(s.tail->stage_ms(stage), 0.f), h->t_n[id] += 1; };
  for (const auto &st : kTailStages)
    if (!st.counted || (text && st.counted(s.opt))) count(st.stage, st.id);
  if (text_id >= 0) count(femt::kText, text_id);
}

// The front of every way a batch's records leave the device (fem_dev_fetch_records, fetch_sam, fetch_bam): waits for the
// slot's mapping, checks it (`out`: the caller's result), makes the records.  copy_records: on the slot's stream, copied home.
// Else a text follows (device_quals: its qualities on the device): records on out_stream_of, a paired slot's paired.
static int tail_records(fem_dev *h, int slot, const void *out, bool copy_records, bool device_quals, TailFront *f) {
  f->t_in = std::chrono::steady_clock::now();
  auto since = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - f->t_in).count(); };
  int rc = fem_dev_sync(h, slot);
  if (rc) return rc;
  f->ms_sync = since();
  if (!out) return fail(h, FEM_ERR_INVALID, "null result");
  Slot &s = h->slot[slot];
  const bool text = !copy_records;
  if (text && !s.text_staged) return fail(h, FEM_ERR_STATE, "qualities and names of this batch were not committed (fem_dev_commit_text_stage)");
  if (text && s.opt.mates() && s.host_quals)
    return fail(h, FEM_ERR_INVALID, "mate tags (fem_dev_set_mate_tags) need the qualities on the device: ms:i is made from them (fem_dev_commit_text_stage, not _names_stage)");
  if (text && s.opt.sam_seq && s.host_quals)
    return fail(h, FEM_ERR_INVALID, "SEQ and QUAL in SAM order (fem_dev_set_sam_seq) need the qualities on the device: QUAL is reversed where it is written (fem_dev_commit_text_stage, not _names_stage)");
  if (text && s.view.trimmed && s.host_quals)
    return fail(h, FEM_ERR_INVALID, "a trimmed batch (fem_dev_set_trim) prints its whole QUAL from the device (fem_dev_commit_text_stage, not _names_stage)");
  if (device_quals && s.host_quals) return fail(h, FEM_ERR_STATE, "BAM records need the qualities on the device (fem_dev_commit_text_stage, not _names_stage)");
  if (text && !h->d_ref_names) return fail(h, FEM_ERR_STATE, "reference names must be uploaded first (fem_dev_upload_reference_names)");
  s.prefetch_results = false;  // this caller takes records, not the per-candidate arrays
  if (!s.tail) s.tail.reset(new (std::nothrow) femt::Tail());
  if (!s.tail) return fail(h, FEM_ERR_NOMEM, "out of host memory");
  f->in = tail_input(h, s);
  if (copy_records && s.out_stream) HIP_TRY(h, hipStreamSynchronize(s.out_stream));  // (a SAM text of this slot still being made reads the tail's arrays)
  f->stream = copy_records ? s.stream : out_stream_of(h, s);
  // the tail reads characters and offsets of the whole batch (traceback, rescue, SAM and BAM text)
  if ((rc = ensure_chars(h, s))) return rc;
  if (s.sent_packed && f->stream != s.stream.s) HIP_TRY(h, hipStreamWaitEvent(f->stream, s.ev_chars, 0));  // (made on the slot's stream)
  std::string err;
  if ((rc = s.tail->run(f->in, f->stream, h->n_cu, h->tiny_buffers, &f->t, &err, copy_records))) return fail(h, rc, err);
  if (text && s.opt.paired && (rc = pair_records(h, s, s.opt, f->stream))) return rc;
  if (text) HIP_TRY(h, hipStreamWaitEvent(f->stream, s.ev_text_staged, 0));  // qualities and names came on the slot's text stream
  f->ms_run = since();
  if (copy_records && h->timing) count_tail_stages(h, s, false, -1);
  return FEM_OK;
}

// The names (and qualities, unless the caller keeps them: qual_hole) the slot's text is rendered with.
static femt::SamInput sam_input(const fem_dev *h, const Slot &s) {
  return {s.host_quals ? nullptr : s.d_quals, s.d_names, s.d_name_off, h->d_ref_names, h->d_ref_name_off, s.host_quals};
}

// What follows a text's sam() / bam() (tag: the caller, for FEM_FETCH_TIMES): the counts, the event the slot's next text
// stage waits for (commit_text), the kernel times (count_tail_stages; text_id: the text's own id, < 0: it was not waited for).
static int text_done(fem_dev *h, int slot, const TailFront &f, const char *tag, int text_id) {
  Slot &s = h->slot[slot];
  s.counts = s.tail->counts();  // (sam() and bam() have waited for the stream once, after sizing the text)
  HIP_TRY(h, s.ev_text_order.create(hipEventDisableTiming));
  HIP_TRY(h, hipEventRecord(s.ev_text_order, f.stream));
  s.have_text_order = true;
  static const bool trace_host = testing_switch("FEM_FETCH_TIMES");  // host time of the call's three stretches, on stderr
  if (trace_host) fprintf(stderr, "[%s] slot %d: mapping synced after %.2f ms, records %.2f, text sized and queued %.2f\n", tag, slot, f.ms_sync,
                          f.ms_run, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - f.t_in).count());
  if (h->timing) count_tail_stages(h, s, true, text_id);
  return FEM_OK;
}

// The coverage field of a text's or BAM fetch's options (fem_dev_set_coverage, rule 4): the first one of the slot's batch carries
// the track and so adds the batch's lines; every other one, and every one with the option off, carries none.  The batch counts
// as added (text_covered, behind sam() / bam() whether or not they succeeded) once coverage_kernel has been queued for it: a fetch
// that failed in front of the kernel leaves the batch to the next one, one that failed behind it is not added twice.
static femt::LineOptions::Coverage text_coverage(fem_dev *h, Slot &s) {
  femt::LineOptions::Coverage c{};
  if (!h->coverage.on || s.covered) return c;
  c.window = h->coverage.set.window, c.all_hits = h->coverage.set.all_hits != 0, c.min_mapq = h->coverage.set.min_mapq;
  c.n_seq = h->n_seq, c.bin_off = h->coverage.d_bin_off, c.seq_len = h->d_seq_len, c.bins = h->coverage.d_bins;
  return c;
}
static void text_covered(Slot &s) {
  if (s.opt.covers() && s.tail->coverage_queued()) s.covered = true;
}

int fem_dev_fetch_records(fem_dev *h, int slot, fem_batch_records *out) {
  TailFront f{};
  int rc = tail_records(h, slot, out, true, false, &f);
  if (rc) return rc;
  out->n_reads = f.t.n_reads, out->n_records = f.t.n_records;
  out->rec_begin = f.t.rec_begin, out->flag = f.t.flag, out->tid = f.t.tid, out->pos0 = f.t.pos0, out->nm = f.t.nm;
  out->cigar_off = f.t.cigar_off, out->cigar = f.t.cigar, out->md_off = f.t.md_off, out->md = f.t.md;
  memcpy(out->stats, h->slot[slot].stats, sizeof out->stats);
  return FEM_OK;
}

static int fetch_sam(fem_dev *h, int slot, fem_batch_sam *out, bool wait) {
  TailFront f{};
  int rc = tail_records(h, slot, out, false, false, &f);
  if (rc) return rc;
  Slot &s = h->slot[slot];
  femt::SamOutput text{};
  std::string err;
  s.opt.coverage = text_coverage(h, s);
  rc = s.tail->sam(f.in, sam_input(h, s), s.opt, f.stream, h->n_cu, &text, &err, wait, &h->text_gate);
  text_covered(s);
  if (rc) return fail(h, rc, err);
  if ((rc = text_done(h, slot, f, "fetch_sam", wait ? 7 : -1))) return rc;
  s.qual_at = text.qual_at;
  out->text = text.text, out->len = text.len, out->n_asserted = text.n_asserted;
  out->n_reads = f.t.n_reads, out->n_records = f.t.n_records - s.counts.n_filtered;  // (the filter drops lines of mapping records only)
  memcpy(out->stats, s.stats, sizeof s.stats);
  return FEM_OK;
}

// ---- BAM output: the SAM lines as BAM records, BGZF-compressed on the device ----
static int fetch_bam(fem_dev *h, int slot, int level, fem_batch_bam *out, bool wait) {
  if (level < 0 || level > 1) return fail(h, FEM_ERR_INVALID, "BAM compression level must be 0 or 1");
  TailFront f{};
  int rc = tail_records(h, slot, out, false, true, &f);
  if (rc) return rc;
  Slot &s = h->slot[slot];
  femt::BamOutput bam{};
  float ms_bgzf = 0.f;
  std::string err;
  s.opt.coverage = text_coverage(h, s);
  rc = s.tail->bam(f.in, sam_input(h, s), s.opt, level, f.stream, h->n_cu, &bam, &err, h->timing ? &ms_bgzf : nullptr, wait, &h->text_gate);
  text_covered(s);
  if (rc) return fail(h, rc, err);
  if ((rc = text_done(h, slot, f, "fetch_bam", 11))) return rc;  // (bam() has waited for its records' stage: the compressor does)
  if (h->timing) {
    FEM_LOCK(h);
    h->t_ms[12] += ms_bgzf, h->t_n[12] += 1;
  }
  s.qual_at = nullptr;
  out->data = bam.data, out->len = bam.len, out->raw_len = bam.raw_len, out->n_blocks = bam.n_blocks;
  out->n_records = f.t.n_records - s.counts.n_filtered, out->n_asserted = bam.n_asserted;
  memcpy(out->stats, s.stats, sizeof s.stats);
  return FEM_OK;
}
int fem_dev_fetch_bam(fem_dev *h, int slot, int level, fem_batch_bam *out) { return fetch_bam(h, slot, level, out, true); }
int fem_dev_fetch_bam_nowait(fem_dev *h, int slot, int level, fem_batch_bam *out) { return fetch_bam(h, slot, level, out, false); }
int fem_dev_bam_wait(fem_dev *h, int slot) { return fem_dev_sam_wait(h, slot); }

int fem_dev_bgzf_compress(fem_dev *h, const void *in, uint64_t n, int level, void *out, uint64_t out_cap, uint64_t *out_len) {
  if (!h) return FEM_ERR_INVALID;
  FEM_LOCK(h);
  if (!out_len || (n && (!in || !out))) return fail(h, FEM_ERR_INVALID, "null argument");
  if (level < 0 || level > 1) return fail(h, FEM_ERR_INVALID, "BGZF compression level must be 0 or 1");
  *out_len = 0;
  if (!n) return FEM_OK;
  HIP_TRY(h, hipSetDevice(h->device));
  if (!h->bgzf) h->bgzf.reset(new (std::nothrow) femz::Bgzf());
  if (!h->bgzf) return fail(h, FEM_ERR_NOMEM, "out of host memory");
  if (!h->z_stream) HIP_TRY(h, h->z_stream.create(hipStreamNonBlocking));
  HIP_TRY(h, h->d_zin.ensure((size_t)n));
  HIP_TRY(h, hipMemcpyAsync(h->d_zin, in, (size_t)n, hipMemcpyHostToDevice, h->z_stream));
  std::vector<uint64_t> starts;
  femz::bgzf_cut(nullptr, 0, n, &starts);
  uint64_t len = 0;
  std::string err;
  int rc = h->bgzf->compress(h->d_zin, n, starts, level, h->z_stream, &len, &err);
  if (rc) return fail(h, rc, err);
  if (len > out_cap) return fail(h, FEM_ERR_INVALID, "output buffer too small for the BGZF members");
  HIP_TRY(h, hipMemcpyAsync(out, h->bgzf->out(), (size_t)len, hipMemcpyDeviceToHost, h->z_stream));
  HIP_TRY(h, hipStreamSynchronize(h->z_stream));
  *out_len = len;
  return FEM_OK;
}

// One of the slot's counts (fem_dev_*_count); pair_mode: the pair counts are a slot's in pair mode only.
static int line_count(fem_dev *h, int slot, uint64_t *out, uint64_t femt::LineCounts::*count, bool pair_mode) {
  return with_slot(h, slot, [&](Slot &s) {
    if (!out) return fail(h, FEM_ERR_INVALID, "null output pointer");
    if (pair_mode && !s.opt.paired) return fail(h, FEM_ERR_STATE, "the slot is not in pair mode (fem_dev_set_pairs)");
    *out = s.counts.*count;
    return (int)FEM_OK;
  });
}
int fem_dev_pair_count(fem_dev *h, int slot, uint64_t *n) { return line_count(h, slot, n, &femt::LineCounts::n_proper, true); }
int fem_dev_rescue_count(fem_dev *h, int slot, uint64_t *n) { return line_count(h, slot, n, &femt::LineCounts::n_rescued, true); }
int fem_dev_rescue_discordant_count(fem_dev *h, int slot, uint64_t *n) {
  return line_count(h, slot, n, &femt::LineCounts::n_rescued_discordant, true);
}
int fem_dev_unmapped_count(fem_dev *h, int slot, uint64_t *n) { return line_count(h, slot, n, &femt::LineCounts::n_unmapped, false); }
int fem_dev_filtered_count(fem_dev *h, int slot, uint64_t *n) { return line_count(h, slot, n, &femt::LineCounts::n_filtered, false); }

int fem_dev_set_pairs(fem_dev *h, int slot, const fem_pair_params *pp) {
  return with_slot(h, slot, [&](Slot &s) {
    if (!pp) return s.opt.paired = false, (int)FEM_OK;
    if (pp->min_insert < 0 || pp->max_insert < pp->min_insert || pp->max_insert > (1 << 30))
      return fail(h, FEM_ERR_INVALID, "insert size range out of bounds (0 <= min_insert <= max_insert <= 2^30)");
    s.opt.paired = true, s.opt.min_insert = pp->min_insert, s.opt.max_insert = pp->max_insert;
    return (int)FEM_OK;
  });
}

int fem_dev_set_orientation(fem_dev *h, int slot, int orientation) {
  return with_slot(h, slot, [&](Slot &s) {
    if (orientation != FEM_ORIENT_FR && orientation != FEM_ORIENT_RF && orientation != FEM_ORIENT_FF)
      return fail(h, FEM_ERR_INVALID, "orientation out of range (FEM_ORIENT_FR, FEM_ORIENT_RF or FEM_ORIENT_FF)");
    s.opt.orientation = orientation;
    return (int)FEM_OK;
  });
}

int fem_dev_set_rescue(fem_dev *h, int slot, const fem_rescue_params *rp) {
  return with_slot(h, slot, [&](Slot &s) {
    if (!rp) return s.opt.rescue = false, (int)FEM_OK;
    if (rp->max_edits < 0 || rp->max_edits > 15) return fail(h, FEM_ERR_INVALID, "rescue edit bound out of range (0 <= max_edits <= 15)");
    s.opt.rescue = true, s.opt.rescue_edits = rp->max_edits;
    return (int)FEM_OK;
  });
}

int fem_dev_set_rescue_discordant(fem_dev *h, int slot, int on) {
  return with_slot(h, slot, [&](Slot &s) { return s.opt.rescue_discordant = on != 0, (int)FEM_OK; });
}
int fem_dev_set_mapq(fem_dev *h, int slot, int on) {
  return with_slot(h, slot, [&](Slot &s) { return s.opt.mapq = on != 0, (int)FEM_OK; });
}
int fem_dev_set_unmapped(fem_dev *h, int slot, int on) {
  return with_slot(h, slot, [&](Slot &s) { return s.opt.unmapped = on != 0, (int)FEM_OK; });
}

int fem_dev_set_mate_tags(fem_dev *h, int slot, int on) {
  return with_slot(h, slot, [&](Slot &s) { return s.opt.mate_tags = on != 0, (int)FEM_OK; });
}

int fem_dev_set_sam_seq(fem_dev *h, int slot, int on) {
  return with_slot(h, slot, [&](Slot &s) { return s.opt.sam_seq = on != 0, (int)FEM_OK; });
}

int fem_dev_set_xa(fem_dev *h, int slot, int32_t max_entries) {
  return with_slot(h, slot, [&](Slot &s) {
    if (max_entries < 0) return fail(h, FEM_ERR_INVALID, "XA entry limit out of range (max_entries >= 1, or 0 for off)");
    s.opt.xa_entries = max_entries;
    return (int)FEM_OK;
  });
}
int fem_dev_xa_count(fem_dev *h, int slot, uint64_t *n) { return line_count(h, slot, n, &femt::LineCounts::n_xa, false); }

// ---- the coverage track: bins of the handle, added to by every slot's texts (Tail::lines, coverage_kernel) ----
// Waits for everything the slots have queued: a text that was not waited for may still be adding.
static int coverage_quiet(fem_dev *h) {
  HIP_TRY(h, hipSetDevice(h->device));
  for (Slot &s : h->slot) {
    if (s.stream) HIP_TRY(h, hipStreamSynchronize(s.stream));
    if (s.out_stream) HIP_TRY(h, hipStreamSynchronize(s.out_stream));
  }
  return FEM_OK;
}

int fem_dev_set_coverage(fem_dev *h, const fem_coverage_params *cp) {
  if (!h) return FEM_ERR_INVALID;
  FEM_LOCK(h);
  if (int rc = coverage_quiet(h)) return rc;
  if (!cp) {
    h->coverage = fem_dev::Coverage{};
    return FEM_OK;
  }
  if (!h->d_ref_raw || !h->n_seq) return fail(h, FEM_ERR_STATE, "the reference must be uploaded first (fem_dev_upload_reference)");
  if (cp->window < 1 || cp->window > femc::kMaxWindow) return fail(h, FEM_ERR_INVALID, "coverage window out of range (1 .. 1000000)");
  if (cp->all_hits != 0 && cp->all_hits != 1) return fail(h, FEM_ERR_INVALID, "coverage all_hits out of range (0 or 1)");
  if (cp->min_mapq < 0 || cp->min_mapq > 60) return fail(h, FEM_ERR_INVALID, "coverage min_mapq out of range (0 .. 60)");
  std::vector<uint64_t> bin_off((size_t)h->n_seq + 1);
  uint64_t n_bins = 0;
  if (femc::layout(h->n_seq, h->seq_len.data(), cp->window, bin_off.data(), &n_bins) != 0)
    return fail(h, FEM_ERR_INVALID, "more than 2^29 coverage windows (" + std::to_string(n_bins) + "); the least window that fits is " +
                                        std::to_string(femc::min_window(h->n_seq, h->seq_len.data())));
  // (in buffers of their own first: a failure leaves the setting, and the track, as they were)
  Buf<uint64_t> d_bin_off;
  Buf<unsigned long long> d_bins;
  HIP_TRY(h, d_bin_off.ensure(bin_off.size()));
  HIP_TRY(h, d_bins.ensure(std::max<uint64_t>(n_bins, 1)));
  HIP_TRY(h, hipMemcpy(d_bin_off, bin_off.data(), bin_off.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
  HIP_TRY(h, hipMemset(d_bins, 0, std::max<uint64_t>(n_bins, 1) * sizeof(unsigned long long)));
  HIP_TRY(h, hipDeviceSynchronize());  // (the slots' streams do not wait for the null stream's)
  fem_dev::Coverage &c = h->coverage;
  c.on = true, c.set = *cp, c.n_bins = n_bins, c.bin_off = std::move(bin_off);
  c.d_bin_off = std::move(d_bin_off), c.d_bins = std::move(d_bins);
  return FEM_OK;
}

int fem_dev_coverage_layout(const fem_dev *h, uint64_t *n_bins, uint64_t *bin_off) {
  if (!h) return FEM_ERR_INVALID;
  if (!h->coverage.on) return FEM_ERR_STATE;
  if (n_bins) *n_bins = h->coverage.n_bins;
  if (bin_off) std::copy(h->coverage.bin_off.begin(), h->coverage.bin_off.end(), bin_off);
  return FEM_OK;
}

int fem_dev_fetch_coverage(fem_dev *h, uint64_t *bins, uint64_t cap) {
  if (!h) return FEM_ERR_INVALID;
  FEM_LOCK(h);
  if (!h->coverage.on) return fail(h, FEM_ERR_STATE, "the coverage track is off (fem_dev_set_coverage)");
  if (cap < h->coverage.n_bins || (!bins && h->coverage.n_bins)) return fail(h, FEM_ERR_INVALID, "room for fewer bins than the track has (fem_dev_coverage_layout)");
  if (int rc = coverage_quiet(h)) return rc;
  if (h->coverage.n_bins) HIP_TRY(h, hipMemcpy(bins, h->coverage.d_bins, h->coverage.n_bins * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return FEM_OK;
}

int fem_dev_reset_coverage(fem_dev *h) {
  if (!h) return FEM_ERR_INVALID;
  FEM_LOCK(h);
  if (!h->coverage.on) return fail(h, FEM_ERR_STATE, "the coverage track is off (fem_dev_set_coverage)");
  if (int rc = coverage_quiet(h)) return rc;
  HIP_TRY(h, hipMemset(h->coverage.d_bins, 0, std::max<uint64_t>(h->coverage.n_bins, 1) * sizeof(unsigned long long)));
  HIP_TRY(h, hipDeviceSynchronize());
  return FEM_OK;
}

int fem_dbg_stage_ms(fem_dev *h, int slot, int stage, float *ms) {
  if (!ms || stage < 0 || stage >= femt::kStages) return FEM_ERR_INVALID;
  return with_slot(h, slot, [&](Slot &s) { return *ms = s.tail ? s.tail->stage_ms((femt::Stage)stage) : -1.f, (int)FEM_OK; });
}

int fem_dev_set_report(fem_dev *h, int slot, const fem_report_params *rp) {
  return with_slot(h, slot, [&](Slot &s) {
    if (!rp) return s.opt.strata = s.opt.max_hits = -1, (int)FEM_OK;
    if (rp->strata < -1 || rp->strata > 15) return fail(h, FEM_ERR_INVALID, "strata out of range (0 <= strata <= 15, or -1 for off)");
    if (rp->max_hits < -1 || rp->max_hits == 0) return fail(h, FEM_ERR_INVALID, "hit limit out of range (max_hits >= 1, or -1 for off)");
    s.opt.strata = rp->strata, s.opt.max_hits = rp->max_hits;
    return (int)FEM_OK;
  });
}

int fem_dev_set_tags(fem_dev *h, int slot, const fem_tag_params *tp) {
  return with_slot(h, slot, [&](Slot &s) {
    if (!tp) return s.opt.read_group.clear(), s.opt.hit_tags = false, (int)FEM_OK;
    size_t n = 0;
    if (tp->read_group) {
      n = strnlen(tp->read_group, 256);
      if (n < 1 || n > 255) return fail(h, FEM_ERR_INVALID, "read group ID out of range (1 to 255 bytes)");
      for (size_t i = 0; i < n; ++i)
        if (tp->read_group[i] < ' ' || tp->read_group[i] > '~') return fail(h, FEM_ERR_INVALID, "read group ID holds a byte outside [ -~]");
    }
    s.opt.read_group.assign(tp->read_group ? tp->read_group : "", n);
    s.opt.hit_tags = tp->hit_tags != 0;
    return (int)FEM_OK;
  });
}

// The records of fem_dev_fetch_records, paired on the device (pair_kernel) and put in output order here on the host: an
// inspection path (tests, tools); FEM map takes the text (fem_dev_fetch_sam).
int fem_dev_fetch_pairs(fem_dev *h, int slot, fem_batch_pairs *out) {
  int rc = check_slot(h, slot);
  if (rc) return rc;
  if (!out) return fail(h, FEM_ERR_INVALID, "null result");
  if (!h->slot[slot].opt.paired) return fail(h, FEM_ERR_STATE, "the slot is not in pair mode (fem_dev_set_pairs)");
  fem_batch_records rec{};
  if ((rc = fem_dev_fetch_records(h, slot, &rec))) return rc;
  Slot &s = h->slot[slot];
  // without the MAPQ bytes: the arrays of this path have no MAPQ column, and a later text must not find pair_mapq set by a
  // pair() that was not its own
  femt::LineOptions opt = s.opt;
  opt.mapq = false;
  if ((rc = pair_records(h, s, opt, s.stream))) return rc;
  std::string err;
  femt::PairOutput po{};
  if ((rc = s.tail->pair_fetch(s.stream, &po, &err))) return fail(h, rc, err);
  const uint64_t nr = po.n_records;
  s.pr_flag.assign(po.flag, po.flag + nr);
  s.pr_tid.resize(nr), s.pr_pos0.resize(nr), s.pr_nm.resize(nr), s.pr_cigar_off.resize(nr + 1), s.pr_md_off.resize(nr + 1);
  s.pr_cigar.clear(), s.pr_md.clear();
  s.pr_cigar_off[0] = 0, s.pr_md_off[0] = 0;
  for (uint64_t k = 0; k < nr; ++k) {
    const uint32_t r = po.perm[k];
    if (r < po.first_rescued) {
      s.pr_tid[k] = rec.tid[r], s.pr_pos0[k] = rec.pos0[r], s.pr_nm[k] = rec.nm[r];
      s.pr_cigar.insert(s.pr_cigar.end(), rec.cigar + rec.cigar_off[r], rec.cigar + rec.cigar_off[r + 1]);
      s.pr_md.insert(s.pr_md.end(), rec.md + rec.md_off[r], rec.md + rec.md_off[r + 1]);
    } else {  // a rescued mate's record
      const uint32_t q = r - po.first_rescued, c0 = po.r_cigar_off[0], m0 = po.r_md_off[0];
      s.pr_tid[k] = po.r_tid[q], s.pr_pos0[k] = po.r_pos0[q], s.pr_nm[k] = po.r_nm[q];
      s.pr_cigar.insert(s.pr_cigar.end(), po.r_cigar + (po.r_cigar_off[q] - c0), po.r_cigar + (po.r_cigar_off[q + 1] - c0));
      s.pr_md.insert(s.pr_md.end(), po.r_md + (po.r_md_off[q] - m0), po.r_md + (po.r_md_off[q + 1] - m0));
    }
    s.pr_cigar_off[k + 1] = (uint32_t)s.pr_cigar.size(), s.pr_md_off[k + 1] = (uint32_t)s.pr_md.size();
  }
  s.counts = s.tail->counts();  // (pair_fetch() has waited for the stream)
  out->n_pairs = po.n_pairs, out->n_records = nr;
  out->rec_begin = po.pair_begin, out->flag = s.pr_flag.data(), out->tid = s.pr_tid.data(), out->pos0 = s.pr_pos0.data();
  out->nm = s.pr_nm.data(), out->cigar_off = s.pr_cigar_off.data(), out->cigar = s.pr_cigar.data();
  out->md_off = s.pr_md_off.data(), out->md = s.pr_md.data();
  out->mate_tid = po.mate_tid, out->mate_pos0 = po.mate_pos0, out->tlen = po.tlen;
  out->n_proper = po.n_proper;
  memcpy(out->stats, s.stats, sizeof s.stats);
  return FEM_OK;
}

static void insert_estimate_out(const femt::InsertEstimate &e, fem_insert_estimate *out) {
  out->n_pairs = e.n_pairs, out->n_unique = e.n_unique, out->n_informative = e.n_informative;
  out->q25 = e.q25, out->q50 = e.q50, out->q75 = e.q75;
  out->min_insert = e.min_insert, out->max_insert = e.max_insert, out->estimated = e.estimated ? 1 : 0;
}

// The insert size range the slot's batch suggests, under the slot's orientation or under all three (include/fem_hip.h: the
// rules): the records of fem_dev_fetch_records, then `run`, the tail's two kernels over them.  Reads the records only: the
// slot's options, counts and whatever a later fetch makes stay.
static int estimate_with(fem_dev *h, int slot, const void *out, const std::function<int(Slot &, std::string *)> &run) {
  int rc = check_slot(h, slot);
  if (rc) return rc;
  if (!out) return fail(h, FEM_ERR_INVALID, "null result");
  if (!h->slot[slot].opt.paired) return fail(h, FEM_ERR_STATE, "the slot is not in pair mode (fem_dev_set_pairs)");
  fem_batch_records rec{};
  if ((rc = fem_dev_fetch_records(h, slot, &rec))) return rc;
  Slot &s = h->slot[slot];
  if (s.n_reads & 1) return fail(h, FEM_ERR_INVALID, "a batch of read pairs holds an even number of reads");
  std::string err;
  if ((rc = run(s, &err))) return fail(h, rc, err);
  if (h->timing) {
    FEM_LOCK(h);
    h->t_ms[16] += std::max(s.tail->stage_ms(femt::kInsert), 0.f), h->t_n[16] += 1;
  }
  return FEM_OK;
}

int fem_dev_estimate_insert(fem_dev *h, int slot, fem_insert_estimate *out) {
  femt::InsertEstimate e{};
  const int rc = estimate_with(h, slot, out, [&](Slot &s, std::string *err) { return s.tail->estimate_insert(s.opt, s.stream, &e, err); });
  if (!rc) insert_estimate_out(e, out);
  return rc;
}

int fem_dev_estimate_library(fem_dev *h, int slot, fem_library_estimate *out) {
  femt::LibraryEstimate e{};
  const int rc = estimate_with(h, slot, out, [&](Slot &s, std::string *err) { return s.tail->estimate_library(s.stream, &e, err); });
  if (rc) return rc;
  for (int o = 0; o < 3; ++o) insert_estimate_out(e.by[o], &out->by[o]);
  out->orientation = e.orientation;
  return FEM_OK;
}

int fem_dev_map_batch_submit(fem_dev *h, int slot, const fem_params *p, const fem_read_batch *reads) {
  int rc = fem_dev_stage_reads(h, slot, reads);
  if (rc) return rc;
  return fem_dev_map_staged(h, slot, p);
}

int fem_dev_set_trim(fem_dev *h, int slot, const fem_trim_params *tp) {
  return with_slot(h, slot, [&](Slot &s) {
    const fem_trim_params t = tp ? *tp : fem_trim_params{0, 0, 0};
    if (t.trim5 < 0 || t.trim5 > 1024 || t.trim3 < 0 || t.trim3 > 1024 || t.qual < 0 || t.qual > 93)
      return fail(h, FEM_ERR_INVALID, "trim out of range (trim5 and trim3 0..1024, qual 0 or 1..93)");
    s.prep.trim = t;
    return (int)FEM_OK;
  });
}

int fem_dev_fetch_trim(fem_dev *h, int slot, const uint16_t **clip5, const uint16_t **clip3, uint64_t *n_reads) {
  return fetch_cuts(h, slot, kTrim, clip5, clip3, n_reads);
}

int fem_dev_trim_count(fem_dev *h, int slot, uint64_t *n_reads_trimmed, uint64_t *n_bases_trimmed) {
  return cut_counts(h, slot, kTrim, n_reads_trimmed, n_bases_trimmed);
}

int fem_dev_set_adapter(fem_dev *h, int slot, const fem_adapter_params *ap) {
  return with_slot(h, slot, [&](Slot &s) {
    PrepSettings::Adapter a;
    if (!ap || !ap->seq1) return s.prep.adapter = a, (int)FEM_OK;
    const char *seq[2] = {ap->seq1, ap->seq2 ? ap->seq2 : ap->seq1};
    for (int k = 0; k < 2; ++k) {
      const size_t m = strnlen(seq[k], 65);
      if (m < 4 || m > 64) return fail(h, FEM_ERR_INVALID, "adapter out of range (4 to 64 letters of ACGT)");
      for (size_t j = 0; j < m; ++j) {
        static const char letters[] = "ACGT";
        const char *at = strchr(letters, seq[k][j] & ~0x20);  // (lower case is accepted)
        if (!at || !*at) return fail(h, FEM_ERR_INVALID, "adapter out of range (4 to 64 letters of ACGT)");
        a.occ[k][at - letters] |= 1ull << j;
      }
      a.len[k] = (int32_t)m;
    }
    if (ap->min_overlap < 1 || ap->min_overlap > std::min(a.len[0], a.len[1]))
      return fail(h, FEM_ERR_INVALID, "adapter overlap out of range (1 to the adapter's length, the shorter one's of two)");
    if (ap->err_pct < 0 || ap->err_pct > 30) return fail(h, FEM_ERR_INVALID, "adapter error percentage out of range (0 to 30)");
    a.on = true, a.min_overlap = ap->min_overlap, a.err_pct = ap->err_pct;
    s.prep.adapter = a;
    return (int)FEM_OK;
  });
}

int fem_dev_fetch_adapter(fem_dev *h, int slot, const uint16_t **adapt3, uint64_t *n_reads) {
  return fetch_cuts(h, slot, kAdapter, adapt3, nullptr, n_reads);
}

int fem_dev_adapter_count(fem_dev *h, int slot, uint64_t *n_reads_cut, uint64_t *n_bases_cut) {
  return cut_counts(h, slot, kAdapter, n_reads_cut, n_bases_cut);
}

int fem_dev_set_pair_overlap(fem_dev *h, int slot, const fem_pair_overlap_params *vp) {
  return with_slot(h, slot, [&](Slot &s) {
    PrepSettings::PairOverlap v;
    if (!vp) return s.prep.overlap = v, (int)FEM_OK;
    if (vp->min_overlap < 8 || vp->min_overlap > 1024) return fail(h, FEM_ERR_INVALID, "pair overlap out of range (8 to 1024)");
    if (vp->err_pct < 0 || vp->err_pct > 30) return fail(h, FEM_ERR_INVALID, "pair overlap error percentage out of range (0 to 30)");
    v.on = true, v.min_overlap = vp->min_overlap, v.err_pct = vp->err_pct;
    s.prep.overlap = v;
    return (int)FEM_OK;
  });
}

int fem_dev_fetch_pair_overlap(fem_dev *h, int slot, const uint16_t **over3, uint64_t *n_reads) {
  return fetch_cuts(h, slot, kOverlap, over3, nullptr, n_reads);
}

int fem_dev_pair_overlap_count(fem_dev *h, int slot, uint64_t *n_pairs_cut, uint64_t *n_bases_cut) {
  return cut_counts(h, slot, kOverlap, n_pairs_cut, n_bases_cut);
}

int fem_dev_map_batch_wait(fem_dev *h, int slot, fem_batch_result *out) { return fem_dev_fetch(h, slot, out); }

int fem_dev_index_info(const fem_dev *h, char *buf, uint64_t cap) {
  if (!h || !buf || cap == 0) return FEM_ERR_INVALID;
  const uint64_t n_buckets = h->n_lookup ? h->n_lookup - 1 : 0;
  std::string s;
  if (!h->d_lookup) {
    s = "no index";
  } else if (has_dense_tables(h)) {
    s = "dense: 32-bit occurrence table, ";
    s += h->list_shift ? "strided with pads (" + std::to_string(((n_buckets + femk::kDensePadBuckets) << h->list_shift) * 4 >> 20) + " MiB)"
                       : "compact (" + std::to_string(h->n_occ * 4 >> 20) + " MiB)";
    s += ", " + std::to_string(h->n_banks) + (h->n_banks == 1 ? " bank" : " banks") + ", freq11 64 MiB";
  } else if (h->d_summary) {
    s = "sparse: bucket summaries";
  } else {
    s = "64-bit occurrence table only";
  }
  s += "; " + std::to_string(h->n_occ) + " entries in " + std::to_string(n_buckets) + " buckets";
  snprintf(buf, (size_t)cap, "%s", s.c_str());
  return FEM_OK;
}

const char *fem_dev_seed_kernel(const fem_dev *h, const fem_params *p) {
  if (!h || !params_ok(p)) return "";
  // (by SeedPath::Kind; the strided table's kernel goes by the compact one's name)
  static const char *const names[] = {"seed_filter_kernel", "seed_fast_kernel<lean>", "seed_fast_kernel<hash>", "seed_join_kernel", "seed_join_banked_kernel", "seed_join_kernel"};
  return names[seed_path(h, *p).kind];
}

int fem_dev_set_timing(fem_dev *h, int on) {
  if (!h) return FEM_ERR_INVALID;
  h->timing = on != 0;
  if (h->timing && h->event_pool.idle.size() < 64) {
    // the events of a few batches in flight, made now: created one by one inside the first timed launches they cost those
    // launches a millisecond each (the pipeline of bench.py was visibly slower over its first steps)
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, h->event_pool.fill(64));
  }
  return FEM_OK;
}

int fem_dev_reset_timing(fem_dev *h) {
  if (!h) return FEM_ERR_INVALID;
  for (int i = 0; i < kTimedKernels; ++i) h->t_ms[i] = 0, h->t_n[i] = 0;
  if (h->timeline) {
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, h->ev_epoch.create());
    HIP_TRY(h, hipEventRecord(h->ev_epoch, h->side_stream));
    h->have_epoch = true;
  }
  return FEM_OK;
}

int fem_dev_kernel_time(fem_dev *h, int kernel, double *ms_total, uint64_t *launches) {
  if (!h || kernel < 0 || kernel >= kTimedKernels) return FEM_ERR_INVALID;
  if (ms_total) *ms_total = h->t_ms[kernel];
  if (launches) *launches = h->t_n[kernel];
  return FEM_OK;
}

int fem_dev_copy_bandwidth(fem_dev *h, uint64_t bytes, int iters, double *gb_per_s) {
  if (!h || !gb_per_s || bytes == 0 || iters <= 0) return FEM_ERR_INVALID;
  HIP_TRY(h, hipSetDevice(h->device));
  Buf<uint8_t> a, b;
  HIP_TRY(h, a.ensure(bytes));
  if (b.ensure(bytes) != hipSuccess) return fail(h, FEM_ERR_NOMEM, "copy bandwidth probe: out of memory");
  hipStream_t st = h->slot[0].stream;
  hipEvent_t e0 = h->event_pool.get(), e1 = h->event_pool.get();
  (void)hipMemsetAsync(a, 1, bytes, st);
  (void)hipMemcpyAsync(b, a, bytes, hipMemcpyDeviceToDevice, st);
  (void)hipEventRecord(e0, st);
  for (int i = 0; i < iters; ++i) (void)hipMemcpyAsync(b, a, bytes, hipMemcpyDeviceToDevice, st);
  (void)hipEventRecord(e1, st);
  hipError_t e = hipStreamSynchronize(st);
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, e0, e1);
  h->event_pool.put(e0);
  h->event_pool.put(e1);
  if (e != hipSuccess) return fail(h, FEM_ERR_HIP, hipGetErrorString(e));
  *gb_per_s = ms > 0 ? (2.0 * (double)bytes * iters) / (ms * 1e6) : 0.0;  // read + write
  return FEM_OK;
}

int fem_dev_h2d_bandwidth(fem_dev *h, uint64_t bytes, int iters, double *gb_per_s) {
  if (!h || !gb_per_s || bytes == 0 || iters <= 0) return FEM_ERR_INVALID;
  HIP_TRY(h, hipSetDevice(h->device));
  PinBuf<uint8_t> a;
  Buf<uint8_t> b;
  HIP_TRY(h, a.ensure(bytes));
  if (b.ensure(bytes) != hipSuccess) return fail(h, FEM_ERR_NOMEM, "h2d bandwidth probe: out of memory");
  memset(a, 1, bytes);
  hipStream_t st = h->slot[0].stream;
  hipEvent_t e0 = h->event_pool.get(), e1 = h->event_pool.get();
  (void)hipMemcpyAsync(b, a, bytes, hipMemcpyHostToDevice, st);
  (void)hipEventRecord(e0, st);
  for (int i = 0; i < iters; ++i) (void)hipMemcpyAsync(b, a, bytes, hipMemcpyHostToDevice, st);
  (void)hipEventRecord(e1, st);
  hipError_t e = hipStreamSynchronize(st);
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, e0, e1);
  h->event_pool.put(e0);
  h->event_pool.put(e1);
  if (e != hipSuccess) return fail(h, FEM_ERR_HIP, hipGetErrorString(e));
  *gb_per_s = ms > 0 ? ((double)bytes * iters) / (ms * 1e6) : 0.0;
  return FEM_OK;
}

#ifdef FEM_STAMPS
// diagnostic build only: read and clear the seed kernel's per-phase cycle totals
int fem_dbg_stamps(uint64_t *out, int n) {
  unsigned long long tmp[femk::kNumStamps];
  if (hipMemcpyFromSymbol(tmp, HIP_SYMBOL(femk::g_stamp_cycles), sizeof tmp) != hipSuccess) return -1;
  for (int i = 0; i < n && i < femk::kNumStamps; ++i) out[i] = tmp[i];
  memset(tmp, 0, sizeof tmp);
  (void)hipMemcpyToSymbol(HIP_SYMBOL(femk::g_stamp_cycles), tmp, sizeof tmp);
  return 0;
}
#endif

// Bytes of device and pinned host memory the library's buffers hold right now, over all handles of the process (the tests'
// check that a closed handle has given everything back).
int fem_dbg_live_bytes(uint64_t *device_bytes, uint64_t *pinned_bytes) {
  if (device_bytes) *device_bytes = femb::g_live_bytes[(int)femb::Mem::Device].load(std::memory_order_relaxed);
  if (pinned_bytes) *pinned_bytes = femb::g_live_bytes[(int)femb::Mem::Pinned].load(std::memory_order_relaxed);
  return FEM_OK;
}

// ---- host placement ----
// The pinned staging buffers are what the GPU's copy engines read: they should sit in the memory of the socket the GPU
// hangs off, and so should the threads that fill them (measured on a two-socket MI355X host, FASTQ -> SAM on 16 M reads:
// 0.30 s with the process on the GPU's node, 0.35-0.45 s unbound, 0.39-0.42 s on the other node).
int fem_device_numa(int device, int32_t *node, char *cpulist, uint64_t cap) {
  if (node) *node = -1;
  if (cpulist && cap) cpulist[0] = 0;
  char bdf[64] = {0};
  if (hipDeviceGetPCIBusId(bdf, (int)sizeof bdf, device) != hipSuccess) return FEM_ERR_HIP;
  for (char *c = bdf; *c; ++c) *c = (char)tolower((unsigned char)*c);  // sysfs spells the address in lower case
  char path[160];
  snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/numa_node", bdf);
  FILE *f = fopen(path, "r");
  if (!f) return FEM_OK;  // (no sysfs: unknown, not an error)
  int n = -1;
  if (fscanf(f, "%d", &n) != 1) n = -1;
  fclose(f);
  if (node) *node = n;
  if (n >= 0 && cpulist && cap) {
    snprintf(path, sizeof path, "/sys/devices/system/node/node%d/cpulist", n);
    if ((f = fopen(path, "r"))) {
      if (!fgets(cpulist, (int)std::min<uint64_t>(cap, 1u << 20), f)) cpulist[0] = 0;
      fclose(f);
      for (char *c = cpulist; *c; ++c)
        if (*c == '\n') *c = 0;
    }
  }
  return FEM_OK;
}

int fem_bind_thread_near_device(int device) {
  const char *env = getenv("FEM_NUMA_BIND");
  if (env && env[0] == '0') return 1;
  int32_t node = -1;
  std::vector<char> list(4096, 0);
  if (fem_device_numa(device, &node, list.data(), list.size()) != FEM_OK || node < 0 || !list[0]) return 1;
  cpu_set_t now, want;
  CPU_ZERO(&now);
  CPU_ZERO(&want);
  if (sched_getaffinity(0, sizeof now, &now) != 0) return 1;
  int n_set = 0;
  for (const char *c = list.data(); *c;) {  // "a-b,c,d-e"
    char *end = nullptr;
    const long lo = strtol(c, &end, 10);
    if (end == c) break;
    long hi = lo;
    if (*end == '-') hi = strtol(end + 1, &end, 10);
    for (long i = lo; i <= hi && i < CPU_SETSIZE; ++i)
      if (i >= 0 && CPU_ISSET((int)i, &now)) {
        CPU_SET((int)i, &want);
        ++n_set;
      }
    if (*end != ',') break;
    c = end + 1;
  }
  if (n_set == 0) return 1;  // the node's CPUs are not ours to run on: leave the thread where it is
  return sched_setaffinity(0, sizeof want, &want) == 0 ? 0 : 1;
}

int fem_dev_allreduce_stats(fem_dev *const *hs, int n, uint64_t *stats) {
  if (!hs || n <= 0 || !stats) return FEM_ERR_INVALID;
  std::vector<int> devs(n);
  for (int i = 0; i < n; ++i) {
    if (!hs[i]) return FEM_ERR_INVALID;
    devs[i] = hs[i]->device;
  }
  fem_dev *h0 = hs[0];
  std::lock_guard<std::mutex> lock(g_comm_mu);
  // one communicator per job: created on the first call, reused while the same devices take part
  if (!g_comm || g_comm->devs != devs) {
    destroy_comm_set();
    CommSet *cs = new (std::nothrow) CommSet();
    if (!cs) return fail(h0, FEM_ERR_NOMEM, "out of host memory");
    cs->devs = devs;
    cs->comms.assign(n, nullptr);
    cs->bufs.resize(n);
    if (ncclCommInitAll(cs->comms.data(), n, devs.data()) != ncclSuccess) {
      delete cs;
      return fail(h0, FEM_ERR_RCCL, "ncclCommInitAll failed");
    }
    g_comm = cs;
    for (int i = 0; i < n; ++i)
      if (hipSetDevice(devs[i]) != hipSuccess || cs->bufs[i].ensure(5) != hipSuccess) {
        destroy_comm_set();
        return fail(h0, FEM_ERR_HIP, "allreduce: allocating the counter buffers failed");
      }
  }
  CommSet &cs = *g_comm;
  int rc = FEM_OK;
  for (int i = 0; i < n && rc == FEM_OK; ++i) {
    if (hipSetDevice(devs[i]) != hipSuccess ||
        hipMemcpyAsync(cs.bufs[i], stats + 5 * i, 5 * sizeof(uint64_t), hipMemcpyHostToDevice, hs[i]->slot[0].stream) != hipSuccess)
      rc = fail(h0, FEM_ERR_HIP, "allreduce: staging the counters failed");
  }
  if (rc == FEM_OK) {
    ncclGroupStart();
    for (int i = 0; i < n; ++i) {
      (void)hipSetDevice(devs[i]);
      if (ncclAllReduce(cs.bufs[i].get(), cs.bufs[i].get(), 5, ncclUint64, ncclSum, cs.comms[i], hs[i]->slot[0].stream) != ncclSuccess)
        rc = fail(h0, FEM_ERR_RCCL, "ncclAllReduce failed");
    }
    if (ncclGroupEnd() != ncclSuccess) rc = fail(h0, FEM_ERR_RCCL, "ncclGroupEnd failed");
  }
  for (int i = 0; i < n && rc == FEM_OK; ++i) {
    (void)hipSetDevice(devs[i]);
    if (hipStreamSynchronize(hs[i]->slot[0].stream) != hipSuccess ||
        hipMemcpy(stats + 5 * i, cs.bufs[i], 5 * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess)
      rc = fail(h0, FEM_ERR_HIP, "allreduce: reading the counters back failed");
  }
  return rc;
}

}  // extern "C"
