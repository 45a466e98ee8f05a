// fem_tail.hip — device mapping tail: kernels + the host-side driver behind fem_dev_fetch_records.
// See fem_tail.hip.h for what is computed and the reference lines it follows.
#include "fem_tail.hip.h"
#include "fem_bgzf.hip.h"
#include "fem_buf.hip.h"
#include "fem_planes.hip.h"

#include <cstring>  // before rocprim: its headers use memcpy unqualified

#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/fem_hip.h"

namespace femt {
namespace {

constexpr uint32_t kOpM = 0, kOpI = 1, kOpD = 2, kOpS = 3;  // S: the traceback's pseudo-run (src/align.c:342), never emitted
constexpr uint32_t kOpsCap = 16, kMdCap = 32;  // first-pass staging per record; anything longer goes to the overflow pass
constexpr uint32_t kSortLdsHits = 2048;         // hits of one read the ordering kernel keeps in LDS
constexpr uint16_t kFlagBroken = 0x8000;

// ---- hit = one accepted candidate: Mapping (src/utils.h:44-49) ----
// misc = end_position_offset (low 16) | edit_distance << 16 | direction << 24
__device__ __forceinline__ uint64_t hit_key(uint64_t cand, uint32_t misc) {  // MappingSortKey, src/align.c:53
  const int64_t end = (int16_t)(misc & 0xFFFFu);
  return ((uint64_t)((misc >> 16) & 0xFFu) << 60) | ((uint64_t)((misc >> 24) & 1u) << 59) | (cand + (uint64_t)end);
}

struct Params {
  // mapping outcome
  const uint8_t *bases;
  const uint64_t *read_off;
  uint32_t n_reads;
  const uint8_t *ref_raw;
  uint64_t ref_bytes;
  const uint8_t *planes;
  const uint8_t *packed;     // TailInput::packed, packed_bpr, exc_bits
  uint32_t packed_bpr;
  const uint32_t *exc_bits;
  const uint64_t *seq_off;
  const uint64_t *cand;
  const uint8_t *ed;
  const int16_t *end;
  const uint32_t *cand_begin, *cand_count;
  int32_t e;
  uint32_t n_records;
  const uint32_t *rec_begin;  // n_reads + 1
  // hits in verify order (u_) and in record order (s_)
  uint64_t *u_cand;
  uint32_t *u_misc;
  uint64_t *s_cand;
  uint32_t *s_misc, *s_read;
  uint32_t *queue;  // reads with three or more hits
  uint32_t *ctl;    // [0] queue length, [1] records of the overflow pass, [2] staging too small even there, [3] length of rec_list
  uint64_t *g_keys;  // ordering scratch for reads with more hits than fit LDS (n_records each)
  uint32_t *g_idx;
  // traceback
  uint32_t lanes, text_words, pat_words, max_len;  // LDS plan of one block of the general kernel
  uint32_t fast_lanes, fast_ops;                   // ... and of the first-pass kernel (lanes, runs kept per lane)
  uint32_t *t_ops;
  uint8_t *t_md;
  uint32_t ops_cap, md_cap;
  const uint32_t *ovf_queue;  // overflow pass: the records to redo, staged at index * cap
  uint32_t *ovf_out;          // first pass: where overflowing records are queued
  uint32_t *rec_list;         // records trace_ident_kernel left to the walking kernels (ctl[3] of them); nullptr = all
  uint32_t *src_slot;         // per record: 0 = first-pass staging, kSlotDiagonal | L = `L M` (MD in the first-pass staging), else 1 + index in the overflow staging
  uint32_t *n_ops, *n_md;
  uint16_t *flag;
  uint32_t *tid, *pos0;
  uint8_t *nm;
};

// ---------------------------------------------------------------------------------------------------------
// Ordering.  One lane per read rebuilds the read's Mapping list in verify_candidates' order (+ strand first,
// candidates ascending, src/map.c:31-49); lists of one or two are ordered on the spot, longer ones are queued.
// ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) gather_kernel(Params p) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= p.n_reads) return;
  const uint32_t b = p.rec_begin[r], n = p.rec_begin[r + 1] - b;
  if (n == 0) return;
  uint32_t j = 0;
  uint64_t c0 = 0, c1 = 0;
  uint32_t m0 = 0, m1 = 0;
  for (uint32_t dir = 0; dir < 2u; ++dir) {
    const uint32_t s = 2u * r + dir, cb = p.cand_begin[s], cn = p.cand_count[s];
    for (uint32_t i = cb; i < cb + cn; ++i) {
      const uint32_t ed = p.ed[i];
      if (ed == 0xFFu) continue;
      const uint64_t c = p.cand[i];
      const uint32_t m = (uint32_t)(uint16_t)p.end[i] | (ed << 16) | (dir << 24);
      if (j == 0) c0 = c, m0 = m;
      if (j == 1) c1 = c, m1 = m;
      if (j < n) p.u_cand[b + j] = c, p.u_misc[b + j] = m;
      ++j;
    }
  }
  if (n <= 2u) {
    const bool swap = n == 2u && hit_key(c1, m1) < hit_key(c0, m0);  // stable: equal keys keep verify order
    p.s_cand[b] = swap ? c1 : c0, p.s_misc[b] = swap ? m1 : m0, p.s_read[b] = r;
    if (n == 2u) p.s_cand[b + 1] = swap ? c0 : c1, p.s_misc[b + 1] = swap ? m0 : m1, p.s_read[b + 1] = r;
  } else {
    p.queue[atomicAdd(&p.ctl[0], 1u)] = r;
  }
}

// klib's radix sort on (key, original index) pairs, run by one lane: KRADIX_SORT_INIT(mapping, Mapping,
// MappingSortKey, 8) (src/ksort.h:101-151).  <= 64 records are never sent here.  Each level is an in-place
// cycle-leader permutation into 256 buckets (not stable); buckets of <= 64 are finished by insertion sort, larger
// ones recurse on the next byte.  Equal keys exist, so the exact permutation decides which record is the primary.
__device__ void insertion_by_key(uint64_t *keys, uint32_t *idx, uint32_t beg, uint32_t end) {
  for (uint32_t i = beg + 1; i < end; ++i) {
    if (keys[i] < keys[i - 1]) {
      const uint64_t tk = keys[i];
      const uint32_t ti = idx[i];
      uint32_t j = i;
      for (; j > beg && tk < keys[j - 1]; --j) keys[j] = keys[j - 1], idx[j] = idx[j - 1];
      keys[j] = tk, idx[j] = ti;
    }
  }
}

__device__ void radix_permute_level(uint64_t *keys, uint32_t *idx, uint32_t beg, uint32_t end, int shift, uint32_t *bin_b,
                                    uint32_t *bin_e) {
  for (int k = 0; k < 256; ++k) bin_e[k] = 0;
  for (uint32_t i = beg; i < end; ++i) ++bin_e[(keys[i] >> shift) & 255u];
  uint32_t run = beg;
  for (int k = 0; k < 256; ++k) {
    const uint32_t c = bin_e[k];
    bin_b[k] = run;
    run += c;
    bin_e[k] = run;
  }
  for (int k = 0; k < 256;) {
    if (bin_b[k] == bin_e[k]) {
      ++k;
      continue;
    }
    uint32_t at = bin_b[k];
    int dst = (int)((keys[at] >> shift) & 255u);
    if (dst == k) {
      ++bin_b[k];
      continue;
    }
    uint64_t ck = keys[at];
    uint32_t ci = idx[at];
    do {  // follow the cycle until an element of bucket k comes back
      const uint32_t to = bin_b[dst]++;
      const uint64_t dk = keys[to];
      const uint32_t di = idx[to];
      keys[to] = ck, idx[to] = ci;
      ck = dk, ci = di;
      dst = (int)((ck >> shift) & 255u);
    } while (dst != k);
    keys[bin_b[k]] = ck, idx[bin_b[k]] = ci;
    ++bin_b[k];
  }
}

struct RadixFrame {
  uint32_t beg, end;
  int shift, k;  // k < 0: level not permuted yet
};

__device__ void klib_radix_sort(uint64_t *keys, uint32_t *idx, uint32_t n, uint32_t *bin_b, uint32_t *bin_e_levels,
                                RadixFrame *frames) {
  int sp = 0;
  frames[0] = RadixFrame{0u, n, 56, -1};
  while (sp >= 0) {
    RadixFrame &f = frames[sp];
    uint32_t *bin_e = bin_e_levels + sp * 256;
    if (f.k < 0) {
      radix_permute_level(keys, idx, f.beg, f.end, f.shift, bin_b, bin_e);
      f.k = 0;
      if (f.shift == 0) {
        --sp;
        continue;
      }
    }
    bool pushed = false;
    while (f.k < 256) {
      const int k = f.k++;
      const uint32_t lo = k ? bin_e[k - 1] : f.beg, hi = bin_e[k];
      if (hi - lo > 64u) {
        frames[sp + 1] = RadixFrame{lo, hi, f.shift > 8 ? f.shift - 8 : 0, -1};
        ++sp;
        pushed = true;
        break;
      }
      if (hi - lo > 1u) insertion_by_key(keys, idx, lo, hi);
    }
    if (!pushed) --sp;
  }
}

__global__ void __launch_bounds__(64) sort_kernel(Params p) {
  __shared__ uint32_t bin_b[256];
  __shared__ uint32_t bin_e[8 * 256];
  __shared__ RadixFrame frames[8];
  __shared__ uint64_t l_keys[kSortLdsHits];
  __shared__ uint32_t l_idx[kSortLdsHits];
  const uint32_t ln = threadIdx.x;
  const uint32_t n_queue = p.ctl[0];
  for (uint32_t q = blockIdx.x; q < n_queue; q += gridDim.x) {
    const uint32_t r = p.queue[q];
    const uint32_t b = p.rec_begin[r], n = p.rec_begin[r + 1] - b;
    if (n <= 64u) {  // insertion sort == any stable sort: rank = keys that must precede
      const bool have = ln < n;
      const uint64_t c = have ? p.u_cand[b + ln] : 0;
      const uint32_t m = have ? p.u_misc[b + ln] : 0;
      const uint64_t key = have ? hit_key(c, m) : ~0ull;
      uint32_t rank = 0;
      for (uint32_t u = 0; u < n; ++u) {
        const uint64_t ku = __shfl(key, (int)u);
        rank += (uint32_t)(ku < key || (ku == key && u < ln));
      }
      if (have) p.s_cand[b + rank] = c, p.s_misc[b + rank] = m, p.s_read[b + rank] = r;
    } else {
      uint64_t *keys = n <= kSortLdsHits ? l_keys : p.g_keys + b;
      uint32_t *idx = n <= kSortLdsHits ? l_idx : p.g_idx + b;
      for (uint32_t i = ln; i < n; i += 64u) keys[i] = hit_key(p.u_cand[b + i], p.u_misc[b + i]), idx[i] = i;
      __threadfence();
      __syncthreads();
      if (ln == 0) klib_radix_sort(keys, idx, n, bin_b, bin_e, frames);
      __threadfence();
      __syncthreads();
      for (uint32_t i = ln; i < n; i += 64u) {
        const uint32_t src = idx[i];
        p.s_cand[b + i] = p.u_cand[b + src], p.s_misc[b + i] = p.u_misc[b + src], p.s_read[b + i] = r;
      }
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------------
// Traceback.  One lane per record; nothing crosses lanes.  Each lane keeps, word-interleaved in LDS (word w of
// lane l at [w * lanes + l]): the read as aligned (raw characters, or the canonical reverse complement of
// prepare_negative_sequence_at), the reference window pattern[0 .. L + 2e), and D0 / HP of every column.
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t base_code(uint32_t c) {  // src/utils.h:72
  const uint32_t x = (c >> 1) & 3u;
  const uint32_t code = x ^ (x >> 1);
  const uint32_t u = c & 0xDFu;
  return ((u == 'A') | (u == 'C') | (u == 'G') | (u == 'T')) ? code : 4u;
}
__device__ __forceinline__ uint32_t load_u32_unaligned(const uint8_t *p) {
  uint32_t w;
  __builtin_memcpy(&w, p, 4);
  return w;
}
__device__ __forceinline__ uint4 load_u128_unaligned(const uint8_t *p) {
  uint4 w;
  __builtin_memcpy(&w, p, 16);
  return w;
}
// four characters -> their complements in canonical upper case, anything but ACGT -> 'N' (src/sequence_batch.h:90-98)
__device__ __forceinline__ uint32_t complement4(uint32_t chars) {
  const uint32_t t = (chars >> 1) & 0x03030303u;
  const uint32_t code = t ^ ((t >> 1) & 0x01010101u);
  const uint32_t upper = chars & 0xDFDFDFDFu;
  const uint32_t expect = __builtin_amdgcn_perm(0u, 0x54474341u /* "ACGT" */, code);
  const uint32_t z = upper ^ expect;
  const uint32_t nflag = ((((z & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | z) >> 7) & 0x01010101u;
  return __builtin_amdgcn_perm(0x4E4E4E4Eu /* "NNNN" */, 0x54474341u, (code ^ 0x03030303u) | (nflag << 2));
}

// four characters at once (SWAR): code per byte 0..3 (0 where the base is not A/C/G/T), complemented on the reverse
// strand; nflag per byte 0/1 (not A/C/G/T in either case, src/utils.h:72); odd = 0x80 in the bytes that are none of "ACGTN"
__device__ __forceinline__ void decode4(uint32_t chars, uint32_t complement, uint32_t &code, uint32_t &nflag, uint32_t &odd) {
  const uint32_t t = (chars >> 1) & 0x03030303u;
  const uint32_t c = t ^ ((t >> 1) & 0x01010101u);
  const uint32_t expect = __builtin_amdgcn_perm(0u, 0x54474341u /* "ACGT" */, c);
  const uint32_t z = (chars & 0xDFDFDFDFu) ^ expect;
  nflag = ((((z & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | z) >> 7) & 0x01010101u;
  code = (c ^ complement) & ~(nflag * 3u);
  const uint32_t ze = chars ^ expect, zn = chars ^ 0x4E4E4E4Eu;
  odd = (((ze & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | ze) & (((zn & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | zn) & 0x80808080u;
}
// The plane windows are consumed sixteen bits at a time: the 32 bits at bit `off` (< 32) of the window's head, and the
// window moving on by sixteen bits — four v_alignbit per plane and step.  (Indexing the window's words by the step made
// the compiler keep the windows in scratch memory: six scratch loads per step in the verify kernel.)
__device__ __forceinline__ uint32_t window_head(const uint4 &w, uint32_t off) { return __builtin_amdgcn_alignbit(w.y, w.x, off); }
__device__ __forceinline__ void window_advance16(uint4 &w) {
  w.x = __builtin_amdgcn_alignbit(w.y, w.x, 16u), w.y = __builtin_amdgcn_alignbit(w.z, w.y, 16u);
  w.z = __builtin_amdgcn_alignbit(w.w, w.z, 16u), w.w >>= 16;
}
constexpr int kStepsPerPlaneLoad = 6;  // 7 (bit offset) + 16 * 5 + 16 + 2 * 7 (band) bits <= 128

struct LaneView {
  const uint32_t *text, *pat;
  uint32_t *d0, *hp;
  uint32_t nl, ln;
  __device__ __forceinline__ uint32_t text_at(uint32_t i) const { return (text[(i >> 2) * nl + ln] >> (8u * (i & 3u))) & 0xFFu; }
  __device__ __forceinline__ uint32_t pat_at(uint32_t i) const { return (pat[(i >> 2) * nl + ln] >> (8u * (i & 3u))) & 0xFFu; }
};

struct Staging {  // where one record's CIGAR runs and MD characters are written
  uint32_t *ops;
  uint8_t *md;
  uint32_t ops_cap, md_cap;
  uint32_t n_ops = 0, n_md = 0;
  bool overflow = false;
  __device__ __forceinline__ void push_op(uint32_t op, uint32_t len) {
    if (n_ops < ops_cap)
      ops[n_ops] = (len << 4) | op;
    else
      overflow = true;
    ++n_ops;
  }
  __device__ __forceinline__ void push_md(uint32_t ch) {
    if (n_md < md_cap)
      md[n_md] = (uint8_t)ch;
    else
      overflow = true;
    ++n_md;
  }
  __device__ void push_number(uint32_t v) {
    uint32_t digits = 1;
    for (uint32_t t = v; t >= 10u; t /= 10u) ++digits;
    uint32_t div = 1;
    for (uint32_t i = 1; i < digits; ++i) div *= 10u;
    for (; div; div /= 10u) push_md('0' + (v / div) % 10u);
  }
};

// generate_alignment (src/align.c:279-499) + generate_MD_tag (src/align.c:501-544) for one record.
// Returns the start offset inside pattern, or -1 where the reference would have tripped one of its asserts.
// pattern = the window's first byte in HBM; [at_min, at_max] = offsets from it that stay inside the reference buffer.
__device__ int trace_record(const LaneView &v, const uint8_t *pattern, int64_t at_min, int64_t at_max, int L, int e, int ed,
                            int end, Staging &st) {
  int start = end - L + 1;
  if (start < 0) return -1;
  const int pat_len = L + 2 * e;
  bool identical = true;
  for (int i = 0; i < L; ++i) {
    if (v.text_at((uint32_t)i) != v.pat_at((uint32_t)(start + i))) {
      identical = false;
      break;
    }
  }
  if (identical) {  // src/align.c:294-300
    st.push_op(kOpM, (uint32_t)L);
    st.push_number((uint32_t)L);
    return start;
  }
  // ---- the recurrence again, D0 and HP of every column kept (src/align.c:303-338) ----
  {
    uint32_t B0 = 0, B1 = 0, B2 = 0;  // bit planes of the pattern window: Peq[c] is a three-way XNOR
    for (int j = 0; j < 2 * e; ++j) {
      const uint32_t pc = base_code(v.pat_at((uint32_t)j));
      B0 |= (pc & 1u) << j, B1 |= ((pc >> 1) & 1u) << j, B2 |= ((pc >> 2) & 1u) << j;
    }
    const int sh = 2 * e;
    const uint32_t band = (2u << sh) - 1u;
    uint32_t vp = 0, vn = 0;
    for (int i = 0; i < L; ++i) {
      const uint32_t pc = base_code(v.pat_at((uint32_t)(i + sh))), tc = base_code(v.text_at((uint32_t)i));
      B0 |= (pc & 1u) << sh, B1 |= ((pc >> 1) & 1u) << sh, B2 |= ((pc >> 2) & 1u) << sh;
      const uint32_t m0 = 0u - (tc & 1u), m1 = 0u - ((tc >> 1) & 1u), m2 = 0u - ((tc >> 2) & 1u);
      uint32_t x = (~((B0 ^ m0) | (B1 ^ m1) | (B2 ^ m2)) & band) | vn;
      const uint32_t d0 = ((vp + (x & vp)) ^ vp) | x;
      const uint32_t hn = vp & d0;
      const uint32_t hp = vn | ~(vp | d0);
      x = d0 >> 1;
      vn = x & hp;
      vp = hn | ~(x | hp);
      v.d0[(uint32_t)i * v.nl + v.ln] = d0;
      v.hp[(uint32_t)i * v.nl + v.ln] = hp;
      B0 >>= 1, B1 >>= 1, B2 >>= 1;
    }
  }
  // ---- walk back from (last read base, end) until `ed` errors are accounted for (src/align.c:340-440) ----
  enum Move { MATCH, MISMATCH, INSERT, DELETE };
  int bit = end - L + 1, t = L - 1, pe = end, n_err = 0;
  auto classify = [&]() -> Move {
    const bool d = (v.d0[(uint32_t)t * v.nl + v.ln] >> bit) & 1u;
    // pe never exceeds `end`, which lies inside the staged window
    if (d && v.pat_at((uint32_t)pe) == v.text_at((uint32_t)t)) return MATCH;
    if (!d) return MISMATCH;
    if ((v.hp[(uint32_t)t * v.nl + v.ln] >> bit) & 1u) return INSERT;
    return DELETE;
  };
  // The pseudo-run 'S' collects the errors at the read's 3' end and is finally added to the run that follows it
  // (src/align.c:398-399,413-414,466-469); here its length rides along in s_len and is added when that run starts.
  uint32_t cur_op = kOpS, cur_n = 1;
  switch (classify()) {  // the first step replaces the initial pseudo-run (src/align.c:345-368)
    case MATCH: --t, --pe, cur_op = kOpM; break;
    case MISMATCH: --t, --pe, ++n_err; break;
    case INSERT: --t, ++bit, ++n_err, ++start; break;
    case DELETE: return -1;  // assert(1 == 0)
  }
  auto extend = [&](uint32_t op) {
    if (cur_op == op) {
      ++cur_n;
    } else if (cur_op == kOpS) {
      cur_op = op, cur_n += 1;  // S(n) followed by op(1) ends up as op(1 + n)
    } else {
      st.push_op(cur_op, cur_n);
      cur_op = op, cur_n = 1;
    }
  };
  while (t >= 0 && n_err != ed) {
    if (bit < 0 || bit > 31 || pe < 0) return -1;
    switch (classify()) {
      case MATCH: --t, --pe, extend(kOpM); break;
      case MISMATCH:
        --t, --pe, ++n_err;
        if (cur_op == kOpS) ++cur_n; else extend(kOpM);
        break;
      case INSERT:
        --t, ++bit, ++n_err, ++start;
        if (cur_op == kOpS) ++cur_n; else extend(kOpI);
        break;
      case DELETE: --bit, --pe, ++n_err, --start, extend(kOpD); break;
    }
  }
  if (t >= 0) {  // everything left of the last error matches (src/align.c:445-455)
    if (cur_op == kOpM || cur_op == kOpS)
      cur_op = kOpM, cur_n += (uint32_t)(t + 1);
    else
      st.push_op(cur_op, cur_n), cur_op = kOpM, cur_n = (uint32_t)(t + 1);
  }
  if (cur_op == kOpS) return -1;  // nothing but the pseudo-run: the reference indexes past its run list
  st.push_op(cur_op, cur_n);
  if (st.overflow) return start;  // redone with room in the overflow pass
  // runs were produced right to left: reverse in place (src/align.c:470-479)
  for (uint32_t i = 0, j = st.n_ops - 1u; i < j; ++i, --j) {
    const uint32_t a = st.ops[i], b = st.ops[j];
    st.ops[i] = b, st.ops[j] = a;
  }
  // ---- generate_MD_tag over pattern + start (src/align.c:501-544) ----
  uint32_t run = 0, tp = 0;
  int64_t rp = start;  // offset from pattern[0]; the 'S' fold can push a run beyond the staged window
  auto ref_char = [&](int64_t at) -> uint32_t {
    if (at >= 0 && at < pat_len) return v.pat_at((uint32_t)at);
    return pattern[at < at_min ? at_min : at > at_max ? at_max : at];  // only walks the reference itself would reject
  };
  for (uint32_t k = 0; k < st.n_ops; ++k) {
    const uint32_t op = st.ops[k] & 0xFu, n = st.ops[k] >> 4;
    if (op == kOpM) {
      for (uint32_t i = 0; i < n; ++i, ++rp, ++tp) {
        const uint32_t rc = ref_char(rp);
        if (rc == v.text_at(tp)) {
          ++run;
        } else {
          if (run) st.push_number(run), run = 0;
          st.push_md(rc);
        }
      }
    } else if (op == kOpI) {
      tp += n;
    } else {
      if (run) st.push_number(run), run = 0;
      st.push_md('^');
      for (uint32_t i = 0; i < n; ++i, ++rp) st.push_md(ref_char(rp));
    }
  }
  if (run) st.push_number(run);
  return start;
}

// General form of the traceback: redoes the records the first pass queued (p.ovf_queue, p.ctl[1] of them).
__global__ void __launch_bounds__(64) trace_kernel(Params p) {
  extern __shared__ uint32_t lds[];
  const uint32_t nl = p.lanes, ln = threadIdx.x;
  uint32_t *text_w = lds;
  uint32_t *pat_w = text_w + p.text_words * nl;
  uint32_t *d0_w = pat_w + p.pat_words * nl;
  uint32_t *hp_w = d0_w + p.max_len * nl;
  const uint32_t n_items = p.ctl[1];
  for (uint32_t base = blockIdx.x * nl; base < n_items; base += gridDim.x * nl) {
    const uint32_t item = base + ln;
    if (ln >= nl || item >= n_items) continue;
    const uint32_t rec = p.ovf_queue[item];
    const uint32_t read = p.s_read[rec], misc = p.s_misc[rec];
    const uint64_t cand = p.s_cand[rec];
    const int end = (int16_t)(misc & 0xFFFFu), ed = (int)((misc >> 16) & 0xFFu);
    const uint32_t dir = (misc >> 24) & 1u;
    const uint64_t off = p.read_off[read];
    const int L = (int)(p.read_off[read + 1] - off);
    const uint8_t *fwd = p.bases + off;
    const uint32_t tid = (uint32_t)(cand >> 32);
    const uint64_t pat_abs = p.seq_off[tid] + (uint32_t)cand;
    const uint8_t *pattern = p.ref_raw + pat_abs;
    // ---- stage the read as aligned ----
    for (int c = 0; c < L; c += 16) {
      uint32_t w[4];
      if (dir == 0) {
        const uint4 q = load_u128_unaligned(fwd + c);  // may run past the read: those bytes are never looked at
        w[0] = q.x, w[1] = q.y, w[2] = q.z, w[3] = q.w;
      } else if (L - 16 - c >= 0) {  // text[c + i] = complement(fwd[L - 1 - c - i])
        const uint4 q = load_u128_unaligned(fwd + (L - 16 - c));
        w[0] = __builtin_bswap32(complement4(q.w)), w[1] = __builtin_bswap32(complement4(q.z));
        w[2] = __builtin_bswap32(complement4(q.y)), w[3] = __builtin_bswap32(complement4(q.x));
      } else {
        for (int k = 0; k < 4; ++k) {
          const int p0 = L - 4 - c - 4 * k;  // fwd offset of the word's last character
          uint32_t raw = 0;
          if (p0 >= 0)
            raw = load_u32_unaligned(fwd + p0);
          else if (p0 > -4)
            raw = load_u32_unaligned(fwd) << (8 * -p0);
          w[k] = __builtin_bswap32(complement4(raw));
        }
      }
      for (int k = 0; k < 4; ++k)
        if ((uint32_t)(c / 4 + k) < p.text_words) text_w[(uint32_t)(c / 4 + k) * nl + ln] = w[k];
    }
    for (int c = 0; c < L + 2 * p.e; c += 16) {  // the reference buffer has 64 bytes of slack behind its last base
      const uint4 q = load_u128_unaligned(pattern + c);
      const uint32_t w[4] = {q.x, q.y, q.z, q.w};
      for (int k = 0; k < 4; ++k)
        if ((uint32_t)(c / 4 + k) < p.pat_words) pat_w[(uint32_t)(c / 4 + k) * nl + ln] = w[k];
    }
    LaneView v{text_w, pat_w, d0_w, hp_w, nl, ln};
    Staging st;
    st.ops = p.t_ops + (size_t)item * p.ops_cap;
    st.md = p.t_md + (size_t)item * p.md_cap;
    st.ops_cap = p.ops_cap, st.md_cap = p.md_cap;
    int start = trace_record(v, pattern, -(int64_t)pat_abs, (int64_t)p.ref_bytes - 1 - (int64_t)pat_abs, L, p.e, ed, end, st);
    if (st.overflow) {
      atomicAdd(&p.ctl[2], 1u);  // cannot happen: this staging holds the longest possible walk
      start = -1;
    }
    const uint32_t rank = rec - p.rec_begin[read];
    uint16_t flag = (uint16_t)((dir ? 16u : 0u) | (rank ? 256u : 0u));  // BAM_FREVERSE, BAM_FSECONDARY (src/align.c:82-84)
    if (start < 0) flag |= kFlagBroken, start = 0, st.n_ops = 0, st.n_md = 0;
    p.flag[rec] = flag;
    p.tid[rec] = tid;
    p.pos0[rec] = (uint32_t)start + (uint32_t)cand;  // src/align.c:80
    p.nm[rec] = (uint8_t)ed;
    p.n_ops[rec] = st.n_ops, p.n_md[rec] = st.n_md;
    p.src_slot[rec] = item + 1u;
  }
}

// ---------------------------------------------------------------------------------------------------------
// Traceback, first pass: the form nearly every record takes.  Same walk as trace_record, but the lane keeps one
// packed word per column in LDS — per diagonal of the band (0 .. 2e) two bits that say what the walk would do in
// that cell: they fold D0, HP and whether the reference character on that diagonal EQUALS the read character (the
// traceback and the MD tag compare characters, not codes, src/align.c:355,523) — and reads the sequences straight
// from HBM, sixteen columns per load.
// Character equality is derived from the code-equality mask Peq: for characters of the canonical alphabet
// "ACGTN" it is the same thing, a reference character outside it (lower case, IUPAC) equals no canonical one, and
// a read with such characters is left to the general kernel.  So is every walk that leaves the band, and every
// record whose CIGAR or MD outgrows the staging; the general kernel (trace_kernel) redoes those from scratch.
// ---------------------------------------------------------------------------------------------------------
// The packed column word (2 x (2e+1) bits) is kept in as few LDS bytes as hold it — LDS per block is what limits the
// waves per CU here, and the walk is a chain of dependent LDS reads that only more waves can hide: a low plane of
// P0 words and, where needed, a high plane of P1 words; column c of lane l sits at [c * lanes + l] of each.
// ---------------------------------------------------------------------------------------------------------
// Traceback, pass zero: records whose alignment is the end position's diagonal — no recurrence, no walk.
//  * Edit distance 0: generate_alignment first compares the read with the reference at its end position character by
//    character (src/align.c:285-300) and, with no mismatch, emits `L M`.
//  * Edit distance ed > 0 with exactly ed mismatching columns on that diagonal (every record of a read whose errors
//    are substitutions: most of a real sequencer's).  The walk of src/align.c:340-479 then never leaves the diagonal:
//    ed is the least cost of any path into (L-1, end), so no path reaches a cell (t, j) of the diagonal for less than
//    the mismatches before it (it would continue down the diagonal for less than ed), D[t][j] is that count, D0 — "the
//    diagonal step costs nothing" — is set exactly in the columns that match, and the walk tests match, then
//    mismatch, before it looks at HP.  It emits M runs only (the 'S' pseudo-run of mismatches at the read's end folds
//    into the M run behind it; L > ed keeps that run from being the only one): CIGAR `L M`, start = end - L + 1, MD
//    from the mismatching columns.  tests/test_traceback_model.py checks that claim on the matrix model.
// Both need character equality to be code equality: no reference character of the window outside "ACGTN" (plane[3]),
// no non-canonical read character on the forward strand (the reverse strand's complement table turns them into N).
// One lane per record, no LDS: read characters sixteen at a time (decoded to code-bit masks), the reference from its
// bit planes, compared on the one diagonal; MD written as the columns go by (a record that turns out to have more
// mismatches than ed is walked later and its MD written again).  Every other record is appended to rec_list for the
// walking kernels.
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t lsb_mask4(uint32_t bytes01) {  // bytes of 0/1 -> their four bits, byte 0 in bit 0
  return ((bytes01 & 0x01010101u) * 0x01020408u) >> 24;
}
__device__ __forceinline__ uint32_t md_number(uint8_t *md, uint32_t at, uint32_t v) {  // decimal of v < 10000 -> md[at ...]
  const uint32_t digits = v >= 1000u ? 4u : v >= 100u ? 3u : v >= 10u ? 2u : 1u;
  for (uint32_t k = digits; k-- > 0; v /= 10u) md[at + k] = (uint8_t)('0' + v % 10u);
  return at + digits;
}
// ---- the read's bases from the packed form of the batch (two bits per base, low bits first; A C G T = 0 1 2 3) ----
// bases j0 .. j0 + 15 of the read whose row starts at `row` (j0 >= 0), base j0 in bits 0-1
__device__ __forceinline__ uint32_t packed16(const uint8_t *row, int j0) {
  const uint8_t *a = row + (j0 >> 2);
  return __builtin_amdgcn_alignbit(load_u32_unaligned(a + 4), load_u32_unaligned(a), 2u * ((uint32_t)j0 & 3u));
}
__device__ __forceinline__ uint32_t reverse_fields2(uint32_t x) {  // the sixteen 2-bit fields in reverse order
  x = __builtin_bitreverse32(x);
  return ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
}
__device__ __forceinline__ uint32_t even_bits16(uint32_t x) {  // bits 0, 2, 4 .. 30 -> bits 0 .. 15
  x &= 0x55555555u;
  x = (x | (x >> 1)) & 0x33333333u;
  x = (x | (x >> 2)) & 0x0F0F0F0Fu;
  x = (x | (x >> 4)) & 0x00FF00FFu;
  return (x | (x >> 8)) & 0xFFFFu;
}
constexpr uint32_t kSlotDiagonal = 0x80000000u;
constexpr uint32_t kIdentChunk = 1024;  // records one block classifies at a time (four per thread)
__global__ void __launch_bounds__(256) trace_ident_kernel(Params p) {
  __shared__ uint32_t walk[kIdentChunk];
  __shared__ uint32_t n_walk, walk_base;
  const int sh = 2 * p.e;
  for (uint32_t base = blockIdx.x * kIdentChunk; base < p.n_records; base += gridDim.x * kIdentChunk) {
    __syncthreads();
    if (threadIdx.x == 0) n_walk = 0;
    __syncthreads();
#pragma unroll 1
    for (uint32_t k = 0; k < kIdentChunk / 256u; ++k) {
      const uint32_t rec = base + k * 256u + threadIdx.x;
      if (rec >= p.n_records) continue;
      bool done = false;
      const uint32_t misc = p.s_misc[rec];
      const uint32_t read = p.s_read[rec];
      const uint64_t cand = p.s_cand[rec];
      const int end = (int16_t)(misc & 0xFFFFu);
      const uint32_t ed = (misc >> 16) & 0xFFu;
      const uint32_t dir = (misc >> 24) & 1u;
      const uint64_t off = p.read_off[read];
      const int L = (int)(p.read_off[read + 1] - off);
      const uint8_t *fwd = p.bases + off;
      const uint32_t tid = (uint32_t)(cand >> 32);
      const int start = end - L + 1;
      const uint32_t digits = L >= 1000 ? 4u : L >= 100 ? 3u : L >= 10 ? 2u : 1u;
      // MD: at most ed reference characters and ed + 1 numbers
      if (start >= 0 && start <= sh && L > (int)ed && L < 10000 && p.ops_cap >= 1u && (ed + 1u) * digits + ed <= p.md_cap) {
        const uint64_t ref0 = p.seq_off[tid] + (uint32_t)cand + (uint32_t)start;  // compared with text[0]
        const uint32_t complement = dir ? 0x03030303u : 0u;
        const uint32_t bit0 = (uint32_t)ref0 & 7u;
        uint8_t *md = p.t_md + (size_t)rec * p.md_cap;
        uint32_t odd_ref = 0, odd_text = 0, n_mm = 0, n_md = 0;
        int last = -1;  // the column of the last mismatch
        uint4 W0{}, W1{}, W2{}, W3{};
        // a read of A C G T only, in a batch that arrived packed: its code bits come out of the packed words with a
        // handful of shifts (sixteen characters decoded to the same masks are a quarter of this kernel's instructions)
        const bool from_packed = p.packed != nullptr && !((p.exc_bits[read >> 5] >> (read & 31u)) & 1u);
        const uint8_t *row = p.packed + (size_t)read * p.packed_bpr;
        for (int col = 0; col < L; col += 16) {
          const int sub = (col >> 4) % 7;  // 7 (bit offset) + 16 * 7 <= 128: one load per plane covers seven steps
          if (sub == 0) {
            const uint64_t at = (ref0 + (uint32_t)col) >> 3;
            W0 = load_u128_unaligned(femk::plane_addr(p.planes, 0, at)), W1 = load_u128_unaligned(femk::plane_addr(p.planes, 1, at));
            W2 = load_u128_unaligned(femk::plane_addr(p.planes, 2, at)), W3 = load_u128_unaligned(femk::plane_addr(p.planes, 3, at));
          } else {
            window_advance16(W0), window_advance16(W1), window_advance16(W2), window_advance16(W3);
          }
          const int ncol = L - col < 16 ? L - col : 16;
          uint32_t m0 = 0, m1 = 0, m2 = 0;
          if (from_packed) {
            uint32_t t16;  // text[col .. col + 16), two bits each
            if (dir == 0) {
              t16 = packed16(row, col);
            } else if (ncol == 16) {  // text[col + i] = complement(fwd[L - 1 - col - i])
              t16 = ~reverse_fields2(packed16(row, L - 16 - col));
            } else {  // the last, partial step: the read's first ncol bases
              t16 = ~(reverse_fields2(packed16(row, 0)) >> (2u * (uint32_t)(16 - ncol)));
            }
            m0 = even_bits16(t16), m1 = even_bits16(t16 >> 1);
          } else {
            const uint4 r = load_u128_unaligned(dir == 0 ? fwd + col : fwd + (L - 16 - col));
            const uint32_t w[4] = {dir ? __builtin_bswap32(r.w) : r.x, dir ? __builtin_bswap32(r.z) : r.y,
                                   dir ? __builtin_bswap32(r.y) : r.z, dir ? __builtin_bswap32(r.x) : r.w};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              uint32_t cw, nw, odd;
              decode4(w[q], complement, cw, nw, odd);
              const int nb = ncol - 4 * q;
              odd_text |= nb >= 4 ? odd : nb > 0 ? odd & ((1u << (8 * nb)) - 1u) : 0u;
              m0 |= lsb_mask4(cw) << (4 * q), m1 |= lsb_mask4(cw >> 1) << (4 * q), m2 |= lsb_mask4(nw) << (4 * q);
            }
          }
          const uint32_t colmask = ncol == 16 ? 0xFFFFu : ((1u << ncol) - 1u);  // ((ref0 + 112 k) & 7 == ref0 & 7)
          odd_ref |= window_head(W3, bit0) & colmask;
          const uint32_t b0 = window_head(W0, bit0), b1 = window_head(W1, bit0), b2 = window_head(W2, bit0);
          uint32_t diff = ((b0 ^ m0) | (b1 ^ m1) | (b2 ^ m2)) & colmask;
          while (diff) {  // generate_MD_tag over an M run (src/align.c:515-529): the matches counted, the reference's character
            const uint32_t i = (uint32_t)__builtin_ctz(diff);
            const int at = col + (int)i;
            diff &= diff - 1u;
            if (++n_mm > ed) break;
            if (at - last > 1) n_md = md_number(md, n_md, (uint32_t)(at - last - 1));
            // the character from its code (it is one of "ACGTN", or odd_ref sends the record to the walk): no load
            const uint32_t code = ((b0 >> i) & 1u) | (((b1 >> i) & 1u) << 1);
            md[n_md++] = (uint8_t)((b2 >> i) & 1u ? 'N' : 0x54474341u >> (8u * code));
            last = at;
          }
          if (n_mm > ed) break;
        }
        if (n_mm == ed && odd_ref == 0u && !(dir == 0 && odd_text)) {
          if (L - 1 - last > 0) n_md = md_number(md, n_md, (uint32_t)(L - 1 - last));
          const uint32_t rank = rec - p.rec_begin[read];
          p.flag[rec] = (uint16_t)((dir ? 16u : 0u) | (rank ? 256u : 0u));
          p.tid[rec] = tid;
          p.pos0[rec] = (uint32_t)start + (uint32_t)cand;
          p.nm[rec] = (uint8_t)ed;
          p.n_ops[rec] = 1u, p.n_md[rec] = n_md;
          p.src_slot[rec] = kSlotDiagonal | (uint32_t)L;  // CIGAR `L M`: compact_kernel writes it from this word
          done = true;
        }
      }
      if (!done) walk[atomicAdd(&n_walk, 1u)] = rec;
    }
    // Records for the walking kernels gather in LDS and go out with ONE atomic on the list's cursor per chunk (one per
    // wave cost 1.3 ms per 8.6 M records: same-address atomics complete at ~10 ns each).
    __syncthreads();
    if (threadIdx.x == 0) walk_base = n_walk ? atomicAdd(&p.ctl[3], n_walk) : 0u;
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n_walk; i += 256u) p.rec_list[walk_base + i] = walk[i];
  }
}

struct NoPlane {};
template <typename P0, typename P1>
struct ColumnHistory {
  P0 *lo;
  P1 *hi;
  uint32_t nl, ln;
  static constexpr bool kTwo = !__is_same(P1, NoPlane);
  __device__ __forceinline__ void put(uint32_t col, uint64_t v) const {
    lo[col * nl + ln] = (P0)v;
    if constexpr (kTwo) hi[col * nl + ln] = (P1)(v >> (8 * sizeof(P0)));
  }
  __device__ __forceinline__ uint64_t get(uint32_t col) const {
    uint64_t v = lo[col * nl + ln];
    if constexpr (kTwo) v |= (uint64_t)hi[col * nl + ln] << (8 * sizeof(P0));
    return v;
  }
};

template <typename P0, typename P1>
__global__ void __launch_bounds__(64) trace_fast_kernel(Params p) {
  extern __shared__ uint32_t lds[];
  const uint32_t nl = p.fast_lanes, ln = threadIdx.x;
  using HistT = uint64_t;
  ColumnHistory<P0, P1> hist;
  hist.lo = (P0 *)lds;
  hist.hi = (P1 *)(hist.lo + (size_t)p.max_len * nl);
  hist.nl = nl, hist.ln = ln;
  // run k of this lane: ops[k * nl + ln] = len << 2 | op
  uint16_t *ops = (uint16_t *)((uint8_t *)lds + (((size_t)p.max_len * nl * (sizeof(P0) + (ColumnHistory<P0, P1>::kTwo ? sizeof(P1) : 0)) + 3u) & ~(size_t)3u));
  const int e = p.e, sh = 2 * e, W = 2 * e + 1;
  const uint32_t band = (1u << W) - 1u;
  const uint32_t n_list = p.rec_list ? p.ctl[3] : p.n_records;
  for (uint32_t base = blockIdx.x * nl; base < n_list; base += gridDim.x * nl) {
    if (ln >= nl || base + ln >= n_list) continue;
    const uint32_t rec = p.rec_list ? p.rec_list[base + ln] : base + ln;
    const uint32_t read = p.s_read[rec], misc = p.s_misc[rec];
    const uint64_t cand = p.s_cand[rec];
    const int end = (int16_t)(misc & 0xFFFFu), ed = (int)((misc >> 16) & 0xFFu);
    const uint32_t dir = (misc >> 24) & 1u;
    const uint64_t off = p.read_off[read];
    const int L = (int)(p.read_off[read + 1] - off);
    const uint8_t *fwd = p.bases + off;
    const uint32_t tid = (uint32_t)(cand >> 32);
    const uint64_t pat_abs = p.seq_off[tid] + (uint32_t)cand;
    const uint8_t *pattern = p.ref_raw + pat_abs;
    int start = end - L + 1;
    bool punt = start < 0 || start > sh;  // (never: end lies in [L-1, L-1+2e])
    uint32_t odd_ref = 0;  // some reference character of the window is none of "ACGTN"

    // ---- the recurrence (src/align.c:303-338), one packed word per column ----
    // Sixteen columns per step.  Reference side: bit planes of the base codes plus the "none of ACGTN" plane; one
    // unaligned 16-byte load per plane covers the windows pattern[col .. col + 16 + 2e) of six steps.  Read side: 16
    // characters per load, decoded four at a time; on the reverse strand the chunk comes from the read's far end,
    // byte-reversed and complemented (src/sequence_batch.h:90-98; the batch's characters have 16 bytes of padding
    // in front).  Loads are issued one step (text) / one stretch (planes) ahead of their use.
    const uint32_t complement = dir ? 0x03030303u : 0u;
    auto text_chunk = [&](int c) { return load_u128_unaligned(dir == 0 ? fwd + c : fwd + (L - 16 - c)); };
    auto plane_chunk = [&](int q, int c) { return load_u128_unaligned(femk::plane_addr(p.planes, q, (pat_abs + (uint32_t)c) >> 3)); };
    const uint32_t pat_bit = (uint32_t)pat_abs & 7u;
    const int n_steps = (L + 15) >> 4;
    uint32_t vp = 0, vn = 0, odd_text = 0, dm = 0;
    int last_bad = -1;  // the last column whose characters differ on the end position's diagonal (-1: the read is identical there)
    uint4 rw = make_uint4(0, 0, 0, 0), W0 = rw, W1 = rw, W2 = rw, W3 = rw, W0n = rw, W1n = rw, W2n = rw, W3n = rw;
    if (n_steps > 0) {
      rw = text_chunk(0);
      W0n = plane_chunk(0, 0), W1n = plane_chunk(1, 0), W2n = plane_chunk(2, 0), W3n = plane_chunk(3, 0);
    }
    auto column = [&](uint32_t col, uint32_t q, uint32_t b0, uint32_t b1, uint32_t b2, uint32_t bw, uint32_t m0, uint32_t m1,
                      uint32_t m2) {
      const uint32_t eq = __builtin_amdgcn_ubfe(~((b0 ^ m0) | (b1 ^ m1) | (b2 ^ m2)), q, (uint32_t)W);  // Peq[text[col]]
      uint32_t x = eq | vn;
      const uint32_t d0 = ((vp + (x & vp)) ^ vp) | x;
      const uint32_t hn = vp & d0;
      const uint32_t hp = vn | ~(vp | d0);
      x = d0 >> 1;
      vn = x & hp;
      vp = hn | ~(x | hp);
      const uint32_t same = eq & ~__builtin_amdgcn_ubfe(bw, q, (uint32_t)W);  // the characters themselves are equal
      dm |= __builtin_amdgcn_ubfe(same, (uint32_t)start, 1u) << q;  // this step's columns that are equal on the end position's diagonal
      // What the walk asks of a cell is one of four things: match (D0 and equal characters), mismatch (not D0),
      // insertion (D0, unequal, HP), deletion (D0, unequal, not HP) — two bits per diagonal, as planes
      // P = match | deletion and Q = match | insertion (so: D0 = P | Q, equal characters = P & Q, HP where it matters = Q).
      hist.put(col + q, (HistT)(d0 & (same | ~hp) & band) | ((HistT)(d0 & (same | hp) & band) << W));
    };
    for (int step = 0; step < n_steps; ++step) {
      const int col = step << 4, sub = step % kStepsPerPlaneLoad;
      const uint4 r = rw;
      if (sub == 0) {
        W0 = W0n, W1 = W1n, W2 = W2n, W3 = W3n;
        if (step + kStepsPerPlaneLoad < n_steps) {
          const int nc = col + 16 * kStepsPerPlaneLoad;
          W0n = plane_chunk(0, nc), W1n = plane_chunk(1, nc), W2n = plane_chunk(2, nc), W3n = plane_chunk(3, nc);
        }
      } else {
        window_advance16(W0), window_advance16(W1), window_advance16(W2), window_advance16(W3);
      }
      if (step + 1 < n_steps) rw = text_chunk(col + 16);
      // ((pat_abs + 96 k) & 7 == pat_abs & 7)
      const uint32_t b0 = window_head(W0, pat_bit), b1 = window_head(W1, pat_bit), b2 = window_head(W2, pat_bit), bw = window_head(W3, pat_bit);
      odd_ref |= bw;
      const uint32_t w[4] = {dir ? __builtin_bswap32(r.w) : r.x, dir ? __builtin_bswap32(r.z) : r.y,
                             dir ? __builtin_bswap32(r.y) : r.z, dir ? __builtin_bswap32(r.x) : r.w};
      const int ncol = L - col < 16 ? L - col : 16;
      uint32_t cw[4], nw[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        uint32_t odd;
        decode4(w[k], complement, cw[k], nw[k], odd);
        const int nb = ncol - 4 * k;  // characters of this word that belong to the read
        odd_text |= nb >= 4 ? odd : nb > 0 ? odd & ((1u << (8 * nb)) - 1u) : 0u;
      }
      if (ncol == 16) {
#pragma unroll
        for (int q = 0; q < 16; ++q)
          column((uint32_t)col, (uint32_t)q, b0, b1, b2, bw, (uint32_t)__builtin_amdgcn_sbfe((int)cw[q >> 2], 8 * (q & 3), 1),
                 (uint32_t)__builtin_amdgcn_sbfe((int)cw[q >> 2], 8 * (q & 3) + 1, 1),
                 (uint32_t)__builtin_amdgcn_sbfe((int)nw[q >> 2], 8 * (q & 3), 1));
      } else {  // up to fifteen trailing columns
        const uint64_t clo = ((uint64_t)cw[1] << 32) | cw[0], chi = ((uint64_t)cw[3] << 32) | cw[2];
        const uint64_t nlo = ((uint64_t)nw[1] << 32) | nw[0], nhi = ((uint64_t)nw[3] << 32) | nw[2];
        for (int q = 0; q < ncol; ++q) {
          const uint32_t cb = (uint32_t)((q < 8 ? clo : chi) >> (8 * (q & 7)));
          const uint32_t nb = (uint32_t)((q < 8 ? nlo : nhi) >> (8 * (q & 7)));
          column((uint32_t)col, (uint32_t)q, b0, b1, b2, bw, 0u - (cb & 1u), 0u - ((cb >> 1) & 1u), 0u - (nb & 1u));
        }
      }
      const uint32_t bad = ~dm & (ncol == 16 ? 0xFFFFu : (1u << ncol) - 1u);
      if (bad) last_bad = col + 31 - (int)__builtin_clz(bad);
      dm = 0;
    }
    if (dir == 0 && odd_text) punt = true;  // a read character outside "ACGTN": character equality is not code equality

    uint32_t n_ops = 0, n_md = 0;
    uint8_t *md = p.t_md + (size_t)rec * p.md_cap;
    auto push_op = [&](uint32_t op, uint32_t len) {
      if (n_ops < p.ops_cap && n_ops < p.fast_ops && len < (1u << 14)) ops[n_ops * nl + ln] = (uint16_t)((len << 2) | op); else punt = true;
      ++n_ops;
    };
    auto push_md = [&](uint32_t ch) {
      if (n_md < p.md_cap) md[n_md] = (uint8_t)ch; else punt = true;
      ++n_md;
    };
    auto push_number = [&](uint32_t v) {  // divisions by constants only (multiply + shift)
      if (v >= 10000u) {
        uint32_t div = 10000u;
        while (v / div >= 10u) div *= 10u;
        for (; div >= 10000u; div /= 10u) push_md('0' + (v / div) % 10u);
        v %= 10000u;
        push_md('0' + v / 1000u), push_md('0' + (v / 100u) % 10u), push_md('0' + (v / 10u) % 10u), push_md('0' + v % 10u);
        return;
      }
      if (v >= 1000u) push_md('0' + v / 1000u);
      if (v >= 100u) push_md('0' + (v / 100u) % 10u);
      if (v >= 10u) push_md('0' + (v / 10u) % 10u);
      push_md('0' + v % 10u);
    };
    bool broken = false;
    uint32_t lead = 0;  // leading read bases the walk never visited: exact matches when no odd reference character is near
    if (!punt && last_bad < 0) {  // src/align.c:294-300
      push_op(kOpM, (uint32_t)L);
      push_number((uint32_t)L);
    } else if (!punt) {
      // ---- walk back (src/align.c:340-440); pe == t + bit throughout ----
      int bit = start, t = L - 1, n_err = 0;
      uint32_t cur_op = kOpS, cur_n = 1;
      // The read positions of the walk's mismatch steps, the leftmost in the low byte: what the MD tag needs to know
      // about an M run besides its length (every other base of it is a match).  Where that does not say it all — see
      // use_hist below — the MD loop reads the history instead.
      uint64_t mm = 0;
      uint32_t n_mm = 0;
      bool use_hist = L > 255;  // (a position is kept in eight bits)
      // Behind the last column that differs on the end position's diagonal the walk only matches (equal characters
      // set D0, and match is the first thing it tests): it starts at that column with the M run already counted.
      const uint32_t trail = (uint32_t)(L - 1 - last_bad);
      if (trail) {
        t = last_bad, cur_op = kOpM, cur_n = trail;
      } else {  // the first step replaces the initial pseudo-run (src/align.c:345-368)
        const HistT h = hist.get((uint32_t)t) >> bit;
        const bool pp = (uint32_t)h & 1u, qq = (uint32_t)(h >> W) & 1u;
        const bool d = pp || qq, same = pp && qq, horiz = qq;
        if (d && same) --t, cur_op = kOpM;
        else if (!d) mm = (uint64_t)(uint32_t)t, n_mm = 1, --t, ++n_err;
        else if (horiz) --t, ++bit, ++n_err, ++start, use_hist = true;  // a read-end insertion folds into the run that follows
        else broken = true;  // assert(1 == 0)
      }
      while (!broken && !punt && t >= 0 && n_err != ed) {
        if (bit < 0) {  // the reference's own guard; above the band it would read bits this pass does not keep
          broken = true;
          break;
        }
        if (bit > sh) {
          punt = true;
          break;
        }
        const HistT h = hist.get((uint32_t)t) >> bit;
        const bool pp = (uint32_t)h & 1u, qq = (uint32_t)(h >> W) & 1u;
        const bool d = pp || qq, same = pp && qq, horiz = qq;
        const bool is_match = d && same, is_ins = d && !same && horiz, is_del = d && !same && !horiz;  // else: mismatch
        const uint32_t op = is_del ? kOpD : is_ins ? kOpI : kOpM;
        const bool absorbed = cur_op == kOpS && !is_match && !is_del;  // read-end errors pile up in the pseudo-run
        // the pseudo-run takes an insertion, or ends in a deletion: the run it folds into is not what the walk stepped through
        use_hist |= cur_op == kOpS && (is_ins || is_del);
        mm = d ? mm : (mm << 8) | (uint64_t)(uint32_t)t;
        n_mm += (uint32_t)!d;
        t -= (int)!is_del;
        bit += (int)is_ins - (int)is_del;
        start += (int)is_ins - (int)is_del;
        n_err += (int)!is_match;
        if (absorbed || op == cur_op) {
          ++cur_n;
        } else if (cur_op == kOpS) {
          cur_op = op, cur_n += 1;  // S(n) followed by op(1) ends up as op(1 + n)
        } else {
          push_op(cur_op, cur_n);
          cur_op = op, cur_n = 1;
        }
      }
      if (!broken && !punt) {
        if (t >= 0 && n_err == ed && odd_ref == 0u) lead = (uint32_t)(t + 1);
        if (t >= 0) {
          if (cur_op == kOpM || cur_op == kOpS)
            cur_op = kOpM, cur_n += (uint32_t)(t + 1);
          else
            push_op(cur_op, cur_n), cur_op = kOpM, cur_n = (uint32_t)(t + 1);
        }
        if (cur_op == kOpS) broken = true; else push_op(cur_op, cur_n);
      }
      // leading bases the walk never visited match on codes; on characters too unless an odd reference character is near
      use_hist |= (t >= 0 && odd_ref != 0u) || n_mm > 8u;
      if (!broken && !punt && !use_hist) {
        // ---- MD (src/align.c:501-544) from the runs (produced right to left) and the mismatch positions: every base of
        //      an M run the walk stepped through as a match is a match of characters, as are the bases in front of the
        //      walk's last step (all ed edits found) and behind its first (`trail`) ----
        uint32_t run = 0, tp = 0;
        int rp = start;
        for (uint32_t k = n_ops; k-- > 0 && !punt;) {
          const uint32_t o = ops[k * nl + ln], op = o & 3u, n = o >> 2;
          if (op == kOpM) {
            const uint32_t end = tp + n;
            while (n_mm && ((uint32_t)mm & 0xFFu) < end) {
              const uint32_t at = (uint32_t)mm & 0xFFu;
              mm >>= 8, --n_mm;
              run += at - tp;
              if (run) push_number(run), run = 0;
              rp += (int)(at - tp);
              push_md(pattern[rp]);
              ++rp, tp = at + 1u;
            }
            run += end - tp, rp += (int)(end - tp), tp = end;
          } else if (op == kOpI) {
            tp += n;
          } else {
            if (rp < 0) {
              punt = true;
              break;
            }
            if (run) push_number(run), run = 0;
            push_md('^');
            for (uint32_t i = 0; i < n; ++i, ++rp) push_md(pattern[rp]);
          }
        }
        if (run) push_number(run);
      } else if (!broken && !punt) {
        // ---- MD over pattern + start, character equality read off the history ----
        uint32_t run = 0, tp = 0;
        int rp = start;
        for (uint32_t k = n_ops; k-- > 0 && !punt;) {
          const uint32_t o = ops[k * nl + ln], op = o & 3u, n = o >> 2;
          if (op == kOpM) {
            const int diag = rp - (int)tp;  // constant along the run
            if (diag < 0 || diag > sh) {
              punt = true;
              break;
            }
            uint32_t i = 0;
            if (tp == 0 && lead) {
              // The walk stopped with all ed edits found: the alignment's cost is ed, so these bases match on codes;
              // with only canonical characters around, on characters too (the history is not read for them).
              i = lead < n ? lead : n;
              run += i, rp += (int)i, tp += i;
            }
            // the rightmost run ends in `trail` matches the walk never visited either (k == 0: it is that run)
            const uint32_t n_walked = k == 0 && trail ? (n > trail ? n - trail : 0u) : n;
            for (; i < n_walked; ++i, ++rp, ++tp) {
              const HistT hd = hist.get(tp) >> diag;
              if ((uint32_t)hd & (uint32_t)(hd >> W) & 1u) {  // equal characters = P & Q
                ++run;
              } else {
                if (run) push_number(run), run = 0;
                push_md(pattern[rp]);
              }
            }
            if (i < n) run += n - i, rp += (int)(n - i), tp += n - i;
          } else if (op == kOpI) {
            tp += n;
          } else {
            if (rp < 0) {
              punt = true;
              break;
            }
            if (run) push_number(run), run = 0;
            push_md('^');
            for (uint32_t i = 0; i < n; ++i, ++rp) push_md(pattern[rp]);
          }
        }
        if (run) push_number(run);
      }
    }
    if (punt) {
      p.ovf_out[atomicAdd(&p.ctl[1], 1u)] = rec;
      p.n_ops[rec] = 0, p.n_md[rec] = 0;
      continue;
    }
    const uint32_t rank = rec - p.rec_begin[read];
    uint16_t flag = (uint16_t)((dir ? 16u : 0u) | (rank ? 256u : 0u));
    if (broken) flag |= kFlagBroken, start = 0, n_ops = 0, n_md = 0;
    uint32_t *out_ops = p.t_ops + (size_t)rec * p.ops_cap;
    for (uint32_t k = 0; k < n_ops; ++k) {
      const uint32_t o = ops[(n_ops - 1u - k) * nl + ln];
      out_ops[k] = ((o >> 2) << 4) | (o & 3u);
    }
    p.flag[rec] = flag;
    p.tid[rec] = tid;
    p.pos0[rec] = (uint32_t)start + (uint32_t)cand;
    p.nm[rec] = (uint8_t)ed;
    p.n_ops[rec] = n_ops, p.n_md[rec] = n_md;
    p.src_slot[rec] = 0u;
  }
}

struct CompactParams {
  uint32_t n_records;
  const uint32_t *src_slot, *n_ops, *n_md, *cigar_off, *md_off;
  const uint32_t *t_ops, *o_ops;  // first-pass and overflow staging
  const uint8_t *t_md, *o_md;
  uint32_t ops_cap, md_cap, o_ops_cap, o_md_cap;
  uint32_t *cigar;
  uint8_t *md;
};

__global__ void __launch_bounds__(256) compact_kernel(CompactParams p) {
  const uint32_t rec = blockIdx.x * blockDim.x + threadIdx.x;
  if (rec >= p.n_records) return;
  uint32_t slot = p.src_slot[rec];
  const uint32_t no = p.n_ops[rec], nm = p.n_md[rec], co = p.cigar_off[rec], mo = p.md_off[rec];
  if (slot & kSlotDiagonal) {  // trace_ident_kernel's records: one M run over the whole read
    p.cigar[co] = (slot & ~kSlotDiagonal) << 4;
    slot = 0;
  } else {
    const uint32_t *ops = slot ? p.o_ops + (size_t)(slot - 1u) * p.o_ops_cap : p.t_ops + (size_t)rec * p.ops_cap;
    for (uint32_t i = 0; i < no; ++i) p.cigar[co + i] = ops[i];
  }
  const uint8_t *md = slot ? p.o_md + (size_t)(slot - 1u) * p.o_md_cap : p.t_md + (size_t)rec * p.md_cap;
  for (uint32_t i = 0; i < nm; ++i) p.md[mo + i] = md[i];
}

struct PairPlus {  // component-wise sum of (run count, MD length) pairs
  __host__ __device__ rocprim::tuple<uint32_t, uint32_t> operator()(const rocprim::tuple<uint32_t, uint32_t> &a,
                                                                   const rocprim::tuple<uint32_t, uint32_t> &b) const {
    return rocprim::make_tuple(rocprim::get<0>(a) + rocprim::get<0>(b), rocprim::get<1>(a) + rocprim::get<1>(b));
  }
};

struct TriplePlus {  // component-wise sum of (kept, runs, MD length) triples (mate rescue)
  __host__ __device__ rocprim::tuple<uint32_t, uint32_t, uint32_t> operator()(const rocprim::tuple<uint32_t, uint32_t, uint32_t> &a,
                                                                             const rocprim::tuple<uint32_t, uint32_t, uint32_t> &b) const {
    return rocprim::make_tuple(rocprim::get<0>(a) + rocprim::get<0>(b), rocprim::get<1>(a) + rocprim::get<1>(b),
                               rocprim::get<2>(a) + rocprim::get<2>(b));
  }
};

// The tail's buffers (fem_buf.hip.h): a quarter more than asked for, freed with the object.
template <typename T>
using DevBuf = femb::Buf<T, femb::Mem::Device, femb::Grow::Quarter>;
template <typename T>
using PinBuf = femb::Buf<T, femb::Mem::Pinned, femb::Grow::Quarter>;


// ---------------------------------------------------------------------------------------------------------
// SAM text.  One line per record, the fields generate_bam1_t packs (src/align.c:546-632) as htslib's sam_format1 prints
// them: QNAME FLAG RNAME POS 255 CIGAR * 0 0 SEQ QUAL NM:i MD:Z.  SEQ is the read as it came (src/align.c:79) through
// the 4-bit round trip of the BAM record (seq_nt16_table / seq_nt16_str: IUPAC letters upper-cased, anything else N);
// only a read's first record carries SEQ and QUAL (src/align.c:83-88).  Same bytes as fem_records_sam (fem_host.cc).
// SamParams::sam_seq (fem_dev_set_sam_seq, opt-in) turns SEQ and QUAL of the lines with 0x10 as the SAM specification has them.
// ---------------------------------------------------------------------------------------------------------
__device__ const uint8_t kSamSeqLut[256] = {
    78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78,
    78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 65, 67, 71, 84, 78, 78, 78, 78, 78, 78, 78, 78, 78, 61, 78, 78,
    78, 65, 66, 67, 68, 78, 78, 71, 72, 78, 78, 75, 78, 77, 78, 78, 78, 78, 82, 83, 84, 78, 86, 87, 78, 89, 78, 78, 78, 78, 78, 78,
    78, 65, 66, 67, 68, 78, 78, 71, 72, 78, 78, 75, 78, 77, 78, 78, 78, 78, 82, 83, 84, 78, 86, 87, 78, 89, 78, 78, 78, 78, 78, 78,
    78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78,
    78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78,
    78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78,
    78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78, 78,
};

struct SamParams {
  uint32_t n_records;
  const uint32_t *rec_begin, *s_read;
  const uint16_t *flag;
  const uint32_t *tid, *pos0;
  const uint8_t *nm;
  const uint32_t *cigar_off, *cigar, *md_off;
  const uint8_t *md;
  const uint8_t *bases;
  const uint64_t *read_off;
  const uint8_t *quals, *names;
  const uint64_t *name_off;
  const uint8_t *ref_names;
  const uint32_t *ref_name_off;
  unsigned long long *line_len;        // n_records + 1 (the last one zero)
  const unsigned long long *line_off;  // exclusive scan of line_len
  uint8_t *text;
  uint32_t *asserted;
  unsigned long long *qual_at;  // qual_hole: n_reads entries, set for the reads that have a record
  uint32_t qual_hole;           // the QUAL field of a primary record is sized but not written (quals == nullptr)
  // pair mode (the kernels' kPair instances): line k renders record perm[k] with FLAG pflag[k] and these mate columns
  const uint32_t *perm;
  const uint16_t *pflag;
  const uint32_t *mtid, *mpos0;  // 0xFFFFFFFF: the other mate has no record
  const int32_t *tlen;
  // MAPQ (fem_dev_set_mapq; nullptr: 255 on every line): single-end per read, its primary line's (the others 0); kPair per line
  const uint8_t *mapq;
  // lines for unmapped reads (fem_dev_set_unmapped; the kernels' kUnm instances): n_records then counts LINES, and line j
  // renders usrc[j]: below u_base a record (pair mode: a line of pair_kernel's), else the unmapped read usrc[j] - u_base
  const uint32_t *usrc;
  uint32_t u_base, n_reads;
  const uint32_t *u_lines;      // the length kernels: the line count itself (n_records there bounds it: lines behind it get length 0)
  const uint32_t *pair_begin;   // pair mode: pair_kernel's (mate m of pair i: its lines [pair_begin[2i+m], pair_begin[2i+m+1]))
  // the tags behind MD:Z (fem_dev_set_tags): NH:i HI:i on a mapped line, RG:Z on every line (an unmapped read's: behind QUAL)
  const uint8_t *rg;            // the read group's ID
  uint32_t rg_len;              // 0: no RG tag
  uint32_t hit_tags;            // != 0: NH and HI
  const uint32_t *hit_begin;    // n_reads + 1, by slot: slot s has the lines [hit_begin[s], hit_begin[s + 1]) ...
  uint32_t hit_by_line;         // ... of the output (the line filter's scan), else of the records (pair mode: of pair_kernel's lines)
  // the mate tags behind those (fem_dev_set_mate_tags; the kernels' kMate instances): MC:Z MQ:i ms:i
  uint32_t mate_tags;           // != 0: the kMate instances run
  const uint32_t *mate_begin;   // pair_kernel's pair_begin, with or without lines for unmapped reads (pair_begin above is theirs)
  const uint32_t *mate_score;   // per read, mate_score_kernel's; nullptr: no qualities on the device, no ms
  // SEQ and QUAL as SAM orders them (fem_dev_set_sam_seq): a line whose FLAG as written has 0x10 and that carries
  // SEQ prints the read's reverse complement and its qualities reversed (the write kernels alone: no length changes)
  uint32_t sam_seq;             // != 0: on
  // secondary lines folded into XA:Z (fem_dev_set_xa; nullptr: off; the kUnm instances alone read them).  By slot:
  // slot s's first line after folding is line xa_begin[s] and carries xa_n[s] entries of xa_bytes[s] bytes (both 0: no tag)
  const uint32_t *xa_begin, *xa_n, *xa_bytes;
};

// The complement of the letter kSamSeqLut prints: =ACMGRSVTWYHKDBN -> =TGKCYSBAWRDMHVN, the 4-bit BAM code with its bits reversed
__device__ __forceinline__ uint8_t sam_seq_complement(uint8_t ch) {
  const char *abc = "=ACMGRSVTWYHKDBN", *cba = "=TGKCYSBAWRDMHVN";
  uint8_t c = 'N';
  for (uint32_t k = 0; k < 16u; ++k)
    if ((uint8_t)abc[k] == ch) c = (uint8_t)cba[k];
  return c;
}

__device__ __forceinline__ uint32_t dec_digits(uint32_t v) {
  return v < 10u ? 1u : v < 100u ? 2u : v < 1000u ? 3u : v < 10000u ? 4u : v < 100000u ? 5u : v < 1000000u ? 6u
       : v < 10000000u ? 7u : v < 100000000u ? 8u : v < 1000000000u ? 9u : 10u;
}
__device__ __forceinline__ uint8_t *put_dec(uint8_t *w, uint32_t v) {
  const uint32_t n = dec_digits(v);
  for (uint32_t i = n; i-- > 0;) {
    w[i] = (uint8_t)('0' + v % 10u);
    v /= 10u;
  }
  return w + n;
}

// ---- lines for unmapped reads (include/fem_hip.h, fem_dev_set_unmapped) ----
constexpr uint32_t kNoMate = 0xFFFFFFFFu;

// Pair order: mate m of pair i (read m n/2 + i) is slot 2i + m
__device__ __forceinline__ uint32_t pair_slot(const SamParams &p, uint32_t r) {
  const uint32_t np = p.n_reads / 2u, m = r >= np ? 1u : 0u;
  return 2u * (r - m * np) + m;
}

// Where the unmapped mate of slot s's mapped read is placed: at that read's first line (no combination was chosen for such a
// pair, so it is the read's first single-end record, or its rescued one)
struct Placed {
  uint32_t t, pos0, rev;
};
__device__ __forceinline__ Placed placed_at(const SamParams &p, uint32_t s) {
  const uint32_t k0 = p.pair_begin[s], rec0 = p.perm[k0];
  return {p.tid[rec0], p.pos0[rec0], p.pflag[k0] & 16u};
}

// The line of unmapped read r: FLAG, and (t, pos0) where it is placed (kNoMate, 0xFFFFFFFF: unplaced, which print * and 0)
struct Unmapped {
  uint32_t r, flag, t, pos0;
};
template <bool kPair>
__device__ __forceinline__ Unmapped unmapped_line(const SamParams &p, uint32_t r) {
  Unmapped u{r, 4u, kNoMate, 0xFFFFFFFFu};
  if (kPair) {
    const uint32_t s = pair_slot(p, r), o = s ^ 1u;
    u.flag = 1u | 4u | ((s & 1u) ? 0x80u : 0x40u);
    if (p.pair_begin[o + 1] == p.pair_begin[o]) {
      u.flag |= 8u;
    } else {
      const Placed a = placed_at(p, o);
      u.t = a.t, u.pos0 = a.pos0;
      if (a.rev) u.flag |= 0x20u;
    }
  }
  return u;
}

// The mate columns of pair_kernel's line k (read r's).  kUnm: a line whose mate has no record names where that mate's line is
// placed, which is this read's own first line.
struct MateCols {
  uint32_t mt, mp;  // mt == kNoMate: "*" and "0"
  int32_t tl;
};
template <bool kUnm>
__device__ __forceinline__ MateCols mate_cols(const SamParams &p, uint32_t k, uint32_t r) {
  MateCols m{p.mtid[k], 0u, 0};
  if (m.mt != kNoMate) {
    m.mp = p.mpos0[k], m.tl = p.tlen[k];
  } else if (kUnm && p.pair_begin) {  // (nullptr: the kUnm instances without lines for unmapped reads, the line filter's)
    const Placed a = placed_at(p, pair_slot(p, r));
    m.mt = a.t, m.mp = a.pos0;
  }
  return m;
}

// RNEXT, PNEXT and TLEN of a line on sequence `tid` in pair mode, without the tabs around them (single-end: "*\t0\t0", 5 characters)
__device__ __forceinline__ uint32_t mate_cols_len(const SamParams &p, const MateCols &m, uint32_t tid) {
  if (m.mt == kNoMate) return 5u;
  const uint32_t rnext = m.mt == tid ? 1u : p.ref_name_off[m.mt + 1] - p.ref_name_off[m.mt];
  const uint32_t tl_len = m.tl < 0 ? 1u + dec_digits((uint32_t)-m.tl) : dec_digits((uint32_t)m.tl);
  return rnext + 1u + dec_digits(m.mp + 1u) + 1u + tl_len;
}

// What every line kernel first reads of line j: the record it renders (pair mode: perm[j]; else j itself), that record's
// read, the FLAG as written (0x8000 kept), whether the line is the read's primary one (SEQ, QUAL), the read's and its name's length.
struct LineHead {
  uint32_t rec, r, flag;
  bool primary;
  uint32_t L, name_len;
};
template <bool kPair>
__device__ __forceinline__ LineHead line_head(const SamParams &p, uint32_t j) {
  const uint32_t rec = kPair ? p.perm[j] : j, r = p.s_read[rec], flag = kPair ? p.pflag[j] : p.flag[rec];
  return {rec, r, flag, kPair ? !(flag & 256u) : p.rec_begin[r] == j, (uint32_t)(p.read_off[r + 1] - p.read_off[r]),
          (uint32_t)(p.name_off[r + 1] - p.name_off[r])};
}

// The MAPQ line j prints (r: its read)
template <bool kPair>
__device__ __forceinline__ uint32_t line_mapq(const SamParams &p, uint32_t j, uint32_t r, bool primary) {
  if (!p.mapq) return 255u;
  return kPair ? p.mapq[j] : primary ? p.mapq[r] : 0u;
}

// SEQ tab QUAL of a line that carries them (a read of length 0: "*\t*")
__device__ __forceinline__ uint32_t seq_qual_len(const SamParams &p, uint32_t L) {
  return L > 0 ? L + 1u + (p.quals || p.qual_hole ? L : 1u) : 3u;
}

// NH and HI of a mapped line: the lines its slot has in the output, and its 1-based place among them.  `line`
// is the line's number in the output, src the record (pair mode: pair_kernel's line) it renders, r its read.  Without the line
// filter a slot's lines are its records (pair mode: its lines of pair_kernel's) and stay together in their order, whether or not
// unmapped reads' lines stand between the slots, so both numbers come from that index; with it they come from the scan of
// report_kernel's counts.
struct HitTags {
  uint32_t nh, hi;
};
// kUnm with folding (p.xa_n): the numbers are those of the index before folding.  A folded line is still a reported hit, and the folded
// ones are the slot's lines 2 .. xa_n + 1, so the slot's count and the place of every line behind its first grow by xa_n.
template <bool kPair, bool kUnm = false>
__device__ __forceinline__ HitTags hit_tags(const SamParams &p, uint32_t line, uint32_t src, uint32_t r) {
  const uint32_t s = kPair ? pair_slot(p, r) : r, b = p.hit_begin[s];
  HitTags h{p.hit_begin[s + 1] - b, (p.hit_by_line ? line : src) - b + 1u};
  if (kUnm && p.xa_n) {
    const uint32_t x = p.xa_n[s];
    h.nh += x;
    if (h.hi > 1u) h.hi += x;
  }
  return h;
}
// SAM: "\tNH:i:<n>\tHI:i:<i>" and "\tRG:Z:<ID>"
__device__ __forceinline__ uint32_t hit_tags_len(const HitTags &h) { return 12u + dec_digits(h.nh) + dec_digits(h.hi); }
__device__ __forceinline__ uint32_t rg_tag_len(const SamParams &p) { return p.rg_len ? 6u + p.rg_len : 0u; }
// BAM: NH and HI as type I (7 bytes each, whatever the value), RG as type Z (the ID and a NUL)
__device__ __forceinline__ uint32_t bam_tags_len(const SamParams &p, bool mapped) {
  return (mapped && p.hit_tags ? 14u : 0u) + (p.rg_len ? 4u + p.rg_len : 0u);
}

// ---- XA:Z (include/fem_hip.h, fem_dev_set_xa): the last field of a folding slot's first line ----
// The bytes of the entries that output line `line`, a line of read r, carries: its slot's where the line is the slot's first, else 0
template <bool kPair>
__device__ __forceinline__ uint32_t xa_bytes_at(const SamParams &p, uint32_t line, uint32_t r) {
  if (!p.xa_n) return 0u;
  const uint32_t s = kPair ? pair_slot(p, r) : r;
  return p.xa_begin[s] == line ? p.xa_bytes[s] : 0u;
}
// SAM: "\tXA:Z:" and the entries; BAM: 'X' 'A' 'Z', the entries and a NUL
__device__ __forceinline__ uint32_t sam_xa_len(uint32_t entry_bytes) { return entry_bytes ? 6u + entry_bytes : 0u; }
__device__ __forceinline__ uint32_t bam_xa_len(uint32_t entry_bytes) { return entry_bytes ? 4u + entry_bytes : 0u; }

// ---- the mate tags (include/fem_hip.h, fem_dev_set_mate_tags): MC:Z MQ:i ms:i, the last fields of every line of a
//      paired text ----
// What the lines of read r say of the other mate.  has: it has a record; then the CIGAR words [c0, c0 + n_ops) and the MAPQ column of
// its primary line, pair_kernel's first line of that slot (where placed_at looks, too).  has_ms: the batch has qualities on the device;
// ms is mate_score_kernel's number of the other read, mapped or not.
struct MateTags {
  bool has, has_ms;
  uint32_t c0, n_ops, mq, ms;
};
__device__ __forceinline__ MateTags mate_tags(const SamParams &p, uint32_t r) {
  const uint32_t np = p.n_reads / 2u, o = pair_slot(p, r) ^ 1u, k0 = p.mate_begin[o];
  MateTags m{p.mate_begin[o + 1] != k0, p.mate_score != nullptr, 0u, 0u, 0u, 0u};
  if (m.has) {
    const uint32_t rec0 = p.perm[k0];
    m.c0 = p.cigar_off[rec0], m.n_ops = p.cigar_off[rec0 + 1] - m.c0;
    m.mq = line_mapq<true>(p, k0, 0u, true);
  }
  if (m.has_ms) m.ms = p.mate_score[r < np ? r + np : r - np];
  return m;
}
// The characters of CIGAR words [c0, c0 + n_ops) as SAM prints them, and their printing
__device__ __forceinline__ uint32_t cigar_chars(const SamParams &p, uint32_t c0, uint32_t n_ops) {
  uint32_t n = 0;
  for (uint32_t c = c0; c < c0 + n_ops; ++c) n += dec_digits(p.cigar[c] >> 4) + 1u;
  return n;
}
__device__ __forceinline__ uint8_t *put_cigar_op(uint8_t *q, uint32_t op) {
  q = put_dec(q, op >> 4);
  *q++ = (uint8_t)"MIDNSHP=XB"[op & 0xFu];
  return q;
}
// SAM: "\tMC:Z:<cigar>" (cig: the CIGAR's characters; none for a primary line that prints *), "\tMQ:i:<n>", "\tms:i:<n>"
__device__ __forceinline__ uint32_t mate_tags_len(const MateTags &m, uint32_t cig) {
  return (m.has && m.n_ops ? 6u + cig : 0u) + (m.has ? 6u + dec_digits(m.mq) : 0u) + (m.has_ms ? 6u + dec_digits(m.ms) : 0u);
}
// BAM: MC as type Z (the characters and a NUL), MQ as type C, ms as type I
__device__ __forceinline__ uint32_t bam_mate_tags_len(const MateTags &m, uint32_t cig) {
  return (m.has && m.n_ops ? 4u + cig : 0u) + (m.has ? 4u : 0u) + (m.has_ms ? 7u : 0u);
}

// The line of an unmapped read: QNAME FLAG RNAME POS 0 * RNEXT PNEXT 0 SEQ QUAL, no tags but RG (and the mate tags behind it)
__device__ __forceinline__ uint32_t unmapped_len(const SamParams &p, const Unmapped &u) {
  const uint32_t name_len = (uint32_t)(p.name_off[u.r + 1] - p.name_off[u.r]), L = (uint32_t)(p.read_off[u.r + 1] - p.read_off[u.r]);
  const uint32_t rname = u.t == kNoMate ? 1u : p.ref_name_off[u.t + 1] - p.ref_name_off[u.t], pos = dec_digits(u.pos0 + 1u);
  return name_len + 1u + dec_digits(u.flag) + 1u + rname + 1u + pos + 5u + (u.t == kNoMate ? 5u : 4u + pos) + 1u + seq_qual_len(p, L) +
         rg_tag_len(p) + 1u;
}

template <bool kPair, bool kUnm = false, bool kMate = false>
__global__ void __launch_bounds__(256) sam_len_kernel(SamParams p) {
  static_assert(kPair || !kMate, "mate tags are a paired text's");
  auto mates = [&](uint32_t r) -> uint32_t {  // the mate tags of a line of read r
    const MateTags m = mate_tags(p, r);
    return mate_tags_len(m, cigar_chars(p, m.c0, m.n_ops));
  };
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i <= p.n_records; i += stride) {
    if (i == p.n_records || (kUnm && i >= p.u_lines[0])) {
      p.line_len[i] = 0;
      continue;
    }
    uint32_t j = i;  // the record (pair mode: pair_kernel's line) that line i renders
    if (kUnm) {
      j = p.usrc[i];
      if (j >= p.u_base) {
        p.line_len[i] = unmapped_len(p, unmapped_line<kPair>(p, j - p.u_base)) + (kMate ? mates(j - p.u_base) : 0u);
        continue;
      }
    }
    const auto [rec, r, flag, primary, L, name_len] = line_head<kPair>(p, j);
    const uint32_t t = p.tid[rec], rname_len = p.ref_name_off[t + 1] - p.ref_name_off[t];
    if (flag & 0x8000u) atomicAdd(p.asserted, 1u);
    uint32_t cig = 0;
    const uint32_t c0 = p.cigar_off[rec], c1 = p.cigar_off[rec + 1];
    for (uint32_t c = c0; c < c1; ++c) cig += dec_digits(p.cigar[c] >> 4) + 1u;
    if (c1 == c0) cig = 1;  // '*'
    const uint32_t md_len = p.md_off[rec + 1] - p.md_off[rec];
    const uint32_t seq_qual = primary ? seq_qual_len(p, L) : 3u;
    const uint32_t mate = kPair ? mate_cols_len(p, mate_cols<kUnm>(p, j, r), t) : 5u;
    const uint32_t mq = line_mapq<kPair>(p, j, r, primary);
    const uint32_t tags = (p.hit_tags ? hit_tags_len(hit_tags<kPair, kUnm>(p, i, j, r)) : 0u) + rg_tag_len(p) + (kMate ? mates(r) : 0u) +
                          (kUnm ? sam_xa_len(xa_bytes_at<kPair>(p, i, r)) : 0u);
    p.line_len[i] = (unsigned long long)name_len + 1u + dec_digits(flag & 0x7FFFu) + 1u + rname_len + 1u + dec_digits(p.pos0[rec] + 1u) + 2u +
                    dec_digits(mq) + cig + 2u + mate + seq_qual + 6u + dec_digits(p.nm[rec]) + 6u + md_len + tags + 1u;
  }
}

// One wave per 64 consecutive records.  First every lane takes a record of its own: its numbers (two levels of small loads —
// 64 records' worth in flight where one record per wave had one, which made the kernel wait for memory 1.4 ms per million
// records), where each field of its line starts, and the short fields (numbers, separators, tags), written by the lane itself.
// Then the wave goes through its records two at a time, the long fields (QNAME, RNAME, SEQ, QUAL, MD) a byte per lane, every
// load of a pair requested before the first store; what a lane knows of record i reaches the others by v_readlane.
// kPair: j counts lines, each rendering record perm[j] with the pair's FLAG and mate columns (the lane writes those itself).
// kUnm: a line may be an unmapped read's, one more shape of line: QNAME, SEQ and QUAL its long fields (a placed one's RNAME too),
// no CIGAR, no MD, no tags but RG.
// The tags behind MD:Z (p.hit_tags, p.rg_len: the same in every lane): NH and HI are short fields; the ID is a long one, the same
// bytes on every line, so each lane loads its bytes of it (up to four: 255 characters) once, in front of the records.
// kMate: MC, MQ and ms are three more short fields of the lane's own line, the other mate's first CIGAR operations in registers as
// the line's own are.
// p.sam_seq (the same in every lane): whether a record's SEQ and QUAL are turned travels with its other numbers (Rec::rev); a
// turned record loads base and quality L - 1 - k where the others load k and prints through the table's second half.
template <bool kPair, bool kUnm = false, bool kMate = false>
__global__ void __launch_bounds__(256) sam_write_kernel(SamParams p) {
  static_assert(kPair || !kMate, "mate tags are a paired text's");
  __shared__ uint8_t lut[512];  // the letter a read character prints; from 256 on that letter's complement (p.sam_seq)
  lut[threadIdx.x] = kSamSeqLut[threadIdx.x];
  if (p.sam_seq) lut[256u + threadIdx.x] = sam_seq_complement(kSamSeqLut[threadIdx.x]);
  __syncthreads();
  const uint32_t ln = threadIdx.x & 63u;
  const uint32_t j0 = ((blockIdx.x * blockDim.x + threadIdx.x) >> 6) * 64u;
  if (j0 >= p.n_records) return;
  const uint32_t n_here = p.n_records - j0 < 64u ? p.n_records - j0 : 64u;
  const bool mine = ln < n_here;
  const uint32_t j = j0 + (mine ? ln : n_here - 1u);  // (lanes behind the last record repeat its loads and write nothing)
  uint32_t src = j;  // the record (pair mode: pair_kernel's line) that line j renders; kUnm: or an unmapped read
  bool unm = false;
  if (kUnm) src = p.usrc[j], unm = src >= p.u_base;
  const unsigned long long at = p.line_off[j];
  // level 1
  uint32_t r, t, flag, pos1, nm = 0, c0 = 0, c1 = 0, m0 = 0, md_len = 0;
  Unmapped um{};
  if (kUnm && unm) {
    um = unmapped_line<kPair>(p, src - p.u_base);
    r = um.r, t = um.t, flag = um.flag, pos1 = um.pos0 + 1u;
  } else {
    const uint32_t rec = kPair ? p.perm[src] : src;
    r = p.s_read[rec];
    t = p.tid[rec];
    flag = (kPair ? p.pflag[src] : p.flag[rec]) & 0x7FFFu, pos1 = p.pos0[rec] + 1u, nm = p.nm[rec];
    c0 = p.cigar_off[rec], c1 = p.cigar_off[rec + 1], m0 = p.md_off[rec], md_len = p.md_off[rec + 1] - m0;
  }
  // level 2
  const bool primary = (kUnm && unm) || (kPair ? !(flag & 256u) : p.rec_begin[r] == src);
  const uint64_t ro = p.read_off[r];
  const uint32_t L = (uint32_t)(p.read_off[r + 1] - ro);
  const uint64_t no = p.name_off[r];
  const uint32_t name_len = (uint32_t)(p.name_off[r + 1] - no);
  const bool no_t = kUnm && unm && t == kNoMate;  // an unplaced line: RNAME is the lane's own '*'
  const uint32_t rn0 = no_t ? 0u : p.ref_name_off[t], rname_len = no_t ? 0u : p.ref_name_off[t + 1] - rn0;
  uint32_t op_a = 0, op_b = 0, op_c = 0;  // the first CIGAR operations (most records have one to three)
  const uint32_t n_ops = c1 - c0;
  if (n_ops > 0) op_a = p.cigar[c0];
  if (n_ops > 1) op_b = p.cigar[c0 + 1];
  if (n_ops > 2) op_c = p.cigar[c0 + 2];
  const bool seq = primary && L > 0;
  const uint32_t mq = kUnm && unm ? 0u : line_mapq<kPair>(p, src, r, primary);
  MateCols mc{kNoMate, 0u, 0};
  if (kUnm && unm) mc.mt = um.t, mc.mp = um.pos0;
  else if (kPair) mc = mate_cols<kUnm>(p, src, r);
  uint32_t cig = 0;
  if (n_ops <= 3u) {
    if (n_ops > 0) cig += dec_digits(op_a >> 4) + 1u;
    if (n_ops > 1) cig += dec_digits(op_b >> 4) + 1u;
    if (n_ops > 2) cig += dec_digits(op_c >> 4) + 1u;
  } else {
    for (uint32_t c = c0; c < c1; ++c) cig += dec_digits(p.cigar[c] >> 4) + 1u;
  }
  if (n_ops == 0) cig = 1;
  // where the line's fields start (offsets from its first byte)
  const uint32_t o_flag = name_len + 1u;
  const uint32_t o_rname = o_flag + dec_digits(flag) + 1u;
  const uint32_t o_pos = o_rname + (no_t ? 1u : rname_len) + 1u;
  const uint32_t o_cig = o_pos + dec_digits(pos1) + 2u + dec_digits(mq);
  const uint32_t o_seq = o_cig + cig + 2u + (kPair ? mate_cols_len(p, mc, t) : 5u);
  const uint32_t o_tags = o_seq + (seq ? L + 1u + (p.quals || p.qual_hole ? L : 1u) : 3u);  // (an unmapped read's line ends here)
  const uint32_t o_nm = o_tags + 6u;
  const uint32_t o_md = kUnm && unm ? o_tags : o_nm + dec_digits(nm) + 6u;
  const bool hits = p.hit_tags && !(kUnm && unm);
  HitTags ht{};
  if (hits) ht = hit_tags<kPair, kUnm>(p, j, src, r);
  const uint32_t o_hit = o_md + md_len;
  const uint32_t o_rg = o_hit + (hits ? hit_tags_len(ht) : 0u);
  const uint32_t o_mate = o_rg + rg_tag_len(p);
  MateTags mt{};
  uint32_t mop_a = 0, mop_b = 0, mop_c = 0, mate_len = 0;
  if (kMate) {
    mt = mate_tags(p, r);
    if (mt.n_ops > 0) mop_a = p.cigar[mt.c0];
    if (mt.n_ops > 1) mop_b = p.cigar[mt.c0 + 1];
    if (mt.n_ops > 2) mop_c = p.cigar[mt.c0 + 2];
    uint32_t mcig = 0;
    if (mt.n_ops <= 3u) {
      if (mt.n_ops > 0) mcig += dec_digits(mop_a >> 4) + 1u;
      if (mt.n_ops > 1) mcig += dec_digits(mop_b >> 4) + 1u;
      if (mt.n_ops > 2) mcig += dec_digits(mop_c >> 4) + 1u;
    } else {
      mcig = cigar_chars(p, mt.c0, mt.n_ops);
    }
    mate_len = mate_tags_len(mt, mcig);
  }
  // (the room of a folding slot's XA:Z lies in front of the newline: xa_write_kernel fills it)
  const uint32_t o_end = o_mate + mate_len + (kUnm && !unm ? sam_xa_len(xa_bytes_at<kPair>(p, j, r)) : 0u);
  if (mine) {  // the short fields of the lane's own record
    uint8_t *w = p.text + at;
    w[name_len] = '\t';
    put_dec(w + o_flag, flag)[0] = '\t';
    if (no_t) w[o_rname] = '*';
    w[o_pos - 1u] = '\t';
    uint8_t *q = put_dec(w + o_pos, pos1);
    q[0] = '\t';
    put_dec(q + 1, mq)[0] = '\t';
    q = w + o_cig;
    if (n_ops == 0) *q++ = '*';
    if (n_ops <= 3u) {
      if (n_ops > 0) q = put_dec(q, op_a >> 4), *q++ = (uint8_t)"MIDNSHP=XB"[op_a & 0xFu];
      if (n_ops > 1) q = put_dec(q, op_b >> 4), *q++ = (uint8_t)"MIDNSHP=XB"[op_b & 0xFu];
      if (n_ops > 2) q = put_dec(q, op_c >> 4), *q++ = (uint8_t)"MIDNSHP=XB"[op_c & 0xFu];
    } else {
      for (uint32_t c = c0; c < c1; ++c) {
        const uint32_t op = p.cigar[c];
        q = put_dec(q, op >> 4);
        *q++ = (uint8_t)"MIDNSHP=XB"[op & 0xFu];
      }
    }
    if (!kPair) {
      q[0] = '\t', q[1] = '*', q[2] = '\t', q[3] = '0', q[4] = '\t', q[5] = '0', q[6] = '\t';
    } else {  // RNEXT PNEXT TLEN
      const uint32_t mt = mc.mt;
      *q++ = '\t';
      if (mt == kNoMate) {
        q[0] = '*', q[1] = '\t', q[2] = '0', q[3] = '\t', q[4] = '0', q[5] = '\t';
      } else {
        if (mt == t) {
          *q++ = '=';
        } else {  // the other mate on another sequence (rare: its name a byte at a time)
          const uint32_t n0 = p.ref_name_off[mt], n1 = p.ref_name_off[mt + 1];
          for (uint32_t c = n0; c < n1; ++c) *q++ = p.ref_names[c];
        }
        *q++ = '\t';
        q = put_dec(q, mc.mp + 1u);
        *q++ = '\t';
        const int32_t tl = mc.tl;
        if (tl < 0) *q++ = '-';
        q = put_dec(q, tl < 0 ? (uint32_t)-tl : (uint32_t)tl);
        *q = '\t';
      }
    }
    uint8_t *w_seq = w + o_seq;
    if (seq) {
      w_seq[L] = '\t';
      if (p.qual_hole) p.qual_at[r] = at + o_seq + L + 1u;  // (the caller has the qualities: it writes them here)
      else if (!p.quals) w_seq[L + 1u] = '*';
    } else {
      w_seq[0] = '*', w_seq[1] = '\t', w_seq[2] = '*';
    }
    if (!(kUnm && unm)) {
      q = w + o_tags;
      q[0] = '\t', q[1] = 'N', q[2] = 'M', q[3] = ':', q[4] = 'i', q[5] = ':';
      q = put_dec(w + o_nm, nm);
      q[0] = '\t', q[1] = 'M', q[2] = 'D', q[3] = ':', q[4] = 'Z', q[5] = ':';
    }
    if (hits) {
      q = w + o_hit;
      q[0] = '\t', q[1] = 'N', q[2] = 'H', q[3] = ':', q[4] = 'i', q[5] = ':';
      q = put_dec(q + 6, ht.nh);
      q[0] = '\t', q[1] = 'H', q[2] = 'I', q[3] = ':', q[4] = 'i', q[5] = ':';
      put_dec(q + 6, ht.hi);
    }
    if (p.rg_len) {
      q = w + o_rg;
      q[0] = '\t', q[1] = 'R', q[2] = 'G', q[3] = ':', q[4] = 'Z', q[5] = ':';
    }
    if (kMate) {
      q = w + o_mate;
      if (mt.has && mt.n_ops) {
        q[0] = '\t', q[1] = 'M', q[2] = 'C', q[3] = ':', q[4] = 'Z', q[5] = ':';
        q += 6;
        if (mt.n_ops <= 3u) {
          q = put_cigar_op(q, mop_a);
          if (mt.n_ops > 1) q = put_cigar_op(q, mop_b);
          if (mt.n_ops > 2) q = put_cigar_op(q, mop_c);
        } else {
          for (uint32_t c = mt.c0; c < mt.c0 + mt.n_ops; ++c) q = put_cigar_op(q, p.cigar[c]);
        }
      }
      if (mt.has) {
        q[0] = '\t', q[1] = 'M', q[2] = 'Q', q[3] = ':', q[4] = 'i', q[5] = ':';
        q = put_dec(q + 6, mt.mq);
      }
      if (mt.has_ms) {
        q[0] = '\t', q[1] = 'm', q[2] = 's', q[3] = ':', q[4] = 'i', q[5] = ':';
        put_dec(q + 6, mt.ms);
      }
    }
    w[o_end] = '\n';
  }
  // ---- the long fields, record by record, all lanes ----
  const uint32_t at_lo = (uint32_t)at, at_hi = (uint32_t)(at >> 32), no_lo = (uint32_t)no, no_hi = (uint32_t)(no >> 32);
  const uint32_t ro_lo = (uint32_t)ro, ro_hi = (uint32_t)(ro >> 32);
  const uint32_t L_seq = seq ? L : 0u;  // (no SEQ / QUAL bytes on a read's further records)
  // p.sam_seq: a line with 0x10 takes base and quality L - 1 - k where the others take k (an unmapped read's line has no 0x10)
  const uint32_t rev = p.sam_seq && (flag & 16u) ? 1u : 0u;
  struct Rec {
    uint8_t *w;
    const uint8_t *name, *rname, *md, *bases, *quals;
    uint32_t name_len, rname_len, md_len, L, o_rname, o_md, o_seq, o_id, rev;
  };
  uint8_t id[4] = {0, 0, 0, 0};  // the lane's bytes of the read group's ID
  if (p.rg_len) {
    for (uint32_t c = 0; c < 4u; ++c)
      if (ln + 64u * c < p.rg_len) id[c] = p.rg[ln + 64u * c];
  }
  auto rl = [](uint32_t v, uint32_t i) -> uint32_t { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)i); };
  auto record = [&](uint32_t i) -> Rec {
    Rec x;
    x.w = p.text + ((uint64_t)rl(at_lo, i) | (uint64_t)rl(at_hi, i) << 32);
    x.name = p.names + ((uint64_t)rl(no_lo, i) | (uint64_t)rl(no_hi, i) << 32);
    const uint64_t ro_i = (uint64_t)rl(ro_lo, i) | (uint64_t)rl(ro_hi, i) << 32;
    x.bases = p.bases + ro_i, x.quals = p.quals ? p.quals + ro_i : nullptr;
    x.rname = p.ref_names + rl(rn0, i), x.md = p.md + rl(m0, i);
    x.name_len = rl(name_len, i), x.rname_len = rl(rname_len, i), x.md_len = rl(md_len, i), x.L = rl(L_seq, i);
    x.o_rname = rl(o_rname, i), x.o_md = rl(o_md, i), x.o_seq = rl(o_seq, i);
    x.o_id = p.rg_len ? rl(o_rg, i) + 6u : 0u;
    x.rev = p.sam_seq ? rl(rev, i) : 0u;
    return x;
  };
  struct Bytes {
    uint8_t n, rn, m, sA, sB, qA, qB;
  };
  const uint32_t k1 = ln + 64u;
  auto load = [&](const Rec &x) -> Bytes {
    Bytes b{};
    if (ln < x.name_len) b.n = x.name[ln];
    if (ln < x.rname_len) b.rn = x.rname[ln];
    if (ln < x.md_len) b.m = x.md[ln];
    const uint32_t kA = x.rev ? x.L - 1u - ln : ln, kB = x.rev ? x.L - 1u - k1 : k1;  // (read only where ln, k1 < L)
    if (ln < x.L) b.sA = x.bases[kA];
    if (k1 < x.L) b.sB = x.bases[kB];
    if (x.quals) {
      if (ln < x.L) b.qA = x.quals[kA];
      if (k1 < x.L) b.qB = x.quals[kB];
    }
    return b;
  };
  auto store = [&](const Rec &x, const Bytes &b) {
    uint8_t *w_seq = x.w + x.o_seq, *w_rname = x.w + x.o_rname, *w_md = x.w + x.o_md;
    if (ln < x.name_len) x.w[ln] = b.n;
    if (ln < x.rname_len) w_rname[ln] = b.rn;
    if (ln < x.md_len) w_md[ln] = b.m;
    const uint8_t *tab = lut + (x.rev << 8);
    if (ln < x.L) w_seq[ln] = tab[b.sA];
    if (k1 < x.L) w_seq[k1] = tab[b.sB];
    if (x.quals) {
      if (ln < x.L) w_seq[x.L + 1u + ln] = b.qA;
      if (k1 < x.L) w_seq[x.L + 1u + k1] = b.qB;
    }
    // fields beyond what a lane holds (wave-uniform conditions): names and reference names over 64 characters, MD strings
    // over 64, reads over 128
    for (uint32_t k = k1; k < x.name_len; k += 64u) x.w[k] = x.name[k];
    for (uint32_t k = k1; k < x.rname_len; k += 64u) w_rname[k] = x.rname[k];
    for (uint32_t k = k1; k < x.md_len; k += 64u) w_md[k] = x.md[k];
    for (uint32_t k = ln + 128u; k < x.L; k += 64u) {
      const uint32_t from = x.rev ? x.L - 1u - k : k;
      w_seq[k] = tab[x.bases[from]];
      if (x.quals) w_seq[x.L + 1u + k] = x.quals[from];
    }
    if (p.rg_len) {
      uint8_t *w_id = x.w + x.o_id;
      for (uint32_t c = 0; c < 4u; ++c)
        if (ln + 64u * c < p.rg_len) w_id[ln + 64u * c] = id[c];
    }
  };
  uint32_t i = 0;
  for (; i + 1u < n_here; i += 2u) {
    const Rec xa = record(i), xb = record(i + 1u);
    const Bytes ba = load(xa), bb = load(xb);
    store(xa, ba);
    store(xb, bb);
  }
  if (i < n_here) {
    const Rec xa = record(i);
    store(xa, load(xa));
  }
}

// ---------------------------------------------------------------------------------------------------------
// BAM records (SAM/BAM specification §4.2): the same lines as the SAM kernels, field for field.  refID pos = tid pos0,
// l_read_name = name + NUL, MAPQ 255 (or line_mapq's), bin = reg2bin(pos0, end0) (end0 = pos0 + the M/D/N/=/X lengths, pos0 + 1 for none),
// the device's CIGAR words as they are, FLAG & 0x7FFF, l_seq = L where SAM prints SEQ else 0, mate columns -1 -1 0 (single-end)
// or pair_kernel's, SEQ in 4-bit codes (the SAM round trip's letters), QUAL - 33 (0xFF where SAM prints *), NM:C, MD:Z.
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t bam_reg2bin(uint32_t beg, uint32_t end) {  // spec §5.3, end exclusive
  --end;
  if (beg >> 14 == end >> 14) return ((1u << 15) - 1u) / 7u + (beg >> 14);
  if (beg >> 17 == end >> 17) return ((1u << 12) - 1u) / 7u + (beg >> 17);
  if (beg >> 20 == end >> 20) return ((1u << 9) - 1u) / 7u + (beg >> 20);
  if (beg >> 23 == end >> 23) return ((1u << 6) - 1u) / 7u + (beg >> 23);
  if (beg >> 26 == end >> 26) return ((1u << 3) - 1u) / 7u + (beg >> 26);
  return 0;
}

// Record sizes (block_size + 4); a read name over 254 characters in the batch sets *bad_name (l_read_name is a uint8).
template <bool kPair, bool kUnm = false, bool kMate = false>
__global__ void __launch_bounds__(256) bam_len_kernel(SamParams p, uint32_t n_reads, uint32_t *bad_name) {
  static_assert(kPair || !kMate, "mate tags are a paired text's");
  auto mates = [&](uint32_t r) -> uint32_t {  // the mate tags of a record of read r
    const MateTags m = mate_tags(p, r);
    return bam_mate_tags_len(m, cigar_chars(p, m.c0, m.n_ops));
  };
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_reads; r += stride)
    if (p.name_off[r + 1] - p.name_off[r] > 254u) atomicOr(bad_name, 1u);
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i <= p.n_records; i += stride) {
    if (i == p.n_records || (kUnm && i >= p.u_lines[0])) {
      p.line_len[i] = 0;
      continue;
    }
    uint32_t j = i;  // (as sam_len_kernel)
    if (kUnm) {
      j = p.usrc[i];
      if (j >= p.u_base) {  // an unmapped read: no CIGAR, SEQ and QUAL, no tags but RG
        const uint32_t r = j - p.u_base, L = (uint32_t)(p.read_off[r + 1] - p.read_off[r]);
        p.line_len[i] = 36ull + (uint32_t)(p.name_off[r + 1] - p.name_off[r]) + 1u + (L + 1u) / 2u + L + bam_tags_len(p, false) +
                        (kMate ? mates(r) : 0u);
        continue;
      }
    }
    const auto [rec, r, flag, primary, L, name_len] = line_head<kPair>(p, j);
    if (flag & 0x8000u) atomicAdd(p.asserted, 1u);
    const uint32_t n_ops = p.cigar_off[rec + 1] - p.cigar_off[rec], md_len = p.md_off[rec + 1] - p.md_off[rec];
    const uint32_t ls = primary ? L : 0u;
    p.line_len[i] = 36ull + name_len + 1u + 4u * n_ops + (ls + 1u) / 2u + ls + 4u + 4u + md_len + bam_tags_len(p, true) + (kMate ? mates(r) : 0u) +
                    (kUnm ? bam_xa_len(xa_bytes_at<kPair>(p, i, r)) : 0u);
  }
}

// One wave per record, a byte (or CIGAR word) per lane.  kMate: what the record says of the other mate is loaded in front of the
// record's own bytes (four loads in a row: pair_begin, perm, cigar_off, cigar); the other mate's CIGAR as characters an operation
// per lane, each lane's place the sum of the lengths in the lanes below it; MQ:C and ms:I a byte per lane.
template <bool kPair, bool kUnm = false, bool kMate = false>
__global__ void __launch_bounds__(256) bam_write_kernel(SamParams p) {
  static_assert(kPair || !kMate, "mate tags are a paired text's");
  __shared__ uint8_t code4[512];  // read character -> 4-bit code of the letter the SAM text prints; from 256 on of its complement
  {
    const uint8_t ch = kSamSeqLut[threadIdx.x];
    const char *abc = "=ACMGRSVTWYHKDBN";
    uint8_t c = 15;
    for (uint8_t k = 0; k < 16; ++k)
      if ((uint8_t)abc[k] == ch) c = k;
    code4[threadIdx.x] = c;
    if (p.sam_seq) code4[256u + threadIdx.x] = (uint8_t)(__builtin_bitreverse32(c) >> 28);  // (the complement: the code's bits reversed)
  }
  __syncthreads();
  const uint32_t ln = threadIdx.x & 63u;
  const uint32_t j = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (j >= p.n_records) return;
  uint32_t src = j;  // the record (pair mode: pair_kernel's line) that record j renders; kUnm: or an unmapped read
  bool unm = false;
  if (kUnm) src = p.usrc[j], unm = src >= p.u_base;
  uint32_t r, fl, ls, name_len, c0 = 0, n_ops = 0, m0 = 0, md_len = 0, tid, pos0, nm = 0, mq = 0, bin;
  uint32_t ntid = 0xFFFFFFFFu, npos = 0xFFFFFFFFu, tlen = 0;
  if (kUnm && unm) {  // (spec: an unplaced read has refID pos -1 -1 and the bin of that, 4680)
    const Unmapped u = unmapped_line<kPair>(p, src - p.u_base);
    r = u.r, fl = u.flag, tid = ntid = u.t, pos0 = npos = u.pos0;
    ls = (uint32_t)(p.read_off[r + 1] - p.read_off[r]), name_len = (uint32_t)(p.name_off[r + 1] - p.name_off[r]);
    bin = u.t == kNoMate ? 4680u : bam_reg2bin(pos0, pos0 + 1u);
  } else {
    const LineHead h = line_head<kPair>(p, src);
    const uint32_t rec = h.rec;
    r = h.r, fl = h.flag, name_len = h.name_len;
    ls = h.primary ? h.L : 0u;
    c0 = p.cigar_off[rec], n_ops = p.cigar_off[rec + 1] - c0;
    m0 = p.md_off[rec], md_len = p.md_off[rec + 1] - m0;
    tid = p.tid[rec], pos0 = p.pos0[rec], nm = p.nm[rec], mq = line_mapq<kPair>(p, src, r, h.primary);
    uint32_t span = 0;
    for (uint32_t c = ln; c < n_ops; c += 64u) {
      const uint32_t op = p.cigar[c0 + c], o = op & 0xFu;
      if (o == 0u || o == 2u || o == 3u || o == 7u || o == 8u) span += op >> 4;
    }
    for (uint32_t o = 32; o; o >>= 1) span += __shfl_xor(span, o);
    bin = bam_reg2bin(pos0, pos0 + (span ? span : 1u));
    if (kPair) {
      const MateCols mc = mate_cols<kUnm>(p, src, r);
      if (mc.mt != kNoMate) ntid = mc.mt, npos = mc.mp, tlen = (uint32_t)mc.tl;
    }
  }
  MateTags mt{};
  uint32_t mop = 0;  // kMate: the other mate's CIGAR operation ln
  if (kMate) {
    mt = mate_tags(p, r);
    if (ln < mt.n_ops) mop = p.cigar[mt.c0 + ln];
  }
  const uint64_t ro = p.read_off[r], no = p.name_off[r];
  const uint64_t at = p.line_off[j];
  const uint32_t size = (uint32_t)(p.line_off[j + 1] - at);
  uint8_t *w = p.text + at;
  if (ln < 36u) {
    const uint32_t q = ln >> 2;
    const uint32_t v = q == 0 ? size - 4u : q == 1 ? tid : q == 2 ? pos0 : q == 3 ? (name_len + 1u) | mq << 8 | bin << 16
                     : q == 4 ? n_ops | (fl & 0x7FFFu) << 16 : q == 5 ? ls : q == 6 ? ntid : q == 7 ? npos : tlen;
    w[ln] = (uint8_t)(v >> (8u * (ln & 3u)));
  }
  uint8_t *x = w + 36;
  const uint8_t *name = p.names + no;
  for (uint32_t k = ln; k <= name_len; k += 64u) x[k] = k < name_len ? name[k] : 0;
  x += name_len + 1u;
  for (uint32_t c = ln; c < n_ops; c += 64u) {
    const uint32_t op = p.cigar[c0 + c];
    uint8_t *y = x + 4u * c;
    y[0] = (uint8_t)op, y[1] = (uint8_t)(op >> 8), y[2] = (uint8_t)(op >> 16), y[3] = (uint8_t)(op >> 24);
  }
  x += 4u * n_ops;
  const uint8_t *bases = p.bases + ro;
  const uint32_t sb = (ls + 1u) / 2u;
  // p.sam_seq: a record with 0x10 holds the reversed read, position i of it base ls - 1 - i complemented; byte k the positions 2k
  // and 2k + 1 as ever, so with an odd ls the last byte's high nibble is base 0 and its low nibble stays 0
  // (the whole wave takes one side: a forward record runs the loops it ran before there was an option)
  const uint8_t *quals = p.quals ? p.quals + ro : nullptr;
  if (p.sam_seq && (fl & 16u) && !(kUnm && unm)) {
    const uint8_t *tab = code4 + 256;
    const uint32_t last = ls - 1u;
    for (uint32_t k = ln; k < sb; k += 64u) {
      const uint32_t hi = tab[bases[last - 2u * k]], lo = 2u * k + 1u < ls ? tab[bases[last - 2u * k - 1u]] : 0u;
      x[k] = (uint8_t)(hi << 4 | lo);
    }
    x += sb;
    for (uint32_t k = ln; k < ls; k += 64u) x[k] = quals ? (uint8_t)(quals[last - k] - 33u) : (uint8_t)0xFF;
  } else {
    for (uint32_t k = ln; k < sb; k += 64u) {
      const uint32_t hi = code4[bases[2u * k]], lo = 2u * k + 1u < ls ? code4[bases[2u * k + 1u]] : 0u;
      x[k] = (uint8_t)(hi << 4 | lo);
    }
    x += sb;
    for (uint32_t k = ln; k < ls; k += 64u) x[k] = quals ? (uint8_t)(quals[k] - 33u) : (uint8_t)0xFF;
  }
  x += ls;
  if (!(kUnm && unm)) {
    if (ln == 0) x[0] = 'N', x[1] = 'M', x[2] = 'C', x[3] = (uint8_t)nm, x[4] = 'M', x[5] = 'D', x[6] = 'Z';
    x += 7;
    const uint8_t *md = p.md + m0;
    for (uint32_t k = ln; k <= md_len; k += 64u) x[k] = k < md_len ? md[k] : 0;
    x += md_len + 1u;
    if (p.hit_tags) {  // NH:I HI:I, lane k byte k of the fourteen
      const HitTags ht = hit_tags<kPair, kUnm>(p, j, src, r);
      if (ln < 14u) {
        const uint32_t b = ln < 7u ? ln : ln - 7u, v = ln < 7u ? ht.nh : ht.hi;
        x[ln] = b < 3u ? (uint8_t)(ln < 7u ? "NHI" : "HII")[b] : (uint8_t)(v >> (8u * (b - 3u)));
      }
      x += 14;
    }
  }
  if (p.rg_len) {  // (an unmapped read's record has this one alone)
    if (ln < 3u) x[ln] = (uint8_t)"RGZ"[ln];
    x += 3;
    for (uint32_t k = ln; k <= p.rg_len; k += 64u) x[k] = k < p.rg_len ? p.rg[k] : 0;
    x += p.rg_len + 1u;
  }
  if (kMate) {
    if (mt.has && mt.n_ops) {
      if (ln < 3u) x[ln] = (uint8_t)"MCZ"[ln];
      uint8_t *y = x + 3;
      uint32_t done = 0;  // characters of the operations in front of this round's
      for (uint32_t cb = 0; cb < mt.n_ops; cb += 64u) {  // (a CIGAR of more than 64 operations goes round)
        const uint32_t c = cb + ln, op = cb == 0 ? mop : c < mt.n_ops ? p.cigar[mt.c0 + c] : 0u;
        const uint32_t len = c < mt.n_ops ? dec_digits(op >> 4) + 1u : 0u;
        uint32_t end = len;
        for (uint32_t o = 1; o < 64u; o <<= 1) {
          const uint32_t below = __shfl_up(end, o);
          if (ln >= o) end += below;
        }
        if (len) put_cigar_op(y + done + end - len, op);
        done += __shfl(end, 63);
      }
      if (ln == 0) y[done] = 0;
      x += 4u + done;
    }
    if (mt.has) {
      if (ln < 4u) x[ln] = ln < 3u ? (uint8_t)"MQC"[ln] : (uint8_t)mt.mq;
      x += 4;
    }
    if (mt.has_ms && ln < 7u) x[ln] = ln < 3u ? (uint8_t)"msI"[ln] : (uint8_t)(mt.ms >> (8u * (ln - 3u)));
  }
}

// ---------------------------------------------------------------------------------------------------------
// ms:i of the mate tags (fem_dev_set_mate_tags): score[r] = the sum of b - 33 over read r's quality bytes b with
// b - 33 >= 15.  One pass over the batch's qualities, 4 bytes written per read.  kScoreLanes lanes share a read, each taking 16
// ALIGNED bytes per step (a read starts wherever the one before ended: the bytes of a chunk in front of the read's first and behind
// its last are loaded and left out of the sum; a chunk that holds a byte of the array lies within its allocation).  Eight lanes
// cover 128 bytes, which holds a 100-base read at any alignment in one step, and eight such reads fill a wave; a longer read
// takes further steps.  The lanes' sums meet by shuffles within their group.
// ---------------------------------------------------------------------------------------------------------
constexpr uint32_t kScoreLanes = 8, kScoreChunk = 16;
__global__ void __launch_bounds__(256) mate_score_kernel(const uint8_t *quals, const uint64_t *read_off, uint32_t n_reads, uint32_t *score) {
  const uint32_t sub = threadIdx.x % kScoreLanes, r = blockIdx.x * (256u / kScoreLanes) + threadIdx.x / kScoreLanes;
  const bool live = r < n_reads;  // (the lanes behind the last read run no step and add zero to nobody's sum)
  const uintptr_t first = (uintptr_t)quals + (live ? read_off[r] : 0u), last = (uintptr_t)quals + (live ? read_off[r + 1] : 0u);
  uint32_t sum = 0;
  for (uintptr_t a = (first & ~(uintptr_t)(kScoreChunk - 1u)) + kScoreChunk * sub; a < last; a += kScoreChunk * kScoreLanes) {
    const uint4 v = *(const uint4 *)a;
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    // the chunk's bytes [lo, hi) are the read's (a whole chunk inside it: 0, 16)
    const uint32_t lo = a < first ? (uint32_t)(first - a) : 0u, hi = last - a < kScoreChunk ? (uint32_t)(last - a) : kScoreChunk;
#pragma unroll
    for (uint32_t k = 0; k < kScoreChunk; ++k) {
      const uint32_t b = w[k / 4u] >> (8u * (k % 4u)) & 0xFFu;
      if (k >= lo && k < hi && b >= 48u) sum += b - 33u;
    }
  }
  for (uint32_t o = kScoreLanes / 2u; o; o >>= 1) sum += __shfl_xor(sum, o);
  if (live && sub == 0) score[r] = sum;
}

// ---------------------------------------------------------------------------------------------------------
// The line index with lines for unmapped reads (fem_dev_set_unmapped).  A read has max(records, 1) lines.
// The reads in output order are the slots: read s single-end, mate m of pair i (slot 2i + m) in pair mode, where a slot's
// lines so far are [begin[s], begin[s + 1]) of the records (rec_begin) or of pair_kernel's lines (pair_begin, rescued mates
// included).  unmapped_mark_kernel: cnt[s] = 1 where slot s has none; an exclusive scan of cnt (the unmapped reads alone:
// one rocPRIM scan over the reads, not the lines); unmapped_src_kernel: line k of the lines so far moves behind the
// unmapped reads in front of its slot, usrc[k + before[s]] = k, and an unmapped slot's line goes where its records
// would have stood, usrc[begin[s] + before[s]] = n_base + its read.
// ---------------------------------------------------------------------------------------------------------
struct UlineParams {
  uint32_t n_reads, n_base;  // n_base: records (pair mode: pair_kernel's lines)
  const uint32_t *begin;     // n_reads + 1, by slot
  const uint32_t *s_read;    // per record
  uint32_t paired;
  const uint32_t *perm;      // pair mode: per line of pair_kernel's
  uint32_t *cnt;             // n_reads + 1 (the last one zero)
  const uint32_t *before;    // n_reads + 1: the exclusive scan of cnt
  uint32_t *usrc;            // n_base + before[n_reads]
  uint32_t *n_lines;         // that number
};

__global__ void __launch_bounds__(256) unmapped_mark_kernel(UlineParams p) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s <= p.n_reads) p.cnt[s] = s < p.n_reads && p.begin[s + 1] == p.begin[s] ? 1u : 0u;
}

__global__ void __launch_bounds__(256) unmapped_src_kernel(UlineParams p) {
  const uint32_t stride = gridDim.x * blockDim.x, first = blockIdx.x * blockDim.x + threadIdx.x, np = p.n_reads / 2u;
  if (first == 0) p.n_lines[0] = p.n_base + p.before[p.n_reads];
  for (uint32_t k = first; k < p.n_base; k += stride) {
    const uint32_t r = p.s_read[p.paired ? p.perm[k] : k];
    const uint32_t s = !p.paired ? r : r >= np ? 2u * (r - np) + 1u : 2u * r;
    p.usrc[k + p.before[s]] = k;
  }
  for (uint32_t s = first; s < p.n_reads; s += stride) {
    if (p.begin[s + 1] != p.begin[s]) continue;
    const uint32_t r = !p.paired ? s : (s & 1u) * np + (s >> 1);
    p.usrc[p.begin[s] + p.before[s]] = p.n_base + r;
  }
}

// ---------------------------------------------------------------------------------------------------------
// Pair mode: the records of read i (mate 1, list A) and of read n_pairs + i (mate 2, list B) of a batch of 2 n_pairs reads.
// A combination (a, b) is concordant when neither carries 0x8000, both lie on one sequence on opposite strands, the forward one
// f starts at or before the reverse one r, and I <= end0(r) - pos0(f) <= X (end0 = pos0 + the M and D lengths of the CIGAR).
// The chosen one has the least nm(a) + nm(b), ties to the smaller a, then the smaller b.  Output lines: mate 1's, then
// mate 2's, the chosen record first in each, the others in their order.
// One lane per pair; a pair with more than kPairAlone combinations is taken by its whole wave after the lanes' own pairs.
// ---------------------------------------------------------------------------------------------------------
constexpr uint64_t kPairAlone = 32;
constexpr uint64_t kNoKey = ~0ull;

struct PairParams {
  uint32_t n_pairs;
  int64_t min_insert, max_insert;
  const uint32_t *rec_begin;  // 2 n_pairs + 1
  const uint16_t *flag;
  const uint32_t *tid, *pos0;
  const uint8_t *nm;
  const uint32_t *cigar_off, *cigar;
  uint32_t *perm;             // per line
  uint16_t *pflag;
  uint32_t *mtid, *mpos0;
  int32_t *tlen;
  uint32_t *pair_begin;       // 2 n_pairs + 1
  uint32_t *n_proper;
  // mate rescue (nullptr: off): exclusive scan of the kept rescued records over the pairs (n_pairs + 1); pair i's one, if it
  // has one, is record resc_first + resc_before[i]; it belongs to the mate its s_read names and stands in front of that mate's
  // own records (none where the mate had no record; with fem_dev_set_rescue_discordant it can have some, which pair with nothing)
  const uint32_t *resc_before;
  uint32_t resc_first;
  const uint32_t *s_read;
  // MAPQ (pair_kernel<true>): per line, 0 on every line but a mate's primary one, which gets kPairProper | qp for a proper pair
  // (| kPairOwn when the chosen record may keep its single-end MAPQ: not rescued, NM = d1 of its mate); mapq_kernel finishes it
  uint8_t *lmq;
  // the library's orientation (fem_dev_set_orientation): 16 where the mate's strand is flipped, else 0; a
  // record's virtual strand is its FLAG's 16 ^ its mate's flip, and the pairing rule reads that one
  uint32_t flip1, flip2;
};
constexpr uint32_t kPairOwn = 0x80u, kPairProper = 0x40u;

// Q(g, c) = min(60, max(0, 20 g - 3 floor(log2 c))) (include/fem_hip.h, fem_dev_set_mapq), c >= 1
__device__ __forceinline__ uint32_t mapq_q(int32_t gap, uint64_t c) {
  const int32_t q = 20 * gap - 3 * (63 - __builtin_clzll(c));
  return q < 0 ? 0u : q > 60 ? 60u : (uint32_t)q;
}

// The two least distinct values seen and how often each was (the hit strata of a read or of a pair's concordant sums)
constexpr uint32_t kNoStratum = 0xFFFFFFFFu;
struct Strata {
  uint32_t s1 = kNoStratum, s2 = kNoStratum;
  uint64_t c1 = 0, c2 = 0;
  __device__ __forceinline__ void add(uint32_t s) {
    if (s < s1) s2 = s1, c2 = c1, s1 = s, c1 = 1;
    else if (s == s1) ++c1;
    else if (s < s2) s2 = s, c2 = 1;
    else if (s == s2) ++c2;
  }
};

__device__ __forceinline__ uint64_t wave_sum64(uint64_t v) {
  for (int d = 32; d > 0; d >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, d);
  return v;
}
__device__ __forceinline__ uint32_t wave_min32(uint32_t v) {
  for (int d = 32; d > 0; d >>= 1) {
    const uint32_t o = (uint32_t)__shfl_xor(v, d);
    v = o < v ? o : v;
  }
  return v;
}

// The wave's strata from each lane's (lanes whose least value is above the wave's least hold their own least as the second)
__device__ __forceinline__ Strata wave_strata(const Strata &x) {
  Strata w;
  w.s1 = wave_min32(x.s1);
  w.c1 = wave_sum64(x.s1 == w.s1 ? x.c1 : 0u);
  w.s2 = wave_min32(x.s1 == w.s1 ? x.s2 : x.s1);
  w.c2 = wave_sum64(w.s2 == kNoStratum ? 0u : x.s1 == w.s2 ? x.c1 : x.s2 == w.s2 ? x.c2 : 0u);
  return w;
}

// qp of a proper pair from the strata of its concordant sums
__device__ __forceinline__ uint32_t pair_qp(const Strata &w) {
  return w.c1 >= 2u ? 0u : w.s2 == kNoStratum ? 60u : mapq_q((int32_t)(w.s2 - w.s1), w.c2);
}

// The byte pair_kernel<true> leaves on a mate's primary line: chosen record x of a list that starts at x0 (rescued: from a window)
__device__ __forceinline__ uint32_t pair_mq_byte(const PairParams &p, bool proper, uint32_t qp, uint32_t x0, uint32_t x, bool rescued) {
  if (!proper) return 0u;
  return kPairProper | qp | (!rescued && p.nm[x0 + x] == p.nm[x0] ? kPairOwn : 0u);
}

struct MateRec {
  uint32_t tid, pos0, flag, nm;
  uint32_t v;  // the virtual strand: 16 = reverse
  uint64_t end0;
};

// record r of a mate whose flip is `flip` (PairParams::flip1 or flip2)
__device__ __forceinline__ MateRec mate_rec(const PairParams &p, uint32_t r, uint32_t flip) {
  MateRec m;
  m.tid = p.tid[r], m.pos0 = p.pos0[r], m.flag = p.flag[r], m.nm = p.nm[r];
  m.v = (m.flag & 16u) ^ flip;
  uint64_t span = 0;
  for (uint32_t c = p.cigar_off[r], c1 = p.cigar_off[r + 1]; c < c1; ++c) {
    const uint32_t op = p.cigar[c];
    if ((op & 0xFu) == kOpM || (op & 0xFu) == kOpD) span += op >> 4;
  }
  m.end0 = (uint64_t)m.pos0 + span;
  return m;
}

// the insert of a concordant combination, -1 otherwise (an insert is never negative: pos0(f) <= pos0(r) <= end0(r)); forward
// and reverse are the virtual strands
__device__ __forceinline__ int64_t concordant(const PairParams &p, const MateRec &a, const MateRec &b) {
  if (((a.flag | b.flag) & 0x8000u) || a.tid != b.tid || a.v == b.v) return -1;
  const MateRec &f = a.v ? b : a, &r = a.v ? a : b;
  if (f.pos0 > r.pos0) return -1;
  const int64_t ins = (int64_t)(r.end0 - f.pos0);
  return ins >= p.min_insert && ins <= p.max_insert ? ins : -1;
}

// lines [first, na + nb) of a pair, every step-th one (kMapq: mq_a, mq_b the bytes of the mates' primary lines).  na, nb: the
// mates' lines, their records from a0, b0 on.  resc (1 = mate 1, 2 = mate 2): that mate's list is its rescued record alone
// (at a0 or b0, the chosen one), which is its first line; its own records, from own0 on, are its other lines.
template <bool kMapq>
__device__ void write_pair(const PairParams &p, uint32_t a0, uint32_t na, uint32_t b0, uint32_t nb, uint32_t ob, bool proper, uint32_t ca,
                           uint32_t cb, int64_t insert, uint32_t first, uint32_t step, uint32_t resc, uint32_t own0, uint32_t mq_a = 0,
                           uint32_t mq_b = 0) {
  for (uint32_t u = first; u < na + nb; u += step) {
    const bool m2 = u >= na;
    const uint32_t t = m2 ? u - na : u, c = m2 ? cb : ca;
    const uint32_t idx = proper ? (t == 0 ? c : t - 1u + (t - 1u >= c ? 1u : 0u)) : t;
    const uint32_t rec = resc == (m2 ? 2u : 1u) && t ? own0 + t - 1u : (m2 ? b0 : a0) + idx;
    const bool has_other = m2 ? na > 0 : nb > 0;
    const uint32_t other = m2 ? a0 + (proper ? ca : 0u) : b0 + (proper ? cb : 0u);
    const uint32_t fl = p.flag[rec];
    uint32_t nf = (fl & 0x8010u) | 1u | (m2 ? 0x80u : 0x40u) | (t ? 256u : 0u) | (proper && t == 0 ? 2u : 0u);
    uint32_t mt = 0xFFFFFFFFu, mp = 0xFFFFFFFFu;
    if (!has_other) {
      nf |= 8u;
    } else {
      if (p.flag[other] & 16u) nf |= 0x20u;
      mt = p.tid[other], mp = p.pos0[other];
    }
    const uint32_t k = ob + u;
    p.perm[k] = rec, p.pflag[k] = (uint16_t)nf, p.mtid[k] = mt, p.mpos0[k] = mp;
    p.tlen[k] = proper && t == 0 ? (int32_t)(((fl & 16u) ^ (m2 ? p.flip2 : p.flip1)) ? -insert : insert) : 0;
    if (kMapq) p.lmq[k] = (uint8_t)(t ? 0u : m2 ? mq_b : mq_a);
  }
}

__device__ __forceinline__ uint32_t wave_bcast(uint32_t v, uint32_t lane) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)lane);
}

// kMapq: also the strata of the concordant sums (cp1 at s1, the least sum s2 above it and cp2 at s2) and each line's MAPQ byte.
template <bool kMapq>
__global__ void __launch_bounds__(256) pair_kernel(PairParams p) {
  const uint32_t ln = threadIdx.x & 63u;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = i < p.n_pairs;
  uint32_t a0 = 0, na = 0, b0 = 0, nb = 0, ob = 0;
  uint32_t resc = 0, own0 = 0, own_n = 0;  // 1 = list A is a rescued record, 2 = list B; that mate's own records (its lines behind it)
  if (live) {
    const uint32_t mid = p.rec_begin[p.n_pairs];
    a0 = p.rec_begin[i], na = p.rec_begin[i + 1] - a0;
    b0 = p.rec_begin[p.n_pairs + i], nb = p.rec_begin[p.n_pairs + i + 1] - b0;
    ob = a0 + b0 - mid;  // the lines of the pairs in front: their mate 1 records and their mate 2 records
    if (p.resc_before) {  // ... and their rescued mates
      const uint32_t before = p.resc_before[i], kept = p.resc_before[i + 1] - before;
      ob += before;
      if (kept) {  // the rescued record alone is its mate's list: the mate's own records, if it has any, pair with nothing
        const uint32_t rrec = p.resc_first + before;
        if (p.s_read[rrec] < p.n_pairs) own0 = a0, own_n = na, a0 = rrec, na = 1, resc = 1;
        else own0 = b0, own_n = nb, b0 = rrec, nb = 1, resc = 2;
      }
    }
    const uint32_t la = na + (resc == 1u ? own_n : 0u), lb = nb + (resc == 2u ? own_n : 0u);
    p.pair_begin[2u * i] = ob, p.pair_begin[2u * i + 1u] = ob + la;
    if (i + 1u == p.n_pairs) p.pair_begin[2u * i + 2u] = ob + la + lb;
  }
  const bool big = live && (uint64_t)na * nb > kPairAlone;
  bool proper_here = false;
  if (live && !big) {  // the lane alone: a ascending, b ascending, only a smaller sum replaces (the tie rule)
    const uint32_t la = na + (resc == 1u ? own_n : 0u), lb = nb + (resc == 2u ? own_n : 0u);
    uint32_t best = 0xFFFFFFFFu, ca = 0, cb = 0;
    int64_t ins = -1;
    Strata st;
    for (uint32_t a = 0; a < na; ++a) {
      const MateRec ra = mate_rec(p, a0 + a, p.flip1);
      if (ra.flag & 0x8000u) continue;
      for (uint32_t b = 0; b < nb; ++b) {
        const MateRec rb = mate_rec(p, b0 + b, p.flip2);
        const int64_t x = concordant(p, ra, rb);
        if (x >= 0 && ra.nm + rb.nm < best) best = ra.nm + rb.nm, ca = a, cb = b, ins = x;
        if (kMapq && x >= 0) st.add(ra.nm + rb.nm);
      }
    }
    proper_here = best != 0xFFFFFFFFu;
    if (kMapq) {
      const uint32_t qp = pair_qp(st);
      write_pair<true>(p, a0, la, b0, lb, ob, proper_here, ca, cb, ins, 0u, 1u, resc, own0, pair_mq_byte(p, proper_here, qp, a0, ca, resc == 1),
                       pair_mq_byte(p, proper_here, qp, b0, cb, resc == 2));
    } else {
      write_pair<false>(p, a0, la, b0, lb, ob, proper_here, ca, cb, ins, 0u, 1u, resc, own0);
    }
  }
  // pairs with many combinations (repeats): the wave, one pair after the other; the lanes stride over the longer list, each
  // walks the shorter one; the least (nm sum, a, b) in two steps: (nm sum << 32 | a), then b among the lanes that hold it;
  // kMapq: each lane's strata, then the wave's (wave_strata: a sum for cp1, a minimum for s2, a sum for cp2)
  uint64_t todo = __ballot(big);
  while (todo) {
    const uint32_t src = (uint32_t)__builtin_ctzll(todo);
    todo &= todo - 1u;
    const uint32_t A0 = wave_bcast(a0, src), NA = wave_bcast(na, src), B0 = wave_bcast(b0, src), NB = wave_bcast(nb, src);
    const uint32_t OB = wave_bcast(ob, src), RESC = wave_bcast(resc, src), OWN0 = wave_bcast(own0, src), OWN_N = wave_bcast(own_n, src);
    const uint32_t LA = NA + (RESC == 1u ? OWN_N : 0u), LB = NB + (RESC == 2u ? OWN_N : 0u);
    const bool lanes_on_a = NA >= NB;
    const uint32_t n_long = lanes_on_a ? NA : NB, n_short = lanes_on_a ? NB : NA;
    const uint32_t flip_long = lanes_on_a ? p.flip1 : p.flip2, flip_short = lanes_on_a ? p.flip2 : p.flip1;
    uint64_t key = kNoKey;
    uint32_t key_b = 0xFFFFFFFFu;
    Strata st;
    for (uint32_t u = ln; u < n_long; u += 64u) {
      const MateRec ru = mate_rec(p, (lanes_on_a ? A0 : B0) + u, flip_long);
      if (ru.flag & 0x8000u) continue;
      for (uint32_t v = 0; v < n_short; ++v) {
        const MateRec rv = mate_rec(p, (lanes_on_a ? B0 : A0) + v, flip_short);
        if (concordant(p, ru, rv) < 0) continue;
        const uint32_t a = lanes_on_a ? u : v, b = lanes_on_a ? v : u;
        const uint64_t k = (uint64_t)(ru.nm + rv.nm) << 32 | a;
        if (k < key || (k == key && b < key_b)) key = k, key_b = b;
        if (kMapq) st.add(ru.nm + rv.nm);
      }
    }
    uint64_t kmin = key;
    for (int d = 32; d > 0; d >>= 1) {
      const uint64_t o = (uint64_t)__shfl_xor((unsigned long long)kmin, d);
      kmin = o < kmin ? o : kmin;
    }
    uint32_t bmin = key == kmin ? key_b : 0xFFFFFFFFu;
    for (int d = 32; d > 0; d >>= 1) {
      const uint32_t o = (uint32_t)__shfl_xor(bmin, d);
      bmin = o < bmin ? o : bmin;
    }
    const bool proper = kmin != kNoKey;
    const uint32_t ca = proper ? (uint32_t)kmin : 0u, cb = proper ? bmin : 0u;
    const int64_t ins = proper ? concordant(p, mate_rec(p, A0 + ca, p.flip1), mate_rec(p, B0 + cb, p.flip2)) : -1;
    if (kMapq) {
      const uint32_t qp = pair_qp(wave_strata(st));
      write_pair<true>(p, A0, LA, B0, LB, OB, proper, ca, cb, ins, ln, 64u, RESC, OWN0, pair_mq_byte(p, proper, qp, A0, ca, RESC == 1),
                       pair_mq_byte(p, proper, qp, B0, cb, RESC == 2));
    } else {
      write_pair<false>(p, A0, LA, B0, LB, OB, proper, ca, cb, ins, ln, 64u, RESC, OWN0);
    }
    if (ln == src) proper_here = proper;
  }
  const uint64_t proper_lanes = __ballot(proper_here);
  if (ln == 0 && proper_lanes) atomicAdd(p.n_proper, (uint32_t)__builtin_popcountll(proper_lanes));
}

// The probe of fem_dev_set_rescue_discordant: disc[i] = 1 for a pair with records on both sides of which no
// combination is concordant, mate rescue's second kind of candidate, else 0.  The work is divided as pair_kernel's: a pair of
// up to kPairAlone combinations is its lane's, a larger one its wave's, the lanes striding over the longer list; the walk
// ends at the first concordant combination (the wave's: a ballot after every step of the stride).
__global__ void __launch_bounds__(256) pair_probe_kernel(PairParams p, uint8_t *disc) {
  const uint32_t ln = threadIdx.x & 63u;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = i < p.n_pairs;
  uint32_t a0 = 0, na = 0, b0 = 0, nb = 0;
  if (live) {
    a0 = p.rec_begin[i], na = p.rec_begin[i + 1] - a0;
    b0 = p.rec_begin[p.n_pairs + i], nb = p.rec_begin[p.n_pairs + i + 1] - b0;
  }
  const bool both = na && nb, big = both && (uint64_t)na * nb > kPairAlone;
  bool found = false;
  if (both && !big) {
    for (uint32_t a = 0; a < na && !found; ++a) {
      const MateRec ra = mate_rec(p, a0 + a, p.flip1);
      if (ra.flag & 0x8000u) continue;
      for (uint32_t b = 0; b < nb && !found; ++b) found = concordant(p, ra, mate_rec(p, b0 + b, p.flip2)) >= 0;
    }
  }
  uint64_t todo = __ballot(big);
  while (todo) {
    const uint32_t src = (uint32_t)__builtin_ctzll(todo);
    todo &= todo - 1u;
    const uint32_t A0 = wave_bcast(a0, src), NA = wave_bcast(na, src), B0 = wave_bcast(b0, src), NB = wave_bcast(nb, src);
    const bool lanes_on_a = NA >= NB;
    const uint32_t long0 = lanes_on_a ? A0 : B0, n_long = lanes_on_a ? NA : NB, short0 = lanes_on_a ? B0 : A0, n_short = lanes_on_a ? NB : NA;
    const uint32_t flip_long = lanes_on_a ? p.flip1 : p.flip2, flip_short = lanes_on_a ? p.flip2 : p.flip1;
    bool any = false;
    for (uint32_t u0 = 0; u0 < n_long && !any; u0 += 64u) {
      const uint32_t u = u0 + ln;
      bool hit = false;
      if (u < n_long) {
        const MateRec ru = mate_rec(p, long0 + u, flip_long);
        if (!(ru.flag & 0x8000u))
          for (uint32_t v = 0; v < n_short && !hit; ++v) hit = concordant(p, ru, mate_rec(p, short0 + v, flip_short)) >= 0;
      }
      any = __ballot(hit) != 0;
    }
    if (ln == src) found = any;
  }
  if (live) disc[i] = both && !found ? 1u : 0u;
}

// ---------------------------------------------------------------------------------------------------------
// The insert size range the batch's own pairs suggest (fem_dev_estimate_insert).  A pair is unique when each
// mate has exactly one record and neither carries 0x8000; a unique pair is informative when its two records are concordant
// within 0 .. FEM_INSERT_MAX (the pairing rule's own statement: p.min_insert, p.max_insert are set to that, whatever the slot's
// range is).  insert_sample_kernel: one lane per pair, one add into the histogram's bin of the insert; ctl[0] unique pairs,
// ctl[1] informative ones.  insert_bounds_kernel (one block): the inserts in ascending order are v[0 .. n); q25 q50 q75 =
// v[k (n - 1) / 4] to ctl[2 .. 4]; with n >= FEM_INSERT_MIN_PAIRS, ctl[7] = 1 and ctl[5], ctl[6] = max(0, q25 - 3 iqr),
// q75 + 3 iqr (iqr = q75 - q25); else the three are 0.  n = 0: the quartiles are -1.
// ---------------------------------------------------------------------------------------------------------
constexpr uint32_t kInsertBins = FEM_INSERT_MAX + 1u;
constexpr uint32_t kInsertCtl = 8;  // words behind the histogram

__global__ void __launch_bounds__(256) insert_sample_kernel(PairParams p, uint32_t *hist, uint32_t *ctl) {
  const uint32_t ln = threadIdx.x & 63u;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  bool unique = false, informative = false;
  if (i < p.n_pairs) {
    const uint32_t a0 = p.rec_begin[i], na = p.rec_begin[i + 1] - a0;
    const uint32_t b0 = p.rec_begin[p.n_pairs + i], nb = p.rec_begin[p.n_pairs + i + 1] - b0;
    if (na == 1u && nb == 1u) {
      const MateRec ra = mate_rec(p, a0, p.flip1), rb = mate_rec(p, b0, p.flip2);
      unique = !((ra.flag | rb.flag) & 0x8000u);
      const int64_t ins = concordant(p, ra, rb);  // (-1 with 0x8000 on either)
      informative = ins >= 0;
      if (informative) atomicAdd(hist + (uint32_t)ins, 1u);  // (ins <= p.max_insert = FEM_INSERT_MAX)
    }
  }
  const uint64_t unique_lanes = __ballot(unique), informative_lanes = __ballot(informative);
  if (ln == 0 && unique_lanes) atomicAdd(ctl, (uint32_t)__builtin_popcountll(unique_lanes));
  if (ln == 0 && informative_lanes) atomicAdd(ctl + 1, (uint32_t)__builtin_popcountll(informative_lanes));
}

// The library estimate (fem_dev_estimate_library): the same sample under the three orientations in one pass.
// hist: three histograms, FR RF FF, then their three control blocks.  One lane per pair reads its two records once and asks
// the pairing rule under each orientation's flips: a unique pair on opposite strands can be informative under FR and under RF
// (under both at equal pos0), one on the same strand under FF alone, so it adds to at most two histograms.  The unique pairs
// are counted into all three blocks.
constexpr uint32_t kOrientations = 3;
__device__ __forceinline__ uint32_t orient_flip1(uint32_t o) { return o == FEM_ORIENT_RF ? 16u : 0u; }
__device__ __forceinline__ uint32_t orient_flip2(uint32_t o) { return o == FEM_ORIENT_FR ? 0u : 16u; }

__global__ void __launch_bounds__(256) library_sample_kernel(PairParams p, uint32_t *hist, uint32_t *ctl) {
  const uint32_t ln = threadIdx.x & 63u;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  bool unique = false;
  int64_t ins[kOrientations] = {-1, -1, -1};
  if (i < p.n_pairs) {
    const uint32_t a0 = p.rec_begin[i], na = p.rec_begin[i + 1] - a0;
    const uint32_t b0 = p.rec_begin[p.n_pairs + i], nb = p.rec_begin[p.n_pairs + i + 1] - b0;
    if (na == 1u && nb == 1u) {
      MateRec ra = mate_rec(p, a0, 0u), rb = mate_rec(p, b0, 0u);
      unique = !((ra.flag | rb.flag) & 0x8000u);
#pragma unroll
      for (uint32_t o = 0; o < kOrientations; ++o) {
        ra.v = (ra.flag & 16u) ^ orient_flip1(o), rb.v = (rb.flag & 16u) ^ orient_flip2(o);
        ins[o] = concordant(p, ra, rb);
        if (ins[o] >= 0) atomicAdd(hist + o * kInsertBins + (uint32_t)ins[o], 1u);  // (ins <= p.max_insert = FEM_INSERT_MAX)
      }
    }
  }
  const uint64_t unique_lanes = __ballot(unique);
#pragma unroll
  for (uint32_t o = 0; o < kOrientations; ++o) {
    const uint64_t informative_lanes = __ballot(ins[o] >= 0);
    if (ln == 0 && unique_lanes) atomicAdd(ctl + o * kInsertCtl, (uint32_t)__builtin_popcountll(unique_lanes));
    if (ln == 0 && informative_lanes) atomicAdd(ctl + o * kInsertCtl + 1, (uint32_t)__builtin_popcountll(informative_lanes));
  }
}

// One block per histogram (fem_dev_estimate_insert: one; fem_dev_estimate_library: three, their control blocks behind them all)
__global__ void __launch_bounds__(256) insert_bounds_kernel(const uint32_t *hist, uint32_t *ctl) {
  hist += blockIdx.x * kInsertBins, ctl += blockIdx.x * kInsertCtl;
  constexpr uint32_t kPerLane = kInsertBins / 256u;
  static_assert(kPerLane * 256u == kInsertBins, "every lane sums as many bins");
  __shared__ uint32_t incl[256];  // inclusive scan of the lanes' sums
  __shared__ int32_t q[3];
  const uint32_t t = threadIdx.x, first = t * kPerLane;
  uint32_t mine = 0;
  for (uint32_t b = 0; b < kPerLane; ++b) mine += hist[first + b];
  incl[t] = mine;
  __syncthreads();
  for (uint32_t d = 1; d < 256u; d <<= 1) {
    const uint32_t below = t >= d ? incl[t - d] : 0u;
    __syncthreads();
    incl[t] += below;
    __syncthreads();
  }
  const uint32_t n = incl[255], before = incl[t] - mine;
  if (t < 3u) q[t] = -1;
  __syncthreads();
  if (n && mine) {
    for (uint32_t k = 1; k <= 3u; ++k) {
      const uint32_t rank = (uint32_t)((uint64_t)k * (n - 1u) / 4u);  // v[rank]
      if (rank < before || rank >= before + mine) continue;
      uint32_t seen = before, b = 0;
      while (seen + hist[first + b] <= rank) seen += hist[first + b], ++b;  // (ends inside the stretch: rank < before + mine)
      q[k - 1u] = (int32_t)(first + b);
    }
  }
  __syncthreads();
  if (t == 0) {
    const int32_t q25 = q[0], q75 = q[2], iqr = q75 - q25;
    const bool estimated = n >= (uint32_t)FEM_INSERT_MIN_PAIRS;
    const int32_t lo = q25 - 3 * iqr;
    ctl[2] = (uint32_t)q[0], ctl[3] = (uint32_t)q[1], ctl[4] = (uint32_t)q75;
    ctl[5] = estimated ? (uint32_t)(lo < 0 ? 0 : lo) : 0u;
    ctl[6] = estimated ? (uint32_t)(q75 + 3 * iqr) : 0u;
    ctl[7] = estimated ? 1u : 0u;
  }
}

// ---------------------------------------------------------------------------------------------------------
// MAPQ (fem_dev_set_mapq).  One lane per read: q_se from its records' NM (d1 the first record's, c1 records
// at d1; d2 the least NM above d1 and c2 records at it, or e + 1 and 1 where there is none): 0 when c1 >= 2, else
// Q(d2 - d1, c2).  A read with more than kMapqAlone records is taken by its whole wave after the lanes' own reads (repeats:
// thousands of records).  Single-end: q_se per read, which the text kernels print on the read's primary line.  Pair mode: the
// byte pair_kernel<true> left on each mate's primary line becomes its MAPQ: q_se without a proper pair, else
// max(q_x, min(qp, q_x + 40)) with q_x = q_se where the chosen record keeps it (kPairOwn), else 0.
// ---------------------------------------------------------------------------------------------------------
constexpr uint32_t kMapqAlone = 32;

struct MapqParams {
  uint32_t n_reads;
  int32_t e;
  const uint32_t *rec_begin;   // n_reads + 1 (run()'s records)
  const uint8_t *nm;
  uint8_t *q_read;             // single-end: per read
  const uint32_t *pair_begin;  // pair mode (else nullptr): n_reads + 1; mate m of pair i has lines [pair_begin[2i+m], pair_begin[2i+m+1])
  uint8_t *lmq;                // pair mode: pair_kernel<true>'s bytes, per line
};

__device__ __forceinline__ uint32_t single_q(uint64_t c1, uint32_t d1, uint32_t d2, uint64_t c2, int32_t e) {
  if (c1 >= 2u) return 0u;
  if (d2 == kNoStratum) d2 = (uint32_t)e + 1u, c2 = 1u;
  return mapq_q((int32_t)d2 - (int32_t)d1, c2);
}

__global__ void __launch_bounds__(256) mapq_kernel(MapqParams p) {
  const uint32_t ln = threadIdx.x & 63u;
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = r < p.n_reads;
  uint32_t r0 = 0, nr = 0;
  if (live) r0 = p.rec_begin[r], nr = p.rec_begin[r + 1] - r0;
  const bool big = nr > kMapqAlone;
  uint32_t q = 0;  // (a read without records: no line; in pair mode a rescued mate, whose q_x is 0)
  if (live && !big && nr) {
    const uint32_t d1 = p.nm[r0];
    uint32_t c1 = 0, d2 = kNoStratum, c2 = 0;
    for (uint32_t k = r0; k < r0 + nr; ++k) {
      const uint32_t v = p.nm[k];
      if (v == d1) ++c1;
      else if (v > d1 && v < d2) d2 = v, c2 = 1;
      else if (v > d1 && v == d2) ++c2;
    }
    q = single_q(c1, d1, d2, c2, p.e);
  }
  uint64_t todo = __ballot(big);
  while (todo) {
    const uint32_t src = (uint32_t)__builtin_ctzll(todo);
    todo &= todo - 1u;
    const uint32_t R0 = wave_bcast(r0, src), NR = wave_bcast(nr, src), d1 = p.nm[R0];
    uint32_t c1 = 0, d2 = kNoStratum, c2 = 0;
    for (uint32_t k = ln; k < NR; k += 64u) {
      const uint32_t v = p.nm[R0 + k];
      if (v == d1) ++c1;
      else if (v > d1 && v < d2) d2 = v, c2 = 1;
      else if (v > d1 && v == d2) ++c2;
    }
    const uint64_t C1 = wave_sum64(c1);
    const uint32_t D2 = wave_min32(d2);
    const uint64_t C2 = wave_sum64(d2 == D2 && D2 != kNoStratum ? c2 : 0u);
    if (ln == src) q = single_q(C1, d1, D2, C2, p.e);
  }
  if (!live) return;
  if (!p.pair_begin) {
    p.q_read[r] = (uint8_t)q;
    return;
  }
  const uint32_t np = p.n_reads / 2u, m = r >= np ? 1u : 0u, i = r - m * np;
  const uint32_t k0 = p.pair_begin[2u * i + m], k1 = p.pair_begin[2u * i + m + 1u];
  if (k1 == k0) return;
  const uint32_t b = p.lmq[k0];
  uint32_t out = q;
  if (b & kPairProper) {
    const uint32_t qx = (b & kPairOwn) ? q : 0u, qp = b & 0x3Fu;
    out = qp < qx + 40u ? qp : qx + 40u;
    out = out > qx ? out : qx;
  }
  p.lmq[k0] = (uint8_t)out;
}

// ---------------------------------------------------------------------------------------------------------
// The line filter (fem_dev_set_report).  A slot (read s single-end, mate m of pair i = slot 2i + m) has the
// lines [begin[s], begin[s + 1]) of the records or of pair_kernel's lines; d = the least NM over them (0x8000 records count).
// Line 0 of the slot stays; line t >= 1 stays iff nm <= d + S (S on) and fewer than N of the slot's lines stay in front of it
// (N on).  The lines that pass the stratum test are taken in order until N are there, so a line's rank among the passing ones
// is its place in the slot's output and the slot keeps min(passing, N) lines.
// report_kernel<false>: cnt[s] = the lines slot s keeps, 1 for a slot without lines when unmapped reads have lines; an
// exclusive scan of cnt (rocPRIM, n_reads + 1 counts); report_kernel<true>: the same walk again, usrc[before[s] + rank] =
// the line, or n_base + the slot's read for an unmapped one.  A slot of up to kReportAlone lines is its lane's; a larger one is
// taken by the whole wave after the lanes' own slots: a wave minimum for d, then 64 lines per step, a ballot of the passing
// ones and the popcount below the lane for the rank, the passing lines so far carried from step to step.
// ---------------------------------------------------------------------------------------------------------
constexpr uint32_t kReportAlone = 32;
constexpr uint32_t kReportOff = 0xFFFFFFFFu;

struct ReportParams {
  uint32_t n_reads, n_base;  // n_base: records (pair mode: pair_kernel's lines)
  const uint32_t *begin;     // n_reads + 1, by slot
  const uint8_t *nm;         // per record
  const uint32_t *perm;      // pair mode (else nullptr): per line of pair_kernel's, its record
  uint32_t strata, max_hits; // kReportOff: off
  uint32_t unmapped;         // a slot without lines has one (fem_dev_set_unmapped)
  uint32_t *cnt;             // n_reads + 1 (the last one zero)
  const uint32_t *before;    // n_reads + 1: the exclusive scan of cnt
  uint32_t *usrc;            // before[n_reads]
  uint32_t *n_lines;         // [0] that number, [1] the unmapped slots among them (zeroed before report_kernel<false>)
};

__device__ __forceinline__ uint32_t report_nm(const ReportParams &p, uint32_t k) { return p.nm[p.perm ? p.perm[k] : k]; }

template <bool kWrite>
__global__ void __launch_bounds__(256) report_kernel(ReportParams p) {
  const uint32_t ln = threadIdx.x & 63u;
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = s < p.n_reads;
  uint32_t b0 = 0, c = 0, at = 0;
  if (live) b0 = p.begin[s], c = p.begin[s + 1] - b0;
  if (kWrite && live) at = p.before[s];
  if (kWrite && s == 0) p.n_lines[0] = p.before[p.n_reads];
  const bool big = c > kReportAlone;
  uint32_t kept = 0;
  if (live && !big && c) {
    uint32_t lim = kReportOff;
    if (p.strata != kReportOff) {
      uint32_t d = 255u;
      for (uint32_t t = 0; t < c; ++t) {
        const uint32_t v = report_nm(p, b0 + t);
        d = v < d ? v : d;
      }
      lim = d + p.strata;
    }
    for (uint32_t t = 0; t < c && kept < p.max_hits; ++t) {
      if (t && lim != kReportOff && report_nm(p, b0 + t) > lim) continue;
      if (kWrite) p.usrc[at + kept] = b0 + t;
      ++kept;
    }
  }
  uint64_t todo = __ballot(big);
  while (todo) {
    const uint32_t src = (uint32_t)__builtin_ctzll(todo);
    todo &= todo - 1u;
    const uint32_t B0 = wave_bcast(b0, src), C = wave_bcast(c, src), AT = kWrite ? wave_bcast(at, src) : 0u;
    uint32_t lim = kReportOff;
    if (p.strata != kReportOff) {
      uint32_t d = 255u;
      for (uint32_t t = ln; t < C; t += 64u) {
        const uint32_t v = report_nm(p, B0 + t);
        d = v < d ? v : d;
      }
      lim = wave_min32(d) + p.strata;
    }
    uint32_t passed = 0;  // (the same in every lane)
    for (uint32_t t0 = 0; t0 < C && passed < p.max_hits; t0 += 64u) {
      const uint32_t t = t0 + ln;
      const bool ok = t < C && (t == 0 || lim == kReportOff || report_nm(p, B0 + t) <= lim);
      const uint64_t oks = __ballot(ok);
      const uint32_t rank = passed + (uint32_t)__builtin_popcountll(oks & ((1ull << ln) - 1ull));
      if (kWrite && ok && rank < p.max_hits) p.usrc[AT + rank] = B0 + t;
      passed += (uint32_t)__builtin_popcountll(oks);
    }
    if (ln == src) kept = passed < p.max_hits ? passed : p.max_hits;
  }
  const bool unm = live && !c && p.unmapped;
  if (kWrite) {
    if (unm) p.usrc[at] = p.n_base + (p.perm ? (s & 1u) * (p.n_reads / 2u) + (s >> 1) : s);
    return;
  }
  if (s <= p.n_reads) p.cnt[s] = unm ? 1u : kept;
  const uint64_t unms = __ballot(unm);
  if (ln == 0 && unms) atomicAdd(p.n_lines + 1, (uint32_t)__builtin_popcountll(unms));
}

// ---------------------------------------------------------------------------------------------------------
// Secondary lines folded into XA:Z (fem_dev_set_xa).  Behind report_kernel's index (which runs with both of its
// tests off where the line filter is off): slot s has the lines usrc[begin[s] .. begin[s + 1]), the first one its primary line or
// an unmapped read's.  The entry of line t >= 1 is <RNAME>,<+-><POS>,<CIGAR>,<NM>; with the bytes its line prints; f = the
// largest f <= min(c - 1, N) whose entries 1 .. f have at most FEM_XA_MAX_BYTES bytes together.  The lengths' running sum grows
// with t, so f is the number of lines t <= N whose sum fits, with no sequential stop.
// xa_index_kernel<false>: per slot the lines that stay (c - f), f, whether it folds, and the entries' bytes; an exclusive scan of
// the three counts (rocPRIM, one pass); xa_index_kernel<true>: the lines that stay into the new index, the folded ones in slot
// order into xsrc, the folding slots into a list, 0x8000 among the folded records into the text's count of them.
// A slot of up to kReportAlone lines is its lane's; a larger one is taken by the whole wave after the lanes' own, 64 lines per
// step: a scan of the lengths by shuffles, the sum so far carried from step to step (the same in every lane).
// xa_write_kernel: a wave per folding slot (from the list), lane i entry i of 64 per step at the sum of the lengths in front of it.
// ---------------------------------------------------------------------------------------------------------
struct XaParams {
  uint32_t n_reads;
  uint32_t max_entries;      // N
  const uint32_t *begin;     // n_reads + 1, by slot: report_kernel's scan
  const uint32_t *usrc;      // report_kernel's index
  uint32_t *cnt;             // 3 (n_reads + 1): the lines that stay, the entries, 1 for a folding slot (the last of each zero)
  uint32_t *bytes;           // n_reads + 1: the entries' bytes
  const uint32_t *scan;      // 3 (n_reads + 1): the exclusive scans of cnt's parts
  uint32_t *usrc_out;        // the index after folding
  uint32_t *xsrc;            // the folded lines' sources, slot s's from scan[n1 + s] on
  uint32_t *xlist;           // the folding slots
  uint32_t *n_lines;         // [0] the lines after folding, [2] the entries, [3] the folding slots
};

// An entry's source as the line kernels resolve a line's: the record, and the FLAG as written (0x8000 kept)
struct XaSource {
  uint32_t rec, flag;
};
__device__ __forceinline__ XaSource xa_source(const SamParams &p, uint32_t src) {
  const uint32_t rec = p.perm ? p.perm[src] : src;
  return {rec, p.perm ? p.pflag[src] : p.flag[rec]};
}
__device__ __forceinline__ uint32_t xa_entry_len(const SamParams &p, uint32_t src) {
  const uint32_t rec = p.perm ? p.perm[src] : src, t = p.tid[rec];
  const uint32_t c0 = p.cigar_off[rec], n_ops = p.cigar_off[rec + 1] - c0;
  return p.ref_name_off[t + 1] - p.ref_name_off[t] + dec_digits(p.pos0[rec] + 1u) + (n_ops ? cigar_chars(p, c0, n_ops) : 1u) + dec_digits(p.nm[rec]) + 5u;
}
// The inclusive sum of v over the lanes up to this one
__device__ __forceinline__ uint32_t wave_scan32(uint32_t v, uint32_t ln) {
  for (uint32_t o = 1; o < 64u; o <<= 1) {
    const uint32_t below = __shfl_up(v, o);
    if (ln >= o) v += below;
  }
  return v;
}

template <bool kWrite>
__global__ void __launch_bounds__(256) xa_index_kernel(SamParams p, XaParams x) {
  constexpr uint32_t kOver = FEM_XA_MAX_BYTES + 1u;  // (a length or a sum above the budget counts as this: no sum leaves 32 bits)
  const uint32_t ln = threadIdx.x & 63u, n1 = x.n_reads + 1u;
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = s < x.n_reads;
  uint32_t b0 = 0, c = 0, f = 0, bytes = 0, at = 0, xat = 0;
  if (live) b0 = x.begin[s], c = x.begin[s + 1] - b0;
  if (kWrite && live) f = x.cnt[n1 + s], at = x.scan[s], xat = x.scan[n1 + s];
  if (kWrite && s == 0) x.n_lines[0] = x.scan[x.n_reads], x.n_lines[2] = x.scan[n1 + x.n_reads], x.n_lines[3] = x.scan[2u * n1 + x.n_reads];
  const bool big = c > kReportAlone;
  if (live && !big && c) {
    if (kWrite) {
      x.usrc_out[at] = x.usrc[b0];
      for (uint32_t t = 1; t < c; ++t) {
        const uint32_t src = x.usrc[b0 + t];
        if (t <= f) {
          x.xsrc[xat + t - 1u] = src;
          if (xa_source(p, src).flag & 0x8000u) atomicAdd(p.asserted, 1u);
        } else {
          x.usrc_out[at + t - f] = src;
        }
      }
    } else {
      for (uint32_t t = 1; t < c && t <= x.max_entries; ++t) {
        const uint32_t len = xa_entry_len(p, x.usrc[b0 + t]);
        if (len > FEM_XA_MAX_BYTES - bytes) break;
        bytes += len, ++f;
      }
    }
  }
  uint64_t todo = __ballot(big);
  while (todo) {
    const uint32_t from = (uint32_t)__builtin_ctzll(todo);
    todo &= todo - 1u;
    const uint32_t B0 = wave_bcast(b0, from), C = wave_bcast(c, from);
    if (kWrite) {
      const uint32_t F = wave_bcast(f, from), AT = wave_bcast(at, from), XAT = wave_bcast(xat, from);
      for (uint32_t t = ln; t < C; t += 64u) {
        const uint32_t src = x.usrc[B0 + t];
        if (t >= 1u && t <= F) {
          x.xsrc[XAT + t - 1u] = src;
          if (xa_source(p, src).flag & 0x8000u) atomicAdd(p.asserted, 1u);
        } else {
          x.usrc_out[AT + (t ? t - F : 0u)] = src;
        }
      }
    } else {
      uint32_t F = 0, sum = 0;  // (the same in every lane)
      for (uint32_t t0 = 1; t0 < C; t0 += 64u) {
        const uint32_t t = t0 + ln;
        const bool in = t < C && t <= x.max_entries;
        uint32_t len = in ? xa_entry_len(p, x.usrc[B0 + t]) : kOver;
        len = len < kOver ? len : kOver;
        const uint32_t upto = sum + wave_scan32(len, ln);  // (at most 65 kOver)
        const uint32_t n_ok = (uint32_t)__builtin_popcountll(__ballot(in && upto <= FEM_XA_MAX_BYTES));  // (the lanes 0 .. n_ok - 1: the sums grow)
        if (n_ok) sum = wave_bcast(upto, n_ok - 1u);
        F += n_ok;
        if (n_ok < 64u) break;
      }
      if (ln == from) f = F, bytes = sum;
    }
  }
  if (kWrite) {
    if (live && f) x.xlist[x.scan[2u * n1 + s]] = s;
    return;
  }
  if (s <= x.n_reads) {
    x.cnt[s] = c - f, x.cnt[n1 + s] = f, x.cnt[2u * n1 + s] = f ? 1u : 0u;
    x.bytes[s] = bytes;
  }
}

// kBam: the tag as a BAM aux field ('X' 'A' 'Z', the entries, a NUL) at the record's end; else "\tXA:Z:" and the entries in front of
// the line's newline.  line_off: the text's, from the scan of the lengths that took the tag into account (sam_xa_len, bam_xa_len).
template <bool kBam>
__global__ void __launch_bounds__(256) xa_write_kernel(SamParams p, XaParams x, uint32_t n_slots) {
  const uint32_t ln = threadIdx.x & 63u, n1 = x.n_reads + 1u;
  const uint32_t w = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (w >= n_slots) return;
  const uint32_t s = x.xlist[w], f = x.cnt[n1 + s], xat = x.scan[n1 + s], bytes = x.bytes[s];
  uint8_t *tag = p.text + p.line_off[x.scan[s] + 1u] - 1u - bytes;  // the first entry's first byte (behind it: the newline, or the NUL)
  if (kBam) {
    if (ln < 3u) tag[(int)ln - 3] = (uint8_t)"XAZ"[ln];
    if (ln == 3u) tag[bytes] = 0;
  } else {
    if (ln < 6u) tag[(int)ln - 6] = (uint8_t)"\tXA:Z:"[ln];
  }
  uint32_t done = 0;  // bytes of the entries in front of this step's (the same in every lane)
  for (uint32_t i0 = 0; i0 < f; i0 += 64u) {
    const uint32_t i = i0 + ln;
    const bool in = i < f;
    uint32_t len = 0, rec = 0, flag = 0, t = 0, c0 = 0, n_ops = 0;
    if (in) {
      const uint32_t src = x.xsrc[xat + i];
      const XaSource e = xa_source(p, src);
      rec = e.rec, flag = e.flag, t = p.tid[rec];
      c0 = p.cigar_off[rec], n_ops = p.cigar_off[rec + 1] - c0;
      len = xa_entry_len(p, src);
    }
    const uint32_t upto = wave_scan32(len, ln);
    if (in) {
      uint8_t *q = tag + done + upto - len;
      for (uint32_t k = p.ref_name_off[t]; k < p.ref_name_off[t + 1]; ++k) *q++ = p.ref_names[k];
      *q++ = ',';
      *q++ = (flag & 16u) ? '-' : '+';
      q = put_dec(q, p.pos0[rec] + 1u);
      *q++ = ',';
      if (!n_ops) *q++ = '*';
      for (uint32_t k = c0; k < c0 + n_ops; ++k) q = put_cigar_op(q, p.cigar[k]);
      *q++ = ',';
      q = put_dec(q, p.nm[rec]);
      *q = ';';
    }
    done += wave_bcast(upto, 63u);
  }
}

// ---- the coverage track (fem_dev_set_coverage): coverage_kernel ----
#include "fem_coverage.hip.h"

// ---------------------------------------------------------------------------------------------------------
// Mate rescue (include/fem_hip.h).  A pair where exactly one mate (B) has no record: its other mate's first
// kRescueAnchors records without 0x8000 are the anchors, and B's pos0 is searched in each anchor's insert window at E edits:
// tiles c = lo + j (2E + 1), each the banded Myers of fo_banded_ed32 over ref[c, c + L + 2E) (first strict minimum, the same
// 32-bit word and character codes); the least (nm(anchor) + ed, anchor, pos0) is traced (trace_record at E) and kept if it is
// concordant with its anchor.  With fem_dev_set_rescue_discordant a pair with records on both sides and no concordant
// combination (pair_probe_kernel's flag) is a candidate too, searched in both directions d (0: B is mate 2, the anchors are
// mate 1's; 1: the other way round); the least (nm(anchor) + ed, d, anchor, pos0) is traced and a kept record goes behind B's
// own.  A pair with one empty list has the one direction that its lists give.  Four kernels (five with the probe in front),
// then an exclusive scan of the kept records, then pair_kernel:
//   rescue_jobs_kernel   lane per pair: candidates and one job per (candidate, direction, anchor)
//   rescue_search_kernel wave per job, lane per tile: the mate's codes staged in LDS once per wave, a 64-bit atomicMin per job
//   rescue_trace_kernel  lane per candidate: the traceback, the concordance check
//   rescue_append_kernel lane per candidate: the kept records behind run()'s (record arrays, CIGAR / MD, s_read)
// ---------------------------------------------------------------------------------------------------------
constexpr uint32_t kRescueAnchors = 8;
constexpr uint32_t kResWaves = 4;  // waves per block of the search kernel
constexpr uint32_t kRescRec = 5;   // words per candidate in RescueParams::c_rec

struct RescueParams {
  uint32_t n_pairs, n_records;  // run()'s records; the rescued ones are numbered from n_records on
  int32_t E;
  int64_t min_insert, max_insert;
  const uint32_t *rec_begin;  // 2 n_pairs + 1
  uint16_t *flag;
  uint32_t *tid, *pos0;
  uint8_t *nm;
  uint32_t *cigar_off, *cigar, *md_off, *s_read;
  uint8_t *md;
  const uint8_t *bases;
  const uint64_t *read_off;
  const uint8_t *ref_raw;
  uint64_t ref_bytes;
  const uint64_t *seq_off;
  const uint32_t *seq_len;
  const uint8_t *disc;           // pair_probe_kernel's flag per pair; nullptr: pairs with records on both sides are no candidates
  uint32_t *ctl;                 // [0] candidates, [1] jobs, [2] overflow queue length, [3] overflow staging too small (never),
                                 // [4] kept records of pairs with records on both sides
  uint32_t *cand_pair;           // per candidate: its pair
  uint32_t *jobs;                // candidate << 4 | direction << 3 | anchor index
  unsigned long long *best;      // per candidate: (nm(a) + ed) << 36 | d << 35 | a << 32 | pos0, ~0 = no hit
  uint32_t lanes, text_words, pat_words, max_len;  // LDS plan of the trace kernel
  uint32_t ops_cap, md_cap;
  uint32_t *t_ops;               // first pass, per candidate: ops_cap runs, md_cap MD characters
  uint8_t *t_md;
  uint32_t o_ops_cap, o_md_cap;  // overflow pass, per queued candidate: room for the longest walk (trace_kernel's staging)
  uint32_t *o_ops;
  uint8_t *o_md;
  uint32_t *ovf_queue;           // candidates whose CIGAR or MD outgrew the first pass's staging
  uint32_t overflow_pass;        // rescue_trace_kernel: 0 = every candidate, 1 = the queued ones
  uint32_t *c_rec;               // per candidate (kRescRec words): tid, pos0, flag | nm << 16, n_ops | n_md << 16, staging
  uint32_t *kept, *k_ops, *k_md; // per pair (n_pairs + 1): the kept record's 1, runs, MD characters (0 0 0 otherwise)
  const uint32_t *s_kept, *s_ops, *s_md;  // their exclusive scans
  uint32_t cig_total, md_total;  // run()'s CIGAR runs and MD characters
  uint32_t flip1, flip2;         // the library's orientation, as PairParams's
};

// pair i's candidate view in direction d: the anchors' mate (A: mate 1 for d = 0, mate 2 for d = 1) and the searched mate (B),
// and the two mates' flips
struct RescuePair {
  uint32_t a0, na, b_read, flip_a, flip_b;
};
__device__ __forceinline__ RescuePair rescue_pair(const RescueParams &p, uint32_t i, uint32_t d) {
  const uint32_t a_read = d ? p.n_pairs + i : i;
  RescuePair r;
  r.a0 = p.rec_begin[a_read], r.na = p.rec_begin[a_read + 1] - r.a0, r.b_read = d ? i : p.n_pairs + i;
  r.flip_a = d ? p.flip2 : p.flip1, r.flip_b = d ? p.flip1 : p.flip2;
  return r;
}
constexpr unsigned long long kBestDir = 1ull << 35;  // the direction's bit of RescueParams::best

// an anchor's window of B's pos0 ([lo, hi], empty when lo > hi) and the strand B is searched on (flip_b: B's mate's flip)
struct RescueWindow {
  int64_t lo, hi;
  uint32_t tid, rc;  // rc: B reverse-complemented (the anchor is virtually forward, or B's mate is flipped, not both)
};
__device__ __forceinline__ RescueWindow rescue_window(const RescueParams &p, const MateRec &an, int64_t L, uint32_t flip_b) {
  RescueWindow w;
  w.tid = an.tid;
  const int64_t pa = an.pos0, ea = (int64_t)an.end0;
  if (!an.v) {
    w.rc = 1u, w.lo = pa + p.min_insert - L > pa ? pa + p.min_insert - L : pa, w.hi = pa + p.max_insert - L;
  } else {
    w.rc = 0u, w.lo = ea - p.max_insert > 0 ? ea - p.max_insert : 0, w.hi = ea - p.min_insert < pa ? ea - p.min_insert : pa;
  }
  w.rc ^= flip_b >> 4;
  return w;
}

__device__ __forceinline__ MateRec rescue_rec(const RescueParams &p, uint32_t r, uint32_t flip) {
  PairParams q{};
  q.tid = p.tid, q.pos0 = p.pos0, q.flag = p.flag, q.nm = p.nm, q.cigar_off = p.cigar_off, q.cigar = p.cigar;
  return mate_rec(q, r, flip);
}

// character j of B as searched: the read itself, or fo_revcomp's reverse complement (ACGT complemented in upper case, anything else N)
__device__ __forceinline__ uint32_t rescue_char(const uint8_t *fwd, int64_t L, int64_t j, uint32_t rc) {
  if (!rc) return fwd[j];
  const uint32_t c = base_code(fwd[L - 1 - j]);
  return c < 4u ? (uint32_t)"TGCA"[c] : (uint32_t)'N';
}

__global__ void __launch_bounds__(256) rescue_jobs_kernel(RescueParams p) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.n_pairs) return;
  const uint32_t na = p.rec_begin[i + 1] - p.rec_begin[i], nb = p.rec_begin[p.n_pairs + i + 1] - p.rec_begin[p.n_pairs + i];
  if ((na == 0) == (nb == 0) && !(na && p.disc && p.disc[i])) return;
  uint32_t anchors = 0;  // bit d << 3 | a: record a of direction d's A is an anchor
  for (uint32_t d = 0; d < 2u; ++d) {
    const RescuePair rp = rescue_pair(p, i, d);
    const uint32_t n_look = rp.na < kRescueAnchors ? rp.na : kRescueAnchors;
    for (uint32_t a = 0; a < n_look; ++a)
      if (!(p.flag[rp.a0 + a] & kFlagBroken)) anchors |= 1u << (d << 3 | a);
  }
  if (!anchors) return;
  const uint32_t k = atomicAdd(&p.ctl[0], 1u);
  p.cand_pair[k] = i, p.best[k] = ~0ull;
  uint32_t j = atomicAdd(&p.ctl[1], (uint32_t)__builtin_popcount(anchors));
  for (; anchors; anchors &= anchors - 1u) p.jobs[j++] = k << 4 | (uint32_t)__builtin_ctz(anchors);
}

// fo_banded_ed32 (E, pat[0 .. L + 2E), text codes tc[0 .. L)): the same operations on the same 32-bit words, the read's code
// mask built from three bit planes of the window (Peq[code] of the reference = the band's bits whose three code bits all agree)
__device__ __forceinline__ int rescue_myers(const uint8_t *pat, const uint8_t *tc, int L, int E, int *end_out) {
  uint32_t B0 = 0, B1 = 0, B2 = 0;
  for (int j = 0; j < 2 * E; ++j) {
    const uint32_t pc = base_code(pat[j]);
    B0 |= (pc & 1u) << j, B1 |= ((pc >> 1) & 1u) << j, B2 |= ((pc >> 2) & 1u) << j;
  }
  const int sh = 2 * E;
  const uint32_t band = (2u << sh) - 1u;
  uint32_t vp = 0, vn = 0;
  int score = 0;
  for (int i0 = 0; i0 < L; i0 += 16) {
    const uint4 w = load_u128_unaligned(pat + sh + i0);  // (up to 15 bytes past the window: inside the reference's slack)
    const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int i = i0 + u;
      if (i >= L) break;
      const uint32_t pc = base_code((ws[u >> 2] >> (8 * (u & 3))) & 0xFFu), t = tc[i];
      B0 |= (pc & 1u) << sh, B1 |= ((pc >> 1) & 1u) << sh, B2 |= ((pc >> 2) & 1u) << sh;
      const uint32_t m0 = 0u - (t & 1u), m1 = 0u - ((t >> 1) & 1u), m2 = 0u - ((t >> 2) & 1u);
      uint32_t x = (~((B0 ^ m0) | (B1 ^ m1) | (B2 ^ m2)) & band) | vn;
      const uint32_t d0 = ((vp + (x & vp)) ^ vp) | x;
      const uint32_t hn = vp & d0;
      const uint32_t hp = vn | ~(vp | d0);
      x = d0 >> 1;
      vn = x & hp;
      vp = hn | ~(x | hp);
      score += 1 - (int)(d0 & 1u);
      if (score > 3 * E) return E + 1;
      B0 >>= 1, B1 >>= 1, B2 >>= 1;
    }
  }
  int best = score, end = L - 1;
  for (int j = 0; j < 2 * E; ++j) {
    score += (int)((vp >> j) & 1u) - (int)((vn >> j) & 1u);
    if (score < best) best = score, end = L + j;  // first strict minimum
  }
  *end_out = end;
  return best;
}

__global__ void __launch_bounds__(256) rescue_search_kernel(RescueParams p) {
  __shared__ uint8_t codes[kResWaves][1024];  // the mate's character codes (reads are <= 1024 bases on the device)
  const uint32_t ln = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  uint8_t *tc = codes[wv];
  const uint32_t n_jobs = p.ctl[1];
  const int E = p.E;
  const int64_t W = 2 * E + 1;
  for (uint32_t job = blockIdx.x * kResWaves + wv; job < n_jobs; job += gridDim.x * kResWaves) {
    const uint32_t k = p.jobs[job] >> 4, d = p.jobs[job] >> 3 & 1u, a = p.jobs[job] & 7u;
    const RescuePair rp = rescue_pair(p, p.cand_pair[k], d);
    const MateRec an = rescue_rec(p, rp.a0 + a, rp.flip_a);
    const uint64_t off = p.read_off[rp.b_read];
    const int64_t L = (int64_t)(p.read_off[rp.b_read + 1] - off);
    const RescueWindow w = rescue_window(p, an, L, rp.flip_b);
    if (w.lo > w.hi || L == 0) continue;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // (the previous job's reads of tc are done)
    __builtin_amdgcn_wave_barrier();
    for (int64_t j = ln; j < L; j += 64) tc[j] = (uint8_t)base_code(rescue_char(p.bases + off, L, j, w.rc));
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int64_t slen = p.seq_len[w.tid];
    const uint8_t *seq = p.ref_raw + p.seq_off[w.tid];
    const int64_t n_tiles = (w.hi - w.lo) / W + 1;
    unsigned long long key = ~0ull;
    for (int64_t t = ln; t < n_tiles; t += 64) {
      const int64_t c = w.lo + t * W;
      if (c + L + 2 * E > slen) continue;
      int end = 0;
      const int ed = rescue_myers(seq + c, tc, (int)L, E, &end);
      const int64_t pos = c + end - L + 1;
      if (ed <= E && pos <= w.hi) {
        const unsigned long long h = (unsigned long long)ed << 32 | (uint64_t)pos;
        key = h < key ? h : key;
      }
    }
    for (int d = 32; d > 0; d >>= 1) {
      const unsigned long long o = (unsigned long long)__shfl_xor(key, d);
      key = o < key ? o : key;
    }
    if (ln == 0 && key != ~0ull)
      atomicMin(&p.best[k], (unsigned long long)(an.nm + (uint32_t)(key >> 32)) << 36 | (unsigned long long)(d << 3 | a) << 32 | (uint32_t)key);
  }
}

// One lane per candidate, the general traceback's LDS layout (trace_kernel) sized for E.  The first pass stages a record's
// CIGAR and MD in room for a walk of E errors on canonical characters; one that outgrows it (lower-case or IUPAC characters on
// either side: the walk and MD compare characters, so every column can be an MD character) is queued and traced again by the
// overflow pass, whose staging holds the longest walk (as trace_kernel's).
__global__ void __launch_bounds__(64) rescue_trace_kernel(RescueParams p) {
  extern __shared__ uint32_t lds[];
  const uint32_t nl = p.lanes, ln = threadIdx.x;
  uint32_t *text_w = lds;
  uint32_t *pat_w = text_w + p.text_words * nl;
  uint32_t *d0_w = pat_w + p.pat_words * nl;
  uint32_t *hp_w = d0_w + p.max_len * nl;
  const bool ovf = p.overflow_pass != 0;
  const uint32_t n_items = ovf ? p.ctl[2] : p.ctl[0];
  const int E = p.E;
  for (uint32_t base = blockIdx.x * nl; base < n_items; base += gridDim.x * nl) {
    const uint32_t item = base + ln;
    if (ln >= nl || item >= n_items) continue;
    const uint32_t k = ovf ? p.ovf_queue[item] : item;
    const unsigned long long best = p.best[k];
    if (best == ~0ull) continue;
    const uint32_t i = p.cand_pair[k], a = (uint32_t)(best >> 32) & 7u, pos = (uint32_t)best;
    const RescuePair rp = rescue_pair(p, i, best & kBestDir ? 1u : 0u);
    const MateRec an = rescue_rec(p, rp.a0 + a, rp.flip_a);
    const int ed = (int)(best >> 36) - (int)an.nm;
    const uint64_t off = p.read_off[rp.b_read];
    const int L = (int)(p.read_off[rp.b_read + 1] - off);
    const RescueWindow w = rescue_window(p, an, L, rp.flip_b);
    const int64_t W = 2 * E + 1;
    const int64_t c = w.lo + ((int64_t)pos - w.lo) / W * W;  // the tile the hit came from (tiles are disjoint in pos0)
    const int end = (int)((int64_t)pos - c) + L - 1;
    for (int j = 0; j < L; j += 4) {
      uint32_t word = 0;
      for (int u = 0; u < 4 && j + u < L; ++u) word |= rescue_char(p.bases + off, L, j + u, w.rc) << (8 * u);
      text_w[(uint32_t)(j / 4) * nl + ln] = word;
    }
    const uint64_t pat_abs = p.seq_off[w.tid] + (uint64_t)c;
    const uint8_t *pattern = p.ref_raw + pat_abs;
    for (int j = 0; j < L + 2 * E; j += 16) {  // (inside the sequence, and the reference buffer has 64 bytes of slack behind it)
      const uint4 q = load_u128_unaligned(pattern + j);
      const uint32_t ws[4] = {q.x, q.y, q.z, q.w};
      for (int u = 0; u < 4; ++u)
        if ((uint32_t)(j / 4 + u) < p.pat_words) pat_w[(uint32_t)(j / 4 + u) * nl + ln] = ws[u];
    }
    LaneView v{text_w, pat_w, d0_w, hp_w, nl, ln};
    Staging st;
    if (ovf) st.ops = p.o_ops + (size_t)item * p.o_ops_cap, st.md = p.o_md + (size_t)item * p.o_md_cap, st.ops_cap = p.o_ops_cap, st.md_cap = p.o_md_cap;
    else st.ops = p.t_ops + (size_t)k * p.ops_cap, st.md = p.t_md + (size_t)k * p.md_cap, st.ops_cap = p.ops_cap, st.md_cap = p.md_cap;
    const int start = trace_record(v, pattern, -(int64_t)pat_abs, (int64_t)p.ref_bytes - 1 - (int64_t)pat_abs, L, E, ed, end, st);
    if (st.overflow) {
      if (ovf) atomicAdd(&p.ctl[3], 1u);  // cannot happen: this staging holds the longest possible walk
      else p.ovf_queue[atomicAdd(&p.ctl[2], 1u)] = k;
      continue;
    }
    if (start < 0) continue;
    MateRec rs;
    rs.tid = w.tid, rs.pos0 = (uint32_t)(c + start), rs.flag = w.rc ? 16u : 0u, rs.v = rs.flag ^ rp.flip_b, rs.nm = (uint32_t)ed;
    uint64_t span = 0;
    for (uint32_t u = 0; u < st.n_ops; ++u)
      if ((st.ops[u] & 0xFu) == kOpM || (st.ops[u] & 0xFu) == kOpD) span += st.ops[u] >> 4;
    rs.end0 = (uint64_t)rs.pos0 + span;
    PairParams q{};
    q.min_insert = p.min_insert, q.max_insert = p.max_insert;
    if (concordant(q, an, rs) < 0) continue;
    uint32_t *cr = p.c_rec + (size_t)k * kRescRec;
    cr[0] = rs.tid, cr[1] = rs.pos0, cr[2] = rs.flag | rs.nm << 16, cr[3] = st.n_ops | st.n_md << 16, cr[4] = ovf ? item + 1u : 0u;
    p.kept[i] = 1u, p.k_ops[i] = st.n_ops, p.k_md[i] = st.n_md;
  }
}

__global__ void __launch_bounds__(256) rescue_append_kernel(RescueParams p) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k == 0) {  // the offsets' end behind the last rescued record
    const uint32_t n_kept = p.s_kept[p.n_pairs];
    p.cigar_off[p.n_records + n_kept] = p.cig_total + p.s_ops[p.n_pairs];
    p.md_off[p.n_records + n_kept] = p.md_total + p.s_md[p.n_pairs];
  }
  if (k >= p.ctl[0]) return;
  const uint32_t i = p.cand_pair[k];
  if (!p.kept[i]) return;
  const uint32_t rec = p.n_records + p.s_kept[i];
  const uint32_t *cr = p.c_rec + (size_t)k * kRescRec;
  p.tid[rec] = cr[0], p.pos0[rec] = cr[1], p.flag[rec] = (uint16_t)(cr[2] & 0xFFFFu), p.nm[rec] = (uint8_t)(cr[2] >> 16);
  p.s_read[rec] = rescue_pair(p, i, p.best[k] & kBestDir ? 1u : 0u).b_read;
  if (p.disc && p.disc[i]) atomicAdd(&p.ctl[4], 1u);
  const uint32_t co = p.cig_total + p.s_ops[i], mo = p.md_total + p.s_md[i];
  p.cigar_off[rec] = co, p.md_off[rec] = mo;
  const uint32_t *ops = cr[4] ? p.o_ops + (size_t)(cr[4] - 1u) * p.o_ops_cap : p.t_ops + (size_t)k * p.ops_cap;
  const uint8_t *md = cr[4] ? p.o_md + (size_t)(cr[4] - 1u) * p.o_md_cap : p.t_md + (size_t)k * p.md_cap;
  for (uint32_t u = 0; u < (cr[3] & 0xFFFFu); ++u) p.cigar[co + u] = ops[u];
  for (uint32_t u = 0; u < (cr[3] >> 16); ++u) p.md[mo + u] = md[u];
}

}  // namespace

#define TAIL_TRY(expr)                                                             \
  do {                                                                             \
    hipError_t e_ = (expr);                                                        \
    if (e_ != hipSuccess) {                                                        \
      if (err) *err = std::string(#expr) + ": " + hipGetErrorString(e_);           \
      return e_ == hipErrorOutOfMemory ? FEM_ERR_NOMEM : FEM_ERR_HIP;              \
    }                                                                              \
  } while (0)

// The <kPair, kUnm, kMate> instance of a text or BAM kernel (K: sam_len_kernel, sam_write_kernel, bam_len_kernel, bam_write_kernel)
// (mate: its kMate form, which only paired texts have)
#define TEXT_KERNEL(K, pair, um, mate) \
  ((mate) ? ((um) ? K<true, true, true> : K<true, false, true>) : (um) ? ((pair) ? K<true, true> : K<false, true>) : ((pair) ? K<true> : K<false>))

// A timed stage: what `stream` does between begin() and end().  A stage that starts where another one ends has no first
// event of its own (follow()).  ran: it was recorded in the last call.
struct Span {
  femb::Event first, last;
  const femb::Event *from = &first;
  bool ran = false;
  hipError_t create() {  // (once: reserve() ahead of the first batch, or the first record())
    const hipError_t e = first.create();
    return e != hipSuccess ? e : last.create();
  }
  hipError_t record(const femb::Event &ev, hipStream_t stream) {
    const hipError_t e = create();
    return e != hipSuccess ? e : hipEventRecord(ev, stream);
  }
  hipError_t begin(hipStream_t stream) { return from = &first, record(first, stream); }
  void follow(const Span &before) { from = &before.last; }
  hipError_t end(hipStream_t stream) { return ran = true, record(last, stream); }
  float ms() const {  // < 0: it did not run, or the stream has not passed its end
    float t = 0.f;
    return ran && hipEventElapsedTime(&t, *from, last) == hipSuccess ? t : -1.f;
  }
};

// The LDS plan of trace_kernel and rescue_trace_kernel for reads of up to max_len characters at e edits: lanes = records one
// 64-thread block walks at a time.
struct TracePlan { uint32_t text_words, pat_words, lanes, lds_bytes; };
static int trace_plan(uint32_t max_len, int e, TracePlan *t, std::string *err) {
  t->text_words = (max_len + 3) / 4 + 4, t->pat_words = (max_len + 2 * (uint32_t)e + 3) / 4 + 4;
  const uint32_t words_per_lane = t->text_words + t->pat_words + 2 * max_len;
  t->lanes = std::min<uint32_t>(64, (64u * 1024u / 4u) / words_per_lane);
  t->lds_bytes = t->lanes * words_per_lane * 4u;
  if (t->lanes) return FEM_OK;
  if (err) *err = "read too long for the device traceback";
  return FEM_ERR_UNSUPPORTED;
}
// ... and a record's room in their overflow staging, the longest possible walk: every step opens a run; the MD of a run
// never exceeds two characters per column.
struct OverflowCaps { uint32_t ops, md; };
static OverflowCaps overflow_caps(uint32_t max_len, int e) { return {2 * max_len + 2 * (uint32_t)e + 8, 8 * max_len + 128}; }

// The scratch bytes rocprim's exclusive scan of n items takes, where that is more than *need.
template <class In, class Out, class T, class Op>
static hipError_t scan_need(size_t *need, In in, Out out, T init, size_t n, Op op) {
  size_t bytes = 0;
  const hipError_t e = rocprim::exclusive_scan(nullptr, bytes, in, out, init, n, op, (hipStream_t) nullptr);
  *need = std::max(*need, bytes);
  return e;
}

// `count` elements of a device array, from element `first` on, to a pinned buffer of min_cap elements at least: queued on `stream`.
template <class T, class S>
static hipError_t copy_home(PinBuf<T> &dst, const DevBuf<S> &src, size_t first, size_t count, size_t min_cap, hipStream_t stream) {
  static_assert(sizeof(T) == sizeof(S), "the pinned copy has the device array's elements");
  const hipError_t e = dst.ensure(std::max(count, min_cap));
  if (e != hipSuccess || !count) return e;
  return hipMemcpyAsync(dst.get(), src.get() + first, count * sizeof(T), hipMemcpyDeviceToHost, stream);
}

// ---- soft clips of a trimmed batch (include/fem_hip.h, fem_dev_set_trim) ----
// The records' CIGAR words once more with the clips of their reads as S operations (op 4) around them, in arrays of their own
// that the text side reads in place of cigar_off / cigar: a record without FLAG 16 gets its read's clip5 in front and clip3
// behind, one with it clip3 in front and clip5 behind (the CIGAR runs in the reference's direction), for counts > 0 only; a
// record without operations (0x8000: it prints *) keeps none.  The records themselves (fem_batch_records, fem_batch_pairs, the
// pairing, the spans) stay as they are.
struct ClipParams {
  uint32_t n_records;
  const uint32_t *s_read;
  const uint16_t *flag;
  const uint32_t *cigar_off, *cigar;
  const uint16_t *clip5, *clip3;
  uint32_t *c_ops, *c_off, *c_cigar;  // c_ops, c_off: n_records + 1
};
__device__ __forceinline__ uint2 clip_sides(const ClipParams &p, uint32_t rec) {
  const uint32_t r = p.s_read[rec], c5 = p.clip5[r], c3 = p.clip3[r];
  return (p.flag[rec] & 16u) ? make_uint2(c3, c5) : make_uint2(c5, c3);
}
__global__ void __launch_bounds__(256) clip_count_kernel(ClipParams p) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > p.n_records) return;
  uint32_t n = 0;
  if (i < p.n_records) {
    n = p.cigar_off[i + 1] - p.cigar_off[i];
    if (n) {
      const uint2 c = clip_sides(p, i);
      n += (c.x ? 1u : 0u) + (c.y ? 1u : 0u);
    }
  }
  p.c_ops[i] = n;
}
__global__ void __launch_bounds__(256) clip_write_kernel(ClipParams p) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.n_records) return;
  const uint32_t c0 = p.cigar_off[i], c1 = p.cigar_off[i + 1];
  if (c1 == c0) return;
  const uint2 c = clip_sides(p, i);
  uint32_t *w = p.c_cigar + p.c_off[i];
  if (c.x) *w++ = (c.x << 4) | 4u;
  for (uint32_t k = c0; k < c1; ++k) *w++ = p.cigar[k];
  if (c.y) *w++ = (c.y << 4) | 4u;
}

// The words of h_ctl, the pinned buffer the kernels' counters come home in: 0 .. 3 run()'s ctl (2: a text's asserted records,
// 3: bam()'s name check), 4 5 run()'s CIGAR and MD totals, 6 7 a text's size, 8 9 a line index's counts, 10 11 the fold index's (entries, folding slots), from kCtlInsert on
// estimate_insert()'s kInsertCtl words (estimate_library(): three times as many).
constexpr size_t kCtlInsert = 12, kCtlWords = kCtlInsert + 3 * kInsertCtl;

struct Tail::Impl {
  DevBuf<uint32_t> rec_begin, queue, ctl, u_misc, s_misc, s_read, t_ops, o_ops, ovf, rec_list, src_slot, n_ops, n_md, tid, pos0, cigar_off, md_off, cigar;
  DevBuf<uint64_t> u_cand, s_cand;
  DevBuf<uint8_t> t_md, o_md, nm, md, scan_tmp;
  DevBuf<uint16_t> flag;
  DevBuf<unsigned long long> line_len, line_off, qual_at;
  DevBuf<uint8_t> text;
  PinBuf<uint32_t> h_ctl, h_rec_begin, h_tid, h_pos0, h_cigar_off, h_md_off, h_cigar;
  PinBuf<uint16_t> h_flag;
  PinBuf<uint8_t> h_nm;
  PinBuf<char> h_md, h_text;
  PinBuf<uint64_t> h_qual_at;
  // pair mode (pair()): per line, the pairs' line ranges, the proper-pair counter; their host copies (pair_fetch())
  DevBuf<uint32_t> perm, mtid, mpos0, pair_begin, pair_ctl;
  DevBuf<uint16_t> pflag;
  DevBuf<int32_t> tlen;
  // MAPQ (LineOptions::mapq): per read (single-end), per line (pair(): pair_kernel<true>'s bytes, then the MAPQ)
  DevBuf<uint8_t> q_read, lmq;
  // lines for unmapped reads (LineOptions::unmapped): the marks, their scan, each line's source, the line count
  // (the line filter, LineOptions::strata / max_hits, uses the same four: its counts, their scan, the sources, the line count)
  DevBuf<uint32_t> u_cnt, u_before, usrc, u_ctl;
  // XA:Z (LineOptions::xa_entries): the slots' three counts and their scans, the entries' bytes, the index after folding, the folded
  // lines' sources, the folding slots; what the last text's write kernel takes of them
  DevBuf<uint32_t> x_cnt, x_scan, x_bytes, x_usrc, x_src, x_list;
  DevBuf<uint8_t> x_scan_tmp;
  XaParams xa{};
  // the RG tag (LineOptions::read_group): the ID on the device, the pinned copy it came from, and what that holds
  DevBuf<uint8_t> rg;
  PinBuf<uint8_t> h_rg;
  std::string rg_id;
  // the mate tags (LineOptions::mate_tags): mate_score_kernel's number per read
  DevBuf<uint32_t> m_score;
  // a trimmed batch (TailInput::clip5): the records' CIGARs with their S operations, for the text side
  DevBuf<uint32_t> c_ops, c_off, c_cigar;
  PinBuf<uint32_t> h_perm, h_mtid, h_mpos0, h_pair_begin, h_pair_ctl;
  PinBuf<uint16_t> h_pflag;
  PinBuf<int32_t> h_tlen;
  // mate rescue (pair() with LineOptions::rescue): candidates, jobs, best hits, the tracebacks' staging, the kept flags and their scans
  DevBuf<uint32_t> r_ctl, r_cand, r_jobs, r_ops, r_rec, r_ovf, r_o_ops, r_kept, r_scan;
  DevBuf<unsigned long long> r_best;
  DevBuf<uint8_t> r_md, r_o_md, r_scan_tmp, r_disc;
  PinBuf<uint32_t> h_r_ctl, h_r_tid, h_r_pos0, h_r_cigar_off, h_r_cigar, h_r_md_off;
  PinBuf<uint16_t> h_r_flag;
  PinBuf<uint8_t> h_r_nm;
  PinBuf<char> h_r_md;
  // the insert estimate (estimate_insert()): the histogram's kInsertBins bins, then the kInsertCtl words of its outcome
  DevBuf<uint32_t> ins_hist;
  // BAM (bam()): the name check, the record offsets home (the member cuts), the compressor
  DevBuf<uint32_t> bam_ctl;
  PinBuf<uint64_t> h_line_off;
  femz::Bgzf bgzf;
  std::vector<uint64_t> cuts;
  uint32_t last_n = 0, last_nr = 0;  // what the last run() left on the device
  bool paired = false;               // pair() has run on it
  uint32_t n_resc = 0;               // rescued records the last pair() appended behind run()'s (records last_nr ..)
  uint32_t n_resc_disc = 0;          // ... those of pairs with records on both sides among them (LineOptions::rescue_discordant)
  bool pair_mapq = false;            // the last pair() left its MAPQ bytes in lmq, not yet made MAPQ by a text
  bool filtered = false;             // the last text went through the line filter
  bool um_kernels = false;           // ... its kernels are the kUnm instances (lines for unmapped reads, or the filter's index)
  uint32_t n_unm = 0;                // lines for unmapped reads in the last text
  uint32_t n_base_last = 0;          // the lines the last text had before the filter and without the unmapped reads'
  uint32_t n_filtered = 0;           // lines the filter left out of the last text
  bool cov_queued = false;           // coverage_kernel has been queued since the last run() (LineOptions::coverage)
  bool folded = false;               // the last text went through the fold index (LineOptions::xa_entries)
  uint32_t n_xa = 0, n_xa_slots = 0; // lines folded into XA:Z entries in the last text, and the slots that carry them
  Span span[kStages];                // (Tail::stage_ms)
  femb::Event ev_text;               // the SAM text has arrived in h_text

  void not_run(std::initializer_list<Stage> stages) {
    for (Stage s : stages) span[s].ran = false;
  }
  // rocprim's exclusive scan of n items on `stream`; its scratch is scan_tmp, which reserve() and lines() make large
  // enough (scan_need), or `tmp`
  template <class In, class Out, class T, class Op>
  hipError_t scan(In in, Out out, T init, size_t n, Op op, hipStream_t stream, const DevBuf<uint8_t> *tmp = nullptr) {
    if (!tmp) tmp = &scan_tmp;
    size_t bytes = tmp->bytes();
    return rocprim::exclusive_scan(tmp->get(), bytes, in, out, init, n, op, stream);
  }
  // Both offsets of n records in one pass: (runs, MD characters) pairs into (cigar_off, md_off).  need: the scratch it takes only.
  hipError_t scan_runs_md(size_t n, hipStream_t stream, size_t *need = nullptr) {
    auto lens = rocprim::make_zip_iterator(rocprim::make_tuple(n_ops.get(), n_md.get()));
    auto offs = rocprim::make_zip_iterator(rocprim::make_tuple(cigar_off.get(), md_off.get()));
    const auto zero = rocprim::make_tuple(0u, 0u);
    return need ? scan_need(need, lens, offs, zero, n, PairPlus()) : scan(lens, offs, zero, n, PairPlus(), stream);
  }
  // Mate rescue: (kept, runs, MD characters) of p1 pairs, the three parts of r_kept, into those of r_scan; its scratch is
  // r_scan_tmp, made large enough here.
  hipError_t scan_kept(size_t p1, hipStream_t stream) {
    auto lens = rocprim::make_zip_iterator(rocprim::make_tuple(r_kept.get(), r_kept + p1, r_kept + 2 * p1));
    auto offs = rocprim::make_zip_iterator(rocprim::make_tuple(r_scan.get(), r_scan + p1, r_scan + 2 * p1));
    const auto zero = rocprim::make_tuple(0u, 0u, 0u);
    size_t need = 16;
    hipError_t e = scan_need(&need, lens, offs, zero, p1, TriplePlus());
    if (e == hipSuccess) e = r_scan_tmp.ensure(need);
    return e != hipSuccess ? e : scan(lens, offs, zero, p1, TriplePlus(), stream, &r_scan_tmp);
  }
  // XA:Z: (lines that stay, entries, folding slots) of n1 slots, the three parts of x_cnt, into those of x_scan
  hipError_t scan_folds(size_t n1, hipStream_t stream) {
    auto lens = rocprim::make_zip_iterator(rocprim::make_tuple(x_cnt.get(), x_cnt + n1, x_cnt + 2 * n1));
    auto offs = rocprim::make_zip_iterator(rocprim::make_tuple(x_scan.get(), x_scan + n1, x_scan + 2 * n1));
    const auto zero = rocprim::make_tuple(0u, 0u, 0u);
    size_t need = 16;
    hipError_t e = scan_need(&need, lens, offs, zero, n1, TriplePlus());
    if (e == hipSuccess) e = x_scan_tmp.ensure(need);
    return e != hipSuccess ? e : scan(lens, offs, zero, n1, TriplePlus(), stream, &x_scan_tmp);
  }
  // The records as pair_kernel reads them ...
  template <class P>
  void bind_pairing(P *p) const {
    p->rec_begin = rec_begin, p->flag = flag, p->tid = tid, p->pos0 = pos0;
    p->nm = nm, p->cigar_off = cigar_off, p->cigar = cigar;
  }
  // ... and whole, as the text and the rescue kernels do (where the arrays are now: again after one of them has grown)
  template <class P>
  void bind_records(P *p) const {
    bind_pairing(p);
    p->s_read = s_read, p->md_off = md_off, p->md = md;
  }

  // sam() and bam(): the lines of run()'s records, or of pair()'s (rescued records included).  Fills *p (all but the text and
  // qual_at); opt.mapq: first the MAPQ kernel (stage kMapq); then stage kText begins: each line's length (bad_name: as BAM, a
  // name over 254 characters setting it; else as SAM), their scan into line_off, the count of asserted records to h_ctl[2].
  // opt.unmapped: the line index first (stage kUnmappedIndex).  The line count is known on the device alone then:
  // p->n_records bounds it (records + reads; the lengths behind the last line are zero, so line_off[p->n_records] is the text's
  // size all the same) and the count comes to h_ctl[8]; counted() puts it into p->n_records once the stream has been waited for.
  // opt.strata / opt.max_hits (the line filter): the line index is report_kernel's instead (stage kFilterIndex),
  // unmapped reads' lines included where opt.unmapped asks for them; the count comes home the same way, the unmapped slots'
  // to h_ctl[9].  The text and BAM kernels are the kUnm instances then, with or without opt.unmapped: without it u_base lies
  // above every source and pair_begin is nullptr (mate_cols), so that no line takes a shape it has not without the filter.
  // opt.read_group / opt.hit_tags (the tags behind MD:Z): the ID goes to the device when it is another than the last text's;
  // NH and HI read the slots' line ranges that are there already (hit_tags(), above): the filter's scan, or the index it began from.
  // opt.mates() (the mate tags, the kernels' kMate instances): with qualities on the device mate_score_kernel runs in front of
  // stage kText (stage kMateScore); without them the lines carry no ms.
  int lines(const TailInput &in, const SamInput &names, const LineOptions &opt, uint32_t *bad_name, hipStream_t stream, int n_cu,
            SamParams *p, std::string *err) {
    // (folding reads report_kernel's index: without the line filter that kernel runs with both of its tests off and keeps every line)
    const bool pair_order = opt.paired, fold = opt.folds(), report = opt.filters() || fold;
    if (pair_order && !paired) {
      if (err) *err = "the records were not paired (Tail::pair)";
      return FEM_ERR_STATE;
    }
    const uint32_t n_base = last_nr + (pair_order ? n_resc : 0u);
    if (opt.unmapped && (uint64_t)n_base + last_n > 0xFFFFFFF0ull) {
      if (err) *err = "more than 2^32 lines in one batch; split the batch";
      return FEM_ERR_UNSUPPORTED;
    }
    const uint32_t nr = n_base + (opt.unmapped ? last_n : 0u);
    const size_t r1 = (size_t)nr + 1, n1 = (size_t)last_n + 1;
    not_run({kText, kMapq, kUnmappedIndex, kFilterIndex, kMateScore, kXaIndex, kCoverage});
    TAIL_TRY(line_len.ensure(r1));
    TAIL_TRY(line_off.ensure(r1));
    TAIL_TRY(h_ctl.ensure(kCtlWords));
    size_t need = 16;
    TAIL_TRY(scan_need(&need, line_len.get(), line_off.get(), 0ull, r1, rocprim::plus<unsigned long long>()));
    if (opt.unmapped || report) {
      TAIL_TRY(u_cnt.ensure(n1));
      TAIL_TRY(u_before.ensure(n1));
      TAIL_TRY(usrc.ensure(std::max<size_t>(nr, 1)));
      TAIL_TRY(u_ctl.ensure(4));
      TAIL_TRY(scan_need(&need, u_cnt.get(), u_before.get(), 0u, n1, rocprim::plus<uint32_t>()));
    }
    TAIL_TRY(scan_tmp.ensure(need));
    bind_records(p);
    p->n_records = nr;
    p->bases = in.bases, p->read_off = in.read_off;
    const uint64_t *text_off = in.read_off;  // the offsets SEQ, QUAL and ms:i go by
    if (in.clip5) {  // a trimmed batch: the whole reads' letters, the CIGARs with the clips (in front of everything that reads them)
      const size_t b1 = (size_t)n_base + 1;
      TAIL_TRY(c_ops.ensure(b1));
      TAIL_TRY(c_off.ensure(b1));
      TAIL_TRY(c_cigar.ensure(cigar.size() + 2 * (size_t)n_base + 1));
      size_t clip_need = 16;
      TAIL_TRY(scan_need(&clip_need, c_ops.get(), c_off.get(), 0u, b1, rocprim::plus<uint32_t>()));
      if (clip_need > need) TAIL_TRY(scan_tmp.ensure(clip_need));
      ClipParams c{};
      c.n_records = n_base, c.s_read = s_read, c.flag = flag, c.cigar_off = cigar_off, c.cigar = cigar;
      c.clip5 = in.clip5, c.clip3 = in.clip3, c.c_ops = c_ops, c.c_off = c_off, c.c_cigar = c_cigar;
      const dim3 clip_grid((n_base + 256u) / 256u);
      hipLaunchKernelGGL(clip_count_kernel, clip_grid, dim3(256), 0, stream, c);
      TAIL_TRY(hipGetLastError());
      TAIL_TRY(scan(c_ops.get(), c_off.get(), 0u, b1, rocprim::plus<uint32_t>(), stream));
      hipLaunchKernelGGL(clip_write_kernel, clip_grid, dim3(256), 0, stream, c);
      TAIL_TRY(hipGetLastError());
      p->cigar_off = c_off, p->cigar = c_cigar;
      p->bases = in.text_bases, p->read_off = text_off = in.text_read_off;
    }
    p->quals = names.quals, p->names = names.names, p->name_off = names.name_off, p->ref_names = names.ref_names, p->ref_name_off = names.ref_name_off;
    p->line_len = line_len, p->line_off = line_off;
    p->asserted = ctl + 2;  // (ctl[2] is zero after a successful run())
    if (pair_order) {
      p->perm = perm, p->pflag = pflag, p->mtid = mtid, p->mpos0 = mpos0;
      p->tlen = tlen;
    }
    p->n_reads = last_n;
    if (!opt.read_group.empty()) {
      const size_t rg_len = opt.read_group.size();
      if (!rg || rg_id != opt.read_group) {
        TAIL_TRY(rg.ensure(256));
        TAIL_TRY(h_rg.ensure(256));
        TAIL_TRY(hipStreamSynchronize(stream));  // (the ID before may still be on its way out of h_rg, or in a text kernel's hands)
        memcpy(h_rg.get(), opt.read_group.data(), rg_len);
        TAIL_TRY(hipMemcpyAsync(rg, h_rg, rg_len, hipMemcpyHostToDevice, stream));
        rg_id = opt.read_group;
      }
      p->rg = rg, p->rg_len = (uint32_t)rg_len;
    }
    if (opt.hit_tags) {
      p->hit_tags = 1u, p->hit_by_line = report ? 1u : 0u;
      p->hit_begin = report ? u_before : pair_order ? pair_begin : rec_begin;
    }
    n_unm = 0;
    filtered = report, um_kernels = opt.unmapped || report, n_filtered = 0, n_base_last = n_base;
    folded = fold, n_xa = n_xa_slots = 0;
    if (report) {
      ReportParams f{};
      f.n_reads = last_n, f.n_base = n_base, f.begin = pair_order ? pair_begin : rec_begin;
      f.nm = nm, f.perm = pair_order ? perm : nullptr;
      f.strata = opt.strata >= 0 ? (uint32_t)opt.strata : kReportOff, f.max_hits = opt.max_hits >= 1 ? (uint32_t)opt.max_hits : kReportOff;
      f.unmapped = opt.unmapped ? 1u : 0u;
      f.cnt = u_cnt, f.before = u_before, f.usrc = usrc, f.n_lines = u_ctl;
      const dim3 grid((last_n + 256u) / 256u);
      Span &index = opt.filters() ? span[kFilterIndex] : span[kXaIndex];
      TAIL_TRY(index.begin(stream));
      TAIL_TRY(hipMemsetAsync(u_ctl, 0, 8, stream));
      hipLaunchKernelGGL(report_kernel<false>, grid, dim3(256), 0, stream, f);
      TAIL_TRY(hipGetLastError());
      TAIL_TRY(scan(u_cnt.get(), u_before.get(), 0u, n1, rocprim::plus<uint32_t>(), stream));
      hipLaunchKernelGGL(report_kernel<true>, grid, dim3(256), 0, stream, f);
      TAIL_TRY(hipGetLastError());
      if (opt.filters()) TAIL_TRY(index.end(stream));
      p->usrc = usrc, p->u_base = opt.unmapped ? n_base : kNoMate, p->n_reads = last_n, p->u_lines = u_ctl;
      p->pair_begin = opt.unmapped ? pair_begin : nullptr;
      if (fold) {  // (the entries read the records' arrays alone: *p holds what xa_index_kernel needs by now)
        TAIL_TRY(x_cnt.ensure(3 * n1));
        TAIL_TRY(x_scan.ensure(3 * n1));
        TAIL_TRY(x_bytes.ensure(n1));
        TAIL_TRY(x_usrc.ensure(std::max<size_t>(nr, 1)));
        TAIL_TRY(x_src.ensure(std::max<size_t>(nr, 1)));
        TAIL_TRY(x_list.ensure(n1));
        xa = XaParams{};
        xa.n_reads = last_n, xa.max_entries = (uint32_t)opt.xa_entries, xa.begin = u_before, xa.usrc = usrc;
        xa.cnt = x_cnt, xa.bytes = x_bytes, xa.scan = x_scan, xa.usrc_out = x_usrc, xa.xsrc = x_src, xa.xlist = x_list, xa.n_lines = u_ctl;
        if (opt.filters()) span[kXaIndex].follow(span[kFilterIndex]);
        hipLaunchKernelGGL(xa_index_kernel<false>, grid, dim3(256), 0, stream, *p, xa);
        TAIL_TRY(hipGetLastError());
        TAIL_TRY(scan_folds(n1, stream));
        hipLaunchKernelGGL(xa_index_kernel<true>, grid, dim3(256), 0, stream, *p, xa);
        TAIL_TRY(hipGetLastError());
        TAIL_TRY(span[kXaIndex].end(stream));
        p->usrc = x_usrc, p->xa_begin = x_scan, p->xa_n = x_cnt + n1, p->xa_bytes = x_bytes;
        if (opt.hit_tags) p->hit_begin = x_scan;
      }
      TAIL_TRY(hipMemcpyAsync(h_ctl + 8, u_ctl, fold ? 16 : 8, hipMemcpyDeviceToHost, stream));
    } else if (opt.unmapped) {
      UlineParams u{};
      u.n_reads = last_n, u.n_base = n_base, u.paired = pair_order ? 1u : 0u;
      u.begin = pair_order ? pair_begin : rec_begin;
      u.s_read = s_read, u.perm = perm;
      u.cnt = u_cnt, u.before = u_before, u.usrc = usrc, u.n_lines = u_ctl;
      TAIL_TRY(span[kUnmappedIndex].begin(stream));
      hipLaunchKernelGGL(unmapped_mark_kernel, dim3((last_n + 256u) / 256u), dim3(256), 0, stream, u);
      TAIL_TRY(hipGetLastError());
      TAIL_TRY(scan(u_cnt.get(), u_before.get(), 0u, n1, rocprim::plus<uint32_t>(), stream));
      const uint32_t work = std::max(n_base, last_n);
      hipLaunchKernelGGL(unmapped_src_kernel, dim3(std::max<uint32_t>(1u, std::min<uint32_t>((work + 255u) / 256u, (uint32_t)n_cu * 16u))),
                         dim3(256), 0, stream, u);
      TAIL_TRY(hipGetLastError());
      TAIL_TRY(span[kUnmappedIndex].end(stream));
      TAIL_TRY(hipMemcpyAsync(h_ctl + 8, u_ctl, 4, hipMemcpyDeviceToHost, stream));
      p->usrc = usrc, p->u_base = n_base, p->n_reads = last_n, p->u_lines = u_ctl;
      p->pair_begin = pair_begin;
    }
    if (opt.mapq) {
      if (pair_order && !pair_mapq) {
        if (err) *err = "the records were paired without MAPQ (Tail::pair)";
        return FEM_ERR_STATE;
      }
      MapqParams q{};
      q.n_reads = last_n, q.e = in.e, q.rec_begin = rec_begin, q.nm = nm;
      if (pair_order) {
        q.pair_begin = pair_begin, q.lmq = lmq;
        p->mapq = lmq;
        pair_mapq = false;  // (made MAPQ in place: once)
      } else {
        TAIL_TRY(q_read.ensure(std::max<size_t>(last_n, 1)));
        q.q_read = q_read;
        p->mapq = q_read;
      }
      TAIL_TRY(span[kMapq].begin(stream));
      if (last_n) {
        hipLaunchKernelGGL(mapq_kernel, dim3((last_n + 255u) / 256u), dim3(256), 0, stream, q);
        TAIL_TRY(hipGetLastError());
      }
      TAIL_TRY(span[kMapq].end(stream));
    }
    if (opt.covers()) {  // behind the MAPQ kernel, whose column it reads, and over the index as it was before folding
      const LineOptions::Coverage &cv = opt.coverage;
      CoverageParams c{};
      c.window = (uint32_t)cv.window, c.all_hits = cv.all_hits ? 1u : 0u, c.min_mapq = (uint32_t)cv.min_mapq, c.n_seq = cv.n_seq;
      c.bin_off = cv.bin_off, c.seq_len = cv.seq_len, c.bins = cv.bins;
      SamParams q = *p;
      c.n_lines = um_kernels ? nr : n_base;
      if (report) q.usrc = usrc, c.n_lines_at = u_before + last_n;  // (u_ctl[0] is the count after folding where the text folds)
      else if (opt.unmapped) c.n_lines_at = u_ctl;
      TAIL_TRY(span[kCoverage].begin(stream));
      if (c.n_lines) {
        const dim3 grid((c.n_lines + 255u) / 256u);
        if (um_kernels)
          hipLaunchKernelGGL((pair_order ? coverage_kernel<true, true> : coverage_kernel<false, true>), grid, dim3(256), 0, stream, q, c);
        else
          hipLaunchKernelGGL((pair_order ? coverage_kernel<true, false> : coverage_kernel<false, false>), grid, dim3(256), 0, stream, q, c);
        TAIL_TRY(hipGetLastError());
      }
      cov_queued = true;  // (a batch without lines is added too: nothing)
      TAIL_TRY(span[kCoverage].end(stream));
    }
    p->sam_seq = opt.sam_seq ? 1u : 0u;
    if (opt.mates()) {
      p->mate_tags = 1u, p->mate_begin = pair_begin;
      if (names.quals) {
        TAIL_TRY(m_score.ensure(std::max<size_t>(last_n, 1)));
        TAIL_TRY(span[kMateScore].begin(stream));
        if (last_n) {
          const uint32_t per_block = 256u / kScoreLanes;
          hipLaunchKernelGGL(mate_score_kernel, dim3((last_n + per_block - 1u) / per_block), dim3(256), 0, stream, names.quals, text_off, last_n,
                             m_score.get());
          TAIL_TRY(hipGetLastError());
        }
        TAIL_TRY(span[kMateScore].end(stream));
        p->mate_score = m_score;
      }
    }
    if (bad_name) TAIL_TRY(hipMemsetAsync(bad_name, 0, 4, stream));
    TAIL_TRY(span[kText].begin(stream));
    const dim3 len_grid(std::max<uint32_t>(1u, std::min<uint32_t>((nr + 256u) / 256u, (uint32_t)n_cu * 16u)));
    if (bad_name)
      hipLaunchKernelGGL(TEXT_KERNEL(bam_len_kernel, pair_order, um_kernels, opt.mates()), len_grid, dim3(256), 0, stream, *p, last_n, bad_name);
    else
      hipLaunchKernelGGL(TEXT_KERNEL(sam_len_kernel, pair_order, um_kernels, opt.mates()), len_grid, dim3(256), 0, stream, *p);
    TAIL_TRY(hipGetLastError());
    TAIL_TRY(scan(line_len.get(), line_off.get(), 0ull, r1, rocprim::plus<unsigned long long>(), stream));
    TAIL_TRY(hipMemcpyAsync(h_ctl + 2, ctl + 2, 4, hipMemcpyDeviceToHost, stream));
    return FEM_OK;
  }
  // after lines() and a wait for its stream: the number of lines (into p->n_records, which bounded it), n_unm
  uint32_t counted(const LineOptions &opt, SamParams *p) {
    if (filtered) {  // (what the filter kept, the unmapped reads' lines among them)
      const uint32_t n_lines = std::min(h_ctl[8], p->n_records);
      n_unm = opt.unmapped ? std::min(h_ctl[9], n_lines) : 0u;
      if (folded) n_xa = std::min(h_ctl[10], n_base_last), n_xa_slots = std::min(h_ctl[11], std::min(n_xa, n_lines));
      n_filtered = n_base_last + n_unm - n_lines - n_xa;
      p->n_records = n_lines;
    } else if (opt.unmapped) {
      const uint32_t n_lines = std::min(h_ctl[8], p->n_records);
      n_unm = n_lines - p->u_base;
      p->n_records = n_lines;
    }
    return p->n_records;
  }

  // A text's way home after stage kText: `bytes` from src into h_text (and bytes2 from src2 into dst2: SAM's qual_at) behind the
  // text that took the gate before (TextGate), ev_text its arrival; wait: until then.
  int send_home(const void *src, size_t bytes, void *dst2, const void *src2, size_t bytes2, hipStream_t stream, bool wait, TextGate *gate,
                  std::string *err) {
    TAIL_TRY(ev_text.create(hipEventDisableTiming));
    static const bool no_gate = getenv("FEM_TESTING") && getenv("FEM_TEXT_NO_GATE");  // (A/B)
    if (no_gate) gate = nullptr;
    {
      std::unique_lock<std::mutex> turn;
      if (gate) {
        turn = std::unique_lock<std::mutex>(gate->mu);
        if (gate->last && gate->last != ev_text) TAIL_TRY(hipEventSynchronize(gate->last));  // (this slot's own last text is home: its stream is in order)
      }
      // (by the copy engine.  The shader cores' stores into the pinned buffer — no engine to queue in — bring a text home in 7-9.5
      //  ms where the engine takes 5.4, and FEM map from 130 to 117 Mreads/s.)
      if (bytes) TAIL_TRY(hipMemcpyAsync(h_text, src, bytes, hipMemcpyDeviceToHost, stream));
      if (bytes2) TAIL_TRY(hipMemcpyAsync(dst2, src2, bytes2, hipMemcpyDeviceToHost, stream));
      TAIL_TRY(hipEventRecord(ev_text, stream));
      if (gate) gate->last = ev_text;
    }
    if (wait) TAIL_TRY(hipStreamSynchronize(stream));
    return FEM_OK;
  }
};

Tail::Tail() = default;  // (both out of line: Impl is incomplete in the header)
Tail::~Tail() = default;

int Tail::impl(Impl **m) {
  if (!impl_) impl_.reset(new (std::nothrow) Impl());
  *m = impl_.get();
  return impl_ ? FEM_OK : FEM_ERR_NOMEM;
}

bool Tail::coverage_queued() const { return impl_ && impl_->cov_queued; }

float Tail::stage_ms(Stage stage) const { return impl_ ? impl_->span[stage].ms() : -1.f; }

// Everything run() and sam() allocate for a batch of n reads with nr records (device arrays sized by the records, the scans'
// scratch).  run() calls it with the batch's own numbers; a caller that knows what is coming (fem_dev_reserve_batch) calls it
// during its setup: thirty allocations per slot otherwise fall into the first batches' way home.
int Tail::reserve(uint32_t n, uint32_t nr, uint32_t max_len_in, int e, bool tiny, std::string *err) {
  Impl *mp;
  if (int rc = impl(&mp)) return rc;
  Impl &m = *mp;
  const uint32_t fast_ops = std::min<uint32_t>(kOpsCap, 2u * (uint32_t)e + 2u);
  const uint32_t ops_cap = tiny ? 1u : std::max<uint32_t>(8u, fast_ops), md_cap = tiny ? 2u : kMdCap;
  (void)max_len_in;
  TAIL_TRY(m.rec_begin.ensure((size_t)n + 1));
  TAIL_TRY(m.queue.ensure(std::max<size_t>(n, 1)));
  TAIL_TRY(m.ctl.ensure(4));
  TAIL_TRY(m.h_ctl.ensure(kCtlWords));
  const size_t r1 = (size_t)nr + 1;
  TAIL_TRY(m.u_cand.ensure(r1));
  TAIL_TRY(m.u_misc.ensure(r1));
  TAIL_TRY(m.s_cand.ensure(r1));
  TAIL_TRY(m.s_misc.ensure(r1));
  TAIL_TRY(m.s_read.ensure(r1));
  TAIL_TRY(m.t_ops.ensure(r1 * ops_cap));
  TAIL_TRY(m.t_md.ensure(r1 * std::max<uint32_t>(md_cap, 12)));  // doubles as the ordering scratch (8 + 4 bytes per hit)
  TAIL_TRY(m.ovf.ensure(r1));
  TAIL_TRY(m.rec_list.ensure(r1));
  TAIL_TRY(m.src_slot.ensure(r1));
  TAIL_TRY(m.n_ops.ensure(r1));
  TAIL_TRY(m.n_md.ensure(r1));
  TAIL_TRY(m.flag.ensure(r1));
  TAIL_TRY(m.tid.ensure(r1));
  TAIL_TRY(m.pos0.ensure(r1));
  TAIL_TRY(m.nm.ensure(r1));
  TAIL_TRY(m.cigar_off.ensure(r1));
  TAIL_TRY(m.md_off.ensure(r1));
  TAIL_TRY(m.cigar.ensure(std::max<size_t>((size_t)nr * ops_cap, 1)));
  TAIL_TRY(m.md.ensure(std::max<size_t>((size_t)nr * md_cap, 1)));
  TAIL_TRY(m.line_len.ensure(r1));
  TAIL_TRY(m.line_off.ensure(r1));
  TAIL_TRY(m.qual_at.ensure((size_t)n + 1));
  TAIL_TRY(m.h_qual_at.ensure((size_t)n + 1));
  size_t need = 16;  // run()'s two scans and the text's
  TAIL_TRY(scan_need(&need, (const uint32_t *)nullptr, m.rec_begin.get(), 0u, (size_t)n, rocprim::plus<uint32_t>()));
  TAIL_TRY(m.scan_runs_md(r1, nullptr, &need));
  TAIL_TRY(scan_need(&need, m.line_len.get(), m.line_off.get(), 0ull, r1, rocprim::plus<unsigned long long>()));
  TAIL_TRY(m.scan_tmp.ensure(need));
  for (Span &s : m.span) TAIL_TRY(s.create());
  TAIL_TRY(m.ev_text.create(hipEventDisableTiming));
  return FEM_OK;
}

// The first launch of a kernel loads its code object (this file's: 12-17 ms of host time in front of the first batch's
// ordering kernels, 7 more in front of its text) and the first use of a stream creates its queue: both belong to the setup.
// Asks for every kernel's attributes (which loads the code object) and runs the three scans over one element on `stream`.
int Tail::warm(hipStream_t stream, std::string *err) {
  if (!impl_) return FEM_ERR_STATE;
  Impl &m = *impl_;
  hipFuncAttributes a;
  const void *kernels[] = {(const void *)gather_kernel, (const void *)sort_kernel, (const void *)trace_ident_kernel,
                           (const void *)trace_fast_kernel<uint8_t, NoPlane>, (const void *)trace_fast_kernel<uint16_t, NoPlane>,
                           (const void *)trace_fast_kernel<uint16_t, uint8_t>, (const void *)trace_fast_kernel<uint32_t, NoPlane>,
                           (const void *)trace_fast_kernel<uint32_t, uint8_t>, (const void *)trace_fast_kernel<uint32_t, uint16_t>,
                           (const void *)trace_kernel, (const void *)compact_kernel, (const void *)sam_len_kernel<false>,
                           (const void *)sam_write_kernel<false>, (const void *)sam_len_kernel<true>,
                           (const void *)sam_write_kernel<true>, (const void *)pair_kernel<false>, (const void *)pair_kernel<true>,
                           (const void *)mapq_kernel, (const void *)unmapped_mark_kernel, (const void *)unmapped_src_kernel,
                           (const void *)report_kernel<false>, (const void *)report_kernel<true>,
                           (const void *)sam_len_kernel<false, true>, (const void *)sam_write_kernel<false, true>,
                           (const void *)sam_len_kernel<true, true>, (const void *)sam_write_kernel<true, true>,
                           (const void *)rescue_jobs_kernel, (const void *)pair_probe_kernel,
                           (const void *)rescue_search_kernel, (const void *)rescue_trace_kernel, (const void *)rescue_append_kernel,
                           (const void *)insert_sample_kernel, (const void *)library_sample_kernel, (const void *)insert_bounds_kernel,
                           (const void *)mate_score_kernel, (const void *)sam_len_kernel<true, false, true>,
                           (const void *)sam_write_kernel<true, false, true>, (const void *)sam_len_kernel<true, true, true>,
                           (const void *)sam_write_kernel<true, true, true>, (const void *)xa_index_kernel<false>,
                           (const void *)xa_index_kernel<true>, (const void *)xa_write_kernel<false>, (const void *)xa_write_kernel<true>};
  for (const void *k : kernels) TAIL_TRY(hipFuncGetAttributes(&a, k));
  if (!m.scan_tmp || !m.rec_begin || !m.n_ops || !m.line_len) return FEM_OK;  // (nothing reserved: the scans load with the first batch)
  TAIL_TRY(hipMemsetAsync(m.n_ops, 0, 4, stream));
  TAIL_TRY(hipMemsetAsync(m.n_md, 0, 4, stream));
  TAIL_TRY(hipMemsetAsync(m.line_len, 0, 8, stream));
  TAIL_TRY(m.scan((const uint32_t *)m.n_ops.get(), m.rec_begin.get(), 0u, (size_t)1, rocprim::plus<uint32_t>(), stream));
  TAIL_TRY(m.scan_runs_md(1, stream));
  TAIL_TRY(m.scan(m.line_len.get(), m.line_off.get(), 0ull, (size_t)1, rocprim::plus<unsigned long long>(), stream));
  if (m.text && m.h_text && m.text.bytes() >= (1u << 20) && m.h_text.bytes() >= (1u << 20))
    TAIL_TRY(hipMemcpyAsync(m.h_text, m.text, 1u << 20, hipMemcpyDeviceToHost, stream));
  TAIL_TRY(hipMemcpyAsync(m.h_ctl, m.ctl, 16, hipMemcpyDeviceToHost, stream));
  TAIL_TRY(hipStreamSynchronize(stream));
  return FEM_OK;
}

int Tail::run(const TailInput &in, hipStream_t stream, int n_cu, bool tiny, TailOutput *out, std::string *err, bool copy_records) {
  Impl *mp;
  if (int rc = impl(&mp)) return rc;
  Impl &m = *mp;
  m.cov_queued = false;
  if (in.n_records > 0xFFFFFFF0ull) {
    if (err) *err = "more than 2^32 mappings in one batch; split the batch";
    return FEM_ERR_UNSUPPORTED;
  }
  const uint32_t n = in.n_reads, nr = (uint32_t)in.n_records;

  const uint32_t max_len = std::max<uint32_t>(in.max_len, 1);
  TracePlan plan;
  if (int rc = trace_plan(max_len, in.e, &plan, err)) return rc;
  const uint32_t lanes = plan.lanes;
  // first-pass kernel: one packed word per column (two fields of 2e+1 bits) + the run list
  const uint32_t hist_bytes = (2u * (2u * (uint32_t)in.e + 1u) + 7u) / 8u;  // 1, 1, 2, 2, 3, 3, 4, 4 for e = 0..7
  const uint32_t fast_ops = std::min<uint32_t>(kOpsCap, 2u * (uint32_t)in.e + 2u);  // a sane walk opens <= 2 ed + 1 runs
  const uint32_t fast_per_lane = max_len * hist_bytes + fast_ops * 2u;
  const uint32_t fast_lanes = std::min<uint32_t>(64, (64u * 1024u - 4u) / fast_per_lane);
  const uint32_t fast_lds = ((max_len * hist_bytes * fast_lanes + 3u) & ~3u) + fast_ops * 2u * fast_lanes;
  // (the staging's rows are read and written one record per lane: the shorter the row, the fewer lines a wave touches)
  const uint32_t ops_cap = tiny ? 1u : std::max<uint32_t>(8u, fast_ops), md_cap = tiny ? 2u : kMdCap;
  const OverflowCaps o_cap = overflow_caps(max_len, in.e);

  static const bool trace_host = getenv("FEM_TESTING") && getenv("FEM_FETCH_TIMES");
  const auto t_in = std::chrono::steady_clock::now();
  auto since_in = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_in).count(); };
  {
    const int rrc = reserve(n, nr, max_len, in.e, tiny, err);
    if (rrc) return rrc;
  }
  const double ms_reserved = since_in();
  const size_t r1 = (size_t)nr + 1;

  Params p{};
  p.bases = in.bases, p.read_off = in.read_off, p.n_reads = n;
  p.ref_raw = in.ref_raw, p.ref_bytes = in.ref_bytes, p.seq_off = in.seq_off;
  p.planes = in.planes;
  p.packed = in.packed, p.packed_bpr = in.packed_bpr, p.exc_bits = in.exc_bits;
  p.cand = in.cand, p.ed = in.ed, p.end = in.end, p.cand_begin = in.cand_begin, p.cand_count = in.cand_count;
  p.e = in.e, p.n_records = nr;
  p.rec_begin = m.rec_begin;
  p.u_cand = m.u_cand, p.u_misc = m.u_misc;
  p.s_cand = m.s_cand, p.s_misc = m.s_misc, p.s_read = m.s_read;
  p.queue = m.queue, p.ctl = m.ctl;
  p.g_keys = (uint64_t *)m.t_md.get();
  p.g_idx = (uint32_t *)(m.t_md + r1 * 8);
  p.lanes = lanes, p.text_words = plan.text_words, p.pat_words = plan.pat_words, p.max_len = max_len, p.fast_lanes = fast_lanes, p.fast_ops = fast_ops;
  p.t_ops = m.t_ops, p.t_md = m.t_md, p.ops_cap = ops_cap, p.md_cap = md_cap;
  p.ovf_queue = nullptr, p.ovf_out = m.ovf, p.src_slot = m.src_slot;
  p.rec_list = m.rec_list;
  p.n_ops = m.n_ops, p.n_md = m.n_md;
  p.flag = m.flag, p.tid = m.tid, p.pos0 = m.pos0, p.nm = m.nm;

  // the three stages share four events: the traceback starts where the ordering ends, the compaction where the traceback does
  Span &ordering = m.span[kOrder], &traceback = m.span[kTrace], &compaction = m.span[kCompact];
  for (Span &s : m.span) s.ran = false;
  traceback.follow(ordering), compaction.follow(traceback);
  uint32_t *h_ctl = m.h_ctl;
  TAIL_TRY(ordering.begin(stream));
  TAIL_TRY(hipMemsetAsync(m.ctl, 0, 16, stream));
  if (n) TAIL_TRY(m.scan((const uint32_t *)in.n_map, m.rec_begin.get(), 0u, (size_t)n, rocprim::plus<uint32_t>(), stream));
  TAIL_TRY(hipMemsetD32Async((hipDeviceptr_t)(m.rec_begin + n), (int)nr, 1, stream));
  uint32_t n_overflow = 0;
  if (nr) {
    hipLaunchKernelGGL(gather_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, p);
    TAIL_TRY(hipGetLastError());
    hipLaunchKernelGGL(sort_kernel, dim3((uint32_t)n_cu * 4u), dim3(64), 0, stream, p);
    TAIL_TRY(hipGetLastError());
    TAIL_TRY(ordering.end(stream));
    // zero-edit records first (no recurrence); what they leave goes through the walking kernel
    hipLaunchKernelGGL(trace_ident_kernel, dim3(std::min<uint32_t>((nr + kIdentChunk - 1u) / kIdentChunk, (uint32_t)n_cu * 8u)), dim3(256), 0, stream, p);
    TAIL_TRY(hipGetLastError());
    const uint32_t blocks = std::min<uint32_t>((nr + fast_lanes - 1) / fast_lanes, (uint32_t)n_cu * 32u);
    switch (hist_bytes) {
      case 1: hipLaunchKernelGGL((trace_fast_kernel<uint8_t, NoPlane>), dim3(blocks), dim3(64), fast_lds, stream, p); break;
      case 2: hipLaunchKernelGGL((trace_fast_kernel<uint16_t, NoPlane>), dim3(blocks), dim3(64), fast_lds, stream, p); break;
      case 3: hipLaunchKernelGGL((trace_fast_kernel<uint16_t, uint8_t>), dim3(blocks), dim3(64), fast_lds, stream, p); break;
      case 4: hipLaunchKernelGGL((trace_fast_kernel<uint32_t, NoPlane>), dim3(blocks), dim3(64), fast_lds, stream, p); break;
      case 5: hipLaunchKernelGGL((trace_fast_kernel<uint32_t, uint8_t>), dim3(blocks), dim3(64), fast_lds, stream, p); break;
      default: hipLaunchKernelGGL((trace_fast_kernel<uint32_t, uint16_t>), dim3(blocks), dim3(64), fast_lds, stream, p); break;
    }
    TAIL_TRY(hipGetLastError());
    TAIL_TRY(hipMemcpyAsync(h_ctl, m.ctl, 16, hipMemcpyDeviceToHost, stream));
    const double ms_queued = since_in();
    TAIL_TRY(hipStreamSynchronize(stream));
    if (trace_host) fprintf(stderr, "[tail] allocations %.2f ms, kernels queued %.2f, walked %.2f\n", ms_reserved, ms_queued, since_in());
    n_overflow = h_ctl[1];
    if (getenv("FEM_TESTING") && getenv("FEM_TAIL_DEBUG"))
      fprintf(stderr, "[tail] records %u, queued for ordering %u, walked %u, overflow pass %u, lanes %u/%u\n", nr, h_ctl[0], h_ctl[3], n_overflow, fast_lanes, lanes);
    if (n_overflow) {  // records whose CIGAR or MD outgrew the first staging: once more, with room for any walk
      TAIL_TRY(m.o_ops.ensure((size_t)n_overflow * o_cap.ops));
      TAIL_TRY(m.o_md.ensure((size_t)n_overflow * o_cap.md));
      Params q = p;
      q.ovf_queue = m.ovf;
      q.t_ops = m.o_ops, q.t_md = m.o_md, q.ops_cap = o_cap.ops, q.md_cap = o_cap.md;
      const uint32_t b2 = std::min<uint32_t>((n_overflow + lanes - 1) / lanes, (uint32_t)n_cu * 16u);
      hipLaunchKernelGGL(trace_kernel, dim3(b2), dim3(64), plan.lds_bytes, stream, q);
      TAIL_TRY(hipGetLastError());
    }
  } else {
    TAIL_TRY(ordering.end(stream));
  }
  TAIL_TRY(traceback.end(stream));
  // ---- compaction: offsets by exclusive scans over n_records + 1 lengths (the last one zero) ----
  TAIL_TRY(hipMemsetAsync(m.n_ops + nr, 0, 4, stream));
  TAIL_TRY(hipMemsetAsync(m.n_md + nr, 0, 4, stream));
  TAIL_TRY(m.scan_runs_md(r1, stream));
  // (the compacted arrays are sized by what the stagings can hold, so that no round trip to the host sits between the scan
  // and the kernel that uses it; the totals come back with everything else)
  TAIL_TRY(m.cigar.ensure(std::max<size_t>((size_t)nr * ops_cap + (size_t)n_overflow * o_cap.ops, 1)));
  TAIL_TRY(m.md.ensure(std::max<size_t>((size_t)nr * md_cap + (size_t)n_overflow * o_cap.md, 1)));
  if (nr) {
    CompactParams c{};
    c.n_records = nr, c.src_slot = p.src_slot, c.n_ops = p.n_ops, c.n_md = p.n_md;
    c.cigar_off = m.cigar_off, c.md_off = m.md_off;
    c.t_ops = p.t_ops, c.t_md = p.t_md, c.o_ops = m.o_ops, c.o_md = m.o_md;
    c.ops_cap = ops_cap, c.md_cap = md_cap, c.o_ops_cap = o_cap.ops, c.o_md_cap = o_cap.md;
    c.cigar = m.cigar, c.md = m.md;
    hipLaunchKernelGGL(compact_kernel, dim3((nr + 255u) / 256u), dim3(256), 0, stream, c);
    TAIL_TRY(hipGetLastError());
  }
  TAIL_TRY(compaction.end(stream));
  TAIL_TRY(hipMemcpyAsync(h_ctl + 4, m.cigar_off + nr, 4, hipMemcpyDeviceToHost, stream));
  TAIL_TRY(hipMemcpyAsync(h_ctl + 5, m.md_off + nr, 4, hipMemcpyDeviceToHost, stream));
  m.last_n = n, m.last_nr = nr, m.paired = false, m.n_resc = 0, m.pair_mapq = false;
  if (copy_records) {  // ---- copy back (else the caller renders the records on the device: sam(), bam()) ----
    TAIL_TRY(hipStreamSynchronize(stream));
    TAIL_TRY(copy_home(m.h_rec_begin, m.rec_begin, 0, (size_t)n + 1, 0, stream));
    TAIL_TRY(copy_home(m.h_cigar_off, m.cigar_off, 0, r1, 0, stream));
    TAIL_TRY(copy_home(m.h_md_off, m.md_off, 0, r1, 0, stream));
    TAIL_TRY(copy_home(m.h_flag, m.flag, 0, nr, r1, stream));
    TAIL_TRY(copy_home(m.h_tid, m.tid, 0, nr, r1, stream));
    TAIL_TRY(copy_home(m.h_pos0, m.pos0, 0, nr, r1, stream));
    TAIL_TRY(copy_home(m.h_nm, m.nm, 0, nr, r1, stream));
    TAIL_TRY(copy_home(m.h_cigar, m.cigar, 0, h_ctl[4], 1, stream));
    TAIL_TRY(copy_home(m.h_md, m.md, 0, h_ctl[5], 1, stream));
  }
  TAIL_TRY(hipMemcpyAsync(h_ctl, m.ctl, 16, hipMemcpyDeviceToHost, stream));
  TAIL_TRY(hipStreamSynchronize(stream));
  if (h_ctl[2] != 0) {
    if (err) *err = "device traceback: a record outgrew the overflow staging (internal error)";
    return FEM_ERR_HIP;
  }
  *out = TailOutput{};
  out->n_reads = n, out->n_records = nr;
  if (copy_records) {
    out->rec_begin = m.h_rec_begin;
    out->flag = m.h_flag, out->tid = m.h_tid, out->pos0 = m.h_pos0;
    out->nm = m.h_nm;
    out->cigar_off = m.h_cigar_off, out->cigar = m.h_cigar;
    out->md_off = m.h_md_off, out->md = m.h_md;
  }
  return FEM_OK;
}

int Tail::reserve_text(uint64_t bytes, std::string *err) {
  Impl *m;
  if (int rc = impl(&m)) return rc;
  TAIL_TRY(m->text.ensure((size_t)bytes));
  TAIL_TRY(m->h_text.ensure((size_t)bytes));
  return FEM_OK;
}

int Tail::wait_text() {
  if (!impl_ || !impl_->ev_text) return FEM_ERR_STATE;
  return hipEventSynchronize(impl_->ev_text) == hipSuccess ? FEM_OK : FEM_ERR_HIP;
}

int Tail::sam(const TailInput &in, const SamInput &names, const LineOptions &opt, hipStream_t stream, int n_cu, SamOutput *out,
              std::string *err, bool wait, TextGate *gate) {
  if (!impl_ || !out) return FEM_ERR_STATE;
  Impl &m = *impl_;
  SamParams p{};
  const bool hole = names.qual_hole && !names.quals;
  const size_t n_reads1 = (size_t)m.last_n + 1;
  if (hole) {  // where each read's QUAL field starts (all ones: the read has no record)
    TAIL_TRY(m.qual_at.ensure(n_reads1));
    TAIL_TRY(m.h_qual_at.ensure(n_reads1));
    TAIL_TRY(hipMemsetAsync(m.qual_at, 0xFF, n_reads1 * 8, stream));
    p.qual_at = m.qual_at, p.qual_hole = 1u;
  }
  int rc = m.lines(in, names, opt, nullptr, stream, n_cu, &p, err);
  if (rc) return rc;
  unsigned long long *h_total = (unsigned long long *)(m.h_ctl + 6);
  TAIL_TRY(hipMemcpyAsync(h_total, m.line_off + p.n_records, 8, hipMemcpyDeviceToHost, stream));
  TAIL_TRY(hipStreamSynchronize(stream));
  const uint32_t nr = m.counted(opt, &p);
  const uint64_t total = *h_total;
  TAIL_TRY(m.text.ensure(std::max<size_t>((size_t)total, 16)));
  TAIL_TRY(m.h_text.ensure(std::max<size_t>((size_t)total + total / 8, 1u << 20)));
  if (nr) {
    p.text = m.text;
    const uint32_t blocks = (nr + 255u) / 256u;  // a wave per 64 records
    hipLaunchKernelGGL(TEXT_KERNEL(sam_write_kernel, opt.paired, m.um_kernels, opt.mates()), dim3(blocks), dim3(256), 0, stream, p);
    TAIL_TRY(hipGetLastError());
    if (m.n_xa_slots) {
      hipLaunchKernelGGL(xa_write_kernel<false>, dim3((m.n_xa_slots + 3u) / 4u), dim3(256), 0, stream, p, m.xa, m.n_xa_slots);
      TAIL_TRY(hipGetLastError());
    }
  }
  TAIL_TRY(m.span[kText].end(stream));
  rc = m.send_home(m.text, (size_t)total, m.h_qual_at, m.qual_at, hole ? n_reads1 * 8 : 0, stream, wait, gate, err);
  if (rc) return rc;
  out->text = m.h_text, out->len = total, out->n_asserted = m.h_ctl[2];
  out->qual_at = hole ? m.h_qual_at : nullptr;
  return FEM_OK;
}

int Tail::bam(const TailInput &in, const SamInput &names, const LineOptions &opt, int level, hipStream_t stream, int n_cu, BamOutput *out,
              std::string *err, float *bgzf_ms, bool wait, TextGate *gate) {
  if (!impl_ || !out) return FEM_ERR_STATE;
  Impl &m = *impl_;
  if (!names.quals || names.qual_hole) {
    if (err) *err = "BAM records need the qualities on the device";
    return FEM_ERR_STATE;
  }
  TAIL_TRY(m.bam_ctl.ensure(4));
  SamParams p{};
  uint32_t *bad_name = m.bam_ctl;
  int rc = m.lines(in, names, opt, bad_name, stream, n_cu, &p, err);
  if (rc) return rc;
  const uint32_t n_bound = p.n_records;
  // the record offsets come home with the total: the member cuts are made here
  TAIL_TRY(copy_home(m.h_line_off, m.line_off, 0, (size_t)n_bound + 1, 0, stream));
  TAIL_TRY(hipMemcpyAsync(m.h_ctl + 3, bad_name, 4, hipMemcpyDeviceToHost, stream));
  TAIL_TRY(hipStreamSynchronize(stream));
  if (m.h_ctl[3]) {
    if (err) *err = "the batch holds a read name over 254 characters: not writable as BAM (l_read_name is one byte)";
    return FEM_ERR_UNSUPPORTED;
  }
  const uint32_t nr = m.counted(opt, &p);
  const uint64_t total = m.h_line_off[nr];
  TAIL_TRY(m.text.ensure(std::max<size_t>((size_t)total, 16)));
  if (nr) {
    p.text = m.text;
    hipLaunchKernelGGL(TEXT_KERNEL(bam_write_kernel, opt.paired, m.um_kernels, opt.mates()), dim3((nr + 3u) / 4u), dim3(256), 0, stream, p);
    TAIL_TRY(hipGetLastError());
    if (m.n_xa_slots) {
      hipLaunchKernelGGL(xa_write_kernel<true>, dim3((m.n_xa_slots + 3u) / 4u), dim3(256), 0, stream, p, m.xa, m.n_xa_slots);
      TAIL_TRY(hipGetLastError());
    }
  }
  TAIL_TRY(m.span[kText].end(stream));
  femz::bgzf_cut(m.h_line_off, nr, total, &m.cuts);
  uint64_t len = 0;
  // (compress() waits for the stream: the stage is over when the text sets out)
  if ((rc = m.bgzf.compress(m.text, total, m.cuts, level, stream, &len, err, bgzf_ms))) return rc;
  TAIL_TRY(m.h_text.ensure(std::max<size_t>((size_t)len, 1u << 20)));
  if ((rc = m.send_home(m.bgzf.out(), (size_t)len, nullptr, nullptr, 0, stream, wait, gate, err))) return rc;
  out->data = (uint8_t *)m.h_text.get(), out->len = len, out->raw_len = total;
  out->n_blocks = m.cuts.empty() ? 0 : m.cuts.size() - 1;
  out->n_asserted = m.h_ctl[2];
  return FEM_OK;
}

int Tail::pair(const LineOptions &opt, const RescueInput &rescue, hipStream_t stream, std::string *err) {
  if (!impl_) return FEM_ERR_STATE;
  Impl &m = *impl_;
  const uint32_t n = m.last_n, nr = m.last_nr, np = n / 2u;
  if (n & 1u) {
    if (err) *err = "a paired batch holds an even number of reads";
    return FEM_ERR_INVALID;
  }
  m.n_resc = 0, m.n_resc_disc = 0, m.pair_mapq = false;
  m.not_run({kRescue, kPairing});
  const uint32_t *resc_before = nullptr;
  if (opt.rescues() && np) {  // ---- mate rescue: the kept records behind run()'s, resc_before their exclusive scan over the pairs ----
    const int32_t E = opt.rescue_edits;
    TAIL_TRY(m.r_ctl.ensure(8));
    TAIL_TRY(m.h_r_ctl.ensure(8));
    TAIL_TRY(m.r_cand.ensure((size_t)np));
    TAIL_TRY(m.r_best.ensure((size_t)np));
    TAIL_TRY(m.r_jobs.ensure((size_t)np * kRescueAnchors * (opt.rescue_discordant ? 2u : 1u)));  // (both directions)
    if (opt.rescue_discordant) TAIL_TRY(m.r_disc.ensure((size_t)np));
    const uint32_t *h_tot = m.h_ctl;  // run() left its CIGAR and MD totals in h_ctl[4], h_ctl[5]
    RescueParams r{};
    r.n_pairs = np, r.n_records = nr, r.E = E, r.min_insert = opt.min_insert, r.max_insert = opt.max_insert;
    r.bases = rescue.bases, r.read_off = rescue.read_off, r.ref_raw = rescue.ref_raw, r.ref_bytes = rescue.ref_bytes;
    r.seq_off = rescue.seq_off, r.seq_len = rescue.seq_len;
    r.ctl = m.r_ctl, r.cand_pair = m.r_cand, r.jobs = m.r_jobs;
    r.best = m.r_best;
    r.cig_total = h_tot[4], r.md_total = h_tot[5];
    r.flip1 = opt.flip1(), r.flip2 = opt.flip2();
    m.bind_records(&r);
    TAIL_TRY(m.span[kRescue].begin(stream));
    TAIL_TRY(hipMemsetAsync(m.r_ctl, 0, 32, stream));
    if (opt.rescue_discordant) {  // the pairs with records on both sides that do not pair are candidates too
      PairParams q{};
      q.n_pairs = np, q.min_insert = opt.min_insert, q.max_insert = opt.max_insert;
      q.flip1 = opt.flip1(), q.flip2 = opt.flip2();
      m.bind_pairing(&q);
      hipLaunchKernelGGL(pair_probe_kernel, dim3((np + 255u) / 256u), dim3(256), 0, stream, q, m.r_disc.get());
      TAIL_TRY(hipGetLastError());
      r.disc = m.r_disc;
    }
    hipLaunchKernelGGL(rescue_jobs_kernel, dim3((np + 255u) / 256u), dim3(256), 0, stream, r);
    TAIL_TRY(hipGetLastError());
    uint32_t *h_rc = m.h_r_ctl;
    TAIL_TRY(hipMemcpyAsync(h_rc, m.r_ctl, 8, hipMemcpyDeviceToHost, stream));
    TAIL_TRY(hipStreamSynchronize(stream));
    const uint32_t n_cand = h_rc[0], n_jobs = h_rc[1];
    if (n_cand) {
      // first pass: the staging of a walk of E errors on canonical characters (<= 2E + 2 runs; MD <= 2E + 1 numbers of <= 4
      // digits and 3E characters); overflow pass: the longest walk, as trace_kernel's (every column an MD character)
      r.max_len = std::max<uint32_t>(rescue.max_len, 1);
      TracePlan plan;  // (trace_kernel's, at E)
      if (int rc = trace_plan(r.max_len, E, &plan, err)) return rc;
      const OverflowCaps o_cap = overflow_caps(r.max_len, E);
      r.text_words = plan.text_words, r.pat_words = plan.pat_words, r.lanes = plan.lanes;
      r.ops_cap = 2u * (uint32_t)E + 8u, r.md_cap = 8u * (uint32_t)E + 64u;
      r.o_ops_cap = o_cap.ops, r.o_md_cap = o_cap.md;
      const size_t rec_cap = (size_t)nr + n_cand + 1;
      TAIL_TRY(m.flag.ensure_keep(rec_cap, (size_t)nr, stream));
      TAIL_TRY(m.tid.ensure_keep(rec_cap, (size_t)nr, stream));
      TAIL_TRY(m.pos0.ensure_keep(rec_cap, (size_t)nr, stream));
      TAIL_TRY(m.nm.ensure_keep(rec_cap, nr, stream));
      TAIL_TRY(m.s_read.ensure_keep(rec_cap, (size_t)nr, stream));
      TAIL_TRY(m.cigar_off.ensure_keep(rec_cap, (size_t)nr + 1, stream));
      TAIL_TRY(m.md_off.ensure_keep(rec_cap, (size_t)nr + 1, stream));
      m.bind_records(&r);
      TAIL_TRY(m.r_ops.ensure((size_t)n_cand * r.ops_cap));
      TAIL_TRY(m.r_md.ensure((size_t)n_cand * r.md_cap));
      TAIL_TRY(m.r_rec.ensure((size_t)n_cand * kRescRec));
      TAIL_TRY(m.r_ovf.ensure((size_t)n_cand));
      r.ovf_queue = m.r_ovf;
      const size_t p1 = (size_t)np + 1;
      TAIL_TRY(m.r_kept.ensure(p1 * 3));
      TAIL_TRY(m.r_scan.ensure(p1 * 3));
      r.t_ops = m.r_ops, r.t_md = m.r_md, r.c_rec = m.r_rec;
      r.kept = m.r_kept, r.k_ops = r.kept + p1, r.k_md = r.kept + 2 * p1;
      r.s_kept = m.r_scan, r.s_ops = r.s_kept + p1, r.s_md = r.s_kept + 2 * p1;
      TAIL_TRY(hipMemsetAsync(m.r_kept, 0, p1 * 12, stream));
      if (n_jobs) {
        const uint32_t blocks = std::min<uint32_t>((n_jobs + kResWaves - 1u) / kResWaves, 16384u);
        hipLaunchKernelGGL(rescue_search_kernel, dim3(blocks), dim3(64 * kResWaves), 0, stream, r);
        TAIL_TRY(hipGetLastError());
      }
      const uint32_t t_blocks = std::min<uint32_t>((n_cand + r.lanes - 1u) / r.lanes, 16384u);
      r.overflow_pass = 0;
      hipLaunchKernelGGL(rescue_trace_kernel, dim3(t_blocks), dim3(64), plan.lds_bytes, stream, r);
      TAIL_TRY(hipGetLastError());
      TAIL_TRY(hipMemcpyAsync(h_rc + 2, m.r_ctl + 2, 4, hipMemcpyDeviceToHost, stream));
      TAIL_TRY(hipStreamSynchronize(stream));
      const uint32_t n_ovf = h_rc[2];
      if (n_ovf) {  // the records that outgrew the first staging, again with room for the longest walk
        TAIL_TRY(m.r_o_ops.ensure((size_t)n_ovf * r.o_ops_cap));
        TAIL_TRY(m.r_o_md.ensure((size_t)n_ovf * r.o_md_cap));
        r.o_ops = m.r_o_ops, r.o_md = m.r_o_md, r.overflow_pass = 1;
        const uint32_t o_blocks = std::min<uint32_t>((n_ovf + r.lanes - 1u) / r.lanes, 16384u);
        hipLaunchKernelGGL(rescue_trace_kernel, dim3(o_blocks), dim3(64), plan.lds_bytes, stream, r);
        TAIL_TRY(hipGetLastError());
      }
      // the kept records' CIGAR runs and MD characters fit what their stagings can hold
      TAIL_TRY(m.cigar.ensure_keep((size_t)r.cig_total + (size_t)n_cand * r.ops_cap + (size_t)n_ovf * r.o_ops_cap, (size_t)r.cig_total, stream));
      TAIL_TRY(m.md.ensure_keep((size_t)r.md_total + (size_t)n_cand * r.md_cap + (size_t)n_ovf * r.o_md_cap, r.md_total, stream));
      m.bind_records(&r);
      TAIL_TRY(m.scan_kept(p1, stream));
      hipLaunchKernelGGL(rescue_append_kernel, dim3((n_cand + 255u) / 256u), dim3(256), 0, stream, r);
      TAIL_TRY(hipGetLastError());
      TAIL_TRY(hipMemcpyAsync(h_rc, m.r_scan + np, 4, hipMemcpyDeviceToHost, stream));
      TAIL_TRY(hipMemcpyAsync(h_rc + 3, m.r_ctl + 3, 8, hipMemcpyDeviceToHost, stream));
      TAIL_TRY(hipStreamSynchronize(stream));
      if (h_rc[3] != 0) {
        if (err) *err = "mate rescue: a traceback outgrew its staging (internal error)";
        return FEM_ERR_HIP;
      }
      m.n_resc = h_rc[0], m.n_resc_disc = h_rc[4];
      if (m.n_resc) resc_before = m.r_scan;
    }
    TAIL_TRY(m.span[kRescue].end(stream));
  }
  const size_t lines = std::max<size_t>((size_t)nr + m.n_resc, 1);
  TAIL_TRY(m.perm.ensure(lines));
  TAIL_TRY(m.pflag.ensure(lines));
  TAIL_TRY(m.mtid.ensure(lines));
  TAIL_TRY(m.mpos0.ensure(lines));
  TAIL_TRY(m.tlen.ensure(lines));
  if (opt.mapq) TAIL_TRY(m.lmq.ensure(lines));
  TAIL_TRY(m.pair_begin.ensure((size_t)n + 1));
  TAIL_TRY(m.pair_ctl.ensure(4));
  TAIL_TRY(m.h_pair_ctl.ensure(4));
  TAIL_TRY(m.span[kPairing].begin(stream));
  TAIL_TRY(hipMemsetAsync(m.pair_ctl, 0, 16, stream));
  if (np) {
    PairParams q{};
    q.n_pairs = np, q.min_insert = opt.min_insert, q.max_insert = opt.max_insert;
    q.flip1 = opt.flip1(), q.flip2 = opt.flip2();
    m.bind_pairing(&q);
    q.perm = m.perm, q.pflag = m.pflag, q.mtid = m.mtid, q.mpos0 = m.mpos0;
    q.tlen = m.tlen, q.pair_begin = m.pair_begin, q.n_proper = m.pair_ctl;
    q.resc_before = resc_before, q.resc_first = nr, q.s_read = m.s_read;
    q.lmq = opt.mapq ? m.lmq : nullptr;
    hipLaunchKernelGGL(opt.mapq ? pair_kernel<true> : pair_kernel<false>, dim3((np + 255u) / 256u), dim3(256), 0, stream, q);
    TAIL_TRY(hipGetLastError());
  } else {
    TAIL_TRY(hipMemsetAsync(m.pair_begin, 0, 4, stream));
  }
  TAIL_TRY(m.span[kPairing].end(stream));
  TAIL_TRY(hipMemcpyAsync(m.h_pair_ctl, m.pair_ctl, 4, hipMemcpyDeviceToHost, stream));
  m.paired = true, m.pair_mapq = opt.mapq;
  return FEM_OK;
}

// The estimate a control block holds (insert_bounds_kernel's words, at home)
static void insert_estimate_of(const uint32_t *h, uint32_t np, InsertEstimate *out) {
  out->n_pairs = np, out->n_unique = h[0], out->n_informative = h[1];
  out->q25 = (int32_t)h[2], out->q50 = (int32_t)h[3], out->q75 = (int32_t)h[4];
  out->min_insert = (int32_t)h[5], out->max_insert = (int32_t)h[6], out->estimated = h[7] != 0;
}

// n_hist = 1: estimate_insert() under the orientation of `opt`; kOrientations: estimate_library(), all three side by side
int Tail::estimate(const LineOptions *opt, uint32_t n_hist, hipStream_t stream, InsertEstimate *out, std::string *err) {
  if (!impl_ || !out) return FEM_ERR_STATE;
  Impl &m = *impl_;
  const uint32_t n = m.last_n, np = n / 2u;
  if (n & 1u) {
    if (err) *err = "a paired batch holds an even number of reads";
    return FEM_ERR_INVALID;
  }
  const size_t words = (size_t)n_hist * (kInsertBins + kInsertCtl);
  TAIL_TRY(m.ins_hist.ensure(words));
  TAIL_TRY(m.h_ctl.ensure(kCtlWords));
  uint32_t *hist = m.ins_hist, *ctl = hist + (size_t)n_hist * kInsertBins;
  m.not_run({kInsert});
  TAIL_TRY(m.span[kInsert].begin(stream));
  TAIL_TRY(hipMemsetAsync(hist, 0, words * sizeof(uint32_t), stream));
  if (np) {
    PairParams q{};
    q.n_pairs = np, q.min_insert = 0, q.max_insert = FEM_INSERT_MAX;
    if (opt) q.flip1 = opt->flip1(), q.flip2 = opt->flip2();
    m.bind_pairing(&q);
    hipLaunchKernelGGL(opt ? insert_sample_kernel : library_sample_kernel, dim3((np + 255u) / 256u), dim3(256), 0, stream, q, hist, ctl);
    TAIL_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(insert_bounds_kernel, dim3(n_hist), dim3(256), 0, stream, (const uint32_t *)hist, ctl);
  TAIL_TRY(hipGetLastError());
  TAIL_TRY(m.span[kInsert].end(stream));
  const uint32_t *h = m.h_ctl + kCtlInsert;
  TAIL_TRY(hipMemcpyAsync(m.h_ctl + kCtlInsert, ctl, (size_t)n_hist * kInsertCtl * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  TAIL_TRY(hipStreamSynchronize(stream));
  for (uint32_t o = 0; o < n_hist; ++o) insert_estimate_of(h + o * kInsertCtl, np, out + o);
  return FEM_OK;
}

int Tail::estimate_insert(const LineOptions &opt, hipStream_t stream, InsertEstimate *out, std::string *err) {
  return estimate(&opt, 1, stream, out, err);
}

int Tail::estimate_library(hipStream_t stream, LibraryEstimate *out, std::string *err) {
  if (!out) return FEM_ERR_STATE;
  if (int rc = estimate(nullptr, kOrientations, stream, out->by, err)) return rc;
  // the choice, from the 24 control words: the most informative pairs among the estimated ones, ties in the order FR RF FF
  out->orientation = -1;
  for (uint32_t o = 0; o < kOrientations; ++o)
    if (out->by[o].estimated && (out->orientation < 0 || out->by[o].n_informative > out->by[out->orientation].n_informative))
      out->orientation = (int32_t)o;
  return FEM_OK;
}

LineCounts Tail::counts() const {
  LineCounts c;
  if (!impl_) return c;
  const Impl &m = *impl_;
  if (m.paired) c.n_proper = m.h_pair_ctl ? m.h_pair_ctl[0] : 0, c.n_rescued = m.n_resc, c.n_rescued_discordant = m.n_resc_disc;
  c.n_unmapped = m.n_unm, c.n_filtered = m.n_filtered, c.n_xa = m.n_xa;
  return c;
}

int Tail::pair_fetch(hipStream_t stream, PairOutput *out, std::string *err) {
  if (!impl_ || !impl_->paired || !out) return FEM_ERR_STATE;
  Impl &m = *impl_;
  const uint32_t n = m.last_n, nr = m.last_nr + m.n_resc;  // (lines)
  TAIL_TRY(copy_home(m.h_perm, m.perm, 0, nr, 1, stream));
  TAIL_TRY(copy_home(m.h_pflag, m.pflag, 0, nr, 1, stream));
  TAIL_TRY(copy_home(m.h_mtid, m.mtid, 0, nr, 1, stream));
  TAIL_TRY(copy_home(m.h_mpos0, m.mpos0, 0, nr, 1, stream));
  TAIL_TRY(copy_home(m.h_tlen, m.tlen, 0, nr, 1, stream));
  TAIL_TRY(copy_home(m.h_pair_begin, m.pair_begin, 0, (size_t)n + 1, 0, stream));
  // the rescued records (records last_nr .. last_nr + n_resc - 1), their offsets as they stand (from run()'s totals on)
  const uint32_t k = m.n_resc, first = m.last_nr;
  const size_t k1 = k ? (size_t)k + 1 : 0;
  TAIL_TRY(copy_home(m.h_r_flag, m.flag, first, k, 1, stream));
  TAIL_TRY(copy_home(m.h_r_tid, m.tid, first, k, 1, stream));
  TAIL_TRY(copy_home(m.h_r_pos0, m.pos0, first, k, 1, stream));
  TAIL_TRY(copy_home(m.h_r_nm, m.nm, first, k, 1, stream));
  TAIL_TRY(copy_home(m.h_r_cigar_off, m.cigar_off, first, k1, 1, stream));
  TAIL_TRY(copy_home(m.h_r_md_off, m.md_off, first, k1, 1, stream));
  TAIL_TRY(hipStreamSynchronize(stream));
  const uint32_t *co = m.h_r_cigar_off, *mo = m.h_r_md_off;
  const size_t n_cig = k ? co[k] - co[0] : 0, n_md = k ? mo[k] - mo[0] : 0;
  TAIL_TRY(copy_home(m.h_r_cigar, m.cigar, k ? co[0] : 0, n_cig, 1, stream));
  TAIL_TRY(copy_home(m.h_r_md, m.md, k ? mo[0] : 0, n_md, 1, stream));
  if (n_cig || n_md) TAIL_TRY(hipStreamSynchronize(stream));
  out->n_pairs = n / 2u, out->n_records = nr, out->n_proper = m.h_pair_ctl[0];
  out->pair_begin = m.h_pair_begin, out->perm = m.h_perm, out->flag = m.h_pflag;
  out->mate_tid = m.h_mtid, out->mate_pos0 = m.h_mpos0, out->tlen = m.h_tlen;
  out->first_rescued = first, out->n_rescued = k;
  out->r_flag = m.h_r_flag, out->r_tid = m.h_r_tid, out->r_pos0 = m.h_r_pos0;
  out->r_nm = m.h_r_nm, out->r_cigar_off = co, out->r_cigar = m.h_r_cigar;
  out->r_md_off = mo, out->r_md = m.h_r_md;
  return FEM_OK;
}

#undef TEXT_KERNEL

}  // namespace femt
