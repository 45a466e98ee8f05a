// fem_verify.hip.h — verification, one lane per candidate (src/align.c:4-51, 102-277): verify_kernel (the read's characters,
// staged in LDS) and verify_kernel_packed (its 2-bit codes, fem_pack.h).  They differ in where the read's side comes from; the
// planes' windows, the character step, the outcome and the block sums are defined once.
#pragma once
#include "fem_kernels.hip.h"

namespace femk {

struct VerifyParams {
  const uint8_t *bases;       // 16 bytes of padding in front of the batch's characters, 64 behind
  const uint64_t *read_off;
  const uint8_t *planes;      // bit planes of the base codes 0..4, all sequences concatenated (plane_window; see verify_kernel)
  const uint64_t *seq_off;
  const uint64_t *cand;
  const uint32_t *cand_meta;
  const uint32_t *ctr;    // [0] = candidate slots handed out by the seed kernels, [1] = overflow flags
  uint32_t cand_cap;
  int32_t e;
  uint8_t *ed;
  int16_t *end;
  // MappingStats (src/map.c:37,48,51): accepted candidates per read (zeroed by the launcher), their sum and the reads
  // with at least one -> stats[2], stats[3]
  uint32_t *n_map;
  unsigned long long *stats;
  // verify_kernel_packed only: the batch's 2-bit codes (fem_pack.h; read r at packed + r * bpr, at least 16 bytes of padding
  // in front of read 0 and 64 behind the last), bit r of exc_bits: read r holds a character other than "ACGT" (its codes
  // are not the whole truth: its lanes take the characters), and the length every read of the batch has
  const uint8_t *packed;
  const uint32_t *exc_bits;
  uint32_t bpr, len;
};

__device__ __forceinline__ uint4 load_u128_unaligned(const uint8_t *p) {
  uint4 w;
  __builtin_memcpy(&w, p, 16);
  return w;
}

__device__ __forceinline__ uint4 plane_window(const uint8_t *planes, int q, uint64_t at) {  // fem_planes.hip.h
  return load_u128_unaligned(plane_addr(planes, q, at));
}

// ---------------------------------------------------------------------------------------------------------
// verify_candidates (src/align.c:4-51): one lane per candidate walks banded_edit_distance (src/align.c:102-147; the
// 16-bit SSE form of :149-277 differs only in the word width, `wm`).
// The kernel is bound by the number of divergent load instructions (every lane walks its own read and window), so
// both sides are fetched in the widest units that hold them:
//   * reference: three bit planes of the base codes (bit q of code(ref[i]) at bit i of plane q).  One unaligned
//     16-byte load per plane covers the windows of six 16-column steps; Peq[c] for a column is a three-way XNOR of
//     the planes, shifted;
//   * read: 16 characters per load, four loads back to back into the lane's LDS words (they share 64-byte sectors;
//     one load per step missed the L1 every time), decoded four at a time (SWAR), byte-reversed and complemented on
//     the reverse strand (prepare_negative_sequence_at, src/sequence_batch.h:90-98).
// MappingStats (src/map.c:37,48,51): an accepted candidate adds one to its read's n_map — the lane that finds it at zero
// counts the read as mapped — and a block adds its sums to the two counters once (round 1's returning atomics on the two
// COUNTERS, same address for every lane, had cost as much as the rest of the kernel; a separate count_mappings_kernel did
// it until round 3, 0.07 ms between one batch's join and the next's).
// ---------------------------------------------------------------------------------------------------------
struct MyersState {
  uint32_t VP, VN;
  int score;
};

// char -> 2-bit code for four bases at once: code per byte 0..3 (0 where the base is not A/C/G/T), nflag per byte 0/1
__device__ __forceinline__ void decode4(uint32_t chars, uint32_t complement, uint32_t &code, uint32_t &nflag) {
  const uint32_t t = (chars >> 1) & 0x03030303u;    // A 0, C 1, G 3, T 2
  const uint32_t c = t ^ ((t >> 1) & 0x01010101u);  // A 0, C 1, G 2, T 3
  const uint32_t upper = chars & 0xDFDFDFDFu;
  const uint32_t expect = __builtin_amdgcn_perm(0u, 0x54474341u /* "ACGT" */, c);
  const uint32_t z = upper ^ expect;  // zero byte <=> one of ACGT in either case (src/utils.h:72)
  nflag = ((((z & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | z) >> 7) & 0x01010101u;
  code = (c ^ complement) & ~(nflag * 3u);  // complement = 0x03030303 on the reverse strand (3 - code); N stays N
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

// The three planes' windows of one candidate whose pattern[0] is base `pat`: the stretch being consumed and the one
// requested behind it (loads of the next stretch are issued one stretch ahead).
struct PlaneCursor {
  const uint8_t *planes;
  uint64_t pat;
  int n_steps;
  uint4 P0, P1, P2, P0n, P1n, P2n;

  __device__ __forceinline__ void request(int col) {
    P0n = plane_window(planes, 0, (pat + (uint32_t)col) >> 3), P1n = plane_window(planes, 1, (pat + (uint32_t)col) >> 3);
    P2n = plane_window(planes, 2, (pat + (uint32_t)col) >> 3);
  }
  __device__ __forceinline__ void start(const uint8_t *planes_, uint64_t pat_, int n_steps_) {
    planes = planes_, pat = pat_, n_steps = n_steps_;
    P0 = make_uint4(0, 0, 0, 0), P1 = P0, P2 = P0, P0n = P0, P1n = P0, P2n = P0;
    if (n_steps > 0) request(0);
  }
  // window of step `step`: pattern[col .. col + 16 + 2e) of col = 16 step, bit j <-> pattern[col + j];
  // (pat + 96 k) & 7 == pat & 7
  __device__ __forceinline__ void step(int step, uint32_t &b0, uint32_t &b1, uint32_t &b2) {
    if (step % kStepsPerPlaneLoad == 0) {
      P0 = P0n, P1 = P1n, P2 = P2n;
      if (step + kStepsPerPlaneLoad < n_steps) request(16 * (step + kStepsPerPlaneLoad));
    } else {
      window_advance16(P0), window_advance16(P1), window_advance16(P2);
    }
    const uint32_t pat_bit = (uint32_t)pat & 7u;
    b0 = window_head(P0, pat_bit), b1 = window_head(P1, pat_bit), b2 = window_head(P2, pat_bit);
  }
};

// One column (src/align.c:118-133).  B0..B2: the step's plane windows; m0..m2: the read base's code bits as masks;
// j = column inside the step.
__device__ __forceinline__ void myers_column(MyersState &m, uint32_t B0, uint32_t B1, uint32_t B2, uint32_t m0, uint32_t m1,
                                             uint32_t m2, uint32_t j, uint32_t width, uint32_t wm) {
  const uint32_t eq = __builtin_amdgcn_ubfe(~((B0 ^ m0) | (B1 ^ m1) | (B2 ^ m2)), j, width);  // Peq[text[col]] over the band
  uint32_t X = eq | m.VN;
  const uint32_t D0 = ((((X & m.VP) + m.VP) ^ m.VP) | X) & wm;
  const uint32_t HN = m.VP & D0;
  const uint32_t HP = (m.VN | ~(m.VP | D0)) & wm;
  X = D0 >> 1;
  m.VN = X & HP;
  m.VP = (HN | ~(X | HP)) & wm;
  m.score += 1 - (int)(D0 & 1u);
}

// The score along the band's lowest diagonal never decreases, so testing the early-reject threshold
// (src/align.c:128-130) once per step rejects exactly the candidates a per-column test would.
__device__ __forceinline__ bool past_threshold(const MyersState &m, int e) { return m.score > 3 * e; }

// The 16 characters of the step at column `col` of the read at `rd`: the reverse strand's chunk comes from the far end;
// the last, partial one may start in front of the read.
__device__ __forceinline__ uint4 text_chunk(const uint8_t *rd, uint32_t strand, int L, int col) {
  return load_u128_unaligned(strand == 0 ? rd + col : rd + (L - 16 - col));
}

// One step from the read's characters.  r: text_chunk of the step; left: L - col, the columns the read still has
// (sixteen of them unrolled, or the up-to-fifteen trailing ones); b0..b2: the step's plane windows.  The unrolled form
// decodes each word in front of its four columns: with all four decoded first, the exception path of verify_kernel_packed
// spilled two registers beside the cursor's look-ahead (80 registers at six waves per SIMD).
__device__ __forceinline__ void char_step(MyersState &m, const uint4 &r, uint32_t strand, int left, uint32_t b0, uint32_t b1, uint32_t b2,
                                          uint32_t width, uint32_t wm) {
  const uint32_t complement = strand ? 0x03030303u : 0u;
  const uint32_t w[4] = {strand ? __builtin_bswap32(r.w) : r.x, strand ? __builtin_bswap32(r.z) : r.y, strand ? __builtin_bswap32(r.y) : r.z,
                         strand ? __builtin_bswap32(r.x) : r.w};
  if (left >= 16) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      uint32_t cw, nw;
      decode4(w[k], complement, cw, nw);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint32_t m0 = (uint32_t)__builtin_amdgcn_sbfe((int)cw, 8 * q, 1), m1 = (uint32_t)__builtin_amdgcn_sbfe((int)cw, 8 * q + 1, 1);
        const uint32_t m2 = (uint32_t)__builtin_amdgcn_sbfe((int)nw, 8 * q, 1);
        myers_column(m, b0, b1, b2, m0, m1, m2, (uint32_t)(4 * k + q), width, wm);
      }
    }
  } else {  // up to fifteen trailing columns
    uint32_t cw[4], nw[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) decode4(w[k], complement, cw[k], nw[k]);
    const uint64_t clo = ((uint64_t)cw[1] << 32) | cw[0], chi = ((uint64_t)cw[3] << 32) | cw[2];
    const uint64_t nlo = ((uint64_t)nw[1] << 32) | nw[0], nhi = ((uint64_t)nw[3] << 32) | nw[2];
    for (int q = 0; q < left; ++q) {
      const uint32_t cb = (uint32_t)((q < 8 ? clo : chi) >> (8 * (q & 7)));
      const uint32_t nb = (uint32_t)((q < 8 ? nlo : nhi) >> (8 * (q & 7)));
      myers_column(m, b0, b1, b2, 0u - (cb & 1u), 0u - ((cb >> 1) & 1u), 0u - (nb & 1u), (uint32_t)q, width, wm);
    }
  }
}

// padding slot of the candidate arrays (kInvalidMeta)
__device__ __forceinline__ void store_invalid(const VerifyParams &p, uint32_t slot) { p.ed[slot] = 0xFF, p.end[slot] = 0; }

// What became of the candidate in `slot`: its ed / end, and its read's n_map.
struct Outcome {
  bool accepted;  // the candidate is a mapping
  bool mapped;    // ... and this lane found its read's n_map at zero: the read became mapped
};
__device__ __forceinline__ Outcome verify_outcome(const VerifyParams &p, const MyersState &m, bool rejected, int L, int e, uint32_t slot,
                                                  uint32_t read) {
  int score = m.score;
  int best = score, endp = L - 1;
  if (!rejected) {
    for (int j = 0; j < 2 * e; ++j) {  // first strict minimum (src/align.c:135-146)
      score += (int)((m.VP >> j) & 1u) - (int)((m.VN >> j) & 1u);
      if (score < best) {
        best = score;
        endp = L + j;
      }
    }
  }
  const bool accepted = !rejected && best <= e;
  p.ed[slot] = accepted ? (uint8_t)best : (uint8_t)0xFF;
  p.end[slot] = accepted ? (int16_t)endp : (int16_t)0;
  // The read's first accepted candidate (whichever atomic comes first) counts the read as mapped.  Neighbouring lanes that
  // accepted candidates of the SAME read add their count with one atomic (round 5): a read inside a repeat has a thousand
  // candidates in a row, and a thousand atomics on one address come one after the other (~10 ns each) — on the repeat-rich
  // 3 Gbp reference that was 7.4 of the kernel's 16.3 ms per 2.5 M reads.  Where every read has one candidate (C2, C3)
  // every lane is its own head and nothing changes but a shuffle and two ballots.
  const uint32_t ln = lane_id();
  const uint64_t acc = __ballot(accepted);
  const uint32_t prev_read = __shfl_up(read, 1);
  const bool joins_prev = accepted && ln > 0u && ((acc >> (ln - 1u)) & 1ull) && prev_read == read;
  const uint64_t heads = __ballot(accepted && !joins_prev);
  bool mapped = false;
  if (accepted && !joins_prev) {
    const uint64_t stop = (heads | ~acc) >> ln >> 1;  // the next head, or the next lane that accepted nothing
    const uint32_t run = stop ? (uint32_t)__builtin_ctzll(stop) + 1u : 64u - ln;
    mapped = atomicAdd(&p.n_map[read], run) == 0u;
  }
  return Outcome{accepted, mapped};
}

// The lanes' counts of mappings and of reads that became mapped -> stats[2], stats[3]: one pair of atomics per block
// (same-address atomics complete at ~10 ns each: a pair per wave had cost more than the verification itself,
// DESIGN.md 4.4).  part: 32 bytes of LDS nobody else is using.
__device__ __forceinline__ void block_sums(const VerifyParams &p, uint32_t (*part)[4], uint32_t mappings, uint32_t mapped) {
  for (int d = 32; d >= 1; d >>= 1) mappings += __shfl_xor(mappings, d), mapped += __shfl_xor(mapped, d);
  if (lane_id() == 0) part[0][threadIdx.x >> 6] = mappings, part[1][threadIdx.x >> 6] = mapped;
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t a = part[0][0] + part[0][1] + part[0][2] + part[0][3], b = part[1][0] + part[1][1] + part[1][2] + part[1][3];
    if (a) atomicAdd(&p.stats[2], (unsigned long long)a);
    if (b) atomicAdd(&p.stats[3], (unsigned long long)b);
  }
}

__global__ void __launch_bounds__(256) verify_kernel(VerifyParams p) {
  // a scratch buffer overflowed while seeding: slots may be unwritten, the host grows the buffer and re-runs the batch
  if (p.ctr[1] != 0) return;
  const uint32_t total = min(p.ctr[0], p.cand_cap);
  const uint32_t stride = gridDim.x * blockDim.x;
  const int e = p.e;
  const uint32_t width = 2u * (uint32_t)e + 1u;
  // Four 16-character chunks of the lane's read wait in LDS: fetched back to back they share their 64-byte sectors,
  // fetched one per step (16 columns = microseconds apart at eight waves per SIMD) every chunk missed the L1 again
  // (1.26 -> 1.14 ms at C2).  Eight chunks at once cost three waves per SIMD and were slower.
  constexpr int kStageChunks = 4;
  // (16 KB exactly, the block sums laid over it at the end)
  __shared__ uint4 stage[kStageChunks][256];
  uint32_t mappings = 0, mapped = 0;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const uint32_t meta = p.cand_meta[i];
    if (meta == kInvalidMeta) {
      store_invalid(p, i);
      continue;
    }
    const uint32_t read = (meta & ~kMeta16) >> 1, strand = meta & 1u;
    const uint32_t wm = (meta & kMeta16) ? 0xFFFFu : 0xFFFFFFFFu;
    const uint64_t c = p.cand[i];
    const uint64_t pat = p.seq_off[(uint32_t)(c >> 32)] + (uint32_t)c;  // base index of pattern[0]
    const uint64_t off = p.read_off[read];
    const int L = (int)(p.read_off[read + 1] - off);
    const uint8_t *rd = p.bases + off;
    MyersState m{0, 0, 0};
    bool rejected = false;
    const int n_steps = (L + 15) >> 4;
    PlaneCursor planes;
    planes.start(p.planes, pat, n_steps);
    for (int step = 0; step < n_steps && !rejected; ++step) {
      const int col = step << 4;
      if (step % kStageChunks == 0) {
        uint4 t4[kStageChunks];
#pragma unroll
        for (int c = 0; c < kStageChunks; ++c) t4[c] = step + c < n_steps ? text_chunk(rd, strand, L, col + 16 * c) : make_uint4(0, 0, 0, 0);
#pragma unroll
        for (int c = 0; c < kStageChunks; ++c) stage[c][threadIdx.x] = t4[c];
      }
      const uint4 r = stage[step % kStageChunks][threadIdx.x];
      uint32_t b0, b1, b2;
      planes.step(step, b0, b1, b2);
      char_step(m, r, strand, L - col, b0, b1, b2, width, wm);
      rejected = past_threshold(m, e);
    }
    const Outcome o = verify_outcome(p, m, rejected, L, e, i, read);
    mappings += o.accepted, mapped += o.mapped;
  }
  __syncthreads();  // (every wave is through with its staged chunks)
  block_sums(p, (uint32_t(*)[4]) & stage[0][0], mappings, mapped);
}

// ---------------------------------------------------------------------------------------------------------
// verify_kernel_packed: verify_kernel for a batch that came packed (equal-length reads at two bits per base, fem_pack.h).
// Same planes, same column, same outcome byte for byte; what differs is the read's side:
//   * the codes come straight out of the packed words — no characters, no decode4: one 16-byte load holds 64 columns and
//     waits in registers (no LDS staging), the next stretch's load is issued one stretch ahead as the planes' are.  On the
//     reverse strand column c is the complement of base L - 1 - c: the 128 bits that hold bases [L - 64 - col, L - col) —
//     a dword more and a funnel shift where L is no multiple of four — with their sixteen-base words and the fields inside
//     them in reverse order.  The last, partial stretch reaches up to 16 bytes in front of the read (of read 0: into the
//     buffer's front padding); nothing of that is consumed;
//   * a read with anything but upper-case ACGT (its bit in exc_bits) takes its characters from `bases`, sixteen per
//     load and step, on a path of its own: rare, it only has to be right;
//   * every read has p.len bases: no gathers from read_off;
//   * the next candidate's meta and position are requested before the current one's columns are walked, its sequence
//     offset and exception word behind them.
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t reverse_fields2(uint32_t x) {  // the sixteen 2-bit fields in reverse order
  x = __builtin_bitreverse32(x);
  return ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
}

constexpr int kStepsPerTextLoad = 4;  // 16 bytes of codes = 64 columns

// The candidate's columns from the packed codes.  row: the read's first packed byte.  Returns whether it was rejected.
__device__ __forceinline__ bool verify_walk_packed(const VerifyParams &p, MyersState &m, const uint8_t *row, uint32_t strand, uint64_t pat,
                                                   int L, int e, uint32_t width, uint32_t wm) {
  const int n_steps = (L + 15) >> 4;
  bool rejected = false;
  // bases [L - 64 - col, L - col) start at bit 2 * (L & 3) of their first byte (col is a multiple of 64); floor division:
  // the last stretch starts in front of the read
  const uint32_t sh = strand ? 2u * ((uint32_t)L & 3u) : 0u;
  auto text_addr = [&](int col) { return strand == 0 ? row + (col >> 2) : row + ((L - 64 - col) >> 2); };
  uint4 T = make_uint4(0, 0, 0, 0), Tn = T;
  uint32_t Tn4 = 0;
  if (n_steps > 0) {
    const uint8_t *a = text_addr(0);
    Tn = load_u128_unaligned(a);
    if (sh) Tn4 = load_u32_unaligned(a + 16);
  }
  PlaneCursor planes;
  planes.start(p.planes, pat, n_steps);
  for (int step = 0; step < n_steps && !rejected; ++step) {
    const int col = step << 4;
    if (step % kStepsPerTextLoad == 0) {
      T = Tn;
      const uint32_t t4 = Tn4;
      if (step + kStepsPerTextLoad < n_steps) {
        const uint8_t *a = text_addr(col + 16 * kStepsPerTextLoad);
        Tn = load_u128_unaligned(a);
        if (sh) Tn4 = load_u32_unaligned(a + 16);
      }
      if (strand) {
        const uint32_t a0 = __builtin_amdgcn_alignbit(T.y, T.x, sh), a1 = __builtin_amdgcn_alignbit(T.z, T.y, sh);
        const uint32_t a2 = __builtin_amdgcn_alignbit(T.w, T.z, sh), a3 = __builtin_amdgcn_alignbit(t4, T.w, sh);
        T = make_uint4(~reverse_fields2(a3), ~reverse_fields2(a2), ~reverse_fields2(a1), ~reverse_fields2(a0));
      }
    } else {
      T.x = T.y, T.y = T.z, T.z = T.w;
    }
    uint32_t b0, b1, b2;
    planes.step(step, b0, b1, b2);
    const uint32_t t = T.x;  // text[col .. col + 16), two bits each; none of them is N
    if (col + 16 <= L) {
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const uint32_t m0 = (uint32_t)__builtin_amdgcn_sbfe((int)t, 2 * q, 1);
        const uint32_t m1 = (uint32_t)__builtin_amdgcn_sbfe((int)t, 2 * q + 1, 1);
        myers_column(m, b0, b1, b2, m0, m1, 0u, (uint32_t)q, width, wm);
      }
    } else {  // up to fifteen trailing columns
      for (int q = 0; q < L - col; ++q) {
        const uint32_t cb = t >> (2 * q);
        myers_column(m, b0, b1, b2, 0u - (cb & 1u), 0u - ((cb >> 1) & 1u), 0u, (uint32_t)q, width, wm);
      }
    }
    rejected = past_threshold(m, e);
  }
  return rejected;
}

// The same from the read's characters (rd: its first), sixteen per plain load and step.
__device__ __forceinline__ bool verify_walk_chars(const VerifyParams &p, MyersState &m, const uint8_t *rd, uint32_t strand, uint64_t pat,
                                                  int L, int e, uint32_t width, uint32_t wm) {
  const int n_steps = (L + 15) >> 4;
  bool rejected = false;
  PlaneCursor planes;
  planes.start(p.planes, pat, n_steps);
  for (int step = 0; step < n_steps && !rejected; ++step) {
    const int col = step << 4;
    const uint4 r = text_chunk(rd, strand, L, col);
    uint32_t b0, b1, b2;
    planes.step(step, b0, b1, b2);
    char_step(m, r, strand, L - col, b0, b1, b2, width, wm);
    rejected = past_threshold(m, e);
  }
  return rejected;
}

__global__ void __launch_bounds__(256, 6) verify_kernel_packed(VerifyParams p) {
  // a scratch buffer overflowed while seeding: slots may be unwritten, the host grows the buffer and re-runs the batch
  if (p.ctr[1] != 0) return;
  const uint32_t total = min(p.ctr[0], p.cand_cap);
  const uint32_t stride = gridDim.x * blockDim.x;
  const int e = p.e, L = (int)p.len;
  const uint32_t width = 2u * (uint32_t)e + 1u;
  __shared__ uint32_t part[2][4];
  uint32_t mappings = 0, mapped = 0;
  // one candidate ahead: meta and position first, then (they need those) the sequence's offset and the read's exception word
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t meta_n = kInvalidMeta, exc_n = 0;
  uint64_t c_n = 0, seq_off_n = 0;
  auto request_second = [&] {
    if (meta_n != kInvalidMeta) {
      seq_off_n = p.seq_off[(uint32_t)(c_n >> 32)];
      exc_n = p.exc_bits[(meta_n & ~kMeta16) >> 6];
    }
  };
  if (i < total) {
    meta_n = p.cand_meta[i], c_n = p.cand[i];
    request_second();
  }
  while (i < total) {
    const uint32_t meta = meta_n, exc_word = exc_n;
    const uint64_t c = c_n, seq_off = seq_off_n;
    const uint32_t at = i;
    const uint32_t next = i + stride;
    i = next > at ? next : total;  // (a wrap past 2^32 ends the lane's range)
    meta_n = kInvalidMeta;
    if (i < total) meta_n = p.cand_meta[i], c_n = p.cand[i];
    if (meta == kInvalidMeta) {
      store_invalid(p, at);
      request_second();
      continue;
    }
    const uint32_t read = (meta & ~kMeta16) >> 1, strand = meta & 1u;
    const uint32_t wm = (meta & kMeta16) ? 0xFFFFu : 0xFFFFFFFFu;
    const uint64_t pat = seq_off + (uint32_t)c;  // base index of pattern[0]
    MyersState m{0, 0, 0};
    bool rejected;
    if ((exc_word >> (read & 31u)) & 1u) {
      rejected = verify_walk_chars(p, m, p.bases + (uint64_t)read * (uint32_t)L, strand, pat, L, e, width, wm);
    } else {
      rejected = verify_walk_packed(p, m, p.packed + (uint64_t)read * p.bpr, strand, pat, L, e, width, wm);
    }
    request_second();
    const Outcome o = verify_outcome(p, m, rejected, L, e, at, read);
    mappings += o.accepted, mapped += o.mapped;
  }
  block_sums(p, part, mappings, mapped);
}

}  // namespace femk
