// fem_adapter.hip.h — 3' adapter matching on the device (include/fem_hip.h, fem_dev_set_adapter): for every read
// the number of bases a3 from the leftmost place where the adapter (or the part of it the read's end leaves) matches within the
// error percentage.  It runs in front of trim_clip_kernel (fem_trim.hip.h), which takes a3 off the 3' end before its quality rule.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fem_trim.hip.h"

namespace femad {

struct AdapterParams {
  const uint8_t *bases;      // the whole-read view's characters
  const uint64_t *read_off;  // n_reads + 1
  uint32_t n_reads;
  uint32_t second_begin;     // reads from here on are matched against adapter 1 (mate 2's), the others against adapter 0
  int32_t trim5, trim3;      // the fixed trims the match runs behind
  int32_t min_overlap, err_pct;
  uint64_t occ[2][4];        // per adapter: bit j of occ[.][c] says that its letter j is "ACGT"[c]
  int32_t len[2];            // 4 .. 64
  uint16_t *adapt3;          // n_reads
  unsigned long long *ctr;   // [0] reads with a3 > 0, [1] the sum of a3
};

// The occurrence words of one window of 64 positions [at, at + 64) of x[0 .. Lp): lane ln looks at position at + ln; the four
// ballots are wave-uniform.  Positions at and past Lp (the next read's bytes) are not loaded and set no bit, and neither does a
// byte that is no letter of ACGTacgt, so such a position matches nothing.
struct OccWords {
  unsigned long long w[4];
};
__device__ inline OccWords occ_words(const uint8_t *x, int at, int Lp, uint32_t ln) {
  const int pos = at + (int)ln;
  const uint32_t ch = pos < Lp ? (uint32_t)x[pos] & 0xDFu : 0u;  // (upper case: 'a' ^ 'A' is the one bit)
  OccWords o;
  o.w[0] = __ballot(ch == 'A'), o.w[1] = __ballot(ch == 'C'), o.w[2] = __ballot(ch == 'G'), o.w[3] = __ballot(ch == 'T');
  return o;
}

// One wave per read, windows of 64 start positions from the 5' end, lane ln the start p = at + ln.  A start reads up to 63 bases
// ahead, so a window needs its own occurrence words and the next window's: each window's are made once and carried over.  For
// letter c the 128-bit pair (cur, next) shifted right by ln has in bit j whether x[p + j] is c; ANDed with the adapter's
// occurrence word of c and counted over the four letters that is the number of matching j.  No bit is set at or past Lp, so with
// o = min(m, Lp - p) the mismatches are o - matches, the rule's mm.  The ballot of the matching starts and its lowest bit give the
// least p; the wave leaves together at the first window that holds one.
__global__ void __launch_bounds__(256) adapter_match_kernel(AdapterParams p) {
  const uint32_t ln = threadIdx.x & 63u;
  const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
  uint32_t n_cut = 0;
  unsigned long long n_bases = 0;
  for (uint32_t r = wave; r < p.n_reads; r += n_waves) {
    const femtr::Window w = femtr::fixed_window(p.read_off + r, p.trim5, p.trim3);
    const int Lp = w.Lp;
    const uint8_t *x = p.bases + w.off + w.c5;
    const int which = r >= p.second_begin ? 1 : 0;
    const int m = p.len[which];
    const unsigned long long a0 = p.occ[which][0], a1 = p.occ[which][1], a2 = p.occ[which][2], a3w = p.occ[which][3];
    int a3 = 0;
    OccWords cur = occ_words(x, 0, Lp, ln);
    for (int at = 0; at < Lp; at += 64) {
      OccWords nxt{{0, 0, 0, 0}};
      if (at + 64 < Lp) nxt = occ_words(x, at + 64, Lp, ln);  // (wave-uniform: the ballots inside see the whole wave)
      int matches = 0;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const unsigned long long t = ln ? (cur.w[c] >> ln) | (nxt.w[c] << (64u - ln)) : cur.w[c];
        matches += __popcll(t & (c == 0 ? a0 : c == 1 ? a1 : c == 2 ? a2 : a3w));
      }
      const int left = Lp - (at + (int)ln);
      const int o = m < left ? m : left;
      const bool hit = o >= p.min_overlap && (o - matches) * 100 <= o * p.err_pct;
      const unsigned long long hits = __ballot(hit);
      if (hits) {
        a3 = Lp - (at + (__ffsll((long long)hits) - 1));
        break;
      }
      cur = nxt;
    }
    if (ln == 0) p.adapt3[r] = (uint16_t)a3;
    if (a3 > 0) ++n_cut, n_bases += (unsigned long long)a3;
  }
  femtr::add_wave_counts(p.ctr, ln, n_cut, n_bases);
}

}  // namespace femad
