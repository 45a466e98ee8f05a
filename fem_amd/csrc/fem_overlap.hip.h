// fem_overlap.hip.h — read-through found from the mates' overlap (include/fem_hip.h, fem_dev_set_pair_overlap):
// when a fragment is shorter than the reads, mate 1 is the reverse complement of mate 2 over the whole fragment; the largest
// fragment length F at which the two agree within the error percentage gives the cut v3 of both mates, with no adapter known.
// It runs in front of trim_clip_kernel (fem_trim.hip.h), which takes the larger of v3 and the adapter's cut off the 3' end.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fem_trim.hip.h"

namespace femov {

constexpr int kWords = 16;  // 64-bit words of a bit plane: reads are <= 1024 bases on the device
constexpr int kWaves = 4;   // waves of a block

struct OverlapParams {
  const uint8_t *bases;      // the whole-read view's characters
  const uint64_t *read_off;  // n_reads + 1
  uint32_t n_reads;          // reads i and n_reads / 2 + i are the mates of pair i
  int32_t trim5, trim3;      // the fixed trims the match runs behind
  int32_t min_overlap, err_pct;
  uint16_t *over3;           // n_reads
  unsigned long long *ctr;   // [0] pairs with F > 0, [1] the sum of v3 over both mates
};

// A read as three bit planes over its positions: two bits of the letter's code (A 0, C 1, T 2, G 3: bits 1 and 2 of the upper-case
// byte) and whether the byte is a letter of ACGTacgt at all.  No bit is set at or past the read's length.
struct Planes {
  unsigned long long b0[kWords], b1[kWords], ok[kWords];
};

// DS operations of one wave execute in order; only the compiler has to be kept from moving them.
__device__ __forceinline__ void wave_sync_lds() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The planes of s[0 .. L), or with rc those of its reverse complement (position i holds the complement of s[L - 1 - i]; in the
// code above that is bit 1 flipped).  Lane ln looks at position 64 k + ln of word k; positions at and past L (the next read's
// bytes) are not loaded.  Words from (L + 63) / 64 on are not written: word() gives 0 for them.
__device__ inline void make_planes(Planes &pl, const uint8_t *s, int L, bool rc, uint32_t ln) {
  for (int k = 0; k * 64 < L && k < kWords; ++k) {
    const int pos = k * 64 + (int)ln;
    const uint32_t ch = pos < L ? (uint32_t)s[rc ? L - 1 - pos : pos] & 0xDFu : 0u;  // (upper case: 'a' ^ 'A' is the one bit)
    const bool ok = ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T';
    const uint32_t code = ((ch >> 1) & 3u) ^ (rc ? 2u : 0u);
    const unsigned long long w0 = __ballot(ok && (code & 1u)), w1 = __ballot(ok && (code & 2u)), wk = __ballot(ok);
    if (ln == 0) pl.b0[k] = w0, pl.b1[k] = w1, pl.ok[k] = wk;
  }
}

__device__ __forceinline__ unsigned long long word(const unsigned long long *plane, int k, int n_words) {
  return (unsigned)k < (unsigned)n_words ? plane[k] : 0ull;
}

// Bits [t, t + 64) of a plane, t of either sign: the two neighbouring words shifted together.
__device__ __forceinline__ unsigned long long shifted(const unsigned long long *plane, int t, int n_words) {
  const int q = t >> 6;
  const uint32_t r = (uint32_t)t & 63u;
  const unsigned long long a = word(plane, q, n_words), b = word(plane, q + 1, n_words);
  return r ? (a >> r) | (b << (64u - r)) : a;
}

// One wave per pair.  x is mate 1 behind the fixed trims, z the reverse complement of mate 2 behind them, both as bit planes in
// the wave's LDS, made once per pair.  For a candidate f the rule compares x[j] with z[j + s], s = L2' - f, over j in [lo, hi):
// x's validity plane has no bit at or past L1' and z's none outside [0, L2'), so the AND of the two validity planes, z's shifted
// by s, is set exactly inside [lo, hi), and the equal positions are counted over whole words with nothing to mask:
// matches = sum over words of popcount(xk & zk & ~(x0 ^ z0) & ~(x1 ^ z1)), mm = o - matches.  The candidates run in windows of 64
// downward from max(L1', L2') - 1, lane ln owning f = top - ln; the words walked are the window's union of [lo, hi) (wave-uniform,
// words outside a lane's own range add nothing).  The wave leaves at the first window with a matching lane; the lowest such lane
// has the largest f.  Candidates below O cannot match (o <= f), so the windows stop there.
__global__ void __launch_bounds__(64 * kWaves) pair_overlap_kernel(OverlapParams p) {
  __shared__ Planes planes[kWaves][2];
  const uint32_t ln = threadIdx.x & 63u;
  const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
  const uint32_t n_pairs = p.n_reads / 2u;
  Planes &X = planes[threadIdx.x >> 6][0], &Z = planes[threadIdx.x >> 6][1];
  if (wave == 0 && ln == 0 && (p.n_reads & 1u)) p.over3[p.n_reads - 1u] = 0;  // (a read without a mate)
  uint32_t n_cut = 0;
  unsigned long long n_bases = 0;
  for (uint32_t i = wave; i < n_pairs; i += n_waves) {
    int Lp[2];
    const uint8_t *at[2];
    for (int k = 0; k < 2; ++k) {
      const femtr::Window w = femtr::fixed_window(p.read_off + (k ? n_pairs + i : i), p.trim5, p.trim3);
      Lp[k] = w.Lp, at[k] = p.bases + w.off + w.c5;
    }
    const int L1 = Lp[0], L2 = Lp[1];
    const int nx = L1 < 64 * kWords ? (L1 + 63) >> 6 : kWords, nz = L2 < 64 * kWords ? (L2 + 63) >> 6 : kWords;
    wave_sync_lds();  // (the previous pair's reads of the planes are done)
    make_planes(X, at[0], L1, false, ln);
    make_planes(Z, at[1], L2, true, ln);
    wave_sync_lds();
    int F = 0;
    for (int top = (L1 > L2 ? L1 : L2) - 1; top >= p.min_overlap; top -= 64) {
      const int f = top - (int)ln;
      const int lo = f - L2 > 0 ? f - L2 : 0, hi = f < L1 ? f : L1, o = hi - lo;
      const int f_least = top - 63 > 1 ? top - 63 : 1;
      const int w_lo = (f_least - L2 > 0 ? f_least - L2 : 0) >> 6, w_hi = ((top < L1 ? top : L1) - 1) >> 6;  // (L1' = 0: no word)
      const int s = L2 - f;
      int matches = 0;
      for (int w = w_lo; w <= w_hi; ++w) {
        const int t = 64 * w + s;
        const unsigned long long eq = word(X.ok, w, nx) & shifted(Z.ok, t, nz) & ~(word(X.b0, w, nx) ^ shifted(Z.b0, t, nz)) &
                                      ~(word(X.b1, w, nx) ^ shifted(Z.b1, t, nz));
        matches += __popcll(eq);
      }
      const bool hit = f >= 1 && o >= p.min_overlap && (o - matches) * 100 <= o * p.err_pct;
      const unsigned long long hits = __ballot(hit);
      if (hits) {
        F = top - (__ffsll((long long)hits) - 1);
        break;
      }
    }
    const int v1 = F > 0 && L1 > F ? L1 - F : 0, v2 = F > 0 && L2 > F ? L2 - F : 0;
    if (ln == 0) p.over3[i] = (uint16_t)v1, p.over3[n_pairs + i] = (uint16_t)v2;
    if (F > 0) ++n_cut, n_bases += (unsigned long long)(v1 + v2);
  }
  femtr::add_wave_counts(p.ctr, ln, n_cut, n_bases);
}

}  // namespace femov
