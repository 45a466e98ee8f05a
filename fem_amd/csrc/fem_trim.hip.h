// fem_trim.hip.h — read trimming on the device (include/fem_hip.h, fem_dev_set_trim): the clip points of
// every read from the fixed counts and the qualities, and the kept parts gathered into the batch's MAPPING VIEW (characters +
// offsets of their own), which the mapping kernels, the traceback and the rescue read as they read any batch.  The staged
// buffer stays the whole-read view: the text kernels print SEQ and QUAL from it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace femtr {

constexpr int kMinKeep = 35;  // FEM_TRIM_MIN_KEEP: the quality trim never keeps fewer bases

struct TrimParams {
  const uint8_t *quals;      // quality bytes, same offsets as the bases; read only with qual > 0
  const uint64_t *read_off;  // n_reads + 1: the whole-read view's offsets
  const uint16_t *adapt3;    // n_reads: bases the adapter match takes off the 3' end behind the fixed trims (fem_adapter.hip.h); nullptr: none
  const uint16_t *over3;     // n_reads: the same from the mates' overlap (fem_overlap.hip.h); nullptr: none.  The larger of the two is taken
  uint32_t n_reads;
  int32_t trim5, trim3, qual;
  uint16_t *clip5, *clip3;   // n_reads
  uint64_t *keep;            // n_reads + 1: the kept lengths, the last one zero (the scan's input)
  unsigned long long *ctr;   // [0] reads with c5 + c3 > 0, [1] the sum of c5 + c3
};

// A read behind the fixed trims, as every kernel of the trim stage sees it: where the read starts, its length L, the fixed
// counts c5 and c3f as the read's length bounds them, and what they leave, L' = L - c5 - c3f.
struct Window {
  uint64_t off;
  int L, c5, c3f, Lp;
};
__device__ __forceinline__ Window fixed_window(const uint64_t *at, int trim5, int trim3) {  // at: the read's entry of the offsets
  const uint64_t off = at[0];
  const int L = (int)(at[1] - off);
  const int c5 = trim5 < L ? trim5 : L;
  const int c3f = trim3 < L - c5 ? trim3 : L - c5;
  return {off, L, c5, c3f, L - c5 - c3f};
}

// What a wave counted over its reads, added to a producer's two counters once per wave.
__device__ __forceinline__ void add_wave_counts(unsigned long long *ctr, uint32_t ln, uint32_t n, unsigned long long n_bases) {
  if (ln == 0 && n) {
    atomicAdd(ctr, (unsigned long long)n);
    atomicAdd(ctr + 1, n_bases);
  }
}

// One wave per read.  The fixed trims are arithmetic; the adapter's cut, or the overlap's where that is the larger, comes off what
// they leave, and the quality trim runs on the rest.  The quality trim is the running-sum rule of the header, run from the 3'
// end in chunks of 64 positions, lane 0 the 3'-most: s = carry + the wave's inclusive scan of Q - q; the ballot of s < 0 gives
// the stop, the lanes in front of it are the rule's range, and a max-reduce over (s, lane) finds that range's maximum with
// the least lane, which is the largest l.  A later chunk (smaller l) replaces the cut only with a strictly larger sum, so
// ties keep the largest l over the chunks as well.  The wave leaves the loop together at the first chunk that holds a stop.
__global__ void __launch_bounds__(256) trim_clip_kernel(TrimParams p) {
  const uint32_t ln = threadIdx.x & 63u;
  const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
  if (wave == 0 && ln == 0) p.keep[p.n_reads] = 0;
  uint32_t n_trimmed = 0;
  unsigned long long n_bases = 0;
  for (uint32_t r = wave; r < p.n_reads; r += n_waves) {
    const Window w = fixed_window(p.read_off + r, p.trim5, p.trim3);
    const int c5 = w.c5, c3f = w.c3f;
    const int v3 = p.over3 ? (int)p.over3[r] : 0;
    const int a3 = p.adapt3 && (int)p.adapt3[r] > v3 ? (int)p.adapt3[r] : v3;  // (both are measured from the same end of the same L')
    const int Lp = w.L - c5 - c3f - a3;  // (the window's L' less the larger cut)
    int cut = Lp;
    if (p.qual > 0 && Lp > kMinKeep) {
      const uint8_t *q = p.quals + w.off + c5;
      int carry = 0, best = 0;
      for (int hi = Lp; hi > kMinKeep; hi -= 64) {  // positions [max(hi - 64, K), hi), lane ln at hi - 1 - ln
        const int l = hi - 1 - (int)ln;
        const bool live = l >= kMinKeep;
        int v = live ? p.qual - ((int)q[l] - 33) : 0;
        for (uint32_t d = 1; d < 64u; d <<= 1) {
          const int t = __shfl_up(v, d, 64);
          if (ln >= d) v += t;
        }
        const int s = carry + v;
        const unsigned long long neg = __ballot(live && s < 0);
        const uint32_t first = neg ? (uint32_t)__ffsll((long long)neg) - 1u : 64u;
        // (s, lane) of the lanes in range as one key: s < 2^17 (1024 positions of at most 93 + 33 each), the least lane wins a tie
        int key = live && ln < first ? (s << 6) | (int)(63u - ln) : -1;
        for (uint32_t d = 32; d > 0; d >>= 1) {
          const int o = __shfl_xor(key, d, 64);
          key = o > key ? o : key;
        }
        if (key >= 0 && (key >> 6) > best) best = key >> 6, cut = hi - 1 - (int)(63u - ((uint32_t)key & 63u));
        if (neg) break;
        carry = __shfl(s, 63, 64);
      }
    }
    const int c3 = c3f + a3 + (Lp - cut);
    if (ln == 0) {
      p.clip5[r] = (uint16_t)c5, p.clip3[r] = (uint16_t)c3;
      p.keep[r] = (uint64_t)(w.L - c5 - c3);
    }
    if (c5 + c3 > 0) ++n_trimmed, n_bases += (unsigned long long)(c5 + c3);
  }
  add_wave_counts(p.ctr, ln, n_trimmed, n_bases);
}

// The kept bytes of every read into the mapping view: a wave per read, the lanes along its bytes.
__global__ void __launch_bounds__(256) trim_gather_kernel(const uint8_t *bases, const uint64_t *read_off, const uint16_t *clip5,
                                                          const uint64_t *map_off, uint32_t n_reads, uint8_t *map_bases) {
  const uint32_t ln = threadIdx.x & 63u;
  const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
  for (uint32_t r = wave; r < n_reads; r += n_waves) {
    const uint64_t to = map_off[r];
    const uint32_t keep = (uint32_t)(map_off[r + 1] - to);
    const uint8_t *from = bases + read_off[r] + clip5[r];
    for (uint32_t j = ln; j < keep; j += 64u) map_bases[to + j] = from[j];
  }
}

}  // namespace femtr
