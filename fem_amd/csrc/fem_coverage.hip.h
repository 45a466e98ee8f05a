// fem_coverage.hip.h — windowed depth of the output lines (include/fem_hip.h, fem_dev_set_coverage: the rule).
// Included by fem_tail.hip behind the line kernels' helpers (SamParams, line_head, line_mapq, wave_bcast): coverage_kernel reads a
// line as they do.  It runs from Tail::lines() behind the line index and the MAPQ kernel and reads the index as it is BEFORE folding
// (report_kernel's, or the unmapped reads'; none: line i is record i), so that a folded line counts as the line it was.
//   One lane takes one line: whether it counts (FLAG as written, CIGAR not *, the MAPQ column against min_mapq), its span s = the
//   M and D lengths of its CIGAR words (S operations of a trimmed batch stand in the same words and are passed over), cut at the
//   sequence's end, and the bins [first, first + nb) it meets.  nb == 1: one 64-bit atomicAdd of s.  nb > 1 (a window smaller than
//   the span): the line is handed round the wave, lane k adding to bin first + k, first + k + 64, .. the bases it shares with the
//   span, so that a 150-base line at W = 1 is three rounds of 64 adds side by side and not 150 adds one behind the other.
// The adds are plain atomicAdd on unsigned long long; equal bins are not merged in the wave (DESIGN.md §4.6q has the figures).
#pragma once

struct CoverageParams {
  uint32_t window;           // W >= 1
  uint32_t all_hits;         // != 0: lines with 0x100 count too
  uint32_t min_mapq;
  uint32_t n_seq;
  const uint64_t *bin_off;   // n_seq + 1
  const uint32_t *seq_len;   // n_seq
  unsigned long long *bins;  // bin_off[n_seq]
  uint32_t n_lines;          // the lines of the index, or a bound on them where the count is on the device alone:
  const uint32_t *n_lines_at;  // ... then the count itself (kUnm), else nullptr
};

template <bool kPair, bool kUnm>
__global__ void __launch_bounds__(256) coverage_kernel(SamParams p, CoverageParams c) {
  const uint32_t ln = threadIdx.x & 63u;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t n = c.n_lines;
  if (kUnm && c.n_lines_at) n = min(n, c.n_lines_at[0]);
  uint64_t first = 0;            // the first bin the line's span meets
  uint32_t nb = 0, pos = 0, s = 0;  // the bins it meets (0: the line does not count), its place on its sequence, its span
  if (i < n) {
    const uint32_t j = kUnm ? p.usrc[i] : i;
    if (!kUnm || j < p.u_base) {  // (else an unmapped read's line: FLAG 4)
      const LineHead h = line_head<kPair>(p, j);
      const uint32_t c0 = p.cigar_off[h.rec], c1 = p.cigar_off[h.rec + 1], t = p.tid[h.rec];
      const bool counts = !(h.flag & 4u) && (c.all_hits || !(h.flag & 0x100u)) && c1 > c0 && t < c.n_seq &&
                          line_mapq<kPair>(p, j, h.r, h.primary) >= c.min_mapq;
      if (counts) {
        uint64_t span = 0;
        for (uint32_t k = c0; k < c1; ++k) {
          const uint32_t w = p.cigar[k], op = w & 0xFu;
          if (op == 0u || op == 2u) span += w >> 4;
        }
        pos = p.pos0[h.rec];
        const uint32_t len = c.seq_len[t];
        if (pos < len && span) {
          s = (uint32_t)(span < (uint64_t)(len - pos) ? span : (uint64_t)(len - pos));
          const uint32_t q0 = pos / c.window, q1 = (pos + (s - 1u)) / c.window;  // (pos + s <= len < 2^32)
          first = c.bin_off[t] + q0, nb = q1 - q0 + 1u;
        }
      }
    }
  }
  if (nb == 1u) atomicAdd(c.bins + first, (unsigned long long)s);
  uint64_t todo = __ballot(nb > 1u);
  while (todo) {
    const uint32_t from = (uint32_t)__builtin_ctzll(todo);
    todo &= todo - 1u;
    const uint64_t F = ((uint64_t)wave_bcast((uint32_t)(first >> 32), from) << 32) | wave_bcast((uint32_t)first, from);
    const uint32_t NB = wave_bcast(nb, from), P = wave_bcast(pos, from), S = wave_bcast(s, from);
    const uint64_t w0 = (uint64_t)(P / c.window) * c.window;  // where the span's first window starts on the sequence
    for (uint32_t k = ln; k < NB; k += 64u) {
      const uint64_t a = w0 + (uint64_t)k * c.window, b = a + c.window;  // window k of the span: [a, b)
      const uint64_t lo = a > P ? a : P, hi = b < (uint64_t)P + S ? b : (uint64_t)P + S;
      atomicAdd(c.bins + F + k, (unsigned long long)(hi - lo));
    }
  }
}
