// fem_coverage.h — the window arithmetic of the coverage track (include/fem_hip.h, fem_dev_set_coverage: rule 3), in one place for
// libfemhost.so (fem_coverage_layout, fem_host.h) and libfemhip.so (fem_dev_set_coverage), so that both lay the bins out alike.
// Host code only; no allocation.
#pragma once
#include <stdint.h>

namespace femc {

constexpr int32_t kMaxWindow = 1000000;
constexpr uint64_t kMaxBins = 1ull << 29;

// The windows of a sequence of `len` bases: ceil(len / window)
inline uint64_t windows_of(uint32_t len, int32_t window) { return ((uint64_t)len + (uint32_t)window - 1u) / (uint32_t)window; }

// bin_off[t] = the windows of the sequences in front of t (n_seq + 1 entries, or nullptr), *n_bins their total, which is set whenever
// the arguments are in range.  0; -1: a null argument or a window outside 1 .. kMaxWindow; -2: more than kMaxBins windows.
inline int layout(uint32_t n_seq, const uint32_t *seq_len, int32_t window, uint64_t *bin_off, uint64_t *n_bins) {
  if ((n_seq && !seq_len) || !n_bins || window < 1 || window > kMaxWindow) return -1;
  uint64_t n = 0;  // (below 2^64: 2^32 sequences of fewer than 2^32 windows each)
  for (uint32_t t = 0; t < n_seq; ++t) n += windows_of(seq_len[t], window);
  *n_bins = n;
  if (n > kMaxBins) return -2;
  if (bin_off) {
    n = 0;
    for (uint32_t t = 0; t < n_seq; ++t) bin_off[t] = n, n += windows_of(seq_len[t], window);
    bin_off[n_seq] = n;
  }
  return 0;
}

// The least window whose layout has at most kMaxBins windows (the count falls as the window grows); 0: none up to kMaxWindow.
inline int32_t min_window(uint32_t n_seq, const uint32_t *seq_len) {
  uint64_t n = 0;
  if (layout(n_seq, seq_len, kMaxWindow, nullptr, &n) != 0) return 0;
  int32_t lo = 1, hi = kMaxWindow;  // (hi fits)
  while (lo < hi) {
    const int32_t mid = lo + (hi - lo) / 2;
    if (layout(n_seq, seq_len, mid, nullptr, &n) == 0) hi = mid; else lo = mid + 1;
  }
  return hi;
}

}  // namespace femc
