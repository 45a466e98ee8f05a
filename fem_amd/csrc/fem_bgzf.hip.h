// BGZF (SAM/BAM specification §4.1) on the device: gzip members of at most 64 KiB, each with its compressed size in a BC extra
// field, deflated by fem_bgzf.hip's kernels (level 1: LZ77 + dynamic Huffman; level 0: stored blocks).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "fem_buf.hip.h"

namespace femz {

constexpr uint32_t kBgzfInput = 65280;  // input bytes per member at most (htslib's BGZF_BLOCK_SIZE)
constexpr uint32_t kBgzfSlot = 65536;   // a member's size at most

// Greedy member cuts: members take whole records while they fit in kBgzfInput (a record over kBgzfInput is split).
// rec_off: n_rec + 1 ascending offsets (rec_off[0] = 0, rec_off[n_rec] = n); nullptr: cut every kBgzfInput bytes.
// starts receives the members' first offsets followed by n (empty for n = 0).
void bgzf_cut(const uint64_t *rec_off, uint64_t n_rec, uint64_t n, std::vector<uint64_t> *starts);

class Bgzf {
 public:
  // Compresses the n bytes at device pointer `in` into the members starts[0..k] describes (bgzf_cut) on `stream`, and waits
  // for the stream once (the members' sizes).  The members then lie back to back at out() (device memory, *len bytes),
  // valid until the next call.  level: 0 (stored) or 1.  ms (optional) receives the kernels' device time.
  int compress(const uint8_t *in, uint64_t n, const std::vector<uint64_t> &starts, int level, hipStream_t stream, uint64_t *len,
               std::string *err, float *ms = nullptr);
  const uint8_t *out() const { return out_; }

 private:
  femb::Buf<uint8_t, femb::Mem::Device, femb::Grow::Quarter> out_, slots_;
  femb::Buf<uint32_t, femb::Mem::Device, femb::Grow::Quarter> tokens_;
  femb::Buf<unsigned long long> starts_d_, sizes_;  // (member starts up; sizes and offsets on the device)
  femb::PinBuf<unsigned long long> h_starts_, h_total_;
  femb::Event ev_[2];
};

}  // namespace femz
