// fem_bgzf.hip — BGZF members deflated on the device (SAM/BAM specification §4.1, RFC 1951/1952).
//
// One workgroup (one wave) per member; the member's input (<= 65280 bytes) and a hash table sit in LDS, two members per CU.
//   CRC-32   each lane over a 1/64 slice (table in LDS), slices combined by multiplying by x^(8 len) mod P.
//   LZ77     64 positions per step: each lane hashes the 3 bytes at its position; its candidates are the two latest earlier
//            positions with the same hash (the wave's own positions, found by v_readlane, then the table's two per bucket).
//            The match length is compared a word at a time.  The greedy parse walks the step's match lengths (scalar loop
//            over v_readlane), and the steps a long match covers skip the comparisons.  Tokens go to global scratch.
//   Huffman  symbol histograms with LDS atomics; lane 0 builds minimum-redundancy code lengths (Moffat-Katajainen, in place
//            on the sorted frequencies; the lanes rank-sort them), limits them (15 bits; 7 for the code-length alphabet) by
//            moving codes down the length counts, and writes the block header (code lengths run-length coded with 16/17/18).
//   Bits     a wave-wide prefix sum over each token's bit count gives its bit offset; bits are OR-ed into LDS words.
//   A member is stored (BTYPE 0) when that is not larger; level 0 stores every member.
// Member sizes are scanned by one block and the members gathered back to back.
#include "fem_bgzf.hip.h"

#include <algorithm>
#include <cstring>

#include "../../include/fem_hip.h"

namespace femz {
namespace {

constexpr uint32_t kHashBits = 12, kBuckets = 1u << kHashBits;
constexpr uint32_t kInWords = (kBgzfInput + 8u) / 4u;  // input + the 8 bytes a word-wise compare may read past its end
constexpr uint32_t kNone = 0xFFFFu;

__device__ __forceinline__ uint32_t rl(uint32_t v, uint32_t i) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)i); }

// CRC-32 arithmetic in the reflected domain (x^0 is bit 31)
__device__ uint32_t crc_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (uint32_t m = 1u << 31; a && m; m >>= 1) {
    if (a & m) {
      p ^= b;
      a &= ~m;
    }
    b = (b & 1u) ? (b >> 1) ^ 0xEDB88320u : b >> 1;
  }
  return p;
}
__device__ uint32_t crc_xpow8(uint32_t n) {  // x^(8 n) mod P
  uint32_t p = 1u << 31, t = 1u << 30;
  t = crc_mul(t, t), t = crc_mul(t, t), t = crc_mul(t, t);
  for (; n; n >>= 1) {
    if (n & 1u) p = crc_mul(t, p);
    t = crc_mul(t, t);
  }
  return p;
}

// deflate's length and distance codes (RFC 1951 §3.2.5), arithmetically
__device__ __forceinline__ void len_code(uint32_t len, uint32_t *sym, uint32_t *eb, uint32_t *ev) {
  const uint32_t l = len - 3u;
  if (len == 258u) *sym = 285u, *eb = 0, *ev = 0;
  else if (l < 8u) *sym = 257u + l, *eb = 0, *ev = 0;
  else {
    const uint32_t nb = 31u - __builtin_clz(l), b = (l >> (nb - 2u)) & 3u;
    *sym = 257u + 4u * (nb - 1u) + b, *eb = nb - 2u, *ev = l - ((4u | b) << (nb - 2u));
  }
}
__device__ __forceinline__ void dist_code(uint32_t dist, uint32_t *sym, uint32_t *eb, uint32_t *ev) {
  const uint32_t d = dist - 1u;
  if (d < 4u) *sym = d, *eb = 0, *ev = 0;
  else {
    const uint32_t nb = 31u - __builtin_clz(d), b = (d >> (nb - 1u)) & 1u;
    *sym = 2u * nb + b, *eb = nb - 1u, *ev = d - ((2u | b) << (nb - 1u));
  }
}

__device__ __forceinline__ uint32_t rev_bits(uint32_t c, uint32_t n) { return __builtin_bitreverse32(c) >> (32u - n); }

struct Huff {  // the Huffman phase's LDS (in the hash table's place)
  uint32_t f_l[288], f_d[32], f_c[20];
  uint32_t len_l[288], len_d[32], len_c[20];
  uint32_t code_l[288], code_d[32], code_c[20];
  uint32_t a[288], sym[288];
  uint32_t rle_sym[320], rle_ext[320];
  uint32_t num[40], next[20];
  uint32_t n_rle, hlit, hdist, hclen, hdr_bits;
};
static_assert(sizeof(Huff) <= kBuckets * 4, "Huffman tables must fit in the hash table's LDS");

// Length-limited code lengths of alphabet f[0..n) into len[0..n) (whole wave; lane 0 does the sequential part).
__device__ void build_lengths(Huff &H, uint32_t *f, uint32_t *len, uint32_t n, uint32_t limit) {
  const uint32_t ln = threadIdx.x;
  uint32_t used = 0;
  for (uint32_t s = ln; s < n; s += 64u) used += f[s] ? 1u : 0u;
  for (uint32_t o = 32; o; o >>= 1) used += __shfl_xor(used, o);
  if (used < 2u) {  // (a complete code needs two symbols: give the first unused ones a weight of 1)
    __syncthreads();
    if (ln == 0) {
      uint32_t u = used;
      for (uint32_t s = 0; s < n && u < 2u; ++s)
        if (!f[s]) f[s] = 1u, ++u;
    }
    __syncthreads();
    used = 2u;
  }
  for (uint32_t s = ln; s < n; s += 64u) {  // rank sort: ascending frequency, ties by symbol
    len[s] = 0;
    const uint32_t fs = f[s];
    if (!fs) continue;
    uint32_t r = 0;
    for (uint32_t t = 0; t < n; ++t) {
      const uint32_t ft = f[t];
      r += (ft && (ft < fs || (ft == fs && t < s))) ? 1u : 0u;
    }
    H.a[r] = fs, H.sym[r] = s;
  }
  __syncthreads();
  if (ln == 0) {
    uint32_t *A = H.a;
    const int N = (int)used;
    // minimum-redundancy code lengths in place (Moffat & Katajainen 1995)
    A[0] += A[1];
    int root = 0, leaf = 2;
    for (int next = 1; next < N - 1; ++next) {
      if (leaf >= N || A[root] < A[leaf]) A[next] = A[root], A[root++] = (uint32_t)next;
      else A[next] = A[leaf++];
      if (leaf >= N || (root < next && A[root] < A[leaf])) A[next] += A[root], A[root++] = (uint32_t)next;
      else A[next] += A[leaf++];
    }
    A[N - 2] = 0;
    for (int next = N - 3; next >= 0; --next) A[next] = A[A[next]] + 1u;
    int avbl = 1, used_d = 0, dpth = 0;
    root = N - 2;
    int next = N - 1;
    while (avbl > 0) {
      while (root >= 0 && (int)A[root] == dpth) ++used_d, --root;
      while (avbl > used_d) A[next--] = (uint32_t)dpth, --avbl;
      avbl = 2 * used_d, ++dpth, used_d = 0;
    }
    // count per length, clamp to the limit, then take codes off the longest lengths until the Kraft sum is exact
    for (uint32_t i = 0; i < 40u; ++i) H.num[i] = 0;
    for (int i = 0; i < N; ++i) H.num[A[i] < 39u ? A[i] : 39u]++;
    for (uint32_t i = limit + 1u; i < 40u; ++i) H.num[limit] += H.num[i], H.num[i] = 0;
    uint32_t total = 0;
    for (uint32_t i = 1; i <= limit; ++i) total += H.num[i] << (limit - i);
    while (total != (1u << limit)) {
      H.num[limit]--;
      for (uint32_t i = limit - 1u; i > 0; --i)
        if (H.num[i]) {
          H.num[i]--, H.num[i + 1] += 2u;
          break;
        }
      total--;
    }
    int j = N;  // the most frequent symbols take the shortest codes
    for (uint32_t i = 1; i <= limit; ++i)
      for (uint32_t k = H.num[i]; k > 0; --k) len[H.sym[--j]] = i;
    // canonical codes, bit-reversed for deflate's LSB-first packing
    uint32_t cnt[16] = {}, code = 0;
    for (uint32_t s = 0; s < n; ++s) cnt[len[s]]++;
    cnt[0] = 0;
    for (uint32_t b = 1; b <= limit; ++b) code = (code + cnt[b - 1]) << 1, H.next[b] = code;
  }
  __syncthreads();
}

__device__ void assign_codes(Huff &H, const uint32_t *len, uint32_t *code, uint32_t n) {  // lane 0, after build_lengths
  for (uint32_t s = 0; s < n; ++s)
    if (len[s]) code[s] = rev_bits(H.next[len[s]]++, len[s]);
}

__device__ __forceinline__ void put_bits(uint32_t *w, uint32_t words, uint32_t pos, uint32_t v, uint32_t n) {
  if (!n) return;
  const uint64_t x = (uint64_t)v << (pos & 31u);
  const uint32_t i = pos >> 5;
  if (i < words && (uint32_t)x) atomicOr(&w[i], (uint32_t)x);
  if (i + 1u < words && (uint32_t)(x >> 32)) atomicOr(&w[i + 1u], (uint32_t)(x >> 32));
}

__device__ __forceinline__ void put_u16(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v, p[1] = (uint8_t)(v >> 8); }
__device__ __forceinline__ void put_u32(uint8_t *p, uint32_t v) { put_u16(p, v), put_u16(p + 2, v >> 16); }

// gzip member header with the BC field (BSIZE = member size - 1), bytes 0..17
__device__ void member_header(uint8_t *o, uint32_t size) {
  const uint8_t h[16] = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 'B', 'C', 2, 0};
  for (int i = 0; i < 16; ++i) o[i] = h[i];
  put_u16(o + 16, size - 1u);
}

__global__ void __launch_bounds__(64) bgzf_member_kernel(const uint8_t *__restrict__ in, const unsigned long long *__restrict__ starts,
                                                         uint32_t n_members, int level, uint32_t *__restrict__ tokens,
                                                         uint8_t *__restrict__ slots, unsigned long long *__restrict__ sizes) {
  __shared__ uint32_t buf[kInWords];  // the input, then the deflate bits
  __shared__ uint32_t tab[kBuckets];  // CRC table, then the hash table (two 16-bit positions per bucket), then Huff
  const uint32_t m = blockIdx.x, ln = threadIdx.x;
  if (m >= n_members) return;
  const uint64_t s0 = starts[m];
  const uint32_t n = (uint32_t)(starts[m + 1] - s0);
  const uint8_t *src = in + s0;
  uint8_t *o = slots + (size_t)m * kBgzfSlot;
  uint8_t *b8 = (uint8_t *)buf;
  // ---- input into LDS; CRC-32 ----
  for (uint32_t w = ln; w < kInWords; w += 64u) {
    uint32_t v = 0;
    for (uint32_t k = 0; k < 4u; ++k) {
      const uint32_t i = 4u * w + k;
      if (i < n) v |= (uint32_t)src[i] << (8u * k);
    }
    buf[w] = v;
  }
  for (uint32_t i = ln; i < 256u; i += 64u) {
    uint32_t c = i;
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
    tab[i] = c;
  }
  __syncthreads();
  const uint32_t S = (n + 63u) / 64u, a0 = std::min(n, ln * S), a1 = std::min(n, a0 + S);
  uint32_t c = 0;
  for (uint32_t i = a0; i < a1; ++i) c = tab[(c ^ b8[i]) & 255u] ^ (c >> 8);
  const uint32_t xp = crc_xpow8(a1 - a0);
  uint32_t crc = 0;
  for (uint32_t l = 0; l < 64u; ++l) crc = crc_mul(crc, rl(xp, l)) ^ rl(c, l);
  crc = ~(crc ^ crc_mul(0xFFFFFFFFu, crc_xpow8(n)));
  __syncthreads();

  uint32_t dyn_bytes = 0xFFFFFFFFu;
  if (level > 0 && n >= 16u) {
    // ---- LZ77 ----
    for (uint32_t i = ln; i < kBuckets; i += 64u) tab[i] = 0xFFFFFFFFu;
    __syncthreads();
    uint32_t *tok = tokens + s0;
    auto word_at = [&](uint32_t x) -> uint32_t {
      return __builtin_amdgcn_alignbyte(buf[(x >> 2) + 1u], buf[x >> 2], x & 3u);
    };
    uint32_t carry = 0, n_tok = 0;
    for (uint32_t base = 0; base < n; base += 64u) {
      const uint32_t i = base + ln;
      const bool valid = i + 3u <= n;
      const uint32_t w = valid ? word_at(i) : 0u;
      const uint32_t h = valid ? (((w & 0xFFFFFFu) * 2654435761u) >> (32u - kHashBits)) : (0x10000u + ln);
      int c0 = -1, c1 = -1;
      bool later = false;
      for (uint32_t k = 0; k < 64u; ++k) {
        const uint32_t hk = rl(h, k);
        if (hk == h && k < ln) c1 = c0, c0 = (int)(base + k);
        later |= hk == h && k > ln;
      }
      const uint32_t t = valid ? tab[h] : 0xFFFFFFFFu;
      const int t0 = (t & 0xFFFFu) == kNone ? -1 : (int)(t & 0xFFFFu), t1 = (t >> 16) == kNone ? -1 : (int)(t >> 16);
      const int ca = c0 >= 0 ? c0 : t0, cb = c0 >= 0 ? (c1 >= 0 ? c1 : t0) : t1;
      __syncthreads();
      if (valid && !later) tab[h] = i | ((uint32_t)(c0 >= 0 ? c0 : (int)(t & 0xFFFFu)) << 16);
      __syncthreads();
      if (carry >= base + 64u) continue;  // (covered by a match: nothing to compare)
      uint32_t best = 0, bdist = 0;
      if (valid && i >= carry) {
        const uint32_t maxlen = std::min<uint32_t>(258u, n - i);
        for (int q = 0; q < 2; ++q) {
          const int cand = q == 0 ? ca : cb;
          if (cand < 0 || i - (uint32_t)cand > 32768u) continue;
          uint32_t k = 0;
          while (k < maxlen) {
            const uint32_t d = word_at((uint32_t)cand + k) ^ word_at(i + k);
            if (d) {
              k += (uint32_t)__builtin_ctz(d) >> 3;
              break;
            }
            k += 4u;
          }
          k = std::min(k, maxlen);
          if (k > best) best = k, bdist = i - (uint32_t)cand;
        }
        if (best < 3u || (best == 3u && bdist > 4096u)) best = 0;
      }
      // the greedy parse through this step
      uint64_t mask = 0;
      uint32_t p = carry - base;
      while (p < 64u && base + p < n) {
        mask |= 1ull << p;
        const uint32_t l = rl(best, p);
        p += l ? l : 1u;
      }
      carry = base + p;
      if ((mask >> ln) & 1ull) {
        const uint32_t idx = n_tok + (uint32_t)__builtin_popcountll(mask & ((1ull << ln) - 1ull));
        tok[idx] = best ? (0x80000000u | ((best - 3u) << 16) | (bdist - 1u)) : (uint32_t)b8[i];
      }
      n_tok += (uint32_t)__builtin_popcountll(mask);
    }
    __syncthreads();
    // ---- Huffman ----
    Huff &H = *(Huff *)tab;
    for (uint32_t s = ln; s < 288u; s += 64u) H.f_l[s] = 0;
    if (ln < 32u) H.f_d[ln] = 0;
    if (ln < 20u) H.f_c[ln] = 0;
    __syncthreads();
    for (uint32_t k = ln; k < n_tok; k += 64u) {
      const uint32_t x = tok[k];
      uint32_t sym, eb, ev;
      if (x & 0x80000000u) {
        len_code(((x >> 16) & 0xFFu) + 3u, &sym, &eb, &ev);
        atomicAdd(&H.f_l[sym], 1u);
        dist_code((x & 0xFFFFu) + 1u, &sym, &eb, &ev);
        atomicAdd(&H.f_d[sym], 1u);
      } else {
        atomicAdd(&H.f_l[x], 1u);
      }
    }
    if (ln == 0) H.f_l[256] = 1;
    __syncthreads();
    build_lengths(H, H.f_l, H.len_l, 286u, 15u);
    if (ln == 0) assign_codes(H, H.len_l, H.code_l, 286u);
    __syncthreads();
    build_lengths(H, H.f_d, H.len_d, 30u, 15u);
    if (ln == 0) {
      assign_codes(H, H.len_d, H.code_d, 30u);
      uint32_t hlit = 286u, hdist = 30u;
      while (hlit > 257u && !H.len_l[hlit - 1u]) --hlit;
      while (hdist > 1u && !H.len_d[hdist - 1u]) --hdist;
      H.hlit = hlit, H.hdist = hdist;
      // run-length code of the hlit + hdist code lengths
      const uint32_t total = hlit + hdist;
      auto L = [&](uint32_t i) { return i < hlit ? H.len_l[i] : H.len_d[i - hlit]; };
      uint32_t r = 0;
      auto emit = [&](uint32_t s, uint32_t e) { H.rle_sym[r] = s, H.rle_ext[r] = e, ++r; };
      for (uint32_t i = 0; i < total;) {
        const uint32_t v = L(i);
        uint32_t run = 1;
        while (i + run < total && L(i + run) == v) ++run;
        uint32_t left = run;
        if (v == 0) {
          while (left >= 11u) {
            const uint32_t k = std::min(left, 138u);
            emit(18u, k - 11u), left -= k;
          }
          if (left >= 3u) emit(17u, left - 3u), left = 0;
          for (; left; --left) emit(0, 0);
        } else {
          emit(v, 0), --left;
          while (left >= 3u) {
            const uint32_t k = std::min(left, 6u);
            emit(16u, k - 3u), left -= k;
          }
          for (; left; --left) emit(v, 0);
        }
        i += run;
      }
      H.n_rle = r;
      for (uint32_t k = 0; k < r; ++k) H.f_c[H.rle_sym[k]]++;
    }
    __syncthreads();
    build_lengths(H, H.f_c, H.len_c, 19u, 7u);
    // ---- bits: header, tokens, end of block ----
    for (uint32_t w = ln; w < kInWords; w += 64u) buf[w] = 0;
    __syncthreads();
    if (ln == 0) {
      assign_codes(H, H.len_c, H.code_c, 19u);
      const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
      uint32_t hclen = 19u;
      while (hclen > 4u && !H.len_c[order[hclen - 1u]]) --hclen;
      uint32_t pos = 0;
      auto put = [&](uint32_t v, uint32_t nb) { put_bits(buf, kInWords, pos, v, nb), pos += nb; };
      put(1u, 1u), put(2u, 2u), put(H.hlit - 257u, 5u), put(H.hdist - 1u, 5u), put(hclen - 4u, 4u);
      for (uint32_t k = 0; k < hclen; ++k) put(H.len_c[order[k]], 3u);
      for (uint32_t k = 0; k < H.n_rle; ++k) {
        const uint32_t s = H.rle_sym[k];
        put(H.code_c[s], H.len_c[s]);
        if (s == 16u) put(H.rle_ext[k], 2u);
        else if (s == 17u) put(H.rle_ext[k], 3u);
        else if (s == 18u) put(H.rle_ext[k], 7u);
      }
      H.hdr_bits = pos;
    }
    __syncthreads();
    uint32_t bitpos = H.hdr_bits;
    for (uint32_t k0 = 0; k0 < n_tok; k0 += 64u) {
      const uint32_t k = k0 + ln;
      uint32_t v1 = 0, n1 = 0, v2 = 0, n2 = 0;
      if (k < n_tok) {
        const uint32_t x = tok[k];
        if (x & 0x80000000u) {
          uint32_t sym, eb, ev;
          len_code(((x >> 16) & 0xFFu) + 3u, &sym, &eb, &ev);
          v1 = H.code_l[sym] | (ev << H.len_l[sym]), n1 = H.len_l[sym] + eb;
          dist_code((x & 0xFFFFu) + 1u, &sym, &eb, &ev);
          v2 = H.code_d[sym] | (ev << H.len_d[sym]), n2 = H.len_d[sym] + eb;
        } else {
          v1 = H.code_l[x], n1 = H.len_l[x];
        }
      }
      uint32_t incl = n1 + n2;
      for (uint32_t o = 1; o < 64u; o <<= 1) {
        const uint32_t y = __shfl_up(incl, o);
        if (ln >= o) incl += y;
      }
      const uint32_t at = bitpos + incl - (n1 + n2);
      put_bits(buf, kInWords, at, v1, n1);
      put_bits(buf, kInWords, at + n1, v2, n2);
      bitpos += rl(incl, 63u);
    }
    __syncthreads();
    if (ln == 0) put_bits(buf, kInWords, bitpos, H.code_l[256], H.len_l[256]);
    bitpos += H.len_l[256];
    __syncthreads();
    dyn_bytes = (bitpos + 7u) / 8u;
  }
  // ---- the member: header, deflate data, CRC-32, ISIZE ----
  const bool stored = dyn_bytes >= n + 5u;
  const uint32_t data = stored ? n + 5u : dyn_bytes, size = 18u + data + 8u;
  if (ln == 0) {
    member_header(o, size);
    if (stored) {
      o[18] = 1;  // BFINAL, BTYPE 00
      put_u16(o + 19, n), put_u16(o + 21, ~n & 0xFFFFu);
    }
    put_u32(o + 18 + data, crc), put_u32(o + 22 + data, n);
    sizes[m] = size;
  }
  if (stored) {
    for (uint32_t i = ln; i < n; i += 64u) o[23 + i] = src[i];
  } else {
    for (uint32_t i = ln; i < data; i += 64u) o[18 + i] = b8[i];
  }
}

// One block: exclusive scan of the member sizes (n_members + 1 entries written, the last the total).
__global__ void __launch_bounds__(1024) bgzf_scan_kernel(const unsigned long long *sizes, uint32_t n, unsigned long long *offs) {
  __shared__ unsigned long long part[1024];
  const uint32_t t = threadIdx.x, per = (n + 1023u) / 1024u, a = std::min(n, t * per), b = std::min(n, a + per);
  unsigned long long s = 0;
  for (uint32_t i = a; i < b; ++i) s += sizes[i];
  part[t] = s;
  __syncthreads();
  for (uint32_t o = 1; o < 1024u; o <<= 1) {
    const unsigned long long y = t >= o ? part[t - o] : 0ull;
    __syncthreads();
    part[t] += y;
    __syncthreads();
  }
  unsigned long long run = part[t] - s;
  for (uint32_t i = a; i < b; ++i) offs[i] = run, run += sizes[i];
  if (t == 1023u) offs[n] = part[1023];
}

__global__ void __launch_bounds__(256) bgzf_gather_kernel(const uint8_t *slots, const unsigned long long *offs, uint32_t n_members,
                                                          uint8_t *out) {
  const uint32_t m = blockIdx.x;
  if (m >= n_members) return;
  const uint32_t size = (uint32_t)(offs[m + 1] - offs[m]);
  const uint8_t *s = slots + (size_t)m * kBgzfSlot;
  uint8_t *d = out + offs[m];
  for (uint32_t i = threadIdx.x; i < size; i += 256u) d[i] = s[i];
}

}  // namespace

void bgzf_cut(const uint64_t *rec_off, uint64_t n_rec, uint64_t n, std::vector<uint64_t> *starts) {
  starts->clear();
  uint64_t s = 0;
  while (s < n) {
    starts->push_back(s);
    uint64_t e = s + kBgzfInput;
    if (e >= n) {
      e = n;
    } else if (rec_off) {  // the last record boundary that fits
      const uint64_t *hi = std::upper_bound(rec_off, rec_off + n_rec + 1, e);
      const uint64_t c = *(hi - 1);
      if (c > s) e = c;  // (else one record over kBgzfInput bytes: split)
    }
    s = e;
  }
  if (!starts->empty()) starts->push_back(n);
}

#define BGZF_TRY(expr)                                          \
  do {                                                          \
    hipError_t e_ = (expr);                                     \
    if (e_ != hipSuccess) {                                     \
      if (err) *err = std::string("HIP: ") + hipGetErrorString(e_); \
      return FEM_ERR_HIP;                                       \
    }                                                           \
  } while (0)

int Bgzf::compress(const uint8_t *in, uint64_t n, const std::vector<uint64_t> &starts, int level, hipStream_t stream, uint64_t *len,
                   std::string *err, float *ms) {
  if (level < 0 || level > 1) {
    if (err) *err = "BGZF compression level must be 0 or 1";
    return FEM_ERR_INVALID;
  }
  *len = 0;
  if (n == 0 || starts.size() < 2) return FEM_OK;
  const uint32_t k = (uint32_t)(starts.size() - 1);
  BGZF_TRY(h_total_.ensure(1));
  if (!sizes_ || starts_d_.size() < starts.size()) {  // (all three or none: sizes_ comes last)
    sizes_.release();
    const size_t cap = starts.size() + 1024;
    BGZF_TRY(femb::alloc_all(cap, h_starts_, starts_d_));
    BGZF_TRY(sizes_.ensure(2 * cap));
  }
  BGZF_TRY(slots_.ensure((size_t)k * kBgzfSlot));
  BGZF_TRY(tokens_.ensure((size_t)n + 16));
  BGZF_TRY(out_.ensure((size_t)k * kBgzfSlot));
  for (femb::Event &e : ev_) BGZF_TRY(e.create());
  memcpy(h_starts_, starts.data(), starts.size() * 8);
  BGZF_TRY(hipMemcpyAsync(starts_d_, h_starts_, starts.size() * 8, hipMemcpyHostToDevice, stream));
  unsigned long long *offs = sizes_ + k + 1;
  BGZF_TRY(hipEventRecord(ev_[0], stream));
  hipLaunchKernelGGL(bgzf_member_kernel, dim3(k), dim3(64), 0, stream, in, starts_d_, k, level, tokens_, slots_, sizes_);
  BGZF_TRY(hipGetLastError());
  hipLaunchKernelGGL(bgzf_scan_kernel, dim3(1), dim3(1024), 0, stream, sizes_, k, offs);
  BGZF_TRY(hipGetLastError());
  hipLaunchKernelGGL(bgzf_gather_kernel, dim3(k), dim3(256), 0, stream, slots_, offs, k, out_);
  BGZF_TRY(hipGetLastError());
  BGZF_TRY(hipEventRecord(ev_[1], stream));
  BGZF_TRY(hipMemcpyAsync(h_total_, offs + k, 8, hipMemcpyDeviceToHost, stream));
  BGZF_TRY(hipStreamSynchronize(stream));
  *len = *h_total_;
  if (ms) {
    float t = 0.f;
    if (hipEventElapsedTime(&t, ev_[0], ev_[1]) == hipSuccess) *ms += t;
  }
  return FEM_OK;
}

}  // namespace femz
