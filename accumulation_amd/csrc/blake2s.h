// BLAKE2s-256 (RFC 7693), unkeyed, of ONE block (a message of at most 64 bytes), and the message layout of the transparent
// key derivation "amsm-sample-v1" (include/amsm.h: amsm_bases_sample).  Written once as host + device code: the sampling
// kernels (sample_kernels.h) and the host backend (api_cpu.inc: bases_sample) run this text, so the two cannot drift apart.
// 32-bit adds, xors and rotates only; the message words are taken through the compile-time sigma table, so nothing is indexed
// at run time.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define AMSM_B2_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define AMSM_B2_HD inline
#endif

namespace amsm {
namespace b2s {

AMSM_B2_HD constexpr uint32_t iv(int i) {
  constexpr uint32_t t[8] = {0x6A09E667u, 0xBB67AE85u, 0x3C6EF372u, 0xA54FF53Au, 0x510E527Fu, 0x9B05688Cu, 0x1F83D9ABu, 0x5BE0CD19u};
  return t[i];
}
AMSM_B2_HD constexpr int sigma(int r, int i) {
  constexpr unsigned char t[10][16] = {
      {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
      {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
      {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
      {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
      {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0}};
  return t[r][i];
}
AMSM_B2_HD uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

template <int R, int I>
AMSM_B2_HD void g(uint32_t& a, uint32_t& b, uint32_t& c, uint32_t& d, const uint32_t (&m)[16]) {
  constexpr int s0 = sigma(R, 2 * I), s1 = sigma(R, 2 * I + 1);
  a = a + b + m[s0];
  d = rotr(d ^ a, 16);
  c = c + d;
  b = rotr(b ^ c, 12);
  a = a + b + m[s1];
  d = rotr(d ^ a, 8);
  c = c + d;
  b = rotr(b ^ c, 7);
}
template <int R>
AMSM_B2_HD void rnd(uint32_t (&v)[16], const uint32_t (&m)[16]) {
  g<R, 0>(v[0], v[4], v[8], v[12], m);
  g<R, 1>(v[1], v[5], v[9], v[13], m);
  g<R, 2>(v[2], v[6], v[10], v[14], m);
  g<R, 3>(v[3], v[7], v[11], v[15], m);
  g<R, 4>(v[0], v[5], v[10], v[15], m);
  g<R, 5>(v[1], v[6], v[11], v[12], m);
  g<R, 6>(v[2], v[7], v[8], v[13], m);
  g<R, 7>(v[3], v[4], v[9], v[14], m);
}

// out = BLAKE2s-256 of the first `len` (<= 64) bytes of m (little-endian words, zero beyond len): one final compression
AMSM_B2_HD void hash_block(const uint32_t (&m)[16], uint32_t len, uint32_t (&out)[8]) {
  uint32_t h[8], v[16];
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll
#endif
  for (int i = 0; i < 8; i++) h[i] = iv(i);
  h[0] ^= 0x01010020u;  // digest 32 bytes, no key, fanout 1, depth 1
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll
#endif
  for (int i = 0; i < 8; i++) {
    v[i] = h[i];
    v[8 + i] = iv(i);
  }
  v[12] ^= len;          // t0 (t1 = 0)
  v[14] ^= 0xffffffffu;  // the last block
  rnd<0>(v, m);
  rnd<1>(v, m);
  rnd<2>(v, m);
  rnd<3>(v, m);
  rnd<4>(v, m);
  rnd<5>(v, m);
  rnd<6>(v, m);
  rnd<7>(v, m);
  rnd<8>(v, m);
  rnd<9>(v, m);
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll
#endif
  for (int i = 0; i < 8; i++) out[i] = h[i] ^ v[i] ^ v[8 + i];
}

// ---- amsm-sample-v1 ------------------------------------------------------------------------------------------------------------
// M(i, j, k) = "amsm-sample-v1" || u8 curve_id || u8 domain_len || domain || u64_le(i) || u32_le(j) || u8(k): the part before i
// is the same for a whole call and is laid out once, on the host.
constexpr int SAMPLE_MAX_DOMAIN = 32;
constexpr int SAMPLE_MAX_ATTEMPTS = 256;
struct SamplePrefix {
  uint32_t w[16];  // the prefix bytes as little-endian words, zero beyond them
  uint32_t len;    // 16 + domain_len (<= 48): where u64_le(i) starts
};
inline SamplePrefix sample_prefix(int curve_id, const uint8_t* domain, size_t domain_len) {
  SamplePrefix p;
  uint8_t bytes[64] = {0};
  const char tag[] = "amsm-sample-v1";
  for (int i = 0; i < 14; i++) bytes[i] = (uint8_t)tag[i];
  bytes[14] = (uint8_t)curve_id;
  bytes[15] = (uint8_t)domain_len;
  for (size_t i = 0; i < domain_len && i < (size_t)SAMPLE_MAX_DOMAIN; i++) bytes[16 + i] = domain[i];
  for (int i = 0; i < 16; i++)
    p.w[i] = (uint32_t)bytes[4 * i] | ((uint32_t)bytes[4 * i + 1] << 8) | ((uint32_t)bytes[4 * i + 2] << 16) | ((uint32_t)bytes[4 * i + 3] << 24);
  p.len = 16u + (uint32_t)domain_len;
  return p;
}
// BLAKE2s-256(M(i, j, k)).  The 13 tail bytes start at byte p.len, at any alignment: they are shifted as four words and merged
// by comparisons against the (uniform) word position, not stored through a run-time index.
AMSM_B2_HD void sample_hash(const SamplePrefix& p, uint64_t i, uint32_t j, uint32_t k, uint32_t (&out)[8]) {
  const uint32_t base = p.len >> 2, sh = (p.len & 3u) * 8u;
  const uint32_t t[4] = {(uint32_t)i, (uint32_t)(i >> 32), j, k & 0xffu};
  uint32_t s[5];
  s[0] = t[0] << sh;
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll
#endif
  for (int q = 1; q < 4; q++) s[q] = sh ? ((t[q] << sh) | (t[q - 1] >> (32u - sh))) : t[q];
  s[4] = sh ? (t[3] >> (32u - sh)) : 0u;
  uint32_t m[16];
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll
#endif
  for (int w = 0; w < 16; w++) {
    uint32_t x = p.w[w];
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll
#endif
    for (int q = 0; q < 5; q++) x |= ((uint32_t)w == base + (uint32_t)q) ? s[q] : 0u;
    m[w] = x;
  }
  hash_block(m, p.len + 13u, out);
}

}  // namespace b2s
}  // namespace amsm
