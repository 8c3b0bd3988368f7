// The keyed scalar stream "amsm-blind-v1" behind amsm_vec_sample (include/amsm.h): blinding vectors of the zero-knowledge proves,
// made where they are used.  The library's own derivation, as "amsm-sample-v1" (blake2s.h) is -- nothing in arkworks corresponds to
// it (the reference takes whatever RngCore the caller hands it).  Written once as host + device code: the kernels of vec_kernels.h
// (k_vec_sample) and the host backend (api_cpu.inc: vec_sample) run this text, so the two cannot drift apart.
//
// Scalar i of stream `stream` under `key` is the first accepted candidate t = 0, 1, .. of
//   M(i, t) = key[32] || "amsm-blind-v1" (13 bytes) || u8 curve_id || u16_le t || u32_le stream || u64_le i          (60 bytes)
//   cand    = BLAKE2s-256(M) read as a little-endian integer, masked to bitlen(r) bits;   accepted iff cand < r
// In b2s::hash_block's message words: 0-7 the key, 8-10 tag bytes 0-11, word 11 = tag[12] | curve_id << 8 | t << 16, word 12 =
// stream, words 13-14 = i, word 15 = 0; every field is word-aligned, so nothing is shifted at run time.
// The mask is the bit length of the curve's r (255, 254 or 253 bits), so a candidate is accepted with probability
// r / 2^bitlen(r) >= 1/2 on every curve (0.500 Pallas and Vesta, 0.906 BLS12-381, 0.756 BN254 and Grumpkin, 0.583 BLS12-377), and
// rejection makes the output exactly uniform in [0, r), given the PRF.
// t stops at MAX_ATTEMPTS = 128: past the cap the value is candidate 127 minus r -- one subtraction suffices, because
// cand < 2^bitlen(r) <= 2 r.  That happens with probability at most 2^-128 per scalar; no test can reach it.
#pragma once
#include "blake2s.h"
#include "fp.h"

namespace amsm {
namespace blind {

constexpr u32 MAX_ATTEMPTS = 128;
struct Key {
  u32 w[8];  // the 32 key bytes as little-endian words; crosses to the device as a kernel argument only
};
inline Key key_words(const uint8_t key[32]) {
  Key k;
  for (int i = 0; i < 8; i++)
    k.w[i] = (u32)key[4 * i] | ((u32)key[4 * i + 1] << 8) | ((u32)key[4 * i + 2] << 16) | ((u32)key[4 * i + 3] << 24);
  return k;
}

// the mask of a candidate's top word: bitlen(r) - 224 low bits
template <class Fr>
AMSM_HD constexpr u32 top_mask() {
  static_assert(Fr::W == 8, "scalar fields of 8 words");
  u32 m = Fr::mod(7);
  m |= m >> 1, m |= m >> 2, m |= m >> 4, m |= m >> 8, m |= m >> 16;
  return m;
}

// Attempt t (< MAX_ATTEMPTS) of scalar i: out = the candidate, true when it is the scalar's value (below r, or the last attempt,
// reduced).  The scalar is the first attempt that returns true; both callers walk t upwards and stop there.
template <class Fr>
AMSM_HD bool attempt(const Key& key, u32 curve_id, u32 stream, u64 i, u32 t, u32 (&out)[8]) {
  static_assert(top_mask<Fr>() >= 0x0fffffffu && Fr::mod(7) > (top_mask<Fr>() >> 1), "the mask is r's own bit length");
  const u32 m[16] = {key.w[0], key.w[1], key.w[2], key.w[3], key.w[4], key.w[5], key.w[6], key.w[7],
                     0x6d736d61u /* "amsm" */, 0x696c622du /* "-bli" */, 0x762d646eu /* "nd-v" */,
                     0x31u /* "1" */ | ((curve_id & 0xffu) << 8) | ((t & 0xffffu) << 16), stream, (u32)i, (u32)(i >> 32), 0u};
  b2s::hash_block(m, 60u, out);
  out[7] &= top_mask<Fr>();
  u32 d[8];
  u32 br = 0;  // d = out - r
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll
#endif
  for (int k = 0; k < 8; k++) {
    const u64 s = (u64)out[k] - Fr::mod(k) - br;
    d[k] = (u32)s;
    br = (u32)(s >> 32) & 1u;
  }
  if (br) return true;  // out < r
  if (t + 1u < MAX_ATTEMPTS) return false;
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll
#endif
  for (int k = 0; k < 8; k++) out[k] = d[k];  // past the cap: cand - r < r
  return true;
}

// scalar i, canonical words
template <class Fr>
AMSM_HD void scalar(const Key& key, u32 curve_id, u32 stream, u64 i, u32 (&out)[8]) {
  for (u32 t = 0; t < MAX_ATTEMPTS; t++)
    if (attempt<Fr>(key, curve_id, stream, i, t, out)) return;
}

}  // namespace blind
}  // namespace amsm
