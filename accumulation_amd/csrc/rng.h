// Synthetic input streams shared by device kernels and the host backend (counter-based splitmix64).
//   rng_scalar      the MULTIPLIER stream: 254-bit integers k_i, only used for G_i = k_i G (any fixed set of distinct
//                   subgroup points serves as a committer key).  On BN254 and Grumpkin (r < 2^254) a k_i may exceed
//                   r: harmless, k_i G is taken over the integers (the oracle does the same) and equals (k_i mod r) G
//   rng_scalar_fr   the SCALAR stream of amsm_vec_random: uniform in [0, r) of the curve's scalar field (round 6: the
//                   254-bit stream never produced the 45 % of BLS12-381 scalars that have bit 254 set); canonical on BLS12-377's
//                   253-bit field through a reduced fallback (below)
#pragma once
#include "fp.h"

namespace amsm {

// ---------------------------------------------------------------------------------------------
// Synthetic scalar stream (identical to oracle/pyref.py:rng_word / rng_scalar).
// ---------------------------------------------------------------------------------------------
AMSM_HD u64 rng_mix64(u64 z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
AMSM_HD u64 rng_word(u64 seed, u64 j) {
  return rng_mix64(seed * 0xD1342543DE82EF95ull + j * 0x9E3779B97F4A7C15ull + 0x632BE59BD9B4E019ull);
}
AMSM_HD void rng_scalar(u64 seed, u64 i, u32 out[8]) {
  for (int k = 0; k < 4; k++) {
    u64 w = rng_word(seed, 4 * i + k);
    if (k == 3) w &= (1ull << 62) - 1;
    out[2 * k] = (u32)w;
    out[2 * k + 1] = (u32)(w >> 32);
  }
}

// Uniform in [0, r): candidate t of scalar i = words (t << 40) + 4 i .. + 3 masked to 255 bits (the scalar fields have 254- or
// 255-bit moduli), the first candidate below r wins (rejection sampling: exactly uniform; acceptance 0.50 Pallas and Vesta, 0.906
// BLS12-381, 0.378 BN254 and Grumpkin).  After 64 rejections candidate 63 with bit 254 cleared: below 2^254 < r on the 255-bit fields
// (probability < 2^-64); on BN254 and Grumpkin (r < 2^254) the fallback is reached with probability 0.622^64 < 10^-13 per scalar and is no
// longer guaranteed below r -- the oracle's rule is kept literally (oracle/pyref.py: rng_fr), not repaired on one side only.
// The checkers restate it (pyref.py: rng_fr; the C restatement: ark_rng_scalars_fr; tools/ark_vectors/src/main.rs: rng_frs).
// A modulus of 253 bits or fewer (BLS12-377: acceptance 0.146, so the fallback is reached with probability 0.854^64 = 4.1e-5 per
// scalar -- five times among the first 2^16 scalars of seed 1) gets a CANONICAL fallback: the value above reduced mod r by at most
// three conditional subtractions (2^254 / r < 3.43), i.e. pyref.rng_fr(..) % r.  The branch is taken on the modulus length at compile
// time; the 254- and 255-bit fields keep the literal rule bit for bit.
template <class Fr>
AMSM_HD constexpr bool rng_fr_reduces_fallback() { return Fr::mod(7) < (1u << 29); }  // r < 2^253
template <class Fr>
AMSM_HD void rng_scalar_fr(u64 seed, u64 i, u32 out[8]) {
  static_assert(Fr::W == 8, "scalar fields of 8 words (254 or 255 bits)");
  for (u64 t = 0; t < 64; t++) {
    for (int k = 0; k < 4; k++) {
      u64 w = rng_word(seed, (t << 40) + 4 * i + k);
      if (k == 3) w &= (1ull << 63) - 1;
      out[2 * k] = (u32)w;
      out[2 * k + 1] = (u32)(w >> 32);
    }
    bool below = false;  // out < r ?
#pragma unroll
    for (int k = 7; k >= 0; k--) {
      if (out[k] != Fr::mod(k)) {
        below = out[k] < Fr::mod(k);
        break;
      }
    }
    if (below) return;
  }
  out[7] &= 0x3fffffffu;
  if constexpr (rng_fr_reduces_fallback<Fr>()) {
    static_assert(Fr::mod(7) >= 0x10000000u, "three subtractions reduce a 254-bit value: r >= 2^252, so 2^254 <= 4 r");
    for (int s = 0; s < 3; s++) {
      u32 d[8];
      u64 br = 0;
      for (int k = 0; k < 8; k++) {
        const u64 t = (u64)out[k] - Fr::mod(k) - br;
        d[k] = (u32)t;
        br = (t >> 32) & 1u;
      }
      if (br) break;  // out < r
      for (int k = 0; k < 8; k++) out[k] = d[k];
    }
  }
}

}  // namespace amsm
