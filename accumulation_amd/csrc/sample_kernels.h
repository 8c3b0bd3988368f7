// Transparent committer keys on the device: G_i by BLAKE2s try-and-increment ("amsm-sample-v1", include/amsm.h:
// amsm_bases_sample; host_sample.h: sample_point is the same derivation on the host and the definition).
//
// Per index the work is a run of attempts j = 0, 1, ...: a hash gives a candidate x; x >= p is rejected for the price of the hash
// (every other candidate on the Pasta curves), x^3 + b not a square for the price of a field exponentiation (every other of the
// rest).  A lane that simply looped until it found its point would hold its wave for the unluckiest of 64 lanes -- about three
// times the mean number of exponentiations.  So the work is cut in two kernels:
//   k_sample_search   one PASS over a list of unsolved indices.  A lane spins on the cheap rejection until it holds a candidate
//                     x < p, then the wave runs ONE square test together.  Winners leave their attempt in jwin[] and what the test
//                     computed in their slot of the key table; losers append (index, next attempt) to the next pass's list.  Each
//                     pass halves the list; the host launches passes while the list is long and lets the last few thousand indices
//                     loop per lane (max_tests = SAMPLE_MAX_ATTEMPTS).
//   k_sample_finish   every index, once: the rest of the square root (Tonelli-Shanks on the 2-adic part, from the search's
//                     rhs^((t+1)/2) and rhs^t), the choice of the root by the hash's sign bit, the cofactor multiplication where the
//                     curve has one, and the store in the key's device radix.
// The result does not depend on the schedule: an index only ever advances through its own attempts in order and stops at the first
// one that passes, in whichever pass that happens; every loop is bounded by SAMPLE_MAX_ATTEMPTS.
//
// The arithmetic runs on the device field forms (fp.h / fpu.h): on the unsaturated fields a product of two values below 2p is a
// tight value below 1.1p, so chains of products and squarings need no care; equality is tested on canonical limbs (fe_canon).
#pragma once
#include "blake2s.h"
#include "curves.h"
#include "ec.h"
#include "msm_types.h"

namespace amsm {

template <class P>
AMSM_DEV Fe<P> fe_canon(const Fe<P>& a) {  // tight, value < 2p -> canonical (no-op on a saturated field)
  Fe<P> r = a;
  if constexpr (P::UNSAT) u_canon<P, 2>(r);
  return r;
}
template <class P>
AMSM_DEV bool fe_is_one(const Fe<P>& a) {  // a < 2p
  return fe_eq<P>(fe_canon<P>(a), fe_one<P>());
}
template <class P>
AMSM_DEV Fe<P> fe_add_g(const Fe<P>& a, const Fe<P>& b) {  // unsat: tight, value a + b
  if constexpr (P::UNSAT) return u_add<P>(a, b);
  else return fe_add<P>(a, b);
}
template <class P>
AMSM_DEV Fe<P> fe_from_abi(const u32* w) {  // C-ABI Montgomery words (kernel arguments) -> device element
  u32 t[P::W];
#pragma unroll
  for (int i = 0; i < P::W; i++) t[i] = w[i];
  return fe_import<P>(fe_from_words<P>(t));
}
// canonical integer words (< p) -> device element: the import reads them as x / R, the product by the element R puts that right
template <class P>
AMSM_DEV Fe<P> fe_from_int(const u32 (&xw)[P::W], const SampleConsts& k) {
  return fe_mul<P>(fe_import<P>(fe_from_words<P>(xw)), fe_from_abi<P>(k.r2));
}
// device element (< 2p) -> canonical integer words
template <class P>
AMSM_DEV void fe_to_int(const Fe<P>& a, u32 (&w)[P::W]) {
  Fe<P> o = fe_zero<P>();
  o.v[0] = 1;
  const Fe<P> c = fe_canon<P>(fe_mul<P>(a, o));
  if constexpr (P::UNSAT) {
    u_pack<P>(c, w);
  } else {
#pragma unroll
    for (int i = 0; i < P::W; i++) w[i] = c.v[i];
  }
}

// a^e for a public exponent (uniform words e, nbits of them used): fixed WIN-bit windows over a table of a^1 .. a^(2^WIN - 1) held in
// registers; the digit is uniform, so the table entry is picked by selects and a zero digit skips its multiplication for the
// whole wave.  a < 3p.
template <class P, int WIN>
AMSM_DEV Fe<P> fe_pow(const Fe<P>& a, const u32* e, u32 nbits) {
  static_assert(32 % WIN == 0, "a digit never straddles two words");
  constexpr int T = (1 << WIN) - 1;
  Fe<P> tab[T];
  tab[0] = a;
#pragma unroll
  for (int i = 1; i < T; i++) tab[i] = fe_mul<P>(tab[i - 1], a);
  Fe<P> r = fe_one<P>();
  for (int d = (int)((nbits + WIN - 1) / WIN) - 1; d >= 0; d--) {
#pragma unroll
    for (int w = 0; w < WIN; w++) r = fe_sqr<P>(r);
    const u32 dig = (e[(d * WIN) >> 5] >> ((d * WIN) & 31)) & (u32)T;
    if (dig) {
      Fe<P> s = tab[0];
#pragma unroll
      for (int i = 1; i < T; i++) s = fe_sel<P>(dig == (u32)(i + 1), tab[i], s);
      r = fe_mul<P>(r, s);
    }
  }
  return r;
}

template <class FQD>
struct SampleShape {
  using S = typename SatOf<FQD>::type;  // the C-ABI field: canonical words, the modulus
  using C = typename CurveOf<S>::type;
  static constexpr int W = FQD::W;
  static constexpr bool SQRT_DIRECT = (S::mod(0) & 3u) == 3u;  // p = 3 mod 4: y = rhs^((p + 1) / 4)
  static constexpr bool HAS_COFACTOR = C::cofactor[0] != 1 || C::cofactor[1] != 0;
  // 2-bit windows: a table of three powers.  Four bits would save 3 % of the Pasta exponentiation on paper (its exponent has a run of
  // 95 zero bits, which costs no multiplication at any width) and 7 % of the BLS12-381 one, and their 15 entries (135 / 210
  // registers) spill: the Pallas search kernel compiled to 245 VGPRs and 544 bytes of scratch per lane with them
  static constexpr int POW_WIN = 2;
  AMSM_HD static constexpr u32 top_mask() {  // x = v mod 2^bits: the bits of the top word
    u32 t = S::mod(W - 1), m = 0;
    while (t) {
      m = (m << 1) | 1u;
      t >>= 1;
    }
    return m;
  }
};

// candidate of (index, attempt j): the canonical words of x and the sign bit (bit 511 of the two digests).  false: x >= p.
// The second digest is only computed when the field is wider than the first one or the caller wants the sign.
template <class FQD, bool WANT_SIGN>
AMSM_DEV bool sample_candidate(const SampleConsts& k, u64 index, u32 j, u32 (&xw)[FQD::W], bool* sign) {
  using SH = SampleShape<FQD>;
  constexpr int W = SH::W;
  u32 h0[8];
  b2s::sample_hash(k.prefix, index, j, 0u, h0);
#pragma unroll
  for (int i = 0; i < (W < 8 ? W : 8); i++) xw[i] = h0[i];
  if constexpr (W > 8 || WANT_SIGN) {
    u32 h1[8];
    b2s::sample_hash(k.prefix, index, j, 1u, h1);
#pragma unroll
    for (int i = 8; i < W; i++) xw[i] = h1[i - 8];
    if (sign) *sign = (h1[7] >> 31) != 0u;
  }
  xw[W - 1] &= SH::top_mask();
  u32 br = 0;
#pragma unroll
  for (int i = 0; i < W; i++) (void)__builtin_subc(xw[i], SH::S::mod(i), br, &br);
  return br != 0u;  // x - p borrowed: x < p
}

template <class FQD>
__global__ void __launch_bounds__(256)
    k_sample_search(u32* __restrict__ table, u32* __restrict__ jwin, const u64* __restrict__ pend_in, u32 n_in, u64* __restrict__ pend_out,
                    u32* __restrict__ counters, SampleConsts k, u64 first, u32 max_tests) {
  using SH = SampleShape<FQD>;
  const u32 g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_in) return;
  u32 t = g, j = 0;
  if (pend_in) {
    const u64 e = pend_in[g];
    t = (u32)e;
    j = (u32)(e >> 32);
  }
  const u64 index = first + t;
  bool done = false;
  for (u32 tests = 0; tests < max_tests; tests++) {
    // the cheap rejection, per lane: until this lane holds an x < p (or has used up its attempts)
    u32 xw[SH::W];
    bool have = false;
    while (j < (u32)b2s::SAMPLE_MAX_ATTEMPTS) {
      have = sample_candidate<FQD, false>(k, index, j, xw, nullptr);
      if (have) break;
      j++;
    }
    if (!have) break;
    // the square test, the wave together
    const Fe<FQD> x = fe_from_int<FQD>(xw, k);
    const Fe<FQD> rhs = fe_add_g<FQD>(fe_mul<FQD>(fe_sqr<FQD>(x), x), fe_from_abi<FQD>(k.b));  // [< 2.1p]
    Affine<FQD> keep;
    bool ok;
    if constexpr (SH::SQRT_DIRECT) {
      const Fe<FQD> y = fe_pow<FQD, SH::POW_WIN>(rhs, k.exp, k.exp_bits);
      ok = fe_is_zero_mod<FQD, 8>(fe_sub_k<FQD, 4>(fe_sqr<FQD>(y), rhs)) && !fe_is_zero_mod<FQD, 4>(rhs);
      keep.x = x;
      keep.y = y;
    } else {
      // w = rhs^((t-1)/2): rhs w = rhs^((t+1)/2), rhs w^2 = rhs^t =: b, whose order divides 2^s; rhs is a non-zero square exactly
      // when it divides 2^(s-1) (rhs = 0 gives b = 0, never one)
      const Fe<FQD> w = fe_pow<FQD, SH::POW_WIN>(rhs, k.exp, k.exp_bits);
      keep.x = fe_mul<FQD>(rhs, w);
      keep.y = fe_mul<FQD>(keep.x, w);
      Fe<FQD> b2 = keep.y;
      for (u32 i = 1; i < k.two_adicity; i++) b2 = fe_sqr<FQD>(b2);
      ok = fe_is_one<FQD>(b2);
    }
    if (ok) {
      affine_store<FQD>(table, t, keep);
      jwin[t] = j;
      done = true;
      break;
    }
    j++;
  }
  if (!done) {
    if (j >= (u32)b2s::SAMPLE_MAX_ATTEMPTS) {
      atomicAdd(&counters[SAMPLE_CNT_EXHAUSTED], 1u);
    } else {
      const u32 slot = atomicAdd(&counters[SAMPLE_CNT_PENDING], 1u);  // (slot < n_in: one per lane of this pass)
      pend_out[slot] = ((u64)j << 32) | t;
    }
  }
}

template <class FQD>
__global__ void __launch_bounds__(256)
    k_sample_finish(u32* __restrict__ table, u32* __restrict__ jwin, u32 n, u32* __restrict__ counters, SampleConsts k, u64 first) {
  using SH = SampleShape<FQD>;
  constexpr int W = SH::W;
  const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const u32 j = jwin[t];
  const Affine<FQD> kept = affine_load<FQD>(table, t);
  u32 xw[W];
  bool sign = false;
  (void)sample_candidate<FQD, true>(k, first + t, j, xw, &sign);
  Affine<FQD> p;
  if constexpr (SH::SQRT_DIRECT) {
    p = kept;
  } else {
    // Tonelli-Shanks from x = rhs^((t+1)/2), b = rhs^t, c a primitive 2^s-th root of unity: x^2 = rhs b throughout, and b's order
    // falls with every round
    Fe<FQD> x = kept.x, b = kept.y, c = fe_from_abi<FQD>(k.root);
    u32 m = k.two_adicity;
    for (u32 round = 0; round < k.two_adicity && !fe_is_one<FQD>(b); round++) {
      u32 i = 1;
      Fe<FQD> b2 = fe_sqr<FQD>(b);
      while (i < m && !fe_is_one<FQD>(b2)) {
        b2 = fe_sqr<FQD>(b2);
        i++;
      }
      if (i >= m) break;  // (not a square: the search does not store one)
      Fe<FQD> e = c;
      for (u32 q = 0; q + i + 1 < m; q++) e = fe_sqr<FQD>(e);
      x = fe_mul<FQD>(x, e);
      c = fe_sqr<FQD>(e);
      b = fe_mul<FQD>(b, c);
      m = i;
    }
    p.x = fe_from_int<FQD>(xw, k);
    p.y = fe_canon<FQD>(x);
  }
  // the root with (y > p - y) == sign, on canonical integers
  u32 yw[W];
  fe_to_int<FQD>(p.y, yw);
  bool larger = false, decided = false;
#pragma unroll
  for (int i = W - 1; i >= 0; i--) {
    const u32 hw = k.half[i];
    larger = (!decided && yw[i] > hw) ? true : larger;
    decided = decided || yw[i] != hw;
  }
  const bool negate = larger != sign;
  if constexpr (SH::HAS_COFACTOR) {
    const Affine<FQD> q = affine_neg_if<FQD>(p, negate);
    XYZZ<FQD> acc = xyzz_inf<FQD>();
    for (int bit = (int)k.cofactor_bits - 1; bit >= 0; bit--) {
      acc = xyzz_dbl<FQD>(acc);
      if ((k.cofactor[bit >> 5] >> (bit & 31)) & 1u) xyzz_madd<FQD>(acc, q);
    }
    if (xyzz_is_inf<FQD>(acc)) {  // a point of the cofactor's torsion: this attempt is rejected too; the host takes the index over
      jwin[t] = j | 0x80000000u;
      atomicAdd(&counters[SAMPLE_CNT_IDENTITY], 1u);
    }
    affine_store<FQD>(table, t, xyzz_to_affine<FQD>(acc));
  } else {
    if (negate) p.y = fe_sub_k<FQD, 2>(fe_zero<FQD>(), p.y);  // p - y (unsat: 2p - y, canonical once stored)
    affine_store<FQD>(table, t, p);
  }
}

}  // namespace amsm
