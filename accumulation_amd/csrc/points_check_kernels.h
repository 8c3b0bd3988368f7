// Validation of caller-supplied points on the device (include/amsm.h: amsm_points_check): one status byte per point, the first
// rule that applies wins --
//     0 valid            flagged infinite (coordinates ignored, as k_apply_inf ignores them), or (0, 0), or none of the below
//     1 non-canonical    the integer in the words of x or of y is >= p (tested on the words as they arrive)
//     2 off the curve    y^2 != x^3 + b
//     3 off the subgroup [r]P != O (curves.h: subgroup_check -- BLS12-381 G1 and BLS12-377 G1; Pallas, Vesta, BN254 G1 and Grumpkin have cofactor 1)
// -- in two kernels, so that the cheap pass does not inherit the ladder's registers:
//   k_points_check_curve     every curve: rules 1 and 2, three multiplications per point over 64 or 96 bytes (memory-shaped: 16-byte
//                            loads as k_points_import makes them).  Writes every status byte.
//   k_points_check_subgroup  BLS12-381, BLS12-377: rule 3 for the points the first kernel left at 0 (the identity apart); every other lane idles.
// Both count the bad points by status into counters[0..2] and keep the smallest bad index in counters[PCHK_FIRST_BAD] (atomics of
// the rare bad lanes only).
//
// The subgroup test is not [r]P.  With z = -0xd201000000010000 on BLS12-381, z = 0x8508c00000000001 on BLS12-377 (r = z^4 - z^2 + 1; only
// z^2 enters, so the sign of z does not; |z|, z^2, their bit lengths and beta are the curve's, curves.h) and phi(x, y) = (beta x, y), beta a primitive
// cube root of unity, phi^2 + phi + 1 = 0 on the whole curve; on G1 phi acts as the scalar -z^2 (for the beta of
// host_points_check.h; G1 is cyclic, so checking the generator settles it).  Hence
//     P in G1   =>   [z^2]P = -phi(P) = (beta x, -y), and [z^2]P != O unless P = O          (complete)
//     [z^2]P = -phi(P)   =>   [z^4]P = phi^2(P), so [z^4 - z^2 + 1]P = (phi^2 + phi + 1)(P) = O   (sound)
// compared projectively on fully reduced values: X == beta x ZZ and Y == -y ZZZ, ZZ != 0.
// Two ladders compute [z^2]P, both over public constant digits (no lane diverges inside them):
//   LADDER 1  one stage over z^2 (128 bits, weight 17): 127 doublings and 16 mixed additions of P; holds one XYZZ value and P
//   LADDER 2  [|z|]([|z|]P) (|z|: 64 bits, weight 6): 126 doublings, 5 mixed and 5 full additions; holds two XYZZ values and P
//   (BLS12-377: z^2 has 127 bits and weight 22 -- 126 doublings and 21 mixed additions; z 64 bits, weight 7 -- 126 doublings, 6 mixed
//   and 6 full additions.)
// Inputs outside the subgroup make intermediates hit O and +-P (points of order 3, 11, 10177; (0, 2), of order 3 with x = 0): every
// addition is one of ec.h's exact-exception forms.  BLS12-377's cofactor is even: (p - 1, 0) has order 2 and (2, 3) order 6, whose
// ladders double a point with Y = 0 mod p -- the one case where ZZ = 0 mod p comes out of a multiplication and not out of
// xyzz_inf(); xyzz_dbl returns the identity's limbs there (ec.h, fp.h: HasTwoTorsion).
#pragma once
#include "curves.h"
#include "ec.h"
#include "msm_types.h"
#include "sample_kernels.h"

namespace amsm {

template <class P, u32 KMAX>
AMSM_DEV Fe<P> fe_canon_k(const Fe<P>& a) {  // tight, value < KMAX p -> canonical (no-op on a saturated field)
  Fe<P> r = a;
  if constexpr (P::UNSAT) u_canon<P, KMAX>(r);
  return r;
}

// words of point i as they arrive: 16-byte loads
template <int W>
AMSM_DEV void point_words_load(const u32* __restrict__ xy, size_t i, u32 (&w)[2 * W]) {
  const uint4* q = reinterpret_cast<const uint4*>(xy + i * (2 * W));
#pragma unroll
  for (int k = 0; k < W / 2; k++) {
    const uint4 v = q[k];
    w[4 * k + 0] = v.x;
    w[4 * k + 1] = v.y;
    w[4 * k + 2] = v.z;
    w[4 * k + 3] = v.w;
  }
}

AMSM_DEV void points_check_report(u32* __restrict__ counters, u32 status, u32 i) {
  atomicAdd(&counters[status - 1u], 1u);
  atomicMin(&counters[PCHK_FIRST_BAD], i);
}

template <class FQD>
__global__ void __launch_bounds__(256)
    k_points_check_curve(const u32* __restrict__ xy, const uint8_t* __restrict__ is_inf, u32 n, uint8_t* __restrict__ status,
                         u32* __restrict__ counters, PointsCheckConsts k) {
  using S = typename SatOf<FQD>::type;  // the C-ABI field: the modulus the words are compared with
  constexpr int W = FQD::W;
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  u32 st = POINT_VALID;
  if (!(is_inf && is_inf[i])) {
    u32 w[2 * W];
    point_words_load<W>(xy, i, w);
    u32 any = 0;
#pragma unroll
    for (int j = 0; j < 2 * W; j++) any |= w[j];
    if (any) {  // (0, 0) is the identity
      u32 bx = 0, by = 0;
#pragma unroll
      for (int j = 0; j < W; j++) {
        (void)__builtin_subc(w[j], S::mod(j), bx, &bx);
        (void)__builtin_subc(w[W + j], S::mod(j), by, &by);
      }
      if (!(bx && by)) {  // a coordinate minus p did not borrow: it is >= p
        st = POINT_NON_CANONICAL;
      } else {
        const Fe<FQD> x = fe_import<FQD>(fe_from_words<FQD>(w)), y = fe_import<FQD>(fe_from_words<FQD>(w + W));  // [< 2p]
        const Fe<FQD> rhs = fe_add_g<FQD>(fe_mul<FQD>(fe_sqr<FQD>(x), x), fe_from_abi<FQD>(k.b));                // [< 2.1p]
        if (!fe_eq<FQD>(fe_canon_k<FQD, 2>(fe_sqr<FQD>(y)), fe_canon_k<FQD, 4>(rhs))) st = POINT_OFF_CURVE;
      }
    }
  }
  status[i] = (uint8_t)st;
  if (st) points_check_report(counters, st, i);
}

// acc = [e]q for the public NBITS-bit constant e (top bit set), by doublings and mixed additions of q
template <class P, int NBITS, class WORD>
AMSM_DEV XYZZ<P> points_check_ladder(const Affine<P>& q, WORD&& word) {
  XYZZ<P> acc = xyzz_from_affine<P>(q);
#pragma unroll 1
  for (int bit = NBITS - 2; bit >= 0; bit--) {
    acc = xyzz_dbl<P>(acc);
    if ((word(bit >> 5) >> (bit & 31)) & 1u) xyzz_madd<P>(acc, q);
  }
  return acc;
}

template <class FQD, int LADDER>
__global__ void __launch_bounds__(256)
    k_points_check_subgroup(const u32* __restrict__ xy, const uint8_t* __restrict__ is_inf, u32 n, uint8_t* __restrict__ status,
                            u32* __restrict__ counters, PointsCheckConsts k) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (status[i] != POINT_VALID || (is_inf && is_inf[i])) return;
  Affine<FQD> p = affine_load<FQD>(xy, i);  // (canonical words: the first kernel said so)
  if (affine_is_inf<FQD>(p)) return;
  p = affine_import<FQD>(p);
  p.x = fe_canon<FQD>(p.x);
  p.y = fe_canon<FQD>(p.y);
  using C = typename CurveOf<typename SatOf<FQD>::type>::type;  // |z|, z^2 and their bit lengths: the curve's (curves.h)
  XYZZ<FQD> acc;
  if constexpr (LADDER == 1) {
    acc = points_check_ladder<FQD, C::z2_bits>(p, [](int w) { return C::z2_word(w); });
  } else {
    const XYZZ<FQD> q = points_check_ladder<FQD, C::z_bits>(p, [](int w) { return C::z_word(w); });
    acc = q;
#pragma unroll 1
    for (int bit = C::z_bits - 2; bit >= 0; bit--) {
      acc = xyzz_dbl<FQD>(acc);
      if ((C::z_word(bit >> 5) >> (bit & 31)) & 1u) xyzz_add<FQD>(acc, q);
    }
  }
  // [z^2]P == (beta x, -y)?  X == beta x ZZ, Y + y ZZZ == 0, ZZ != 0, on canonical limbs
  bool ok = !xyzz_is_inf<FQD>(acc);
  const Fe<FQD> bx = fe_mul<FQD>(fe_mul<FQD>(fe_from_abi<FQD>(k.beta), p.x), acc.zz);
  ok = ok && fe_eq<FQD>(fe_canon_k<FQD, 8>(acc.x), fe_canon_k<FQD, 2>(bx));
  const Fe<FQD> ny = fe_sub_k<FQD, 2>(fe_zero<FQD>(), fe_mul<FQD>(p.y, acc.zzz));  // [<= 2p]
  ok = ok && fe_eq<FQD>(fe_canon_k<FQD, 4>(acc.y), fe_canon_k<FQD, 4>(ny));
  if (!ok) {
    status[i] = (uint8_t)POINT_OFF_SUBGROUP;
    points_check_report(counters, POINT_OFF_SUBGROUP, i);
  }
}

}  // namespace amsm
