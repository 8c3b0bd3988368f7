// Point validation, host side (include/amsm.h: amsm_points_check): the status of one point straight from the definition -- an
// integer compare with p, on_curve (host_serialize.h) and the full multiplication by the group order r -- which is the host backend's
// implementation and what the kernels of points_check_kernels.h must agree with byte for byte (their subgroup test is a different,
// faster one: two independent implementations); and the argument block of those kernels.
#pragma once
#include <string.h>

#include "curves.h"
#include "host_serialize.h"
#include "msm_types.h"

namespace amsm {
namespace host {

template <class Fq>
inline PointsCheckConsts points_check_consts() {
  using C = typename CurveOf<Fq>::type;
  constexpr int N = HFe<Fq>::N;
  PointsCheckConsts k;
  memset(&k, 0, sizeof(k));
  const HFe<Fq> b = curve_b_mont<Fq>(C::b);
  memcpy(k.b, b.v, 8 * N);
  if constexpr (C::subgroup_check) {
    static_assert(sizeof(C::beta) == 8 * N, "the curve's endomorphism constant (curves.h), one word per limb");
    HFe<Fq> beta;
    memcpy(beta.v, C::beta, 8 * N);
    beta = h_to_mont<Fq>(beta);
    memcpy(k.beta, beta.v, 8 * N);
  }
  return k;
}

// status of the point (x | y Montgomery words as the C ABI gives them, flagged: its infinity byte): the first rule that applies
template <class Fq, class Fr>
inline uint8_t point_status(const u64* xy, bool flagged) {
  using C = typename CurveOf<Fq>::type;
  constexpr int N = HFe<Fq>::N;
  if (flagged) return POINT_VALID;
  HFe<Fq> x, y;
  memcpy(x.v, xy, 8 * N);
  memcpy(y.v, xy + N, 8 * N);
  if (h_is_zero<Fq>(x) && h_is_zero<Fq>(y)) return POINT_VALID;
  if (h_geq_mod<Fq>(x) || h_geq_mod<Fq>(y)) return POINT_NON_CANONICAL;
  if (!on_curve<Fq>(x, y, C::b)) return POINT_OFF_CURVE;
  if constexpr (C::subgroup_check) {
    u64 r[4];
    for (int k = 0; k < 4; k++) r[k] = hmod<Fr>(k);
    if (!hx_is_inf<Fq>(hx_mul<Fq>(hx_from_affine<Fq>(xy, false), r))) return POINT_OFF_SUBGROUP;
  }
  return POINT_VALID;
}

}  // namespace host
}  // namespace amsm
