// Transparent committer keys, host side: the derivation "amsm-sample-v1" of include/amsm.h (amsm_bases_sample) on the host field
// arithmetic -- the host backend's implementation, and the definition the sampling kernels (sample_kernels.h) are bit-identical
// to -- and the per-field constants those kernels take as arguments.  Every constant is computed here from the modulus (the odd
// part t of p - 1, its exponents, a 2^s-th root of unity, (p - 1) / 2), as h_sqrt computes its own; none is a pasted literal.
#pragma once
#include <string.h>

#include "blake2s.h"
#include "curves.h"
#include "host_serialize.h"
#include "msm_types.h"

namespace amsm {
namespace host {

template <class Fq>
struct SampleField {
  static constexpr int N = HFe<Fq>::N;
  int s = 0;              // p - 1 = 2^s t, t odd
  u64 t[N], t_half[N];    // t; (t - 1) / 2
  u64 p_quarter[N];       // (p + 1) / 4   (the square root exponent when p = 3 mod 4)
  u64 half[N];            // (p - 1) / 2
  HFe<Fq> root;           // z^t for the smallest non-residue z = 2, 3, ...: a primitive 2^s-th root of unity (Montgomery)
  SampleField() {
    for (int i = 0; i < N; i++) t[i] = hmod<Fq>(i);
    t[0] -= 1;
    shr1(t, half);
    while (!(t[0] & 1)) {
      shr1(t, t);
      s++;
    }
    shr1(t, t_half);
    u64 p1[N];
    u128 c = 1;
    for (int i = 0; i < N; i++) {
      c += hmod<Fq>(i);
      p1[i] = (u64)c;
      c >>= 64;
    }
    shr1(p1, p_quarter);
    shr1(p_quarter, p_quarter);
    HFe<Fq> z = h_one<Fq>();
    for (;;) {
      z = h_add<Fq>(z, h_one<Fq>());
      if (!h_eq<Fq>(h_pow<Fq>(z, half, N), h_one<Fq>())) break;
    }
    root = h_pow<Fq>(z, t, N);
  }
  static void shr1(const u64* a, u64* o) {
    for (int i = 0; i < N; i++) o[i] = (a[i] >> 1) | (i + 1 < N ? a[i + 1] << 63 : 0);
  }
  static int bit_len(const u64* a) {
    for (int i = N - 1; i >= 0; i--)
      if (a[i]) return 64 * i + 64 - __builtin_clzll(a[i]);
    return 0;
  }
  static const SampleField& get() {
    static const SampleField f;
    return f;
  }
};

// the kernels' argument block for this curve and domain (msm_types.h: SampleConsts; field elements as C-ABI Montgomery words)
template <class Fq>
inline SampleConsts sample_consts(const uint8_t* domain, size_t domain_len) {
  using C = typename CurveOf<Fq>::type;
  constexpr int N = HFe<Fq>::N;
  const SampleField<Fq>& f = SampleField<Fq>::get();
  SampleConsts k;
  memset(&k, 0, sizeof(k));
  k.prefix = b2s::sample_prefix(C::id, domain, domain_len);
  const HFe<Fq> b = curve_b_mont<Fq>(C::b);
  memcpy(k.b, b.v, 8 * N);
  for (int i = 0; i < N; i++) {
    const u64 r2 = hr2<Fq>(i);
    memcpy(k.r2 + 2 * i, &r2, 8);
  }
  memcpy(k.root, f.root.v, 8 * N);
  memcpy(k.half, f.half, 8 * N);
  const u64* e = f.s == 1 ? f.p_quarter : f.t_half;
  memcpy(k.exp, e, 8 * N);
  k.exp_bits = (u32)SampleField<Fq>::bit_len(e);
  k.two_adicity = (u32)f.s;
  memcpy(k.cofactor, C::cofactor, 16);
  u64 cof[N] = {0};
  cof[0] = C::cofactor[0];
  cof[1] = C::cofactor[1];
  k.cofactor_bits = (u32)SampleField<Fq>::bit_len(cof);
  return k;
}

// G_i from attempt `j0` on (j0 = 0: the definition).  false: every attempt up to 255 was rejected.  *j_out: the attempt that won.
template <class Fq>
inline bool sample_point(const b2s::SamplePrefix& prefix, u64 index, u32 j0, u64* xy_mont, u32* j_out) {
  using C = typename CurveOf<Fq>::type;
  constexpr int N = HFe<Fq>::N;
  constexpr int bits = h_modulus_bits<Fq>();
  const HFe<Fq> b = curve_b_mont<Fq>(C::b);
  for (u32 j = j0; j < (u32)b2s::SAMPLE_MAX_ATTEMPTS; j++) {
    u32 d[16];
    {
      u32 h0[8], h1[8];
      b2s::sample_hash(prefix, index, j, 0, h0);
      b2s::sample_hash(prefix, index, j, 1, h1);
      memcpy(d, h0, 32);
      memcpy(d + 8, h1, 32);
    }
    const bool sign = (d[15] >> 31) != 0;
    HFe<Fq> xi = h_zero<Fq>();
    memcpy(xi.v, d, 8 * N);  // little-endian host
    if (bits % 64) xi.v[N - 1] &= (1ull << (bits % 64)) - 1;
    if (h_geq_mod<Fq>(xi)) continue;
    const HFe<Fq> x = h_to_mont<Fq>(xi);
    const HFe<Fq> rhs = h_add<Fq>(h_mul<Fq>(h_sqr<Fq>(x), x), b);
    HFe<Fq> y;
    if (h_is_zero<Fq>(rhs) || !h_sqrt<Fq>(rhs, &y)) continue;
    const HFe<Fq> ny = h_neg<Fq>(y);
    if (h_gt_canonical<Fq>(y, ny) != sign) y = ny;
    memcpy(xy_mont, x.v, 8 * N);
    memcpy(xy_mont + N, y.v, 8 * N);
    if (C::cofactor[0] != 1 || C::cofactor[1] != 0) {
      const u64 k[4] = {C::cofactor[0], C::cofactor[1], 0, 0};
      const HXYZZ<Fq> q = hx_mul<Fq>(hx_from_affine<Fq>(xy_mont, false), k);
      if (hx_is_inf<Fq>(q)) continue;
      uint8_t inf = 0;
      hx_to_affine<Fq>(q, xy_mont, &inf);
    }
    if (j_out) *j_out = j;
    return true;
  }
  return false;
}

}  // namespace host
}  // namespace amsm
