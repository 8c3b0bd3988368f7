// The curves the library knows, in ONE table: curve id (include/amsm.h) -> base / scalar field packs (fp.h), b of
// y^2 = x^3 + b, the generator, and whether deserialisation checks the prime-order subgroup.  (The wrappers' own per-curve
// numbers -- limbs, IPA fold thresholds -- are include/amsm.hpp: curve_info and accumulation_amd/ipa_pc.py: IPA_FOLD.)
// Every entry point that takes a curve id or a context reaches its templates through with_curve(); an id that is not
// in the table is refused there, with AMSM_E_INVALID_ARG (or the entry point's own "unknown" value).
#pragma once
#include <type_traits>
#include <vector>

#include "../../include/amsm.h"
#include "host_field.h"

namespace amsm {

struct PallasCurve {  // ark-pallas 0.2: y^2 = x^3 + 5, cofactor 1
  using Fq = PallasFq;
  using Fr = PallasFr;
  static constexpr int id = AMSM_PALLAS;
  static constexpr int b = 5;
  static constexpr bool subgroup_check = false;
  static constexpr u64 gx[4] = {0x992d30ed00000000ull, 0x224698fc094cf91bull, 0, 0x4000000000000000ull};  // -1
  static constexpr u64 gy[4] = {2, 0, 0, 0};
  static constexpr u64 cofactor[2] = {1, 0};
};
struct Bls12381Curve {  // ark-bls12-381 0.2 G1: y^2 = x^3 + 4, cofactor != 1
  using Fq = Bls12381Fq;
  using Fr = Bls12381Fr;
  static constexpr int id = AMSM_BLS12_381_G1;
  static constexpr int b = 4;
  static constexpr bool subgroup_check = true;
  static constexpr u64 gx[6] = {0xfb3af00adb22c6bbull, 0x6c55e83ff97a1aefull, 0xa14e3a3f171bac58ull,
                                0xc3688c4f9774b905ull, 0x2695638c4fa9ac0full, 0x17f1d3a73197d794ull};
  static constexpr u64 gy[6] = {0x0caa232946c5e7e1ull, 0xd03cc744a2888ae4ull, 0x00db18cb2c04b3edull,
                                0xfcf5e095d5d00af6ull, 0xa09e30ed741d8ae4ull, 0x08b3f481e3aaa0f1ull};
  static constexpr u64 cofactor[2] = {0x8c00aaab0000aaabull, 0x396c8c005555e156ull};  // #E(Fq) / r
  // the subgroup test (points_check_kernels.h): |z| = 0xd201000000010000 (z is negative; the test only uses z^2), z^2, and the
  // primitive cube root of unity beta (a canonical integer) for which phi(x, y) = (beta x, y) is -[z^2] on G1
  static constexpr int z_bits = 64, z2_bits = 128;
  AMSM_TABLE(z_word, 2, 0x00010000u, 0xd2010000u)
  AMSM_TABLE(z2_word, 4, 0x00000000u, 0x00000001u, 0x0001a402u, 0xac45a401u)
  static constexpr u64 beta[6] = {0x2e01fffffffefffeull, 0xde17d813620a0002ull, 0xddb3a93be6f89688ull,
                                  0xba69c6076a0f77eaull, 0x5f19672fdf76ce51ull, 0};
};
struct VestaCurve {  // ark-vesta 0.2: y^2 = x^3 + 5, cofactor 1; Fq = Pallas Fr, Fr = Pallas Fq
  using Fq = VestaFq;
  using Fr = VestaFr;
  static constexpr int id = AMSM_VESTA;
  static constexpr int b = 5;
  static constexpr bool subgroup_check = false;
  static constexpr u64 gx[4] = {0x8c46eb2100000000ull, 0x224698fc0994a8ddull, 0, 0x4000000000000000ull};  // -1
  static constexpr u64 gy[4] = {2, 0, 0, 0};
  static constexpr u64 cofactor[2] = {1, 0};
};

struct Bn254Curve {  // ark-bn254 G1 (alt_bn128): y^2 = x^3 + 3, cofactor 1, generator (1, 2)
  using Fq = Bn254Fq;
  using Fr = Bn254Fr;
  static constexpr int id = AMSM_BN254_G1;
  static constexpr int b = 3;
  static constexpr bool subgroup_check = false;
  static constexpr u64 gx[4] = {1, 0, 0, 0};
  static constexpr u64 gy[4] = {2, 0, 0, 0};
  static constexpr u64 cofactor[2] = {1, 0};
};

struct GrumpkinCurve {  // ark-grumpkin: y^2 = x^3 - 17, cofactor 1; Fq = BN254 Fr, Fr = BN254 Fq (the other half of that cycle)
  using Fq = GrumpkinFq;
  using Fr = GrumpkinFr;
  static constexpr int id = AMSM_GRUMPKIN;
  static constexpr int b = -17;  // host_serialize.h: curve_b_mont gives q - 17
  static constexpr bool subgroup_check = false;
  static constexpr u64 gx[4] = {1, 0, 0, 0};
  static constexpr u64 gy[4] = {0x833fc48d823f272cull, 0x2d270d45f1181294ull, 0xcf135e7506a45d63ull, 0x0000000000000002ull};  // y^2 = -16
  static constexpr u64 cofactor[2] = {1, 0};
};

// ark-bls12-377 G1: y^2 = x^3 + 1, z = 0x8508c00000000001 (positive), r = z^4 - z^2 + 1 (253 bits), cofactor (z - 1)^2 / 3 =
// 0x170b5d44300000000000000000000000: EVEN (divisible by 2^92), so the curve has points of order 2 (y = 0: (p - 1, 0)) and 6
// ((2, 3)) beside (0, 1) of order 3 -- the group law meets y = 0 here and nowhere else (fp.h: HasTwoTorsion)
struct Bls12377Curve {
  using Fq = Bls12377Fq;
  using Fr = Bls12377Fr;
  static constexpr int id = AMSM_BLS12_377_G1;
  static constexpr int b = 1;
  static constexpr bool subgroup_check = true;
  static constexpr u64 gx[6] = {0xeab9b16eb21be9efull, 0xd5481512ffcd394eull, 0x188282c8bd37cb5cull,
                                0x85951e2caa9d41bbull, 0xc8fc6225bf87ff54ull, 0x008848defe740a67ull};
  static constexpr u64 gy[6] = {0xfd82de55559c8ea6ull, 0xc2fe3d3634a9591aull, 0x6d182ad44fb82305ull,
                                0xbd7fb348ca3e52d9ull, 0x1f674f5d30afeec4ull, 0x01914a69c5102effull};
  static constexpr u64 cofactor[2] = {0, 0x170b5d4430000000ull};  // #E(Fq) / r
  // the subgroup test: z (64 bits, weight 7), z^2 (127 bits, weight 22) and the beta with [z^2]P = (beta x, -y) on G1
  static constexpr int z_bits = 64, z2_bits = 127;
  AMSM_TABLE(z_word, 2, 0x00000001u, 0x8508c000u)
  AMSM_TABLE(z2_word, 4, 0x00000001u, 0x0a118000u, 0x90000001u, 0x452217ccu)
  static constexpr u64 beta[6] = {0xffffffffffffffffull, 0xd1e945779fffffffull, 0x59064ee822fb5bffull,
                                  0xb8882a75cc9bc8e3ull, 0xbc8756ba8f8c524eull, 0x01ae3a4617c510eaull};
};

// base field pack -> its curve
template <class Fq>
struct CurveOf;
template <>
struct CurveOf<PallasFq> {
  using type = PallasCurve;
};
template <>
struct CurveOf<Bls12381Fq> {
  using type = Bls12381Curve;
};
template <>
struct CurveOf<VestaFq> {
  using type = VestaCurve;
};
template <>
struct CurveOf<Bn254Fq> {
  using type = Bn254Curve;
};
template <>
struct CurveOf<GrumpkinFq> {
  using type = GrumpkinCurve;
};
template <>
struct CurveOf<Bls12377Fq> {
  using type = Bls12377Curve;
};

// f(Curve{}) for the curve with this id; `unknown` for any other id
template <class R, class F>
R with_curve_or(int curve, R unknown, F&& f) {
  switch (curve) {
    case AMSM_PALLAS: return f(PallasCurve{});
    case AMSM_BLS12_381_G1: return f(Bls12381Curve{});
    case AMSM_VESTA: return f(VestaCurve{});
    case AMSM_BN254_G1: return f(Bn254Curve{});  // (ids 3 and 5 are not curves: include/amsm.h)
    case AMSM_GRUMPKIN: return f(GrumpkinCurve{});
    case AMSM_BLS12_377_G1: return f(Bls12377Curve{});  // (7 is not a curve either)
    default: return unknown;
  }
}
template <class F>
auto with_curve(int curve, F&& f) {
  using R = decltype(f(PallasCurve{}));
  return with_curve_or<R>(curve, R(AMSM_E_INVALID_ARG), f);
}
inline bool curve_known(int curve) {
  return with_curve_or(curve, false, [](auto) { return true; });
}
inline int curve_fq_limbs(int curve) {  // u64 limbs of a base-field element in the C ABI
  return with_curve(curve, [](auto cv) { return decltype(cv)::Fq::W / 2; });
}

// the generator of curve `curve`, affine, Montgomery form, words of the C-ABI radix (x then y); empty when Fq is not that
// curve's base field
template <class Fq>
std::vector<u32> generator_mont(int curve) {
  std::vector<u32> g;
  with_curve(curve, [&](auto cv) {
    using C = decltype(cv);
    if constexpr (std::is_same<typename C::Fq, Fq>::value) {
      using H = host::HFe<Fq>;
      static_assert(sizeof(C::gx) == 8 * H::N, "generator limbs");
      H gx, gy;
      for (int i = 0; i < H::N; i++) {
        gx.v[i] = C::gx[i];
        gy.v[i] = C::gy[i];
      }
      gx = host::h_to_mont<Fq>(gx);
      gy = host::h_to_mont<Fq>(gy);
      g.resize(2 * Fq::L);
      memcpy(g.data(), gx.v, 4 * Fq::L);
      memcpy(g.data() + Fq::L, gy.v, 4 * Fq::L);
    }
    return AMSM_OK;
  });
  return g;
}
template <class Fq>
std::vector<u32> generator_mont() {
  return generator_mont<Fq>(CurveOf<Fq>::type::id);
}

}  // namespace amsm

// Inside a with_curve lambda taking `cv`: the curve's Fq and Fr packs under those names.
#define AMSM_CURVE_FIELDS(cv)              \
  using Fq = typename decltype(cv)::Fq;    \
  using Fr = typename decltype(cv)::Fr;    \
  (void)cv
