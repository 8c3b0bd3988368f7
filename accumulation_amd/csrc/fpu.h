// Unsaturated-limb Montgomery arithmetic for the base fields of the MSM hot loop (gfx950): Pallas Fq, Vesta Fq,
// BN254 Fq and Grumpkin Fq on 9 x 29 bits, BLS12-381 Fq and BLS12-377 Fq on 14 x 28 bits.
//
// gfx950 has no carry-in on v_mad_u64_u32 and a VALU carry write costs wait states, so the saturated 8 x 32-bit
// schedule (fp_mul_gfx950.h) pays one v_addc per product.  Here an element is L limbs of B bits (Pallas Fq: 9 x 29,
// R' = 2^261): every column sum of a product fits a 64-bit accumulator, so a multiplication is one v_mad_u64_u32
// per limb product and NO carry handling (measured 17-21 % faster, tools/fp29_proto.hip), squarings need 45
// instead of 81 products, and additions / subtractions are carry-free limb-wise adds followed by one
// carry-propagation pass.
//
// Representation rules (every function states what it needs and gives):
//   * "tight"  : limbs 0..L-2 < 2^B, value < 2^(B*L).  Everything held in registers between operations is tight.
//   * "lazy"   : limbs < 2^(B+1), only allowed as ONE operand of a multiplication.
//   * values are only bounded, not reduced: a multiplication gives  out < p + A*B / 2^(B*L)  and the group-law
//     formulas in ec.h carry the bound of every intermediate in comments (cap = 2^261 ~ 128 p for Pallas and Vesta,
//     169 p for BN254 and Grumpkin: a value that is only known to be TIGHT may be as large as 169 p there -- nothing may canonicalise one with
//     a KMAX chosen from "tight" alone; every u_canon / u_is_zero_mod call site has a bound from the formulas).
//   * memory holds canonical values (< p), packed into W 32-bit words, in the INTERNAL Montgomery radix R'.  The
//     C ABI's radix is R = 2^(32 W); fe_import / fe_export convert (one multiplication by a constant) at the
//     edges (key load / read, the final fold of an MSM, amsm_points_fold), see DESIGN.md.
//
// Included from fp.h (after Fe<>), not on its own.
#pragma once

namespace amsm {

struct PallasFq;  // the saturated pack (fp.h) this field shadows

struct PallasFqU {
  using Sat = PallasFq;
  static constexpr int L = 9;  // register limbs
  static constexpr int W = 8;  // 32-bit words in memory
  static constexpr int B = 29;
  static constexpr bool UNSAT = true;
  static constexpr u32 NINV = 0x1fffffffu;  // -p^-1 mod 2^B
  static constexpr bool CHAIN = true;       // u_opaque after every column (measured, tools/fp_bench.hip: mixed addition -1 %)
  // p, R' mod p, R'^2 / R mod p (ABI -> internal), R mod p (internal -> ABI); radix 2^29, checked in tests/test_oracle.py
  AMSM_TABLE(mod, 9, 0x00000001u, 0x09698768u, 0x133e46e6u, 0x0d31f812u, 0x00000224u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00400000u)
  AMSM_TABLE(one, 9, 0x1fffff81u, 0x14a5d367u, 0x141ad3c0u, 0x1435eec5u, 0x1ffeefefu, 0x1fffffffu, 0x1fffffffu, 0x1fffffffu, 0x003fffffu)
  AMSM_TABLE(k_import, 9, 0x1ffff001u, 0x10f30767u, 0x0ecfe231u, 0x0db0ce73u, 0x1fddbb8bu, 0x1fffffffu, 0x1fffffffu, 0x1fffffffu, 0x003fffffu)
  AMSM_TABLE(k_export, 9, 0x1ffffffdu, 0x03c369c7u, 0x06452b4du, 0x186a17c8u, 0x1ffff992u, 0x1fffffffu, 0x1fffffffu, 0x1fffffffu, 0x003fffffu)
};

struct VestaFq;
struct VestaFqU {  // Vesta Fq = Pallas Fr: the same shape as PallasFqU (p_0 = 1, zero limbs 5-7, top limb 2^22, R' / p = 127.99...)
  using Sat = VestaFq;
  static constexpr int L = 9;
  static constexpr int W = 8;
  static constexpr int B = 29;
  static constexpr bool UNSAT = true;
  static constexpr u32 NINV = 0x1fffffffu;
  static constexpr bool CHAIN = true;  // Pallas's setting (not measured separately)
  AMSM_TABLE(mod, 9, 0x00000001u, 0x02375908u, 0x052a3763u, 0x0d31f813u, 0x00000224u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00400000u)
  AMSM_TABLE(one, 9, 0x1fffff81u, 0x068ad507u, 0x100e85dau, 0x1435ee7eu, 0x1ffeefefu, 0x1fffffffu, 0x1fffffffu, 0x1fffffffu, 0x003fffffu)
  AMSM_TABLE(k_import, 9, 0x1ffff001u, 0x0ca6d907u, 0x01b40647u, 0x0db0c57eu, 0x1fddbb8bu, 0x1fffffffu, 0x1fffffffu, 0x1fffffffu, 0x003fffffu)
  AMSM_TABLE(k_export, 9, 0x1ffffffdu, 0x1959f4e7u, 0x108159d6u, 0x186a17c6u, 0x1ffff992u, 0x1fffffffu, 0x1fffffffu, 0x1fffffffu, 0x003fffffu)
};

struct Bn254Fq;
// BN254 Fq: 254 bits, R' / p = 169.28 (more head-room than Pallas's 127.99, so every `[< k p]` line of ec.h holds).  The first
// 9 x 29 field on the GENERAL reduction path: all nine limbs of p are non-zero, p_0 != 1 (m_k costs a multiplication by NINV and
// a product by p_0) and no limb is a power of two -- 9 x 9 reduction products per multiplication against Pallas's 5 x 9.
// Column sums: 9 products with one lazy operand (< 2^59 each) + 9 reduction products (< 2^58) + the carry stay below 2^63; two
// product sets with one lazy operand each (u_mul_add_mul) below 18 * 2^59 + 9 * 2^58 + 2^35 < 2^64.
struct Bn254FqU {
  using Sat = Bn254Fq;
  static constexpr int L = 9;
  static constexpr int W = 8;
  static constexpr int B = 29;
  static constexpr bool UNSAT = true;
  static constexpr u32 NINV = 0x04866389u;  // -p^-1 mod 2^B
  // measured both ways in one run of tools/fp_bench.hip (MI355X, cycles per SIMD at 2 waves per SIMD, chain / no chain): multiplication
  // 985 / 998, squaring 826 / 820, mixed addition 10 330 / 10 357 -- the multiplication gains 1-2 % at every occupancy, the mixed
  // addition is within 0.5 % either way, and k_accum_bpl keeps 3 waves without scratch with it
  static constexpr bool CHAIN = true;
  AMSM_TABLE(mod, 9, 0x187cfd47u, 0x010460b6u, 0x1c72a34fu, 0x02d522d0u, 0x1585d978u, 0x02db40c0u, 0x00a6e141u, 0x0e5c2634u, 0x0030644eu)
  AMSM_TABLE(one, 9, 0x157ccc21u, 0x141c2758u, 0x185230d3u, 0x014c0419u, 0x0aa36fb9u, 0x1d4240ceu, 0x11d54c07u, 0x052ac7a8u, 0x000dc836u)
  AMSM_TABLE(k_import, 9, 0x13349ca1u, 0x1a5d84a8u, 0x0a3e5cacu, 0x100249e0u, 0x12b951e8u, 0x0e92d304u, 0x14cb95b3u, 0x041b9d3du, 0x00058003u)
  AMSM_TABLE(k_export, 9, 0x058f0d9du, 0x1aea1c6eu, 0x11c2cf74u, 0x11d651ebu, 0x1462c0a7u, 0x11b7bc3cu, 0x1cbd99bau, 0x183340fbu, 0x000e0a77u)
};

struct GrumpkinFq;
// Grumpkin Fq = BN254 Fr: 254 bits, R' / q = 169.28, the head-room of BN254 Fq, so every `[< k p]` line of ec.h holds.  The second
// field on the GENERAL reduction path: no limb of q is zero, none of limbs 1..8 is a power of two, q_0 = 2^28 + 1 and
// NINV = 2^28 - 1 != 2^29 - 1, so u_red_low takes the general branch (m_k = lo * NINV, then one ordinary MAD by q_0: no shortcut
// for this q_0 is taken) -- 9 x 9 reduction products per multiplication.  The column sums of Bn254FqU above hold unchanged:
// the limb widths are the same.
struct GrumpkinFqU {
  using Sat = GrumpkinFq;
  static constexpr int L = 9;
  static constexpr int W = 8;
  static constexpr int B = 29;
  static constexpr bool UNSAT = true;
  static constexpr u32 NINV = 0x0fffffffu;  // -q^-1 mod 2^B
  // measured both ways in one run of tools/fp_bench.hip beside BN254's lines (MI355X, cycles per SIMD at 2 waves per SIMD, chain / no
  // chain): multiplication 959 / 929, squaring 868 / 889, mixed addition 9 639 / 9 934 -- the mixed addition decides, and its 3 %
  // are six times what BN254's two lines differ by in that run (10 413 / 10 363); profiles/grumpkin_fp_bench.txt, DESIGN.md 4.1
  static constexpr bool CHAIN = true;
  AMSM_TABLE(mod, 9, 0x10000001u, 0x1f0fac9fu, 0x0e5c2450u, 0x07d090f3u, 0x1585d283u, 0x02db40c0u, 0x00a6e141u, 0x0e5c2634u, 0x0030644eu)
  AMSM_TABLE(one, 9, 0x0fffff57u, 0x1ea70ab4u, 0x052c068bu, 0x17504f49u, 0x0aa8075bu, 0x1d4240ceu, 0x11d54c07u, 0x052ac7a8u, 0x000dc836u)
  AMSM_TABLE(k_import, 9, 0x0fffead7u, 0x1d5444f4u, 0x04438aa5u, 0x03b4d096u, 0x134c84dau, 0x0e92d304u, 0x14cb95b3u, 0x041b9d3du, 0x00058003u)
  AMSM_TABLE(k_export, 9, 0x0ffffffbu, 0x04b1a0e2u, 0x18334a6bu, 0x18ed2b3eu, 0x1462e36fu, 0x11b7bc3cu, 0x1cbd99bau, 0x183340fbu, 0x000e0a77u)
};

struct Bls12381Fq;
struct Bls12381FqU {  // 14 x 28 bits, R' = 2^392 ~ 2520 p: measured against the saturated schedule in tools/fp_bench.hip
  using Sat = Bls12381Fq;
  static constexpr int L = 14;
  static constexpr int W = 12;
  static constexpr int B = 28;
  static constexpr bool UNSAT = true;
  static constexpr u32 NINV = 0x0ffcfffdu;
  static constexpr bool CHAIN = false;  // measured: the opaque carry costs the 14-limb mixed addition 4 % (register pressure)
  AMSM_TABLE(mod, 14, 0x0fffaaabu, 0x0fefffffu, 0x03ffffb9u, 0x0fffeb15u, 0x06241eabu, 0x0a0f6b0fu, 0x0f6730d2u, 0x0f38512bu, 0x04774b84u, 0x04bacd76u, 0x0ba7b643u, 0x0e69a4b1u, 0x01ea397fu, 0x0001a011u)
  AMSM_TABLE(one, 14, 0x0347fcb8u, 0x0d800000u, 0x0002b119u, 0x00cde6d2u, 0x0c7212e0u, 0x083a2090u, 0x0037669fu, 0x0da0f73eu, 0x09b09b42u, 0x01297bb0u, 0x0515d98fu, 0x0012ca7cu, 0x0659fcfau, 0x0000577au)
  AMSM_TABLE(k_import, 14, 0x080e6299u, 0x03500034u, 0x0eb12856u, 0x0deb2699u, 0x0c988670u, 0x04ef6697u, 0x070983e8u, 0x0a4e6fe9u, 0x03e8a053u, 0x0ecf271eu, 0x0c20d323u, 0x06eb6385u, 0x047f1286u, 0x000156dau)
  AMSM_TABLE(k_export, 14, 0x0002fffdu, 0x00900000u, 0x0c000276u, 0x0000bc40u, 0x08baebf4u, 0x05753c75u, 0x055f4898u, 0x07052574u, 0x07ce5853u, 0x056ec6d7u, 0x071a97a2u, 0x0e4935c0u, 0x0ec3fa80u, 0x00015f65u)
};

struct Bls12377Fq;
// BLS12-377 Fq: 377 bits on the 14 x 28 shape, R' = 2^392 ~ 38996 p (BLS12-381: 2520), so every `[< k p]` line of ec.h holds with
// room to spare, and p > 6883 * 2^364 gives u_kp_minus_lazy's exact condition y < K p - 2^(B (L - 1)) from y < (K - 1) p.  The first
// 14-limb field with p = 1 mod 2^28: NINV = 2^28 - 1, so u_red_low takes the p_0 = 1 branch (no m_k p_0 product, one 64-bit add of a
// constant) at B = 28.  No limb of p is zero and none above limb 0 is a power of two: 13 reduction products per column against
// BLS12-381's 14.  Column sums as for BLS12-381 (same limb widths): 2 * 14 products with one lazy operand (< 2^57 each) + 13
// reduction products (< 2^56) + an addend and the carry stay below 2^63.
struct Bls12377FqU {
  using Sat = Bls12377Fq;
  static constexpr int L = 14;
  static constexpr int W = 12;
  static constexpr int B = 28;
  static constexpr bool UNSAT = true;
  static constexpr u32 NINV = 0x0fffffffu;  // -p^-1 mod 2^B: p_0 = 1
  // measured both ways in two runs of tools/fp_bench.hip beside BLS12-381's lines, the order of the two settings swapped (MI355X, cycles
  // per SIMD at 2 waves per SIMD, chain / no chain): mixed addition 21 400 / 22 489 and 21 724 / 22 618 (BLS12-381: 22 796, 22 832) --
  // the mixed addition decides, 4-5 % in either order; the bare multiplication's 3 % follow the position in the run.  The
  // accumulation kernels keep 2 waves without scratch with it; the three ladder kernels (k_generate_bases, k_sample_finish,
  // k_points_check_subgroup<1>) drop to 1 wave: profiles/bls12_377_fp_bench.txt, DESIGN.md 4.1
  static constexpr bool CHAIN = true;
  AMSM_TABLE(mod, 14, 0x00000001u, 0x008c0000u, 0x00000085u, 0x05d44300u, 0x0800170bu, 0x02fba094u, 0x0f1ef362u, 0x000f5138u, 0x0a22d9f3u, 0x0a1493b1u, 0x0b05c06cu, 0x010eac63u, 0x0a4617c5u, 0x00001ae3u)
  AMSM_TABLE(one, 14, 0x0fff67acu, 0x020fffffu, 0x0fb0d727u, 0x0e9203ffu, 0x0249b0e4u, 0x0e172345u, 0x0955d771u, 0x02bf89aau, 0x0b2833b2u, 0x098e116bu, 0x07dc5c97u, 0x00d43e93u, 0x02e3314bu, 0x000003b4u)
  AMSM_TABLE(k_import, 14, 0x0f67abddu, 0x0cdbffffu, 0x00d714f0u, 0x05fed6fbu, 0x01adbe5bu, 0x0ebc50d7u, 0x049c2b74u, 0x0d718fccu, 0x056fe5f2u, 0x0d413a69u, 0x0a9348beu, 0x0f3d01dcu, 0x0b9c0b1bu, 0x0000070eu)
  AMSM_TABLE(k_export, 14, 0x0fffff68u, 0x0cdfffffu, 0x0fffb102u, 0x09f837ffu, 0x0ff25140u, 0x0a98a7d3u, 0x059f7db3u, 0x06e7c630u, 0x0b4e97b7u, 0x03c84e87u, 0x0495bf80u, 0x0f49a4cfu, 0x0661e2fdu, 0x000008d6u)
};

template <class P>
AMSM_HD constexpr u32 u_mask() {
  return (1u << P::B) - 1u;
}

// ---- the reduction step's two tricks (round 3; the A/B against round 2's schedule is in DESIGN.md 4.1) ----
// The compiler's own schedule of a 9 x 29 product (round 2) kept one 64-bit accumulator chain PER COLUMN, started from zero,
// and merged it with the carry of the column below by a 64-bit add (v_lshl_add_u64: half rate); the reduction step added
// m * p_0 = m as a zero-extended 64-bit add (v_mov + v_lshl_add_u64) and m * 2^22 as a 64-bit shift + 64-bit add: 99 non-MAD
// instructions per multiplication, 63 of them half rate, next to 117 MADs.  Round 3:
//   chain:  an opaque (empty-asm) use of the accumulator after every column shift, so that the next column's MADs chain
//                from the carry instead of from zero (no merge add);
//   const:  p_0 = 1 (Pallas: p = 1 mod 2^29): (acc + m) >> B == (acc + 2^B - 1) >> B, one 64-bit add of a constant and no
//                m in the low column; a power-of-two limb of p (2^22 at limb 8) as a MAD by a constant held in an SGPR the
//                compiler cannot see through (one half-rate instruction instead of shift + add).
// Measured (MI355X, cycles per operation per SIMD at 2 / 4 waves per SIMD): Pallas multiplication 899 / 862 -> 877 / 822, squaring
// 747 / 709 -> 715 / 685, mixed addition 8 640 / 8 288 -> 8 208 / 7 963 (-5 % / -4 %); 126 MADs + 81 full-rate + 40 half-rate
// instructions per multiplication instead of 117 + 89 + 59.  BLS12-381 (p_0 != 1, no power-of-two limb) is unchanged.  A strictly
// linear chain (an opaque use after EVERY product) removes the remaining merge adds but spills: 12 300.
template <class P>
AMSM_DEV void u_opaque(u64& acc) {
  if constexpr (P::CHAIN) asm("" : "+v"(acc));
}
template <u32 V>
AMSM_DEV u32 u_sgpr_const() {  // V in an SGPR, opaque to the optimiser (hoisted out of loops like any pure expression)
  u32 r;
  asm("s_mov_b32 %0, %1" : "=s"(r) : "i"(V));
  return r;
}
AMSM_HD constexpr bool u_is_pow2(u32 v) { return v != 0 && (v & (v - 1)) == 0; }

// acc += m_i * p_j for the limbs j >= 1 of p that are not zero (column k of a product: i + j = k)
template <class P, int I, int K>
AMSM_DEV void u_red_term(u64& acc, const u32* m) {
  constexpr int J = K - I;
  if constexpr (I < K && J >= 1 && J < P::L) {
    if constexpr (P::mod(J) != 0) {
      if constexpr (u_is_pow2(P::mod(J))) acc += (u64)m[I] * u_sgpr_const<P::mod(J)>();
      else acc += (u64)m[I] * P::mod(J);
    }
  }
}
template <class P, int K, int I = 0>
AMSM_DEV void u_red_terms(u64& acc, const u32* m) {
  if constexpr (I < P::L) {
    u_red_term<P, I, K>(acc, m);
    u_red_terms<P, K, I + 1>(acc, m);
  }
}
// low column k < L: m_k = -acc * p^-1 mod 2^B, acc = (acc + m_k p_0) >> B
template <class P>
AMSM_DEV u32 u_red_low(u64& acc) {
  constexpr u32 M = u_mask<P>();
  const u32 lo = (u32)acc & M;
  u32 mk;
  if constexpr (P::NINV == M) {  // p_0 = 1
    mk = (0u - lo) & M;
    acc = (acc + (u64)M) >> P::B;  // == (acc + mk) >> B: lo + mk is 0 or 2^B
  } else {
    mk = (lo * P::NINV) & M;
    acc += (u64)mk * P::mod(0);
    acc >>= P::B;
  }
  u_opaque<P>(acc);
  return mk;
}
// high column k >= L: emit limb k - L
template <class P>
AMSM_DEV u32 u_red_high(u64& acc, bool top) {
  const u32 r = top ? (u32)acc : ((u32)acc & u_mask<P>());
  acc >>= P::B;
  if (!top) u_opaque<P>(acc);
  return r;
}

// K*p as tight limbs (compile-time)
template <class P, u32 K>
struct UKp {
  u32 v[P::L];
  AMSM_HD constexpr UKp() : v{} {
    u64 carry = 0;
    for (int j = 0; j < P::L; j++) {
      u64 t = (u64)K * P::mod(j) + carry;
      if (j < P::L - 1) {
        v[j] = (u32)t & u_mask<P>();
        carry = t >> P::B;
      } else {
        v[j] = (u32)t;
      }
    }
  }
};

// K*p in a redundant form whose limbs 0..L-2 are all >= S*(2^B - 1): a + UKpBp - (sum of S tight values) never
// borrows below the top limb (compile-time)
template <class P, u32 K, u32 S>
struct UKpBp {
  u32 v[P::L];
  AMSM_HD constexpr UKpBp() : v{} {
    UKp<P, K> t;
    for (int j = 0; j < P::L; j++) {
      if (j == 0) v[j] = t.v[j] + (S << P::B);
      else if (j < P::L - 1) v[j] = t.v[j] + (S << P::B) - S;
      else v[j] = t.v[j] - S;
    }
  }
};

// carry propagation: limbs < 2^32 (true value in [0, 2^(B*L))) -> tight.  The top limb may have wrapped mod 2^32
// during limb-wise arithmetic; it is exact again after the carries arrive.
template <class P>
AMSM_DEV void u_carry(Fe<P>& a) {
#pragma unroll
  for (int i = 0; i < P::L - 1; i++) {
    a.v[i + 1] += a.v[i] >> P::B;
    a.v[i] &= u_mask<P>();
  }
}

// Montgomery product a*b / 2^(B*L) mod p.  Needs: limbs of a < 2^(B+1), limbs of b < 2^B (or the reverse).
// Gives: limbs 0..L-2 < 2^B, value < p + a*b / 2^(B*L) -- TIGHT only where that bound (with the addend, if any) is <= 2^(B*L): limb
// widths alone do not give it (a lazy a near 2^(B*L+1) times a tight b near 2^(B*L) lands above 2^(B*L), in a top limb wider than
// B bits).  Every call site in ec.h has the bound from its `[< k p]` line; u_mul_add_mul and u_sqr are the same.
// With ADD: returns a*b / 2^(B*L) + add, the addend's limbs (any u32, e.g. the unnormalised K*p - x) going straight
// into the upper columns of the product, so "product minus value" costs L 64-bit adds instead of a subtraction and
// a carry pass, and the result is tight.
template <class P, int K, class F>
AMSM_DEV void u_column(u64& acc, u32* m, Fe<P>& r, const Fe<P>* add, bool has_add, F&& products) {
  products(acc);
  u_red_terms<P, K>(acc, m);
  if constexpr (K < P::L) {
    m[K] = u_red_low<P>(acc);
  } else {
    if (has_add) acc += add->v[K - P::L];
    r.v[K - P::L] = u_red_high<P>(acc, K == 2 * P::L - 1);
  }
}
template <class P, int K, class F>
AMSM_DEV void u_columns(u64& acc, u32* m, Fe<P>& r, const Fe<P>* add, bool has_add, F&& products) {
  if constexpr (K < 2 * P::L) {
    u_column<P, K>(acc, m, r, add, has_add, [&](u64& a) { products(a, K); });
    u_columns<P, K + 1>(acc, m, r, add, has_add, products);
  }
}

template <class P, bool ADD = false>
AMSM_DEV Fe<P> u_mul(const Fe<P>& a, const Fe<P>& b, const Fe<P>* add = nullptr) {
  constexpr int L = P::L;
  u64 acc = 0;
  u32 m[L];
  Fe<P> r;
  u_columns<P, 0>(acc, m, r, add, ADD, [&](u64& ac, int k) {
#pragma unroll
    for (int i = 0; i < L; i++) {
      int j = k - i;
      if (j >= 0 && j < L) {
        ac += (u64)a.v[i] * b.v[j];
      }
    }
  });
  return r;
}

// (a*b + c*d) / 2^(B*L) mod p with ONE reduction: both products are accumulated column by column before the
// Montgomery step (saves a whole reduction, ~40 % of a multiplication, wherever the group law subtracts two products).
// Needs: limbs of a, c < 2^(B+1), limbs of b, d < 2^B.  Gives: tight, value < p + (a*b + c*d) / 2^(B*L).
template <class P>
AMSM_DEV Fe<P> u_mul_add_mul(const Fe<P>& a, const Fe<P>& b, const Fe<P>& c, const Fe<P>& d) {
  constexpr int L = P::L;
  u64 acc = 0;
  u32 m[L];
  Fe<P> r;
  u_columns<P, 0>(acc, m, r, nullptr, false, [&](u64& ac, int k) {
#pragma unroll
    for (int i = 0; i < L; i++) {
      int j = k - i;
      if (j >= 0 && j < L) {
        ac += (u64)a.v[i] * b.v[j];
        ac += (u64)c.v[i] * d.v[j];
      }
    }
  });
  return r;
}

// limb-wise a + b (both tight, sum < 2^(B*L)): tight
template <class P>
AMSM_DEV Fe<P> u_add(const Fe<P>& a, const Fe<P>& b) {
  Fe<P> r;
#pragma unroll
  for (int i = 0; i < P::L; i++) r.v[i] = a.v[i] + b.v[i];
  u_carry<P>(r);
  return r;
}

// K*p - y with lazy limbs (< 2^(B+1)): multiplication operand only.  Needs y tight and y < (K - 1)*p, so that the
// (unnormalised) top limb cannot go negative (exactly: y < K*p - 2^(B (L - 1)); there is no carry pass to repair it).
template <class P, u32 K>
AMSM_DEV Fe<P> u_kp_minus_lazy(const Fe<P>& y) {
  constexpr UKpBp<P, K, 1> c{};
  Fe<P> r;
#pragma unroll
  for (int i = 0; i < P::L; i++) r.v[i] = c.v[i] - y.v[i];
  return r;
}

// a^2 / 2^(B*L): the cross products are taken once against doubled limbs (45 instead of 81 products for L = 9).
// Needs: a tight.  Gives: tight, value < p + a^2 / 2^(B*L).
template <class P, bool ADD = false>
AMSM_DEV Fe<P> u_sqr(const Fe<P>& a, const Fe<P>* add = nullptr) {
  constexpr int L = P::L;
  u32 a2[L];
#pragma unroll
  for (int i = 0; i < L; i++) a2[i] = a.v[i] << 1;
  u64 acc = 0;
  u32 m[L];
  Fe<P> r;
  u_columns<P, 0>(acc, m, r, add, ADD, [&](u64& ac, int k) {
#pragma unroll
    for (int i = 0; i < L; i++) {
      int j = k - i;
      if (j >= 0 && j < L) {
        if (i < j) ac += (u64)a2[i] * a.v[j];
        else if (i == j) ac += (u64)a.v[i] * a.v[i];

      }
    }
  });
  return r;
}

// a + K*p - b.  Needs: a, b tight, b < K*p.  Gives: tight, value = a - b + K*p.
template <class P, u32 K>
AMSM_DEV Fe<P> u_sub_k(const Fe<P>& a, const Fe<P>& b) {
  constexpr UKpBp<P, K, 1> c{};
  Fe<P> r;
#pragma unroll
  for (int i = 0; i < P::L; i++) r.v[i] = a.v[i] + c.v[i] - b.v[i];
  u_carry<P>(r);
  return r;
}

// a + K*p - b - 2c.  Needs: a, b, c tight, b + 2c < K*p.  Gives: tight, value = a - b - 2c + K*p.
template <class P, u32 K>
AMSM_DEV Fe<P> u_sub_bcc_k(const Fe<P>& a, const Fe<P>& b, const Fe<P>& c) {
  constexpr UKpBp<P, K, 3> kp{};
  Fe<P> r;
#pragma unroll
  for (int i = 0; i < P::L; i++) r.v[i] = a.v[i] + kp.v[i] - b.v[i] - 2u * c.v[i];
  u_carry<P>(r);
  return r;
}

// K*p - b - 2c, unnormalised (limbs < 2^32): addend of u_mul<ADD> / u_sqr<ADD> only.  Needs b, c tight, b + 2c < K*p.
template <class P, u32 K>
AMSM_DEV Fe<P> u_kp_minus_bcc_raw(const Fe<P>& b, const Fe<P>& c) {
  constexpr UKpBp<P, K, 3> kp{};
  Fe<P> r;
#pragma unroll
  for (int i = 0; i < P::L; i++) r.v[i] = kp.v[i] - b.v[i] - 2u * c.v[i];
  return r;
}

// small multiples.  Needs: a tight.  Gives: tight, value = MULT*a (MULT <= 4).
template <class P, u32 MULT>
AMSM_DEV Fe<P> u_times(const Fe<P>& a) {
  Fe<P> r;
#pragma unroll
  for (int i = 0; i < P::L; i++) r.v[i] = MULT * a.v[i];
  u_carry<P>(r);
  return r;
}

// 2p - y for a canonical y (< p).  Gives: LAZY limbs (< 2^(B+1)), value in (p, 2p]: multiplication operand only.
template <class P>
AMSM_DEV Fe<P> u_neg_lazy(const Fe<P>& y) {
  constexpr UKpBp<P, 2, 1> c{};
  Fe<P> r;
#pragma unroll
  for (int i = 0; i < P::L; i++) r.v[i] = c.v[i] - y.v[i];
  return r;
}

// conditional subtraction of K*p, K*p/2, ..., p: a tight with value < 2*K*p  ->  canonical (< p) for K a power of 2
template <class P, u32 K>
AMSM_DEV void u_canon_steps(Fe<P>& a) {
  constexpr UKp<P, K> kp{};
  constexpr u32 M = u_mask<P>();
  u32 d[P::L];
  u32 br = 0;
#pragma unroll
  for (int i = 0; i < P::L - 1; i++) {
    u32 x = a.v[i] - kp.v[i] - br;
    br = x >> 31;
    d[i] = x & M;
  }
  u32 x = a.v[P::L - 1] - kp.v[P::L - 1] - br;
  bool lt = (int)x < 0;
  d[P::L - 1] = x;
#pragma unroll
  for (int i = 0; i < P::L; i++) a.v[i] = lt ? a.v[i] : d[i];
  if constexpr (K > 1) u_canon_steps<P, K / 2>(a);
}

// a tight, value < KMAX*p (KMAX a power of two) -> canonical
template <class P, u32 KMAX>
AMSM_DEV void u_canon(Fe<P>& a) {
  static_assert((KMAX & (KMAX - 1)) == 0 && KMAX >= 2, "KMAX must be a power of two");
  u_canon_steps<P, KMAX / 2>(a);
}

// is a == 0 (mod p)?  a tight, value < KMAX*p.  The low limb of k*p filters all but ~KMAX/2^B of the non-zero
// values; the exact test behind it canonicalises.
template <class P, u32 KMAX>
AMSM_DEV bool u_is_zero_mod(const Fe<P>& a) {
  constexpr u32 M = u_mask<P>();
  bool maybe = false;
  if constexpr (P::mod(0) == 1) {
    maybe = a.v[0] < KMAX;
  } else {
#pragma unroll
    for (u32 k = 0; k < KMAX; k++) maybe |= a.v[0] == ((k * P::mod(0)) & M);
  }
  if (!maybe) return false;
  Fe<P> c = a;
  u_canon<P, KMAX>(c);
  u32 o = 0;
#pragma unroll
  for (int i = 0; i < P::L; i++) o |= c.v[i];
  return o == 0;
}

// memory (W packed 32-bit words, value < 2^(32 W)) <-> register limbs
template <class P>
AMSM_DEV Fe<P> u_unpack(const u32* w) {
  constexpr u32 M = u_mask<P>();
  Fe<P> r;
#pragma unroll
  for (int i = 0; i < P::L; i++) {
    int o = i * P::B, j = o >> 5, sh = o & 31;
    u32 lo = j < P::W ? w[j] : 0u;
    u32 hi = (j + 1) < P::W ? w[j + 1] : 0u;
    u32 x = sh ? (u32)((((u64)hi << 32) | lo) >> sh) : lo;
    r.v[i] = (i < P::L - 1) ? (x & M) : x;
  }
  return r;
}

template <class P>
AMSM_DEV void u_pack(const Fe<P>& a, u32* w) {  // a tight, value < 2^(32 W)
#pragma unroll
  for (int j = 0; j < P::W; j++) {
    // word j = bits [32j, 32j+32): limbs i0 .. i0+2 overlap it
    int i0 = (32 * j) / P::B;
    u32 x = 0;
#pragma unroll
    for (int i = i0; i < i0 + 3 && i < P::L; i++) {
      int s = i * P::B - 32 * j;  // bit position of limb i inside the word (may be negative)
      if (s <= -32 || s >= 32) continue;
      x |= s >= 0 ? (a.v[i] << s) : (a.v[i] >> (-s));
    }
    w[j] = x;
  }
}

}  // namespace amsm
