// Test-only device unit: one function of csrc/fp.h / fpu.h / ec.h per launch, on RAW register limbs.
//
// k_probe<P, OP> runs one thread per case.  A case is up to eight operands, each P::L limb words at a stride of 16 words
// (no fe_load / u_unpack in the way: a test chooses the representative -- lazy limbs, k p multiples, values near the
// stated bounds), and up to four results at the same stride (raw limbs, or a 0/1 word for a predicate).
// tests/field_model.py holds the contracts the results are checked against; tests/test_field_probe_gpu.py runs them.
//
// One source, one object per pack: -DPROBE_PACK=<id> instantiates the kernels of that pack and defines
// field_probe_run_<id>; without it the unit is the dispatcher field_probe_run (accumulation_amd/build.py: build_probe).
// Not part of libamsm.so.
#include <hip/hip_runtime.h>
#include "ec.h"
using namespace amsm;

// The operation table.  tests/field_model.py: OPS names the same operations in the same order (tests/test_field_probe_cpu.py).
#define PROBE_OPS(X)                                                                                         \
  X(mul) X(sqr)                                                                                              \
  X(mul_sub_k4) X(mul_sub_k9) X(mul_sub_k10) X(mul_sub_k13) X(mul_sub_k14)                                   \
  X(sqr_sub_bcc_k4) X(sqr_sub_bcc_k10)                                                                       \
  X(mul_sub_mul_k2) X(mul_sub_mul_k4) X(mul_sub_mul_k16)                                                     \
  X(sub_k2) X(sub_k4) X(sub_k8) X(sub_k12)                                                                   \
  X(sub_bcc_k4) X(dbl) X(triple) X(neg_lazy) X(neg_lazy_tight)                                               \
  X(is_zero_mod4) X(is_zero_mod8) X(is_zero_mod16)                                                           \
  X(canon2) X(canon4) X(canon8)                                                                              \
  X(import) X(export) X(from_words) X(store)                                                                 \
  X(xyzz_dbl) X(xyzz_dbl_affine) X(xyzz_madd) X(xyzz_add) X(affine_neg_if)                                   \
  X(jac_dbl) X(jac_madd) X(xyzz_from_jac) X(xyzz_dbl_quad) X(xyzz_add_quad)                                  \
  X(sat_mul) X(sat_dot2) X(sat_dot3) X(sat_add) X(sat_sub) X(sat_neg) X(sat_inv)

enum ProbeOp {
#define X(n) OP_##n,
  PROBE_OPS(X)
#undef X
  OP_COUNT
};

constexpr int STRIDE = 16;   // words per operand / result slot
constexpr int N_IN = 8;      // operand slots per case
constexpr int N_OUT = 4;     // result slots per case
constexpr int FIRST_SAT_OP = OP_sat_mul;

// pack ids: 0-4 and 9 the unsaturated base fields, 5-8 the 9 x 29 packs with CHAIN flipped and 20 the 14 x 28 one (BLS12-377; BLS12-381
// has no flipped pack), 10-19 and 21-22 the saturated packs
struct PallasFqUOther : PallasFqU { static constexpr bool CHAIN = !PallasFqU::CHAIN; };
struct VestaFqUOther : VestaFqU { static constexpr bool CHAIN = !VestaFqU::CHAIN; };
struct Bn254FqUOther : Bn254FqU { static constexpr bool CHAIN = !Bn254FqU::CHAIN; };
struct GrumpkinFqUOther : GrumpkinFqU { static constexpr bool CHAIN = !GrumpkinFqU::CHAIN; };
struct Bls12377FqUOther : Bls12377FqU { static constexpr bool CHAIN = !Bls12377FqU::CHAIN; };
namespace amsm {
template <>
struct HasTwoTorsion<Bls12377FqUOther> : HasTwoTorsion<Bls12377FqU> {};  // the same curve: the same guarded doublings
}  // namespace amsm
#define PROBE_PACKS(X)                                                                                                 \
  X(0, PallasFqU) X(1, Bls12381FqU) X(2, VestaFqU) X(3, Bn254FqU) X(4, GrumpkinFqU)                                   \
  X(5, PallasFqUOther) X(6, VestaFqUOther) X(7, Bn254FqUOther) X(8, GrumpkinFqUOther) X(9, Bls12377FqU)                \
  X(10, PallasFq) X(11, PallasFr) X(12, Bls12381Fq) X(13, Bls12381Fr) X(14, VestaFq) X(15, VestaFr) X(16, Bn254Fq)    \
  X(17, Bn254Fr) X(18, GrumpkinFq) X(19, GrumpkinFr) X(20, Bls12377FqUOther) X(21, Bls12377Fq) X(22, Bls12377Fr)

#ifdef PROBE_PACK

template <class P>
__device__ __forceinline__ Fe<P> ld(const u32* ci, int slot) {
  Fe<P> r;
#pragma unroll
  for (int i = 0; i < P::L; i++) r.v[i] = ci[slot * STRIDE + i];
  return r;
}
template <class P>
__device__ __forceinline__ void st(u32* co, int slot, const Fe<P>& a) {
#pragma unroll
  for (int i = 0; i < P::L; i++) co[slot * STRIDE + i] = a.v[i];
}
template <class P>
__device__ __forceinline__ XYZZ<P> ld_xyzz(const u32* ci, int slot) {
  XYZZ<P> r;
  r.x = ld<P>(ci, slot);
  r.y = ld<P>(ci, slot + 1);
  r.zz = ld<P>(ci, slot + 2);
  r.zzz = ld<P>(ci, slot + 3);
  return r;
}
template <class P>
__device__ __forceinline__ void st_xyzz(u32* co, const XYZZ<P>& a) {
  st<P>(co, 0, a.x);
  st<P>(co, 1, a.y);
  st<P>(co, 2, a.zz);
  st<P>(co, 3, a.zzz);
}
template <class P>
__device__ __forceinline__ Jac<P> ld_jac(const u32* ci, int slot) {
  Jac<P> r;
  r.x = ld<P>(ci, slot);
  r.y = ld<P>(ci, slot + 1);
  r.z = ld<P>(ci, slot + 2);
  return r;
}
template <class P>
__device__ __forceinline__ void st_jac(u32* co, const Jac<P>& a) {
  st<P>(co, 0, a.x);
  st<P>(co, 1, a.y);
  st<P>(co, 2, a.z);
}
template <class P>
__device__ __forceinline__ Affine<P> ld_affine(const u32* ci, int slot) {
  Affine<P> r;
  r.x = ld<P>(ci, slot);
  r.y = ld<P>(ci, slot + 1);
  return r;
}

template <class P, int OP>
__device__ __forceinline__ void probe_unsat(const u32* ci, u32* co) {
  const Fe<P> a = ld<P>(ci, 0), b = ld<P>(ci, 1), c = ld<P>(ci, 2), d = ld<P>(ci, 3);
  if constexpr (OP == OP_mul) st<P>(co, 0, fe_mul<P>(a, b));
  else if constexpr (OP == OP_sqr) st<P>(co, 0, fe_sqr<P>(a));
  else if constexpr (OP == OP_mul_sub_k4) st<P>(co, 0, fe_mul_sub_k<P, 4>(a, b, c));
  else if constexpr (OP == OP_mul_sub_k9) st<P>(co, 0, fe_mul_sub_k<P, 9>(a, b, c));
  else if constexpr (OP == OP_mul_sub_k10) st<P>(co, 0, fe_mul_sub_k<P, 10>(a, b, c));
  else if constexpr (OP == OP_mul_sub_k13) st<P>(co, 0, fe_mul_sub_k<P, 13>(a, b, c));
  else if constexpr (OP == OP_mul_sub_k14) st<P>(co, 0, fe_mul_sub_k<P, 14>(a, b, c));
  else if constexpr (OP == OP_sqr_sub_bcc_k4) st<P>(co, 0, fe_sqr_sub_bcc_k<P, 4>(a, b, c));
  else if constexpr (OP == OP_sqr_sub_bcc_k10) st<P>(co, 0, fe_sqr_sub_bcc_k<P, 10>(a, b, c));
  else if constexpr (OP == OP_mul_sub_mul_k2) st<P>(co, 0, fe_mul_sub_mul_k<P, 2>(a, b, c, d));
  else if constexpr (OP == OP_mul_sub_mul_k4) st<P>(co, 0, fe_mul_sub_mul_k<P, 4>(a, b, c, d));
  else if constexpr (OP == OP_mul_sub_mul_k16) st<P>(co, 0, fe_mul_sub_mul_k<P, 16>(a, b, c, d));
  else if constexpr (OP == OP_sub_k2) st<P>(co, 0, fe_sub_k<P, 2>(a, b));
  else if constexpr (OP == OP_sub_k4) st<P>(co, 0, fe_sub_k<P, 4>(a, b));
  else if constexpr (OP == OP_sub_k8) st<P>(co, 0, fe_sub_k<P, 8>(a, b));
  else if constexpr (OP == OP_sub_k12) st<P>(co, 0, fe_sub_k<P, 12>(a, b));
  else if constexpr (OP == OP_sub_bcc_k4) st<P>(co, 0, fe_sub_bcc_k<P, 4>(a, b, c));
  else if constexpr (OP == OP_dbl) st<P>(co, 0, fe_dbl<P>(a));
  else if constexpr (OP == OP_triple) st<P>(co, 0, fe_triple<P>(a));
  else if constexpr (OP == OP_neg_lazy) st<P>(co, 0, fe_neg_lazy<P>(a));
  else if constexpr (OP == OP_neg_lazy_tight) st<P>(co, 0, fe_tight<P>(fe_neg_lazy<P>(a)));
  else if constexpr (OP == OP_is_zero_mod4) co[0] = fe_is_zero_mod<P, 4>(a) ? 1u : 0u;
  else if constexpr (OP == OP_is_zero_mod8) co[0] = fe_is_zero_mod<P, 8>(a) ? 1u : 0u;
  else if constexpr (OP == OP_is_zero_mod16) co[0] = fe_is_zero_mod<P, 16>(a) ? 1u : 0u;
  else if constexpr (OP == OP_canon2 || OP == OP_canon4 || OP == OP_canon8) {
    Fe<P> r = a;
    u_canon<P, OP == OP_canon2 ? 2 : OP == OP_canon4 ? 4 : 8>(r);
    st<P>(co, 0, r);
  } else if constexpr (OP == OP_import) st<P>(co, 0, fe_import<P>(a));
  else if constexpr (OP == OP_export) st<P>(co, 0, fe_export<P>(a));
  else if constexpr (OP == OP_from_words) st<P>(co, 0, fe_from_words<P>(ci));  // slot 0 holds P::W packed words
  else if constexpr (OP == OP_store) fe_store<P>(co, a);                         // P::W packed canonical words into slot 0
  else if constexpr (OP == OP_xyzz_dbl) st_xyzz<P>(co, xyzz_dbl<P>(ld_xyzz<P>(ci, 0)));
  else if constexpr (OP == OP_xyzz_dbl_affine) st_xyzz<P>(co, xyzz_dbl_affine<P>(ld_affine<P>(ci, 0)));
  else if constexpr (OP == OP_xyzz_madd) {
    XYZZ<P> acc = ld_xyzz<P>(ci, 0);
    xyzz_madd<P>(acc, ld_affine<P>(ci, 4));
    st_xyzz<P>(co, acc);
  } else if constexpr (OP == OP_xyzz_add) {
    XYZZ<P> acc = ld_xyzz<P>(ci, 0);
    xyzz_add<P>(acc, ld_xyzz<P>(ci, 4));
    st_xyzz<P>(co, acc);
  } else if constexpr (OP == OP_affine_neg_if) {
    Affine<P> r = affine_neg_if<P>(ld_affine<P>(ci, 0), ci[2 * STRIDE] != 0);
    st<P>(co, 0, r.x);
    st<P>(co, 1, r.y);
  } else if constexpr (OP == OP_jac_dbl) st_jac<P>(co, jac_dbl<P>(ld_jac<P>(ci, 0)));
  else if constexpr (OP == OP_jac_madd) {
    Jac<P> acc = ld_jac<P>(ci, 0);
    jac_madd<P>(acc, ld_affine<P>(ci, 4));
    st_jac<P>(co, acc);
  } else if constexpr (OP == OP_xyzz_from_jac) st_xyzz<P>(co, xyzz_from_jac<P>(ld_jac<P>(ci, 0)));
  else if constexpr (OP == OP_xyzz_dbl_quad) st_xyzz<P>(co, xyzz_dbl_quad<P>(ld_xyzz<P>(ci, 0)));
  else if constexpr (OP == OP_xyzz_add_quad) {  // the host replicates each case over an aligned quad
    XYZZ<P> acc = ld_xyzz<P>(ci, 0);
    xyzz_add_quad<P>(acc, ld_xyzz<P>(ci, 4));
    st_xyzz<P>(co, acc);
  }
}

template <class P, int OP>
__device__ __forceinline__ void probe_sat(const u32* ci, u32* co) {
  const Fe<P> a = ld<P>(ci, 0), b = ld<P>(ci, 1);
  if constexpr (OP == OP_sat_mul) {  // the generated schedule and its definition in the same launch
    st<P>(co, 0, fe_mul<P>(a, b));
    st<P>(co, 1, fe_mul_ref<P>(a, b));
  } else if constexpr (OP == OP_sat_dot2) st<P>(co, 0, fe_dot2<P>(a, b, ld<P>(ci, 2), ld<P>(ci, 3)));
  else if constexpr (OP == OP_sat_dot3) st<P>(co, 0, fe_dot3<P>(a, b, ld<P>(ci, 2), ld<P>(ci, 3), ld<P>(ci, 4), ld<P>(ci, 5)));
  else if constexpr (OP == OP_sat_add) st<P>(co, 0, fe_add<P>(a, b));
  else if constexpr (OP == OP_sat_sub) st<P>(co, 0, fe_sub<P>(a, b));
  else if constexpr (OP == OP_sat_neg) st<P>(co, 0, fe_neg<P>(a));
  else if constexpr (OP == OP_sat_inv) st<P>(co, 0, fe_inv<P>(a));
}

template <class P, int OP>
__global__ void __launch_bounds__(64) k_probe(const u32* __restrict__ in, u32* __restrict__ out, int n) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;  // n is a multiple of 4: an aligned quad is active as a whole or not at all
  const u32* ci = in + (size_t)t * (N_IN * STRIDE);
  u32* co = out + (size_t)t * (N_OUT * STRIDE);
  if constexpr (P::UNSAT) probe_unsat<P, OP>(ci, co);
  else probe_sat<P, OP>(ci, co);
}

template <class P, int OP>
constexpr bool probe_applies() {
  return P::UNSAT ? OP < FIRST_SAT_OP : OP >= FIRST_SAT_OP;
}

template <class P, int OP = 0>
static hipError_t probe_launch(int op, const u32* d_in, u32* d_out, int n) {
  if constexpr (OP < OP_COUNT) {
    if (op == OP) {
      if constexpr (probe_applies<P, OP>()) {
        k_probe<P, OP><<<(n + 63) / 64, 64>>>(d_in, d_out, n);
        return hipGetLastError();
      } else {
        return hipErrorInvalidValue;
      }
    }
    return probe_launch<P, OP + 1>(op, d_in, d_out, n);
  } else {
    return hipErrorInvalidValue;
  }
}

#define PROBE_CAT2(a, b) a##b
#define PROBE_CAT(a, b) PROBE_CAT2(a, b)
template <int ID>
struct PackOf;
#define X(id, name) \
  template <>       \
  struct PackOf<id> { using type = name; };
PROBE_PACKS(X)
#undef X
using ProbeP = PackOf<PROBE_PACK>::type;

// in: n cases of N_IN * STRIDE words, out: n cases of N_OUT * STRIDE words (host pointers); n a multiple of 4
extern "C" int PROBE_CAT(field_probe_run_, PROBE_PACK)(int op, const u32* in, u32* out, int n) {
  if (n <= 0 || (n & 3) || op < 0 || op >= OP_COUNT) return (int)hipErrorInvalidValue;
  const size_t in_bytes = (size_t)n * N_IN * STRIDE * sizeof(u32), out_bytes = (size_t)n * N_OUT * STRIDE * sizeof(u32);
  u32 *d_in = nullptr, *d_out = nullptr;
  hipError_t e = hipMalloc(&d_in, in_bytes);
  if (e == hipSuccess) e = hipMalloc(&d_out, out_bytes);
  if (e == hipSuccess) e = hipMemcpy(d_in, in, in_bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(d_out, 0, out_bytes);
  if (e == hipSuccess) e = probe_launch<ProbeP>(op, d_in, d_out, n);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, d_out, out_bytes, hipMemcpyDeviceToHost);
  if (d_in) (void)hipFree(d_in);
  if (d_out) (void)hipFree(d_out);
  return (int)e;
}

#else  // the dispatcher

#define X(id, name) extern "C" int field_probe_run_##id(int op, const u32* in, u32* out, int n);
PROBE_PACKS(X)
#undef X

extern "C" int field_probe_op_count() { return OP_COUNT; }

// The one entry: pack id, operation id, host pointers, case count; returns the HIP status (0 = success).
extern "C" int field_probe_run(int pack, int op, const u32* in, u32* out, int n) {
  switch (pack) {
#define X(id, name) \
  case id:          \
    return field_probe_run_##id(op, in, out, n);
    PROBE_PACKS(X)
#undef X
  }
  return (int)hipErrorInvalidValue;
}

#endif
