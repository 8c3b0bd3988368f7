// C ABI implementation (include/amsm.h): contexts, resident committer keys, the MSM pipeline launcher,
// host-side finalisation.  One context = one GPU + one HIP stream + a grow-only HBM workspace.
#include "../../include/amsm.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <dlfcn.h>
#include <functional>
#include <memory>
#include <mutex>
#include <new>
#include <pthread.h>
#include <system_error>
#include <thread>
#include <unordered_map>
#include <rocprim/rocprim.hpp>
#include <vector>

#include "curves.h"
#include "fp.h"
#include "host_field.h"
#include "host_glv.h"
#include "host_points_check.h"
#include "host_poseidon.h"
#include "host_sample.h"
#include "host_serialize.h"
#include "launch.h"
#include "msm_geom.h"
#include "msm_jobs.h"
#include "msm_select.h"
#include "rng.h"

using namespace amsm;

#include "api_types.h"

namespace {

#include "api_gate.inc"
#include "api_pipeline.inc"
#include "api_keys.inc"
#include "api_host.inc"
#include "api_schemes.inc"
#include "api_multi.inc"
#include "api_cpu.inc"

// CALL evaluated with Fq / Fr bound to the context's curve (curves.h; a context's curve is known: amsm_ctx_create checks it)
#define DISPATCH(ctx, ...) with_curve((ctx)->curve, [&](auto cv_) { AMSM_CURVE_FIELDS(cv_); return (__VA_ARGS__); })
// the statement(s) run with Fq / Fr bound to the context's curve; a `return` among them (TRY's included) leaves with that
// status, the end gives AMSM_OK
#define DISPATCH_DO(ctx, ...) \
  with_curve((ctx)->curve, [&](auto cv_) -> int { AMSM_CURVE_FIELDS(cv_); __VA_ARGS__; return AMSM_OK; })

int bind_device(const amsm_ctx* ctx) {
  // every entry point branches to the host backend BEFORE it binds a device; one that forgot to must fail, not touch HIP
  if (ctx->host_only) return AMSM_E_UNSUPPORTED;
  HIP_TRY(hipSetDevice(ctx->device));
  return AMSM_OK;
}

}  // namespace

// =============================================================================================
// extern "C"
// =============================================================================================
// Host scalar-field helpers (no device work): what a scheme driver needs for its O(#inputs) challenge arithmetic.
template <class Fr, class F>
static void fr_map2(const uint64_t* a, const uint64_t* b, size_t n, uint64_t* out, F&& f) {
  for (size_t i = 0; i < n; i++) {
    host::HFe<Fr> x, y;
    memcpy(x.v, a + 4 * i, 32);
    if (b) memcpy(y.v, b + 4 * i, 32);
    host::HFe<Fr> r = f(x, y);
    memcpy(out + 4 * i, r.v, 32);
  }
}
#define AMSM_FR_OP(NAME, EXPR)                                                                               \
  static int NAME(int curve, const uint64_t* a, const uint64_t* b, size_t n, uint64_t* out) {                \
    if (!curve_known(curve) || (n && (!a || !out))) return AMSM_E_INVALID_ARG;                               \
    return with_curve(curve, [&](auto cv) {                                                                  \
      using F = typename decltype(cv)::Fr;                                                                   \
      fr_map2<F>(a, b, n, out, [](const host::HFe<F>& x, const host::HFe<F>& y) { (void)y; return EXPR; });  \
      return AMSM_OK;                                                                                        \
    });                                                                                                      \
  }
AMSM_FR_OP(amsm_fr_mul_impl, host::h_mul<F>(x, y))
AMSM_FR_OP(amsm_fr_add_impl, host::h_add<F>(x, y))
AMSM_FR_OP(amsm_fr_sub_impl, host::h_sub<F>(x, y))
AMSM_FR_OP(amsm_fr_inv_impl, host::h_inv<F>(x))
AMSM_FR_OP(amsm_fr_to_mont_impl, host::h_to_mont<F>(x))
AMSM_FR_OP(amsm_fr_from_mont_impl, host::h_from_mont<F>(x))
extern "C" {

#include "api_entry_ctx.inc"
#include "api_entry_msm.inc"
#include "api_entry_host.inc"
#include "api_entry_vec.inc"

}  // extern "C"
