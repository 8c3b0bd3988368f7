// C-ABI caller of amsm_poly_div_linear(_batch) / amsm_poly_evaluate(_batch) through the wrappers of include/amsm.hpp: for a batch
// of polynomials of unequal lengths (an empty and a constant one among them) the remainder equals the value at the same point and
// q(X) (X - z) + rem == p(X) coefficient for coefficient (host arithmetic: amsm_fr_*); the single-polynomial entries agree with
// the batch.  Prints the values so that a test can compare the GPU with the host backend.
#include <cstdio>

#include "amsm_hp_as.hpp"
#include "check_device.hpp"

using namespace amsm;

int main() {
  Context ctx = check_context(AMSM_PALLAS);
  hp_as::FrOps fr{amsm_ctx_curve(ctx.get())};
  const size_t lens[] = {5000, 0, 1, 1024, 1025, 4097, 2, 300, 12345};
  const size_t K = sizeof(lens) / sizeof(lens[0]);
  std::vector<FrVector> vecs;
  std::vector<const FrVector*> ptrs;
  std::vector<Fr> zs;
  for (size_t k = 0; k < K; k++) {
    vecs.push_back(FrVector::random(ctx, 100 + k, lens[k], false));  // (values below r: read as Montgomery elements)
    zs.push_back(FrVector::random(ctx, 200 + k, 1, false).to_host()[0]);
  }
  zs[3] = fr.zero();
  zs[4] = fr.one();
  for (auto& v : vecs) ptrs.push_back(&v);
  std::vector<Fr> rems;
  std::vector<FrVector> quots = poly_div_linear(ctx, ptrs, zs, &rems);
  std::vector<FrVector> quots_async = poly_div_linear(ctx, ptrs, zs);
  const Fr minus_one = [&] {  // r - 1 = the additive inverse of one: found as x with x + 1 == 0 through sub
    Fr one = fr.one(), zero = fr.zero(), out;
    check(amsm_fr_sub(fr.curve, zero.data(), one.data(), 1, out.data()), "amsm_fr_sub");
    return out;
  }();
  for (size_t k = 0; k < K; k++) {
    std::vector<Fr> p = vecs[k].to_host(), q = quots[k].to_host();
    if (q.size() != (lens[k] ? lens[k] - 1 : 0) || quots_async[k].to_host() != q) return printf("FAIL quotient length / async %zu\n", k), 1;
    Fr value = poly_evaluate(ctx, {&vecs[k]}, zs[k])[0], single_rem;
    if (value != rems[k]) return printf("FAIL remainder != value %zu\n", k), 1;
    FrVector q1(ctx, q.size());
    check(amsm_poly_div_linear(ctx.get(), vecs[k].ptr(), lens[k], zs[k].data(), q1.ptr(), single_rem.data()), "amsm_poly_div_linear");
    if (single_rem != rems[k] || q1.to_host() != q) return printf("FAIL single != batch %zu\n", k), 1;
    check(amsm_poly_evaluate(ctx.get(), vecs[k].ptr(), lens[k], zs[k].data(), single_rem.data()), "amsm_poly_evaluate");
    if (single_rem != value) return printf("FAIL single evaluate %zu\n", k), 1;
    const Fr mz = fr.mul(minus_one, zs[k]);
    for (size_t i = 0; i < lens[k]; i++) {  // p[i] = q[i-1] - z q[i]  (q[-1] = rem, q[n-1] = 0)
      Fr want = i ? q[i - 1] : rems[k];
      if (i < q.size()) want = fr.add(want, fr.mul(mz, q[i]));
      if (want != p[i]) return printf("FAIL identity %zu at %zu\n", k, i), 1;
    }
    printf("value %zu %016llx %016llx %016llx %016llx\n", k, (unsigned long long)value[0], (unsigned long long)value[1],
           (unsigned long long)value[2], (unsigned long long)value[3]);
  }
  std::vector<Fr> all = poly_evaluate(ctx, ptrs, zs[0]);
  for (size_t k = 0; k < K; k++)
    if (all[k] != poly_evaluate(ctx, {&vecs[k]}, zs[0])[0]) return printf("FAIL batch evaluate %zu\n", k), 1;
  // argument errors come back before anything is launched
  const void* none = nullptr;
  size_t two = 2;
  void* noq = nullptr;
  Fr out;
  if (amsm_poly_div_linear_batch(ctx.get(), &none, &two, 1, zs[0].data(), &noq, out.data()) != AMSM_E_INVALID_ARG ||
      amsm_poly_evaluate_batch(ctx.get(), nullptr, nullptr, 1, zs[0].data(), out.data()) != AMSM_E_INVALID_ARG ||
      amsm_poly_evaluate_batch(ctx.get(), nullptr, nullptr, 0, zs[0].data(), nullptr) != AMSM_OK)
    return printf("FAIL argument checks\n"), 1;
  printf("done\n");
  return 0;
}
