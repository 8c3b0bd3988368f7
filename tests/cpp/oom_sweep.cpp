// The out-of-memory sweep of tests/oom_sweep.py written against the C ABI (include/amsm.h) and the C++ wrappers (include/amsm.hpp):
// for every family, refuse the k-th allocation request of the call for k = 0, 1, 2, ... (amsm_ctx_fail_alloc_after) and check the
// contract after AMSM_E_OOM -- *out untouched, nothing held after a trim, the context still computes the known point -- and that a
// call that succeeds, with or without a tolerated refusal, gives what a clean call gave.  Runs on the host backend by default
// (AMSM_CHECK_DEVICE=-1; a device id runs the same sweeps on a GPU).  No Python, nothing preloaded: this is the program to build
// with -fsanitize=address,undefined together with the library's host side -- error paths are where leaks and double frees live.
// Prints one line per family and "done"; exits non-zero at the first broken promise.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "amsm.h"
#include "amsm.hpp"

namespace {

constexpr uintptr_t SENTINEL = 0x5E7712E0u;
constexpr int CAP = 200;

[[noreturn]] void die(const std::string& what) {
  std::fprintf(stderr, "oom_sweep: %s\n", what.c_str());
  std::exit(1);
}
void ok(int rc, const char* where) {
  if (rc != AMSM_OK) die(std::string(where) + ": " + amsm_strerror(rc));
}

struct Probe {  // a 64-pair MSM over a 64-generator key made beforehand
  amsm_ctx* c;
  amsm_bases* key = nullptr;
  void* vec = nullptr;
  std::vector<uint64_t> want;
  uint8_t want_inf = 0;
  explicit Probe(amsm_ctx* ctx) : c(ctx), want(2 * (size_t)amsm_ctx_fq_limbs(ctx)) {
    ok(amsm_bases_generate(c, 0x9B0BE, 64, AMSM_BASES_DEFAULT, &key), "probe key");
    ok(amsm_dev_alloc(c, 64 * 32, &vec), "probe vector");
    ok(amsm_vec_random(c, 0x9B0BF, 64, 0, vec), "probe scalars");
    ok(amsm_msm_device(c, key, 0, vec, 64, 0, want.data(), &want_inf), "probe MSM");
  }
  void run(const std::string& where) const {
    std::vector<uint64_t> got(want.size());
    uint8_t inf = 0;
    const int rc = amsm_msm_device(c, key, 0, vec, 64, 0, got.data(), &inf);
    if (rc != AMSM_OK) die(where + ": the probe MSM returned " + amsm_strerror(rc));
    if (inf != want_inf || got != want) die(where + ": the probe MSM gave a wrong point");
  }
  ~Probe() {
    amsm_dev_free(c, vec);
    amsm_bases_free(key);
  }
};

// call() -> status; on AMSM_OK check() compares with the clean result and release() gives the product back
struct Family {
  std::string name;
  std::function<int()> call;
  std::function<void()> check;
  std::function<void()> release;
  bool require_oom = true;
};

void sweep(amsm::Context& ctx, const Probe& probe, const Family& f) {
  int n_oom = 0, n_tolerated = 0;
  for (int k = 0; k < CAP; k++) {
    ok(amsm_ctx_trim(ctx.get()), "amsm_ctx_trim");
    const size_t held = ctx.memory_held().held;
    const amsm::Context::AllocStats before = ctx.alloc_stats();
    ctx.fail_alloc_after(k);
    const int rc = f.call();
    ctx.fail_alloc_after(-1);
    const amsm::Context::AllocStats after = ctx.alloc_stats();
    const bool fired = after.refused_by_hook > before.refused_by_hook;
    const std::string where = f.name + ", request " + std::to_string(k);
    if (rc != AMSM_OK && rc != AMSM_E_OOM) die(where + ": status " + amsm_strerror(rc));
    if (after.refused_by_limit != before.refused_by_limit || after.failed_in_driver != before.failed_in_driver)
      die(where + ": a refusal that was not the hook's");
    if (rc == AMSM_E_OOM) {
      if (!fired) die(where + ": AMSM_E_OOM without a refused request");
      n_oom++;
      ok(amsm_ctx_trim(ctx.get()), "amsm_ctx_trim");
      if (ctx.memory_held().held != held) die(where + ": bytes still held after AMSM_E_OOM and a trim");
      probe.run(where);
      continue;
    }
    f.check();
    if (f.release) f.release();
    if (!fired) {
      if (f.require_oom && !n_oom) die(f.name + ": no iteration returned AMSM_E_OOM");
      probe.run(where);
      std::printf("family %s oom %d tolerated %d iterations %d\n", f.name.c_str(), n_oom, n_tolerated, k + 1);
      return;
    }
    n_tolerated++;
  }
  die(f.name + ": still refusing after " + std::to_string(CAP) + " iterations");
}

}  // namespace

int main() {
  const char* dev = std::getenv("AMSM_CHECK_DEVICE");
  const int device = dev ? std::atoi(dev) : AMSM_DEVICE_HOST;
  try {
    amsm::Context ctx(AMSM_PALLAS, device);
    amsm_ctx* c = ctx.get();
    const size_t L2 = 2 * (size_t)ctx.fq_limbs(), n = 1 << 10;
    Probe probe(c);

    // ---- the wrappers themselves: limit, books, statistics ----
    {
      const amsm::Context::MemoryHeld h0 = ctx.memory_held();
      ctx.set_memory_limit(h0.held + 1000);
      void* const untouched_ptr = reinterpret_cast<void*>(SENTINEL);
      void* p = untouched_ptr;
      if (amsm_dev_alloc(c, 4096, &p) != AMSM_E_OOM) die("a request past the limit was not refused");
      if (p != untouched_ptr) die("a refused amsm_dev_alloc wrote *d_ptr");
      if (ctx.alloc_stats().refused_by_limit != 1 || ctx.memory_held().limit != h0.held + 1000) die("limit statistics");
      ctx.set_memory_limit(0);
      ok(amsm_dev_alloc(c, 4096, &p), "amsm_dev_alloc");
      if (ctx.memory_held().held != h0.held + 4096) die("held bytes do not follow amsm_dev_alloc");
      ok(amsm_dev_free(c, p), "amsm_dev_free");
      bool threw = false;
      ctx.fail_alloc_after(0);
      try {
        amsm::FrVector v(ctx, 100);
      } catch (const amsm::Error&) {
        threw = true;
      }
      if (!threw) die("amsm::FrVector did not throw on a refused request");
    }

    // ---- keys ----
    std::vector<uint64_t> xy(n * L2), got(n * L2);
    std::vector<uint8_t> inf(n);
    {
      amsm_bases* ref = nullptr;
      ok(amsm_bases_generate(c, 0x6E11, n, AMSM_BASES_DEFAULT, &ref), "reference key");
      ok(amsm_bases_read(c, ref, 0, n, xy.data(), inf.data()), "amsm_bases_read");
      amsm_bases_free(ref);
    }
    amsm_bases* out = nullptr;
    auto arm = [&] { out = reinterpret_cast<amsm_bases*>(SENTINEL); };
    auto untouched = [&](int rc, const char* who) {
      if (rc != AMSM_OK && out != reinterpret_cast<amsm_bases*>(SENTINEL)) die(std::string(who) + ": a failing creator wrote *out");
      return rc;
    };
    const std::vector<uint64_t>* want_xy = &xy;
    auto check_key = [&] {
      ok(amsm_bases_read(c, out, 0, amsm_bases_len(out), got.data(), inf.data()), "amsm_bases_read");
      if (std::memcmp(got.data(), want_xy->data(), amsm_bases_len(out) * L2 * 8) != 0) die("a key's points differ from the clean key's");
    };
    auto free_key = [&] { amsm_bases_free(out); };
    sweep(ctx, probe, {"amsm_bases_generate", [&] { arm(); return untouched(amsm_bases_generate(c, 0x6E11, n, AMSM_BASES_DEFAULT, &out), "generate"); },
                       check_key, free_key});
    sweep(ctx, probe, {"amsm_bases_load|CHECK", [&] { arm(); return untouched(amsm_bases_load(c, xy.data(), nullptr, n, AMSM_BASES_CHECK, &out), "load"); },
                       check_key, free_key});
    {
      void* d_xy = nullptr;
      ok(amsm_dev_alloc(c, n * L2 * 8, &d_xy), "amsm_dev_alloc");
      ok(amsm_dev_upload(c, d_xy, xy.data(), n * L2 * 8), "amsm_dev_upload");
      sweep(ctx, probe, {"amsm_bases_from_device", [&] { arm(); return untouched(amsm_bases_from_device(c, d_xy, n, AMSM_BASES_CHECK, &out), "from_device"); },
                         check_key, free_key});
      ok(amsm_dev_free(c, d_xy), "amsm_dev_free");
    }
    {
      std::vector<uint64_t> sxy(n * L2);
      amsm_bases* ref = nullptr;
      const uint8_t dom[] = "oom-sweep";
      ok(amsm_bases_sample(c, dom, 9, 0, n, AMSM_BASES_DEFAULT, &ref), "reference sampled key");
      ok(amsm_bases_read(c, ref, 0, n, sxy.data(), inf.data()), "amsm_bases_read");
      amsm_bases_free(ref);
      want_xy = &sxy;
      sweep(ctx, probe, {"amsm_bases_sample", [&] { arm(); return untouched(amsm_bases_sample(c, dom, 9, 0, n, AMSM_BASES_DEFAULT, &out), "sample"); },
                         check_key, free_key});
      want_xy = &xy;
    }
    {
      amsm_bases* full = nullptr;
      ok(amsm_bases_generate(c, 0x6E11, n, AMSM_BASES_NO_PRECOMPUTE, &full), "key to fold");
      const uint64_t x[4] = {0xDEADBEEF12345ull, 0, 0, 1};
      std::vector<uint64_t> fxy(n / 2 * L2);
      amsm_bases* ref = nullptr;
      ok(amsm_bases_fold(c, full, n / 2, x, 255, &ref), "reference fold");
      ok(amsm_bases_read(c, ref, 0, n / 2, fxy.data(), inf.data()), "amsm_bases_read");
      amsm_bases_free(ref);
      want_xy = &fxy;
      sweep(ctx, probe, {"amsm_bases_fold", [&] { arm(); return untouched(amsm_bases_fold(c, full, n / 2, x, 255, &out), "fold"); }, check_key, free_key});
      want_xy = &xy;
      amsm_bases_free(full);
    }

    // ---- a matrix ----
    {
      const size_t rows = n, per = 3;
      std::vector<uint32_t> row_ptr(rows + 1), col(rows * per);
      std::vector<uint64_t> vals(rows * per * 4, 0);
      for (size_t r = 0; r <= rows; r++) row_ptr[r] = (uint32_t)(r * per);
      for (size_t k = 0; k < rows * per; k++) {
        col[k] = (uint32_t)((k * 7 + 3) % 64);
        vals[4 * k] = k + 1;
      }
      amsm_matrix* m = nullptr;
      void *inp = nullptr, *wit = nullptr, *res = nullptr;
      ok(amsm_dev_alloc(c, 16 * 32, &inp), "amsm_dev_alloc");
      ok(amsm_dev_alloc(c, 48 * 32, &wit), "amsm_dev_alloc");
      ok(amsm_dev_alloc(c, rows * 32, &res), "amsm_dev_alloc");
      ok(amsm_vec_random(c, 71, 16, 1, inp), "amsm_vec_random");
      ok(amsm_vec_random(c, 72, 48, 1, wit), "amsm_vec_random");
      std::vector<uint64_t> want(rows * 4), have(rows * 4);
      ok(amsm_matrix_load(c, row_ptr.data(), col.data(), vals.data(), rows, rows * per, &m), "reference matrix");
      ok(amsm_matrix_vec_mul(c, m, inp, 16, wit, 48, res), "amsm_matrix_vec_mul");
      ok(amsm_dev_download(c, want.data(), res, rows * 32), "amsm_dev_download");
      amsm_matrix_free(m);
      auto sentinel = reinterpret_cast<amsm_matrix*>(SENTINEL);
      sweep(ctx, probe,
            {"amsm_matrix_load",
             [&] {
               m = sentinel;
               const int rc = amsm_matrix_load(c, row_ptr.data(), col.data(), vals.data(), rows, rows * per, &m);
               if (rc != AMSM_OK && m != sentinel) die("amsm_matrix_load: a failing call wrote *out");
               return rc;
             },
             [&] {
               ok(amsm_matrix_vec_mul(c, m, inp, 16, wit, 48, res), "amsm_matrix_vec_mul");
               ok(amsm_dev_download(c, have.data(), res, rows * 32), "amsm_dev_download");
               if (have != want) die("amsm_matrix_load: A z differs from the clean matrix's");
             },
             [&] { amsm_matrix_free(m); }});
      for (void* p : {inp, wit, res}) ok(amsm_dev_free(c, p), "amsm_dev_free");
    }

    // ---- MSMs: device scalars over plain and default keys, host slices, the one-shot form ----
    {
      amsm_bases* key = nullptr;
      ok(amsm_bases_generate(c, 0x6B12, 1 << 12, AMSM_BASES_NO_PRECOMPUTE, &key), "MSM key");
      void* vec = nullptr;
      ok(amsm_dev_alloc(c, (1 << 12) * 32, &vec), "amsm_dev_alloc");
      ok(amsm_vec_random(c, 0xD2, 1 << 12, 0, vec), "amsm_vec_random");
      std::vector<uint64_t> hs((1 << 12) * 4), want(L2), have(L2), kxy((size_t)(1 << 12) * L2);
      std::vector<uint8_t> kinf(1 << 12);
      ok(amsm_dev_download(c, hs.data(), vec, hs.size() * 8), "amsm_dev_download");
      ok(amsm_bases_read(c, key, 0, 1 << 12, kxy.data(), kinf.data()), "amsm_bases_read");
      uint8_t winf = 0, hinf = 0;
      ok(amsm_msm_device(c, key, 0, vec, 1 << 12, 0, want.data(), &winf), "reference MSM");
      auto same = [&] {
        if (hinf != winf || have != want) die("an MSM differs from the clean one");
      };
      // (the host backend's MSM works in scratch the gate does not cover: no request of its own there)
      const bool host = amsm_ctx_is_host(c) != 0;
      sweep(ctx, probe, {"amsm_msm_device", [&] { return amsm_msm_device(c, key, 0, vec, 1 << 12, 0, have.data(), &hinf); }, same, nullptr, !host});
      sweep(ctx, probe, {"amsm_msm", [&] { return amsm_msm(c, key, 0, hs.data(), 1 << 12, 0, have.data(), &hinf); }, same, nullptr, !host});
      sweep(ctx, probe, {"amsm_msm_oneshot",
                         [&] { return amsm_msm_oneshot(c, kxy.data(), nullptr, 1 << 12, hs.data(), 1 << 12, 0, have.data(), &hinf); }, same, nullptr});
      ok(amsm_dev_free(c, vec), "amsm_dev_free");
      amsm_bases_free(key);
    }
    ok(amsm_ctx_trim(c), "amsm_ctx_trim");
  } catch (const amsm::Error& e) {
    die(std::string("amsm::Error: ") + e.what());
  }
  std::printf("done\n");
  return 0;
}
