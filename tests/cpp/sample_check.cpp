// Transparent keys through the wrappers of include/amsm.hpp and the scheme headers: CommitterKey::sample (a window of a longer
// key equals a key sampled with the matching `first`), PedersenCommitment / TrivialPC / InnerProductArgPC::setup_transparent
// (generators G_0 .. G_(n-1), the hiding generators at G_n and G_(n+1), as the seeded setups place theirs), a commitment over a
// sampled key against the same points loaded, and the argument errors.  Prints the values so that a test can compare the GPU
// with the host backend.
#include <cstdio>

#include "amsm_ipa_pc_as.hpp"
#include "amsm_trivial_pc_as.hpp"
#include "check_device.hpp"

using namespace amsm;

static void print_point(const char* what, const uint64_t* xy, size_t words) {
  printf("value %s", what);
  for (size_t i = 0; i < words; i++) printf(" %016llx", (unsigned long long)xy[i]);
  printf("\n");
}

int main() {
  const std::string domain = "amsm-test";
  for (int curve : {AMSM_PALLAS, AMSM_BLS12_381_G1, AMSM_VESTA}) {
    Context ctx(curve, check_device());
    const size_t w = 2 * (size_t)ctx.fq_limbs(), n = 1000;
    CommitterKey key = CommitterKey::sample(ctx, domain, n);
    if (key.supported_num_elems() != n) return printf("FAIL length %d\n", curve), 1;
    const std::vector<uint64_t> all = key.read(0, n);
    const std::vector<uint64_t> window = CommitterKey::sample_points(ctx, domain, 700, 50);
    if (!std::equal(window.begin(), window.end(), all.begin() + (long)(700 * w))) return printf("FAIL window %d\n", curve), 1;
    if (CommitterKey::sample_points(ctx, "other", 0, 4) == std::vector<uint64_t>(all.begin(), all.begin() + (long)(4 * w)))
      return printf("FAIL domains %d\n", curve), 1;
    for (size_t i : {(size_t)0, (size_t)1, n - 1}) {
      char name[32];
      snprintf(name, sizeof(name), "c%d G_%zu", curve, i);
      print_point(name, all.data() + i * w, w);
    }
    // the setups: generators and hiding generators at the seeded setups' positions
    CommitterKey ped = PedersenCommitment::setup_transparent(ctx, 256, domain);
    if (ped.supported_num_elems() != 256 || ped.read(0, 256) != std::vector<uint64_t>(all.begin(), all.begin() + (long)(256 * w)) ||
        ped.hiding_generator != std::vector<uint64_t>(all.begin() + (long)(256 * w), all.begin() + (long)(257 * w)))
      return printf("FAIL pedersen setup %d\n", curve), 1;
    CommitterKey triv = trivial_pc_as::TrivialPC::setup_transparent(ctx, 99, domain);
    if (triv.supported_num_elems() != 100 || triv.hiding_generator != std::vector<uint64_t>(all.begin() + (long)(100 * w), all.begin() + (long)(101 * w)))
      return printf("FAIL trivial_pc setup %d\n", curve), 1;
    auto ipa = ipa_pc::InnerProductArgPC<>::setup_transparent(ctx, 100, domain);  // 128 generators, h = G_128, s = G_129
    if (ipa.max_degree != 127 || ipa.comm_key->supported_num_elems() != 128 ||
        ipa.comm_key->read(0, 128) != std::vector<uint64_t>(all.begin(), all.begin() + (long)(128 * w)) ||
        ipa.h.xy != std::vector<uint64_t>(all.begin() + (long)(128 * w), all.begin() + (long)(129 * w)) ||
        ipa.s.xy != std::vector<uint64_t>(all.begin() + (long)(129 * w), all.begin() + (long)(130 * w)))
      return printf("FAIL ipa_pc setup %d\n", curve), 1;
    // a hiding commitment over the sampled key == over the same points loaded
    CommitterKey loaded = CommitterKey::load(ctx, ped.read(0, 256), nullptr);
    loaded.hiding_generator = ped.hiding_generator;
    FrVector v = FrVector::random(ctx, 31 + (uint64_t)curve, 256, true);
    const Fr rnd = FrVector::random(ctx, 77, 1, true).to_host()[0];
    Affine a = PedersenCommitment::commit(ped, v, &rnd), b = PedersenCommitment::commit(loaded, v, &rnd);
    if (a.infinity || a.infinity != b.infinity || a.xy != b.xy) return printf("FAIL commit %d\n", curve), 1;
    char name[32];
    snprintf(name, sizeof(name), "c%d commit", curve);
    print_point(name, a.xy.data(), w);
    // argument errors come back before anything is launched
    amsm_bases* out = nullptr;
    const uint8_t dom[40] = {0};
    if (amsm_bases_sample(ctx.get(), dom, 33, 0, 4, AMSM_BASES_NO_PRECOMPUTE, &out) != AMSM_E_INVALID_ARG ||
        amsm_bases_sample(ctx.get(), nullptr, 1, 0, 4, AMSM_BASES_NO_PRECOMPUTE, &out) != AMSM_E_INVALID_ARG ||
        amsm_bases_sample(ctx.get(), dom, 4, 0, 4, 32u, &out) != AMSM_E_INVALID_ARG ||
        amsm_bases_sample(ctx.get(), dom, 4, 0, (size_t)1 << 31, AMSM_BASES_NO_PRECOMPUTE, &out) != AMSM_E_UNSUPPORTED || out)
      return printf("FAIL errors %d\n", curve), 1;
    bool threw = false;
    try {
      CommitterKey::sample(ctx, std::string(33, 'x'), 4);
    } catch (const Error&) {
      threw = true;
    }
    if (!threw) return printf("FAIL wrapper error %d\n", curve), 1;
    CommitterKey empty = CommitterKey::sample(ctx, "", 0);
    if (empty.supported_num_elems() != 0) return printf("FAIL empty %d\n", curve), 1;
  }
  printf("done\n");
  return 0;
}
