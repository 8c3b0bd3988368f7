// The C++ drivers with a VectorRng (include/amsm_hp_as.hpp): R1CSNark::prove with make_zk and a hiding InnerProductArgPC::open take
// their long random vectors from FrVector::sample (amsm_vec_sample, "amsm-blind-v1") instead of the rng.  Each proof is verified here
// and printed serialised, for the byte-for-byte comparison with the Python mirrors under the same key and rng
// (tests/test_vec_sample_cpu.py).  One VectorRng serves both proves: the NARK takes stream 0, the opening stream 1.
#include <cstdio>

#include "amsm_ipa_pc_as.hpp"
#include "amsm_r1cs_nark.hpp"
#include "amsm_serialize.hpp"

#include "check_device.hpp"

using namespace amsm;
using Sponge = hp_as::Sha256Sponge;
using Nark = r1cs_nark::R1CSNark<Sponge>;
using Ipa = ipa_pc::InnerProductArgPC<Sponge>;

struct SchemeRng {  // tests/test_hp_as_scheme_gpu.py:SchemeRng
  uint64_t seed, i = 0;
  explicit SchemeRng(uint64_t s) : seed(s) {}
  Fr field() {
    Fr x;
    for (uint64_t k = 0; k < 4; k++) {
      uint64_t z = seed * 0xD1342543DE82EF95ull + (4 * i + k) * 0x9E3779B97F4A7C15ull + 0x632BE59BD9B4E019ull;
      z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
      z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
      z ^= z >> 31;
      x[k] = z;
    }
    i++;
    x[3] &= (1ull << 62) - 1;
    return x;
  }
};

static void print_bytes(const char* name, const std::vector<uint8_t>& b) {
  printf("%s ", name);
  for (uint8_t v : b) printf("%02x", v);
  printf("\n");
}

int main() {
  try {
    Context ctx = check_context(AMSM_PALLAS);
    hp_as::FrOps fr{amsm_ctx_curve(ctx.get())};
    hp_as::VectorRng vrng;
    for (int k = 0; k < 32; k++) vrng.key[k] = (uint8_t)k;
    const Fr one = {1, 0, 0, 0};
    {  // the DummyCircuit with 2^6 constraints and a witness of 2^6 variables [a, b, a, .., a]
      const size_t n_con = 64, n_inst = 6, n_wit = n_con;
      std::vector<r1cs_nark::Matrix::Row> A, B, C;
      for (size_t k = 0; k + 1 < n_con; k++) {
        A.push_back({{one, n_inst + 0}});
        B.push_back({{one, n_inst + 1}});
        C.push_back({{one, 1}});
      }
      A.push_back({});
      B.push_back({});
      C.push_back({});
      r1cs_nark::IndexProverKey ipk = Nark::index(ctx, A, B, C, n_inst, n_inst + n_wit, 31337);
      const Fr a = {0x1234567, 0, 0, 0}, b = {0x7654321, 0, 0, 0};
      Fr am = fr.to_mont(a), bm = fr.to_mont(b), abm = fr.mul(am, bm), ab;
      check(amsm_fr_from_mont(amsm_ctx_curve(ctx.get()), abm.data(), 1, ab.data()), "from_mont");
      std::vector<Fr> inst{one, ab, a, a, a, a};
      std::vector<Fr> w(n_wit, am);
      w[1] = bm;
      SchemeRng rng(11);
      hp_as::Rng prng([&rng]() { return rng.field(); });
      r1cs_nark::Proof proof = Nark::prove(ipk, inst, std::make_shared<FrVector>(ctx, w), prng, Sponge(), &vrng);
      printf("nark_verified %d\n", Nark::verify(ipk, inst, proof) ? 1 : 0);
      print_bytes("nark_proof", ser::serialize(ctx, proof));
    }
    {  // a hiding opening of a polynomial of degree 2^6 - 1
      const size_t degree = 63;
      ipa_pc::FrX fx(amsm_ctx_curve(ctx.get()));
      ipa_pc::CommitterKey ck = Ipa::trim(Ipa::setup(ctx, degree, 0x1BA5EED), degree);
      FrVector poly = FrVector::random(ctx, 77, degree + 1, true);
      SchemeRng rng(12);
      hp_as::Rng prng([&rng]() { return rng.field(); });
      auto cr = Ipa::commit(ck, poly, true, prng);
      const Fr point = fx.to_mont(Fr{0xABCDEF, 0, 0, 0});
      FrVector z(ctx, degree + 1);
      check(amsm_vec_powers(ctx.get(), point.data(), degree + 1, z.ptr()), "amsm_vec_powers");
      Fr value;
      check(amsm_vec_inner_product(ctx.get(), poly.ptr(), z.ptr(), degree + 1, value.data()), "amsm_vec_inner_product");
      ipa_pc::Proof proof = Ipa::open(ck, poly, cr.first, point, cr.second, true, prng, &vrng);
      printf("ipa_verified %d\n", (Ipa::check(ck, cr.first, point, value, proof) && vrng.next_stream == 2) ? 1 : 0);
      print_bytes("ipa_proof", ser::serialize(ctx, proof));
    }
    return 0;
  } catch (const std::exception& e) {
    printf("exception %s\n", e.what());
    return 1;
  }
}
