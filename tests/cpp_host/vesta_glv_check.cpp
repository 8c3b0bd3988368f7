// CPU check of the GLV set-up (accumulation_amd/csrc/host_glv.h) on Vesta against the host group law: lambda and beta pair up on
// the curve table's generator, [lambda] G = (beta Gx, Gy).  Prints lambda and beta (canonical, hex) for the Python side to check
// against the big-int oracle.  Built and run by tests/test_vesta_cpu.py (no GPU, no libamsm.so); the split itself is checked
// through the key folds of tests/test_vesta_gpu.py.
#include <stdio.h>

#include "host_glv.h"

using namespace amsm;
using namespace amsm::host;
using Fq = VestaFq;
using Fr = VestaFr;

template <class F>
static void print_hex(const HFe<F>& mont) {
  HFe<F> c = h_from_mont<F>(mont);
  printf("0x");
  for (int i = HFe<F>::N - 1; i >= 0; i--) printf("%016llx", (unsigned long long)c.v[i]);
}

int main() {
  constexpr int NQ = HFe<Fq>::N;
  std::vector<u32> g32 = generator_mont<Fq>();
  if (g32.size() != 2 * (size_t)Fq::L) return printf("no generator\n"), 1;
  u64 gen[2 * NQ];
  memcpy(gen, g32.data(), sizeof(gen));
  Glv<Fq, Fr> glv;
  glv.setup(gen);
  if (!glv.ok) return printf("set-up failed\n"), 1;
  printf("lambda ");
  print_hex<Fr>(glv.lambda);
  printf(" beta ");
  print_hex<Fq>(glv.beta);
  printf("\n");

  // [lambda] G == (beta Gx, Gy)
  HXYZZ<Fq> G = hx_from_affine<Fq>(gen, false);
  HFe<Fr> lc = h_from_mont<Fr>(glv.lambda);
  u64 lam[4];
  memcpy(lam, lc.v, 32);
  u64 lg[2 * NQ];
  uint8_t inf = 0;
  hx_to_affine<Fq>(hx_mul<Fq>(G, lam), lg, &inf);
  HFe<Fq> gx;
  memcpy(gx.v, gen, 8 * NQ);
  HFe<Fq> bgx = h_mul<Fq>(glv.beta, gx);
  if (inf || memcmp(lg, bgx.v, 8 * NQ) || memcmp(lg + NQ, gen + NQ, 8 * NQ)) return printf("pairing FAIL\n"), 1;

  printf("OK\n");
  return 0;
}
