// CPU check of the GLV set-up (accumulation_amd/csrc/host_glv.h) on one curve of tests/curve_rows.py against the host group law:
// lambda and beta pair up on the curve table's generator, [lambda] G = (beta Gx, Gy), and the split k = k1 + k2 lambda holds with
// short halves for the scalars at the ends and the middle of the scalar field.  Prints lambda and beta (canonical, hex) for the Python
// side to check against the big-int oracle.  Built once per row, with the row's field packs as -DGLV_FQ=... -DGLV_FR=..., and run by
// tests/curve_cases_cpu.py::test_glv_pairing_and_split (no GPU, no libamsm.so); the device's use of the split is checked through
// the key folds of tests/curve_cases_gpu.py.
#include <stdio.h>

#include "host_glv.h"

using namespace amsm;
using namespace amsm::host;
using Fq = GLV_FQ;
using Fr = GLV_FR;

template <class F>
static void print_hex(const HFe<F>& mont) {
  HFe<F> c = h_from_mont<F>(mont);
  printf("0x");
  for (int i = HFe<F>::N - 1; i >= 0; i--) printf("%016llx", (unsigned long long)c.v[i]);
}

int main() {
  constexpr int NQ = HFe<Fq>::N, NR = HFe<Fr>::N;  // 64-bit words of a coordinate and of a scalar
  static_assert(NR == 4, "the edge scalars below are written as four words");
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
  u64 lam[NR];
  memcpy(lam, lc.v, sizeof(lam));
  u64 lg[2 * NQ];
  uint8_t inf = 0;
  hx_to_affine<Fq>(hx_mul<Fq>(G, lam), lg, &inf);
  HFe<Fq> gx;
  memcpy(gx.v, gen, 8 * NQ);
  HFe<Fq> bgx = h_mul<Fq>(glv.beta, gx);
  if (inf || memcmp(lg, bgx.v, 8 * NQ) || memcmp(lg + NQ, gen + NQ, 8 * NQ)) return printf("pairing FAIL\n"), 1;

  // the split: decompose() verifies k1 + k2 lambda = k itself; here the halves are short (the masks of a fold hold 160 digits) and
  // [k1] G + [k2] (beta Gx, Gy) = [k] G on the group.  With 2^k < r < 2^(k + 1) (k = 254, 253 or 252), every scalar below is below r.
  u64 r[NR], ks[9][NR];
  for (int i = 0; i < NR; i++) r[i] = hmod<Fr>(i);
  const int top = 63 - __builtin_clzll(r[NR - 1]);  // bit k - 192 of the top word
  auto set = [&](int at, u64 a, u64 b, u64 c, u64 d) { ks[at][0] = a, ks[at][1] = b, ks[at][2] = c, ks[at][3] = d; };
  set(0, 0, 0, 0, 0);
  set(1, 1, 0, 0, 0);
  set(2, 2, 0, 0, 0);
  set(3, r[0] - 1, r[1], r[2], r[3]);  // r - 1 (r is odd and its low word is above 1: no borrow)
  set(4, r[0] - 2, r[1], r[2], r[3]);  // r - 2
  for (int i = 0; i < NR; i++) ks[5][i] = (r[i] >> 1) | (i < NR - 1 ? r[i + 1] << 63 : 0);  // (r - 1) / 2
  memcpy(ks[6], ks[5], sizeof(ks[6]));
  ks[6][0] += 1;                       // (r + 1) / 2
  set(7, 0, 0, 0, 1ull << top);        // 2^k
  set(8, 0x0123456789abcdefull, 0xfedcba9876543210ull, 0x0f1e2d3c4b5a6978ull, ((r[3] >> 60) << 60) - 1);  // 0x2fff.., 0x0fff.. on BLS12-377
  HXYZZ<Fq> phiG = hx_from_affine<Fq>(lg, false);
  for (int t = 0; t < 9; t++) {
    Big k1, k2;
    if (!glv.decompose(ks[t], k1, k2)) return printf("split FAIL at %d\n", t), 1;
    if (big_bits(k1) > 131 || big_bits(k2) > 131) return printf("long half at %d: %d %d bits\n", t, big_bits(k1), big_bits(k2)), 1;
    HXYZZ<Fq> sum = hx_inf<Fq>();
    for (int half = 0; half < 2; half++) {
      const Big& k = half ? k2 : k1;
      u64 m[NR];
      for (int i = 0; i < NR; i++) m[i] = (u64)k.w[2 * i] | ((u64)k.w[2 * i + 1] << 32);
      HXYZZ<Fq> part = hx_mul<Fq>(half ? phiG : G, m);
      if (k.neg) part = hx_neg<Fq>(part);
      sum = hx_add<Fq>(sum, part);
    }
    u64 a[2 * NQ], b[2 * NQ];
    uint8_t ai = 0, bi = 0;
    hx_to_affine<Fq>(sum, a, &ai);
    hx_to_affine<Fq>(hx_mul<Fq>(G, ks[t]), b, &bi);
    if (ai != bi || (!ai && memcmp(a, b, sizeof(a)))) return printf("split point FAIL at %d\n", t), 1;
  }

  printf("OK\n");
  return 0;
}
