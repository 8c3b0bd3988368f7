// Prints how the host recodes the scalar of a key fold (accumulation_amd/csrc/fold_recode.h, and host_glv.h for the GLV form) for the
// cases of a file that tests/test_fold_recode_cpu.py writes, one per line:
//   plain NBITS X                 the plain non-adjacent form of the low NBITS bits of X (fold_low_bits + fold_digits_plain)
//   tab C W NN LEVELS NBITS X     the op list of the table ladder (fold_tab_ops)
//   fold CURVE NBITS X            what a fold on that curve launches with (fold_digits<Fq>): GLV above 140 bits, else the plain form
// X in hex, below 2^256.  Built twice from this one source: plain `g++ -Wall -Werror` over fold_recode.h alone (no HIP, no library)
// answers the `plain` and `tab` lines; with -DFOLD_RECODE_GLV and the host side of hipcc it answers the `fold` lines of all six curves
// and prints each curve's lambda and beta in canonical form.  Masks and field elements are printed as hex integers, ops as four hex
// digits each.  A refused table case prints ok=0 and must have left the structure zeroed: anything else ends the run with status 2.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#ifdef FOLD_RECODE_GLV
#include "host_glv.h"
#else
#include "../../accumulation_amd/csrc/fold_recode.h"
#endif

using namespace amsm;

static void parse_hex(const char* s, u32 out[8]) {
  memset(out, 0, 32);
  if (s[0] == '0' && s[1] == 'x') s += 2;
  const int n = (int)strlen(s);
  for (int i = 0; i < n && i < 64; i++) {
    const char ch = s[n - 1 - i];
    const u32 v = ch <= '9' ? (u32)(ch - '0') : (u32)((ch | 0x20) - 'a' + 10);
    out[i >> 3] |= v << (4 * (i & 7));
  }
}
static void print_hex(const char* name, const u32* w, int n) {
  printf(" %s=", name);
  int top = n - 1;
  while (top > 0 && w[top] == 0) top--;
  printf("%x", w[top]);
  for (int i = top - 1; i >= 0; i--) printf("%08x", w[i]);
}
static void print_digits(const FoldDigits& d) {
  printf(" nd=%u", d.nd);
  print_hex("pos1", d.pos1, 8);
  print_hex("neg1", d.neg1, 8);
  print_hex("pos2", d.pos2, 5);
  print_hex("neg2", d.neg2, 5);
  print_hex("beta", d.beta, 12);
  printf("\n");
}

#ifdef FOLD_RECODE_GLV
template <class F>
static void print_canonical(const char* name, const host::HFe<F>& mont) {
  const host::HFe<F> c = host::h_from_mont<F>(mont);
  u32 w[2 * host::HFe<F>::N];
  memcpy(w, c.v, sizeof(w));
  print_hex(name, w, 2 * host::HFe<F>::N);
}
template <class Fq>
static int run_curve(const char* curve, const char* path) {
  const auto& g = host::curve_glv<Fq>();
  if (!g.ok) return printf("curve %s: set-up failed\n", curve), 1;
  printf("curve %s", curve);
  print_canonical("lambda", g.lambda);
  print_canonical("beta", g.beta);
  printf("\n");
  FILE* f = fopen(path, "r");
  if (!f) return 1;
  char kind[16], name[32], xs[80];
  unsigned nbits;
  char line[256];
  while (fgets(line, sizeof(line), f)) {
    if (sscanf(line, "%15s %31s %u %79s", kind, name, &nbits, xs) != 4 || strcmp(kind, "fold") || strcmp(name, curve)) continue;
    u32 x[8];
    parse_hex(xs, x);
    FoldDigits d;
    memset(&d, 0xA5, sizeof(d));
    const bool glv = host::fold_digits<Fq>(x, nbits, &d);
    printf("fold %s %u %s glv=%d", curve, nbits, xs, glv ? 1 : 0);
    print_digits(d);
  }
  fclose(f);
  return 0;
}
int main(int argc, char** argv) {
  if (argc < 2) return 1;
  int rc = run_curve<PallasFq>("pallas", argv[1]);
  rc |= run_curve<Bls12381Fq>("bls12_381", argv[1]);
  rc |= run_curve<VestaFq>("vesta", argv[1]);
  rc |= run_curve<Bn254Fq>("bn254", argv[1]);
  rc |= run_curve<GrumpkinFq>("grumpkin", argv[1]);
  rc |= run_curve<Bls12377Fq>("bls12_377", argv[1]);
  return rc;
}
#else
int main(int argc, char** argv) {
  if (argc < 2) return 1;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 1;
  char line[256], kind[16], xs[80];
  while (fgets(line, sizeof(line), f)) {
    unsigned c, W, nn, levels, nbits;
    u32 x[8];
    if (sscanf(line, "%15s", kind) != 1) continue;
    if (!strcmp(kind, "plain") && sscanf(line, "%*s %u %79s", &nbits, xs) == 2) {
      parse_hex(xs, x);
      u32 k[9];
      const int top = fold_low_bits(x, nbits, k);
      FoldDigits d;
      memset(&d, 0xA5, sizeof(d));
      fold_digits_plain(k, &d);
      printf("plain %u %s top=%d", nbits, xs, top);
      print_digits(d);
    } else if (!strcmp(kind, "tab") && sscanf(line, "%*s %u %u %u %u %u %79s", &c, &W, &nn, &levels, &nbits, xs) == 6) {
      parse_hex(xs, x);
      FoldTabOps d;
      memset(&d, 0xA5, sizeof(d));
      const bool ok = fold_tab_ops(c, W, nn, levels, x, nbits, &d);
      printf("tab %u %u %u %u %u %s ok=%d", c, W, nn, levels, nbits, xs, ok ? 1 : 0);
      if (!ok) {
        const unsigned char* b = (const unsigned char*)&d;
        for (size_t i = 0; i < sizeof(d); i++)
          if (b[i]) return fprintf(stderr, "refused, but byte %zu of the ops is 0x%02x: %s", i, b[i], line), 2;
        printf("\n");
        continue;
      }
      printf(" e=");
      for (u32 w = 0; w < levels; w++) printf(w ? ",%u" : "%u", window_exponent_of(c, W, nn, 0u, w));
      printf(" nd=%u n_ops=%u ops=", d.nd, d.n_ops);
      for (u32 t = 0; t < d.n_ops && t < 160u; t++) printf("%04x", d.op[t]);
      printf("\n");
    }
  }
  fclose(f);
  return 0;
}
#endif
