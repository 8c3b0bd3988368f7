// The scalar of a key fold out[i] = l[i] + x r[i], recoded once on the host into what the fold kernels take as arguments
// (msm_kernels.h: k_points_fold, k_points_fold_tab): the low bits of x, their non-adjacent form, and the op list of the ladder over a
// key's window multiples with the rules by which it refuses a scalar.  Pure integer arithmetic, no HIP and nothing of a curve: the GLV
// form of a full-size scalar is host_glv.h's fold_digits, which ends in the plain form below.  api_entry_vec.inc recodes where it has
// the scalar and hands the launchers (launch.h) the ready structures; tests/cpp_host/fold_recode_check.cpp prints them without a GPU.
#pragma once
#include <string.h>

#include <algorithm>
#include <cstddef>
#include <vector>

#include "msm_types.h"

namespace amsm {

struct FoldDigits {  // the scalar as kernel-argument digit masks (uniform over the grid)
  // plain form: x in non-adjacent form (digits +1 / -1 / 0, a third non-zero) in pos1 / neg1, up to 256 digits.
  // GLV form (host_glv.h): x = k1 + k2 lambda, |k_i| ~ 2^128: NAF(k1) in pos1 / neg1, NAF(k2) in pos2 / neg2 (signs folded
  // in), and beta (C-ABI Montgomery words) with phi(x, y) = (beta x, y) = [lambda](x, y): half the doublings.
  u32 pos1[8], neg1[8], pos2[5], neg2[5];
  u32 nd;         // digit positions to run
  u32 beta[12];   // W words used
};
// The host flattens the digits of the table ladder into one list of additions, most significant position first; they are uniform
// over the grid, so the next table row is requested while the current addition runs.
struct FoldTabOps {
  uint16_t op[160];  // bits 0..4: digit position, 5..9: level, 15: negate
  u32 n_ops, nd;
};
// kernel arguments: the layout is the kernels'
static_assert(sizeof(FoldDigits) == 156 && sizeof(FoldTabOps) == 328, "kernel-argument layout");
static_assert(offsetof(FoldDigits, neg1) == 32 && offsetof(FoldDigits, pos2) == 64 && offsetof(FoldDigits, neg2) == 84 &&
                  offsetof(FoldDigits, nd) == 104 && offsetof(FoldDigits, beta) == 108,
              "kernel-argument layout");
static_assert(offsetof(FoldTabOps, n_ops) == 320 && offsetof(FoldTabOps, nd) == 324, "kernel-argument layout");

// Non-adjacent form of the little-endian integer k[0 .. nw) (used up; its top bit must be clear: a digit -1 adds one): the digits at
// positions below `limit` into the masks pos / neg, which the caller zeroed.  Returns the top digit's position + 1 (0 for k = 0), or
// NAF_NO_FIT when k has a digit at `limit` or above -- the digits below it stand.
constexpr u32 NAF_NO_FIT = 0xffffffffu;
inline u32 naf_words(u32* k, int nw, u32 limit, u32* pos, u32* neg) {
  u32 nd = 0;
  for (u32 dg = 0;; dg++) {
    bool any = false;
    for (int w = 0; w < nw; w++) any |= k[w] != 0;
    if (!any) return nd;
    if (dg == limit) return NAF_NO_FIT;
    if (k[0] & 1u) {
      if ((k[0] & 3u) == 1u) {  // digit +1: k -= 1
        pos[dg >> 5] |= 1u << (dg & 31);
        k[0] &= ~1u;
      } else {  // digit -1: k += 1
        neg[dg >> 5] |= 1u << (dg & 31);
        for (int w = 0; w < nw; w++)
          if (++k[w] != 0) break;
      }
      nd = dg + 1;
    }
    for (int w = 0; w + 1 < nw; w++) k[w] = (k[w] >> 1) | (k[w + 1] << 31);
    k[nw - 1] >>= 1;
  }
}

// the low `nbits` bits of x (x < 2^255) into k, a ninth word of headroom above them; returns their length
inline int fold_low_bits(const u32 x_canon[8], u32 nbits, u32 k[9]) {
  memset(k, 0, 9 * sizeof(u32));
  int top = 0;
  for (u32 b = 0; b < nbits && b < 256; b++) {
    const u32 bit = (x_canon[b >> 5] >> (b & 31)) & 1u;
    k[b >> 5] |= bit << (b & 31);
    if (bit) top = (int)b + 1;
  }
  return top;
}

// the plain form of k (fold_low_bits' words, used up): pos1 / neg1 and nd, everything else zero
inline void fold_digits_plain(u32 k[9], FoldDigits* d) {
  memset(d, 0, sizeof(*d));
  d->nd = naf_words(k, 9, 256, d->pos1, d->neg1);
  if (d->nd == NAF_NO_FIT) d->nd = 256;  // (k >= 2^255 only: outside the folds' domain; the masks hold the 256 digits they can)
}

// The op list of the fold over a key's window multiples: level w stands for 2^(e_w) (msm_types.h: window_exponent_of; a narrow level
// sits one doubling below its window), levels 0 .. levels - 1 are usable.  x is cut at the e_w, digit w = bits [e_w, e_(w+1)) -- at
// most c of them --, every digit goes into non-adjacent form (up to one position more than its bits) and all additions are ordered
// by position, the levels of one position in ascending order.  False, with *d zeroed, when the geometry is none the ladder takes or
// x does not fit the usable levels: the caller folds by the plain ladder.
inline bool fold_tab_ops(u32 c, u32 W, u32 n_narrow, u32 levels, const u32 x_canon[8], u32 nbits, FoldTabOps* d) {
  memset(d, 0, sizeof(*d));
  if (c < 4 || c > 30 || levels == 0 || levels > 32 || levels > W || n_narrow >= W) return false;
  u32 k[9];
  const u32 top = (u32)fold_low_bits(x_canon, nbits, k);
  auto e_of = [&](u32 w) { return w < W ? window_exponent_of(c, W, n_narrow, 0u, w) : 0xffffu; };
  if (top > (levels < W ? e_of(levels) : 256u)) return false;
  std::vector<uint16_t> ops;
  u32 nd = 0;
  for (u32 w = 0; w < levels && e_of(w) < top; w++) {
    const u32 lo = e_of(w), hi = w + 1u < levels ? e_of(w + 1u) : top;
    // (only the last level of a table that does not span x can be this long, and its top bit is set: its form would not fit either)
    if (hi - lo > 31u) return false;
    u32 v = 0, plus = 0, minus = 0;
    for (u32 pos = lo; pos < hi; pos++) v |= ((k[pos >> 5] >> (pos & 31)) & 1u) << (pos - lo);
    nd = std::max(nd, naf_words(&v, 1, 32, &plus, &minus));
    for (u32 dg = 0; dg < 32; dg++)
      if ((plus | minus) >> dg & 1u) ops.push_back((uint16_t)(dg | (w << 5) | ((minus >> dg & 1u) ? 0x8000u : 0u)));
  }
  // (160 additions are out of reach: a digit of b bits has at most (b + 2) / 2 of them, 32 levels over 255 bits 159)
  if (ops.size() > sizeof(d->op) / sizeof(d->op[0]) || nd > 31) return false;
  std::stable_sort(ops.begin(), ops.end(), [](uint16_t a, uint16_t b) { return (a & 31u) > (b & 31u); });
  d->n_ops = (u32)ops.size();
  d->nd = nd;
  for (size_t t = 0; t < ops.size(); t++) d->op[t] = ops[t];
  return true;
}

}  // namespace amsm
