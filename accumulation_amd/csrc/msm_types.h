// Plain-data types shared by the host launcher (api.hip) and the kernel translation units.
#pragma once
#include <stdint.h>

#include "blake2s.h"

namespace amsm {

typedef uint32_t u32;
typedef uint64_t u64;

// Arguments of the key sampling kernels (sample_kernels.h), filled by host_sample.h: sample_consts from the modulus.  Field elements
// are C-ABI Montgomery words (12 hold the widest base field), integers little-endian words.
struct SampleConsts {
  b2s::SamplePrefix prefix;  // the part of the hashed message in front of the index
  u32 b[12];                 // the curve's b
  u32 r2[12];                // R^2 mod p: the Montgomery form of R (takes a canonical integer into the field)
  u32 root[12];              // a primitive 2^two_adicity-th root of unity
  u32 half[12];              // the integer (p - 1) / 2: y > p - y  <=>  y > half
  u32 exp[12];               // two_adicity 1: (p + 1) / 4, the square root's exponent; else (t - 1) / 2, p - 1 = 2^two_adicity t
  u32 exp_bits;
  u32 two_adicity;
  u32 cofactor[4];
  u32 cofactor_bits;
};
// counters of one sampling call (device words)
enum { SAMPLE_CNT_PENDING = 0, SAMPLE_CNT_EXHAUSTED = 1, SAMPLE_CNT_IDENTITY = 2, SAMPLE_CNT_WORDS = 3 };

// Arguments of the point validation kernels (points_check_kernels.h), filled by host_points_check.h: points_check_consts.  Field
// elements are C-ABI Montgomery words.
struct PointsCheckConsts {
  u32 b[12];     // the curve's b
  u32 beta[12];  // BLS12-381: the cube root of unity of the endomorphism phi(x, y) = (beta x, y) with phi(P) = -[z^2]P on G1
};
// status byte of one point (include/amsm.h: amsm_points_check) and the device words of one call's report
enum { POINT_VALID = 0, POINT_NON_CANONICAL = 1, POINT_OFF_CURVE = 2, POINT_OFF_SUBGROUP = 3 };
enum { PCHK_FIRST_BAD = 3, PCHK_WORDS = 4 };  // words 0..2: the counts of status 1, 2, 3; word 3: atomicMin of the bad indices

constexpr int VEC_MAX = 8;        // max vectors combined in one launch (reference uses 2..4)
constexpr int HP_MAX_INPUTS = 8;  // max inputs+accumulators of one hp_as t-vector launch (reference tests reach 6)

struct MsmGeom {
  u32 n;             // pairs in this call
  u32 c;             // window bits (2..24)
  u32 W;             // windows (windows_for below)
  u32 S;             // entry slots per scalar (slots_for below)
  u32 nb;            // buckets per set = 2^(c-1)
  u32 n_sets;        // bucket sets = groups * (1 when precomputed, else W)
  u32 groups;        // 1, or 2: scalar i adds into the sum of group (i >> group_shift) & 1 (two MSMs in one pass)
  u32 group_shift;
  u32 B;             // n_sets * nb  (key B = "digit 0", dropped)
  u32 E;             // n * S entries (upper bound; zero digits emit none)
  u32 base_off;      // first generator used
  u32 table_stride;  // generators per table level (key length)
  u32 precomp;       // table has W levels
  u32 idx_rel_bits;  // 0: the prep's interchange word carries the absolute table index base_off + i + w * table_stride.
                     // b > 0 (an MSM over a b-bit window of a longer precomputed key): it carries (w << b) | i -- the bits a
                     // partition pass has for bucket ids do not shrink with the KEY's length -- and k_prep_local /
                     // k_prep_heavy_place expand it to the absolute index when they write the list accumulate L0 reads
  u32 K0;            // entries per accumulate-L0 work item (chunk) of phase A: chunks [0, nA)
  u32 K0b;           // ... of phase B: chunks [nA, n_chunks).  Two sizes (K0 > K0b, both multiples of 4) let the grid be a
                     // WHOLE number of rounds of the resident wave slots: with one size the last round of a 2^20-pair
                     // launch was 56 % full (3.56 rounds of 24 entries: 11 % of the kernel's time on half-empty SIMDs)
  u32 nA;            // chunks of phase A (a multiple of 256: a workgroup never straddles the phases)
  u32 T0;            // entries covered by phase A = nA * K0
  u32 n_chunks;      // work items of accumulate L0 (upper bound: sized for E entries)
  u32 K1;            // max partials folded by one L1 lane
  u32 top_split;     // plain keys on the bucket-per-lane pipeline: the TOP window owns T = top_split + 1 = 2, 4 or 8 bucket sets (a mask:
                     // 1, 3 or 7), picked by log2 T low bits of the scalar's index that leave the group's bit out (window_set); the
                     // host adds the T sums (msm_collect) -- its digits reach only (r - 1) >> lo of their range and carry no sign to
                     // fold, so its partitions run 10 % fuller than the others' on uniform BLS12-381 scalars, 1.3 times on BN254 /
                     // Grumpkin and 1.7 times on BLS12-377, and twice that on scalars a bit short of the field's width (the
                     // synthetic stream of rng.h).  T is the smallest that fits the prep's stage (msm_select.h: plain_top_sets;
                     // 2 wherever 2 fits); sets per group = W + top_split
  u32 part_max;      // host only (bucket-per-lane prep): entries the fullest partition is expected to hold on uniform scalars -- the
                     // top window's digits cover only r / 2^256 of its range (no sign to fold), 10 % denser than the others'
                     // on BLS12-381; a plain key gives that window a bucket set of its own
  u32 top_shift;     // s > 0 (bucket-per-lane keys): the TOP window holds only 255 - c (W - 1) scalar bits, so its digits would all
                     // fall into the lowest 2^(that - 1) buckets -- a sixteenth of the partitions would receive a whole window.
                     // Its table level is 2^(c (W - 1) - s) G instead and its digit is shifted left by s: the same product, spread
                     // over every 2^s-th bucket of the whole range (raw digit <= 2^(c - 1 - s): never negative, no carry out)
  u32 n_narrow;      // round 4: the TOP n_narrow windows are c - 1 bits wide, so that the W widths add up to EXACTLY 256 bits (W c - 256
                     // narrow ones): every window is full -- no short top window -- and the recoding never carries out of the top.
                     // A narrow window's signed digit is DOUBLED (it lands on the even buckets of the full range) and what it
                     // multiplies stands one doubling short: table level w = 2^(e_w) G (precomputed key) / the set's sum counts
                     // 2^(e_w) (plain key), e_w = window_exponent().  0: the legacy walk (equal widths, top_shift)
  u32 bpl;           // 1: bucket-per-lane pipeline (k_prep_local_t + k_accum_bpl; 20-bit windows), 2: bucket-split pipeline
                     // (k_prep_local_s + k_accum_bps; small and medium MSMs), 0: chunked pipeline
  u32 bps_log2_l;    // bucket-split: log2 of the lanes per bucket
  u32 skip_ones;     // round 5: scalars equal to ONE emit no entries (their generators are summed apart, k_tv_sum: ark-ec's
                     // multi_scalar_mul adds the bases of unit scalars directly too) -- a witness with a share of boolean wires
                     // would otherwise put all of them into bucket 1 of the lowest window
  u32 red_s;         // buckets per reduce lane
  u32 red_threads;   // reduce lanes per set
};

// chunk <-> entry position of the two-phase chunking (host and device)
#if defined(__HIPCC__)
#define AMSM_GEOM_FN __host__ __device__ inline
#else
#define AMSM_GEOM_FN inline
#endif
// width of window w, and the power of two its digit multiplies (MsmGeom::n_narrow, MsmGeom::top_shift)
AMSM_GEOM_FN u32 window_bits_of(u32 c, u32 W, u32 n_narrow, u32 w) { return c - ((w + n_narrow >= W) ? 1u : 0u); }
// first bit of window w
AMSM_GEOM_FN u32 window_position_of(u32 c, u32 W, u32 n_narrow, u32 w) {
  const u32 R = W - n_narrow;  // regular windows
  return w < R ? w * c : R * c + (w - R) * (c - 1u);
}
AMSM_GEOM_FN u32 window_exponent_of(u32 c, u32 W, u32 n_narrow, u32 top_shift, u32 w) {
  // the window's position, minus the doubling a narrow window's digit carries, minus the top window's spread
  return window_position_of(c, W, n_narrow, w) - ((w + n_narrow >= W) ? 1u : 0u) - ((w == W - 1u) ? top_shift : 0u);
}
AMSM_GEOM_FN u32 window_exponent(const MsmGeom& g, u32 w) { return window_exponent_of(g.c, g.W, g.n_narrow, g.top_shift, w); }
// the parameters of the signed-digit walk (vec_kernels.h: digit_step), as every kernel that walks scalars receives them
struct DigitWalk {
  u32 c, W, n_narrow, top_shift;
  u32 skip_ones;  // (k_skew_probe: unit scalars are not looked at -- numerous ones are summed apart, few ones skew nothing)
};
AMSM_GEOM_FN DigitWalk digit_walk_of(const MsmGeom& g) {
  DigitWalk d;
  d.c = g.c;
  d.W = g.W;
  d.n_narrow = g.n_narrow;
  d.top_shift = g.top_shift;
  d.skip_ones = g.skip_ones;
  return d;
}
// The skew probe's sampling (host: msm_jobs.h skew_probe_host, device: vec_kernels.h k_skew_probe -- stated here once, for both):
// PROBE_SAMPLES evenly spaced samples, per window a histogram of their non-zero digits hashed into PROBE_BINS bins; the vector is
// skewed when a bin reaches PROBE_LIMIT (uniform digits put at most ~6 samples into a bin)
constexpr u32 PROBE_SAMPLES = 1024, PROBE_BINS = 2048, PROBE_LIMIT = 24;
static_assert(PROBE_BINS == 1u << 11, "probe_bin keeps the top 11 bits of the hash");
AMSM_GEOM_FN u64 probe_sample(u32 t, u64 n) { return ((u64)t * n) / PROBE_SAMPLES; }  // the index of sample t of n scalars
AMSM_GEOM_FN u32 probe_bin(u32 d) { return (d * 2654435761u) >> 21; }
// windows of a width-c walk: W c >= 256 (signed digits need one spare bit); entry slots per scalar
AMSM_GEOM_FN int windows_for(int c) { return 255 / c + 1; }
AMSM_GEOM_FN int slots_for(int c) { return windows_for(c); }
// narrow windows a width-c walk over 256 bits needs (0 when the widths divide evenly; ~0u when c - 1 is not narrow enough)
AMSM_GEOM_FN u32 narrow_windows_for(u32 c) {
  const u32 W = (u32)windows_for((int)c), nn = W * c - 256u;
  return nn < W ? nn : ~0u;
}
// MsmGeom::top_shift for window width c over the scalar field of modulus `mod` (8 little-endian words, odd): the largest s for which
// every CANONICAL scalar's top digit, shifted left by s (on top of the doubling of a narrow window), stays <= 2^(c - 1) (never
// negative, no carry out).  The top window starts at bit lo: its raw value is at most top(r - 1), plus the recoding's carry from the
// window below -- which cannot arrive when the scalars that reach the maximum have nothing in that window (Pallas: r = 2^254 +
// 2^125.1, so the maximal top value forces bits 126..253 to zero).  *raw_max_out: the largest raw top digit.  Host only, no HIP:
// tests/cpp_host/top_sets_check.cpp pins it for every curve.
inline int top_window_shift_of(const u32 mod[8], int c, int W, int n_narrow = 0, unsigned long long* raw_max_out = nullptr) {
  const int lo = (int)window_position_of((u32)c, (u32)W, (u32)n_narrow, (u32)W - 1u);
  const int narrow = n_narrow > 0 ? 1 : 0;  // (the narrow windows are the top ones)
  if (raw_max_out) *raw_max_out = 0;
  if (lo >= 255 || c < 2 || W < 2) return 0;
  u32 r1[8];  // r - 1
  for (int i = 0; i < 8; i++) r1[i] = mod[i];
  r1[0] -= 1u;  // r is odd
  auto bits = [&](int from, int n) -> unsigned long long {  // n <= 32 bits of r - 1 starting at bit `from`
    unsigned long long v = 0;
    for (int k = 0; k < n; k++) {
      int bit = from + k;
      if (bit >= 0 && bit < 256 && ((r1[bit >> 5] >> (bit & 31)) & 1u)) v |= 1ull << k;
    }
    return v;
  };
  const unsigned long long top = bits(lo, 256 - lo < 32 ? 256 - lo : 32);
  // can a scalar with the maximal top value receive a carry?  Only if its window below can exceed half its range (a carry into
  // THAT window included): its raw value there is at most the field of r - 1
  const int cb = (int)window_bits_of((u32)c, (u32)W, (u32)n_narrow, (u32)W - 2u);
  const unsigned long long below = bits(lo - cb, cb);
  const unsigned long long raw_max = top + (below + 1ull > (1ull << (cb - 1)) ? 1ull : 0ull);
  if (raw_max_out) *raw_max_out = raw_max;
  const unsigned long long half = 1ull << (c - 1);
  int s = 0;
  while (s + 1 < c && (raw_max << (narrow + s + 1)) <= half) s++;
  return raw_max == 0 ? 0 : s;
}
// buckets of its set's nb that the top window's digits reach (at least one partition of 1024): what its n entries spread over
inline unsigned long long top_window_reach(u32 nb, unsigned long long raw_max, u32 top_shift, u32 n_narrow) {
  unsigned long long reach = raw_max << (top_shift + (n_narrow ? 1u : 0u));
  if (reach > nb) reach = nb;
  return reach < 1024ull ? 1024ull : reach;
}
// bucket sets per group / the set window w of scalar i feeds, relative to its group's first
AMSM_GEOM_FN u32 sets_per_group(const MsmGeom& g) { return g.precomp ? 1u : g.W + g.top_split; }
AMSM_GEOM_FN u32 window_set(const MsmGeom& g, u32 w, u32 i) {
  // the top window's set: the low bits of i under the mask top_split -- with the bit that picks the group squeezed out first (a
  // group would feed half, a quarter or one of its top sets otherwise); a group bit above the mask changes nothing
  const u32 gs = g.group_shift;
  const u32 j = (g.groups > 1u && gs < 3u) ? ((i & ((1u << gs) - 1u)) | ((i >> (gs + 1u)) << gs)) : i;
  return g.precomp ? 0u : w + ((w == g.W - 1u) ? (j & g.top_split) : 0u);
}
// interchange index -> table index (see idx_rel_bits)
AMSM_GEOM_FN u32 entry_abs_index(const MsmGeom& g, u32 v) {
  return g.idx_rel_bits ? (g.base_off + (v & ((1u << g.idx_rel_bits) - 1u)) + (v >> g.idx_rel_bits) * g.table_stride) : v;
}
AMSM_GEOM_FN u32 chunk_of(const MsmGeom& g, u32 pos) { return pos < g.T0 ? pos / g.K0 : g.nA + (pos - g.T0) / g.K0b; }
AMSM_GEOM_FN u32 chunk_start(const MsmGeom& g, u32 c) { return c < g.nA ? c * g.K0 : g.T0 + (c - g.nA) * g.K0b; }

struct CombineArgs {
  const u32* vec[VEC_MAX];
  u32 len[VEC_MAX];
  u32 coeff[VEC_MAX][8];
  const u32* hiding;
  u32 hiding_len;
  u32 n_vecs;
  u32 n;
};

// Batched polynomial division by (X - z) / evaluation (vec_kernels.h: k_poly_*).  A workgroup owns a tile of POLY_T
// consecutive coefficients, each of its 256 lanes a run of POLY_E; up to POLY_MAX polynomials per launch (blockIdx.y).
constexpr int POLY_MAX = 8;
constexpr u32 POLY_LOG_E = 2, POLY_E = 1u << POLY_LOG_E, POLY_T = 256u * POLY_E;
struct PolyArgs {
  const u32* c[POLY_MAX];  // coefficients, little-endian in the degree
  u32* q[POLY_MAX];        // quotient (len - 1 elements); unused by the evaluation
  u32 len[POLY_MAX];
  u32 off[POLY_MAX];       // first tile of polynomial k in the per-tile workspace
  u32 z[POLY_MAX][8];      // the point (Montgomery)
  u32 pw[POLY_MAX][8][8];  // (z^POLY_E)^(2^k), k < 8: the multipliers of the scan over the lanes' runs
  u32 zt[8];               // evaluation: point^POLY_T
  u32* rem;                // POLY_MAX elements, p_k(z_k) (may be null)
};

struct TVecArgs {
  const u32* a[HP_MAX_INPUTS];
  const u32* b[HP_MAX_INPUTS];
  u32 a_len[HP_MAX_INPUTS];
  u32 b_len[HP_MAX_INPUTS];
  u32 mu[HP_MAX_INPUTS + 1][8];
  const u32* hiding_a;
  const u32* hiding_b;
  u32 hiding_a_len, hiding_b_len;
  u32* t[2 * HP_MAX_INPUTS - 1];
  u32 len;
};

// direct sum over a small key's table of digit multiples (msm_kernels.h k_direct_sum): 64 four-bit windows, multiples 1 .. 8
constexpr u32 DS_W = 64, DS_MULT = 8;
// up to DS_BATCH MSMs over the same key in one launch (blockIdx.y = which): the provers' batched commits
constexpr int DS_BATCH = 16;
struct DsBatch {
  const u32* scalars[DS_BATCH];
  u32 n[DS_BATCH];
  u32 base_off[DS_BATCH];
};

}  // namespace amsm
