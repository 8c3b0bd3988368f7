// How many bucket sets a plain key's top window owns on the bucket-per-lane pipeline -- msel::plain_top_sets (csrc/msm_select.h), the
// set routing of the prep (csrc/msm_types.h: window_set) and the top window's reach per curve (top_window_shift_of, top_window_reach)
// -- without a GPU: plain C++ over the two headers (tests/test_top_sets_cpu.py builds this with g++, runs it and pins the lines).
//   rule <n> <nb> <reach> <W> <groups> T=<T>          the rule at the rows the test names
//   edge <nb> <reach> last_T2=<n> first_T4=<n> last_T4=<n>   where the rule changes its mind over n in (2^17, 2^20]
//   parent_equiv cases=<k> mismatches=<m> over_two=<m2>      T == 2 <=> the geometry with two top sets fits, restated below
//   group_bit T=<T> groups=<g> shift=<s> min=<a> max=<b> parent=<0|1|-> other_windows=<0|1>
//   reach <curve> c=<c> W=<W> narrow=<nn> lo=<bit> shift=<s> raw_max=<d> reach=<buckets>
//   tail <case> <place> partials=<p> covered=<0|1>    what msm_plan reserves covers the tail over W + 8 sets, 2 (W + 8) when grouped
// Exit status 1 when a parent_equiv, group_bit or tail line is not as it must be.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "../../accumulation_amd/csrc/msm_select.h"
#include "../../accumulation_amd/csrc/msm_types.h"

using namespace amsm;
using namespace amsm::msel;

// The inequality before the rule, restated from the geometry of two top sets (api_pipeline.inc: bpl_geom, kern_fr.hip:
// prep_bpl_supported as they stood): part_max = max(per_win, per_top), halved for two groups; P = groups (W + 2) nb / 1024
static bool parent_accepts(unsigned long long n, unsigned nb, unsigned long long reach, unsigned W, unsigned groups) {
  const unsigned long long cap = 40960ull - 3620ull;
  const unsigned long long per_win = (n * 1024ull + nb - 1) / nb, per_top = (n * 1024ull + reach - 1) / reach;
  unsigned long long part_max = per_win > per_top ? per_win : per_top;
  if (groups > 1u) part_max = (part_max + 1ull) / 2ull;
  const unsigned long long E = n * W, P = ((unsigned long long)groups * (W + 2u) * nb) >> 10;
  if (E / P + 1024ull > cap) return false;
  return part_max + 5ull * (unsigned long long)std::sqrt((double)part_max) <= cap;
}

int main() {
  int bad = 0;
  static_assert(BPL_STAGE_CAP == 40960u - 3620u, "the stage of k_prep_local_t");
  // ---- the rule at the rows of the test ----
  {
    struct R {
      unsigned long long n;
      unsigned nb;
      unsigned long long reach;
      unsigned groups;
    };
    const R rows[] = {
        {786432, 32768, 24776, 1}, {917504, 32768, 24776, 1}, {1u << 20, 32768, 24776, 1},  // BN254 / Grumpkin, 16-bit windows
        {1u << 19, 32768, 19116, 1}, {786432, 32768, 19116, 1}, {1u << 20, 32768, 19116, 1},  // BLS12-377 as the issue reads it
        {1u << 19, 32768, 19120, 1}, {786432, 32768, 19120, 1}, {1u << 20, 32768, 19120, 1},  // ... with the carry into the top digit
        {1u << 20, 32768, 29678, 1}, {1u << 20, 32768, 32768, 1}, {(1u << 18) + 1, 32768, 32768, 1},  // BLS12-381, Pallas / Vesta
        {1u << 20, 32768, 9560, 1}, {1u << 20, 32768, 4000, 1}, {1u << 18, 16384, 9560, 1}, {1u << 18, 16384, 4780, 1},
        {(1u << 18) + 2, 32768, 19120, 2}, {1u << 20, 32768, 19120, 2}, {1u << 20, 32768, 9560, 2}, {1u << 20, 32768, 4000, 2}};
    for (const R& r : rows) {
      const unsigned W = r.nb == 32768u ? 16u : 18u;
      printf("rule %llu %u %llu %u %u T=%u\n", r.n, r.nb, r.reach, W, r.groups, plain_top_sets((size_t)r.n, r.nb, r.reach, W, r.groups));
    }
    for (unsigned long long reach : {24776ull, 19116ull, 19120ull, 9560ull}) {
      unsigned long long last2 = 0, first4 = 0, last4 = 0;
      for (unsigned long long n = (1ull << 17) + 1; n <= (1ull << 20); n++) {
        const unsigned T = plain_top_sets((size_t)n, 32768, reach, 16, 1);
        if (T == 2u) last2 = n;
        if (T == 4u && !first4) first4 = n;
        if (T == 4u) last4 = n;
      }
      printf("edge 32768 %llu last_T2=%llu first_T4=%llu last_T4=%llu\n", reach, last2, first4, last4);
    }
  }
  // ---- T == 2 exactly where two sets fitted before; the cap of AMSM_TOP_SETS=2 ----
  {
    unsigned long long cases = 0, mismatches = 0, over_two = 0, bad_t = 0;
    for (unsigned nb : {32768u, 16384u}) {
      const unsigned W = nb == 32768u ? 16u : 18u;
      for (unsigned groups = 1; groups <= 2; groups++)
        for (unsigned long long n = (1ull << 17) + 1;; n = n + 4099 < (1ull << 20) ? n + 4099 : (1ull << 20)) {  // ... and 2^20 itself
          for (unsigned long long reach = 1024;; reach = reach + 97 < nb ? reach + 97 : nb) {                      // ... and nb itself
            const unsigned T = plain_top_sets((size_t)n, nb, reach, W, groups);
            const unsigned T2 = plain_top_sets((size_t)n, nb, reach, W, groups, BPL_STAGE_CAP, plain_top_sets_cap(2));
            cases++;
            if ((T == 2u) != parent_accepts(n, nb, reach, W, groups)) mismatches++;
            if (T2 > 2u || (T2 == 2u) != (T == 2u)) over_two++;
            if (T != 0u && T != 2u && T != 4u && T != 8u) bad_t++;
            if (reach == nb) break;
          }
          if (n == (1ull << 20)) break;
        }
    }
    printf("parent_equiv cases=%llu mismatches=%llu over_two=%llu bad_T=%llu\n", cases, mismatches, over_two, bad_t);
    if (mismatches || over_two || bad_t || plain_top_sets_cap(0) != 8u || plain_top_sets_cap(4) != 8u || plain_top_sets_cap(8) != 8u) bad = 1;
  }
  // ---- the group bit never picks the top set ----
  for (unsigned T : {2u, 4u, 8u})
    for (unsigned groups = 1; groups <= 2; groups++)
      for (unsigned gs : {0u, 1u, 2u, 3u, 17u}) {
        MsmGeom g;
        memset(&g, 0, sizeof(g));
        g.W = 16;
        g.c = 16;
        g.groups = groups;
        g.group_shift = groups > 1u ? gs : 0u;
        g.top_split = T - 1u;
        unsigned cnt[2][8] = {};
        bool parent = true, other = true, in_range = true;
        // i < 2^12, and the same indices with the group's bit set where it lies above them (shift 17: both groups are visited)
        const u32 high = (groups > 1u && gs >= 12u) ? (1u << gs) : 0u;
        for (u32 k = 0; k < (high ? 8192u : 4096u); k++) {
          const u32 i = (k & 4095u) | (k >= 4096u ? high : 0u);
          const u32 grp = groups > 1u ? (i >> g.group_shift) & 1u : 0u;
          const u32 s = window_set(g, g.W - 1u, i);
          if (s < g.W - 1u || s >= g.W - 1u + T || s >= sets_per_group(g)) {
            in_range = false;
            continue;
          }
          cnt[grp][s - (g.W - 1u)]++;
          const u32 sb = (g.groups > 1u && g.group_shift == 0u) ? 1u : 0u;  // the expression before the rule
          if (T == 2u && s != g.W - 1u + ((i >> sb) & 1u)) parent = false;
          for (u32 w = 0; w + 1u < g.W; w++) other = other && window_set(g, w, i) == w;
          MsmGeom p = g;  // a precomputed key has one set
          p.precomp = 1;
          p.top_split = 0;
          other = other && window_set(p, g.W - 1u, i) == 0u && sets_per_group(p) == 1u;
        }
        unsigned lo = ~0u, hi = 0;
        for (unsigned grp = 0; grp < groups; grp++)
          for (unsigned k = 0; k < T; k++) {
            lo = cnt[grp][k] < lo ? cnt[grp][k] : lo;
            hi = cnt[grp][k] > hi ? cnt[grp][k] : hi;
          }
        printf("group_bit T=%u groups=%u shift=%u min=%u max=%u parent=%s other_windows=%d\n", T, groups, gs, lo, hi,
               T == 2u ? (parent ? "1" : "0") : "-", other ? 1 : 0);
        if (!in_range || hi - lo > 1u || lo == 0u || !parent || !other) bad = 1;
      }
  // ---- the top window per curve ----
  {
    struct F {
      const char* name;
      u32 mod[8];
    };
    const F fields[] = {
        {"pallas", {0x00000001u, 0x8c46eb21u, 0x0994a8ddu, 0x224698fcu, 0x00000000u, 0x00000000u, 0x00000000u, 0x40000000u}},
        {"vesta", {0x00000001u, 0x992d30edu, 0x094cf91bu, 0x224698fcu, 0x00000000u, 0x00000000u, 0x00000000u, 0x40000000u}},
        {"bls12_381_g1", {0x00000001u, 0xffffffffu, 0xfffe5bfeu, 0x53bda402u, 0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u}},
        {"bn254_g1", {0xf0000001u, 0x43e1f593u, 0x79b97091u, 0x2833e848u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u}},
        {"grumpkin", {0xd87cfd47u, 0x3c208c16u, 0x6871ca8du, 0x97816a91u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u}},
        {"bls12_377_g1", {0x00000001u, 0x0a118000u, 0xd0000001u, 0x59aa76feu, 0x5c37b001u, 0x60b44d1eu, 0x9a2ca556u, 0x12ab655eu}},
    };
    for (const F& f : fields) {
      printf("modulus %s ", f.name);
      for (int i = 7; i >= 0; i--) printf("%08x", f.mod[i]);
      printf("\n");
      for (int c : {15, 16, 20}) {
        const int W = 255 / c + 1;
        const u32 nn = narrow_windows_for((u32)c);
        unsigned long long raw_max = 0;
        const int s = top_window_shift_of(f.mod, c, W, (int)nn, &raw_max);
        const u32 nb = 1u << (c - 1);
        printf("reach %s c=%d W=%d narrow=%u lo=%u shift=%d raw_max=%llu reach=%llu\n", f.name, c, W, nn,
               window_position_of((u32)c, (u32)W, nn, (u32)W - 1u), s, raw_max, top_window_reach(nb, raw_max, (u32)s, nn));
      }
    }
  }
  // ---- the tail over the widest set counts: what is reserved before the Place is known covers every launch ----
  {
    struct T {
      const char* name;
      unsigned nb, W, top, groups;
      unsigned long long n;
    };
    const T cases[] = {{"16_bit_8_sets", 1u << 15, 16, 8, 1, 1u << 20},
                       {"16_bit_8_sets_grouped", 1u << 15, 16, 8, 2, 1u << 20},
                       {"16_bit_4_sets", 1u << 15, 16, 4, 1, 1u << 20},
                       {"15_bit_8_sets", 1u << 14, 18, 8, 1, (1u << 17) + 1},
                       {"15_bit_8_sets_grouped", 1u << 14, 18, 8, 2, (1u << 18) + 2}};
    const Place places[] = {Place::LONE, Place::BATCH_LAST, Place::BATCH_INNER};
    const char* place_names[] = {"lone", "batch_last", "batch_inner"};
    for (const T& c : cases) {
      const unsigned n_sets = c.groups * (c.W + c.top), B = n_sets * c.nb, E = (unsigned)(c.n * c.W);
      const TailPlan w = tail_plan_any_place(c.nb, n_sets, B, E, true);
      for (int p = 0; p < 3; p++) {
        const TailPlan t = tail_plan(c.nb, n_sets, B, E, true, places[p]);
        const size_t lanes = ((size_t)t.partials * 256u) >> (t.quad ? 2u : 0u);
        bool ok = t.partials >= 1 && t.partials <= w.partials && t.rc_records <= w.rc_records && (!t.ticket || w.ticket);
        ok = ok && t.form != RED2 && t.red_s >= 1 && (size_t)t.red_threads * t.red_s == c.nb && lanes >= t.red_threads;
        printf("tail %s %s partials=%u covered=%d\n", c.name, place_names[p], t.partials, ok ? 1 : 0);
        if (!ok) bad = 1;
      }
    }
  }
  return bad;
}
