// Prints what accumulation_amd/csrc/msm_geom.h makes of a key, a range and a context at every rule edge of the MSM geometry (plain
// C++: no HIP, no library) -- tests/test_msm_geom_cpu.py compares the output with tests/golden/msm_geom.txt.  One line per case:
//   modulus <curve> <hex>
//   <fn> <case> st=<ok|false|invalid_arg|unsupported> [short=<0|1>] <every field of MsmGeom> [l1=<hidden>,<exposed>] [tail=<lone>,<batch_last>,<batch_inner>]
//   unit <case> nv=<nv> <every field of MsmGeom> tail=...
//   l1 <case> B= n_chunks= l1=<hidden>,<exposed>
// <fn> is make (make_geom), chunked (chunked_geom), bpl (bpl_geom), bps (bps_geom) or unit_ok (bps_unit_geom_ok).  The properties of
// the chunk split that accumulate L0 relies on are asserted here on every accepted case: exit status 1 and a line on stderr.
// Built from this one source twice: by plain g++ over the header alone, with the scalar fields' moduli written out below, and (with
// -DMSM_GEOM_MODULI_FROM_CURVES_H, the host side of a hipcc build) with the moduli taken from csrc/curves.h -- the same output.
#include <cstdio>
#include <string>
#include <vector>

#include "../../accumulation_amd/csrc/msm_geom.h"
#ifdef MSM_GEOM_MODULI_FROM_CURVES_H
#include "../../accumulation_amd/csrc/curves.h"
#endif

using namespace amsm;
using msel::Place;

struct Field {
  const char* name;
  u32 mod[8];
};
#ifdef MSM_GEOM_MODULI_FROM_CURVES_H
template <class Curve>
static Field field_of(const char* name) {
  Field f;
  f.name = name;
  for (int i = 0; i < 8; i++) f.mod[i] = Curve::Fr::mod(i);
  return f;
}
static const Field FIELDS[] = {field_of<PallasCurve>("pallas"),     field_of<VestaCurve>("vesta"),       field_of<Bls12381Curve>("bls12_381_g1"),
                               field_of<Bn254Curve>("bn254_g1"), field_of<GrumpkinCurve>("grumpkin"), field_of<Bls12377Curve>("bls12_377_g1")};
#else
static const Field FIELDS[] = {
    {"pallas", {0x00000001u, 0x8c46eb21u, 0x0994a8ddu, 0x224698fcu, 0x00000000u, 0x00000000u, 0x00000000u, 0x40000000u}},
    {"vesta", {0x00000001u, 0x992d30edu, 0x094cf91bu, 0x224698fcu, 0x00000000u, 0x00000000u, 0x00000000u, 0x40000000u}},
    {"bls12_381_g1", {0x00000001u, 0xffffffffu, 0xfffe5bfeu, 0x53bda402u, 0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u}},
    {"bn254_g1", {0xf0000001u, 0x43e1f593u, 0x79b97091u, 0x2833e848u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u}},
    {"grumpkin", {0xd87cfd47u, 0x3c208c16u, 0x6871ca8du, 0x97816a91u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u}},
    {"bls12_377_g1", {0x00000001u, 0x0a118000u, 0xd0000001u, 0x59aa76feu, 0x5c37b001u, 0x60b44d1eu, 0x9a2ca556u, 0x12ab655eu}},
};
#endif

static int bad = 0;
#define EXPECT(cond, name)                                             \
  do {                                                                 \
    if (!(cond)) {                                                     \
      fprintf(stderr, "%s: %s does not hold\n", name.c_str(), #cond); \
      bad = 1;                                                         \
    }                                                                  \
  } while (0)

static GeomCtx ctx_of(const Field& f, int wave_slots = 4096, int window_override = 0, int top_sets = 0) {
  GeomCtx c;
  c.window_override = window_override;
  c.wave_slots = wave_slots;
  c.top_sets = top_sets;
  for (int i = 0; i < 8; i++) c.r_mod[i] = f.mod[i];
  return c;
}
static GeomKey plain_key(size_t n) {
  GeomKey k;
  k.n = n;
  return k;
}
// a key with a table of c-bit windows, as bases_finish builds it; bpl: the bucket-per-lane table (widths adding up to 256 bits, the top
// window spread by top_shift)
static GeomKey table_key(const Field& f, size_t n, int c, bool bpl = false) {
  GeomKey k;
  k.n = n;
  k.precomp = true;
  k.c = c;
  k.W = windows_for(c);
  if (bpl) {
    k.n_narrow = (int)narrow_windows_for((u32)c);
    k.top_shift = top_window_shift_of(f.mod, c, k.W, k.n_narrow);
  }
  return k;
}

static const char* status_name(int s) {
  return s == AMSM_OK ? "ok" : s == AMSM_E_INVALID_ARG ? "invalid_arg" : s == AMSM_E_UNSUPPORTED ? "unsupported" : "other";
}
static void print_fields(const MsmGeom& g) {
  printf(" n=%u c=%u W=%u S=%u nb=%u n_sets=%u groups=%u group_shift=%u B=%u E=%u base_off=%u table_stride=%u precomp=%u idx_rel_bits=%u K0=%u K0b=%u nA=%u "
         "T0=%u n_chunks=%u K1=%u top_split=%u part_max=%u top_shift=%u n_narrow=%u bpl=%u bps_log2_l=%u skip_ones=%u red_s=%u red_threads=%u",
         g.n, g.c, g.W, g.S, g.nb, g.n_sets, g.groups, g.group_shift, g.B, g.E, g.base_off, g.table_stride, g.precomp, g.idx_rel_bits, g.K0, g.K0b,
         g.nA, g.T0, g.n_chunks, g.K1, g.top_split, g.part_max, g.top_shift, g.n_narrow, g.bpl, g.bps_log2_l, g.skip_ones, g.red_s, g.red_threads);
}
static void print_tail(const msel::TailPlan& lone, const msel::TailPlan& last, const msel::TailPlan& inner) {
  printf(" tail=%s,%s,%s", msel::tail_form_name(lone.form), msel::tail_form_name(last.form), msel::tail_form_name(inner.form));
}
static void print_tails(const MsmGeom& g) {
  print_tail(tail_plan_of(g, Place::LONE), tail_plan_of(g, Place::BATCH_LAST), tail_plan_of(g, Place::BATCH_INNER));
}
// what accumulate L0 and the kernels that walk its chunks rely on (msm_types.h: chunk_of, chunk_start)
static void expect_chunks(const std::string& name, const MsmGeom& g) {
  EXPECT(g.nA % 256u == 0u, name);
  EXPECT(g.K0 % 4u == 0u && g.K0b % 4u == 0u, name);
  EXPECT(g.K0b <= g.K0 && g.K0 <= (u32)tune::K0_MAX + 4u, name);
  EXPECT(g.K0b >= 12u, name);
  EXPECT((unsigned long long)g.nA * g.K0 == g.T0, name);
  if (g.E == 0u) return;
  EXPECT(chunk_start(g, g.n_chunks) >= g.E, name);
  EXPECT(chunk_of(g, g.E - 1u) < g.n_chunks, name);
  for (u32 pos : {g.T0 - 1u, g.T0, g.T0 + 1u}) {
    if (g.T0 == 0u && pos == g.T0 - 1u) continue;
    const u32 c = chunk_of(g, pos);
    EXPECT(chunk_start(g, c) <= pos && pos < chunk_start(g, c + 1u), name);
  }
}

static void make_case(const std::string& name, const GeomCtx& ctx, const GeomKey& key, size_t off, size_t n, int group_shift = -1, int c_plain = 0,
                      u32 top_sets = 2) {
  MsmGeom g;
  Walk w;  // (the top digit of the walk, where there is one: bpl_geom hands it down)
  const u32 top_shift = walk_of(ctx, key, n, c_plain, &w) == AMSM_OK ? top_digit_of(ctx, key, w).shift : 0u;
  const int st = make_geom(ctx, key, off, n, &g, group_shift, c_plain, top_sets, top_shift);
  printf("make %s st=%s", name.c_str(), status_name(st));
  if (st == AMSM_OK) {
    print_fields(g);
    expect_chunks(name, g);
    MsmGeom s = {};  // the split is a function of E and the wave slots alone
    s.E = g.E;
    chunk_split(s, ctx.wave_slots);
    EXPECT(s.K0 == g.K0 && s.K0b == g.K0b && s.nA == g.nA && s.T0 == g.T0 && s.n_chunks == g.n_chunks, name);
  }
  printf("\n");
}
static MsmGeom chunked_case(const std::string& name, const GeomCtx& ctx, const GeomKey& key, size_t off, size_t n, int group_shift = -1) {
  MsmGeom g = {};
  bool short_prep = false;
  const int st = chunked_geom(ctx, key, off, n, group_shift, &g, &short_prep);
  printf("chunked %s st=%s", name.c_str(), status_name(st));
  if (st == AMSM_OK) {
    printf(" short=%d", short_prep ? 1 : 0);
    print_fields(g);
    printf(" l1=%u,%u", l1_lanes(g, true), l1_lanes(g, false));
    print_tails(g);
    expect_chunks(name, g);
    EXPECT(g.bpl == 0u, name);
  }
  printf("\n");
  return g;
}
static bool bpl_case(const std::string& name, const GeomCtx& ctx, const GeomKey& key, size_t off, size_t n, int group_shift, int c_plain) {
  MsmGeom g;
  const bool ok = bpl_geom(ctx, key, off, n, group_shift, c_plain, &g);
  printf("bpl %s st=%s", name.c_str(), ok ? "ok" : "false");
  if (ok) {
    print_fields(g);
    print_tails(g);
    expect_chunks(name, g);
    EXPECT(g.bpl == 1u && prep_bpl_supported(g), name);
  }
  printf("\n");
  return ok;
}
static MsmGeom bps_case(const std::string& name, const GeomCtx& ctx, const GeomKey& key, size_t off, size_t n, int group_shift = -1) {
  MsmGeom g = {};
  const bool ok = bps_geom(ctx, key, off, n, group_shift, &g);
  printf("bps %s st=%s", name.c_str(), ok ? "ok" : "false");
  if (ok) {
    print_fields(g);
    print_tails(g);
    expect_chunks(name, g);
    EXPECT(g.bpl == 2u && prep_bps_choose(g) == (int)g.bps_log2_l, name);
  }
  printf("\n");
  return g;
}
static std::string p2(size_t n) {  // 2p16, 2p16_plus_1, else the number
  for (int k = 1; k < 40; k++) {
    if (n == ((size_t)1 << k)) return "2p" + std::to_string(k);
    if (n == ((size_t)1 << k) + 1) return "2p" + std::to_string(k) + "_plus_1";
  }
  return std::to_string(n);
}

int main() {
  for (const Field& f : FIELDS) {
    printf("modulus %s ", f.name);
    for (int i = 7; i >= 0; i--) printf("%08x", f.mod[i]);
    printf("\n");
  }
  const Field& pallas = FIELDS[0];
  const GeomCtx ctx = ctx_of(pallas);

  // ---- window and limits ----
  for (size_t n : {(size_t)1, (size_t)255, (size_t)256, (size_t)1 << 10, (size_t)1 << 16, (size_t)1 << 18, (size_t)1 << 20})
    chunked_case("plain_n_" + p2(n), ctx, plain_key(n), 0, n);
  for (int c : {1, 2, 7, 8, 12, 24, 25})  // (1 and 25 are refused)
    chunked_case("override_" + std::to_string(c), ctx_of(pallas, 4096, c), plain_key(1u << 10), 0, 1u << 10);
  // entry words carry a 30-bit index: n * S (16-bit windows: 16 slots) ...
  make_case("nS_2p30_minus_16", ctx_of(pallas, 4096, 16), plain_key(1u << 26), 0, (1u << 26) - 1u);
  make_case("nS_2p30", ctx_of(pallas, 4096, 16), plain_key(1u << 26), 0, 1u << 26);
  // ... and the table's last level: 16 levels of 2^26 generators, against the same key without a table
  make_case("table_nW_2p30", ctx, table_key(pallas, 1u << 26, 16), 0, 1u << 16);
  make_case("table_nW_2p30_minus_16", ctx, table_key(pallas, (1u << 26) - 1u, 16), 0, 1u << 16);
  make_case("plain_key_2p26", ctx, plain_key(1u << 26), 0, 1u << 16);
  // a plain key's bucket-per-lane walk: 23-bit windows would need 20 narrow ones of 12; the top window owns 2, 4 or 8 sets
  make_case("plain_c23_no_walk", ctx, plain_key(1u << 20), 0, 1u << 20, -1, 23, 2);
  make_case("plain_c17_no_walk", ctx, plain_key(1u << 20), 0, 1u << 20, -1, 17, 2);
  for (u32 t : {1u, 2u, 3u, 4u, 8u, 16u}) make_case("plain_c16_top_sets_" + std::to_string(t), ctx, plain_key(1u << 20), 0, 1u << 20, -1, 16, t);

  // ---- the chunk split: E = 16 n entries (16-bit windows) at `share` entries per resident lane ----
  for (int ws : {4, 2048, 3072, 4096}) {
    const std::string tag = "ws" + std::to_string(ws);
    const GeomCtx c16 = ctx_of(pallas, ws, 16), c20 = ctx_of(pallas, ws, 20);
    // share < 12: one size | 12: two sizes, no long round | 13: one round, it is long | 40, 42: two rounds, none / one long | 47: both
    // long | 100: four rounds, one long | 33: two rounds of 16 and 20
    for (unsigned share : {1u, 5u, 11u, 12u, 13u, 33u, 40u, 42u, 47u, 100u}) {
      const size_t n = (size_t)share * 4u * (size_t)ws;  // E = share * 64 * ws
      make_case("chunks_" + tag + "_share_" + std::to_string(share), c16, plain_key(n), 0, n);
      if (share == 42u) make_case("chunks_" + tag + "_share_42_plus_1", c16, plain_key(n + 1), 0, n + 1);
    }
    // phase A covers everything: E = 13 n (20-bit windows) an exact multiple of K0 = 12, and one scalar (13 entries) more
    const size_t n12 = (size_t)10 * 64u * (size_t)ws / 13u / 12u * 12u;
    for (size_t n : {n12, n12 + 1}) {
      MsmGeom g;
      const std::string name = "chunks_" + tag + (n == n12 ? "_whole_chunks" : "_whole_chunks_plus_1");
      make_case(name, c20, plain_key(n), 0, n);
      if (make_geom(c20, plain_key(n), 0, n, &g) == AMSM_OK) EXPECT(g.K0 == 12u && g.E % g.K0 == (n == n12 ? 0u : 1u) && g.T0 >= g.E, name);
    }
  }

  // ---- groups ----
  for (int gs : {-1, 0, 1, 2, 3, 17}) {
    const std::string tag = "group_shift_" + (gs < 0 ? std::string("none") : std::to_string(gs));
    chunked_case(tag + "_table17", ctx, table_key(pallas, 1u << 17, 17), 0, 1u << 17, gs);
    chunked_case(tag + "_plain", ctx, plain_key(1u << 18), 0, 1u << 18, gs);
    bps_case(tag + "_table17", ctx, table_key(pallas, 1u << 17, 17), 0, 1u << 17, gs);
  }

  // ---- window-relative indices: ranges of 17-bit and 20-bit keys of 2^20 and 2^22 generators ----
  for (size_t kn : {(size_t)1 << 20, (size_t)1 << 22}) {
    const GeomKey k17 = table_key(pallas, kn, 17), k20 = table_key(pallas, kn, 20, true);
    for (size_t off : {(size_t)0, (size_t)3 << 18})
      for (int gs : {-1, 0}) {
        const std::string tail = "_of_" + p2(kn) + (off ? "_off" : "") + (gs >= 0 ? "_groups2" : "");
        for (size_t n : {(size_t)1, (size_t)1 << 16, ((size_t)1 << 16) + 1, (size_t)1 << 17, ((size_t)1 << 17) + 1, (size_t)1 << 20}) {
          if (off + n > kn) continue;
          chunked_case("rel17_n_" + p2(n) + tail, ctx, k17, off, n, gs);
          if (n >= ((size_t)1 << 16) && n <= ((size_t)1 << 17) + 1) bps_case("rel17_n_" + p2(n) + tail, ctx, k17, off, n, gs);
        }
        for (size_t n : {((size_t)1 << 18) + 1, (size_t)1 << 19, ((size_t)1 << 19) + 1, (size_t)1 << 20}) {
          if (off + n > kn) continue;
          bpl_case("rel20_n_" + p2(n) + tail, ctx, k20, off, n, gs, 0);
        }
      }
  }
  // the chunked plan keeps the bits only where the short prep chain takes the geometry: a table of 7-bit windows (37 slots) has none
  chunked_case("rel_refused_c7_S37", ctx, table_key(pallas, 1u << 12, 7), 0, 1u << 10);
  chunked_case("rel_kept_c8_S32", ctx, table_key(pallas, 1u << 12, 8), 0, 1u << 10);
  // the bucket-split pipeline over a key without a table: no lane count, with or without the bits
  bps_case("plain_key", ctx, plain_key(1u << 17), 0, 1u << 16);

  // ---- bucket-per-lane ----
  for (const Field& f : FIELDS) {
    const std::string cv = f.name;
    const GeomCtx fc = ctx_of(f);
    const GeomKey k20 = table_key(f, 1u << 20, 20, true), k22 = table_key(f, 1u << 22, 20, true);
    bpl_case(cv + "_table20_n_2p18_plus_1", fc, k20, 0, (1u << 18) + 1u, -1, 0);
    bpl_case(cv + "_table20_n_2p20", fc, k20, 0, 1u << 20, -1, 0);
    bpl_case(cv + "_table20_n_2p20_groups2", fc, k20, 0, 1u << 20, 0, 0);
    bpl_case(cv + "_table20_n_2p20_of_2p22", fc, k22, 1u << 20, 1u << 20, -1, 0);
    // a plain key with 16-bit windows: the rule's T (AMSM_TOP_SETS unset, or 2: two or none) and the forced 4 and 8
    for (int top_sets : {0, 2, 4, 8}) {
      const GeomCtx tc = ctx_of(f, 4096, 0, top_sets);
      const std::string ts = "_top_sets_" + std::to_string(top_sets);
      bpl_case(cv + "_plain_c16_n_2p18_plus_1" + ts, tc, plain_key(1u << 20), 0, (1u << 18) + 1u, -1, 16);
      bpl_case(cv + "_plain_c16_n_2p20" + ts, tc, plain_key(1u << 20), 0, 1u << 20, -1, 16);
      bpl_case(cv + "_plain_c16_n_2p20_groups2" + ts, tc, plain_key(1u << 20), 0, 1u << 20, 0, 16);
    }
    bpl_case(cv + "_plain_c16_n_2p21_too_long", fc, plain_key(1u << 21), 0, 1u << 21, -1, 16);
    bpl_case(cv + "_plain_c15_n_2p18", fc, plain_key(1u << 18), 0, 1u << 18, -1, 15);
  }
  // the forced 8 sets do not fit (two groups of 15 + 7 sets of 2^17 buckets: 5632 partitions), the rule's two do (4096)
  bpl_case("pallas_plain_c18_groups2_top_sets_8", ctx_of(pallas, 4096, 0, 8), plain_key(1u << 20), 0, 1u << 20, 0, 18);
  bpl_case("pallas_plain_c18_groups2_top_sets_0", ctx, plain_key(1u << 20), 0, 1u << 20, 0, 18);
  bpl_case("pallas_plain_c23_no_walk", ctx, plain_key(1u << 20), 0, 1u << 20, -1, 23);
  bpl_case("pallas_plain_c23_no_walk_top_sets_8", ctx_of(pallas, 4096, 0, 8), plain_key(1u << 20), 0, 1u << 20, -1, 23);
  bpl_case("pallas_plain_no_window", ctx, plain_key(1u << 20), 0, 1u << 20, -1, 0);

  // ---- bucket-split, and the units of its MSMs ----
  for (int c : {15, 16, 17})
    for (size_t n : {(size_t)1 << 16, (size_t)1 << 17}) {
      const std::string name = "table" + std::to_string(c) + "_n_" + p2(n);
      const GeomKey key = table_key(pallas, 1u << 17, c);
      const MsmGeom g = bps_case(name, ctx, key, 0, n);
      MsmGeom u = {};
      const bool unit_ok = bps_unit_geom_ok(ctx, key, 0, n, &u);  // (16 slots at most: 16- and 17-bit windows)
      printf("unit_ok %s st=%s\n", name.c_str(), unit_ok ? "ok" : "false");
      if (!unit_ok || n != ((size_t)1 << 16)) continue;
      for (u32 nv : {2u, 8u}) {
        const MsmGeom ug = bps_unit_geom(g, nv);
        printf("unit %s nv=%u", name.c_str(), nv);
        print_fields(ug);
        print_tail(bps_unit_tail(g, nv, Place::LONE), bps_unit_tail(g, nv, Place::BATCH_LAST), bps_unit_tail(g, nv, Place::BATCH_INNER));
        printf("\n");
      }
    }
  bps_case("table17_n_2p17_groups2", ctx, table_key(pallas, 1u << 17, 17), 0, 1u << 17, 0);  // (two sets: msm_plan's, never a unit's)
  bps_case("table12_n_2p19_no_lane_count", ctx, table_key(pallas, 1u << 19, 12), 0, 1u << 19);

  // ---- lanes per bucket of accumulate L1: both sides of its five thresholds ----
  {
    struct L {
      const char* name;
      u32 B, n_chunks;
    };
    const L rows[] = {{"hidden_B_16383_avg_48", 16383, 48 * 16383},  {"hidden_B_16384_avg_48", 16384, 48 * 16384},
                      {"hidden_B_16384_below_48", 16384, 48 * 16384 - 1}, {"B_4096_avg_24", 4096, 24 * 4096},
                      {"B_4096_below_24", 4096, 24 * 4096 - 1},      {"B_4097_avg_24", 4097, 24 * 4097},
                      {"B_4096_avg_3", 4096, 3 * 4096},              {"B_4096_below_3", 4096, 3 * 4096 - 1},
                      {"B_2p20_avg_3", 1u << 20, 3u << 20},          {"B_2p20_below_3", 1u << 20, (3u << 20) - 1u}};
    for (const L& r : rows) {
      MsmGeom g = {};
      g.B = r.B;
      g.n_chunks = r.n_chunks;
      printf("l1 %s B=%u n_chunks=%u l1=%u,%u\n", r.name, g.B, g.n_chunks, l1_lanes(g, true), l1_lanes(g, false));
    }
  }
  return bad;
}
