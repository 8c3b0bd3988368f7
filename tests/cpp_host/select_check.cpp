// Prints what accumulation_amd/csrc/msm_select.h decides at every threshold edge (plain C++: no HIP, no library) --
// tests/test_pipeline_select_cpu.py holds the expected table.  One line per (key, pairs, form):
//   <key> <pairs> <plain|grouped|grouped_irregular|skewed> <pipeline> twin=<0|1> plain_window=<c> range=<pairs>
// and one per case of msel::classify:  classify <case> <verdict of each vector>
// and three (one per Place) per geometry of msel::tail_plan:
//   tail <case> <place> form=.. quad=.. latency=.. red_s=.. red_threads=.. partials=.. rc=.. ticket=.. whole=.. covered=..
// covered: what tail_plan_any_place reserves (msm_plan, before the Place is known) holds everything the launches of this plan write, and
// their grids reach every bucket and sum without reading past the sets; the program fails if any line is not covered
#include <cstdio>
#include <vector>

#include "../../accumulation_amd/csrc/msm_select.h"

using namespace amsm::msel;

int main() {
  struct K {
    const char* name;
    KeyDesc d;
  };
  const std::vector<K> keys = {
      {"direct_2p15", {P2(15), true, false, true, 13}},    // precomputed, carries the direct-sum table
      {"table_2p16", {P2(16), true, false, false, 16}},    // precomputed, 16-bit windows
      {"table_2p19", {P2(19), true, false, false, 16}},
      {"bpl_2p20", {P2(20), true, true, false, 20}},       // the 20-bit table
      {"bpl_2p22", {P2(22), true, true, false, 20}},
      {"plain_2p22", {P2(22), false, false, false, 0}},
  };
  std::vector<size_t> ns;
  for (int lg : {15, 16, 17, 18, 19, 20}) {
    ns.push_back(P2(lg) - 1);
    ns.push_back(P2(lg));
    ns.push_back(P2(lg) + 1);
  }
  ns.push_back(1);
  ns.push_back(P2(21));
  ns.push_back(P2(22) - 1);
  ns.push_back(P2(22));
  Switches sw;
  for (const K& k : keys)
    for (size_t n : ns) {
      if (n > k.d.n) continue;
      struct F {
        const char* name;
        bool grouped, regular, skewed;
      } forms[] = {{"plain", false, false, false}, {"grouped", true, true, false}, {"grouped_irregular", true, false, false},
                   {"skewed", false, false, true}};
      for (const F& f : forms) {
        const Choice c = choose(k.d, n, f.grouped, f.regular, f.skewed, sw);
        printf("%s %zu %s %s twin=%d plain_window=%d range=%zu probe=%d\n", k.name, n, f.name, pipeline_name(c.pipeline), c.over_twin ? 1 : 0,
               c.plain_window, c.range, wants_skew_probe(k.d, n, sw) ? 1 : 0);
      }
    }
  // the switches
  Switches off = sw;
  off.bpl = false;
  printf("switch bpl=0 bpl_2p20 %s\n", pipeline_name(choose(keys[3].d, P2(20), false, false, false, off).pipeline));
  off = sw;
  off.bpl_plain = false;
  printf("switch bpl_plain=0 plain %s range=%zu\n", pipeline_name(choose(keys[5].d, P2(20), false, false, false, off).pipeline), range_of(keys[5].d, P2(22), off));
  off = sw;
  off.bps = 0;
  printf("switch bps=0 table_2p16 %s\n", pipeline_name(choose(keys[1].d, P2(16), false, false, false, off).pipeline));
  off.bps = 1;
  printf("switch bps=1 table_2p16 plain %s grouped %s\n", pipeline_name(choose(keys[1].d, P2(16), false, false, false, off).pipeline),
         pipeline_name(choose(keys[1].d, P2(16), true, true, false, off).pipeline));
  off = sw;
  off.direct = false;
  printf("switch direct=0 direct_2p15 %s\n", pipeline_name(choose(keys[0].d, P2(12), false, false, false, off).pipeline));
  off = sw;
  off.window_override = true;
  printf("switch window_override bpl_2p20 %s twin=%d plain %s\n", pipeline_name(choose(keys[3].d, P2(20), false, false, false, off).pipeline),
         choose(keys[3].d, P2(20), false, false, false, off).over_twin ? 1 : 0, pipeline_name(choose(keys[5].d, P2(20), false, false, false, off).pipeline));
  off = sw;
  off.split_log2 = 0;
  K big{"table_2p23", {P2(23), true, false, false, 17}};
  printf("split table_2p23 default range=%zu off range=%zu below range=%zu\n", range_of(big.d, P2(23), sw), range_of(big.d, P2(23), off),
         range_of(big.d, P2(22) - 1, sw));
  // table 1: the window a key is built for
  for (int lg : {1, 8, 9, 12, 13, 14, 15, 16, 17, 18, 19, 20, 22})
    printf("key_window 2p%d precomputed=%d precomputed_bpl_off=%d plain=%d\n", lg, key_window(P2(lg), true, true), key_window(P2(lg), true, false),
           key_window(P2(lg), false, true));
  // what a call makes of its vectors' two-valued probes (classify): one line per case, one verdict per vector
  {
    static char mem[(size_t)3 << 22];  // the scalars' addresses (never read): three vectors of 2^17 scalars
    struct V {
      unsigned words[32];
      bool probed;
      VecProbe p;
    };
    // mixed / two_valued / all_zero: the probe's flag words; ones: unit scalars among its 1024 samples; top: the value's highest word
    auto vec = [&](bool probed, unsigned mixed, unsigned two_valued, unsigned all_zero, unsigned ones, unsigned top, size_t n, size_t at) {
      V v{};
      v.words[TVW_MIXED] = mixed;
      v.words[TVW_TWO_VALUED] = two_valued;
      v.words[TVW_ALL_ZERO] = all_zero;
      v.words[TVW_ONES] = ones;
      v.words[TVW_VALUE + 7] = top;
      v.probed = probed;
      v.p = VecProbe{nullptr, n, mem + at * 32};
      return v;
    };
    auto run = [&](const char* name, std::vector<V> vs, bool mont, const KeyDesc& key, const Switches& s) {
      std::vector<VecProbe> ps;
      for (V& v : vs) {
        if (v.probed) v.p.words = v.words;
        ps.push_back(v.p);
      }
      std::vector<unsigned char> verdict(ps.size());
      classify(ps.data(), ps.size(), mont, key, s, verdict.data());
      printf("classify %s", name);
      const char* names[] = {"regular", "two_valued", "all_zero", "ones_apart"};
      for (unsigned char x : verdict) printf(" %s", names[x]);
      printf("\n");
    };
    const KeyDesc table17{P2(17), true, false, false, 17};
    const size_t n = P2(17);
    const unsigned heavy = 400, few = 0;  // sampled ones of a 40 % boolean vector / of 40 ones in 2^17
    run("two_valued", {vec(true, 0, 1, 0, 0, 0x3fffffffu, n, 0)}, false, table17, sw);
    run("mixed_flag_wins", {vec(true, 1, 1, 0, 0, 0, n, 0)}, false, table17, sw);
    run("value_2p255_canonical", {vec(true, 0, 1, 0, 0, 0x80000000u, n, 0)}, false, table17, sw);
    run("value_2p255_montgomery", {vec(true, 0, 1, 0, 0, 0x80000000u, n, 0)}, true, table17, sw);
    run("all_zero", {vec(true, 0, 0, 1, 0, 0, n, 0)}, false, table17, sw);
    run("ones_7_samples", {vec(true, 1, 0, 0, TV_ONES_MIN_SAMPLES - 1, 0, n, 0)}, false, table17, sw);
    run("ones_8_samples", {vec(true, 1, 0, 0, TV_ONES_MIN_SAMPLES, 0, n, 0)}, false, table17, sw);
    run("not_probed", {vec(false, 0, 0, 0, heavy, 0, n, 0)}, false, table17, sw);
    run("ones_over_20_bit_table", {vec(true, 1, 0, 0, heavy, 0, P2(20), 0)}, false, keys[3].d, sw);
    run("ones_plain_key", {vec(true, 1, 0, 0, heavy, 0, P2(20), 0)}, false, keys[5].d, sw);
    run("ones_direct_sum", {vec(true, 1, 0, 0, heavy, 0, P2(14), 0)}, false, keys[0].d, sw);
    off = sw;
    off.direct = false;
    run("ones_direct_sum_off", {vec(true, 1, 0, 0, heavy, 0, P2(14), 0)}, false, keys[0].d, off);
    // tests/test_unit_scalars_gpu.py: a boolean-heavy vector, a view that starts 100 scalars before its end and keeps its few ones,
    // an unrelated witness
    run("shared_memory_view", {vec(true, 1, 0, 0, heavy, 0, n, 0), vec(true, 1, 0, 0, few, 0, n, n - 100), vec(true, 1, 0, 0, heavy, 0, n, 2 * n)},
        false, table17, sw);
    run("shared_memory_no_view", {vec(true, 1, 0, 0, heavy, 0, n, 0), vec(true, 1, 0, 0, heavy, 0, n, 2 * n)}, false, table17, sw);
    run("shared_memory_adjacent", {vec(true, 1, 0, 0, heavy, 0, n, 0), vec(true, 1, 0, 0, few, 0, n, n)}, false, table17, sw);
    run("shared_memory_unprobed_view", {vec(true, 1, 0, 0, heavy, 0, n, 0), vec(false, 0, 0, 0, 0, 0, 100, n - 100)}, false, table17, sw);
    run("shared_memory_empty_view", {vec(true, 1, 0, 0, heavy, 0, n, 0), vec(false, 0, 0, 0, 0, 0, 0, n - 100)}, false, table17, sw);
    run("shared_memory_two_valued_view", {vec(true, 1, 0, 0, heavy, 0, n, 0), vec(true, 0, 1, 0, 0, 0, P2(14), 0)}, false, table17, sw);
    run("shared_memory_both_ones", {vec(true, 1, 0, 0, heavy, 0, n, 0), vec(true, 1, 0, 0, heavy, 0, P2(16), 0)}, false, table17, sw);
    // the give-up spreads: the middle vector overlaps one that keeps its ones, the first overlaps the middle one
    run("shared_memory_chain", {vec(true, 1, 0, 0, heavy, 0, n, 0), vec(true, 1, 0, 0, heavy, 0, n, n - 100), vec(true, 1, 0, 0, few, 0, n, 2 * n - 200)},
        false, table17, sw);
  }
  // the tail (table 3): every rule edge, the jump fold's geometry and the shapes of tests/test_tail_forms_gpu.py
  int uncovered = 0;
  {
    struct T {
      const char* name;
      unsigned nb, n_sets, B, E;
      bool bpl;
    };
    const unsigned E0 = 1u << 20;
    const T cases[] = {
        {"B_2p17", 1u << 15, 4, 1u << 17, E0, false},            // TAIL_QUAD_HIDDEN_LOG2: the last table whose hidden tail stays quad
        {"B_2p17_plus_1", 1u << 15, 4, (1u << 17) + 1u, E0, false},
        {"B_5_sets_of_2p15", 1u << 15, 5, 5u << 15, E0, false},
        {"E_5_2p20", 1u << 15, 1, 1u << 15, 5u << 20, false},
        {"E_5_2p20_plus_1", 1u << 15, 1, 1u << 15, (5u << 20) + 1u, false},
        {"nb_2p18_minus_1024", (1u << 18) - 1024u, 1, (1u << 18) - 1024u, E0, false},
        {"nb_2p18", 1u << 18, 1, 1u << 18, E0, false},
        {"nb_2p18_plus_1", (1u << 18) + 1u, 1, (1u << 18) + 1u, E0, false},  // (no real geometry: nb is a power of two; the rule's edge)
        {"nb_256", 256, 8, 2048, E0, false},
        {"nb_257", 257, 8, 2056, E0, false},
        {"nb_65535", 65535, 1, 65535, E0, false},
        {"nb_65536", 65536, 1, 65536, E0, false},
        {"bpl_20_bit_table", 1u << 19, 1, 1u << 19, 13u << 20, true},   // tests/test_bpl_gpu.py: the row / column form, both strip shapes
        {"bpl_off_2p19", 1u << 19, 1, 1u << 19, 13u << 20, false},
        {"bpl_plain_16_bit", 1u << 15, 17, 17u << 15, 16u << 20, true},
        {"bpl_off_plain_16_bit", 1u << 15, 17, 17u << 15, 16u << 20, false},
        {"two_sets_of_2p19", 1u << 19, 2, 1u << 20, 13u << 20, true},    // grouped over the 20-bit table
        {"jump_fold", 256, 2 * 3 * 64, 2 * 3 * 64 * 256, 0, false},     // api_schemes.inc: JUMP_NB buckets, 2 n_rep m0 sets
        {"gpu_a_plain_2p10", 128, 32, 32 * 128, 32u << 10, false},       // 8-bit windows: 32 sets of 128 buckets
        {"gpu_b_table_2p15", 4096, 1, 4096, 20u << 12, false},           // 13-bit windows, 2^12 pairs
        {"gpu_c_plain_2p17_plus_64", 1u << 14, 19, 19u << 14, ((1u << 17) + 64u) * 18u, true},  // 15-bit windows, 18 + 1 sets
    };
    const Place places[] = {Place::LONE, Place::BATCH_LAST, Place::BATCH_INNER};
    const char* place_names[] = {"lone", "batch_last", "batch_inner"};
    for (const T& c : cases) {
      const TailPlan w = tail_plan_any_place(c.nb, c.n_sets, c.B, c.E, c.bpl);  // what msm_plan reserves
      for (int p = 0; p < 3; p++) {
        const TailPlan t = tail_plan(c.nb, c.n_sets, c.B, c.E, c.bpl, places[p]);
        const unsigned shift = t.quad ? 2u : 0u;
        const size_t lanes = ((size_t)t.partials * 256u) >> shift;  // logical lanes of a set's t.partials workgroups
        bool ok = t.partials >= 1 && t.partials <= w.partials && t.rc_records <= w.rc_records && (!t.ticket || w.ticket);
        bool whole = true;
        if (t.form == RED2) {
          const Red2Geom r = red2_geom(c.nb, t.latency);
          const size_t items = (size_t)r.A + RED2_COLS;
          auto pow2_le_64 = [](unsigned x) { return x >= 1 && x <= 64 && (x & (x - 1)) == 0; };
          // k_red2_sums: every row and column has a group, strips tile them exactly, records [0, n_sets * items) are written
          ok = ok && (size_t)r.A * RED2_COLS == c.nb && pow2_le_64(r.gw) && pow2_le_64(r.gc) && RED2_COLS % r.gw == 0 && r.A % r.gc == 0;
          ok = ok && (size_t)r.row_waves * (64u / r.gw) >= r.A && (size_t)r.col_waves * (64u / r.gc) >= RED2_COLS;
          ok = ok && (size_t)c.n_sets * items <= w.rc_records;
          // k_red2_weighted: a logical lane per sum
          ok = ok && lanes >= items && !t.ticket;
        } else {
          // k_bucket_reduce: a logical lane per run of red_s buckets, no bucket read past its set
          ok = ok && t.red_s >= 1 && (size_t)t.red_threads * t.red_s <= c.nb && lanes >= t.red_threads && t.rc_records == 0;
          ok = ok && t.ticket == (t.form == FUSED_QUAD) && t.quad == (t.form == FUSED_QUAD);
          whole = (size_t)t.red_threads * t.red_s == c.nb;
        }
        // the partial records: n_sets * t.partials written (and folded), n_sets * w.partials reserved
        ok = ok && (size_t)c.n_sets * t.partials <= (size_t)c.n_sets * w.partials;
        if (!ok) uncovered++;
        printf("tail %s %s form=%s quad=%d latency=%d red_s=%u red_threads=%u partials=%u rc=%zu ticket=%d whole=%d covered=%d\n", c.name,
               place_names[p], tail_form_name(t.form), t.quad ? 1 : 0, t.latency ? 1 : 0, t.red_s, t.red_threads, t.partials, t.rc_records,
               t.ticket ? 1 : 0, whole ? 1 : 0, ok ? 1 : 0);
      }
    }
  }
  return uncovered ? 1 : 0;
}
