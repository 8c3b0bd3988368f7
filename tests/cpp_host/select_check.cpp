// Prints what accumulation_amd/csrc/msm_select.h decides at every threshold edge (plain C++: no HIP, no library) --
// tests/test_pipeline_select_cpu.py holds the expected table.  One line per (key, pairs, form):
//   <key> <pairs> <plain|grouped|grouped_irregular|skewed> <pipeline> twin=<0|1> plain_window=<c> range=<pairs>
// and one per case of msel::classify:  classify <case> <verdict of each vector>
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
  return 0;
}
