// Prints what accumulation_amd/csrc/prep_geom.h makes of hand-filled MsmGeom records at every rule edge of the three prep chains
// (plain C++: no HIP, no library) -- tests/test_prep_geom_cpu.py compares the output with tests/golden/prep_geom.txt.  Per record:
//   geom  <case> n= c= W= S= nb= n_sets= groups= B= E= base_off= stride= precomp= rel= top_split= part_max=
//   short <case> <PrepGeom> scatter_lds= local_lds= supported= small_words= fill= fill_heavy=
//   bpl   <case> <PrepGeom> scatter_lds= local_lds= supported= stride= partitions= groups_per_part= part_entries= needs=a,b,grp,order,small
//   bps   <case> choose=                                     (precomputed keys only)
//   bps_l <case> l= <PrepGeom> scatter_lds= local_lds= stride= partitions= part_entries= [needs=...]   (needs: at the chosen l)
// and one `small` line with the layout of the small arrays (offsets in words from d_small) for both fills.
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "../../accumulation_amd/csrc/prep_geom.h"

using namespace amsm;

// a key of `stride` generators with c-bit windows (precomputed: one bucket set per group; plain: W + top_split), n pairs from 0
static MsmGeom geom(u32 n, u32 c, bool precomp, u32 groups, u32 stride, u32 top_split = 0) {
  MsmGeom g = {};
  g.n = n;
  g.c = c;
  g.W = 255u / c + 1u;
  g.S = g.W;
  g.nb = 1u << (c - 1u);
  g.groups = groups;
  g.top_split = top_split;
  g.precomp = precomp ? 1u : 0u;
  g.n_sets = groups * (precomp ? 1u : g.W + top_split);
  g.B = g.n_sets * g.nb;
  g.E = n * g.S;
  g.table_stride = stride;
  return g;
}
static MsmGeom with_B(MsmGeom g, u32 B) {
  g.B = B;
  return g;
}
static MsmGeom with_S(MsmGeom g, u32 S) {
  g.S = S;
  g.E = g.n * S;
  return g;
}
static MsmGeom with_rel(MsmGeom g, u32 bits) {
  g.idx_rel_bits = bits;
  return g;
}
static MsmGeom with_part_max(MsmGeom g, u32 part_max) {
  g.part_max = part_max;
  return g;
}
static MsmGeom with_off(MsmGeom g, u32 off) {
  g.base_off = off;
  return g;
}

static void print_pg(const PrepGeom& pg) {
  printf(" SH=%u P=%u SPB=%u IB=%u CAP=%u HEAVY=%u FIX=%u", pg.SH, pg.P, pg.SPB, pg.IB, pg.CAP, pg.HEAVY, pg.FIX);
}
static void print_needs(const PrepNeeds& nd) {
  printf(" needs=%zu,%zu,%zu,%zu,%zu", nd.vals_a, nd.vals_b, nd.bpl_grp, nd.bpl_order, nd.prep_small);
}

int main() {
  struct Case {
    const char* name;
    MsmGeom g;
  };
  const u32 K = 1024u;
  const std::vector<Case> cases = {
      // the short chain takes S <= 32: a plain key at c = 8 (32 windows), not at c = 7 (37), nor one slot over
      {"plain_c8_S32", geom(1u << 10, 8, false, 1, 1u << 10)},
      {"plain_c8_S33", with_S(geom(1u << 10, 8, false, 1, 1u << 10), 33)},
      {"plain_c7_S37", geom(1u << 10, 7, false, 1, 1u << 10)},
      {"empty", geom(0, 16, true, 1, 1u << 16)},
      // IB + SH <= 31: 16 levels of a 2^24 / 2^25 / 2^26-generator table leave 3 / 2 / 1 bits for the bucket id; window-relative
      // indices (idx_rel_bits) give them back
      {"table_2p24_W16", geom(1u << 16, 16, true, 1, 1u << 24)},
      {"table_2p25_W16", geom(1u << 16, 16, true, 1, 1u << 25)},
      {"table_2p26_W16", geom(1u << 16, 16, true, 1, 1u << 26)},
      {"table_2p26_W16_rel16", with_rel(geom(1u << 16, 16, true, 1, 1u << 26), 16)},
      {"table_2p26_W16_rel16_off", with_off(with_rel(geom(1u << 16, 16, true, 1, 1u << 26), 16), 3u << 16)},
      // partitions: 512 of 2^SH buckets while SH < 10, then up to PREP_MAX_P of 1024, then larger ones
      {"B_512x16", with_B(geom(1u << 12, 14, true, 1, 1u << 12), 512u * 16u)},
      {"B_512x16_plus_1", with_B(geom(1u << 12, 14, true, 1, 1u << 12), 512u * 16u + 1u)},
      {"B_512x1024", with_B(geom(1u << 18, 20, true, 1, 1u << 18), 512u * K)},
      {"B_512x1024_plus_1", with_B(geom(1u << 18, 20, true, 1, 1u << 18), 512u * K + 1u)},
      {"B_4096x1024", with_B(geom(1u << 18, 23, true, 1, 1u << 18), 4096u * K)},
      {"B_4096x1024_plus_1", with_B(geom(1u << 18, 23, true, 1, 1u << 18), 4096u * K + 1u)},
      // the scatter's LDS crosses 64 KiB between 1365 and 1366 partitions (8192 staged entries)
      {"scatter_lds_P1365", with_B(geom(1u << 18, 16, false, 1, 1u << 18), 1365u * K)},
      {"scatter_lds_P1366", with_B(geom(1u << 18, 16, false, 1, 1u << 18), 1366u * K)},
      {"scatter_lds_S32_P1366", with_B(geom(1u << 18, 8, false, 1, 1u << 18), 1366u * K)},
      // bucket-per-lane, the 20-bit table: 2^19 buckets, the shortest and the longest range, window-relative and absolute
      {"bpl_2p20_n_2p18_plus_1", with_part_max(with_rel(geom((1u << 18) + 1u, 20, true, 1, 1u << 20), 19), 6800)},
      {"bpl_2p20_n_2p20", with_part_max(geom(1u << 20, 20, true, 1, 1u << 20), 26700)},
      {"bpl_2p20_n_2p20_no_part_max", geom(1u << 20, 20, true, 1, 1u << 20)},
      {"bpl_2p22_n_2p20_off", with_off(with_part_max(with_rel(geom(1u << 20, 20, true, 1, 1u << 22), 20), 26700), 3u << 20)},
      {"bpl_2p20_n_2p20_groups2", with_part_max(geom(1u << 20, 20, true, 2, 1u << 20), 13350)},
      {"bpl_2p20_stage_full", with_part_max(geom(1u << 20, 20, true, 1, 1u << 20), 36400)},   // 36400 + 5 sqrt: over the stage
      {"bpl_2p20_stage_fits", with_part_max(geom(1u << 20, 20, true, 1, 1u << 20), 36300)},
      // ... a plain key with 16-bit windows: the top window on 2, 4 or 8 sets; one and two groups
      {"bpl_plain_c16_top2", with_part_max(geom(1u << 20, 16, false, 1, 1u << 20, 1), 36200)},
      {"bpl_plain_c16_top4", with_part_max(geom(1u << 20, 16, false, 1, 1u << 20, 3), 32768)},
      {"bpl_plain_c16_top8", with_part_max(geom(1u << 20, 16, false, 1, 1u << 20, 7), 32768)},
      {"bpl_plain_c16_top2_groups2", with_part_max(geom(1u << 20, 16, false, 2, 1u << 20, 1), 18100)},
      {"bpl_plain_c15_n_2p18", with_part_max(geom(1u << 18, 15, false, 1, 1u << 22, 1), 16384)},
      {"bpl_plain_c8_S32", with_part_max(with_B(geom(1u << 16, 8, false, 1, 1u << 16, 1), 64u * K), 2048)},
      // ... buckets that are no whole number of 4 partitions (4096 buckets) are refused, as are too few and too many
      {"bpl_B_512x1024_plus_512", with_B(geom(1u << 20, 20, true, 1, 1u << 20), 512u * K + 512u)},
      {"bpl_B_513x1024", with_B(geom(1u << 20, 20, true, 1, 1u << 20), 513u * K)},
      {"bpl_B_516x1024", with_B(geom(1u << 20, 20, true, 1, 1u << 20), 516u * K)},
      {"bpl_B_2p15", with_B(geom(1u << 20, 16, true, 1, 1u << 20), 32u * K)},
      {"bpl_B_4100x1024", with_B(geom(1u << 20, 20, true, 1, 1u << 20), 4100u * K)},
      // bucket-split: 2^16 and 2^17 pairs at c = 16 and 17, every lane count prep_bps_choose returns (c = 18 .. 11), refusals
      {"bps_c16_n_2p16", with_rel(geom(1u << 16, 16, true, 1, 1u << 19), 16)},
      {"bps_c16_n_2p17", with_rel(geom(1u << 17, 16, true, 1, 1u << 19), 17)},
      {"bps_c17_n_2p16", geom(1u << 16, 17, true, 1, 1u << 17)},
      {"bps_c17_n_2p17", geom(1u << 17, 17, true, 1, 1u << 17)},
      {"bps_c16_n_2p17_groups2", geom(1u << 17, 16, true, 2, 1u << 17)},
      {"bps_c18_l0", geom(1u << 16, 18, true, 1, 1u << 16)},
      {"bps_c15_l3", geom(1u << 16, 15, true, 1, 1u << 16)},
      {"bps_c14_l4", geom(1u << 16, 14, true, 1, 1u << 16)},
      {"bps_c13_l5", geom(1u << 16, 13, true, 1, 1u << 16)},
      {"bps_c12_l6", geom(1u << 16, 12, true, 1, 1u << 16)},
      {"bps_c11_l6_P64", geom(1u << 16, 11, true, 1, 1u << 16)},
      {"bps_c17_n_2p19_wants_256", geom(1u << 19, 17, true, 1, 1u << 19)},
      {"bps_c12_n_2p19_over_cap", geom(1u << 19, 12, true, 1, 1u << 19)},   // E / P + 1024 > CAP at the last lane count
      {"bps_c6_B_32", geom(1u << 10, 6, true, 1, 1u << 10)},
      {"bps_B_not_pow2", with_B(geom(1u << 16, 16, true, 1, 1u << 16), 3u << 14)},
      {"bps_table_2p26_W16", geom(1u << 16, 16, true, 1, 1u << 26)},        // IB + SH > 31
  };
  u32* const d_small = reinterpret_cast<u32*>(static_cast<uintptr_t>(1) << 32);  // (only offsets from it are printed)
  for (const Case& cs : cases) {
    MsmGeom g = cs.g;
    printf("geom %s n=%u c=%u W=%u S=%u nb=%u n_sets=%u groups=%u B=%u E=%u base_off=%u stride=%u precomp=%u rel=%u top_split=%u part_max=%u\n",
           cs.name, g.n, g.c, g.W, g.S, g.nb, g.n_sets, g.groups, g.B, g.E, g.base_off, g.table_stride, g.precomp, g.idx_rel_bits,
           g.top_split, g.part_max);
    {
      const PrepGeom pg = prep_geom(g);
      printf("short %s", cs.name);
      print_pg(pg);
      printf(" scatter_lds=%zu local_lds=%zu supported=%d small_words=%zu fill=%zu fill_heavy=%zu\n", prep_scatter_lds(g, pg),
             prep_local_lds(pg), prep_supported(g) ? 1 : 0, prep_small_words(g), PrepSmall::of(d_small, 0).fill_bytes,
             PrepSmall::of(d_small, prep_heavy_words(g)).fill_bytes);
    }
    {
      const PrepGeom pg = prep_bpl_geom(g);
      printf("bpl %s", cs.name);
      print_pg(pg);
      printf(" scatter_lds=%zu local_lds=%zu supported=%d stride=%u partitions=%u groups_per_part=%u part_entries=%zu", prep_bpl_scatter_lds(g, pg),
             prep_bpl_local_lds(pg), prep_bpl_supported(g) ? 1 : 0, prep_bpl_stride(g), prep_bpl_partitions(g), prep_bpl_groups_per_partition(),
             prep_bpl_part_entries(g));
      print_needs(prep_bpl_needs(g));
      printf("\n");
    }
    if (g.precomp) {
      const int l = prep_bps_choose(g);
      printf("bps %s choose=%d\n", cs.name, l);
      for (u32 k = 0; k <= 6u; k++) {
        const PrepGeom pg = prep_bps_geom(g, k);
        printf("bps_l %s l=%u", cs.name, k);
        print_pg(pg);
        printf(" scatter_lds=%zu local_lds=%zu stride=%u partitions=%u part_entries=%zu", prep_scatter_lds(g, pg), prep_bps_local_lds(pg),
               prep_bps_stride(g, k), prep_bps_partitions(g, k), prep_bps_part_entries(g, k));
        if ((int)k == l) {
          g.bps_log2_l = k;
          print_needs(prep_bps_needs(g));
        }
        printf("\n");
      }
    }
  }
  // the small arrays behind the 16 flag words, for a chain without and with the heavy-partition tables (B = 2^15)
  const size_t hw = prep_heavy_words(geom(1u << 16, 16, true, 1, 1u << 16));
  for (size_t heavy_words : {(size_t)0, hw}) {
    const PrepSmall s = PrepSmall::of(d_small, heavy_words);
    printf("small heavy_words=%zu part_total=%td part_start=%td part_cursor=%td part_items=%td hv_n=%td hv_cnt=%td hv_ids=%td hv_cur=%td hv_end=%td "
           "fill=%zu block_words=%u\n",
           heavy_words, s.part_total - d_small, s.part_start - d_small, s.part_cursor - d_small, s.part_items - d_small, s.hv.n - d_small,
           s.hv.cnt - d_small, s.hv.ids - d_small, s.hv.cur - d_small, s.hv.end - d_small, s.fill_bytes, prep_bps_small_block_words());
  }
  return 0;
}
