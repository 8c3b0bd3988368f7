// The geometry of the prep chains (prep_kernels.h): partitions, index bits, LDS sizes, strides and buffer needs of an MSM, as pure
// host arithmetic on MsmGeom.  No HIP: kern_fr.hip launches by these numbers, api_pipeline.inc allocates by them, the kernels carve
// their LDS by the same constants, and tests/cpp_host/prep_geom_check.cpp prints them at every rule edge without a GPU.
#pragma once
#include <algorithm>
#include <cstddef>

#include "msm_select.h"
#include "msm_types.h"

namespace amsm {

struct PrepGeom {
  u32 SH;   // log2(buckets per partition)
  u32 P;    // partitions = ceil(B / 2^SH)
  u32 SPB;  // scalars per workgroup of k_prep_hist / k_prep_scatter (256 lanes x 2)
  u32 IB;   // bits of a table index (entry word: negate | bucket id low bits << IB | index)
  u32 CAP;  // entries k_prep_local can assemble in LDS (larger partitions scatter straight to memory)
  u32 HEAVY;  // partitions with more entries than this are split over PREP_HEAVY_SLICES workgroups (k_prep_heavy_*)
  // FIX != 0 (bucket-per-lane prep, round 3): partition p owns entries [p * FIX, (p + 1) * FIX) of the interchange buffer --
  // no histogram, no scan: uniform digits fill a partition to E / P +- a few hundred entries, and FIX = CAP, what
  // k_prep_local_t can stage anyway; a partition that would overflow drops the excess and its count (the cursor) trips the
  // overflow flag there, i.e. the skew fallback that a partition above CAP takes in any case
  u32 FIX;
};

constexpr u32 PREP_MAX_HEAVY = 4096;  // heavy partitions k_prep_scan can list (prep_kernels.h: PrepHeavy)

constexpr u32 BPL_GROUP = 64;            // lanes per accumulate wave
constexpr u32 BPL_BINS = 256;            // size classes of the bucket ordering (sizes >= 255 share the last one)
// The 64 LARGEST buckets of a partition are split in two halves, one lane each, whose sums the accumulate kernel adds with one
// lane exchange.  On uniform scalars the largest are the buckets the spread top window feeds (MsmGeom::top_shift: every 32nd
// bucket holds ~88 entries against ~24; Pallas has 32 of them per partition, BLS12-381 64): unsplit, the group holding them
// ran 108 rows with half its lanes idle after 35 (rows per MSM 242 k -> 225 k, 88 % -> 94 % of the lane-iterations useful).
// Lane slots of a partition: [0, 64) halves of the buckets at positions 0..31 of the size order | [64, 1024) the buckets at
// positions 64..1023, one lane each | [1024, 1088) halves of positions 32..63 -- 17 groups of 64 lanes, rows nearly descending.
constexpr u32 BPL_SPLIT = 64;
constexpr u32 BPL_NB = 1024;                                   // buckets per partition
constexpr u32 BPL_LANES = BPL_NB + BPL_SPLIT;                  // 1088 lane slots per partition
constexpr u32 BPL_GROUPS = BPL_LANES / BPL_GROUP;              // 17
constexpr u32 BPS_LANES = 1024, BPS_GROUPS = BPS_LANES / BPL_GROUP;  // lane slots / 64-lane groups per partition

// bits of the largest table index an entry of this MSM carries (PrepGeom::IB): absolute, or relative to the MSM's window of a longer
// precomputed key (MsmGeom::idx_rel_bits)
inline u32 prep_index_bits(const MsmGeom& g) {
  unsigned long long max_idx = (unsigned long long)g.base_off + g.n - 1ull +
                               (g.precomp ? (unsigned long long)(g.W - 1u) * g.table_stride : 0ull);
  if (g.idx_rel_bits) max_idx = ((unsigned long long)(g.W - 1u) << g.idx_rel_bits) | ((1ull << g.idx_rel_bits) - 1ull);
  u32 ib = 1;
  while ((max_idx >> ib) != 0ull) ib++;
  return ib;
}
// partitions of 2^SH consecutive buckets, at most PREP_MAX_P of them (about 512 when the bucket count allows)
constexpr u32 PREP_MAX_P = 4096;
inline PrepGeom prep_geom(const MsmGeom& g) {
  PrepGeom pg;
  pg.SH = 4;
  while (((g.B + (1u << pg.SH) - 1u) >> pg.SH) > 512u && pg.SH < 10u) pg.SH++;
  while (((g.B + (1u << pg.SH) - 1u) >> pg.SH) > PREP_MAX_P) pg.SH++;
  pg.P = (g.B + (1u << pg.SH) - 1u) >> pg.SH;
  pg.SPB = g.S <= 16u ? 512u : 256u;  // SPB * S <= 8192 staged entries
  pg.IB = prep_index_bits(g);
  // the entry word has 31 bits for index + bucket-id low bits: trade partition size for partitions when it is tight
  while (pg.IB + pg.SH > 31u && pg.SH > 0u && ((g.B + (1u << (pg.SH - 1)) - 1u) >> (pg.SH - 1)) <= PREP_MAX_P) pg.SH--;
  pg.P = (g.B + (1u << pg.SH) - 1u) >> pg.SH;
  // k_prep_local stages a partition in LDS when it fits: a 148 KiB budget (counters + scan words + entries; one
  // 1024-lane workgroup per CU) holds the ~32 k entries of one of 512 partitions at 2^20 pairs with 4 k to spare
  const u32 budget_words = 37888u, fixed_words = 2u * (1u << pg.SH) + 1024u;
  pg.CAP = budget_words > fixed_words + 4096u ? budget_words - fixed_words : 0u;
  // heavy: several times the expected size AND big enough for 64 workgroups to beat one (below, one workgroup is fine)
  pg.HEAVY = std::max<u32>(4u * (g.E / pg.P + 1u), 1u << 17);
  pg.FIX = 0;
  return pg;
}
// words per per-bucket array of the heavy-partition path (every partition's 2^SH buckets, padded)
inline size_t prep_heavy_words(const MsmGeom& g) { return (size_t)g.B + 4096 + 64; }
inline size_t prep_small_words(const MsmGeom& g) { return 4 * (PREP_MAX_P + 1) + 1 + 3 * prep_heavy_words(g) + PREP_MAX_HEAVY; }
// The small arrays of one MSM, carved from the prep_small_words(g) words at d_small.  The PREP_FLAG_WORDS flag words of the MSM stand
// directly in front of d_small, so that ONE fill clears them with the arrays that must start at zero: fill_bytes from d_small -
// PREP_FLAG_WORDS, a whole number of 256-byte lines (an odd size made the runtime split the fill into two dispatches); the words
// the rounding spills into (hv.ids) are written before they are read.
// heavy_words: prep_heavy_words(g) for the chain that splits heavy partitions (launch_prep: hv.cnt is zeroed too); 0 for the chains
// whose HEAVY is 2^32 - 1 -- no partition is listed, hv.ids / cur / end are never touched and the fill ends behind the heavy count.
struct PrepHeavy {
  u32* n;      // number of heavy partitions (k_prep_scan)
  u32* ids;    // their ids
  u32* cnt;    // B words, zeroed by the launcher: entries per bucket (heavy partitions only)
  u32* cur;    // B words: running cursor of every bucket of a heavy partition (offset inside the partition)
  u32* end;    // B words: end offset of the bucket inside the partition
};
constexpr u32 PREP_FLAG_WORDS = 16;
constexpr size_t prep_small_fill_bytes(size_t heavy_words) {
  return ((PREP_FLAG_WORDS + 4 * (PREP_MAX_P + 1) + 1 + heavy_words) * sizeof(u32) + 255) & ~(size_t)255;
}
struct PrepSmall {
  u32 *part_total, *part_start, *part_cursor, *part_items;  // PREP_MAX_P + 1 words each
  PrepHeavy hv;
  size_t fill_bytes;
  static PrepSmall of(u32* d_small, size_t heavy_words) {
    PrepSmall s;
    s.part_total = d_small;
    s.part_start = d_small + (PREP_MAX_P + 1);
    s.part_cursor = d_small + 2 * (PREP_MAX_P + 1);
    s.part_items = d_small + 3 * (PREP_MAX_P + 1);
    s.hv.n = d_small + 4 * (PREP_MAX_P + 1);
    s.hv.cnt = s.hv.n + 1;
    s.hv.ids = s.hv.cnt + (heavy_words ? heavy_words : 64);
    s.hv.cur = heavy_words ? s.hv.ids + PREP_MAX_HEAVY : s.hv.ids;
    s.hv.end = s.hv.cur + heavy_words;
    s.fill_bytes = prep_small_fill_bytes(heavy_words);
    return s;
  }
};
inline size_t prep_local_lds(const PrepGeom& pg) { return (2 * (size_t)(1u << pg.SH) + 1024 + pg.CAP) * sizeof(u32); }
constexpr size_t PREP_LDS_LIMIT = 160 * 1024;  // gfx950: 160 KiB per workgroup
inline size_t prep_scatter_lds(const MsmGeom& g, const PrepGeom& pg) {
  const size_t cap = (size_t)pg.SPB * g.S;
  return (3 * (size_t)pg.P + cap) * sizeof(u32) + cap * sizeof(uint16_t);
}
inline bool prep_supported(const MsmGeom& g) {
  if (g.n == 0 || g.S > 32u) return false;  // S > 32 <=> c < 8: tiny problems, the rocPRIM chain is fine there
  PrepGeom pg = prep_geom(g);
  // entry word = negate | bucket-id low bits << IB | index; k_prep_local keeps 2 * 2^SH + 256 words in LDS; the dynamic
  // LDS of every kernel of the chain must fit a workgroup (wide windows / many bucket sets: fall back to rocPRIM)
  return pg.SH <= 12u && pg.IB + pg.SH <= 31u && prep_scatter_lds(g, pg) <= PREP_LDS_LIMIT &&
         prep_local_lds(pg) <= PREP_LDS_LIMIT && (pg.P + 256) * sizeof(u32) <= 64 * 1024;
}

// ---- bucket-per-lane prep (k_prep_local_t): partitions of exactly 1024 buckets, one 1024-lane workgroup each ----
// words of LDS k_prep_local_t keeps beside its CAP staged entries (the kernel carves the same layout)
constexpr u32 BPL_LOCAL_FIXED_WORDS = 3u * BPL_NB + 2u * BPL_BINS + 2u * BPL_GROUPS + 2u;
// round 4: the whole 160 KiB a workgroup may declare (round 3: 148 KiB, and 1792 more fixed words) -- a plain-key MSM of 2^20
// pairs over 16 bucket sets of 2^15 puts 32 768 entries into a partition, 36 200 into those of the top window on BLS12-381
constexpr u32 BPL_LOCAL_BUDGET_WORDS = 40960u;
static_assert(BPL_LOCAL_BUDGET_WORDS - BPL_LOCAL_FIXED_WORDS == msel::BPL_STAGE_CAP, "msm_select.h plans for k_prep_local_t's stage");
inline PrepGeom prep_bpl_geom(const MsmGeom& g) {
  PrepGeom pg;
  pg.SH = 10;
  pg.P = g.B >> pg.SH;
  pg.SPB = g.S <= 16u ? 512u : 256u;  // SPB * S <= 8192 staged entries
  pg.IB = prep_index_bits(g);
  pg.CAP = BPL_LOCAL_BUDGET_WORDS - BPL_LOCAL_FIXED_WORDS;  // ~35.3 k entries: a partition of a 2^20-pair MSM holds ~26.6 k
  pg.HEAVY = 0xffffffffu;
  // fixed partitions: what uniform digits bring plus a quarter and a constant, at most what the LDS stage takes (a partition
  // beyond it takes the skew fallback either way)
  const unsigned long long per = std::max<unsigned long long>(((unsigned long long)g.E + pg.P - 1) / std::max(1u, pg.P), g.part_max);
  pg.FIX = (u32)std::min<unsigned long long>(pg.CAP, (per + per / 4ull + 2048ull + 15ull) & ~15ull);
  return pg;
}
// 8-byte interchange entries the partition pass may write (fixed partitions reserve FIX each)
inline size_t prep_bpl_part_entries(const MsmGeom& g) {
  PrepGeom pg = prep_bpl_geom(g);
  return std::max<size_t>(g.E, pg.FIX ? (size_t)pg.P * pg.FIX : 0);
}
inline size_t prep_bpl_local_lds(const PrepGeom& pg) { return (size_t)(BPL_LOCAL_FIXED_WORDS + pg.CAP) * sizeof(u32); }
inline size_t prep_bpl_scatter_lds(const MsmGeom& g, const PrepGeom& pg) {
  const size_t cap = (size_t)pg.SPB * g.S;
  return (3 * (size_t)pg.P + 2 * cap) * sizeof(u32) + cap * sizeof(uint16_t);
}
inline u32 prep_bpl_partitions(const MsmGeom& g) { return g.B >> 10; }
inline u32 prep_bpl_groups_per_partition() { return BPL_GROUPS; }  // 17 groups of 64 lane slots (BPL_SPLIT)
// transposed entries per partition: the expected partition size + 25 % (the padding to each group's largest bucket is ~6 %
// on uniform digits) + a constant; anything that does not fit is a skewed input and takes the fallback
inline u32 prep_bpl_stride(const MsmGeom& g) {
  const u32 P = std::max(1u, prep_bpl_partitions(g));
  const unsigned long long per = std::max<unsigned long long>(((unsigned long long)g.E + P - 1) / P, g.part_max);
  return (u32)((per + per / 4ull + 4096ull + 1023ull) & ~1023ull);
}
inline bool prep_bpl_supported(const MsmGeom& g) {
  // one bucket set per group over a precomputed key, W per group over a plain one (round 4); <= 16 entry slots per scalar
  if (g.S > 32u || g.n == 0 || g.n_sets != g.groups * sets_per_group(g)) return false;
  if (g.B < (1u << 16) || (g.B & 1023u) || (g.B >> 10) > PREP_MAX_P || ((g.B >> 10) & 3u)) return false;
  PrepGeom pg = prep_bpl_geom(g);
  if (pg.IB > 30u) return false;
  // the expected partition -- the fullest one -- must fit the LDS stage with room for the digits' spread (sigma ~ 180 entries at
  // 30 k: 1024 on the average partition, 5 sigma on the fullest)
  // (msm_select.h: bpl_stage_fits states the two inequalities -- the rule that picks a plain key's top sets asks the same question)
  if (!msel::bpl_stage_fits(g.E, pg.P, g.part_max, pg.CAP)) return false;
  return prep_bpl_scatter_lds(g, pg) <= PREP_LDS_LIMIT && prep_bpl_local_lds(pg) <= PREP_LDS_LIMIT &&
         (unsigned long long)pg.P * prep_bpl_stride(g) < (1ull << 31);
}

// ---- bucket-split prep (k_prep_local_s): partitions of 1024 / L buckets = 1024 lanes, 32-bit interchange entries ----
// words of LDS k_prep_local_s keeps beside its CAP staged entries: cnt / cur / beg / ord (4 NBP), 1024 scan words, the size
// classes, rows and bases of the 16 groups -- ONE expression for the geometry, the launch size and the kernel's carving
// (round 3 budgeted 3 NBP + 1024 + 34 after the size ordering had added NBP + BPL_BINS: the top of stage[] lay past the
// allocation, reachable once a partition held more than CAP - NBP - 256 entries)
constexpr u32 bps_local_fixed_words(u32 nbp) { return 4u * nbp + 1024u + BPL_BINS + 2u * BPS_GROUPS + 2u; }
constexpr u32 BPS_LOCAL_BUDGET_WORDS = 37888u;  // 148 KiB
inline PrepGeom prep_bps_geom(const MsmGeom& g, u32 log2_l) {
  PrepGeom pg;
  pg.SH = 10u - log2_l;
  pg.P = g.B >> pg.SH;
  pg.SPB = g.S <= 16u ? 512u : 256u;
  pg.IB = prep_index_bits(g);
  pg.CAP = BPS_LOCAL_BUDGET_WORDS - bps_local_fixed_words(1u << pg.SH);
  pg.HEAVY = 0xffffffffu;
  // fixed partitions (PrepGeom::FIX): half as much again as a uniform partition holds, at most what the LDS stage takes
  const unsigned long long per = ((unsigned long long)g.E + pg.P - 1) / std::max(1u, pg.P);
  pg.FIX = (u32)std::min<unsigned long long>(pg.CAP, (per + per / 2ull + 1024ull + 15ull) & ~15ull);
  return pg;
}
// 4-byte interchange entries the partition pass may write
inline size_t prep_bps_part_entries(const MsmGeom& g, u32 log2_l) {
  PrepGeom pg = prep_bps_geom(g, log2_l);
  return std::max<size_t>(g.E, pg.FIX ? (size_t)pg.P * pg.FIX : 0);
}
inline size_t prep_bps_local_lds(const PrepGeom& pg) {
  return (size_t)(bps_local_fixed_words(1u << pg.SH) + pg.CAP) * sizeof(u32);
}
inline u32 prep_bps_partitions(const MsmGeom& g, u32 log2_l) { return g.B >> (10u - log2_l); }
inline u32 prep_bps_stride(const MsmGeom& g, u32 log2_l) {
  const u32 P = std::max(1u, prep_bps_partitions(g, log2_l));
  const unsigned long long per = ((unsigned long long)g.E + P - 1) / P;
  return (u32)((per + per / 2ull + 4096ull + 1023ull) & ~1023ull);
}
// lanes per bucket (log2): enough partitions that one fits the LDS stage and that the chip is filled (>= 128 partitions =
// 131 072 lanes), at most a wave per bucket.  -1: this geometry does not take the bucket-split pipeline.
inline int prep_bps_choose(const MsmGeom& g) {
  if (!g.precomp || g.n == 0 || g.S > 32u || g.B < 64u || (g.B & (g.B - 1u))) return -1;
  unsigned long long want = 128;
  while (want * 24576ull < g.E) want <<= 1;
  for (int l = 0; l <= 6; l++) {
    if ((10 - l) < 0 || (g.B >> (10 - l)) == 0) continue;
    const unsigned long long P = g.B >> (10 - l);
    if (P < want && l < 6) continue;
    if (P > PREP_MAX_P || (P & 1ull)) return -1;
    MsmGeom g2 = g;
    PrepGeom pg = prep_bps_geom(g2, (u32)l);
    if (pg.IB + pg.SH > 31u) return -1;
    if ((unsigned long long)g.E / P + 1024ull > pg.CAP) return -1;
    if (prep_scatter_lds(g, pg) > PREP_LDS_LIMIT || prep_bps_local_lds(pg) > PREP_LDS_LIMIT) return -1;
    if (P * (unsigned long long)prep_bps_stride(g, (u32)l) >= (1ull << 31)) return -1;
    return l;
  }
  return -1;
}
// what launch_prep_bps zeroes of one MSM, in words: the 16 flag words, the partition totals / starts / cursors, the heavy count --
// rounded up to a whole number of 256-byte lines (a batch's block of flag words and small arrays: BpsBatchBuffers::small_stride)
inline u32 prep_bps_small_block_words() { return (u32)(prep_small_fill_bytes(0) / sizeof(u32)); }

// ---- what a chain needs of a slot, in bytes (api_pipeline.inc: msm_plan allocates exactly these; each figure includes the slack
// the kernels may read or write past the end: 64 bytes, and behind the small arrays the 256 the fill's rounding may take) ----
struct PrepNeeds {
  size_t vals_a;      // the partition pass's interchange entries
  size_t vals_b;      // the transposed entry blocks
  size_t bpl_grp;     // group headers (8 bytes each)
  size_t bpl_order;   // the bucket every lane slot sums / every position of a partition's size order
  size_t prep_small;  // the flag words and the small arrays behind them
};
inline size_t prep_small_bytes(const MsmGeom& g) { return PREP_FLAG_WORDS * sizeof(u32) + prep_small_words(g) * sizeof(u32) + 256; }
inline PrepNeeds prep_bpl_needs(const MsmGeom& g) {
  const size_t groups = (size_t)prep_bpl_partitions(g) * prep_bpl_groups_per_partition();
  PrepNeeds nd;
  nd.vals_a = prep_bpl_part_entries(g) * 8 + 64;  // 64-bit interchange entries
  nd.vals_b = (size_t)prep_bpl_partitions(g) * prep_bpl_stride(g) * 4 + 64;
  nd.bpl_grp = groups * 8 + 64;
  nd.bpl_order = groups * BPL_GROUP * 4 + 64;
  nd.prep_small = prep_small_bytes(g);
  return nd;
}
inline PrepNeeds prep_bps_needs(const MsmGeom& g) {  // at g.bps_log2_l lanes per bucket
  const size_t P = prep_bps_partitions(g, g.bps_log2_l);
  PrepNeeds nd;
  nd.vals_a = prep_bps_part_entries(g, g.bps_log2_l) * 4 + 64;
  nd.vals_b = P * prep_bps_stride(g, g.bps_log2_l) * 4 + 64;
  nd.bpl_grp = P * BPS_GROUPS * 8 + 64;
  nd.bpl_order = (size_t)g.B * 4 + 64;  // position in a partition's size order -> bucket
  nd.prep_small = prep_small_bytes(g);
  return nd;
}

}  // namespace amsm
