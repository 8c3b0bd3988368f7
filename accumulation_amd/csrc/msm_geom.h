// The geometry of an MSM (msm_types.h: MsmGeom) as pure host arithmetic: window counts, the top digit of a walk, the chunk split of
// accumulate L0, window-relative indices, and what each pipeline makes of a key and a range.  No HIP, no amsm_ctx, no amsm_bases:
// api_pipeline.inc hands in the two records below (geom_key / geom_ctx), every launch grid and every ensure() size follows from the
// MsmGeom that comes out, and tests/cpp_host/msm_geom_check.cpp prints it at every rule edge without a GPU.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstring>

#include "../../include/amsm.h"
#include "msm_select.h"
#include "msm_types.h"
#include "prep_geom.h"

// Measured constants of accumulate L0 / L1 (each was A/B'd, the numbers are in DESIGN.md / profiles/)
namespace tune {
constexpr int K0_MAX = 32;      // largest chunk of accumulate L0 (24 -> 805, 32 -> 811-816 M pairs/s in 2^20 batches)
constexpr amsm::u32 K1 = 1024;  // buckets with more partials than this go to the workgroup-per-bucket path (extreme skew)
}  // namespace tune

namespace amsm {

// The key as geometry sees it (api_pipeline.inc: geom_key)
struct GeomKey {
  size_t n = 0;          // generators
  bool precomp = false;  // it carries a table of W levels: c, W, n_narrow and top_shift are the table's
  int c = 0, W = 0, n_narrow = 0, top_shift = 0;
};
// The context as geometry sees it (api_pipeline.inc: geom_ctx)
struct GeomCtx {
  int window_override = 0;  // amsm_ctx_set_window
  int wave_slots = 4096;    // resident accumulate-L0 waves (a multiple of 4)
  int top_sets = 0;         // AMSM_TOP_SETS
  u32 r_mod[8] = {};        // the scalar field's modulus, little-endian words (what top_window_shift_of takes)
};

// (window counts -- windows_for, slots_for, narrow_windows_for -- stand beside MsmGeom in msm_types.h, for the kernels' side too)
inline msel::TailPlan tail_plan_of(const MsmGeom& g, msel::Place place) { return msel::tail_plan(g.nb, g.n_sets, g.B, g.E, g.bpl == 1u, place); }

// The windows an MSM walks: its key's table's; c_plain > 0 (plain keys, the bucket-per-lane pipeline): that width, the widths adding
// up to 256 bits (n_narrow); else the window of its size, or the override.  Refused: a width the narrow windows cannot even out (23
// bits: 12 windows would need 20 narrow ones), and c outside 2..24.
struct Walk {
  int c = 0, W = 0;
  u32 n_narrow = 0;
  bool plain_bpl = false;  // a plain key's bucket-per-lane walk: top_shift and top_split apply
};
inline int walk_of(const GeomCtx& ctx, const GeomKey& key, size_t n, int c_plain, Walk* out) {
  Walk w;
  if (key.precomp) {
    w.c = key.c;
    w.W = key.W;
    w.n_narrow = (u32)key.n_narrow;
  } else {
    w.plain_bpl = c_plain > 0;
    w.c = w.plain_bpl ? c_plain : (ctx.window_override ? ctx.window_override : msel::key_window(n, false, false));
    w.W = windows_for(w.c);
    if (w.plain_bpl) w.n_narrow = narrow_windows_for((u32)w.c);
    if (w.n_narrow == ~0u) return AMSM_E_INVALID_ARG;
  }
  if (w.c < 2 || w.c > 24) return AMSM_E_INVALID_ARG;
  *out = w;
  return AMSM_OK;
}

// The top digit of a walk over the context's scalar field, once per geometry: MsmGeom::top_shift (a table's is the key's), the largest
// raw top digit, and the buckets of a set the shifted digits reach -- what the top window's entries spread over
struct TopDigit {
  u32 shift = 0;
  unsigned long long raw_max = 0, reach = 0;
};
inline TopDigit top_digit_of(const GeomCtx& ctx, const GeomKey& key, const Walk& w) {
  TopDigit t;
  const int s = top_window_shift_of(ctx.r_mod, w.c, w.W, (int)w.n_narrow, &t.raw_max);
  t.shift = key.precomp ? (u32)key.top_shift : (w.plain_bpl ? (u32)s : 0u);
  t.reach = top_window_reach(1u << (w.c - 1), t.raw_max, t.shift, w.n_narrow);
  return t;
}

// Chunk length of accumulate L0 for g.E entries: the grid should be a whole number of rounds of the resident wave slots (queried from
// the kernel's occupancy), so that no SIMD idles while a partial last round drains.  Sets K0, K0b, nA, T0 and n_chunks.
inline void chunk_split(MsmGeom& g, int wave_slots) {
  {
    // <= K0_max entries per lane per round of resident waves (24 measured best on MI355X for batches of MSMs,
    // tools/ab_pipeline.py: shorter chunks let the other MSMs' prep / tail kernels in sooner, longer ones save partials),
    // and the grid a WHOLE number of rounds: every resident lane gets `rounds` chunks whose sizes (multiples of 4: the
    // entries are read 16 bytes at a time) add up to its share of the list -- ra rounds of kb + 4 entries, then
    // rounds - ra of kb.  One size for all rounds left the last round of a 2^20-pair launch 56 % full.
    const unsigned long long lanes = (unsigned long long)wave_slots * 64ull;
    const unsigned long long kmax = (unsigned long long)tune::K0_MAX;
    const unsigned long long share = (g.E + lanes - 1) / lanes;  // entries per resident lane
    const unsigned long long rounds = std::max<unsigned long long>(1, (share + kmax - 1) / kmax);
    unsigned long long kb = (share / rounds) & ~3ull;
    if (kb < 12ull) {  // small problems: one size, at least 12 (2^16: 12 -> 0.57 ms per blocking call, 16 -> 0.59)
      unsigned long long k = (share + rounds - 1) / rounds;
      g.K0 = ((u32)std::min<unsigned long long>(std::max<unsigned long long>(k, 12ull), kmax) + 3u) & ~3u;
      g.K0b = g.K0;
      g.nA = 0xffffff00u;
    } else {
      const unsigned long long ra = (share - rounds * kb + 3ull) / 4ull;  // rounds that take 4 more entries (<= rounds)
      g.K0 = (u32)(kb + 4ull);
      g.K0b = (u32)kb;
      g.nA = (u32)(ra * lanes);  // lanes = 64 * wave_slots, wave_slots a multiple of 4: a multiple of 256
      if (ra >= rounds) {
        g.K0b = g.K0;
        g.nA = 0xffffff00u;
      }
    }
  }
  {
    unsigned long long t0 = (unsigned long long)g.nA * g.K0;
    if (t0 >= g.E) {  // phase A covers everything
      g.nA = (g.E + g.K0 - 1) / g.K0;
      g.nA = (g.nA + 255u) & ~255u;
      g.T0 = g.nA * g.K0;  // < E + 256 * K0: fits
      g.n_chunks = (g.E + g.K0 - 1) / g.K0;
    } else {
      g.T0 = (u32)t0;
      g.n_chunks = g.nA + (g.E - g.T0 + g.K0b - 1) / g.K0b;
    }
  }
}

// n pairs from base_off of the key.  The top window of a plain key's bucket-per-lane walk (c_plain > 0) owns top_sets = 2, 4 or 8
// bucket sets (MsmGeom::top_split) and is spread by top_shift (top_digit_of: bpl_geom has it)
inline int make_geom(const GeomCtx& ctx, const GeomKey& key, size_t base_off, size_t n, MsmGeom* out, int group_shift = -1, int c_plain = 0,
                     u32 top_sets = 2, u32 top_shift = 0) {
  MsmGeom g;
  memset(&g, 0, sizeof(g));
  Walk w;
  if (int s = walk_of(ctx, key, n, c_plain, &w)) return s;
  if (w.plain_bpl) {
    if (top_sets != 2u && top_sets != 4u && top_sets != 8u) return AMSM_E_INVALID_ARG;
    g.top_split = top_sets - 1u;
  }
  g.n = (u32)n;
  g.c = (u32)w.c;
  g.W = (u32)w.W;
  g.n_narrow = w.n_narrow;
  g.top_shift = key.precomp ? (u32)key.top_shift : (w.plain_bpl ? top_shift : 0u);
  g.nb = 1u << (w.c - 1);
  g.groups = group_shift >= 0 ? 2u : 1u;
  g.group_shift = group_shift >= 0 ? (u32)group_shift : 0u;
  g.n_sets = g.groups * (key.precomp ? 1u : g.W + g.top_split);
  g.B = g.n_sets * g.nb;
  g.S = (u32)slots_for(w.c);
  if ((unsigned long long)n * g.S >= (1ull << 30)) return AMSM_E_UNSUPPORTED;  // entry words carry a 30-bit index
  g.E = (u32)(n * g.S);
  g.base_off = (u32)base_off;
  g.table_stride = (u32)key.n;
  g.precomp = key.precomp ? 1u : 0u;
  if ((unsigned long long)key.n * (key.precomp ? w.W : 1) >= (1ull << 30)) return AMSM_E_UNSUPPORTED;
  chunk_split(g, ctx.wave_slots);
  g.K1 = tune::K1;
  *out = g;  // (red_s / red_threads: the tail's plan, msm_select.h -- launch_tail fills them in)
  return AMSM_OK;
}

// MsmGeom::idx_rel_bits of an MSM over a window of a longer precomputed key: b = ceil log2 n where the window-relative word
// (w << b) | i is SHORTER than the absolute index, else 0.  One group only, and a table only: bpl_geom_sets and chunked_geom asked for
// both; bps_geom asked for one group alone, but for a key without a table it returns false with the bits or without
// (prep_bps_choose refuses it first), so the one guard changes nothing there.
// What follows differs by caller: bucket-per-lane keeps the bits, bucket-split tries again without them, chunked keeps them only
// where the short prep chain takes the geometry with them.
inline u32 idx_rel_bits_for(const MsmGeom& g) {
  if (g.groups != 1u || !g.precomp) return 0u;
  u32 b = 1;
  while ((1ull << b) < g.n) b++;
  const unsigned long long abs_max = (unsigned long long)g.base_off + g.n - 1ull + (unsigned long long)(g.W - 1u) * g.table_stride;
  const unsigned long long rel_max = ((unsigned long long)(g.W - 1u) << b) | ((1ull << b) - 1ull);
  return rel_max < abs_max ? b : 0u;
}

// lanes cooperating on one bucket in accumulate L1 (tree over partials): more lanes = lower latency,
// but only worth it when buckets have several partials each
// `hidden`: the tail runs behind the next MSM's accumulation (inside a batch): what counts is its ALU work, not its
// depth -- one lane per bucket does no butterfly additions at all when there are buckets enough to fill the lanes.
// Measured (round 2, 2^20 Pallas, stand-alone kernel): 16 lanes per bucket 0.23 ms, 4 lanes 0.107 ms for ~21-26 partials per
// bucket -- the wide tree only pays when there are too few buckets to occupy the chip with 4 lanes each.
inline u32 l1_lanes(const MsmGeom& g, bool hidden) {
  double avg = (double)g.n_chunks / g.B;
  if (hidden && g.B >= 16384u) return avg >= 48.0 ? 4u : 1u;
  if (avg >= 24.0 && g.B * 16ull <= 65536ull) return 16u;
  return avg >= 3.0 ? 4u : 1u;
}

// The geometry of an MSM on the bucket-per-lane pipeline with the top window of a plain key on top_sets sets -- false when the prep
// cannot take it (prep_bpl_supported)
inline bool bpl_geom_sets(const GeomCtx& ctx, const GeomKey& key, size_t base_off, size_t n, int group_shift, int c_plain, u32 top_sets,
                          const TopDigit& top, MsmGeom* out) {
  MsmGeom g;
  if (make_geom(ctx, key, base_off, n, &g, group_shift, c_plain, top_sets, top.shift) != AMSM_OK) return false;
  g.idx_rel_bits = idx_rel_bits_for(g);
  g.bpl = 1;
  // entries the fullest 1024-bucket partition expects: a window's n digits spread over the bucket range -- the top window's
  // over the part of it its raw values reach (r / 2^256 of the range: no sign to fold, and only as far as top_shift spreads it)
  if (g.precomp) {  // W windows share one bucket set
    const unsigned long long per_win = ((unsigned long long)n * 1024ull + g.nb - 1) / g.nb;  // a regular window's, per partition
    const unsigned long long per_top = ((unsigned long long)n * 1024ull + top.reach - 1) / top.reach;
    g.part_max = (u32)std::min<unsigned long long>(0xffffffffull, (g.W - 1ull) * per_win + per_top);
    if (g.groups > 1u) g.part_max = (g.part_max + 1u) / 2u;  // (a group sees half the scalars)
  } else {
    // (a plain key's top window is split over T sets, MsmGeom::top_split; what is sized for is TWICE the uniform load of one:
    // msm_select.h: plain_part_max)
    g.part_max = (u32)std::min<unsigned long long>(0xffffffffull, msel::plain_part_max(n, g.nb, top.reach, top_sets, g.groups));
  }
  if (!prep_bpl_supported(g)) return false;
  *out = g;
  return true;
}
// The geometry of an MSM on the bucket-per-lane pipeline (msm_select.h chose it; c_plain = the window of a plain key, 0 for a
// 20-bit table) -- false when the prep cannot take it (the caller falls back to the chunked pipeline).
inline bool bpl_geom(const GeomCtx& ctx, const GeomKey& key, size_t base_off, size_t n, int group_shift, int c_plain, MsmGeom* out) {
  Walk w;
  if (walk_of(ctx, key, n, c_plain, &w) != AMSM_OK) return false;
  const TopDigit top = top_digit_of(ctx, key, w);
  if (!w.plain_bpl) return bpl_geom_sets(ctx, key, base_off, n, group_shift, c_plain, 2, top, out);
  // a plain key: the sets of its top window (msm_select.h: plain_top_sets) -- AMSM_TOP_SETS = 4 / 8 where the prep takes that geometry,
  // else the smallest count that fits its stage (AMSM_TOP_SETS=2: two or none)
  if (ctx.top_sets > 2 && bpl_geom_sets(ctx, key, base_off, n, group_shift, c_plain, (u32)ctx.top_sets, top, out)) return true;
  const u32 T = msel::plain_top_sets(n, 1u << (w.c - 1), top.reach, (u32)w.W, group_shift >= 0 ? 2u : 1u, msel::BPL_STAGE_CAP,
                                     msel::plain_top_sets_cap(ctx.top_sets));
  return T != 0u && bpl_geom_sets(ctx, key, base_off, n, group_shift, c_plain, T, top, out);
}

// The geometry of an MSM on the bucket-split pipeline (precomputed key, one or two bucket sets, 2^16 .. 2^17 pairs: msm_select.h) --
// false when no lane count fits (prep_bps_choose).  Where it was measured to win (same-process A/B against the chunked pipeline,
// Pallas, uniform scalars): 2^16 pairs -- a blocking call 0.400 -> 0.354 ms, batches 216 -> 250 M pairs/s -- and 2^17 (357 -> 383);
// below 2^16 the parts get too short (the padded blocks overflow their stride), from 2^18 up the chunked pipeline's longer runs win.
inline bool bps_geom(const GeomCtx& ctx, const GeomKey& key, size_t base_off, size_t n, int group_shift, MsmGeom* out) {
  MsmGeom g;
  if (make_geom(ctx, key, base_off, n, &g, group_shift) != AMSM_OK) return false;
  g.idx_rel_bits = idx_rel_bits_for(g);
  int l = prep_bps_choose(g);
  if (l < 0 && g.idx_rel_bits) {
    g.idx_rel_bits = 0;
    l = prep_bps_choose(g);
  }
  if (l < 0) return false;
  g.bpl = 2;
  g.bps_log2_l = (u32)l;
  *out = g;
  return true;
}

// The geometry of an MSM on the chunked pipeline, and which prep chain it takes: the short one (prep_kernels.h) where its word layout
// takes the geometry; else (windows below 8 bits: tiny plain keys, window overrides) the rocPRIM sort.  The interchange word of the
// short chain's partition pass carries window-relative indices, so that its bucket-id bits -- the number of partitions -- follow the
// MSM's size, not the key's
inline int chunked_geom(const GeomCtx& ctx, const GeomKey& key, size_t base_off, size_t n, int group_shift, MsmGeom* out, bool* short_prep_out) {
  MsmGeom g;
  if (int s = make_geom(ctx, key, base_off, n, &g, group_shift)) return s;
  MsmGeom g2 = g;
  g2.idx_rel_bits = idx_rel_bits_for(g);
  if (g2.idx_rel_bits && prep_supported(g2)) g = g2;
  *short_prep_out = prep_supported(g);
  *out = g;
  return AMSM_OK;
}

// ---- a unit of bucket-split MSMs (msm_select.h: batch_units) ----
// The unit as its tail sees it: nv * n_sets bucket sets in one table, one result ("group") per MSM -- what msm_collect's horner hands out
inline MsmGeom bps_unit_geom(const MsmGeom& g, u32 nv) {
  MsmGeom u = g;
  u.n_sets = g.n_sets * nv;
  u.groups = nv;
  u.B = g.B * nv;
  return u;
}
inline msel::TailPlan bps_unit_tail(const MsmGeom& g, u32 nv, msel::Place place) {
  return msel::tail_plan(g.nb, g.n_sets * nv, g.B * nv, g.E * nv, false, place);
}
// Does the bucket-split geometry of n pairs at `off` of `key` (the key the MSMs run over) take the batched kernels?  One bucket set
// per MSM, and at most 16 entry slots per scalar (windows of 16 bits and more: what every key long enough for 2^16 pairs has --
// k_prep_scatter_batch is built for that width only)
inline bool bps_unit_geom_ok(const GeomCtx& ctx, const GeomKey& key, size_t off, size_t n, MsmGeom* g) {
  return bps_geom(ctx, key, off, n, -1, g) && g->n_sets == 1u && g->S <= 16u;
}

}  // namespace amsm
