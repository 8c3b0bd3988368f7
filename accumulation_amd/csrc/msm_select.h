// Which pipeline an MSM takes, which table a key is built with, and which form its tail takes: ONE place, three tables, no HIP -- plain
// C++ that the host launcher (api_pipeline.inc, api_keys.inc) and the kernels' launchers (kern_ec.inc) include and that
// tests/cpp_host/select_check.cpp compiles on its own to check every threshold edge without a GPU (tests/test_pipeline_select_cpu.py).
// Every size threshold of the library lives here; the numbers are measured on MI355X (same-process A/B, DESIGN.md section 4.2 and
// profiles/), not derived.
//
// The four accumulation forms:
//   DIRECT_SUM       keys of up to 2^15 generators that carry every multiple a 4-bit signed digit can ask for: one launch that sums
//                    table points, no buckets (msm_kernels.h k_direct_sum)
//   BUCKET_SPLIT     2^16 .. 2^17 pairs over a precomputed key: every bucket on 2 .. 64 adjacent lanes (k_prep_local_s + k_accum_bps)
//   BUCKET_PER_LANE  (2^18, 2^20] pairs: a lane sums one whole bucket; 20-bit windows over a precomputed key of >= 2^20 generators,
//                    one bucket set per 16- / 15-bit window over a plain key, 2, 4 or 8 for the top one: plain_top_sets
//                    (k_prep_local_t + k_accum_bpl)
//   CHUNKED          everything else, and every vector whose digits are skewed: equal-sized work items whatever the digit
//                    distribution (k_accum_l0 + k_accum_l1)
// Longer MSMs are cut into ranges first (`range`), each range is chosen again; the ranges of one vector over a bucket-per-lane key
// share one bucket set (api_types.h: struct Share).
// Table 3, `tail_plan`: the bucket reduction, fold and export behind any of them -- form, grids and what the slot must hold.
// Beside the tables: `classify`, what a call makes of its vectors' two-valued probes (two-valued, all zero, unit scalars summed apart).
#pragma once
#include <math.h>
#include <stddef.h>

#include <initializer_list>

namespace amsm {
namespace msel {

enum Pipeline { DIRECT_SUM = 0, BUCKET_SPLIT = 1, BUCKET_PER_LANE = 2, CHUNKED = 3 };
inline const char* pipeline_name(int p) {
  return p == DIRECT_SUM ? "direct_sum" : (p == BUCKET_SPLIT ? "bucket_split" : (p == BUCKET_PER_LANE ? "bucket_per_lane" : "chunked"));
}

inline int ilog2_ceil(size_t n) {
  int l = 0;
  while (((size_t)1 << l) < n) l++;
  return l;
}
constexpr size_t P2(int k) { return (size_t)1 << k; }

// ---- table 1: the window width a key's table is built for --------------------------------------------------------------------------
// Measured, not derived (tools/sweep_window.py): a width whose TOP window holds only 2-3 scalar bits (255 mod c small: 9, 11, 12, 14,
// 18, 19) puts 1/8 of that window's entries into a handful of buckets.
constexpr int BPL_WINDOW = 20;      // keys of >= 2^20 generators: 13 windows whose widths add up to 256 bits (9 x 20 + 4 x 19)
constexpr int DIRECT_MAX_LOG2 = 15; // largest key (log2 generators) that also carries the direct-sum table (AMSM_DIRECT_SUM_MAX_LOG2)
struct KeyWindowRow {
  int lg_lo, lg_hi;  // ceil(log2 generators) in [lg_lo, lg_hi]
  int c;
};
// precomputed keys (all windows share one bucket set)
constexpr KeyWindowRow kPrecomputedWindow[] = {
    {0, 12, 8}, {13, 14, 10}, {15, 15, 13}, {16, 16, 16}, {17, 17, 17}, {18, 19, 16}, {20, 64, 17 /* AMSM_BPL=0; else BPL_WINDOW */}};
// plain keys on the chunked pipeline (one bucket set per window; longer ones take the bucket-per-lane rows of table 2)
constexpr KeyWindowRow kPlainChunkedWindow[] = {{0, 8, 4}, {9, 19, 8}, {20, 20, 13}, {21, 21, 15}, {22, 64, 16}};
inline int key_window(size_t n_generators, bool precomputed, bool bpl_enabled) {
  const int lg = ilog2_ceil(n_generators < 2 ? 2 : n_generators);
  if (precomputed && bpl_enabled && lg >= 20) return BPL_WINDOW;
  if (precomputed) {
    for (const KeyWindowRow& r : kPrecomputedWindow)
      if (lg >= r.lg_lo && lg <= r.lg_hi) return r.c;
    return 17;
  }
  for (const KeyWindowRow& r : kPlainChunkedWindow)
    if (lg >= r.lg_lo && lg <= r.lg_hi) return r.c;
  return 16;
}

// ---- table 2: the pipeline of an MSM -----------------------------------------------------------------------------------------------
enum KeyKind {
  KEY_DIRECT = 0,  // precomputed, <= 2^15 generators, carries the direct-sum table
  KEY_BPL = 1,     // precomputed for 20-bit windows (>= 2^20 generators): amsm_bases::bpl
  KEY_TABLE = 2,   // any other precomputed key
  KEY_PLAIN = 3    // one copy of the generators
};
struct KeyDesc {
  size_t n;           // generators
  bool precomputed;
  bool bpl;           // 20-bit bucket-per-lane table
  bool direct_table;  // 512 points per generator present
  int c;              // the table's window width (0: plain)
};
inline KeyKind key_kind(const KeyDesc& k) {
  if (!k.precomputed) return KEY_PLAIN;
  if (k.direct_table) return KEY_DIRECT;
  return k.bpl ? KEY_BPL : KEY_TABLE;
}
struct Switches {              // the context's documented switches (include/amsm.h lists the environment variables)
  bool bpl = true;             // AMSM_BPL=0: no MSM takes the bucket-per-lane pipeline (and keys are built without 20-bit tables)
  bool bpl_plain = true;       // AMSM_BPL_PLAIN=0: plain keys stay on the chunked pipeline
  int bps = 2;                 // AMSM_BPS: 0 never, 1 grouped MSMs only, 2 every candidate
  int split_log2 = 21;         // AMSM_SPLIT_LOG2: range of an MSM over a key WITHOUT a 20-bit table (0: never cut)
  bool direct = true;          // AMSM_DIRECT_SUM_MAX_LOG2=0: no direct sums
  bool window_override = false;  // amsm_ctx_set_window: everything chunked with that width
  int bps_batch = 8;           // AMSM_BPS_BATCH: bucket-split MSMs per launch (batch_units below); 0 or 1: every MSM a chain of its own
  int top_sets = 0;            // AMSM_TOP_SETS: bucket sets of a plain key's top window -- 0 the rule (plain_top_sets), 2, 4 or 8
};
struct Row {
  KeyKind kind;
  size_t lo, hi;       // pairs in (lo, hi]
  Pipeline pipeline;
  bool over_twin;      // KEY_BPL only: the MSM runs over the key's 17-bit twin (built on first use)
  int plain_window;    // KEY_PLAIN on the bucket-per-lane pipeline: its window width
  const char* why;
};
constexpr size_t BPS_MIN_PAIRS = P2(16), BPS_MAX_PAIRS = P2(17), RANGE_PAIRS = P2(20), SPLIT_MIN_LOG2 = 22;
// First matching row wins.  (2^20 pairs = one window of a 20-bit key; a range below a QUARTER of it fills the 2^19 buckets too thinly.)
constexpr Row kPipeline[] = {
    {KEY_DIRECT, 0, P2(DIRECT_MAX_LOG2), DIRECT_SUM, false, 0, "latency regime: one launch + the fold, 0.10-0.28 ms against 0.24-0.36"},
    {KEY_BPL, P2(18), RANGE_PAIRS, BUCKET_PER_LANE, false, 0, "13 gathered additions per pair, no partial records"},
    {KEY_BPL, BPS_MIN_PAIRS - 1, BPS_MAX_PAIRS, BUCKET_SPLIT, true, 0, "a short range of a long key: the twin's 17-bit windows"},
    {KEY_BPL, 0, P2(18), CHUNKED, true, 0, "a short range of a long key: the twin's 17-bit windows"},
    {KEY_TABLE, BPS_MIN_PAIRS - 1, BPS_MAX_PAIRS, BUCKET_SPLIT, false, 0, "three dispatches fewer in a latency-bound chain"},
    {KEY_TABLE, 0, ~(size_t)0, CHUNKED, false, 0, "round 2's path: 2^18 / 2^19 generators, BLS12-381 below 2^20, tiny keys"},
    {KEY_DIRECT, 0, ~(size_t)0, CHUNKED, false, 0, "(a direct-sum key asked for more pairs than it has: never reached, n <= key)"},
    {KEY_PLAIN, P2(18), RANGE_PAIRS, BUCKET_PER_LANE, false, 16, "16 x 16-bit windows, one bucket set each: the VariableBaseMSM shape"},
    {KEY_PLAIN, P2(17), P2(18), BUCKET_PER_LANE, false, 15, "18 windows whose widths add up to 256 bits (14 of 14 bits)"},
    {KEY_PLAIN, 0, P2(17), CHUNKED, false, 0, "8-bit windows (4 up to 2^8 pairs) win below 2^17 pairs"},
};
struct Choice {
  Pipeline pipeline;
  bool over_twin;
  int plain_window;
  size_t range;      // > 0: cut the MSM into ranges of this many pairs first (each range is chosen again)
  const Row* row;    // the table row (null: decided by a switch or by skew)
};
// How an MSM longer than the pipelines take is cut: windows of 2^20 pairs over a 20-bit key or a plain key, of 2^split_log2
// (from 2^22 pairs up) over any other precomputed key.
inline size_t range_of(const KeyDesc& k, size_t n, const Switches& sw) {
  if (!k.precomputed) return (sw.bpl && sw.bpl_plain && !sw.window_override && n > RANGE_PAIRS) ? RANGE_PAIRS : 0;
  if (k.bpl && sw.bpl) return n > RANGE_PAIRS ? RANGE_PAIRS : 0;
  return (sw.split_log2 > 0 && (n >> SPLIT_MIN_LOG2) != 0) ? P2(sw.split_log2) : 0;
}
// grouped: two sums by one bit of the index (the IPA rounds); grouped_regular: both classes hold n / 2 indices in the regular pattern
// (n a multiple of 2 << group_shift) -- what the direct sum needs; skewed: the digit probe's verdict (or a prep's overflow flag).
inline Choice choose(const KeyDesc& k, size_t n, bool grouped, bool grouped_regular, bool skewed, const Switches& sw) {
  Choice ch{CHUNKED, false, 0, 0, nullptr};
  const KeyKind kind = key_kind(k);
  ch.over_twin = kind == KEY_BPL;  // whatever does not take the 20-bit table runs over the twin
  if (n == 0) return ch;
  // the direct sum has no buckets: nothing to skew, nothing to cut
  if (kind == KEY_DIRECT && sw.direct && !sw.window_override && n <= k.n && (!grouped || grouped_regular)) {
    ch.pipeline = DIRECT_SUM;
    ch.over_twin = false;
    ch.row = &kPipeline[0];
    return ch;
  }
  ch.range = range_of(k, n, sw);
  if (ch.range) {
    ch.over_twin = false;
    return ch;  // (the pipeline is chosen per range)
  }
  if (skewed || sw.window_override) return ch;
  for (const Row& r : kPipeline) {
    if (r.kind != kind || n <= r.lo || n > r.hi || r.pipeline == DIRECT_SUM) continue;
    if (r.pipeline == BUCKET_PER_LANE && (!sw.bpl || (kind == KEY_PLAIN && !sw.bpl_plain))) continue;
    if (r.pipeline == BUCKET_SPLIT && (sw.bps == 0 || (sw.bps == 1 && !grouped))) continue;
    ch.pipeline = r.pipeline;
    ch.over_twin = r.over_twin;
    ch.plain_window = r.plain_window;
    ch.row = &r;
    return ch;
  }
  return ch;
}
// Is a digit probe worth its launch for this vector?  Only where a skewed vector would otherwise pay an aborted prep and a re-run:
// the sorted pipelines over precomputed keys (plain keys find out from the prep's overflow flag).
inline bool wants_skew_probe(const KeyDesc& k, size_t n, const Switches& sw) {
  if (!k.precomputed) return false;
  const size_t r = range_of(k, n, sw);
  const Choice ch = choose(k, r ? r : n, false, false, false, sw);
  return ch.pipeline == BUCKET_PER_LANE || ch.pipeline == BUCKET_SPLIT;
}

// ---- the jobs of one call: which bucket-split MSMs run as ONE launch per pipeline stage ---------------------------------------------
// One bucket-split MSM of 2^16 pairs fills about a sixth of the chip and is a chain of five commands; the provers issue 2 .. 11 such
// commitments per round over one key.  batch_units cuts the live job list of a call into UNITS: one job (today's path), or a run
// of 2 .. BPS_BATCH consecutive jobs that share everything but their scalars -- key, range, scalar form, unit-scalar handling -- and
// so one MsmGeom; the unit runs as memset, scatter, local sort, accumulate (grid.y = MSM) and one tail over all its bucket sets
// (api_pipeline.inc: msm_enqueue_bps_batch).  6 to 8 MSMs of 2^16 pairs fill the chip: BPS_BATCH = 8.
constexpr int BPS_BATCH = 8;
// what a unit may take of a slot (entry buffers, group headers, bucket order, buckets, small arrays of all its MSMs).  A stated
// cap, not a measurement: three slots then stay below 1.5 GiB
constexpr size_t BPS_BATCH_MAX_BYTES = (size_t)512 << 20;
struct BatchJob {
  const void* key;     // identity of the key the job names
  KeyDesc desc;        // ... and how it looks to `choose`
  size_t off, n;
  int mont;
  int group_shift;     // >= 0: grouped (never joins a unit)
  bool shared;         // one range of a shared bucket set (never joins a unit)
  bool force_chunked;
  bool skip_ones;
  bool geom_ok;        // the bucket-split geometry exists for it (api_pipeline.inc: bps_geom)
  size_t slot_bytes;   // what ONE such MSM takes of a slot
};
struct Unit {
  size_t first, count;  // jobs [first, first + count)
};
// may job j stand in a unit at all?
inline bool batch_candidate(const BatchJob& j, const Switches& sw) {
  if (sw.bps_batch < 2 || j.n == 0 || j.group_shift >= 0 || j.shared || j.force_chunked || !j.geom_ok) return false;
  return choose(j.desc, j.n, false, false, false, sw).pipeline == BUCKET_SPLIT;
}
inline bool batch_same_run(const BatchJob& a, const BatchJob& b) {
  return a.key == b.key && a.off == b.off && a.n == b.n && a.mont == b.mont && a.skip_ones == b.skip_ones;
}
// units[0 .. return) cover jobs [0, k) in order (room for k units); a run longer than the cap is cut into full units, a remainder of one
// is a single
inline size_t batch_units(const BatchJob* jobs, size_t k, const Switches& sw, Unit* units) {
  size_t n_units = 0;
  for (size_t i = 0; i < k;) {
    size_t run = 1;
    if (batch_candidate(jobs[i], sw))
      while (i + run < k && batch_candidate(jobs[i + run], sw) && batch_same_run(jobs[i], jobs[i + run])) run++;
    size_t cap = (size_t)(sw.bps_batch < BPS_BATCH ? sw.bps_batch : BPS_BATCH);
    if (run > 1 && jobs[i].slot_bytes) {
      const size_t fit = BPS_BATCH_MAX_BYTES / jobs[i].slot_bytes;
      if (fit < cap) cap = fit;
    }
    if (cap < 1) cap = 1;
    for (size_t done = 0; done < run;) {
      const size_t v = run - done < cap ? run - done : cap;
      units[n_units++] = Unit{i + done, v};
      done += v;
    }
    i += run;
  }
  return n_units;
}

// ---- the vectors of one call: which skip the windowed pipelines, which run them without their unit scalars -------------------------
// What the host reads of a device vector's two-valued probe (vec_kernels.h k_tv_probe: exact test plus 1024 samples) and what it
// makes of it.  words: the vector's probe block as read back (null: not probed -- too short, or the shortcut is off).
constexpr unsigned TVW_MIXED = 0, TVW_TWO_VALUED = 1, TVW_ALL_ZERO = 2, TVW_N_EXC = 3, TVW_ONES = 4, TVW_VALUE = 8;  // word indices
// unit scalars among the probe's 1024 samples from which a vector's ones are summed apart (0.8 %: below the skew probe's 24 of
// 1024 in one bin, so what that probe no longer sees is always taken out)
constexpr unsigned TV_ONES_MIN_SAMPLES = 8;
enum Verdict {
  V_REGULAR = 0,     // the windowed pipelines, as it is
  V_TWO_VALUED = 1,  // every scalar 0 or one value v: v * (sum of the generators under v), no pipeline
  V_ALL_ZERO = 2,    // the identity, nothing to launch
  V_ONES_APART = 3   // the pipelines without its unit scalars (MsmJob::skip_ones), their generators summed apart
};
struct VecProbe {
  const unsigned* words;
  size_t n;             // pairs
  const char* scalars;  // first byte of its n * 32 bytes of scalars
};
inline void classify(const VecProbe* vec, size_t k, bool mont, const KeyDesc& key, const Switches& sw, unsigned char* verdict) {
  for (size_t v = 0; v < k; v++) {
    verdict[v] = V_REGULAR;
    const unsigned* f = vec[v].words;
    if (!f) continue;
    // canonical-form vectors (mont == 0) whose value is 2^255 or more keep to the windowed pipelines, which report such
    // scalars (include/amsm.h: AMSM_E_SCALAR_RANGE) -- the shortcut must not turn that error into a result; values in
    // [r, 2^255) give the same point either way.  The vector's exceptions, a handful of scalars read back after the sum, are
    // checked when they arrive (msm_multi_split_xyzz: tv_bad)
    if (f[TVW_MIXED] == 0u && f[TVW_TWO_VALUED] == 1u && (mont || (f[TVW_VALUE + 7] >> 31) == 0u)) {
      verdict[v] = V_TWO_VALUED;
      continue;
    }
    if (f[TVW_MIXED] == 0u && f[TVW_TWO_VALUED] != 1u && f[TVW_ALL_ZERO] == 1u) {
      verdict[v] = V_ALL_ZERO;
      continue;
    }
    // Round 5: vectors with a SHARE of unit scalars (the boolean wires of an R1CS witness; ark-ec's multi_scalar_mul adds their bases
    // directly) are not two-valued, but all their ones would land in bucket 1 of the lowest window (measured, M pairs/s in batches:
    // 2^18 pairs with 10 % booleans 2.2x slower than uniform, a plain 2^20 key 2.3x).
    // (not where the MSM would be a direct sum: that form has no buckets to skew)
    // (nor over a 20-bit table: the skew probe sends such a vector to the chunked pipeline over the key's 17-bit twin, where the
    // ones cost little -- 2^20 pairs in batches, 10 / 50 / 90 % booleans: 1.21 / 0.85 / 0.52 ms against 1.13 / 0.91 / 0.75 with the
    // separate sum, a uniform vector 1.10)
    if (f[TVW_ONES] >= TV_ONES_MIN_SAMPLES && !key.bpl && choose(key, vec[v].n, false, false, false, sw).pipeline != DIRECT_SUM)
      verdict[v] = V_ONES_APART;
  }
  // a vector sharing memory with one of the call that keeps its ones gives the form up (protects nothing now that MsmJob carries skip_ones)
  for (bool changed = true; changed;) {
    changed = false;
    for (size_t v = 0; v < k; v++) {
      if (verdict[v] != V_ONES_APART) continue;
      const char *a0 = vec[v].scalars, *a1 = a0 + vec[v].n * 32;
      for (size_t u = 0; u < k && verdict[v] == V_ONES_APART; u++) {
        if (u == v || verdict[u] != V_REGULAR || vec[u].n == 0) continue;
        const char *b0 = vec[u].scalars, *b1 = b0 + vec[u].n * 32;
        if (a0 < b1 && b0 < a1) verdict[v] = V_REGULAR, changed = true;
      }
    }
  }
}

// ---- plain keys on the bucket-per-lane pipeline: how many bucket sets the TOP window owns --------------------------------------------
// The prep sorts one 1024-bucket partition per workgroup in an LDS stage of BPL_STAGE_CAP entries (prep_geom.h asserts the figure
// against k_prep_local_t's layout).  bpl_stage_fits: the two inequalities every bucket-per-lane geometry must meet (prep_geom.h:
// prep_bpl_supported calls it) -- E entries over P partitions, the average one with 1024 to spare, and the fullest one expected on
// uniform scalars (part_max; 0: not known) with 5 sigma of the digits' spread to spare (sigma = sqrt(part_max): ~180 at 30 k).
constexpr unsigned BPL_STAGE_CAP = 37340;
inline bool bpl_stage_fits(unsigned long long E, unsigned long long P, unsigned long long part_max, unsigned cap) {
  if (P == 0 || E / P + 1024ull > cap) return false;
  return !(part_max && part_max + 5ull * (unsigned long long)sqrt((double)part_max) > cap);
}
// A plain key's top window starts at bit 240 (16-bit windows) or 242 (15-bit): its raw digits reach only (r - 1) >> lo, carry no sign
// to fold, and top_shift spreads them by a power of two only -- they cover `reach` of the set's nb buckets (msm_types.h:
// top_window_reach), so a partition of the top window expects n * 1024 / reach entries where the others expect n * 1024 / nb.  The
// top window therefore owns T bucket sets, picked by index bits (MsmGeom::top_split, window_set), and the stage is sized for TWICE
// the uniform load of one of them: scalars a bit short of the field's width -- the 254-bit stream of rng.h on BLS12-381 -- fill half
// the reach.  groups == 2: a group sees half the scalars.
inline unsigned long long plain_part_max(size_t n, unsigned nb, unsigned long long reach, unsigned T, unsigned groups) {
  const unsigned long long per_win = ((unsigned long long)n * 1024ull + nb - 1) / nb;  // a regular window's, per partition
  const unsigned long long per_top = ((unsigned long long)n * 1024ull + reach - 1) / reach;
  const unsigned long long top = (2ull * per_top + T - 1) / T;
  const unsigned long long pm = per_win > top ? per_win : top;
  return groups > 1u ? (pm + 1ull) / 2ull : pm;
}
// T: the smallest of 2, 4, 8 (<= max_sets) with which n pairs over W windows of nb buckets fit the stage; 0: none does -- the MSM
// stays chunked.  T = 2 is what every plain key had before the rule: a shape that fitted then keeps its geometry bit for bit.
inline unsigned plain_top_sets(size_t n, unsigned nb, unsigned long long reach, unsigned W, unsigned groups, unsigned cap = BPL_STAGE_CAP,
                               unsigned max_sets = 8) {
  if (n == 0 || nb < 1024u || reach == 0 || W == 0) return 0;
  for (unsigned T = 2; T <= max_sets && T <= 8u; T *= 2u) {
    const unsigned long long P = ((unsigned long long)groups * (W + T) * nb) >> 10;
    if (bpl_stage_fits((unsigned long long)n * W, P, plain_part_max(n, nb, reach, T, groups), cap)) return T;
  }
  return 0;
}
// AMSM_TOP_SETS (Switches::top_sets): 0 the rule decides, 2 never more than two sets (the behaviour before the rule), 4 / 8 that
// many wherever the prep takes the geometry (api_pipeline.inc: bpl_geom falls back to the rule where it does not)
inline unsigned plain_top_sets_cap(int top_sets) { return top_sets == 2 ? 2u : 8u; }

// ---- table 3: the tail of an MSM -- the bucket reduction (per set sum_j (j + 1) bucket_j), the fold of its partial records, the export ----
// Where an MSM stands in its call (msm_enqueue): whether anybody waits for its tail, and whether anything can overlap with it
enum class Place {
  LONE,         // the only MSM of a blocking call: exposed tail, the whole chain on the caller's stream
  BATCH_LAST,   // the last MSM of a batch (or a re-run inside one): exposed tail, on the per-stage streams
  BATCH_INNER,  // another MSM is queued behind it: its tail is hidden behind that one's accumulation
};
inline Place place_of(size_t i, size_t count) { return count == 1 ? Place::LONE : (i + 1 == count ? Place::BATCH_LAST : Place::BATCH_INNER); }
enum TailForm {
  RED2 = 0,        // row / column sums, their small multiples, the fold: three launches (k_red2_sums, k_red2_weighted, k_fold)
  FUSED_QUAD = 1,  // running sums on quads of lanes; the last workgroup of a set to arrive folds it: one launch (k_bucket_reduce)
  ONE_LANE = 2     // running sums on single lanes, then the one-wave fold: two launches (k_bucket_reduce, k_fold)
};
inline const char* tail_form_name(int f) { return f == RED2 ? "red2" : (f == FUSED_QUAD ? "fused_quad" : "one_lane"); }
constexpr int TAIL_QUAD_HIDDEN_LOG2 = 17;  // bucket tables up to 2^this take the quad tail inside a batch too (2^16 234 -> 283 M pairs/s)
constexpr unsigned RED2_COLS = 1024, RED2_MIN_NB = 1u << 18;
inline unsigned cdiv_u(unsigned a, unsigned b) { return (a + b - 1) / b; }
// the row / column form's grid (msm_kernels.h: k_red2_sums): nb a multiple of RED2_COLS
struct Red2Geom {
  unsigned A;      // rows = nb / 1024
  unsigned gw;     // lanes per row group (power of two <= 64): row strips of 1024 / gw columns
  unsigned gc;     // lanes per column group (power of two <= 64, <= A): column strips of A / gc rows
  unsigned row_waves, col_waves;  // waves per set in each mode
};
inline Red2Geom red2_geom(unsigned nb, bool latency) {
  Red2Geom r;
  r.A = nb / RED2_COLS;
  // latency (an exposed tail, or a small table whose chain would bound a batch): short strips, wide butterflies; otherwise long
  // strips -- fewer butterfly additions (a butterfly level costs every lane of the wave one addition)
  r.gw = latency ? 64u : 16u;
  r.gc = r.A < r.gw ? r.A : r.gw;
  unsigned p2 = 1;
  while (p2 * 2u <= r.gc) p2 *= 2u;
  r.gc = p2;
  while (r.A % r.gc) r.gc >>= 1;  // (A is a power of two for every geometry that gets here; defensive)
  r.row_waves = cdiv_u(r.A, 64u / r.gw);
  r.col_waves = cdiv_u(RED2_COLS, 64u / r.gc);
  return r;
}
struct TailPlan {
  TailForm form;
  bool quad;        // a quad of lanes per logical lane (ec.h: xyzz_add_quad) in every kernel of the tail
  bool latency;     // RED2: the strip shape (red2_geom)
  unsigned red_s, red_threads;  // running sums: buckets per logical lane, logical lanes per set
  unsigned partials;  // partial records per set that the reduction leaves in the slot's red_out
  size_t rc_records;  // RED2: records of row / column scratch (all sets), else 0
  bool ticket;        // FUSED_QUAD: one zeroed arrival counter per set
};
// nb buckets in each of n_sets sets (B in all), E sorted entries; bpl: the bucket-per-lane accumulation filled the buckets
inline TailPlan tail_plan(unsigned nb, unsigned n_sets, unsigned B, unsigned E, bool bpl, Place place) {
  TailPlan t{};
  // exposed: nothing is queued behind this MSM, so the caller waits for its tail (bucket reduce + fold, a chain of dependent point
  // operations on a few waves): run it on the quad-cooperative kernels (-0.08 ms).  Inside a batch the tail is hidden behind the
  // next MSM's accumulation and the one-lane kernels cost less ALU time (measured: 1 % of the batch throughput).
  const bool exposed = place != Place::BATCH_INNER;
  // Round 4: a HIDDEN tail (inside a batch) also takes the quad kernels when the bucket table is small.  The tails of
  // consecutive MSMs queue on one stream, and the one-lane kernels are latency chains whatever the bucket count -- accumulate
  // L1 80 + reduce 240 + fold 120 us for the 2^15 buckets of a 2^18-pair MSM whose accumulation takes 300 us (rocprofv3, round
  // 4): the batch ran at one MSM per tail (0.46 ms at 2^18, 0.71 at 2^19).  The quad kernels cost four times the lanes of
  // almost nothing there and halve the chain; from 2^18 buckets up the one-lane kernels' lower ALU cost wins (2^20 pairs).
  // (... and only while the accumulation is shorter than the tail chain: up to 2^18 pairs of 16 entries -- at 2^19 the batch
  // is bound by the accumulation's work and the quad kernels' extra lanes cost 2-6 %; measured, same box, M pairs/s in batches:
  // 2^16 234 -> 283, 2^17 395 -> 451, 2^18 582 -> 617, 2^19 754 -> 741; BLS12-381 2^18 207 -> 297, 2^19 352 -> 332)
  const bool small_table = B <= (1u << TAIL_QUAD_HIDDEN_LOG2) && E <= (5u << 20);
  t.quad = exposed || small_table;
  t.latency = t.quad;
  // buckets per lane of the running sums: 4; 8 for the 2^16-bucket sets of 17-bit windows (half the 16-bit small
  // multiples, the reduction's largest ALU item; batches 821 -> 826 M pairs/s at 2^20, 845 -> 853 at 2^22; 2 and 16 do not pay)
  // round 6: 2 for the 128-bucket sets of 8-bit windows (plain keys up to 2^17 pairs: the rounds of a large IPA opening over its
  // folded key, 64 sets of 128 buckets) -- a set is one workgroup either way, and its chain is the leaf's additions + a 7-bit multiple
  // + the tree: 3 additions instead of 7 at the leaf
  // bucket-per-lane: the reduction is hidden behind the next MSM's accumulation or exposed on few waves either way: long per-lane runs
  // keep its small multiples (one per lane) rare -- 2^19 buckets / 32 = 16 384 lanes (measured: 16 / 32 / 64 -> 911 / 955 / 895 M
  // pairs/s in batches, 0.45 / 0.37 / 0.52 ms exposed)
  t.red_s = bpl ? 32u : (nb >= 65536u ? 8u : (nb <= 256u ? 2u : 4u));
  if (t.red_s > nb) t.red_s = nb;
  t.red_threads = nb / t.red_s;
  const unsigned lanes = t.quad ? 4u : 1u;  // hardware lanes per logical lane
  // round 4: bucket sets of 2^18 buckets and more reduce as row / column sums.  Measured, same box, batches / blocking call: 2^20
  // pairs over the 20-bit key 908 -> 928 M pairs/s, 1.409 -> 1.381 ms; smaller sets LOSE (2^15 buckets: 2^16 pairs 280 -> 212,
  // 2^19 pairs 717 -> 598; a plain key's 16 sets of 2^15: 794 -> 731): with few rows the column sums are all butterfly, and
  // 1024 + A small multiples cost more than the per-lane ones of a short running-sum kernel
  if (nb >= RED2_MIN_NB && nb % RED2_COLS == 0u) {
    const unsigned items = nb / RED2_COLS + RED2_COLS;  // one logical lane per row or column sum
    t.form = RED2;
    t.partials = cdiv_u(items * lanes, 256);
    t.rc_records = (size_t)n_sets * items;
    return t;
  }
  // round 6: the quad reduction and its fold as ONE launch (profiles/r06_fused_fold_ab.txt: equal or ahead of the two launches everywhere)
  t.form = t.quad ? FUSED_QUAD : ONE_LANE;
  t.partials = cdiv_u(t.red_threads * lanes, 256);
  t.ticket = t.quad;
  return t;
}
// What a slot must hold for the MSM wherever it stands in its call: msm_plan reserves before the Place is known (a caller with side
// effects reserves first), msm_enqueue decides.  The form-independent fields are LONE's.
inline TailPlan tail_plan_any_place(unsigned nb, unsigned n_sets, unsigned B, unsigned E, bool bpl) {
  TailPlan w = tail_plan(nb, n_sets, B, E, bpl, Place::LONE);
  for (Place p : {Place::BATCH_LAST, Place::BATCH_INNER}) {
    const TailPlan t = tail_plan(nb, n_sets, B, E, bpl, p);
    if (t.partials > w.partials) w.partials = t.partials;
    if (t.rc_records > w.rc_records) w.rc_records = t.rc_records;
    w.ticket = w.ticket || t.ticket;
  }
  return w;
}

}  // namespace msel
}  // namespace amsm
