// Prints what accumulation_amd/csrc/msm_jobs.h makes of a call at every rule edge of the job list (plain C++: no HIP, no library) --
// tests/test_msm_jobs_cpu.py compares the output with tests/golden/msm_jobs.txt.  One line per case:
//   ranges <case> twin=<needs the twin> n=<ranges> sets=<shared sets> r<i>=<vec>,<lo>,<n>,<over_twin>,<force_chunked>,<set>,<first>,<last>,<B> ...
//   halves <case> h1=<first half> B=<bpl_geom's buckets for it>          (behind the ranges line of a host slice in two halves)
//   units <case> n=<units> slot_bytes=<of job 0> u<i>=<first>,<count> ... j<i>=<geometry found>,<over the twin> ...
//   probe <case> verdict=<0|1> loads=<scalars looked at>
//   tv <case> looks=<0|1> | ones <case> has=<0|1> | identical <case> first=<..>,<..>
// What every plan must satisfy is asserted here (exit status 1 and a line on stderr): the ranges of a vector tile it in order, a
// shared set is a run of ranges of one vector with one first and one last, the units cover the live jobs in order, exactly once.
#include <cstdio>
#include <string>
#include <vector>

#include "../../accumulation_amd/csrc/msm_jobs.h"

using namespace amsm;
using namespace amsm::mjobs;

static const u32 PALLAS_R[8] = {0x00000001u, 0x8c46eb21u, 0x0994a8ddu, 0x224698fcu, 0x00000000u, 0x00000000u, 0x00000000u, 0x40000000u};

static int bad = 0;
#define EXPECT(cond, name)                                             \
  do {                                                                 \
    if (!(cond)) {                                                     \
      fprintf(stderr, "%s: %s does not hold\n", name.c_str(), #cond); \
      bad = 1;                                                         \
    }                                                                  \
  } while (0)

constexpr size_t P(int k) { return (size_t)1 << k; }

static PlanCtx ctx_of() {
  PlanCtx c;
  for (int i = 0; i < 8; i++) c.geom.r_mod[i] = PALLAS_R[i];
  return c;
}
static void fill_key(size_t n, int c, bool bpl, msel::KeyDesc* d, GeomKey* g) {
  d->n = n;
  d->precomputed = c != 0;
  d->bpl = bpl;
  d->direct_table = false;
  d->c = c;
  g->n = n;
  g->precomp = c != 0;
  if (c) {
    g->c = c;
    g->W = windows_for(c);
    if (bpl) {
      g->n_narrow = (int)narrow_windows_for((u32)c);
      g->top_shift = top_window_shift_of(PALLAS_R, c, g->W, g->n_narrow);
    }
  }
}
// a key of n generators with a table of c-bit windows (0: plain), as bases_finish builds it; a 20-bit key may carry its 17-bit twin
static JobKey key_of(size_t n, int c, bool twin = false) {
  static int ids[16];
  static int next = 0;
  JobKey k;
  k.id = &ids[next++ % 16];
  fill_key(n, c, c == 20, &k.desc, &k.geom);
  k.has_twin = twin;
  if (twin) fill_key(n, 17, false, &k.twin_desc, &k.twin_geom);
  return k;
}
static PlanVec vec(size_t off, size_t n, bool skew = false) {
  PlanVec v;
  v.off = off;
  v.n = n;
  v.skew = skew;
  return v;
}

static std::vector<Range> ranges_case(const std::string& name, const PlanCtx& ctx, const JobKey& key, const std::vector<PlanVec>& vecs, const Form& form,
                                      bool keeps_empty) {
  std::vector<Range> r;
  const bool twin = needs_twin(key, vecs.data(), vecs.size());
  EXPECT(!twin || key.has_twin, name);  // (the callers build it first)
  plan_ranges(ctx, key, vecs.data(), vecs.size(), form, &r);
  int sets = 0;
  for (const Range& x : r) sets = std::max(sets, x.set + 1);
  printf("ranges %s twin=%d n=%zu sets=%d", name.c_str(), twin ? 1 : 0, r.size(), sets);
  for (size_t i = 0; i < r.size(); i++)
    printf(" r%zu=%zu,%zu,%zu,%d,%d,%d,%d,%d,%u", i, r[i].vec, r[i].lo, r[i].n, r[i].over_twin, r[i].force_chunked, r[i].set, r[i].first, r[i].last,
           r[i].set_buckets);
  printf("\n");
  // the ranges of a vector tile it, in order; vectors in order
  size_t at = 0;
  for (size_t v = 0; v < vecs.size(); v++) {
    size_t lo = 0, count = 0;
    while (at < r.size() && r[at].vec == v) {
      EXPECT(r[at].lo == lo && (r[at].n > 0 || vecs[v].n == 0), name);
      lo += r[at].n;
      at++;
      count++;
    }
    EXPECT(lo == vecs[v].n, name);
    EXPECT(count >= 1 || (vecs[v].n == 0 && !keeps_empty), name);
    EXPECT(count <= 1 || vecs[v].n > 0, name);
  }
  EXPECT(at == r.size(), name);
  // a set: consecutive ranges of one vector, at least two, the first one first, the last one last, one bucket count, numbered in order
  int next_set = 0;
  for (size_t i = 0; i < r.size(); i++) {
    if (r[i].set < 0) {
      EXPECT(!r[i].first && !r[i].last && r[i].set_buckets == 0u, name);
      continue;
    }
    const bool opens = i == 0 || r[i - 1].set != r[i].set, closes = i + 1 == r.size() || r[i + 1].set != r[i].set;
    EXPECT(r[i].first == opens && r[i].last == closes && !(opens && closes), name);
    EXPECT(!opens || r[i].set == next_set, name);
    if (opens) next_set++;
    EXPECT(opens || (r[i - 1].vec == r[i].vec && r[i - 1].set_buckets == r[i].set_buckets), name);
    EXPECT(r[i].set_buckets > 0u && !r[i].over_twin && !r[i].force_chunked, name);
  }
  return r;
}
// a host slice that must run in two halves: their sizes, and one set of bpl_geom's buckets
static void halves_case(const std::string& name, const PlanCtx& ctx, const JobKey& key, const PlanVec& v, const std::vector<Range>& r) {
  MsmGeom hg = {};
  const size_t h1 = first_half(v.n);
  const bool ok = bpl_geom(ctx.geom, key.geom, v.off, h1, -1, 0, &hg);
  printf("halves %s h1=%zu B=%u\n", name.c_str(), h1, hg.B);
  EXPECT(ok && h1 % 64 == 0 && h1 >= v.n - h1 && h1 - (v.n - h1) < 128, name);
  EXPECT(r.size() == 2 && r[0].n == h1 && r[1].lo == h1 && r[1].n == v.n - h1, name);
  EXPECT(r.size() == 2 && r[0].set == 0 && r[1].set == 0 && r[0].first && r[1].last && r[0].set_buckets == hg.B && r[1].set_buckets == hg.B, name);
}

static UnitJob ujob(size_t key, size_t off, size_t n, int mont = 0) {
  UnitJob j;
  j.key = key;
  j.off = off;
  j.n = n;
  j.mont = mont;
  return j;
}
static void units_case(const std::string& name, const PlanCtx& ctx, const std::vector<JobKey>& keys, const std::vector<UnitJob>& jobs, size_t rec_bytes) {
  std::vector<msel::Unit> units(jobs.size());
  std::vector<UnitGeom> ug(jobs.size());
  const size_t n = plan_units(ctx, keys.data(), jobs.data(), jobs.size(), rec_bytes, units.data(), ug.data());
  printf("units %s n=%zu slot_bytes=%zu", name.c_str(), n, ug[0].g.bpl == 2u ? bps_slot_bytes(ug[0].g, rec_bytes) : (size_t)0);
  for (size_t u = 0; u < n; u++) printf(" u%zu=%zu,%zu", u, units[u].first, units[u].count);
  for (size_t i = 0; i < jobs.size(); i++) printf(" j%zu=%d,%d", i, ug[i].g.bpl == 2u ? 1 : 0, ug[i].over_twin ? 1 : 0);
  printf("\n");
  size_t at = 0;  // the units cover the live jobs in order, exactly once; a unit of several has a geometry, and one key for all
  for (size_t u = 0; u < n; u++) {
    EXPECT(units[u].first == at && units[u].count >= 1 && units[u].count <= (size_t)msel::BPS_BATCH, name);
    if (units[u].count > 1) {
      EXPECT(ug[at].g.bpl == 2u && ug[at].g.n_sets == 1u && ug[at].g.n == jobs[at].n, name);
      for (size_t v = 1; v < units[u].count; v++)
        EXPECT(jobs[at + v].key == jobs[at].key && jobs[at + v].off == jobs[at].off && jobs[at + v].n == jobs[at].n && ug[at + v].g.bpl == 2u, name);
    }
    at += units[u].count;
  }
  EXPECT(at == jobs.size(), name);
}

// a fixed generator of scalars below 2^254 (xorshift64*)
struct Gen {
  unsigned long long s = 0x9e3779b97f4a7c15ull;
  u32 next() {
    s ^= s >> 12;
    s ^= s << 25;
    s ^= s >> 27;
    return (u32)((s * 0x2545f4914f6cdd1dull) >> 32);
  }
};
static void probe_case(const std::string& name, const std::vector<u32>& words, size_t n, size_t min_len, const DigitWalk& dw) {
  size_t loads = 0;
  const bool v = skew_probe_host(n, min_len, dw, [&](size_t i, u32* out) {
    loads++;
    memcpy(out, &words[i * 8], 32);
  });
  printf("probe %s verdict=%d loads=%zu\n", name.c_str(), v ? 1 : 0, loads);
  EXPECT(loads == (n < min_len ? 0u : (size_t)PROBE_SAMPLES), name);
}

int main() {
  const PlanCtx ctx = ctx_of();
  const JobKey k20 = key_of(P(23), 20, true), k17 = key_of(P(23), 17), plain = key_of(P(21), 0);
  const Form dev = device_form();
  auto one = [](size_t n, bool skew = false) { return std::vector<PlanVec>{vec(0, n, skew)}; };
  auto sized = [](size_t n) -> std::string {
    for (int k = 4; k < 40; k++)
      for (long d : {-1L, 0L, 1L})
        if (n == P(k) + (size_t)d) return "2p" + std::to_string(k) + (d < 0 ? "_minus_1" : d > 0 ? "_plus_1" : "");
    return std::to_string(n);
  };

  // ---- 20-bit key, device vectors: ranges of 2^20, the leading bucket-per-lane ranges in one set ----
  for (size_t n : {P(20), P(20) + 1, P(21), P(21) + P(18), P(21) + P(18) + 1, P(22)}) {
    const std::string tag = n == P(21) + P(18) ? "2p21_plus_2p18" : n == P(21) + P(18) + 1 ? "2p21_plus_2p18_plus_1" : sized(n);
    ranges_case("dev20_n_" + tag, ctx, k20, one(n), dev, true);
  }
  ranges_case("dev20_n_2p20_plus_2p18_only_first_bpl", ctx, k20, one(P(20) + P(18)), dev, true);
  ranges_case("dev20_n_2p22_off_2p20", ctx, k20, {vec(P(20), P(22))}, dev, true);
  {
    PlanCtx c = ctx;
    c.share_buckets = false;
    ranges_case("dev20_n_2p22_share_off", c, k20, one(P(22)), dev, true);
    c = ctx;
    c.sw.bpl = false;
    ranges_case("dev20_n_2p22_bpl_off", c, k20, one(P(22)), dev, true);
  }
  // skewed: over the twin, cut by the twin's rule
  ranges_case("dev20_skew_n_2p20_plus_1", ctx, k20, one(P(20) + 1, true), dev, true);
  ranges_case("dev20_skew_n_2p22_minus_1", ctx, k20, one(P(22) - 1, true), dev, true);
  ranges_case("dev20_skew_n_2p22", ctx, k20, one(P(22), true), dev, true);
  for (int sl : {0, 20}) {
    PlanCtx c = ctx;
    c.sw.split_log2 = sl;
    ranges_case("dev20_skew_n_2p22_split_log2_" + std::to_string(sl), c, k20, one(P(22), true), dev, true);
  }
  ranges_case("dev20_skew_and_not", ctx, k20, {vec(0, P(21) + 1, true), vec(0, P(21) + 1, false)}, dev, true);
  ranges_case("dev20_two_sets", ctx, k20, {vec(0, P(21)), vec(P(21), P(21) + 1)}, dev, true);

  // ---- 17-bit precomputed key: ranges of 2^split_log2 from 2^22 pairs; the skew verdicts of a call with a vector that splits ----
  ranges_case("dev17_n_2p22_minus_1", ctx, k17, one(P(22) - 1), dev, true);
  ranges_case("dev17_n_2p22", ctx, k17, one(P(22)), dev, true);
  for (bool host : {false, true}) {
    const std::string f = host ? "host17" : "dev17";
    const Form form = host ? host_form(2, false, 0, false) : dev;
    ranges_case(f + "_skew_alone", ctx, k17, {vec(0, P(17), true), vec(0, P(17), false)}, form, !host);
    ranges_case(f + "_skew_beside_a_split", ctx, k17, {vec(0, P(17), true), vec(0, P(22), false)}, form, !host);
    ranges_case(f + "_skew_is_the_split", ctx, k17, {vec(0, P(22), true)}, host ? host_form(1, false, 0, false) : dev, !host);
  }

  // ---- plain key: ranges of 2^20 where plain keys take the bucket-per-lane pipeline ----
  for (size_t n : {P(20), P(20) + 1}) {
    ranges_case("devplain_n_" + sized(n), ctx, plain, one(n), dev, true);
    PlanCtx c = ctx;
    c.sw.bpl_plain = false;
    ranges_case("devplain_n_" + sized(n) + "_bpl_plain_off", c, plain, one(n), dev, true);
    c = ctx;
    c.sw.window_override = true;
    c.geom.window_override = 12;
    ranges_case("devplain_n_" + sized(n) + "_window_override", c, plain, one(n), dev, true);
    ranges_case("hostplain_n_" + sized(n), ctx, plain, one(n), host_form(1, false, 0, false), false);
  }

  // ---- empty vectors ----
  ranges_case("dev20_empty", ctx, k20, {vec(5, 0)}, dev, true);
  ranges_case("dev20_empty_at_the_key_s_end", ctx, k20, {vec(P(23), 0)}, dev, true);
  ranges_case("dev17_empty_between", ctx, k17, {vec(0, P(16)), vec(7, 0), vec(0, P(16))}, dev, true);
  ranges_case("host20_empty", ctx, k20, {vec(5, 0)}, host_form(1, false, 0, false), false);
  ranges_case("host20_empty_at_the_key_s_end", ctx, k20, {vec(P(23), 0)}, host_form(1, false, 0, false), false);
  ranges_case("host17_empty_between", ctx, k17, {vec(0, P(16)), vec(7, 0), vec(0, P(16))}, host_form(3, false, 0, false), false);

  // ---- host slices: the lone slice in two halves, the one-shot step ----
  for (size_t n : {3 * P(18) - 1, 3 * P(18), 3 * P(18) + 1, P(20), P(20) + 1}) {
    const std::string tag = n == 3 * P(18) - 1 ? "3x2p18_minus_1" : n == 3 * P(18) ? "3x2p18" : n == 3 * P(18) + 1 ? "3x2p18_plus_1" : sized(n);
    const std::vector<Range> r = ranges_case("host20_n_" + tag, ctx, k20, {vec(64, n)}, host_form(1, false, 0, false), false);
    if (n >= 3 * P(18) && n <= P(20)) halves_case("host20_n_" + tag, ctx, k20, vec(64, n), r);
    ranges_case("host20_n_" + tag + "_k2", ctx, k20, {vec(64, n), vec(64, n)}, host_form(2, false, 0, false), false);
    ranges_case("host20_n_" + tag + "_no_halves", ctx, k20, {vec(64, n)}, host_form(1, false, 0, true), false);
    ranges_case("host20_n_" + tag + "_skew", ctx, k20, {vec(64, n, true)}, host_form(1, false, 0, false), false);
    ranges_case("host20_n_" + tag + "_oneshot_step_2p19", ctx, k20, {vec(64, n)}, host_form(1, true, P(19), false), false);
    ranges_case("host20_n_" + tag + "_oneshot_no_step", ctx, k20, {vec(64, n)}, host_form(1, true, 0, false), false);
    PlanCtx c = ctx;
    c.host_halves = false;
    ranges_case("host20_n_" + tag + "_host_halves_off", c, k20, {vec(64, n)}, host_form(1, false, 0, false), false);
    c = ctx;
    c.share_buckets = false;
    ranges_case("host20_n_" + tag + "_share_off", c, k20, {vec(64, n)}, host_form(1, false, 0, false), false);
  }
  ranges_case("host17_n_2p20_no_halves_without_a_20_bit_table", ctx, k17, {vec(0, P(20))}, host_form(1, false, 0, false), false);
  // (a long host slice is cut like a device vector, but its ranges stay MSMs of their own)
  ranges_case("host20_n_2p22", ctx, k20, one(P(22)), host_form(1, false, 0, false), false);
  for (size_t n : {(size_t)1, P(18), P(18) + 1})
    ranges_case("hostplain_oneshot_step_2p18_n_" + sized(n), ctx, plain, one(n), host_form(1, true, P(18), false), false);

  // ---- the units of bucket-split MSMs ----
  {
    const std::vector<JobKey> keys = {key_of(P(17), 17), key_of(P(20), 20, true), key_of(P(20), 20, false)};
    const size_t rec = 4 * 8 * 4;  // (Pallas: four coordinates of eight words)
    const UnitJob a = ujob(0, 0, P(16));
    for (size_t run : {1, 2, 8, 9, 17}) units_case("run_of_" + std::to_string(run), ctx, keys, std::vector<UnitJob>(run, a), rec);
    // a job that never joins a unit between equal jobs: nothing is inherited across it
    UnitJob skewed = a, grouped = a, shared = a;
    skewed.force_chunked = true;
    grouped.group_shift = 0;
    shared.shared = true;
    units_case("skewed_between", ctx, keys, {a, skewed, a, a}, rec);
    units_case("grouped_between", ctx, keys, {a, grouped, a, a}, rec);
    units_case("shared_between", ctx, keys, {a, shared, a, a}, rec);
    units_case("skewed_first", ctx, keys, {skewed, a, a}, rec);
    UnitJob off = a, mont = a, ones = a;
    off.off = 64;
    mont.mont = 1;
    ones.skip_ones = true;
    units_case("differ_in_off", ctx, keys, {a, off, off, a}, rec);
    units_case("differ_in_mont", ctx, keys, {a, mont}, rec);
    units_case("differ_in_skip_ones", ctx, keys, {a, ones}, rec);
    units_case("differ_in_key", ctx, keys, {a, ujob(1, 0, P(16)), ujob(1, 0, P(16))}, rec);
    units_case("not_bucket_split_2p15", ctx, keys, {ujob(0, 0, P(15)), ujob(0, 0, P(15))}, rec);
    for (int b : {0, 1, 2}) {
      PlanCtx c = ctx;
      c.sw.bps_batch = b;
      units_case("bps_batch_" + std::to_string(b), c, keys, std::vector<UnitJob>(5, a), rec);
    }
    units_case("slot_bytes_cap", ctx, keys, std::vector<UnitJob>(8, a), 1500);  // (a record so wide that eight MSMs pass 512 MiB)
    units_case("twin_present", ctx, keys, std::vector<UnitJob>(3, ujob(1, 0, P(16))), rec);
    units_case("twin_absent", ctx, keys, std::vector<UnitJob>(3, ujob(2, 0, P(16))), rec);
  }

  // ---- the probes ----
  {
    const size_t n = P(16);
    const JobKey k = key_of(P(17), 17);
    const DigitWalk dw = key_walk(k.geom);
    EXPECT(dw.c == 17u && dw.W == 16u && dw.n_narrow == 0u && dw.skip_ones == 0u, std::string("key_walk"));
    EXPECT(key_walk(k20.geom).c == 20u && key_walk(k20.geom).W == 13u && key_walk(k20.geom).n_narrow == 4u, std::string("key_walk"));
    const size_t min_len = probe_min_len(k.desc);
    printf("probe_min_len table17=%zu table20=%zu\n", min_len, probe_min_len(k20.desc));
    Gen gen;
    std::vector<u32> uniform(P(19) * 8), constant(n * 8);
    for (size_t i = 0; i < P(19); i++) {
      for (int w = 0; w < 8; w++) uniform[i * 8 + w] = gen.next();
      uniform[i * 8 + 7] &= 0x3fffffffu;  // below 2^254
    }
    for (size_t i = 0; i < n * 8; i++) constant[i] = uniform[i % 8];
    probe_case("uniform_below_2p254", uniform, n, min_len, dw);
    probe_case("constant", constant, n, min_len, dw);
    probe_case("uniform_over_the_20_bit_walk", uniform, P(19), probe_min_len(k20.desc), key_walk(k20.geom));
    probe_case("constant_n_min_len_minus_1", constant, min_len - 1, min_len, dw);
    probe_case("constant_n_min_len", constant, min_len, min_len, dw);
    // exactly 23 / 24 samples share one digit of window 0, every other sample has a digit and a bin of its own
    for (u32 same : {PROBE_LIMIT - 1, PROBE_LIMIT}) {
      std::vector<u32> words(n * 8, 0u);
      std::vector<unsigned char> used(PROBE_BINS, 0);
      u32 d = 1;
      used[probe_bin(d)] = 1;
      for (u32 t = 0; t < PROBE_SAMPLES; t++) {
        u32 mine = 1;
        if (t >= same) {
          do d++;
          while (used[probe_bin(d)]);
          used[probe_bin(d)] = 1;
          mine = d;
        }
        words[(size_t)probe_sample(t, n) * 8] = mine;
      }
      EXPECT(d < (1u << 16), std::string("limit edge"));
      probe_case("samples_sharing_a_digit_" + std::to_string(same), words, n, min_len, dw);
    }
    EXPECT(probe_sample(0, n) == 0 && probe_sample(PROBE_SAMPLES - 1, n) == n - n / PROBE_SAMPLES && probe_sample(1, P(33)) == P(23), std::string("probe_sample"));
    printf("probe_wanted table17_n_2p16=%d table17_n_2p15=%d table20_n_2p19=%d plain_n_2p20=%d empty=%d\n", probe_wanted(ctx, k.desc, P(16)),
           probe_wanted(ctx, k.desc, P(15)), probe_wanted(ctx, k20.desc, P(19)), probe_wanted(ctx, plain.desc, P(20)), probe_wanted(ctx, k.desc, 0));

    // two-valued / unit scalars: the same samples
    std::vector<uint64_t> s(n * 4, 0);
    printf("tv distinct_0 looks=%d\n", looks_two_valued(s.data(), n));
    for (u32 t = 0; t < PROBE_SAMPLES; t += 3) s[(size_t)probe_sample(t, n) * 4 + 1] = 77;
    printf("tv distinct_1 looks=%d\n", looks_two_valued(s.data(), n));
    s[(size_t)probe_sample(PROBE_SAMPLES - 1, n) * 4 + 1] = 78;
    printf("tv distinct_2 looks=%d\n", looks_two_valued(s.data(), n));
    s[(size_t)probe_sample(PROBE_SAMPLES - 1, n) * 4 + 1] = 0;
    s[(size_t)probe_sample(PROBE_SAMPLES - 1, n) * 4 + 5] = 78;  // (between the samples: not seen)
    printf("tv distinct_2_between_samples looks=%d\n", looks_two_valued(s.data(), n));
    const u32 unit[8] = {1u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    for (u32 cnt : {TV_ONES_MIN_SAMPLES - 1, TV_ONES_MIN_SAMPLES}) {
      std::vector<uint64_t> o(n * 4, 5);
      for (u32 t = 0; t < cnt; t++) {
        uint64_t* e = &o[(size_t)probe_sample(100 * t, n) * 4];
        e[0] = 1;
        e[1] = e[2] = e[3] = 0;
      }
      printf("ones samples_%u has=%d\n", cnt, has_unit_scalars(o.data(), n, unit));
    }

    // identical vectors: the pointer AND the length; a chain resolves to its first
    const int x = 0, y = 0;
    const std::vector<VecRef> refs = {{&x, 10}, {&y, 10}, {&x, 10}, {&x, 11}, {&x, 10}, {&x, 11}};
    std::vector<size_t> first(refs.size());
    first_identical(refs.size(), [&](size_t j) { return refs[j]; }, first.data());
    printf("identical chain first=");
    for (size_t j = 0; j < first.size(); j++) printf("%s%zu", j ? "," : "", first[j]);
    printf("\n");
  }
  return bad;
}
