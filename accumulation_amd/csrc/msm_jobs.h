// The job list of a call as pure host arithmetic: how the vectors of a call are cut into ranges of the key (plan_ranges), which
// ranges share one bucket set, which consecutive bucket-split MSMs run as one unit (plan_units), and what the host's sampling looks
// (the skew probe, "looks two-valued", "has unit scalars", identical vectors) make of a vector.  No HIP, no amsm_ctx, no amsm_bases,
// no pointer into device memory: api_pipeline.inc hands in plain records (plan_ctx / job_key), materialises MsmJobs from the plan and
// keeps what touches HIP -- bases_alt, the shared sets' buffers and events, the staging ring, the probe launches, run_ring.
// tests/cpp_host/msm_jobs_check.cpp prints the plans at every rule edge without a GPU (tests/test_msm_jobs_cpu.py).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstring>
#include <vector>

#include "msm_geom.h"
#include "msm_select.h"
#include "msm_types.h"

namespace amsm {
namespace mjobs {

// A key as the planner sees it; the 17-bit twin of a 20-bit key is optional: absent = not built, or not to be had
struct JobKey {
  const void* id = nullptr;  // identity (what msel::BatchJob::key compares)
  msel::KeyDesc desc = {};
  GeomKey geom;
  bool has_twin = false;
  msel::KeyDesc twin_desc = {};
  GeomKey twin_geom;
};
// The context as the planner sees it
struct PlanCtx {
  msel::Switches sw;
  GeomCtx geom;
  bool share_buckets = true;  // AMSM_SHARE_BUCKETS
  bool host_halves = true;    // AMSM_HOST_HALVES
  bool bpl_probe = true;      // AMSM_BPL_PROBE: the skew probes run at all
};
// A vector of the call: generators [off, off + n) of the key (n clamped to it), and the skew probe's verdict on its scalars
struct PlanVec {
  size_t off = 0, n = 0;
  bool skew = false;
};
// One range of a vector = one job of the slot ring
struct Range {
  size_t vec = 0;      // the owner: its place among the call's vectors
  size_t lo = 0, n = 0;  // pairs [lo, lo + n) of the vector: generators from off + lo, scalars from lo
  bool over_twin = false;      // a skewed vector over a 20-bit key: chunked over the twin
  bool force_chunked = false;  // a skewed vector over any other precomputed key: chunked over the key itself
  int set = -1;                // >= 0: one range of a shared bucket set (api_types.h: struct Share), numbered within the call
  bool first = false, last = false;  // ... the range that writes the set / the one that carries its tail
  u32 set_buckets = 0;               // ... and the set's bucket count (MsmGeom::B)
};

// ---- the cut -------------------------------------------------------------------------------------------------------------------------
// Large MSMs run as ranges of the key (msm_select.h: range_of)
inline bool split_needed(const msel::Switches& sw, const msel::KeyDesc& key, size_t n) { return msel::range_of(key, n, sw) != 0; }
inline size_t split_chunk(const msel::Switches& sw, const msel::KeyDesc& key) {
  const size_t r = msel::range_of(key, ~(size_t)0 >> 1, sw);
  return r ? r : ((size_t)1 << 20);
}
// A LONE host slice of [3 x 2^18, 2^20] pairs over a 20-bit key (one blocking `commit(&ck, &[Fr], ..)` at a time) used to be upload
// (0.6 ms) + MSM (1.4 ms) in series by construction.  It runs as TWO ranges over ONE bucket set: the second half crosses the link
// while the first half is sorted and accumulated.  (measured at 2^20: 2.03 -> 1.90 ms; thinner halves fill the 2^19 buckets too thinly)
inline bool halves_apply(const PlanCtx& ctx, const msel::KeyDesc& key, size_t len) {
  return ctx.host_halves && ctx.share_buckets && ctx.sw.bpl && key.bpl && key.precomputed && len >= ((size_t)3 << 18) && len <= ((size_t)1 << 20);
}
inline size_t first_half(size_t len) { return ((len + 1) / 2 + 63) & ~(size_t)63; }

// What distinguishes the job list of device vectors (msm_multi_split_impl) from that of host slices (msm_multi_host_xyzz).  This
// block states the differences; it does not settle them: where no reason is known the comment says so, and the behaviour stays.
struct Form {
  // A call with a vector that is cut anyway forgets EVERY skew verdict over a key without a 20-bit table ("longer than 2^21: ranges
  // of the key, chunked anyway" -- true of the vector that splits; why the short vectors beside it lose theirs is not known: they
  // then find out from their prep's overflow flag).  Device vectors only; host slices keep their verdicts one by one.
  bool any_split_clears_skew = false;
  // An empty vector stays ONE empty job (the device form: a batch with one is then no batch of direct sums, msm_multi_xyzz, and
  // the ring skips it) or is dropped (the host form: there is nothing to upload, and its staging ring counts jobs).
  bool keep_empty = false;
  // The leading bucket-per-lane ranges of a vector that is cut share ONE bucket set (api_types.h: struct Share).  Device vectors
  // only.  No reason is written down for host slices; a supposed one: a set whose range overflows is re-run from all its ranges'
  // scalars, and the staging ring keeps only the last few.
  bool share_split_ranges = false;
  // amsm_msm_oneshot: the generators cross the link with the scalars, range by range, so the call names its own range (0: none)
  size_t step = 0;
  // the lone slice in two halves over one set (halves_apply).  Off for a call of several slices (their uploads overlap with each
  // other's MSMs already), for a one-shot call (it has its step), and for the re-run of a call one of whose halves met skewed digits
  bool halves = false;
};
inline Form device_form() {
  Form f;
  f.any_split_clears_skew = f.keep_empty = f.share_split_ranges = true;
  return f;
}
inline Form host_form(size_t k, bool oneshot, size_t oneshot_step, bool no_halves) {
  Form f;
  f.step = oneshot ? oneshot_step : 0;
  f.halves = !no_halves && !oneshot && k == 1;
  return f;
}

// Does the call need the twin of its 20-bit key?  (a skewed vector: answerable before the twin is built)
inline bool needs_twin(const JobKey& key, const PlanVec* vecs, size_t k) {
  if (!key.desc.bpl) return false;
  for (size_t v = 0; v < k; v++)
    if (vecs[v].skew) return true;
  return false;
}

// The job list of a call: every vector in ranges of `step` pairs (an empty vector: one empty range, or none), in the vectors' order.
// A skewed vector over a 20-bit key runs chunked over the twin (key.has_twin: needs_twin said so) and is cut by ITS rule; over any
// other precomputed key it runs chunked over the key itself.
inline void plan_ranges(const PlanCtx& ctx, const JobKey& key, const PlanVec* vecs, size_t k, const Form& form, std::vector<Range>* out) {
  out->clear();
  bool forget_skew = false;
  if (form.any_split_clears_skew && !key.desc.bpl)
    for (size_t v = 0; v < k; v++) forget_skew = forget_skew || split_needed(ctx.sw, key.desc, vecs[v].n);
  int n_sets = 0;
  for (size_t v = 0; v < k; v++) {
    const size_t len = vecs[v].n;
    if (!len && !form.keep_empty) continue;
    const bool skew = vecs[v].skew && !forget_skew;
    Range r;
    r.vec = v;
    r.over_twin = skew && key.desc.bpl;
    r.force_chunked = skew && !key.desc.bpl;
    const msel::KeyDesc& kd = r.over_twin ? key.twin_desc : key.desc;
    const GeomKey& kg = r.over_twin ? key.twin_geom : key.geom;
    auto bpl_range = [&](size_t lo, size_t n, MsmGeom* g) {  // does the range take the bucket-per-lane pipeline, over one set?
      return msel::choose(kd, n, false, false, false, ctx.sw).pipeline == msel::BUCKET_PER_LANE &&
             bpl_geom(ctx.geom, kg, vecs[v].off + lo, n, -1, 0, g) && g->n_sets == 1u;
    };
    const bool split = split_needed(ctx.sw, kd, len);
    size_t step = form.step ? form.step : (split ? split_chunk(ctx.sw, kd) : std::max<size_t>(len, 1));
    MsmGeom g;
    const size_t h1 = first_half(len);
    // (both halves must choose the bucket-per-lane pipeline; the geometry asked for is the first half's, the larger one)
    // (a skewed slice never: over the twin or chunked over a key without a 20-bit table, halves_apply is false)
    const bool halve = form.halves && !split && halves_apply(ctx, kd, len) &&
                       msel::choose(kd, len - h1, false, false, false, ctx.sw).pipeline == msel::BUCKET_PER_LANE && bpl_range(0, h1, &g);
    if (halve) step = h1;
    const size_t first = out->size();
    size_t lo = 0;
    do {
      r.lo = lo;
      r.n = std::min(step, len - lo);
      out->push_back(r);
      lo += step;
    } while (lo < len);
    const size_t count = out->size() - first;
    // the set: both halves; or every leading range that takes the bucket-per-lane pipeline -- a short last range (below a quarter
    // of the window: the twin's pipelines) stays an MSM of its own, and one range alone is no set
    size_t n_sh = halve ? count : 0;
    if (!halve && form.share_split_ranges && split && ctx.share_buckets && kd.bpl && kd.precomputed && ctx.sw.bpl && count >= 2)
      while (n_sh < count && bpl_range((*out)[first + n_sh].lo, (*out)[first + n_sh].n, &g)) n_sh++;
    if (n_sh < 2) continue;
    for (size_t j = 0; j < n_sh; j++) {
      Range& x = (*out)[first + j];
      x.set = n_sets;
      x.first = j == 0;
      x.last = j + 1 == n_sh;
      x.set_buckets = g.B;  // (one table, one group: every range's geometry has the key's nb buckets)
    }
    n_sets++;
  }
}

// ---- the units -----------------------------------------------------------------------------------------------------------------------
// What ONE bucket-split MSM of geometry g takes of a slot: what msm_plan reserves for its prep (prep_geom.h: prep_bps_needs) and its
// buckets of rec_bytes each.  batch_units keeps a unit's V of them below msel::BPS_BATCH_MAX_BYTES.
inline size_t bps_slot_bytes(const MsmGeom& g, size_t rec_bytes) {
  const PrepNeeds nd = prep_bps_needs(g);
  return nd.vals_a + nd.vals_b + nd.bpl_grp + nd.bpl_order + (size_t)g.B * rec_bytes + nd.prep_small;
}
// A live job of the ring as plan_units sees it
struct UnitJob {
  size_t key = 0;  // its key: an index into the call's JobKeys
  size_t off = 0, n = 0;
  int mont = 0, group_shift = -1;
  bool shared = false, force_chunked = false, skip_ones = false;
};
// What plan_units found for a job when it formed the units: ONE MSM's geometry, shared by all MSMs of its unit (skip_ones set), over
// the key they run over (a 20-bit key's twin)
struct UnitGeom {
  MsmGeom g = {};
  bool over_twin = false;
};
// does plan_units look at this job's geometry (and so want the twin of its 20-bit key)?
inline bool unit_looks_at(const PlanCtx& ctx, const JobKey& key, const UnitJob& j) {
  return !(j.group_shift >= 0 || j.shared || j.force_chunked || msel::choose(key.desc, j.n, false, false, false, ctx.sw).pipeline != msel::BUCKET_SPLIT);
}
// does the call want the twin of 20-bit key `ki` for its units?  (some job over it is looked at: answerable before the twin is built)
inline bool units_need_twin(const PlanCtx& ctx, const JobKey& key, size_t ki, const UnitJob* jobs, size_t k) {
  if (!key.desc.bpl) return false;
  for (size_t i = 0; i < k; i++)
    if (jobs[i].key == ki && unit_looks_at(ctx, key, jobs[i])) return true;
  return false;
}
// The ring runs over UNITS (msm_select.h: batch_units): a live job on the single path, or 2 .. BPS_BATCH consecutive bucket-split MSMs
// that differ in their scalars only.  units[0 .. return) cover jobs [0, k) in order (room for k); ugeom[first] is a unit's geometry.
inline size_t plan_units(const PlanCtx& ctx, const JobKey* keys, const UnitJob* jobs, size_t k, size_t rec_bytes, msel::Unit* units, UnitGeom* ugeom) {
  std::vector<msel::BatchJob> bj(k);
  size_t last_eval = k;  // the last job whose geometry was looked at (none yet)
  for (size_t i = 0; i < k; i++) {
    const UnitJob& j = jobs[i];
    const JobKey& key = keys[j.key];
    msel::BatchJob& b = bj[i];
    b = msel::BatchJob{key.id, key.desc, j.off, j.n, j.mont, j.group_shift, j.shared, j.force_chunked, j.skip_ones, false, 0};
    if (!unit_looks_at(ctx, key, j)) continue;
    // one geometry per run -- taken from a neighbour only if that neighbour's geometry was itself looked at (a job skipped above,
    // a skewed vector for instance, says nothing about the jobs behind it).  (Adjacency only saves a look: equal jobs have equal
    // geometries, so inheriting from a job further back would find the same.)
    if (last_eval + 1 == i && msel::batch_same_run(bj[last_eval], b)) {
      b.geom_ok = bj[last_eval].geom_ok;
      b.slot_bytes = bj[last_eval].slot_bytes;
      ugeom[i] = ugeom[last_eval];
      last_eval = i;
      continue;
    }
    last_eval = i;
    // bps_geom must take the run's geometry, over the key the MSMs run over (a 20-bit key's twin; one that cannot be had is the
    // single path's to report)
    ugeom[i].over_twin = key.desc.bpl;
    if ((!key.desc.bpl || key.has_twin) && bps_unit_geom_ok(ctx.geom, key.desc.bpl ? key.twin_geom : key.geom, j.off, j.n, &ugeom[i].g)) {
      ugeom[i].g.skip_ones = j.skip_ones ? 1u : 0u;
      b.geom_ok = true;
      b.slot_bytes = bps_slot_bytes(ugeom[i].g, rec_bytes);
    }
  }
  return msel::batch_units(bj.data(), bj.size(), ctx.sw, units);
}

// ---- the probes ----------------------------------------------------------------------------------------------------------------------
// The skew probe: would this scalar vector overflow the bucket-per-lane / bucket-split prep?  Its samples, bins and limit
// (PROBE_SAMPLES, PROBE_BINS, PROBE_LIMIT, probe_sample, probe_bin) stand in msm_types.h, where the kernel (vec_kernels.h:
// k_skew_probe) takes the same ones without including the planner.
// the walk a key's MSMs use (msm_types.h: DigitWalk), as the skew probes need it
inline DigitWalk key_walk(const GeomKey& key) {
  DigitWalk d;
  memset(&d, 0, sizeof(d));
  d.c = (u32)key.c;
  d.W = d.c ? (u32)windows_for((int)d.c) : 0u;  // (a plain key has no window of its own: c = 0, never walked)
  if (key.precomp) {
    d.W = (u32)key.W;
    d.n_narrow = (u32)key.n_narrow;
  }
  return d;
}
// shortest vector worth probing: the shortest range of a 20-bit key that takes the bucket-per-lane pipeline (a quarter of its window:
// msm_select.h), the shortest bucket-split MSM over any other key
inline size_t bpl_min_pairs() { return msel::P2(18) + 1; }
inline size_t probe_min_len(const msel::KeyDesc& key) { return key.bpl ? bpl_min_pairs() : msel::BPS_MIN_PAIRS; }
// does a vector of n pairs over `key` want the probe?
inline bool probe_wanted(const PlanCtx& ctx, const msel::KeyDesc& key, size_t n) {
  return ctx.bpl_probe && key.precomputed && n && msel::wants_skew_probe(key, n, ctx.sw);
}
// One window of the signed-digit walk on the host, over a canonical scalar of 8 words (vec_kernels.h: digit_step is the device's, and
// stays there: the kernels' code is not touched).  Three things the device's probe does and this one does not:
//  - skip_ones: set only behind the two-valued probe; a slice with TV_ONES_MIN_SAMPLES unit samples goes to that probe before it
//    gets here, and fewer than 8 samples are a third of what a bin needs -- an optimisation's verdict, the prep's flag is the net
//  - a narrow window's digit is not doubled: doubling is one-to-one within a window, so which samples share a digit does not
//    change, only the bin they hash to
//  - no `t < n` guard: every probed vector has n >= min_len > PROBE_SAMPLES, so every sample is a scalar of the vector
inline u32 host_digit_step(u32 v[8], const DigitWalk& dw, u32 w, u32& carry) {
  const u32 cw = window_bits_of(dw.c, dw.W, dw.n_narrow, w);
  const u32 half = 1u << (cw - 1);
  const u32 raw = (v[0] & ((1u << cw) - 1u)) + carry;
  for (int k = 0; k < 7; k++) v[k] = (v[k] >> cw) | (v[k + 1] << (32 - cw));
  v[7] >>= cw;
  carry = 0;
  u32 d = raw;
  if (raw > half && w + 1 < dw.W) {
    d = (1u << cw) - raw;
    carry = 1;
  }
  return d;
}
// The host's verdict on a slice of n scalars; canonical_at(i, out) writes scalar i in canonical form, 8 little-endian words (the
// caller keeps the conversion from Montgomery form).  Shorter than min_len: false without looking.
template <class Load>
bool skew_probe_host(size_t n, size_t min_len, const DigitWalk& dw, Load&& canonical_at) {
  if (n < min_len) return false;
  std::vector<u32> smp((size_t)PROBE_SAMPLES * 8);
  for (u32 t = 0; t < PROBE_SAMPLES; t++) canonical_at((size_t)probe_sample(t, n), &smp[(size_t)t * 8]);
  std::vector<u32> carry(PROBE_SAMPLES, 0), bins(PROBE_BINS);
  for (u32 w = 0; w < dw.W; w++) {
    std::fill(bins.begin(), bins.end(), 0u);
    for (u32 t = 0; t < PROBE_SAMPLES; t++) {
      const u32 d = host_digit_step(&smp[(size_t)t * 8], dw, w, carry[t]);
      if (d != 0 && ++bins[probe_bin(d)] >= PROBE_LIMIT) return true;
    }
  }
  return false;
}
// Does a host slice LOOK two-valued (every scalar 0 or one value v)?  The probe's samples with at most one non-zero value among them.
// The exact test is the device probe's (k_tv_probe); this only decides whether the slices go there.
inline bool looks_two_valued(const uint64_t* s, size_t n) {
  const uint64_t* v = nullptr;
  for (u32 t = 0; t < PROBE_SAMPLES; t++) {
    const uint64_t* e = s + 4 * (size_t)probe_sample(t, n);
    if (!(e[0] | e[1] | e[2] | e[3])) continue;
    if (!v) v = e;
    else if (memcmp(v, e, 32) != 0) return false;
  }
  return true;
}
// ... or hold a share of UNIT scalars (the boolean wires of a witness: their generators are summed apart)?  The same samples, the
// same threshold as the device probe's count; `one`: the unit as the slice stores it.
constexpr u32 TV_ONES_MIN_SAMPLES = msel::TV_ONES_MIN_SAMPLES;
inline bool has_unit_scalars(const uint64_t* s, size_t n, const u32 one[8]) {
  u32 cnt = 0;
  for (u32 t = 0; t < PROBE_SAMPLES; t++)
    if (memcmp(s + 4 * (size_t)probe_sample(t, n), one, 32) == 0) cnt++;
  return cnt >= TV_ONES_MIN_SAMPLES;
}
// Identical vectors (a prover commits to the same accumulator vector more than once) are probed once: first[j] = the first i <= j
// with the scalars and the length of vector j.  The offset into the key is deliberately not compared: what the probes say depends
// on the scalars, their number and the key alone.
struct VecRef {
  const void* scalars;
  size_t n;
};
template <class At>
void first_identical(size_t k, At&& at, size_t* first) {  // at(j): vector j's VecRef
  for (size_t j = 0; j < k; j++) {
    first[j] = j;
    const VecRef b = at(j);
    for (size_t i = 0; i < j; i++) {
      const VecRef a = at(i);
      if (a.scalars == b.scalars && a.n == b.n) {
        first[j] = first[i];
        break;
      }
    }
  }
}

}  // namespace mjobs
}  // namespace amsm
