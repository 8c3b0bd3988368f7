// msel::batch_units (accumulation_amd/csrc/msm_select.h) -- which bucket-split MSMs of one call run as one launch per pipeline stage --
// at every edge, without a GPU.  Plain C++ over the header alone; tests/test_batch_units_cpu.py holds the expected lines.
//   units <case> <count of unit 0>+<count of unit 1>+...          the units of the case's job list, in order
//   unit_tail <case> <place> form=.. partials=.. ticket=.. covered=..  the tail of a unit of nv MSMs (nv * n_sets bucket sets in one
//                                                                  table) against what tail_plan_any_place reserves for it
// The program fails if a unit list does not cover its jobs exactly once in order, or a tail is not covered.
#include <cstdio>
#include <string>
#include <vector>

#include "../../accumulation_amd/csrc/msm_select.h"

using namespace amsm::msel;

static int bad = 0;
static int key_a, key_b;  // two key identities

static KeyDesc table_key(size_t n, int c) { return KeyDesc{n, true, false, false, c}; }
static KeyDesc bpl_key(size_t n) { return KeyDesc{n, true, true, false, BPL_WINDOW}; }
static KeyDesc plain_key(size_t n) { return KeyDesc{n, false, false, false, 0}; }

// a bucket-split candidate: 2^16 pairs at offset 500 of a 16-bit table, canonical scalars, 40 MiB of slot
static BatchJob job(size_t n = P2(16)) {
  return BatchJob{&key_a, table_key(P2(16) + 1000, 16), 500, n, 0, -1, false, false, false, true, (size_t)40 << 20};
}

static void show(const char* name, const std::vector<BatchJob>& jobs, const Switches& sw) {
  std::vector<Unit> units(jobs.size() + 1);
  const size_t n = batch_units(jobs.data(), jobs.size(), sw, units.data());
  std::string s;
  size_t at = 0;
  for (size_t u = 0; u < n; u++) {
    if (units[u].first != at || units[u].count < 1 || units[u].count > (size_t)BPS_BATCH) bad++;
    for (size_t v = 1; v < units[u].count; v++)  // the jobs of a unit share everything but their scalars
      if (!batch_same_run(jobs[units[u].first], jobs[units[u].first + v]) || !batch_candidate(jobs[units[u].first + v], sw)) bad++;
    if (units[u].count > 1 && units[u].count * jobs[units[u].first].slot_bytes > BPS_BATCH_MAX_BYTES) bad++;
    at += units[u].count;
    s += (u ? "+" : "") + std::to_string(units[u].count);
  }
  if (at != jobs.size()) bad++;
  printf("units %s %s\n", name, jobs.empty() ? "-" : s.c_str());
}

int main() {
  const Switches sw;
  // runs of 1, 2, 8, 9 and 17 jobs
  for (size_t k : {0, 1, 2, 8, 9, 17}) show(("run_" + std::to_string(k)).c_str(), std::vector<BatchJob>(k, job()), sw);
  // a job in the middle of five that differs in one field splits the run
  {
    struct M {
      const char* name;
      void (*change)(BatchJob&);
    };
    const M mids[] = {
        {"mid_n", [](BatchJob& j) { j.n = P2(16) + 1; }},
        {"mid_off", [](BatchJob& j) { j.off = 501; }},
        {"mid_mont", [](BatchJob& j) { j.mont = 1; }},
        {"mid_skip_ones", [](BatchJob& j) { j.skip_ones = true; }},
        {"mid_force_chunked", [](BatchJob& j) { j.force_chunked = true; }},
        {"mid_key", [](BatchJob& j) { j.key = &key_b; }},
        {"mid_grouped", [](BatchJob& j) { j.group_shift = 5; }},
        {"mid_shared", [](BatchJob& j) { j.shared = true; }},
        {"mid_no_geom", [](BatchJob& j) { j.geom_ok = false; }},
        {"mid_empty", [](BatchJob& j) { j.n = 0; }},
    };
    for (const M& m : mids) {
      std::vector<BatchJob> jobs(5, job());
      m.change(jobs[2]);
      show(m.name, jobs, sw);
    }
    // two different runs back to back: each is a unit of its own
    std::vector<BatchJob> jobs(3, job());
    for (int i = 0; i < 3; i++) jobs.push_back(job(P2(16) + 1));
    show("two_runs", jobs, sw);
    // grouped / shared jobs never join a unit, not even with their like
    std::vector<BatchJob> grouped(4, job());
    for (BatchJob& j : grouped) j.group_shift = 5;
    show("all_grouped", grouped, sw);
    std::vector<BatchJob> shared(4, job());
    for (BatchJob& j : shared) j.shared = true;
    show("all_shared", shared, sw);
  }
  // the switch: AMSM_BPS_BATCH = 0 / 1 all singles, 2 / 3 / 8 the cap; AMSM_BPS = 0 / 1: no plain MSM takes the pipeline at all
  for (int cap : {0, 1, 2, 3, 8}) {
    Switches s;
    s.bps_batch = cap;
    show(("cap_" + std::to_string(cap)).c_str(), std::vector<BatchJob>(7, job()), s);
  }
  for (int bps : {0, 1}) {
    Switches s;
    s.bps = bps;
    show(("bps_" + std::to_string(bps)).c_str(), std::vector<BatchJob>(4, job()), s);
  }
  {
    Switches s;
    s.window_override = true;
    show("window_override", std::vector<BatchJob>(4, job()), s);
  }
  // the 512 MiB rule: a geometry made large on purpose shrinks V
  for (size_t mib : {64, 65, 128, 200, 256, 257, 600}) {
    std::vector<BatchJob> jobs(8, job());
    for (BatchJob& j : jobs) j.slot_bytes = mib << 20;
    show(("slot_" + std::to_string(mib) + "_mib").c_str(), jobs, sw);
  }
  // sizes just outside [2^16, 2^17] never form units; the edges inside do
  for (size_t n : {P2(16) - 1, P2(16), P2(17), P2(17) + 1}) {
    std::vector<BatchJob> jobs(3, job(n));
    for (BatchJob& j : jobs) j.desc = table_key(P2(18), 16), j.off = 0;
    show(("pairs_" + std::to_string(n)).c_str(), jobs, sw);
  }
  // the key kinds: a 20-bit key's ranges of 2^16 pairs run over the twin and batch; plain keys and direct-sum keys do not
  {
    std::vector<BatchJob> jobs(3, job());
    for (BatchJob& j : jobs) j.desc = bpl_key(P2(20));
    show("key_bpl_over_twin", jobs, sw);
    for (BatchJob& j : jobs) j.desc = plain_key(P2(17));
    show("key_plain", jobs, sw);
    for (BatchJob& j : jobs) j.desc = KeyDesc{P2(15), true, false, true, 13}, j.n = P2(15), j.off = 0;
    show("key_direct", jobs, sw);
  }

  // the tail of a unit: nv * n_sets sets of nb buckets in one table -- what the plan reserves before the Place is known covers the
  // launches at every Place (as select_check.cpp checks for single MSMs)
  struct G {
    const char* name;
    unsigned nb, n_sets, E;  // of ONE MSM
  };
  const G geoms[] = {{"w16_2p16", 1u << 15, 1, 16u << 16}, {"w16_2p17", 1u << 15, 1, 16u << 17}, {"w17_2p17", 1u << 16, 1, 16u << 17}};
  const Place places[] = {Place::LONE, Place::BATCH_LAST, Place::BATCH_INNER};
  const char* place_names[] = {"lone", "batch_last", "batch_inner"};
  for (const G& g : geoms)
    for (unsigned nv = 2; nv <= (unsigned)BPS_BATCH; nv++) {
      const unsigned sets = g.n_sets * nv, B = g.nb * sets, E = g.E * nv;
      const TailPlan w = tail_plan_any_place(g.nb, sets, B, E, false);
      for (int p = 0; p < 3; p++) {
        const TailPlan t = tail_plan(g.nb, sets, B, E, false, places[p]);
        const size_t lanes = ((size_t)t.partials * 256u) >> (t.quad ? 2u : 0u);
        bool ok = t.form != RED2 && t.partials >= 1 && t.partials <= w.partials && t.rc_records == 0 && (!t.ticket || w.ticket);
        ok = ok && t.red_s >= 1 && (size_t)t.red_threads * t.red_s == g.nb && lanes >= t.red_threads;
        ok = ok && t.ticket == (t.form == FUSED_QUAD) && t.quad == (t.form == FUSED_QUAD);
        if (!ok) bad++;
        printf("unit_tail %s_x%u %s form=%s partials=%u ticket=%d covered=%d\n", g.name, nv, place_names[p], tail_form_name(t.form), t.partials,
               t.ticket ? 1 : 0, ok ? 1 : 0);
      }
    }
  return bad ? 1 : 0;
}
