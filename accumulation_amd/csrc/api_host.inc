// Part of api.hip (inside its anonymous namespace): the host side of the schemes -- fixed-base cache, linear combinations
// (single, split over the host pool, batched).
// Bases that recur with full-size scalars get a fixed-base table (HFixedBase) on their third use; a handful of tables per thread
// and field, least recently used evicted.  What has been SEEN is tracked apart from what has been BUILT (round 5): the one-time
// points of a combination (commitments, proof elements) pass through the `seen` ring without ever evicting a table.
template <class Fq>
struct FixedBaseCache {
  static constexpr size_t SLOTS = 4, SEEN = 32;
  static constexpr unsigned BUILD_AT = 3;
  static constexpr uint64_t STALE_CALLS = 64;
  static constexpr int N = host::HFe<Fq>::N;
  std::vector<host::HFixedBase<Fq>> entries;  // built tables
  struct Seen {
    uint64_t key[2 * N];
    unsigned uses;
    uint64_t stamp;
  };
  std::vector<Seen> seen;
  uint64_t call = 0;  // tables touched by the current host_lincomb call (stamp == call) are never evicted
  FixedBaseCache() { entries.reserve(SLOTS); }  // no reallocation: pointers handed out stay valid
  const host::HFixedBase<Fq>* lookup(const uint64_t* xy, const host::HXYZZ<Fq>& p) {
    for (auto& c : entries)
      if (memcmp(c.key, xy, 16 * N) == 0) {
        c.stamp = call;
        return &c;
      }
    Seen* e = nullptr;
    for (auto& c : seen)
      if (memcmp(c.key, xy, 16 * N) == 0) e = &c;
    if (!e) {
      if (seen.size() < SEEN) {
        seen.emplace_back();
        e = &seen.back();
      } else {
        e = &seen[0];
        for (auto& c : seen)
          if (c.stamp < e->stamp) e = &c;
      }
      memcpy(e->key, xy, 16 * N);
      e->uses = 0;
    }
    e->stamp = call;
    if (++e->uses < BUILD_AT) return nullptr;
    host::HFixedBase<Fq>* victim = nullptr;
    if (entries.size() < SLOTS) {
      entries.emplace_back();
      victim = &entries.back();
    } else {
      // a table costs ~3.5 windowed multiplications to build and saves about one per use: it is only ever replaced once it has
      // gone STALE_CALLS combinations without a hit -- more recurring bases than slots must not rebuild tables in turn
      for (auto& c : entries)
        if (c.stamp + STALE_CALLS < call && (!victim || c.stamp < victim->stamp)) victim = &c;
      if (!victim) {
        e->uses = BUILD_AT - 1;  // (asks again on its next use)
        return nullptr;
      }
    }
    memcpy(victim->key, xy, 16 * N);
    victim->stamp = call;
    victim->build(p);
    e->uses = 0;
    return victim;
  }
};

inline bool fixed_base_enabled() { return true; }
template <class Fq>
FixedBaseCache<Fq>& fixed_base_cache() {
  thread_local FixedBaseCache<Fq> cache;
  return cache;
}
// k * P for a point that recurs over calls (h' of an IPA opening): the thread's fixed-base table once it exists
template <class Fq, class Fr>
host::HXYZZ<Fq> host_mul_cached(const uint64_t* xy, const host::HFe<Fr>& k_mont) {
  host::HFe<Fr> k = host::h_from_mont<Fr>(k_mont);
  host::HXYZZ<Fq> p = host::hx_from_affine<Fq>(xy, false);
  const host::HFixedBase<Fq>* fb = nullptr;
  if (fixed_base_enabled() && host::hx_scalar_bits(k.v) > 128) {
    FixedBaseCache<Fq>& cache = fixed_base_cache<Fq>();
    cache.call++;
    fb = cache.lookup(xy, p);
  }
  return fb ? fb->mul(k.v) : host::hx_mul<Fq>(p, k.v);
}

// The curve's GLV set-up on the host (host_glv.h: curve_glv -- lambda, beta, the lattice basis, all verified at first use); null if it
// failed
template <class Fq, class Fr>
const host::Glv<Fq, Fr>* host_glv() {
  const host::Glv<Fq, Fr>& g = host::curve_glv<Fq>();
  return g.ok ? &g : nullptr;
}

// Independent combinations sum_i k_i P_i (k Montgomery) as XYZZ points.  Round 5: every scalar of more than 136 bits goes in as
// its two GLV halves (128 shared doublings per Straus loop instead of 255: the powers nu^i, mu^i of the 128-bit challenges are
// full-size), digits are signed (8-entry tables), and the TERMS of all jobs -- not the jobs -- are what the host pool shares
// out: a task is a slice of one job's terms with its own doublings, so the longest job no longer bounds the call (hp_as's
// combine: three jobs of 2 / 2 / 5 full-size terms, 260 -> ~100 us).
constexpr size_t LINCOMB_TASK_MIN_TERMS = 2;
template <class Fq, class Fr>
void host_lincomb_jobs(size_t n_jobs, const size_t* n_terms, const uint64_t* const* xy, const uint8_t* const* is_inf,
                       const uint64_t* const* scalars_mont, bool use_pool, host::HXYZZ<Fq>* out) {
  constexpr int N = host::HFe<Fq>::N;
  const host::Glv<Fq, Fr>* glv = host_glv<Fq, Fr>();
  FixedBaseCache<Fq>& cache = fixed_base_cache<Fq>();  // per thread: looked up here, on the calling thread
  cache.call++;
  struct Fixed {
    size_t job;
    const host::HFixedBase<Fq>* fb;
    u64 k[4];
  };
  std::vector<host::HTerm<Fq>> terms;
  std::vector<size_t> job_lo(n_jobs + 1, 0);
  std::vector<Fixed> fixed;
  for (size_t j = 0; j < n_jobs; j++) {
    out[j] = host::hx_inf<Fq>();
    job_lo[j] = terms.size();
    for (size_t i = 0; i < n_terms[j]; i++) {
      host::HFe<Fr> s;
      memcpy(s.v, scalars_mont[j] + 4 * i, 32);
      s = host::h_from_mont<Fr>(s);
      const host::HXYZZ<Fq> p = host::hx_from_affine<Fq>(xy[j] + i * 2 * N, is_inf && is_inf[j] && is_inf[j][i]);
      const int bits = host::hx_scalar_bits(s.v);
      if (bits == 0 || host::hx_is_inf<Fq>(p)) continue;
      if (bits == 1) {
        out[j] = host::hx_add<Fq>(out[j], p);
        continue;
      }
      if (fixed_base_enabled() && bits > 128) {
        if (const host::HFixedBase<Fq>* fb = cache.lookup(xy[j] + i * 2 * N, p)) {
          Fixed f{j, fb, {s.v[0], s.v[1], s.v[2], s.v[3]}};
          fixed.push_back(f);
          continue;
        }
      }
      host::hx_push_terms<Fq, Fr>(glv, p, s.v, terms);
    }
  }
  job_lo[n_jobs] = terms.size();
  // tasks: slices of a job's terms (never across jobs), sized so that the pool's threads all get one; a fixed-base product is a task
  struct Task {
    size_t job, lo, hi;
    const Fixed* fx;
  };
  std::vector<Task> tasks;
  const size_t threads = use_pool ? HostPool::get().workers.size() + 1 : 1;
  const size_t per = std::max(LINCOMB_TASK_MIN_TERMS, (terms.size() + fixed.size() + threads - 1) / threads);
  for (size_t j = 0; j < n_jobs; j++) {
    const size_t cnt = job_lo[j + 1] - job_lo[j];
    const size_t parts = cnt ? (cnt + per - 1) / per : 0;
    for (size_t t = 0; t < parts; t++) tasks.push_back(Task{j, job_lo[j] + cnt * t / parts, job_lo[j] + cnt * (t + 1) / parts, nullptr});
  }
  for (const Fixed& f : fixed) tasks.push_back(Task{f.job, 0, 0, &f});
  std::vector<host::HXYZZ<Fq>> part(tasks.size());
  auto run_task = [&](size_t t) {
    const Task& k = tasks[t];
    part[t] = k.fx ? k.fx->fb->mul(k.fx->k) : host::hx_straus_signed<Fq>(terms.data() + k.lo, k.hi - k.lo);
  };
  if (threads > 1 && tasks.size() > 1) HostPool::get().run(tasks.size(), run_task);
  else
    for (size_t t = 0; t < tasks.size(); t++) run_task(t);
  for (size_t t = 0; t < tasks.size(); t++) out[tasks[t].job] = host::hx_add<Fq>(out[tasks[t].job], part[t]);
}
template <class Fq, class Fr>
host::HXYZZ<Fq> host_lincomb_xyzz(const uint64_t* xy, const uint8_t* is_inf, const uint64_t* scalars_mont, size_t n,
                                  bool may_split) {
  host::HXYZZ<Fq> r;
  host_lincomb_jobs<Fq, Fr>(1, &n, &xy, is_inf ? &is_inf : nullptr, &scalars_mont, may_split, &r);
  return r;
}

template <class Fq, class Fr>
int host_lincomb_impl(const uint64_t* xy, const uint8_t* is_inf, const uint64_t* scalars_mont, size_t n,
                      uint64_t* out_xy, uint8_t* out_inf) {
  write_affine<Fq>(host_lincomb_xyzz<Fq, Fr>(xy, is_inf, scalars_mont, n, true), out_xy, out_inf);
  return AMSM_OK;
}

// independent combinations in one call: the terms of all jobs shared out over the pool, ONE batched normalisation
template <class Fq, class Fr>
int host_lincomb_batch_impl(size_t n_jobs, const size_t* n_terms, const uint64_t* const* xy, const uint8_t* const* is_inf,
                            const uint64_t* const* scalars_mont, uint64_t* out_xy, uint8_t* out_inf) {
  std::vector<host::HXYZZ<Fq>> r(n_jobs, host::hx_inf<Fq>());
  if (n_jobs) host_lincomb_jobs<Fq, Fr>(n_jobs, n_terms, xy, is_inf, scalars_mont, true, r.data());
  if (out_inf) memset(out_inf, 0, n_jobs);
  write_affine_batch<Fq>(r, out_xy, out_inf);
  return AMSM_OK;
}
