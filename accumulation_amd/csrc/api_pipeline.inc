// Part of api.hip (included inside its anonymous namespace): error macros, workspace buffers, MSM geometry, the pipeline
// launcher (msm_enqueue / msm_collect) and the single / batch / multi / split drivers.

#define HIP_TRY(expr)                                                                                  \
  do {                                                                                                 \
    hipError_t _e = (expr);                                                                            \
    if (_e != hipSuccess) {                                                                            \
      fprintf(stderr, "[amsm] HIP error %s (%d) at %s:%d: %s\n", hipGetErrorName(_e), (int)_e, __FILE__, \
              __LINE__, #expr);                                                                        \
      return _e == hipErrorOutOfMemory ? AMSM_E_OOM : AMSM_E_HIP;                                      \
    }                                                                                                  \
  } while (0)

#define TRY(expr)            \
  do {                       \
    int _s = (expr);         \
    if (_s != AMSM_OK) return _s; \
  } while (0)

// Grow-only workspace: the old buffer goes back BEFORE the new one is asked for (the peak stays at the larger of the two), so a
// refusal leaves the buffer empty: p null and bytes 0, and the next use asks again
int ensure(DevBuf& b, size_t bytes) {
  if (b.bytes >= bytes && b.p) return AMSM_OK;
  if (b.p) HIP_TRY(gate_free(b.p));
  b.p = nullptr;
  b.bytes = 0;
  size_t want = bytes + bytes / 8 + 256;
  TRY(gate_alloc(b.owner, GATE_DEVICE, want, false, &b.p));
  b.bytes = want;
  return AMSM_OK;
}
void DevBuf::release() {
  if (p) (void)gate_free(p);
  p = nullptr;
  bytes = 0;
}

// ensure() for an allocation the caller can do without: no message, and HIP's sticky last error is cleared (the gate does) -- a
// tolerated failure must not surface as AMSM_E_OOM at the next HIP_TRY(hipGetLastError()) of an unrelated call (ADVICE r4)
bool try_ensure(DevBuf& b, size_t bytes) {
  if (b.bytes >= bytes && b.p) return true;
  if (b.p) (void)gate_free(b.p);
  b.p = nullptr;
  b.bytes = 0;
  const size_t want = bytes + bytes / 8 + 256;
  if (gate_alloc(b.owner, GATE_DEVICE, want, true, &b.p) != AMSM_OK) return false;
  b.bytes = want;
  return true;
}

int ensure_pinned(Slot* sl, size_t bytes) {
  if (sl->h_pinned_bytes >= bytes) return AMSM_OK;
  if (sl->h_pinned) HIP_TRY(gate_free(sl->h_pinned));
  sl->h_pinned = nullptr;
  sl->h_pinned_bytes = 0;
  TRY(gate_alloc(sl->owner, GATE_PINNED, bytes + 4096, false, &sl->h_pinned));
  sl->h_pinned_bytes = bytes + 4096;
  return AMSM_OK;
}

// The slot's arrival counters of the fused tail (k_bucket_reduce<QUAD, FUSED>), one per bucket set: zeroed when the buffer grows (a memset, then the
// caller's stream is synchronised), left clear by every launch
int ensure_red_ticket(amsm_ctx* ctx, Slot* sl, size_t n_sets) {
  if (sl->red_ticket.bytes < n_sets * 4) {
    TRY(ensure(sl->red_ticket, std::max<size_t>(n_sets * 4, 4096)));
    // (hipMemset on device memory may return before it has run, and the null stream does not order the context's non-blocking
    // streams: a reduction that found the counters not yet zeroed never saw its last workgroup -- one wrong sum in ~3 of 10 proves over
    // eight contexts, none with the two-launch tail: profiles/r06_experiments.md section 1b)
    HIP_TRY(hipMemsetAsync(sl->red_ticket.p, 0, sl->red_ticket.bytes, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
  }
  return AMSM_OK;
}

using msel::ilog2_ceil;

template <class Fq>
constexpr size_t xyzz_bytes() {
  return 4 * Fq::L * 4;
}
// Everything a tail of n_sets sets needs on slot `sl` (msm_select.h: tail_plan says how much; launch_tail / launch_fold write no more):
// the partial records, the folded ones with their two flag words on the device and in page-locked memory, the row / column scratch and
// the arrival counters
template <class Fq>
int reserve_tail(amsm_ctx* ctx, Slot* sl, size_t n_sets, const msel::TailPlan& t) {
  const size_t rec = xyzz_bytes<Fq>();
  if (t.rc_records) TRY(ensure(sl->red2_rc, t.rc_records * rec));
  TRY(ensure(sl->red_out, n_sets * t.partials * rec));
  TRY(ensure(sl->fold_out, n_sets * rec + 64));
  TRY(ensure_pinned(sl, n_sets * rec + 64));
  return t.ticket ? ensure_red_ticket(ctx, sl, n_sets) : AMSM_OK;
}

// Every size threshold -- which window a key's table is built for, which pipeline an MSM takes, where a long MSM is cut -- lives in
// msm_select.h (two tables, plain C++, unit-tested without a GPU: tests/test_pipeline_select_cpu.py).  Here: how the context's
// switches and a key look to it.
inline msel::KeyDesc key_desc(const amsm_bases* b) {
  msel::KeyDesc k;
  k.n = b->n;
  k.precomputed = b->precomp != 0;
  k.bpl = b->bpl != 0;
  k.direct_table = b->d_small != nullptr;
  k.c = b->precomp ? b->c : 0;
  return k;
}
inline msel::Switches switches_of(const amsm_ctx* c) {
  msel::Switches s;
  s.bpl = c->bpl;
  s.bpl_plain = c->bpl_plain;
  s.bps = c->bps;
  s.split_log2 = c->split_log2;
  s.direct = c->direct_max_log2 > 0;
  s.window_override = c->window_override != 0;
  s.bps_batch = c->bps_batch;
  s.top_sets = c->top_sets;
  return s;
}
inline msel::Choice choose_pipeline(const amsm_ctx* ctx, const amsm_bases* bases, size_t n, int group_shift, bool skewed) {
  const bool grouped = group_shift >= 0;
  const bool regular = grouped && group_shift < 30 && n % ((size_t)2 << group_shift) == 0;
  return msel::choose(key_desc(bases), n, grouped, regular, skewed, switches_of(ctx));
}
constexpr int BPL_WINDOW = msel::BPL_WINDOW;
constexpr size_t BPS_MIN_PAIRS = msel::BPS_MIN_PAIRS, BPS_MAX_PAIRS = msel::BPS_MAX_PAIRS;
// ... and to the geometry (msm_geom.h: make_geom, bpl_geom, bps_geom, chunked_geom -- plain C++ too: tests/test_msm_geom_cpu.py)
inline GeomKey geom_key(const amsm_bases* b) {
  GeomKey k;
  k.n = b->n;
  k.precomp = b->precomp != 0;
  k.c = b->c;
  k.W = b->W;
  k.n_narrow = b->n_narrow;
  k.top_shift = b->top_shift;
  return k;
}
inline GeomCtx geom_ctx(const amsm_ctx* c) {
  GeomCtx g;
  g.window_override = c->window_override;
  g.wave_slots = c->wave_slots;
  g.top_sets = c->top_sets;
  memcpy(g.r_mod, c->r_mod, sizeof(g.r_mod));
  return g;
}

// ... and to the job list (msm_jobs.h: plan_ranges, plan_units, the probes' rules -- plain C++ as well: tests/test_msm_jobs_cpu.py)
inline mjobs::PlanCtx plan_ctx(const amsm_ctx* c) {
  mjobs::PlanCtx p;
  p.sw = switches_of(c);
  p.geom = geom_ctx(c);
  p.share_buckets = c->share_buckets;
  p.host_halves = c->host_halves;
  p.bpl_probe = c->bpl_probe;
  return p;
}
inline mjobs::JobKey job_key(const amsm_bases* b, const amsm_bases* twin = nullptr) {  // twin: the 17-bit twin of a 20-bit key, once built
  mjobs::JobKey k;
  k.id = b;
  k.desc = key_desc(b);
  k.geom = geom_key(b);
  k.has_twin = twin != nullptr;
  if (twin) {
    k.twin_desc = key_desc(twin);
    k.twin_geom = geom_key(twin);
  }
  return k;
}

template <class Fq>
constexpr size_t affine_bytes() {
  return 2 * Fq::L * 4;
}

// ---------------------------------------------------------------------------------------------
// The MSM pipeline.  Leaves n_sets folded XYZZ records in ctx->fold_out.
// ---------------------------------------------------------------------------------------------
void stage_mark(amsm_ctx* ctx, Slot* sl, int idx, hipStream_t st) {
  if (ctx->profiling) (void)hipEventRecord(sl->ev[idx], st);
}

// AMSM_DEBUG=1: synchronise after every stage of the pipeline and report it on stderr (finds the faulting kernel)
inline bool amsm_debug() {
  static const bool on = getenv("AMSM_DEBUG") != nullptr;
  return on;
}
#define AMSM_DBG(name)                                    \
  do {                                                    \
    if (amsm_debug()) {                                   \
      fprintf(stderr, "[amsm] %s ...", name);             \
      hipError_t e_ = hipDeviceSynchronize();             \
      fprintf(stderr, " %s\n", hipGetErrorString(e_));    \
    }                                                     \
  } while (0)

// Work already queued on the caller's stream (e.g. the kernels that produced the scalars) must be
// visible to the prep stream.  Called ONCE per API call, before its MSMs are enqueued -- never between the MSMs of
// a batch: an event recorded on the caller's stream there would sit behind the previous MSM's accumulate L0.
int prep_fork(amsm_ctx* ctx) {
  HIP_TRY(hipEventRecord(ctx->fork, ctx->stream));
  HIP_TRY(hipStreamWaitEvent(ctx->s_prep, ctx->fork, 0));
  return AMSM_OK;
}

template <class Fq>
int bases_alt(amsm_ctx* ctx, const amsm_bases* b, const amsm_bases** out);

// one MSM over generators [off, off + n) of `key` (n already clamped to the key), as the single-MSM entry points describe it
inline MsmJob single_job(const amsm_bases* key, size_t off, const void* scalars, size_t n, int mont, int group_shift = -1) {
  MsmJob j;
  j.key = key;
  j.off = off;
  j.n = n;
  j.scalars = scalars;
  j.mont = mont;
  j.group_shift = group_shift;
  return j;
}

// Direct sum (round 4; msm_kernels.h k_direct_sum): an MSM over (a range of) a small key that carries the table of digit
// multiples -- ONE launch of mixed additions with its workgroup trees, the quad fold, the records mirrored to the host: three
// commands on the caller's stream against the ~14 of the sorted pipelines.  Grouped MSMs (two sums) keep the windowed pipelines.
inline bool direct_sum_applies(const amsm_ctx* ctx, const amsm_bases* bases, size_t n, int group_shift, bool force_chunked) {
  return !force_chunked && n >= 1 && choose_pipeline(ctx, bases, n, group_shift, false).pipeline == msel::DIRECT_SUM;
}
inline bool direct_sum_applies(const amsm_ctx* ctx, const MsmJob& j) { return direct_sum_applies(ctx, j.key, j.n, j.group_shift, j.force_chunked); }
// Geometry and every allocation of nv direct sums over one key in one launch on slot `sl` (msm_enqueue_direct_batch; nv = 1 may be
// grouped); nothing of the MSM is launched
struct DirectPlan {
  u32 m;       // windows per lane
  u32 blocks;  // workgroups per MSM / per class
};
template <class Fq>
int direct_plan(amsm_ctx* ctx, Slot* sl, const MsmJob* jobs, size_t nv, DirectPlan* out) {
  if (nv == 0 || nv > (size_t)DS_BATCH) return AMSM_E_INVALID_ARG;
  const int group_shift = jobs[0].group_shift;  // (a batch shares one scalar form and is not grouped: msm_multi_xyzz)
  if (group_shift >= 0 && nv != 1) return AMSM_E_INVALID_ARG;
  size_t n_max = 0;
  for (size_t v = 0; v < nv; v++) n_max = std::max(n_max, jobs[v].n);
  MsmGeom g;
  memset(&g, 0, sizeof(g));
  g.n = (u32)n_max;
  g.base_off = (u32)jobs[0].off;
  g.n_sets = group_shift >= 0 ? 2 : (u32)nv;
  g.groups = g.n_sets;
  g.group_shift = group_shift >= 0 ? (u32)group_shift : 0u;
  g.W = 1;
  g.c = 4;
  g.precomp = 1;
  sl->geom = g;
  // windows per lane: ~2^16 lanes for one MSM (one workgroup per CU) -- fewer lanes lengthen every lane's chain of additions,
  // more lengthen the fold's; a batch may fill the three waves per SIMD the kernel's registers allow
  const size_t lane_cap = nv > 1 ? (size_t)3 << 16 : (size_t)1 << 16;
  u32 m = 4;
  while (m < DS_W && (nv * n_max * (size_t)(DS_W / m)) > lane_cap) m <<= 1;
  const u32 blocks = cdiv((u32)((group_shift >= 0 ? n_max / 2 : n_max) * (DS_W / m)), 256);  // per MSM / per class
  msel::TailPlan fold{};  // no bucket reduction: the sum kernel leaves the partial records, the bare fold follows
  fold.partials = blocks;
  TRY(reserve_tail<Fq>(ctx, sl, g.n_sets, fold));
  if (!sl->ds_flags.p) {  // zeroed once: k_fold leaves the words clear behind every MSM
    TRY(ensure(sl->ds_flags, 64));
    HIP_TRY(hipMemsetAsync(sl->ds_flags.p, 0, 64, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
  }
  out->m = m;
  out->blocks = blocks;
  return AMSM_OK;
}

// Geometry and EVERY allocation of one MSM on slot `sl`: what can fail for lack of memory fails here, so a caller with side effects
// to apply first (amsm_ipa_round_fused folds its vectors in place) can reserve before it commits.  Nothing of the MSM is launched --
// but flag words and arrival counters are zeroed when they are first allocated or grow: a memset on the caller's stream, which is
// then synchronised (direct_plan, ensure_red_ticket).
// *eff = the key the MSM runs over: job.key, or its 17-bit twin when msm_select.h sends a range of a 20-bit key there.
template <class Fq>
int msm_plan(amsm_ctx* ctx, Slot* sl, const MsmJob& job, bool* short_prep_out, const amsm_bases** eff = nullptr) {
  const amsm_bases* bases = job.key;
  const size_t base_off = job.off, n = job.n;
  const int group_shift = job.group_shift;
  MsmGeom g;
  const size_t rec = xyzz_bytes<Fq>();
  if (direct_sum_applies(ctx, job)) {  // no prep, no buckets
    DirectPlan dp;
    if (eff) *eff = bases;
    *short_prep_out = false;
    return direct_plan<Fq>(ctx, sl, &job, 1, &dp);
  }
  const msel::Choice ch = choose_pipeline(ctx, bases, n, group_shift, job.force_chunked);
  const GeomCtx gc = geom_ctx(ctx);
  auto common = [&]() -> int {  // what every sorted pipeline needs behind its accumulation: the buckets, and the tail wherever the
    TRY(ensure(sl->buckets, (size_t)g.B * rec));  // MSM will stand in its call (msm_enqueue knows, callers that reserve first do not)
    return reserve_tail<Fq>(ctx, sl, g.n_sets, msel::tail_plan_any_place(g.nb, g.n_sets, g.B, g.E, g.bpl == 1u));
  };
  auto prep_reserve = [&](const PrepNeeds& nd) -> int {  // a bucket-per-lane / bucket-split MSM (prep_geom.h: what its prep chain needs)
    TRY(ensure(sl->vals_a, nd.vals_a));
    TRY(ensure(sl->vals_b, nd.vals_b));
    TRY(ensure(sl->bpl_grp, nd.bpl_grp));
    TRY(ensure(sl->bpl_order, nd.bpl_order));
    TRY(common());
    return ensure(sl->prep_small, nd.prep_small);
  };
  if (ch.pipeline == msel::BUCKET_PER_LANE && bpl_geom(gc, geom_key(bases), base_off, n, group_shift, ch.plain_window, &g)) {
    sl->geom = g;
    if (eff) *eff = bases;
    TRY(prep_reserve(prep_bpl_needs(g)));
    *short_prep_out = true;
    return AMSM_OK;
  }
  // everything a 20-bit key's table does not take runs over its 17-bit twin (built on first use)
  if (bases->bpl) TRY(bases_alt<Fq>(ctx, bases, &bases));
  if (eff) *eff = bases;
  if (ch.pipeline == msel::BUCKET_SPLIT && bps_geom(gc, geom_key(bases), base_off, n, group_shift, &g)) {
    sl->geom = g;
    TRY(prep_reserve(prep_bps_needs(g)));
    *short_prep_out = true;
    return AMSM_OK;
  }
  // chunked pipeline: window-relative indices where the short prep chain (prep_kernels.h) takes them, and that chain wherever its word
  // layout takes the geometry; else (windows below 8 bits: tiny plain keys, window overrides) the rocPRIM sort
  TRY(chunked_geom(gc, geom_key(bases), base_off, n, group_shift, &g, short_prep_out));
  sl->geom = g;
  const u32 max_items = g.n_chunks + g.B + 1;
  TRY(ensure(sl->vals_a, (size_t)g.E * 4 + 64));
  TRY(ensure(sl->vals_b, (size_t)g.E * 4 + 64));  // read in groups of 4 entries
  TRY(ensure(sl->start, (size_t)(g.B + 2) * 4));
  TRY(ensure(sl->items, (size_t)(g.B + 2) * 4));
  TRY(ensure(sl->item_off, (size_t)(g.B + 2) * 4));
  TRY(ensure(sl->partials, (size_t)max_items * rec));
  TRY(common());
  TRY(ensure(sl->heavy, (size_t)(g.B + 1) * 4));
  // at most max_items / K1 buckets can hold more than K1 partials each
  TRY(ensure(sl->heavy_scratch, ((size_t)max_items / std::max<u32>(g.K1, 1u) + 2) * accum_l2_slices<Fq>() * rec));
  // 16 flag words (scalar-range error, heavy-bucket count) lead the short chain's block of small arrays, so that ONE fill clears both
  if (*short_prep_out) {
    TRY(ensure(sl->prep_small, prep_small_bytes(g)));
  } else {  // only the rocPRIM chain sorts (key, value) pairs
    TRY(ensure(sl->misc, 64));
    TRY(ensure(sl->keys_a, (size_t)g.E * 4));
    TRY(ensure(sl->keys_b, (size_t)g.E * 4));
  }
  return AMSM_OK;
}

// a bucket-per-lane MSM whose prep found a skewed digit distribution: the same MSM through the chunked pipeline over the
// key's 17-bit-window twin (msm_collect calls this through Slot::rerun)
template <class Fq, class Fr>
int msm_rerun_chunked(amsm_ctx* ctx, Slot* sl);

// nv <= DS_BATCH direct sums over one key in ONE launch (the provers' batched commits: eight per r1cs_nark prove) -- the slot then
// carries nv results, msm_collect hands them out as nv "groups" of one record each.  nv = 1: a single MSM, plain or grouped.
template <class Fq, class Fr>
int msm_enqueue_direct_batch(amsm_ctx* ctx, Slot* sl, const MsmJob* jobs, size_t nv, Place place) {
  DirectPlan dp;
  TRY(direct_plan<Fq>(ctx, sl, jobs, nv, &dp));
  const MsmGeom g = sl->geom;
  const amsm_bases* bases = jobs[0].key;
  sl->job = jobs[0];
  sl->unit_nv = 0;
  sl->rerun = &msm_rerun_chunked<Fq, Fr>;
  // inside a batch the launches alternate between the two streams every caller has ordered behind the scalars' producers (the
  // caller's and the prep stream: prep_fork, the host-slice uploads): a sum kernel fills one wave per SIMD, two run side by side
  hipStream_t st = (place != Place::LONE && (ctx->direct_rr++ & 1u)) ? ctx->s_prep : ctx->stream;
  u32* d_err = (u32*)sl->ds_flags.p;
  for (int i = ST_DIGITS; i <= ST_ACCUM_L0; i++) stage_mark(ctx, sl, i, st);
  if (ctx->profiling) (void)hipEventRecord(sl->ev_prep_end, st);
  const u32* sp[DS_BATCH];
  u32 n32[DS_BATCH], o32[DS_BATCH];
  for (size_t v = 0; v < nv; v++) {
    sp[v] = (const u32*)jobs[v].scalars;
    n32[v] = (u32)jobs[v].n;
    o32[v] = (u32)jobs[v].off;
  }
  launch_direct_sum<Fq>(st, (const u32*)bases->d_small, (u32)bases->n, (u32)nv, sp, n32, o32, jobs[0].mont, dp.m, jobs[0].group_shift, d_err,
                        (u32*)sl->red_out.p);
  if (ctx->profiling) {
    (void)hipEventRecord(sl->ev_l0_end, st);
    (void)hipEventRecord(sl->ev[ST_ACCUM_L12], st);
    (void)hipEventRecord(sl->ev[ST_REDUCE], st);
  }
  launch_fold<Fq>(st, true, g.n_sets, (const u32*)sl->red_out.p, dp.blocks, (u32*)sl->fold_out.p, d_err, (u32*)sl->h_pinned, true);
  if (ctx->profiling) (void)hipEventRecord(sl->ev[ST_COUNT], st);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(sl->done, st));
  sl->tail = st;
  sl->busy = true;
  ctx->n_direct += nv;
  return AMSM_OK;
}

// Enqueue the whole pipeline for one MSM on slot `sl` (asynchronous); leaves n_sets folded XYZZ records
// in sl->fold_out and queues their D2H into sl->h_pinned.
template <class Fq, class Fr>
int msm_enqueue(amsm_ctx* ctx, Slot* sl, const MsmJob& job, Place place) {
  const bool exposed_tail = place != Place::BATCH_INNER;  // nothing is queued behind this MSM: the caller waits for its tail
  if (direct_sum_applies(ctx, job)) return msm_enqueue_direct_batch<Fq, Fr>(ctx, sl, &job, 1, place);
  bool short_prep = false;
  const amsm_bases* bases = nullptr;  // the key the MSM runs over: job.key or its 17-bit twin
  TRY(msm_plan<Fq>(ctx, sl, job, &short_prep, &bases));
  sl->geom.skip_ones = job.skip_ones ? 1u : 0u;  // (msm_multi_split_xyzz: this vector's unit scalars are summed apart)
  const MsmGeom g = sl->geom;
  const void* d_scalars = job.scalars;
  const int scalars_mont = job.mont;
  const msel::TailPlan tp = tail_plan_of(g, place);  // the form of the tail, its grids and what msm_plan reserved for it (msm_select.h)
  // one range of a longer MSM over ONE bucket set (struct Share): the caller made the decision with bpl_geom, as msm_plan did
  const Share share = job.share;
  const bool shared = share.buf >= 0;
  if (shared && !(g.bpl == 1u && g.groups == 1u && g.precomp && g.n_sets == 1u)) return AMSM_E_INVALID_ARG;
  u32* d_buckets = shared ? (u32*)ctx->shared_buckets[share.buf].p : (u32*)sl->buckets.p;
  sl->job = job;
  sl->unit_nv = 0;
  sl->share_overflow = false;
  sl->rerun = &msm_rerun_chunked<Fq, Fr>;
  // alone: the only MSM of a blocking call.  Nothing can overlap, and every hand-over between streams (an event wait on
  // another hardware queue) costs ~10 us of idle GPU -- three of them in a chain of 0.4 ms at 2^16 (rocprofv3 timeline of an
  // IPA round, round 2): the whole chain goes on the caller's stream.
  const bool one = place == Place::LONE;
  hipStream_t st = one ? ctx->stream : ctx->s_prep;  // digits / sort / bounds
  hipStream_t sm = ctx->stream;                      // accumulate L0
  const size_t rec = xyzz_bytes<Fq>();
  u32* d_err = short_prep ? (u32*)sl->prep_small.p : (u32*)sl->misc.p;
  u32* d_heavy_count = d_err + 1;
  u32* vals_a = (u32*)sl->vals_a.p;
  u32* vals_b = (u32*)sl->vals_b.p;

  // ---- prep, on `st`: the scalars' digits sorted by bucket, by one of four chains ----
  auto prep = [&]() -> int {
    if (!short_prep) HIP_TRY(hipMemsetAsync(sl->misc.p, 0, 64, st));
    stage_mark(ctx, sl, ST_DIGITS, st);
    if (g.bpl) {
      // bucket-split pipeline (bpl == 2; small / medium MSMs): fill, histogram, scan, scatter, splitting local sort | accumulate | reduce, fold
      // bucket-per-lane pipeline (bpl == 1): fill, histogram, scan, wide scatter, transposing local sort | accumulate | reduce, fold
      PrepBplBuffers pb;
      pb.d_small = d_err + 16;
      pb.part = vals_a;
      pb.ents_t = vals_b;
      pb.grp = sl->bpl_grp.p;
      pb.order = (u32*)sl->bpl_order.p;
      pb.err = d_err;
      const int rc = g.bpl == 2 ? launch_prep_bps<Fr>(st, (const u32*)d_scalars, scalars_mont, g, g.bps_log2_l, pb)
                                : launch_prep_bpl<Fr>(st, (const u32*)d_scalars, scalars_mont, g, pb);
      if (rc != 0) return AMSM_E_HIP;
      stage_mark(ctx, sl, ST_SORT, st);
      stage_mark(ctx, sl, ST_BOUNDS, st);
      if (g.bpl != 2) ctx->n_bpl++;
      else if (!job.counted) ctx->n_bps++;  // (a unit's MSM run again on its own was counted with its unit)
      if (g.bpl == 1u && g.top_split) ctx->n_top_sets[(g.top_split + 1u) / 4u]++;  // (a plain key: amsm_ctx_top_sets_msms)
    } else if (short_prep) {
      // short prep chain (prep_kernels.h: 5 dispatches + 2 for skewed inputs); the stage marks keep their names: "sort" = scatter + local sort
      PrepBuffers pb;
      pb.d_small = d_err + 16;
      pb.part = vals_a;
      pb.vals_sorted = vals_b;
      pb.start = (u32*)sl->start.p;
      pb.items = (u32*)sl->items.p;
      pb.item_off = (u32*)sl->item_off.p;
      pb.err = d_err;
      if (launch_prep<Fr>(st, (const u32*)d_scalars, scalars_mont, g, pb) != 0) return AMSM_E_HIP;
      stage_mark(ctx, sl, ST_SORT, st);
      stage_mark(ctx, sl, ST_BOUNDS, st);
    } else {
      TRY(ensure(sl->keys_a, (size_t)g.E * 4));  // only the rocPRIM chain sorts (key, value) pairs
      TRY(ensure(sl->keys_b, (size_t)g.E * 4));
      u32* keys_a = (u32*)sl->keys_a.p;
      u32* keys_b = (u32*)sl->keys_b.p;
      const bool keys16 = g.B < 65536u;  // every key (incl. the "digit 0" key B) fits 16 bits
      launch_digits<Fr>(st, (const u32*)d_scalars, scalars_mont, g, keys_a, keys16, vals_a, d_err);
      stage_mark(ctx, sl, ST_SORT, st);
      {
        int bits = 1;
        while ((1u << bits) <= g.B) bits++;
        size_t tmp = 0;
        if (keys16) {
          uint16_t* ka = (uint16_t*)keys_a;
          uint16_t* kb = (uint16_t*)keys_b;
          HIP_TRY(rocprim::radix_sort_pairs(nullptr, tmp, ka, kb, vals_a, vals_b, (size_t)g.E, 0u, (unsigned)bits, st));
          TRY(ensure(sl->sort_tmp, tmp));
          tmp = sl->sort_tmp.bytes;
          HIP_TRY(rocprim::radix_sort_pairs(sl->sort_tmp.p, tmp, ka, kb, vals_a, vals_b, (size_t)g.E, 0u, (unsigned)bits, st));
        } else {
          HIP_TRY(rocprim::radix_sort_pairs(nullptr, tmp, keys_a, keys_b, vals_a, vals_b, (size_t)g.E, 0u, (unsigned)bits, st));
          TRY(ensure(sl->sort_tmp, tmp));
          tmp = sl->sort_tmp.bytes;
          HIP_TRY(rocprim::radix_sort_pairs(sl->sort_tmp.p, tmp, keys_a, keys_b, vals_a, vals_b, (size_t)g.E, 0u, (unsigned)bits, st));
        }
      }
      stage_mark(ctx, sl, ST_BOUNDS, st);
      launch_bounds(st, (const void*)keys_b, keys16, vals_b, g, (u32*)sl->start.p, (u32*)sl->items.p);
      {
        size_t tmp = 0;
        HIP_TRY(rocprim::exclusive_scan(nullptr, tmp, (u32*)sl->items.p, (u32*)sl->item_off.p, 0u, (size_t)(g.B + 1),
                                        rocprim::plus<u32>(), st));
        TRY(ensure(sl->scan_tmp, tmp));
        tmp = sl->scan_tmp.bytes;
        HIP_TRY(rocprim::exclusive_scan(sl->scan_tmp.p, tmp, (u32*)sl->items.p, (u32*)sl->item_off.p, 0u, (size_t)(g.B + 1),
                                        rocprim::plus<u32>(), st));
      }
      AMSM_DBG("pre-l0");
    }
    if (ctx->profiling) (void)hipEventRecord(sl->ev_prep_end, st);
    return AMSM_OK;
  };

  // ---- accumulate, on `sm` behind the prep: the sorted entries' points into buckets (or into partial records: the chunked pipeline) ----
  auto accumulate = [&]() -> int {
    if (!one) {
      HIP_TRY(hipEventRecord(sl->prep_done, st));
      HIP_TRY(hipStreamWaitEvent(sm, sl->prep_done, 0));
    }
    if (shared && share.first && ctx->shared_used[share.buf])  // the previous user's tail may still be reading the table
      HIP_TRY(hipStreamWaitEvent(sm, ctx->shared_free[share.buf], 0));
    stage_mark(ctx, sl, ST_ACCUM_L0, sm);
    if (g.bpl == 2) {
      launch_accum_bps<Fq>(sm, (const u32*)bases->d_table, (const u32*)vals_b, sl->bpl_grp.p, (const u32*)sl->bpl_order.p,
                           prep_bps_partitions(g, g.bps_log2_l) * 16u, g.bps_log2_l, d_err, (u32*)sl->buckets.p);
    } else if (g.bpl) {
      const u32 n_grp = prep_bpl_partitions(g) * prep_bpl_groups_per_partition(), n_wg = cdiv(n_grp, 4u), cus = (u32)std::max(1, ctx->cu_count);
      // few workgroups: spread them over all CUs (launch_accum_bpl) -- one per CU up to 1.25 CUs' worth, two up to 2.5
      const u32 per_cu = n_wg * 4u <= cus * 5u ? 1u : (n_wg * 2u <= cus * 5u ? 2u : 0u);
      launch_accum_bpl<Fq>(sm, (const u32*)bases->d_table, (const u32*)vals_b, sl->bpl_grp.p, (const u32*)sl->bpl_order.p, n_grp,
                           prep_bpl_groups_per_partition(), d_err, d_buckets, per_cu, shared && !share.first);
    } else {
      launch_accum_l0<Fq>(sm, (const u32*)bases->d_table, (const u32*)vals_b, (const u32*)sl->start.p, (const u32*)sl->item_off.p, g,
                          (u32*)sl->partials.p);
    }
    AMSM_DBG("l0");
    if (ctx->profiling) (void)hipEventRecord(sl->ev_l0_end, sm);
    return AMSM_OK;
  };

  // ---- tail: partial records into buckets (chunked pipeline only), then the bucket reduction, the fold and the export as tail_plan chose
  // them; the records and the flag words go straight to the slot's page-locked block (msm_kernels.h: emit_record's mirror): no copy
  // command between the fold and the slot's `done` event ----
  auto tail = [&]() -> int {
    // The tail the caller waits for -- a blocking call's, or the LAST MSM's of a batch -- stays on the caller's stream, behind its own
    // accumulation: on the tail stream it would queue behind the previous MSM's tail, which runs beside this accumulation and takes
    // 2-3x its stand-alone time (rocprofv3, a prover's batch of two 2^18-pair MSMs: the second tail started 127 us after its
    // accumulation had ended; 1.30 ms for the batch).
    hipStream_t tl = exposed_tail ? ctx->stream : ctx->s_tail;
    sl->tail = tl;
    if (tl != sm) {
      HIP_TRY(hipEventRecord(sl->l0_done, sm));
      HIP_TRY(hipStreamWaitEvent(tl, sl->l0_done, 0));
    }
    if (ctx->profiling) (void)hipEventRecord(sl->ev[ST_ACCUM_L12], tl);
    if (!g.bpl) {  // the bucket-per-lane accumulation leaves finished buckets: no partial records to fold
      launch_accum_l1<Fq>(tl, l1_lanes(g, !tp.quad), (const u32*)sl->partials.p, (const u32*)sl->items.p, (const u32*)sl->item_off.p, g,
                          (u32*)sl->buckets.p, d_heavy_count, (u32*)sl->heavy.p);
      AMSM_DBG("l1");
      launch_accum_l2<Fq>(tl, (const u32*)sl->partials.p, (const u32*)sl->items.p, (const u32*)sl->item_off.p, (const u32*)d_heavy_count,
                          (const u32*)sl->heavy.p, (u32*)sl->heavy_scratch.p, (u32*)sl->buckets.p);
      AMSM_DBG("l2");
    }
    if (ctx->profiling) (void)hipEventRecord(sl->ev[ST_REDUCE], tl);
    launch_tail<Fq>(tl, tp, (const u32*)d_buckets, g, (u32*)sl->red2_rc.p, (u32*)sl->red_out.p, (u32*)sl->red_ticket.p, (u32*)sl->fold_out.p,
                    d_err, (u32*)sl->h_pinned);
    if (amsm_debug()) {
      char stage[32];
      snprintf(stage, sizeof(stage), "tail %s", msel::tail_form_name(tp.form));
      AMSM_DBG(stage);
    }
    if (ctx->profiling) (void)hipEventRecord(sl->ev[ST_COUNT], tl);
    HIP_TRY(hipGetLastError());
    if (shared) {  // the table may be rewritten once this tail has read it
      HIP_TRY(hipEventRecord(ctx->shared_free[share.buf], tl));
      ctx->shared_used[share.buf] = true;
    }
    HIP_TRY(hipEventRecord(sl->done, tl));
    return AMSM_OK;
  };

  TRY(prep());
  TRY(accumulate());
  if (shared && !share.last) {
    // its sums stay in the shared table: no tail.  The slot's flag words reach the host behind the accumulation (the place
    // msm_collect reads them: behind the slot's n_sets records)
    if (ctx->profiling)
      for (int i = ST_ACCUM_L12; i <= ST_COUNT; i++) (void)hipEventRecord(sl->ev[i], sm);
    launch_mirror_flags(sm, d_err, (u32*)((char*)sl->h_pinned + g.n_sets * rec));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(sl->done, sm));
    sl->tail = sm;
  } else {
    TRY(tail());
  }
  sl->busy = true;
  return AMSM_OK;
}

// ---- a unit of bucket-split MSMs: one launch per pipeline stage (msm_select.h: batch_units; DESIGN.md 4.2h) ----
// What msm_multi_xyzz found when it formed the unit (msm_jobs.h: plan_units, once per run of jobs): ONE MSM's geometry, shared by all of the
// unit's MSMs (skip_ones set), and the key they run over (a 20-bit key's twin)
struct BpsUnitGeom {
  MsmGeom g = {};
  const amsm_bases* eff = nullptr;
};
// EVERY allocation of a unit of nv MSMs of geometry g on slot `sl` (the counterpart of direct_plan): nothing is launched.
// AMSM_E_OOM: the caller runs the unit's MSMs singly.
struct BpsBatchPlan {
  BpsBatchBuffers buf;
};
template <class Fq>
int bps_batch_plan(amsm_ctx* ctx, Slot* sl, const MsmGeom& g, size_t nv, BpsBatchPlan* out) {
  if (nv < 2 || nv > (size_t)msel::BPS_BATCH || g.bpl != 2u || g.n_sets != 1u || g.S > 16u) return AMSM_E_INVALID_ARG;
  const size_t rec = xyzz_bytes<Fq>();
  const PrepNeeds nd = prep_bps_needs(g);
  BpsBatchBuffers& b = out->buf;
  // MSM v's share of every buffer: what msm_plan gives a single MSM (the 64 bytes of slack included), v strides in
  b.small_stride = prep_bps_small_block_words();
  b.part_stride = (u32)(nd.vals_a / 4);    // words
  b.ents_stride = (u32)(nd.vals_b / 4);    // words
  b.grp_stride = (u32)(nd.bpl_grp / 8);    // headers
  b.order_stride = (u32)(nd.bpl_order / 4);  // words
  if (nd.vals_b / 4 >= ((size_t)1 << 31)) return AMSM_E_INVALID_ARG;
  TRY(ensure(sl->vals_a, nv * (size_t)b.part_stride * 4));
  TRY(ensure(sl->vals_b, nv * (size_t)b.ents_stride * 4));
  TRY(ensure(sl->bpl_grp, nv * (size_t)b.grp_stride * 8));
  TRY(ensure(sl->bpl_order, nv * (size_t)b.order_stride * 4));
  TRY(ensure(sl->buckets, nv * (size_t)g.B * rec));
  TRY(ensure(sl->prep_small, nv * (size_t)b.small_stride * 4 + 256));
  TRY(reserve_tail<Fq>(ctx, sl, (size_t)g.n_sets * nv, msel::tail_plan_any_place(g.nb, g.n_sets * (u32)nv, g.B * (u32)nv, g.E * (u32)nv, false)));
  b.small = (u32*)sl->prep_small.p;
  b.part = (u32*)sl->vals_a.p;
  b.ents_t = (u32*)sl->vals_b.p;
  b.grp = sl->bpl_grp.p;
  b.order = (u32*)sl->bpl_order.p;
  return AMSM_OK;
}
template <class Fq, class Fr>
int msm_rerun_unit(amsm_ctx* ctx, Slot* sl, void* out);
// nv = 2 .. BPS_BATCH bucket-split MSMs that share key, range and scalar form (msm_select.h: batch_units) as FIVE commands: one fill,
// scatter, local sort and accumulation with grid.y = MSM, one tail over the unit's nv bucket sets -- instead of five per MSM.  The
// slot then carries nv results; msm_collect hands them out as nv "groups" of one record each, as for a batch of direct sums.
// One pair of flag words for the unit: a scalar out of range fails the call, an overflowing prep sends ALL nv MSMs through the single
// path again, one by one (msm_rerun_unit), each with its own chunked fallback.
template <class Fq, class Fr>
int msm_enqueue_bps_batch(amsm_ctx* ctx, Slot* sl, const MsmJob* jobs, size_t nv, const BpsUnitGeom& found, Place place) {
  BpsBatchPlan bp;
  const amsm_bases* bases = found.eff;
  if (!bases) return AMSM_E_INVALID_ARG;
  const MsmGeom g = found.g;
  TRY(bps_batch_plan<Fq>(ctx, sl, g, nv, &bp));
  const MsmGeom ug = bps_unit_geom(g, (u32)nv);
  const msel::TailPlan tp = bps_unit_tail(g, (u32)nv, place);
  sl->geom = ug;
  sl->job = jobs[0];
  sl->share_overflow = false;
  sl->rerun = &msm_rerun_chunked<Fq, Fr>;
  sl->rerun_unit = &msm_rerun_unit<Fq, Fr>;
  for (size_t v = 0; v < nv; v++) sl->unit_jobs[v] = jobs[v];
  sl->unit_nv = (u32)nv;
  // LONE: the whole call is this unit (the provers' 2 .. 8 commits): one stream, no hand-overs.  Inside a longer call: the stages on
  // their streams, as msm_enqueue places them
  const bool one = place == Place::LONE;
  hipStream_t st = one ? ctx->stream : ctx->s_prep, sm = ctx->stream;
  hipStream_t tl = place != Place::BATCH_INNER ? ctx->stream : ctx->s_tail;
  u32* d_err = bp.buf.small;
  const u32* sp[msel::BPS_BATCH];
  for (size_t v = 0; v < nv; v++) sp[v] = (const u32*)jobs[v].scalars;
  stage_mark(ctx, sl, ST_DIGITS, st);
  if (launch_prep_bps_batch<Fr>(st, sp, (u32)nv, jobs[0].mont, g, g.bps_log2_l, bp.buf) != 0) return AMSM_E_HIP;
  stage_mark(ctx, sl, ST_SORT, st);
  stage_mark(ctx, sl, ST_BOUNDS, st);
  if (ctx->profiling) (void)hipEventRecord(sl->ev_prep_end, st);
  AMSM_DBG("unit prep");
  if (!one) {
    HIP_TRY(hipEventRecord(sl->prep_done, st));
    HIP_TRY(hipStreamWaitEvent(sm, sl->prep_done, 0));
  }
  stage_mark(ctx, sl, ST_ACCUM_L0, sm);
  launch_accum_bps_batch<Fq>(sm, (const u32*)bases->d_table, bp.buf, (u32)nv, prep_bps_partitions(g, g.bps_log2_l) * 16u, g.bps_log2_l, g.B,
                             (u32*)sl->buckets.p);
  AMSM_DBG("unit accumulate");
  if (ctx->profiling) (void)hipEventRecord(sl->ev_l0_end, sm);
  sl->tail = tl;
  if (tl != sm) {
    HIP_TRY(hipEventRecord(sl->l0_done, sm));
    HIP_TRY(hipStreamWaitEvent(tl, sl->l0_done, 0));
  }
  if (ctx->profiling) {
    (void)hipEventRecord(sl->ev[ST_ACCUM_L12], tl);
    (void)hipEventRecord(sl->ev[ST_REDUCE], tl);
  }
  launch_tail<Fq>(tl, tp, (const u32*)sl->buckets.p, ug, (u32*)sl->red2_rc.p, (u32*)sl->red_out.p, (u32*)sl->red_ticket.p, (u32*)sl->fold_out.p,
                  d_err, (u32*)sl->h_pinned);
  AMSM_DBG("unit tail");
  if (ctx->profiling) (void)hipEventRecord(sl->ev[ST_COUNT], tl);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(sl->done, tl));
  sl->busy = true;
  ctx->n_bps += nv;  // each MSM once, when it is first put on the pipeline
  ctx->n_bps_batched += nv;
  ctx->n_bps_units++;
  return AMSM_OK;
}

// Wait for slot `sl`, then host Horner over the window sums (plain key) -> one XYZZ per group on the host
// (`out` has room for sl->geom.groups results).
template <class Fq>
int msm_collect(amsm_ctx* ctx, Slot* sl, host::HXYZZ<Fq>* out) {
  const MsmGeom& g = sl->geom;
  size_t rec = xyzz_bytes<Fq>();
  sl->busy = false;  // (whatever comes of the wait: a slot whose event cannot be waited for has nothing left to collect)
  HIP_TRY(hipEventSynchronize(sl->done));
  if (ctx->profiling) {
    for (int s = 0; s < ST_COUNT; s++) {
      float ms = 0;
      // a stage ends on its own stream: the next stage's begin mark sits on another stream for prep -> L0 -> tail, and
      // would add that stream's queueing (the tail stream is still busy with the previous MSM inside a batch)
      hipEvent_t end = s == ST_BOUNDS ? sl->ev_prep_end : (s == ST_ACCUM_L0 ? sl->ev_l0_end : sl->ev[s + 1]);
      (void)hipEventElapsedTime(&ms, sl->ev[s], end);
      ctx->stage_acc[s] += ms;
    }
    ctx->stage_n++;
  }
  u32* h = (u32*)sl->h_pinned;
  u32 err = *(u32*)((char*)h + g.n_sets * rec);
  if (err) return AMSM_E_SCALAR_RANGE;
  if (sl->job.share.buf >= 0) {  // one range of a shared MSM: only the last one carries the sum; skew is the CALLER's to handle
    if (*(u32*)((char*)h + g.n_sets * rec + 4)) sl->share_overflow = true;
    if (!sl->job.share.last || sl->share_overflow) {
      out[0] = host::hx_inf<Fq>();
      return AMSM_OK;
    }
  } else if (g.bpl && *(u32*)((char*)h + g.n_sets * rec + 4)) {  // the prep's overflow flag: skewed digits (SURVEY.md F8)
    // a unit shares one flag word: which of its preps overflowed is not known -- every MSM again on its own, each with its own fallback
    if (sl->unit_nv) return sl->rerun_unit(ctx, sl, out);
    if (g.bpl == 2) ctx->n_bps_fallbacks++;
    else ctx->n_bpl_fallbacks++;
    TRY(sl->rerun(ctx, sl));
    return msm_collect<Fq>(ctx, sl, out);  // the re-run is chunked: no second fallback
  } else if (!g.bpl) {
    // the chunked pipeline's second flag word is k_accum_l1's count of heavy buckets (a direct sum leaves it zero): amsm_ctx_heavy_buckets
    ctx->n_heavy_buckets += *(u32*)((char*)h + g.n_sets * rec + 4);
  }
  // one result per group: Horner over the group's window sums (plain key) or its single record (precomputed key)
  const u32 sets = g.n_sets / g.groups, per = sets - g.top_split;  // per = windows (the top one owns 1 + top_split sets)
  auto horner = [&](size_t grp) {
    const u32* base = h + grp * sets * (rec / 4);
    host::HXYZZ<Fq> acc = host::hx_from_device<Fq>(base + (size_t)(per - 1) * (rec / 4));
    // the top window's other sets (an empty set's record is the identity)
    for (u32 k = 0; k < g.top_split; k++) acc = host::hx_add<Fq>(acc, host::hx_from_device<Fq>(base + (size_t)(per + k) * (rec / 4)));
    for (int w = (int)per - 2; w >= 0; w--) {
      // window w's sum counts 2^(e_w): c doublings between equal windows, c - 1 where a narrow one is involved (n_narrow)
      const u32 dbl = per > 1u ? window_exponent(g, (u32)w + 1u) - window_exponent(g, (u32)w) : 0u;
      for (u32 k = 0; k < dbl; k++) acc = host::hx_dbl<Fq>(acc);
      acc = host::hx_add<Fq>(acc, host::hx_from_device<Fq>(base + (size_t)w * (rec / 4)));
    }
    out[grp] = acc;
  };
  // the two groups of a grouped MSM over a PLAIN key (the IPA rounds behind the physical folds) are ~250 host doublings each:
  // side by side on the host pool
  if (g.groups > 1u && per > 4u) HostPool::get().run(g.groups, horner);
  else
    for (u32 grp = 0; grp < g.groups; grp++) horner(grp);
  return AMSM_OK;
}

template <class Fq, class Fr>
int msm_rerun_chunked(amsm_ctx* ctx, Slot* sl) {
  // the same MSM with the chunked pipeline forced: over the key itself, or over its 17-bit twin when the key was precomputed
  // for 20-bit windows (msm_plan resolves that).  On the per-stage streams (not Place::LONE): other MSMs of a batch may be in
  // flight, and the prep stream has already been ordered behind the producers of the scalars by the call's prep_fork.
  MsmJob j = sl->job;
  j.force_chunked = true;
  j.share = Share();
  return msm_enqueue<Fq, Fr>(ctx, sl, j, Place::BATCH_LAST);
}

// A unit one of whose preps overflowed (msm_collect): its MSMs one after the other through the single path on the same slot, on the
// per-stage streams like any re-run.  Each was counted when the unit was enqueued (MsmJob::counted); the ones whose own prep
// overflows again fall back to the chunked pipeline there and are counted as fallbacks, once.  The result does not depend on the path.
template <class Fq, class Fr>
int msm_rerun_unit(amsm_ctx* ctx, Slot* sl, void* out) {
  host::HXYZZ<Fq>* res = (host::HXYZZ<Fq>*)out;
  const u32 nv = sl->unit_nv;
  MsmJob jobs[msel::BPS_BATCH];
  for (u32 v = 0; v < nv; v++) jobs[v] = sl->unit_jobs[v];  // (msm_enqueue rewrites the slot's description)
  sl->unit_nv = 0;
  ctx->n_bps_unit_reruns++;
  for (u32 v = 0; v < nv; v++) {
    jobs[v].counted = true;
    TRY((msm_enqueue<Fq, Fr>(ctx, sl, jobs[v], Place::BATCH_LAST)));
    TRY(msm_collect<Fq>(ctx, sl, &res[v]));
  }
  return AMSM_OK;
}

void stage_begin(amsm_ctx* ctx) {
  for (int s = 0; s < ST_COUNT; s++) ctx->stage_acc[s] = 0;
  ctx->stage_n = 0;
}
void stage_end(amsm_ctx* ctx) {
  if (!ctx->stage_n) return;
  for (int s = 0; s < ST_COUNT; s++) ctx->stage_ms[s] = ctx->stage_acc[s] / ctx->stage_n;
}

// The slot ring every batch of MSMs runs through, N_SLOTS in flight on the per-stage streams.  Items 0 .. n - 1 (an empty MSM is no
// item: it takes no slot) go in order, item i to slot i % N_SLOTS, whose previous item is collected first; the rest are drained in
// enqueue order.  enqueue(i, sl) queues item i on slot sl, collect(i, sl) reads it back (msm_collect); overflow[i] (if given) is set
// when item i, one range of a shared bucket set, found skewed digits (its whole MSM is the caller's to re-run).  The call's one
// prep_fork comes before the first enqueue.  Every way out leaves all slots idle: after an error the busy slots are still drained and
// the first error is returned, and a slot found busy on entry is refused -- no item of this call owns it.
template <class Enqueue, class Collect>
int run_ring(amsm_ctx* ctx, size_t n, Enqueue&& enqueue, Collect&& collect, uint8_t* overflow = nullptr) {
  for (const Slot& sl : ctx->slot)
    if (sl.busy) return AMSM_E_INVALID_ARG;
  stage_begin(ctx);
  TRY(prep_fork(ctx));
  size_t owner[N_SLOTS] = {};  // the item a busy slot carries
  auto take = [&](size_t s) -> int {
    Slot* sl = &ctx->slot[s];
    const int r = collect(owner[s], sl);
    if (overflow && sl->share_overflow) overflow[owner[s]] = 1;
    sl->share_overflow = false;
    return r;
  };
  int rc = AMSM_OK;
  size_t i = 0;
  for (; i < n && rc == AMSM_OK; i++) {
    const size_t s = i % N_SLOTS;
    if (ctx->slot[s].busy) rc = take(s);
    if (rc != AMSM_OK) break;
    rc = enqueue(i, &ctx->slot[s]);
    owner[s] = i;
  }
  for (size_t t = 0; t < N_SLOTS; t++) {  // drain in enqueue order
    const size_t s = (i + t) % N_SLOTS;
    if (ctx->slot[s].busy) {
      const int r2 = take(s);
      if (rc == AMSM_OK) rc = r2;
    }
  }
  stage_end(ctx);
  return rc;
}

// Ranges jobs[first, first + count) of one MSM over ONE bucket set (struct Share): the context's next set -- consecutive long MSMs
// alternate between its two, so both are grown here --, the first range writes it, the last one carries the tail
template <class Fq>
int arm_shared_set(amsm_ctx* ctx, std::vector<MsmJob>& jobs, size_t first, size_t count, size_t buckets) {
  const int buf = (int)(ctx->shared_rr++ & 1u);
  for (int b = 0; b < 2; b++) {
    TRY(ensure(ctx->shared_buckets[b], buckets * xyzz_bytes<Fq>()));
    if (!ctx->shared_free[b]) HIP_TRY(hipEventCreateWithFlags(&ctx->shared_free[b], hipEventDisableTiming));
  }
  for (size_t j = 0; j < count; j++) {
    jobs[first + j].share.buf = buf;
    jobs[first + j].share.first = j == 0;
    jobs[first + j].share.last = j + 1 == count;
  }
  ctx->n_shared++;
  return AMSM_OK;
}

template <class Fq, class Fr>
int msm_multi_split_xyzz(amsm_ctx* ctx, const std::vector<MsmJob>& vecs, std::vector<host::HXYZZ<Fq>>* out);
// Large MSMs run as ranges of the key (msm_jobs.h)
inline bool split_needed(const amsm_ctx* ctx, const amsm_bases* bases, size_t n) { return mjobs::split_needed(switches_of(ctx), key_desc(bases), n); }

// Which of the k device vectors would overflow the bucket-per-lane prep (vec_kernels.h: k_skew_probe)?  One tiny launch per
// candidate on the caller's stream (behind the kernels that produce the vectors), one copy, one synchronisation per CALL.
struct SkewProbe {  // launched, not yet read back
  std::vector<size_t> cand, first;
  size_t k = 0;
};
// Identical vectors are probed once (msm_jobs.h: first_identical): first[j] is an index into cand
inline std::vector<size_t> first_identical(const std::vector<MsmJob>& vecs, const std::vector<size_t>& cand) {
  std::vector<size_t> first(cand.size());
  mjobs::first_identical(cand.size(), [&](size_t j) { return mjobs::VecRef{vecs[cand[j]].scalars, vecs[cand[j]].n}; }, first.data());
  return first;
}
template <class Fr>
int bpl_probe_enqueue(amsm_ctx* ctx, const std::vector<MsmJob>& vecs, DigitWalk walk, size_t min_len, SkewProbe* p,
                      const u32* const* tv_words = nullptr) {  // tv_words[v]: vector v's two-valued probe words, if probed
  p->k = vecs.size();
  p->cand.clear();
  for (size_t v = 0; v < vecs.size(); v++)
    if (vecs[v].n >= min_len) p->cand.push_back(v);
  const std::vector<size_t>& cand = p->cand;
  if (cand.empty()) return AMSM_OK;
  TRY(ensure(ctx->probe_flags, std::max<size_t>(cand.size() * 4, 4096)));
  Slot* aux = &ctx->slot[N_SLOTS - 1];
  TRY(ensure_pinned(aux, std::max<size_t>(cand.size() * 4, 4096) + 64));
  HIP_TRY(hipMemsetAsync(ctx->probe_flags.p, 0, cand.size() * 4, ctx->stream));
  p->first = first_identical(vecs, cand);
  for (size_t j = 0; j < cand.size(); j++) {
    const MsmJob& vec = vecs[cand[j]];
    if (p->first[j] == j)
      launch_skew_probe<Fr>(ctx->stream, (const u32*)vec.scalars, vec.mont, (u32)std::min<size_t>(vec.n, 0xffffffffu), walk,
                            (u32*)ctx->probe_flags.p + j, tv_words ? tv_words[cand[j]] : nullptr);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(aux->h_pinned, ctx->probe_flags.p, cand.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
  return AMSM_OK;
}
// after the caller's stream has been synchronised
inline void bpl_probe_finish(amsm_ctx* ctx, const SkewProbe& p, std::vector<uint8_t>* skew) {
  skew->assign(p.k, 0);
  const u32* f = (const u32*)ctx->slot[N_SLOTS - 1].h_pinned;
  for (size_t j = 0; j < p.cand.size(); j++) (*skew)[p.cand[j]] = f[p.first[j]] ? 1 : 0;
}
template <class Fr>
int bpl_probe_device(amsm_ctx* ctx, const std::vector<MsmJob>& vecs, std::vector<uint8_t>* skew, DigitWalk walk, size_t min_len) {
  SkewProbe p;
  TRY(bpl_probe_enqueue<Fr>(ctx, vecs, walk, min_len, &p, nullptr));
  if (!p.cand.empty()) HIP_TRY(hipStreamSynchronize(ctx->stream));
  bpl_probe_finish(ctx, p, skew);
  return AMSM_OK;
}
// Which skew probe (if any) the pipelines behind msm_multi_split_impl want for these vectors over `bases`: 0 none, else the window
// width / the shortest vector probed.  (msm_multi_split_xyzz launches it together with the two-valued probe: one synchronisation for both.)
inline int skew_probe_params(const amsm_ctx* ctx, const amsm_bases* bases, const std::vector<MsmJob>& vecs, size_t* min_len, DigitWalk* walk) {
  const mjobs::PlanCtx pc = plan_ctx(ctx);
  const msel::KeyDesc kd = key_desc(bases);
  bool want = false;
  for (const MsmJob& v : vecs) want = want || mjobs::probe_wanted(pc, kd, v.n);
  if (!want) return 0;
  *walk = mjobs::key_walk(geom_key(bases));
  *min_len = mjobs::probe_min_len(kd);
  return bases->c;
}
// the same test on a host slice (msm_jobs.h: skew_probe_host, over the samples in canonical form)
template <class Fr>
bool bpl_probe_host(const uint64_t* scalars, size_t n, int mont, DigitWalk dw, size_t min_len) {
  return mjobs::skew_probe_host(n, min_len, dw, [&](size_t i, u32* out) {
    host::HFe<Fr> s;
    memcpy(s.v, scalars + 4 * i, 32);
    if (mont) s = host::h_from_mont<Fr>(s);
    memcpy(out, s.v, 32);
  });
}

// The callers' k vectors over windows of one key -- vector v: generators [offs[v], offs[v] + ns[v]) and the scalars at scalars[v] -- as
// a job list: one job per vector, owner = its index, lengths clamped to the key
inline int jobs_from_arrays(const amsm_bases* bases, size_t k, const size_t* offs, const void* const* scalars, const size_t* ns, int mont,
                            std::vector<MsmJob>* jobs) {
  jobs->assign(k, MsmJob());
  for (size_t v = 0; v < k; v++) {
    if (offs[v] > bases->n) return AMSM_E_INVALID_ARG;
    MsmJob& j = (*jobs)[v];
    j.owner = v;
    j.key = bases;
    j.off = offs[v];
    j.n = std::min(ns[v], bases->n - offs[v]);
    j.scalars = scalars[v];
    j.mont = mont;
  }
  return AMSM_OK;
}
// (*out)[jobs[j].owner] += part[j]
template <class Fq>
void add_by_owner(const std::vector<MsmJob>& jobs, const std::vector<host::HXYZZ<Fq>>& part, std::vector<host::HXYZZ<Fq>>* out) {
  for (size_t j = 0; j < jobs.size(); j++) (*out)[jobs[j].owner] = host::hx_add<Fq>((*out)[jobs[j].owner], part[j]);
}
// The job list of a call (msm_jobs.h: plan_ranges says how its vectors are cut, which ranges share a bucket set, which run over the
// twin) as MsmJobs: the twin is built first where a skewed vector needs it, every range inherits its vector's fields, every shared
// set gets its buffers (arm_shared_set).  skew: the probes' verdict per vector (null: none skewed)
template <class Fq>
int plan_jobs(amsm_ctx* ctx, const amsm_bases* bases, const std::vector<MsmJob>& vecs, const uint8_t* skew, const mjobs::Form& form,
              std::vector<MsmJob>* jobs) {
  std::vector<mjobs::PlanVec> pv(vecs.size());
  for (size_t v = 0; v < vecs.size(); v++) pv[v] = mjobs::PlanVec{vecs[v].off, vecs[v].n, skew && skew[v]};
  const amsm_bases* alt = nullptr;
  if (mjobs::needs_twin(job_key(bases), pv.data(), pv.size())) TRY(bases_alt<Fq>(ctx, bases, &alt));
  std::vector<mjobs::Range> plan;
  mjobs::plan_ranges(plan_ctx(ctx), job_key(bases, alt), pv.data(), pv.size(), form, &plan);
  jobs->clear();
  jobs->reserve(plan.size());
  size_t set_first = 0;
  for (const mjobs::Range& r : plan) {
    jobs->push_back(vecs[r.vec]);
    MsmJob& j = jobs->back();
    j.owner = r.vec;  // the vector's place in `vecs`
    j.key = r.over_twin ? alt : bases;
    j.force_chunked = r.force_chunked;
    j.off += r.lo;
    j.n = r.n;
    j.scalars = (const char*)j.scalars + r.lo * 32;
    if (r.first) set_first = jobs->size() - 1;
    if (r.last) TRY(arm_shared_set<Fq>(ctx, *jobs, set_first, jobs->size() - set_first, r.set_buckets));
  }
  return AMSM_OK;
}

// The jobs' MSMs through the slot ring; (*part)[j] = job j's result (the identity for an empty job, and for every range of a shared
// bucket set but its last), (*overflow)[j] = 1 where job j, a range of a shared set, found skewed digits (run_ring)
template <class Fq, class Fr>
int msm_multi_xyzz(amsm_ctx* ctx, const std::vector<MsmJob>& jobs, std::vector<host::HXYZZ<Fq>>* part, std::vector<uint8_t>* overflow = nullptr) {
  const size_t k = jobs.size();
  part->assign(k, host::hx_inf<Fq>());
  if (overflow) overflow->assign(k, 0);
  if (k == 0) return AMSM_OK;
  // every MSM a direct sum over this key (small keys: DESIGN.md 4.2g): up to DS_BATCH of them per launch
  const amsm_bases* key = jobs[0].key;
  bool all_direct = k >= 2;
  for (const MsmJob& j : jobs) all_direct = all_direct && j.key == key && j.mont == jobs[0].mont && j.group_shift < 0 && direct_sum_applies(ctx, j);
  if (all_direct) {
    const size_t n_launches = (k + DS_BATCH - 1) / DS_BATCH;
    return run_ring(
        ctx, n_launches,
        [&](size_t b, Slot* sl) {
          const size_t v0 = b * DS_BATCH;
          return msm_enqueue_direct_batch<Fq, Fr>(ctx, sl, &jobs[v0], std::min<size_t>(DS_BATCH, k - v0), place_of(b, n_launches));
        },
        [&](size_t b, Slot* sl) { return msm_collect<Fq>(ctx, sl, &(*part)[b * DS_BATCH]); });
  }
  std::vector<size_t> live;  // the non-empty jobs; the last one's tail is the only one the caller waits for
  for (size_t j = 0; j < k; j++)
    if (jobs[j].n) live.push_back(j);
  // The ring runs over UNITS (msm_select.h: batch_units): a live job on today's path, or 2 .. BPS_BATCH consecutive bucket-split
  // MSMs that differ in their scalars only, one launch per pipeline stage (msm_enqueue_bps_batch).  Every caller that ends here
  // inherits the batching; a call of one job, or with the switch off, never looks at a geometry.
  std::vector<msel::Unit> units(live.size());
  size_t n_units = live.size();
  std::vector<MsmJob> ujobs;  // the live jobs in order (a unit's are adjacent in memory)
  std::vector<mjobs::UnitGeom> ugeom;  // per live job: the geometry its unit would run with (msm_jobs.h: plan_units)
  std::vector<mjobs::UnitJob> uj;
  std::vector<mjobs::JobKey> keys;          // the keys the live jobs name (one; or a 20-bit key and, for its skewed vectors, the twin)
  std::vector<const amsm_bases*> twin;      // ... and their twins, where plan_units will look at a job over a 20-bit key
  if (live.size() >= 2 && ctx->bps_batch >= 2) {
    const mjobs::PlanCtx pc = plan_ctx(ctx);
    ugeom.resize(live.size());
    uj.resize(live.size());
    for (size_t i = 0; i < live.size(); i++) {
      const MsmJob& j = jobs[live[i]];
      size_t ki = 0;
      while (ki < keys.size() && keys[ki].id != j.key) ki++;
      if (ki == keys.size()) {
        keys.push_back(job_key(j.key));
        twin.push_back(nullptr);
      }
      uj[i] = mjobs::UnitJob{ki, j.off, j.n, j.mont, j.group_shift, j.share.buf >= 0, j.force_chunked, j.skip_ones};
    }
    // the key a unit's MSMs would run over: a 20-bit key's twin, built on first use -- asked for once per key (one that cannot be
    // had is the single path's to report: the jobs then stay singles)
    for (size_t ki = 0; ki < keys.size(); ki++)
      if (mjobs::units_need_twin(pc, keys[ki], ki, uj.data(), uj.size()) && bases_alt<Fq>(ctx, (const amsm_bases*)keys[ki].id, &twin[ki]) == AMSM_OK)
        keys[ki] = job_key((const amsm_bases*)keys[ki].id, twin[ki]);
    n_units = mjobs::plan_units(pc, keys.data(), uj.data(), uj.size(), xyzz_bytes<Fq>(), units.data(), ugeom.data());
    ujobs.reserve(live.size());
    for (size_t i : live) ujobs.push_back(jobs[i]);
  } else {
    for (size_t i = 0; i < live.size(); i++) units[i] = msel::Unit{i, 1};
  }
  std::vector<uint8_t> ovf(n_units, 0), degraded(n_units, 0);
  const int rc = run_ring(
      ctx, n_units,
      [&](size_t u, Slot* sl) -> int {
        const msel::Unit un = units[u];
        if (un.count == 1) return msm_enqueue<Fq, Fr>(ctx, sl, jobs[live[un.first]], place_of(u, n_units));
        const BpsUnitGeom found{ugeom[un.first].g, ugeom[un.first].over_twin ? twin[uj[un.first].key] : ujobs[un.first].key};
        int r = msm_enqueue_bps_batch<Fq, Fr>(ctx, sl, &ujobs[un.first], un.count, found, place_of(u, n_units));
        if (r != AMSM_E_OOM) return r;
        // the unit's buffers could not be had (nothing was launched): its MSMs singly on this slot, the last one left to the ring
        (void)hipGetLastError();
        degraded[u] = 1;
        for (size_t v = 0; v < un.count; v++) {
          TRY((msm_enqueue<Fq, Fr>(ctx, sl, ujobs[un.first + v], Place::BATCH_LAST)));
          if (v + 1 < un.count) TRY(msm_collect<Fq>(ctx, sl, &(*part)[live[un.first + v]]));
        }
        return AMSM_OK;
      },
      [&](size_t u, Slot* sl) -> int {
        const msel::Unit un = units[u];
        if (un.count == 1 || degraded[u]) return msm_collect<Fq>(ctx, sl, &(*part)[live[un.first + un.count - 1]]);
        host::HXYZZ<Fq> res[msel::BPS_BATCH];
        TRY(msm_collect<Fq>(ctx, sl, res));
        for (size_t v = 0; v < un.count; v++) (*part)[live[un.first + v]] = res[v];
        return AMSM_OK;
      },
      ovf.data());
  if (overflow)
    for (size_t u = 0; u < n_units; u++)
      if (units[u].count == 1) (*overflow)[live[units[u].first]] = ovf[u];
  return rc;
}

template <class Fq, class Fr>
int msm_device_xyzz(amsm_ctx* ctx, const amsm_bases* bases, size_t base_off, const void* d_scalars, size_t n,
                    int scalars_mont, host::HXYZZ<Fq>* out) {
  std::vector<MsmJob> vec;
  TRY(jobs_from_arrays(bases, 1, &base_off, &d_scalars, &n, scalars_mont, &vec));
  n = vec[0].n;
  if (n == 0) {
    *out = host::hx_inf<Fq>();
    return AMSM_OK;
  }
  const bool probe_wanted = mjobs::probe_wanted(plan_ctx(ctx), key_desc(bases), n);
  // (long single vectors are worth the two-valued probe's synchronisation: ~20 us against 0.45 ms and up)
  const bool split = split_needed(ctx, bases, n) || probe_wanted || (ctx->two_valued && n >= ((size_t)1 << 17));  // windows of the key / the probes
  std::vector<host::HXYZZ<Fq>> r;
  TRY((split ? msm_multi_split_xyzz<Fq, Fr>(ctx, vec, &r) : msm_multi_xyzz<Fq, Fr>(ctx, vec, &r)));
  *out = r[0];
  return AMSM_OK;
}

// Large MSMs over a precomputed key run as pipelined sub-MSMs over windows of 2^split_log2 generators, summed on the host.
// The partition pass of the prep sorts entries by (bucket, index) in one 32-bit word: above 2^21 pairs the index bits leave
// too few for bucket ids and the pass needs 2048-4096 partitions (8- to 4-byte runs: prep 7.2 ms at 2^23; 2^24 fell back to
// the rocPRIM sort).  A window carries window-relative indices (MsmGeom::idx_rel_bits) and sorts like a 2^21-pair MSM
// whatever the key's length; the extra bucket reductions hide behind the next window's accumulation, and a blocking call of
// that size becomes a pipeline.  Measured (batches, M pairs/s, whole / 2^20 windows / 2^21 windows): 2^22 815 / 822 / 845,
// 2^23 507 / 841 / 868, 2^24 725 / 848 / 874; the workspace of a 2^24-pair MSM drops from 25.6 GB to 1.5 GB.
// vecs: one job per caller vector, all over one key and in one scalar form (vecs[0].mont); (*out)[i] = the MSM of vecs[i]
template <class Fq, class Fr>
int msm_multi_split_impl(amsm_ctx* ctx, const std::vector<MsmJob>& vecs, std::vector<host::HXYZZ<Fq>>* out,
                         const std::vector<uint8_t>* pre_skew = nullptr);  // the skew probe's verdicts when the caller ran it

// Two-valued vectors first (vec_kernels.h k_tv_probe: EXACT test on the device, one launch per distinct vector, one copy and
// one synchronisation per call): such a vector's MSM is v * (sum of the generators with a non-zero scalar) -- k_tv_sum + k_fold
// on a stream of their own beside the other MSMs of the call, the scalar multiplication on the host when they are collected.
// Everything else goes on as before.  Vectors below 2^14 pairs are not probed (their whole MSM is a few launches).
// Four steps, plain data between them: tv_probe (launch the probes, one synchronisation), msel::classify (msm_select.h),
// tv_launch_sums (the sums on their own stream), then msm_multi_split_xyzz runs the rest and finishes on the host.
constexpr size_t TV_MIN_PAIRS = (size_t)1 << 14;
constexpr size_t TV_PW = TV_PROBE_WORDS, TV_PB = TV_PROBE_WORDS * 4;  // probe block per vector: words, bytes
template <class Fq>
constexpr size_t tv_exc_rec() { return (8 + 2 * Fq::W) * 4; }  // one exception record: the scalar, its generator
template <class Fq>
constexpr size_t tv_exc_bytes() { return TV_EXC_SLOTS * tv_exc_rec<Fq>(); }  // exception records per vector

struct TvProbes {  // step (a): what the probes said, read back behind one synchronisation
  std::vector<const u32*> host_words, dev_words;  // per vector: its probe block in ctx->tv_pinned / on the device (null: not probed)
  std::vector<uint8_t> skew;                       // the skew probe's verdict per vector
  bool have_skew = false;                          // ... if the pipelines want one for this key
  size_t cap_vecs = 0;                             // probe blocks the first half of ctx->tv_flags has room for
  u32 one_words[8] = {1u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};  // the unit scalar as these vectors store it
};
// (a) the two-valued probe of the vectors `cand`, and the skew probe the pipelines would run anyway riding on its synchronisation
template <class Fq, class Fr>
int tv_probe(amsm_ctx* ctx, const std::vector<MsmJob>& vecs, const std::vector<size_t>& cand, TvProbes* p) {
  const amsm_bases* bases = vecs[0].key;
  const size_t rec = xyzz_bytes<Fq>();
  // (sized for at least 256 vectors: a first call with more vectors than any before it would otherwise re-allocate device and
  // page-locked memory -- milliseconds -- inside that call: the first 20-MSM batch after a 3-MSM warm-up ran 1.8 ms longer)
  p->cap_vecs = std::max<size_t>(cand.size(), 256);
  TRY(ensure(ctx->tv_flags, 2 * p->cap_vecs * TV_PB));  // (second half: the synthetic probe blocks of the unit-scalar sums)
  const size_t pin_need = 2 * p->cap_vecs * (TV_PB + rec + tv_exc_bytes<Fq>()) + 64;
  if (ctx->tv_pinned_bytes < pin_need) {
    if (ctx->tv_pinned) (void)gate_free(ctx->tv_pinned);
    ctx->tv_pinned = nullptr;
    ctx->tv_pinned_bytes = 0;
    TRY(gate_alloc(ctx, GATE_PINNED, pin_need * 2, false, &ctx->tv_pinned));
    ctx->tv_pinned_bytes = pin_need * 2;
  }
  HIP_TRY(hipMemsetAsync(ctx->tv_flags.p, 0, cand.size() * TV_PB, ctx->stream));
  if (vecs[0].mont)
    for (int i = 0; i < 8; i++) p->one_words[i] = Fr::one(i);
  const std::vector<size_t> first = first_identical(vecs, cand);
  p->host_words.assign(vecs.size(), nullptr);
  p->dev_words.assign(vecs.size(), nullptr);
  for (size_t j = 0; j < cand.size(); j++) {
    const MsmJob& vec = vecs[cand[j]];
    if (first[j] == j) launch_tv_probe(ctx->stream, (const u32*)vec.scalars, (u32)vec.n, (u32*)ctx->tv_flags.p + TV_PW * j, p->one_words);
    p->host_words[cand[j]] = (const u32*)ctx->tv_pinned + TV_PW * first[j];
    p->dev_words[cand[j]] = (const u32*)ctx->tv_flags.p + TV_PW * first[j];
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(ctx->tv_pinned, ctx->tv_flags.p, cand.size() * TV_PB, hipMemcpyDeviceToHost, ctx->stream));
  SkewProbe sp;
  size_t sp_min = 0;
  DigitWalk sp_walk;
  p->have_skew = skew_probe_params(ctx, bases, vecs, &sp_min, &sp_walk) != 0;
  sp_walk.skip_ones = bases->bpl ? 0u : 1u;  // (numerous unit scalars are summed apart -- not over a 20-bit table --; a few skew nothing)
  if (p->have_skew) TRY(bpl_probe_enqueue<Fr>(ctx, vecs, sp_walk, sp_min, &sp, p->dev_words.data()));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (p->have_skew) bpl_probe_finish(ctx, sp, &p->skew);
  return AMSM_OK;
}

struct TvSums {  // step (c): the sums in flight on ctx->s_tv
  std::vector<size_t> tv;               // the vectors summed there: the two-valued ones, then (from n_proper on) those whose ones are summed apart
  size_t n_proper = 0;
  std::vector<std::array<u64, 4>> vals;  // per sum: the value v its result is multiplied by (canonical form)
  std::vector<u32> n_exc;                // ... and how many exception records come with it
};
// (c) the sums of the generators under a two-valued vector's value / under the unit scalars of a vector that sums them apart -- the
// two-valued machinery with v = 1, no scalar multiplication --: k_tv_sum + the fold on s_tv, the records' copy queued behind them
template <class Fq, class Fr>
int tv_launch_sums(amsm_ctx* ctx, const std::vector<MsmJob>& vecs, const TvProbes& p, const std::vector<uint8_t>& verdict, TvSums* s) {
  const size_t rec = xyzz_bytes<Fq>(), EXC_B = tv_exc_bytes<Fq>();
  for (size_t v = 0; v < vecs.size(); v++)
    if (verdict[v] == msel::V_TWO_VALUED) s->tv.push_back(v);
  s->n_proper = s->tv.size();
  for (size_t v = 0; v < vecs.size(); v++)
    if (verdict[v] == msel::V_ONES_APART) s->tv.push_back(v);
  const std::vector<size_t>& tv = s->tv;
  if (tv.empty()) return AMSM_OK;
  // the scalars' values, before the pinned block is reused for the records
  s->vals.resize(tv.size());
  s->n_exc.resize(tv.size());
  for (size_t t = 0; t < tv.size(); t++) {
    if (t >= s->n_proper) {  // a unit-scalar sum: v = 1, no exceptions
      s->vals[t] = {1, 0, 0, 0};
      s->n_exc[t] = 0;
      continue;
    }
    const u32* f = p.host_words[tv[t]];
    host::HFe<Fr> val;
    memcpy(val.v, f + msel::TVW_VALUE, 32);
    if (vecs[0].mont) val = host::h_from_mont<Fr>(val);
    memcpy(s->vals[t].data(), val.v, 32);
    s->n_exc[t] = std::min<u32>(f[msel::TVW_N_EXC], TV_EXC_SLOTS);
  }
  if (!ctx->s_tv) HIP_TRY(hipStreamCreateWithFlags(&ctx->s_tv, hipStreamNonBlocking));
  if (!ctx->tv_done) HIP_TRY(hipEventCreateWithFlags(&ctx->tv_done, hipEventDisableTiming));
  // one launch per group of up to 8 vectors (and one fold for the group): every sum is a short latency-bound chain
  size_t max_len = 0;
  for (size_t t = 0; t < tv.size(); t++) max_len = std::max(max_len, vecs[tv[t]].n);
  // 8 points per lane (r1cs_nark_as 2^18 harness-zk prove with 8 / 4 / 2: 2.04 / 2.15 / 2.46 ms: fewer records to fold wins)
  const u32 blocks = (u32)std::max<size_t>(32, std::min<size_t>(1024, max_len / (256 * 8)));
  TRY(ensure(ctx->tv_parts, tv.size() * (size_t)blocks * rec));
  TRY(ensure(ctx->tv_out, tv.size() * (rec + EXC_B) + 64));  // the folded records, then the vectors' exception records
  u32* d_exc = (u32*)((char*)ctx->tv_out.p + tv.size() * rec);
  // the unit-scalar sums read a synthetic probe block each: [3] = 0 exceptions, [8..15] = the unit as stored
  std::vector<u32> ones_blocks((tv.size() - s->n_proper) * TV_PW, 0u);
  for (size_t t = s->n_proper; t < tv.size(); t++) memcpy(&ones_blocks[(t - s->n_proper) * TV_PW + msel::TVW_VALUE], p.one_words, 32);
  u32* d_ones_blocks = (u32*)ctx->tv_flags.p + TV_PW * p.cap_vecs;
  if (!ones_blocks.empty()) {
    HIP_TRY(hipMemcpyAsync(d_ones_blocks, ones_blocks.data(), ones_blocks.size() * 4, hipMemcpyHostToDevice, ctx->s_tv));
    HIP_TRY(hipStreamSynchronize(ctx->s_tv));  // (pageable source: must outlive the copy; only vectors with unit scalars pay this)
  }
  // (the caller's stream was synchronised by tv_probe: the scalars are complete, s_tv needs no event to see them)
  for (size_t t0 = 0; t0 < tv.size(); t0 += 8) {
    const u32 nv = (u32)std::min<size_t>(8, tv.size() - t0);
    const u32 *ptrs[8], *probes[8];
    u32 nn[8], oo[8];
    for (u32 j = 0; j < nv; j++) {
      const MsmJob& vec = vecs[tv[t0 + j]];
      ptrs[j] = (const u32*)vec.scalars;
      probes[j] = t0 + j >= s->n_proper ? d_ones_blocks + TV_PW * (t0 + j - s->n_proper) : p.dev_words[tv[t0 + j]];
      nn[j] = (u32)vec.n;
      oo[j] = (u32)vec.off;
    }
    u32* parts = (u32*)((char*)ctx->tv_parts.p + t0 * (size_t)blocks * rec);
    launch_tv_sum<Fq>(ctx->s_tv, (const u32*)vecs[0].key->d_table, nv, ptrs, probes, nn, oo, blocks, parts, (u32*)((char*)d_exc + t0 * EXC_B));
    // (the caller waits for these sums: the quad-cooperative fold, as for an exposed MSM tail)
    launch_fold<Fq>(ctx->s_tv, true, nv, parts, blocks, (u32*)((char*)ctx->tv_out.p + t0 * rec), nullptr);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(ctx->tv_pinned, ctx->tv_out.p, tv.size() * (rec + EXC_B), hipMemcpyDeviceToHost, ctx->s_tv));
  HIP_TRY(hipEventRecord(ctx->tv_done, ctx->s_tv));
  return AMSM_OK;
}

template <class Fq, class Fr>
int msm_multi_split_xyzz(amsm_ctx* ctx, const std::vector<MsmJob>& vecs, std::vector<host::HXYZZ<Fq>>* out) {
  const size_t k = vecs.size();
  std::vector<size_t> cand;
  // (also over a direct-sum key: at 2^14 pairs a two-valued vector's MSM is still 4x cheaper than the sum of 2^14 * 60 points)
  for (size_t v = 0; v < k; v++)
    if (ctx->two_valued && vecs[v].n >= TV_MIN_PAIRS && vecs[v].n < (1ull << 32) && vecs[v].off + vecs[v].n < (1ull << 32)) cand.push_back(v);
  if (cand.empty()) return msm_multi_split_impl<Fq, Fr>(ctx, vecs, out);
  const amsm_bases* bases = vecs[0].key;
  const int scalars_mont = vecs[0].mont;
  const size_t rec = xyzz_bytes<Fq>(), EXC_REC = tv_exc_rec<Fq>(), EXC_B = tv_exc_bytes<Fq>();
  TvProbes probes;
  TRY((tv_probe<Fq, Fr>(ctx, vecs, cand, &probes)));
  const std::vector<uint8_t>* pre = probes.have_skew ? &probes.skew : nullptr;
  // (b) two-valued, all zero, unit scalars summed apart, or as it is: msm_select.h
  std::vector<uint8_t> verdict(k);
  {
    std::vector<msel::VecProbe> vp(k);
    for (size_t v = 0; v < k; v++) vp[v] = msel::VecProbe{probes.host_words[v], vecs[v].n, (const char*)vecs[v].scalars};
    msel::classify(vp.data(), k, scalars_mont != 0, key_desc(bases), switches_of(ctx), verdict.data());
  }
  bool any_apart = false;  // vectors that skip the pipelines, or run them without their ones
  for (size_t v = 0; v < k; v++) {
    any_apart = any_apart || verdict[v] != msel::V_REGULAR;
    if (verdict[v] == msel::V_ALL_ZERO) ctx->n_two_valued++;
  }
  if (!any_apart) return msm_multi_split_impl<Fq, Fr>(ctx, vecs, out, pre);
  TvSums sums;
  TRY((tv_launch_sums<Fq, Fr>(ctx, vecs, probes, verdict, &sums)));
  const std::vector<size_t>& tv = sums.tv;
  // (d) the other vectors through the regular pipelines meanwhile
  std::vector<MsmJob> rest;
  std::vector<uint8_t> r_skew;
  for (size_t v = 0; v < k; v++)
    if (verdict[v] == msel::V_REGULAR || verdict[v] == msel::V_ONES_APART) {
      rest.push_back(vecs[v]);
      rest.back().owner = v;
      rest.back().skip_ones = verdict[v] == msel::V_ONES_APART;
      if (pre) r_skew.push_back(probes.skew[v]);
    }
  out->assign(k, host::hx_inf<Fq>());
  int rc = AMSM_OK;
  if (!rest.empty()) {
    std::vector<host::HXYZZ<Fq>> part;
    rc = msm_multi_split_impl<Fq, Fr>(ctx, rest, &part, pre ? &r_skew : nullptr);
    if (rc == AMSM_OK) add_by_owner<Fq>(rest, part, out);
  }
  if (!tv.empty()) HIP_TRY(hipEventSynchronize(ctx->tv_done));
  if (rc != AMSM_OK || tv.empty()) return rc;
  // a scalar of 2^255 or more among a vector's exceptions (canonical form): that vector goes back to the windowed pipelines,
  // whose verdict on such scalars stands (an error where the key's windows cannot take them, the integer's multiple where they can)
  std::vector<uint8_t> tv_bad(tv.size(), 0);
  auto finish = [&](size_t t) {
    const size_t v = tv[t];
    if (t >= sums.n_proper) {  // the sum of the generators under unit scalars joins what the pipelines computed without them
      (*out)[v] = host::hx_add<Fq>((*out)[v], host::hx_from_device<Fq>((const u32*)((const char*)ctx->tv_pinned + t * rec)));
      return;
    }
    // v * sum + s_j G_j for the few scalars that are neither 0 nor v: one combination with shared doublings
    host::HXYZZ<Fq> pts[1 + TV_EXC_SLOTS];
    u64 ks[1 + TV_EXC_SLOTS][4];
    pts[0] = host::hx_from_device<Fq>((const u32*)((const char*)ctx->tv_pinned + t * rec));
    memcpy(ks[0], sums.vals[t].data(), 32);
    const char* ex = (const char*)ctx->tv_pinned + tv.size() * rec + t * EXC_B;
    for (u32 e = 0; e < sums.n_exc[t]; e++) {
      host::HFe<Fr> s;
      memcpy(s.v, ex + e * EXC_REC, 32);
      if (scalars_mont) s = host::h_from_mont<Fr>(s);
      else if ((s.v[host::HFe<Fr>::N - 1] >> 63) != 0) tv_bad[t] = 1;  // >= 2^255
      memcpy(ks[1 + e], s.v, 32);
      u64 xy[2 * host::HFe<Fq>::N];
      memcpy(xy, ex + e * EXC_REC + 32, sizeof(xy));
      pts[1 + e] = host::hx_from_affine<Fq>(xy, false);
    }
    (*out)[v] = host::hx_lincomb<Fq>(pts, ks, 1 + sums.n_exc[t], nullptr);
  };
  if (tv.size() > 1) HostPool::get().run(tv.size(), finish);
  else finish(0);
  std::vector<MsmJob> bad;
  for (size_t t = 0; t < tv.size(); t++) {
    if (t >= sums.n_proper) ctx->n_ones_split++;
    else if (!tv_bad[t]) ctx->n_two_valued++;
    else {
      bad.push_back(vecs[tv[t]]);
      bad.back().owner = tv[t];
    }
  }
  if (!bad.empty()) {
    std::vector<host::HXYZZ<Fq>> part;
    TRY((msm_multi_split_impl<Fq, Fr>(ctx, bad, &part)));
    for (size_t j = 0; j < bad.size(); j++) (*out)[bad[j].owner] = part[j];  // (in place of the shortcut's result)
  }
  return AMSM_OK;
}

template <class Fq, class Fr>
int msm_multi_split_impl(amsm_ctx* ctx, const std::vector<MsmJob>& vecs, std::vector<host::HXYZZ<Fq>>* out, const std::vector<uint8_t>* pre_skew) {
  const size_t k = vecs.size();
  out->assign(k, host::hx_inf<Fq>());
  if (k == 0) return AMSM_OK;
  const amsm_bases* bases = vecs[0].key;
  // the digit probe's verdicts (msm_select.h: wants_skew_probe), where the pipelines want them for this key
  std::vector<uint8_t> skew(k, 0);
  size_t probe_min = 0;
  DigitWalk probe_walk;
  if (skew_probe_params(ctx, bases, vecs, &probe_min, &probe_walk) != 0) {
    if (pre_skew) skew = *pre_skew;
    else TRY(bpl_probe_device<Fr>(ctx, vecs, &skew, probe_walk, probe_min));
  }
  std::vector<MsmJob> jobs;  // the vectors' ranges (msm_jobs.h: plan_ranges, the device form); owner: the vector's place in `vecs`
  TRY(plan_jobs<Fq>(ctx, bases, vecs, skew.data(), mjobs::device_form(), &jobs));
  std::vector<host::HXYZZ<Fq>> part;
  std::vector<uint8_t> ovf;
  TRY((msm_multi_xyzz<Fq, Fr>(ctx, jobs, &part, &ovf)));
  // a range of a shared MSM met skewed digits (what the probe's 1024 samples missed): that vector's shared ranges again, each an
  // MSM of its own with its own fallback -- the result does not depend on the path
  std::vector<uint8_t> redo(k, 0);
  bool any_redo = false;
  for (size_t j = 0; j < jobs.size(); j++)
    if (ovf[j]) redo[jobs[j].owner] = 1, any_redo = true;
  if (any_redo) {
    std::vector<MsmJob> again;  // (owner: here the place in `jobs` whose part the re-run replaces -- not added: the range's own part is stale)
    for (size_t j = 0; j < jobs.size(); j++)
      if (redo[jobs[j].owner] && jobs[j].share.buf >= 0) {
        again.push_back(jobs[j]);
        again.back().share = Share();
        again.back().owner = j;
      }
    std::vector<host::HXYZZ<Fq>> r;
    TRY((msm_multi_xyzz<Fq, Fr>(ctx, again, &r)));
    for (size_t t = 0; t < again.size(); t++) part[again[t].owner] = r[t];
    ctx->n_bpl_fallbacks++;
  }
  add_by_owner<Fq>(jobs, part, out);
  return AMSM_OK;
}

// page-locked (hipHostRegister / hipHostMalloc) host memory?  (include/amsm.h: amsm_host_register)
bool host_ptr_pinned(const void* p) {
  if (!p) return false;
  hipPointerAttribute_t a;
  memset(&a, 0, sizeof(a));
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();  // pageable memory the runtime has never seen
    return false;
  }
  return a.type == hipMemoryTypeHost;
}

// k MSMs whose scalars are HOST slices (a Rust `&[BigInt]` / `&[Fr]` per commitment -- the form the reference's call sites
// hand over back to back: src/hp_as/mod.rs:372-385, :196-214, src/r1cs_nark_as/r1cs_nark/mod.rs:216-218).  The upload of
// vector j + 1 runs on a copy stream while MSM j computes: a ring of staging buffers longer than the pipeline has slots, so
// that a buffer is rewritten only after the MSM that read it was collected (a bucket-per-lane MSM may be re-run from it,
// msm_collect): upload(j + RING) is issued after enqueue(j + RING - 1), which collected MSM j's slot long before.
// Long vectors over a precomputed key are cut into the same windows as msm_multi_split_xyzz cuts device vectors.
// What the host learns about a slice before anything is uploaded -- does it LOOK two-valued (the reference harness's `vec![rand; len]`
// inputs and the DummyCircuit's constant A z, B z, C z), does it hold a share of unit scalars, are its digits skewed -- is sampled by
// the rules of msm_jobs.h (looks_two_valued, has_unit_scalars, skew_probe_host).
// amsm_msm_oneshot (round 6): the generators are HOST memory too (`VariableBaseMSM::multi_scalar_mul(&[G], &[BigInt])`, the ark-ec
// call shape: SURVEY.md section 8(b) attachment 1).  `key` is the call's temporary plain key over the context's one-shot buffer;
// the job loop of msm_multi_host_xyzz uploads and imports the generators of a range on the copy stream right in front of that
// range's scalars, so the copy engine never waits for the arithmetic and the arithmetic of range j hides behind the upload of
// range j + 1: the call is bound by the link (96 B per Pallas pair), not by upload + MSM in series.
struct OneshotBases {
  const uint64_t* xy = nullptr;      // n * 2 * limbs u64, C-ABI Montgomery radix
  const uint8_t* is_inf = nullptr;   // n flags or null
  size_t step = 0;                   // pairs per range
};
template <class Fq>
int oneshot_upload_range(amsm_ctx* ctx, const amsm_bases* key, const OneshotBases* os, size_t off, size_t n, hipStream_t st) {
  if (!n) return AMSM_OK;
  u32* dst = key->d_table + off * (affine_bytes<Fq>() / 4);
  HIP_TRY(hipMemcpyAsync(dst, (const char*)os->xy + off * affine_bytes<Fq>(), n * affine_bytes<Fq>(), hipMemcpyHostToDevice, st));
  if (os->is_inf) {
    HIP_TRY(hipMemcpyAsync((char*)ctx->oneshot_inf.p + off, os->is_inf + off, n, hipMemcpyHostToDevice, st));
    launch_apply_inf<Fq>(st, dst, (const uint8_t*)ctx->oneshot_inf.p + off, (u32)n);
  }
  launch_points_import<Fq>(st, dst, dst, (u32)n);  // C-ABI radix -> device radix, in place
  return AMSM_OK;
}
// Round 6 -- a LONE host slice of [3 x 2^18, 2^20] pairs over a 20-bit key (the reference's `commit(&ck, &[Fr], ..)`: one blocking call at a
// time, src/hp_as/mod.rs:372-385,911-918) runs as TWO ranges over ONE bucket set (struct Share: range 1 writes the set, range 2 adds to
// it and carries the only tail): msm_jobs.h: halves_apply has the rule and its measurements.  A range whose digits turn out skewed sends
// the call back to the one-range form (no_halves).
inline bool host_halves_apply(const amsm_ctx* ctx, const amsm_bases* key, size_t len) { return mjobs::halves_apply(plan_ctx(ctx), key_desc(key), len); }
template <class Fq, class Fr>
int msm_multi_host_xyzz(amsm_ctx* ctx, const amsm_bases* bases, size_t k, const size_t* offs, const uint64_t* const* h_scalars,
                        const size_t* ns, int scalars_mont, std::vector<host::HXYZZ<Fq>>* out, const OneshotBases* os = nullptr,
                        bool no_halves = false) {
  out->assign(k, host::hx_inf<Fq>());
  std::vector<MsmJob> vecs;  // one job per slice (scalars: host pointers)
  TRY(jobs_from_arrays(bases, k, offs, (const void* const*)h_scalars, ns, scalars_mont, &vecs));
  // What the host learns about the slices before anything is uploaded: 1024 samples each for "looks two-valued" and for the digit
  // histogram of the skew probe.  Round 5: the samples are 1024 cache and TLB misses per look and the histogram 13 windows of
  // them -- ~0.1 ms per slice, serial in front of the first upload: 1.1-1.3 ms of a 17.5 ms call of twelve 2^20-scalar slices
  // (rocprofv3 timeline against the call's wall clock, profiles/r05_host_slices.md).  Now one task per DISTINCT slice on the host pool.
  std::vector<uint8_t> looks_tv(k, 0), skew(k, 0);
  {
    const mjobs::PlanCtx pc = plan_ctx(ctx);
    const msel::KeyDesc kd = key_desc(bases);
    std::vector<size_t> all(k);
    for (size_t v = 0; v < k; v++) all[v] = v;
    const std::vector<size_t> first = first_identical(vecs, all);
    HostPool::get().run(k, [&](size_t v) {
      if (first[v] != v || !h_scalars[v]) return;
      const size_t len = vecs[v].n;
      if (ctx->two_valued && len >= TV_MIN_PAIRS) looks_tv[v] = mjobs::looks_two_valued(h_scalars[v], len);
      if (!looks_tv[v] && ctx->two_valued && len >= TV_MIN_PAIRS && !bases->bpl) {  // (a witness with boolean wires goes there too)
        u32 one_words[8] = {1u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
        if (scalars_mont)
          for (int i = 0; i < 8; i++) one_words[i] = Fr::one(i);
        looks_tv[v] = mjobs::has_unit_scalars(h_scalars[v], len, one_words);
      }
      if (looks_tv[v]) return;  // (such a call goes to the device path's exact probe: the digit verdicts are not used)
      // (a skewed slice -- the constant hiding vectors of the zk provers -- would pay an aborted prep plus a re-run)
      if (mjobs::probe_wanted(pc, kd, len))
        skew[v] = bpl_probe_host<Fr>(h_scalars[v], len, scalars_mont, mjobs::key_walk(geom_key(bases)), mjobs::probe_min_len(kd));
    });
    for (size_t v = 0; v < k; v++) looks_tv[v] = looks_tv[first[v]], skew[v] = skew[first[v]];
  }
  // Round 4: slices that look two-valued take the device path's exact probe and its n-addition form (4.2d) -- a constant vector of
  // 2^20 scalars is 0.3 ms there against ~3 ms through the skew fallback here.  All slices of the call are copied into one staging
  // buffer first (no upload / compute overlap for this call: the MSMs it is about are ten times shorter than their uploads).
  if (ctx->two_valued && k >= 1) {
    bool any = false;
    size_t total = 0;
    for (size_t v = 0; v < k; v++) {
      total += vecs[v].n * 32;
      any = any || looks_tv[v];
    }
    if (any && total <= ((size_t)4 << 30)) {
      if (os) TRY(oneshot_upload_range<Fq>(ctx, bases, os, vecs[0].off, vecs[0].n, ctx->stream));  // (one vector: k = 1)
      TRY(ensure(ctx->stage, total));
      size_t at = 0;
      for (MsmJob& vec : vecs) {  // from here on device vectors
        char* dst = (char*)ctx->stage.p + at;
        if (vec.n) HIP_TRY(hipMemcpyAsync(dst, vec.scalars, vec.n * 32, hipMemcpyHostToDevice, ctx->stream));
        vec.scalars = dst;
        at += vec.n * 32;
      }
      return msm_multi_split_xyzz<Fq, Fr>(ctx, vecs, out);
    }
  }
  // the slices' ranges (msm_jobs.h: plan_ranges, the host form; scalars: host pointers): long slices cut like device vectors, the
  // lone slice in two halves over one bucket set (host_halves_apply above), a one-shot call by its own step
  std::vector<MsmJob> jobs;
  TRY(plan_jobs<Fq>(ctx, bases, vecs, skew.data(), mjobs::host_form(k, os != nullptr, os ? os->step : 0, no_halves), &jobs));
  size_t n_max = 0;
  for (const MsmJob& j : jobs) n_max = std::max(n_max, j.n);
  const bool halved = !jobs.empty() && jobs[0].share.buf >= 0;  // (the only shared set of this form)
  if (jobs.empty()) return AMSM_OK;
  const size_t J = jobs.size();
  std::vector<host::HXYZZ<Fq>> part;
  // small keys (direct sums, DESIGN.md 4.2g): the slices are a few hundred KiB each -- copied behind one another on the caller's
  // stream into one staging buffer, then ONE batched launch per 16 MSMs (msm_multi_xyzz) instead of an upload / launch pair each
  {
    bool all_direct = J >= 2;
    size_t total = 0;
    for (const MsmJob& j : jobs) {
      all_direct = all_direct && j.key == bases && direct_sum_applies(ctx, j);
      total += j.n * 32;
    }
    if (all_direct && total <= ((size_t)64 << 20)) {
      TRY(ensure(ctx->stage_ring[0], total));
      std::vector<MsmJob> staged = jobs;
      size_t at = 0;
      for (MsmJob& j : staged) {
        char* dst = (char*)ctx->stage_ring[0].p + at;
        HIP_TRY(hipMemcpyAsync(dst, j.scalars, j.n * 32, hipMemcpyHostToDevice, ctx->stream));
        j.scalars = dst;
        at += j.n * 32;
      }
      TRY((msm_multi_xyzz<Fq, Fr>(ctx, staged, &part)));
      add_by_owner<Fq>(jobs, part, out);
      return AMSM_OK;
    }
  }
  constexpr int RING = amsm_ctx::STAGE_RING;
  if (!ctx->s_copy) HIP_TRY(hipStreamCreateWithFlags(&ctx->s_copy, hipStreamNonBlocking));
  for (int r = 0; r < RING && (size_t)r < J; r++) {
    TRY(ensure(ctx->stage_ring[r], n_max * 32));
    if (!ctx->up_ev[r]) HIP_TRY(hipEventCreateWithFlags(&ctx->up_ev[r], hipEventDisableTiming));
  }
  auto upload = [&](size_t j) -> int {
    const int r = (int)(j % RING);
    if (os) TRY(oneshot_upload_range<Fq>(ctx, jobs[j].key, os, jobs[j].off, jobs[j].n, ctx->s_copy));  // the range's generators first
    HIP_TRY(hipMemcpyAsync(ctx->stage_ring[r].p, jobs[j].scalars, jobs[j].n * 32, hipMemcpyHostToDevice, ctx->s_copy));
    HIP_TRY(hipEventRecord(ctx->up_ev[r], ctx->s_copy));
    return AMSM_OK;
  };
  part.assign(J, host::hx_inf<Fq>());
  std::vector<uint8_t> ovf(J, 0);
  const int rc = run_ring(
      ctx, J,
      [&](size_t j, Slot* sl) -> int {
        if (j == 0) {
          // the ring's buffers may still be read by the prep kernels of an earlier call's MSMs?  No: every call collects all its
          // MSMs before it returns.  The copy stream only has to stay behind the caller's stream (buffers freshly grown above).
          HIP_TRY(hipStreamWaitEvent(ctx->s_copy, ctx->fork, 0));
          TRY(upload(0));
        }
        const int r = (int)(j % RING);
        // both streams a prep chain may start on (the caller's for a lone MSM, the prep stream otherwise) wait for the upload
        HIP_TRY(hipStreamWaitEvent(ctx->s_prep, ctx->up_ev[r], 0));
        // (the caller's stream reads scalars only in those two cases: inside a batch it carries the accumulations, and a barrier
        // packet in front of each costs the queue ~10 us)
        if (J == 1 || direct_sum_applies(ctx, jobs[j]))
          HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->up_ev[r], 0));
        MsmJob staged = jobs[j];  // the slot's job reads the staging buffer (a re-run too: msm_collect)
        staged.scalars = ctx->stage_ring[r].p;
        TRY((msm_enqueue<Fq, Fr>(ctx, sl, staged, place_of(j, J))));
        // ONE upload ahead of the MSM being enqueued, the host copies while the GPU computes MSM j (two ahead were measured slower
        // twice: the ring has N_SLOTS + 2 buffers all the same)
        return j + 1 < J ? upload(j + 1) : AMSM_OK;
      },
      [&](size_t j, Slot* sl) { return msm_collect<Fq>(ctx, sl, &part[j]); }, ovf.data());
  (void)hipStreamSynchronize(ctx->s_copy);
  if (rc != AMSM_OK) return rc;
  if (halved && (ovf[0] || ovf[1])) {  // skewed digits in one of the halves (what the host's 1024 samples missed): the one-range form,
    ctx->n_bpl_fallbacks++;             // with its own fallback -- the result does not depend on the path
    return msm_multi_host_xyzz<Fq, Fr>(ctx, bases, k, offs, h_scalars, ns, scalars_mont, out, os, true);
  }
  add_by_owner<Fq>(jobs, part, out);
  return AMSM_OK;
}

// n_vecs MSMs over the same generators (the prover's back-to-back commits)
template <class Fq, class Fr>
int msm_batch_xyzz(amsm_ctx* ctx, const amsm_bases* bases, size_t base_off, const void* const* d_scalars,
                   size_t n_vecs, size_t n, int scalars_mont, std::vector<host::HXYZZ<Fq>>* out) {
  std::vector<size_t> offs(n_vecs, base_off), ns(n_vecs, n);
  std::vector<MsmJob> vecs;
  TRY(jobs_from_arrays(bases, n_vecs, offs.data(), d_scalars, ns.data(), scalars_mont, &vecs));
  return msm_multi_split_xyzz<Fq, Fr>(ctx, vecs, out);
}
