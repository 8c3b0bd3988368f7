// Part of api.hip (inside extern "C"): status strings, contexts, profiling.

const char* amsm_strerror(int s) {
  switch (s) {
    case AMSM_OK: return "ok";
    case AMSM_E_INVALID_ARG: return "invalid argument";
    case AMSM_E_OOM: return "out of (device) memory";
    case AMSM_E_HIP: return "HIP runtime error";
    case AMSM_E_UNSUPPORTED: return "unsupported size or configuration";
    case AMSM_E_NO_DEVICE: return "no usable gfx950 device (the host backend is never chosen implicitly: ask for AMSM_DEVICE_HOST)";
    case AMSM_E_SCALAR_RANGE: return "scalar out of range (not a canonical into_repr value)";
    case AMSM_E_RCCL: return "RCCL collective failed";
    case AMSM_E_INVALID_POINT: return "invalid point (non-canonical, off the curve or outside the prime-order subgroup)";
    default: return "unknown error";
  }
}

int amsm_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}

static size_t pool_cap_from_env(size_t dflt) {
  const char* e = getenv("AMSM_POOL_MAX_MB");
  return e ? (size_t)std::max(0, atoi(e)) << 20 : dflt;
}
static size_t mem_limit_from_env() {  // AMSM_MEM_LIMIT_MB: amsm_ctx_set_memory_limit at creation (unset, 0 or not a number: no limit)
  const char* e = getenv("AMSM_MEM_LIMIT_MB");
  return e ? (size_t)std::max(0ll, atoll(e)) << 20 : 0;
}
int amsm_ctx_create(amsm_ctx** out, int curve, int device_id, void* stream) {
  if (!out) return AMSM_E_INVALID_ARG;
  *out = nullptr;
  if (!curve_known(curve)) return AMSM_E_INVALID_ARG;
  if (device_id == AMSM_DEVICE_HOST) {  // the host backend (api_cpu.inc), only ever by explicit request
    if (stream) return AMSM_E_INVALID_ARG;
    amsm_ctx* c = new (std::nothrow) amsm_ctx();
    if (!c) return AMSM_E_OOM;
    c->curve = curve;
    c->device = AMSM_DEVICE_HOST;
    c->host_only = true;
    c->pool_cap_bytes = pool_cap_from_env(c->pool_cap_bytes);
    c->gate.limit = mem_limit_from_env();
    ctx_bind_bufs(c);
    *out = c;
    return AMSM_OK;
  }
  int ndev = amsm_device_count();
  if (ndev <= 0) return AMSM_E_NO_DEVICE;
  if (device_id < 0 || device_id >= ndev) return AMSM_E_INVALID_ARG;
  HIP_TRY(hipSetDevice(device_id));
  amsm_ctx* c = new (std::nothrow) amsm_ctx();
  if (!c) return AMSM_E_OOM;
  c->curve = curve;
  c->device = device_id;
  with_curve(curve, [&](auto cv) {
    for (int i = 0; i < 8; i++) c->r_mod[i] = decltype(cv)::Fr::mod(i);
    return AMSM_OK;
  });
  ctx_bind_bufs(c);
  bool ok = true;
  if (stream) {
    c->stream = (hipStream_t)stream;
  } else {
    ok = ok && hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) == hipSuccess;
    c->own_stream = ok;
  }
  {
    // prep and tail run beside another MSM's accumulate L0, which fills every wave slot: high priority lets their
    // kernels take the slots L0 frees first
    int prio_lo = 0, prio_hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    ok = ok && hipStreamCreateWithPriority(&c->s_prep, hipStreamNonBlocking, prio_hi) == hipSuccess;
    ok = ok && hipStreamCreateWithPriority(&c->s_tail, hipStreamNonBlocking, prio_hi) == hipSuccess;
  }
  for (int k = 0; k < N_SLOTS && ok; k++) {
    for (int i = 0; i <= ST_COUNT && ok; i++) ok = hipEventCreate(&c->slot[k].ev[i]) == hipSuccess;
    ok = ok && hipEventCreate(&c->slot[k].ev_prep_end) == hipSuccess && hipEventCreate(&c->slot[k].ev_l0_end) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&c->slot[k].done, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&c->slot[k].l0_done, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&c->slot[k].prep_done, hipEventDisableTiming) == hipSuccess;
  }
  ok = ok && hipEventCreateWithFlags(&c->fork, hipEventDisableTiming) == hipSuccess;
  ok = ok && hipEventCreateWithFlags(&c->ip_ready, hipEventDisableTiming) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    amsm_ctx_destroy(c);
    return AMSM_E_HIP;
  }
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) == hipSuccess && prop.multiProcessorCount > 0) {
      c->cu_count = prop.multiProcessorCount;
      int per_cu = with_curve(curve, [](auto cv) { return accum_l0_blocks_per_cu<typename decltype(cv)::Fq>(); });
      c->wave_slots = prop.multiProcessorCount * std::max(1, per_cu) * 4;
    }
  }
  // the documented switches (include/amsm.h "Environment")
  c->pool_cap_bytes = pool_cap_from_env(c->pool_cap_bytes);
  c->gate.limit = mem_limit_from_env();
  if (const char* e = getenv("AMSM_BPL")) c->bpl = atoi(e) != 0;
  if (const char* e = getenv("AMSM_BPL_PLAIN")) c->bpl_plain = atoi(e) != 0;
  if (const char* e = getenv("AMSM_TOP_SETS")) {
    const int t = atoi(e);
    c->top_sets = (t == 2 || t == 4 || t == 8) ? t : 0;
  }
  if (const char* e = getenv("AMSM_BPL_PROBE")) c->bpl_probe = atoi(e) != 0;
  if (const char* e = getenv("AMSM_BPS")) c->bps = std::max(0, std::min(2, atoi(e)));
  if (const char* e = getenv("AMSM_BPS_BATCH")) c->bps_batch = std::max(0, std::min((int)msel::BPS_BATCH, atoi(e)));
  if (const char* e = getenv("AMSM_SPLIT_LOG2")) c->split_log2 = std::max(0, std::min(28, atoi(e)));
  if (const char* e = getenv("AMSM_DIRECT_SUM_MAX_LOG2")) c->direct_max_log2 = std::max(0, std::min(16, atoi(e)));
  if (const char* e = getenv("AMSM_TWO_VALUED")) c->two_valued = atoi(e) != 0;
  if (const char* e = getenv("AMSM_SHARE_BUCKETS")) c->share_buckets = atoi(e) != 0;
  if (const char* e = getenv("AMSM_HOST_HALVES")) c->host_halves = atoi(e) != 0;
  if (const char* e = getenv("AMSM_SUBGROUP_LADDER")) c->subgroup_ladder = atoi(e) == 2 ? 2 : 1;
  if (const char* e = getenv("AMSM_VEC_SAMPLE_FORM")) c->vec_sample_form = std::max(0, std::min(2, atoi(e)));
  *out = c;
  return AMSM_OK;
}

void amsm_ctx_destroy(amsm_ctx* c) {
  if (!c) return;
  if (c->parent) return;  // a shard context is borrowed: it goes with its parent
  for (ShardWorker* w : c->workers) delete w;  // joins the threads
  c->workers.clear();
  if (c->rccl_comms) {
    const RcclApi& api = RcclApi::get();
    for (size_t g = 0; g < c->shard_ctx.size(); g++)
      if (c->rccl_comms[g] && api.comm_destroy) (void)api.comm_destroy(c->rccl_comms[g]);
    delete[] c->rccl_comms;
    c->rccl_comms = nullptr;
  }
  for (size_t g = 1; g < c->shard_ctx.size(); g++) {
    c->shard_ctx[g]->parent = nullptr;
    amsm_ctx_destroy(c->shard_ctx[g]);
  }
  c->shard_ctx.clear();
  if (c->host_only) {
    pool_release_all(c);
    pool_forget_ctx(c);
    gate_forget_ctx(c);
    delete c;
    return;
  }
  (void)hipSetDevice(c->device);
  if (c->s_prep) (void)hipStreamSynchronize(c->s_prep);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->s_tail) (void)hipStreamSynchronize(c->s_tail);
  if (c->s_copy) (void)hipStreamSynchronize(c->s_copy);
  if (c->s_tv) (void)hipStreamSynchronize(c->s_tv);
  auto free_buf = [](DevBuf& b) { b.release(); };
  for_each_ctx_buf(c, free_buf);
  for (int k = 0; k < N_SLOTS; k++) {
    Slot* sl = &c->slot[k];
    for_each_slot_buf(sl, free_buf);
    (void)gate_free(sl->h_pinned);
    for (int i = 0; i <= ST_COUNT; i++)
      if (sl->ev[i]) (void)hipEventDestroy(sl->ev[i]);
    if (sl->ev_prep_end) (void)hipEventDestroy(sl->ev_prep_end);
    if (sl->ev_l0_end) (void)hipEventDestroy(sl->ev_l0_end);
    if (sl->done) (void)hipEventDestroy(sl->done);
    if (sl->l0_done) (void)hipEventDestroy(sl->l0_done);
    if (sl->prep_done) (void)hipEventDestroy(sl->prep_done);
  }
  if (c->fork) (void)hipEventDestroy(c->fork);
  if (c->ip_ready) (void)hipEventDestroy(c->ip_ready);
  if (c->s_prep) (void)hipStreamDestroy(c->s_prep);
  if (c->s_tail) (void)hipStreamDestroy(c->s_tail);
  if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
  if (c->s_copy) (void)hipStreamDestroy(c->s_copy);
  for (hipEvent_t e : c->up_ev)
    if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : c->shared_free)
    if (e) (void)hipEventDestroy(e);
  (void)gate_free(c->tv_pinned);
  if (c->s_tv) (void)hipStreamDestroy(c->s_tv);
  if (c->tv_done) (void)hipEventDestroy(c->tv_done);
  pool_release_all(c);
  pool_forget_ctx(c);
  gate_forget_ctx(c);
  if (c->multi_fork) (void)hipEventDestroy(c->multi_fork);
  delete c;
}

static int ctx_create_multi_impl(amsm_ctx*& c, amsm_ctx** out, int curve, const int* device_ids, int n_dev) {
  TRY(amsm_ctx_create(&c, curve, device_ids[0], nullptr));
  c->shard_ctx.push_back(c);
  bool ok = hipEventCreateWithFlags(&c->multi_fork, hipEventDisableTiming) == hipSuccess;
  for (int g = 1; g < n_dev && ok; g++) {
    amsm_ctx* cg = nullptr;
    int rc = amsm_ctx_create(&cg, curve, device_ids[g], nullptr);
    if (rc != AMSM_OK) {
      amsm_ctx_destroy(c);
      c = nullptr;
      return rc;
    }
    cg->parent = c;
    c->shard_ctx.push_back(cg);
    c->workers.push_back(new ShardWorker());
  }
  if (!ok) {
    amsm_ctx_destroy(c);
    c = nullptr;
    return AMSM_E_HIP;
  }
  // A memory limit over several devices' books is not defined yet (include/amsm.h: the setters refuse such a context), so the
  // environment's limit, which amsm_ctx_create gave every shard, does not apply either: it could not be changed or read afterwards
  if (n_dev > 1)
    for (amsm_ctx* cg : c->shard_ctx) cg->gate.limit = 0;
  (void)hipSetDevice(c->device);
  const char* want = getenv("AMSM_COLLECTIVE");  // "rccl" (fail if unavailable) | "peer" | unset (RCCL when possible)
  const bool force_rccl = want && strcmp(want, "rccl") == 0, force_peer = want && strcmp(want, "peer") == 0;
  // (a single device with AMSM_COLLECTIVE=rccl: a one-rank communicator, api_multi.inc ctx_shards_keys)
  if (n_dev > 1 || force_rccl) {
    bool distinct = true;
    for (int a = 0; a < n_dev; a++)
      for (int b = a + 1; b < n_dev; b++) distinct = distinct && device_ids[a] != device_ids[b];
    c->collective = 2;
    if (!force_peer && distinct) {
      const RcclApi& api = RcclApi::get();
      int e = -1;
      if (api.ok) {
        c->rccl_comms = new void*[n_dev]();
        e = api.comm_init_all(c->rccl_comms, n_dev, device_ids);
        (void)hipSetDevice(c->device);
        if (e != 0) {
          fprintf(stderr, "[amsm] ncclCommInitAll failed (%s)%s\n", api.error_string ? api.error_string(e) : "?",
                  force_rccl ? "" : ": falling back to peer copies");
          delete[] c->rccl_comms;
          c->rccl_comms = nullptr;
        }
      }
      if (e == 0) c->collective = 1;
    }
    if (c->collective != 1 && force_rccl) {
      amsm_ctx_destroy(c);
      c = nullptr;
      return AMSM_E_RCCL;
    }
    if (c->collective == 2 && distinct) {  // direct peer copies where the fabric allows (xGMI); else HIP stages them
      for (int a = 0; a < n_dev; a++)
        for (int b = 0; b < n_dev; b++) {
          int can = 0;
          if (a != b && hipDeviceCanAccessPeer(&can, device_ids[a], device_ids[b]) == hipSuccess && can) {
            (void)hipSetDevice(device_ids[a]);
            (void)hipDeviceEnablePeerAccess(device_ids[b], 0);
            (void)hipGetLastError();
          }
        }
      (void)hipSetDevice(c->device);
    }
  }
  *out = c;
  return AMSM_OK;
}
int amsm_ctx_create_multi(amsm_ctx** out, int curve, const int* device_ids, int n_dev) {
  if (!out) return AMSM_E_INVALID_ARG;
  *out = nullptr;
  if (n_dev == 0) return amsm_ctx_create(out, curve, AMSM_DEVICE_HOST, nullptr);  // SURVEY.md 8(b): the host backend
  if (!device_ids || n_dev < 1 || n_dev > 64) return AMSM_E_INVALID_ARG;
  amsm_ctx* c = nullptr;
  // `new ShardWorker` starts a thread (std::system_error when the process is out of threads) and the vectors grow
  // (std::bad_alloc): nothing may unwind through the C ABI
  try {
    return ctx_create_multi_impl(c, out, curve, device_ids, n_dev);
  } catch (const std::bad_alloc&) {
  } catch (const std::system_error&) {
  } catch (...) {
  }
  if (c) amsm_ctx_destroy(c);
  *out = nullptr;
  return AMSM_E_OOM;
}
unsigned long long amsm_ctx_collectives(const amsm_ctx* c) { return c ? c->n_collectives : 0ull; }
unsigned long long amsm_ctx_replicated_msms(const amsm_ctx* c) { return c ? c->n_replicated : 0ull; }
int amsm_ctx_set_replicate_below(amsm_ctx* c, size_t n_generators) {
  if (!c) return AMSM_E_INVALID_ARG;
  c->replicate_below = n_generators;
  return AMSM_OK;
}
int amsm_ctx_pipeline_stats(const amsm_ctx* c, unsigned long long* n_bucket_per_lane, unsigned long long* n_fallbacks) {
  if (!c) return AMSM_E_INVALID_ARG;
  if (n_bucket_per_lane) *n_bucket_per_lane = c->n_bpl;
  if (n_fallbacks) *n_fallbacks = c->n_bpl_fallbacks;
  return AMSM_OK;
}
int amsm_ctx_pipeline_stats_small(const amsm_ctx* c, unsigned long long* n_bucket_split, unsigned long long* n_fallbacks) {
  if (!c) return AMSM_E_INVALID_ARG;
  if (n_bucket_split) *n_bucket_split = c->n_bps;
  if (n_fallbacks) *n_fallbacks = c->n_bps_fallbacks;
  return AMSM_OK;
}
int amsm_ctx_batched_split_stats(const amsm_ctx* c, unsigned long long* n_units, unsigned long long* n_msms, unsigned long long* n_unit_reruns) {
  if (!c) return AMSM_E_INVALID_ARG;
  if (n_units) *n_units = c->n_bps_units;  // (the host backend has no pipelines: zeros)
  if (n_msms) *n_msms = c->n_bps_batched;
  if (n_unit_reruns) *n_unit_reruns = c->n_bps_unit_reruns;
  return AMSM_OK;
}

unsigned long long amsm_ctx_two_valued_msms(const amsm_ctx* c) { return c ? c->n_two_valued : 0ull; }
unsigned long long amsm_ctx_heavy_buckets(const amsm_ctx* c) { return c ? c->n_heavy_buckets : 0ull; }
unsigned long long amsm_ctx_unit_scalar_msms(const amsm_ctx* c) { return c ? c->n_ones_split : 0ull; }
unsigned long long amsm_ctx_direct_sum_msms(const amsm_ctx* c) { return c ? c->n_direct : 0ull; }
unsigned long long amsm_ctx_shared_bucket_msms(const amsm_ctx* c) { return c ? c->n_shared : 0ull; }
unsigned long long amsm_ctx_top_sets_msms(const amsm_ctx* c, int sets) {
  return (c && (sets == 2 || sets == 4 || sets == 8)) ? c->n_top_sets[sets / 4] : 0ull;
}
unsigned long long amsm_ctx_tables_denied(const amsm_ctx* c) {
  if (!c) return 0ull;
  unsigned long long n = c->n_tables_denied;
  for (size_t g = 1; g < c->shard_ctx.size(); g++) n += c->shard_ctx[g]->n_tables_denied;
  return n;
}
int amsm_ctx_set_table_budget(amsm_ctx* c, size_t bytes) {
  if (!c) return AMSM_E_INVALID_ARG;
  c->table_budget = bytes;
  for (size_t g = 1; g < c->shard_ctx.size(); g++) c->shard_ctx[g]->table_budget = bytes;
  return AMSM_OK;
}

// ---- the allocation gate (api_gate.inc) ----
int amsm_ctx_set_memory_limit(amsm_ctx* c, size_t bytes) {
  if (!c) return AMSM_E_INVALID_ARG;
  if (c->shard_ctx.size() > 1 || c->parent) return AMSM_E_UNSUPPORTED;  // (one limit over several devices' books: not defined yet)
  std::lock_guard<std::mutex> lk(gate_mu());
  c->gate.limit = bytes;
  c->gate.peak = c->gate.held;  // the peak is counted anew: what was held at most BEFORE the limit says nothing about the limit
  return AMSM_OK;
}
int amsm_ctx_memory_held(const amsm_ctx* c, size_t out[4]) {
  if (!c || !out) return AMSM_E_INVALID_ARG;
  std::lock_guard<std::mutex> lk(gate_mu());
  out[0] = c->gate.held;
  out[1] = c->gate.peak;
  out[2] = c->gate.limit;
  out[3] = c->gate.pinned;
  return AMSM_OK;
}
int amsm_ctx_fail_alloc_after(amsm_ctx* c, long n) {
  if (!c) return AMSM_E_INVALID_ARG;
  if (c->shard_ctx.size() > 1 || c->parent) return AMSM_E_UNSUPPORTED;
  std::lock_guard<std::mutex> lk(gate_mu());
  c->gate.fail_after = n < 0 ? -1 : n;
  return AMSM_OK;
}
int amsm_ctx_alloc_stats(const amsm_ctx* c, unsigned long long out[4]) {
  if (!c || !out) return AMSM_E_INVALID_ARG;
  std::lock_guard<std::mutex> lk(gate_mu());
  out[0] = c->gate.requests;
  out[1] = c->gate.refused_limit;
  out[2] = c->gate.refused_hook;
  out[3] = c->gate.failed_driver;
  return AMSM_OK;
}

int amsm_ctx_num_devices(const amsm_ctx* c) { return c ? (int)n_shards(c) : AMSM_E_INVALID_ARG; }
amsm_ctx* amsm_ctx_shard(amsm_ctx* c, int g) {
  if (!c || g < 0 || (size_t)g >= n_shards(c)) return nullptr;
  return c->shard_ctx.empty() ? c : c->shard_ctx[g];
}
const char* amsm_ctx_collective(const amsm_ctx* c) {
  if (!c) return "none";
  return c->collective == 1 ? "rccl" : (c->collective == 2 ? "peer-copy" : "none");
}

int amsm_ctx_is_host(const amsm_ctx* c) { return c && c->host_only ? 1 : 0; }
int amsm_ctx_curve(const amsm_ctx* c) { return c ? c->curve : AMSM_E_INVALID_ARG; }
int amsm_ctx_fq_limbs(const amsm_ctx* c) { return !c ? AMSM_E_INVALID_ARG : curve_fq_limbs(c->curve); }
int amsm_ctx_set_window(amsm_ctx* c, int bits) {
  if (!c || (bits != 0 && (bits < 2 || bits > 24))) return AMSM_E_INVALID_ARG;
  c->window_override = bits;
  return AMSM_OK;
}
int amsm_ctx_set_vec_grid_max(amsm_ctx* c, unsigned max_workgroups) {
  if (!c) return AMSM_E_INVALID_ARG;
  c->vec_grid_max = max_workgroups;
  for (size_t g = 1; g < c->shard_ctx.size(); g++) c->shard_ctx[g]->vec_grid_max = max_workgroups;
  return AMSM_OK;
}
int amsm_ctx_vec_grid(const amsm_ctx* c, size_t n, unsigned* stream_workgroups, unsigned* reduce_workgroups) {
  if (!c || n >= (1ull << 32)) return AMSM_E_INVALID_ARG;
  if (stream_workgroups) *stream_workgroups = vec_stream_grid((u32)n, vec_grid_of(c));
  if (reduce_workgroups) *reduce_workgroups = vec_reduce_grid((u32)n, vec_grid_of(c));
  return AMSM_OK;
}
int amsm_ctx_synchronize(amsm_ctx* c) {
  if (!c) return AMSM_E_INVALID_ARG;
  if (c->host_only) return AMSM_OK;  // every host-backend call is synchronous
  for (size_t g = 1; g < c->shard_ctx.size(); g++) TRY(amsm_ctx_synchronize(c->shard_ctx[g]));
  TRY(bind_device(c));
  HIP_TRY(hipStreamSynchronize(c->s_prep));
  HIP_TRY(hipStreamSynchronize(c->stream));
  HIP_TRY(hipStreamSynchronize(c->s_tail));
  return AMSM_OK;
}
int amsm_ctx_set_profiling(amsm_ctx* c, int on) {
  if (!c) return AMSM_E_INVALID_ARG;
  c->profiling = on != 0;
  return AMSM_OK;
}
int amsm_stage_count(void) { return ST_COUNT; }
const char* amsm_stage_name(int s) { return (s >= 0 && s < ST_COUNT) ? kStageNames[s] : ""; }
int amsm_ctx_stage_ms(amsm_ctx* c, int s, float* ms) {
  if (!c || !ms || s < 0 || s >= ST_COUNT) return AMSM_E_INVALID_ARG;
  *ms = c->stage_ms[s];
  return AMSM_OK;
}
