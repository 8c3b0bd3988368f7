// Part of api.hip (inside its anonymous namespace): multi-device contexts -- sharded keys, per-device workers, the RCCL / peer
// exchange of partial sums.
// =============================================================================================
// Multi-device contexts: ONE process drives the GPUs of a node.  The key is sharded over the devices by contiguous ranges
// (the split of accumulation_amd/dist.py: shard_bounds); every device runs the ordinary single-device pipeline on its
// shard, driven by its own host thread; the per-device partial sums (one folded XYZZ record per MSM) are gathered on the
// primary device with one RCCL all-gather (raw bytes: EC addition is not an RCCL reduce op) or peer copies, folded and
// normalised once.
// =============================================================================================
// RCCL is bound at run time (dlopen): libamsm.so carries no link-time dependency on it, a process that already loaded a
// copy (PyTorch ships its own) keeps using that one, and a box without RCCL still gets the peer-copy exchange.
struct RcclApi {
  typedef int (*comm_init_all_t)(void** comms, int ndev, const int* devlist);
  typedef int (*comm_destroy_t)(void* comm);
  typedef int (*all_gather_t)(const void* send, void* recv, size_t count, int datatype, void* comm, hipStream_t st);
  typedef int (*group_t)();
  typedef const char* (*err_t)(int);
  comm_init_all_t comm_init_all = nullptr;
  comm_destroy_t comm_destroy = nullptr;
  all_gather_t all_gather = nullptr;
  group_t group_start = nullptr, group_end = nullptr;
  err_t error_string = nullptr;
  bool ok = false;
  static const RcclApi& get() {
    static RcclApi api = [] {
      RcclApi a;
      void* h = nullptr;
      const char* names[] = {"librccl.so", "librccl.so.1"};
      for (const char* n : names)  // a copy that is already in the process first
        if (!h) h = dlopen(n, RTLD_NOW | RTLD_NOLOAD);
      for (const char* n : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"})
        if (!h) h = dlopen(n, RTLD_NOW | RTLD_LOCAL);
      if (!h) return a;
      a.comm_init_all = (comm_init_all_t)dlsym(h, "ncclCommInitAll");
      a.comm_destroy = (comm_destroy_t)dlsym(h, "ncclCommDestroy");
      a.all_gather = (all_gather_t)dlsym(h, "ncclAllGather");
      a.group_start = (group_t)dlsym(h, "ncclGroupStart");
      a.group_end = (group_t)dlsym(h, "ncclGroupEnd");
      a.error_string = (err_t)dlsym(h, "ncclGetErrorString");
      a.ok = a.comm_init_all && a.comm_destroy && a.all_gather && a.group_start && a.group_end;
      return a;
    }();
    return api;
  }
};
constexpr int kNcclUint8 = 1;  // rccl.h: ncclUint8

inline size_t n_shards(const amsm_ctx* c) { return c->shard_ctx.empty() ? 1 : c->shard_ctx.size(); }
inline bool key_sharded(const amsm_bases* b) { return !b->shards.empty(); }
// Does this context build sharded keys?  More than one device -- or ONE device with an RCCL communicator (AMSM_COLLECTIVE=rccl
// on a single-device list, round 4): the whole sharded path, ncclAllGather included, then runs with one rank, so that a box
// with one GPU executes the code an 8-GPU node will
inline bool ctx_shards_keys(const amsm_ctx* c) { return n_shards(c) > 1 || c->collective == 1; }

// dist.shard_bounds: the first n % world shards get one extra element
std::vector<size_t> shard_bounds(size_t n, size_t world) {
  std::vector<size_t> b(world + 1);
  size_t q = n / world, r = n % world;
  for (size_t g = 0; g <= world; g++) b[g] = g * q + std::min(g, r);
  return b;
}

// Run job(g) for every shard: shard 0 on the calling thread, the others on their workers.  Returns the first error.
template <class F>
int for_each_shard(amsm_ctx* c, F&& job) {
  const size_t N = n_shards(c);
  std::vector<int> rc(N, AMSM_OK);
  // nothing may unwind through a worker thread (std::terminate) or out of the C ABI: allocation failures inside a job
  // (std::vector growth, `new`) become AMSM_E_OOM
  auto guarded = [&](size_t g) -> int {
    try {
      return job(g);
    } catch (const std::bad_alloc&) {
      return AMSM_E_OOM;
    } catch (...) {
      return AMSM_E_HIP;
    }
  };
  for (size_t g = 1; g < N; g++) c->workers[g - 1]->submit([&, g] { rc[g] = guarded(g); });
  rc[0] = guarded(0);
  for (size_t g = 1; g < N; g++) c->workers[g - 1]->wait();
  (void)hipSetDevice(c->device);
  for (size_t g = 0; g < N; g++)
    if (rc[g] != AMSM_OK) return rc[g];
  return AMSM_OK;
}

enum SliceKind {
  SLICE_HOST,     // srcs[v]: host scalars of vector v (whole vector)
  SLICE_PRIMARY,  // srcs[v]: device pointer on the primary device (whole vector)
  SLICE_SHARDED   // srcs[v * N + g]: shard g's slice of vector v, resident on device g
};

// One shard's part of a GROUPED MSM (two sums by bit `shift` of the scalar's position in the WHOLE vector: the IPA rounds): the
// shard holds positions [pos0, pos0 + cnt).  Where its slice starts on a multiple of the group period the shard's own grouped
// MSM has the same classes; a slice (or its ragged ends) inside ONE half-period is a plain MSM for that class.  The two class sums
// come back ON THE HOST (r[0], r[1]): every piece ends in a host-side collect anyway, and a round of an IPA opening is a latency
// chain -- sending two records back to the device for an all-gather and down again cost three more synchronisations per round.
// (Round 5: grouped MSMs and the IPA round over sharded keys.)
template <class Fq, class Fr>
int msm_grouped_partial(amsm_ctx* cg, const amsm_bases* shard_key, size_t key_off, const void* d_scalars, size_t cnt, int mont,
                        unsigned shift, size_t pos0, host::HXYZZ<Fq>* r) {
  const size_t half = (size_t)1 << shift, period = half << 1;
  r[0] = r[1] = host::hx_inf<Fq>();
  size_t p = pos0;
  const size_t end = pos0 + cnt;
  auto plain = [&](size_t a, size_t b) -> int {
    host::HXYZZ<Fq> s;
    TRY((msm_device_xyzz<Fq, Fr>(cg, shard_key, key_off + (a - pos0), (const char*)d_scalars + (a - pos0) * 32, b - a, mont, &s)));
    const int grp = (int)((a >> shift) & 1u);
    r[grp] = host::hx_add<Fq>(r[grp], s);
    return AMSM_OK;
  };
  while (p < end && (p % period) != 0) {  // ragged head: pieces inside one half-period each
    const size_t stop = std::min(end, (p / half + 1) * half);
    TRY(plain(p, stop));
    p = stop;
  }
  const size_t mid_end = p + ((end - p) / period) * period;
  if (mid_end > p) {  // whole periods: the shard's own grouped MSM
    host::HXYZZ<Fq> s[2];
    stage_begin(cg);
    TRY(prep_fork(cg));
    const MsmJob whole = single_job(shard_key, key_off + (p - pos0), (const char*)d_scalars + (p - pos0) * 32, mid_end - p, mont, (int)shift);
    TRY((msm_enqueue<Fq, Fr>(cg, &cg->slot[0], whole, Place::LONE)));
    int rc = msm_collect<Fq>(cg, &cg->slot[0], s);
    stage_end(cg);
    if (rc != AMSM_OK) return rc;
    r[0] = host::hx_add<Fq>(r[0], s[0]);
    r[1] = host::hx_add<Fq>(r[1], s[1]);
    p = mid_end;
  }
  while (p < end) {  // ragged tail
    const size_t stop = std::min(end, (p / half + 1) * half);
    TRY(plain(p, stop));
    p = stop;
  }
  return AMSM_OK;
}

// n_vecs MSMs over generators [base_off, base_off + n) of a sharded key -> one XYZZ per vector on the host.
// group_shift >= 0 (n_vecs = 1): the two sums of a grouped MSM -> (*out)[0], (*out)[1].
template <class Fq, class Fr>
int msm_sharded(amsm_ctx* c, const amsm_bases* key, size_t base_off, size_t n, size_t n_vecs, int mont, SliceKind kind,
                const void* const* srcs, std::vector<host::HXYZZ<Fq>>* out, int group_shift = -1) {
  const size_t N = n_shards(c);
  const size_t G = group_shift >= 0 ? 2 : 1;  // records per vector
  if (G == 2 && n_vecs != 1) return AMSM_E_INVALID_ARG;
  out->assign(n_vecs * G, host::hx_inf<Fq>());
  if (base_off > key->n) return AMSM_E_INVALID_ARG;
  const size_t n_eff = std::min(n, key->n - base_off);
  if (n_vecs == 0 || n_eff == 0) return AMSM_OK;
  const size_t rec = xyzz_bytes<Fq>(), per = n_vecs * G * rec;
  if (kind == SLICE_PRIMARY) HIP_TRY(hipEventRecord(c->multi_fork, c->stream));  // the producers of the vectors
  const bool rccl = c->collective == 1;
  std::vector<host::HXYZZ<Fq>> grouped_part(G == 2 ? 2 * N : 0, host::hx_inf<Fq>());  // shard g's two class sums (host)
  TRY(for_each_shard(c, [&](size_t g) -> int {
    amsm_ctx* cg = c->shard_ctx[g];
    HIP_TRY(hipSetDevice(cg->device));
    const size_t lo = std::max(key->bound[g], base_off), hi = std::min(key->bound[g + 1], base_off + n_eff);
    const size_t cnt = hi > lo ? hi - lo : 0;
    if (G == 2 && cnt == 0) return AMSM_OK;
    if (G == 1) {
      TRY(ensure(cg->rec_send, per));
      if (rccl) TRY(ensure(cg->rec_recv, N * per));
    }
    if (cnt == 0) {  // this shard holds none of the range: identity records (ZZ = 0)
      HIP_TRY(hipMemsetAsync(cg->rec_send.p, 0, per, cg->stream));
      HIP_TRY(hipStreamSynchronize(cg->stream));
      return AMSM_OK;
    }
    std::vector<const void*> ptrs(n_vecs);
    const size_t skip = (lo - base_off) * 32, bytes = cnt * 32;
    if (kind == SLICE_SHARDED) {
      for (size_t v = 0; v < n_vecs; v++) ptrs[v] = srcs[v * N + g];
    } else if (kind == SLICE_PRIMARY && g == 0) {
      for (size_t v = 0; v < n_vecs; v++) ptrs[v] = (const char*)srcs[v] + skip;
    } else {
      TRY(ensure(cg->stage, n_vecs * bytes));
      if (kind == SLICE_PRIMARY) HIP_TRY(hipStreamWaitEvent(cg->stream, c->multi_fork, 0));
      for (size_t v = 0; v < n_vecs; v++) {
        char* dst = (char*)cg->stage.p + v * bytes;
        const char* src = (const char*)srcs[v] + skip;
        if (kind == SLICE_HOST)
          HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, cg->stream));
        else
          HIP_TRY(hipMemcpyPeerAsync(dst, cg->device, src, c->device, bytes, cg->stream));
        ptrs[v] = dst;
      }
    }
    if (G == 2)
      return msm_grouped_partial<Fq, Fr>(cg, key->shards[g], lo - key->bound[g], ptrs[0], cnt, mont, (unsigned)group_shift, lo - base_off,
                                         &grouped_part[2 * g]);
    return msm_partial_batch_impl<Fq, Fr>(cg, key->shards[g], lo - key->bound[g], ptrs.data(), n_vecs, cnt, mont,
                                          cg->rec_send.p);
  }));
  if (G == 2) {  // the class sums are on the host already: fold them here (no device exchange on this latency-bound path)
    for (size_t g = 0; g < N; g++)
      for (size_t k = 0; k < 2; k++) (*out)[k] = host::hx_add<Fq>((*out)[k], grouped_part[2 * g + k]);
    c->n_host_gathers++;
    return AMSM_OK;
  }
  // exchange: every shard's records -> the primary (rank-major: record (g, v) at (g * n_vecs + v) * rec)
  TRY(ensure(c->rec_recv, N * per));
  if (rccl) {
    const RcclApi& api = RcclApi::get();
    // an error inside the group must not leave it open (every later collective on these communicators would wedge) nor
    // the calling thread on another device: record it, always close the group, go back to the primary, then report
    int e = api.group_start();
    hipError_t he = hipSuccess;
    for (size_t g = 0; g < N && e == 0 && he == hipSuccess; g++) {
      amsm_ctx* cg = c->shard_ctx[g];
      he = hipSetDevice(cg->device);
      if (he == hipSuccess)
        e = api.all_gather(cg->rec_send.p, cg->rec_recv.p, per, kNcclUint8, c->rccl_comms[g], cg->stream);
    }
    int e2 = api.group_end();
    (void)hipSetDevice(c->device);
    if (he != hipSuccess) {
      fprintf(stderr, "[amsm] hipSetDevice failed inside the RCCL group: %s\n", hipGetErrorName(he));
      return AMSM_E_HIP;
    }
    if (e != 0 || e2 != 0) {
      fprintf(stderr, "[amsm] RCCL all-gather failed: %s\n", api.error_string ? api.error_string(e ? e : e2) : "?");
      return AMSM_E_RCCL;
    }
    c->n_collectives++;
  } else {
    for (size_t g = 0; g < N; g++) {
      amsm_ctx* cg = c->shard_ctx[g];  // its records are complete: msm_partial_batch_impl synchronised cg's stream
      HIP_TRY(hipMemcpyPeerAsync((char*)c->rec_recv.p + g * per, c->device, cg->rec_send.p, cg->device, per, c->stream));
    }
    c->n_collectives++;
  }
  Slot* sl = &c->slot[0];
  TRY(ensure_pinned(sl, N * per + 64));
  HIP_TRY(hipMemcpyAsync(sl->h_pinned, c->rec_recv.p, N * per, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  const u32* h = (const u32*)sl->h_pinned;
  for (size_t v = 0; v < n_vecs * G; v++)
    for (size_t g = 0; g < N; g++)
      (*out)[v] = host::hx_add<Fq>((*out)[v], host::hx_from_device<Fq>(h + (g * n_vecs * G + v) * (rec / 4)));
  return AMSM_OK;
}

// The IPA opening round over a SHARDED key (round 5): the vector half on the primary device (where the coefficient and evaluation
// vectors live), the round's scalars peer-copied to the shards slice by slice, the grouped MSM as msm_sharded's two-record form --
// one exchange per round.  (The single-device form reserves every allocation before it folds the vectors in place; here the shards
// allocate inside their MSMs: an out-of-memory return leaves the vectors CONSUMED, like any later error.)
template <class Fq, class Fr>
int ipa_round_sharded_impl(amsm_ctx* ctx, const amsm_bases* key, const uint64_t* xi_mont, size_t j, size_t log_key, const void* d_coeffs,
                           const void* d_z, size_t half, void* d_u, uint64_t* out_lr_xy, uint8_t* out_lr_inf, uint64_t* out_ip_mont,
                           const uint64_t* fold_x_mont, const uint64_t* h_prime_xy) {
  const size_t n = (size_t)1 << log_key;
  if (n > key->n) return AMSM_E_INVALID_ARG;
  u32 blocks = 0;
  TRY((ipa_round_vectors<Fr>(ctx, xi_mont, j, log_key, d_coeffs, d_z, half, d_u, fold_x_mont, &blocks)));
  std::vector<host::HXYZZ<Fq>> r;
  const void* src = d_u;
  TRY((msm_sharded<Fq, Fr>(ctx, key, 0, n, 1, 1, SLICE_PRIMARY, &src, &r, (int)(log_key - 1 - j))));
  host::HXYZZ<Fq> hterm[2];
  TRY((ipa_round_inner_products<Fq, Fr>(ctx, blocks, h_prime_xy, out_ip_mont, hterm)));
  if (h_prime_xy)
    for (int k = 0; k < 2; k++) r[k] = host::hx_add<Fq>(r[k], hterm[k]);
  write_affine_batch<Fq>(r, out_lr_xy, out_lr_inf);
  return AMSM_OK;
}

// A sharded key: make_shard(g, ctx_g, lo, cnt, &shard) builds shard g on its device.
template <class F>
int bases_create_sharded(amsm_ctx* c, size_t n, amsm_bases** out, F&& make_shard) {
  const size_t N = n_shards(c);
  amsm_bases* b = new (std::nothrow) amsm_bases();
  if (!b) return AMSM_E_OOM;
  b->curve = c->curve;
  b->device = c->device;
  b->n = n;
  b->owner = c;
  b->bound = shard_bounds(n, N);
  b->shards.assign(N, nullptr);
  int rc = for_each_shard(c, [&](size_t g) -> int {
    amsm_ctx* cg = c->shard_ctx[g];
    HIP_TRY(hipSetDevice(cg->device));
    return make_shard(g, cg, b->bound[g], b->bound[g + 1] - b->bound[g], &b->shards[g]);
  });
  if (rc != AMSM_OK) {
    for (amsm_bases* s : b->shards) amsm_bases_free(s);
    delete b;
    return rc;
  }
  b->precomp = 1;
  for (amsm_bases* s : b->shards) b->precomp &= s->precomp;
  *out = b;
  return AMSM_OK;
}

// A REPLICATED key (AMSM_BASES_REPLICATE, round 6): make_copy(g, ctx_g, &key_g) builds the WHOLE key on device g; the primary's
// copy is the handle the caller gets (an ordinary single-device key to every entry point), the others hang off it.
template <class F>
int bases_create_replicated(amsm_ctx* c, amsm_bases** out, F&& make_copy) {
  const size_t N = n_shards(c);
  std::vector<amsm_bases*> copies(N, nullptr);
  int rc = for_each_shard(c, [&](size_t g) -> int {
    amsm_ctx* cg = c->shard_ctx[g];
    HIP_TRY(hipSetDevice(cg->device));
    return make_copy(g, cg, &copies[g]);
  });
  if (rc != AMSM_OK) {
    for (amsm_bases* s : copies) amsm_bases_free(s);
    return rc;
  }
  if (N > 1) {
    copies[0]->replicas = copies;
    copies[0]->replicas[0] = nullptr;
    copies[0]->owner = c;
  }
  *out = copies[0];
  return AMSM_OK;
}
inline bool key_replicated(const amsm_bases* b) { return !b->replicas.empty(); }
inline bool wants_replicas(const amsm_ctx* c, size_t n, unsigned flags) {
  return n_shards(c) > 1 && ((flags & AMSM_BASES_REPLICATE) != 0 || (c->replicate_below && n <= c->replicate_below));
}

// n_vecs INDEPENDENT MSMs over a replicated key, dealt round-robin: MSM v runs whole on device v mod N through that device's
// ordinary batch pipeline (its own worker thread), the sums come back to the host per device -- no partial records, no exchange.
// kind: SLICE_HOST (srcs[v] host scalars, uploaded straight to their device) or SLICE_PRIMARY (device vectors on the primary:
// peer-copied whole to the device that runs them).  ns[v] pairs each (cut to the key like every entry point cuts them).
template <class Fq, class Fr>
int msm_replicated(amsm_ctx* c, const amsm_bases* key, size_t base_off, const size_t* ns, size_t n_vecs, int mont, SliceKind kind,
                   const void* const* srcs, std::vector<host::HXYZZ<Fq>>* out) {
  const size_t N = n_shards(c);
  out->assign(n_vecs, host::hx_inf<Fq>());
  if (base_off > key->n) return AMSM_E_INVALID_ARG;
  if (n_vecs == 0) return AMSM_OK;
  if (kind == SLICE_PRIMARY) HIP_TRY(hipEventRecord(c->multi_fork, c->stream));  // the producers of the vectors
  TRY(for_each_shard(c, [&](size_t g) -> int {
    amsm_ctx* cg = c->shard_ctx[g];
    const amsm_bases* kg = g == 0 ? key : key->replicas[g];
    std::vector<size_t> mine;
    for (size_t v = g; v < n_vecs; v += N) mine.push_back(v);
    if (mine.empty()) return AMSM_OK;
    HIP_TRY(hipSetDevice(cg->device));
    const size_t k = mine.size();
    std::vector<size_t> offs(k, base_off), lens(k);
    std::vector<const void*> ptrs(k);
    size_t total = 0;
    for (size_t i = 0; i < k; i++) {
      lens[i] = std::min(ns[mine[i]], key->n - base_off);
      ptrs[i] = srcs[mine[i]];
      total += lens[i] * 32;
    }
    std::vector<host::HXYZZ<Fq>> r;
    if (kind == SLICE_HOST) {
      TRY((msm_multi_host_xyzz<Fq, Fr>(cg, kg, k, offs.data(), (const uint64_t* const*)ptrs.data(), lens.data(), mont, &r)));
    } else {
      if (g != 0) {
        TRY(ensure(cg->stage, std::max<size_t>(total, 32)));
        HIP_TRY(hipStreamWaitEvent(cg->stream, c->multi_fork, 0));
        size_t at = 0;
        for (size_t i = 0; i < k; i++) {
          char* dst = (char*)cg->stage.p + at;
          if (lens[i]) HIP_TRY(hipMemcpyPeerAsync(dst, cg->device, ptrs[i], c->device, lens[i] * 32, cg->stream));
          ptrs[i] = dst;
          at += lens[i] * 32;
        }
      }
      std::vector<MsmJob> vecs;
      TRY(jobs_from_arrays(kg, k, offs.data(), ptrs.data(), lens.data(), mont, &vecs));
      TRY((msm_multi_split_xyzz<Fq, Fr>(cg, vecs, &r)));
    }
    for (size_t i = 0; i < k; i++) (*out)[mine[i]] = r[i];
    return AMSM_OK;
  }));
  c->n_replicated += n_vecs - (n_vecs + N - 1) / N;
  return AMSM_OK;
}

// ... to affine points, with the optional r_v * hiding_generator terms of a Pedersen commitment batch (a11: host)
template <class Fq, class Fr>
int msm_replicated_affine(amsm_ctx* c, const amsm_bases* key, size_t base_off, const size_t* ns, size_t n_vecs, int mont, SliceKind kind,
                          const void* const* srcs, const uint64_t* const* rand_mont, const uint64_t* hiding_xy, uint64_t* out_xy,
                          uint8_t* out_inf) {
  std::vector<host::HXYZZ<Fq>> r;
  TRY((msm_replicated<Fq, Fr>(c, key, base_off, ns, n_vecs, mont, kind, srcs, &r)));
  if (rand_mont && hiding_xy) {
    const host::HXYZZ<Fq> h = host::hx_from_affine<Fq>(hiding_xy, false);
    HostPool::get().run(n_vecs, [&](size_t v) {
      if (!rand_mont[v]) return;
      host::HFe<Fr> k;
      memcpy(k.v, rand_mont[v], 32);
      k = host::h_from_mont<Fr>(k);
      r[v] = host::hx_add<Fq>(r[v], host::hx_mul<Fq>(h, k.v));
    });
  }
  write_affine_batch<Fq>(r, out_xy, out_inf);
  return AMSM_OK;
}

// Does (ctx, key) form a valid pair?  A sharded key needs the multi-device context that made it.
inline bool key_matches(const amsm_ctx* c, const amsm_bases* b) {
  if (b->curve != c->curve) return false;
  if (key_sharded(b)) return b->owner == c && b->shards.size() == n_shards(c);
  return b->device == c->device;
}

// commit(ck, v, r) over a sharded key: the sharded MSM, then + r * hiding_generator on the host (a11)
template <class Fq, class Fr>
int pedersen_sharded_impl(amsm_ctx* c, const amsm_bases* ck, size_t n, SliceKind kind, const void* const* src,
                                 const uint64_t* rand_mont, const uint64_t* hiding_xy, uint64_t* out_xy, uint8_t* out_inf) {
  std::vector<host::HXYZZ<Fq>> r;
  TRY((msm_sharded<Fq, Fr>(c, ck, 0, n, 1, 1, kind, src, &r)));
  host::HXYZZ<Fq> acc = r[0];
  if (rand_mont && hiding_xy) {
    host::HFe<Fr> k;
    memcpy(k.v, rand_mont, 32);
    k = host::h_from_mont<Fr>(k);
    acc = host::hx_add<Fq>(acc, host::hx_mul<Fq>(host::hx_from_affine<Fq>(hiding_xy, false), k.v));
  }
  write_affine<Fq>(acc, out_xy, out_inf);
  return AMSM_OK;
}

// ---- amsm_msm_oneshot (round 6) ---------------------------------------------------------------------------------------------
// One shard's (or the only device's) part of amsm_msm_oneshot: a temporary plain key over the context's one-shot buffer, ranges of
// 2^19 pairs whose generators and scalars ride the copy stream in front of their MSM (api_pipeline.inc: OneshotBases)
template <class Fq, class Fr>
int msm_oneshot_impl(amsm_ctx* c, const uint64_t* xy, const uint8_t* is_inf, const uint64_t* scalars, size_t n, int mont,
                            host::HXYZZ<Fq>* out) {
  *out = host::hx_inf<Fq>();
  if (!n) return AMSM_OK;
  HIP_TRY(hipSetDevice(c->device));
  TRY(ensure(c->oneshot_table, n * affine_bytes<Fq>()));
  if (is_inf) TRY(ensure(c->oneshot_inf, n));
  amsm_bases key;  // plain: no levels, no tables, nothing owned (the buffer is the context's)
  key.curve = c->curve;
  key.device = c->device;
  key.n = n;
  key.d_table = (u32*)c->oneshot_table.p;
  OneshotBases os;
  os.xy = xy;
  os.is_inf = is_inf;
  os.step = n > tune::ONESHOT_RANGE ? tune::ONESHOT_RANGE : 0;
  const size_t off = 0;
  std::vector<host::HXYZZ<Fq>> r;
  TRY((msm_multi_host_xyzz<Fq, Fr>(c, &key, 1, &off, &scalars, &n, mont, &r, &os)));
  *out = r[0];
  return AMSM_OK;
}
template <class Fq, class Fr>
int msm_oneshot_any(amsm_ctx* c, const uint64_t* xy, const uint8_t* is_inf, const uint64_t* scalars, size_t n, int mont,
                           uint64_t* out_xy, uint8_t* out_inf) {
  const size_t N = n_shards(c), PW = 2 * (size_t)amsm_ctx_fq_limbs(c);
  std::vector<host::HXYZZ<Fq>> part(N, host::hx_inf<Fq>());
  if (N == 1) {
    TRY((msm_oneshot_impl<Fq, Fr>(c, xy, is_inf, scalars, n, mont, &part[0])));
  } else {  // every device takes a contiguous range of the pairs (dist.shard_bounds); the N sums are folded on the host: no exchange
    const std::vector<size_t> b = shard_bounds(n, N);
    TRY(for_each_shard(c, [&](size_t g) {
      return msm_oneshot_impl<Fq, Fr>(c->shard_ctx[g], xy + b[g] * PW, is_inf ? is_inf + b[g] : nullptr, scalars + b[g] * 4, b[g + 1] - b[g],
                                      mont, &part[g]);
    }));
  }
  host::HXYZZ<Fq> acc = part[0];
  for (size_t g = 1; g < N; g++) acc = host::hx_add<Fq>(acc, part[g]);
  write_affine<Fq>(acc, out_xy, out_inf);
  return AMSM_OK;
}
