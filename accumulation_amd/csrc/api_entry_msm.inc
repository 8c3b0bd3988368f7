// Part of api.hip (inside extern "C"): keys, MSM entry points, partial records, Pedersen commitments.
int amsm_bases_load(amsm_ctx* c, const uint64_t* xy, const uint8_t* is_inf, size_t n, unsigned flags, amsm_bases** out) {
  if (!c || !out || (n && !xy)) return AMSM_E_INVALID_ARG;
  if (n >= (1ull << 31)) return AMSM_E_UNSUPPORTED;
  if (c->host_only) return CPU_CALL(c, bases_load, c, xy, is_inf, n, flags, out);
  TRY(bind_device(c));
  if (wants_replicas(c, n, flags))  // (round 6) every device loads the whole key
    return bases_create_replicated(c, out, [&](size_t g, amsm_ctx* cg, amsm_bases** o) {
      // (AMSM_BASES_CHECK: the points are the same on every device -- the primary checks them, once)
      const unsigned f = flags & ~(unsigned)(AMSM_BASES_REPLICATE | (g ? AMSM_BASES_CHECK : 0));
      return DISPATCH(cg, bases_load_impl<Fq, Fr>(cg, xy, is_inf, n, f, o));
    });
  flags &= ~(unsigned)AMSM_BASES_REPLICATE;
  if (ctx_shards_keys(c)) {  // shard g copies its own range of the caller's arrays
    const size_t L2 = 2 * (size_t)amsm_ctx_fq_limbs(c);
    return bases_create_sharded(c, n, out, [&](size_t, amsm_ctx* cg, size_t lo, size_t cnt, amsm_bases** o) {
      // the impl, not the entry point: shard 0's context IS this (multi-device) context
      return DISPATCH(cg, bases_load_impl<Fq, Fr>(cg, xy + lo * L2, is_inf ? is_inf + lo : nullptr, cnt, flags, o));
    });
  }
  return DISPATCH(c, bases_load_impl<Fq, Fr>(c, xy, is_inf, n, flags, out));
}
int amsm_bases_generate(amsm_ctx* c, uint64_t seed, size_t n, unsigned flags, amsm_bases** out) {
  if (!c || !out || (flags & AMSM_BASES_CHECK)) return AMSM_E_INVALID_ARG;  // (its points are valid by construction)
  if (n >= (1ull << 31)) return AMSM_E_UNSUPPORTED;
  if (c->host_only) return CPU_CALL(c, bases_generate, c, seed, n, flags, out);
  TRY(bind_device(c));
  if (wants_replicas(c, n, flags))  // (round 6) every device generates the whole key
    return bases_create_replicated(c, out, [&](size_t, amsm_ctx* cg, amsm_bases** o) {
      return DISPATCH(cg, bases_generate_impl<Fq, Fr>(cg, seed, n, flags & ~(unsigned)AMSM_BASES_REPLICATE, o));
    });
  flags &= ~(unsigned)AMSM_BASES_REPLICATE;
  if (ctx_shards_keys(c))  // shard g generates its own range of the synthetic stream
    return bases_create_sharded(c, n, out, [&](size_t, amsm_ctx* cg, size_t lo, size_t cnt, amsm_bases** o) {
      return DISPATCH(cg, bases_generate_impl<Fq, Fr>(cg, seed, cnt, flags, o, lo));
    });
  return DISPATCH(c, bases_generate_impl<Fq, Fr>(c, seed, n, flags, out));
}
int amsm_bases_sample(amsm_ctx* c, const uint8_t* domain, size_t domain_len, uint64_t first, size_t n, unsigned flags, amsm_bases** out) {
  if (!c || !out || domain_len > (size_t)b2s::SAMPLE_MAX_DOMAIN || (domain_len && !domain) || flags > 31u) return AMSM_E_INVALID_ARG;
  if (n >= (1ull << 31)) return AMSM_E_UNSUPPORTED;
  if (c->host_only) return CPU_CALL(c, bases_sample, c, domain, domain_len, first, n, flags, out);
  TRY(bind_device(c));
  if (wants_replicas(c, n, flags))  // every device samples the whole key
    return bases_create_replicated(c, out, [&](size_t, amsm_ctx* cg, amsm_bases** o) {
      return DISPATCH(cg, bases_sample_impl<Fq, Fr>(cg, domain, domain_len, first, n, flags & ~(unsigned)AMSM_BASES_REPLICATE, o));
    });
  flags &= ~(unsigned)AMSM_BASES_REPLICATE;
  if (ctx_shards_keys(c))  // shard g samples its own index range
    return bases_create_sharded(c, n, out, [&](size_t, amsm_ctx* cg, size_t lo, size_t cnt, amsm_bases** o) {
      return DISPATCH(cg, bases_sample_impl<Fq, Fr>(cg, domain, domain_len, first + lo, cnt, flags, o));
    });
  return DISPATCH(c, bases_sample_impl<Fq, Fr>(c, domain, domain_len, first, n, flags, out));
}
int amsm_points_check(amsm_ctx* c, const uint64_t* xy, const uint8_t* is_inf, size_t n, uint64_t* report, uint8_t* status) {
  if (!c || !report || (n && !xy)) return AMSM_E_INVALID_ARG;
  if (c->host_only) return CPU_CALL(c, points_check, xy, is_inf, n, report, status);
  TRY(bind_device(c));  // (a multi-device context: its primary device)
  return DISPATCH(c, points_check_host_impl<Fq>(c, xy, is_inf, n, report, status));
}
int amsm_points_check_device(amsm_ctx* c, const void* d_xy, size_t n, uint64_t* report, void* d_status) {
  if (!c || !report || (n && !d_xy)) return AMSM_E_INVALID_ARG;
  if (n >= (1ull << 31)) return AMSM_E_UNSUPPORTED;
  if (c->host_only) return CPU_CALL(c, points_check, (const uint64_t*)d_xy, nullptr, n, report, (uint8_t*)d_status);
  TRY(bind_device(c));
  return DISPATCH(c, points_check_device_impl<Fq>(c, d_xy, n, report, (uint8_t*)d_status));
}
int amsm_bases_read(amsm_ctx* c, const amsm_bases* b, size_t off, size_t n, uint64_t* xy, uint8_t* is_inf) {
  if (!c || !b || (n && !xy) || b->curve != c->curve) return AMSM_E_INVALID_ARG;
  if (key_sharded(b)) {
    if (!key_matches(c, b) || off > b->n || n > b->n - off) return AMSM_E_INVALID_ARG;
    const size_t L2 = 2 * (size_t)amsm_ctx_fq_limbs(c);
    for (size_t g = 0; g < b->shards.size(); g++) {
      const size_t lo = std::max(b->bound[g], off), hi = std::min(b->bound[g + 1], off + n);
      if (hi > lo)
        TRY(amsm_bases_read(c->shard_ctx[g], b->shards[g], lo - b->bound[g], hi - lo, xy + (lo - off) * L2,
                            is_inf ? is_inf + (lo - off) : nullptr));
    }
    return bind_device(c);
  }
  if (c->host_only != b->host) return AMSM_E_INVALID_ARG;
  if (b->host) return DISPATCH(c, cpu::bases_read<Fq>(b, off, n, xy, is_inf));
  TRY(bind_device(c));
  return DISPATCH(c, bases_read_impl<Fq>(c, b, off, n, xy, is_inf));
}
size_t amsm_bases_len(const amsm_bases* b) { return b ? b->n : 0; }
int amsm_bases_precomputed(const amsm_bases* b) { return b ? b->precomp : 0; }
int amsm_bases_window_bits(const amsm_bases* b) {
  if (!b) return 0;
  if (!b->shards.empty()) return b->shards[0] ? b->shards[0]->c : 0;
  return b->precomp ? b->c : 0;
}
int amsm_bases_replicas(const amsm_bases* b) { return !b ? 0 : (b->replicas.empty() ? 1 : (int)b->replicas.size()); }
int amsm_bases_num_shards(const amsm_bases* b) { return !b ? 0 : (key_sharded(b) ? (int)b->shards.size() : 1); }
int amsm_bases_shard_range(const amsm_bases* b, int g, size_t* lo, size_t* hi) {
  if (!b || !lo || !hi || g < 0 || g >= amsm_bases_num_shards(b)) return AMSM_E_INVALID_ARG;
  *lo = key_sharded(b) ? b->bound[g] : 0;
  *hi = key_sharded(b) ? b->bound[g + 1] : b->n;
  return AMSM_OK;
}
int amsm_bases_memory(const amsm_bases* b, size_t* table_bytes, size_t* abi_copy_bytes, size_t* twin_bytes) {
  if (!b) return AMSM_E_INVALID_ARG;
  size_t t = 0, a = 0, w = 0;
  if (key_sharded(b)) {
    for (const amsm_bases* s : b->shards) {
      size_t t1 = 0, a1 = 0, w1 = 0;
      if (s) TRY(amsm_bases_memory(s, &t1, &a1, &w1));
      t += t1, a += a1, w += w1;
    }
  } else {
    const size_t pb = DISPATCH(b, affine_bytes<Fq>());
    t = std::max<size_t>(b->n, 1) * (b->precomp ? (size_t)b->W : 1) * pb;
    if (b->d_small) t += b->n * (size_t)(DS_W * DS_MULT) * pb;  // a small key's direct-sum table
    {
      std::lock_guard<std::mutex> lk(b->abi_mu);
      a = b->d_abi ? b->n * pb : 0;
    }
    {
      std::lock_guard<std::mutex> lk(b->alt_mu);
      if (b->alt) w = b->alt->n * (b->alt->precomp ? (size_t)b->alt->W : 1) * pb;
    }
    for (const amsm_bases* s : b->replicas) {  // a replicated key: what every device holds
      size_t t1 = 0, a1 = 0, w1 = 0;
      if (s) TRY(amsm_bases_memory(s, &t1, &a1, &w1));
      t += t1, a += a1, w += w1;
    }
  }
  if (table_bytes) *table_bytes = t;
  if (abi_copy_bytes) *abi_copy_bytes = a;
  if (twin_bytes) *twin_bytes = w;
  return AMSM_OK;
}
int amsm_bases_tables(const amsm_bases* b, size_t out[7]) {
  if (!b || !out) return AMSM_E_INVALID_ARG;
  for (int i = 0; i < 7; i++) out[i] = 0;
  if (key_sharded(b)) {
    for (const amsm_bases* s : b->shards) {
      size_t o[7];
      if (!s) continue;
      TRY(amsm_bases_tables(s, o));
      for (int i = 0; i < 4; i++) out[i] += o[i];
      out[4] = std::max(out[4], o[4]);
      out[5] = std::max(out[5], o[5]);
      out[6] = std::max(out[6], o[6]);
    }
    return AMSM_OK;
  }
  const size_t pb = DISPATCH(b, affine_bytes<Fq>());
  out[0] = std::max<size_t>(b->n, 1) * (b->precomp ? (size_t)b->W : 1) * pb;
  out[1] = b->d_small ? b->n * (size_t)(DS_W * DS_MULT) * pb : 0;
  {
    std::lock_guard<std::mutex> lk(b->alt_mu);
    out[2] = b->alt ? b->alt->n * (b->alt->precomp ? (size_t)b->alt->W : 1) * pb : 0;
    out[6] = (size_t)b->twin_denied;
  }
  {
    std::lock_guard<std::mutex> lk(b->abi_mu);
    out[3] = b->d_abi ? b->n * pb : 0;
  }
  out[4] = b->precomp ? (size_t)b->W : 1;
  out[5] = (size_t)b->direct_denied;
  return AMSM_OK;
}
int amsm_bases_prebuild_twin(amsm_ctx* c, const amsm_bases* b) {
  if (!c || !b || !key_matches(c, b)) return AMSM_E_INVALID_ARG;
  if (key_sharded(b)) {
    for (size_t g = 0; g < b->shards.size(); g++) TRY(amsm_bases_prebuild_twin(c->shard_ctx[g], b->shards[g]));
    return bind_device(c);
  }
  if (!b->bpl || b->host) return AMSM_OK;
  TRY(bind_device(c));
  const amsm_bases* alt = nullptr;
  return DISPATCH(c, bases_alt<Fq>(c, b, &alt));
}
void amsm_bases_free(amsm_bases* b) {
  if (!b) return;
  for (amsm_bases* s : b->shards) amsm_bases_free(s);
  b->shards.clear();
  for (amsm_bases* s : b->replicas) amsm_bases_free(s);
  b->replicas.clear();
  if (b->alt) amsm_bases_free(b->alt);
  b->alt = nullptr;
  if (b->host) {
    (void)gate_free(b->d_table);
    delete b;
    return;
  }
  (void)hipSetDevice(b->device);
  if (b->ready) {
    (void)hipEventSynchronize(b->ready);
    (void)hipEventDestroy(b->ready);
  }
  (void)gate_free(b->d_table);
  (void)gate_free(b->d_small);
  (void)gate_free(b->d_abi);
  delete b;
}

// n_vecs MSMs over a sharded key -> n_vecs affine points (shared by every entry point that accepts one)
static int msm_sharded_affine(amsm_ctx* c, const amsm_bases* b, size_t off, size_t n, size_t n_vecs, int mont, SliceKind kind,
                              const void* const* srcs, uint64_t* out_xy, uint8_t* out_inf) {
  TRY(bind_device(c));
  TRY(DISPATCH_DO(c, {
    std::vector<host::HXYZZ<Fq>> r;
    TRY((msm_sharded<Fq, Fr>(c, b, off, n, n_vecs, mont, kind, srcs, &r)));
    write_affine_batch<Fq>(r, out_xy, out_inf);
  }));
  return AMSM_OK;
}

int amsm_msm(amsm_ctx* c, const amsm_bases* b, size_t off, const uint64_t* scalars, size_t n, int mont, uint64_t* out_xy,
             uint8_t* out_inf) {
  if (!c || !b || !out_xy || (n && !scalars) || !key_matches(c, b)) return AMSM_E_INVALID_ARG;
  if (key_sharded(b)) {
    const void* src = scalars;
    return msm_sharded_affine(c, b, off, n, 1, mont, SLICE_HOST, &src, out_xy, out_inf);
  }
  if (c->host_only) return CPU_CALL(c, msm_affine, b, off, scalars, n, mont, out_xy, out_inf);
  TRY(bind_device(c));
  TRY(DISPATCH_DO(c, {
    host::HXYZZ<Fq> r;
    TRY((msm_host_scalars<Fq, Fr>(c, b, off, scalars, n, mont, &r)));
    write_affine<Fq>(r, out_xy, out_inf);
  }));
  return AMSM_OK;
}

int amsm_msm_oneshot(amsm_ctx* c, const uint64_t* xy, const uint8_t* is_inf, size_t n_bases, const uint64_t* scalars, size_t n_scalars,
                     int mont, uint64_t* out_xy, uint8_t* out_inf) {
  const size_t n = std::min(n_bases, n_scalars);  // ark-ec: `size = min(bases.len(), scalars.len())`
  if (!c || !out_xy || (n && (!xy || !scalars))) return AMSM_E_INVALID_ARG;
  if (n >= (1ull << 31)) return AMSM_E_UNSUPPORTED;
  if (c->host_only) {
    amsm_bases* b = nullptr;
    TRY(CPU_CALL(c, bases_load, c, xy, is_inf, n, AMSM_BASES_NO_PRECOMPUTE, &b));
    const int rc = CPU_CALL(c, msm_affine, b, 0, scalars, n, mont, out_xy, out_inf);
    amsm_bases_free(b);
    return rc;
  }
  return DISPATCH(c, msm_oneshot_any<Fq, Fr>(c, xy, is_inf, scalars, n, mont, out_xy, out_inf));
}

int amsm_msm_device(amsm_ctx* c, const amsm_bases* b, size_t off, const void* d_scalars, size_t n, int mont,
                    uint64_t* out_xy, uint8_t* out_inf) {
  if (!c || !b || !out_xy || (n && !d_scalars) || !key_matches(c, b)) return AMSM_E_INVALID_ARG;
  if (key_sharded(b)) return msm_sharded_affine(c, b, off, n, 1, mont, SLICE_PRIMARY, &d_scalars, out_xy, out_inf);
  if (c->host_only) return CPU_CALL(c, msm_affine, b, off, d_scalars, n, mont, out_xy, out_inf);
  TRY(bind_device(c));
  TRY(DISPATCH_DO(c, {
    host::HXYZZ<Fq> r;
    TRY((msm_device_xyzz<Fq, Fr>(c, b, off, d_scalars, n, mont, &r)));
    write_affine<Fq>(r, out_xy, out_inf);
  }));
  return AMSM_OK;
}

int amsm_msm_batch_device(amsm_ctx* c, const amsm_bases* b, size_t off, const void* const* d_scalars, size_t n_vecs,
                          size_t n, int mont, uint64_t* out_xy, uint8_t* out_inf) {
  if (!c || !b || (n_vecs && (!d_scalars || !out_xy)) || !key_matches(c, b)) return AMSM_E_INVALID_ARG;
  for (size_t v = 0; v < n_vecs; v++)
    if (n && !d_scalars[v]) return AMSM_E_INVALID_ARG;
  if (key_sharded(b)) return msm_sharded_affine(c, b, off, n, n_vecs, mont, SLICE_PRIMARY, d_scalars, out_xy, out_inf);
  if (c->host_only) {
    std::vector<size_t> h_offs(n_vecs, off), h_ns(n_vecs, n);
    return CPU_CALL(c, msm_multi_affine, b, n_vecs, h_offs.data(), d_scalars, h_ns.data(), mont, nullptr, nullptr, out_xy, out_inf);
  }
  if (key_replicated(b) && n_vecs >= 2 && b->owner == c) {  // (round 6) whole MSMs dealt to the devices, no exchange
    TRY(bind_device(c));
    std::vector<size_t> r_ns(n_vecs, n);
    return DISPATCH(c, msm_replicated_affine<Fq, Fr>(c, b, off, r_ns.data(), n_vecs, mont, SLICE_PRIMARY, d_scalars, nullptr, nullptr, out_xy, out_inf));
  }
  TRY(bind_device(c));
  TRY(DISPATCH_DO(c, {
    std::vector<host::HXYZZ<Fq>> r;
    TRY((msm_batch_xyzz<Fq, Fr>(c, b, off, d_scalars, n_vecs, n, mont, &r)));
    write_affine_batch<Fq>(r, out_xy, out_inf);
  }));
  return AMSM_OK;
}

int amsm_msm_batch(amsm_ctx* c, const amsm_bases* b, size_t off, const uint64_t* const* scalars, size_t n_vecs, size_t n,
                   int mont, uint64_t* out_xy, uint8_t* out_inf) {
  if (!c || !b || (n_vecs && (!scalars || !out_xy)) || !key_matches(c, b)) return AMSM_E_INVALID_ARG;
  for (size_t v = 0; v < n_vecs; v++)
    if (n && !scalars[v]) return AMSM_E_INVALID_ARG;
  if (key_sharded(b))
    return msm_sharded_affine(c, b, off, n, n_vecs, mont, SLICE_HOST, (const void* const*)scalars, out_xy, out_inf);
  if (c->host_only) {
    std::vector<size_t> h_offs(n_vecs, off), h_ns(n_vecs, n);
    return CPU_CALL(c, msm_multi_affine, b, n_vecs, h_offs.data(), (const void* const*)scalars, h_ns.data(), mont, nullptr, nullptr, out_xy,
                    out_inf);
  }
  TRY(bind_device(c));
  std::vector<size_t> ns(n_vecs, n);
  if (key_replicated(b) && n_vecs >= 2 && b->owner == c)
    return DISPATCH(c, msm_replicated_affine<Fq, Fr>(c, b, off, ns.data(), n_vecs, mont, SLICE_HOST, (const void* const*)scalars, nullptr, nullptr, out_xy, out_inf));
  return DISPATCH(c, msm_host_batch_impl<Fq, Fr>(c, b, off, scalars, ns.data(), n_vecs, mont, nullptr, nullptr,
                                                              out_xy, out_inf));
}

int amsm_pedersen_commit_batch(amsm_ctx* c, const amsm_bases* ck, const uint64_t* const* elems, const size_t* ns, size_t n_vecs,
                               const uint64_t* const* rand_mont, const uint64_t* hiding_xy, uint64_t* out_xy,
                               uint8_t* out_inf) {
  if (!c || !ck || (n_vecs && (!elems || !ns || !out_xy)) || !key_matches(c, ck)) return AMSM_E_INVALID_ARG;
  bool any_rand = false;
  for (size_t v = 0; v < n_vecs; v++) {
    if (ns[v] && !elems[v]) return AMSM_E_INVALID_ARG;
    any_rand = any_rand || (rand_mont && rand_mont[v]);
  }
  if (any_rand && !hiding_xy) return AMSM_E_INVALID_ARG;
  if (key_sharded(ck)) {  // the sharded exchange carries equal-length vectors: one call per commitment otherwise
    for (size_t v = 0; v < n_vecs; v++)
      TRY(amsm_pedersen_commit(c, ck, elems[v], ns[v], rand_mont ? rand_mont[v] : nullptr,
                               (rand_mont && rand_mont[v]) ? hiding_xy : nullptr, out_xy + v * 2 * amsm_ctx_fq_limbs(c),
                               out_inf ? out_inf + v : nullptr));
    return AMSM_OK;
  }
  if (c->host_only) {
    std::vector<size_t> h_offs(n_vecs, 0);
    return CPU_CALL(c, msm_multi_affine, ck, n_vecs, h_offs.data(), (const void* const*)elems, ns, 1, any_rand ? rand_mont : nullptr,
                    hiding_xy, out_xy, out_inf);
  }
  TRY(bind_device(c));
  if (key_replicated(ck) && n_vecs >= 2 && ck->owner == c)
    return DISPATCH(c, msm_replicated_affine<Fq, Fr>(c, ck, 0, ns, n_vecs, 1, SLICE_HOST, (const void* const*)elems, any_rand ? rand_mont : nullptr, hiding_xy, out_xy, out_inf));
  return DISPATCH(c, msm_host_batch_impl<Fq, Fr>(c, ck, 0, elems, ns, n_vecs, 1, any_rand ? rand_mont : nullptr,
                                                              hiding_xy, out_xy, out_inf));
}

int amsm_msm_multi_device(amsm_ctx* c, const amsm_bases* b, size_t n_msms, const size_t* base_offs,
                          const void* const* d_scalars, const size_t* ns, int mont, uint64_t* out_xy, uint8_t* out_inf) {
  if (!c || !b || (n_msms && (!base_offs || !d_scalars || !ns || !out_xy)) || b->curve != c->curve ||
      (!key_sharded(b) && b->device != c->device))
    return AMSM_E_INVALID_ARG;
  for (size_t v = 0; v < n_msms; v++)
    if (ns[v] && !d_scalars[v]) return AMSM_E_INVALID_ARG;
  if (key_sharded(b)) {  // runs of jobs over the same key range go out as one sharded batch (one exchange per run)
    if (!key_matches(c, b)) return AMSM_E_INVALID_ARG;
    TRY(bind_device(c));
    const size_t L2 = 2 * (size_t)amsm_ctx_fq_limbs(c);
    for (size_t v = 0; v < n_msms;) {
      size_t e = v + 1;
      while (e < n_msms && base_offs[e] == base_offs[v] && ns[e] == ns[v]) e++;
      TRY(DISPATCH_DO(c, {
        std::vector<host::HXYZZ<Fq>> r;
        TRY((msm_sharded<Fq, Fr>(c, b, base_offs[v], ns[v], e - v, mont, SLICE_PRIMARY, d_scalars + v, &r)));
        write_affine_batch<Fq>(r, out_xy + v * L2, out_inf ? out_inf + v : nullptr);
      }));
      v = e;
    }
    return AMSM_OK;
  }
  if (c->host_only) return CPU_CALL(c, msm_multi_affine, b, n_msms, base_offs, d_scalars, ns, mont, nullptr, nullptr, out_xy, out_inf);
  TRY(bind_device(c));
  // a job longer than the key's window is cut like every other entry point cuts it (ranges over one bucket set, round 5); short
  // jobs -- the two cross commitments of an IPA round -- keep the direct path and its single synchronisation
  bool split = false;
  for (size_t v = 0; v < n_msms; v++) split = split || (base_offs[v] <= b->n && split_needed(c, b, std::min(ns[v], b->n - base_offs[v])));
  TRY(DISPATCH_DO(c, {
    std::vector<host::HXYZZ<Fq>> r;
    std::vector<MsmJob> vecs;
    TRY(jobs_from_arrays(b, n_msms, base_offs, d_scalars, ns, mont, &vecs));
    if (split) TRY((msm_multi_split_xyzz<Fq, Fr>(c, vecs, &r)));
    else TRY((msm_multi_xyzz<Fq, Fr>(c, vecs, &r)));
    write_affine_batch<Fq>(r, out_xy, out_inf);
  }));
  return AMSM_OK;
}

int amsm_msm_grouped_device(amsm_ctx* c, const amsm_bases* b, size_t off, const void* d_scalars, size_t n, int mont,
                            unsigned group_shift, uint64_t* out_xy, uint8_t* out_inf) {
  if (!c || !b || !out_xy || (n && !d_scalars) || group_shift > 31 || !key_matches(c, b)) return AMSM_E_INVALID_ARG;
  if (key_sharded(b)) {  // (round 5) every shard sums its part of both index classes; one exchange of two records per shard
    TRY(bind_device(c));
    TRY(DISPATCH_DO(c, {
      std::vector<host::HXYZZ<Fq>> r;
      TRY((msm_sharded<Fq, Fr>(c, b, off, n, 1, mont, SLICE_PRIMARY, &d_scalars, &r, (int)group_shift)));
      write_affine_batch<Fq>(r, out_xy, out_inf);
    }));
    return AMSM_OK;
  }
  if (c->host_only) return CPU_CALL(c, msm_grouped, b, off, d_scalars, n, mont, group_shift, out_xy, out_inf);
  TRY(bind_device(c));
  return DISPATCH(c, msm_grouped_impl<Fq, Fr>(c, b, off, d_scalars, n, mont, group_shift, out_xy, out_inf));
}

size_t amsm_partial_bytes(const amsm_ctx* c) {
  if (!c) return 0;
  return DISPATCH(c, xyzz_bytes<Fq>());
}

int amsm_msm_partial_device(amsm_ctx* c, const amsm_bases* b, size_t off, const void* d_scalars, size_t n, int mont,
                            void* d_out) {
  if (!c || !b || !d_out || (n && !d_scalars) || b->curve != c->curve || b->device != c->device)
    return AMSM_E_INVALID_ARG;
  if (key_sharded(b)) return AMSM_E_UNSUPPORTED;  // does not shard (include/amsm.h: amsm_ctx_create_multi)
  if (c->host_only) return CPU_CALL(c, msm_partial_batch, b, off, &d_scalars, 1, n, mont, d_out);
  TRY(bind_device(c));
  return DISPATCH(c, msm_partial_impl<Fq, Fr>(c, b, off, d_scalars, n, mont, d_out));
}

int amsm_msm_partial_batch_device(amsm_ctx* c, const amsm_bases* b, size_t off, const void* const* d_scalars, size_t n_vecs,
                                  size_t n, int mont, void* d_out) {
  if (!c || !b || (n_vecs && (!d_scalars || !d_out)) || b->curve != c->curve || b->device != c->device)
    return AMSM_E_INVALID_ARG;
  for (size_t v = 0; v < n_vecs; v++)
    if (n && !d_scalars[v]) return AMSM_E_INVALID_ARG;
  if (key_sharded(b)) return AMSM_E_UNSUPPORTED;  // does not shard (include/amsm.h: amsm_ctx_create_multi)
  if (c->host_only) return CPU_CALL(c, msm_partial_batch, b, off, d_scalars, n_vecs, n, mont, d_out);
  TRY(bind_device(c));
  return DISPATCH(c, msm_partial_batch_impl<Fq, Fr>(c, b, off, d_scalars, n_vecs, n, mont, d_out));
}

int amsm_partials_combine_batch(amsm_ctx* c, const void* d_partials, size_t n_groups, size_t count, uint64_t* out_xy,
                                uint8_t* out_inf) {
  if (!c || (n_groups && !out_xy) || (n_groups && count && !d_partials)) return AMSM_E_INVALID_ARG;
  if (c->host_only) return CPU_CALL(c, partials_combine_batch, d_partials, n_groups, count, out_xy, out_inf);
  TRY(bind_device(c));
  return DISPATCH(c, partials_combine_batch_impl<Fq>(c, d_partials, n_groups, count, out_xy, out_inf));
}

int amsm_partials_combine(amsm_ctx* c, const void* d_partials, size_t count, uint64_t* out_xy, uint8_t* out_inf) {
  if (!c || !out_xy || (count && !d_partials)) return AMSM_E_INVALID_ARG;
  if (c->host_only) return CPU_CALL(c, partials_combine_batch, d_partials, 1, count, out_xy, out_inf);
  TRY(bind_device(c));
  return DISPATCH(c, partials_combine_impl<Fq>(c, d_partials, count, out_xy, out_inf));
}

static int pedersen_sharded(amsm_ctx* c, const amsm_bases* ck, size_t n, SliceKind kind, const void* const* src,
                            const uint64_t* rand_mont, const uint64_t* hiding_xy, uint64_t* out_xy, uint8_t* out_inf) {
  TRY(bind_device(c));
  return DISPATCH(c, pedersen_sharded_impl<Fq, Fr>(c, ck, n, kind, src, rand_mont, hiding_xy, out_xy, out_inf));
}

int amsm_msm_batch_sharded_device(amsm_ctx* c, const amsm_bases* b, const void* const* d_slices, size_t n_vecs, int mont,
                                  uint64_t* out_xy, uint8_t* out_inf) {
  if (!c || !b || (n_vecs && (!d_slices || !out_xy)) || !key_matches(c, b)) return AMSM_E_INVALID_ARG;
  if (!key_sharded(b)) {
    // (a replicated or folded key of a multi-device context has no shards to hand slices to: its vectors are whole)
    if (n_shards(c) > 1) return AMSM_E_INVALID_ARG;
    return amsm_msm_batch_device(c, b, 0, d_slices, n_vecs, b->n, mont, out_xy, out_inf);
  }
  const size_t N = b->shards.size();
  for (size_t v = 0; v < n_vecs; v++)
    for (size_t g = 0; g < N; g++)
      if (b->bound[g + 1] > b->bound[g] && !d_slices[v * N + g]) return AMSM_E_INVALID_ARG;
  return msm_sharded_affine(c, b, 0, b->n, n_vecs, mont, SLICE_SHARDED, d_slices, out_xy, out_inf);
}

int amsm_pedersen_commit(amsm_ctx* c, const amsm_bases* ck, const uint64_t* elems, size_t n, const uint64_t* rand_mont,
                         const uint64_t* hiding_xy, uint64_t* out_xy, uint8_t* out_inf) {
  if (!c || !ck || !out_xy || (n && !elems) || !key_matches(c, ck)) return AMSM_E_INVALID_ARG;
  if ((rand_mont == nullptr) != (hiding_xy == nullptr)) return AMSM_E_INVALID_ARG;
  if (key_sharded(ck)) {
    const void* src = elems;
    return pedersen_sharded(c, ck, n, SLICE_HOST, &src, rand_mont, hiding_xy, out_xy, out_inf);
  }
  if (c->host_only) return CPU_CALL(c, pedersen, ck, elems, n, rand_mont, hiding_xy, out_xy, out_inf);
  TRY(bind_device(c));
  return DISPATCH(c, pedersen_impl<Fq, Fr>(c, ck, elems, n, rand_mont, hiding_xy, out_xy, out_inf));
}

int amsm_pedersen_commit_device(amsm_ctx* c, const amsm_bases* ck, const void* d_elems, size_t n,
                                const uint64_t* rand_mont, const uint64_t* hiding_xy, uint64_t* out_xy, uint8_t* out_inf) {
  if (!c || !ck || !out_xy || (n && !d_elems) || !key_matches(c, ck)) return AMSM_E_INVALID_ARG;
  if ((rand_mont == nullptr) != (hiding_xy == nullptr)) return AMSM_E_INVALID_ARG;
  if (key_sharded(ck)) return pedersen_sharded(c, ck, n, SLICE_PRIMARY, &d_elems, rand_mont, hiding_xy, out_xy, out_inf);
  if (c->host_only) return CPU_CALL(c, pedersen, ck, d_elems, n, rand_mont, hiding_xy, out_xy, out_inf);
  TRY(bind_device(c));
  return DISPATCH(c, pedersen_device_impl<Fq, Fr>(c, ck, d_elems, n, rand_mont, hiding_xy, out_xy, out_inf));
}
