// Part of api.hip (inside extern "C"): device vectors and their allocator, vector kernels, key folds, IPA rounds, R1CS
// matrices, hp_as t-vectors.
int amsm_vec_fill(amsm_ctx* c, const uint64_t* value_mont, size_t n, void* d_out) {
  if (!c || !value_mont || (n && !d_out) || n >= (1ull << 32)) return AMSM_E_INVALID_ARG;
  if (c->host_only) {
    for (size_t i = 0; i < n; i++) memcpy((char*)d_out + 32 * i, value_mont, 32);
    return AMSM_OK;
  }
  TRY(bind_device(c));
  if (!n) return AMSM_OK;
  u32 v[8];
  memcpy(v, value_mont, 32);
  launch_vec_fill(c->stream, (u32*)d_out, v, (u32)n);
  HIP_TRY(hipGetLastError());
  return AMSM_OK;
}

// (the pool's books -- pool_round, g_pool_mu, pool_owner, pool_release_all, pool_forget_ctx -- are in api_gate.inc)
int amsm_dev_alloc(amsm_ctx* c, size_t bytes, void** d_ptr) {
  if (!c || !d_ptr) return AMSM_E_INVALID_ARG;
  if (c->host_only) {  // host memory, no free lists (malloc does not synchronise anything)
    const size_t hsz = pool_round(bytes);
    void* hp = nullptr;  // (*d_ptr is written on success only: the contract after AMSM_E_OOM, include/amsm.h)
    TRY(gate_alloc(c, GATE_HOST, hsz, false, &hp));
    *d_ptr = hp;
    std::lock_guard<std::mutex> lk(g_pool_mu);
    c->pool_size[*d_ptr] = hsz;
    c->pool_live_bytes += hsz;
    return AMSM_OK;
  }
  TRY(bind_device(c));
  const size_t sz = pool_round(bytes);
  {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    auto it = c->pool.find(sz);
    if (it != c->pool.end() && !it->second.empty()) {
      *d_ptr = it->second.back();
      it->second.pop_back();
      c->pool_free_bytes -= sz;
      c->pool_live_bytes += sz;
      return AMSM_OK;
    }
  }
  int why = GATE_GRANTED;
  void* p = nullptr;  // (*d_ptr is written on success only: the contract after AMSM_E_OOM, include/amsm.h)
  int rc = gate_alloc(c, GATE_DEVICE, sz, true, &p, &why);
  if (rc != AMSM_OK && why == GATE_BY_DRIVER) {  // give the free lists back to the driver and try once more (a refusal by the
    (void)hipStreamSynchronize(c->stream);       // limit has done so already; one by the test hook stands)
    pool_release_all(c);
    rc = gate_alloc(c, GATE_DEVICE, sz, true, &p);
  }
  if (rc != AMSM_OK) {
    // (asked for as tolerated because of the second try above; for the caller -- the library's own scratch vectors included, which may
    // have queued work before they asked: t_vecs_impl -- the vector was required: nothing stays in flight)
    gate_drain(c);
    return AMSM_E_OOM;
  }
  *d_ptr = p;
  std::lock_guard<std::mutex> lk(g_pool_mu);
  c->pool_size[*d_ptr] = sz;
  c->pool_live_bytes += sz;
  pool_owner()[*d_ptr] = c;
  return AMSM_OK;
}
int amsm_dev_free(amsm_ctx* c, void* d_ptr) {
  if (!c) return AMSM_E_INVALID_ARG;
  if (c->host_only) {
    if (!d_ptr) return AMSM_OK;
    {
      std::lock_guard<std::mutex> lk(g_pool_mu);
      auto it = c->pool_size.find(d_ptr);
      if (it == c->pool_size.end()) return AMSM_E_INVALID_ARG;  // not a buffer of this host context
      c->pool_live_bytes -= it->second;
      c->pool_size.erase(it);
    }
    (void)gate_free(d_ptr);
    return AMSM_OK;
  }
  TRY(bind_device(c));
  if (!d_ptr) return AMSM_OK;
  std::unique_lock<std::mutex> lk(g_pool_mu);
  auto it = c->pool_size.find(d_ptr);
  if (it == c->pool_size.end()) {
    // Not this context's: a buffer another context of this process allocated (its books are settled here), or a foreign
    // pointer.  Either way a REAL free: hipFree synchronises the device, so a consumer still running on the other
    // context's streams finishes first -- the buffer never enters a free list whose stream order does not cover it.
    auto ow = pool_owner().find(d_ptr);
    if (ow != pool_owner().end()) {
      amsm_ctx* o = ow->second;
      auto io = o->pool_size.find(d_ptr);
      if (io != o->pool_size.end()) {
        o->pool_live_bytes -= io->second;
        o->pool_size.erase(io);
      }
      pool_owner().erase(ow);
    }
    lk.unlock();
    HIP_TRY(gate_free(d_ptr));
    return AMSM_OK;
  }
  const size_t sz = it->second;
  c->pool_live_bytes -= sz;
  if (c->pool_free_bytes + sz > c->pool_cap_bytes) {
    c->pool_size.erase(it);
    pool_owner().erase(d_ptr);
    lk.unlock();
    HIP_TRY(gate_free(d_ptr));
    return AMSM_OK;
  }
  c->pool[sz].push_back(d_ptr);
  c->pool_free_bytes += sz;
  return AMSM_OK;
}
int amsm_ctx_memory(const amsm_ctx* c, size_t* workspace_bytes, size_t* vectors_live_bytes, size_t* vectors_pooled_bytes) {
  if (!c) return AMSM_E_INVALID_ARG;
  size_t ws = 0;
  auto count = [&](const DevBuf& b) { ws += b.bytes; };
  for_each_ctx_buf(c, count);
  for (const Slot& sl : c->slot) for_each_slot_buf(&sl, count);
  if (workspace_bytes) *workspace_bytes = ws;
  if (vectors_live_bytes) *vectors_live_bytes = c->pool_live_bytes;
  if (vectors_pooled_bytes) *vectors_pooled_bytes = c->pool_free_bytes;
  return AMSM_OK;
}
int amsm_ctx_trim(amsm_ctx* c) {
  if (!c) return AMSM_E_INVALID_ARG;
  if (c->host_only) return AMSM_OK;  // no workspace, no free lists
  for (size_t g = 1; g < c->shard_ctx.size(); g++) TRY(amsm_ctx_trim(c->shard_ctx[g]));
  TRY(amsm_ctx_synchronize(c));
  pool_release_all(c);
  if (c->s_copy) (void)hipStreamSynchronize(c->s_copy);
  auto release = [](DevBuf& b) { b.release(); };
  for_each_ctx_buf(c, release);
  for (Slot& sl : c->slot) for_each_slot_buf(&sl, release);
  return AMSM_OK;
}
int amsm_dev_upload(amsm_ctx* c, void* d_dst, const void* h_src, size_t bytes) {
  if (!c || (bytes && (!d_dst || !h_src))) return AMSM_E_INVALID_ARG;
  if (c->host_only) {
    if (bytes) memmove(d_dst, h_src, bytes);
    return AMSM_OK;
  }
  TRY(bind_device(c));
  if (bytes) {
    HIP_TRY(hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  return AMSM_OK;
}
int amsm_dev_download(amsm_ctx* c, void* h_dst, const void* d_src, size_t bytes) {
  if (!c || (bytes && (!h_dst || !d_src))) return AMSM_E_INVALID_ARG;
  if (c->host_only) {
    if (bytes) memmove(h_dst, d_src, bytes);
    return AMSM_OK;
  }
  TRY(bind_device(c));
  if (bytes) {
    HIP_TRY(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  return AMSM_OK;
}

int amsm_vec_random(amsm_ctx* c, uint64_t seed, size_t n, int mont, void* d_out) {
  if (!c || (n && !d_out) || n >= (1ull << 32)) return AMSM_E_INVALID_ARG;
  if (c->host_only) return CPU_CALL(c, vec_random, seed, n, mont, d_out);
  TRY(bind_device(c));
  if (!n) return AMSM_OK;
  DISPATCH_DO(c, launch_vec_random<Fr>(c->stream, (u32*)d_out, seed, (u32)n, mont));
  HIP_TRY(hipGetLastError());
  return AMSM_OK;
}

int amsm_vec_sample(amsm_ctx* c, const uint8_t key[32], uint32_t stream, uint64_t first, size_t n, int mont, void* d_out) {
  if (!c || !key || !d_out || n >= (1ull << 32) || first + n < first) return AMSM_E_INVALID_ARG;
  if (c->host_only) return CPU_CALL(c, vec_sample, c->curve, key, stream, first, n, mont, d_out);
  TRY(bind_device(c));
  if (!n) return AMSM_OK;
  const blind::Key k = blind::key_words(key);  // a kernel argument: the key is staged in no buffer and printed nowhere
  DISPATCH_DO(c, launch_vec_sample<Fr>(c->stream, (u32*)d_out, k, (u32)c->curve, stream, first, (u32)n, mont, c->vec_sample_form));
  HIP_TRY(hipGetLastError());
  return AMSM_OK;
}

int amsm_vec_hadamard(amsm_ctx* c, const void* d_a, const void* d_b, void* d_out, size_t n) {
  if (!c || (n && (!d_a || !d_b || !d_out)) || n >= (1ull << 32)) return AMSM_E_INVALID_ARG;
  if (c->host_only) return CPU_CALL(c, vec_hadamard, d_a, d_b, d_out, n);
  TRY(bind_device(c));
  if (!n) return AMSM_OK;
  DISPATCH_DO(c, launch_vec_hadamard<Fr>(c->stream, vec_grid_of(c), (const u32*)d_a, (const u32*)d_b, (u32*)d_out, (u32)n));
  HIP_TRY(hipGetLastError());
  return AMSM_OK;
}

int amsm_vec_combine(amsm_ctx* c, const void* const* d_vecs, const size_t* lens, size_t n_vecs, const uint64_t* coeffs,
                     const void* d_hiding, size_t hiding_len, void* d_out, size_t n) {
  if (!c || (n && !d_out) || (n_vecs && (!d_vecs || !coeffs)) || n >= (1ull << 32)) return AMSM_E_INVALID_ARG;
  if (c->host_only) return CPU_CALL(c, vec_combine, d_vecs, lens, n_vecs, coeffs, d_hiding, hiding_len, d_out, n);
  TRY(bind_device(c));
  return DISPATCH(c, vec_combine_impl<Fr>(c, d_vecs, lens, n_vecs, coeffs, d_hiding, hiding_len, d_out, n));
}

int amsm_bases_from_device(amsm_ctx* c, const void* d_xy, size_t n, unsigned flags, amsm_bases** out) {
  if (!c || !out || (n && !d_xy) || n >= (1ull << 30)) return AMSM_E_INVALID_ARG;
  if (c->host_only) return CPU_CALL(c, bases_load, c, (const uint64_t*)d_xy, nullptr, n, flags, out);
  TRY(bind_device(c));
  amsm_bases* b = new (std::nothrow) amsm_bases();
  if (!b) return AMSM_E_OOM;
  b->curve = c->curve;
  b->device = c->device;
  b->n = n;
  size_t pb = DISPATCH(c, affine_bytes<Fq>());
  if (gate_alloc(c, GATE_DEVICE, std::max<size_t>(n, 1) * pb, false, (void**)&b->d_table) != AMSM_OK) {
    delete b;
    return AMSM_E_OOM;
  }
  int s = AMSM_OK;
  if (n) {
    if (hipMemcpyAsync(b->d_table, d_xy, n * pb, hipMemcpyDeviceToDevice, c->stream) != hipSuccess) s = AMSM_E_HIP;
    if (s == AMSM_OK && (flags & AMSM_BASES_CHECK)) s = DISPATCH(c, points_check_for_key<Fq>(c, b->d_table, nullptr, n));
    if (s == AMSM_OK) {
      DISPATCH_DO(c, launch_points_import<Fq>(c->stream, b->d_table, b->d_table, (u32)n));
      if (hipStreamSynchronize(c->stream) != hipSuccess || hipGetLastError() != hipSuccess) s = AMSM_E_HIP;
    }
    if (s == AMSM_OK)
      s = DISPATCH(c, bases_finish<Fq, Fr>(c, b, (flags & ~(unsigned)AMSM_BASES_CHECK) ? flags : AMSM_BASES_NO_PRECOMPUTE));
  }
  if (s != AMSM_OK) {
    (void)hipStreamSynchronize(c->stream);  // (the copy into the table may still run)
    (void)hipGetLastError();
    bases_discard(b);
    return s;
  }
  *out = b;
  return AMSM_OK;
}
const void* amsm_bases_device_ptr(const amsm_bases* b) {
  if (!b || key_sharded(b)) return nullptr;
  if (b->host) return b->d_table;  // already in the C-ABI radix
  bool internal = DISPATCH(b, device_internal_radix<Fq>());
  // the table may still be written by the fold that created the key (queued on that context's non-blocking stream,
  // which the NULL stream below does not order behind)
  if (b->ready && hipEventSynchronize(b->ready) != hipSuccess) return nullptr;
  if (!internal) return b->d_table;
  std::lock_guard<std::mutex> lock(b->abi_mu);
  if (!b->d_abi && b->n) {  // the table is in the device radix: hand out a C-ABI-radix copy of level 0
    size_t pb = DISPATCH(b, affine_bytes<Fq>());
    int prev = 0;
    if (hipGetDevice(&prev) != hipSuccess || hipSetDevice(b->device) != hipSuccess) return nullptr;
    u32* p = nullptr;
    // on the books of the context that holds the key's table (if it still lives).  Tolerated: the caller gets a null pointer
    bool ok = gate_alloc(gate_owner_of(b->d_table), GATE_DEVICE, b->n * pb, true, (void**)&p) == AMSM_OK;
    if (ok) {
      DISPATCH_DO(b, launch_points_export<Fq>(nullptr, b->d_table, p, (u32)b->n));
      ok = hipStreamSynchronize(nullptr) == hipSuccess && hipGetLastError() == hipSuccess;
      if (!ok) (void)gate_free(p);
    }
    (void)hipSetDevice(prev);
    if (ok) b->d_abi = p;
  }
  return b->n ? b->d_abi : b->d_table;
}

static void canonical_scalar(int curve, const uint64_t* x_mont, u32 out[8]) {
  with_curve(curve, [&](auto cv) {
    AMSM_CURVE_FIELDS(cv);
    host::HFe<Fr> x;
    memcpy(x.v, x_mont, 32);
    x = host::h_from_mont<Fr>(x);
    memcpy(out, x.v, 32);
    return AMSM_OK;
  });
}

// scratch for the unconverted sums of a large fold (null: the kernel converts in place); stream-ordered reuse is safe
// because every user runs on the context's stream
static u32* fold_scratch(amsm_ctx* c, size_t n) {
  bool pays = DISPATCH(c, batch_affine_pays<Fq>((u32)n));
  size_t rec = DISPATCH(c, xyzz_bytes<Fq>());
  if (!pays || ensure(c->xyzz_scratch, n * rec) != AMSM_OK) return nullptr;
  return (u32*)c->xyzz_scratch.p;
}

int amsm_points_fold(amsm_ctx* c, const void* d_l, const void* d_r, size_t n, const uint64_t* x_mont, unsigned nbits,
                     void* d_out) {
  if (!c || !x_mont || (n && (!d_l || !d_r || !d_out)) || n >= (1ull << 32) || nbits > 256) return AMSM_E_INVALID_ARG;
  if (c->host_only) return CPU_CALL(c, points_fold, d_l, d_r, n, x_mont, nbits, d_out);
  TRY(bind_device(c));
  if (!n) return AMSM_OK;
  u32 canon[8];
  canonical_scalar(c->curve, x_mont, canon);
  u32* scratch = fold_scratch(c, n);
  FoldDigits d;
  const bool glv = DISPATCH(c, host::fold_digits<Fq>(canon, nbits, &d));
  DISPATCH_DO(c, launch_points_fold<Fq>(c->stream, (const u32*)d_l, (const u32*)d_r, (u32)n, d, glv, (u32*)d_out, true, scratch));
  HIP_TRY(hipGetLastError());
  return AMSM_OK;
}

int amsm_bases_fold(amsm_ctx* c, const amsm_bases* key, size_t n_half, const uint64_t* x_mont, unsigned nbits,
                    amsm_bases** out) {
  if (!c || !key || !out || !x_mont || key->curve != c->curve || key->device != c->device || nbits > 256 ||
      n_half == 0 || 2 * n_half > key->n)
    return AMSM_E_INVALID_ARG;
  if (key_sharded(key)) return AMSM_E_UNSUPPORTED;
  if (c->host_only) {
    amsm_bases* hb = DISPATCH(c, cpu::bases_new<Fq>(c, n_half));
    if (!hb) return AMSM_E_OOM;
    const size_t hpb = DISPATCH(c, affine_bytes<Fq>());
    int rc = CPU_CALL(c, points_fold, key->d_table, (const char*)key->d_table + n_half * hpb, n_half, x_mont, nbits, hb->d_table);
    if (rc != AMSM_OK) {
      amsm_bases_free(hb);
      return rc;
    }
    *out = hb;
    return AMSM_OK;
  }
  TRY(bind_device(c));
  size_t pb = DISPATCH(c, affine_bytes<Fq>());
  amsm_bases* b = new (std::nothrow) amsm_bases();
  if (!b) return AMSM_E_OOM;
  b->curve = c->curve;
  b->device = c->device;
  b->n = n_half;
  if (gate_alloc(c, GATE_DEVICE, n_half * pb, false, (void**)&b->d_table) != AMSM_OK) {
    delete b;
    return AMSM_E_OOM;
  }
  u32 canon[8];
  canonical_scalar(c->curve, x_mont, canon);
  const u32* l = key->d_table;  // level 0 of a precomputed table is the key itself
  const u32* r = (const u32*)((const char*)key->d_table + n_half * pb);
  u32* scratch = fold_scratch(c, n_half);
  // a key with window multiples folds through them (c + 1 doublings instead of nbits; msm_kernels.h k_points_fold_tab) -- the
  // top level of a bucket-per-lane table sits 2^top_shift short of its place and is left out.  An x that does not fit the usable
  // levels (fold_recode.h: fold_tab_ops says) takes the plain ladder
  bool done = false;
  if (key->precomp && key->W > 1 && key->n < (1ull << 31)) {
    const u32 levels = (u32)(key->top_shift ? key->W - 1 : key->W);
    FoldTabOps ops;
    done = fold_tab_ops((u32)key->c, (u32)key->W, (u32)key->n_narrow, levels, canon, nbits, &ops);
    if (done) DISPATCH_DO(c, launch_points_fold_tab<Fq>(c->stream, l, (u32)key->n, (u32)n_half, ops, b->d_table, scratch));
  }
  if (!done) {
    FoldDigits d;
    const bool glv = DISPATCH(c, host::fold_digits<Fq>(canon, nbits, &d));
    DISPATCH_DO(c, launch_points_fold<Fq>(c->stream, l, r, (u32)n_half, d, glv, b->d_table, false, scratch));
  }
  if (hipGetLastError() != hipSuccess || hipEventCreateWithFlags(&b->ready, hipEventDisableTiming) != hipSuccess ||
      hipEventRecord(b->ready, c->stream) != hipSuccess) {
    (void)hipGetLastError();
    if (b->ready) (void)hipEventDestroy(b->ready);
    (void)hipStreamSynchronize(c->stream);
    (void)gate_free(b->d_table);
    delete b;
    return AMSM_E_HIP;
  }
  *out = b;  // stream-ordered: MSM prep and further folds are ordered behind the context's stream; others wait for `ready`
  return AMSM_OK;
}

int amsm_vec_inner_product(amsm_ctx* c, const void* d_a, const void* d_b, size_t n, uint64_t* out_mont) {
  if (!c || !out_mont || (n && (!d_a || !d_b)) || n >= (1ull << 32)) return AMSM_E_INVALID_ARG;
  if (c->host_only) return CPU_CALL(c, vec_inner_product, d_a, d_b, n, out_mont);
  TRY(bind_device(c));
  memset(out_mont, 0, 32);
  if (!n) return AMSM_OK;
  const u32 blocks = vec_reduce_grid((u32)n, vec_grid_of(c));
  Slot* sl = &c->slot[0];
  TRY(ensure(sl->red_out, (size_t)blocks * 32 + 4096));
  TRY(ensure_pinned(sl, (size_t)blocks * 32));
  DISPATCH_DO(c, launch_vec_inner_product<Fr>(c->stream, (const u32*)d_a, (const u32*)d_b, (u32)n, blocks, (u32*)sl->red_out.p));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(sl->h_pinned, sl->red_out.p, (size_t)blocks * 32, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  const u64* h = (const u64*)sl->h_pinned;
  DISPATCH_DO(c, {
    host::HFe<Fr> acc = host::h_zero<Fr>(), t;
    for (u32 i = 0; i < blocks; i++) {
      memcpy(t.v, h + 4 * i, 32);
      acc = host::h_add<Fr>(acc, t);
    }
    memcpy(out_mont, acc.v, 32);
  });
  return AMSM_OK;
}

int amsm_vec_powers(amsm_ctx* c, const uint64_t* point_mont, size_t n, void* d_out) {
  if (!c || !point_mont || (n && !d_out) || n >= (1ull << 32)) return AMSM_E_INVALID_ARG;
  if (c->host_only) return CPU_CALL(c, vec_powers, point_mont, n, d_out);
  TRY(bind_device(c));
  if (!n) return AMSM_OK;
  u32 pt[8];
  memcpy(pt, point_mont, 32);
  DISPATCH_DO(c, launch_vec_powers<Fr>(c->stream, pt, (u32)n, (u32*)d_out));
  HIP_TRY(hipGetLastError());
  return AMSM_OK;
}

static bool poly_args_ok(const void* const* d_coeffs, const size_t* lens, size_t n_polys, void* const* d_quot, bool div) {
  if (!n_polys) return true;
  if (!d_coeffs || !lens || (div && !d_quot)) return false;
  for (size_t k = 0; k < n_polys; k++) {
    if (lens[k] >= (1ull << 32) || (lens[k] && !d_coeffs[k])) return false;
    if (div && lens[k] > 1 && !d_quot[k]) return false;
  }
  return true;
}
int amsm_poly_evaluate_batch(amsm_ctx* c, const void* const* d_coeffs, const size_t* lens, size_t n_polys, const uint64_t* point_mont,
                             uint64_t* out_mont) {
  if (!c || (n_polys && (!point_mont || !out_mont)) || !poly_args_ok(d_coeffs, lens, n_polys, nullptr, false)) return AMSM_E_INVALID_ARG;
  if (c->host_only) return CPU_CALL(c, poly_div_linear_batch, d_coeffs, lens, n_polys, point_mont, true, nullptr, out_mont);
  TRY(bind_device(c));
  if (!n_polys) return AMSM_OK;
  return DISPATCH(c, poly_impl<Fr>(c, d_coeffs, lens, n_polys, point_mont, true, nullptr, out_mont));
}
int amsm_poly_evaluate(amsm_ctx* c, const void* d_coeffs, size_t n, const uint64_t* point_mont, uint64_t* out_mont) {
  return amsm_poly_evaluate_batch(c, &d_coeffs, &n, 1, point_mont, out_mont);
}
int amsm_poly_div_linear_batch(amsm_ctx* c, const void* const* d_coeffs, const size_t* lens, size_t n_polys, const uint64_t* z_mont,
                               void* const* d_quot, uint64_t* rem_mont) {
  if (!c || (n_polys && !z_mont) || !poly_args_ok(d_coeffs, lens, n_polys, d_quot, true)) return AMSM_E_INVALID_ARG;
  if (c->host_only) return CPU_CALL(c, poly_div_linear_batch, d_coeffs, lens, n_polys, z_mont, false, d_quot, rem_mont);
  TRY(bind_device(c));
  if (!n_polys) return AMSM_OK;
  return DISPATCH(c, poly_impl<Fr>(c, d_coeffs, lens, n_polys, z_mont, false, d_quot, rem_mont));
}
int amsm_poly_div_linear(amsm_ctx* c, const void* d_coeffs, size_t n, const uint64_t* z_mont, void* d_quot, uint64_t* rem_mont) {
  return amsm_poly_div_linear_batch(c, &d_coeffs, &n, 1, z_mont, &d_quot, rem_mont);
}

int amsm_ipa_jump_fold(amsm_ctx* c, const amsm_bases* key, size_t log_key, const uint64_t* xi_mont, size_t j, uint64_t* out_xy,
                       uint8_t* out_inf) {
  if (!c || !key || !out_xy || (j && !xi_mont) || log_key == 0 || log_key > 30 || j > log_key || !key_matches(c, key)) return AMSM_E_INVALID_ARG;
  if (((size_t)1 << log_key) > key->n) return AMSM_E_INVALID_ARG;  // (the key has fewer generators than the opening names: both backends)
  for (size_t r = 0; r < j; r++) {
    bool zero = true;
    for (int k = 0; k < 4; k++) zero = zero && xi_mont[4 * r + k] == 0;
    if (zero) return AMSM_E_INVALID_ARG;
  }
  if (key_sharded(key)) return AMSM_E_UNSUPPORTED;  // (a fold pairs generators of different shards)
  if (c->host_only) return CPU_CALL(c, ipa_jump_fold, key, log_key, xi_mont, j, out_xy, out_inf);
  TRY(bind_device(c));
  return DISPATCH(c, ipa_jump_fold_impl<Fq, Fr>(c, key, log_key, xi_mont, j, out_xy, out_inf));
}
int amsm_ipa_check_poly_coeffs(amsm_ctx* c, const uint64_t* xi_mont, size_t k, void* d_out) {
  if (!c || !d_out || (k && !xi_mont) || k > 30) return AMSM_E_INVALID_ARG;
  if (c->host_only) return CPU_CALL(c, check_poly_coeffs, xi_mont, k, d_out);
  TRY(bind_device(c));
  DISPATCH_DO(c, launch_check_poly_coeffs<Fr>(c->stream, (const u32*)xi_mont, (u32)k, (u32*)d_out));
  HIP_TRY(hipGetLastError());
  return AMSM_OK;
}

int amsm_ipa_round_scalars(amsm_ctx* c, const uint64_t* xi_mont, size_t j, size_t log_n, const void* d_coeffs,
                           void* d_out_l, void* d_out_r) {
  if (!c || !d_coeffs || !d_out_l || (j && !xi_mont) || log_n == 0 || log_n > 30 || j >= log_n)
    return AMSM_E_INVALID_ARG;
  if (c->host_only) return CPU_CALL(c, ipa_round_scalars, xi_mont, j, log_n, d_coeffs, d_out_l, d_out_r);
  TRY(bind_device(c));
  DISPATCH_DO(c, launch_ipa_round_scalars<Fr>(c->stream, (const u32*)xi_mont, (u32)j, (u32)log_n, (const u32*)d_coeffs,
                                       (u32*)d_out_l, (u32*)d_out_r));
  HIP_TRY(hipGetLastError());
  return AMSM_OK;
}

int amsm_ipa_round(amsm_ctx* c, const amsm_bases* key, const uint64_t* xi_mont, size_t j, size_t log_key, const void* d_coeffs,
                   const void* d_z, void* d_u, uint64_t* out_lr_xy, uint8_t* out_lr_inf, uint64_t* out_ip_mont) {
  if (!c || !key || !d_coeffs || !d_z || !d_u || !out_lr_xy || !out_ip_mont || (j && !xi_mont) || log_key == 0 || log_key > 30 ||
      j >= log_key || !key_matches(c, key))
    return AMSM_E_INVALID_ARG;
  if (c->host_only)
    return CPU_CALL(c, ipa_round, key, xi_mont, j, log_key, (void*)d_coeffs, (void*)d_z, d_u, out_lr_xy, out_lr_inf, out_ip_mont, nullptr,
                    nullptr);
  TRY(bind_device(c));
  const size_t half = (size_t)1 << (log_key - j - 1);
  if (key_sharded(key))
    return DISPATCH(c, ipa_round_sharded_impl<Fq, Fr>(c, key, xi_mont, j, log_key, d_coeffs, d_z, half, d_u, out_lr_xy, out_lr_inf,
                                                                    out_ip_mont, nullptr, nullptr));
  return DISPATCH(c, ipa_round_impl<Fq, Fr>(c, key, xi_mont, j, log_key, d_coeffs, d_z, half, d_u, out_lr_xy, out_lr_inf,
                                                          out_ip_mont));
}

int amsm_ipa_round_fused(amsm_ctx* c, const amsm_bases* key, const uint64_t* xi_mont, size_t j, size_t log_key, void* d_coeffs,
                         void* d_z, const uint64_t* fold_x_mont, const uint64_t* h_prime_xy, void* d_u, uint64_t* out_lr_xy,
                         uint8_t* out_lr_inf, uint64_t* out_ip_mont) {
  if (!c || !key || !d_coeffs || !d_z || !d_u || !out_lr_xy || !out_ip_mont || (j && !xi_mont) || log_key == 0 || log_key > 30 ||
      j >= log_key || !key_matches(c, key))
    return AMSM_E_INVALID_ARG;
  if (fold_x_mont) {
    bool zero = true;
    for (int k = 0; k < 4; k++) zero = zero && fold_x_mont[k] == 0;
    if (zero) return AMSM_E_INVALID_ARG;  // a zero challenge has no inverse (the reference's verifier rejects it too)
  }
  if (c->host_only)
    return CPU_CALL(c, ipa_round, key, xi_mont, j, log_key, d_coeffs, d_z, d_u, out_lr_xy, out_lr_inf, out_ip_mont, fold_x_mont,
                    h_prime_xy);
  TRY(bind_device(c));
  const size_t half = (size_t)1 << (log_key - j - 1);
  if (key_sharded(key))
    return DISPATCH(c, ipa_round_sharded_impl<Fq, Fr>(c, key, xi_mont, j, log_key, d_coeffs, d_z, half, d_u, out_lr_xy, out_lr_inf,
                                                                    out_ip_mont, fold_x_mont, h_prime_xy));
  return DISPATCH(c, ipa_round_impl<Fq, Fr>(c, key, xi_mont, j, log_key, d_coeffs, d_z, half, d_u, out_lr_xy, out_lr_inf,
                                                          out_ip_mont, fold_x_mont, h_prime_xy));
}

int amsm_matrix_load(amsm_ctx* c, const uint32_t* row_ptr, const uint32_t* col_idx, const uint64_t* vals, size_t n_rows,
                     size_t nnz, amsm_matrix** out) {
  if (!c || !out || !row_ptr || (nnz && (!col_idx || !vals)) || n_rows >= (1ull << 32) || nnz >= (1ull << 32))
    return AMSM_E_INVALID_ARG;
  if (row_ptr[0] != 0 || row_ptr[n_rows] != nnz) return AMSM_E_INVALID_ARG;
  if (!c->host_only) TRY(bind_device(c));
  amsm_matrix* m = new (std::nothrow) amsm_matrix();
  if (!m) return AMSM_E_OOM;
  m->curve = c->curve;
  m->device = c->device;
  m->n_rows = n_rows;
  m->nnz = nnz;
  if (c->host_only) {
    m->host = true;
    if (gate_alloc(c, GATE_HOST, (n_rows + 1) * 4, false, (void**)&m->d_row_ptr) != AMSM_OK ||
        gate_alloc(c, GATE_HOST, std::max<size_t>(nnz, 1) * 4, false, (void**)&m->d_col) != AMSM_OK ||
        gate_alloc(c, GATE_HOST, std::max<size_t>(nnz, 1) * 32, false, (void**)&m->d_val) != AMSM_OK) {
      amsm_matrix_free(m);
      return AMSM_E_OOM;
    }
    memcpy(m->d_row_ptr, row_ptr, (n_rows + 1) * 4);
    if (nnz) {
      memcpy(m->d_col, col_idx, nnz * 4);
      memcpy(m->d_val, vals, nnz * 32);
    }
    *out = m;
    return AMSM_OK;
  }
  // (the three arrays: a refusal of the second or third leaves the earlier ones to amsm_matrix_free below)
  if (gate_alloc(c, GATE_DEVICE, (n_rows + 1) * 4, false, (void**)&m->d_row_ptr) != AMSM_OK ||
      gate_alloc(c, GATE_DEVICE, std::max<size_t>(nnz, 1) * 4, false, (void**)&m->d_col) != AMSM_OK ||
      gate_alloc(c, GATE_DEVICE, std::max<size_t>(nnz, 1) * 32, false, (void**)&m->d_val) != AMSM_OK) {
    amsm_matrix_free(m);
    return AMSM_E_OOM;
  }
  bool ok = hipMemcpyAsync(m->d_row_ptr, row_ptr, (n_rows + 1) * 4, hipMemcpyHostToDevice, c->stream) == hipSuccess;
  if (ok && nnz) {
    ok = hipMemcpyAsync(m->d_col, col_idx, nnz * 4, hipMemcpyHostToDevice, c->stream) == hipSuccess &&
         hipMemcpyAsync(m->d_val, vals, nnz * 32, hipMemcpyHostToDevice, c->stream) == hipSuccess;
  }
  ok = hipStreamSynchronize(c->stream) == hipSuccess && ok;  // (synchronised either way: the arrays are freed below)
  if (!ok) {
    (void)hipGetLastError();
    amsm_matrix_free(m);
    return AMSM_E_OOM;
  }
  *out = m;
  return AMSM_OK;
}
size_t amsm_matrix_rows(const amsm_matrix* m) { return m ? m->n_rows : 0; }
void amsm_matrix_free(amsm_matrix* m) {
  if (!m) return;
  if (m->host) {
    (void)gate_free(m->d_row_ptr);
    (void)gate_free(m->d_col);
    (void)gate_free(m->d_val);
    delete m;
    return;
  }
  (void)hipSetDevice(m->device);
  (void)gate_free(m->d_row_ptr);
  (void)gate_free(m->d_col);
  (void)gate_free(m->d_val);
  delete m;
}
int amsm_matrix_vec_mul(amsm_ctx* c, const amsm_matrix* m, const void* d_input, size_t n_input, const void* d_witness,
                        size_t n_witness, void* d_out) {
  if (!c || !m || m->curve != c->curve || m->device != c->device || (m->n_rows && !d_out) ||
      (n_input && !d_input) || (n_witness && !d_witness) || n_input >= (1ull << 32) || n_witness >= (1ull << 32))
    return AMSM_E_INVALID_ARG;
  if (c->host_only) return CPU_CALL(c, spmv, m, d_input, n_input, d_witness, n_witness, d_out);
  TRY(bind_device(c));
  if (!m->n_rows) return AMSM_OK;
  DISPATCH_DO(c, launch_spmv<Fr>(c->stream, m->d_row_ptr, m->d_col, m->d_val, (const u32*)d_input, (u32)n_input,
                          (const u32*)d_witness, (u32)n_witness, (u32*)d_out, (u32)m->n_rows));
  HIP_TRY(hipGetLastError());
  return AMSM_OK;
}

int amsm_hp_t_vecs(amsm_ctx* c, const void* const* d_a, const size_t* a_lens, const void* const* d_b,
                   const size_t* b_lens, size_t n_inputs, const uint64_t* mu_mont, size_t n_mu, const void* d_hiding_a,
                   size_t hiding_a_len, const void* d_hiding_b, size_t hiding_b_len, void* const* d_t, size_t len) {
  if (!c || !d_a || !d_b || !mu_mont || !d_t || len >= (1ull << 32)) return AMSM_E_INVALID_ARG;
  if (c->host_only)
    return CPU_CALL(c, t_vecs, d_a, a_lens, d_b, b_lens, n_inputs, mu_mont, n_mu, d_hiding_a, hiding_a_len, d_hiding_b, hiding_b_len, d_t,
                    len);
  TRY(bind_device(c));
  return DISPATCH(c, t_vecs_impl<Fr>(c, d_a, a_lens, d_b, b_lens, n_inputs, mu_mont, n_mu, d_hiding_a, hiding_a_len,
                                         d_hiding_b, hiding_b_len, d_t, len));
}
