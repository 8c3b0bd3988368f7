// Part of api.hip (inside its anonymous namespace): partial records, the grouped MSM and the IPA opening round, the
// scalar-field vector entry points' implementations.
template <class Fq>
int partials_combine_impl(amsm_ctx* ctx, const void* d_partials, size_t count, uint64_t* out_xy, uint8_t* out_inf) {
  size_t rec = xyzz_bytes<Fq>();
  Slot* sl = &ctx->slot[0];
  TRY(ensure_pinned(sl, count * rec));
  if (count) {
    HIP_TRY(hipMemcpyAsync(sl->h_pinned, d_partials, count * rec, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
  }
  host::HXYZZ<Fq> acc = host::hx_inf<Fq>();
  for (size_t i = 0; i < count; i++)
    acc = host::hx_add<Fq>(acc, host::hx_from_device<Fq>((const u32*)sl->h_pinned + i * (rec / 4)));
  write_affine<Fq>(acc, out_xy, out_inf);
  return AMSM_OK;
}

template <class Fq, class Fr>
int msm_grouped_impl(amsm_ctx* ctx, const amsm_bases* bases, size_t base_off, const void* d_scalars, size_t n, int mont,
                     unsigned group_shift, uint64_t* out_xy, uint8_t* out_inf) {
  if (base_off > bases->n) return AMSM_E_INVALID_ARG;
  n = std::min(n, bases->n - base_off);
  std::vector<host::HXYZZ<Fq>> r(2, host::hx_inf<Fq>());
  if (n) {
    stage_begin(ctx);
    TRY(prep_fork(ctx));
    TRY((msm_enqueue<Fq, Fr>(ctx, &ctx->slot[0], single_job(bases, base_off, d_scalars, n, mont, (int)group_shift), Place::LONE)));
    int rc = msm_collect<Fq>(ctx, &ctx->slot[0], r.data());
    stage_end(ctx);
    if (rc != AMSM_OK) return rc;
  }
  write_affine_batch<Fq>(r, out_xy, out_inf);
  return AMSM_OK;
}

// One IPA opening round with ONE synchronisation: the round's scalar expansion, the grouped MSM over the key and the two
// inner products <c_r, z_l>, <c_l, z_r>; the inner-product kernels are queued behind accumulate L0 on the context's
// stream and run beside the MSM's tail.
// The vector half of a round (shared with the sharded form, api_multi.inc): the two inner products -- their per-workgroup partial
// sums go straight to pinned host memory (no copy in the chain) -- with the previous round's fold c <- c_l + x^-1 c_r, z <- z_l + x z_r
// in the same launch when one is pending, then the round's scalars into d_u.
template <class Fr>
int ipa_round_vectors(amsm_ctx* ctx, const uint64_t* xi_mont, size_t j, size_t log_key, const void* d_coeffs, const void* d_z, size_t half,
                      void* d_u, const uint64_t* fold_x_mont, u32* blocks_out) {
  const u32 blocks = vec_reduce_grid((u32)half, vec_grid_of(ctx));
  *blocks_out = blocks;
  Slot* aux = &ctx->slot[1];  // only its pinned buffer: slot 1 carries no MSM during a single-MSM call
  TRY(ensure_pinned(aux, (size_t)2 * blocks * 32));
  u32* co = (u32*)d_coeffs;
  u32* z = (u32*)d_z;
  u32* part = (u32*)aux->h_pinned;
  if (fold_x_mont) {
    host::HFe<Fr> x, xinv;
    memcpy(x.v, fold_x_mont, 32);
    xinv = host::h_inv<Fr>(x);
    launch_ipa_fold_ip<Fr>(ctx->stream, co, z, (u32)half, (const u32*)x.v, (const u32*)xinv.v, blocks, part);
  } else {
    launch_vec_inner_product_pair<Fr>(ctx->stream, co + half * 8, z, co, z + half * 8, (u32)half, blocks, part);  // <c_r, z_l>, <c_l, z_r>
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(ctx->ip_ready, ctx->stream));
  launch_ipa_round_scalars<Fr>(ctx->stream, (const u32*)xi_mont, (u32)j, (u32)log_key, (const u32*)d_coeffs, (u32*)d_u, nullptr);
  HIP_TRY(hipGetLastError());
  return AMSM_OK;
}
// ... and its host half: the inner products summed from the partials, the h' multiples (on the host WHILE the MSM runs)
template <class Fq, class Fr>
int ipa_round_inner_products(amsm_ctx* ctx, u32 blocks, const uint64_t* h_prime_xy, uint64_t* out_ip_mont, host::HXYZZ<Fq> hterm[2]) {
  HIP_TRY(hipEventSynchronize(ctx->ip_ready));
  const u64* h = (const u64*)ctx->slot[1].h_pinned;
  for (int k = 0; k < 2; k++) {
    host::HFe<Fr> acc = host::h_zero<Fr>(), t;
    for (u32 i = 0; i < blocks; i++) {
      memcpy(t.v, h + 4 * ((size_t)k * blocks + i), 32);
      acc = host::h_add<Fr>(acc, t);
    }
    memcpy(out_ip_mont + 4 * k, acc.v, 32);
    hterm[k] = h_prime_xy ? host_mul_cached<Fq, Fr>(h_prime_xy, acc) : host::hx_inf<Fq>();
  }
  return AMSM_OK;
}
template <class Fq, class Fr>
int ipa_round_impl(amsm_ctx* ctx, const amsm_bases* key, const uint64_t* xi_mont, size_t j, size_t log_key, const void* d_coeffs,
                   const void* d_z, size_t half, void* d_u, uint64_t* out_lr_xy, uint8_t* out_lr_inf, uint64_t* out_ip_mont,
                   const uint64_t* fold_x_mont = nullptr, const uint64_t* h_prime_xy = nullptr) {
  const size_t n = (size_t)1 << log_key;
  if (n > key->n) return AMSM_E_INVALID_ARG;
  // every allocation the round's MSM needs, BEFORE the in-place fold below: an out-of-memory return must leave the caller's
  // vectors as they were (a retry would otherwise fold them twice and produce a wrong proof without any error).  What
  // can still fail after the fold is a scalar outside the field (AMSM_E_SCALAR_RANGE) or a device fault: amsm.h says that
  // d_coeffs / d_z are consumed whenever the call got past its argument checks.
  // (a small key: the round is a grouped direct sum -- msm_plan reserves for that form too)
  const MsmJob round_msm = single_job(key, 0, d_u, n, 1, (int)(log_key - 1 - j));
  {
    bool sp = false;
    TRY((msm_plan<Fq>(ctx, &ctx->slot[0], round_msm, &sp)));
  }
  u32 blocks = 0;
  TRY((ipa_round_vectors<Fr>(ctx, xi_mont, j, log_key, d_coeffs, d_z, half, d_u, fold_x_mont, &blocks)));
  std::vector<host::HXYZZ<Fq>> r(2, host::hx_inf<Fq>());
  stage_begin(ctx);
  TRY(prep_fork(ctx));
  {
    int rc_e = msm_enqueue<Fq, Fr>(ctx, &ctx->slot[0], round_msm, Place::LONE);
    if (rc_e != AMSM_OK) {
      stage_end(ctx);
      return rc_e;
    }
  }
  host::HXYZZ<Fq> hterm[2];
  TRY((ipa_round_inner_products<Fq, Fr>(ctx, blocks, h_prime_xy, out_ip_mont, hterm)));
  int rc = msm_collect<Fq>(ctx, &ctx->slot[0], r.data());
  stage_end(ctx);
  if (rc != AMSM_OK) return rc;
  if (h_prime_xy)
    for (int k = 0; k < 2; k++) r[k] = host::hx_add<Fq>(r[k], hterm[k]);
  write_affine_batch<Fq>(r, out_lr_xy, out_lr_inf);
  return AMSM_OK;
}

// groups of `count` consecutive records -> one affine point per group (one D2H copy, one batched normalisation)
template <class Fq>
int partials_combine_batch_impl(amsm_ctx* ctx, const void* d_partials, size_t n_groups, size_t count, uint64_t* out_xy,
                                uint8_t* out_inf) {
  size_t rec = xyzz_bytes<Fq>();
  Slot* sl = &ctx->slot[0];
  size_t total = n_groups * count;
  TRY(ensure_pinned(sl, total * rec + 64));
  if (total) {
    HIP_TRY(hipMemcpyAsync(sl->h_pinned, d_partials, total * rec, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
  }
  std::vector<host::HXYZZ<Fq>> pts(n_groups, host::hx_inf<Fq>());
  for (size_t g = 0; g < n_groups; g++)
    for (size_t i = 0; i < count; i++)
      pts[g] = host::hx_add<Fq>(pts[g], host::hx_from_device<Fq>((const u32*)sl->h_pinned + (g * count + i) * (rec / 4)));
  write_affine_batch<Fq>(pts, out_xy, out_inf);
  return AMSM_OK;
}

// n_vecs MSMs (pipelined like msm_batch_xyzz) -> n_vecs consecutive device records at d_out
template <class Fq, class Fr>
int msm_partial_batch_impl(amsm_ctx* ctx, const amsm_bases* bases, size_t base_off, const void* const* d_scalars,
                           size_t n_vecs, size_t n, int mont, void* d_out) {
  std::vector<host::HXYZZ<Fq>> r;
  TRY((msm_batch_xyzz<Fq, Fr>(ctx, bases, base_off, d_scalars, n_vecs, n, mont, &r)));
  if (!n_vecs) return AMSM_OK;
  size_t rec = xyzz_bytes<Fq>();
  Slot* sl = &ctx->slot[0];
  TRY(ensure_pinned(sl, n_vecs * rec + 64));
  u32* h = (u32*)sl->h_pinned;
  for (size_t v = 0; v < n_vecs; v++) {
    u32* o = h + v * (rec / 4);
    memcpy(o, r[v].x.v, rec / 4);
    memcpy(o + Fq::L, r[v].y.v, rec / 4);
    memcpy(o + 2 * Fq::L, r[v].zz.v, rec / 4);
    memcpy(o + 3 * Fq::L, r[v].zzz.v, rec / 4);
  }
  HIP_TRY(hipMemcpyAsync(d_out, h, n_vecs * rec, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return AMSM_OK;
}

// store a host XYZZ as a device record
template <class Fq>
int upload_xyzz(amsm_ctx* ctx, const host::HXYZZ<Fq>& p, void* d_out) {
  size_t rec = xyzz_bytes<Fq>();
  Slot* sl = &ctx->slot[0];
  TRY(ensure_pinned(sl, rec + 64));
  u32* h = (u32*)sl->h_pinned;
  memcpy(h, p.x.v, rec / 4);
  memcpy(h + Fq::L, p.y.v, rec / 4);
  memcpy(h + 2 * Fq::L, p.zz.v, rec / 4);
  memcpy(h + 3 * Fq::L, p.zzz.v, rec / 4);
  HIP_TRY(hipMemcpyAsync(d_out, h, rec, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return AMSM_OK;
}

template <class Fq, class Fr>
int msm_partial_impl(amsm_ctx* ctx, const amsm_bases* bases, size_t base_off, const void* d_scalars, size_t n, int mont,
                     void* d_out) {
  if (base_off > bases->n) return AMSM_E_INVALID_ARG;
  n = std::min(n, bases->n - base_off);
  if (n == 0) return upload_xyzz<Fq>(ctx, host::hx_inf<Fq>(), d_out);
  Slot* sl = &ctx->slot[0];
  stage_begin(ctx);
  TRY(prep_fork(ctx));
  TRY((msm_enqueue<Fq, Fr>(ctx, sl, single_job(bases, base_off, d_scalars, n, mont), Place::LONE)));
  if (sl->geom.n_sets == 1) {
    // single folded record: it stays on the device (copied record-to-record); the host only waits for
    // the range flag
    HIP_TRY(hipMemcpyAsync(d_out, sl->fold_out.p, xyzz_bytes<Fq>(), hipMemcpyDeviceToDevice, sl->tail));
    HIP_TRY(hipEventRecord(sl->done, sl->tail));
    host::HXYZZ<Fq> unused;
    int rc = msm_collect<Fq>(ctx, sl, &unused);
    stage_end(ctx);
    return rc;
  }
  host::HXYZZ<Fq> acc;
  int rc = msm_collect<Fq>(ctx, sl, &acc);
  stage_end(ctx);
  if (rc != AMSM_OK) return rc;
  return upload_xyzz<Fq>(ctx, acc, d_out);
}

template <class Fr>
int vec_combine_impl(amsm_ctx* ctx, const void* const* d_vecs, const size_t* lens, size_t n_vecs,
                     const uint64_t* coeffs, const void* d_hiding, size_t hiding_len, void* d_out, size_t n) {
  if (!n) return AMSM_OK;
  // more than VEC_MAX vectors (the reference has no limit): groups of VEC_MAX, the running sum carried as the "hiding"
  // addend of the next launch (in place: a lane reads its own element of d_out before it writes it)
  size_t done = 0;
  do {
    const size_t k = std::min(n_vecs - done, (size_t)VEC_MAX);
    CombineArgs a;
    memset(&a, 0, sizeof(a));
    for (size_t j = 0; j < k; j++) {
      a.vec[j] = (const u32*)d_vecs[done + j];
      a.len[j] = (u32)(lens ? std::min(lens[done + j], n) : n);
      memcpy(a.coeff[j], coeffs + 4 * (done + j), 32);
    }
    a.hiding = done ? (const u32*)d_out : (const u32*)d_hiding;
    a.hiding_len = done ? (u32)n : (u32)hiding_len;
    a.n_vecs = (u32)k;
    a.n = (u32)n;
    launch_vec_combine<Fr>(ctx->stream, vec_grid_of(ctx), a, (u32*)d_out);
    HIP_TRY(hipGetLastError());
    done += k;
  } while (done < n_vecs);
  return AMSM_OK;
}

// the point and the scan multipliers (z^POLY_E)^(2^k) of one polynomial; returns z^POLY_T
template <class Fr>
host::HFe<Fr> poly_powers(const host::HFe<Fr>& z, u32 z_out[8], u32 pw[8][8]) {
  host::HFe<Fr> x = z;
  memcpy(z_out, x.v, 32);
  for (u32 i = 0; i < POLY_LOG_E; i++) x = host::h_sqr<Fr>(x);
  for (int k = 0; k < 8; k++) {
    memcpy(pw[k], x.v, 32);
    x = host::h_sqr<Fr>(x);
  }
  return x;
}
// amsm_poly_evaluate_batch (d_quot == null; out_mont = the values) and amsm_poly_div_linear_batch (out_mont = the remainders, may be
// null: then nothing is waited for).  Workspace in slot 0's red_out: tile values | carries | remainders.
template <class Fr>
int poly_impl(amsm_ctx* ctx, const void* const* d_coeffs, const size_t* lens, size_t n_polys, const uint64_t* z_mont, bool one_point,
              void* const* d_quot, uint64_t* out_mont) {
  using H = host::HFe<Fr>;
  const bool eval = d_quot == nullptr;
  std::vector<u32> off(n_polys), nt(n_polys);
  size_t total = 0;
  for (size_t k = 0; k < n_polys; k++) {
    nt[k] = (u32)((lens[k] + POLY_T - 1) / POLY_T);
    off[k] = (u32)total;
    total += nt[k];
  }
  if (total >= (1ull << 32)) return AMSM_E_INVALID_ARG;
  if (out_mont) memset(out_mont, 0, n_polys * 32);
  if (!total) return AMSM_OK;
  Slot* sl = &ctx->slot[0];
  TRY(ensure(sl->red_out, (2 * total + n_polys) * 32 + 4096));
  if (out_mont) TRY(ensure_pinned(sl, (eval ? total : n_polys) * 32));
  u32* d_h = (u32*)sl->red_out.p;
  u32* d_carry = d_h + total * 8;
  u32* d_rem = d_carry + total * 8;
  if (!eval && out_mont) HIP_TRY(hipMemsetAsync(d_rem, 0, n_polys * 32, ctx->stream));
  for (size_t first = 0; first < n_polys; first += POLY_MAX) {
    const u32 m = (u32)std::min<size_t>(POLY_MAX, n_polys - first);
    PolyArgs a, b;
    memset(&a, 0, sizeof(a));
    memset(&b, 0, sizeof(b));
    u32 max_t = 0;
    for (u32 j = 0; j < m; j++) {
      const size_t k = first + j;
      H z;
      memcpy(z.v, z_mont + (one_point ? 0 : 4 * k), 32);
      a.c[j] = (const u32*)d_coeffs[k];
      a.q[j] = eval ? nullptr : (u32*)d_quot[k];
      a.len[j] = (u32)lens[k];
      a.off[j] = off[k];
      const H zt = poly_powers<Fr>(z, a.z[j], a.pw[j]);
      memcpy(a.zt, zt.v, 32);  // (read by the evaluation only: one point for all)
      b.c[j] = d_h + (size_t)off[k] * 8;
      b.q[j] = d_carry + (size_t)off[k] * 8;
      b.len[j] = nt[k];
      (void)poly_powers<Fr>(zt, b.z[j], b.pw[j]);
      max_t = std::max(max_t, nt[k]);
    }
    if (!max_t) continue;
    if (eval) {
      launch_poly_tile_values<Fr>(ctx->stream, a, m, max_t, true, d_h);
    } else {
      a.rem = out_mont ? d_rem + first * 8 : nullptr;
      if (max_t > 1) {  // (the grid covers the one-tile polynomials of a mixed batch too: their value is written and never read)
        launch_poly_tile_values<Fr>(ctx->stream, a, m, max_t, false, d_h);
        launch_poly_carries<Fr>(ctx->stream, b, m);
      }
      launch_poly_div_tiles<Fr>(ctx->stream, a, m, max_t, d_carry);
    }
    HIP_TRY(hipGetLastError());
  }
  if (!out_mont) return AMSM_OK;
  const size_t n_back = eval ? total : n_polys;
  HIP_TRY(hipMemcpyAsync(sl->h_pinned, eval ? d_h : d_rem, n_back * 32, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  const u64* h = (const u64*)sl->h_pinned;
  if (!eval) {
    memcpy(out_mont, h, n_polys * 32);
    return AMSM_OK;
  }
  for (size_t k = 0; k < n_polys; k++) {
    H acc = host::h_zero<Fr>(), t;
    for (u32 i = 0; i < nt[k]; i++) {
      memcpy(t.v, h + 4 * ((size_t)off[k] + i), 32);
      acc = host::h_add<Fr>(acc, t);
    }
    memcpy(out_mont + 4 * k, acc.v, 32);
  }
  return AMSM_OK;
}

template <class Fr>
int t_vecs_blocked(amsm_ctx* ctx, const void* const* d_a, const size_t* a_lens, const void* const* d_b, const size_t* b_lens,
                   size_t n_in, const uint64_t* mu, size_t n_mu, const void* d_ha, size_t ha_len, const void* d_hb,
                   size_t hb_len, void* const* d_t, size_t len);

template <class Fr>
int t_vecs_impl(amsm_ctx* ctx, const void* const* d_a, const size_t* a_lens, const void* const* d_b,
                const size_t* b_lens, size_t n_in, const uint64_t* mu, size_t n_mu, const void* d_ha, size_t ha_len,
                const void* d_hb, size_t hb_len, void* const* d_t, size_t len) {
  if (n_in < 1) return AMSM_E_INVALID_ARG;
  if (n_in > (size_t)HP_MAX_INPUTS)  // the reference has no limit (src/hp_as/mod.rs:288-349): blocks of HP_MAX_INPUTS
    return t_vecs_blocked<Fr>(ctx, d_a, a_lens, d_b, b_lens, n_in, mu, n_mu, d_ha, ha_len, d_hb, hb_len, d_t, len);
  bool hiding = d_ha != nullptr || d_hb != nullptr;
  // assert!(num_inputs + hiding <= mu_challenges.len())  (src/hp_as/mod.rs:295)
  if (n_in + (hiding ? 1 : 0) > n_mu) return AMSM_E_INVALID_ARG;
  if (!len) return AMSM_OK;
  TVecArgs a;
  memset(&a, 0, sizeof(a));
  for (size_t j = 0; j < n_in; j++) {
    a.a[j] = (const u32*)d_a[j];
    a.b[j] = (const u32*)d_b[j];
    a.a_len[j] = (u32)(a_lens ? std::min(a_lens[j], len) : len);
    a.b_len[j] = (u32)(b_lens ? std::min(b_lens[j], len) : len);
  }
  for (size_t j = 0; j < std::min<size_t>(n_mu, HP_MAX_INPUTS + 1); j++) memcpy(a.mu[j], mu + 4 * j, 32);
  a.hiding_a = (const u32*)d_ha;
  a.hiding_b = (const u32*)d_hb;
  a.hiding_a_len = (u32)ha_len;
  a.hiding_b_len = (u32)hb_len;
  for (size_t k = 0; k < 2 * n_in - 1; k++) a.t[k] = (u32*)d_t[k];
  a.len = (u32)len;
  launch_hp_t_vecs<Fr>(ctx->stream, vec_grid_of(ctx), a, (int)n_in);
  HIP_TRY(hipGetLastError());
  return AMSM_OK;
}

// More inputs + accumulators than one launch of the fused kernel takes.  The coefficient vectors are those of the product
// of  A(X) = sum_i mu_i a_i X^i (+ mu_n hiding_a)  and  B(X) = sum_j b_{n-1-j} X^j (+ mu_1 hiding_b):  cut both into blocks of
// M = HP_MAX_INPUTS coefficients, A = sum_p X^(M p) A_p, B = sum_q X^(M q) B_q; block product (p, q) is one launch of the
// fused kernel on a_{M p ..} and b_{n - M q - m ..} (it reverses its own b's) into scratch vectors, added into
// t[M (p + q) + k].  hiding_a belongs to A_0 (the kernel's own path, mu[m] = mu_n); hiding_b belongs to B_0 and the kernel
// would scale it by ITS mu[1]: right for p = 0, so for p > 0 its terms mu_i mu_1 (a_i o hiding_b) are added separately.
template <class Fr>
int t_vecs_blocked(amsm_ctx* ctx, const void* const* d_a, const size_t* a_lens, const void* const* d_b, const size_t* b_lens,
                   size_t n_in, const uint64_t* mu, size_t n_mu, const void* d_ha, size_t ha_len, const void* d_hb,
                   size_t hb_len, void* const* d_t, size_t len) {
  constexpr size_t M = HP_MAX_INPUTS;
  const bool hiding = d_ha != nullptr || d_hb != nullptr;
  if (n_in + (hiding ? 1 : 0) > n_mu) return AMSM_E_INVALID_ARG;  // src/hp_as/mod.rs:295
  if (!len) return AMSM_OK;
  const size_t n_t = 2 * n_in - 1, blocks = (n_in + M - 1) / M;
  using H = host::HFe<Fr>;
  H one = host::h_one<Fr>();
  u32 zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (size_t k = 0; k < n_t; k++)
    if (d_t[k]) launch_vec_fill(ctx->stream, (u32*)d_t[k], zero, (u32)len);
  std::vector<void*> scratch(2 * M, nullptr);  // 2 M - 1 block coefficients + one Hadamard product
  int rc = AMSM_OK;
  for (size_t k = 0; k < 2 * M && rc == AMSM_OK; k++) rc = amsm_dev_alloc(ctx, len * 32, &scratch[k]);
  auto add_into = [&](void* dst, const void* src, const uint64_t* coeff_src) -> int {  // dst += coeff * src (in place)
    const void* vs[2] = {dst, src};
    uint64_t cf[8];
    memcpy(cf, one.v, 32);
    memcpy(cf + 4, coeff_src, 32);
    return vec_combine_impl<Fr>(ctx, vs, nullptr, 2, cf, nullptr, 0, dst, len);
  };
  for (size_t p = 0; p < blocks && rc == AMSM_OK; p++)
    for (size_t q = 0; q < blocks && rc == AMSM_OK; q++) {
      const size_t ma = std::min(M, n_in - M * p), mb = std::min(M, n_in - M * q), m = std::max(ma, mb);
      const void* pa[M];
      const void* pb[M];
      size_t la[M], lb[M];
      uint64_t mu_blk[(M + 1) * 4];
      memset(mu_blk, 0, sizeof(mu_blk));
      for (size_t r = 0; r < m; r++) {
        const bool has_a = r < ma;
        pa[r] = has_a ? d_a[M * p + r] : d_a[0];
        la[r] = has_a ? (a_lens ? std::min(a_lens[M * p + r], len) : len) : 0;  // length 0: a zero coefficient
        if (has_a) memcpy(mu_blk + 4 * r, mu + 4 * (M * p + r), 32);
        // the kernel takes bc_j = b_set[m - 1 - j]; block q of B is bc_{M q + j'} = b_{n - 1 - M q - j'}, j' < mb
        const long src = (long)n_in - (long)(M * q) - (long)m + (long)r;
        const bool has_b = src >= 0 && (size_t)src < n_in && (m - 1 - r) < mb;
        pb[r] = has_b ? d_b[src] : d_b[0];
        lb[r] = has_b ? (b_lens ? std::min(b_lens[src], len) : len) : 0;
      }
      const bool use_ha = p == 0 && d_ha, use_hb = p == 0 && q == 0 && d_hb;
      if (use_ha) memcpy(mu_blk + 4 * m, mu + 4 * n_in, 32);  // the kernel scales hiding_a by mu[m]
      void* tb[2 * M - 1];
      for (size_t k = 0; k < 2 * m - 1; k++) tb[k] = scratch[k];
      rc = t_vecs_impl<Fr>(ctx, pa, la, pb, lb, m, mu_blk, m + 1, use_ha ? d_ha : nullptr, use_ha ? ha_len : 0,
                           use_hb ? d_hb : nullptr, use_hb ? hb_len : 0, tb, len);
      for (size_t k = 0; k < 2 * m - 1 && rc == AMSM_OK; k++) {
        const size_t dst = M * (p + q) + k;
        if (dst < n_t && d_t[dst]) rc = add_into(d_t[dst], tb[k], one.v);
      }
      if (p > 0 && q == 0 && d_hb && rc == AMSM_OK) {  // mu_i mu_1 (a_i o hiding_b) into t[M p + i]
        H mu1;
        memcpy(mu1.v, mu + 4, 32);
        for (size_t r = 0; r < ma && rc == AMSM_OK; r++) {
          const size_t i = M * p + r;
          if (i >= n_t || !d_t[i]) continue;
          const size_t l = std::min(std::min(a_lens ? a_lens[i] : len, hb_len), len);
          launch_vec_fill(ctx->stream, (u32*)scratch[2 * M - 1], zero, (u32)len);
          if (l) launch_vec_hadamard<Fr>(ctx->stream, vec_grid_of(ctx), (const u32*)d_a[i], (const u32*)d_hb, (u32*)scratch[2 * M - 1], (u32)l);
          H mi;
          memcpy(mi.v, mu + 4 * i, 32);
          H cf = host::h_mul<Fr>(mi, mu1);
          rc = add_into(d_t[i], scratch[2 * M - 1], cf.v);
        }
      }
    }
  if (hipGetLastError() != hipSuccess && rc == AMSM_OK) rc = AMSM_E_HIP;
  for (void* sp : scratch)
    if (sp) (void)amsm_dev_free(ctx, sp);  // stream-ordered reuse: the kernels above run on this context's stream
  return rc;
}

// ---- the jump fold of an IPA opening (round 6; msm_kernels.h: k_ipa_jump_accum) ---------------------------------------------------
// B_k = sum_t S_t G_(t m0 + k), k < m0 = 2^(log_key - j): the key folded by the j challenges xs (the first one pairs the two halves
// of the key: it is picked by the TOP bit of t), straight from the key's window table.  Eligible: a single-device precomputed key
// with plain equal-width windows that cover 256 bits (the tables of 2^8 .. 2^16- and 2^18 / 2^19-generator keys), m0 a multiple
// of 64.  Everything else: AMSM_E_UNSUPPORTED (the driver keeps running its rounds on the device).
constexpr u32 JUMP_NB = 256;  // values a digit's byte takes: buckets per set
template <class Fr>
void jump_fold_scalars(const uint64_t* xs_mont, size_t j, std::vector<std::array<u64, 4>>* canon) {
  std::vector<host::HFe<Fr>> s(1, host::h_one<Fr>());
  for (size_t r = 0; r < j; r++) {  // index = 2 * old + bit: the first challenge ends up on the top bit
    host::HFe<Fr> x;
    memcpy(x.v, xs_mont + 4 * r, 32);
    std::vector<host::HFe<Fr>> nx(s.size() * 2);
    for (size_t t = 0; t < s.size(); t++) {
      nx[2 * t] = s[t];
      nx[2 * t + 1] = host::h_mul<Fr>(s[t], x);
    }
    s.swap(nx);
  }
  canon->resize(s.size());
  for (size_t t = 0; t < s.size(); t++) {
    const host::HFe<Fr> c = host::h_from_mont<Fr>(s[t]);
    memcpy((*canon)[t].data(), c.v, 32);
  }
}
template <class Fq, class Fr>
int ipa_jump_fold_impl(amsm_ctx* ctx, const amsm_bases* key, size_t log_key, const uint64_t* xs_mont, size_t j, uint64_t* out_xy,
                       uint8_t* out_inf) {
  const size_t n = (size_t)1 << log_key, T = (size_t)1 << j, m0 = n >> j;
  const u32 c = (u32)key->c, W = (u32)key->W;
  // (a key that carries the direct-sum table runs its rounds as direct sums of ~0.15 ms: faster than the host's -- measured at 2^12 ..
  // 2^15 generators, profiles/r06_experiments.md section 2)
  if (key->d_small) return AMSM_E_UNSUPPORTED;
  if (!key->precomp || key->bpl || key->top_shift || key->n_narrow || n > key->n || (m0 & 63u) || c < 2 || c > 16 || (size_t)c * W < 256 ||
      (size_t)W * key->n >= ((size_t)1 << 31) || T * W * 2 >= ((size_t)1 << 26))
    return AMSM_E_UNSUPPORTED;
  // n_sets = 2 n_rep m0 (below) is the gridDim.y of the reduction launch: HIP takes at most 65535.  With n_rep >= 1 a small j is
  // out before any work; the callers keep such rounds on the device (amsm_ipa_round_fused)
  constexpr size_t MAX_GRID_Y = 65535;
  if (2 * m0 > MAX_GRID_Y) return AMSM_E_UNSUPPORTED;
  std::vector<std::array<u64, 4>> S;
  jump_fold_scalars<Fr>(xs_mont, j, &S);
  // signed c-bit digits (|d| <= 2^(c-1) <= 2^15), each split into two bytes; one list per (half, value) with entries
  struct Ent {
    u32 slot, word;
  };
  std::vector<Ent> ents;
  ents.reserve(T * W * 2);
  const u64 full = 1ull << c, halfw = 1ull << (c - 1);
  for (size_t t = 0; t < T; t++) {
    u64 carry = 0;
    for (u32 w = 0; w < W; w++) {
      const u32 bit = c * w, q = bit >> 6, r = bit & 63u;
      u64 raw = q < 4 ? S[t][q] >> r : 0;
      if (r + c > 64 && q + 1 < 4) raw |= S[t][q + 1] << (64 - r);
      raw = (raw & (full - 1)) + carry;
      long d = (long)raw;
      carry = 0;
      if (raw > halfw) {
        d = (long)raw - (long)full;
        carry = 1;
      }
      if (d == 0) continue;
      const u32 neg = d < 0 ? 0x80000000u : 0u, mag = (u32)(d < 0 ? -d : d);
      const u32 word = (u32)((size_t)w * key->n + t * m0) | neg;
      if (mag & 255u) ents.push_back({(mag & 255u) - 1u, word});
      if (mag >> 8) ents.push_back({JUMP_NB + (mag >> 8) - 1u, word});
    }
    if (carry) return AMSM_E_SCALAR_RANGE;  // (cannot happen: c W >= 256 > the scalars' 255 bits)
  }
  // counting sort by slot
  std::vector<u32> count(2 * JUMP_NB + 1, 0);
  for (const Ent& e : ents) count[e.slot + 1]++;
  for (size_t s = 0; s < 2 * JUMP_NB; s++) count[s + 1] += count[s];
  std::vector<u32> sorted(std::max<size_t>(ents.size(), 1)), cursor(count.begin(), count.end() - 1);
  for (const Ent& e : ents) sorted[cursor[e.slot]++] = e.word;
  // pieces: ~700 workgroups fill the chip once (three 4-wave workgroups of this kernel are resident per CU); at most 6 pieces per list
  u32 longest = 0;
  for (u32 s = 0; s < 2 * JUMP_NB; s++) longest = std::max(longest, count[s + 1] - count[s]);
  // (ONE generation of workgroups: ~890 pieces were two generations, the second nearly empty -- 205 us instead of ~100)
  u32 piece = std::max<u32>(32u, (u32)((ents.size() + 699) / 700));
  piece = std::max(piece, (longest + 5u) / 6u);
  piece = (piece + 3u) / 4u * 4u;  // (a multiple of the kernel's waves per workgroup: msm_kernels.h JUMP_WAVES = 4)
  for (;; piece += 4u) {
    size_t n_pieces = 0;
    for (u32 s = 0; s < 2 * JUMP_NB; s++) n_pieces += (count[s + 1] - count[s] + piece - 1) / piece;
    if (n_pieces <= 720 || piece >= 4096u) break;
  }
  const u32 n_rep = std::max(1u, (longest + piece - 1) / piece);
  std::vector<u32> list_off, list_slot;
  for (u32 s = 0; s < 2 * JUMP_NB; s++) {
    const u32 half = s / JUMP_NB, v = s % JUMP_NB;
    for (u32 at = count[s], p = 0; at < count[s + 1]; at += piece, p++) {
      list_off.push_back(at);
      list_slot.push_back((2 * p + half) * JUMP_NB + v);
    }
  }
  // (list_off[l + 1] must end piece l: pieces of one list are consecutive, and the next list starts where this one ends)
  list_off.push_back((u32)ents.size());
  const u32 n_lists = (u32)list_slot.size();
  const size_t rec = xyzz_bytes<Fq>();
  MsmGeom g;
  memset(&g, 0, sizeof(g));
  g.nb = JUMP_NB;
  if ((size_t)2 * n_rep * m0 > MAX_GRID_Y) return AMSM_E_UNSUPPORTED;  // (decided before anything is allocated)
  g.n_sets = (u32)(2 * n_rep * m0);
  const msel::TailPlan tp = tail_plan_of(g, Place::LONE);  // (the caller waits: the fused quad tail, two buckets per logical lane)
  Slot* sl = &ctx->slot[0];
  if (sl->busy) return AMSM_E_INVALID_ARG;
  TRY(ensure(sl->buckets, (size_t)g.n_sets * JUMP_NB * rec));
  TRY(reserve_tail<Fq>(ctx, sl, g.n_sets, tp));
  const size_t words = sorted.size() + list_off.size() + list_slot.size();
  TRY(ensure(sl->vals_a, words * 4 + 64));
  u32* d_ent = (u32*)sl->vals_a.p;
  u32* d_off = d_ent + sorted.size();
  u32* d_slot = d_off + list_off.size();
  hipStream_t st = ctx->stream;
  HIP_TRY(hipMemsetAsync(sl->buckets.p, 0, (size_t)g.n_sets * JUMP_NB * rec, st));
  if (n_lists) {
    HIP_TRY(hipMemcpyAsync(d_ent, sorted.data(), sorted.size() * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_off, list_off.data(), list_off.size() * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_slot, list_slot.data(), list_slot.size() * 4, hipMemcpyHostToDevice, st));
    if (key->ready) HIP_TRY(hipStreamWaitEvent(st, key->ready, 0));
    launch_ipa_jump_accum<Fq>(st, key->d_table, d_ent, d_off, d_slot, n_lists, (u32)m0, JUMP_NB, (u32*)sl->buckets.p);
  }
  launch_tail<Fq>(st, tp, (const u32*)sl->buckets.p, g, (u32*)sl->red2_rc.p, (u32*)sl->red_out.p, (u32*)sl->red_ticket.p, (u32*)sl->fold_out.p,
                  nullptr, (u32*)sl->h_pinned);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));  // (the host vectors above were pageable: their copies are done as well)
  const u32* h = (const u32*)sl->h_pinned;
  std::vector<host::HXYZZ<Fq>> out(m0);
  HostPool::get().run(m0, [&](size_t k) {  // set ((piece p, half), k) sits at (2 p + half) m0 + k
    host::HXYZZ<Fq> lo = host::hx_inf<Fq>(), hi = host::hx_inf<Fq>();
    for (u32 p = 0; p < n_rep; p++) {
      lo = host::hx_add<Fq>(lo, host::hx_from_device<Fq>(h + ((2 * p) * m0 + k) * (rec / 4)));
      hi = host::hx_add<Fq>(hi, host::hx_from_device<Fq>(h + ((2 * p + 1) * m0 + k) * (rec / 4)));
    }
    for (int d = 0; d < 8; d++) hi = host::hx_dbl<Fq>(hi);
    out[k] = host::hx_add<Fq>(lo, hi);
  });
  write_affine_batch<Fq>(out, out_xy, out_inf);
  return AMSM_OK;
}
