// Part of api.hip (inside its anonymous namespace): the HOST backend of the C ABI (SURVEY.md section 8(b): "CPU fallback selected
// by n_dev == 0"; BASELINE.json config 1 "plumbing, no GPU").  A context created with device_id = AMSM_DEVICE_HOST (or
// amsm_ctx_create_multi with n_dev = 0) owns no GPU: its "device" pointers are host allocations, its keys are host copies of the
// generators, and every entry point computes here -- a window-parallel signed-digit Pippenger on host_field.h for the MSMs
// (what ark-ec's `parallel` feature does with rayon, ark-ec ^0.2.0 msm, not in /root/reference: Cargo.toml:15), plain loops over
// the host pool for the scalar-field vector work.  Product code: nothing here touches oracle/.
// The selection is EXPLICIT: a GPU context never degrades to this path, and with no GPU amsm_ctx_create(.., device_id >= 0, ..)
// still fails with AMSM_E_NO_DEVICE.  Results are the same canonical affine points / field elements the HIP path produces.
namespace cpu {

template <class Fq>
constexpr size_t pt_words() {  // u64 words of one affine point
  return 2 * host::HFe<Fq>::N;
}

// chunked parallel loop over [0, n) on the host pool
template <class F>
void par_for(size_t n, size_t grain, F&& fn) {
  if (n == 0) return;
  const size_t chunks = std::max<size_t>(1, std::min<size_t>((n + grain - 1) / grain, 4 * (HostPool::get().workers.size() + 1)));
  if (chunks == 1) {
    fn((size_t)0, n);
    return;
  }
  HostPool::get().run(chunks, [&](size_t t) { fn(n * t / chunks, n * (t + 1) / chunks); });
}

template <class Fr>
inline host::HFe<Fr> ld(const void* p, size_t i) {
  host::HFe<Fr> x;
  memcpy(x.v, (const char*)p + 32 * i, 32);
  return x;
}
template <class Fr>
inline void st(void* p, size_t i, const host::HFe<Fr>& x) {
  memcpy((char*)p + 32 * i, x.v, 32);
}

// ---- keys ----------------------------------------------------------------------------------------------------------
template <class Fq>
amsm_bases* bases_new(amsm_ctx* c, size_t n) {
  amsm_bases* b = new (std::nothrow) amsm_bases();
  if (!b) return nullptr;
  b->curve = c->curve;
  b->device = c->device;
  b->host = true;
  b->n = n;
  if (gate_alloc(c, GATE_HOST, std::max<size_t>(n, 1) * affine_bytes<Fq>(), false, (void**)&b->d_table) != AMSM_OK) {
    delete b;
    return nullptr;
  }
  return b;
}
// amsm_points_check on the host pool: host_points_check.h point_status, the definition itself (a 255-bit multiplication by r per
// BLS12-381 point).  report: counts of status 1, 2, 3 and the first bad index (n: none); status: n bytes or null
template <class Fq, class Fr>
int points_check(const uint64_t* xy, const uint8_t* is_inf, size_t n, uint64_t report[4], uint8_t* status) {
  constexpr size_t PW = pt_words<Fq>();
  std::mutex mu;
  uint64_t cnt[4] = {0, 0, 0, n};
  par_for(n, 16, [&](size_t lo, size_t hi) {
    uint64_t mine[4] = {0, 0, 0, n};
    for (size_t i = lo; i < hi; i++) {
      const uint8_t st = host::point_status<Fq, Fr>(xy + i * PW, is_inf && is_inf[i]);
      if (status) status[i] = st;
      if (st) {
        mine[st - 1]++;
        mine[3] = std::min<uint64_t>(mine[3], i);
      }
    }
    std::lock_guard<std::mutex> lk(mu);
    for (int k = 0; k < 3; k++) cnt[k] += mine[k];
    cnt[3] = std::min(cnt[3], mine[3]);
  });
  memcpy(report, cnt, sizeof(cnt));
  return AMSM_OK;
}
template <class Fq, class Fr>
int bases_load(amsm_ctx* c, const uint64_t* xy, const uint8_t* is_inf, size_t n, unsigned flags, amsm_bases** out) {
  if (flags > 63u) return AMSM_E_INVALID_ARG;  // (every other flag is a hint here: host keys carry no tables)
  if (flags & AMSM_BASES_CHECK) {
    uint64_t report[4];
    TRY((points_check<Fq, Fr>(xy, is_inf, n, report, nullptr)));
    if (report[0] | report[1] | report[2]) return AMSM_E_INVALID_POINT;
  }
  amsm_bases* b = bases_new<Fq>(c, n);
  if (!b) return AMSM_E_OOM;
  constexpr size_t PW = pt_words<Fq>();
  if (n) memcpy(b->d_table, xy, n * PW * 8);
  if (is_inf)
    for (size_t i = 0; i < n; i++)
      if (is_inf[i]) memset((u64*)b->d_table + i * PW, 0, PW * 8);
  *out = b;
  return AMSM_OK;
}
// G_i = k_i G, k_i = rng_scalar(seed, first + i) (msm_kernels.h: k_generate_bases): a fixed-base table of G, 64 additions each
template <class Fq, class Fr>
int bases_generate(amsm_ctx* c, uint64_t seed, size_t n, unsigned flags, amsm_bases** out) {
  if (flags > 31u) return AMSM_E_INVALID_ARG;
  amsm_bases* b = bases_new<Fq>(c, n);
  if (!b) return AMSM_E_OOM;
  constexpr size_t PW = pt_words<Fq>();
  if (n) {
    std::vector<u32> gen = generator_mont<Fq>();
    host::HFixedBase<Fq> fb;
    fb.build(host::hx_from_affine<Fq>((const u64*)gen.data(), false));
    par_for(n, 64, [&](size_t lo, size_t hi) {
      std::vector<host::HXYZZ<Fq>> pts(hi - lo);
      for (size_t i = lo; i < hi; i++) {
        u32 k32[8];
        rng_scalar(seed, i, k32);
        u64 k[4];
        memcpy(k, k32, 32);
        pts[i - lo] = fb.mul(k);
      }
      write_affine_batch<Fq>(pts, (u64*)b->d_table + lo * PW, nullptr);
    });
  }
  *out = b;
  return AMSM_OK;
}
// G_(first + i) of the derivation "amsm-sample-v1" (host_sample.h: sample_point; the kernels of sample_kernels.h give the same bits)
template <class Fq, class Fr>
int bases_sample(amsm_ctx* c, const uint8_t* domain, size_t domain_len, uint64_t first, size_t n, unsigned flags, amsm_bases** out) {
  if (flags > 31u) return AMSM_E_INVALID_ARG;
  amsm_bases* b = bases_new<Fq>(c, n);
  if (!b) return AMSM_E_OOM;
  constexpr size_t PW = pt_words<Fq>();
  const b2s::SamplePrefix prefix = b2s::sample_prefix(CurveOf<Fq>::type::id, domain, domain_len);
  std::atomic<int> exhausted{0};
  par_for(n, 16, [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; i++)
      if (!host::sample_point<Fq>(prefix, first + i, 0, (u64*)b->d_table + i * PW, nullptr)) exhausted.store(1, std::memory_order_relaxed);
  });
  if (exhausted.load()) {  // an index used up its 256 attempts: no key
    amsm_bases_free(b);
    return AMSM_E_UNSUPPORTED;
  }
  *out = b;
  return AMSM_OK;
}
template <class Fq>
int bases_read(const amsm_bases* b, size_t off, size_t n, uint64_t* xy, uint8_t* is_inf) {
  if (off > b->n || n > b->n - off) return AMSM_E_INVALID_ARG;
  constexpr size_t PW = pt_words<Fq>();
  if (n) memcpy(xy, (const u64*)b->d_table + off * PW, n * PW * 8);
  if (is_inf)
    for (size_t i = 0; i < n; i++) {
      u64 o = 0;
      for (size_t k = 0; k < PW; k++) o |= xy[i * PW + k];
      is_inf[i] = o == 0;
    }
  return AMSM_OK;
}

// ---- MSM -------------------------------------------------------------------------------------------------------------
// scalars -> canonical integers; AMSM_E_SCALAR_RANGE for a canonical-form scalar of 2^255 or more (include/amsm.h)
template <class Fr>
int canon_scalars(const void* scalars, size_t n, int mont, std::vector<std::array<u64, 4>>* ks) {
  ks->resize(n);
  std::atomic<int> bad{0};
  par_for(n, 4096, [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; i++) {
      host::HFe<Fr> s = ld<Fr>(scalars, i);
      if (mont) s = host::h_from_mont<Fr>(s);
      else if (s.v[3] >> 63) bad.store(1, std::memory_order_relaxed);
      memcpy((*ks)[i].data(), s.v, 32);
    }
  });
  return bad.load() ? AMSM_E_SCALAR_RANGE : AMSM_OK;
}
inline int window_for(size_t n) {
  int lg = ilog2_ceil(n < 2 ? 2 : n);
  return lg <= 8 ? 4 : (lg <= 11 ? 7 : (lg <= 14 ? 9 : (lg <= 17 ? 12 : (lg <= 20 ? 14 : 16))));
}
// sum over i in [0, n) (of group g when group_shift >= 0: ((i >> group_shift) & 1) == g) of ks[i] * pts[i]
template <class Fq>
void pippenger(const u64* pts, const std::vector<std::array<u64, 4>>& ks, size_t n, int group_shift, host::HXYZZ<Fq>* out) {
  using X = host::HXYZZ<Fq>;
  using H = host::HFe<Fq>;
  constexpr size_t PW = pt_words<Fq>();
  constexpr int N = H::N;
  const int groups = group_shift >= 0 ? 2 : 1;
  auto point = [&](size_t i, H* x, H* y) {
    memcpy(x->v, pts + i * PW, 8 * N);
    memcpy(y->v, pts + i * PW + N, 8 * N);
    return !(host::h_is_zero<Fq>(*x) && host::h_is_zero<Fq>(*y));
  };
  if (n <= 32) {  // a handful of pairs: shared doublings (Straus)
    for (int g = 0; g < groups; g++) {
      std::vector<X> p;
      std::vector<std::array<u64, 4>> k;
      for (size_t i = 0; i < n; i++) {
        if (groups == 2 && (int)((i >> group_shift) & 1) != g) continue;
        p.push_back(host::hx_from_affine<Fq>(pts + i * PW, false));
        k.push_back(ks[i]);
      }
      out[g] = host::hx_lincomb<Fq>(p.data(), reinterpret_cast<const u64(*)[4]>(k.data()), p.size(), nullptr);
    }
    return;
  }
  // signed digits without a carry chain: s' = s + sum_{w < W-1} 2^(c-1) 2^(c w); digit w = window w of s' minus 2^(c-1), the top
  // window as it is (s < 2^255 <= 2^(c (W-1) + c): it fits c bits)
  const int c = window_for(n), W = 255 / c + 1;
  const u64 half = 1ull << (c - 1);
  u64 off[4] = {0, 0, 0, 0};
  for (int w = 0; w + 1 < W; w++) {
    const int bit = c * w + c - 1;
    off[bit >> 6] |= 1ull << (bit & 63);
  }
  std::vector<X> win((size_t)groups * W, host::hx_inf<Fq>());
  HostPool::get().run((size_t)groups * W, [&](size_t t) {
    const int g = (int)(t / W), w = (int)(t % W);
    const bool top = w == W - 1;
    std::vector<X> bucket((size_t)half + 2, host::hx_inf<Fq>());  // |digit| <= 2^(c-1); the top window's <= 2^(c-1) + 1
    for (size_t i = 0; i < n; i++) {
      if (groups == 2 && (int)((i >> group_shift) & 1) != g) continue;
      const u64* k = ks[i].data();
      if (!(k[0] | k[1] | k[2] | k[3])) continue;
      u64 s[5];
      unsigned __int128 cy = 0;
      for (int j = 0; j < 4; j++) {
        cy += (unsigned __int128)k[j] + off[j];
        s[j] = (u64)cy;
        cy >>= 64;
      }
      s[4] = (u64)cy;
      const int bit = c * w, q = bit >> 6, r = bit & 63;
      u64 raw = s[q] >> r;
      if (r + c > 64 && q + 1 < 5) raw |= s[q + 1] << (64 - r);
      raw &= (1ull << c) - 1;
      long d = top ? (long)raw : (long)raw - (long)half;
      if (d == 0) continue;
      H x, y;
      if (!point(i, &x, &y)) continue;
      if (d < 0) {
        y = host::h_neg<Fq>(y);
        d = -d;
      }
      host::hx_madd<Fq>(bucket[(size_t)d], x, y);
    }
    X run = host::hx_inf<Fq>(), sum = host::hx_inf<Fq>();
    for (size_t j = bucket.size() - 1; j >= 1; j--) {
      run = host::hx_add<Fq>(run, bucket[j]);
      sum = host::hx_add<Fq>(sum, run);
    }
    win[t] = sum;
  });
  for (int g = 0; g < groups; g++) {
    X acc = win[(size_t)g * W + W - 1];
    for (int w = W - 2; w >= 0; w--) {
      for (int k = 0; k < c; k++) acc = host::hx_dbl<Fq>(acc);
      acc = host::hx_add<Fq>(acc, win[(size_t)g * W + w]);
    }
    out[g] = acc;
  }
}
template <class Fq, class Fr>
int msm_xyzz(const amsm_bases* b, size_t off, const void* scalars, size_t n, int mont, int group_shift, host::HXYZZ<Fq>* out) {
  if (off > b->n) return AMSM_E_INVALID_ARG;
  n = std::min(n, b->n - off);
  out[0] = host::hx_inf<Fq>();
  if (group_shift >= 0) out[1] = host::hx_inf<Fq>();
  if (n == 0) return AMSM_OK;
  std::vector<std::array<u64, 4>> ks;
  TRY(canon_scalars<Fr>(scalars, n, mont, &ks));
  pippenger<Fq>((const u64*)b->d_table + off * pt_words<Fq>(), ks, n, group_shift, out);
  return AMSM_OK;
}
template <class Fq, class Fr>
int msm_affine(const amsm_bases* b, size_t off, const void* scalars, size_t n, int mont, uint64_t* out_xy, uint8_t* out_inf) {
  host::HXYZZ<Fq> r;
  TRY((msm_xyzz<Fq, Fr>(b, off, scalars, n, mont, -1, &r)));
  write_affine<Fq>(r, out_xy, out_inf);
  return AMSM_OK;
}
// k MSMs (offs[v], ns[v], scalars[v]) -> k affine points, one batched normalisation; rand_mont / hiding_xy: + r_v * H
template <class Fq, class Fr>
int msm_multi_affine(const amsm_bases* b, size_t k, const size_t* offs, const void* const* scalars, const size_t* ns, int mont,
                     const uint64_t* const* rand_mont, const uint64_t* hiding_xy, uint64_t* out_xy, uint8_t* out_inf) {
  std::vector<host::HXYZZ<Fq>> r(k, host::hx_inf<Fq>());
  for (size_t v = 0; v < k; v++) {
    TRY((msm_xyzz<Fq, Fr>(b, offs[v], scalars[v], ns[v], mont, -1, &r[v])));
    if (rand_mont && rand_mont[v] && hiding_xy) {
      host::HFe<Fr> kk = host::h_from_mont<Fr>(ld<Fr>(rand_mont[v], 0));
      r[v] = host::hx_add<Fq>(r[v], host::hx_mul<Fq>(host::hx_from_affine<Fq>(hiding_xy, false), kk.v));
    }
  }
  write_affine_batch<Fq>(r, out_xy, out_inf);
  return AMSM_OK;
}
template <class Fq, class Fr>
int msm_grouped(const amsm_bases* b, size_t off, const void* scalars, size_t n, int mont, unsigned group_shift, uint64_t* out_xy,
                uint8_t* out_inf) {
  std::vector<host::HXYZZ<Fq>> r(2);
  TRY((msm_xyzz<Fq, Fr>(b, off, scalars, n, mont, (int)group_shift, r.data())));
  write_affine_batch<Fq>(r, out_xy, out_inf);
  return AMSM_OK;
}
template <class Fq>
void store_record(const host::HXYZZ<Fq>& p, void* out) {  // the partial record of amsm_msm_partial_device (ABI radix)
  u32* o = (u32*)out;
  constexpr size_t q = xyzz_bytes<Fq>() / 4;
  memcpy(o, p.x.v, q);
  memcpy(o + Fq::L, p.y.v, q);
  memcpy(o + 2 * Fq::L, p.zz.v, q);
  memcpy(o + 3 * Fq::L, p.zzz.v, q);
}
template <class Fq, class Fr>
int msm_partial_batch(const amsm_bases* b, size_t off, const void* const* scalars, size_t n_vecs, size_t n, int mont, void* out) {
  for (size_t v = 0; v < n_vecs; v++) {
    host::HXYZZ<Fq> r;
    TRY((msm_xyzz<Fq, Fr>(b, off, scalars[v], n, mont, -1, &r)));
    store_record<Fq>(r, (char*)out + v * xyzz_bytes<Fq>());
  }
  return AMSM_OK;
}
template <class Fq, class Fr>
int partials_combine_batch(const void* partials, size_t n_groups, size_t count, uint64_t* out_xy, uint8_t* out_inf) {
  std::vector<host::HXYZZ<Fq>> pts(n_groups, host::hx_inf<Fq>());
  const size_t q = xyzz_bytes<Fq>() / 4;
  for (size_t g = 0; g < n_groups; g++)
    for (size_t i = 0; i < count; i++) pts[g] = host::hx_add<Fq>(pts[g], host::hx_from_device<Fq>((const u32*)partials + (g * count + i) * q));
  write_affine_batch<Fq>(pts, out_xy, out_inf);
  return AMSM_OK;
}
template <class Fq, class Fr>
int pedersen(const amsm_bases* ck, const void* elems, size_t n, const uint64_t* rand_mont, const uint64_t* hiding_xy, uint64_t* out_xy,
             uint8_t* out_inf) {
  const size_t off = 0;
  const uint64_t* rm[1] = {rand_mont};
  return msm_multi_affine<Fq, Fr>(ck, 1, &off, &elems, &n, 1, rand_mont ? rm : nullptr, hiding_xy, out_xy, out_inf);
}

// ---- key folds (amsm_points_fold / amsm_bases_fold): out[i] = l[i] + x r[i], affine in, affine out ----------------------------
template <class Fq, class Fr>
int points_fold(const void* l, const void* r, size_t n, const uint64_t* x_mont, unsigned nbits, void* out) {
  constexpr size_t PW = pt_words<Fq>();
  host::HFe<Fr> x = host::h_from_mont<Fr>(ld<Fr>(x_mont, 0));
  for (unsigned bit = nbits; bit < 256; bit++) x.v[bit >> 6] &= ~(1ull << (bit & 63));  // the ladders walk the low nbits only
  par_for(n, 32, [&](size_t lo, size_t hi) {
    std::vector<host::HXYZZ<Fq>> acc(hi - lo);
    for (size_t i = lo; i < hi; i++) {
      host::HXYZZ<Fq> pr = host::hx_from_affine<Fq>((const u64*)r + i * PW, false);
      acc[i - lo] = host::hx_add<Fq>(host::hx_from_affine<Fq>((const u64*)l + i * PW, false), host::hx_mul<Fq>(pr, x.v));
    }
    write_affine_batch<Fq>(acc, (u64*)out + lo * PW, nullptr);
  });
  return AMSM_OK;
}

// ---- scalar-field vectors ----------------------------------------------------------------------------------------------------
template <class Fq, class Fr>
int vec_random(uint64_t seed, size_t n, int mont, void* out) {
  par_for(n, 4096, [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; i++) {
      u32 k[8];
      rng_scalar_fr<Fr>(seed, i, k);
      host::HFe<Fr> s;
      memcpy(s.v, k, 32);
      if (mont) s = host::h_to_mont<Fr>(s);
      st<Fr>(out, i, s);
    }
  });
  return AMSM_OK;
}
// amsm_vec_sample: the text of blind.h that k_vec_sample runs
template <class Fq, class Fr>
int vec_sample(int curve, const uint8_t* key, uint32_t stream, uint64_t first, size_t n, int mont, void* out) {
  const blind::Key k = blind::key_words(key);
  par_for(n, 1024, [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; i++) {
      u32 w[8];
      blind::scalar<Fr>(k, (u32)curve, stream, first + i, w);
      host::HFe<Fr> s;
      memcpy(s.v, w, 32);
      if (mont) s = host::h_to_mont<Fr>(s);
      st<Fr>(out, i, s);
    }
  });
  return AMSM_OK;
}
template <class Fq, class Fr>
int vec_hadamard(const void* a, const void* b, void* out, size_t n) {
  par_for(n, 4096, [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; i++) st<Fr>(out, i, host::h_mul<Fr>(ld<Fr>(a, i), ld<Fr>(b, i)));
  });
  return AMSM_OK;
}
// out[i] = sum_j coeff[j] vecs[j][i] (+ hiding[i]); entries beyond a vector's length read as zero (src/hp_as/mod.rs:492-512)
template <class Fq, class Fr>
int vec_combine(const void* const* vecs, const size_t* lens, size_t n_vecs, const uint64_t* coeffs, const void* hiding, size_t hiding_len,
                void* out, size_t n) {
  par_for(n, 2048, [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; i++) {
      host::HFe<Fr> acc = (hiding && i < hiding_len) ? ld<Fr>(hiding, i) : host::h_zero<Fr>();
      for (size_t j = 0; j < n_vecs; j++)
        if (i < (lens ? std::min(lens[j], n) : n)) acc = host::h_add<Fr>(acc, host::h_mul<Fr>(ld<Fr>(coeffs, j), ld<Fr>(vecs[j], i)));
      st<Fr>(out, i, acc);
    }
  });
  return AMSM_OK;
}
// compute_t_vecs (src/hp_as/mod.rs:288-349): coefficients of (sum_j mu_j a_j X^j + mu_n hiding_a) (sum_j b_{n-1-j} X^j + mu_1 hiding_b)
template <class Fq, class Fr>
int t_vecs(const void* const* a, const size_t* a_lens, const void* const* b, const size_t* b_lens, size_t n_in, const uint64_t* mu,
           size_t n_mu, const void* ha, size_t ha_len, const void* hb, size_t hb_len, void* const* t, size_t len) {
  if (n_in < 1) return AMSM_E_INVALID_ARG;
  const bool hiding = ha != nullptr || hb != nullptr;
  if (n_in + (hiding ? 1 : 0) > n_mu) return AMSM_E_INVALID_ARG;  // the reference's assert at :295
  using H = host::HFe<Fr>;
  par_for(len, 1024, [&](size_t lo, size_t hi) {
    std::vector<H> ac(n_in), bc(n_in);
    for (size_t li = lo; li < hi; li++) {
      for (size_t j = 0; j < n_in; j++) {
        H x = li < (a_lens ? std::min(a_lens[j], len) : len) ? ld<Fr>(a[j], li) : host::h_zero<Fr>();
        ac[j] = host::h_mul<Fr>(ld<Fr>(mu, j), x);
        bc[n_in - 1 - j] = li < (b_lens ? std::min(b_lens[j], len) : len) ? ld<Fr>(b[j], li) : host::h_zero<Fr>();
      }
      if (ha) ac[0] = host::h_add<Fr>(ac[0], host::h_mul<Fr>(li < ha_len ? ld<Fr>(ha, li) : host::h_zero<Fr>(), ld<Fr>(mu, n_in)));
      if (hb) bc[0] = host::h_add<Fr>(bc[0], host::h_mul<Fr>(li < hb_len ? ld<Fr>(hb, li) : host::h_zero<Fr>(), ld<Fr>(mu, 1)));
      for (size_t k = 0; k < 2 * n_in - 1; k++) {
        if (!t[k]) continue;
        H s = host::h_zero<Fr>();
        for (size_t i = (k < n_in ? 0 : k - (n_in - 1)); i <= std::min(k, n_in - 1); i++)
          s = host::h_add<Fr>(s, host::h_mul<Fr>(ac[i], bc[k - i]));
        st<Fr>(t[k], li, s);
      }
    }
  });
  return AMSM_OK;
}
template <class Fq, class Fr>
int vec_inner_product(const void* a, const void* b, size_t n, uint64_t* out_mont) {
  using H = host::HFe<Fr>;
  const size_t chunks = std::max<size_t>(1, std::min<size_t>(64, n / 4096));
  std::vector<H> part(chunks, host::h_zero<Fr>());
  HostPool::get().run(chunks, [&](size_t t) {
    H acc = host::h_zero<Fr>();
    for (size_t i = n * t / chunks; i < n * (t + 1) / chunks; i++) acc = host::h_add<Fr>(acc, host::h_mul<Fr>(ld<Fr>(a, i), ld<Fr>(b, i)));
    part[t] = acc;
  });
  H acc = host::h_zero<Fr>();
  for (const H& p : part) acc = host::h_add<Fr>(acc, p);
  memcpy(out_mont, acc.v, 32);
  return AMSM_OK;
}
template <class Fq, class Fr>
int vec_powers(const uint64_t* point_mont, size_t n, void* out) {
  using H = host::HFe<Fr>;
  const H x = ld<Fr>(point_mont, 0);
  par_for(n, 4096, [&](size_t lo, size_t hi) {
    H acc = host::h_one<Fr>(), base = x;  // x^lo, then a running product
    for (size_t e = lo; e; e >>= 1) {
      if (e & 1) acc = host::h_mul<Fr>(acc, base);
      base = host::h_sqr<Fr>(base);
    }
    for (size_t i = lo; i < hi; i++) {
      st<Fr>(out, i, acc);
      acc = host::h_mul<Fr>(acc, x);
    }
  });
  return AMSM_OK;
}
// x^e by square-and-multiply
template <class Fr>
host::HFe<Fr> fr_pow(host::HFe<Fr> base, size_t e) {
  host::HFe<Fr> acc = host::h_one<Fr>();
  for (; e; e >>= 1) {
    if (e & 1) acc = host::h_mul<Fr>(acc, base);
    base = host::h_sqr<Fr>(base);
  }
  return acc;
}
// chunk [lo, hi) of a polynomial by Horner from `acc`: r[i] = c[i] + z r[i+1]; q (may be null) receives q[i-1] = r[i], i >= 1
template <class Fr>
host::HFe<Fr> poly_chunk(const void* c, size_t lo, size_t hi, const host::HFe<Fr>& z, host::HFe<Fr> acc, void* q) {
  for (size_t i = hi; i-- > lo;) {
    acc = host::h_add<Fr>(ld<Fr>(c, i), host::h_mul<Fr>(z, acc));
    if (q && i) st<Fr>(q, i - 1, acc);
  }
  return acc;
}
// vec_kernels.h k_poly_*: the same three passes over chunks of the host pool (chunk values, a serial recurrence over the few
// chunks with the multipliers z^(chunk length), the chunks again from their carries); quot == null: evaluation only
template <class Fq, class Fr>
int poly_div_linear_batch(const void* const* coeffs, const size_t* lens, size_t n_polys, const uint64_t* z_mont, bool one_point,
                          void* const* quot, uint64_t* rem_mont) {
  using H = host::HFe<Fr>;
  for (size_t k = 0; k < n_polys; k++) {
    const size_t n = lens[k];
    const H z = ld<Fr>(z_mont, one_point ? 0 : k);
    void* q = quot ? quot[k] : nullptr;
    const size_t chunks = std::max<size_t>(1, std::min<size_t>((n + 4095) / 4096, 4 * (HostPool::get().workers.size() + 1)));
    auto bound = [&](size_t t) { return n * t / chunks; };
    std::vector<H> val(chunks), carry(chunks + 1, host::h_zero<Fr>());
    if (chunks > 1) {
      HostPool::get().run(chunks, [&](size_t t) { val[t] = poly_chunk<Fr>(coeffs[k], bound(t), bound(t + 1), z, host::h_zero<Fr>(), nullptr); });
      for (size_t t = chunks; t-- > 0;)  // carry[t] = r[bound(t)]
        carry[t] = host::h_add<Fr>(val[t], host::h_mul<Fr>(fr_pow<Fr>(z, bound(t + 1) - bound(t)), carry[t + 1]));
      if (q) HostPool::get().run(chunks, [&](size_t t) { (void)poly_chunk<Fr>(coeffs[k], bound(t), bound(t + 1), z, carry[t + 1], q); });
    } else {
      carry[0] = poly_chunk<Fr>(coeffs[k], 0, n, z, host::h_zero<Fr>(), q);
    }
    if (rem_mont) memcpy(rem_mont + 4 * k, carry[0].v, 32);
  }
  return AMSM_OK;
}
// coefficient p of prod_{i=1..k} (1 + xi_i X^(2^(k-i))) = product of the xi_i whose bit (k - i) is set in p
template <class Fq, class Fr>
int check_poly_coeffs(const uint64_t* xi, size_t k, void* out) {
  using H = host::HFe<Fr>;
  st<Fr>(out, 0, host::h_one<Fr>());
  for (size_t i = k; i >= 1; i--) {  // bit (k - i) joins: out[p + 2^(k-i)] = out[p] xi_i for the 2^(k-i) coefficients built so far
    const size_t step = (size_t)1 << (k - i);
    const H x = ld<Fr>(xi, i - 1);
    par_for(step, 4096, [&](size_t lo, size_t hi) {
      for (size_t p = lo; p < hi; p++) st<Fr>(out, p + step, host::h_mul<Fr>(ld<Fr>(out, p), x));
    });
  }
  return AMSM_OK;
}
// vec_kernels.h k_ipa_round_scalars
template <class Fq, class Fr>
int ipa_round_scalars(const uint64_t* xi, size_t j, size_t log_n, const void* c, void* out_l, void* out_r) {
  using H = host::HFe<Fr>;
  const size_t n = (size_t)1 << log_n, h = (size_t)1 << (log_n - 1 - j);
  // s_j over the top j bits of k: a table of 2^j products
  std::vector<H> s((size_t)1 << j, host::h_one<Fr>());
  for (size_t t = 0; t < j; t++) {
    const H x = ld<Fr>(xi, t);
    for (size_t p = 0; p < s.size(); p++)
      if ((p >> (j - 1 - t)) & 1) s[p] = host::h_mul<Fr>(s[p], x);
  }
  par_for(n, 2048, [&](size_t lo, size_t hi) {
    for (size_t k = lo; k < hi; k++) {
      const size_t idx = k & (h - 1);
      const bool right = (k >> (log_n - 1 - j)) & 1;
      const H v = host::h_mul<Fr>(ld<Fr>(c, right ? idx : h + idx), s[k >> (log_n - j)]);
      if (!out_r) {
        st<Fr>(out_l, k, v);
      } else {
        st<Fr>(out_l, k, right ? host::h_zero<Fr>() : v);
        st<Fr>(out_r, k, right ? v : host::h_zero<Fr>());
      }
    }
  });
  return AMSM_OK;
}
// api_schemes.inc ipa_jump_fold_impl on the host: the m0 folded generators as m0 MSMs of 2^j pairs over strided bases (any key)
template <class Fq, class Fr>
int ipa_jump_fold(const amsm_bases* key, size_t log_key, const uint64_t* xs, size_t j, uint64_t* out_xy, uint8_t* out_inf) {
  const size_t n = (size_t)1 << log_key, T = (size_t)1 << j, m0 = n >> j;
  if (n > key->n || m0 == 0) return AMSM_E_INVALID_ARG;
  std::vector<std::array<u64, 4>> S;
  jump_fold_scalars<Fr>(xs, j, &S);
  constexpr size_t PW = pt_words<Fq>();
  std::vector<host::HXYZZ<Fq>> out(m0);
  std::vector<u64> pts(T * PW);
  for (size_t k = 0; k < m0; k++) {
    for (size_t t = 0; t < T; t++) memcpy(pts.data() + t * PW, (const u64*)key->d_table + (t * m0 + k) * PW, PW * 8);
    pippenger<Fq>(pts.data(), S, T, -1, &out[k]);
  }
  write_affine_batch<Fq>(out, out_xy, out_inf);
  return AMSM_OK;
}
// api_schemes.inc ipa_round_impl on the host: optional in-place fold, the two inner products, the round's scalars, the grouped MSM
template <class Fq, class Fr>
int ipa_round(const amsm_bases* key, const uint64_t* xi, size_t j, size_t log_key, void* co, void* z, void* u, uint64_t* out_lr_xy,
              uint8_t* out_lr_inf, uint64_t* out_ip, const uint64_t* fold_x, const uint64_t* h_prime_xy) {
  using H = host::HFe<Fr>;
  const size_t n = (size_t)1 << log_key, half = (size_t)1 << (log_key - j - 1), cur = 2 * half;
  if (n > key->n) return AMSM_E_INVALID_ARG;
  if (fold_x) {
    const H x = ld<Fr>(fold_x, 0), xinv = host::h_inv<Fr>(x);
    par_for(cur, 2048, [&](size_t lo, size_t hi) {
      for (size_t i = lo; i < hi; i++) {
        st<Fr>(co, i, host::h_add<Fr>(ld<Fr>(co, i), host::h_mul<Fr>(xinv, ld<Fr>(co, cur + i))));
        st<Fr>(z, i, host::h_add<Fr>(ld<Fr>(z, i), host::h_mul<Fr>(x, ld<Fr>(z, cur + i))));
      }
    });
  }
  TRY((vec_inner_product<Fq, Fr>((const char*)co + 32 * half, z, half, out_ip)));      // <c_r, z_l>
  TRY((vec_inner_product<Fq, Fr>(co, (const char*)z + 32 * half, half, out_ip + 4)));  // <c_l, z_r>
  TRY((ipa_round_scalars<Fq, Fr>(xi, j, log_key, co, u, nullptr)));
  std::vector<host::HXYZZ<Fq>> r(2);
  TRY((msm_xyzz<Fq, Fr>(key, 0, u, n, 1, (int)(log_key - 1 - j), r.data())));
  if (h_prime_xy)
    for (int k = 0; k < 2; k++) r[k] = host::hx_add<Fq>(r[k], host_mul_cached<Fq, Fr>(h_prime_xy, ld<Fr>(out_ip, k)));
  write_affine_batch<Fq>(r, out_lr_xy, out_lr_inf);
  return AMSM_OK;
}
// vec_kernels.h k_spmv
template <class Fq, class Fr>
int spmv(const amsm_matrix* m, const void* input, size_t n_input, const void* witness, size_t n_witness, void* out) {
  using H = host::HFe<Fr>;
  par_for(m->n_rows, 1024, [&](size_t lo, size_t hi) {
    for (size_t r = lo; r < hi; r++) {
      H acc = host::h_zero<Fr>();
      for (u32 k = m->d_row_ptr[r]; k < m->d_row_ptr[r + 1]; k++) {
        const size_t i = m->d_col[k];
        H x = i < n_input ? ld<Fr>(input, i) : (i - n_input < n_witness ? ld<Fr>(witness, i - n_input) : host::h_zero<Fr>());
        acc = host::h_add<Fr>(acc, host::h_mul<Fr>(x, ld<Fr>(m->d_val, k)));
      }
      st<Fr>(out, r, acc);
    }
  });
  return AMSM_OK;
}

}  // namespace cpu

// curve dispatch of a cpu:: template
#define CPU_CALL(c, fn, ...) \
  with_curve((c)->curve, [&](auto cv_) { AMSM_CURVE_FIELDS(cv_); return cpu::fn<Fq, Fr>(__VA_ARGS__); })
