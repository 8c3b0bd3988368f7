// Part of api.hip (inside extern "C"): context-free host helpers -- linear combinations, scalar-field arithmetic, wire
// format, Poseidon sponge.
int amsm_host_lincomb(int curve, const uint64_t* xy, const uint8_t* is_inf, const uint64_t* scalars_mont, size_t n,
                      uint64_t* out_xy, uint8_t* out_inf) {
  if (!out_xy || (n && (!xy || !scalars_mont))) return AMSM_E_INVALID_ARG;
  return with_curve(curve, [&](auto cv) {
    AMSM_CURVE_FIELDS(cv);
    return host_lincomb_impl<Fq, Fr>(xy, is_inf, scalars_mont, n, out_xy, out_inf);
  });
}

int amsm_host_lincomb_batch(int curve, size_t n_jobs, const size_t* n_terms, const uint64_t* const* xy, const uint8_t* const* is_inf,
                            const uint64_t* const* scalars_mont, uint64_t* out_xy, uint8_t* out_inf) {
  if (n_jobs && (!n_terms || !xy || !scalars_mont || !out_xy)) return AMSM_E_INVALID_ARG;
  for (size_t j = 0; j < n_jobs; j++)
    if (n_terms[j] && (!xy[j] || !scalars_mont[j])) return AMSM_E_INVALID_ARG;
  return with_curve(curve, [&](auto cv) {
    AMSM_CURVE_FIELDS(cv);
    return host_lincomb_batch_impl<Fq, Fr>(n_jobs, n_terms, xy, is_inf, scalars_mont, out_xy, out_inf);
  });
}

int amsm_host_threads(void) { return (int)HostPool::get().workers.size(); }

int amsm_fr_mul(int curve, const uint64_t* a_mont, const uint64_t* b_mont, size_t n, uint64_t* out_mont) {
  if (n && !b_mont) return AMSM_E_INVALID_ARG;
  return amsm_fr_mul_impl(curve, a_mont, b_mont, n, out_mont);
}
int amsm_fr_add(int curve, const uint64_t* a_mont, const uint64_t* b_mont, size_t n, uint64_t* out_mont) {
  if (n && !b_mont) return AMSM_E_INVALID_ARG;
  return amsm_fr_add_impl(curve, a_mont, b_mont, n, out_mont);
}
int amsm_fr_sub(int curve, const uint64_t* a_mont, const uint64_t* b_mont, size_t n, uint64_t* out_mont) {
  if (n && !b_mont) return AMSM_E_INVALID_ARG;
  return amsm_fr_sub_impl(curve, a_mont, b_mont, n, out_mont);
}
int amsm_fr_inv(int curve, const uint64_t* a_mont, size_t n, uint64_t* out_mont) {
  return amsm_fr_inv_impl(curve, a_mont, nullptr, n, out_mont);
}
int amsm_fr_to_mont(int curve, const uint64_t* canonical, size_t n, uint64_t* out_mont) {
  return amsm_fr_to_mont_impl(curve, canonical, nullptr, n, out_mont);
}
int amsm_fr_from_mont(int curve, const uint64_t* a_mont, size_t n, uint64_t* out_canonical) {
  return amsm_fr_from_mont_impl(curve, a_mont, nullptr, n, out_canonical);
}

// ---- wire format (host_serialize.h) ------------------------------------------------------------------------------
size_t amsm_fr_serialized_size(int curve) {
  return with_curve_or(curve, (size_t)0, [](auto cv) {
    AMSM_CURVE_FIELDS(cv);
    return host::h_serialized_size<Fr>(0);
  });
}
size_t amsm_point_serialized_size(int curve, int compressed) {
  return with_curve_or(curve, (size_t)0, [&](auto cv) {
    AMSM_CURVE_FIELDS(cv);
    return host::point_serialized_size<Fq>(compressed != 0);
  });
}
int amsm_fr_serialize(int curve, const uint64_t* a_mont, size_t n, uint8_t* out) {
  if (!curve_known(curve) || (n && (!a_mont || !out))) return AMSM_E_INVALID_ARG;
  return with_curve(curve, [&](auto cv) {
    AMSM_CURVE_FIELDS(cv);
    for (size_t i = 0; i < n; i++) {
      host::HFe<Fr> x;
      memcpy(x.v, a_mont + 4 * i, 32);
      host::h_write_le<Fr>(x, out + 32 * i, 32);
    }
    return AMSM_OK;
  });
}
int amsm_fr_deserialize(int curve, const uint8_t* in, size_t n, uint64_t* out_mont) {
  if (!curve_known(curve) || (n && (!in || !out_mont))) return AMSM_E_INVALID_ARG;
  return with_curve(curve, [&](auto cv) {
    AMSM_CURVE_FIELDS(cv);
    for (size_t i = 0; i < n; i++) {
      host::HFe<Fr> x;
      const bool ok = host::h_read_le<Fr>(in + 32 * i, 32, &x);
      memcpy(out_mont + 4 * i, x.v, 32);
      if (!ok) return AMSM_E_INVALID_ARG;
    }
    return AMSM_OK;
  });
}
int amsm_points_serialize(int curve, const uint64_t* xy_mont, const uint8_t* is_inf, size_t n, int compressed, uint8_t* out) {
  if (!curve_known(curve) || (n && (!xy_mont || !out))) return AMSM_E_INVALID_ARG;
  const size_t sz = amsm_point_serialized_size(curve, compressed);
  return with_curve(curve, [&](auto cv) {
    AMSM_CURVE_FIELDS(cv);
    for (size_t i = 0; i < n; i++) {
      const bool inf = is_inf && is_inf[i];
      host::point_serialize<Fq>(xy_mont + i * Fq::W, inf, compressed != 0, out + i * sz);
    }
    return AMSM_OK;
  });
}
int amsm_points_deserialize(int curve, const uint8_t* in, size_t n, int compressed, uint64_t* xy_mont, uint8_t* is_inf) {
  if (!curve_known(curve) || (n && (!in || !xy_mont || !is_inf))) return AMSM_E_INVALID_ARG;
  const size_t sz = amsm_point_serialized_size(curve, compressed);
  return with_curve(curve, [&](auto cv) {
    AMSM_CURVE_FIELDS(cv);
    using C = decltype(cv);
    u64 r[4];  // the subgroup order, for the curves whose points need the check (cofactor != 1)
    for (int k = 0; k < 4; k++) r[k] = host::hmod<Fr>(k);
    for (size_t i = 0; i < n; i++) {
      const bool ok = host::point_deserialize<Fq>(in + i * sz, compressed != 0, C::b, C::subgroup_check,
                                                  C::subgroup_check ? r : nullptr, xy_mont + i * Fq::W, is_inf + i);
      if (!ok) return AMSM_E_INVALID_ARG;
    }
    return AMSM_OK;
  });
}

// ---- Poseidon sponge (host_poseidon.h) ---------------------------------------------------------------------------------
// runs the statement with `sp` = the sponge state of s's curve (a sponge's curve is known: amsm_poseidon_new checks it)
#define SPONGE_DO(s, ...)                                 \
  (void)with_curve((s)->curve, [&](auto cv_) {            \
    using FQ = typename decltype(cv_)::Fq;                \
    auto& sp = (s)->of<FQ>();                             \
    __VA_ARGS__;                                          \
    return AMSM_OK;                                       \
  })
int amsm_poseidon_new(int curve, amsm_sponge** out) {
  if (!out || !curve_known(curve)) return AMSM_E_INVALID_ARG;
  amsm_sponge* s = new (std::nothrow) amsm_sponge();
  if (!s) return AMSM_E_OOM;
  s->curve = curve;
  *out = s;
  return AMSM_OK;
}
int amsm_poseidon_clone(const amsm_sponge* s, amsm_sponge** out) {
  if (!s || !out) return AMSM_E_INVALID_ARG;
  amsm_sponge* c = new (std::nothrow) amsm_sponge(*s);
  if (!c) return AMSM_E_OOM;
  *out = c;
  return AMSM_OK;
}
void amsm_poseidon_free(amsm_sponge* s) { delete s; }
int amsm_poseidon_absorb_native(amsm_sponge* s, const uint64_t* fq_mont, size_t n) {
  if (!s || (n && !fq_mont)) return AMSM_E_INVALID_ARG;
  SPONGE_DO(s, sp.absorb_words(fq_mont, n));
  return AMSM_OK;
}
int amsm_poseidon_absorb_u64(amsm_sponge* s, uint64_t v) {
  if (!s) return AMSM_E_INVALID_ARG;
  SPONGE_DO(s, sp.absorb_u64(v));
  return AMSM_OK;
}
int amsm_poseidon_absorb_bytes(amsm_sponge* s, const uint8_t* b, size_t n) {
  if (!s || (n && !b)) return AMSM_E_INVALID_ARG;
  SPONGE_DO(s, sp.absorb_bytes(b, n));
  return AMSM_OK;
}
int amsm_poseidon_absorb_points(amsm_sponge* s, const uint64_t* xy_mont, const uint8_t* is_inf, size_t n) {
  if (!s || (n && !xy_mont)) return AMSM_E_INVALID_ARG;
  SPONGE_DO(s, sp.absorb_points(xy_mont, is_inf, n));
  return AMSM_OK;
}
int amsm_poseidon_fork(const amsm_sponge* s, const uint8_t* domain, size_t n, amsm_sponge** out) {
  if (!s || !out || (n && !domain)) return AMSM_E_INVALID_ARG;
  TRY(amsm_poseidon_clone(s, out));
  std::vector<uint8_t> input(8 + n);  // `domain.len()` as u64 little-endian, then the domain
  for (int i = 0; i < 8; i++) input[i] = (uint8_t)((uint64_t)n >> (8 * i));
  if (n) memcpy(input.data() + 8, domain, n);
  return amsm_poseidon_absorb_bytes(*out, input.data(), input.size());
}
int amsm_poseidon_squeeze_native(amsm_sponge* s, size_t n, uint64_t* out_fq_mont) {
  if (!s || (n && !out_fq_mont)) return AMSM_E_INVALID_ARG;
  SPONGE_DO(s, sp.squeeze_words(n, out_fq_mont));
  return AMSM_OK;
}
int amsm_poseidon_squeeze_bits(amsm_sponge* s, size_t n_bits, uint8_t* out_bytes) {
  if (!s || (n_bits && !out_bytes)) return AMSM_E_INVALID_ARG;
  std::vector<uint8_t> b;
  SPONGE_DO(s, b = sp.squeeze_bits(n_bits));
  if (!b.empty()) memcpy(out_bytes, b.data(), b.size());
  return AMSM_OK;
}
int amsm_poseidon_squeeze_nonnative(amsm_sponge* s, unsigned n_bits, size_t count, uint64_t* out_canonical) {
  if (!s || (count && !out_canonical) || n_bits == 0 || n_bits > 254) return AMSM_E_INVALID_ARG;
  std::vector<uint8_t> b;
  const size_t total = (size_t)n_bits * count;
  SPONGE_DO(s, b = sp.squeeze_bits(total));
  memset(out_canonical, 0, count * 32);
  for (size_t k = 0; k < count; k++)
    for (unsigned i = 0; i < n_bits; i++) {
      const size_t bit = k * n_bits + i;
      if ((b[bit >> 3] >> (bit & 7)) & 1) out_canonical[4 * k + (i >> 6)] |= 1ull << (i & 63);
    }
  return AMSM_OK;
}
int amsm_poseidon_permute(int curve, uint64_t* state_mont) {
  if (!state_mont || !curve_known(curve)) return AMSM_E_INVALID_ARG;
  amsm_sponge s;
  s.curve = curve;
  SPONGE_DO(&s, {
    constexpr int N = host::HFe<FQ>::N;
    for (int i = 0; i < 3; i++) memcpy(sp.state[i].v, state_mont + i * N, 8 * N);
    sp.permute();
    for (int i = 0; i < 3; i++) memcpy(state_mont + i * N, sp.state[i].v, 8 * N);
  });
  return AMSM_OK;
}
int amsm_poseidon_round_constants(int curve, uint64_t* out_mont) {  // (8 + 31) * 3 elements, round-major
  if (!out_mont) return AMSM_E_INVALID_ARG;
  return with_curve(curve, [&](auto cv) {
    AMSM_CURVE_FIELDS(cv);
    constexpr int N = host::HFe<Fq>::N;
    const auto& p = host::PoseidonParams<Fq>::get();
    for (int r = 0; r < 39; r++)
      for (int i = 0; i < 3; i++) memcpy(out_mont + (r * 3 + i) * N, p.ark[r][i].v, 8 * N);
    return AMSM_OK;
  });
}

// ---- page-locked caller memory (include/amsm.h: amsm_host_register) ----
// Round 5: both are documented NO-OPS.  Measured on five MI355X boxes (profiles/r05_host_slices.md): hipMemcpyAsync moves a 32 MiB
// scalar vector at 55-56 GB/s from pageable, registered and hipHostMalloc'ed memory alike (and so does a copy kernel reading the
// page-locked pages: it is the link), so registration can win nothing -- and it LOST: the first copy out of every freshly registered
// region stalls the calling thread for ~2 ms (lazy pinning: 8.7 ms for the four vectors of a batch, rocprofv3 timeline), on some
// boxes every copy does (batches of twelve 2^20-scalar slices 1.70 against 1.37 ms per MSM; the driver's round-4 box: -27 %).
int amsm_host_register(void* ptr, size_t bytes) { return (!ptr || !bytes) ? AMSM_E_INVALID_ARG : AMSM_OK; }
int amsm_host_unregister(void* ptr) { return ptr ? AMSM_OK : AMSM_E_INVALID_ARG; }
int amsm_host_is_pinned(const void* ptr) { return host_ptr_pinned(ptr) ? 1 : 0; }

