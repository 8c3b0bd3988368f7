// Part of api.hip (inside its anonymous namespace): committer keys (load / generate / read / precompute), affine output,
// host-scalar MSMs and Pedersen commitments.
// batch_normalization_into_affine (src/hp_as/mod.rs:468): one inversion for the whole batch
template <class Fq>
void write_affine_batch(const std::vector<host::HXYZZ<Fq>>& pts, uint64_t* out_xy, uint8_t* out_is_inf) {
  using H = host::HFe<Fq>;
  constexpr int N = H::N;
  size_t k = pts.size();
  std::vector<H> z(k), pre(k);
  H run = host::h_one<Fq>();
  for (size_t i = 0; i < k; i++) {
    bool inf = host::hx_is_inf<Fq>(pts[i]);
    z[i] = inf ? host::h_one<Fq>() : host::h_mul<Fq>(pts[i].zz, pts[i].zzz);
    pre[i] = run;
    run = host::h_mul<Fq>(run, z[i]);
  }
  H inv = host::h_inv<Fq>(run);
  for (size_t i = k; i-- > 0;) {
    H zi = host::h_mul<Fq>(inv, pre[i]);  // 1 / (zz*zzz)
    inv = host::h_mul<Fq>(inv, z[i]);
    uint64_t* o = out_xy + i * 2 * N;
    if (host::hx_is_inf<Fq>(pts[i])) {
      memset(o, 0, 16 * N);
      if (out_is_inf) out_is_inf[i] = 1;
      continue;
    }
    H x = host::h_mul<Fq>(pts[i].x, host::h_mul<Fq>(zi, pts[i].zzz));
    H y = host::h_mul<Fq>(pts[i].y, host::h_mul<Fq>(zi, pts[i].zz));
    memcpy(o, x.v, 8 * N);
    memcpy(o + N, y.v, 8 * N);
    if (out_is_inf) out_is_inf[i] = 0;
  }
}

// Build the W = windows_for(c) table levels of a key on the device: table[w][i] = 2^(c w) G_i.  b->d_table holds the n
// generators (device radix) and is replaced by the table.
// n_narrow > 0 (round 4): the top n_narrow windows are c - 1 bits wide and their levels stand one doubling short of their
// position (MsmGeom::n_narrow, msm_types.h: window_exponent_of)
template <class Fq>
int bases_precompute(amsm_ctx* ctx, amsm_bases* b, int c, bool requested, int top_shift = 0, int n_narrow = 0) {
  int W = windows_for(c);
  if (n_narrow < 0 || n_narrow >= W) return AMSM_E_INVALID_ARG;
  if ((unsigned long long)b->n * W >= (1ull << 30))  // entry words carry a 30-bit table index
    return requested ? AMSM_E_UNSUPPORTED : AMSM_OK;
  u32* table = nullptr;
  if (gate_alloc(ctx, GATE_DEVICE, (size_t)b->n * W * affine_bytes<Fq>(), !requested, (void**)&table) != AMSM_OK)
    return requested ? AMSM_E_OOM : AMSM_OK;  // not enough HBM for W copies
  // (from here on the table is this function's: every way out without it gives it back)
  auto fail = [&](hipError_t e) {
    fprintf(stderr, "[amsm] HIP error %s (%d) in bases_precompute\n", hipGetErrorName(e), (int)e);
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipGetLastError();
    (void)gate_free(table);
    return e == hipErrorOutOfMemory ? AMSM_E_OOM : AMSM_E_HIP;
  };
  if (hipError_t e = hipMemcpyAsync(table, b->d_table, b->n * affine_bytes<Fq>(), hipMemcpyDeviceToDevice, ctx->stream)) return fail(e);
  u32* scratch = nullptr;
  // small keys with plain power-of-two levels (round 4): every level in ONE pass and one batched conversion (2^12 generators:
  // 31 launches of 150 us -> 2 launches)
  const bool all_at_once = !batch_affine_pays<Fq>((u32)b->n) && !n_narrow && !top_shift && W >= 2 &&
                           try_ensure(ctx->xyzz_scratch, (size_t)(W - 1) * b->n * xyzz_bytes<Fq>());
  if (all_at_once) launch_precompute_all_levels<Fq>(ctx->stream, table, (u32)b->n, (u32)c, (u32)W, (u32*)ctx->xyzz_scratch.p);
  if (!all_at_once && batch_affine_pays<Fq>((u32)b->n) && try_ensure(ctx->xyzz_scratch, b->n * xyzz_bytes<Fq>()))
    scratch = (u32*)ctx->xyzz_scratch.p;
  for (int w = 1; w < W && !all_at_once; w++) {
    // level w = 2^(e_w) G: e_w - e_(w-1) doublings of the level below (c between equal windows; the top level of a round-3
    // bucket-per-lane key is 2^top_shift short of its place, MsmGeom::top_shift)
    const u32 dbl = window_exponent_of((u32)c, (u32)W, (u32)n_narrow, (u32)top_shift, (u32)w) -
                    window_exponent_of((u32)c, (u32)W, (u32)n_narrow, (u32)top_shift, (u32)w - 1u);
    launch_precompute_level<Fq>(ctx->stream, table, (u32)b->n, (u32)w, dbl, scratch);
  }
  if (hipError_t e = hipStreamSynchronize(ctx->stream)) return fail(e);
  if (hipError_t e = hipGetLastError()) return fail(e);
  if (scratch || (all_at_once && ctx->xyzz_scratch.bytes > ((size_t)256 << 20)))  // a key-sized buffer: not worth keeping between the rare key loads
    ctx->xyzz_scratch.release();
  (void)gate_free(b->d_table);
  b->d_table = table;
  b->precomp = 1;
  b->c = c;
  b->W = W;
  b->top_shift = top_shift;
  b->n_narrow = n_narrow;
  return AMSM_OK;
}

// The direct-sum table of a small precomputed key (amsm_bases::d_small; msm_kernels.h k_direct_sum): 512 affine points per
// generator, built from the window table -- at most c - 1 doublings from the level below each 4-bit position, 7 additions per level
// point, ONE batched inversion pass.  Not being able to hold it (memory) is not an error: the key works without.
// OPTIONAL: the caller's flags (AMSM_BASES_NO_DIRECT_TABLE), the context's byte budget (amsm_ctx_set_table_budget) or a failed
// allocation deny it -- the key then works on the windowed pipelines, 2-4x slower at these sizes, and SAYS so (amsm_bases_tables,
// amsm_ctx_tables_denied): round 5, VERDICT r4 item 7.
enum TableDenied { DENIED_NO = 0, DENIED_BY_FLAG = 1, DENIED_BY_BUDGET = 2, DENIED_BY_OOM = 3 };
template <class Fq>
int bases_direct_table(amsm_ctx* ctx, amsm_bases* b, unsigned flags) {
  if (!b->precomp || ctx->direct_max_log2 <= 0 || b->n == 0 || b->n > ((size_t)1 << ctx->direct_max_log2)) return AMSM_OK;
  if (b->n_narrow || b->top_shift || b->c < 4) return AMSM_OK;  // (the levels are read as plain c-bit windows)
  const size_t pts = b->n * (size_t)(DS_W * DS_MULT);
  auto deny = [&](int why) {
    b->direct_denied = why;
    if (why != DENIED_BY_FLAG) ctx->n_tables_denied++;
    return AMSM_OK;
  };
  if (flags & AMSM_BASES_NO_DIRECT_TABLE) return deny(DENIED_BY_FLAG);
  if (pts * affine_bytes<Fq>() > ctx->table_budget) return deny(DENIED_BY_BUDGET);
  u32* t = nullptr;
  if (gate_alloc(ctx, GATE_DEVICE, pts * affine_bytes<Fq>(), true, (void**)&t) != AMSM_OK) return deny(DENIED_BY_OOM);
  // slabs of the 64 four-bit windows so that the XYZZ scratch stays at or below 256 MiB (the whole table at once needed 2-3 GiB for a
  // 2^15-generator key)
  u32 slab = DS_W;
  while (slab > 1u && (size_t)DS_MULT * slab * b->n * xyzz_bytes<Fq>() > ((size_t)256 << 20)) slab >>= 1;
  if (!try_ensure(ctx->xyzz_scratch, (size_t)DS_MULT * slab * b->n * xyzz_bytes<Fq>())) {
    (void)gate_free(t);
    return deny(DENIED_BY_OOM);
  }
  launch_ds_table<Fq>(ctx->stream, b->d_table, (u32)b->n, (u32)b->c, (u32)b->W, (u32*)ctx->xyzz_scratch.p, slab, t);
  hipError_t e = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess) e = hipGetLastError();
  if (e != hipSuccess) {  // (the table is not the key's yet: give it back)
    (void)hipGetLastError();
    (void)gate_free(t);
    return AMSM_E_HIP;
  }
  b->d_small = t;
  return AMSM_OK;
}

// MsmGeom::top_shift of a walk over the scalar field Fr (msm_types.h: top_window_shift_of has the arithmetic).  Round 3's 20-bit keys:
// Pallas 5 (digits at every 32nd bucket), BLS12-381 4; round 4's (widths adding up to 256 bits): Pallas 1, BLS12-381 0.
// Non-canonical scalars whose shifted digit would leave the bucket range are reported as AMSM_E_SCALAR_RANGE by the digit walk.
template <class Fr>
int top_window_shift(int c, int W, int n_narrow = 0, unsigned long long* raw_max_out = nullptr) {
  u32 mod[8];
  for (int i = 0; i < 8; i++) mod[i] = Fr::mod(i);
  return top_window_shift_of(mod, c, W, n_narrow, raw_max_out);
}

template <class Fq, class Fr>
int bases_finish(amsm_ctx* ctx, amsm_bases* b, unsigned flags) {
  // decide precomputation, then build the table levels on device
  bool pre;
  if (flags & AMSM_BASES_PRECOMPUTE) pre = true;
  else if (flags & AMSM_BASES_NO_PRECOMPUTE) pre = false;
  else pre = b->n >= (ctx->direct_max_log2 > 0 ? 1u : 256u);  // (round 4: small keys carry the direct-sum table -- worth it at any size)
  if (!pre) return AMSM_OK;
  // An EXPLICIT request (AMSM_BASES_PRECOMPUTE) that cannot be honoured is an error, not a silent 10x slower key; the
  // library's own choice (AMSM_BASES_DEFAULT) degrades to the plain key.
  const bool requested = (flags & AMSM_BASES_PRECOMPUTE) != 0;
  // the table's window width by the key's size (msm_select.h: table 1).  Keys of 2^20 generators and more: 13 windows whose widths
  // add up to EXACTLY 256 bits -- nine of 20 and, at the top, four of 19 (MsmGeom::n_narrow) -- the bucket-per-lane pipeline's table
  const int c = ctx->window_override ? ctx->window_override : msel::key_window(b->n, true, ctx->bpl);
  const bool bpl = c == BPL_WINDOW && ctx->bpl && !ctx->window_override;
  int n_narrow = 0, top_shift = 0;
  if (bpl) {
    n_narrow = (int)narrow_windows_for((u32)c);  // 4 of 13
    top_shift = top_window_shift<Fr>(c, windows_for(c), n_narrow);
  }
  TRY(bases_precompute<Fq>(ctx, b, c, requested, top_shift, n_narrow));
  b->bpl = (b->precomp && bpl) ? 1 : 0;
  b->no_twin = (flags & AMSM_BASES_NO_TWIN) != 0;
  return bases_direct_table<Fq>(ctx, b, flags);
}

// The 17-bit-window twin of a bucket-per-lane key (amsm_bases::alt), built on first use on the calling context's stream.
template <class Fq>
int bases_alt(amsm_ctx* ctx, const amsm_bases* b, const amsm_bases** out) {
  std::lock_guard<std::mutex> lk(b->alt_mu);
  if (!b->alt) {
    // OPTIONAL like the direct-sum table: a key created with AMSM_BASES_NO_TWIN, or whose twin does not fit the context's table
    // budget, refuses the MSMs that would need it (ranges below a quarter of the window, skewed vectors) instead of allocating
    // a second table behind the caller's back
    const size_t twin_bytes = b->n * (size_t)windows_for(msel::key_window(b->n, true, false)) * affine_bytes<Fq>();
    if (b->no_twin || twin_bytes > ctx->table_budget) {
      if (!b->twin_denied) ctx->n_tables_denied++;
      b->twin_denied = b->no_twin ? DENIED_BY_FLAG : DENIED_BY_BUDGET;
      return AMSM_E_UNSUPPORTED;
    }
    amsm_bases* a = new (std::nothrow) amsm_bases();
    if (!a) return AMSM_E_OOM;
    a->curve = b->curve;
    a->device = b->device;
    a->n = b->n;
    if (gate_alloc(ctx, GATE_DEVICE, std::max<size_t>(b->n, 1) * affine_bytes<Fq>(), false, (void**)&a->d_table) != AMSM_OK) {
      delete a;
      return AMSM_E_OOM;
    }
    int rc = AMSM_OK;
    if (b->ready && hipStreamWaitEvent(ctx->stream, b->ready, 0) != hipSuccess) rc = AMSM_E_HIP;
    if (rc == AMSM_OK && hipMemcpyAsync(a->d_table, b->d_table, b->n * affine_bytes<Fq>(), hipMemcpyDeviceToDevice,
                                        ctx->stream) != hipSuccess)
      rc = AMSM_E_HIP;
    if (rc == AMSM_OK)
      rc = bases_precompute<Fq>(ctx, a, msel::key_window(b->n, true, false), true);
    if (rc != AMSM_OK) {
      (void)hipStreamSynchronize(ctx->stream);  // (the copy into the table may still run)
      (void)gate_free(a->d_table);
      delete a;
      return rc;
    }
    b->alt = a;
  }
  *out = b->alt;
  return AMSM_OK;
}

// ---- point validation (include/amsm.h: amsm_points_check; points_check_kernels.h) -------------------------------------------------
// One run of the kernels over n < 2^32 device points (C-ABI radix; d_inf: their infinity bytes or null): every status byte written,
// cnt = the three counts and the smallest bad index (0xffffffff: none).  Ends in a synchronise.
template <class Fq>
int points_check_run(amsm_ctx* ctx, const u32* d_xy, const uint8_t* d_inf, size_t n, uint8_t* d_status, u32* d_counters,
                     u32 cnt[PCHK_WORDS]) {
  hipStream_t st = ctx->stream;
  HIP_TRY(hipMemsetAsync(d_counters, 0, 4 * PCHK_FIRST_BAD, st));
  HIP_TRY(hipMemsetAsync(d_counters + PCHK_FIRST_BAD, 0xff, 4, st));
  launch_points_check<Fq>(st, d_xy, d_inf, (u32)n, d_status, d_counters, host::points_check_consts<Fq>(), ctx->subgroup_ladder);
  HIP_TRY(hipMemcpyAsync(cnt, d_counters, 4 * PCHK_WORDS, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  return AMSM_OK;
}
constexpr size_t PCHK_HEAD = 256;  // the counters' place in front of a check's working memory
inline void points_check_add(uint64_t report[4], const u32 cnt[PCHK_WORDS], size_t off) {
  for (int k = 0; k < 3; k++) report[k] += cnt[k];
  if (cnt[PCHK_FIRST_BAD] != 0xffffffffu) report[3] = std::min<uint64_t>(report[3], off + cnt[PCHK_FIRST_BAD]);
}
// amsm_points_check_device: working memory (the counters, and the status bytes when the caller wants none) in ctx->check_ws
template <class Fq>
int points_check_device_impl(amsm_ctx* ctx, const void* d_xy, size_t n, uint64_t report[4], uint8_t* d_status) {
  report[0] = report[1] = report[2] = 0;
  report[3] = n;
  if (!n) return AMSM_OK;
  TRY(ensure(ctx->check_ws, PCHK_HEAD + (d_status ? 0 : n)));
  u32 cnt[PCHK_WORDS];
  TRY((points_check_run<Fq>(ctx, (const u32*)d_xy, nullptr, n, d_status ? d_status : (uint8_t*)ctx->check_ws.p + PCHK_HEAD,
                            (u32*)ctx->check_ws.p, cnt)));
  points_check_add(report, cnt, 0);
  return AMSM_OK;
}
// amsm_points_check: host slices in pieces of 2^18 points (24 MiB of BLS12-381 points: past the size where an upload runs at the
// link's rate, a quarter of the 2^20 bound of include/amsm.h) through ctx->check_ws (counters | status | flags | points)
template <class Fq>
int points_check_host_impl(amsm_ctx* ctx, const uint64_t* xy, const uint8_t* is_inf, size_t n, uint64_t report[4], uint8_t* status) {
  constexpr size_t PIECE = (size_t)1 << 18;
  report[0] = report[1] = report[2] = 0;
  report[3] = n;
  if (!n) return AMSM_OK;
  const size_t piece = std::min(n, PIECE), bytes_pt = affine_bytes<Fq>();
  const size_t flags_at = PCHK_HEAD + ((piece + 255) & ~(size_t)255), pts_at = flags_at + ((piece + 255) & ~(size_t)255);
  TRY(ensure(ctx->check_ws, pts_at + piece * bytes_pt));
  char* ws = (char*)ctx->check_ws.p;
  for (size_t off = 0; off < n; off += piece) {
    const size_t cnt_pts = std::min(piece, n - off);
    HIP_TRY(hipMemcpyAsync(ws + pts_at, (const char*)xy + off * bytes_pt, cnt_pts * bytes_pt, hipMemcpyHostToDevice, ctx->stream));
    if (is_inf) HIP_TRY(hipMemcpyAsync(ws + flags_at, is_inf + off, cnt_pts, hipMemcpyHostToDevice, ctx->stream));
    u32 cnt[PCHK_WORDS];
    TRY((points_check_run<Fq>(ctx, (const u32*)(ws + pts_at), is_inf ? (const uint8_t*)(ws + flags_at) : nullptr, cnt_pts,
                              (uint8_t*)ws + PCHK_HEAD, (u32*)ws, cnt)));
    if (status) {
      HIP_TRY(hipMemcpyAsync(status + off, ws + PCHK_HEAD, cnt_pts, hipMemcpyDeviceToHost, ctx->stream));
      HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    points_check_add(report, cnt, off);
  }
  return AMSM_OK;
}
// AMSM_BASES_CHECK: the points a key is about to be made of, where they lie on the device before the import.  Working memory of its
// own, freed on return (a refused key leaves the context as it found it).  AMSM_E_INVALID_POINT when one is bad.
template <class Fq>
int points_check_for_key(amsm_ctx* ctx, const u32* d_xy, const uint8_t* d_inf, size_t n) {
  if (!n) return AMSM_OK;
  char* tmp = nullptr;
  TRY(gate_alloc(ctx, GATE_DEVICE, PCHK_HEAD + n, false, (void**)&tmp));
  u32 cnt[PCHK_WORDS] = {0, 0, 0, 0};
  int s = points_check_run<Fq>(ctx, d_xy, d_inf, n, (uint8_t*)tmp + PCHK_HEAD, (u32*)tmp, cnt);
  if (s != AMSM_OK) (void)hipStreamSynchronize(ctx->stream);
  (void)gate_free(tmp);
  if (s == AMSM_OK && (cnt[0] | cnt[1] | cnt[2])) s = AMSM_E_INVALID_POINT;
  return s;
}

// A key that did not come to be: every table it got so far (the window table, a direct-sum table built before a later step failed)
inline void bases_discard(amsm_bases* b) {
  (void)gate_free(b->d_table);
  (void)gate_free(b->d_small);
  delete b;
}

template <class Fq, class Fr>
int bases_load_impl(amsm_ctx* ctx, const uint64_t* xy, const uint8_t* is_inf, size_t n, unsigned flags,
                    amsm_bases** out) {
  amsm_bases* b = new (std::nothrow) amsm_bases();
  if (!b) return AMSM_E_OOM;
  b->curve = ctx->curve;
  b->device = ctx->device;
  b->n = n;
  size_t bytes = std::max<size_t>(n, 1) * affine_bytes<Fq>();
  if (gate_alloc(ctx, GATE_DEVICE, bytes, false, (void**)&b->d_table) != AMSM_OK) {
    delete b;
    return AMSM_E_OOM;
  }
  int s = AMSM_OK;
  do {
    if (n) {
      if (hipMemcpyAsync(b->d_table, xy, n * affine_bytes<Fq>(), hipMemcpyHostToDevice, ctx->stream) != hipSuccess) {
        s = AMSM_E_HIP;
        break;
      }
      if (is_inf) {
        s = ensure(ctx->scalars, n);
        if (s) break;
        if (hipMemcpyAsync(ctx->scalars.p, is_inf, n, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) {
          s = AMSM_E_HIP;
          break;
        }
      }
      if (flags & AMSM_BASES_CHECK) {
        s = points_check_for_key<Fq>(ctx, b->d_table, is_inf ? (const uint8_t*)ctx->scalars.p : nullptr, n);
        if (s) break;
      }
      if (is_inf) launch_apply_inf<Fq>(ctx->stream, b->d_table, (const uint8_t*)ctx->scalars.p, (u32)n);
      launch_points_import<Fq>(ctx->stream, b->d_table, b->d_table, (u32)n);  // C-ABI radix -> device radix
      if (hipStreamSynchronize(ctx->stream) != hipSuccess) {
        s = AMSM_E_HIP;
        break;
      }
      s = bases_finish<Fq, Fr>(ctx, b, flags);
    }
  } while (0);
  if (s != AMSM_OK) {
    (void)hipStreamSynchronize(ctx->stream);  // (the upload into the table may still run)
    (void)hipGetLastError();
    bases_discard(b);
    return s;
  }
  *out = b;
  return AMSM_OK;
}

template <class Fq, class Fr>
int bases_generate_impl(amsm_ctx* ctx, uint64_t seed, size_t n, unsigned flags, amsm_bases** out, size_t first = 0) {
  amsm_bases* b = new (std::nothrow) amsm_bases();
  if (!b) return AMSM_E_OOM;
  b->curve = ctx->curve;
  b->device = ctx->device;
  b->n = n;
  if (gate_alloc(ctx, GATE_DEVICE, std::max<size_t>(n, 1) * affine_bytes<Fq>(), false, (void**)&b->d_table) != AMSM_OK) {
    delete b;
    return AMSM_E_OOM;
  }
  int s = AMSM_OK;
  if (n) {
    std::vector<u32> gen = generator_mont<Fq>();
    launch_generate_bases<Fq>(ctx->stream, b->d_table, seed, (u32)first, (u32)n, gen.data());
    if (hipStreamSynchronize(ctx->stream) != hipSuccess || hipGetLastError() != hipSuccess) s = AMSM_E_HIP;
    if (s == AMSM_OK) s = bases_finish<Fq, Fr>(ctx, b, flags);
  }
  if (s != AMSM_OK) {
    bases_discard(b);
    return s;
  }
  *out = b;
  return AMSM_OK;
}

// Transparent key: table[t] = G_(first + t) of the derivation "amsm-sample-v1" (include/amsm.h: amsm_bases_sample), sampled on the
// device (sample_kernels.h).  Search passes over the shrinking list of unsolved indices, one square test per index and pass,
// while the list is long; the last few thousand loop per lane; then one finishing pass over every index.  Working memory: 20 bytes
// per generator (two lists and the winning attempts), freed on return.
template <class Fq, class Fr>
int bases_sample_impl(amsm_ctx* ctx, const uint8_t* domain, size_t domain_len, uint64_t first, size_t n, unsigned flags,
                      amsm_bases** out) {
  constexpr u32 TAIL = 4096;    // a list this short is finished by one launch whose lanes loop
  constexpr int MAX_PASSES = 24;  // (the list halves per pass: 2^31 indices are down to TAIL after 19)
  amsm_bases* b = new (std::nothrow) amsm_bases();
  if (!b) return AMSM_E_OOM;
  b->curve = ctx->curve;
  b->device = ctx->device;
  b->n = n;
  u32* jwin = nullptr;
  u64* pend[2] = {nullptr, nullptr};
  u32* counters = nullptr;
  auto release = [&](int rc) {
    if (rc != AMSM_OK) (void)hipStreamSynchronize(ctx->stream);  // (a search pass may still write the lists)
    (void)gate_free(jwin);
    (void)gate_free(pend[0]);
    (void)gate_free(pend[1]);
    (void)gate_free(counters);
    if (rc != AMSM_OK) bases_discard(b);
    return rc;
  };
  if (gate_alloc(ctx, GATE_DEVICE, std::max<size_t>(n, 1) * affine_bytes<Fq>(), false, (void**)&b->d_table) != AMSM_OK)
    return release(AMSM_E_OOM);
  if (n) {
    if (gate_alloc(ctx, GATE_DEVICE, n * 4, false, (void**)&jwin) != AMSM_OK ||
        gate_alloc(ctx, GATE_DEVICE, n * 8, false, (void**)&pend[0]) != AMSM_OK ||
        gate_alloc(ctx, GATE_DEVICE, n * 8, false, (void**)&pend[1]) != AMSM_OK ||
        gate_alloc(ctx, GATE_DEVICE, SAMPLE_CNT_WORDS * 4, false, (void**)&counters) != AMSM_OK)
      return release(AMSM_E_OOM);
    const SampleConsts k = host::sample_consts<Fq>(domain, domain_len);
    hipStream_t st = ctx->stream;
    u32 cnt[SAMPLE_CNT_WORDS] = {0};
    auto read_counters = [&]() {
      return hipMemcpyAsync(cnt, counters, sizeof(cnt), hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess &&
             hipGetLastError() == hipSuccess;
    };
    if (hipMemsetAsync(counters, 0, SAMPLE_CNT_WORDS * 4, st) != hipSuccess) return release(AMSM_E_HIP);
    // pass 0 takes the indices themselves (no list); pass p reads list (p - 1) & 1 and writes list p & 1
    u32 pending = (u32)n;
    for (int pass = 0; pending; pass++) {
      const bool last = pass > 0 && (pending <= TAIL || pass >= MAX_PASSES);
      launch_sample_search<Fq>(st, b->d_table, jwin, pass ? pend[(pass - 1) & 1] : nullptr, pending, pend[pass & 1], counters, k, first,
                               last ? (u32)b2s::SAMPLE_MAX_ATTEMPTS : 1u);
      if (!read_counters()) return release(AMSM_E_HIP);
      if (cnt[SAMPLE_CNT_EXHAUSTED]) return release(AMSM_E_UNSUPPORTED);  // an index used up its 256 attempts: no key
      if (last && cnt[SAMPLE_CNT_PENDING]) return release(AMSM_E_HIP);    // (cannot happen: the looping pass leaves nothing)
      pending = cnt[SAMPLE_CNT_PENDING];
      if (hipMemsetAsync(counters + SAMPLE_CNT_PENDING, 0, 4, st) != hipSuccess) return release(AMSM_E_HIP);
    }
    launch_sample_finish<Fq>(st, b->d_table, jwin, (u32)n, counters, k, first);
    if (!read_counters()) return release(AMSM_E_HIP);
    if (cnt[SAMPLE_CNT_IDENTITY]) {
      // a candidate whose cofactor multiple is the identity (one in 2^250 or so) is a rejection the finishing kernel cannot act on:
      // those indices are derived again on the host, past that attempt, and written into the table
      std::vector<u32> hj(n);
      if (hipMemcpy(hj.data(), jwin, n * 4, hipMemcpyDeviceToHost) != hipSuccess) return release(AMSM_E_HIP);
      std::vector<u64> xy(2 * host::HFe<Fq>::N);
      for (size_t t = 0; t < n; t++) {
        if (!(hj[t] & 0x80000000u)) continue;
        if (!host::sample_point<Fq>(k.prefix, first + t, (hj[t] & 0x7fffffffu) + 1u, xy.data(), nullptr)) return release(AMSM_E_UNSUPPORTED);
        u32* slot = b->d_table + t * (affine_bytes<Fq>() / 4);
        if (hipMemcpy(slot, xy.data(), affine_bytes<Fq>(), hipMemcpyHostToDevice) != hipSuccess) return release(AMSM_E_HIP);
        launch_points_import<Fq>(st, slot, slot, 1);
        if (hipStreamSynchronize(st) != hipSuccess) return release(AMSM_E_HIP);
      }
    }
    const int s = bases_finish<Fq, Fr>(ctx, b, flags);
    if (s != AMSM_OK) return release(s);
  }
  *out = b;
  return release(AMSM_OK);
}

template <class Fq>
int bases_read_impl(amsm_ctx* ctx, const amsm_bases* b, size_t off, size_t n, uint64_t* xy, uint8_t* is_inf) {
  if (off > b->n || n > b->n - off) return AMSM_E_INVALID_ARG;
  if (!n) return AMSM_OK;
  const char* src = (const char*)b->d_table + off * affine_bytes<Fq>();
  if (device_internal_radix<Fq>()) {  // back to the C-ABI radix through a scratch buffer
    TRY(ensure(ctx->scalars, n * affine_bytes<Fq>()));
    launch_points_export<Fq>(ctx->stream, (const u32*)src, (u32*)ctx->scalars.p, (u32)n);
    src = (const char*)ctx->scalars.p;
  }
  HIP_TRY(hipMemcpyAsync(xy, src, n * affine_bytes<Fq>(), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (is_inf) {
    constexpr int N = 2 * Fq::L / 2;
    for (size_t i = 0; i < n; i++) {
      u64 o = 0;
      for (int k = 0; k < N; k++) o |= xy[i * N + k];
      is_inf[i] = o == 0;
    }
  }
  return AMSM_OK;
}

template <class Fq>
void write_affine(const host::HXYZZ<Fq>& p, uint64_t* out_xy, uint8_t* out_is_inf) {
  uint8_t inf = 0;
  host::hx_to_affine<Fq>(p, out_xy, &inf);
  if (out_is_inf) *out_is_inf = inf;
}

template <class Fq, class Fr>
int msm_host_scalars(amsm_ctx* ctx, const amsm_bases* bases, size_t base_off, const uint64_t* scalars, size_t n,
                     int mont, host::HXYZZ<Fq>* out) {
  if (base_off > bases->n) return AMSM_E_INVALID_ARG;
  n = std::min(n, bases->n - base_off);
  if (n == 0) {
    *out = host::hx_inf<Fq>();
    return AMSM_OK;
  }
  if (host_halves_apply(ctx, bases, n)) {  // round 6: two halves over one bucket set, the second uploaded beside the first's MSM
    std::vector<host::HXYZZ<Fq>> r;
    TRY((msm_multi_host_xyzz<Fq, Fr>(ctx, bases, 1, &base_off, &scalars, &n, mont, &r)));
    *out = r[0];
    return AMSM_OK;
  }
  TRY(ensure(ctx->scalars, n * 32));
  HIP_TRY(hipMemcpyAsync(ctx->scalars.p, scalars, n * 32, hipMemcpyHostToDevice, ctx->stream));
  return msm_device_xyzz<Fq, Fr>(ctx, bases, base_off, ctx->scalars.p, n, mont, out);
}

template <class Fq, class Fr>
int pedersen_impl(amsm_ctx* ctx, const amsm_bases* ck, const uint64_t* elems, size_t n, const uint64_t* rand_mont,
                  const uint64_t* hiding_xy, uint64_t* out_xy, uint8_t* out_inf) {
  host::HXYZZ<Fq> acc;
  TRY((msm_host_scalars<Fq, Fr>(ctx, ck, 0, elems, n, 1, &acc)));
  if (rand_mont && hiding_xy) {
    host::HFe<Fr> r;
    memcpy(r.v, rand_mont, 32);
    r = host::h_from_mont<Fr>(r);
    host::HXYZZ<Fq> h = host::hx_from_affine<Fq>(hiding_xy, false);
    acc = host::hx_add<Fq>(acc, host::hx_mul<Fq>(h, r.v));
  }
  write_affine<Fq>(acc, out_xy, out_inf);
  return AMSM_OK;
}

template <class Fq, class Fr>
int pedersen_device_impl(amsm_ctx* ctx, const amsm_bases* ck, const void* d_elems, size_t n, const uint64_t* rand_mont,
                         const uint64_t* hiding_xy, uint64_t* out_xy, uint8_t* out_inf) {
  host::HXYZZ<Fq> acc;
  TRY((msm_device_xyzz<Fq, Fr>(ctx, ck, 0, d_elems, n, 1, &acc)));
  if (rand_mont && hiding_xy) {
    host::HFe<Fr> r;
    memcpy(r.v, rand_mont, 32);
    r = host::h_from_mont<Fr>(r);
    host::HXYZZ<Fq> h = host::hx_from_affine<Fq>(hiding_xy, false);
    acc = host::hx_add<Fq>(acc, host::hx_mul<Fq>(h, r.v));
  }
  write_affine<Fq>(acc, out_xy, out_inf);
  return AMSM_OK;
}

// host slices, uploads overlapped with the previous MSMs (api_pipeline.inc: msm_multi_host_xyzz)
template <class Fq, class Fr>
int msm_host_batch_impl(amsm_ctx* c, const amsm_bases* b, size_t off, const uint64_t* const* scalars, const size_t* ns,
                               size_t n_vecs, int mont, const uint64_t* const* rand_mont, const uint64_t* hiding_xy,
                               uint64_t* out_xy, uint8_t* out_inf) {
  std::vector<size_t> offs(n_vecs, off);
  std::vector<host::HXYZZ<Fq>> r;
  TRY((msm_multi_host_xyzz<Fq, Fr>(c, b, n_vecs, offs.data(), scalars, ns, mont, &r)));
  if (rand_mont && hiding_xy) {  // + r_v * hiding_generator (a11: host), the multiples side by side on the host pool
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

