// Scalar-field kernels (digit extraction, synthetic vectors, Hadamard / linear-combination / t-vector
// loops) instantiated for the scalar fields of every curve, plus the curve-independent bounds kernel.
// The launchers are ordinary function templates over the scalar field (launch.h declares them); the list at the end of the file
// instantiates each for every field.  The geometry they launch by is prep_geom.h's.
#include "launch.h"
#include "vec_kernels.h"
#include "prep_kernels.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace amsm {

void launch_bounds(hipStream_t st, const void* keys_sorted, bool keys16, u32* vals_sorted, MsmGeom g, u32* start,
                   u32* items) {
  if (keys16)
    hipLaunchKernelGGL((k_bounds<uint16_t>), dim3(cdiv(g.B, 256)), dim3(256), 0, st, (const uint16_t*)keys_sorted,
                       vals_sorted, g, start, items);
  else
    hipLaunchKernelGGL((k_bounds<u32>), dim3(cdiv(g.B, 256)), dim3(256), 0, st, (const u32*)keys_sorted, vals_sorted,
                       g, start, items);
}

__global__ void k_mirror_flags(const u32* __restrict__ flags, u32* __restrict__ host_mirror) {
  if (threadIdx.x < 2u) host_mirror[threadIdx.x] = flags[threadIdx.x];
}
void launch_mirror_flags(hipStream_t st, const u32* flags, u32* host_mirror) {
  hipLaunchKernelGGL(k_mirror_flags, dim3(1), dim3(64), 0, st, flags, host_mirror);
}
void launch_vec_fill(hipStream_t st, u32* out, const u32 v[8], u32 n) {
  hipLaunchKernelGGL(k_vec_fill, dim3(cdiv(n, 256)), dim3(256), 0, st, out, make_uint4(v[0], v[1], v[2], v[3]),
                     make_uint4(v[4], v[5], v[6], v[7]), n);
}

void launch_tv_probe(hipStream_t st, const u32* scalars, u32 n, u32* out16, const u32 one[8]) {
  static_assert(TV_PROBE_WORDS == TV_WORDS && TV_EXC_SLOTS == TV_EXC_MAX && TV_ONES_SAMPLE_COUNT == TV_ONES_SAMPLES,
                "launch.h mirrors vec_kernels.h");
  const u32 blocks = std::max(1u, std::min(512u, (n + 1023u) / 1024u));
  TvOne o;
  memcpy(o.w, one, 32);
  hipLaunchKernelGGL(k_tv_probe, dim3(blocks), dim3(256), 0, st, scalars, n, out16, o);
}

// ---- the prep chains (prep_kernels.h; sizes and layouts: prep_geom.h) ----
// more than 64 KiB of dynamic LDS needs the attribute, once per device (launch.h: DeviceOnce)
static void prep_local_attr() {
  static DeviceOnce once;
  once.run([] { (void)hipFuncSetAttribute((const void*)k_prep_local, hipFuncAttributeMaxDynamicSharedMemorySize, 152 * 1024); });
}
static void prep_bpl_attr() {
  static DeviceOnce once;
  static_assert((BPL_LOCAL_BUDGET_WORDS) * sizeof(u32) <= PREP_LDS_LIMIT, "k_prep_local_t's LDS must fit a workgroup");
  once.run([] { (void)hipFuncSetAttribute((const void*)k_prep_local_t, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PREP_LDS_LIMIT); });
}
static void prep_bps_attr() {
  static DeviceOnce once;
  static_assert(BPS_LOCAL_BUDGET_WORDS * sizeof(u32) <= 152 * 1024, "k_prep_local_s's LDS must fit its attribute");
  once.run([] {
    (void)hipFuncSetAttribute((const void*)k_prep_local_s, hipFuncAttributeMaxDynamicSharedMemorySize, 152 * 1024);
    (void)hipFuncSetAttribute((const void*)k_prep_local_s_batch, hipFuncAttributeMaxDynamicSharedMemorySize, 152 * 1024);
  });
}
// one fill: the flag words in front of d_small (err) and the arrays that must start at zero (PrepSmall::fill_bytes)
static int prep_fill(hipStream_t st, u32* err, u32* d_small, const PrepSmall& s) {
  if (err != d_small - PREP_FLAG_WORDS) return -1;
  return hipMemsetAsync(err, 0, s.fill_bytes, st) == hipSuccess ? 0 : -1;
}
// partition sizes and their exclusive scan.  The histogram's blocking is independent of the scatter's: 1024 scalars, one per lane
template <class FR>
static void launch_hist_scan(hipStream_t st, const u32* scalars, int mont, const MsmGeom& g, const PrepGeom& pg, const PrepSmall& s,
                             u32* err) {
  PrepGeom ph = pg;
  ph.SPB = 1024;
  hipLaunchKernelGGL((k_prep_hist<FR>), dim3(cdiv(g.n, 1024)), dim3(1024), pg.P * sizeof(u32), st, scalars, mont, g, ph, s.part_total,
                     err);
  hipLaunchKernelGGL(k_prep_scan, dim3(1), dim3(1024), 0, st, s.part_total, s.part_start, pg.P, pg.HEAVY, s.hv);
}
// k_prep_scatter with `lds` bytes of dynamic LDS: 16 entry slots per scalar and 512 scalars per workgroup up to S = 16, else 32 slots
// and 256 scalars (PrepGeom::SPB; plain keys with 18 / 19 windows).  The opt-in to more than 64 KiB is per instantiation, so it is not
// remembered per device: the narrow scatter needs it rarely (P above ~1300) and sets it whenever it does, the WIDE one on every launch.
template <class FR, bool WIDE>
static void launch_scatter(hipStream_t st, const u32* scalars, int mont, const MsmGeom& g, const PrepGeom& pg, size_t lds,
                           const PrepSmall& s, u32* part, u32* err) {
  auto launch = [&](auto kernel, u32 lanes) {
    if (WIDE || lds > 64 * 1024)
      (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PREP_LDS_LIMIT);
    hipLaunchKernelGGL(kernel, dim3(cdiv(g.n, pg.SPB)), dim3(lanes), lds, st, scalars, mont, g, pg, s.part_start, s.part_cursor, part,
                       err);
  };
  if (g.S <= 16u) launch(k_prep_scatter<FR, 16, 1, WIDE>, 512u);
  else launch(k_prep_scatter<FR, 32, 1, WIDE>, 256u);
}

template <class FR>
int launch_prep(hipStream_t st, const u32* scalars, int mont, MsmGeom g, const PrepBuffers& b) {
  PrepGeom pg = prep_geom(g);
  prep_local_attr();
  const PrepSmall s = PrepSmall::of(b.d_small, prep_heavy_words(g));  // (hv.cnt is zeroed with the words before it)
  if (prep_fill(st, b.err, b.d_small, s) != 0) return -1;
  launch_hist_scan<FR>(st, scalars, mont, g, pg, s, b.err);
  launch_scatter<FR, false>(st, scalars, mont, g, pg, prep_scatter_lds(g, pg), s, b.part, nullptr);
  const size_t lds_heavy = 2 * (size_t)(1u << pg.SH) * sizeof(u32);
  if (pg.HEAVY != 0xffffffffu)
    hipLaunchKernelGGL(k_prep_heavy_count, dim3(PREP_HEAVY_GRID), dim3(256), lds_heavy, st, s.part_start, b.part, pg, s.hv);
  hipLaunchKernelGGL(k_prep_local, dim3(pg.P), dim3(1024), prep_local_lds(pg), st, s.part_start, b.part, g, pg, b.vals_sorted, b.start,
                     b.items, b.item_off, s.part_items, s.hv);
  if (pg.HEAVY != 0xffffffffu)
    hipLaunchKernelGGL(k_prep_heavy_place, dim3(PREP_HEAVY_GRID), dim3(256), lds_heavy, st, s.part_start, b.part, g, pg, s.hv,
                       b.vals_sorted);
  hipLaunchKernelGGL(k_prep_offsets, dim3(cdiv(g.B, 256)), dim3(256), (pg.P + 256) * sizeof(u32), st, s.part_start, s.part_items, pg, g,
                     b.start, b.items, b.item_off, b.vals_sorted);
  return 0;
}
template <class FR>
int launch_prep_bps(hipStream_t st, const u32* scalars, int mont, MsmGeom g, u32 log2_l, const PrepBplBuffers& b) {
  PrepGeom pg = prep_bps_geom(g, log2_l);
  const PrepSmall s = PrepSmall::of(b.d_small, 0);
  if (prep_fill(st, b.err, b.d_small, s) != 0) return -1;
  prep_bps_attr();
  if (!pg.FIX) launch_hist_scan<FR>(st, scalars, mont, g, pg, s, b.err);
  launch_scatter<FR, false>(st, scalars, mont, g, pg, prep_scatter_lds(g, pg), s, b.part, b.err);
  hipLaunchKernelGGL(k_prep_local_s, dim3(pg.P), dim3(1024), prep_bps_local_lds(pg), st, pg.FIX ? s.part_cursor : s.part_start, b.part, g,
                     pg, prep_bps_stride(g, log2_l), log2_l, b.ents_t, (BplGroup*)b.grp, b.order, b.err);
  return 0;
}
template <class FR>
int launch_prep_bps_batch(hipStream_t st, const u32* const* scalars, u32 nv, int mont, MsmGeom g, u32 log2_l, const BpsBatchBuffers& b) {
  PrepGeom pg = prep_bps_geom(g, log2_l);
  const u32 stride = prep_bps_stride(g, log2_l);
  // every MSM's share of the buffers holds what launch_prep_bps would write of it
  // (16 entry slots per scalar: every key long enough for a bucket-split MSM has windows of 16 bits or more; the
  // 32-slot scatter with the record of pointers would spill to scratch and is not built: bps_batch_plan asks)
  if (nv < 1u || nv > (u32)PREP_BPS_BATCH || !pg.FIX || g.S > 16u || b.small_stride < prep_bps_small_block_words() ||
      (b.small_stride & 63u) || b.part_stride < prep_bps_part_entries(g, log2_l) ||
      (unsigned long long)b.ents_stride < (unsigned long long)pg.P * stride || b.grp_stride < pg.P * BPS_GROUPS ||
      b.order_stride < g.B)
    return -1;
  BpsBatchScalars sc;
  for (u32 v = 0; v < (u32)PREP_BPS_BATCH; v++) sc.scalars[v] = scalars[v < nv ? v : 0u];
  const PrepSmall s0 = PrepSmall::of(b.small + PREP_FLAG_WORDS, 0);  // MSM 0's small arrays, behind its flag words
  // ONE fill: all nv blocks of flag words and small arrays
  if (hipMemsetAsync(b.small, 0, (size_t)nv * b.small_stride * sizeof(u32), st) != hipSuccess) return -1;
  prep_bps_attr();
  const size_t lds_scatter = prep_scatter_lds(g, pg);
  if (lds_scatter > 64 * 1024)
    (void)hipFuncSetAttribute((const void*)k_prep_scatter_batch<FR, 16, 1>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)PREP_LDS_LIMIT);
  hipLaunchKernelGGL((k_prep_scatter_batch<FR, 16, 1>), dim3(cdiv(g.n, pg.SPB), nv), dim3(512), lds_scatter, st, sc, mont, g, pg,
                     s0.part_start, s0.part_cursor, b.small_stride, b.part, b.part_stride, b.small);
  hipLaunchKernelGGL(k_prep_local_s_batch, dim3(pg.P, nv), dim3(1024), prep_bps_local_lds(pg), st, s0.part_cursor, b.small_stride, b.part,
                     b.part_stride, g, pg, stride, log2_l, b.ents_t, b.ents_stride, (BplGroup*)b.grp, b.grp_stride, b.order, b.order_stride,
                     b.small);
  return 0;
}
template <class FR>
int launch_prep_bpl(hipStream_t st, const u32* scalars, int mont, MsmGeom g, const PrepBplBuffers& b) {
  PrepGeom pg = prep_bpl_geom(g);
  const PrepSmall s = PrepSmall::of(b.d_small, 0);
  if (prep_fill(st, b.err, b.d_small, s) != 0) return -1;
  prep_bpl_attr();
  if (!pg.FIX) launch_hist_scan<FR>(st, scalars, mont, g, pg, s, b.err);
  launch_scatter<FR, true>(st, scalars, mont, g, pg, prep_bpl_scatter_lds(g, pg), s, b.part, b.err);
  hipLaunchKernelGGL(k_prep_local_t, dim3(pg.P), dim3(1024), prep_bpl_local_lds(pg), st, pg.FIX ? s.part_cursor : s.part_start,
                     (const u64*)b.part, g, pg, prep_bpl_stride(g), b.ents_t, (BplGroup*)b.grp, b.order, b.err);
  return 0;
}

// ---- digits, probes and the Fr vector kernels ----
template <class FR>
void launch_digits(hipStream_t st, const u32* scalars, int mont, MsmGeom g, void* keys, bool keys16, u32* vals, u32* err) {
  if (keys16)
    hipLaunchKernelGGL((k_digits<FR, uint16_t>), dim3(cdiv(g.n, 256)), dim3(256), 0, st, scalars, mont, g, (uint16_t*)keys, vals, err);
  else
    hipLaunchKernelGGL((k_digits<FR, u32>), dim3(cdiv(g.n, 256)), dim3(256), 0, st, scalars, mont, g, (u32*)keys, vals, err);
}
template <class FR>
void launch_skew_probe(hipStream_t st, const u32* scalars, int mont, u32 n, DigitWalk walk, u32* d_flag, const u32* d_tv_words) {
  hipLaunchKernelGGL((k_skew_probe<FR>), dim3(1), dim3(1024), 0, st, scalars, mont, n, walk, d_flag, d_tv_words);
}
template <class FR>
void launch_vec_random(hipStream_t st, u32* out, u64 seed, u32 n, int mont) {
  hipLaunchKernelGGL((k_vec_random<FR>), dim3(cdiv(n, 256)), dim3(256), 0, st, out, seed, n, mont);
}
template <class FR>
void launch_vec_sample(hipStream_t st, u32* out, const blind::Key& key, u32 curve_id, u32 stream, u64 first, u32 n, int mont, int form) {
  static_assert(VEC_SAMPLE_TILE == 1024u || VEC_SAMPLE_TILE == 4096u, "one of the two instantiated tiles");
  if (form == 0) form = VEC_SAMPLE_TILE == 1024u ? 1 : 2;
  if (form == 1)
    hipLaunchKernelGGL((k_vec_sample<FR, 1024>), dim3(cdiv(n, 1024)), dim3(256), 0, st, out, key, curve_id, stream, first, n, mont);
  else
    hipLaunchKernelGGL((k_vec_sample<FR, 4096>), dim3(cdiv(n, 4096)), dim3(256), 0, st, out, key, curve_id, stream, first, n, mont);
}
template <class FR>
void launch_vec_hadamard(hipStream_t st, VecGrid vg, const u32* a, const u32* b, u32* out, u32 n) {
  hipLaunchKernelGGL((k_vec_hadamard<FR>), dim3(vec_stream_grid(n, vg)), dim3(256), 0, st, a, b, out, n);
}
template <class FR>
void launch_vec_combine(hipStream_t st, VecGrid vg, const CombineArgs& a, u32* out) {
  dim3 grid(vec_stream_grid(a.n, vg)), block(256);
  switch (a.n_vecs) {
    case 0:  // only the hiding addend
    case 1: hipLaunchKernelGGL((k_vec_combine<FR, 1>), grid, block, 0, st, a, out); break;
    case 2: hipLaunchKernelGGL((k_vec_combine<FR, 2>), grid, block, 0, st, a, out); break;
    case 3: hipLaunchKernelGGL((k_vec_combine<FR, 3>), grid, block, 0, st, a, out); break;
    case 4: hipLaunchKernelGGL((k_vec_combine<FR, 4>), grid, block, 0, st, a, out); break;
    case 5: hipLaunchKernelGGL((k_vec_combine<FR, 5>), grid, block, 0, st, a, out); break;
    case 6: hipLaunchKernelGGL((k_vec_combine<FR, 6>), grid, block, 0, st, a, out); break;
    case 7: hipLaunchKernelGGL((k_vec_combine<FR, 7>), grid, block, 0, st, a, out); break;
    default: hipLaunchKernelGGL((k_vec_combine<FR, 8>), grid, block, 0, st, a, out); break;
  }
}
template <class FR>
void launch_vec_powers(hipStream_t st, const u32 point[8], u32 n, u32* out) {
  CombineArgs a;
  memset(&a, 0, sizeof(a));
  memcpy(a.coeff[0], point, 32);
  a.n = n;
  hipLaunchKernelGGL((k_vec_powers<FR>), dim3(cdiv(n, 256)), dim3(256), 0, st, a, out);
}
template <class FR>
void launch_poly_tile_values(hipStream_t st, const PolyArgs& a, u32 n_polys, u32 max_tiles, bool eval, u32* out) {
  if (eval) hipLaunchKernelGGL((k_poly_tile_values<FR, true>), dim3(max_tiles, n_polys), dim3(256), 0, st, a, out);
  else hipLaunchKernelGGL((k_poly_tile_values<FR, false>), dim3(max_tiles, n_polys), dim3(256), 0, st, a, out);
}
template <class FR>
void launch_poly_carries(hipStream_t st, const PolyArgs& a, u32 n_polys) {
  hipLaunchKernelGGL((k_poly_carries<FR>), dim3(1, n_polys), dim3(256), 0, st, a);
}
template <class FR>
void launch_poly_div_tiles(hipStream_t st, const PolyArgs& a, u32 n_polys, u32 max_tiles, const u32* carries) {
  hipLaunchKernelGGL((k_poly_div_tiles<FR>), dim3(max_tiles, n_polys), dim3(256), 0, st, a, carries);
}
template <class FR>
void launch_vec_inner_product(hipStream_t st, const u32* a, const u32* b, u32 n, u32 blocks, u32* out) {
  hipLaunchKernelGGL((k_vec_inner_product<FR>), dim3(blocks), dim3(256), 0, st, a, b, n, out);
}
template <class FR>
void launch_vec_inner_product_pair(hipStream_t st, const u32* a0, const u32* b0, const u32* a1, const u32* b1, u32 n, u32 blocks,
                                   u32* out) {
  hipLaunchKernelGGL((k_vec_inner_product_pair<FR>), dim3(blocks, 2), dim3(256), 0, st, a0, b0, a1, b1, n, out);
}
template <class FR>
void launch_ipa_fold_ip(hipStream_t st, u32* c, u32* z, u32 half, const u32 x[8], const u32 xinv[8], u32 blocks, u32* out) {
  IpaFoldArgs a;
  memcpy(a.x, x, 32);
  memcpy(a.xinv, xinv, 32);
  hipLaunchKernelGGL((k_ipa_fold_ip<FR>), dim3(blocks), dim3(256), 0, st, c, z, half, a, out);
}
template <class FR>
void launch_check_poly_coeffs(hipStream_t st, const u32* xi, u32 k, u32* out) {
  CheckPolyArgs a;
  memset(&a, 0, sizeof(a));
  memcpy(a.xi, xi, (size_t)k * 32);
  a.k = k;
  hipLaunchKernelGGL((k_check_poly_coeffs<FR>), dim3(cdiv(1u << k, 256)), dim3(256), 0, st, a, out);
}
template <class FR>
void launch_ipa_round_scalars(hipStream_t st, const u32* xi, u32 j, u32 log_n, const u32* c, u32* out_l, u32* out_r) {
  CheckPolyArgs a;
  memset(&a, 0, sizeof(a));
  memcpy(a.xi, xi, (size_t)j * 32);
  a.k = j;
  hipLaunchKernelGGL((k_ipa_round_scalars<FR>), dim3(cdiv(1u << log_n, 256)), dim3(256), 0, st, a, j, log_n, c, out_l, out_r);
}
template <class FR>
void launch_spmv(hipStream_t st, const u32* row_ptr, const u32* col, const u32* val, const u32* input, u32 n_input, const u32* witness,
                 u32 n_witness, u32* out, u32 n_rows) {
  hipLaunchKernelGGL((k_spmv<FR>), dim3(cdiv(n_rows, 256)), dim3(256), 0, st, row_ptr, col, val, input, n_input, witness, n_witness, out,
                     n_rows);
}
template <class FR>
void launch_hp_t_vecs(hipStream_t st, VecGrid vg, const TVecArgs& a, int n_inputs) {
  dim3 grid(vec_stream_grid(a.len, vg)), block(256);
  switch (n_inputs) {
    case 1: hipLaunchKernelGGL((k_hp_t_vecs<FR, 1>), grid, block, 0, st, a); break;
    case 2: hipLaunchKernelGGL((k_hp_t_vecs<FR, 2>), grid, block, 0, st, a); break;
    case 3: hipLaunchKernelGGL((k_hp_t_vecs<FR, 3>), grid, block, 0, st, a); break;
    case 4: hipLaunchKernelGGL((k_hp_t_vecs<FR, 4>), grid, block, 0, st, a); break;
    case 5: hipLaunchKernelGGL((k_hp_t_vecs<FR, 5>), grid, block, 0, st, a); break;
    case 6: hipLaunchKernelGGL((k_hp_t_vecs<FR, 6>), grid, block, 0, st, a); break;
    case 7: hipLaunchKernelGGL((k_hp_t_vecs<FR, 7>), grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL((k_hp_t_vecs<FR, 8>), grid, block, 0, st, a); break;
  }
}

// Every launcher above instantiated for one scalar field: a list of names with no logic in it (the signatures are launch.h's).
#define AMSM_FR_LAUNCHERS(FR)                                                        \
  template decltype(launch_prep<FR>) launch_prep<FR>;                                  \
  template decltype(launch_prep_bps<FR>) launch_prep_bps<FR>;                          \
  template decltype(launch_prep_bps_batch<FR>) launch_prep_bps_batch<FR>;              \
  template decltype(launch_prep_bpl<FR>) launch_prep_bpl<FR>;                          \
  template decltype(launch_digits<FR>) launch_digits<FR>;                              \
  template decltype(launch_skew_probe<FR>) launch_skew_probe<FR>;                      \
  template decltype(launch_vec_random<FR>) launch_vec_random<FR>;                      \
  template decltype(launch_vec_sample<FR>) launch_vec_sample<FR>;                      \
  template decltype(launch_vec_hadamard<FR>) launch_vec_hadamard<FR>;                  \
  template decltype(launch_vec_combine<FR>) launch_vec_combine<FR>;                    \
  template decltype(launch_vec_powers<FR>) launch_vec_powers<FR>;                      \
  template decltype(launch_poly_tile_values<FR>) launch_poly_tile_values<FR>;          \
  template decltype(launch_poly_carries<FR>) launch_poly_carries<FR>;                  \
  template decltype(launch_poly_div_tiles<FR>) launch_poly_div_tiles<FR>;              \
  template decltype(launch_vec_inner_product<FR>) launch_vec_inner_product<FR>;        \
  template decltype(launch_vec_inner_product_pair<FR>) launch_vec_inner_product_pair<FR>; \
  template decltype(launch_ipa_fold_ip<FR>) launch_ipa_fold_ip<FR>;                    \
  template decltype(launch_check_poly_coeffs<FR>) launch_check_poly_coeffs<FR>;        \
  template decltype(launch_ipa_round_scalars<FR>) launch_ipa_round_scalars<FR>;        \
  template decltype(launch_spmv<FR>) launch_spmv<FR>;                                  \
  template decltype(launch_hp_t_vecs<FR>) launch_hp_t_vecs<FR>;

AMSM_FR_LAUNCHERS(PallasFr)
AMSM_FR_LAUNCHERS(Bls12381Fr)
AMSM_FR_LAUNCHERS(VestaFr)
AMSM_FR_LAUNCHERS(Bn254Fr)
AMSM_FR_LAUNCHERS(GrumpkinFr)
AMSM_FR_LAUNCHERS(Bls12377Fr)

}  // namespace amsm
