// Launcher definitions for the elliptic-curve kernels, as ordinary function templates over the (C-ABI) base-field parameter pack
// (launch.h declares them).  kern_pallas.hip, kern_bls12_381.hip, kern_vesta.hip, kern_bn254.hip, kern_grumpkin.hip and
// kern_bls12_377.hip include this file and instantiate the list at its end for their curve's Fq, one unit per curve so that the
// library builds in parallel.  The kernels are instantiated for FQD = DevField<Fq>::type, the field the device computes in (fp.h).
// Launches and nothing else: what a launch needs computed on the host arrives computed (msm_select.h, fold_recode.h).
#include <algorithm>
#include <atomic>
#include <vector>

#include "curves.h"
#include "launch.h"
#include "msm_kernels.h"
#include "points_check_kernels.h"
#include "sample_kernels.h"

namespace amsm {

template <class Fq>
void launch_accum_l0(hipStream_t st, const u32* table, const u32* vals_sorted, const u32* start,
                     const u32* item_off, MsmGeom g, u32* partials) {
  using FQD = typename DevField<Fq>::type;
  hipLaunchKernelGGL((k_accum_l0<FQD>), dim3(cdiv(g.n_chunks, 256)), dim3(256), 0, st, table, vals_sorted,
                     start, item_off, g, partials);
}
template <class Fq>
void launch_accum_bpl(hipStream_t st, const u32* table, const u32* ents_t, const void* grp, const u32* order,
                      u32 n_groups, u32 groups_per_part, const u32* flags, u32* buckets, u32 wg_per_cu, bool accumulate) {
  using FQD = typename DevField<Fq>::type;
  // wg_per_cu = 1 / 2: unused dynamic LDS caps the residency (160 KiB per CU) -- the dispatcher fills a CU to the kernel's
  // occupancy before it moves on, so a grid of fewer workgroups than the chip holds (a 2^18-pair MSM: 544 against 768 places)
  // would leave a third of the CUs idle and the others with three waves per SIMD sharing one multiplier
  constexpr u32 STATIC_LDS = 2u * 4u * GatherLds<FQD>::WAVE_BYTES;
  u32 pad = 0;
  if (wg_per_cu == 1u) pad = 82u * 1024u > STATIC_LDS ? 82u * 1024u - STATIC_LDS : 0u;
  else if (wg_per_cu == 2u) pad = 54u * 1024u > STATIC_LDS ? 54u * 1024u - STATIC_LDS : 0u;
  if (STATIC_LDS + pad > 64u * 1024u) {  // opt in, once per device
    static DeviceOnce once;
    once.run([] {
      (void)hipFuncSetAttribute((const void*)k_accum_bpl<FQD, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
      (void)hipFuncSetAttribute((const void*)k_accum_bpl<FQD, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
    });
  }
  if (accumulate)
    hipLaunchKernelGGL((k_accum_bpl<FQD, true>), dim3(cdiv(n_groups, 4)), dim3(256), pad, st, table, ents_t,
                       (const BplGroupHdr*)grp, order, n_groups, groups_per_part, flags, buckets);
  else
    hipLaunchKernelGGL((k_accum_bpl<FQD, false>), dim3(cdiv(n_groups, 4)), dim3(256), pad, st, table, ents_t,
                       (const BplGroupHdr*)grp, order, n_groups, groups_per_part, flags, buckets);
}
template <class Fq>
void launch_accum_bps(hipStream_t st, const u32* table, const u32* ents_t, const void* grp, const u32* order,
                      u32 n_groups, u32 log2_l, const u32* flags, u32* buckets) {
  using FQD = typename DevField<Fq>::type;
  hipLaunchKernelGGL((k_accum_bps<FQD>), dim3(cdiv(n_groups, 4)), dim3(256), 0, st, table, ents_t,
                     (const BplGroupHdr*)grp, order, n_groups, log2_l, flags, buckets);
}
template <class Fq>
void launch_accum_bps_batch(hipStream_t st, const u32* table, const BpsBatchBuffers& b, u32 nv, u32 n_groups, u32 log2_l,
                            u32 n_buckets, u32* buckets) {
  using FQD = typename DevField<Fq>::type;
  hipLaunchKernelGGL((k_accum_bps_batch<FQD>), dim3(cdiv(n_groups, 4), nv), dim3(256), 0, st, table, (const u32*)b.ents_t, b.ents_stride,
                     (const BplGroupHdr*)b.grp, b.grp_stride, (const u32*)b.order, b.order_stride, n_groups, log2_l, (const u32*)b.small,
                     buckets, n_buckets);
}
template <class Fq>
int accum_l0_blocks_per_cu() {
  using FQD = typename DevField<Fq>::type;
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_accum_l0<FQD>, 256, 0) != hipSuccess) {
    (void)hipGetLastError();
    return 4;
  }
  return n;
}
template <class Fq>
void launch_accum_l1(hipStream_t st, u32 lanes_per_bucket, const u32* partials, const u32* items,
                     const u32* item_off, MsmGeom g, u32* buckets, u32* heavy_count, u32* heavy_list) {
  using FQD = typename DevField<Fq>::type;
  // 64-bit grid arithmetic: B * lanes can exceed 2^32 only for absurd geometries; B <= 2^24 here
  if (lanes_per_bucket >= 16)
    hipLaunchKernelGGL((k_accum_l1<FQD, 16>), dim3(cdiv(g.B * 16u, 256)), dim3(256), 0, st, partials, items,
                       item_off, g, buckets, heavy_count, heavy_list);
  else if (lanes_per_bucket >= 4)
    hipLaunchKernelGGL((k_accum_l1<FQD, 4>), dim3(cdiv(g.B * 4u, 256)), dim3(256), 0, st, partials, items,
                       item_off, g, buckets, heavy_count, heavy_list);
  else
    hipLaunchKernelGGL((k_accum_l1<FQD, 1>), dim3(cdiv(g.B, 256)), dim3(256), 0, st, partials, items, item_off,
                       g, buckets, heavy_count, heavy_list);
}
template <class Fq>
void launch_accum_l2(hipStream_t st, const u32* partials, const u32* items, const u32* item_off,
                     const u32* heavy_count, const u32* heavy_list, u32* scratch, u32* buckets) {
  using FQD = typename DevField<Fq>::type;
  hipLaunchKernelGGL((k_accum_l2a<FQD>), dim3(L2_SLICES, 64), dim3(256), 0, st, partials, items, item_off, heavy_count,
                     heavy_list, scratch);
  hipLaunchKernelGGL((k_accum_l2b<FQD>), dim3(64), dim3(64), 0, st, scratch, heavy_count, heavy_list, buckets);
}
template <class Fq>
u32 accum_l2_slices() {
  return L2_SLICES;
}
// the bare fold over ready partial records (the tail's last launch; the direct sum's and the two-valued sums' only one)
template <class Fq>
void launch_fold(hipStream_t st, bool quad, u32 n_sets, const u32* in, u32 n_per_set, u32* out, const u32* flags, u32* mirror,
                 bool clear_flags) {
  using FQD = typename DevField<Fq>::type;
  // quad: four waves when there are enough records to share out (msm_kernels.h), one otherwise
  if (quad)
    hipLaunchKernelGGL((k_fold<FQD, true>), dim3(n_sets), dim3(n_per_set > 32u ? 256 : 64), 0, st, in, n_per_set, out, flags, mirror,
                       clear_flags ? 1u : 0u);
  else hipLaunchKernelGGL((k_fold<FQD, false>), dim3(n_sets), dim3(64), 0, st, in, n_per_set, out, flags, mirror, 0u);
}
// The tail of an MSM as msm_select.h planned it (tail_plan: the form, the grids and what the buffers hold): the buckets of g.n_sets sets
// of g.nb to one exported record per set in `out`, mirrored.  rc: t.rc_records records (RED2), partial: g.n_sets * t.partials records,
// ticket: g.n_sets zeroed words (where t.ticket).
template <class Fq>
void launch_tail(hipStream_t st, const msel::TailPlan& t, const u32* buckets, MsmGeom g, u32* rc, u32* partial, u32* ticket,
                 u32* out, const u32* flags, u32* mirror) {
  using FQD = typename DevField<Fq>::type;
  g.red_s = t.red_s;
  g.red_threads = t.red_threads;
  const dim3 grid(t.partials, g.n_sets);
  if (t.form == msel::FUSED_QUAD) {
    hipLaunchKernelGGL((k_bucket_reduce<FQD, true, true>), grid, dim3(256), 0, st, buckets, g, partial, ticket, out, flags, mirror);
    return;
  }
  if (t.form == msel::RED2) {  // row / column sums, then their small multiples
    const Red2Geom r = msel::red2_geom(g.nb, t.latency);
    hipLaunchKernelGGL((k_red2_sums<FQD>), dim3(cdiv(r.row_waves + r.col_waves, 4), g.n_sets), dim3(256), 0, st, buckets, g.nb, r, rc);
    if (t.quad) hipLaunchKernelGGL((k_red2_weighted<FQD, true>), grid, dim3(256), 0, st, rc, r.A, partial);
    else hipLaunchKernelGGL((k_red2_weighted<FQD, false>), grid, dim3(256), 0, st, rc, r.A, partial);
  } else {
    hipLaunchKernelGGL((k_bucket_reduce<FQD, false, false>), grid, dim3(256), 0, st, buckets, g, partial, (u32*)nullptr, (u32*)nullptr,
                       (const u32*)nullptr, (u32*)nullptr);
  }
  launch_fold<Fq>(st, t.quad, g.n_sets, partial, t.partials, out, flags, mirror, false);
}
template <class Fq>
void launch_ipa_jump_accum(hipStream_t st, const u32* table, const u32* entries, const u32* list_off, const u32* list_slot,
                           u32 n_lists, u32 m0, u32 nb, u32* buckets) {
  using FQD = typename DevField<Fq>::type;
  hipLaunchKernelGGL((k_ipa_jump_accum<FQD>), dim3(n_lists, m0 / 64u), dim3(64 * JUMP_WAVES), 0, st, table, entries, list_off, list_slot, m0,
                     nb, buckets);
}
// Points per lane of the batched XYZZ -> affine conversion: 4 (one inversion per 4 points; 8 would starve the GPU of
// lanes at the sizes that matter).  Below BATCH_AFFINE_MIN points the kernels convert in place, one inversion each.
constexpr u32 BATCH_AFFINE_K = 4, BATCH_AFFINE_MIN = 1u << 17;
// ... and 8 per lane from 2^19 points up, where that still leaves a wave per SIMD: 1.9x less work per point (the inversion
// is ~480 of a lane's ~520 multiplications on BLS12-381)
template <class FQD, bool ABI>
static void launch_batch_to_affine(hipStream_t st, const u32* xyzz, u32 n, u32* out) {
  if (n >= (1u << 19))
    hipLaunchKernelGGL((k_batch_to_affine<FQD, 8, ABI>), dim3(cdiv(cdiv(n, 8), 256)), dim3(256), 0, st, xyzz, n, out);
  else
    hipLaunchKernelGGL((k_batch_to_affine<FQD, BATCH_AFFINE_K, ABI>), dim3(cdiv(cdiv(n, BATCH_AFFINE_K), 256)), dim3(256), 0, st,
                       xyzz, n, out);
}
template <class Fq>
void launch_precompute_all_levels(hipStream_t st, u32* table, u32 n, u32 c, u32 W, u32* xyzz_scratch) {
  using FQD = typename DevField<Fq>::type;
  if (W < 2) return;
  hipLaunchKernelGGL((k_precompute_all_levels<FQD>), dim3(cdiv(n, 64)), dim3(64), 0, st, table, n, c, W, xyzz_scratch);
  launch_batch_to_affine<FQD, false>(st, xyzz_scratch, (W - 1u) * n, table + (size_t)n * (2 * FQD::W));
}
template <class Fq>
void launch_ds_table(hipStream_t st, const u32* win_table, u32 n, u32 c, u32 W, u32* xyzz_scratch, u32 slab_windows,
                     u32* table) {
  using FQD = typename DevField<Fq>::type;
  // slabs of `slab_windows` of the 64 four-bit windows: scratch = 8 planes x slab_windows x n XYZZ records (the whole table at once
  // was 2-3 GiB of scratch for a 2^15-generator key: ADVICE r4)
  for (u32 w0 = 0; w0 < DS_W; w0 += slab_windows) {
    const u32 wn = std::min(slab_windows, DS_W - w0), count = n * wn;
    hipLaunchKernelGGL((k_ds_levels<FQD>), dim3(cdiv(count, 256)), dim3(256), 0, st, win_table, n, c, W, w0, wn, xyzz_scratch);
    hipLaunchKernelGGL((k_ds_multiples<FQD>), dim3(cdiv(count, 256)), dim3(256), 0, st, xyzz_scratch, count);
    for (u32 j = 0; j < DS_MULT; j++)  // plane j of the slab -> d_small[(j 64 + w0) n ...]
      launch_batch_to_affine<FQD, false>(st, xyzz_scratch + (size_t)j * count * (4 * FQD::W), count,
                                    table + ((size_t)j * DS_W + w0) * n * (2 * FQD::W));
  }
}
template <class Fq>
u32 launch_direct_sum(hipStream_t st, const u32* table, u32 key_n, u32 nv, const u32* const* scalars, const u32* ns,
                      const u32* base_offs, int mont, u32 m, int group_shift, u32* flags, u32* partials) {
  using FQD = typename DevField<Fq>::type;
  using Fr = typename CurveOf<Fq>::type::Fr;  // the scalars' field
  DsBatch b;
  memset(&b, 0, sizeof(b));
  u32 n_max = 0;
  for (u32 v = 0; v < nv && v < (u32)DS_BATCH; v++) {
    b.scalars[v] = scalars[v];
    b.n[v] = ns[v];
    b.base_off[v] = base_offs[v];
    n_max = std::max(n_max, ns[v]);
  }
  // per MSM (grouped: per class, n / 2 indices each); a shorter vector's surplus workgroups write the identity
  const u32 blocks = cdiv((group_shift >= 0 ? n_max / 2u : n_max) * (DS_W / m), 256);
  hipLaunchKernelGGL((k_direct_sum<FQD, Fr>), dim3(blocks, group_shift >= 0 ? 2u : nv), dim3(256), 0, st, table, key_n, b, mont, m,
                     group_shift, flags, partials);
  return blocks;
}
template <class Fq>
bool batch_affine_pays(u32 n) { return n >= BATCH_AFFINE_MIN; }
                       template <class Fq>
                       void launch_precompute_level(hipStream_t st, u32* table, u32 stride, u32 level, u32 c, u32* xyzz_scratch) {
  using FQD = typename DevField<Fq>::type;
  if (xyzz_scratch && stride >= BATCH_AFFINE_MIN) {
    hipLaunchKernelGGL((k_precompute_level<FQD, true>), dim3(cdiv(stride, 256)), dim3(256), 0, st, table, stride, level, c,
                       xyzz_scratch);
    launch_batch_to_affine<FQD, false>(st, xyzz_scratch, stride, table + (size_t)level * stride * (2 * FQD::W));
  } else {
    hipLaunchKernelGGL((k_precompute_level<FQD, false>), dim3(cdiv(stride, 256)), dim3(256), 0, st, table, stride, level, c,
                       (u32*)nullptr);
  }
}
template <class FQD, bool ABI, bool XO>
static void points_fold_dispatch(hipStream_t st, dim3 grid, bool glv, const u32* l, const u32* r, u32 n, const FoldDigits& d,
                                 u32* out) {
  // the ladder runs in Jacobian coordinates (ec.h: jac_dbl 3M + 4S against the XYZZ doubling's 6M + 3S; measured -2 % of an opening)
  if (glv) hipLaunchKernelGGL((k_points_fold<FQD, ABI, XO, true, true>), grid, dim3(256), 0, st, l, r, n, d, out);
  else hipLaunchKernelGGL((k_points_fold<FQD, ABI, XO, false, true>), grid, dim3(256), 0, st, l, r, n, d, out);
}
template <class Fq>
void launch_points_fold(hipStream_t st, const u32* l, const u32* r, u32 n, const FoldDigits& d, bool glv, u32* out,
                        bool abi_radix, u32* xyzz_scratch) {
  using FQD = typename DevField<Fq>::type;
  const dim3 grid(cdiv(n, 256));
  if (xyzz_scratch && n >= BATCH_AFFINE_MIN) {  // sums to scratch, then one inversion per BATCH_AFFINE_K points
    if (abi_radix) {
      points_fold_dispatch<FQD, true, true>(st, grid, glv, l, r, n, d, xyzz_scratch);
      launch_batch_to_affine<FQD, true>(st, xyzz_scratch, n, out);
    } else {
      points_fold_dispatch<FQD, false, true>(st, grid, glv, l, r, n, d, xyzz_scratch);
      launch_batch_to_affine<FQD, false>(st, xyzz_scratch, n, out);
    }
  } else if (abi_radix) {
    points_fold_dispatch<FQD, true, false>(st, grid, glv, l, r, n, d, out);
  } else {
    points_fold_dispatch<FQD, false, false>(st, grid, glv, l, r, n, d, out);
  }
}
template <class Fq>
void launch_points_fold_tab(hipStream_t st, const u32* table, u32 stride, u32 n, const FoldTabOps& d, u32* out,
                            u32* xyzz_scratch) {
  using FQD = typename DevField<Fq>::type;
  const dim3 grid(cdiv(n, 256));
  if (xyzz_scratch && n >= BATCH_AFFINE_MIN) {
    hipLaunchKernelGGL((k_points_fold_tab<FQD, true>), grid, dim3(256), 0, st, table, stride, n, d, xyzz_scratch);
    launch_batch_to_affine<FQD, false>(st, xyzz_scratch, n, out);
  } else {
    hipLaunchKernelGGL((k_points_fold_tab<FQD, false>), grid, dim3(256), 0, st, table, stride, n, d, out);
  }
}
template <class Fq>
void launch_tv_sum(hipStream_t st, const u32* table, u32 nv, const u32* const* scalars, const u32* const* probes,
                   const u32* ns, const u32* base_offs, u32 blocks, u32* parts, u32* exc) {
  using FQD = typename DevField<Fq>::type;
  TvBatch b;
  memset(&b, 0, sizeof(b));
  for (u32 v = 0; v < nv && v < (u32)TV_BATCH; v++) {
    b.scalars[v] = scalars[v];
    b.probe[v] = probes[v];
    b.n[v] = ns[v];
    b.base_off[v] = base_offs[v];
  }
  hipLaunchKernelGGL((k_tv_sum<FQD>), dim3(blocks, std::min<u32>(nv, TV_BATCH)), dim3(256), 0, st, table, b, parts, exc);
}
template <class Fq>
void launch_apply_inf(hipStream_t st, u32* table, const uint8_t* is_inf, u32 n) {
  using FQD = typename DevField<Fq>::type;
  hipLaunchKernelGGL((k_apply_inf<FQD>), dim3(cdiv(n, 256)), dim3(256), 0, st, table, is_inf, n);
}
template <class Fq>
void launch_generate_bases(hipStream_t st, u32* table, u64 seed, u32 first, u32 n, const u32* gen_xy_mont) {
  using FQD = typename DevField<Fq>::type;
  AffineWords<FQD> gen;
  for (int i = 0; i < 2 * FQD::W; i++) gen.w[i] = gen_xy_mont[i];
  hipLaunchKernelGGL((k_generate_bases<FQD>), dim3(cdiv(n, 256)), dim3(256), 0, st, table, seed, first, n, gen);
}
template <class Fq>
void launch_sample_search(hipStream_t st, u32* table, u32* jwin, const u64* pend_in, u32 n_in, u64* pend_out, u32* counters,
                          const SampleConsts& k, u64 first, u32 max_tests) {
  using FQD = typename DevField<Fq>::type;
  if (n_in == 0) return;
  hipLaunchKernelGGL((k_sample_search<FQD>), dim3(cdiv(n_in, 256)), dim3(256), 0, st, table, jwin, pend_in, n_in, pend_out, counters, k,
                     first, max_tests);
}
template <class Fq>
void launch_sample_finish(hipStream_t st, u32* table, u32* jwin, u32 n, u32* counters, const SampleConsts& k, u64 first) {
  using FQD = typename DevField<Fq>::type;
  if (n == 0) return;
  hipLaunchKernelGGL((k_sample_finish<FQD>), dim3(cdiv(n, 256)), dim3(256), 0, st, table, jwin, n, counters, k, first);
}
template <class Fq>
void launch_points_check(hipStream_t st, const u32* xy, const uint8_t* is_inf, u32 n, uint8_t* status, u32* counters,
                         const PointsCheckConsts& k, int ladder) {
  using FQD = typename DevField<Fq>::type;
  if (n == 0) return;
  hipLaunchKernelGGL((k_points_check_curve<FQD>), dim3(cdiv(n, 256)), dim3(256), 0, st, xy, is_inf, n, status, counters, k);
  if constexpr (CurveOf<Fq>::type::subgroup_check) {
    if (ladder == 2)
      hipLaunchKernelGGL((k_points_check_subgroup<FQD, 2>), dim3(cdiv(n, 256)), dim3(256), 0, st, xy, is_inf, n, status, counters, k);
    else
      hipLaunchKernelGGL((k_points_check_subgroup<FQD, 1>), dim3(cdiv(n, 256)), dim3(256), 0, st, xy, is_inf, n, status, counters, k);
  }
}
template <class Fq>
bool device_internal_radix() {
  using FQD = typename DevField<Fq>::type;
  return FQD::UNSAT;
}
template <class Fq>
void launch_points_import(hipStream_t st, const u32* src, u32* dst, u32 n) {
  using FQD = typename DevField<Fq>::type;
  static_assert(FQD::W == Fq::W, "device field must share the memory layout of the ABI field");  // (src may equal dst)
  if (!FQD::UNSAT || n == 0) return;
  hipLaunchKernelGGL((k_points_import<FQD>), dim3(cdiv(n, 256)), dim3(256), 0, st, src, dst, n);
}
template <class Fq>
void launch_points_export(hipStream_t st, const u32* src, u32* dst, u32 n) {
  using FQD = typename DevField<Fq>::type;
  if (!FQD::UNSAT || n == 0) return;
  hipLaunchKernelGGL((k_points_export<FQD>), dim3(cdiv(n, 256)), dim3(256), 0, st, src, dst, n);
}

}  // namespace amsm

// Every launcher and query above instantiated for one base field: a list of names with no logic in it (the signatures are launch.h's).
// A curve's unit is this line under the include.
#define AMSM_EC_LAUNCHERS(FQ) \
  namespace amsm { \
  template decltype(launch_accum_l0<FQ>) launch_accum_l0<FQ>; \
  template decltype(launch_accum_bpl<FQ>) launch_accum_bpl<FQ>; \
  template decltype(launch_accum_bps<FQ>) launch_accum_bps<FQ>; \
  template decltype(launch_accum_bps_batch<FQ>) launch_accum_bps_batch<FQ>; \
  template decltype(accum_l0_blocks_per_cu<FQ>) accum_l0_blocks_per_cu<FQ>; \
  template decltype(launch_accum_l1<FQ>) launch_accum_l1<FQ>; \
  template decltype(launch_accum_l2<FQ>) launch_accum_l2<FQ>; \
  template decltype(accum_l2_slices<FQ>) accum_l2_slices<FQ>; \
  template decltype(launch_fold<FQ>) launch_fold<FQ>; \
  template decltype(launch_tail<FQ>) launch_tail<FQ>; \
  template decltype(launch_ipa_jump_accum<FQ>) launch_ipa_jump_accum<FQ>; \
  template decltype(launch_precompute_all_levels<FQ>) launch_precompute_all_levels<FQ>; \
  template decltype(launch_ds_table<FQ>) launch_ds_table<FQ>; \
  template decltype(launch_direct_sum<FQ>) launch_direct_sum<FQ>; \
  template decltype(batch_affine_pays<FQ>) batch_affine_pays<FQ>; \
  template decltype(launch_precompute_level<FQ>) launch_precompute_level<FQ>; \
  template decltype(launch_points_fold<FQ>) launch_points_fold<FQ>; \
  template decltype(launch_points_fold_tab<FQ>) launch_points_fold_tab<FQ>; \
  template decltype(launch_tv_sum<FQ>) launch_tv_sum<FQ>; \
  template decltype(launch_apply_inf<FQ>) launch_apply_inf<FQ>; \
  template decltype(launch_generate_bases<FQ>) launch_generate_bases<FQ>; \
  template decltype(launch_sample_search<FQ>) launch_sample_search<FQ>; \
  template decltype(launch_sample_finish<FQ>) launch_sample_finish<FQ>; \
  template decltype(launch_points_check<FQ>) launch_points_check<FQ>; \
  template decltype(device_internal_radix<FQ>) device_internal_radix<FQ>; \
  template decltype(launch_points_import<FQ>) launch_points_import<FQ>; \
  template decltype(launch_points_export<FQ>) launch_points_export<FQ>; \
  }
