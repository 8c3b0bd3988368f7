// Host-callable launchers for the device kernels.  The heavy elliptic-curve kernels are compiled in one
// translation unit per curve (kern_pallas.hip / kern_bls12_381.hip / kern_vesta.hip / kern_bn254.hip / kern_grumpkin.hip / kern_bls12_377.hip:
// each instantiates kern_ec.inc's templates for its base field), the scalar-field kernels in kern_fr.hip, so the library builds in
// parallel; api.hip only sees these declarations.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>

#include "blind.h"
#include "fold_recode.h"
#include "msm_select.h"
#include "msm_types.h"
#include "prep_geom.h"

namespace amsm {

// What a launcher must do once per DEVICE before its kernel runs there -- opting in to more than 64 KiB of dynamic LDS: the attribute
// is per device, a second context on another GPU of the same process needs its own.  One bit per device; a device the runtime does
// not name (or beyond 62) takes bit 63, which never counts as done: there the work is repeated on every call.
struct DeviceOnce {
  std::atomic<unsigned long long> done{0};
  template <class F>
  void run(F&& f) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 63;
    const unsigned long long bit = 1ull << dev;
    if (dev != 63 && (done.load(std::memory_order_acquire) & bit)) return;
    f();
    done.fetch_or(bit, std::memory_order_release);
  }
};

// workgroups of b lanes (or lanes of b items) that cover a items
inline u32 cdiv(u32 a, u32 b) { return (a + b - 1) / b; }

// ---- per-curve (Fq) launchers ------------------------------------------------------------------
template <class Fq>
void launch_accum_l0(hipStream_t st, const u32* table, const u32* vals_sorted, const u32* start,
                     const u32* item_off, MsmGeom g, u32* partials);
// bucket-per-lane accumulation (msm_kernels.h: k_accum_bpl) over the transposed layout k_prep_local_t wrote
template <class Fq>
void launch_accum_bpl(hipStream_t st, const u32* table, const u32* ents_t, const void* grp, const u32* order, u32 n_groups,
                      u32 groups_per_part, const u32* flags, u32* buckets, u32 wg_per_cu = 0, bool accumulate = false);
// resident 256-lane workgroups of accumulate L0 per CU (occupancy query)
template <class Fq>
int accum_l0_blocks_per_cu();
template <class Fq>
void launch_accum_l1(hipStream_t st, u32 lanes_per_bucket, const u32* partials, const u32* items, const u32* item_off, MsmGeom g,
                     u32* buckets, u32* heavy_count, u32* heavy_list);
template <class Fq>
void launch_accum_l2(hipStream_t st, const u32* partials, const u32* items, const u32* item_off,
                     const u32* heavy_count, const u32* heavy_list, u32* scratch, u32* buckets);
template <class Fq>
u32 accum_l2_slices();  // scratch records per heavy bucket
// The tail of an MSM (msm_kernels.h: k_bucket_reduce / k_red2_* / k_fold) as msel::tail_plan planned it: form, grids and buffer sizes
// all come from the plan.  rc: t.rc_records records of scratch (RED2), partial: g.n_sets * t.partials records, ticket: g.n_sets zeroed
// words (t.ticket), out: g.n_sets records + the two flag words (flags may be null), mirror: the same in page-locked host memory.
template <class Fq>
void launch_tail(hipStream_t st, const msel::TailPlan& t, const u32* buckets, MsmGeom g, u32* rc, u32* partial, u32* ticket, u32* out,
                 const u32* flags, u32* host_mirror);
// the bare fold of n_per_set ready partial records per set; quad: a quad of lanes per logical lane (ec.h: xyzz_add_quad).
// flags (may be null): two words copied behind the n_sets records (out needs 8 bytes more); clear_flags (quad only): the two words are
// zeroed once they have been copied out
template <class Fq>
void launch_fold(hipStream_t st, bool quad, u32 n_sets, const u32* in, u32 n_per_set, u32* out, const u32* flags, u32* host_mirror = nullptr,
                 bool clear_flags = false);
// round 6: the jump fold of an IPA opening (msm_kernels.h: k_ipa_jump_accum): n_lists lists, m0 (a multiple of 64) outputs
template <class Fq>
void launch_ipa_jump_accum(hipStream_t st, const u32* table, const u32* entries, const u32* list_off, const u32* list_slot, u32 n_lists,
                           u32 m0, u32 nb, u32* buckets);
template <class Fq>
// level = 2^c * mul_m * (level - 1); mul_m = 0 / 1: no small multiple (power-of-two windows)
void launch_precompute_level(hipStream_t st, u32* table, u32 stride, u32 level, u32 c, u32* xyzz_scratch);
// levels 1 .. W - 1 of a small key (plain c-bit windows) from level 0 in two launches; xyzz_scratch: (W - 1) n records
template <class Fq>
void launch_precompute_all_levels(hipStream_t st, u32* table, u32 n, u32 c, u32 W, u32* xyzz_scratch);
// Direct sum (msm_kernels.h k_direct_sum): the 512-points-per-generator table of a small key from its window table (W levels of
// plain c-bit windows, device radix), built in slabs of `slab_windows` of its 64 four-bit windows (xyzz_scratch: 8 * slab_windows * n
// records), and one MSM as cdiv(n * 64 / m, 256) partial records (returned) for launch_fold
template <class Fq>
void launch_ds_table(hipStream_t st, const u32* win_table, u32 n, u32 c, u32 W, u32* xyzz_scratch, u32 slab_windows, u32* table);
// nv <= DS_BATCH MSMs over the key in one launch: MSM v's `blocks` records (the return value, sized by the longest vector) at
// partials[v * blocks ...].  group_shift >= 0 (nv = 1): two sums by that bit of the scalar's index (n a multiple of
// 2 << group_shift): class c's `blocks` records are partials[c * blocks ...]
template <class Fq>
u32 launch_direct_sum(hipStream_t st, const u32* table, u32 key_n, u32 nv, const u32* const* scalars, const u32* ns, const u32* base_offs,
                      int mont, u32 m, int group_shift, u32* flags, u32* partials);
template <class Fq>
void launch_apply_inf(hipStream_t st, u32* table, const uint8_t* is_inf, u32 n);
template <class Fq>
void launch_generate_bases(hipStream_t st, u32* table, u64 seed, u32 first, u32 n, const u32* gen_xy_mont);
// Transparent keys (sample_kernels.h).  One SEARCH pass gives every listed index (pend_in: n_in words (attempt << 32 | t); null: t =
// 0 .. n_in - 1 from attempt 0) up to `max_tests` square tests: a winner leaves its attempt in jwin[t] and its candidate in table[t],
// a loser is appended to pend_out (counters[SAMPLE_CNT_PENDING]) with its next attempt.  FINISH turns the candidates into the points
// G_(first + t), in the device radix.
template <class Fq>
void launch_sample_search(hipStream_t st, u32* table, u32* jwin, const u64* pend_in, u32 n_in, u64* pend_out, u32* counters,
                          const SampleConsts& k, u64 first, u32 max_tests);
template <class Fq>
void launch_sample_finish(hipStream_t st, u32* table, u32* jwin, u32 n, u32* counters, const SampleConsts& k, u64 first);

// Point validation (points_check_kernels.h; include/amsm.h: amsm_points_check): status[i] (n bytes, every one written) of the n points
// at xy (C-ABI radix; is_inf: their infinity bytes or null), the counts of status 1, 2, 3 added to counters[0..2] and the smallest bad
// index min-ed into counters[PCHK_FIRST_BAD].  Two launches where the curve needs the subgroup test; ladder: 1 or 2, its shape.
template <class Fq>
void launch_points_check(hipStream_t st, const u32* xy, const uint8_t* is_inf, u32 n, uint8_t* status, u32* counters,
                         const PointsCheckConsts& k, int ladder);

// The device may keep points in an internal Montgomery radix (fpu.h): key tables, partials and buckets are in it,
// everything the C ABI exposes is not.  import/export convert a point array (src may equal dst); they do
// nothing when device_internal_radix<Fq>() is false.
template <class Fq>
bool device_internal_radix();
template <class Fq>
void launch_points_import(hipStream_t st, const u32* src, u32* dst, u32 n);
template <class Fq>
void launch_points_export(hipStream_t st, const u32* src, u32* dst, u32 n);

// xyzz_scratch (n XYZZ records, may be null): large folds / precompute levels leave their sums there and convert them to
// affine in a second kernel with one inversion per few points (batch_affine_pays(n) says when the scratch is used)
template <class Fq>
bool batch_affine_pays(u32 n);
// out[i] = l[i] + x r[i], i < n, with x as the caller recoded it (host_glv.h: fold_digits -- glv is what it returned; the scalar is
// where the entry point is, api_entry_vec.inc, and so is its recoding: these units only launch).  abi_radix: l, r and out are
// caller-visible buffers in the C ABI's radix, else key tables in the device's.
template <class Fq>
void launch_points_fold(hipStream_t st, const u32* l, const u32* r, u32 n, const FoldDigits& d, bool glv, u32* out, bool abi_radix,
                        u32* xyzz_scratch);

// Fold of a key that carries window multiples (table level w at w * stride points, = 2^(e_w) G with e_w =
// window_exponent_of(c, W, n_narrow, 0, w)): out[i] = table[i] + x * table[n + i], i < n, by the additions fold_recode.h: fold_tab_ops
// listed -- which refuses an x that does not fit the usable levels; the caller then takes launch_points_fold.
template <class Fq>
void launch_points_fold_tab(hipStream_t st, const u32* table, u32 stride, u32 n, const FoldTabOps& ops, u32* out, u32* xyzz_scratch);

// two-valued vectors (vec_kernels.h k_tv_probe, msm_kernels.h k_tv_sum): exact probe into TV_PROBE_WORDS zeroed words, and the
// sum of the generators with non-zero scalars as `blocks` partial records
// out_words: TV_PROBE_WORDS words, zeroed; one: the unit scalar as the vector stores it (word 4 of the output counts how many of
// TV_ONES_SAMPLE_COUNT evenly spaced scalars equal it)
constexpr u32 TV_ONES_SAMPLE_COUNT = 1024;
void launch_tv_probe(hipStream_t st, const u32* scalars, u32 n, u32* out_words, const u32 one[8]);
// nv <= 8 vectors in one launch: vector v's `blocks` partial records at parts + v * blocks, its exception records (8 slots of
// 8 + 2 W words: scalar | generator in the C-ABI radix) at exc + v * 8 slots; probes[v] = the vector's k_tv_probe words
template <class Fq>
void launch_tv_sum(hipStream_t st, const u32* table, u32 nv, const u32* const* scalars, const u32* const* probes, const u32* ns,
                   const u32* base_offs, u32 blocks, u32* parts, u32* exc);
constexpr u32 TV_PROBE_WORDS = 32, TV_EXC_SLOTS = 8;  // == TV_WORDS / TV_EXC_MAX of vec_kernels.h

// ---- scalar-field (Fr) launchers ----------------------------------------------------------------
template <class Fr>
void launch_digits(hipStream_t st, const u32* scalars, int mont, MsmGeom g, void* keys, bool keys16, u32* vals, u32* err);
// Custom prep chain (prep_kernels.h): scalars -> sorted entry list + bucket table in 7 dispatches.  d_small holds
// prep_small_words(g) words (partition totals, starts, cursors, partial counts, the heavy-partition tables); the launcher
// zeroes what needs it.  The geometry of the three chains -- what they support, their partitions, strides and buffer needs -- is
// prep_geom.h's.
struct PrepBuffers {
  u32* d_small;       // >= prep_small_words(g) words (+ 256 bytes of slack), directly behind the 16 words at `err`
  u32* part;          // E words: entries grouped by partition
  u32* vals_sorted;   // E + 16 words
  u32* start;         // B + 2 words
  u32* items;         // B + 2 words
  u32* item_off;      // B + 2 words
  u32* err;           // == d_small - 16: the MSM's flag words, cleared by the same fill
};
// Bucket-per-lane prep (prep_kernels.h: hist, scan, wide scatter, k_prep_local_t): 4 dispatches + the fill
struct PrepBplBuffers {
  u32* d_small;   // as PrepBuffers
  u32* part;      // 2 * E words: 64-bit interchange entries
  u32* ents_t;    // P * stride words: the transposed entry blocks (prep_bpl_stride / prep_bps_stride entries per partition)
  void* grp;      // partitions x prep_bpl_groups_per_partition() group headers (8 bytes each)
  u32* order;     // 64 words per group: the bucket every lane slot sums
  u32* err;       // == d_small - 16; err[1] = overflow (the host falls back to the chunked pipeline)
};
template <class Fr>
int launch_prep_bpl(hipStream_t st, const u32* scalars, int mont, MsmGeom g, const PrepBplBuffers& b);
// Bucket-split prep for small / medium MSMs (prep_kernels.h: k_prep_local_s): every bucket on 2^log2_l adjacent lanes.
// log2_l: prep_bps_choose(g).
template <class Fr>
int launch_prep_bps(hipStream_t st, const u32* scalars, int mont, MsmGeom g, u32 log2_l, const PrepBplBuffers& b);
template <class Fq>
void launch_accum_bps(hipStream_t st, const u32* table, const u32* ents_t, const void* grp, const u32* order, u32 n_groups,
                      u32 log2_l, const u32* flags, u32* buckets);
// A unit of nv <= msel::BPS_BATCH bucket-split MSMs that share one geometry (msm_select.h: batch_units), one launch per stage with
// grid.y = MSM.  MSM v's buffers sit v strides behind MSM 0's; the strides are at least what one MSM needs (PrepBplBuffers).
struct BpsBatchBuffers {
  u32* small;        // nv blocks of small_stride words: 16 flag words (block 0's are the unit's: err) and the MSM's small arrays
  u32 small_stride;  // >= prep_bps_small_block_words(), a multiple of 64 (ONE fill clears all nv blocks)
  u32* part;         // interchange entries
  u32 part_stride;   // words
  u32* ents_t;       // entry blocks
  u32 ents_stride;   // words
  void* grp;         // group headers
  u32 grp_stride;    // headers (8 bytes each)
  u32* order;        // bucket order
  u32 order_stride;  // words
};
// the fill, the scatter and the local sort of the whole unit: three commands
template <class Fr>
int launch_prep_bps_batch(hipStream_t st, const u32* const* scalars, u32 nv, int mont, MsmGeom g, u32 log2_l, const BpsBatchBuffers& b);
// buckets: MSM v's g.B records at v * g.B (one contiguous table of nv * g.n_sets sets for the unit's one tail)
template <class Fq>
void launch_accum_bps_batch(hipStream_t st, const u32* table, const BpsBatchBuffers& b, u32 nv, u32 n_groups, u32 log2_l, u32 n_buckets,
                            u32* buckets);
template <class Fr>
int launch_prep(hipStream_t st, const u32* scalars, int mont, MsmGeom g, const PrepBuffers& b);

// *d_flag (zeroed by the caller) = 1 when the vector's c-bit digits look skewed (vec_kernels.h: k_skew_probe)
template <class Fr>
void launch_skew_probe(hipStream_t st, const u32* scalars, int mont, u32 n, DigitWalk walk, u32* d_flag,
                       const u32* d_tv_words = nullptr);
template <class Fr>
void launch_vec_random(hipStream_t st, u32* out, u64 seed, u32 n, int mont);
// amsm_vec_sample (vec_kernels.h: k_vec_sample).  form: 0 the form that ships (VEC_SAMPLE_TILE), 1 / 2 tiles of 1024 / 4096 scalars
// (the A/B of tools/vec_sample_rates.py) -- the same values from every form
constexpr u32 VEC_SAMPLE_TILE = 1024;
template <class Fr>
void launch_vec_sample(hipStream_t st, u32* out, const blind::Key& key, u32 curve_id, u32 stream, u64 first, u32 n, int mont, int form);
// Grids of the grid-stride Fr kernels (256-lane workgroups), the ONE place they are computed: the launchers below, the callers that
// size partial-sum buffers by `blocks`, and amsm_ctx_vec_grid all call these two.  cus: the CUs of the context's device; max_wg:
// amsm_ctx_set_vec_grid_max (0: none) -- a further upper bound, so that a test reaches the loops' second pass at a small n.
struct VecGrid {
  u32 cus;
  u32 max_wg;
};
// streaming kernels (k_vec_hadamard, k_vec_combine, k_hp_t_vecs): enough workgroups to fill the wave slots a few times over, not one
// per 256 elements beyond that (64 per CU: one element per lane up to 2^22 elements on 256 CUs; round 2, 2^22 elements: 64 -> 0.57-0.79
// of 8 TB/s, 8 -> 0.52-0.75)
inline u32 vec_stream_grid(u32 n, VecGrid vg) {
  constexpr u32 per_cu = 64;
  u32 g = std::max(1u, std::min((n + 255u) / 256u, std::max(1u, vg.cus) * per_cu));
  return vg.max_wg ? std::min(g, vg.max_wg) : g;
}
// block-reduction kernels (k_vec_inner_product, k_vec_inner_product_pair, k_ipa_fold_ip): one partial sum per workgroup, folded on the host
inline u32 vec_reduce_grid(u32 n, VecGrid vg) {
  u32 g = std::min<u32>(1024u, (n + 255u) / 256u);
  return vg.max_wg ? std::min(g, vg.max_wg) : g;
}
template <class Fr>
void launch_vec_hadamard(hipStream_t st, VecGrid vg, const u32* a, const u32* b, u32* out, u32 n);
template <class Fr>
void launch_vec_combine(hipStream_t st, VecGrid vg, const CombineArgs& a, u32* out);
template <class Fr>
void launch_hp_t_vecs(hipStream_t st, VecGrid vg, const TVecArgs& a, int n_inputs);

template <class Fr>
void launch_spmv(hipStream_t st, const u32* row_ptr, const u32* col, const u32* val, const u32* input, u32 n_input,
                 const u32* witness, u32 n_witness, u32* out, u32 n_rows);

template <class Fr>
void launch_vec_powers(hipStream_t st, const u32 point_mont[8], u32 n, u32* out);
// Polynomial division by (X - z) / evaluation over up to POLY_MAX polynomials (vec_kernels.h: k_poly_*; grid.y = polynomial).
// tile_values: out[a.off[k] + b] = value of tile b (eval: times point^(b POLY_T)); carries: `a` describes the polynomials of tile
// values; div_tiles: the quotients (and a.rem) from the carries.
template <class Fr>
void launch_poly_tile_values(hipStream_t st, const PolyArgs& a, u32 n_polys, u32 max_tiles, bool eval, u32* out);
template <class Fr>
void launch_poly_carries(hipStream_t st, const PolyArgs& a, u32 n_polys);
template <class Fr>
void launch_poly_div_tiles(hipStream_t st, const PolyArgs& a, u32 n_polys, u32 max_tiles, const u32* carries);
template <class Fr>
void launch_vec_inner_product(hipStream_t st, const u32* a, const u32* b, u32 n, u32 blocks, u32* out);
template <class Fr>
void launch_vec_inner_product_pair(hipStream_t st, const u32* a0, const u32* b0, const u32* a1, const u32* b1, u32 n,
                                   u32 blocks, u32* out);
// in-place fold of c and z (2 * 2 * half elements -> 2 * half) + the two inner products of the folded halves
template <class Fr>
void launch_ipa_fold_ip(hipStream_t st, u32* c, u32* z, u32 half, const u32 x_mont[8], const u32 xinv_mont[8], u32 blocks,
                        u32* out);
template <class Fr>
void launch_ipa_round_scalars(hipStream_t st, const u32* xi_mont, u32 j, u32 log_n, const u32* c, u32* out_l, u32* out_r);
template <class Fr>
void launch_check_poly_coeffs(hipStream_t st, const u32* xi_mont, u32 k, u32* out);
void launch_vec_fill(hipStream_t st, u32* out, const u32 value[8], u32 n);
// the two flag words of an MSM slot (scalar-range error, prep overflow) into page-locked host memory: what k_fold's mirror does
// for an MSM with a tail, for a range that leaves its sums in a shared bucket set and has none (api_pipeline.inc: Share)
void launch_mirror_flags(hipStream_t st, const u32* flags, u32* host_mirror);
void launch_bounds(hipStream_t st, const void* keys_sorted, bool keys16, u32* vals_sorted, MsmGeom g, u32* start, u32* items);

}  // namespace amsm
