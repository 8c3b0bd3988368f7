"""Bucket-split MSMs of one call that differ in their scalars only run as UNITS of 2 .. 8: one fill, one scatter, one local sort and one
accumulation with grid.y = MSM, one tail over the unit's bucket sets (msm_select.h: batch_units; api_pipeline.inc:
msm_enqueue_bps_batch; k_prep_scatter_batch, k_prep_local_s_batch, k_accum_bps_batch).  Every result against the C oracle bit for bit
(BN254, which that oracle does not know: against the multiplier stream of the generated key, as tests/test_bn254_gpu.py does) and
against the same vector's single call; the counters say which path ran.  2^16 pairs is the smallest size at which the path exists."""
import os

import numpy as np
import pytest

from oracle import pyref as o
from tests import helpers as h

pytestmark = pytest.mark.gpu

N16 = 1 << 16
KEY_SEED, VEC_SEED, OFF = 0xB5B0, 0xB5C0, 500
NEW = ("bucket_split_units", "bucket_split_batched", "bucket_split_unit_reruns")


def make_ctx(curve_id, **env):
    from accumulation_amd import Context
    before = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return Context(curve_id)
    finally:
        for k, old in before.items():  # (a value the caller's environment already had comes back)
            if old is None:
                del os.environ[k]
            else:
                os.environ[k] = old


def delta(before, after):
    return {k: after[k] - before[k] for k in after}


_ORACLE = {}


def oracle(cref, curve_id, key_seed, xy, off, seed, n):
    """the C oracle's MSM of rng_scalars(seed, n) over xy[off:off + n], computed once per module"""
    k = (curve_id, key_seed, off, seed, n)
    if k not in _ORACLE:
        _ORACLE[k] = cref.msm(curve_id, xy[off:off + n], cref.rng_scalars(seed, n), threads=8)
    return _ORACLE[k]


@pytest.mark.parametrize("V", [2, 3, 8, 9])
def test_units_of_uniform_vectors_vs_c_oracle_and_single_calls(cref, V):
    from accumulation_amd import CommitterKey, VariableBaseMSM
    c = o.PALLAS
    ctx = make_ctx(c.curve_id)
    try:
        ck = CommitterKey.generate(ctx, KEY_SEED, N16 + 1000)
        xy, _ = ck.read()
        vecs = [ctx.upload(cref.rng_scalars(VEC_SEED + v, N16)) for v in range(V)]
        before = ctx.pipeline_stats()
        out, inf = VariableBaseMSM.multi_scalar_mul_batch(ck, vecs, mont=False, base_off=OFF)
        d = delta(before, ctx.pipeline_stats())
        print("V", V, "counters", d)
        for v in range(V):
            ref, rinf = oracle(cref, c.curve_id, KEY_SEED, xy, OFF, VEC_SEED + v, N16)
            assert bool(inf[v]) == bool(rinf) and np.array_equal(out[v], ref), v
            one, oinf = VariableBaseMSM.multi_scalar_mul(ck, vecs[v], base_off=OFF)
            assert bool(oinf) == bool(rinf) and np.array_equal(one, out[v]), v
        # V = 9: a unit of eight and a single, which counts in neither new counter
        assert d["bucket_split"] == V and d["bucket_split_batched"] == min(V, 8) and d["bucket_split_units"] == 1
        assert d["bucket_split_fallbacks"] == 0 and d["bucket_split_unit_reruns"] == 0
        ck.free()
    finally:
        ctx.close()


def _bn254_case(ctx, n, seeds, cref):
    from accumulation_amd import CommitterKey
    from tests.curve_rows import expect, ints, mults
    ck = CommitterKey.generate(ctx, KEY_SEED, n)
    mult = mults(KEY_SEED, n)
    scs = [cref.rng_scalars(s, n) for s in seeds]
    return ck, scs, [expect(h.BN254, mult, ints(sc)) for sc in scs], lambda xy, inf: h.np_to_point(h.BN254, xy, inf)


@pytest.mark.parametrize("curve,n", [("pallas", N16 + 12345), ("bls12_381_g1", N16 + 12345), ("bn254_g1", N16 + 12345), ("pallas", 1 << 17)])
def test_the_three_field_shapes_and_the_upper_edge(cref, curve, n):
    """28-bit limbs x 9 (Pallas), 14 x 28 with 192-byte records (BLS12-381 G1), the general 9 x 29 (BN254 G1); 2^17 pairs: the largest unit size"""
    from accumulation_amd import CommitterKey, VariableBaseMSM, ffi
    V, seeds = 3, [VEC_SEED + 16 + v for v in range(3)]
    if curve == "bn254_g1":
        ctx = make_ctx(ffi.AMSM_BN254_G1)
        try:
            ck, scs, want, to_point = _bn254_case(ctx, n, seeds, cref)
            before = ctx.pipeline_stats()
            out, inf = VariableBaseMSM.multi_scalar_mul_batch(ck, [ctx.upload(s) for s in scs], mont=False)
            d = delta(before, ctx.pipeline_stats())
            for v in range(V):
                assert to_point(out[v], inf[v]) == want[v], v
            assert (d["bucket_split"], d["bucket_split_batched"], d["bucket_split_units"], d["bucket_split_fallbacks"]) == (V, V, 1, 0)
            ck.free()
        finally:
            ctx.close()
        return
    c = o.PALLAS if curve == "pallas" else o.BLS12_381_G1
    ctx = make_ctx(c.curve_id)
    try:
        ck = CommitterKey.generate(ctx, KEY_SEED + 1, n)
        xy, _ = ck.read()
        before = ctx.pipeline_stats()
        out, inf = VariableBaseMSM.multi_scalar_mul_batch(ck, [ctx.upload(cref.rng_scalars(s, n)) for s in seeds], mont=False)
        d = delta(before, ctx.pipeline_stats())
        for v in range(V):
            ref, rinf = oracle(cref, c.curve_id, KEY_SEED + 1, xy, 0, seeds[v], n)
            assert bool(inf[v]) == bool(rinf) and np.array_equal(out[v], ref), v
        assert (d["bucket_split"], d["bucket_split_batched"], d["bucket_split_units"], d["bucket_split_fallbacks"]) == (V, V, 1, 0)
        ck.free()
    finally:
        ctx.close()


def test_ranges_of_a_key_with_a_20_bit_table_run_over_its_twin(cref):
    """2^19 + 1 generators: the smallest key that gets the 20-bit table; ranges of 2^16 pairs of it take the bucket-split pipeline over
    the 17-bit twin (built on first use) -- three of them as one unit"""
    from accumulation_amd import CommitterKey, VariableBaseMSM, ffi
    c = o.PALLAS
    ctx = make_ctx(c.curve_id)
    try:
        ck = CommitterKey.generate(ctx, KEY_SEED + 2, (1 << 19) + 1, ffi.AMSM_BASES_PRECOMPUTE)
        assert ck.window_bits == 20
        xy, _ = ck.read(OFF, N16)
        seeds = [VEC_SEED + 32 + v for v in range(3)]
        before = ctx.pipeline_stats()
        out, inf = VariableBaseMSM.multi_scalar_mul_batch(ck, [ctx.upload(cref.rng_scalars(s, N16)) for s in seeds], mont=False, base_off=OFF)
        d = delta(before, ctx.pipeline_stats())
        for v in range(3):
            ref, rinf = cref.msm(c.curve_id, xy, cref.rng_scalars(seeds[v], N16), threads=8)
            assert bool(inf[v]) == bool(rinf) and np.array_equal(out[v], ref), v
        assert (d["bucket_split"], d["bucket_split_batched"], d["bucket_split_units"], d["bucket_per_lane"]) == (3, 3, 1, 0)
        assert ck.memory()["twin"] > 0
        ck.free()
    finally:
        ctx.close()


def test_mixed_lists_stay_correct(cref):
    """lengths [2^16, 2^16, 2^15, 2^16, 2^16 + 1, 2^16 + 1]: units {0, 1}, single (chunked), single, {4, 5}; results in caller order"""
    from accumulation_amd import CommitterKey, VariableBaseMSM
    c = o.PALLAS
    ctx = make_ctx(c.curve_id)
    try:
        lens = [N16, N16, 1 << 15, N16, N16 + 1, N16 + 1]
        ck = CommitterKey.generate(ctx, KEY_SEED + 3, N16 + 1)
        xy, _ = ck.read()
        jobs = [(0, ctx.upload(cref.rng_scalars(VEC_SEED + 48 + j, n))) for j, n in enumerate(lens)]
        before = ctx.pipeline_stats()
        out, inf = VariableBaseMSM.multi_scalar_mul_multi(ck, jobs, mont=False)
        d = delta(before, ctx.pipeline_stats())
        for j, n in enumerate(lens):
            ref, rinf = oracle(cref, c.curve_id, KEY_SEED + 3, xy, 0, VEC_SEED + 48 + j, n)
            assert bool(inf[j]) == bool(rinf) and np.array_equal(out[j], ref), j
        assert (d["bucket_split"], d["bucket_split_batched"], d["bucket_split_units"], d["bucket_split_fallbacks"]) == (5, 4, 2, 0)
        ck.free()
    finally:
        ctx.close()


def test_a_skewed_vector_in_a_unit_sends_every_msm_of_it_through_the_single_path(cref):
    """Without the digit probe (and without the two-valued shortcut, which would take a constant vector out of the call) the constant
    middle vector joins the unit and every prep of the unit overflows on it: the unit's MSMs run again one by one, the uniform ones
    on the bucket-split pipeline, the constant one chunked -- counted as a fallback once, and no MSM counted twice."""
    from accumulation_amd import CommitterKey, VariableBaseMSM
    c = o.PALLAS
    const = np.tile(h.scalars_to_np([o.rng_scalar(24, 0)]), (N16, 1))
    want = {}
    for env, expect in (
            (dict(AMSM_BPL_PROBE=0, AMSM_TWO_VALUED=0), dict(bucket_split=3, bucket_split_batched=3, bucket_split_units=1,
                                                              bucket_split_unit_reruns=1, bucket_split_fallbacks=1)),
            # the probe (default) marks the constant vector: it never joins a unit, its neighbours are singles
            (dict(AMSM_TWO_VALUED=0), dict(bucket_split=2, bucket_split_batched=0, bucket_split_units=0, bucket_split_unit_reruns=0,
                                           bucket_split_fallbacks=0)),
            # all defaults: the two-valued form takes it out of the call, the two uniform vectors are adjacent and form a unit
            (dict(), dict(bucket_split=2, bucket_split_batched=2, bucket_split_units=1, bucket_split_unit_reruns=0, bucket_split_fallbacks=0))):
        ctx = make_ctx(c.curve_id, **env)
        try:
            ck = CommitterKey.generate(ctx, KEY_SEED, N16 + 1000)
            if not want:
                xy, _ = ck.read()
                want = {0: oracle(cref, c.curve_id, KEY_SEED, xy, OFF, VEC_SEED, N16), 1: cref.msm(c.curve_id, xy[OFF:OFF + N16], const, threads=8),
                        2: oracle(cref, c.curve_id, KEY_SEED, xy, OFF, VEC_SEED + 1, N16)}
            vecs = [ctx.upload(cref.rng_scalars(VEC_SEED, N16)), ctx.upload(const), ctx.upload(cref.rng_scalars(VEC_SEED + 1, N16))]
            before = ctx.pipeline_stats()
            out, inf = VariableBaseMSM.multi_scalar_mul_batch(ck, vecs, mont=False, base_off=OFF)
            d = delta(before, ctx.pipeline_stats())
            print(env, d)
            for v in range(3):
                assert bool(inf[v]) == bool(want[v][1]) and np.array_equal(out[v], want[v][0]), (env, v)
            assert {k: d[k] for k in expect} == expect, env
            ck.free()
        finally:
            ctx.close()


def test_a_skewed_vector_in_front_does_not_keep_its_neighbours_from_a_unit(cref):
    """[constant, u, u, u] with the digit probe on and the two-valued form off: the probe marks the first vector (chunked, a single);
    the three uniform ones behind it share everything with it but that mark and still form a unit"""
    from accumulation_amd import CommitterKey, VariableBaseMSM
    c = o.PALLAS
    ctx = make_ctx(c.curve_id, AMSM_TWO_VALUED=0)
    try:
        ck = CommitterKey.generate(ctx, KEY_SEED, N16 + 1000)
        xy, _ = ck.read()
        const = np.tile(h.scalars_to_np([o.rng_scalar(24, 0)]), (N16, 1))
        vecs = [ctx.upload(const)] + [ctx.upload(cref.rng_scalars(VEC_SEED + v, N16)) for v in range(3)]
        before = ctx.pipeline_stats()
        out, inf = VariableBaseMSM.multi_scalar_mul_batch(ck, vecs, mont=False, base_off=OFF)
        d = delta(before, ctx.pipeline_stats())
        ref, rinf = cref.msm(c.curve_id, xy[OFF:OFF + N16], const, threads=8)
        assert bool(inf[0]) == bool(rinf) and np.array_equal(out[0], ref)
        for v in range(3):
            ref, rinf = oracle(cref, c.curve_id, KEY_SEED, xy, OFF, VEC_SEED + v, N16)
            assert bool(inf[v + 1]) == bool(rinf) and np.array_equal(out[v + 1], ref), v
        assert (d["bucket_split"], d["bucket_split_batched"], d["bucket_split_units"], d["bucket_split_unit_reruns"]) == (3, 3, 1, 0)
        ck.free()
    finally:
        ctx.close()


def test_a_scalar_out_of_range_in_a_unit_fails_the_call_as_the_single_call_does(cref):
    from accumulation_amd import CommitterKey, VariableBaseMSM, ffi
    c = o.PALLAS
    ctx = make_ctx(c.curve_id)
    try:
        ck = CommitterKey.generate(ctx, KEY_SEED + 6, N16)  # 2^16 generators: 16 signed windows of 16 bits, which cannot take 2^256 - 12345
        assert ck.window_bits == 16
        xy, _ = ck.read()
        bad = cref.rng_scalars(VEC_SEED + 1, N16).copy()
        bad[N16 // 2] = np.array(o.int_to_limbs((1 << 256) - 12345, 4), dtype=np.uint64)  # canonical form (mont=False), >= r
        vecs = [ctx.upload(cref.rng_scalars(VEC_SEED, N16)), ctx.upload(bad), ctx.upload(cref.rng_scalars(VEC_SEED + 2, N16))]
        with pytest.raises(ffi.AmsmError) as single:
            VariableBaseMSM.multi_scalar_mul(ck, vecs[1])
        before = ctx.pipeline_stats()
        with pytest.raises(ffi.AmsmError) as unit:
            VariableBaseMSM.multi_scalar_mul_batch(ck, vecs, mont=False)
        assert unit.value.status == single.value.status == ffi.AMSM_E_SCALAR_RANGE
        assert delta(before, ctx.pipeline_stats())["bucket_split_units"] == 1
        # the flag words were cleared: the next call on the same context succeeds
        out, inf = VariableBaseMSM.multi_scalar_mul_batch(ck, [vecs[0], vecs[2]], mont=False)
        for j, v in enumerate((0, 2)):
            ref, rinf = oracle(cref, c.curve_id, KEY_SEED + 6, xy, 0, VEC_SEED + v, N16)
            assert bool(inf[j]) == bool(rinf) and np.array_equal(out[j], ref), v
        ck.free()
    finally:
        ctx.close()


def test_the_switch_changes_no_byte(cref):
    from accumulation_amd import CommitterKey, VariableBaseMSM
    c = o.PALLAS
    outs = {}
    for cap in (0, 1, 2, 8):
        ctx = make_ctx(c.curve_id, AMSM_BPS_BATCH=cap)
        try:
            ck = CommitterKey.generate(ctx, KEY_SEED, N16 + 1000)
            vecs = [ctx.upload(cref.rng_scalars(VEC_SEED + v, N16)) for v in range(3)]
            before = ctx.pipeline_stats()
            outs[cap] = VariableBaseMSM.multi_scalar_mul_batch(ck, vecs, mont=False, base_off=OFF)
            d = delta(before, ctx.pipeline_stats())
            assert d["bucket_split"] == 3
            assert [d[k] for k in NEW] == {0: [0, 0, 0], 1: [0, 0, 0], 2: [1, 2, 0], 8: [1, 3, 0]}[cap], cap
            ck.free()
        finally:
            ctx.close()
    for cap in (0, 1, 2):
        assert np.array_equal(outs[cap][0], outs[8][0]) and np.array_equal(outs[cap][1], outs[8][1]), cap


def test_boolean_witness_vectors_in_a_unit(cref):
    """10 % unit scalars: summed apart (MsmJob::skip_ones), the rest of both vectors as one unit at 2^17 pairs"""
    from accumulation_amd import CommitterKey, VariableBaseMSM
    c = o.PALLAS
    n = 1 << 17
    ctx = make_ctx(c.curve_id)
    try:
        ck = CommitterKey.generate(ctx, KEY_SEED + 4, n)
        xy, _ = ck.read()
        rng = np.random.default_rng(5)
        scs = []
        for v in range(2):
            s = cref.rng_scalars(VEC_SEED + 64 + v, n).copy()
            pick = rng.random(n) < 0.1
            s[pick] = np.array([1, 0, 0, 0], dtype=np.uint64)
            scs.append(s)
        vecs = [ctx.upload(s) for s in scs]
        singles, moved = [], 0
        for v in range(2):
            b = ctx.pipeline_stats()
            singles.append(VariableBaseMSM.multi_scalar_mul_batch(ck, [vecs[v]], mont=False))
            moved += delta(b, ctx.pipeline_stats())["unit_scalar_sums"]
        before = ctx.pipeline_stats()
        out, inf = VariableBaseMSM.multi_scalar_mul_batch(ck, vecs, mont=False)
        d = delta(before, ctx.pipeline_stats())
        for v in range(2):
            ref, rinf = cref.msm(c.curve_id, xy, scs[v], threads=8)
            assert bool(inf[v]) == bool(rinf) and np.array_equal(out[v], ref), v
            assert np.array_equal(singles[v][0][0], ref)
        assert moved == 2 and d["unit_scalar_sums"] == moved
        assert (d["bucket_split"], d["bucket_split_batched"], d["bucket_split_units"], d["bucket_split_fallbacks"]) == (2, 2, 1, 0)
        ck.free()
    finally:
        ctx.close()


def test_pedersen_commit_batch_with_hiding_randomizers(cref):
    from accumulation_amd import PedersenCommitment
    c = o.PALLAS
    ctx = make_ctx(c.curve_id)
    try:
        ck = PedersenCommitment.setup(ctx, N16, seed=KEY_SEED + 5)
        vecs = [ctx.random_vector(VEC_SEED + 80 + v, N16, mont=True) for v in range(3)]
        rs = [cref.fr_to_mont(c.curve_id, cref.rng_scalars(VEC_SEED + 90 + v, 1))[0] for v in range(3)]
        before = ctx.pipeline_stats()
        got = PedersenCommitment.commit_batch(ck, vecs, rs)
        d = delta(before, ctx.pipeline_stats())
        assert (d["bucket_split_batched"], d["bucket_split_units"]) == (3, 1)
        for v in range(3):
            pt, inf = PedersenCommitment.commit(ck, vecs[v], rs[v])
            assert bool(inf) == bool(got[v][1]) and np.array_equal(pt, got[v][0]), v
        # and one of them against the oracle: commit = MSM over the generators and the hiding generator
        xy, _ = ck.read()
        sc = np.concatenate([cref.fr_from_mont(c.curve_id, vecs[0].download()), cref.fr_from_mont(c.curve_id, rs[0].reshape(1, 4))])
        ref, rinf = cref.msm(c.curve_id, np.concatenate([xy, np.asarray(ck.hiding_generator).reshape(1, -1)]), sc, threads=8)
        assert bool(got[0][1]) == bool(rinf) and np.array_equal(got[0][0], ref)
        ck.free()
    finally:
        ctx.close()
