"""Plain keys on the bucket-per-lane pipeline with 2, 4 or 8 bucket sets for their top window (csrc/msm_select.h: plain_top_sets,
csrc/msm_types.h: window_set, AMSM_TOP_SETS): the shapes that ran chunked while the top window had two sets -- 2^20 pairs on BN254,
Grumpkin and BLS12-377, 786 432 on BLS12-377 --, every forced count at the smallest shapes that take the form, grouped MSMs whose
group bit lies inside, at the edge of and above the bits that pick the top set, empty and lopsided top sets, and one MSM cut into a
range with four sets and one with two.

No big oracle: a generated key has G_i = k_i G with k_i = rng_scalar(seed, i) (restated with numpy in tests/curve_rows.py), so
sum s_i G_i = (sum s_i k_i mod r) G, one scalar multiplication in Python.  tests/test_top_sets_cpu.py pins the rule without a GPU."""
import numpy as np
import pytest

from oracle import pyref as o
from tests import helpers as h
from tests.curve_rows import edge_scalars, ints, mults  # (the multiplier stream of generated keys is the same on every curve)

pytestmark = pytest.mark.gpu

SEED = 0x5EED70B5
PLAIN = 2  # AMSM_BASES_NO_PRECOMPUTE
CURVES = {c.name: c for c in (o.PALLAS, o.BLS12_381_G1, h.BN254, h.GRUMPKIN, h.BLS12_377)}


def expect(c, mult, scalars):
    return o.mul(c, sum(a * b for a, b in zip(scalars, mult)) % c.r, o.generator(c))


def make_ctx(c, monkeypatch, top_sets=None):
    from accumulation_amd import Context
    with monkeypatch.context() as m:  # (the context reads its switches when it is made)
        if top_sets is None:
            m.delenv("AMSM_TOP_SETS", raising=False)
        else:
            m.setenv("AMSM_TOP_SETS", str(top_sets))
        return Context(c.curve_id)


def uniform(ctx, seed, n):
    v = ctx.random_vector(seed, n, False)
    sc = ints(v.download())
    v.free()
    return sc


def msm(ctx, ck, sc):
    """-> (affine point, the pipeline counters that moved, the top-set counters that moved)"""
    from accumulation_amd import VariableBaseMSM
    v = ctx.upload(h.scalars_to_np(sc))
    before, tb = ctx.pipeline_stats(), ctx.top_sets_stats()
    xy, inf = VariableBaseMSM.multi_scalar_mul(ck, v, mont=False)
    moved = {k: x - before[k] for k, x in ctx.pipeline_stats().items() if x != before[k]}
    tops = {k: x - tb[k] for k, x in ctx.top_sets_stats().items() if x != tb[k]}
    v.free()
    return (np.array(xy), bool(inf)), moved, tops


# ---- 1. the shapes that needed more than two top sets ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", [("bn254_g1", 1 << 20), ("grumpkin", 1 << 20), ("bls12_377_g1", 1 << 20), ("bls12_377_g1", 786432)])
def test_long_plain_keys_take_the_bucket_per_lane_pipeline(built_lib, monkeypatch, name, n):
    """uniform scalars with the curve's edge scalars over the first and last lanes: the MSM is ONE bucket-per-lane MSM (four top
    sets by the rule: tests/test_top_sets_cpu.py), no fallback re-runs it, and the point is the oracle's.  With two top sets these
    shapes expected 43 338 (BN254 / Grumpkin), 56 170 and 42 128 (BLS12-377) entries in a partition of the top window against a stage
    of 37 340 and ran chunked: moved == {}."""
    from accumulation_amd import CommitterKey
    c = CURVES[name]
    ctx = make_ctx(c, monkeypatch)
    try:
        ck = CommitterKey.generate(ctx, SEED, n, PLAIN)
        assert not ck.precomputed
        sc, edge = uniform(ctx, 31, n), edge_scalars(c)
        sc[:len(edge)] = edge
        sc[n - len(edge):] = edge
        res, moved, tops = msm(ctx, ck, sc)
        print(name, n, "moved", moved, "top sets", tops)
        assert moved == {"bucket_per_lane": 1}, (name, n, moved)
        assert tops == {4: 1}
        assert h.np_to_point(c, *res) == expect(c, mults(SEED, n), sc)
        ck.free()
    finally:
        ctx.close()


# ---- 2. every forced count at the smallest shapes that take the form ---------------------------------------------------------------------
_two_sets = {}


def two_sets_case(monkeypatch, name, n):
    """(scalars, the AMSM_TOP_SETS=2 context's result, the oracle's point) for (curve, n): computed once for the module"""
    from accumulation_amd import CommitterKey
    if (name, n) not in _two_sets:
        c = CURVES[name]
        ctx = make_ctx(c, monkeypatch, 2)
        try:
            ck = CommitterKey.generate(ctx, SEED, n, PLAIN)
            sc = uniform(ctx, 37, n)
            sc[0], sc[1], sc[2], sc[n - 1] = 0, 1, c.r - 1, c.r - 2
            res, moved, tops = msm(ctx, ck, sc)
            assert moved == {"bucket_per_lane": 1} and tops == {2: 1}, (name, n, moved, tops)
            ck.free()
        finally:
            ctx.close()
        _two_sets[(name, n)] = (sc, res, expect(c, mults(SEED, n), sc))
    return _two_sets[(name, n)]


@pytest.mark.parametrize("n", [(1 << 17) + 1, (1 << 18) + 1], ids=["15_bit_windows", "16_bit_windows"])
@pytest.mark.parametrize("name", ["pallas", "bls12_381_g1", "bls12_377_g1"])
@pytest.mark.parametrize("top_sets", [4, 8])
def test_forced_top_sets_give_the_same_point(built_lib, monkeypatch, top_sets, name, n):
    from accumulation_amd import CommitterKey
    c = CURVES[name]
    sc, res2, want = two_sets_case(monkeypatch, name, n)
    ctx = make_ctx(c, monkeypatch, top_sets)
    try:
        ck = CommitterKey.generate(ctx, SEED, n, PLAIN)
        res, moved, tops = msm(ctx, ck, sc)
        assert moved == {"bucket_per_lane": 1} and tops == {top_sets: 1}, (moved, tops)
        assert res[1] == res2[1] and np.array_equal(res[0], res2[0])
        assert h.np_to_point(c, *res) == want
        ck.free()
    finally:
        ctx.close()


# ---- 3. grouped: the bit that picks the group never picks the top set --------------------------------------------------------------------
def test_grouped_msm_with_eight_top_sets(built_lib, monkeypatch):
    """multi_scalar_mul_grouped over a plain key of 2^18 + 2 pairs, AMSM_TOP_SETS=8: group bit 0, 1, 2 (inside the three bits that
    pick the top set: squeezed out of them) and 17 (above them) -- both sums against the oracle and the two-set context's"""
    from accumulation_amd import CommitterKey, VariableBaseMSM
    c, n = h.BLS12_377, (1 << 18) + 2
    mult, out = mults(SEED, n), {}
    for top_sets in (2, 8):
        ctx = make_ctx(c, monkeypatch, top_sets)
        try:
            ck = CommitterKey.generate(ctx, SEED, n, PLAIN)
            if top_sets == 2:
                sc = uniform(ctx, 41, n)
                sc[0], sc[1], sc[n - 1] = c.r - 1, 1, c.r - 2
            v = ctx.upload(h.scalars_to_np(sc))
            for shift in (0, 1, 2, 17):
                before, tb = ctx.pipeline_stats(), ctx.top_sets_stats()
                pts, infs = VariableBaseMSM.multi_scalar_mul_grouped(ck, v, shift, mont=False)
                st, ts = ctx.pipeline_stats(), ctx.top_sets_stats()
                assert st["bucket_per_lane"] - before["bucket_per_lane"] == 1 and st["fallbacks"] == before["fallbacks"], shift
                assert ts[top_sets] - tb[top_sets] == 1, (shift, ts)
                out[(top_sets, shift)] = [(np.array(pts[g]), bool(infs[g])) for g in (0, 1)]
            v.free()
            ck.free()
        finally:
            ctx.close()
    for shift in (0, 1, 2, 17):
        for g in (0, 1):
            a, b = out[(2, shift)][g], out[(8, shift)][g]
            assert a[1] == b[1] and np.array_equal(a[0], b[0]), (shift, g)
            cls = [s if ((i >> shift) & 1) == g else 0 for i, s in enumerate(sc)]
            assert h.np_to_point(c, *b) == expect(c, mult, cls), (shift, g)


# ---- 4. empty and lopsided top sets -------------------------------------------------------------------------------------------------------
def test_empty_and_lopsided_top_sets(built_lib, monkeypatch):
    """AMSM_TOP_SETS=4 on BN254, 2^18 + 1 pairs (16-bit windows, the top one at bit 240).
    Scalars below 2^239: window 14 never carries, every top set stays empty (the identity) and nothing is skewed -- one bucket-per-lane
    MSM, no fallback, the sum exact.
    Scalars below 2^128: the top sets are empty as well and the sum is exact; here the recoding's carry out of window 7 puts half the
    scalars into bucket 1 of window 8, which is skew whatever the top window owns -- the prep's overflow flag may send the MSM to the
    chunked re-run (at most one fallback).
    Scalars non-zero only at indices that are 1 mod 4: ONE top set carries the whole top window -- it fits, or the overflow flag sends
    the MSM to the chunked re-run (at most one fallback); the sum is exact either way."""
    from accumulation_amd import CommitterKey
    c, n = h.BN254, (1 << 18) + 1
    mult = mults(SEED, n)
    ctx = make_ctx(c, monkeypatch, 4)
    try:
        ck = CommitterKey.generate(ctx, SEED, n, PLAIN)
        full = uniform(ctx, 43, n)
        below = [s & ((1 << 239) - 1) for s in full]
        res, moved, tops = msm(ctx, ck, below)
        print("below 2^239", moved, tops)
        assert moved == {"bucket_per_lane": 1} and tops == {4: 1}, (moved, tops)
        assert h.np_to_point(c, *res) == expect(c, mult, below)
        for name, sc in (("below 2^128", [s & ((1 << 128) - 1) for s in full]), ("1 mod 4", [s if i % 4 == 1 else 0 for i, s in enumerate(full)])):
            res, moved, tops = msm(ctx, ck, sc)
            print(name, moved, tops)
            assert moved.pop("bucket_per_lane") == 1 and moved.pop("fallbacks", 0) <= 1 and moved == {} and tops == {4: 1}, (name, moved, tops)
            assert h.np_to_point(c, *res) == expect(c, mult, sc), name
        ck.free()
    finally:
        ctx.close()


# ---- 5. one MSM longer than a range -------------------------------------------------------------------------------------------------------
def test_msm_cut_into_a_range_with_four_sets_and_one_with_two(built_lib, monkeypatch):
    """BN254, 2^20 + 2^18 + 1 pairs over a plain key: a range of 2^20 pairs (four top sets) and one of 2^18 + 1 (two)"""
    from accumulation_amd import CommitterKey
    c, n = h.BN254, (1 << 20) + (1 << 18) + 1
    ctx = make_ctx(c, monkeypatch)
    try:
        ck = CommitterKey.generate(ctx, SEED, n, PLAIN)
        sc = uniform(ctx, 47, n)
        sc[0], sc[(1 << 20) - 1], sc[1 << 20], sc[n - 1] = c.r - 1, c.r - 2, c.r - 1, 1
        res, moved, tops = msm(ctx, ck, sc)
        assert moved == {"bucket_per_lane": 2} and tops == {4: 1, 2: 1}, (moved, tops)
        assert h.np_to_point(c, *res) == expect(c, mults(SEED, n), sc)
        ck.free()
    finally:
        ctx.close()
