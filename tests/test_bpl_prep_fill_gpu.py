"""k_prep_local_t at exact fills of its workgroup.  The kernel keeps a partition's entries in per-lane register slots (entry
i * 1024 + t in slot i of lane t), sorts them by bucket in LDS and writes them transposed by whole rows; these vectors set the
number of entries of ONE partition exactly, so that idle lanes, lanes with a single entry, a ragged last slot, empty buckets, the
split halves of the largest buckets and the overflow edges are each hit on purpose.

All MSMs have n = 2^18 + 1 pairs (the shortest range the bucket-per-lane pipeline takes) over a 2^20-generator key with 20-bit
windows.  The vector is zero (zeros emit no entry) except K scalars with values in [1024 p + 1, 1024 p + 1024]: below 2^19, so
only window 0 has a digit, it is positive, and bucket `value - 1` lies in partition p -- partition p holds exactly K entries and
every other partition none.  Every result is compared bit for bit with oracle/ark_msm.c; amsm_ctx_pipeline_stats says which
route ran.  The skew probe is off (AMSM_BPL_PROBE=0): every vector is attempted on the pipeline and only the prep's own overflow
flag sends it to the chunked pipeline.
Replaces ark-ec `VariableBaseMSM::multi_scalar_mul` (ext; call sites src/hp_as/mod.rs:196-214,377)."""
import os

import numpy as np
import pytest

from oracle import pyref as o

pytestmark = pytest.mark.gpu
C = o.PALLAS
KEY_N = 1 << 20
N = (1 << 18) + 1
NB = 1024  # buckets per partition


@pytest.fixture(scope="module")
def env(cref):
    from accumulation_amd import CommitterKey, Context
    os.environ["AMSM_BPL_PROBE"] = "0"
    os.environ["AMSM_TWO_VALUED"] = "0"  # (K equal scalars among zeros are a two-valued vector: they must reach the prep)
    try:
        ctx = Context(C.curve_id)
    finally:
        del os.environ["AMSM_BPL_PROBE"]
        del os.environ["AMSM_TWO_VALUED"]
    ck = CommitterKey.generate(ctx, 0x5EED1001, KEY_N)
    assert ck.precomputed and ck.window_bits == 20
    xy, _ = ck.read()
    yield ctx, ck, xy[:N].copy()
    ck.free()
    ctx.close()


def buckets_spread(k):
    """bucket i mod 1024 for entry i: sizes differ by at most one"""
    return np.arange(k, dtype=np.uint64) % np.uint64(NB)


def buckets_one(k):
    return np.full(k, 517, dtype=np.uint64)


def buckets_staircase(k):
    """bucket b gets b mod 7 entries, bucket after bucket, round after round, until k entries are out: every seventh bucket
    stays empty, the sizes take few distinct values in no order, the last round stops inside the partition"""
    one_round = np.repeat(np.arange(NB, dtype=np.uint64), np.arange(NB) % 7)
    return np.tile(one_round, k // len(one_round) + 1)[:k]


def vector(p, buckets, seed):
    """zeros, except len(buckets) scalars at seeded places: value 1024 p + 1 + bucket"""
    sc = np.zeros((N, 4), dtype=np.uint64)
    where = np.random.default_rng(seed).permutation(N)[:len(buckets)]
    sc[where, 0] = np.uint64(NB * p + 1) + buckets
    return sc


def run(env, cref, sc):
    """the MSM against the oracle; returns (MSMs that took the bucket-per-lane pipeline, fallbacks counted)"""
    from accumulation_amd import VariableBaseMSM
    ctx, ck, xy = env
    before = ctx.pipeline_stats()
    got, inf = VariableBaseMSM.multi_scalar_mul(ck, sc)
    after = ctx.pipeline_stats()
    ref, rinf = cref.msm(C.curve_id, xy, sc, threads=17)
    assert bool(inf) == bool(rinf) and np.array_equal(got, ref)
    return after["bucket_per_lane"] - before["bucket_per_lane"], after["fallbacks"] - before["fallbacks"]


@pytest.mark.parametrize("p", [0, 510])
@pytest.mark.parametrize("k", [1, 63, 64, 65, 1023, 1024, 1025, 2065, 8192])
def test_exact_fill_of_one_partition(env, cref, p, k):
    """K entries in 1024 lanes: all but one lane idle, part of a wave, a wave and one lane, every lane but one, one each, one
    lane with two, a ragged third slot (2065 = 2 x 1024 + 17), eight full slots"""
    took, fell = run(env, cref, vector(p, buckets_spread(k), 1000 * p + k))
    assert took >= 1 and fell == 0, (took, fell)


@pytest.mark.parametrize("p", [0, 510])
@pytest.mark.parametrize("k", [2065, 8192])
def test_staircase_of_bucket_sizes(env, cref, p, k):
    """empty buckets, the size ordering and the padding of each group of 64 lanes to its largest bucket"""
    took, fell = run(env, cref, vector(p, buckets_staircase(k), 2000 * p + k))
    assert took >= 1 and fell == 0, (took, fell)


@pytest.mark.parametrize("p", [0, 510])
@pytest.mark.parametrize("k", [2065, 8192])
def test_one_bucket_takes_every_entry(env, cref, p, k):
    """the size class >= 255 and the split halves: the bucket is cut into halves of ceil(K / 2) and K - ceil(K / 2) entries on two
    lanes of group 0, whose 64 lanes are padded to ceil(K / 2) rows -- 64 x 1033 entries for K = 2065, five times the 13 312
    entries a partition's block holds for this n (kern_fr.hip: prep_bpl_stride), so the prep raises its overflow flag, writes
    no entry, and the MSM is re-run chunked: attempted, fallback counted, exact"""
    took, fell = run(env, cref, vector(p, buckets_one(k), 3000 * p + k))
    assert took >= 1 and fell >= 1, (took, fell)


@pytest.mark.parametrize("k", [10000, 10367, 10368, 10369, 12000])
def test_fills_around_the_fixed_partition_size(env, cref, k):
    """the scatter reserves 10 368 interchange entries per partition for this n (kern_fr.hip: PrepGeom::FIX) and drops what comes
    after; whichever route the counters report, the result is exact"""
    run(env, cref, vector(510, buckets_spread(k), 4000 + k))


def test_partition_above_the_lds_stage(env, cref):
    """40 000 entries: more than the 37 340 the LDS stage (and the register slots) hold"""
    took, fell = run(env, cref, vector(510, buckets_spread(40000), 5000))
    assert took >= 1 and fell >= 1, (took, fell)


def test_negative_digits_and_their_carry(env, cref):
    """64 of 1024 values are 2^20 - v: window 0 recodes to the NEGATIVE digit -v (same bucket, negate flag set) and carries one
    into window 1, i.e. 64 entries in bucket 0 of partition 0"""
    sc = vector(510, buckets_spread(1024), 6000)
    nz = np.flatnonzero(sc[:, 0])
    flip = nz[:: len(nz) // 64][:64]
    assert len(flip) == 64
    sc[flip, 0] = np.uint64(1 << 20) - sc[flip, 0]
    run(env, cref, sc)


def test_uniform_vector(env, cref):
    """uniform scalars: 13 entries each, about 6 660 per partition, 7 register slots per lane"""
    took, fell = run(env, cref, cref.rng_scalars(0x5EED7001, N))
    assert took >= 1 and fell == 0, (took, fell)
