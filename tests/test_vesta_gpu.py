"""Vesta (AMSM_VESTA = 2) on the GPU: the synthetic key stream, MSMs over explicit keys with duplicates, negations and identities,
every MSM pipeline forced once, edge scalars through every accumulation form, 2^20 / 2^22 MSMs checked exactly, the scalar-field
vector kernels, key folds (GLV ladder), the four schemes' C++ drivers and a 2-shard key.

The explicit keys here are "adversarial" in their STRUCTURE only: duplicates, negations and identities of random generated points,
whose coordinates are never tiny or just below p in the device's internal radix.  Points with such extreme coordinates
(tests/golden/adversarial_points.json) go through the group law in tests/test_adversarial_points_gpu.py, Vesta included, and the
scalar-field kernels meet their edge values in tests/test_vec_gpu.py::test_scalar_field_kernels_on_edge_values.

Large MSMs need no big oracle: a generated key has G_i = k_i G with k_i = rng_scalar(seed, i) (pyref.rng_scalar, restated below
with numpy), so sum s_i G_i = (sum s_i k_i mod r) G, one scalar multiplication in Python.  Explicit keys are built the same way
from a generated key's points: duplicates, negations and identities change the multipliers, not the check."""
import os

import numpy as np
import pytest

from oracle import pyref as o
from tests import helpers as h

pytestmark = pytest.mark.gpu

PALLAS = o.PALLAS
VESTA = h.VESTA
SEED = 0x5EED2002
RINV = pow(1 << 256, -1, VESTA.r)


def rng_scalar_limbs(seed, n):
    """(n, 4) uint64: the limbs of pyref.rng_scalar(seed, i), i < n (the multiplier stream of generated keys)"""
    M = (1 << 64) - 1
    j = np.arange(4 * n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64((seed * 0xD1342543DE82EF95 + 0x632BE59BD9B4E019) & M) + j * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    z = z.reshape(n, 4)
    z[:, 3] &= np.uint64((1 << 62) - 1)
    return z


def ints(a):
    b = np.ascontiguousarray(a, dtype="<u8").reshape(-1, 4).tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def mults(seed, n):
    return ints(rng_scalar_limbs(seed, n))


def expect(mult, scalars, mont=False):
    """sum s_i (m_i G): the affine oracle point (scalars in Montgomery form when mont)"""
    s = sum(a * b for a, b in zip(scalars, mult)) % VESTA.r
    return o.mul(VESTA, s * RINV % VESTA.r if mont else s, o.generator(VESTA))


def got(xy, inf):
    return h.np_to_point(VESTA, xy, inf)


def scalars_np(vals):
    return h.scalars_to_np([v % VESTA.r for v in vals])


@pytest.fixture(scope="module")
def ctx(built_lib):
    from accumulation_amd import Context, ffi
    c = Context(ffi.AMSM_VESTA)
    yield c
    c.close()


def test_multiplier_stream_restatement():
    assert mults(SEED, 64) == [o.rng_scalar(SEED, i) for i in range(64)]


def test_bases_generate_vs_oracle(ctx):
    from accumulation_amd import CommitterKey, ffi
    ck = CommitterKey.generate(ctx, 77, 2048, ffi.AMSM_BASES_NO_PRECOMPUTE)
    xy, inf = ck.read()
    assert [got(xy[i], inf[i]) for i in range(2048)] == o.rng_points(VESTA, 77, 2048)
    ck.free()


def adversarial_key(ctx, n, seed):
    """explicit points from a generated key with identities, duplicates and P / -P pairs: (xy, inf, multipliers)"""
    from accumulation_amd import CommitterKey, ffi
    g = CommitterKey.generate(ctx, seed, n, ffi.AMSM_BASES_NO_PRECOMPUTE)
    xy, inf = g.read()
    g.free()
    xy, inf, mult = xy.copy(), inf.copy(), mults(seed, n)
    for i in range(0, n, 89):
        xy[i], inf[i], mult[i] = 0, 1, 0
    for i in range(7, n, 41):
        xy[i], inf[i], mult[i] = xy[i - 5], inf[i - 5], mult[i - 5]
    for i in range(13, n, 37):
        q = got(xy[i - 1], inf[i - 1])
        q = None if q is None else o.neg(VESTA, q)
        qxy, qinf = h.points_to_np(VESTA, [q])
        xy[i], inf[i], mult[i] = qxy[0], qinf[0], (-mult[i - 1]) % VESTA.r
    return xy, inf, mult


@pytest.mark.parametrize("log2n", [8, 10, 12, 14, 16])
@pytest.mark.parametrize("flags", [1, 2], ids=["precomp", "plain"])
def test_msm_explicit_adversarial_keys(ctx, log2n, flags):
    from accumulation_amd import CommitterKey, VariableBaseMSM
    n = 1 << log2n
    xy, inf, mult = adversarial_key(ctx, n, log2n)
    ck = CommitterKey.load(ctx, xy, inf, flags)
    sc = [o.rng_fr(VESTA, 3, i) for i in range(n)]
    sc[0], sc[1], sc[2] = 0, 1, VESTA.r - 1
    assert got(*VariableBaseMSM.multi_scalar_mul(ck, scalars_np(sc))) == expect(mult, sc)
    ck.free()


def test_pipelines_forced_once(ctx):
    """bucket-per-lane (2^20), the twin, a short range of the 2^20 key, the two-valued form, bucket-split (a 2^16 key), direct sum
    (a precomputed 2^12 key), one-shot, and the chunked pipeline (a context without bucket-per-lane)"""
    from accumulation_amd import CommitterKey, Context, VariableBaseMSM, ffi
    n = 1 << 20
    ck = CommitterKey.generate(ctx, SEED, n, ffi.AMSM_BASES_PRECOMPUTE)
    mult = mults(SEED, n)
    v = ctx.random_vector(11, n, True)
    s = ints(v.download())
    before = ctx.pipeline_stats()
    out, inf = VariableBaseMSM.multi_scalar_mul_batch(ck, [v])
    assert got(out[0], inf[0]) == expect(mult, s, mont=True)
    assert ctx.pipeline_stats()["bucket_per_lane"] > before["bucket_per_lane"]
    ck.prebuild_twin()
    out, inf = VariableBaseMSM.multi_scalar_mul_batch(ck, [v])
    assert got(out[0], inf[0]) == expect(mult, s, mont=True)
    off, m = 123457, 3001
    assert got(*VariableBaseMSM.multi_scalar_mul(ck, v.view(0, m), base_off=off, mont=True)) == expect(mult[off:off + m], s[:m], mont=True)
    v.free()
    # two-valued (every scalar 0 or w)
    w = h.fr_mont_np(VESTA, [o.rng_fr(VESTA, 12, 0)])[0]
    mask = (np.arange(n) * 7) % 3 != 0
    t0 = ctx.two_valued_msms()
    vec = ctx.upload(np.where(mask[:, None], w[None, :], np.uint64(0)))
    out, inf = VariableBaseMSM.multi_scalar_mul_batch(ck, [vec])
    assert got(out[0], inf[0]) == expect(mult, ints(vec.download()), mont=True) and ctx.two_valued_msms() > t0
    vec.free()
    ck.free()
    # bucket-split (a 2^16 key, a device vector) and direct sum (a precomputed 2^12 key, host scalars)
    for log2n, flags, counter in ((16, ffi.AMSM_BASES_DEFAULT, "bucket_split"), (12, ffi.AMSM_BASES_PRECOMPUTE, "direct_sum")):
        small = CommitterKey.generate(ctx, SEED, 1 << log2n, flags)
        b = ctx.pipeline_stats()[counter]
        sv = ctx.random_vector(log2n, 1 << log2n, True)
        arg = sv if counter == "bucket_split" else sv.download()
        assert got(*VariableBaseMSM.multi_scalar_mul(small, arg, mont=True)) == expect(mult, ints(sv.download()), mont=True), counter
        assert ctx.pipeline_stats()[counter] > b, counter
        sv.free()
        small.free()
    # one-shot: host bases and host scalars of this call only
    small = CommitterKey.generate(ctx, SEED, 4096, ffi.AMSM_BASES_NO_PRECOMPUTE)
    xy, xinf = small.read()
    small.free()
    sc = [o.rng_fr(VESTA, 13, i) for i in range(4096)]
    assert got(*VariableBaseMSM.multi_scalar_mul_oneshot(ctx, xy, scalars_np(sc), xinf)) == expect(mult, sc)
    # chunked: a context without the bucket-per-lane pipeline, plain key
    os.environ["AMSM_BPL"] = "0"
    try:
        c2 = Context(ffi.AMSM_VESTA)
    finally:
        del os.environ["AMSM_BPL"]
    try:
        plain = CommitterKey.generate(c2, SEED, 1 << 18, ffi.AMSM_BASES_NO_PRECOMPUTE)
        sv = c2.random_vector(18, 1 << 18, True)
        out, inf = VariableBaseMSM.multi_scalar_mul_batch(plain, [sv])
        assert got(out[0], inf[0]) == expect(mult, ints(sv.download()), mont=True)
        assert c2.pipeline_stats()["bucket_per_lane"] == 0
        sv.free()
        plain.free()
    finally:
        c2.close()


def edge_scalars():
    """the scalars a digit recoding can get wrong, all below r: the ends of the field, its middle, single bits and runs of ones at
    window boundaries, and for every window width c the library uses (msm_select.h: 8, 13, 15, 16, 17, 20) the window patterns
    around the signed digits' carry.  r is just above 2^254, so a scalar below r has 254 free bits: the patterns fill those."""
    r = VESTA.r
    vals = [0, 1, 2, r - 1, r - 2, (r - 1) // 2, (r + 1) // 2, 1 << 254]
    for k in (16, 17, 20, 40, 128, 200, 254):
        vals += [(1 << k) - 1, 1 << k]
    # 2^254 - 1 (above) has EVERY window of every width all ones: each signed digit is -1 or 0 with a carry into the next, up to the top
    # window.  Beside it, per width: every window 2^c - 2 (with the carry all ones: every digit non-zero, negative and carrying),
    # 2^(c-1) (the sign boundary itself) and 2^(c-1) - 1 (the largest digit that does not carry)
    for c in (8, 13, 15, 16, 17, 20):
        for w in ((1 << c) - 2, 1 << (c - 1), (1 << (c - 1)) - 1):
            vals.append(sum(w << (c * j) for j in range(254 // c + 1)) & ((1 << 254) - 1))
    assert all(0 <= v < r for v in vals) and (1 << 254) - 1 in vals
    return vals


# One case per accumulation form, at the smallest size the selection table (csrc/msm_select.h: kPipeline, key_window, tail_plan;
# pinned without a GPU by tests/test_pipeline_select_cpu.py) gives that form -- (key flags, generators, pairs, the counter of
# Context.pipeline_stats() that must move (None: the chunked pipeline, which has none), AMSM_BPL):
#   direct sum          any precomputed key of up to 2^15 generators carries the table of 4-bit signed digits
#   13-bit windows      a precomputed key of 2^15 generators without that table, chunked (key_window 2p15)
#   bucket-split        precomputed, 2^16 pairs: the lower edge of (2^16 - 1, 2^17]; 16-bit windows
#   one record per set  a plain key, 2^10 pairs, a blocking call: 8-bit windows, 32 sets of 128 buckets, the fused tail whose first quad
#                       folds serially (test_tail_plan_of_the_gpu_shapes: gpu_a_plain_2p10)
#   bucket-per-lane     plain keys from 2^17 + 1 pairs (15-bit windows) and from 2^18 + 1 (16-bit); over a precomputed key only with
#                       the 20-bit table, 2^20 generators, from 2^18 + 1 pairs (a precomputed key of 2^17 generators is bucket-split)
#   chunked             the same 2^17 + 1 pairs over a plain key in a context without bucket-per-lane: 8-bit windows at the size where
#                       the switch decides
# The chunked pipeline has no counter, so for its three cases (13-bit windows, one record per set, bucket-per-lane off) the device
# says only that no OTHER form ran: that these sizes mean these window widths and this tail form is pinned by
# tests/test_pipeline_select_cpu.py (key_window 2p15 / 2p9 .. 2p19, gpu_a_plain_2p10, "switch bpl=0") -- a change to the selection
# table shows there, and these sizes move with it.
FORMS = {
    "direct_sum": (1, 1 << 12, 1 << 12, "direct_sum", None),
    "chunked_13_bit_table": (1 | 4, 1 << 15, 1 << 12, None, None),
    "bucket_split": (1, 1 << 16, 1 << 16, "bucket_split", None),
    "fused_tail_one_record": (2, 1 << 10, 1 << 10, None, None),
    "bucket_per_lane_plain_15_bit": (2, (1 << 17) + 1, (1 << 17) + 1, "bucket_per_lane", None),
    "bucket_per_lane_plain_16_bit": (2, (1 << 18) + 1, (1 << 18) + 1, "bucket_per_lane", None),
    "bucket_per_lane_20_bit_table": (1, 1 << 20, (1 << 18) + 1, "bucket_per_lane", None),
    "chunked_bpl_off": (2, (1 << 17) + 1, (1 << 17) + 1, None, "0"),
}


@pytest.mark.parametrize("form", list(FORMS))
def test_edge_scalars_through_every_accumulation_form(ctx, monkeypatch, form):
    """sum s_i G_i for a vector that opens with three rounds of edge_scalars(), closes with a fourth (the last lanes of the last
    block) and is uniform in between -- few enough edge values that no skew probe sends the vector elsewhere: the counters say which
    form ran, and no fallback re-ran it"""
    from accumulation_amd import CommitterKey, Context, VariableBaseMSM
    flags, gens, n, counter, bpl = FORMS[form]
    c = ctx
    if bpl is not None:
        with monkeypatch.context() as m:  # (the context reads its switches when it is made)
            m.setenv("AMSM_BPL", bpl)
            c = Context(VESTA.curve_id)
    try:
        ck = CommitterKey.generate(c, SEED, gens, flags)
        assert ck.precomputed == bool(flags & 1)
        edge = edge_scalars()
        pad = c.random_vector(17, n, False)  # pyref.rng_fr's stream (test_vector_kernels)
        sc = ints(pad.download())
        pad.free()
        assert n >= 4 * len(edge)
        sc[:3 * len(edge)] = edge * 3
        sc[n - len(edge):] = edge
        v = c.upload(h.scalars_to_np(sc))
        before = c.pipeline_stats()
        res = VariableBaseMSM.multi_scalar_mul(ck, v, mont=False)
        moved = {k: x - before[k] for k, x in c.pipeline_stats().items() if x != before[k]}
        assert moved == ({counter: 1} if counter else {}), (form, moved)
        assert got(*res) == expect(mults(SEED, n), sc), form
        v.free()
        ck.free()
    finally:
        if c is not ctx:
            c.close()


def test_unit_scalars_summed_apart(ctx):
    """a witness-like vector (a tenth of its scalars replaced by 0 / 1) in a batch beside a uniform one: its unit scalars are
    summed apart (the form tests/test_unit_scalars_gpu.py checks for the other curves)"""
    from accumulation_amd import CommitterKey, VariableBaseMSM, ffi
    n = (1 << 16) + 11
    ck = CommitterKey.generate(ctx, SEED, n, ffi.AMSM_BASES_PRECOMPUTE | ffi.AMSM_BASES_NO_DIRECT_TABLE)
    uni = ctx.random_vector(15, n, False)
    wit = uni.download()
    rng = np.random.default_rng(1)
    pick = rng.random(n) < 0.1
    vals = np.zeros((n, 4), dtype=np.uint64)
    vals[:, 0] = rng.integers(0, 2, n)
    wit[pick] = vals[pick]
    wv = ctx.upload(wit)
    before = ctx.pipeline_stats()["unit_scalar_sums"]
    out, inf = VariableBaseMSM.multi_scalar_mul_batch(ck, [wv, uni], mont=False)
    assert ctx.pipeline_stats()["unit_scalar_sums"] - before == 1
    mult = mults(SEED, n)
    assert got(out[0], inf[0]) == expect(mult, ints(wit))
    assert got(out[1], inf[1]) == expect(mult, ints(uni.download()))
    wv.free()
    uni.free()
    ck.free()


def test_msm_2p22_exact(ctx):
    from accumulation_amd import CommitterKey, VariableBaseMSM, ffi
    n = 1 << 22
    ck = CommitterKey.generate(ctx, 4242, n, ffi.AMSM_BASES_PRECOMPUTE)
    v = ctx.random_vector(5, n, True)
    out, inf = VariableBaseMSM.multi_scalar_mul_batch(ck, [v])
    assert got(out[0], inf[0]) == expect(mults(4242, n), ints(v.download()), mont=True)
    v.free()
    ck.free()


def test_vector_kernels(ctx, built_lib):
    from accumulation_amd.engine import _ptr
    n, r = 5000, VESTA.r
    a, b, out = ctx.random_vector(1, n, True), ctx.random_vector(2, n, True), ctx.vector(n)
    av, bv = h.fr_from_mont_np(VESTA, a.download()), h.fr_from_mont_np(VESTA, b.download())
    assert av == [o.rng_fr(VESTA, 1, i) for i in range(n)]  # uniform below r_V (pyref.rng_fr's rejection rule over VESTA.r)
    assert built_lib.amsm_vec_hadamard(ctx._h, a.ptr, b.ptr, out.ptr, n) == 0
    assert h.fr_from_mont_np(VESTA, out.download()) == [x * y % r for x, y in zip(av, bv)]
    ip = np.zeros((1, 4), dtype=np.uint64)
    assert built_lib.amsm_vec_inner_product(ctx._h, a.ptr, b.ptr, n, _ptr(ip)) == 0
    assert h.fr_from_mont_np(VESTA, ip)[0] == sum(x * y for x, y in zip(av, bv)) % r
    pt = h.fr_mont_np(VESTA, [12345])
    assert built_lib.amsm_vec_powers(ctx._h, _ptr(pt), n, out.ptr) == 0
    assert h.fr_from_mont_np(VESTA, out.download()) == [pow(12345, i, r) for i in range(n)]
    for x in (a, b, out):
        x.free()


@pytest.mark.parametrize("flags", [1, 2], ids=["precomp", "plain"])
def test_key_fold_vs_oracle(ctx, flags):
    """CommitterKey.fold: out_i = P_i + x P_{n+i}, for a full-size x (the GLV ladder) and a short one"""
    from accumulation_amd import CommitterKey
    n = 1024
    ck = CommitterKey.generate(ctx, 31, 2 * n, flags)
    pts = o.rng_points(VESTA, 31, 2 * n)
    for x in (o.rng_fr(VESTA, 9, 0), 0xDEADBEEF):
        f = ck.fold(n, h.fr_mont_np(VESTA, [x])[0], 255)
        xy, inf = f.read()
        assert [got(xy[i], inf[i]) for i in range(0, n, 16)] == [o.add(VESTA, pts[i], o.mul(VESTA, x, pts[n + i]))
                                                                  for i in range(0, n, 16)]
        f.free()
    ck.free()


@pytest.mark.parametrize("scheme,lg", [("hp_as", 12), ("r1cs_nark_as", 10), ("ipa_pc_as", 10), ("trivial_pc_as", 8)])
def test_cpp_driver_bytes_equal_the_mirror(built_lib, tmp_path, scheme, lg):
    """the four schemes' C++ drivers over Vesta on the GPU (IPA rounds, key folds, the jump fold, commitments), byte for byte
    against the Python mirror on the host backend (tests/test_vesta_cpu.py checks the schemes' transcripts against the oracle)"""
    from tests.test_profile_as_dump import compare
    compare(tmp_path, scheme, lg, "harness", "poseidon", 0, seed=2, curve=2)


def test_two_shards_on_one_gpu_equal_the_single_key(built_lib):
    from accumulation_amd import CommitterKey, Context, MultiContext, VariableBaseMSM, ffi
    n = 1 << 16
    single, multi = Context(ffi.AMSM_VESTA), MultiContext(ffi.AMSM_VESTA, devices=(0, 0))
    try:
        a = CommitterKey.generate(single, 8, n, ffi.AMSM_BASES_PRECOMPUTE)
        b = CommitterKey.generate(multi, 8, n, ffi.AMSM_BASES_PRECOMPUTE)
        assert b.num_shards == 2
        xa, ia = a.read()
        xb, ib = b.read()
        assert np.array_equal(xa, xb) and np.array_equal(ia, ib)
        sc = scalars_np([o.rng_fr(VESTA, 4, i) for i in range(n)])
        ra, rb = VariableBaseMSM.multi_scalar_mul(a, sc), VariableBaseMSM.multi_scalar_mul(b, sc)
        assert np.array_equal(ra[0], rb[0]) and ra[1] == rb[1]
        assert got(*ra) == expect(mults(8, n), h.np_to_ints(sc))
        a.free()
        b.free()
    finally:
        single.close()
        multi.close()
