"""BLS12-377 G1 (AMSM_BLS12_377_G1 = 8) on the GPU: the second 14 x 28-bit base field and the first of that shape with p_0 = 1
(csrc/fpu.h: Bls12377FqU) through every kernel family at the smallest shape that reaches it -- the synthetic key stream, MSMs over
keys that open with the adversarial points of tests/golden/bls12_377_adversarial_points.json, edge scalars through every
accumulation form, one MSM over a shared bucket set, unit scalars summed apart, the scalar-field vector and polynomial kernels over
the 253-bit r (the generated fe_dot2 / fe_dot3 of Bls12377Fr), key folds (GLV ladder), transparent keys -- the sampling kernels'
first run of Tonelli-Shanks on 14 limbs, and of an even cofactor --, point validation over the curve's points of order 2, 3 and 6
under both subgroup ladders against the host backend, the scalar stream with its reduced fallback, the four schemes' C++ drivers and
a 2-shard key.

Large MSMs need no big oracle: a generated key has G_i = k_i G with k_i = rng_scalar(seed, i) (pyref.rng_scalar, restated below
with numpy; most k_i exceed r here, which changes nothing: k_i G is taken over the integers), so
sum s_i G_i = (sum s_i k_i mod r) G, one scalar multiplication in Python.  The adversarial points at the head of an explicit key go
through the oracle's multiplication, one per point."""
import json
import os

import numpy as np
import pytest

from oracle import pyref as o
from tests import helpers as h
from tests.test_bls12_377_cpu import BLS12_377, FALLBACK_INDICES, P, R, points_check_case, scalar_stream

pytestmark = pytest.mark.gpu

C = BLS12_377
SEED = 0x5EED8008
RINV = pow(1 << 256, -1, R)
FIX = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bls12_377_adversarial_points.json")))
# csrc/msm_select.h: an MSM over a 20-bit key is cut into ranges of RANGE_PAIRS = 2^20; a last range takes the bucket-per-lane row
# (and so joins the shared bucket set) only above a quarter of that, P2(18) -- a shorter one runs over the key's 17-bit twin, which
# it would have to build.  The smallest pair count above 2^20 that shares one bucket set without a twin:
N_SHARED = (1 << 20) + (1 << 18) + 1


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
    s = sum(a * b for a, b in zip(scalars, mult)) % R
    return o.mul(C, s * RINV % R if mont else s, o.generator(C))


def got(xy, inf):
    return h.np_to_point(C, xy, inf)


@pytest.fixture(scope="module")
def ctx(built_lib):
    from accumulation_amd import Context, ffi
    c = Context(ffi.AMSM_BLS12_377_G1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def host(built_lib):
    from accumulation_amd import Context, ffi
    c = Context(ffi.AMSM_BLS12_377_G1, device=ffi.AMSM_DEVICE_HOST)
    yield c
    c.close()


@pytest.fixture(scope="module")
def long_key(ctx):
    """ONE key with the 20-bit table for the module: the 20-bit case of the edge-scalar test and the shared bucket set"""
    from accumulation_amd import CommitterKey, ffi
    ck = CommitterKey.generate(ctx, SEED, N_SHARED, ffi.AMSM_BASES_PRECOMPUTE)
    assert ck.precomputed and ck.window_bits == 20
    yield ck, mults(SEED, N_SHARED)
    ck.free()


def test_multiplier_stream_restatement():
    m = mults(SEED, 256)
    assert m == [o.rng_scalar(SEED, i) for i in range(256)] and sum(k >= R for k in m) > 128


def test_bases_generate_vs_oracle(ctx):
    from accumulation_amd import CommitterKey, ffi
    n = 1 << 8
    ck = CommitterKey.generate(ctx, 77, n, ffi.AMSM_BASES_NO_PRECOMPUTE)
    xy, inf = ck.read()
    assert [got(xy[i], inf[i]) for i in range(n)] == o.rng_points(C, 77, n)
    ck.free()


# ---- adversarial keys ----------------------------------------------------------------------------------------------------------------
def adversarial_head():
    """the fixture's points, each as (P, P, -P, P) under one scalar -- equal digits double, double the negated point and cancel in
    one bucket --, then the negated-doubling pair as (l, r, r); -> (points, scalars, their sum by the oracle)"""
    pts, sc, acc = [], [], None
    edge = [R - 1, R - 2, (1 << 17) - 1, 15, (1 << 200) - 1, (1 << 16) - 1, 3, (1 << 128) + 1]
    k = 0
    for kind in FIX["curves"][C.name].values():
        for x, y in kind:
            pt, s = (int(x, 16), int(y, 16)), edge[k % len(edge)]
            k += 1
            pts += [pt, pt, o.neg(C, pt), pt]
            sc += [s] * 4
            acc = o.add(C, acc, o.mul(C, 2 * s % R, pt))
    pair = FIX["negated_doubling_pair"]
    l, r = ((int(pair[key][0], 16), int(pair[key][1], 16)) for key in ("l", "r"))
    pts += [l, r, r]
    sc += [1, R - 2, R - 2]
    acc = o.add(C, acc, o.add(C, l, o.mul(C, 2 * (R - 2) % R, r)))
    return pts, sc, acc


@pytest.fixture(scope="module")
def head():
    return adversarial_head()


def adversarial_key(ctx, head_pts, n, seed):
    """explicit points: the adversarial head, then a generated key's points with identities, duplicates and P / -P pairs:
    (xy, inf, multipliers of the entries behind the head)"""
    from accumulation_amd import CommitterKey, ffi
    hn = len(head_pts)
    assert hn < n
    hxy, hinf = h.points_to_np(C, head_pts)
    g = CommitterKey.generate(ctx, seed, n - hn, ffi.AMSM_BASES_NO_PRECOMPUTE)
    xy, inf = g.read()
    g.free()
    xy, inf, mult = xy.copy(), inf.copy(), mults(seed, n - hn)
    for i in range(0, n - hn, 89):
        xy[i], inf[i], mult[i] = 0, 1, 0
    for i in range(7, n - hn, 41):
        xy[i], inf[i], mult[i] = xy[i - 5], inf[i - 5], mult[i - 5]
    for i in range(13, n - hn, 37):
        q = got(xy[i - 1], inf[i - 1])
        q = None if q is None else o.neg(C, q)
        qxy, qinf = h.points_to_np(C, [q])
        xy[i], inf[i], mult[i] = qxy[0], qinf[0], (-mult[i - 1]) % R
    return np.concatenate([hxy, xy]), np.concatenate([hinf, inf]), mult


@pytest.mark.parametrize("log2n", [8, 12, 16])
@pytest.mark.parametrize("flags", [1, 2], ids=["precomp", "plain"])
def test_msm_adversarial_keys(ctx, head, log2n, flags):
    from accumulation_amd import CommitterKey, VariableBaseMSM
    head_pts, head_sc, head_sum = head
    n, hn = 1 << log2n, len(head_pts)
    xy, inf, mult = adversarial_key(ctx, head_pts, n, log2n)
    ck = CommitterKey.load(ctx, xy, inf, flags)
    pad = ctx.random_vector(3, n - hn, False)
    sc = ints(pad.download())
    pad.free()
    sc[0], sc[1], sc[2] = 0, 1, R - 1
    res = VariableBaseMSM.multi_scalar_mul(ck, h.scalars_to_np(head_sc + sc))
    assert got(*res) == o.add(C, head_sum, expect(mult, sc))
    ck.free()


# ---- edge scalars through every accumulation form ------------------------------------------------------------------------------------
def edge_scalars():
    """the scalars a digit recoding can get wrong, all below r: the ends of the field, its middle, single bits and runs of ones at
    window boundaries, and for every window width c the library uses (msm_select.h: 8, 13, 15, 16, 17, 20) the window patterns
    around the signed digits' carry.  r lies between 2^252 and 2^253, so a scalar below r has 252 free bits: the patterns fill those."""
    vals = [0, 1, 2, R - 1, R - 2, (R - 1) // 2, (R + 1) // 2, 1 << 252]
    for k in (16, 17, 20, 40, 128, 200, 252):
        vals += [(1 << k) - 1, 1 << k]
    # 2^252 - 1 (above) has EVERY window of every width all ones: each signed digit is -1 or 0 with a carry into the next, up to the top
    # window.  Beside it, per width: every window 2^c - 2 (with the carry all ones: every digit non-zero, negative and carrying),
    # 2^(c-1) (the sign boundary itself) and 2^(c-1) - 1 (the largest digit that does not carry)
    for c in (8, 13, 15, 16, 17, 20):
        for w in ((1 << c) - 2, 1 << (c - 1), (1 << (c - 1)) - 1):
            vals.append(sum(w << (c * j) for j in range(252 // c + 1)) & ((1 << 252) - 1))
    assert all(0 <= v < R for v in vals) and (1 << 252) - 1 in vals and (1 << 252) < R < (1 << 253)
    return vals


# One case per accumulation form, at the smallest size the selection table (csrc/msm_select.h: kPipeline, key_window, tail_plan;
# pinned without a GPU by tests/test_pipeline_select_cpu.py) gives that form -- (key flags, generators, pairs, the counter of
# Context.pipeline_stats() that must move (None: the chunked pipeline, which has none), AMSM_BPL).  generators = 0: the module's
# 20-bit key.  msel::choose is the same for every curve; what depends on r is bpl_geom's part_max (api_pipeline.inc), the entries
# the fullest 1024-bucket partition expects, which the top window decides: raw top digits reach r >> 240 = 0x12ab (+ 1 for the
# carry), the narrowest so far.  At these shapes, against the stage's CAP = 40960 - 3620 = 37340 entries (kern_fr.hip):
#   plain, 15-bit windows, 2^17 + 1 pairs: top window 14 bits wide at bit 242, raw <= 1195, top_shift 1: reach 4780 buckets,
#                                          (2^17 + 1) * 1024 / 4780 = 28 080 (+ 5 sigma = 838): fits
#   plain, 16-bit windows, 2^18 + 1 pairs: raw <= 4780, top_shift 1: reach 9560, (2^18 + 1) * 1024 / 9560 = 28 080: fits
#   20-bit table, 2^18 + 1 pairs:          top_shift 5: reach 152 960; 12 * 512 + 1755 = 7899: fits (2^20 pairs: 31 596 + 889: fits)
# so every row stays on the pipeline the other curves take -- no row moves because of r's top window.  (A PLAIN key of 2^20 pairs
# would expect 2^20 * 1024 / 9560 = 112 316 entries and runs chunked, as on BN254: DESIGN.md 4.1.)
FORMS = {
    "direct_sum": (1, 1 << 12, 1 << 12, "direct_sum", None),
    "chunked_13_bit_table": (1 | 4, 1 << 15, 1 << 12, None, None),
    "bucket_split": (1, 1 << 16, 1 << 16, "bucket_split", None),
    "fused_tail_one_record": (2, 1 << 10, 1 << 10, None, None),
    "bucket_per_lane_plain_15_bit": (2, (1 << 17) + 1, (1 << 17) + 1, "bucket_per_lane", None),
    "bucket_per_lane_plain_16_bit": (2, (1 << 18) + 1, (1 << 18) + 1, "bucket_per_lane", None),
    "bucket_per_lane_20_bit_table": (1, 0, (1 << 18) + 1, "bucket_per_lane", None),
    "chunked_bpl_off": (2, (1 << 17) + 1, (1 << 17) + 1, None, "0"),
}


@pytest.mark.parametrize("form", list(FORMS))
def test_edge_scalars_through_every_accumulation_form(ctx, long_key, monkeypatch, form):
    """sum s_i G_i for a vector that opens with three rounds of edge_scalars(), closes with a fourth (the last lanes of the last
    block) and is uniform in between -- few enough edge values that no skew probe sends the vector elsewhere: the counters say which
    form ran, and no fallback re-ran it"""
    from accumulation_amd import CommitterKey, Context, VariableBaseMSM
    flags, gens, n, counter, bpl = FORMS[form]
    c = ctx
    if bpl is not None:
        with monkeypatch.context() as m:  # (the context reads its switches when it is made)
            m.setenv("AMSM_BPL", bpl)
            c = Context(C.curve_id)
    try:
        ck = long_key[0] if gens == 0 else CommitterKey.generate(c, SEED, gens, flags)
        assert ck.precomputed == bool(flags & 1)
        edge = edge_scalars()
        pad = c.random_vector(17, n, False)
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
        if gens:
            ck.free()
    finally:
        if c is not ctx:
            c.close()


def test_msm_over_a_shared_bucket_set(ctx, long_key):
    """N_SHARED pairs over the 20-bit key: two ranges (2^20 and 2^18 + 1 pairs), the second adding to the first's bucket table
    (k_accum_bpl<ACC>), one reduction and one fold; no twin is built"""
    from accumulation_amd import VariableBaseMSM
    ck, mult = long_key
    v = ctx.random_vector(23, N_SHARED, True)
    before = ctx.pipeline_stats()
    out, inf = VariableBaseMSM.multi_scalar_mul(ck, v, mont=True)
    after = ctx.pipeline_stats()
    assert after["shared_bucket_sets"] - before["shared_bucket_sets"] == 1 and after["fallbacks"] == before["fallbacks"]
    assert got(out, inf) == expect(mult, ints(v.download()), mont=True)
    v.free()


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


# ---- scalar-field kernels ------------------------------------------------------------------------------------------------------------
def test_scalar_stream_is_canonical(ctx):
    """k_vec_random over Bls12377Fr, seed 1, indices 0 .. 2^16: every value below r and equal to the restated rule, rng_fr(..) % r;
    the fallback indices (2008 and four more, where the literal rule gives >= r) are among them"""
    n = 1 << 16
    want, over = scalar_stream(1, n)
    assert over == FALLBACK_INDICES and o.rng_fr(C, 1, 2008) >= R
    v = ctx.random_vector(1, n, False)
    out = ints(v.download())
    v.free()
    assert all(x < R for x in out) and tuple(out) == want


def test_vector_kernels(ctx, built_lib):
    """the r launchers of kern_fr.hip over Bls12377Fr, with fe_dot2 / fe_dot3 schedules generated for this modulus (the inner product
    and the polynomial kernels below run them)"""
    from accumulation_amd.engine import _ptr
    n = 1 << 12
    a, b, out = ctx.random_vector(1, n, True), ctx.random_vector(2, n, True), ctx.vector(n)
    av, bv = h.fr_from_mont_np(C, a.download()), h.fr_from_mont_np(C, b.download())
    assert tuple(av) == scalar_stream(1, 1 << 16)[0][:n] and all(x < R for x in av)
    assert built_lib.amsm_vec_hadamard(ctx._h, a.ptr, b.ptr, out.ptr, n) == 0
    assert h.fr_from_mont_np(C, out.download()) == [x * y % R for x, y in zip(av, bv)]
    ip = np.zeros((1, 4), dtype=np.uint64)
    assert built_lib.amsm_vec_inner_product(ctx._h, a.ptr, b.ptr, n, _ptr(ip)) == 0
    assert h.fr_from_mont_np(C, ip)[0] == sum(x * y for x, y in zip(av, bv)) % R
    pt = h.fr_mont_np(C, [12345])
    assert built_lib.amsm_vec_powers(ctx._h, _ptr(pt), n, out.ptr) == 0
    assert h.fr_from_mont_np(C, out.download()) == [pow(12345, i, R) for i in range(n)]
    # the field's edge values through the product: (r - 1)^2 = 1, (r - 1) * 1, 0, and the middle of the field
    edge = [0, 1, 2, R - 1, R - 2, (R - 1) // 2, (R + 1) // 2, 1 << 252, (1 << 252) - 1]
    ea, eb = ctx.upload(h.fr_mont_np(C, edge * len(edge))), ctx.upload(h.fr_mont_np(C, [x for x in edge for _ in edge]))
    eo = ctx.vector(len(edge) ** 2)
    assert built_lib.amsm_vec_hadamard(ctx._h, ea.ptr, eb.ptr, eo.ptr, len(edge) ** 2) == 0
    assert h.fr_from_mont_np(C, eo.download()) == [x * y % R for y in edge for x in edge]
    for x in (a, b, out, ea, eb, eo):
        x.free()


@pytest.mark.parametrize("pattern", ["random", "max"])
def test_polynomial_kernels(ctx, pattern):
    """amsm_poly_div_linear / amsm_poly_evaluate over r at 2^12 coefficients (four tiles), against the serial recurrence"""
    from tests.test_poly_gpu import _check_one, _coeffs
    n = 1 << 12
    for z in (o.rng_fr(C, 5, 0) % R, R - 1):
        _check_one(ctx, C, _coeffs(ctx, C, 40, n, pattern), z)


# ---- key folds, transparent keys, validation -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [1, 2], ids=["precomp", "plain"])
def test_key_fold_vs_oracle(ctx, flags):
    """CommitterKey.fold: out_i = P_i + x P_{n+i} over 2^10 generators, for a full-size x (the GLV ladder), the x whose ladder ends in
    a negated doubling and a short one; every 16th output against the oracle"""
    from accumulation_amd import CommitterKey
    n = 1 << 9
    ck = CommitterKey.generate(ctx, 31, 2 * n, flags)
    pts = o.rng_points(C, 31, 2 * n)
    for x in (o.rng_fr(C, 9, 0) % R, R - 2, 0xDEADBEEF):
        f = ck.fold(n, h.fr_mont_np(C, [x])[0], 255)
        xy, inf = f.read()
        assert [got(xy[i], inf[i]) for i in range(0, n, 16)] == [o.add(C, pts[i], o.mul(C, x, pts[n + i])) for i in range(0, n, 16)]
        f.free()
    ck.free()


def test_key_fold_over_the_negated_doubling_pair(ctx):
    """l + (r_order - 2) r: the ladder's last step doubles the negated r, whose internal y is below 2^364"""
    from accumulation_amd import CommitterKey
    pair = FIX["negated_doubling_pair"]
    l, r = ((int(pair[key][0], 16), int(pair[key][1], 16)) for key in ("l", "r"))
    xy, _ = h.points_to_np(C, [l, r])
    for x in (R - 2, R - 1, R - 3):
        ck = CommitterKey.load(ctx, xy, None, 2)
        f = ck.fold(1, h.fr_mont_np(C, [x])[0], 255)
        fxy, finf = f.read()
        assert got(fxy[0], finf[0]) == o.add(C, l, o.mul(C, x, r)), hex(x)
        f.free()
        ck.free()


def test_bases_sample_equals_the_host_backend(ctx, host):
    """amsm_bases_sample: k_sample_search / k_sample_finish with Tonelli-Shanks (two_adicity = 46) on 14 limbs -- BLS12-381 takes the
    direct root -- and the ladder over the even cofactor 0x170b5d443 << 92, bit for bit against the host backend (which
    tests/test_bls12_377_cpu.py holds to the big-integer sampler); 2^8 indices, then a domain string of odd length"""
    from accumulation_amd import ffi
    from accumulation_amd.engine import CommitterKey
    for domain, n, first in ((b"PC-DL-2020", 1 << 8, 0), (b"PC-DL-2020", 1 << 6, (1 << 32) + 5), (b"bls12-377-odd-domain7", 1 << 6, 0)):
        assert len(b"bls12-377-odd-domain7") % 2 == 1
        keys = [CommitterKey.sample(c, domain, n, ffi.AMSM_BASES_NO_PRECOMPUTE, first=first) for c in (ctx, host)]
        (dxy, dinf), (hxy, hinf) = (k.read() for k in keys)
        assert not dinf.any() and np.array_equal(dxy, hxy) and np.array_equal(dinf, hinf)
        for k in keys:
            k.free()


@pytest.mark.parametrize("ladder", ["1", "2"])
def test_points_check_equals_the_host_backend(host, monkeypatch, ladder):
    """k_points_check_curve and k_points_check_subgroup<LADDER> over 512 points -- the fixture's, (p - 1, 0) of order 2, (0, 1) of order
    3, (2, 3) of order 6 (its ladder doubles the point of order 2: ec.h, HasTwoTorsion), three [r]Q of the cofactor's torsion, a point
    of full order, non-canonical words, points off the curve, the identity's forms -- byte for byte against the host backend's [r]P,
    under both ladder shapes (126 doublings and 21 mixed additions over z^2; [z]([z]P)); a fresh context per setting"""
    from accumulation_amd import Context
    from tests.test_points_check_cpu import check_device, report_of
    with monkeypatch.context() as m:  # (the context reads its switches when it is made)
        m.setenv("AMSM_SUBGROUP_LADDER", ladder)
        c = Context(C.curve_id)
    try:
        xy, inf, want, k = points_check_case(512)
        assert xy.shape[0] == 512 and (want == 3).sum() == 7
        (drep, dst), (hrep, hst) = (x.check_points(xy, inf, want_status=True) for x in (c, host))
        assert np.array_equal(dst, hst) and drep == hrep
        assert np.array_equal(dst, want) and drep == report_of(want) and drep["off_subgroup"] == 7 and drep["first_bad"] == k
        xy0 = xy.copy()
        xy0[inf != 0] = 0  # the device-pointer variant has no infinity bytes
        rep, st = check_device(c, xy0)
        assert np.array_equal(st, want) and rep == report_of(want)
    finally:
        c.close()


@pytest.mark.parametrize("flags", [1, 2], ids=["precomp", "plain"])
def test_group_law_on_the_small_order_points(ctx, flags):
    """doubling the point of order 2 gives the identity and the identity plus P gives P, through the device's group law: MSMs over
    plain and precomputed keys of small-order points (the table of a precomputed key holds the doublings of (p - 1, 0) as (0, 0):
    k_precompute_level / k_precompute_all_levels); tests/test_bls12_377_cpu.py runs the same cases on the host backend"""
    from tests.test_msm_gpu import run_msm
    g = o.generator(C)
    for pts, sc in (([(P - 1, 0)], [2]), ([(2, 3)], [3]), ([(2, 3)], [6]), ([(0, 1)], [3]), ([(P - 1, 0), g], [2, 1]),
                    ([(2, 3), (P - 1, 0), g], [3, 1, 5]), ([(P - 1, 0), (P - 1, 0)], [1, 1])):
        want = None
        for pt, s in zip(pts, sc):
            want = o.add(C, want, o.mul(C, s, pt))
        xy, inf = run_msm(ctx, C, pts, sc, flags)
        assert got(xy, inf) == want, (pts, sc)


# ---- the schemes, shards -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme,lg", [("hp_as", 12), ("r1cs_nark_as", 10), ("ipa_pc_as", 10), ("trivial_pc_as", 8)])
def test_cpp_driver_bytes_equal_the_mirror(built_lib, tmp_path, scheme, lg):
    """the four schemes' C++ drivers over BLS12-377 on the GPU (IPA rounds, key folds, the jump fold, commitments), byte for byte
    against the Python mirror (tests/test_bls12_377_cpu.py checks the schemes' transcripts against the oracle)"""
    from tests.test_profile_as_dump import compare
    compare(tmp_path, scheme, lg, "harness", "poseidon", 0, seed=2, curve=8)


def test_two_shards_on_one_gpu_equal_the_single_key(built_lib):
    from accumulation_amd import CommitterKey, Context, MultiContext, VariableBaseMSM, ffi
    n = 1 << 16
    single, multi = Context(ffi.AMSM_BLS12_377_G1), MultiContext(ffi.AMSM_BLS12_377_G1, devices=(0, 0))
    try:
        a = CommitterKey.generate(single, 8, n, ffi.AMSM_BASES_PRECOMPUTE)
        b = CommitterKey.generate(multi, 8, n, ffi.AMSM_BASES_PRECOMPUTE)
        assert b.num_shards == 2
        xa, ia = a.read()
        xb, ib = b.read()
        assert np.array_equal(xa, xb) and np.array_equal(ia, ib)
        v = single.random_vector(4, n, False)
        sc = v.download()
        v.free()
        ra, rb = VariableBaseMSM.multi_scalar_mul(a, sc), VariableBaseMSM.multi_scalar_mul(b, sc)
        assert np.array_equal(ra[0], rb[0]) and ra[1] == rb[1]
        assert got(*ra) == expect(mults(8, n), ints(sc))
        a.free()
        b.free()
    finally:
        single.close()
        multi.close()
