"""The GPU cases that Vesta, BN254 G1, Grumpkin and BLS12-377 G1 share, each written once: tests/test_<curve>_gpu.py takes from here the
fixtures and the cases its row of tests/curve_rows.py lists (Row.gpu_cases), under its own module name, so a case a curve does not
have does not exist for it.  Each curve's base field (csrc/fpu.h: VestaFqU and the general 9 x 29-bit Bn254FqU and GrumpkinFqU, the
14 x 28-bit Bls12377FqU with p_0 = 1) goes through every kernel family at the smallest shape that reaches it -- the synthetic key
stream, MSMs over keys that open with the adversarial points of the row's fixture, edge scalars through every accumulation form, one
MSM over a shared bucket set, unit scalars summed apart, the scalar-field vector and polynomial kernels, key folds (GLV ladder),
transparent keys and point validation against the host backend, the four schemes' C++ drivers and a 2-shard key.  The cases of one
row alone follow the shared ones.

The fixtures are module-scoped and read the importing module's ROW: each per-curve module has its own context, host-backend context
and 20-bit key, freed when that module ends, so one long key is alive at a time.

Vesta's explicit keys are "adversarial" in their STRUCTURE only: duplicates, negations and identities of random generated points,
whose coordinates are never tiny or just below p in the device's internal radix.  Points with such extreme coordinates
(tests/golden/adversarial_points.json) go through the group law in tests/test_adversarial_points_gpu.py, Vesta included, and the
scalar-field kernels meet their edge values in tests/test_vec_gpu.py::test_scalar_field_kernels_on_edge_values."""
import os

import numpy as np
import pytest

from oracle import pyref as o
from tests import curve_rows as cr
from tests import helpers as h
from tests.curve_rows import FORMS, N_SHARED, edge_scalars, expect, got, ints, mults

SHARED = ("pytest_generate_tests", "row", "ctx", "host", "long_key", "head", "ladder")  # what every per-curve module takes beside its cases


def pytest_generate_tests(metafunc):
    """the parameters whose values the row gives"""
    row = metafunc.module.ROW
    if "log2n" in metafunc.fixturenames:  # (the key's flags first, as the ids always had them)
        metafunc.parametrize("flags", [1, 2], ids=["precomp", "plain"])
        metafunc.parametrize("log2n", row.adv_log2n)
    if "ladder" in metafunc.fixturenames and row.ladders:
        metafunc.parametrize("ladder", row.ladders)


@pytest.fixture(scope="module")
def row(request):
    return request.module.ROW


@pytest.fixture
def ladder():
    """AMSM_SUBGROUP_LADDER of the points-check case; None (the module's context) where the row sets none"""
    return None


@pytest.fixture(scope="module")
def ctx(built_lib, row):
    from accumulation_amd import Context, ffi
    c = Context(getattr(ffi, row.ffi))
    yield c
    c.close()


@pytest.fixture(scope="module")
def host(built_lib, row):
    from accumulation_amd import Context, ffi
    c = Context(getattr(ffi, row.ffi), device=ffi.AMSM_DEVICE_HOST)
    yield c
    c.close()


@pytest.fixture(scope="module")
def long_key(ctx, row):
    """ONE key with the 20-bit table for the row: the 20-bit case of the edge-scalar test and the shared bucket set"""
    from accumulation_amd import CommitterKey, ffi
    ck = CommitterKey.generate(ctx, row.seed, N_SHARED, ffi.AMSM_BASES_PRECOMPUTE)
    assert ck.precomputed and ck.window_bits == 20
    yield ck, mults(row.seed, N_SHARED)
    ck.free()


@pytest.fixture(scope="module")
def head(row):
    return cr.adversarial_head(row)


def test_multiplier_stream_restatement(row):
    m = mults(row.seed, row.stream_n)
    assert m == [o.rng_scalar(row.seed, i) for i in range(row.stream_n)] and sum(k >= row.R for k in m) >= row.over_r[0]


def test_bases_generate_vs_oracle(ctx, row):
    from accumulation_amd import CommitterKey, ffi
    C, n = row.curve, row.generate_n
    ck = CommitterKey.generate(ctx, 77, n, ffi.AMSM_BASES_NO_PRECOMPUTE)
    xy, inf = ck.read()
    assert [got(C, xy[i], inf[i]) for i in range(n)] == o.rng_points(C, 77, n)
    ck.free()


# ---- adversarial keys ----------------------------------------------------------------------------------------------------------------
def test_msm_adversarial_keys(ctx, row, head, log2n, flags):
    from accumulation_amd import CommitterKey, VariableBaseMSM
    C, R = row.curve, row.R
    head_pts, head_sc, head_sum = head
    n, hn = 1 << log2n, len(head_pts)
    xy, inf, mult = cr.adversarial_key(ctx, row, head_pts, n, log2n)
    ck = CommitterKey.load(ctx, xy, inf, flags)
    pad = ctx.random_vector(3, n - hn, False)
    sc = ints(pad.download())
    pad.free()
    sc[0], sc[1], sc[2] = 0, 1, R - 1
    res = VariableBaseMSM.multi_scalar_mul(ck, h.scalars_to_np(head_sc + sc))
    assert got(C, *res) == o.add(C, head_sum, expect(C, mult, sc))
    ck.free()


# ---- edge scalars through every accumulation form ------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
def test_edge_scalars_through_every_accumulation_form(ctx, row, request, monkeypatch, form):
    """sum s_i G_i for a vector that opens with three rounds of edge_scalars(), closes with a fourth (the last lanes of the last
    block) and is uniform in between -- few enough edge values that no skew probe sends the vector elsewhere: the counters say which
    form ran, and no fallback re-ran it"""
    from accumulation_amd import CommitterKey, Context, VariableBaseMSM
    C = row.curve
    flags, gens, n, counter, bpl = FORMS[form]
    own = gens != 0 or row.own_long_key
    c = ctx
    if bpl is not None:
        with monkeypatch.context() as m:  # (the context reads its switches when it is made)
            m.setenv("AMSM_BPL", bpl)
            c = Context(C.curve_id)
    try:
        ck = CommitterKey.generate(c, row.seed, gens or 1 << 20, flags) if own else request.getfixturevalue("long_key")[0]
        assert ck.precomputed == bool(flags & 1)
        edge = edge_scalars(C)
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
        assert got(C, *res) == expect(C, mults(row.seed, n), sc), form
        v.free()
        if own:
            ck.free()
    finally:
        if c is not ctx:
            c.close()


def test_msm_over_a_shared_bucket_set(ctx, row, long_key):
    """N_SHARED pairs over the 20-bit key: two ranges (2^20 and 2^18 + 1 pairs), the second adding to the first's bucket table
    (k_accum_bpl<ACC>), one reduction and one fold; no twin is built"""
    from accumulation_amd import VariableBaseMSM
    ck, mult = long_key
    v = ctx.random_vector(23, N_SHARED, True)
    before = ctx.pipeline_stats()
    out, inf = VariableBaseMSM.multi_scalar_mul(ck, v, mont=True)
    after = ctx.pipeline_stats()
    assert after["shared_bucket_sets"] - before["shared_bucket_sets"] == 1 and after["fallbacks"] == before["fallbacks"]
    assert got(row.curve, out, inf) == expect(row.curve, mult, ints(v.download()), mont=True)
    v.free()


def test_unit_scalars_summed_apart(ctx, row):
    """a witness-like vector (a tenth of its scalars replaced by 0 / 1) in a batch beside a uniform one: its unit scalars are
    summed apart (the form tests/test_unit_scalars_gpu.py checks for Pallas and BLS12-381)"""
    from accumulation_amd import CommitterKey, VariableBaseMSM, ffi
    C = row.curve
    n = (1 << 16) + 11
    ck = CommitterKey.generate(ctx, row.seed, n, ffi.AMSM_BASES_PRECOMPUTE | ffi.AMSM_BASES_NO_DIRECT_TABLE)
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
    mult = mults(row.seed, n)
    assert got(C, out[0], inf[0]) == expect(C, mult, ints(wit))
    assert got(C, out[1], inf[1]) == expect(C, mult, ints(uni.download()))
    wv.free()
    uni.free()
    ck.free()


# ---- scalar-field kernels ------------------------------------------------------------------------------------------------------------
def test_vector_kernels(ctx, row, built_lib):
    """the r launchers of kern_fr.hip over the row's Fr (generated fe_mul / fe_dot2 / fe_dot3 schedules for its modulus, with every
    reduction product; the inner product and the polynomial kernels below run them)"""
    from accumulation_amd.engine import _ptr
    C, R, n = row.curve, row.R, row.vec_n
    a, b, out = ctx.random_vector(1, n, True), ctx.random_vector(2, n, True), ctx.vector(n)
    av, bv = h.fr_from_mont_np(C, a.download()), h.fr_from_mont_np(C, b.download())
    # uniform below r: pyref.rng_fr's rule over this r (reduced where r has 253 bits: cr.scalar_stream)
    assert av == [o.rng_fr(C, 1, i) % R for i in range(n)] and all(x < R for x in av)
    assert built_lib.amsm_vec_hadamard(ctx._h, a.ptr, b.ptr, out.ptr, n) == 0
    assert h.fr_from_mont_np(C, out.download()) == [x * y % R for x, y in zip(av, bv)]
    ip = np.zeros((1, 4), dtype=np.uint64)
    assert built_lib.amsm_vec_inner_product(ctx._h, a.ptr, b.ptr, n, _ptr(ip)) == 0
    assert h.fr_from_mont_np(C, ip)[0] == sum(x * y for x, y in zip(av, bv)) % R
    pt = h.fr_mont_np(C, [12345])
    assert built_lib.amsm_vec_powers(ctx._h, _ptr(pt), n, out.ptr) == 0
    assert h.fr_from_mont_np(C, out.download()) == [pow(12345, i, R) for i in range(n)]
    for x in (a, b, out):
        x.free()
    if not row.vec_edge:
        return
    # the field's edge values through the product: (r - 1)^2 = 1, (r - 1) * 1, 0, and the middle of the field
    k = R.bit_length() - 1
    edge = [0, 1, 2, R - 1, R - 2, (R - 1) // 2, (R + 1) // 2, 1 << k, (1 << k) - 1]
    ea, eb = ctx.upload(h.fr_mont_np(C, edge * len(edge))), ctx.upload(h.fr_mont_np(C, [x for x in edge for _ in edge]))
    eo = ctx.vector(len(edge) ** 2)
    assert built_lib.amsm_vec_hadamard(ctx._h, ea.ptr, eb.ptr, eo.ptr, len(edge) ** 2) == 0
    assert h.fr_from_mont_np(C, eo.download()) == [x * y % R for y in edge for x in edge]
    for x in (ea, eb, eo):
        x.free()


@pytest.mark.parametrize("pattern", ["random", "max"])
def test_polynomial_kernels(ctx, row, pattern):
    """amsm_poly_div_linear / amsm_poly_evaluate over r at 2^12 coefficients (four tiles), against the serial recurrence"""
    from tests.test_poly_gpu import _check_one, _coeffs
    C, n = row.curve, 1 << 12
    for z in (o.rng_fr(C, 5, 0) % row.R, row.R - 1):
        _check_one(ctx, C, _coeffs(ctx, C, 40, n, pattern), z)


# ---- key folds, transparent keys, validation -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [1, 2], ids=["precomp", "plain"])
def test_key_fold_vs_oracle(ctx, row, flags):
    """CommitterKey.fold: out_i = P_i + x P_{n+i}, for a full-size x (the GLV ladder), the x whose ladder ends in a negated doubling
    (not on Vesta) and a short one; every 8th or 16th output against the oracle"""
    from accumulation_amd import CommitterKey
    C, R, (n, step) = row.curve, row.R, row.fold
    ck = CommitterKey.generate(ctx, 31, 2 * n, flags)
    pts = o.rng_points(C, 31, 2 * n)
    for x in (o.rng_fr(C, 9, 0) % R,) + ((R - 2,) if row.fold_negated_doubling else ()) + (0xDEADBEEF,):
        f = ck.fold(n, h.fr_mont_np(C, [x])[0], 255)
        xy, inf = f.read()
        assert [got(C, xy[i], inf[i]) for i in range(0, n, step)] == [o.add(C, pts[i], o.mul(C, x, pts[n + i])) for i in range(0, n, step)]
        f.free()
    ck.free()


def test_key_fold_over_the_negated_doubling_pair(ctx, row):
    """l + (r_order - 2) r: the ladder's last step doubles the negated r, whose internal y has a zero top limb (below 2^232 on the
    9 x 29-bit fields, below 2^364 on BLS12-377)"""
    from accumulation_amd import CommitterKey
    C, R = row.curve, row.R
    l, r = cr.negated_doubling_pair(row)
    xy, _ = h.points_to_np(C, [l, r])
    for x in (R - 2, R - 1, R - 3):
        ck = CommitterKey.load(ctx, xy, None, 2)
        f = ck.fold(1, h.fr_mont_np(C, [x])[0], 255)
        fxy, finf = f.read()
        assert got(C, fxy[0], finf[0]) == o.add(C, l, o.mul(C, x, r)), hex(x)
        f.free()
        ck.free()


def test_bases_sample_equals_the_host_backend(ctx, row, host):
    """amsm_bases_sample: k_sample_search / k_sample_finish, byte for byte against the host backend (which tests/curve_cases_cpu.py
    holds to the big-integer sampler) -- BN254: ONE digest word (254 bits) and the direct root together; Grumpkin: Tonelli-Shanks with
    two_adicity = 28; BLS12-377: Tonelli-Shanks (two_adicity = 46) on 14 limbs and the ladder over the even cofactor
    0x170b5d443 << 92.  The last two also take a domain string of odd length"""
    from accumulation_amd import ffi
    from accumulation_amd.engine import CommitterKey
    if len(row.samples) == 3:
        assert len(row.samples[2][0]) % 2 == 1
    for domain, n, first in row.samples:
        keys = [CommitterKey.sample(c, domain, n, ffi.AMSM_BASES_NO_PRECOMPUTE, first=first) for c in (ctx, host)]
        (dxy, dinf), (hxy, hinf) = (k.read() for k in keys)
        assert not dinf.any() and np.array_equal(dxy, hxy) and np.array_equal(dinf, hinf)
        for k in keys:
            k.free()


def test_points_check_equals_the_host_backend(ctx, row, host, monkeypatch, ladder):
    """k_points_check_curve (and, on BLS12-377, k_points_check_subgroup<LADDER>) over the row's points-check case (cr.points_check_case:
    the adversarial points, bad ones, Grumpkin's b-cases; BLS12-377's points of order 2, 3 and 6 -- the ladder of (2, 3) doubles the
    point of order 2: ec.h, HasTwoTorsion -- and of the cofactor's torsion), statuses and report byte for byte against the host
    backend's; status 3 only where the row expects it.  BLS12-377 runs under both ladder shapes (126 doublings and 21 mixed additions
    over z^2; [z]([z]P)), a fresh context per setting"""
    from accumulation_amd import Context
    from tests.test_points_check_cpu import check_device, report_of
    c = ctx
    if ladder is not None:
        with monkeypatch.context() as m:  # (the context reads its switches when it is made)
            m.setenv("AMSM_SUBGROUP_LADDER", ladder)
            c = Context(row.curve.curve_id)
    try:
        xy, inf, want, k = cr.points_check_case(row, row.check_n)
        assert xy.shape[0] == row.check_n and (want == 3).sum() == row.off_subgroup
        (drep, dst), (hrep, hst) = (x.check_points(xy, inf, want_status=True) for x in (c, host))
        assert np.array_equal(dst, hst) and drep == hrep
        assert np.array_equal(dst, want) and drep == report_of(want) and drep["off_subgroup"] == row.off_subgroup and drep["first_bad"] == k
        xy0 = xy.copy()
        xy0[inf != 0] = 0  # the device-pointer variant has no infinity bytes
        rep, st = check_device(c, xy0)
        assert np.array_equal(st, want) and rep == report_of(want)
    finally:
        if c is not ctx:
            c.close()


# ---- the schemes, shards -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme,lg", [("hp_as", 12), ("r1cs_nark_as", 10), ("ipa_pc_as", 10), ("trivial_pc_as", 8)])
def test_cpp_driver_bytes_equal_the_mirror(built_lib, row, tmp_path, scheme, lg):
    """the four schemes' C++ drivers over the row's curve on the GPU (IPA rounds, key folds, the jump fold, commitments), byte for
    byte against the Python mirror (tests/curve_cases_cpu.py checks the schemes' transcripts against the oracle)"""
    from tests.test_profile_as_dump import compare
    compare(tmp_path, scheme, lg, "harness", "poseidon", 0, seed=2, curve=row.curve.curve_id)


def test_two_shards_on_one_gpu_equal_the_single_key(built_lib, row):
    from accumulation_amd import CommitterKey, Context, MultiContext, VariableBaseMSM, ffi
    C, cid = row.curve, getattr(ffi, row.ffi)
    n = 1 << 16
    single, multi = Context(cid), MultiContext(cid, devices=(0, 0))
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
        assert got(C, *ra) == expect(C, mults(8, n), ints(sc))
        a.free()
        b.free()
    finally:
        single.close()
        multi.close()


# ---- Vesta alone -------------------------------------------------------------------------------------------------------------------------
def test_pipelines_forced_once(ctx, row):
    """bucket-per-lane (2^20), the twin, a short range of the 2^20 key, the two-valued form, bucket-split (a 2^16 key), direct sum
    (a precomputed 2^12 key), one-shot, and the chunked pipeline (a context without bucket-per-lane)"""
    from accumulation_amd import CommitterKey, Context, VariableBaseMSM, ffi
    VESTA, SEED = row.curve, row.seed
    n = 1 << 20
    ck = CommitterKey.generate(ctx, SEED, n, ffi.AMSM_BASES_PRECOMPUTE)
    mult = mults(SEED, n)
    v = ctx.random_vector(11, n, True)
    s = ints(v.download())
    before = ctx.pipeline_stats()
    out, inf = VariableBaseMSM.multi_scalar_mul_batch(ck, [v])
    assert got(VESTA, out[0], inf[0]) == expect(VESTA, mult, s, mont=True)
    assert ctx.pipeline_stats()["bucket_per_lane"] > before["bucket_per_lane"]
    ck.prebuild_twin()
    out, inf = VariableBaseMSM.multi_scalar_mul_batch(ck, [v])
    assert got(VESTA, out[0], inf[0]) == expect(VESTA, mult, s, mont=True)
    off, m = 123457, 3001
    assert got(VESTA, *VariableBaseMSM.multi_scalar_mul(ck, v.view(0, m), base_off=off, mont=True)) == expect(VESTA, mult[off:off + m], s[:m], mont=True)
    v.free()
    # two-valued (every scalar 0 or w)
    w = h.fr_mont_np(VESTA, [o.rng_fr(VESTA, 12, 0)])[0]
    mask = (np.arange(n) * 7) % 3 != 0
    t0 = ctx.two_valued_msms()
    vec = ctx.upload(np.where(mask[:, None], w[None, :], np.uint64(0)))
    out, inf = VariableBaseMSM.multi_scalar_mul_batch(ck, [vec])
    assert got(VESTA, out[0], inf[0]) == expect(VESTA, mult, ints(vec.download()), mont=True) and ctx.two_valued_msms() > t0
    vec.free()
    ck.free()
    # bucket-split (a 2^16 key, a device vector) and direct sum (a precomputed 2^12 key, host scalars)
    for log2n, flags, counter in ((16, ffi.AMSM_BASES_DEFAULT, "bucket_split"), (12, ffi.AMSM_BASES_PRECOMPUTE, "direct_sum")):
        small = CommitterKey.generate(ctx, SEED, 1 << log2n, flags)
        b = ctx.pipeline_stats()[counter]
        sv = ctx.random_vector(log2n, 1 << log2n, True)
        arg = sv if counter == "bucket_split" else sv.download()
        assert got(VESTA, *VariableBaseMSM.multi_scalar_mul(small, arg, mont=True)) == expect(VESTA, mult, ints(sv.download()), mont=True), counter
        assert ctx.pipeline_stats()[counter] > b, counter
        sv.free()
        small.free()
    # one-shot: host bases and host scalars of this call only
    small = CommitterKey.generate(ctx, SEED, 4096, ffi.AMSM_BASES_NO_PRECOMPUTE)
    xy, xinf = small.read()
    small.free()
    sc = [o.rng_fr(VESTA, 13, i) for i in range(4096)]
    assert got(VESTA, *VariableBaseMSM.multi_scalar_mul_oneshot(ctx, xy, h.scalars_to_np([v % VESTA.r for v in sc]), xinf)) == expect(VESTA, mult, sc)
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
        assert got(VESTA, out[0], inf[0]) == expect(VESTA, mult, ints(sv.download()), mont=True)
        assert c2.pipeline_stats()["bucket_per_lane"] == 0
        sv.free()
        plain.free()
    finally:
        c2.close()


def test_msm_2p22_exact(ctx, row):
    from accumulation_amd import CommitterKey, VariableBaseMSM, ffi
    n = 1 << 22
    ck = CommitterKey.generate(ctx, 4242, n, ffi.AMSM_BASES_PRECOMPUTE)
    v = ctx.random_vector(5, n, True)
    out, inf = VariableBaseMSM.multi_scalar_mul_batch(ck, [v])
    assert got(row.curve, out[0], inf[0]) == expect(row.curve, mults(4242, n), ints(v.download()), mont=True)
    v.free()
    ck.free()


# ---- Grumpkin alone: the cycle ---------------------------------------------------------------------------------------------------------
def test_the_cycle_closes(ctx, row, built_lib):
    """cr.cycle_closes on GPU contexts -- BN254 commitments' x | y words, unchanged, as Montgomery scalars of a Grumpkin MSM, and
    Grumpkin's as BN254's"""
    from accumulation_amd import Context, ffi
    bn = Context(ffi.AMSM_BN254_G1)
    try:
        cr.cycle_closes(bn, h.BN254, ctx, row.curve, 41)
        cr.cycle_closes(ctx, row.curve, bn, h.BN254, 43)
    finally:
        bn.close()


# ---- BLS12-377 alone: the reduced scalar stream, the points of small order ---------------------------------------------------------------
def test_scalar_stream_is_canonical(ctx, row):
    """k_vec_random over Bls12377Fr, seed 1, indices 0 .. 2^16: every value below r and equal to the restated rule, rng_fr(..) % r;
    the fallback indices (2008 and four more, where the literal rule gives >= r) are among them"""
    n = 1 << 16
    want, over = cr.scalar_stream(1, n)
    assert over == cr.FALLBACK_INDICES and o.rng_fr(row.curve, 1, 2008) >= row.R
    v = ctx.random_vector(1, n, False)
    out = ints(v.download())
    v.free()
    assert all(x < row.R for x in out) and tuple(out) == want


@pytest.mark.parametrize("flags", [1, 2], ids=["precomp", "plain"])
def test_group_law_on_the_small_order_points(ctx, row, flags):
    """doubling the point of order 2 gives the identity and the identity plus P gives P, through the device's group law: MSMs over
    plain and precomputed keys of small-order points (the table of a precomputed key holds the doublings of (p - 1, 0) as (0, 0):
    k_precompute_level / k_precompute_all_levels); tests/test_bls12_377_cpu.py runs the same cases on the host backend"""
    from tests.test_msm_gpu import run_msm
    C, P = row.curve, row.P
    g = o.generator(C)
    for pts, sc in (([(P - 1, 0)], [2]), ([(2, 3)], [3]), ([(2, 3)], [6]), ([(0, 1)], [3]), ([(P - 1, 0), g], [2, 1]),
                    ([(2, 3), (P - 1, 0), g], [3, 1, 5]), ([(P - 1, 0), (P - 1, 0)], [1, 1])):
        want = None
        for pt, s in zip(pts, sc):
            want = o.add(C, want, o.mul(C, s, pt))
        xy, inf = run_msm(ctx, C, pts, sc, flags)
        assert got(C, xy, inf) == want, (pts, sc)
