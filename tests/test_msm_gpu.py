"""GPU parity tests (run with -m gpu on MI355X): the HIP MSM through the C ABI against the committed
golden vectors, the Python big-integer oracle and the plain-C restatement, bit-exact on the canonical
affine result (Montgomery limbs + infinity flag).  Mirrors what the reference checks with its
decider / verifier identities (src/hp_as/mod.rs:883-922), plus the edge cases its harness feeds
(SURVEY.md F8, Appendix E.9)."""
import numpy as np
import pytest

from oracle import pyref as o
from tests import helpers as h

pytestmark = pytest.mark.gpu

CURVES = [o.PALLAS, o.BLS12_381_G1]
FLAGS = {"plain": 2, "precomp": 1}


@pytest.fixture(scope="module")
def ctxs():
    from accumulation_amd import Context
    out = {c.name: Context(c.curve_id) for c in CURVES}
    yield out
    for c in out.values():
        c.close()


def run_msm(ctx, c, pts, scalars, flags, mont=False, base_off=0):
    from accumulation_amd import CommitterKey, VariableBaseMSM
    xy, inf = h.points_to_np(c, pts)
    ck = CommitterKey.load(ctx, xy, inf, flags)
    sc = [int(s) % c.r for s in scalars]
    s_np = h.fr_mont_np(c, sc) if mont else h.scalars_to_np(sc)
    out, oinf = VariableBaseMSM.multi_scalar_mul(ck, s_np, base_off=base_off, mont=mont)
    ck.free()
    return out, oinf


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("mode", ["plain", "precomp"])
def test_golden_cases(ctxs, c, mode):
    g = h.load_golden()["curves"][c.name]
    for case in g["cases"]:
        pts = [h.pt_from_hex(p) for p in case["points"]]
        sc = [int(s, 16) for s in case["scalars"]]
        out, oinf = run_msm(ctxs[c.name], c, pts, sc, FLAGS[mode])
        assert [hex(int(v)) for v in out] == case["expected_mont_limbs"], (case["name"], mode)
        assert int(oinf) == case["expected_is_inf"], (case["name"], mode)


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_golden_seeded_device_key(ctxs, c):
    """Keys generated ON the device (amsm_bases_generate) equal the oracle's stream, and the MSM over them
    reproduces the committed results."""
    from accumulation_amd import CommitterKey, VariableBaseMSM
    g = h.load_golden()["curves"][c.name]
    for case in g["seeded"]:
        ck = CommitterKey.generate(ctxs[c.name], case["seed_points"], case["n"])
        xy, inf = ck.read(0, 8)
        exp_xy, _ = h.points_to_np(c, o.rng_points(c, case["seed_points"], 8))
        assert np.array_equal(xy, exp_xy) and not inf.any()
        sc = h.scalars_to_np(o.rng_frs(c, case["seed_scalars"], case["n"]))
        out, oinf = VariableBaseMSM.multi_scalar_mul(ck, sc)
        assert [hex(int(v)) for v in out] == case["expected_mont_limbs"], case["name"]
        # scalars generated on the device too
        dv = ctxs[c.name].random_vector(case["seed_scalars"], case["n"], mont=False)
        assert np.array_equal(dv.download(), sc)
        out2, _ = VariableBaseMSM.multi_scalar_mul(ck, dv)
        assert np.array_equal(out, out2)
        ck.free()


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("mode", ["plain", "precomp"])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 1000, 4097])
def test_random_sizes_vs_c_oracle(ctxs, cref, c, mode, n):
    from accumulation_amd import CommitterKey, VariableBaseMSM
    xy = cref.rng_points(c.curve_id, 0xA000 + n, n)
    sc = cref.rng_scalars(0xB000 + n, n)
    ck = CommitterKey.load(ctxs[c.name], xy, None, FLAGS[mode])
    out, oinf = VariableBaseMSM.multi_scalar_mul(ck, sc)
    ref, rinf = cref.msm(c.curve_id, xy, sc, threads=4)
    assert oinf == rinf and np.array_equal(out, ref)
    # Montgomery-form scalars (raw Vec<Fr> memory): the device performs into_repr
    out_m, inf_m = VariableBaseMSM.multi_scalar_mul(ck, cref.fr_to_mont(c.curve_id, sc), mont=True)
    assert inf_m == rinf and np.array_equal(out_m, ref)
    ck.free()


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_window_override_sweep(ctxs, cref, c):
    """Every window width gives the same canonical result (signed digits, carries, top window)."""
    from accumulation_amd import CommitterKey, VariableBaseMSM
    n = 600
    xy = cref.rng_points(c.curve_id, 3, n)
    sc = cref.rng_scalars(4, n)
    sc[0] = h.scalars_to_np([c.r - 1])[0]
    sc[1] = h.scalars_to_np([(1 << 254) - 1])[0]
    ref, rinf = cref.msm(c.curve_id, xy, sc, threads=4)
    ctx = ctxs[c.name]
    try:
        for w in (2, 3, 5, 7, 8, 11, 13, 15, 16, 17, 20):
            ctx.set_window(w)
            for flags in (1, 2):
                ck = CommitterKey.load(ctx, xy, None, flags)
                out, oinf = VariableBaseMSM.multi_scalar_mul(ck, sc)
                assert oinf == rinf and np.array_equal(out, ref), (w, flags)
                ck.free()
    finally:
        ctx.set_window(0)


@pytest.mark.parametrize("mode", ["plain", "precomp"])
def test_degenerate_distributions_large(ctxs, cref, mode):
    """the reference's harness commits to vec![x; len] and to all-zero / all-one vectors.
    All n points then hit ONE bucket per window -- must stay correct (heavy-bucket path)."""
    from accumulation_amd import CommitterKey, VariableBaseMSM
    c = o.PALLAS
    n = 1 << 13
    xy = cref.rng_points(c.curve_id, 11, n)
    ck = CommitterKey.load(ctxs[c.name], xy, None, FLAGS[mode])
    x = o.rng_scalar(12, 0)
    for name, val in (("all_equal", x), ("all_zero", 0), ("all_one", 1), ("all_r_minus_1", c.r - 1)):
        sc = np.tile(h.scalars_to_np([val]), (n, 1))
        out, oinf = VariableBaseMSM.multi_scalar_mul(ck, sc)
        ref, rinf = cref.msm(c.curve_id, xy, sc, threads=4)
        assert oinf == rinf and np.array_equal(out, ref), name
    ck.free()


def test_scalar_out_of_range_is_an_error(ctxs):
    from accumulation_amd import CommitterKey, VariableBaseMSM, ffi
    c = o.PALLAS
    ctx = ctxs[c.name]
    ctx.set_window(16)
    try:
        xy, inf = h.points_to_np(c, o.rng_points(c, 1, 4))
        ck = CommitterKey.load(ctx, xy, None, 2)
        sc = h.scalars_to_np([1, 2, (1 << 256) - 1, 4])
        with pytest.raises(ffi.AmsmError) as e:
            VariableBaseMSM.multi_scalar_mul(ck, sc)
        assert e.value.status == ffi.AMSM_E_SCALAR_RANGE
        ck.free()
    finally:
        ctx.set_window(0)


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_base_offset_and_min_len(ctxs, cref, c):
    from accumulation_amd import CommitterKey, VariableBaseMSM
    n = 500
    xy = cref.rng_points(c.curve_id, 21, n)
    sc = cref.rng_scalars(22, n)
    for flags in (1, 2):
        ck = CommitterKey.load(ctxs[c.name], xy, None, flags)
        out, oinf = VariableBaseMSM.multi_scalar_mul(ck, sc[:100], base_off=137)
        ref, rinf = cref.msm(c.curve_id, xy[137:237], sc[:100])
        assert oinf == rinf and np.array_equal(out, ref)
        # more scalars than remaining bases: min(len) pairs are used
        out, oinf = VariableBaseMSM.multi_scalar_mul(ck, sc, base_off=450)
        ref, rinf = cref.msm(c.curve_id, xy[450:], sc[:50])
        assert oinf == rinf and np.array_equal(out, ref)
        ck.free()


@pytest.mark.parametrize("c,log2n", [(o.PALLAS, 16), (o.BLS12_381_G1, 14)], ids=["pallas_2^16", "bls_2^14"])
def test_config_sizes_vs_c_oracle(ctxs, cref, c, log2n):
    """BASELINE.json config 2 (2^16-point Pallas MSM) and a BLS12-381 size the oracle finishes in seconds."""
    from accumulation_amd import CommitterKey, VariableBaseMSM
    n = 1 << log2n
    ck = CommitterKey.generate(ctxs[c.name], 0x5EED1001, n)
    xy, inf = ck.read()
    assert not inf.any()
    assert np.array_equal(xy[:64], cref.rng_points(c.curve_id, 0x5EED1001, 64))
    sc = cref.rng_scalars(0x5EED0002, n)
    out, oinf = VariableBaseMSM.multi_scalar_mul(ck, sc)
    ref, rinf = cref.msm(c.curve_id, xy, sc, threads=8)
    assert oinf == rinf and np.array_equal(out, ref)
    ck.free()


def test_north_star_size_pallas_2_20(ctxs, cref):
    """BASELINE.json metric size: 2^20 Pallas pairs.  Checked (1) bit-exact against the window-parallel
    CPU restatement on the same inputs, (2) through size-independent properties: linearity
    commit(a + b) = commit(a) + commit(b) and commit(k*a) = k*commit(a) -- the homomorphism the
    reference's verifier relies on (src/hp_as/mod.rs:883-891)."""
    from accumulation_amd import CommitterKey, VariableBaseMSM
    c = o.PALLAS
    ctx = ctxs[c.name]
    n = 1 << 20
    ck = CommitterKey.generate(ctx, 0x5EED1001, n)
    assert ck.precomputed
    a = ctx.random_vector(0x5EED0001, n, mont=True)
    b = ctx.random_vector(0x5EED0002, n, mont=True)
    ca, ia = VariableBaseMSM.multi_scalar_mul(ck, a, mont=True)
    cb, ib = VariableBaseMSM.multi_scalar_mul(ck, b, mont=True)
    # a + 3*b on the device (combine_vectors), then commit
    coeffs = h.fr_mont_np(c, [1, 3])
    from accumulation_amd.hp_as import combine_vectors
    s = combine_vectors(ctx, [a, b], coeffs)
    cs, is_ = VariableBaseMSM.multi_scalar_mul(ck, s, mont=True)
    Pa, Pb, Ps = h.np_to_point(c, ca, ia), h.np_to_point(c, cb, ib), h.np_to_point(c, cs, is_)
    assert Ps == o.add(c, Pa, o.mul(c, 3, Pb))
    # bit-exact vs the CPU restatement
    xy, _ = ck.read()
    sc = cref.fr_from_mont(c.curve_id, a.download())
    ref, rinf = cref.msm(c.curve_id, xy, sc, threads=17)
    assert ia == rinf and np.array_equal(ca, ref)
    ck.free()


@pytest.mark.parametrize("bpl", ["1", "0"], ids=["bucket_per_lane_key", "chunked_17_bit_key"])
def test_carry_window_at_north_star_size(cref, bpl):
    """Round 2's keys of 2^20 generators use 17-bit windows (AMSM_BPL=0; since round 3 the twin key behind the fallback): 15
    of them cover the 255-bit scalars and the 16th holds only the signed recoding's carry.  For Pallas that carry needs a
    scalar above 2^254 -- one in 2^128 at random -- so the batch path would never see it in the other tests: here every
    997th scalar sits at the top of the field (r - 1, r - 2, 2^254 + k), and one vector is ALL r - 1 (every entry of the carry
    window in ONE bucket).  The same vectors go through round 3's 20-bit-window key (the top window's spread digit at its
    maximum, the constant vector through the fallback).  Bit-exact against the CPU restatement, blocking and in a batch."""
    import os
    from accumulation_amd import CommitterKey, Context, VariableBaseMSM, ffi
    c = o.PALLAS
    os.environ["AMSM_BPL"] = bpl
    try:
        ctx = Context(c.curve_id)
    finally:
        del os.environ["AMSM_BPL"]
    n = 1 << 20
    ck = CommitterKey.generate(ctx, 0x5EED1011, n)
    assert ck.precomputed and ck.window_bits == (20 if bpl == "1" else 17)
    small = CommitterKey.generate(ctx, 0x5EED1012, 1 << 18)
    plain = CommitterKey.generate(ctx, 0x5EED1013, 1 << 10, ffi.AMSM_BASES_NO_PRECOMPUTE)
    assert small.window_bits == 16 and plain.window_bits == 0
    small.free()
    plain.free()
    sc = ctx.random_vector(0x5EED0011, n, mont=False).download()
    top = [c.r - 1, c.r - 2, 1 << 254, (1 << 254) + 12345, c.r - (1 << 200)]
    for k, i in enumerate(range(0, n, 997)):
        sc[i] = h.scalars_to_np([top[k % len(top)]])[0]
    all_top = np.tile(h.scalars_to_np([c.r - 1])[0], (n, 1))
    xy, _ = ck.read()
    dv, dt = ctx.upload(sc), ctx.upload(all_top)
    for vec, host in ((dv, sc), (dt, all_top)):
        ref, rinf = cref.msm(c.curve_id, xy, host, threads=17)
        out, oinf = VariableBaseMSM.multi_scalar_mul(ck, vec)
        assert oinf == rinf and np.array_equal(out, ref)
        outs, infs = VariableBaseMSM.multi_scalar_mul_batch(ck, [vec, dv, vec], mont=False)
        assert np.array_equal(outs[0], ref) and np.array_equal(outs[2], ref) and not infs.any()
    ck.free()
    ctx.close()


def test_config5_size_pallas_2_22(ctxs, cref):
    """BASELINE.json config 5 size: 2^22 Pallas pairs (4 GiB of precomputed key).  Size-independent properties --
    the whole MSM equals the sum of the MSMs over its four 2^20-generator windows, and commit(a + 3b) = commit(a) +
    3 commit(b) -- plus the bit-exact comparison with the window-parallel CPU restatement."""
    from accumulation_amd import CommitterKey, VariableBaseMSM
    from accumulation_amd.hp_as import combine_vectors
    c = o.PALLAS
    ctx = ctxs[c.name]
    n, q = 1 << 22, 1 << 20
    ck = CommitterKey.generate(ctx, 0x5EED1005, n)
    assert ck.precomputed
    a = ctx.random_vector(0x5EED0051, n, mont=True)
    b = ctx.random_vector(0x5EED0052, n, mont=True)
    ca, ia = VariableBaseMSM.multi_scalar_mul(ck, a, mont=True)
    cb, ib = VariableBaseMSM.multi_scalar_mul(ck, b, mont=True)
    Pa, Pb = h.np_to_point(c, ca, ia), h.np_to_point(c, cb, ib)
    s = combine_vectors(ctx, [a, b], h.fr_mont_np(c, [1, 3]))
    cs, is_ = VariableBaseMSM.multi_scalar_mul(ck, s, mont=True)
    assert h.np_to_point(c, cs, is_) == o.add(c, Pa, o.mul(c, 3, Pb))
    parts, pinf = VariableBaseMSM.multi_scalar_mul_multi(ck, [(k * q, a.view(k * q, q)) for k in range(4)], mont=True)
    acc = None
    for k in range(4):
        acc = o.add(c, acc, h.np_to_point(c, parts[k], pinf[k]))
    assert acc == Pa
    xy, _ = ck.read()
    sc = cref.fr_from_mont(c.curve_id, a.download())
    ref, rinf = cref.msm(c.curve_id, xy, sc, threads=17)
    assert ia == rinf and np.array_equal(ca, ref)
    ck.free()
    ctx.empty_cache()


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_pedersen_commit_with_hiding(ctxs, cref, c):
    """PedersenCommitment::commit(ck, v, Some(r)) = msm(ck, v) + r*H  (src/hp_as/mod.rs:196,911-918)."""
    from accumulation_amd import PedersenCommitment
    ctx = ctxs[c.name]
    n = 300
    ck = PedersenCommitment.setup(ctx, n, seed=77)
    xy, _ = ck.read()
    pts = [h.np_to_point(c, xy[i], 0) for i in range(n)]
    H = h.np_to_point(c, ck.hiding_generator, 0)
    assert o.is_on_curve(c, H) and H is not None
    v = o.rng_scalars(5, n)
    r = o.rng_scalar(6, 0) % c.r
    exp = o.pedersen_commit(c, pts, H, v, r)
    out, oinf = PedersenCommitment.commit(ck, h.fr_mont_np(c, v), h.fr_mont_np(c, [r])[0])
    assert h.np_to_point(c, out, oinf) == exp
    out0, inf0 = PedersenCommitment.commit(ck, h.fr_mont_np(c, v), None)
    assert h.np_to_point(c, out0, inf0) == o.pedersen_commit(c, pts, H, v, None)
    # shorter vector than the key: generators[..len]
    out1, inf1 = PedersenCommitment.commit(ck, h.fr_mont_np(c, v[:17]), None)
    assert h.np_to_point(c, out1, inf1) == o.msm_naive(c, pts[:17], v[:17])
    ck.free()


def test_partials_roundtrip_single_rank(ctxs, cref):
    """The multi-GPU entry points on one rank: partial record -> combine == plain MSM."""
    import ctypes as C
    from accumulation_amd import CommitterKey, VariableBaseMSM, ffi
    from accumulation_amd.engine import _ptr
    c = o.PALLAS
    ctx = ctxs[c.name]
    n = 3000
    xy = cref.rng_points(c.curve_id, 31, n)
    sc = cref.rng_scalars(32, n)
    ref, rinf = cref.msm(c.curve_id, xy, sc, threads=4)
    for flags in (1, 2):
        # two "ranks" on one device: shard the key, gather the two partial records, combine
        half = n // 2
        rec = int(ctx._lib.amsm_partial_bytes(ctx._h))
        buf = ctx.vector((2 * rec + 31) // 32)
        for r, (lo, hi) in enumerate(((0, half), (half, n))):
            ck = CommitterKey.load(ctx, xy[lo:hi], None, flags)
            dv = ctx.upload(sc[lo:hi])
            ffi.check(ctx._lib.amsm_msm_partial_device(ctx._h, ck._h, 0, dv.ptr, hi - lo, 0,
                                                       C.c_void_p(buf.ptr.value + r * rec)), "partial")
            ck.free()
        out = np.zeros((2 * ctx.fq_limbs,), dtype=np.uint64)
        inf = C.c_uint8(0)
        ffi.check(ctx._lib.amsm_partials_combine(ctx._h, buf.ptr, 2, _ptr(out), C.byref(inf)), "combine")
        assert bool(inf.value) == rinf and np.array_equal(out, ref)


def test_partials_batch_roundtrip_single_rank(ctxs, cref):
    """Batched multi-GPU entry points on one device: two key shards play two ranks; each leaves 3 records, the
    records are regrouped as an all-gather would deliver them and folded in one call."""
    import torch
    from accumulation_amd import CommitterKey
    from accumulation_amd.dist import HipEngine
    c = o.PALLAS
    ctx = ctxs[c.name]
    n, half = 2500, 1200
    xy = cref.rng_points(c.curve_id, 41, n)
    scs = [cref.rng_scalars(50 + j, n) for j in range(3)]
    refs = [cref.msm(c.curve_id, xy, sc, threads=4) for sc in scs]
    for flags in (1, 2):
        parts = []
        engs = []
        for lo, hi in ((0, half), (half, n)):
            eng = HipEngine(ctx, CommitterKey.load(ctx, xy[lo:hi], None, flags))
            engs.append(eng)
            parts.append(eng.partial_batch([ctx.upload(sc[lo:hi]) for sc in scs], mont=False).clone())
        rec = engs[0].record_bytes
        gathered = torch.cat(parts)  # [rank][msm][record]
        grouped = gathered.view(2, 3, rec).permute(1, 0, 2).contiguous().view(-1)
        outs, infs = engs[0].combine_batch(grouped, 3, 2)
        for j in range(3):
            assert bool(infs[j]) == refs[j][1] and np.array_equal(outs[j], refs[j][0]), (flags, j)
        for e in engs:
            e.ck.free()


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_grouped_msm_vs_two_msms(ctxs, cref, c):
    """amsm_msm_grouped_device: one pass, two sums over the index classes ((i >> shift) & 1); equals two MSMs with the
    other class zeroed (CPU oracle), for precomputed and plain keys and several shifts."""
    from accumulation_amd import CommitterKey, VariableBaseMSM
    ctx = ctxs[c.name]
    n = 2048
    xy = cref.rng_points(c.curve_id, 81, n)
    sc = cref.rng_scalars(82, n)
    idx = np.arange(n)
    for flags in (1, 2):
        ck = CommitterKey.load(ctx, xy, None, flags)
        dv = ctx.upload(sc)
        for shift in (0, 3, 10):
            out, inf = VariableBaseMSM.multi_scalar_mul_grouped(ck, dv, shift, mont=False)
            for g in (0, 1):
                masked = sc.copy()
                masked[((idx >> shift) & 1) != g] = 0
                ref, rinf = cref.msm(c.curve_id, xy, masked, threads=4)
                assert bool(inf[g]) == rinf and np.array_equal(out[g], ref), (c.name, flags, shift, g)
        ck.free()


def test_sharded_msm_batch_world1(ctxs, cref):
    """dist.ShardedMSM over the HIP engine without a process group (world 1): msm() and msm_batch() both return the
    whole-job MSM; this is the code path bench.py --gpus N runs per rank (the all-gather itself is covered on CPU)."""
    from accumulation_amd import CommitterKey
    from accumulation_amd.dist import HipEngine, ShardedMSM
    c = o.PALLAS
    ctx = ctxs[c.name]
    n = 3000
    xy = cref.rng_points(c.curve_id, 61, n)
    scs = [cref.rng_scalars(70 + j, n) for j in range(4)]
    refs = [cref.msm(c.curve_id, xy, sc, threads=4) for sc in scs]
    ck = CommitterKey.load(ctx, xy, None, 1)
    sm = ShardedMSM(HipEngine(ctx, ck))
    out, inf = sm.msm(ctx.upload(scs[0]), mont=False)
    assert inf == refs[0][1] and np.array_equal(out, refs[0][0])
    outs, infs = sm.msm_batch([ctx.upload(sc) for sc in scs], mont=False)
    for j in range(4):
        assert bool(infs[j]) == refs[j][1] and np.array_equal(outs[j], refs[j][0]), j
    ck.free()


def test_randomized_geometry_stress(ctxs, cref):
    """Random (n, window, key kind, chunk length) combinations against the C oracle: exercises entry counts that are
    not multiples of the group size, chunks that straddle many / few buckets, windows whose last digit is short."""
    import os
    from accumulation_amd import CommitterKey, VariableBaseMSM
    c = o.PALLAS
    ctx = ctxs[c.name]
    xy_all = cref.rng_points(c.curve_id, 4242, 3000)
    sc_all = cref.rng_scalars(4343, 3000)
    try:
        for t in range(24):
            n = 1 + o.rng_word(99, 3 * t) % 2999
            w = 2 + o.rng_word(99, 3 * t + 1) % 18
            flags = 1 + o.rng_word(99, 3 * t + 2) % 2
            ctx.set_window(w)
            ck = CommitterKey.load(ctx, xy_all[:n], None, flags)
            out, oinf = VariableBaseMSM.multi_scalar_mul(ck, sc_all[:n])
            ref, rinf = cref.msm(c.curve_id, xy_all[:n], sc_all[:n], threads=2)
            assert oinf == rinf and np.array_equal(out, ref), (n, w, flags)
            ck.free()
    finally:
        ctx.set_window(0)


def test_top_of_field_scalars(cref):
    """Window widths that divide the 255-bit scalar width (3, 5, 15, 17) leave the top window holding only the carry
    of the signed recoding.  Scalars at and around the top of the field (r - 1, r - 2, 2^254 + k, all-ones low windows
    so that the carry reaches the top) must match the CPU oracle, with both prep chains (windows below 8 bits take the rocPRIM
    sort, the others the short chain of prep_kernels.h) and both key kinds."""
    from accumulation_amd import CommitterKey, Context, VariableBaseMSM
    c = o.PALLAS
    ctx = Context(c.curve_id)
    n = 600
    xy = cref.rng_points(c.curve_id, 21, n)
    special = [c.r - 1, c.r - 2, 1 << 254, (1 << 254) + 1, (1 << 254) - 1, c.r - (1 << 237), (1 << 254) + (1 << 253) % 1,
               c.r - 1 - (1 << 16), (1 << 238) - 1, (1 << 239) - 1, 0, 1]
    ints = [special[i % len(special)] if i % 3 == 0 else o.rng_scalar(22, i) % c.r for i in range(n)]
    sc = h.scalars_to_np(ints)
    ref, rinf = cref.msm(c.curve_id, xy, sc, threads=4)
    try:
        for w in (3, 5, 15, 17, 16):
            ctx.set_window(w)
            for flags in (1, 2):
                ck = CommitterKey.load(ctx, xy, None, flags)
                out, oinf = VariableBaseMSM.multi_scalar_mul(ck, sc)
                assert oinf == rinf and np.array_equal(out, ref), (w, flags)
                ck.free()
    finally:
        ctx.set_window(0)
    ctx.close()


@pytest.mark.parametrize("window", [0, 5, 7], ids=["short_chain", "rocprim_5_bit", "rocprim_7_bit"])
def test_prep_chain_variants_agree(cref, window):
    """The short prep chain (prep_kernels.h) and its fallback for windows below 8 bits (digits + rocPRIM sort + bounds + scan: what
    plain keys of up to 2^8 pairs and narrow window overrides take) feed accumulate L0 the same buckets: both must reproduce the
    CPU oracle on uniform, all-equal and sparse scalars, with precomputed and plain keys, on both curves."""
    from accumulation_amd import CommitterKey, Context, VariableBaseMSM
    for c in (o.PALLAS, o.BLS12_381_G1):
        ctx = Context(c.curve_id)
        ctx.set_window(window)
        n = 6001
        xy = cref.rng_points(c.curve_id, 11, n)
        cases = {"uniform": cref.rng_scalars(12, n)}
        eq = cases["uniform"].copy()
        eq[:] = eq[0]
        cases["all_equal"] = eq
        sp = np.zeros_like(cases["uniform"])
        sp[::97] = cases["uniform"][::97]
        cases["sparse"] = sp
        for name, sc in cases.items():
            ref, rinf = cref.msm(c.curve_id, xy, sc, threads=4)
            for flags in (1, 2):
                ck = CommitterKey.load(ctx, xy, None, flags)
                out, oinf = VariableBaseMSM.multi_scalar_mul(ck, sc)
                assert oinf == rinf and np.array_equal(out, ref), (window, c.name, name, flags)
                ck.free()
        ctx.close()


@pytest.mark.parametrize("log2n", [18, 20])
def test_bls12_381_vs_c_oracle(ctxs, cref, log2n):
    """BASELINE.json config 3 (384-bit base field): 2^18 and the full 2^20 BLS12-381 G1 pairs, bit-exact vs the CPU
    restatement."""
    from accumulation_amd import CommitterKey, VariableBaseMSM
    c = o.BLS12_381_G1
    ctx = ctxs[c.name]
    n = 1 << log2n
    ck = CommitterKey.generate(ctx, 0x5EED1002, n)
    assert ck.precomputed
    dv = ctx.random_vector(0x5EED0003, n, mont=False)
    out, oinf = VariableBaseMSM.multi_scalar_mul(ck, dv)
    xy, _ = ck.read()
    ref, rinf = cref.msm(c.curve_id, xy, dv.download(), threads=17)
    assert oinf == rinf and np.array_equal(out, ref)
    ck.free()


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_large_key_precompute_and_fold_batched_affine(ctxs, cref, c):
    """Keys and folds of >= 2^17 points convert their sums to affine in a second kernel with one inversion per four
    points (k_batch_to_affine).  (1) a 2^17 precomputed key that contains identity points against the C oracle;
    (2) the key fold l + x r at 2^17 through a size-independent property: an MSM over the folded key equals the MSM over
    the original key with scalars [s ; x s] (identity results included: the pairs (identity, identity))."""
    from accumulation_amd import CommitterKey, VariableBaseMSM
    from accumulation_amd.scalar_field import Fr
    ctx = ctxs[c.name]
    fr = Fr(ctx.curve)
    n = 1 << 18
    half = n // 2
    xy = cref.rng_points(c.curve_id, 0x717, n)
    inf = np.zeros(n, dtype=np.uint8)
    dead = [0, 5, half - 1]
    for i in dead:                      # identity in BOTH halves -> identity in the folded key
        inf[i] = inf[half + i] = 1
    inf[7] = 1                          # identity on one side only
    xy[inf.astype(bool)] = 0
    ck = CommitterKey.load(ctx, xy, inf, 1)   # precomputed: 2^18 >= 2^17 -> batched conversion of every level
    assert ck.precomputed
    sc = cref.rng_scalars(0x718, n)
    out, oinf = VariableBaseMSM.multi_scalar_mul(ck, ctx.upload(sc), mont=False)
    ref, rinf = cref.msm(c.curve_id, xy, sc, threads=8)
    assert bool(oinf) == rinf and np.array_equal(out, ref)
    # fold with a 128-bit and with a full-size challenge
    for x in (o.rng_scalar(0x719, 0) % (1 << 128), c.r - 12345):
        nbits = 128 if x < (1 << 128) else 255
        folded = ck.fold(half, fr.to_limbs(x), nbits)
        fxy, finf = folded.read(0, 8)
        for i in dead:
            if i < 8:
                assert finf[i] and not fxy[i].any()
        s = [o.rng_scalar(0x71A, i) % c.r for i in range(64)]          # a few distinct scalars, tiled
        s_half = (s * (half // 64))[:half]
        got, ginf = VariableBaseMSM.multi_scalar_mul(folded, ctx.upload(h.scalars_to_np(s_half)), mont=False)
        s_full = s_half + [(v * x) % c.r for v in s_half]
        exp, einf = VariableBaseMSM.multi_scalar_mul(ck, ctx.upload(h.scalars_to_np(s_full)), mont=False)
        assert bool(ginf) == bool(einf) and np.array_equal(got, exp), hex(x)
        folded.free()
    ck.free()


@pytest.mark.parametrize("mode", ["precomp", "plain"])
def test_skewed_scalars_heavy_partitions_vs_c_oracle(ctxs, cref, mode):
    """Skewed vectors at a size where one bucket holds more than 2^17 entries, bit-exact against the CPU oracle; which path each takes
    today is asserted by the context's counters.  The constant vectors -- all equal, all one, all r - 1: 2^18 pairs, from 2^17 up a
    lone vector is probed -- are taken by the two-valued form (k_tv_probe / k_tv_sum) and never reach a bucket.  Two values alternating,
    and a constant vector with a uniform tenth mixed in (giant and ordinary buckets inside one partition), reach the chunked pipeline --
    over the plain key behind a bucket-per-lane prep that overflows --, where the prep splits their partitions over 64 workgroups
    (k_prep_heavy_count / k_prep_heavy_place) and the accumulation lists their buckets as heavy (k_accum_l2a / k_accum_l2b:
    Context.heavy_buckets()); the grouped form as well.  All six curves, with the two-valued form off too: tests/test_skew_gpu.py."""
    from accumulation_amd import CommitterKey, VariableBaseMSM
    c = o.PALLAS
    ctx = ctxs[c.name]
    n = 1 << 18
    xy = cref.rng_points(c.curve_id, 0x5E1, n)
    ck = CommitterKey.load(ctx, xy, None, FLAGS[mode])
    uni = cref.rng_scalars(0x5E2, n)
    x, y = uni[0].copy(), uni[1].copy()
    cases = {"all_equal": np.tile(x, (n, 1)), "all_one": np.tile(h.scalars_to_np([1]), (n, 1)),
             "all_r_minus_1": np.tile(h.scalars_to_np([c.r - 1]), (n, 1))}
    two = np.tile(x, (n, 1))
    two[1::2] = y
    cases["two_values"] = two
    mixed = np.tile(x, (n, 1))
    mixed[::10] = uni[::10]
    cases["mostly_equal"] = mixed
    for name, sc in cases.items():
        sc = np.ascontiguousarray(sc)
        heavy, tv = ctx.heavy_buckets(), ctx.two_valued_msms()
        out, oinf = VariableBaseMSM.multi_scalar_mul(ck, sc)
        ref, rinf = cref.msm(c.curve_id, xy, sc, threads=8)
        assert oinf == rinf and np.array_equal(out, ref), (mode, name)
        if name in ("two_values", "mostly_equal"):
            assert ctx.heavy_buckets() > heavy and ctx.two_valued_msms() == tv, (mode, name)
        else:
            assert ctx.two_valued_msms() == tv + 1 and ctx.heavy_buckets() == heavy, (mode, name)
    # grouped: two sums over the index classes of bit 17 (= halves), constant scalars
    sc = np.ascontiguousarray(cases["mostly_equal"])
    heavy = ctx.heavy_buckets()
    out, inf = VariableBaseMSM.multi_scalar_mul_grouped(ck, ctx.upload(sc), 17, mont=False)
    assert ctx.heavy_buckets() > heavy
    for g in (0, 1):
        masked = sc.copy()
        masked[(np.arange(n) >> 17) & 1 != g] = 0
        ref, rinf = cref.msm(c.curve_id, xy, masked, threads=8)
        assert bool(inf[g]) == rinf and np.array_equal(out[g], ref), (mode, "grouped", g)
    ck.free()


def _negated_doubling_pair():
    import json
    import os
    d = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "bls12_381_negated_doubling.json")))
    return np.array([[int(v, 16) for v in d["l"]], [int(v, 16) for v in d["r"]]], dtype=np.uint64)


@pytest.mark.parametrize("flags", [1, 2], ids=["precomputed", "plain"])
def test_doubling_of_a_negated_duplicate_base(ctxs, flags):
    """Two equal bases whose signed digits are both negative land in one bucket: the second mixed addition finds
    acc == q and doubles the NEGATED affine point (y -> 2p - y, lazy limbs).  For a point whose Montgomery y is tiny
    (tests/golden/bls12_381_negated_doubling.json: found by the fuzzer as one wrong point in 124 124) the doubling's
    `K p - y` went negative in its top limb with K = 2.  Checked against the big-int oracle for several digit patterns."""
    from accumulation_amd import CommitterKey, VariableBaseMSM
    c = o.BLS12_381_G1
    ctx = ctxs[c.name]
    pair = _negated_doubling_pair()
    R = h.np_to_point(c, pair[1], False)
    L = h.np_to_point(c, pair[0], False)
    for pts_np, pts in ((np.stack([pair[1], pair[1]]), [R, R]), (np.stack([pair[1], pair[0], pair[1], pair[1]]), [R, L, R, R])):
        ck = CommitterKey.load(ctx, pts_np, None, flags)
        for s in (15, (1 << 16) - 1, (1 << 17) - 1, c.r - 1, c.r - 2, 7, (1 << 200) - 1):
            scal = [s] * len(pts)
            out, inf = VariableBaseMSM.multi_scalar_mul(ck, ctx.upload(h.scalars_to_np(scal)), mont=False)
            want = None
            for P_, s_ in zip(pts, scal):
                want = o.add(c, want, o.mul(c, s_, P_))
            assert h.np_to_point(c, out, inf) == want, (flags, len(pts), hex(s))
        ck.free()


def test_key_fold_that_ends_in_a_negated_doubling(ctxs):
    """amsm_bases_fold (l + x r by a NAF ladder) with x = r_order - 2: the ladder's last step adds -r to -r.  For the pair
    of tests/golden/bls12_381_negated_doubling.json that doubling went wrong (see the test above); x = r_order - 1 / - 3 and
    a 128-bit x take other paths and are checked as well, the pair alone and inside a 64-point fold."""
    from accumulation_amd import CommitterKey
    from accumulation_amd.scalar_field import Fr
    c = o.BLS12_381_G1
    ctx = ctxs[c.name]
    fr = Fr(ctx.curve)
    pair = _negated_doubling_pair()
    L, R = h.np_to_point(c, pair[0], False), h.np_to_point(c, pair[1], False)
    filler = [o.mul(c, 5 + 3 * i, o.generator(c)) for i in range(126)]
    fxy, _ = h.points_to_np(c, filler)
    for x, nbits in ((c.r - 2, 255), (c.r - 1, 255), (c.r - 3, 255), ((1 << 128) - 1, 128), (o.rng_scalar(0x77, 1) % c.r, 255)):
        ck = CommitterKey.load(ctx, pair, None, 2)
        f = ck.fold(1, fr.to_limbs(x), nbits)
        got, ginf = f.read()
        assert h.np_to_point(c, got[0], bool(ginf[0])) == o.add(c, L, o.mul(c, x, R)), (hex(x), nbits)
        f.free()
        ck.free()
        # position 36 of the left half / of the right half of a 128-point key (the lane the fuzzer's case sat on, mod 64)
        xy = np.concatenate([fxy[:36], pair[:1], fxy[36:63], fxy[63:99], pair[1:], fxy[99:126]])
        pts = filler[:36] + [L] + filler[36:63] + filler[63:99] + [R] + filler[99:126]
        ck = CommitterKey.load(ctx, xy, None, 2)
        f = ck.fold(64, fr.to_limbs(x), nbits)
        got, ginf = f.read()
        for i in (0, 35, 36, 37, 63):
            assert h.np_to_point(c, got[i], bool(ginf[i])) == o.add(c, pts[i], o.mul(c, x, pts[64 + i])), (hex(x), nbits, i)
        f.free()
        ck.free()


def test_large_msm_as_windows_of_the_key_equals_the_whole(ctxs):
    """MSMs of 2^22 pairs and more over a precomputed key run as pipelined sub-MSMs over 2^21-generator windows with
    window-relative indices in the prep (msm_multi_split_xyzz).  Same canonical results as the unsplit pipeline
    (AMSM_SPLIT_LOG2=0), for a size that is not a multiple of the window, blocking and in a batch, and with 2^20 windows."""
    import os
    from accumulation_amd import CommitterKey, Context, VariableBaseMSM
    c = o.PALLAS
    n = (1 << 22) + 12345
    results = []
    for split in ("21", "0", "20"):
        old = os.environ.get("AMSM_SPLIT_LOG2")
        os.environ["AMSM_SPLIT_LOG2"] = split
        try:
            ctx = Context(c.curve_id)
        finally:
            if old is None:
                os.environ.pop("AMSM_SPLIT_LOG2", None)
            else:
                os.environ["AMSM_SPLIT_LOG2"] = old
        ck = CommitterKey.generate(ctx, 0x5EED2211, n)
        assert ck.precomputed
        a = ctx.random_vector(0x5EED2212, n, mont=True)
        b = ctx.random_vector(0x5EED2213, n, mont=False)
        one, oinf = VariableBaseMSM.multi_scalar_mul(ck, a, mont=True)
        outs, infs = VariableBaseMSM.multi_scalar_mul_batch(ck, [a, a, a], mont=True)
        ob, _ = VariableBaseMSM.multi_scalar_mul(ck, b, mont=False)
        assert np.array_equal(outs[0], one) and np.array_equal(outs[2], one) and not infs.any() and not oinf
        results.append((one.copy(), ob.copy()))
        ck.free()
        ctx.close()
    for r in results[1:]:
        assert np.array_equal(r[0], results[0][0]) and np.array_equal(r[1], results[0][1])


def test_published_bls12_381_multiples_through_the_device_msm(ctxs):
    """third-party vectors (tests/test_third_party_kats_cpu.py: the zkcrypto / consensus-spec encodings of 1 G, 2 G, 3 G): MSMs over
    copies of the generator with unit scalars and over [G] with the scalar k, plain and precomputed keys"""
    from accumulation_amd import CommitterKey, VariableBaseMSM
    from tests.test_third_party_kats_cpu import KATS, decode
    c = o.BLS12_381_G1
    ctx = ctxs[c.name]
    g = o.generator(c)
    assert decode(KATS[1]) == g
    for flags in (1, 2):
        xy, _ = h.points_to_np(c, [g] * 300)
        ck = CommitterKey.load(ctx, xy, None, flags)
        for k in (2, 3):
            out, inf = VariableBaseMSM.multi_scalar_mul(ck, h.scalars_to_np([1] * k + [0] * (300 - k)))
            assert h.np_to_point(c, out, inf) == decode(KATS[k]), (flags, k)
            out, inf = VariableBaseMSM.multi_scalar_mul(ck, h.scalars_to_np([k]))
            assert h.np_to_point(c, out, inf) == decode(KATS[k]), (flags, k)
        ck.free()
