"""The four accumulation schemes over TRANSPARENT committer keys (setup(domain=...) of the Python mirrors, setup_transparent of the C++
headers; include/amsm.h: amsm_bases_sample): prove, verify and decide at small sizes on the library's host backend, the keys
themselves against the big-integer sampler, and `profile_as --transparent DOMAIN --dump` byte for byte against the mirrors over the
same key (compared as tests/test_profile_as_dump.py compares the seeded keys).  A `-m gpu` counterpart opens one ipa_pc_as
polynomial of 2^16 coefficients over a sampled key."""
import numpy as np
import pytest

from tests import harness_mirror, sample_ref as sr
from tests.test_profile_as_dump import cpp_dump, first_difference

DOMAIN = b"PC-DL-2020"


@pytest.fixture
def host_ctx(built_lib):
    from accumulation_amd import Context, ffi
    ctx = Context(ffi.AMSM_PALLAS, device=ffi.AMSM_DEVICE_HOST)
    yield ctx
    ctx.close()


@pytest.fixture
def transparent_setups(monkeypatch):
    """every setup of the mirrors takes domain=DOMAIN for the duration of one test: tests/harness_mirror.py then rebuilds
    profile_as's workloads over the transparent key"""
    from accumulation_amd import engine
    from accumulation_amd.ipa_pc import InnerProductArgPC as IpaPC
    ped, ipa = engine.PedersenCommitment.setup, IpaPC.setup.__func__
    monkeypatch.setattr(engine.PedersenCommitment, "setup",
                        staticmethod(lambda ctx, n, seed=0, flags=0, domain=None: ped(ctx, n, seed, flags, domain=DOMAIN)))
    monkeypatch.setattr(IpaPC, "setup", classmethod(lambda cls, ctx, max_degree, seed=0, domain=None: ipa(cls, ctx, max_degree, seed, domain=DOMAIN)))


def _sponge(ctx):
    return harness_mirror.make_sponge("poseidon", ctx.curve)


def test_setups_place_the_generators_like_the_seeded_ones(host_ctx):
    from accumulation_amd import PedersenCommitment
    from accumulation_amd.ipa_pc import InnerProductArgPC as IpaPC
    from accumulation_amd.trivial_pc_as import TrivialPC
    ref = sr.to_words(sr.PALLAS, sr.sample(sr.PALLAS, DOMAIN, 0, 34))
    ck = PedersenCommitment.setup(host_ctx, 20, domain=DOMAIN)
    assert len(ck) == 20 and np.array_equal(ck.read()[0], ref[:20]) and np.array_equal(ck.hiding_generator, ref[20])
    tk = TrivialPC.setup(host_ctx, 9, domain=DOMAIN)
    assert len(tk) == 10 and np.array_equal(tk.read()[0], ref[:10]) and np.array_equal(tk.hiding_generator, ref[10])
    pp = IpaPC.setup(host_ctx, 20, domain=DOMAIN)  # 32 generators, h = G_32, s = G_33
    assert pp.max_degree == 31 and np.array_equal(pp.comm_key.read()[0], ref[:32])
    assert np.array_equal(pp.h[0], ref[32]) and np.array_equal(pp.s[0], ref[33]) and not pp.h[1] and not pp.s[1]
    # the seeded keys stay what they were: the default of every setup
    seeded = PedersenCommitment.setup(host_ctx, 20)
    assert not np.array_equal(seeded.read()[0], ref[:20])


def test_hp_as_over_a_transparent_key(host_ctx):
    from accumulation_amd import PedersenCommitment
    from accumulation_amd.hp_as import ASForHadamardProducts as AS, Accumulator, InputInstance, InputWitness, InputWitnessRandomness, compute_hp
    from accumulation_amd.scalar_field import Fr
    ctx, fr, n = host_ctx, Fr(host_ctx.curve), 1 << 6
    hr = harness_mirror.HarnessRng(0xA11CE)
    ck = PedersenCommitment.setup(ctx, n, domain=DOMAIN)
    pk, vk, dk = AS.index(ck)
    a, b = ctx.random_vector(100, n, mont=True), ctx.random_vector(101, n, mont=True)
    prod = compute_hp(ctx, a, b)
    rnd = InputWitnessRandomness(hr.field() % fr.r, hr.field() % fr.r, hr.field() % fr.r)
    c = [PedersenCommitment.commit(ck, v, fr.to_limbs(r)) for v, r in ((a, rnd.rand_1), (b, rnd.rand_2), (prod, rnd.rand_3))]
    inputs = [Accumulator(InputInstance(*c), InputWitness(a, b, rnd))]
    first, _ = AS.prove(pk, inputs, [], hr, _sponge(ctx))
    acc, proof = AS.prove(pk, inputs, [first], hr, _sponge(ctx))
    assert AS.verify(ctx, vk, [i.instance for i in inputs], [first.instance], acc.instance, proof, _sponge(ctx))
    assert AS.decide(dk, acc, None)


def test_r1cs_nark_as_over_a_transparent_key(host_ctx):
    from accumulation_amd import PedersenCommitment
    from accumulation_amd import r1cs_nark as nark
    from accumulation_amd.r1cs_nark_as import ASForR1CSNark as AS, Input, InputInstance
    from accumulation_amd.scalar_field import Fr
    ctx, fr = host_ctx, Fr(host_ctx.curve)
    n_con, n_inst = 1 << 5, 6
    hr = harness_mirror.HarnessRng(0xB0B)
    A = [[(1, n_inst)] for _ in range(n_con - 1)] + [[]]
    B = [[(1, n_inst + 1)] for _ in range(n_con - 1)] + [[]]
    Cm = [[(1, 1)] for _ in range(n_con - 1)] + [[]]
    ipk = nark.index(ctx, A, B, Cm, n_inst, n_inst + 2, ck=PedersenCommitment.setup(ctx, n_con, domain=DOMAIN))
    pk, vk, dk = AS.index(ipk)
    a, b = hr.field() % fr.r, hr.field() % fr.r
    inst = [1, a * b % fr.r] + [a] * 4
    nark_sponge, _, _ = AS._sponges(_sponge(ctx))
    proof = nark.prove(ipk, inst, ctx.upload(fr.to_limbs_many([a, b])), True, nark_sponge, hr)
    inputs = [Input(InputInstance(inst, proof.first_msg), proof.second_msg)]
    first, _ = AS.prove(pk, inputs, [], hr, _sponge(ctx))
    acc, pr = AS.prove(pk, inputs, [first], hr, _sponge(ctx))
    assert AS.verify(ctx, vk, [i.instance for i in inputs], [first.instance], acc.instance, pr, _sponge(ctx))
    assert AS.decide(dk, acc, None)


def _ipa_accumulate(ctx, lg):
    from accumulation_amd import ffi, ipa_pc_as as M
    from accumulation_amd.engine import _ptr
    from accumulation_amd.ipa_pc import InnerProductArgPC as IpaPC
    from accumulation_amd.scalar_field import Fr
    AS = M.AtomicASForInnerProductArgPC
    fr, degree = Fr(ctx.curve), (1 << lg) - 1
    hr = harness_mirror.HarnessRng(0xD1)
    pp = IpaPC.setup(ctx, degree, domain=DOMAIN)
    pk, vk, dk = AS.index(pp, degree)
    poly = ctx.random_vector(77, degree + 1, mont=True)
    comm, rand = IpaPC.commit(pk.ipa_ck, poly, True, hr)
    point = hr.field() % fr.r
    z = ctx.vector(degree + 1)
    ffi.check(ctx._lib.amsm_vec_powers(ctx._h, _ptr(fr.to_limbs(point)), degree + 1, z.ptr), "amsm_vec_powers")
    value = IpaPC._inner_product(ctx, fr, poly, z)
    proof = IpaPC.open(pk.ipa_ck, poly, comm, point, rand, True, hr)
    inputs = [M.InputInstance(comm, point, value, proof)]
    first, _ = AS.prove(pk, inputs, [], hr, None)
    acc, pr = AS.prove(pk, inputs, [first.instance], hr, None)
    assert AS.verify(ctx, vk, inputs, [first.instance], acc.instance, pr, None)
    assert AS.decide(dk, acc, None)


def test_ipa_pc_as_over_a_transparent_key(host_ctx):
    _ipa_accumulate(host_ctx, 5)


@pytest.mark.gpu
def test_ipa_pc_as_opening_at_2p16_over_a_sampled_key_on_the_gpu(built_lib):
    from accumulation_amd import Context, ffi
    ctx = Context(ffi.AMSM_PALLAS)
    try:
        _ipa_accumulate(ctx, 16)
    finally:
        ctx.close()


def test_trivial_pc_as_over_a_transparent_key(host_ctx):
    from accumulation_amd import trivial_pc_as as M
    from accumulation_amd.scalar_field import Fr
    AS = M.ASForTrivialPC
    ctx, fr, degree = host_ctx, Fr(host_ctx.curve), (1 << 5) - 1
    hr = harness_mirror.HarnessRng(0x7121A1)
    pp = M.TrivialPC.setup(ctx, degree, domain=DOMAIN)
    ck, _ = M.TrivialPC.trim(pp, degree)
    pk, vk, dk = AS.index(pp, degree)
    poly = M.LabeledPolynomial([hr.field() % fr.r for _ in range(degree + 1)])
    comm = M.TrivialPC.commit(ck, poly)
    point = hr.field() % fr.r
    inputs = [M.Input(M.InputInstance(comm, point, poly.evaluate(fr, point)), poly)]
    first, _ = AS.prove(pk, inputs, [], None, _sponge(ctx))
    acc, pr = AS.prove(pk, inputs, [first], None, _sponge(ctx))
    assert AS.verify(ctx, vk, [i.instance for i in inputs], [first.instance], acc.instance, pr, _sponge(ctx))
    assert AS.decide(dk, acc, None)


@pytest.mark.parametrize("scheme,lg", [("hp_as", 7), ("r1cs_nark_as", 6), ("ipa_pc_as", 5), ("trivial_pc_as", 6)])
def test_cpp_driver_bytes_equal_the_mirror_over_a_transparent_key(built_lib, tmp_path, transparent_setups, scheme, lg):
    from accumulation_amd import Context
    (acc_cpp, proof_cpp), _ = cpp_dump(tmp_path, scheme, lg, "harness", "poseidon", -1, 3, extra=("--transparent", DOMAIN.decode()))
    (acc_seeded, _), _ = cpp_dump(tmp_path, scheme, lg, "harness", "poseidon", -1, 3)
    assert acc_cpp != acc_seeded  # the flag changed the key
    ctx = Context(0, device=-1)
    try:
        acc_py, proof_py = harness_mirror.SCHEMES[scheme](ctx, lg, True, "poseidon", 3)
    finally:
        ctx.close()
    assert first_difference(proof_cpp, proof_py) is None, ("proof", first_difference(proof_cpp, proof_py))
    assert first_difference(acc_cpp, acc_py) is None, ("accumulator", first_difference(acc_cpp, acc_py))
