"""amsm_vec_sample on the library's host backend: the keyed derivation "amsm-blind-v1" (accumulation_amd/csrc/blind.h) against its
plain-Python restatement tests/blind_ref.py (hashlib's BLAKE2s), the `first` argument, the argument checks, and the drivers that take a
VectorRng: a proof made with (rng, vector_rng = K) is byte for byte the proof made with an rng that REPLAYS blind_ref's stream 0 under
K for the long vector and then goes on with rng's own stream -- the drivers changed where the numbers come from and nothing else."""
import os
import subprocess

import numpy as np
import pytest

from tests import blind_ref as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = bytes(range(32))
N = 4096
# curve name -> (id, the attempts some index of the first N must need): half of Pallas's and Vesta's candidates are rejected
CURVES = {"pallas": (0, 8), "vesta": (2, 8), "bls12_381": (1, 4), "bn254": (4, 4), "grumpkin": (6, 4), "bls12_377": (8, 4)}


def to_ints(limbs):
    raw = np.ascontiguousarray(limbs, dtype="<u8").tobytes()
    return [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(len(raw) // 32)]


_ref_cache = {}


def reference(cid, stream=0, n=N, first=0, key=KEY):
    k = (cid, stream, n, first, key)
    if k not in _ref_cache:
        _ref_cache[k] = [br.scalar_attempts(cid, key, stream, first + j) for j in range(n)]
    return _ref_cache[k]


@pytest.fixture(scope="module")
def ctxs(built_lib):
    from accumulation_amd import Context, ffi
    out = {name: Context(cid, device=ffi.AMSM_DEVICE_HOST) for name, (cid, _) in CURVES.items()}
    yield out
    for c in out.values():
        c.close()


def sample(ctx, stream, n, mont=False, first=0, key=KEY):
    v = ctx.sample_vector(key, stream, n, mont=mont, first=first)
    out = v.download()
    v.free()
    return out


# ---- 1. against the reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CURVES))
def test_against_the_python_reference(ctxs, name):
    from accumulation_amd.scalar_field import MODULI, Fr
    cid, deep = CURVES[name]
    ref = reference(cid)
    attempts = [a for _, a in ref]
    assert max(attempts) >= deep, max(attempts)  # the case is worth running: rejection chains, ...
    assert sum(1 for a in attempts if a >= 2) >= 300  # ... and many of them
    want = [s for s, _ in ref]
    got = to_ints(sample(ctxs[name], 0, N))
    assert got == want
    assert all(x < MODULI[cid] for x in got)
    assert np.array_equal(sample(ctxs[name], 0, N, mont=True), Fr(cid).to_limbs_many(want))


# ---- 2. pieces -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pallas", "bls12_377"])
def test_pieces_of_one_long_vector(ctxs, name):
    whole = sample(ctxs[name], 3, N + 64)
    for a, b in ((1, 300), (255, 257), (4095, 65)):
        assert np.array_equal(sample(ctxs[name], 3, b, first=a), whole[a:a + b]), (a, b)


@pytest.mark.parametrize("name", ["pallas", "bls12_381"])
def test_the_index_is_64_bits_wide(ctxs, name):
    first = (1 << 32) - 8
    assert to_ints(sample(ctxs[name], 0, 16, first=first)) == [s for s, _ in reference(CURVES[name][0], 0, 16, first)]


def test_streams_and_keys_share_no_element(ctxs):
    ctx = ctxs["pallas"]
    other_key = KEY[:31] + bytes([KEY[31] ^ 1])
    sets = [set(to_ints(sample(ctx, 0, N))), set(to_ints(sample(ctx, 1, N))), set(to_ints(sample(ctx, 0, N, key=other_key)))]
    assert all(len(s) == N for s in sets)
    assert not (sets[0] & sets[1]) and not (sets[0] & sets[2]) and not (sets[1] & sets[2])
    assert to_ints(sample(ctx, 0, 8, key=other_key)) == [s for s, _ in reference(0, 0, 8, 0, other_key)]


# ---- 3. edges ------------------------------------------------------------------------------------------------------------------------
def test_argument_checks(ctxs):
    from accumulation_amd import ffi
    ctx = ctxs["pallas"]
    lib = ctx._lib
    v = ctx.fill(np.array([7, 7, 7, 7], dtype=np.uint64), 4)
    before = v.download().copy()
    assert lib.amsm_vec_sample(ctx._h, KEY, 0, 0, 0, 0, v.ptr) == ffi.AMSM_OK  # n == 0: nothing written
    assert np.array_equal(v.download(), before)
    assert lib.amsm_vec_sample(ctx._h, KEY, 0, (1 << 64) - 1, 2, 0, v.ptr) == ffi.AMSM_E_INVALID_ARG  # first + n past 2^64
    assert np.array_equal(v.download(), before)
    assert lib.amsm_vec_sample(ctx._h, None, 0, 0, 4, 0, v.ptr) == ffi.AMSM_E_INVALID_ARG
    assert lib.amsm_vec_sample(ctx._h, KEY, 0, 0, 4, 0, None) == ffi.AMSM_E_INVALID_ARG
    assert lib.amsm_vec_sample(None, KEY, 0, 0, 4, 0, v.ptr) == ffi.AMSM_E_INVALID_ARG
    assert np.array_equal(v.download(), before)
    assert lib.amsm_vec_sample(ctx._h, KEY, 0, (1 << 64) - 3, 2, 0, v.ptr) == ffi.AMSM_OK  # the last indices that fit
    assert to_ints(v.download()[:2]) == [br.scalar(0, KEY, 0, (1 << 64) - 3 + j) for j in range(2)]
    with pytest.raises(ValueError):
        ctx.sample_vector(b"short", 0, 4)
    v.free()


# ---- 4. replay: the drivers with a VectorRng ---------------------------------------------------------------------------------------------
class Replay:
    """rng whose first scalars are given; then the stream of `base`"""

    def __init__(self, head, base):
        self.head, self.base, self.at = list(head), base, 0

    def field(self):
        if self.at < len(self.head):
            self.at += 1
            return self.head[self.at - 1]
        return self.base.field()


def _nark_case(ctx, lg):
    from accumulation_amd import r1cs_nark as nark
    from accumulation_amd.scalar_field import Fr
    fr = Fr(ctx.curve)
    n_con, n_inst = 1 << lg, 6
    n_wit = n_con  # a, b, then copies of a: a witness-length blinder of n_con scalars
    A = [[(1, n_inst)] for _ in range(n_con - 1)] + [[]]
    B = [[(1, n_inst + 1)] for _ in range(n_con - 1)] + [[]]
    Cm = [[(1, 1)] for _ in range(n_con - 1)] + [[]]
    ipk = nark.index(ctx, A, B, Cm, n_inst, n_inst + n_wit, key_seed=31337)
    a, b = 0x1234567 % fr.r, 0x7654321 % fr.r
    inst = [1, a * b % fr.r] + [a] * 4
    wit = [a, b] + [a] * (n_wit - 2)
    return nark, fr, ipk, inst, wit


def test_r1cs_nark_prove_replays(ctxs):
    from accumulation_amd.hp_as import VectorRng
    from accumulation_amd.sponge import Sha256Sponge
    from tests.ser_mirror import Ser
    from tests.test_hp_as_scheme_gpu import SchemeRng
    ctx = ctxs["pallas"]
    nark, fr, ipk, inst, wit = _nark_case(ctx, 6)
    s = Ser(ctx)

    def run(rng, vrng):
        p = nark.prove(ipk, inst, ctx.upload(fr.to_limbs_many(wit)), True, Sha256Sponge(), rng, vector_rng=vrng)
        assert nark.verify(ipk, inst, p, Sha256Sponge())
        return s.nark_first_msg(p.first_msg) + s.nark_second_msg(p.second_msg)

    vr = VectorRng(KEY)
    sampled = run(SchemeRng(11), vr)
    assert vr.next_stream == 1
    replayed = run(Replay(br.scalars(ctx.curve, KEY, 0, len(wit)), SchemeRng(11)), None)
    assert sampled == replayed
    assert run(SchemeRng(11), None) != sampled  # (the blinder really is another vector)


def test_hiding_ipa_opening_replays(ctxs):
    from accumulation_amd.hp_as import VectorRng
    from accumulation_amd.ipa_pc import InnerProductArgPC as IpaPC
    from accumulation_amd.scalar_field import Fr
    from tests.ser_mirror import Ser
    from tests.test_hp_as_scheme_gpu import SchemeRng
    ctx = ctxs["pallas"]
    fr = Fr(ctx.curve)
    degree = (1 << 6) - 1
    pp = IpaPC.setup(ctx, degree, seed=0x1BA5EED)
    ck, vk = IpaPC.trim(pp, degree)
    poly = ctx.random_vector(77, degree + 1, mont=True)
    point = 0xABCDEF
    s = Ser(ctx)

    def open_with(vrng, head):
        base = SchemeRng(12)
        comm, rand = IpaPC.commit(ck, poly, True, base)
        rng = Replay(head, base)
        proof = IpaPC.open(ck, poly, comm, point, rand, True, rng, vector_rng=vrng)
        value = IpaPC._inner_product(ctx, fr, poly, _powers(ctx, fr, point, degree + 1))
        assert IpaPC.check(vk, comm, point, value, proof)
        return s.ipa_proof(proof)

    vr = VectorRng(KEY)
    sampled = open_with(vr, [])
    assert vr.next_stream == 1
    assert sampled == open_with(None, br.scalars(ctx.curve, KEY, 0, degree + 1))
    assert sampled != open_with(None, [])


def _powers(ctx, fr, point, n):
    from accumulation_amd import ffi
    from accumulation_amd.engine import _ptr
    z = ctx.vector(n)
    ffi.check(ctx._lib.amsm_vec_powers(ctx._h, _ptr(fr.to_limbs(point)), n, z.ptr), "amsm_vec_powers")
    return z


# ---- 5. the C++ drivers against the mirrors --------------------------------------------------------------------------------------------
SRC = os.path.join(ROOT, "tests", "cpp", "vec_sample_drivers.cpp")
EXE = os.path.join(ROOT, "build", "vec_sample_drivers")


def build_cpp():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    libdir = os.path.join(ROOT, "accumulation_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), SRC, "-o", EXE,
                           "-L", libdir, "-l:libamsm.so", f"-Wl,-rpath,{libdir}", "-Wl,--allow-shlib-undefined"])


def test_cpp_drivers_with_a_vector_rng_equal_the_mirrors(ctxs, built_lib):
    """tests/cpp/vec_sample_drivers.cpp: R1CSNark::prove (zk) and a hiding InnerProductArgPC::open with a VectorRng on the host backend;
    each proof verifies there and serialises to the bytes of the Python mirror under the same key and rng"""
    from accumulation_amd.hp_as import VectorRng
    from accumulation_amd.ipa_pc import InnerProductArgPC as IpaPC
    from accumulation_amd.sponge import Sha256Sponge
    from tests.ser_mirror import Ser
    from tests.test_hp_as_scheme_gpu import SchemeRng
    build_cpp()
    out = subprocess.run([EXE], capture_output=True, text=True, env=dict(os.environ, AMSM_CHECK_DEVICE="-1"), timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    vals = dict(ln.split() for ln in out.stdout.splitlines() if len(ln.split()) == 2)
    assert vals["nark_verified"] == "1" and vals["ipa_verified"] == "1"
    ctx = ctxs["pallas"]
    s = Ser(ctx)
    nark, fr, ipk, inst, wit = _nark_case(ctx, 6)
    vr = VectorRng(KEY)
    p = nark.prove(ipk, inst, ctx.upload(fr.to_limbs_many(wit)), True, Sha256Sponge(), SchemeRng(11), vector_rng=vr)
    assert vals["nark_proof"] == (s.nark_first_msg(p.first_msg) + s.nark_second_msg(p.second_msg)).hex()
    degree = (1 << 6) - 1
    ck, _ = IpaPC.trim(IpaPC.setup(ctx, degree, seed=0x1BA5EED), degree)
    poly = ctx.random_vector(77, degree + 1, mont=True)
    rng = SchemeRng(12)
    comm, rand = IpaPC.commit(ck, poly, True, rng)
    proof = IpaPC.open(ck, poly, comm, 0xABCDEF, rand, True, rng, vector_rng=vr)  # the same VectorRng carried on: stream 1
    assert vr.next_stream == 2
    assert vals["ipa_proof"] == s.ipa_proof(proof).hex()


@pytest.mark.parametrize("scheme,lg", [("r1cs_nark_as", 6), ("ipa_pc_as", 6)])
def test_profile_as_with_device_blinders_decides_on_the_host_backend(built_lib, tmp_path, scheme, lg):
    from tests.test_profile_as_dump import cpp_dump
    blind = ("--device-blinders", KEY.hex())
    (acc, proof), out = cpp_dump(tmp_path, scheme, lg, "harness", "poseidon", -1, extra=blind)  # asserts verified and decided
    assert '"device_blinders": true' in out and '"serialize_roundtrip_decides": true' in out
    (acc0, proof0), out0 = cpp_dump(tmp_path, scheme, lg, "harness", "poseidon", -1)
    assert "device_blinders" not in out0
    assert (acc, proof) != (acc0, proof0)
