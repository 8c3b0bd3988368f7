"""ASForTrivialPC with its polynomial arithmetic on the device (amsm_poly_div_linear_batch / amsm_poly_evaluate_batch /
amsm_vec_combine; accumulation_amd/trivial_pc_as.py and include/amsm_trivial_pc_as.hpp say when).  AMSM_TRIVIAL_PC_DEVICE=1 forces
that path at any size, =0 the host path; both must produce the same bytes.

HOST_MAX_LOG: the host-backend re-collection of this file (tests/host_backend/test_host_trivial_pc_as_device_cpu.py) skips the
sizes above 2^HOST_MAX_LOG (the 2^20 harness); the GPU run covers them."""
import numpy as np
import pytest

from oracle import pyref as o
from tests import helpers as h
from tests.ser_mirror import Ser
from tests.test_hp_as_scheme_gpu import SchemeRng
from tests.test_profile_as_dump import compare
from tests.test_trivial_pc_as_scheme_gpu import env, run_template  # noqa: F401  (env: the template's fixture)

pytestmark = pytest.mark.gpu
HOST_MAX_LOG = 18
OVERRIDE = "AMSM_TRIVIAL_PC_DEVICE"


@pytest.fixture
def device_calls(monkeypatch):
    """counts the division calls the mirror makes: the forced path must really be the device one"""
    from accumulation_amd.engine import Context
    calls = []
    orig = Context.poly_div_linear

    def spy(self, vectors, zs, remainders=True):
        calls.append(len(vectors))
        return orig(self, vectors, zs, remainders)

    monkeypatch.setattr(Context, "poly_div_linear", spy)
    return calls


@pytest.mark.parametrize("scenario,iterations", [([1], 3), ([3], 3), ([1, 1], 3), ([1, 1, 2, 3], 2), ([1, 0, 0, 0], 3), ([0], 1)],
                         ids=["single_input_init", "multiple_inputs_init", "simple_accumulation", "multiple_inputs_accumulation",
                              "accumulators_only", "no_inputs_init"])
def test_template_on_the_device_path(env, monkeypatch, device_calls, scenario, iterations):  # noqa: F811
    """the six scenarios of the reference's template (src/lib.rs:263-461) at degree 11, as test_trivial_pc_as_scheme_gpu.py runs them"""
    monkeypatch.setenv(OVERRIDE, "1")
    assert run_template(env, scenario, num_iterations=iterations)
    assert len(device_calls) == iterations * len(scenario)  # one batched division per prove


def test_override_rule(monkeypatch):
    """0: never; 1: always; unset, empty or anything else: the threshold -- the rule both drivers read the override by"""
    from accumulation_amd.trivial_pc_as import TRIVIAL_PC_DEVICE_MIN, _on_device
    below, at = TRIVIAL_PC_DEVICE_MIN - 1, TRIVIAL_PC_DEVICE_MIN
    monkeypatch.delenv(OVERRIDE, raising=False)
    assert not _on_device(below) and _on_device(at)
    for value in ("", "yes", "2", " 1"):
        monkeypatch.setenv(OVERRIDE, value)
        assert not _on_device(below) and _on_device(at)
    monkeypatch.setenv(OVERRIDE, "0")
    assert not _on_device(at)
    monkeypatch.setenv(OVERRIDE, "1")
    assert _on_device(below)


def _inputs(ctx, ck, n_coeffs, count, seed):
    """seeded inputs whose coefficients are limb arrays read as canonical integers (no per-coefficient big-int generation)"""
    from accumulation_amd.scalar_field import Fr
    from accumulation_amd.trivial_pc_as import Input, InputInstance, LabeledPolynomial, TrivialPC
    fr = Fr(ctx.curve)
    out = []
    for j in range(count):
        v = ctx.random_vector(seed + j, n_coeffs, False)
        raw = v.download().tobytes()
        v.free()
        poly = LabeledPolynomial([int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)])
        point = o.rng_scalar(seed, 1000 + j) % fr.r
        out.append(Input(InputInstance(TrivialPC.commit(ck, poly), point, poly.evaluate(fr, point)), poly))
    return out


def _harness(ctx, pp, degree, seed):
    """one input accumulated into two old accumulators (examples/scaling-as.rs:62-63, 91-104) -> everything a caller sees"""
    from accumulation_amd.trivial_pc_as import ASForTrivialPC as AS, TrivialPC
    ck, _ = TrivialPC.trim(pp, degree)
    pk, vk, dk = AS.index(pp, degree)
    ins = _inputs(ctx, ck, degree + 1, 3, seed)
    acc_a, proof_a = AS.prove(pk, [ins[0]], [], None, None)
    acc_b, _ = AS.prove(pk, [ins[1]], [], None, None)
    acc, proof = AS.prove(pk, [ins[2]], [acc_a, acc_b], None, None)
    return dict(ck=ck, vk=vk, dk=dk, ins=ins, old=[acc_a, acc_b], acc=acc, proof=proof, first=(acc_a, proof_a))


@pytest.mark.parametrize("degree", [11, (1 << 10) - 1, (1 << 12) + 4])
def test_both_paths_serialise_to_the_same_bytes(monkeypatch, device_calls, degree):
    from accumulation_amd import Context, ffi
    from accumulation_amd.trivial_pc_as import ASForTrivialPC as AS, TrivialPC
    ctx = Context(ffi.AMSM_PALLAS)
    pp = TrivialPC.setup(ctx, degree)
    s = Ser(ctx)
    got = {}
    for force in ("0", "1"):
        monkeypatch.setenv(OVERRIDE, force)
        before = len(device_calls)
        r = _harness(ctx, pp, degree, seed=900 + degree)
        assert (len(device_calls) - before) == (3 if force == "1" else 0)
        assert AS.verify(ctx, r["vk"], [r["ins"][2].instance], [a.instance for a in r["old"]], r["acc"].instance, r["proof"], None)
        assert AS.decide(r["dk"], r["acc"], None)
        got[force] = (s.trivial_accumulator(r["first"][0]), s.trivial_proof(r["first"][1]),
                      s.trivial_accumulator(r["acc"]), s.trivial_proof(r["proof"]))
    assert got["0"] == got["1"]
    ctx.close()


@pytest.mark.parametrize("shape", ["n2", "harness"])
def test_cpp_driver_bytes_equal_the_mirror_at_2_16(built_lib, tmp_path, monkeypatch, shape):
    """`profile_as trivial_pc_as 16 16 --dump` against the Python mirror, as tests/test_profile_as_dump.py does for config 1, with the
    default threshold: at 2^16 coefficients both are on the device path"""
    from accumulation_amd import Context
    from accumulation_amd.trivial_pc_as import TRIVIAL_PC_DEVICE_MIN
    monkeypatch.delenv(OVERRIDE, raising=False)
    assert (1 << 10) < TRIVIAL_PC_DEVICE_MIN <= (1 << 16)
    probe = Context()
    device = -1 if probe.is_host else 0
    probe.close()
    compare(tmp_path, "trivial_pc_as", 16, shape, "poseidon", device, seed=16)


def test_harness_shape_at_2_20(cref, monkeypatch):
    """Pallas, 2^20 coefficients, one input and two old accumulators, default threshold: verify and decide accept, a tampered
    coefficient makes decide refuse, the accumulator's commitment is the CPU oracle's MSM of its coefficients"""
    from accumulation_amd import Context, ffi
    from accumulation_amd.trivial_pc_as import ASForTrivialPC as AS, TrivialPC
    monkeypatch.delenv(OVERRIDE, raising=False)
    ctx = Context(ffi.AMSM_PALLAS)
    if ctx.is_host:
        ctx.close()
        pytest.skip(f"host backend: sizes above 2^{HOST_MAX_LOG} run on the GPU only")
    c = o.PALLAS
    degree = (1 << 20) - 1
    pp = TrivialPC.setup(ctx, degree)
    r = _harness(ctx, pp, degree, seed=2020)
    acc = r["acc"]
    assert AS.verify(ctx, r["vk"], [r["ins"][2].instance], [a.instance for a in r["old"]], acc.instance, r["proof"], None)
    assert AS.decide(r["dk"], acc, None)
    xy, _ = r["ck"].read()
    raw = b"".join((v % c.r).to_bytes(32, "little") for v in acc.witness.coeffs)
    ref, rinf = cref.msm(c.curve_id, xy[: degree + 1], np.frombuffer(raw, dtype="<u8").reshape(-1, 4).copy(), threads=16)
    assert bool(acc.instance.commitment.elem[1]) == rinf and np.array_equal(np.asarray(acc.instance.commitment.elem[0]), ref)
    acc.witness.coeffs[degree // 2] = (acc.witness.coeffs[degree // 2] + 1) % c.r
    assert not AS.decide(r["dk"], acc, None)
    ctx.close()
