"""amsm_vec_sample on the GPU: k_vec_sample (accumulation_amd/csrc/vec_kernels.h) against the plain-Python derivation of
tests/blind_ref.py and, bit for bit, against the library's host backend at the sizes where the compaction of the rejects can go wrong
(around a wave, a workgroup round and a tile, lists shorter than a wave, several tiles); the kernel's other forms; pieces; and the
C++ drivers through `profile_as --device-blinders` on both backends.  The host-backend re-collection of this file is
tests/host_backend/test_host_vec_sample_cpu.py."""
import os

import numpy as np
import pytest

from tests.test_vec_sample_cpu import CURVES, KEY, N, reference, to_ints

pytestmark = pytest.mark.gpu

TILE = 1024  # launch.h: VEC_SAMPLE_TILE, the tile of the form that ships; form 2 has tiles of 4096


@pytest.fixture(scope="module")
def ctxs(built_lib):
    """per curve: (the context under test -- the GPU's, or the host backend's in the re-collection -- and a host-backend context)"""
    from accumulation_amd import Context, ffi
    out = {name: (Context(cid), Context(cid, device=ffi.AMSM_DEVICE_HOST)) for name, (cid, _) in CURVES.items()}
    yield out
    for a, b in out.values():
        a.close()
        b.close()


def sample(ctx, n, mont=False, first=0, stream=0):
    v = ctx.sample_vector(KEY, stream, n, mont=mont, first=first)
    out = v.download()
    v.free()
    return out


# ---- 1. the device against the reference ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CURVES))
def test_device_against_the_python_reference(ctxs, name):
    assert to_ints(sample(ctxs[name][0], N)) == [s for s, _ in reference(CURVES[name][0])]


# ---- 2. the device against the host backend, bit for bit ----------------------------------------------------------------------------------
SIZES = [1, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 3 * TILE + 5, 4095, 4096, 4097, 3 * 4096 + 5]


@pytest.mark.parametrize("name", ["pallas", "bls12_377"])
@pytest.mark.parametrize("mont", [False, True], ids=["canonical", "montgomery"])
def test_device_and_host_backend_are_bit_identical(ctxs, name, mont):
    dev, host = ctxs[name]
    whole = sample(host, max(SIZES), mont=mont, stream=5)
    for n in SIZES:
        got = sample(dev, n, mont=mont, stream=5)
        assert got.shape == (n, 4) and np.array_equal(got, whole[:n]), n


@pytest.mark.parametrize("name", ["pallas", "bls12_381"])
def test_far_indices(ctxs, name):
    dev, host = ctxs[name]
    for first in ((1 << 32) - 8, (1 << 40) + 1):
        assert np.array_equal(sample(dev, 300, first=first), sample(host, 300, first=first)), first
    assert to_ints(sample(dev, 16, first=(1 << 32) - 8)) == [s for s, _ in reference(CURVES[name][0], 0, 16, (1 << 32) - 8)]


def test_few_rejects_lists_shorter_than_a_wave(ctxs):
    dev, host = ctxs["bls12_381"]
    for n in (TILE, 4096):
        assert np.array_equal(sample(dev, n, mont=True, stream=2), sample(host, n, mont=True, stream=2)), n


def test_many_tiles(ctxs):
    dev, host = ctxs["pallas"]
    n = (1 << 16) + 3
    assert np.array_equal(sample(dev, n, mont=True, stream=9), sample(host, n, mont=True, stream=9))


# ---- 3. the kernel's forms ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pallas", "bls12_377"])
def test_kernel_forms_are_identical(built_lib, ctxs, name):
    """AMSM_VEC_SAMPLE_FORM at context creation: tiles of 1024 (1) and 4096 (2) scalars, and the default (the lane-per-scalar loop
    the A/B began with was never faster and is gone)"""
    from accumulation_amd import Context
    n = 3 * 4096 + 5
    want = sample(ctxs[name][0], n, mont=True, stream=4)
    old = os.environ.get("AMSM_VEC_SAMPLE_FORM")
    try:
        for form in ("1", "2"):
            os.environ["AMSM_VEC_SAMPLE_FORM"] = form
            c = Context(CURVES[name][0])
            try:
                assert np.array_equal(sample(c, n, mont=True, stream=4), want), form
                assert np.array_equal(sample(c, 3 * TILE + 5, mont=True, stream=4), want[:3 * TILE + 5]), form
            finally:
                c.close()
    finally:
        if old is None:
            os.environ.pop("AMSM_VEC_SAMPLE_FORM", None)
        else:
            os.environ["AMSM_VEC_SAMPLE_FORM"] = old


# ---- 4. pieces across contexts ----------------------------------------------------------------------------------------------------------
def test_a_vector_sampled_in_two_calls_from_two_contexts(built_lib, ctxs):
    from accumulation_amd import Context
    dev, _ = ctxs["pallas"]
    a, b = 1000 + 37, 2 * TILE + 11  # a is no multiple of 64
    whole = sample(dev, a + b, mont=True, stream=6)
    other = Context(CURVES["pallas"][0])
    try:
        assert np.array_equal(np.concatenate([sample(dev, a, mont=True, stream=6), sample(other, b, mont=True, first=a, stream=6)]), whole)
    finally:
        other.close()


# ---- 5. / 6. whole drivers ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ["r1cs_nark_as", "ipa_pc_as"])
def test_profile_as_with_device_blinders_same_bytes_on_both_backends(built_lib, ctxs, tmp_path, scheme):
    from tests.test_profile_as_dump import cpp_dump
    device = -1 if ctxs["pallas"][0].is_host else 0
    blind = ("--device-blinders", KEY.hex())
    g, out = cpp_dump(tmp_path, scheme, 8, "harness", "poseidon", device, extra=blind)  # asserts "verified" and "decided"
    assert '"device_blinders": true' in out
    h, _ = cpp_dump(tmp_path, scheme, 8, "harness", "poseidon", -1, extra=blind)
    assert g == h


@pytest.mark.parametrize("scheme", ["r1cs_nark_as", "ipa_pc_as"])
def test_without_a_vector_rng_the_drivers_are_untouched(built_lib, ctxs, tmp_path, scheme):
    """no --device-blinders: the dumps equal what tests/harness_mirror.py builds (this test passes before and after the feature)"""
    from tests.test_profile_as_dump import compare
    compare(tmp_path, scheme, 8, "harness", "poseidon", -1 if ctxs["pallas"][0].is_host else 0)
