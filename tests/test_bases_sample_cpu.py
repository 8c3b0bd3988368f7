"""amsm_bases_sample on the library's host backend, without a GPU: the transparent key derivation "amsm-sample-v1" (include/amsm.h)
against the big-integer sampler of tests/sample_ref.py (hashlib's BLAKE2s, pow, the oracle's square root and scalar multiplication)
on all three curves, the properties a committer key needs, the error returns, and the golden points that pin the derivation."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from oracle import pyref as o
from tests import sample_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "bases_sample_v1.json")
DOMAIN = b"PC-DL-2020"
FAR = (1 << 32) + 5
# indices from first = 0 and from first = 2^32 + 5 (BLS12-381: its cofactor multiplication costs the big-integer sampler ~10 ms each)
SIZES = {"pallas": (1024, 64), "vesta": (1024, 64), "bls12_381": (256, 32)}
AMSM_E_INVALID_ARG, AMSM_E_UNSUPPORTED = -1, -4


@pytest.fixture(scope="module")
def ctxs(built_lib):
    from accumulation_amd import Context, ffi
    ids = {"pallas": ffi.AMSM_PALLAS, "bls12_381": ffi.AMSM_BLS12_381_G1, "vesta": ffi.AMSM_VESTA}
    out = {name: Context(cid, device=ffi.AMSM_DEVICE_HOST) for name, cid in ids.items()}
    yield out
    for c in out.values():
        c.close()


def sample(ctx, domain, n, first=0, flags=None):
    from accumulation_amd import ffi
    from accumulation_amd.engine import CommitterKey
    ck = CommitterKey.sample(ctx, domain, n, ffi.AMSM_BASES_NO_PRECOMPUTE if flags is None else flags, first=first)
    xy, inf = ck.read()
    ck.free()
    assert not inf.any()
    return xy


def points(c, xy):
    return [o.point_from_mont_limbs(c, [int(w) for w in row], 0) for row in xy]


@pytest.mark.parametrize("name", list(SIZES))
def test_against_the_python_sampler(ctxs, name):
    c = sr.CURVES[name]
    n0, n1 = SIZES[name]
    for first, n in ((0, n0), (FAR, n1)):
        got = sample(ctxs[name], DOMAIN, n, first)
        assert np.array_equal(got, sr.to_words(c, sr.sample(c, DOMAIN, first, n))), (name, first)


@pytest.mark.parametrize("name", list(SIZES))
def test_points_are_on_the_curve_and_distinct(ctxs, name):
    c = sr.CURVES[name]
    n0, n1 = SIZES[name]
    pts = points(c, sample(ctxs[name], DOMAIN, n0)) + points(c, sample(ctxs[name], DOMAIN, n1, FAR))
    assert all(P is not None and o.is_on_curve(c, P) for P in pts)
    assert len(set(pts)) == len(pts)


def test_bls12_381_points_are_in_the_prime_order_subgroup(ctxs):
    c = sr.BLS
    for P in points(c, sample(ctxs["bls12_381"], DOMAIN, 16)):
        assert o.mul(c, c.r, P) is None


@pytest.mark.parametrize("name", list(SIZES))
def test_prefix_stability(ctxs, name):
    assert np.array_equal(sample(ctxs[name], DOMAIN, 100)[37:50], sample(ctxs[name], DOMAIN, 13, first=37))


@pytest.mark.parametrize("name", list(SIZES))
def test_domains_are_separate_and_the_empty_one_is_legal(ctxs, name):
    c = sr.CURVES[name]
    a, b, e = (sample(ctxs[name], d, 64) for d in (b"domain-a", b"domain-b", b""))
    rows = {bytes(r.tobytes()) for r in a} | {bytes(r.tobytes()) for r in b} | {bytes(r.tobytes()) for r in e}
    assert len(rows) == 3 * 64
    assert np.array_equal(e[:8], sr.to_words(c, sr.sample(c, b"", 0, 8)))
    full = bytes(range(32))  # the longest domain: the hashed message fills 61 of the block's 64 bytes
    assert np.array_equal(sample(ctxs[name], full, 8), sr.to_words(c, sr.sample(c, full, 0, 8)))


def test_every_domain_length_lays_the_message_out_right(ctxs):
    """the index, attempt and block bytes follow the domain at any alignment"""
    c = sr.PALLAS
    for ln in range(33):
        d = bytes((7 * i + ln) & 0xFF for i in range(ln))
        assert np.array_equal(sample(ctxs["pallas"], d, 3, first=FAR), sr.to_words(c, sr.sample(c, d, FAR, 3))), ln


def test_error_returns(ctxs):
    from accumulation_amd import ffi
    ctx = ctxs["pallas"]
    lib = ctx._lib
    h = C.c_void_p()
    dom = bytes(40)
    NP = ffi.AMSM_BASES_NO_PRECOMPUTE
    assert lib.amsm_bases_sample(ctx._h, dom, 33, 0, 4, NP, C.byref(h)) == AMSM_E_INVALID_ARG
    assert lib.amsm_bases_sample(ctx._h, None, 3, 0, 4, NP, C.byref(h)) == AMSM_E_INVALID_ARG
    assert lib.amsm_bases_sample(ctx._h, dom, 4, 0, 4, 32, C.byref(h)) == AMSM_E_INVALID_ARG  # an unknown flag bit
    assert lib.amsm_bases_sample(None, dom, 4, 0, 4, NP, C.byref(h)) == AMSM_E_INVALID_ARG
    assert lib.amsm_bases_sample(ctx._h, dom, 4, 0, 4, NP, None) == AMSM_E_INVALID_ARG
    assert lib.amsm_bases_sample(ctx._h, dom, 4, 0, 1 << 31, NP, C.byref(h)) == AMSM_E_UNSUPPORTED
    assert h.value is None
    # n = 0: an empty key, as amsm_bases_generate makes one; a null domain of length 0 is the empty domain
    assert lib.amsm_bases_sample(ctx._h, None, 0, 0, 0, NP, C.byref(h)) == 0 and h.value
    assert lib.amsm_bases_len(h) == 0
    lib.amsm_bases_free(h)
    g = C.c_void_p()
    assert lib.amsm_bases_generate(ctx._h, 1, 0, NP, C.byref(g)) == 0 and lib.amsm_bases_len(g) == 0
    lib.amsm_bases_free(g)


def test_a_sampled_key_is_an_ordinary_key(ctxs):
    """MSM over it == MSM over the same points loaded"""
    from accumulation_amd import ffi
    from accumulation_amd.engine import CommitterKey, VariableBaseMSM
    ctx = ctxs["pallas"]
    n = 300
    ck = CommitterKey.sample(ctx, DOMAIN, n)
    xy, _ = ck.read()
    loaded = CommitterKey.load(ctx, xy)
    scalars = np.array([o.int_to_limbs(o.rng_scalar(11, i) % sr.PALLAS.r, 4) for i in range(n)], dtype=np.uint64)
    a, ainf = VariableBaseMSM.multi_scalar_mul(ck, scalars)
    b, binf = VariableBaseMSM.multi_scalar_mul(loaded, scalars)
    assert ainf == binf and np.array_equal(a, b)
    want = o.msm_pippenger(sr.PALLAS, points(sr.PALLAS, xy), [o.limbs_to_int(r) for r in scalars])
    assert o.point_from_mont_limbs(sr.PALLAS, [int(w) for w in a], int(ainf)) == want


def test_golden_points_pin_the_derivation(ctxs):
    """tests/golden/bases_sample_v1.json (written by tools/gen_bases_sample_golden.py from the Python sampler): G_0 .. G_3 of every
    curve over b"amsm-test" -- a change of the derivation, in the library or in the reference sampler, shows here"""
    gold = json.load(open(GOLDEN))
    assert gold["derivation"] == "amsm-sample-v1" and bytes.fromhex(gold["domain_hex"]) == b"amsm-test"
    for name, c in sr.CURVES.items():
        want = [(int(p["x"], 16), int(p["y"], 16)) for p in gold["curves"][name]]
        assert len(want) == 4
        assert sr.sample(c, b"amsm-test", 0, 4) == want
        assert points(c, sample(ctxs[name], b"amsm-test", 4)) == want
