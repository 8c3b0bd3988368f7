"""amsm_poly_div_linear(_batch) / amsm_poly_evaluate(_batch) against a big-integer restatement written here: the serial
recurrence q[i-1] = c[i] + z q[i] (what falls off the end is p(z)) and sum_i c_i x^i, in Python integers mod r.  Everything is
exact: limbs are compared for equality.

The restatement works on the Montgomery representatives themselves: division and evaluation are linear in the coefficients, so
with C_i = c_i R and the CANONICAL z the same recurrence yields q_i R and p(z) R.  The inputs are therefore raw limb arrays
(`Context.random_vector`, values below r) and no list-of-integer conversion is paid at 2^20 / 2^22.

HOST_MAX_LOG: the host-backend re-collection of this file (tests/host_backend/test_host_poly_cpu.py) skips the sizes above
2^HOST_MAX_LOG; the GPU run covers all of them."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyref as o
from tests.helpers import VESTA

pytestmark = pytest.mark.gpu

TILE = 1024  # coefficients per workgroup (accumulation_amd/csrc/msm_types.h: POLY_T)
HOST_MAX_LOG = 18
CURVES = {c.name: c for c in (o.PALLAS, o.BLS12_381_G1, VESTA)}
SIZES = [0, 1, 2, 3, 255, 256, 257, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, (1 << 16) + 3, 1 << 20, 1 << 22]
AMSM_E_INVALID_ARG = -1


@pytest.fixture(scope="module")
def ctxs():
    from accumulation_amd import Context
    out = {name: Context(c.curve_id) for name, c in CURVES.items()}
    yield out
    for c in out.values():
        c.close()


def _size_guard(ctx, n):
    if ctx.is_host and n > (1 << HOST_MAX_LOG):
        pytest.skip(f"host backend: sizes above 2^{HOST_MAX_LOG} run on the GPU only")


def _ints(limbs: np.ndarray):
    b = np.ascontiguousarray(limbs, dtype="<u8").tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def _limbs(vals):
    if not len(vals):
        return np.zeros((0, 4), dtype=np.uint64)
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in vals), dtype="<u8").reshape(-1, 4).copy()


def ref_div(c, z, r):
    """serial synthetic division -> (quotient, remainder)"""
    n = len(c)
    q = [0] * max(n - 1, 0)
    acc = 0
    for i in range(n - 1, -1, -1):
        acc = (c[i] + z * acc) % r
        if i:
            q[i - 1] = acc
    return q, acc


def ref_eval(c, x, r):
    """sum_i c_i x^i with a running power (0^0 = 1)"""
    s, xp = 0, 1
    for ci in c:
        s = (s + ci * xp) % r
        xp = xp * x % r
    return s


def _mont(curve, x):
    m = (x % curve.r) * (1 << 256) % curve.r
    return np.array([(m >> (64 * i)) & o.MASK64 for i in range(4)], dtype=np.uint64)


def _coeffs(ctx, curve, seed, n, pattern="random"):
    if pattern == "zero":
        return np.zeros((n, 4), dtype=np.uint64)
    if pattern == "max":
        return _limbs([curve.r - 1] * n)
    v = ctx.random_vector(seed, n, False)
    a = v.download()
    v.free()
    if pattern == "trailing_zeros":
        a[n - n // 3:] = 0
    return a


def _check_one(ctx, curve, coeffs, z):
    n = coeffs.shape[0]
    vec = ctx.upload(coeffs)
    zm = _mont(curve, z)
    quots, rem = ctx.poly_div_linear([vec], zm)
    val = ctx.poly_evaluate([vec], zm)
    c = _ints(coeffs)
    q_exp, rem_exp = ref_div(c, z, curve.r)
    assert quots[0].n == max(n - 1, 0)
    assert quots[0].download().tobytes() == _limbs(q_exp).tobytes()
    assert _ints(rem)[0] == rem_exp
    assert _ints(val)[0] == ref_eval(c, z, curve.r) == rem_exp  # the remainder IS the value at the same point
    # stream-ordered form: no remainder asked for, same quotient
    q2, none = ctx.poly_div_linear([vec], zm, remainders=False)
    assert none is None and q2[0].download().tobytes() == _limbs(q_exp).tobytes()
    for v in (vec, quots[0], q2[0]):
        v.free()


@pytest.mark.parametrize("n", SIZES)
def test_sizes_pallas(ctxs, n):
    ctx, curve = ctxs["pallas"], o.PALLAS
    _size_guard(ctx, n)
    _check_one(ctx, curve, _coeffs(ctx, curve, 100 + n % 97, n), o.rng_scalar(7, n) % curve.r)


@pytest.mark.parametrize("curve", [VESTA, o.BLS12_381_G1], ids=lambda c: c.name)
def test_other_curves(ctxs, curve):
    ctx = ctxs[curve.name]
    n = (1 << 16) + 3
    _check_one(ctx, curve, _coeffs(ctx, curve, 5, n), o.rng_scalar(8, 1) % curve.r)


@pytest.mark.parametrize("name", sorted(CURVES))
@pytest.mark.parametrize("pattern", ["random", "zero", "trailing_zeros", "max"])
@pytest.mark.parametrize("point", ["zero", "one", "minus_one", "random"])
def test_points_and_patterns(ctxs, name, pattern, point):
    ctx, curve = ctxs[name], CURVES[name]
    z = {"zero": 0, "one": 1, "minus_one": curve.r - 1, "random": o.rng_scalar(9, 3) % curve.r}[point]
    for n in (257, 2 * TILE + 1):
        _check_one(ctx, curve, _coeffs(ctx, curve, 11, n, pattern), z)


@pytest.mark.parametrize("lens", [[3000, 0, 1, TILE + 1, 70001], [5, TILE, 0, 2, 300, 2 * TILE + 7, 1, 4100, 9, 0, 2049]],
                         ids=["five", "eleven"])
def test_batch_equals_single_calls(ctxs, lens):
    """unequal lengths, an empty polynomial among them, a different z each; eleven: more than one launch's worth"""
    ctx, curve = ctxs["pallas"], o.PALLAS
    k = len(lens)
    coeffs = [_coeffs(ctx, curve, 40 + j, n) for j, n in enumerate(lens)]
    vecs = [ctx.upload(a) for a in coeffs]
    zs = [o.rng_scalar(41, j) % curve.r for j in range(k)]
    zm = np.stack([_mont(curve, z) for z in zs])
    quots, rems = ctx.poly_div_linear(vecs, zm)
    vals = ctx.poly_evaluate(vecs, zm[0])
    for j in range(k):
        q1, r1 = ctx.poly_div_linear([vecs[j]], zm[j])
        assert quots[j].download().tobytes() == q1[0].download().tobytes()
        assert rems[j].tobytes() == r1[0].tobytes()
        assert vals[j].tobytes() == ctx.poly_evaluate([vecs[j]], zm[0])[0].tobytes()
        c = _ints(coeffs[j])
        q_exp, rem_exp = ref_div(c, zs[j], curve.r)
        assert quots[j].download().tobytes() == _limbs(q_exp).tobytes() and _ints(rems[j:j + 1])[0] == rem_exp
        assert _ints(vals[j:j + 1])[0] == ref_eval(c, zs[0], curve.r)


def test_quotient_times_divisor_2_20(ctxs):
    """q(X) (X - z) + rem == p(X), coefficient for coefficient, through amsm_vec_combine: with A = rem | q (q shifted up by one
    degree) and q itself, p = 1 * A + (-z) * q"""
    from accumulation_amd.hp_as import combine_vectors
    ctx, curve = ctxs["pallas"], o.PALLAS
    n = 1 << 20
    _size_guard(ctx, n)
    p = ctx.random_vector(77, n, False)
    z = o.rng_scalar(78, 0) % curve.r
    quots, rem = ctx.poly_div_linear([p], _mont(curve, z))
    assert rem.tobytes() == ctx.poly_evaluate([p], _mont(curve, z)).tobytes()
    shifted = ctx.upload(np.concatenate([rem, quots[0].download()]))
    back = combine_vectors(ctx, [shifted, quots[0]], np.stack([_mont(curve, 1), _mont(curve, curve.r - z)]))
    assert back.n == n and back.download().tobytes() == p.download().tobytes()


def test_invalid_arguments(ctxs):
    ctx = ctxs["pallas"]
    lib, h = ctx._lib, ctx._h
    vec = ctx.random_vector(1, 16, False)
    quot = ctx.vector(15)
    pt = np.zeros(4, dtype=np.uint64)
    out = np.zeros(4, dtype=np.uint64)
    ptrs, lens = (C.c_void_p * 1)(vec.ptr), (C.c_size_t * 1)(16)
    qptrs, nullq, nullc = (C.c_void_p * 1)(quot.ptr), (C.c_void_p * 1)(None), (C.c_void_p * 1)(None)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    bad = AMSM_E_INVALID_ARG
    assert lib.amsm_poly_evaluate_batch(None, ptrs, lens, 1, P(pt), P(out)) == bad
    assert lib.amsm_poly_evaluate_batch(h, None, lens, 1, P(pt), P(out)) == bad
    assert lib.amsm_poly_evaluate_batch(h, ptrs, None, 1, P(pt), P(out)) == bad
    assert lib.amsm_poly_evaluate_batch(h, nullc, lens, 1, P(pt), P(out)) == bad
    assert lib.amsm_poly_evaluate_batch(h, ptrs, lens, 1, None, P(out)) == bad
    assert lib.amsm_poly_evaluate_batch(h, ptrs, lens, 1, P(pt), None) == bad
    assert lib.amsm_poly_evaluate(h, None, 16, P(pt), P(out)) == bad
    assert lib.amsm_poly_evaluate(h, vec.ptr, 1 << 32, P(pt), P(out)) == bad
    assert lib.amsm_poly_div_linear_batch(None, ptrs, lens, 1, P(pt), qptrs, P(out)) == bad
    assert lib.amsm_poly_div_linear_batch(h, None, lens, 1, P(pt), qptrs, P(out)) == bad
    assert lib.amsm_poly_div_linear_batch(h, ptrs, None, 1, P(pt), qptrs, P(out)) == bad
    assert lib.amsm_poly_div_linear_batch(h, ptrs, lens, 1, None, qptrs, P(out)) == bad
    assert lib.amsm_poly_div_linear_batch(h, ptrs, lens, 1, P(pt), None, P(out)) == bad
    assert lib.amsm_poly_div_linear_batch(h, ptrs, lens, 1, P(pt), nullq, P(out)) == bad  # lens[0] > 1 needs a quotient
    assert lib.amsm_poly_div_linear(h, vec.ptr, 16, None, quot.ptr, P(out)) == bad
    assert lib.amsm_poly_div_linear(h, vec.ptr, 16, P(pt), None, P(out)) == bad
    # nothing to do is fine, and so is a null quotient for a constant polynomial
    assert lib.amsm_poly_evaluate_batch(h, None, None, 0, P(pt), None) == 0
    assert lib.amsm_poly_evaluate_batch(h, None, None, 0, None, None) == 0
    assert lib.amsm_poly_div_linear_batch(h, None, None, 0, None, None, None) == 0
    one = (C.c_size_t * 1)(1)
    assert lib.amsm_poly_div_linear_batch(h, ptrs, one, 1, P(pt), nullq, P(out)) == 0
    assert out.tobytes() == vec.download()[0].tobytes()
    assert lib.amsm_poly_div_linear(h, vec.ptr, 16, P(pt), quot.ptr, None) == 0
    ctx.synchronize()


def test_workspace_is_accounted(ctxs):
    """the per-tile workspace comes from the context's grow-only buffers: amsm_ctx_memory sees it, amsm_ctx_trim releases it"""
    from accumulation_amd import Context
    ctx = Context(o.PALLAS.curve_id)
    if ctx.is_host:
        ctx.close()
        pytest.skip("the host backend has no workspace")
    vec = ctx.random_vector(3, 1 << 16, False)
    before = ctx.memory()["workspace_bytes"]
    ctx.poly_evaluate([vec], _mont(o.PALLAS, 5))
    grown = ctx.memory()["workspace_bytes"]
    assert grown > before
    ctx.trim()
    assert ctx.memory()["workspace_bytes"] < grown
    vec.free()
    ctx.close()
